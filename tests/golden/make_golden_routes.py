"""The Aggregator's routing decisions on the host, recorded as data (``routes.json``).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_routes.py

Every combination of scheme, opt-in key, condition and round of stub clients (or of host-built
wire payloads) is put to the public route predicates of ``openmsftl_amd.aggregation`` and to
``aggregate_grads`` / ``aggregate_wire`` themselves, with ``aggregation._device_of`` replaced by
a function that raises a sentinel: a round that passes every host check ends there ("reaches the
device"), so no GPU is needed.  Per case the value or ``"<ExceptionType>: <message>"`` of each call
is recorded, then ``agg_path``.  The file holds the distinct outcome strings once
(``outcomes``), the distinct rows of outcome indices (``grads_rows`` / ``wire_rows``) and one row
index per case, in the order of :func:`grads_cases` / :func:`wire_cases`.

The file was written by this script at the commit BEFORE the routing layer was refactored and is
never regenerated to make tests/test_routes_host.py pass: that test recomputes the table and
requires equality with the file.  Only public names of the package are used, so the script runs
unchanged on either side of such a change.
"""
from __future__ import annotations

import itertools
import json
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
TESTS = os.path.dirname(HERE)
ROOT = os.path.dirname(TESTS)
for _p in (ROOT, TESTS):
    if _p not in sys.path:
        sys.path.insert(0, _p)

OUT = os.path.join(HERE, "routes.json")
F = np.float32
DEVICE = "reaches the device"

SCHEMES = (("fed_avg", "fed_avg", {}),
           ("fed_avg+pc", "fed_avg", {"pc_analysis": "gram"}),
           ("krum", "krum", {}),
           ("spectral_gram", "spectral_gram", {"rank": 2, "adaptive_rank_th": 0}),
           ("geometric_median", "geometric_median", {}),
           ("centered_clip", "centered_clip", {"cclip_tau": 1.0}),
           ("trimmed_mean", "trimmed_mean", {"trim_count": 1}),
           ("coordinate_median", "coordinate_median", {}),
           ("sign_majority", "sign_majority", {}))

KEYS = (("none", {}),
        ("sign_geometry", {"sign_geometry": True}),
        ("sign_trim", {"sign_trim": True}),
        ("sign_geometry+sign_trim", {"sign_geometry": True, "sign_trim": True}),
        ("sign_packets=False", {"sign_packets": False}),
        ("batched_error_feedback", {"batched_error_feedback": True}))

_HIER = {"num_hierarchies": 1, "cluster_size_list": [2]}
#: name, config, dtype of gradient_weights (None: unweighted)
CONDITIONS = (("none", {}, None),
              ("hierarchies", _HIER, None),
              ("devices=2", {"devices": 2}, None),
              ("budget=1000", {"device_budget_bytes": 1000}, None),
              ("weights f32", {}, np.float32),
              ("weights f64", {}, np.float64),
              ("hierarchies+devices=2+weights f64", dict(_HIER, devices=2), np.float64))


class _ReachedDevice(Exception):
    """Raised in place of the first touch of the device."""


def _reach(agg):
    raise _ReachedDevice()


def _clients(m=3, n=100, fn="sign", dtype=F, **cfg):
    from openmsftl_amd import Compression
    return [types.SimpleNamespace(C=Compression(dict({"compression_function": fn}, **cfg)),
                                  grad=np.zeros(n, dtype), client_id=i) for i in range(m)]


def client_rounds():
    top = dict(n=1000, fn="top", fraction_coordinate=0.1)
    stub = _clients()
    stub[1].C = types.SimpleNamespace(compression_function="sign", error_feedback=False)
    return (("sign", _clients()),
            ("sign+ef", _clients(error_feedback=True)),
            ("top", _clients(**top)),
            ("top+ef", _clients(error_feedback=True, **top)),
            ("sign and one top", _clients() + _clients(1, fn="top", fraction_coordinate=0.1)),
            ("a stub codec", stub),
            ("float64", _clients(dtype=np.float64)),
            ("two lengths", _clients() + _clients(1, n=101)),
            ("n=0", _clients(n=0)),
            ("129 sign", _clients(m=129)),
            ("129 top", _clients(m=129, **top)),
            ("top f=0", _clients(n=1000, fn="top", fraction_coordinate=0)),
            ("top f=1", _clients(n=1000, fn="top", fraction_coordinate=1)),
            ("top two fractions", _clients(2, **top) + _clients(1, n=1000, fn="top", fraction_coordinate=0.2)),
            ("full", _clients(fn="full")))


def payload_rounds():
    import sign_geometry_model as gm
    import wire_model as wm
    from oracle import packet_oracle as po
    rng = np.random.default_rng(5)
    B, s = rng.random((3, 129)) < 0.5, F([0.5, 1.0, 2.0])
    sign = gm.packets(B, s)
    sign_other = gm.packets(B[:1, :128], s[:1])[0]
    bad = bytearray(sign[1])
    bad[-1] = 0x80                                     # a pad bit of the last word

    def top_payload(n, idx):
        idx = np.asarray(idx, np.int64)
        val = (np.arange(idx.size) + 1).astype(F)
        return wm.pack(po.build_idxval(n, idx, val, thresh=0, codec=po.CODEC_TOP, k=idx.size))

    top = [top_payload(129, ix) for ix in ([3, 50, 100], [0, 64, 128], [7, 8, 9])]
    top_other = top_payload(128, [1, 2, 3])
    return (("sign", sign),
            ("top", top),
            ("mixed", [sign[0], top[0], sign[1]]),
            ("129 sign", [sign[0]] * 129),
            ("129 top", [top[0]] * 129),
            ("sign, pad word of payload 1 corrupted", [sign[0], bytes(bad), sign[2]]),
            ("sign of two lengths", [sign[0], sign_other]),
            ("top of two lengths", [top[0], top_other]))


def _outcome(fn, *args):
    try:
        return repr(fn(*args))
    except _ReachedDevice:
        return DEVICE
    except Exception as e:                              # noqa: BLE001 (the refusal is the record)
        return f"{type(e).__name__}: {e}"


def _aggregator(scheme, key, cond, m):
    from openmsftl_amd.aggregation import Aggregator
    _, name, scfg = scheme
    _, ccfg, wdt = cond
    agg = Aggregator(dict({"aggregation_scheme": name}, **scfg, **key[1], **ccfg))
    if wdt is not None:
        agg.gar.gradient_weights = np.full(m, 1.0 / m, wdt)
    return agg


def grads_cases():
    """(case name, scheme, key, condition, clients) in the order of ``routes.json``."""
    rounds = client_rounds()
    for scheme, key, cond, (rname, clients) in itertools.product(SCHEMES, KEYS, CONDITIONS, rounds):
        yield f"{scheme[0]} | {key[0]} | {cond[0]} | {rname}", scheme, key, cond, clients


def wire_cases():
    rounds = payload_rounds()
    for scheme, key, cond, (rname, raws) in itertools.product(SCHEMES, KEYS, CONDITIONS, rounds):
        yield f"{scheme[0]} | {key[0]} | {cond[0]} | {rname}", scheme, key, cond, raws


GRADS_FIELDS = ("sign_route", "sign_gram_route", "sign_trim_route", "gram_route_k", "ef_batch_k",
                "aggregate_grads", "agg_path")
WIRE_FIELDS = ("aggregate_wire", "agg_path")


def grads_row(scheme, key, cond, clients):
    """The outcomes of one case, in the order of :data:`GRADS_FIELDS`."""
    from openmsftl_amd import aggregation as ag
    agg = _aggregator(scheme, key, cond, len(clients))
    row = [_outcome(ag.sign_route, agg, clients), _outcome(ag.sign_gram_route, agg, clients),
           _outcome(ag.sign_trim_route, agg, clients),
           _outcome(ag.gram_route_k, agg, clients) if ag.gram_wanted(agg) else "not wanted",
           _outcome(ag.ef_batch_k, agg, clients)]
    assert agg.agg_path is None
    row.append(_outcome(agg.aggregate_grads, clients))
    row.append(repr(agg.agg_path))
    return row


def wire_row(scheme, key, cond, raws):
    agg = _aggregator(scheme, key, cond, len(raws))
    return [_outcome(agg.aggregate_wire, raws), repr(agg.agg_path)]


def tabulate(grads_fields, grads_rows, wire_fields, wire_rows):
    """The dict a routes file holds.  ``grads_rows()`` / ``wire_rows()`` give every case's row of
    outcomes; they run with the device sentinel in place."""
    from openmsftl_amd import aggregation as ag
    from openmsftl_amd import build
    build.build(verbose=False)
    outcomes, index = [], {}

    def ids(row):
        for s in row:
            if s not in index:
                index[s] = len(outcomes)
                outcomes.append(s)
        return tuple(index[s] for s in row)

    def fold(rows):
        distinct, where, cases = [], {}, []
        for r in rows:
            r = ids(r)
            if r not in where:
                where[r] = len(distinct)
                distinct.append(list(r))
            cases.append(where[r])
        return distinct, cases

    saved = ag._device_of
    ag._device_of = _reach
    try:
        g_rows, g_cases = fold(grads_rows())
        w_rows, w_cases = fold(wire_rows())
    finally:
        ag._device_of = saved
    return {"grads_fields": list(grads_fields), "wire_fields": list(wire_fields),
            "outcomes": outcomes, "grads_rows": g_rows, "grads_cases": g_cases,
            "wire_rows": w_rows, "wire_cases": w_cases}


def table():
    """The whole table as the dict ``routes.json`` holds."""
    return tabulate(GRADS_FIELDS, lambda: (grads_row(*c[1:]) for c in grads_cases()),
                    WIRE_FIELDS, lambda: (wire_row(*c[1:]) for c in wire_cases()))


def dumps(tab) -> str:
    return json.dumps(tab, sort_keys=True, separators=(",", ":")) + "\n"


def main():
    tab = table()
    with open(OUT, "w") as fh:
        fh.write(dumps(tab))
    print(f"{len(tab['grads_cases'])} aggregate_grads cases ({len(tab['grads_rows'])} distinct rows), "
          f"{len(tab['wire_cases'])} aggregate_wire cases ({len(tab['wire_rows'])} distinct rows), "
          f"{len(tab['outcomes'])} distinct outcomes -> {OUT}")


if __name__ == "__main__":
    sys.dont_write_bytecode = True
    main()
