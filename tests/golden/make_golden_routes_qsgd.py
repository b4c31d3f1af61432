"""The Aggregator's routing of QSGD clients and QSGD payloads on the host (``routes_qsgd.json``).

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_golden_routes_qsgd.py

The table of make_golden_routes.py predates the QSGD packet; this one covers what it lacks, with
that file's helpers: every scheme and condition, with and without ``qsgd_packets`` (the
``fed_avg+pc`` scheme row under the key is the ``pc_analysis: "gram"`` case), put to ``qsgd_route``
and ``round_route`` on rounds of stub clients and to ``aggregate_wire`` on host-built payloads, the
first touch of the device replaced by the sentinel.  Same file layout as ``routes.json``.

The file was written by this script at the commit BEFORE aggregate_wire's payload kinds were given
one layer and is never regenerated to make tests/test_routes_qsgd_host.py pass.  Only public names
of the package are used, so the script runs unchanged on either side of such a change.
"""
from __future__ import annotations

import itertools
import os
import sys

import numpy as np

import make_golden_routes as mg
from make_golden_routes import CONDITIONS, DEVICE, SCHEMES, F, _aggregator, _clients, _outcome  # noqa: F401

OUT = os.path.join(mg.HERE, "routes_qsgd.json")
N, BITS = 129, (2, 8)

KEYS = (("none", {}),
        ("qsgd_packets", {"qsgd_packets": True}))

GRADS_FIELDS = ("qsgd_route", "round_route")
WIRE_FIELDS = mg.WIRE_FIELDS


def client_rounds():
    def qsgd(m=3, **kw):
        return _clients(m, fn="qsgd", **dict({"qsgd": "native"}, **kw))
    return (("one width", qsgd()),
            ("differing widths", qsgd(2, num_bits=2) + qsgd(1, num_bits=12)),
            ("one with error feedback", qsgd(2) + qsgd(1, error_feedback=True)),
            ("one with num_bits 15", qsgd(2) + qsgd(1, num_bits=15)),
            ("one with num_bits True", qsgd(2) + qsgd(1, num_bits=True)),
            ("one not native", qsgd(2) + _clients(1, fn="qsgd")),
            ("one top", qsgd(2) + _clients(1, fn="top", fraction_coordinate=0.1)),
            ("two lengths", qsgd(2) + qsgd(1, n=101)),
            ("n=0", qsgd(n=0)))


def payload_rounds():
    """(name, payloads, the ``n=`` argument) of each round."""
    import qsgd_ef_model as qm
    import sign_model as sm
    import wire_model as wm
    from oracle import packet_oracle as po
    rng = np.random.default_rng(11)

    def qsgd(n, bits, seed):
        g = rng.standard_normal(n).astype(F)
        _, norm, words, _, _ = qm.encode(g, None, bits, seed, 3)
        return qm.pack(n, bits, seed, 3, norm, words)

    lo = [qsgd(N, BITS[0], i) for i in range(3)]
    hi = [qsgd(N, BITS[1], 10 + i) for i in range(3)]
    bad = bytearray(lo[1])
    bad[qm.WIRE_HDR_BYTES] = (bad[qm.WIRE_HDR_BYTES] & 0xF8) | 5       # element 0: level 5 above s = 4
    sign = sm.pack(N, 1.0, sm.words_of(rng.random(N) < 0.5))
    top = wm.pack(po.build_idxval(N, np.array([3, 50, 100]), F([1, 2, 3]), thresh=0, codec=po.CODEC_TOP, k=3))
    return ((f"qsgd at {BITS[0]} bits", lo, None),
            (f"qsgd at {BITS[1]} bits", hi, None),
            ("qsgd at differing bits", [lo[0], hi[0], lo[1]], None),
            ("qsgd with sign", [lo[0], sign, lo[1]], None),
            ("sign first, then qsgd", [sign, lo[0]], None),
            ("qsgd with top", [lo[0], top, hi[0]], None),
            ("qsgd of two lengths", [lo[0], qsgd(N - 1, BITS[0], 7)], None),
            ("a level above s in payload 1", [lo[0], bytes(bad), lo[2]], None),
            ("n= disagrees", lo, N + 1))


def grads_cases():
    """(case name, scheme, key, condition, clients) in the order of ``routes_qsgd.json``."""
    rounds = client_rounds()
    for scheme, key, cond, (rname, clients) in itertools.product(SCHEMES, KEYS, CONDITIONS, rounds):
        yield f"{scheme[0]} | {key[0]} | {cond[0]} | {rname}", scheme, key, cond, clients


def wire_cases():
    rounds = payload_rounds()
    for scheme, key, cond, (rname, raws, n) in itertools.product(SCHEMES, KEYS, CONDITIONS, rounds):
        yield f"{scheme[0]} | {key[0]} | {cond[0]} | {rname}", scheme, key, cond, raws, n


def grads_row(scheme, key, cond, clients):
    from openmsftl_amd import aggregation as ag
    agg = _aggregator(scheme, key, cond, len(clients))
    row = [_outcome(ag.qsgd_route, agg, clients), _outcome(ag.round_route, agg, clients)]
    assert agg.agg_path is None
    return row


def wire_row(scheme, key, cond, raws, n):
    agg = _aggregator(scheme, key, cond, len(raws))
    return [_outcome(agg.aggregate_wire, raws, n), repr(agg.agg_path)]


def table():
    """The whole table as the dict ``routes_qsgd.json`` holds."""
    return mg.tabulate(GRADS_FIELDS, lambda: (grads_row(*c[1:]) for c in grads_cases()),
                       WIRE_FIELDS, lambda: (wire_row(*c[1:]) for c in wire_cases()))


dumps = mg.dumps


def main():
    tab = table()
    with open(OUT, "w") as fh:
        fh.write(dumps(tab))
    print(f"{len(tab['grads_cases'])} client cases ({len(tab['grads_rows'])} distinct rows), "
          f"{len(tab['wire_cases'])} aggregate_wire cases ({len(tab['wire_rows'])} distinct rows), "
          f"{len(tab['outcomes'])} distinct outcomes -> {OUT}")


if __name__ == "__main__":
    sys.dont_write_bytecode = True
    main()
