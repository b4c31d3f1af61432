"""The batched scaled-sign encode on the host: the C ABI of fc_sign_encode_batch (the job struct,
the declarations, the workspace size, the argument errors) and that the Aggregator's
"batched_sign_encode" key leaves the routing answers alone.

Run:  python -m pytest tests/test_sign_batch_host.py -m "not gpu" -q

No GPU is needed: the library loads without one (tests/test_lib_abi.py).
"""
import ctypes
import re
import types
import os

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fedcodec.h")
F = np.float32
NEW = {"fc_sign_batch_workspace_bytes": 2, "fc_sign_encode_batch": 8}


@pytest.fixture(scope="module")
def lib():
    from openmsftl_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_sign_job_layout():
    from openmsftl_amd import _lib
    J = _lib.SignJob
    assert ctypes.sizeof(J) == 48
    assert [(name, getattr(J, name).offset) for name, _ in J._fields_] == [
        ("g", 0), ("res_in", 8), ("res_out", 16), ("words", 24), ("hdr", 32), ("reserved", 40)]
    src = open(HEADER).read()
    body = re.search(r"typedef struct fc_sign_job \{(.*?)\} fc_sign_job;", src, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = [re.split(r"[\s*]+", f.strip())[-1] for f in body.split(";") if f.strip()]
    assert fields == [name for name, _ in J._fields_]


def test_new_symbols_are_declared_and_bound(lib):
    """tests/test_lib_abi.py then checks the export of everything the header declares."""
    from openmsftl_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    decl = {name: args.count(",") + 1
            for name, args in re.findall(r"\b(fc_sign_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S)}
    for name, nargs in NEW.items():
        assert decl.get(name) == nargs, name
        assert len(_lib.SIGNATURES[name][1]) == nargs, name
        getattr(lib, name)
    assert lib.fc_abi_version() == 4


def test_batch_workspace_is_a_host_function_monotone_in_m(lib):
    for n in (1, 8193, 1 << 27):
        lone = lib.fc_sign_workspace_bytes(n)
        prev = 0
        for m in (1, 2, 3, 64, 65, 1000, 65535):
            b = lib.fc_sign_batch_workspace_bytes(n, m)
            assert b >= prev and m * lone <= b < m * lone + 256, (n, m, b)
            prev = b
        assert lib.fc_sign_batch_workspace_bytes(n, 1) >= lone


def test_argument_errors_do_not_touch_gpu(lib):
    buf = ctypes.create_string_buffer(1 << 12)
    a = (ctypes.addressof(buf) + 15) & ~15
    n, m = 64, 3
    need = lib.fc_sign_batch_workspace_bytes(n, m)
    good = dict(jobs=a, m=m, n=n, ri=0, ro=0, ws=a + 1024, wsb=need)

    def enc(**kw):
        p = dict(good, **kw)
        return lib.fc_sign_encode_batch(p["jobs"], p["m"], p["n"], p["ri"], p["ro"], p["ws"], p["wsb"], None)
    err = lambda: lib.fc_last_error()                                  # noqa: E731
    assert enc(jobs=None) == -1 and b"NULL" in err()
    assert enc(ws=None) == -1 and b"NULL" in err()
    assert enc(m=0) == -1 and b"m=0" in err()
    assert enc(m=65536) == -1 and b"m=65536" in err()
    assert enc(m=-1) == -1
    assert enc(n=0) == -1 and b"n=0" in err()
    assert enc(n=1 << 32) == -1 and b"n=" in err()
    assert enc(ws=a + 1028) == -1 and b"aligned" in err()
    assert enc(wsb=need - 1) == -3 and b"workspace" in err()
    assert enc(wsb=lib.fc_sign_workspace_bytes(n)) == -3             # one client's is not three's
    for flags in ((1, 0), (0, 1), (1, 1)):                             # the same with residuals
        assert enc(ri=flags[0], ro=flags[1], wsb=16) == -3


# ---- the key and the routing predicates ---------------------------------------------------------
def _clients(m=3, n=100, fn="sign", **cfg):
    from openmsftl_amd import Compression
    return [types.SimpleNamespace(C=Compression(dict({"compression_function": fn}, **cfg)),
                                  grad=np.zeros(n, F), client_id=i) for i in range(m)]


def _agg(scheme="fed_avg", **cfg):
    from openmsftl_amd.aggregation import Aggregator
    return Aggregator(dict({"aggregation_scheme": scheme}, **cfg))


def _answer(fn):
    try:
        return ("ok", fn())
    except (NotImplementedError, ValueError) as e:
        return (type(e).__name__, str(e))


def test_the_key_leaves_round_route_unchanged(lib):
    from openmsftl_amd.aggregation import round_route
    rounds = [
        ({}, lambda: _clients()),
        ({}, lambda: _clients(error_feedback=True)),
        ({}, lambda: _clients(fn="top", fraction_coordinate=0.1)),
        ({}, lambda: _clients() + _clients(1, fn="top", fraction_coordinate=0.1)),
        ({"sign_packets": False}, lambda: _clients()),
        ({"aggregation_scheme": "sign_majority"}, lambda: _clients()),
        ({"aggregation_scheme": "sign_majority", "device_budget_bytes": 1000}, lambda: _clients(m=8, n=4096)),
        ({"aggregation_scheme": "krum"}, lambda: _clients(m=5)),
        ({"aggregation_scheme": "krum", "sign_geometry": True}, lambda: _clients(m=5)),
        ({"aggregation_scheme": "coordinate_median", "sign_trim": True}, lambda: _clients(m=5)),
        ({"aggregation_scheme": "coordinate_median"}, lambda: _clients(m=5)),
        ({"aggregation_scheme": "trimmed_mean", "sign_trim": True, "device_budget_bytes": 1000},
         lambda: _clients(m=5, n=4096)),
        ({"devices": 2}, lambda: _clients()),
    ]
    seen = set()
    for cfg, make in rounds:
        base = dict({"aggregation_scheme": "fed_avg"}, **cfg)
        without = _answer(lambda: round_route(_agg(**base), make()))
        for value in (True, False):
            with_key = _answer(lambda: round_route(_agg(**dict(base, batched_sign_encode=value)), make()))
            assert with_key == without, (cfg, value)
        seen.add(without[0] if without[0] != "ok" else without[1] and without[1][0])
    assert {"sign", "sign-gram", "sign-trim", "NotImplementedError"} <= seen, seen
