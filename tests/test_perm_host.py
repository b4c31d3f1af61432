"""Device ``np.random.permutation`` ('rand' rows, openmsftl_amd/csrc/fc_perm.hip): what can be
checked without a GPU.

A. tests/perm_model.py — the NumPy restatement of the kernels' parse, backward trace and
   state-after stages over the oracle's raw MT19937 stream — equals
   ``np.random.permutation(n)[:k]``, order included, and the RNG state after the call.
B. The C ABI: struct size, sizes as host functions, argument errors before the GPU is touched
   (header / exports / bindings: tests/test_lib_abi.py).
C. The switches: ``row_plan(..., device_perm=)`` and ``Compression({"device_permutation": ..})``
   default off and plan the rows as the issue states.
"""
import ctypes

import numpy as np
import pytest

import perm_model as pm
from oracle import mt19937 as mt


# ---- A: the model against NumPy ---------------------------------------------------------------
def _odd_state(seed, skip):
    np.random.seed(seed)
    if skip:
        np.random.bytes(4 * skip)              # `skip` 32-bit outputs
    return mt.state_key_pos()


@pytest.mark.parametrize("n", [2, 3, 5, 64, 65, 1000, 65536, 65537, 200003])
def test_model_equals_numpy_permutation_and_state(n):
    for skip in (0, 397):
        key, pos = _odd_state(n + 11, skip)
        want = np.random.permutation(n)
        key2, pos2 = mt.state_key_pos()
        for k in sorted({n, n // 10, 1}):
            idx, (ka, pa), consumed = pm.permutation(key, pos, n, k)
            assert idx.dtype == np.uint32 and np.array_equal(idx, want[:k]), (n, k, skip)
            assert np.array_equal(ka, key2) and pa == pos2, (n, k, skip)
            ke, pe = mt.advance(key, pos, consumed)
            assert np.array_equal(ke, key2) and pe == pos2
        assert n - 1 <= consumed <= pm.budget(n)


def test_model_parse_takes_both_paths_and_reports_a_short_budget():
    n = 200003
    key, pos = _odd_state(5, 1)
    words = mt.outputs(key, pos, pm.budget(n))
    J, consumed, slow = pm.parse(words, n)
    groups = (consumed + pm.GROUP - 1) // pm.GROUP
    # every mask crossing (17) and the groups with a word within 255 of the threshold: all of
    # the tail (i < 2^16: ~360 groups of 256 words) plus 256 * 255 / 2^b of the epochs above it
    # (~180 of 360 groups for b = 17, ~100 of 390 for b = 18 at this n): ~640 of ~1140
    assert 17 <= slow < groups * 3 // 4
    assert all(int(J[i]) <= i for i in (1, 2, 63, 64, 65535, 65536, n - 1))
    idx, (ka, pa), c = pm.permutation(key, pos, 4099, 10, max_words=4099)
    assert idx is None and c == 0 and pa == pos and np.array_equal(ka, key)


def test_untemper_inverts_temper():
    y = np.random.default_rng(3).integers(0, 2 ** 32, 4096, dtype=np.uint64).astype(np.uint32)
    assert np.array_equal(pm.untemper(mt.temper(y)), y)


# ---- B: the C ABI -----------------------------------------------------------------------------
@pytest.fixture(scope="module")
def lib():
    from openmsftl_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def test_state_struct_and_sizes(lib):
    from openmsftl_amd import _lib
    assert ctypes.sizeof(_lib.PermState) == 2520
    assert _lib.PermState.pos.offset == 2496 and _lib.PermState.fallback.offset == 2500
    assert _lib.PermState.rows_done.offset == 2504 and _lib.PermState.consumed.offset == 2512
    sizes = [0, 1, 2, 3, 64, 1000, 30719, 30720, 30721, 65536, 65537, 200003, 2097153,
             25_500_000, 2 ** 31 - 1]
    ws = [lib.fc_mt_perm_workspace_bytes(n) for n in sizes]
    pl = [lib.fc_mt_perm_plan_bytes(n) for n in sizes]
    assert all(a <= b for a, b in zip(ws, ws[1:])) and all(a <= b for a, b in zip(pl, pl[1:]))
    assert ws[0] > 0 and pl[0] > 0
    for n, w in zip(sizes, ws):                # J + the word budget, at the least
        assert w >= 4 * n + 4 * (2 * n + 4096)
    assert lib.fc_mt_perm_workspace_bytes(2 ** 31) == 0 and lib.fc_mt_perm_plan_bytes(2 ** 31) == 0
    assert lib.fc_abi_version() == 4


def test_argument_errors_do_not_touch_gpu(lib):
    buf = ctypes.create_string_buffer(1024)
    addr = (ctypes.addressof(buf) + 255) & ~255
    n = 1000
    pb, wb = lib.fc_mt_perm_plan_bytes(n), lib.fc_mt_perm_workspace_bytes(n)

    def call(plan=addr, plan_bytes=pb, n=n, k=10, state=addr, idx=addr, mask=addr, ws=addr,
             ws_bytes=wb):
        return lib.fc_mt_permutation(plan, plan_bytes, n, k, 0, state, idx, mask, ws, ws_bytes, None)

    assert call(k=n + 1) == -1 and b"k=1001 > n=1000" in lib.fc_last_error()
    assert call(n=2 ** 31, k=0, plan_bytes=1 << 40, ws_bytes=1 << 40) == -1
    assert b"2^31" in lib.fc_last_error()
    for kw in ({"plan": None}, {"state": None}, {"ws": None}):
        assert call(**kw) == -1 and b"non-NULL" in lib.fc_last_error(), kw
    assert call(idx=None, mask=None) == -1 and b"both NULL" in lib.fc_last_error()
    assert call(ws=addr + 4) == -1 and b"aligned" in lib.fc_last_error()
    assert call(ws_bytes=wb - 1) == -3 and b"workspace" in lib.fc_last_error()
    assert call(plan_bytes=pb - 1) == -3 and b"plan" in lib.fc_last_error()
    assert lib.fc_mt_perm_plan(2 ** 31, addr, 1 << 40, None) == -1
    assert lib.fc_mt_perm_plan(n, None, pb, None) == -1
    assert lib.fc_mt_perm_plan(n, addr, pb - 1, None) == -3
    key = (ctypes.c_uint32 * 624)()
    assert lib.fc_mt_perm_begin(None, 0, addr, None) == -1
    assert lib.fc_mt_perm_begin(key, 0, None, None) == -1
    assert lib.fc_mt_perm_begin(key, 625, addr, None) == -1 and b"pos=625" in lib.fc_last_error()
    assert lib.fc_mt_perm_timing(0, (ctypes.c_double * 5)()) == -1     # nothing timed yet


# ---- C: the switches --------------------------------------------------------------------------
class _Client:
    def __init__(self, cid, grad, C):
        self.client_id, self.grad, self.C = cid, grad, C


RAND = {"compression_function": "rand", "fraction_coordinate": 0.1}
TOP = {"compression_function": "top", "fraction_coordinate": 0.1}
FULL = {"compression_function": "full"}
DROP = {"compression_function": "dropout-biased", "dropout_p": 0.1}
PHILOX = {"compression_function": "rand", "fraction_coordinate": 0.2, "rng": "philox", "seed": 3}


def _clients(cfgs, n):
    from openmsftl_amd import Compression
    return [_Client(i, np.zeros(n, np.float32), Compression(c)) for i, c in enumerate(cfgs)]


def _shape(plan):
    return [(r.kind, r.mask_src) for r in plan.specs], sorted(plan.draws), plan.mt_rows


def test_switches_default_off():
    from openmsftl_amd import Compression, aggregation, compression
    assert compression.DEVICE_PERM is False and aggregation.DEVICE_PERM is False
    assert Compression(RAND).device_permutation is False
    assert Compression({}).device_permutation is False
    assert Compression(dict(RAND, device_permutation=True)).device_permutation is True


def test_row_plan_is_unchanged_by_default():
    from openmsftl_amd.aggregation import row_plan
    n = 1000
    plan = row_plan(_clients([RAND, TOP, RAND, FULL, PHILOX], n), n)
    assert _shape(plan) == ([("mask", "host"), ("top", "none"), ("mask", "host"),
                             ("dense", "none"), ("top", "none")], [0, 2], 0)
    assert plan.perm_rows == 0
    plan.close(wait=False)


def test_row_plan_device_perm_rows():
    from openmsftl_amd import _lib as L
    from openmsftl_amd.aggregation import row_plan
    n = 1000
    state = np.random.get_state()
    plan = row_plan(_clients([RAND, RAND, dict(RAND, fraction_coordinate=1.0)], n), n,
                    device_perm=True)
    assert [(r.kind, r.mask_src, r.offset, r.k, r.codec) for r in plan.specs] == [
        ("mask", "perm", 0, 100, L.FC_CODEC_RAND), ("mask", "perm", 1, 100, L.FC_CODEC_RAND),
        ("mask", "perm", 2, 1000, L.FC_CODEC_RAND)]
    assert plan.perm_rows == 3 and not plan.draws and plan.mt_rows == 0
    plan.close(wait=False)
    plan = row_plan(_clients([FULL, RAND, TOP, PHILOX, RAND], n), n, device_perm=True)
    assert _shape(plan) == ([("dense", "none"), ("mask", "perm"), ("top", "none"),
                             ("top", "none"), ("mask", "perm")], [], 0)
    assert [plan.specs[i].offset for i in (1, 4)] == [0, 1] and plan.perm_rows == 2
    plan.close(wait=False)
    assert np.array_equal(np.random.get_state()[1], state[1])      # nothing drawn by planning


def test_row_plan_device_perm_keeps_host_draws_next_to_a_numpy_dropout_row():
    from openmsftl_amd.aggregation import row_plan
    n = 1000
    cfgs = [RAND, DROP, TOP, RAND]
    today = row_plan(_clients(cfgs, n), n)
    plan = row_plan(_clients(cfgs, n), n, device_perm=True)
    assert _shape(plan) == _shape(today) == ([("mask", "host"), ("mask", "host"), ("top", "none"),
                                              ("mask", "host")], [0, 1, 3], 0)
    assert plan.perm_rows == 0
    today.close(wait=False)
    plan.close(wait=False)
    # nothing to draw (no numpy 'rand' row) or nothing the device call takes (n < 2): today's plan
    for cfgs, m in (([TOP, FULL, PHILOX], n), ([RAND], 1)):
        plan = row_plan(_clients(cfgs, m), m, device_perm=True)
        assert plan.perm_rows == 0
        plan.close(wait=False)
