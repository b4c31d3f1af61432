"""Error feedback for 'top' on the GPU (fc_topk_encode_ef and everything above it).

Contract (include/fedcodec.h): a = fl32(g + e); the packet is the top-k packet of a (oracle:
oracle/packet_oracle.py applied to a); the new residual is +0 at the k selected coordinates
and a everywhere else.  Every comparison is byte equality.

Run on an MI355X:  python -m pytest tests/test_error_feedback_gpu.py -m gpu -q
"""
import ctypes
import functools
import types

import numpy as np
import pytest

from oracle import compression_oracle as co
from oracle import gar_oracle as go
from oracle import packet_oracle as po

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from openmsftl_amd import _lib
    assert _lib.load().fc_abi_version() == 4


def _codec():
    from openmsftl_amd import codec
    return codec


# ---- the expected values: packet_oracle on a, plus the two-line residual rule ------------
def ef_expect(g, e, k):
    """(a, selected indices ascending, dense q, new residual) of one error-feedback call."""
    a = np.add(g, e, dtype=np.float32)
    idx = po.selected_indices(po.mag_key(a), k)
    res = a.copy()
    res[idx] = np.float32(0.0)
    return a, idx, po.decode_dense(a.shape[0], idx, a[idx]), res


def scaled_gaussian(n, seed_a, seed_b):
    """test_top_sizes' gradient family: N(0, 1) times 10^U(-4, 1) per element."""
    g = np.random.default_rng(seed_a).standard_normal(n, dtype=np.float32)
    g *= np.float32(10.0) ** np.random.default_rng(seed_b).uniform(-4, 1, n).astype(np.float32)
    return g


@functools.lru_cache(maxsize=None)
def ef_inputs(n, f):
    """g, and an independent residual of comparable scale that is zero where a previous top-k
    would have taken its coordinate, as a real residual is.  Cached: read-only."""
    k = co.effective_k(co.num_kept(f, n), n)
    g = scaled_gaussian(n, n * 7 + int(f * 1000), n)
    e = scaled_gaussian(n, n * 13 + int(f * 1000) + 1, n + 1)
    e[po.selected_indices(po.mag_key(e), k)] = np.float32(0.0)
    g.setflags(write=False)
    e.setflags(write=False)
    return g, e, k


def dev(x):
    return torch.from_numpy(np.array(x, dtype=np.float32)).cuda()      # (a writable copy)


def check_ef_packet(a, k, pkt, out):
    """tests/test_gpu_parity.py::_check_top_packet, every assertion, stated against a."""
    keys = po.mag_key(a)
    want_idx = po.selected_indices(keys, k)
    want_out = po.decode_dense(a.shape[0], want_idx, a[want_idx])
    assert out.tobytes() == want_out.tobytes()
    idx, val, h = pkt.raw_entries()
    assert h.status == 0
    assert np.all(np.diff(idx.astype(np.int64)) > 0), "packet indices must ascend"
    assert np.uint64(h.thresh) == po.threshold(keys, k)
    c = po.comps(keys)[idx]
    kept = c >= np.uint64(h.thresh)
    np.testing.assert_array_equal(idx[kept], want_idx)
    assert val.tobytes() == a[idx].tobytes()
    assert h.n_entries >= k and kept.sum() == k
    assert np.uint64(h.lower) <= np.uint64(h.thresh)
    assert len(c) == 0 or c.min() >= np.uint64(h.lower)
    if k and h.n_entries > k:
        assert h.lower > 0 or po.comps(keys).min() == 0
    from openmsftl_amd import _lib as L
    assert (h.codec, h.format, h.n, h.k) == (L.FC_CODEC_TOP, L.FC_FMT_IDXVAL, a.shape[0], k)


def run_ef(g, e, k, **kw):
    """One encode_top_ef call; checks g and the residual input are byte-identical after it.
    Returns (packet, decoded dense q, new residual) with the arrays on the host."""
    codec = _codec()
    gd, ed = dev(g), dev(e)
    pkt, rd = codec.encode_top_ef(gd, ed, k, **kw)
    out = codec.decode(pkt).cpu().numpy()
    assert gd.cpu().numpy().tobytes() == g.tobytes(), "g was written"
    assert ed.cpu().numpy().tobytes() == e.tobytes(), "res_in was written"
    return pkt, out, rd.cpu().numpy()


# ---- 1. one call ------------------------------------------------------------------------
SIZES = [5, 4095, 8191, 8192, 8193, 100_003, (1 << 20) + 17, 3_000_001]
FRACS = [0.1, 0.01, 0.5]


@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("f", FRACS)
def test_one_call(n, f):
    g, e, k = ef_inputs(n, f)
    a, _, _, want_res = ef_expect(g, e, k)
    pkt, out, res = run_ef(g, e, k)
    check_ef_packet(a, k, pkt, out)
    assert res.tobytes() == want_res.tobytes()
    if n >= 100_003:
        # the parent's encode_top(a, k) needs no exact re-encode for these inputs: neither may
        # the fast path here (a silent fallback would hide a broken one)
        assert pkt.retried is False


def test_residual_none_means_zeros():
    g, _, k = ef_inputs(100_003, 0.1)
    codec = _codec()
    pkt, rd = codec.encode_top_ef(dev(g), None, k)
    a, _, _, want_res = ef_expect(g, np.zeros_like(g), k)
    check_ef_packet(a, k, pkt, codec.decode(pkt).cpu().numpy())
    assert rd.cpu().numpy().tobytes() == want_res.tobytes()


# ---- 2. exact=True and the fallback chain equal the fast path -----------------------------
def _kept(pkt):
    idx, val, h = pkt.raw_entries()
    ib = np.uint64(po.index_bits(pkt.n))
    c = (po.mag_key(val).astype(np.uint64) << ib) | idx.astype(np.uint64)
    keep = c >= np.uint64(h.thresh)
    return idx[keep], val[keep], int(h.thresh)


@pytest.mark.parametrize("n,f", [(100_003, 0.1), (3_000_001, 0.01)])
def test_exact_and_fallback_chain_equal_fast(n, f):
    from openmsftl_amd import _lib as L
    codec = _codec()
    g, e, k = ef_inputs(n, f)
    p1, o1, r1 = run_ef(g, e, k)
    assert p1.retried is False
    p2, o2, r2 = run_ef(g, e, k, exact=True)
    assert p2.retried is True and p2.header().n_entries == k
    # the chain by hand: fc_ef_sum, the exact encode of the sum, fc_ef_clear
    lib = L.load()
    gd, ed = dev(g), dev(e)
    r3 = torch.empty(n, dtype=torch.float32, device="cuda")
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(lib.fc_ef_sum(gd.data_ptr(), ed.data_ptr(), r3.data_ptr(), n, s), "fc_ef_sum")
    assert r3.cpu().numpy().tobytes() == np.add(g, e, dtype=np.float32).tobytes()
    p3 = codec.encode_top(r3, k, exact=True)
    v = p3.view()
    L.check(lib.fc_ef_clear(ctypes.byref(v), n, r3.data_ptr(), s), "fc_ef_clear")
    o3, r3 = codec.decode(p3).cpu().numpy(), r3.cpu().numpy()
    i1, v1, t1 = _kept(p1)
    for p, o, r in ((p2, o2, r2), (p3, o3, r3)):
        i, v_, t = _kept(p)
        assert i.tobytes() == i1.tobytes() and v_.tobytes() == v1.tobytes() and t == t1
        assert o.tobytes() == o1.tobytes() and r.tobytes() == r1.tobytes()
    a, _, _, want_res = ef_expect(g, e, k)
    check_ef_packet(a, k, p2, o2)
    assert r1.tobytes() == want_res.tobytes()


# ---- 3. tie-heavy input --------------------------------------------------------------------
def test_tie_heavy_small_integers():
    n, f = 100_003, 0.1
    g = np.random.default_rng(31).integers(-2, 3, n).astype(np.float32)
    e = np.random.default_rng(32).integers(-2, 3, n).astype(np.float32)
    k = co.effective_k(co.num_kept(f, n), n)
    a, _, _, want_res = ef_expect(g, e, k)
    pkt, out, res = run_ef(g, e, k)                  # whichever path ran: highest index first
    check_ef_packet(a, k, pkt, out)
    assert res.tobytes() == want_res.tobytes()


# ---- 4. edge values --------------------------------------------------------------------------
def _edge_inputs(n=8193):
    rng = np.random.default_rng(44)
    g = rng.standard_normal(n).astype(np.float32)
    e = (rng.standard_normal(n) * 0.5).astype(np.float32)
    cancel = rng.choice(n, 900, replace=False)        # e = -g: a = +0
    e[cancel] = -g[cancel]
    special = rng.choice(np.setdiff1d(np.arange(n), cancel), 60, replace=False)
    g[special[:20]] = np.nan                            # (e stays finite there: a's NaN / inf
    g[special[20:40]] = np.inf                          # bits are g's on every IEEE machine)
    g[special[40:]] = -np.inf
    mz = np.setdiff1d(np.arange(n), np.concatenate([cancel, special]))[:300]
    g[mz] = np.float32(-0.0)                            # -0 + -0 = -0
    e[mz] = np.float32(-0.0)
    g[[0, n - 1]] = [np.nan, -np.inf]                   # first element, and the partial chunk's
    e[[0, n - 1]] = [1.0, 2.0]
    return g, e


@pytest.mark.parametrize("f", [0.1, 0.001, 0.5])
def test_edge_values(f):
    g, e = _edge_inputs()
    n = g.shape[0]
    k = co.effective_k(co.num_kept(f, n), n)
    a, _, _, want_res = ef_expect(g, e, k)
    assert np.signbit(a[a == 0]).any() and (~np.signbit(a[a == 0])).any()
    pkt, out, res = run_ef(g, e, k)
    check_ef_packet(a, k, pkt, out)
    assert res.tobytes() == want_res.tobytes()
    sel = po.selected_indices(po.mag_key(a), k)
    assert not np.isnan(res[sel]).any() and not np.signbit(res[sel]).any()   # +0, never NaN


@pytest.mark.parametrize("kind", ["cancel", "zeros", "neg_zeros"])
def test_all_zero_sum(kind):
    n, f = 8193, 0.1
    g = np.random.default_rng(45).standard_normal(n).astype(np.float32)
    if kind == "zeros":
        g[:] = 0.0
    elif kind == "neg_zeros":
        g[:] = -0.0
    e = -g if kind == "cancel" else g.copy()
    k = co.effective_k(co.num_kept(f, n), n)
    a, idx, _, want_res = ef_expect(g, e, k)
    assert not a.any() and idx.min() == n - k           # every key ties: the k highest indices
    pkt, out, res = run_ef(g, e, k)
    check_ef_packet(a, k, pkt, out)
    assert res.tobytes() == want_res.tobytes()


def test_resolve_runs_the_fallback_chain_for_a_retried_packet():
    """check=False leaves a RETRY_EXACT packet (8193 equal keys cannot be ranked in the 4096-entry
    list); codec.resolve re-encodes it from g + e (not from g) and rewrites the residual."""
    codec = _codec()
    n, k = 8193, 819
    g = np.full(n, 0.25, np.float32)
    e = np.full(n, 0.5, np.float32)
    gd, ed = dev(g), dev(e)
    pkt, rd = codec.encode_top_ef(gd, ed, k, check=False)
    assert pkt.header().status == 1 and pkt.retried is False
    assert codec.resolve([pkt]) == 1 and pkt.retried is True
    a, _, _, want_res = ef_expect(g, e, k)
    check_ef_packet(a, k, pkt, codec.decode(pkt).cpu().numpy())
    assert rd.cpu().numpy().tobytes() == want_res.tobytes()
    assert gd.cpu().numpy().tobytes() == g.tobytes() and ed.cpu().numpy().tobytes() == e.tobytes()
    assert codec.resolve([pkt]) == 0


@pytest.mark.parametrize("n", [5, 8193, 100_003])
@pytest.mark.parametrize("which", ["zero", "all"])
def test_trivial_k(n, which):
    g, e, _ = ef_inputs(n, 0.1)
    k = 0 if which == "zero" else n
    a, idx, _, want_res = ef_expect(g, e, k)
    pkt, out, res = run_ef(g, e, k)
    check_ef_packet(a, k, pkt, out)
    assert res.tobytes() == want_res.tobytes()
    assert len(idx) == k
    if k == 0:
        assert res.tobytes() == a.tobytes() and pkt.header().n_entries == 0
    else:
        assert res.tobytes() == np.zeros(n, np.float32).tobytes()


# ---- 5. chained rounds -------------------------------------------------------------------------
@pytest.mark.parametrize("n", [100_003, (1 << 20) + 17])
def test_chained_rounds(n):
    codec = _codec()
    f, rounds = 0.01, 4
    k = co.effective_k(co.num_kept(f, n), n)
    e_np = np.zeros(n, np.float32)
    e_dev = torch.zeros(n, dtype=torch.float32, device="cuda")
    spare = torch.empty(n, dtype=torch.float32, device="cuda")
    fold_np = fold_dev = None
    for r in range(rounds):
        g = scaled_gaussian(n, 1000 * n + r, 77 + r)
        a, _, q_np, e_next = ef_expect(g, e_np, k)
        pkt, new = codec.encode_top_ef(dev(g), e_dev, k, residual_out=spare)
        assert new is spare and pkt.retried is False
        out = codec.decode(pkt).cpu().numpy()
        check_ef_packet(a, k, pkt, out)
        e_dev, spare, e_np = new, e_dev, e_next       # the device residual carries over
        fold_np = q_np.copy() if fold_np is None else np.add(fold_np, q_np)
        fold_dev = out.copy() if fold_dev is None else np.add(fold_dev, out)
    e_final = e_dev.cpu().numpy()
    assert e_final.tobytes() == e_np.tobytes()
    # sum of what was sent plus what is still owed: the same sequential fp32 fold either way
    assert np.add(fold_dev, e_final).tobytes() == np.add(fold_np, e_np).tobytes()


# ---- 6. Compression({"error_feedback": True}) -------------------------------------------------
def _as_np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else x


@pytest.mark.parametrize("on_device", [False, True])
def test_compression_error_feedback(on_device):
    from openmsftl_amd import Compression
    n, f = 100_003, 0.1
    k = co.effective_k(co.num_kept(f, n), n)
    C = Compression({"compression_function": "top", "fraction_coordinate": f,
                     "error_feedback": True})
    assert C.get_residual() is None
    e_np = np.zeros(n, np.float32)
    snap = None
    for r in range(3):
        g = scaled_gaussian(n, 500 + r, 600 + r)
        x = dev(g) if on_device else g.copy()
        out = C.compress(x)
        _, _, q_np, e_np = ef_expect(g, e_np, k)
        assert isinstance(out, torch.Tensor) == on_device and out is not x
        assert _as_np(out).dtype == np.float32 and _as_np(out).tobytes() == q_np.tobytes()
        assert _as_np(x).tobytes() == g.tobytes()     # the input is untouched
        res = C.get_residual()
        assert isinstance(res, torch.Tensor) == on_device
        assert _as_np(res).tobytes() == e_np.tobytes()
        if r == 1:
            snap = (res, e_np.copy(), g)
    # get_residual returns a copy; set_residual restores a snapshot: the call repeats exactly
    res, e1, g2 = snap[0], snap[1], scaled_gaussian(n, 502, 602)
    C.set_residual(res)
    assert _as_np(C.get_residual()).tobytes() == e1.tobytes()
    out = C.compress(dev(g2) if on_device else g2.copy())
    _, _, q_np, e2 = ef_expect(g2, e1, k)
    assert _as_np(out).tobytes() == q_np.tobytes()
    assert _as_np(C.get_residual()).tobytes() == e2.tobytes() == e_np.tobytes()
    # a change of n, or a float64 gradient, raises; the residual is left as it was
    with pytest.raises(ValueError):
        C.compress(np.zeros(n + 1, np.float32))
    with pytest.raises((NotImplementedError, ValueError)):
        C.compress(np.zeros(n, np.float64))
    assert _as_np(C.get_residual()).tobytes() == e2.tobytes()
    C.reset_residual()
    assert C.get_residual() is None
    g = scaled_gaussian(n + 1, 9, 10)                 # any length after a reset, from zeros
    out = C.compress(g.copy())
    _, _, q_np, e_new = ef_expect(g, np.zeros_like(g), co.effective_k(co.num_kept(f, n + 1), n + 1))
    assert out.tobytes() == q_np.tobytes() and C.get_residual().tobytes() == e_new.tobytes()


def test_compression_without_the_key_is_unchanged():
    from openmsftl_amd import Compression
    cfg = {"compression_function": "top", "fraction_coordinate": 0.1}
    g = scaled_gaussian(100_003, 1, 2)
    C = Compression(dict(cfg))
    for _ in range(2):                                 # no state: the same answer twice
        out = C.compress(g.copy())
        assert out.tobytes() == co.compress(cfg, g).tobytes()
    assert C.get_residual() is None


# ---- 7. fold ------------------------------------------------------------------------------------
def test_packets_fold_with_decode_accumulate():
    codec = _codec()
    M, n, f = 4, 100_003, 0.1
    k = co.effective_k(co.num_kept(f, n), n)
    rows, pkts = [], []
    for i in range(M):
        g = scaled_gaussian(n, 40 + i, 50 + i)
        e = scaled_gaussian(n, 60 + i, 70 + i)
        pkt, _ = codec.encode_top_ef(dev(g), dev(e), k)
        pkts.append(pkt)
        rows.append(ef_expect(g, e, k)[2])
    w = np.full(M, 1.0 / M, np.float32)
    agg = codec.decode_accumulate(pkts, list(w)).cpu().numpy()
    want = go.FedAvgOracle({}).aggregate(go.build_dense_G(rows, np.float32))
    assert agg.tobytes() == want.tobytes()


def test_aggregator_routes_error_feedback_clients_through_dense_fold():
    from openmsftl_amd import Compression
    from openmsftl_amd.aggregation import Aggregator
    M, n, f = 4, 100_003, 0.05
    k = co.effective_k(co.num_kept(f, n), n)
    cfg = {"compression_function": "top", "fraction_coordinate": f, "error_feedback": True}
    clients = [types.SimpleNamespace(C=Compression(dict(cfg)), grad=None, client_id=i)
               for i in range(M)]
    agg = Aggregator({"aggregation_scheme": "fed_avg"})
    gar = go.FedAvgOracle({})
    e_np = [np.zeros(n, np.float32) for _ in range(M)]
    for r in range(2):
        rows = []
        for i, c in enumerate(clients):
            c.grad = scaled_gaussian(n, 200 + 10 * r + i, 300 + 10 * r + i)
            _, _, q, e_np[i] = ef_expect(c.grad, e_np[i], k)
            rows.append(q)
        agg.aggregate_grads(clients)
        assert agg.agg_path == "dense-fold"
        want = gar.aggregate(go.build_dense_G(rows, np.float32))
        assert agg.agg_grad.dtype == np.float32 and agg.agg_grad.tobytes() == want.tobytes()
        for i, c in enumerate(clients):                # advanced exactly once this round
            assert _as_np(c.C.get_residual()).tobytes() == e_np[i].tobytes()
