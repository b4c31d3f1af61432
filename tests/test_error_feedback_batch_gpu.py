"""Batched error feedback for 'top' on the GPU (fc_topk_encode_ef_batch and everything above it).

Contract (include/fedcodec.h), per client c of the batch: a_c = fl32(g_c + e_c); packet c is the
top-k packet of a_c (oracle: oracle/packet_oracle.py applied to a_c, the rule
tests/test_error_feedback_gpu.py states); the new residual is +0 at the k selected coordinates
and a_c everywhere else; and every byte equals what the lone call encode_top_ef(g_c, e_c, k)
writes.  Every comparison is byte equality.

Run on an MI355X:  python -m pytest tests/test_error_feedback_batch_gpu.py -m gpu -q
"""
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


def scaled_gaussian(n, seed_a, seed_b, scale=1.0):
    """N(0, 1) times 10^U(-4, 1) per element, times the client's scale."""
    g = np.random.default_rng(seed_a).standard_normal(n, dtype=np.float32)
    g *= np.float32(10.0) ** np.random.default_rng(seed_b).uniform(-4, 1, n).astype(np.float32)
    g *= np.float32(scale)
    return g


def k_of(n, f):
    return co.effective_k(co.num_kept(f, n), n)


@functools.lru_cache(maxsize=32)
def client_inputs(n, f, c):
    """Client c's g, and a residual of comparable scale that is zero where a previous top-k took
    the coordinate, as a real residual is.  Another seed and scale per client.  Read-only."""
    k = k_of(n, f)
    scale = 10.0 ** ((c % 7) - 3)
    g = scaled_gaussian(n, 7 * n + int(f * 1000) + 1009 * c, n + c, scale)
    e = scaled_gaussian(n, 13 * n + int(f * 1000) + 1013 * c + 1, n + c + 1, scale)
    e[po.selected_indices(po.mag_key(e), k)] = np.float32(0.0)
    g.setflags(write=False)
    e.setflags(write=False)
    return g, e


def dev(x):
    return torch.from_numpy(np.array(x, dtype=np.float32)).cuda()      # (a writable copy)


def hdr_bytes(pkt):
    return pkt.hdr.cpu().numpy().tobytes()


def check_against_oracle(g, e, k, pkt, res_out):
    """Entries (ascending, values a[idx]), cnt, qoff, the 96-B header, the decoded q and the new
    residual of one client against packet_oracle on a = g + e."""
    from openmsftl_amd import _lib as L
    codec = _codec()
    n = g.shape[0]
    a, want_idx, want_q, want_res = ef_expect(g, e, k)
    keys = po.mag_key(a)
    idx, val, h = pkt.raw_entries()
    assert h.status == 0
    assert np.all(np.diff(idx.astype(np.int64)) > 0), "packet indices must ascend"
    assert val.tobytes() == a[idx].tobytes()
    assert np.uint64(h.thresh) == po.threshold(keys, k)
    c = po.comps(keys)[idx]
    kept = c >= np.uint64(h.thresh)
    np.testing.assert_array_equal(idx[kept], want_idx)
    assert kept.sum() == k and h.n_entries == len(idx) >= k
    assert np.uint64(h.lower) <= np.uint64(h.thresh)
    assert len(c) == 0 or c.min() >= np.uint64(h.lower)
    # the listed entries laid out by the oracle's packet builder: counts and quarter offsets
    want = po.build_idxval(n, idx, val, thresh=h.thresh, lower=h.lower, codec=po.CODEC_TOP, k=k)
    assert pkt.cnt.cpu().numpy().view(np.uint32).tobytes() == want["cnt"].tobytes()
    assert pkt.qoff.cpu().numpy().view(np.uint64).tobytes() == want["qoff"].tobytes()
    # the header: every static field (magnitude keys: seed and offset 0), then all 96 bytes
    assert (h.codec, h.format, h.n, h.k, h.key_mode) == \
        (L.FC_CODEC_TOP, L.FC_FMT_IDXVAL, n, k, L.FC_KEY_MAGNITUDE)
    assert (h.seed, h.offset, h.p, h.chunk, h.index_bits) == (0, 0, 0.0, 8192, po.index_bits(n))
    assert tuple(h.reserved) == (0, 0, 0)
    wh = want["hdr"].copy()
    wh["n_definite"], wh["n_cand"] = h.n_definite, h.n_cand    # (encoder diagnostics)
    assert hdr_bytes(pkt) == wh.tobytes()
    assert codec.decode(pkt).cpu().numpy().tobytes() == want_q.tobytes()
    assert res_out.cpu().numpy().tobytes() == want_res.tobytes()
    return want_q, want_res


def check_against_lone(g, e, k, pkt, res_out):
    """raw_entries() bytes, cnt, qoff, header bytes and res_out against encode_top_ef run alone.
    Returns the lone packet."""
    codec = _codec()
    lone, lone_res = codec.encode_top_ef(dev(g), None if e is None else dev(e), k)
    (i1, v1, _), (i2, v2, _) = pkt.raw_entries(), lone.raw_entries()
    assert i1.tobytes() == i2.tobytes() and v1.tobytes() == v2.tobytes()
    assert torch.equal(pkt.cnt, lone.cnt) and torch.equal(pkt.qoff, lone.qoff)
    assert hdr_bytes(pkt) == hdr_bytes(lone)
    assert torch.equal(res_out.view(torch.int32), lone_res.view(torch.int32))
    return lone


def run_batch(gs, es, k, **kw):
    """One encode_top_ef_batch call on fresh device copies; checks that no g and no residual
    input was written.  Returns (packets, residuals_out)."""
    codec = _codec()
    gd = [dev(g) for g in gs]
    ed = [None if e is None else dev(e) for e in es]
    pkts, outs = codec.encode_top_ef_batch(gd, ed, k, **kw)
    for g, e, x, y in zip(gs, es, gd, ed):
        assert x.cpu().numpy().tobytes() == g.tobytes(), "g was written"
        assert y is None or y.cpu().numpy().tobytes() == e.tobytes(), "res_in was written"
    return pkts, outs


# ---- 1. the batch against the oracle and against the lone call ----------------------------
# M = 65: the smallest batch with a partial second client group in the 3-D grid; 8193: one full
# chunk plus a one-element partial chunk; all three n end in a partial chunk
@pytest.mark.parametrize("f", [0.1, 0.01])
@pytest.mark.parametrize("n", [8193, 100_003, (1 << 20) + 17])
@pytest.mark.parametrize("M", [1, 3, 65])
def test_batch_equals_oracle_and_lone_call(M, n, f):
    k = k_of(n, f)
    ins = [client_inputs(n, f, c) for c in range(M)]
    pkts, outs = run_batch([g for g, _ in ins], [e for _, e in ins], k)
    assert len(pkts) == len(outs) == M
    for (g, e), pkt, out in zip(ins, pkts, outs):
        check_against_oracle(g, e, k, pkt, out)
        lone = check_against_lone(g, e, k, pkt, out)
        if n >= 100_003:
            # no silent fallback: these inputs need no exact re-encode, neither alone (the
            # reference of this condition) nor in the batch
            assert lone.retried is False
            assert pkt.retried is False


# ---- 2. clients that differ inside one batch ------------------------------------------------
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
    g[[0, n - 1]] = [np.nan, -np.inf]                   # the first element of two chunks
    e[[0, n - 1]] = [1.0, 2.0]
    return g, e


def test_clients_that_differ_inside_one_batch():
    n, f = 100_003, 0.1
    k = k_of(n, f)
    g0, _ = client_inputs(n, f, 0)
    g1, _ = client_inputs(n, f, 1)
    ties_g = np.random.default_rng(31).integers(-2, 3, n).astype(np.float32)
    ties_e = np.random.default_rng(32).integers(-2, 3, n).astype(np.float32)
    eg, ee = _edge_inputs()                             # padded to the batch length
    pad = client_inputs(n, f, 2)
    edge_g = np.concatenate([eg, pad[0][8193:]])
    edge_e = np.concatenate([ee, pad[1][8193:]])
    gs = [g0, g1, ties_g, edge_g, client_inputs(n, f, 3)[0]]
    es = [None, -g1, ties_e, edge_e, client_inputs(n, f, 3)[1]]
    pkts, outs = run_batch(gs, es, k)
    assert not np.add(gs[1], es[1]).any()               # client 1's sum is all zeros
    for g, e, pkt, out in zip(gs, es, pkts, outs):
        check_against_lone(g, e, k, pkt, out)
        check_against_oracle(g, np.zeros_like(g) if e is None else e, k, pkt, out)
    sel = po.selected_indices(po.mag_key(np.add(edge_g, edge_e)), k)
    r = outs[3].cpu().numpy()
    assert not np.isnan(r[sel]).any() and not np.signbit(r[sel]).any()   # +0, never NaN


# ---- 3. one client retried, the others not ---------------------------------------------------
def test_one_client_retried_the_others_not():
    codec = _codec()
    M, n, f, bad = 4, 100_003, 0.1, 2
    k = k_of(n, f)
    ins = [client_inputs(n, f, c) for c in range(M)]
    pkts, outs = run_batch([g for g, _ in ins], [e for _, e in ins], k, check=False)
    assert all(p.retried is False for p in pkts)
    assert [h.status for h in codec.headers(pkts)] == [0] * M
    # client `bad` reports RETRY_EXACT: its packet and residual are then invalid by contract
    status = pkts[bad].hdr[36:40]                        # fc_packet_hdr.status
    status.copy_(torch.tensor([1, 0, 0, 0], dtype=torch.uint8))
    outs[bad].fill_(float("nan"))
    pkts[bad].cnt.zero_()
    assert pkts[bad].header().status == 1
    assert codec.resolve(pkts) == 1
    assert [p.retried for p in pkts] == [c == bad for c in range(M)]
    for (g, e), pkt, out in zip(ins, pkts, outs):
        _, idx, want_q, want_res = ef_expect(g, e, k)
        assert codec.decode(pkt).cpu().numpy().tobytes() == want_q.tobytes()
        assert out.cpu().numpy().tobytes() == want_res.tobytes()
        h = pkt.header()
        assert h.status == 0 and np.uint64(h.thresh) == po.threshold(po.mag_key(np.add(g, e)), k)
    for c in (0, 1, 3):                                  # untouched by the resolve
        check_against_oracle(*ins[c], k, pkts[c], outs[c])
    i_bad, v_bad, h_bad = pkts[bad].raw_entries()        # the exact chain lists no slack
    a_bad, idx_bad, _, _ = ef_expect(*ins[bad], k)
    assert h_bad.n_entries == k and i_bad.tobytes() == idx_bad.tobytes()
    assert v_bad.tobytes() == a_bad[idx_bad].tobytes()
    assert codec.resolve(pkts) == 0


# ---- 4. trivial k ------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["zero", "all"])
def test_trivial_k(which):
    M, n = 3, 100_003
    ins = [client_inputs(n, 0.1, c) for c in range(M)]
    k = 0 if which == "zero" else n
    pkts, outs = run_batch([g for g, _ in ins], [e for _, e in ins], k)
    for (g, e), pkt, out in zip(ins, pkts, outs):
        a, idx, want_q, want_res = ef_expect(g, e, k)
        assert len(idx) == k
        h = pkt.header()
        assert h.status == 0 and h.n_entries == k and (h.n, h.k) == (n, k)
        assert _codec().decode(pkt).cpu().numpy().tobytes() == want_q.tobytes()
        assert out.cpu().numpy().tobytes() == want_res.tobytes()
        assert want_res.tobytes() == (a if k == 0 else np.zeros(n, np.float32)).tobytes()


# ---- 5. Python argument errors, before any launch ---------------------------------------------
def test_python_argument_errors_raise_before_any_launch():
    codec = _codec()
    n, k, M = 8193, 819, 3
    gs = [dev(client_inputs(n, 0.1, c)[0]) for c in range(M)]
    es = [dev(client_inputs(n, 0.1, c)[1]) for c in range(M)]
    slab = torch.full((2 * n + 8,), 7.0, dtype=torch.float32, device="cuda")
    ok = [torch.full((n,), 7.0, dtype=torch.float32, device="cuda") for _ in range(M)]

    def call(outs, grads=gs, res=es):
        with pytest.raises(ValueError):
            codec.encode_top_ef_batch(grads, res, k, residuals_out=outs)

    call([ok[0], slab[:n], slab[n - 5:2 * n - 5]])       # two outputs overlap by 5 elements
    call([ok[0], ok[1], ok[1]])                          # the same output twice
    call([ok[0], gs[2], ok[2]])                          # an output is another client's gradient
    call([es[1], ok[1], ok[2]])                          # ... or another client's residual
    call([ok[0], ok[1], torch.empty(n + 4, dtype=torch.float32, device="cuda")])   # wrong length
    call(ok, res=[es[0], es[1], torch.zeros(n - 1, dtype=torch.float32, device="cuda")])
    call([ok[0], ok[1], slab[1:n + 1]])                  # misaligned output
    call(ok, grads=[gs[0], slab[1:n + 1], gs[2]])        # misaligned gradient
    call(ok[:2])                                         # one output per gradient
    torch.cuda.synchronize()
    for t in ok + [slab]:                                # nothing was launched: nothing written
        assert bool((t == 7.0).all())


# ---- 6. chained rounds ----------------------------------------------------------------------
def test_chained_rounds():
    codec = _codec()
    M, n, f, rounds = 4, 100_003, 0.01, 3
    k = k_of(n, f)
    e_np = [np.zeros(n, np.float32) for _ in range(M)]
    e_dev = [torch.zeros(n, dtype=torch.float32, device="cuda") for _ in range(M)]
    spare = [torch.empty(n, dtype=torch.float32, device="cuda") for _ in range(M)]
    for r in range(rounds):
        gs = [scaled_gaussian(n, 1000 * n + 10 * r + c, 77 + 10 * r + c, 10.0 ** (c - 2))
              for c in range(M)]
        pkts, new = codec.encode_top_ef_batch([dev(g) for g in gs], e_dev, k, residuals_out=spare)
        assert all(x is y for x, y in zip(new, spare))
        assert all(p.retried is False for p in pkts)
        for c in range(M):
            _, e_np_next = check_against_oracle(gs[c], e_np[c], k, pkts[c], new[c])
            e_np[c] = e_np_next
        e_dev, spare = list(new), e_dev               # the device residuals carry over


# ---- 7. fold -------------------------------------------------------------------------------------
def test_packets_fold_with_decode_accumulate():
    codec = _codec()
    M, n, f = 4, 100_003, 0.1
    k = k_of(n, f)
    ins = [client_inputs(n, f, c) for c in range(M)]
    pkts, _ = run_batch([g for g, _ in ins], [e for _, e in ins], k)
    rows = [ef_expect(g, e, k)[2] for g, e in ins]
    w = np.full(M, 1.0 / M, np.float32)
    agg = codec.decode_accumulate(pkts, list(w)).cpu().numpy()
    want = go.FedAvgOracle({}).aggregate(go.build_dense_G(rows, np.float32))
    assert agg.tobytes() == want.tobytes()


# ---- 8. the Aggregator's opt-in "ef-batch" route --------------------------------------------
AGG_M, AGG_N, AGG_F = 5, 100_003, 0.05


def _as_np(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else x


def _clients():
    from openmsftl_amd import Compression
    cfg = {"compression_function": "top", "fraction_coordinate": AGG_F, "error_feedback": True}
    return [types.SimpleNamespace(C=Compression(dict(cfg)), grad=None, client_id=i)
            for i in range(AGG_M)]


def _two_group_budget():
    """A device budget that holds the aggregate and two clients of the "ef-batch" route."""
    from openmsftl_amd import _lib as L
    from openmsftl_amd.pipeline import packet_bytes
    per = 8 * AGG_N + packet_bytes(AGG_N) + int(L.load().fc_workspace_bytes(AGG_N))
    return 4 * AGG_N + 2 * per + per // 2


def _round_grads(r):
    return [scaled_gaussian(AGG_N, 200 + 10 * r + i, 300 + 10 * r + i, 10.0 ** (i - 2))
            for i in range(AGG_M)]


@pytest.mark.parametrize("weights", [None, [0.4, 0.3, 0.15, 0.1, 0.05]])
def test_aggregator_ef_batch_route(weights):
    from openmsftl_amd import aggregation as ag
    k = k_of(AGG_N, AGG_F)
    batched = ag.Aggregator({"aggregation_scheme": "fed_avg", "batched_error_feedback": True,
                             "device_budget_bytes": _two_group_budget()})
    plain = ag.Aggregator({"aggregation_scheme": "fed_avg"})
    gar = go.FedAvgOracle({})
    if weights is not None:                              # persisted, non-uniform, float32
        for x in (batched.gar, plain.gar, gar):
            x.gradient_weights = np.array(weights, np.float32)
    assert ag.ef_batch_group(batched, AGG_N, AGG_M, ag._device_of(batched)) == 2   # 3 groups
    cb, cp = _clients(), _clients()
    e_np = [np.zeros(AGG_N, np.float32) for _ in range(AGG_M)]
    for r in range(3):
        rows = []
        for i, g in enumerate(_round_grads(r)):
            cb[i].grad, cp[i].grad = g, g.copy()
            _, _, q, e_np[i] = ef_expect(g, e_np[i], k)
            rows.append(q)
        batched.aggregate_grads(cb)
        plain.aggregate_grads(cp)
        assert batched.agg_path == "ef-batch" and plain.agg_path == "dense-fold"
        want = gar.aggregate(go.build_dense_G(rows, np.float32))
        assert batched.agg_grad.dtype == np.float32
        assert batched.agg_grad.tobytes() == want.tobytes() == plain.agg_grad.tobytes()
        for i in range(AGG_M):                            # advanced exactly once this round
            assert _as_np(cb[i].C.get_residual()).tobytes() == e_np[i].tobytes()
            assert _as_np(cp[i].C.get_residual()).tobytes() == e_np[i].tobytes()


def test_aggregator_ef_batch_wrong_residual_length_advances_nobody():
    from openmsftl_amd import aggregation as ag
    agg = ag.Aggregator({"aggregation_scheme": "fed_avg", "batched_error_feedback": True,
                         "device_budget_bytes": _two_group_budget()})
    clients = _clients()
    for c, g in zip(clients, _round_grads(0)):
        c.grad = g
    agg.aggregate_grads(clients)
    assert agg.agg_path == "ef-batch"
    before = [_as_np(c.C.get_residual()) for c in clients]
    clients[-1].C.set_residual(np.zeros(AGG_N + 1, np.float32))   # the last group's client
    for c, g in zip(clients, _round_grads(1)):
        c.grad = g
    with pytest.raises(ValueError, match="reset_residual"):
        agg.aggregate_grads(clients)
    for c, b in zip(clients[:-1], before):
        assert _as_np(c.C.get_residual()).tobytes() == b.tobytes()
    assert _as_np(clients[-1].C.get_residual()).shape == (AGG_N + 1,)
