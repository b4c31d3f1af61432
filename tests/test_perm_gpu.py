"""Device ``np.random.permutation`` ('rand' rows, openmsftl_amd/csrc/fc_perm.hip) on the GPU.

Expected values come from ``np.random.permutation`` itself, run from the same seeded state:
the ordered indices, the mask words, the RNG state after the call and the number of outputs
consumed (read off the raw MT19937 stream: the block the end key is).  No tolerance anywhere.
"""
import numpy as np
import pytest

from oracle import compression_oracle as co
from oracle import gar_oracle as go
from oracle import mt19937 as mt

pytestmark = pytest.mark.gpu


def _start(seed, pos):
    """A legacy state (key of ``seed``, stream position ``pos``: 624 is a fresh seed's)."""
    np.random.seed(seed)
    key, _ = mt.state_key_pos()
    return key, pos


def _host(key, pos, n, k):
    np.random.set_state(("MT19937", key, pos, 0, 0.0))
    idx = np.random.permutation(n)[:k].astype(np.uint32)
    return (idx,) + mt.state_key_pos()


def _consumed(key, pos, key2, pos2, budget):
    """Outputs between the states: key2 is block b of key's raw sequence."""
    blocks = mt.raw_sequence(key, 624 * ((pos + budget) // 624 + 2)).reshape(-1, 624)
    (b,) = np.nonzero((blocks[:, :4] == key2[:4]).all(axis=1))[0][:1]
    assert np.array_equal(blocks[b], key2)
    return 624 * int(b) + pos2 - pos


def _words(idx, n):
    from openmsftl_amd.compression import bitmask_words
    return bitmask_words(idx.astype(np.int64), n, False)


def _check(n, k, key, pos, device=None):
    from openmsftl_amd import codec
    want, key2, pos2 = _host(key, pos, n, k)
    R = codec.PermRound(n, key, pos, device)
    idx, mask = R.permutation(k)
    ka, pa, fallback, consumed = R.end_state()
    assert fallback == 0
    assert np.array_equal(idx.cpu().numpy().view(np.uint32), want), (n, k, pos)
    assert mask.cpu().numpy().view(np.uint32).tobytes() == _words(want, n).tobytes(), (n, k, pos)
    assert np.array_equal(ka, key2) and pa == pos2, (n, k, pos)
    assert consumed == _consumed(key, pos, key2, pos2, 2 * n + 4096), (n, k, pos)
    assert R.rows_done() == 1
    return R


# ---- A ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [1, 2, 3, 5, 63, 64, 65, 623, 624, 625, 1000, 4099, 65535, 65536,
                               65537])
def test_perm_round_equals_numpy(n):
    for pos in (624, 1, 397, 623):
        key, pos = _start(1000 + n, pos)
        for k in sorted({0, 1, n // 10, n}):
            _check(n, k, key, pos)


@pytest.mark.parametrize("n", [200003, 2097153])
def test_perm_round_equals_numpy_many_segments(n):
    """Several generator segments and workgroups, and (2097153) a 2^21 mask crossing."""
    for pos in (624, 397):
        key, pos = _start(n, pos)
        _check(n, n // 10, key, pos)


def test_perm_round_single_outputs():
    """Only the indices, or only the mask, into the caller's tensors."""
    import torch
    from openmsftl_amd import codec
    n, k = 4099, 409
    key, pos = _start(3, 397)
    want, key2, pos2 = _host(key, pos, n, k)
    R = codec.PermRound(n, key, pos)
    oi = torch.empty(k, dtype=torch.int32, device="cuda")
    idx, mask = R.permutation(k, out_idx=oi)
    assert idx is oi and mask is None
    om = torch.full(((n + 31) // 32,), -1, dtype=torch.int32, device="cuda")
    idx, mask = R.permutation(k, out_mask=om)
    assert idx is None and mask is om
    np.random.set_state(("MT19937", key2, pos2, 0, 0.0))
    second = np.random.permutation(n)[:k].astype(np.uint32)
    assert np.array_equal(oi.cpu().numpy().view(np.uint32), want)
    assert om.cpu().numpy().view(np.uint32).tobytes() == _words(second, n).tobytes()
    ka, pa, fallback, _ = R.end_state()
    assert fallback == 0 and pa == mt.state_key_pos()[1] and np.array_equal(ka, mt.state_key_pos()[0])


# ---- B ----------------------------------------------------------------------------------------
def test_chain_of_five_calls_without_a_host_read():
    from openmsftl_amd import codec
    n = 4099
    key, pos = _start(77, 1)
    ks = [409, 0, n, 1, 2049]
    R = codec.PermRound(n, key, pos)
    got = [R.permutation(k) for k in ks]                  # queued back to back
    np.random.set_state(("MT19937", key, pos, 0, 0.0))
    for k, (idx, mask) in zip(ks, got):
        want = np.random.permutation(n)[:k].astype(np.uint32)
        assert np.array_equal(idx.cpu().numpy().view(np.uint32), want), k
        assert mask.cpu().numpy().view(np.uint32).tobytes() == _words(want, n).tobytes(), k
    key2, pos2 = mt.state_key_pos()
    ka, pa, fallback, consumed = R.end_state()
    assert fallback == 0 and pa == pos2 and np.array_equal(ka, key2)
    assert consumed == _consumed(key, pos, key2, pos2, 5 * (2 * n + 4096))
    assert R.rows_done() == 5


# ---- C ----------------------------------------------------------------------------------------
def test_other_stream_and_indexed_device():
    import torch
    from openmsftl_amd import codec
    n, k = 65537, 6553
    key, pos = _start(9, 623)
    dev = torch.device("cuda", 0)
    side = torch.cuda.Stream(dev)
    with torch.cuda.stream(side):
        _check(n, k, key, pos, dev)
    # begun on the default stream, drawn on another, then on the default one again
    R = codec.PermRound(n, key, pos, dev)
    with torch.cuda.stream(side):
        a = R.permutation(k)
    b = R.permutation(k)
    np.random.set_state(("MT19937", key, pos, 0, 0.0))
    for idx, _ in (a, b):
        want = np.random.permutation(n)[:k].astype(np.uint32)
        assert np.array_equal(idx.cpu().numpy().view(np.uint32), want)
    ka, pa, fallback, _ = R.end_state()
    assert fallback == 0 and pa == mt.state_key_pos()[1] and np.array_equal(ka, mt.state_key_pos()[0])


# ---- D ----------------------------------------------------------------------------------------
def test_forced_fallback_is_sticky_and_leaves_the_state():
    from openmsftl_amd import codec
    n = 4099
    key, pos = _start(5, 397)
    R = codec.PermRound(n, key, pos)
    R.permutation(n // 10, max_words=n)                  # the draw needs ~1.4 n outputs
    ka, pa, fallback, consumed = R.end_state()
    assert fallback == 1 and pa == pos and np.array_equal(ka, key) and consumed == 0
    R.permutation(n // 10)                               # the full budget: draws nothing now
    ka, pa, fallback, consumed = R.end_state()
    assert fallback == 1 and pa == pos and np.array_equal(ka, key) and consumed == 0
    assert R.rows_done() == 0


# ---- E ----------------------------------------------------------------------------------------
def _compress_pair(kind, n, f, budget, monkeypatch):
    import torch
    from openmsftl_amd import Compression, codec
    if budget:
        monkeypatch.setattr(codec.PermRound, "max_words", budget)
    rng = np.random.default_rng(n + int(100 * f))
    g = rng.standard_normal(n).astype(np.float64 if kind == "f64" else np.float32)
    cfg = {"compression_function": "rand", "fraction_coordinate": f}
    out, states = [], []
    for on in (False, True):
        np.random.seed(123)
        np.random.standard_normal(1)                     # has_gauss = 1, and an odd position
        x = torch.from_numpy(g).cuda() if kind == "cuda" else g
        q = Compression(dict(cfg, device_permutation=on)).compress(x)
        if kind == "cuda":
            assert isinstance(q, torch.Tensor) and q.is_cuda
            q = q.cpu().numpy()
        out.append(q)
        states.append(np.random.get_state())
    assert out[0].dtype == out[1].dtype == g.dtype and out[0].tobytes() == out[1].tobytes()
    a, b = states
    assert a[0] == b[0] and np.array_equal(a[1], b[1]) and a[2:] == b[2:] and b[3] == 1
    return out[1]


@pytest.mark.parametrize("kind", ["f32", "cuda", "f64"])
@pytest.mark.parametrize("n", [0, 1, 4099, 65537])
def test_compress_with_the_switch_on(kind, n, monkeypatch):
    for f in (0.1, 1.0, 0.0):
        q = _compress_pair(kind, n, f, 0, monkeypatch)
        assert np.count_nonzero(q) <= round(f * n)


@pytest.mark.parametrize("kind", ["f32", "cuda", "f64"])
def test_compress_host_fallback(kind, monkeypatch):
    """A device call that runs out of its budget: NumPy's own call from the untouched state."""
    _compress_pair(kind, 4099, 0.1, 64, monkeypatch)


# ---- F ----------------------------------------------------------------------------------------
N, M = 40003, 10
RAND = {"compression_function": "rand", "fraction_coordinate": 0.1}
TOP = {"compression_function": "top", "fraction_coordinate": 0.1}
FULL = {"compression_function": "full"}
DROP = {"compression_function": "dropout-unbiased", "dropout_p": 0.25}
PHILOX = {"compression_function": "rand", "fraction_coordinate": 0.2, "rng": "philox", "seed": 3}
ROUNDS = {
    "rand": ([RAND] * M, []),
    "mixed": ([RAND, TOP, FULL, PHILOX, RAND, dict(RAND, fraction_coordinate=1.0), FULL, RAND,
               dict(RAND, fraction_coordinate=0.0), TOP], []),
    "merge": ([RAND] * M, [3]),
    "dropout": ([RAND, DROP, RAND, TOP, RAND, RAND, FULL, RAND, RAND, RAND], []),
}


class _Client:
    def __init__(self, cid, grad, C):
        self.client_id, self.grad, self.C = cid, grad, C


def _budget(n, packets):
    from openmsftl_amd import _lib as L
    from openmsftl_amd.pipeline import packet_bytes
    return 6 * 4 * n + int(L.load().fc_workspace_bytes(n)) + packets * packet_bytes(n)


_cache = {}


def _round(name):
    """The round's gradients and the oracle's (agg_grad, next draw), computed once: the
    reference's loop over the oracle codec (a Philox row, which the reference does not have,
    is the drop-in's own compress() row)."""
    if name not in _cache:
        import torch
        from openmsftl_amd import Compression
        cfgs, sizes = ROUNDS[name]
        rng = np.random.default_rng(len(name))
        grads = [(rng.standard_normal(N) * 10.0 ** rng.uniform(-4, -1)).astype(np.float32)
                 for _ in cfgs]
        np.random.seed(2025)
        rows = [Compression(c).compress(torch.from_numpy(g).cuda()).cpu().numpy()
                if c.get("rng") == "philox" else co.compress(c, g) for c, g in zip(cfgs, grads)]
        nxt = int(np.random.randint(0, 2 ** 31 - 1))
        G = go.build_dense_G(rows, np.float32)
        for cs in sizes:
            G = go.merge_gradient(G, cs)
        _cache[name] = (grads, go.FedAvgOracle({}).aggregate(G), nxt)
    return _cache[name]


def _aggregate(name, on):
    from openmsftl_amd import Compression
    from openmsftl_amd.aggregation import Aggregator
    cfgs, sizes = ROUNDS[name]
    grads, _, _ = _round(name)
    agg = Aggregator({"aggregation_scheme": "fed_avg", "device_budget_bytes": _budget(N, 3),
                      "num_hierarchies": len(sizes), "cluster_size_list": sizes,
                      "device_permutation": on})
    np.random.seed(2025)
    agg.aggregate_grads([_Client(i, g, Compression(c)) for i, (g, c) in enumerate(zip(grads, cfgs))])
    nxt = int(np.random.randint(0, 2 ** 31 - 1))
    assert agg.agg_path == "stream"
    (pipe,) = agg._host_pipelines.values()
    assert pipe.group == 3                                # several fold groups
    return agg, nxt


@pytest.mark.parametrize("name", ["rand", "mixed", "merge"])
def test_aggregator_device_permutation(name):
    _, want, nxt = _round(name)
    off, nxt_off = _aggregate(name, False)
    on, nxt_on = _aggregate(name, True)
    assert off.agg_draws == "host" and on.agg_draws == "device-perm"
    assert on.agg_grad.tobytes() == off.agg_grad.tobytes() == want.tobytes()
    assert nxt_on == nxt_off == nxt


def test_aggregator_keeps_host_draws_next_to_a_numpy_dropout_row():
    _, want, nxt = _round("dropout")
    on, nxt_on = _aggregate("dropout", True)
    assert on.agg_draws == "host"
    assert on.agg_grad.tobytes() == want.tobytes() and nxt_on == nxt


def test_aggregator_forced_fallback_redoes_the_round_on_the_host(monkeypatch):
    from openmsftl_amd import codec
    monkeypatch.setattr(codec.PermRound, "max_words", 64)
    _, want, nxt = _round("rand")
    on, nxt_on = _aggregate("rand", True)
    assert on.agg_draws == "host"
    assert on.agg_grad.tobytes() == want.tobytes() and nxt_on == nxt
