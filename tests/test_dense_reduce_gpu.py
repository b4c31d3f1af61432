"""GPU: the dense reduces (k_wsum, k_wsum64, k_div_scalar, k_div_scalar64) through
codec.weighted_sum_dense, codec.div_scalar, gar.FedAvg.aggregate and the hierarchical merge,
against NumPy: oracle.gar_oracle.sequential_weighted_sum / FedAvgOracle, a left-to-right float64
loop from +0.0, x / d and np.mean.

Sizes: the n % 4 tails, odd n (rows of an (M, n) tensor that are not 16-byte aligned), and one
element count past each kernel's grid (4096 x 256 float4 = 4,194,304 float32 elements;
2048 x 256 = 524,288 float64 elements), where the grid-stride loop wraps.

Run on an MI355X:  python -m pytest tests/test_dense_reduce_gpu.py -m gpu -q
"""
import numpy as np
import pytest

from oracle import gar_oracle as go

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

WRAP32 = 4_194_304               # k_wsum / k_div_scalar: 4096 workgroups x 256 threads x 4
WRAP64 = 524_288                 # k_wsum64 / k_div_scalar64: 2048 workgroups x 256 threads


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _codec():
    from openmsftl_amd import codec
    return codec


def _first_diff(got, want):
    u = np.uint32 if got.dtype == np.float32 else np.uint64
    got, want = np.ascontiguousarray(got).ravel(), np.ascontiguousarray(want).ravel()
    d = np.nonzero(got.view(u) != want.view(u))[0]
    if d.shape[0] == 0:
        return "equal"
    i = int(d[0])
    return f"{d.shape[0]} elements differ, first at {i}: got {got[i]!r} want {want[i]!r}"


def _same_bytes(got, want, what=""):
    assert got.dtype == want.dtype and got.shape == want.shape, (got.dtype, want.dtype)
    assert got.tobytes() == want.tobytes(), f"{what}: {_first_diff(got, want)}"


def _same_but_nan(got, want, what=""):
    """test_fedavg_packets_signed_zeros_and_weight_classes' rule: equal NaN positions, equal
    bytes everywhere else."""
    assert got.dtype == want.dtype and got.shape == want.shape
    nan = np.isnan(want)
    np.testing.assert_array_equal(np.isnan(got), nan, err_msg=what)
    _same_bytes(np.where(nan, 0, got).astype(want.dtype), np.where(nan, 0, want).astype(want.dtype), what)


# ---- weighted_sum_dense, float32 --------------------------------------------------------------
def _rows32(M, n, seed):
    rng = np.random.default_rng(seed)
    G = rng.standard_normal((M, n)).astype(np.float32)
    G[rng.random((M, n)) < 0.05] = np.float32(-0.0)
    G[rng.random((M, n)) < 0.05] = np.float32(3e-45)              # denormal
    G[rng.random((M, n)) < 0.02] = np.float32(-1e30)
    w = np.concatenate([[-0.75, 1e-45, -0.0, 0.0], rng.uniform(-1, 1, M)]).astype(np.float32)[:M]
    return G, w


def _wsum32_check(G, w, splits=True):
    codec = _codec()
    M, n = G.shape
    want = go.sequential_weighted_sum(list(G), w)
    assert want.dtype == np.float32
    wt = torch.from_numpy(w)
    as_list = [torch.from_numpy(np.ascontiguousarray(r)).cuda() for r in G]   # own allocations
    as_matrix = torch.from_numpy(G).cuda()                                  # rows r * n * 4 B apart
    for name, rows in (("list", as_list), ("matrix", as_matrix)):
        out = torch.empty(n, dtype=torch.float32, device="cuda")
        assert out.data_ptr() % 16 == 0
        got = codec.weighted_sum_dense(rows, wt, out=out)
        assert got is out
        _same_bytes(out.cpu().numpy(), want, f"{name} M={M} n={n}")
        if not splits:
            continue
        for s in sorted({1, M - 1} - {0, M}):
            part = list(rows.unbind(0)) if isinstance(rows, torch.Tensor) else rows
            out2 = torch.full((n,), 7.0, dtype=torch.float32, device="cuda")
            codec.weighted_sum_dense(part[:s], wt[:s], out=out2)
            codec.weighted_sum_dense(part[s:], wt[s:], out=out2, continue_sum=True)
            _same_bytes(out2.cpu().numpy(), want, f"{name} M={M} n={n} split at {s}")
    return as_matrix


@pytest.mark.parametrize("M,n", [(M, n) for M in (1, 3, 70) for n in (1, 3, 4, 5, 1001)]
                         + [(3, WRAP32 + 5)])
def test_weighted_sum_dense_f32(M, n):
    """k_wsum: fl32(acc + fl32(g w)) in row order from +0, byte for byte, for separately
    allocated rows (every row on the float4 branch) and for the rows of one (M, n) tensor (odd n:
    only every fourth row is 16-byte aligned, so both row branches run in one call); weights with
    a negative, a denormal, -0.0 and 0.0; continue_sum over rows[:s] / rows[s:] gives the same
    bytes.  4,194,304 + 5 wraps the grid-stride loop and ends on an n % 4 tail."""
    G, w = _rows32(M, n, 100 * M + n % 1000)
    Gd = _wsum32_check(G, w)
    if n % 4 and M >= 2:
        ptr = [r.data_ptr() % 16 for r in Gd.unbind(0)]
        assert ptr[0] == 0 and any(ptr), "the (M, n) tensor must mix aligned and unaligned rows"


def test_weighted_sum_dense_f32_nonfinite():
    """inf and NaN in the rows and in the weights (0 x inf, inf - inf): NaN where NumPy has NaN,
    NumPy's bytes elsewhere."""
    codec = _codec()
    M, n = 6, 1001
    G, w = _rows32(M, n, 5)
    rng = np.random.default_rng(6)
    G[rng.random((M, n)) < 0.03] = np.inf
    G[rng.random((M, n)) < 0.03] = -np.inf
    G[rng.random((M, n)) < 0.03] = np.nan
    for wx in ([0.0, -0.0], [np.inf, 0.0], [-np.inf, 1.0], [np.nan, -0.0]):
        w2 = w.copy()
        w2[1], w2[4] = wx
        with np.errstate(all="ignore"):
            want = go.sequential_weighted_sum(list(G), w2)
        assert np.isnan(want).any()
        assert np.isnan(wx[0]) or (~np.isnan(want)).any()      # (a NaN weight makes every sum NaN)
        for rows in ([torch.from_numpy(np.ascontiguousarray(r)).cuda() for r in G],
                     torch.from_numpy(G).cuda()):
            got = codec.weighted_sum_dense(rows, torch.from_numpy(w2))
            _same_but_nan(got.cpu().numpy(), want, f"weights {wx}")


# ---- weighted_sum_dense, float64 --------------------------------------------------------------
def _loop64(G, w):
    """np.sum(G * w[:, None], axis=0) in float64, restated: left to right from +0.0, the product
    rounded before the add (no FMA)."""
    acc = np.zeros(G.shape[1], np.float64)
    with np.errstate(all="ignore"):
        for i in range(G.shape[0]):
            acc = acc + G[i].astype(np.float64) * np.float64(w[i])
    return acc


def _case64(combo, n, seed):
    rng = np.random.default_rng(seed)
    M = 10 if n <= 1001 else 5
    rdt = np.float64 if combo == "f64_w64" else np.float32
    wdt = np.float32 if combo == "f32_w32_out64" else np.float64
    G = (rng.standard_normal((M, n)) * 10.0 ** rng.uniform(-3, 3, (M, 1))).astype(rdt)
    G[rng.random((M, n)) < 0.05] = -0.0
    w = rng.uniform(-1, 1, M).astype(wdt)
    w[2], w[3], w[4] = -0.0, 0.0, np.finfo(wdt).tiny / 4            # signed zeros, a denormal
    if n > 64:
        # columns where a fused multiply-add would differ: acc = -1, then x w with an inexact
        # product.  float64 rows: (1 + 2^-30)(1 - 2^-30) = 1 - 2^-60 rounds to 1, the sum is +0
        # (fused: -2^-60).  float32 rows, float64 weight: (1 + 2^-23)(1 - 2^-40) loses its 2^-63.
        # (float32 x float32 is exact in float64: no such column exists for that combination.)
        c = slice(8, 24)
        G[:, c] = 0
        G[0, c], w[0] = -1.0, 1.0
        if combo == "f64_w64":
            G[1, c], w[1] = 1.0 + 2.0 ** -30, 1.0 - 2.0 ** -30
        elif combo == "f32_w64":
            G[1, c], w[1] = np.float32(1.0 + 2.0 ** -23), 1.0 - 2.0 ** -40
        # inf and NaN in the rows (rows 2 and 3 carry the weights -0.0 and 0.0: 0 x inf)
        G[2, 30:34] = [np.inf, -np.inf, np.nan, 1.0]
        G[3, 30:34] = [np.inf, 2.0, 1.0, -np.inf]
        G[4, 40:44] = [np.inf, -np.inf, np.nan, np.inf]
        G[M - 2, 40:44] = [np.inf, np.inf, 1.0, 0.0]
        G[M - 1, n - 1] = np.nan
    return G, w


@pytest.mark.parametrize("n", [1, 1001, WRAP64 + 3, 2 * WRAP64 + 7])
@pytest.mark.parametrize("combo", ["f64_w64", "f32_w64", "f32_w32_out64"])
def test_weighted_sum_dense_f64(combo, n):
    """k_wsum64: float64 rows x float64 weights, float32 rows x float64 weights, and float32 rows
    x float32 weights with out_dtype = float64: fl64(acc + fl64(double(g) w)) in row order from
    +0.0, a float64 result.  524,288 + 3 wraps the grid-stride loop once, 1,048,576 + 7 twice;
    continue_sum over rows[:s] / rows[s:] gives the same bytes."""
    codec = _codec()
    G, w = _case64(combo, n, n % 997 + len(combo))
    M = G.shape[0]
    want = _loop64(G, w)
    if n > 64 and combo != "f32_w32_out64":
        assert (want[8:24] == (0.0 if combo == "f64_w64" else 2.0 ** -23 - 2.0 ** -40)).all()
    kw = {"out_dtype": torch.float64} if combo == "f32_w32_out64" else {}
    Gd, wt = torch.from_numpy(G).cuda(), torch.from_numpy(w)
    got = codec.weighted_sum_dense(Gd, wt, **kw)
    assert got.dtype == torch.float64
    _same_but_nan(got.cpu().numpy(), want, f"{combo} n={n}")
    rows = [torch.from_numpy(np.ascontiguousarray(r)).cuda() for r in G]
    for s in (1, M - 1):
        out = torch.full((n,), 7.0, dtype=torch.float64, device="cuda")
        codec.weighted_sum_dense(rows[:s], wt[:s], out=out, out_dtype=torch.float64)
        codec.weighted_sum_dense(rows[s:], wt[s:], out=out, out_dtype=torch.float64, continue_sum=True)
        _same_but_nan(out.cpu().numpy(), want, f"{combo} n={n} split at {s}")


# ---- div_scalar -------------------------------------------------------------------------------
DIVISORS = (3.0, 7.0, 10.0, 0.1)     # float32(0.1) != 0.1: the float32 kernel divides by float32(d)


def _div_input(n, dt, seed):
    rng = np.random.default_rng(seed)
    x = (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 3, n)).astype(dt)
    tiny = np.finfo(dt).tiny
    x[rng.random(n) < 0.1] = -0.0
    x[rng.random(n) < 0.1] = dt(tiny * 2.5)          # quotients by 3, 7, 10 are denormal
    x[rng.random(n) < 0.05] = dt(-tiny / 8)          # a denormal dividend
    if n >= 4:
        x[n - 1], x[n - 2] = -0.0, dt(tiny * 2.5)
    return x


@pytest.mark.parametrize("n", [1, 2, 3, 4, 5, 1023, WRAP32 + 3])
def test_div_scalar_f32(n):
    codec = _codec()
    x = _div_input(n, np.float32, n)
    for d in DIVISORS:
        want = x / np.float32(d)
        assert want.dtype == np.float32
        xd = torch.from_numpy(x.copy()).cuda()
        assert codec.div_scalar(xd, d) is xd
        _same_bytes(xd.cpu().numpy(), want, f"n={n} d={d}")
    if n >= 1023:
        wide = (x.astype(np.float64) / 0.1).astype(np.float32)
        assert (x / np.float32(0.1)).tobytes() != wide.tobytes(), "0.1 must tell float32(d) from d"
        by3 = x / np.float32(3.0)
        assert ((np.abs(by3) < np.finfo(np.float32).tiny) & (by3 != 0)).any()   # denormal results
        assert (np.signbit(by3) & (by3 == 0)).any()


@pytest.mark.parametrize("n", [1, 3, WRAP64 + 1])
def test_div_scalar_f64(n):
    codec = _codec()
    x = _div_input(n, np.float64, n)
    for d in DIVISORS:
        want = x / d
        xd = torch.from_numpy(x.copy()).cuda()
        assert codec.div_scalar(xd, d) is xd
        _same_bytes(xd.cpu().numpy(), want, f"n={n} d={d}")


def test_div_scalar_f32_refuses_a_misaligned_tensor():
    codec = _codec()
    base = torch.arange(1, 42, dtype=torch.float32, device="cuda")
    x = base[1:]
    assert x.data_ptr() % 16 == 4
    with pytest.raises(ValueError, match="x must be 16-byte aligned"):
        codec.div_scalar(x, 3.0)
    assert base.cpu().numpy().tobytes() == np.arange(1, 42, dtype=np.float32).tobytes()   # not run


# ---- gar.FedAvg.aggregate and the hierarchical merge -----------------------------------------
class _Client:
    """The attributes aggregate_grads reads (aggregation.py:61-63, 76)."""

    def __init__(self, cid, grad, C):
        self.client_id, self.grad, self.C = cid, grad, C


def _np_mean_merge(G, cluster_size):
    """aggregation.py:80-93: np.mean over consecutive clusters, the last takes the remainder."""
    num = G.shape[0] // cluster_size
    assert num > 0, "Too small cluter size: {} // {} == 0".format(G.shape[0], cluster_size)
    bounds = [[i * cluster_size, (i + 1) * cluster_size] for i in range(num)]
    if bounds[-1][1] < G.shape[0]:
        bounds[-1][1] = G.shape[0]
    return np.stack([np.mean(G[s:e, :], axis=0) for s, e in bounds]).astype(G.dtype)


def _round(G, sizes):
    """One Aggregator round of 'full' clients, as test_gpu_aggregator_f64 drives it."""
    from openmsftl_amd.aggregation import Aggregator
    from openmsftl_amd.compression import Compression
    cfg = {"aggregation_scheme": "fed_avg", "num_hierarchies": len(sizes), "cluster_size_list": list(sizes)}
    clients = [_Client(i, G[i].copy(), Compression({"compression_function": "full"}))
               for i in range(G.shape[0])]
    A = Aggregator(cfg)
    A.aggregate_grads(clients)
    return A


def _oracle_round(G, sizes):
    for cs in sizes:
        G = _np_mean_merge(G, cs)
    return go.FedAvgOracle({}).aggregate(G)


def _grads(M, n, dt, seed):
    rng = np.random.default_rng(seed)
    G = (rng.standard_normal((M, n)) * 10.0 ** rng.uniform(-3, 0, (M, 1))).astype(dt)
    G[rng.random((M, n)) < 0.02] = -0.0
    return G


@pytest.mark.parametrize("M,n,dt", [(5, WRAP64 + 3, np.float64), (3, WRAP32 + 5, np.float32)])
def test_fedavg_aggregate_past_one_grid(M, n, dt):
    """FedAvg.aggregate on a host G (the route weighted_sum_dense serves): FedAvgOracle's bytes."""
    from openmsftl_amd.gar import FedAvg
    G = _grads(M, n, dt, M)
    got = FedAvg({}).aggregate(G)
    want = go.FedAvgOracle({}).aggregate(G)
    assert want.dtype == dt
    _same_bytes(got, want, f"FedAvg M={M} n={n}")


@pytest.mark.parametrize("M,n,dt,sizes", [(5, WRAP64 + 3, np.float64, (3,)),
                                          (5, WRAP64 + 3, np.float64, (2, 2)),
                                          (3, WRAP32 + 5, np.float32, (2,))])
def test_hierarchical_merge_past_one_grid(M, n, dt, sizes):
    """merge_stages (weights 1, then div_scalar by the count) and a whole Aggregator round with
    cluster_size_list = sizes: np.mean per cluster, then FedAvgOracle, byte for byte."""
    from openmsftl_amd import aggregation
    G = _grads(M, n, dt, 10 * M + len(sizes))
    merged = G
    for cs in sizes:
        merged = _np_mean_merge(merged, cs)
    got = aggregation.merge_stages(torch.from_numpy(G).cuda(), sizes).cpu().numpy()
    _same_bytes(got, merged, f"merge_stages {sizes}")
    A = _round(G, sizes)
    want = _oracle_round(G, sizes)
    assert A.agg_grad.dtype == want.dtype == dt
    _same_bytes(A.agg_grad, want, f"round {sizes} via {A.agg_path}")


def test_hierarchical_merge_five_clients_sizes_3_2_is_refused_like_the_reference():
    """cluster_size_list = [3, 2] on five clients: the first stage leaves ONE cluster (the last
    cluster takes the remainder, aggregation.py:86-87) and the second finds 1 // 2 == 0 clusters.
    The reference asserts there (aggregation.py:83); the product raises the same assertion and
    aggregates nothing."""
    G = _grads(5, WRAP64 + 3, np.float64, 7)
    with pytest.raises(AssertionError, match="Too small cluter size: 1 // 2 == 0"):
        _oracle_round(G, (3, 2))
    with pytest.raises(AssertionError, match="Too small cluter size: 1 // 2 == 0"):
        _round(G, (3, 2))
