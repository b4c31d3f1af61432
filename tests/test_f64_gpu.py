"""GPU: the float64 codec (csrc/fc_f64.hip through fc_topk_dense_f64*, fc_mask_dense_f64) against
NumPy: oracle.compression_oracle.compress, oracle.philox, and plain g * mask / p.

Every expected value is computed on the host; no assertion compares two kernels of the library.
The crafted inputs come from tests/f64_inputs.py, and tests/test_f64_inputs_host.py proves on the
CPU that each reaches its branch (a chunk's candidate slot overflowing, the slack of bin beta, a
cut in the clamped key group, a bracket that misses, hi_none / lo_all plans, the double2 tail).

Run on an MI355X:  python -m pytest tests/test_f64_gpu.py -m gpu -q
"""
import functools

import numpy as np
import pytest

import f64_inputs as fi
from oracle import compression_oracle as co
from oracle import packet_oracle as po
from oracle import philox as ph

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def _codec():
    from openmsftl_amd import codec
    return codec


def _L():
    from openmsftl_amd import _lib
    return _lib


def _first_diff(got: np.ndarray, want: np.ndarray) -> str:
    d = np.nonzero(got.view(np.uint64) != want.view(np.uint64))[0]
    if d.shape[0] == 0:
        return "equal"
    i = int(d[0])
    return (f"{d.shape[0]} elements differ, first at {i}: got {got.view(np.uint64)[i]:#018x} "
            f"want {want.view(np.uint64)[i]:#018x}")


def _same_bytes(got: np.ndarray, want: np.ndarray, what: str = ""):
    assert got.dtype == want.dtype == np.float64 and got.shape == want.shape
    assert got.tobytes() == want.tobytes(), f"{what}: {_first_diff(got, want)}"


# ---- plain sweeps: sizes around the chunk and the full-sample limit, both engines -----------
@pytest.mark.parametrize("n", fi.SWEEP_N)
def test_top_f64_sweep_matches_oracle(n):
    """compress_top_dense_f64 (sampled where 0 < k < n, checked) and exact=True (the radix
    engine) give the oracle's bytes: odd n and n % 8192 in {1, 8191} go through load64_chunk's
    double2 tail, k = 1 and k = n - 1 above 2^20 through the hi_none and lo_all plans, k = n - 1
    cuts inside the group of zeros (the dropped one is the lowest index: +0.0 for a -0.0)."""
    codec = _codec()
    g = fi.sweep(n)
    gd = torch.from_numpy(g).cuda()
    for k in fi.sweep_ks(n):
        want = fi.oracle_top(g, k)
        got = codec.compress_top_dense_f64(gd, k).cpu().numpy()
        _same_bytes(got, want, f"sampled n={n} k={k}")
        got = codec.compress_top_dense_f64(gd, k, exact=True).cpu().numpy()
        _same_bytes(got, want, f"exact n={n} k={k}")


# ---- crafted inputs: the sampled kernels themselves must produce the oracle's bytes ---------
@functools.lru_cache(maxsize=None)
def _clamped(n):
    return fi.clamped(n)


def _crafted(name):
    kind, _, arg = name.partition(":")
    if kind == "overflow":
        return fi.chunk_overflow(edge=arg == "edge")
    if kind == "tie":
        return fi.tie_group(int(arg))[:2]
    n, k = (int(x) for x in arg.split(","))
    return _clamped(n)[0], k


CRAFTED = (["overflow:strat", "overflow:edge", "tie:1", "tie:750", "tie:1499"]
           + [f"clamped:{n},{k}" for n in (100_003, (1 << 20) + 3) for k in fi.CLAMP_KS])


@pytest.mark.parametrize("name", CRAFTED)
def test_top_f64_crafted_sampled_path_matches_oracle(name):
    """check=False, then resolve_f64: the bytes are the oracle's AND resolve_f64 returned 0, so
    k_fused64 / k_resolve64 wrote them and not the exact fallback.  Twice on one workspace: the
    second call meets the state the first left (chist, small_n, fz_seq, the shard totals)."""
    codec = _codec()
    g, k = _crafted(name)
    want = fi.oracle_top(g, k)
    gd = torch.from_numpy(g).cuda()
    for rep in range(2):
        out = codec.compress_top_dense_f64(gd, k, check=False)
        redo = codec.resolve_f64(out)
        _same_bytes(out.cpu().numpy(), want, f"{name} call {rep}")
        assert redo == 0, f"{name} call {rep}: the sampled path reported RETRY"


@functools.lru_cache(maxsize=None)
def _miss():
    g, k = fi.bracket_miss()
    return g, k, fi.oracle_top(g, k)


def test_top_f64_bracket_miss_retries_exactly():
    codec = _codec()
    g, k, want = _miss()
    out = codec.compress_top_dense_f64(torch.from_numpy(g).cuda(), k, check=False)
    assert codec.resolve_f64(out) == 1, "a sample of zeros must miss the bracket"
    _same_bytes(out.cpu().numpy(), want, "bracket miss")


def test_top_f64_unchecked_outputs_keep_their_own_status():
    """Three check=False encodes on one workspace, resolved in reverse order: each output has
    its own status word, only the bracket-miss one is redone, all three are the oracle's."""
    codec = _codec()
    g0, k0, want0 = _miss()
    rng = np.random.default_rng(31)
    g1, g2 = fi.gauss((1 << 20) + 8191, rng), fi.gauss(300_001, rng)
    k1, k2 = co.num_kept(0.1, g1.shape[0]), co.num_kept(0.1, g2.shape[0])
    ins = [(g0, k0, want0), (g1, k1, fi.oracle_top(g1, k1)), (g2, k2, fi.oracle_top(g2, k2))]
    outs = [codec.compress_top_dense_f64(torch.from_numpy(g).cuda(), k, check=False)
            for g, k, _ in ins]
    redo = [codec.resolve_f64(o) for o in reversed(outs)][::-1]
    for j, (o, (_, _, want)) in enumerate(zip(outs, ins)):
        _same_bytes(o.cpu().numpy(), want, f"output {j}")
    assert redo == [1, 0, 0]


# ---- native rand-k on float64: k_engine64<kKeyPhilox> against oracle.philox ------------------
@pytest.mark.parametrize("n", [1000, 24_581, 65_537, 600_001])
@pytest.mark.parametrize("f", [0.1, 0.5])
def test_rand_philox_f64_matches_oracle(n, f):
    """The kept set is the k largest (Philox word >> 1) << 32 | index of oracle.philox, whatever
    g holds (NaN, inf, -0.0: kept elements are bit copies, dropped ones +0.0).  65,537 is one
    element past k_engine64's grid (kEngineGrid = 256 workgroups x 256), 600,001 past
    k_select_dense64's (2048 x 256)."""
    codec, L = _codec(), _L()
    rng = np.random.default_rng(n)
    g = rng.standard_normal(n)
    g[rng.choice(n, 40, replace=False)] = np.repeat([np.nan, -np.nan, np.inf, -np.inf, -0.0], 8)
    g[n - 1] = fi.from_bits(np.array([0xFFF4000000000123], np.uint64))[0]   # negative sNaN, payload
    k = co.num_kept(f, n)
    seed, off = 0xDEADBEEF12345, 7
    out = codec.compress_top_dense_f64(torch.from_numpy(g).cuda(), k, key_mode=L.FC_KEY_PHILOX,
                                       seed=seed, offset=off).cpu().numpy()
    keys = (ph.element_words(n, seed, off) >> np.uint32(1)).astype(np.uint32)
    kept = np.zeros(n, bool)
    kept[po.selected_indices(keys, k)] = True
    assert np.count_nonzero(kept) == k
    _same_bytes(out, np.where(kept, g, 0.0), f"philox rand n={n} f={f}")


# ---- k_mask_dense64 on a float64 gradient -----------------------------------------------------
MASK_SEED, MASK_OFF = 9, 4


@functools.lru_cache(maxsize=None)
def _numpy_has_x86_default_nan() -> bool:
    """NumPy on x86 gives the default NaN 0xFFF8000000000000 for inf * 0 (what x86_mul / x86_div
    in fc_f64.hip reproduce); another host's NaN bits cannot be compared."""
    with np.errstate(all="ignore"):
        r = np.array([np.inf]) * np.array([0], np.int64)
    return int(r.view(np.uint64)[0]) == 0xFFF8000000000000


def _mask_same(got, want, what):
    if _numpy_has_x86_default_nan():
        _same_bytes(got, want, what)
        return
    nan = np.isnan(want)
    what += " (this host's NumPy has another default NaN: NaN entries compared by position only)"
    np.testing.assert_array_equal(np.isnan(got), nan, err_msg=what)
    _same_bytes(np.where(nan, 0.0, got), np.where(nan, 0.0, want), what)


def _mask_gradient(n):
    """Negative values, +-inf, -0.0, denormals and NaNs with payloads (one signalling, one
    negative), wherever n has room; every kind at the head and at the tail."""
    rng = np.random.default_rng(n)
    g = rng.standard_normal(n)
    special = fi.from_bits(np.array([0x7FF4000000000ABC,      # signalling NaN, payload
                                     0xFFF8000000000123,      # negative quiet NaN, payload
                                     0x7FF0000000000000, 0xFFF0000000000000,   # +-inf
                                     0x8000000000000000,      # -0.0
                                     0x0000000000000003, 0x8000000000000007,   # denormals
                                     0x7FF0000000000001], np.uint64))           # sNaN, inf's high word
    m = special.shape[0]
    if n >= 2 * m:
        g[:m] = special
        g[n - m:] = special[::-1]
        if n > 4096:
            pos = rng.choice(n, n // 64, replace=False)
            g[pos] = special[rng.integers(0, m, pos.shape[0])]
    else:
        g[:] = special[(np.arange(n) * 3 + 1) % m]
    return g


def _bits_tensor(mask: np.ndarray) -> "torch.Tensor":
    """Bit i of word i // 32 (little-endian), the mask_bits layout of fc_mask_dense_f64."""
    n = mask.shape[0]
    b = np.zeros((n + 31) // 32 * 32, bool)
    b[:n] = mask != 0
    return torch.from_numpy(np.packbits(b, bitorder="little").view(np.int32).copy()).cuda()


@pytest.mark.parametrize("n", [1, 255, 257, 100_003, 2_097_152 + 259])
def test_mask_dense_f64_byte_exact(n):
    """'dropout-biased' g * mask, 'dropout-unbiased' (g * mask) / p and 'rand' where(mask, g, +0)
    on a float64 g, host mask and native Bernoulli mask (word < round(p 2^32) of oracle.philox),
    p in {0, 0.1, 1}: NumPy's float64 bytes, NaN bits included (-0.0 for a dropped negative, the
    x86 default NaN for inf * 0 and 0 / 0, quieted payloads).  2,097,152 + 259 is past one grid of
    k_mask_dense64 (2048 workgroups x 256 threads x 4 elements)."""
    codec, L = _codec(), _L()
    g = _mask_gradient(n)
    gd = torch.from_numpy(g).cuda()
    words = ph.element_words(n, MASK_SEED, MASK_OFF).astype(np.uint64)
    hrng = np.random.default_rng(3)
    for p in (0.0, 0.1, 1.0):
        thr = round(p * 4294967296.0)
        assert thr == ph.bernoulli_threshold(p)
        native = (words < np.uint64(thr)).astype(np.int64)
        # a host mask need not follow p: with p = 0 a mixed mask also divides kept values by 0
        host = hrng.binomial(1, p if p else 0.37, n).astype(np.int64)
        for name, cid in (("dropout-biased", L.FC_CODEC_DROPOUT_BIASED),
                          ("dropout-unbiased", L.FC_CODEC_DROPOUT_UNBIASED)):
            for src, mask in (("native", native), ("host", host)):
                with np.errstate(all="ignore"):
                    want = g * mask if name == "dropout-biased" else (g * mask) / p
                if src == "native":
                    out = codec.mask_dense_f64(gd, cid, p=p, seed=MASK_SEED, offset=MASK_OFF)
                else:
                    out = codec.mask_dense_f64(gd, cid, p=p, mask_bits=_bits_tensor(mask))
                _mask_same(out.cpu().numpy(), want, f"{name} {src} mask n={n} p={p}")
        out = codec.mask_dense_f64(gd, L.FC_CODEC_RAND, p=p, mask_bits=_bits_tensor(host))
        _same_bytes(out.cpu().numpy(), np.where(host != 0, g, 0.0), f"rand host mask n={n} p={p}")
