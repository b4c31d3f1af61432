"""Crafted float64 gradients for the sampled float64 top-k (csrc/fc_f64.hip), as (g, k).

Every builder aims at ONE branch of k_fused64 / k_resolve64.  tests/test_f64_inputs_host.py
proves on the CPU that each input has the property its branch needs, so the GPU tests of
tests/test_f64_gpu.py cannot pass by missing the branch.  Vocabulary (fc_f64.hip):

  high word   hw(x)    = (|x| bits) >> 32: exponent + 20 mantissa bits, 31 bits
  key32       key32(x) = hw(x), every hw above 0x7f800000 clamped to 0x7f800001 (key32_of):
                         all finite |x| >= 2^1017 (1 + 2^-20), +-inf and every NaN share it
  key64       key64(x) = |x| bits, every NaN 0x7ff0000000000001 (mag_key64)
  comp                 = key64 << 32 | index: the k largest comps are kept (ties: highest index)
  chunk                = 8192 consecutive elements, one k_fused64 workgroup, a 128-entry slot
                         for its candidates (key32 inside the sample's bracket)
"""
import math

import numpy as np

from oracle import compression_oracle as co

CHUNK = 8192
SLOT = 128                       # kC64Slot: candidate comps a chunk's slot holds
SMALL_CAP = 2048                 # kSmallCap64: bin beta's candidates the last arriver sorts
FULL_SAMPLE_MAX = 1 << 20        # kFullSampleMax (fc_state.h)
CLAMP_HW = 0x7F800000            # key32_of: high words above it are one key
NAN_KEY32 = 0x7F800001
N_STRAT = (1 << 20) + CHUNK * 3 + 5          # stratified plan, 132 chunks, odd tail
N_FULL = (1 << 19) + CHUNK * 3 + 5           # full-sample plan, 68 chunks, odd tail
N_MISS = 4 << 20


def bits(g) -> np.ndarray:
    return np.ascontiguousarray(g, dtype=np.float64).view(np.uint64)


def from_bits(u) -> np.ndarray:
    return np.ascontiguousarray(u, dtype=np.uint64).view(np.float64)


def hi_word(g) -> np.ndarray:
    return ((bits(g) & np.uint64(0x7FFFFFFFFFFFFFFF)) >> np.uint64(32)).astype(np.uint32)


def key32(g) -> np.ndarray:
    hw = hi_word(g)
    return np.where(hw > np.uint32(CLAMP_HW), np.uint32(NAN_KEY32), hw)


def key64(g) -> np.ndarray:
    u = bits(g) & np.uint64(0x7FFFFFFFFFFFFFFF)
    return np.where(u > np.uint64(0x7FF0000000000000), np.uint64(0x7FF0000000000001), u)


def kth_key64(g, k: int) -> np.uint64:
    """key64 of the k-th largest magnitude (1 <= k <= n)."""
    ks = key64(g)
    return np.partition(ks, ks.shape[0] - k)[ks.shape[0] - k]


def oracle_top(g: np.ndarray, k: int) -> np.ndarray:
    """oracle.compression_oracle.compress for 'top' with exactly k kept: the fraction is chosen
    so that compression.py:34's round(f * N) gives k."""
    n = g.shape[0]
    f = k / n
    if co.num_kept(f, n) != k:
        f = (k + 0.25) / n
    assert co.num_kept(f, n) == k
    return co.compress({"compression_function": "top", "fraction_coordinate": f}, g.copy())


# ---- the sampling plan of fc_topk_dense_f64_sampled: make_plan(n, k, single = true) ----------
def plan_of(n: int, k: int) -> dict:
    """fc_capi.hip's make_plan for a lone encode (FC_SAMPLE_DIV_SINGLE = 32, at most
    FC_MAX_SAMPLE_SEGS_SINGLE = 2048 segments, at least 64), the fields a test relies on."""
    if n <= FULL_SAMPLE_MAX:
        P = dict(full=True, nseg=(n + 1023) // 1024, r_hi=k, r_lo=k, lo_all=False)
    else:
        seg = min(max(n // 32 // 1024, 64), 2048)
        S = seg * 1024.0
        q = k / n
        rho = q * S
        m = 6.0 * math.sqrt(S * q * (1.0 - q)) + 16.0
        r_hi, r_lo = math.floor(rho - m), math.ceil(rho + m)
        P = dict(full=False, nseg=seg, r_hi=r_hi, r_lo=r_lo, lo_all=r_lo > int(S))
    P["hi_none"] = P["r_hi"] < 1
    return P


def sampled_mask(n: int, k: int) -> np.ndarray:
    """True at every element the sample of a lone encode reads: segment s of P.nseg covers
    [seg_start(P, s), + 1024) (fc_state.h; seg_lane clips a full plan's last segment to n)."""
    P = plan_of(n, k)
    s = np.arange(P["nseg"], dtype=np.int64)
    if P["full"] or P["nseg"] == 1:
        starts = s * 1024
    else:
        starts = ((s * (n - 1024)) // (P["nseg"] - 1)) & ~np.int64(3)
    m = np.zeros(n, bool)
    for st in starts:
        m[st:min(st + 1024, n)] = True
    return m


def gauss(n: int, rng) -> np.ndarray:
    return rng.standard_normal(n) * 10.0 ** rng.uniform(-4, -1)


# ---- chunk overflow --------------------------------------------------------------------------
OVER_BIG, OVER_SMALL = 7, 9      # the chunk with 300 near-threshold values, the one with 60


def chunk_overflow(edge: bool = False, seed: int = 21):
    """Gaussian x 10^U(-4, -1), f = 0.1, plus 300 values in chunk 7 and 60 in chunk 9, all in
    ONE high-word bucket around the cut (spread over half the bucket: every two of them within a
    relative 2^-21), random signs, random low words (no tie).  About half of the 360 land above
    the k-th magnitude, so the cut is inside the cluster: chunk 7 lists > 128 candidates with the
    threshold's key32 and k_resolve64 has to rescan it from g.

    edge = False: n = 2^20 + 3 * 8192 + 5 (stratified plan).
    edge = True:  n = 2^19 + 3 * 8192 + 5 (full-sample plan: the bracket is the ONE fine bin that
    holds the k-th key) and the gradient is scaled so that the cluster's high word is 0x3fefffff,
    |x| in [1 - 2^-21, 1): its low 20 bits are ones.  A fine bin's upper edge is
    klo + ((j + 1) << fs) - 1 with klo a multiple of 2^19 (fc_topk.hip fine_upper / win_of), so for
    every fs <= 19 this high word IS t_hi, the last key of the bracket: the rescan's
    `key <= t_hi` decides whether the whole cluster is seen."""
    rng = np.random.default_rng(seed)
    n = N_FULL if edge else N_STRAT
    g = gauss(n, rng)
    k = co.num_kept(0.1, n)
    pos = np.concatenate([OVER_BIG * CHUNK + rng.choice(CHUNK, 300, replace=False),
                          OVER_SMALL * CHUNK + rng.choice(CHUNK, 60, replace=False)])
    rest = np.sort(np.abs(np.delete(g, pos)))[::-1]
    c = rest[k - 181]            # k - 180 untouched magnitudes are >= c: the cut falls mid-cluster
    if edge:
        g *= (1.0 + 2.0 ** -30) / c          # that magnitude becomes 1 + 2^-30: just above the bucket
        hw = np.uint64(0x3FEFFFFF)
    else:
        hw = np.uint64(hi_word(np.array([c]))[0])
    low = rng.integers(1 << 30, 3 << 30, pos.shape[0], dtype=np.uint64)   # the bucket's middle half
    sign = rng.integers(0, 2, pos.shape[0], dtype=np.uint64) << np.uint64(63)
    g[pos] = from_bits(sign | (hw << np.uint64(32)) | low)
    return g, k


# ---- a tie group on the cut ------------------------------------------------------------------
TIE_BIG = 11                     # the chunk that holds 200 of the 1500 copies
TIE_COUNT = 1500


def tie_group(kept: int, seed: int = 22):
    """n = 2^20 + 3 * 8192 + 5: 1500 copies of one magnitude with mixed signs, 200 in chunk 11 and
    100 in each of 13 other chunks; k leaves `kept` of them (1 <= kept <= 1499) above the cut.
    Returns (g, k, group indices ascending)."""
    rng = np.random.default_rng(seed)
    n = N_STRAT
    g = gauss(n, rng)
    chunks = [TIE_BIG] + [3 + 9 * j for j in range(13)]           # 3, 12, ..., 111
    assert TIE_BIG not in chunks[1:] and max(chunks) < n // CHUNK
    pos = np.concatenate([c * CHUNK + rng.choice(CHUNK, 200 if c == TIE_BIG else 100, replace=False)
                          for c in chunks])
    assert pos.shape[0] == TIE_COUNT
    rest = np.sort(np.abs(np.delete(g, pos)))[::-1]
    k0 = co.num_kept(0.1, n)
    v = 0.5 * (rest[k0] + rest[k0 + 1])      # between two neighbours: no other element has it
    assert rest[k0] > v > rest[k0 + 1]
    g[pos] = v * rng.choice([-1.0, 1.0], TIE_COUNT)
    k = int(np.count_nonzero(np.abs(g) > v)) + kept
    return g, k, np.sort(pos)


# ---- the clamped key group -------------------------------------------------------------------
CLAMP_EACH = 500
CLAMP_KS = (250, 700, 1200, 1499, 1501)
NAN_INF_HW = 0x7FF0000000000001   # a NaN whose high word equals inf's


def clamped(n: int, seed: int = 23):
    """Gaussian base plus 500 finite giants log-uniform in [2^1017, 2^1023), 500 +-inf and 500
    NaNs of mixed sign and payload (0x7ff0000000000001 and its negative among them): 1500 elements
    with ONE key32.  By key64 the NaNs are on top (one tie group), then the infs (one tie group),
    then the giants.  Returns (g, nan indices, inf indices, giant indices), each ascending."""
    rng = np.random.default_rng(seed)
    g = gauss(n, rng)
    pos = rng.choice(n, 3 * CLAMP_EACH, replace=False)
    i_nan, i_inf, i_big = (np.sort(pos[j * CLAMP_EACH:(j + 1) * CLAMP_EACH]) for j in range(3))
    g[i_big] = 2.0 ** rng.uniform(1017.001, 1023.0, CLAMP_EACH) * rng.choice([-1.0, 1.0], CLAMP_EACH)
    g[i_inf] = np.inf * rng.choice([-1.0, 1.0], CLAMP_EACH)
    payload = rng.integers(1, 1 << 52, CLAMP_EACH, dtype=np.uint64)
    sign = rng.integers(0, 2, CLAMP_EACH, dtype=np.uint64) << np.uint64(63)
    nan = sign | np.uint64(0x7FF0000000000000) | payload
    nan[0] = np.uint64(NAN_INF_HW)
    nan[1] = np.uint64(NAN_INF_HW | (1 << 63))
    nan[2] = np.uint64(0x7FF4000000000000)                   # signalling, positive
    nan[3] = np.uint64(0xFFFFFFFFFFFFFFFF)
    g[i_nan] = from_bits(nan)
    return g, i_nan, i_inf, i_big


def clamped_expected_kept(g, k: int, i_nan, i_inf, i_big) -> np.ndarray:
    """The kept indices the description promises for k of CLAMP_KS (ascending)."""
    E = CLAMP_EACH
    if k <= E:                                   # inside the NaN tie group: its highest indices
        kept = i_nan[E - k:]
    elif k <= 2 * E:                             # every NaN, the highest indices of the infs
        kept = np.concatenate([i_nan, i_inf[2 * E - k:]])
    elif k <= 3 * E:                             # ... and the largest giants (all distinct)
        order = i_big[np.argsort(np.abs(g[i_big]))[::-1]]
        kept = np.concatenate([i_nan, i_inf, order[:k - 2 * E]])
    else:                                        # the whole group and the largest of the rest
        m = np.abs(g).copy()
        m[np.concatenate([i_nan, i_inf, i_big])] = -1.0
        kept = np.concatenate([i_nan, i_inf, i_big, np.argsort(m)[::-1][:k - 3 * E]])
    return np.sort(kept)


# ---- a bracket that misses -------------------------------------------------------------------
def bracket_miss(seed: int = 24):
    """n = 4 * 2^20, k = n / 10, n / 8 Gaussian values only where the lone encode's sample never
    reads: the sample sees zeros, the bracket sits at key 0, more than k elements are above it
    and k_resolve64 reports RETRY."""
    n = N_MISS
    k = n // 10
    hidden = np.nonzero(~sampled_mask(n, k))[0]
    g = np.zeros(n)
    step = hidden.shape[0] // (n // 8)
    g[hidden[::step][:n // 8]] = gauss(n // 8, np.random.default_rng(seed))
    return g, k


# ---- plain sweeps ----------------------------------------------------------------------------
SWEEP_N = (2, 3, 5, 8191, 8192, 8193, 16_385, 1 << 20, (1 << 20) + 1, (1 << 20) + 8191)
SWEEP_F = (0.5, 0.1, 0.01)


def sweep(n: int):
    """Gaussian x 10^U(-4, 1) per element, 1 % -0.0, a few denormals (5e-324 x small ints)."""
    rng = np.random.default_rng(1000 + n)
    g = rng.standard_normal(n) * 10.0 ** rng.uniform(-4, 1, n)
    g[rng.random(n) < 0.01] = -0.0
    m = min(6, n // 3)
    if m:
        g[rng.choice(n, m, replace=False)] = 5e-324 * rng.integers(1, 9, m) * rng.choice([-1.0, 1.0], m)
    return g


def sweep_ks(n: int):
    ks = {co.num_kept(f, n) for f in SWEEP_F}
    if n >= 3:
        ks |= {1, n - 1}
    return sorted(ks)
