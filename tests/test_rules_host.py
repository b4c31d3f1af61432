"""The rules that are linear in the rows of G — the checks that need no GPU: the C ABI surface of
fc_packets_dot and its argument errors (reported before the GPU is touched), the workspace size,
the three pure coefficient functions of gar.py against dense float64 oracles written here, the
reference's quirks of the spectral rule, the golden results of the reference's analytic
SpectralFedAvg branch, and the routing of the three schemes (include/fedcodec.h, gar.py,
aggregation.py).

Tolerances are derived from the inputs and asserted per test (never tuned); every test prints
its measured error / bound ratio.  The unit is the rounding error of one M-term sum of products
c_j K_ij, eta = M * c_max * 2^-53 * max K_ii (c_max the largest |coefficient| met, at least 1):

* a squared distance in coefficient space is a handful of such sums, so |delta d_i^2| <= 8 eta,
  and through the square root the RELATIVE error of d_i is 8 eta / d_i^2 (the factor 1 / d_i^2
  per distance).  K itself is a float64 product here, N-term sums: 4 N 2^-53 max K_ii more in
  d_i^2.  The dense oracle's own distance, an N-term float64 sum, carries N 2^-53 relative.  Each iteration turns the distances' relative errors into coefficient errors
  of at most twice the largest (a ratio of sums of 1 / d_i), and the iterations' errors ADD:
  centered clipping is z - grad F(z) for a convex 1-smooth F (a sum of Huber functions), a
  non-expansive map, and the smoothed Weiszfeld step is a descent step of a convex objective
  that contracts towards its fixed point; neither compounds an error.  So after T iterations
  |delta c| <= T * 2 * max_i ((8 eta + 4 N 2^-53 max K_ii) / d_i^2 + N 2^-53) * c_max.  Preconditions, asserted on the
  oracle: d_i >= 1e-3 sqrt(max K_ii) and |d_i - tau| >= 1e-6 tau at every iteration.
* the spectral projector P = V_k^T V_k moves by at most 2 |delta K| / gap (Davis-Kahan), gap the
  smallest difference of sigma^2 between a kept and a dropped component; |delta K| <= (M c_nz
  2^-53 + M 2^-52) sigma_max^2 (the Gram's summation error over c_nz non-zero products and the
  eigen-solver's, _sigma_check's two terms), once for the function under test and once for the
  oracle's SVD.  Precondition: gap >= 1e-3 sigma_max^2.
"""
import ctypes
import json
import os
import re
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fedcodec.h")
GOLDEN = os.path.join(ROOT, "tests", "golden")
FC_ERR_ARG, FC_ERR_WORKSPACE = -1, -3
U = 2.0 ** -53


@pytest.fixture(scope="module")
def lib():
    from openmsftl_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


# ---- ABI ---------------------------------------------------------------------------------------
def test_header_declares_and_library_exports_the_entry_points(lib):
    from openmsftl_amd import _lib
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                         text=True, check=True).stdout
    exported = set(re.findall(r"\s[TW]\s+(\S+)", out))
    for name in ("fc_dot_workspace_bytes", "fc_packets_dot"):
        assert re.search(r"\b%s\s*\(" % name, src), name
        assert name in exported and name in _lib.SIGNATURES, name
        assert getattr(lib, name).argtypes == _lib.SIGNATURES[name][1], name
    assert lib.fc_abi_version() == 4          # additions only


def test_packets_dot_argument_errors_do_not_touch_gpu(lib):
    n, m, big = 3 * 8192 + 5, 7, 1 << 40
    views = ctypes.create_string_buffer(56 * m + 32)      # host buffers stand in for the device
    vec = ctypes.create_string_buffer(64)                 # arrays: a call that got past the
    out = ctypes.create_string_buffer(8 * (m + 1) + 32)   # checks would fault, not return a code
    ws = ctypes.create_string_buffer(64)
    V, X, O, W = (((ctypes.addressof(b) + 15) & ~15) for b in (views, vec, out, ws))

    def call(v_=V, m_=m, n_=n, x_=X, o_=O, w_=W, ws_bytes=16):
        return lib.fc_packets_dot(v_, m_, n_, x_, o_, w_, ws_bytes, None)

    err = lib.fc_last_error
    assert call(v_=None) == FC_ERR_ARG and b"views_dev is NULL" in err()
    assert call(o_=None) == FC_ERR_ARG and b"out is NULL" in err()
    assert call(w_=None) == FC_ERR_ARG and b"workspace is NULL" in err()
    assert call(m_=0) == FC_ERR_ARG and b"m=0" in err()
    assert call(m_=-1) == FC_ERR_ARG and b"m=-1" in err()
    assert call(m_=129) == FC_ERR_ARG and b"m=129" in err()
    assert call(n_=0) == FC_ERR_ARG and b"n=0" in err()
    assert call(n_=1 << 32) == FC_ERR_ARG and b"outside [1, 2^32-1]" in err()
    assert call(x_=X + 4) == FC_ERR_ARG and b"v must be 16-byte aligned" in err()
    assert call(o_=O + 8) == FC_ERR_ARG and b"out must be 16-byte aligned" in err()
    assert call(w_=W + 8, ws_bytes=big) == FC_ERR_ARG and b"workspace must be 16-byte aligned" in err()
    # a short workspace, with a vector and with the all-ones NULL
    assert call(ws_bytes=16) == FC_ERR_WORKSPACE and b"workspace" in err()
    assert call(x_=None, ws_bytes=16) == FC_ERR_WORKSPACE and b"workspace" in err()
    need = lib.fc_dot_workspace_bytes(n, m)
    assert need > 0
    assert call(ws_bytes=need - 1) == FC_ERR_WORKSPACE and b"workspace" in err()


def test_dot_workspace_bytes_is_monotone_in_n_and_m(lib):
    ns = [1, 3, 2048, 8192, 8193, 6 * 8192 + 2048 + 3, 1 << 20, (1 << 24) + 1, 1 << 27, (1 << 32) - 1]
    table = [[lib.fc_dot_workspace_bytes(n, m) for m in range(1, 129)] for n in ns]
    for row in table:
        assert all(b > 0 for b in row)
        assert all(a <= b for a, b in zip(row, row[1:])), "not monotone in m"
    for lo, hi in zip(table, table[1:]):
        assert all(a <= b for a, b in zip(lo, hi)), "not monotone in n"
    assert lib.fc_dot_workspace_bytes(0, 4) == 0
    assert lib.fc_dot_workspace_bytes(1 << 32, 4) == 0
    assert lib.fc_dot_workspace_bytes(4096, 0) == 0
    assert lib.fc_dot_workspace_bytes(4096, 129) == 0
    assert lib.fc_dot_workspace_bytes(1 << 27, 128) <= 4 << 20      # far below a gradient (4 n)


# ---- the rows of the rule tests ----------------------------------------------------------------
M_R, N_ROWS = 9, 5000


def rule_rows():
    """M = 9 rows of N = 5000: a seeded normal matrix, every |value| < 1.2 zeroed (about 23 % of
    the entries stay), row 3 scaled x8 and row 7 = -4 x row 1.  float64, with K = R R^T."""
    rng = np.random.default_rng(20261020)
    R = rng.standard_normal((M_R, N_ROWS))
    R[np.abs(R) < 1.2] = 0.0
    R[3] *= 8.0
    R[7] = -4.0 * R[1]
    frac = np.count_nonzero(R) / R.size
    assert 0.2 < frac < 0.26
    return R, R @ R.T


def _eta(K, c_max):
    return K.shape[0] * max(1.0, c_max) * U * float(np.max(np.diagonal(K)))


def _iter_bound(K, T, c_max, d_min):
    own = 4.0 * N_ROWS * U * float(np.max(np.diagonal(K)))     # K itself: N-term float64 sums
    return T * 2.0 * ((8.0 * _eta(K, c_max) + own) / d_min ** 2 + N_ROWS * U) * max(1.0, c_max)


# ---- geometric median --------------------------------------------------------------------------
def dense_weiszfeld(R, alpha, T, nu):
    """T smoothed Weiszfeld updates on the dense rows; (coefficients, every distance met)."""
    z = alpha @ R
    nu_abs = nu * np.sqrt(np.max(np.sum(R * R, axis=1)))
    c, seen = alpha.copy(), []
    for _ in range(T):
        dist = np.sqrt(np.sum((R - z[None, :]) ** 2, axis=1))
        seen.append(dist)
        beta = alpha / np.maximum(nu_abs, dist)
        c = beta / np.sum(beta)
        z = c @ R
    return c, np.array(seen)


@pytest.mark.parametrize("weights", ["uniform", "skewed"])
def test_geometric_median_against_the_dense_iteration(weights):
    from openmsftl_amd.gar import geometric_median_coeffs
    R, K = rule_rows()
    alpha = np.full(M_R, 1.0 / M_R, np.float32).astype(np.float64)
    if weights == "skewed":
        alpha = (np.arange(1, M_R + 1) / 45.0).astype(np.float32).astype(np.float64)
    T = 40
    want, seen = dense_weiszfeld(R, alpha, T, 1e-6)
    got, iters = geometric_median_coeffs(K, alpha, iters=T, tol=-1.0, nu=1e-6)   # no early stop
    assert iters == T and got.dtype == np.float64 and got.shape == (M_R,)
    top = np.sqrt(np.max(np.diagonal(K)))
    assert seen.min() >= 1e-3 * top                                   # precondition, on the oracle
    bound = _iter_bound(K, T, float(np.max(np.abs(want))), float(seen.min()))
    err = float(np.max(np.abs(got - want)))
    print(f"geometric median ({weights}): coefficients {got}, max |err| {err:.3e}, err/bound {err / bound:.3e}")
    assert err <= bound
    assert abs(np.sum(got) - 1.0) <= 4 * M_R * U and np.all(got > 0)
    rel = got / alpha
    assert rel[3] < rel[0] and rel[7] < rel[0]                        # the outliers count less


def test_geometric_median_stops_on_the_objective_and_handles_zero_rows():
    from openmsftl_amd.gar import geometric_median_coeffs
    R, K = rule_rows()
    alpha = np.full(M_R, 1.0 / M_R, np.float32).astype(np.float64)
    c, iters = geometric_median_coeffs(K, alpha)                      # gm_iters 100, gm_tol 1e-12
    assert 1 < iters < 100
    obj = lambda x: float(alpha @ np.sqrt(np.sum((R - (x @ R)[None, :]) ** 2, axis=1)))  # noqa: E731
    assert obj(c) < obj(alpha)
    c1, one = geometric_median_coeffs(K, alpha, iters=1)
    assert one == 1 and obj(c) < obj(c1) < obj(alpha)
    z, zero = geometric_median_coeffs(np.zeros((4, 4)), np.full(4, 0.25))
    assert zero == 0 and np.array_equal(z, np.full(4, 0.25))
    # a client that IS the iterate: the smoothing floor nu_abs keeps the weight finite
    same = np.ones((3, 3))
    c3, _ = geometric_median_coeffs(same, np.full(3, 1 / 3))
    assert np.all(np.isfinite(c3)) and abs(np.sum(c3) - 1.0) < 1e-15


# ---- centered clipping -------------------------------------------------------------------------
def dense_centered_clip(R, v, tau, T):
    """T clipping steps on the dense rows from v (None: zero); (a, c, every distance met)."""
    M = R.shape[0]
    z = np.zeros(R.shape[1]) if v is None else v.astype(np.float64).copy()
    a, c, seen = 1.0, np.zeros(M), []
    for _ in range(T):
        dist = np.sqrt(np.sum((R - z[None, :]) ** 2, axis=1))
        seen.append(dist)
        s = np.where(dist > tau, tau / dist, 1.0)
        z = z + (s[:, None] * (R - z[None, :])).sum(axis=0) / M
        S = s.sum()
        a, c = a * (1.0 - S / M), c * (1.0 - S / M) + s / M
    return a, c, z, np.array(seen)


@pytest.mark.parametrize("carried", [False, True])
@pytest.mark.parametrize("tau", [100.0, 30.0])
def test_centered_clip_against_the_dense_iteration(carried, tau):
    from openmsftl_amd.gar import centered_clip_coeffs
    R, K = rule_rows()
    v = None
    if carried:
        v = (0.5 * R[0] + np.random.default_rng(7).standard_normal(N_ROWS)).astype(np.float32)
    T = 3
    a_w, c_w, z_w, seen = dense_centered_clip(R, v, tau, T)
    if carried:
        v64 = v.astype(np.float64)
        a_g, c_g = centered_clip_coeffs(K, R @ v64, float(v64 @ v64), tau, T)
        Kx = max(float(np.max(np.diagonal(K))), float(v64 @ v64))
    else:
        a_g, c_g = centered_clip_coeffs(K, None, 0.0, tau, T)
        Kx = float(np.max(np.diagonal(K)))
    top = np.sqrt(np.max(np.diagonal(K)))
    assert seen.min() >= 1e-3 * top                                   # preconditions, on the oracle
    assert np.min(np.abs(seen - tau)) >= 1e-6 * tau
    assert np.any(seen > tau) and (tau < 50 or np.any(seen < tau))    # both branches at tau = 100
    c_max = max(1.0, float(np.max(np.abs(c_w))), abs(a_w))
    bound = T * 2.0 * ((8.0 * (M_R + 1) * c_max + 4.0 * N_ROWS) * U * Kx / seen.min() ** 2 + N_ROWS * U) * c_max
    err = max(float(np.max(np.abs(c_g - c_w))), abs(a_g - a_w))
    print(f"centered clip (tau {tau}, carried {carried}): a {a_g:.6f}, c {c_g}, max |err| {err:.3e}, "
          f"err/bound {err / bound:.3e}")
    assert err <= bound
    # the coefficient form reproduces the dense iterate
    z_g = c_g @ R + (a_g * v.astype(np.float64) if carried else 0.0)
    # ... up to the coefficients' error and the float64 rounding of the two evaluations: every
    # iterate is a convex combination of the rows and v, so it stays within B = max(|R|, |v|); a dense
    # step rounds R_i - z, the product with s_i, an M-term sum, the division and the update (at most
    # 4 (M + 2) 2^-53 B per coordinate), and the coefficient form is one (M + 1)-term dot product
    # whose coefficients are non-negative and sum to 1 ((M + 2) 2^-53 B).
    B = max(float(np.max(np.abs(R))), float(np.max(np.abs(v))) if carried else 0.0)
    rounding = (4 * T + 1) * (M_R + 2) * U * B
    assert np.max(np.abs(z_g - z_w)) <= (M_R + 1) * bound * np.max(np.abs(R)) + rounding
    if not carried:
        assert centered_clip_coeffs(K, np.zeros(M_R), 0.0, tau, T)[1].tobytes() == c_g.tobytes()


# ---- the spectral rule -------------------------------------------------------------------------
def rng_state():
    """The whole state of np.random: the key words, the position among them (all that a draw of
    fewer than 624 words moves) and the cached Gaussian."""
    name, key, pos, has_gauss, cached = np.random.get_state()
    return name, key.tobytes(), int(pos), int(has_gauss), float(cached)


def dense_spectral(R, w, rank, th, drop):
    """The reference's algorithm (spectral_aggregation.py:87-130, gar.py:123-134) on an exact
    float64 SVD of the rows: (aggregate, coefficients, S, kept component indices)."""
    X = R.T
    M = R.shape[0]
    if not rank or rank > min(X.shape):
        rank = min(X.shape)
    Uu, S, V = np.linalg.svd(X, full_matrices=False)
    S, V = S[:rank], V[:rank]
    lo, hi = 0, rank
    if th:
        ratio = (S ** 2) / (X.shape[0] - 1) / np.var(X, ddof=1, axis=0).sum()
        ar = int(np.searchsorted(np.cumsum(ratio), th))
        if ar == 0:
            ar += 2 if drop else 1
        hi = min(ar, rank)
    if drop:
        lo = 1
    Vk = V[lo:hi]
    c = Vk.T @ (Vk @ w)
    return c @ R, c, S, (lo, hi), M


def _spectral_bound(R, K, kept, w):
    """2 |delta K| / gap * |w|_2, twice (the function's eigenvectors and the oracle's)."""
    M = K.shape[0]
    lam = np.sort(np.linalg.eigvalsh(K))[::-1]
    lo, hi = kept
    inside = lam[lo:hi]
    outside = np.concatenate([lam[:lo], lam[hi:]])
    floor = 8 * M * U * np.linalg.norm(w)
    if inside.size == 0 or outside.size == 0:
        return floor, np.inf
    gap = float(np.min(np.abs(inside[:, None] - outside[None, :])))
    cnz = max(int(np.count_nonzero((R[i] != 0) & (R[j] != 0))) for i in range(M) for j in range(i, M))
    dK = (M * cnz * U + M * 2.0 ** -52) * lam[0]
    return 2 * 2 * dK / gap * np.linalg.norm(w) + floor, gap / lam[0]


# The rows' spectrum: one large component (the x8 row), a second (row 1 and -4 x row 1), six close
# ones (the independent rows) and a zero (the dependent row): the cases put the cut between kept
# and dropped components where the gap is wide — after 1, after 2, after 8, or nowhere.
SPECTRAL_CASES = [(9, 0.9, False), (2, 0, False), (8, 0, False), (9, 0.6, True), (2, 0, True),
                  (9, 0, False), (None, 0.9, True)]


@pytest.mark.parametrize("rank,th,drop", SPECTRAL_CASES)
def test_spectral_against_the_dense_svd(rank, th, drop):
    from openmsftl_amd.gar import spectral_coeffs
    R, K = rule_rows()
    w = np.full(M_R, 1.0 / M_R, np.float32).astype(np.float64)
    agg_w, c_w, S_w, kept, _ = dense_spectral(R, w, rank, th, drop)
    state = rng_state()
    c_g, S_g = spectral_coeffs(K, w, N_ROWS, rank=rank, adaptive_rank_th=th, drop_top_comp=drop,
                               row_sums=R.sum(axis=1))
    assert rng_state() == state                                       # draws nothing
    bound, rel_gap = _spectral_bound(R, K, kept, w)
    assert rel_gap >= 1e-3                                            # precondition, on the oracle
    err = float(np.max(np.abs(c_g - c_w)))
    print(f"spectral {rank, th, drop}: kept {kept}, relative gap {rel_gap:.3e}, max |err| {err:.3e}, "
          f"err/bound {err / bound:.3e}")
    assert c_g.dtype == np.float64 and c_g.shape == (M_R,) and err <= bound
    assert S_g.shape == S_w.shape
    # singular values: _sigma_check's bound (tests/test_gram_gpu.py), zero ones by the square root
    cnz = N_ROWS
    sb = (M_R * cnz * U + M_R * 2.0 ** -52) * S_w[0] ** 2 / np.maximum(S_w, 1e-300)
    sb = np.minimum(sb, np.sqrt((M_R * cnz * U + M_R * 2.0 ** -52)) * S_w[0])
    assert np.all(np.abs(S_g - S_w) <= sb)
    # the aggregate: the coefficients' error, and the rounding of two M-term float64 dot products
    rounding = (M_R + 1) * U * (np.sum(np.abs(c_g)) + np.sum(np.abs(c_w))) * np.max(np.abs(R))
    assert np.max(np.abs(c_g @ R - agg_w)) <= M_R * bound * np.max(np.abs(R)) + rounding


def _sc(K, **kw):
    from openmsftl_amd.gar import spectral_coeffs
    w = np.full(K.shape[0], 1.0 / K.shape[0], np.float32).astype(np.float64)
    return spectral_coeffs(K, w, N_ROWS, **kw), w


def test_spectral_quirk_rank_falsy_and_rank_above_m_keep_everything():
    R, K = rule_rows()
    for rank in (None, 0, False, M_R + 1, 10 ** 6):
        (c, S), w = _sc(K, rank=rank, adaptive_rank_th=0)
        assert S.shape == (M_R,)                                      # min(M, N) components
        assert np.max(np.abs(c - w)) <= 64 * M_R * U                  # the projector is the identity


def test_spectral_quirk_threshold_falsy_means_no_truncation():
    R, K = rule_rows()
    for th in (0, 0.0, None, False):
        (c, S), _ = _sc(K, rank=4, adaptive_rank_th=th)               # no row sums needed
        (c4, S4), _ = _sc(K, rank=4, adaptive_rank_th=0.999999, row_sums=R.sum(axis=1))
        assert S.shape == (4,) and c.tobytes() == c4.tobytes()        # all four stay either way
    with pytest.raises(ValueError, match="row sums"):
        _sc(K, rank=4, adaptive_rank_th=0.5)


def test_spectral_quirk_adaptive_rank_zero_with_and_without_drop():
    """A threshold below the first component's share gives searchsorted == 0: one component is
    kept, and with drop_top_comp two are kept and the first dropped (the SECOND one stays)."""
    R, K = rule_rows()
    s = R.sum(axis=1)
    lam, Q = np.linalg.eigh(K)
    v0, v1 = Q[:, -1], Q[:, -2]
    w = np.full(M_R, 1.0 / M_R, np.float32).astype(np.float64)
    (c, _), _ = _sc(K, rank=M_R, adaptive_rank_th=1e-6, row_sums=s)
    assert np.max(np.abs(c - v0 * (v0 @ w))) <= 64 * M_R * U
    (c, _), _ = _sc(K, rank=M_R, adaptive_rank_th=1e-6, drop_top_comp=True, row_sums=s)
    assert np.max(np.abs(c - v1 * (v1 @ w))) <= 64 * M_R * U


def test_spectral_quirk_drop_top_comp_can_leave_nothing():
    """searchsorted == 1 keeps [0:1]; dropping the top component leaves no component: all 0."""
    R, K = rule_rows()
    s = R.sum(axis=1)
    (c1, S), _ = _sc(K, rank=M_R, adaptive_rank_th=0.8, row_sums=s)
    total = np.sum((np.diagonal(K) - s * s / N_ROWS) / (N_ROWS - 1))
    cum = np.cumsum(S ** 2 / (N_ROWS - 1) / total)
    assert cum[0] < 0.8 <= cum[1]                                     # the case is the one meant
    (c, S2), _ = _sc(K, rank=M_R, adaptive_rank_th=0.8, drop_top_comp=True, row_sums=s)
    assert np.array_equal(c, np.zeros(M_R)) and S2.tobytes() == S.tobytes()
    (c, _), _ = _sc(K, rank=1, adaptive_rank_th=0, drop_top_comp=True)
    assert np.array_equal(c, np.zeros(M_R))


def test_spectral_quirk_the_default_threshold_raises_at_construction():
    from openmsftl_amd.gar import SpectralGram, spectral_coeffs
    for th in (-1, 1, 1.5, -0.25, True):
        with pytest.raises(ValueError, match="adaptive_rank_th should be between 0 and 1"):
            SpectralGram({"adaptive_rank_th": th})
    with pytest.raises(ValueError, match="adaptive_rank_th should be between 0 and 1"):
        SpectralGram({})                                              # the reference's default, -1
    with pytest.raises(ValueError, match="adaptive_rank_th should be between 0 and 1"):
        spectral_coeffs(np.eye(3), np.ones(3) / 3, 10, adaptive_rank_th=-1)
    g = SpectralGram({"adaptive_rank_th": 0.95, "rank": 3, "drop_top_comp": True})
    assert (g.rank, g.adaptive_rank_th, g.drop_top_comp) == (3, 0.95, True)
    g = SpectralGram({"adaptive_rank_th": 0})
    assert g.rank is None and g.drop_top_comp is False and g.coeffs is None and g.excluded == []


# ---- the golden results of the reference -------------------------------------------------------
def golden():
    sys.path.insert(0, GOLDEN)
    try:
        from npz_parts import load_parts
    finally:
        sys.path.remove(GOLDEN)
    with open(os.path.join(GOLDEN, "manifest_spectral.json")) as fh:
        return load_parts(GOLDEN, "golden_spectral"), json.load(fh)


def round_rows(seed=20261020, n=3 * 8192 + 5, frac=0.25):
    """The oracle's 'top' rows of tests/test_gram_gpu.py's round_clients()."""
    from oracle import compression_oracle as co
    rng = np.random.default_rng(seed)
    base = rng.standard_normal(n)
    rows = []
    for i in range(7):
        noise = rng.standard_normal(n)
        g = 5.0 * noise if i == 2 else -3.0 * base if i == 6 else base + 0.3 * noise
        rows.append(co.compress({"compression_function": "top", "fraction_coordinate": frac},
                                g.astype(np.float32)))
    return np.stack(rows)


def fold32(c32, rows, start=None):
    """The row-order float32 fold: acc = fl32(acc + fl32(c32_i * row_i)) from +0 (or start)."""
    acc = np.zeros(rows.shape[1], np.float32) if start is None else start.astype(np.float32).copy()
    for ci, r in zip(c32, rows):
        acc = np.add(acc, np.multiply(r, np.float32(ci)))
    return acc


def golden_check(name, case, arrays, rows, agg, coeffs, S):
    """The two assertions of the golden test on an aggregate made with ``coeffs``: against the
    exact dense-SVD aggregate within the float32 fold bound plus the coefficient bound, and
    against the reference's within 2 e_ref max|agg_exact| on top (the reference's own distance
    to the exact result is the yardstick: it is float32 and randomized)."""
    M = rows.shape[0]
    R = rows.astype(np.float64)
    K = R @ R.T
    w = np.full(M, 1.0 / M, np.float32).astype(np.float64)
    _, _, S_w, kept, _ = dense_spectral(R, w, case["rank"], case["adaptive_rank_th"], case["drop_top_comp"])
    cb, rel_gap = _spectral_bound(R, K, kept, w)
    assert rel_gap >= 1e-3
    exact, ref, S_ref = arrays[f"{name}|agg_exact"], arrays[f"{name}|agg_ref"], arrays[f"{name}|S_ref"]
    e_ref, top = case["e_ref"], float(np.max(np.abs(exact)))
    fold = (M + 1) * 2.0 ** -24 * np.sum(np.abs(coeffs[:, None] * R), axis=0)
    # the stored exact aggregate is itself a float64 reconstruction (U_k S_k) V_k averaged over
    # the rows: M sums of at most M terms of the rows' magnitude, non-zero (1e-15) even where
    # every row is 0
    own = 8 * M * M * U * float(np.max(np.abs(R)))
    per = fold + cb * np.sum(np.abs(R), axis=0) + own
    err_x = np.abs(agg.astype(np.float64) - exact)
    err_r = np.abs(agg.astype(np.float64) - ref.astype(np.float64))
    slack = per + 2 * e_ref * top
    print(f"golden {name}: e_ref {e_ref:.3e}, vs exact max err/bound "
          f"{np.max(err_x / np.maximum(per, 1e-300)) if top else 0.0:.3e}, vs reference "
          f"{np.max(err_r / np.maximum(slack, 1e-300)) if top else 0.0:.3e}")
    assert agg.dtype == np.float32
    assert np.all(err_x <= per), f"{name}: against the exact aggregate"
    assert np.all(err_r <= slack), f"{name}: against the reference's aggregate"
    if e_ref > 0:
        assert np.all(np.abs(S - S_ref) <= 2 * e_ref * S_ref), f"{name}: S"
    return S_ref


def test_spectral_golden_of_the_reference():
    """Ours = spectral_coeffs on the float64 Gram of the regenerated rows, folded in float32 in
    row order.  S against the reference's within 2 e_ref relative.  In the setting whose
    aggregate is identically 0 (drop_top_comp leaves nothing) e_ref is 0 / 0 and carries no
    information: there S is tied bit for bit to the first setting's (the same rank, the same
    seed), which is checked against the reference within that setting's 2 e_ref."""
    from openmsftl_amd.gar import spectral_coeffs
    arrays, man = golden()
    assert (man["seed"], man["n"], man["fraction"], man["clients"]) == (20261020, 3 * 8192 + 5, 0.25, 7)
    rows = round_rows()
    R = rows.astype(np.float64)
    K, s = R @ R.T, R.sum(axis=1)
    w = np.full(7, 1.0 / 7, np.float32).astype(np.float64)
    want = [(7, 0.95, False), (3, 0, False), (7, 0.95, True), (4, 0.5, True), (7, 0, True)]
    assert sorted((c["rank"], c["adaptive_rank_th"], c["drop_top_comp"]) for c in man["cases"].values()) \
        == sorted(want)
    seen = {}
    for name, case in man["cases"].items():
        c, S = spectral_coeffs(K, w, rows.shape[1], rank=case["rank"],
                               adaptive_rank_th=case["adaptive_rank_th"],
                               drop_top_comp=case["drop_top_comp"], row_sums=s)
        agg = fold32(c.astype(np.float32), rows)
        S_ref = golden_check(name, case, arrays, rows, agg, c, S)
        seen[name] = (S, S_ref, case["e_ref"], float(np.max(np.abs(arrays[f"{name}|agg_exact"]))))
    zero = [k for k, v in seen.items() if v[3] == 0.0]
    assert zero == ["rank7__th0.95__drop1"]
    first = seen["rank7__th0.95__drop0"]
    assert first[2] > 0
    assert seen[zero[0]][0].tobytes() == first[0].tobytes()
    assert seen[zero[0]][1].tobytes() == first[1].tobytes()


# ---- routing and the excluded clients -----------------------------------------------------------
TOP = {"compression_function": "top", "fraction_coordinate": 0.1}
SCHEMES = [{"aggregation_scheme": "spectral_gram", "adaptive_rank_th": 0.95},
           {"aggregation_scheme": "geometric_median"},
           {"aggregation_scheme": "centered_clip", "cclip_tau": 10.0}]


def _client(cfg, n=1000, dtype=np.float32):
    from openmsftl_amd import Compression
    return types.SimpleNamespace(C=Compression(dict(cfg)), grad=np.zeros(n, dtype), client_id=0)


def _agg(**cfg):
    from openmsftl_amd.aggregation import Aggregator
    return Aggregator(dict({"aggregation_scheme": "fed_avg"}, **cfg))


def test_the_three_schemes_select_the_route():
    from openmsftl_amd import aggregation as ag
    from openmsftl_amd.gar import CenteredClip, GeometricMedian, LinearRule, SpectralGram
    kinds = (SpectralGram, GeometricMedian, CenteredClip)
    clients = [_client(TOP) for _ in range(3)]
    for scheme, kind in zip(SCHEMES, kinds):
        a = _agg(**scheme)
        assert type(a.gar) is kind and isinstance(a.gar, LinearRule)
        assert ag.gram_wanted(a) and ag.gram_route_k(a, clients) == 100
        with pytest.raises(NotImplementedError, match="aggregate_packets"):
            a.gar.aggregate(np.zeros((3, 8), np.float32))
    gm = _agg(aggregation_scheme="geometric_median", gm_iters=7, gm_tol=1e-9, gm_nu=1e-3).gar
    assert (gm.gm_iters, gm.gm_tol, gm.gm_nu) == (7, 1e-9, 1e-3)
    d = _agg(aggregation_scheme="geometric_median").gar
    assert (d.gm_iters, d.gm_tol, d.gm_nu) == (100, 1e-12, 1e-6)
    cc = _agg(aggregation_scheme="centered_clip", cclip_tau=2).gar
    assert cc.cclip_tau == 2.0 and cc.cclip_iters == 3 and cc.v is None and cc.carry == 0.0
    for bad in ({}, {"cclip_tau": 0}, {"cclip_tau": -1.0}, {"cclip_tau": None}, {"cclip_tau": float("nan")}):
        with pytest.raises(ValueError, match="cclip_tau"):
            _agg(aggregation_scheme="centered_clip", **bad)
    with pytest.raises(NotImplementedError, match="SpectralFedAvg"):
        _agg(aggregation_scheme="fed_spectral_avg")
    with pytest.raises(NotImplementedError, match="pc_analysis"):
        _agg(pc_analysis=True).aggregate_grads(clients)
    assert ag.gram_resident_bytes(1000, 2) > 1000


def test_each_failing_condition_raises_for_the_three_schemes_without_a_gpu():
    """tests/test_gram_host.py's table, for the new schemes: the same conditions, the same words."""
    top = _client(TOP)
    rounds = {
        "'top'": [top, _client({"compression_function": "full"})],
        "'top' ": [top, _client({"compression_function": "rand", "fraction_coordinate": 0.1})],
        "without error feedback": [top, _client(dict(TOP, error_feedback=True))],
        "one common fraction": [top, _client(dict(TOP, fraction_coordinate=0.2))],
        "float32 gradients": [top, _client(TOP, dtype=np.float64)],
        "one length": [top, _client(TOP, n=1001)],
        "0 < k < n": [_client(dict(TOP, fraction_coordinate=0.0)) for _ in range(2)],
        "0 < k < n ": [_client(dict(TOP, fraction_coordinate=1.0)) for _ in range(2)],
        "at most 128 clients": [top] * 129,
    }
    for scheme in SCHEMES:
        for why, clients in rounds.items():
            agg = _agg(**scheme)
            with pytest.raises(NotImplementedError, match=why.strip()):
                agg.aggregate_grads(clients)
            assert agg.agg_path is None and agg.agg_grad is None, why
        with pytest.raises(NotImplementedError, match="hierarchies"):
            _agg(num_hierarchies=1, cluster_size_list=[2], **scheme).aggregate_grads([top, top])
        with pytest.raises(NotImplementedError, match="one device"):
            _agg(devices=2, **scheme).aggregate_grads([top, top])
        f64w = _agg(**scheme)
        f64w.gar.gradient_weights = np.array([0.5, 0.5], np.float64)
        with pytest.raises(NotImplementedError, match="float32 GAR weights"):
            f64w.aggregate_grads([top, top])
        small = _agg(device_budget_bytes=1000, **scheme)
        with pytest.raises(NotImplementedError, match="device_budget_bytes"):
            small.aggregate_grads([top, top])
    # the words the existing routes' message carries stay
    from openmsftl_amd import aggregation as ag
    stranger = _agg()
    stranger.gar = object()
    with pytest.raises(NotImplementedError, match="the device FedAvg or Krum"):
        ag.gram_route_k(stranger, [top, top])


class _FakePackets:
    """Stands in for codec while LinearRule.aggregate_packets runs on the host: records what is
    given to the fold and to dot_dense."""

    def __init__(self, K, b=None):
        import torch
        self.torch, self.K, self.b, self.folds, self.dots = torch, K, b, [], 0

    def gram(self, packets):
        return self.torch.from_numpy(self.K)

    def dot_dense(self, packets, v=None):
        self.dots += 1
        return self.torch.from_numpy(self.b)

    def decode_accumulate(self, packets, weights, out=None, continue_sum=False):
        self.folds.append(([p.tag for p in packets], list(weights), continue_sum))
        return self.torch.zeros(4)


@pytest.mark.parametrize("scheme", [0, 1, 2])
def test_a_client_with_a_nan_gram_row_is_excluded(scheme, monkeypatch):
    from openmsftl_amd import gar
    R, K = rule_rows()
    Kn = K.copy()
    Kn[4, :] = np.nan
    Kn[:, 4] = np.nan
    keep = [i for i in range(M_R) if i != 4]
    sums = np.append(R.sum(axis=1), float(N_ROWS))
    sums[4] = np.nan
    fake = _FakePackets(Kn, sums)
    monkeypatch.setattr(gar, "codec", fake)
    cfg = dict(SCHEMES[scheme])
    rule = {0: gar.SpectralGram, 1: gar.GeometricMedian, 2: gar.CenteredClip}[scheme](cfg)
    packets = [types.SimpleNamespace(tag=i, n=N_ROWS) for i in range(M_R)]
    rule.aggregate_packets(packets)
    assert rule.excluded == [4] and rule.coeffs[4] == 0.0 and rule.coeffs.dtype == np.float64
    assert np.all(np.isfinite(rule.coeffs)) and rule.carry == 0.0
    tags, weights, cont = fake.folds[0]
    assert tags == keep and not cont                                  # the packet is not folded
    assert weights == [float(x) for x in rule.coeffs.astype(np.float32)[keep]]
    # the rule ran on the sub-block, weights restricted (1/9 each), not renormalised
    Ks = K[np.ix_(keep, keep)]
    w = np.full(M_R, 1.0 / M_R, np.float32)[keep]
    if scheme == 0:
        want, _ = gar.spectral_coeffs(Ks, w, N_ROWS, adaptive_rank_th=0.95, row_sums=sums[:M_R][keep])
        assert fake.dots == 1 and len(rule.Sigma_tracked) == 1 and rule.Sigma_tracked[0].shape == (8,)
    elif scheme == 1:
        want, it = gar.geometric_median_coeffs(Ks, w)
        assert fake.dots == 0 and rule.iterations == it
    else:
        _, want = gar.centered_clip_coeffs(Ks, None, 0.0, 10.0, 3)
        assert fake.dots == 0                                         # the zero start: no dot call
    assert rule.coeffs[keep].tobytes() == want.tobytes()


def test_all_clients_excluded_and_a_non_finite_dot_raise(monkeypatch):
    from openmsftl_amd import gar
    R, K = rule_rows()
    packets = [types.SimpleNamespace(tag=i, n=N_ROWS) for i in range(M_R)]
    monkeypatch.setattr(gar, "codec", _FakePackets(np.full((M_R, M_R), np.nan)))
    for scheme, kind in zip(SCHEMES, (gar.SpectralGram, gar.GeometricMedian, gar.CenteredClip)):
        with pytest.raises(ValueError, match="every client"):
            kind(dict(scheme)).aggregate_packets(packets)
    # a NaN among the finite clients' row sums / dot products, or in |v|^2
    for bad_at in (2, M_R):
        sums = np.append(R.sum(axis=1), float(N_ROWS))
        sums[bad_at] = np.nan
        monkeypatch.setattr(gar, "codec", _FakePackets(K, sums))
        with pytest.raises(ValueError, match="non-finite"):
            gar.SpectralGram({"adaptive_rank_th": 0.5}).aggregate_packets(packets)
