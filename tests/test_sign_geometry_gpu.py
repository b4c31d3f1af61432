"""fc_sign_gram / fc_sign_dot (csrc/fc_sign_gram.hip) and their consumers (codec.gram_sign,
codec.dot_sign, gar.Krum, the linear rules, the Aggregator's "sign-gram" routes) on an MI355X.

Run:  python -m pytest tests/test_sign_geometry_gpu.py -m gpu -q

Packets are built on the host from hand-made bits and scales (sign_model.pack) and uploaded through
the validator (codec.sign_from_host).  The Gram matrix is compared BIT FOR BIT with the model
(tests/sign_geometry_model.py): Hamming distances are integers and each entry is one IEEE multiply,
so there is nothing to tolerate.  The dot is bit-exact where every partial sum is exact
(integer-valued v, v=None) and otherwise within the rounding bound of any order of float64
summation (sign_model.sum_bound) plus the roundings of the model's own sum and of the one multiply
by the scale: |got - s D| <= s (bound + 2^-52 |D|).
"""
import types

import numpy as np
import pytest

import sign_geometry_model as gm
import sign_model as sm

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F = np.float32
NS = (1, 31, 32, 33, 127, 128, 129, 8191, 8193)
MS = (1, 2, 3, 63, 64, 65, 127, 128)
BIG = 1_000_003
GRAM_SHAPES = [(m, n) for n in NS for m in MS] + [(3, BIG), (128, BIG)]
DOT_SHAPES = [(m, n) for n in NS for m in MS] + [(3, BIG)]


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from openmsftl_amd import _lib
    assert _lib.load().fc_abi_version() == 4
    yield
    _MEMO.clear()
    torch.cuda.empty_cache()


_MEMO = {}


def memo(key, make):
    if key not in _MEMO:
        if len(_MEMO) > 6:                         # the large cases are used once each
            _MEMO.clear()
        _MEMO[key] = make()
    return _MEMO[key]


def _codec():
    from openmsftl_amd import codec
    return codec


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def host(t):
    return t.cpu().numpy()


def same_bits(got, want, what=""):
    """Bit for bit; NaN positions compare as NaN."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, what
    u = {4: np.uint32, 8: np.uint64}[got.dtype.itemsize]
    gn, wn = np.isnan(got), np.isnan(want)
    bad = np.argwhere((gn != wn) | (~gn & ~wn & (got.view(u) != want.view(u))))
    assert bad.size == 0, (f"{what}: {len(bad)} of {got.size} differ, first at {bad[:4].tolist()}: "
                           f"got {[got[tuple(b)] for b in bad[:4]]} want {[want[tuple(b)] for b in bad[:4]]}")


def make_bits(m, n, seed):
    """Random rows with per-client densities from 0.05 to 0.95; client 1 duplicates client 0,
    client 2 is its complement, client 3 has only bit n - 1 set and client 4 only the first word of
    every 2048-word span (as far as m reaches)."""
    rng = np.random.default_rng(seed)
    dens = np.linspace(0.05, 0.95, m) if m > 1 else np.array([0.5])
    B = np.empty((m, n), bool)
    for i in range(m):
        B[i] = rng.random(n, dtype=F) < dens[i]
    if m > 1:
        B[1] = B[0]
    if m > 2:
        B[2] = ~B[0]
    if m > 3:
        B[3] = False
        B[3, n - 1] = True
    if m > 4:
        B[4] = (np.arange(n) % (2048 * 32)) < 32
    return B


def make_scales(m, seed):
    """Random float32 across 2^-60 .. 2^60: the products need the float64 range."""
    rng = np.random.default_rng(seed)
    return (rng.uniform(1.0, 2.0, m) * 2.0 ** rng.integers(-60, 61, m)).astype(F)


def upload(B, s):
    c = _codec()
    return [c.sign_from_host(raw) for raw in gm.packets(B, s)]


def case(m, n, wide=True):
    def make():
        B = make_bits(m, n, 1000 * m + n % 997)
        s = make_scales(m, 7 * m + n % 991) if wide else \
            np.random.default_rng(m + n).uniform(0.5, 2.0, m).astype(F)
        return B, s, upload(B, s)
    return memo((m, n, wide), make)


def gram_call(pk):
    """codec.gram_sign into a NaN-filled matrix with the workspace filled with 0xFF."""
    c = _codec()
    m, n = len(pk), pk[0].n
    c.SignGramWorkspace.get(n, m, pk[0].words.device).buf.fill_(255)
    out = torch.full((m, m), float("nan"), dtype=torch.float64, device="cuda")
    assert c.gram_sign(pk, out=out) is out
    return host(out)


def dot_call(pk, v=None):
    c = _codec()
    m, n = len(pk), pk[0].n
    c.SignDotWorkspace.get(n, m, pk[0].words.device).buf.fill_(255)
    out = torch.full((m + 1,), float("nan"), dtype=torch.float64, device="cuda")
    assert c.dot_sign(pk, v, out=out) is out
    return host(out)


# ---- the Gram matrix ----------------------------------------------------------------------------
@pytest.mark.parametrize("m,n", GRAM_SHAPES)
def test_gram_equals_the_model_bit_for_bit(m, n):
    B, s, pk = case(m, n)
    want = gm.gram(B, s)
    got = gram_call(pk)
    same_bits(got, want, f"m={m} n={n}")
    assert got.view(np.uint64).tolist() == got.T.copy().view(np.uint64).tolist()      # symmetric bitwise
    assert (np.diagonal(got) == s.astype(np.float64) ** 2 * n).all()
    same_bits(gram_call(pk), got, "second call")
    perm = np.random.default_rng(m + n).permutation(m)
    same_bits(gram_call([pk[i] for i in perm]), got[np.ix_(perm, perm)], "clients permuted")


def test_gram_non_finite_scales_mark_their_rows_and_columns():
    m, n = 6, 8193
    B = make_bits(m, n, 5)
    s = make_scales(m, 6)
    s[1], s[4] = np.nan, np.inf
    got = gram_call(upload(B, s))
    want = gm.gram(B, s)
    bad = np.zeros((m, m), bool)
    bad[[1, 4], :] = True
    bad[:, [1, 4]] = True
    assert (np.isnan(got) == bad).all() and (np.isnan(want) == bad).all()
    same_bits(got, want, "non-finite scales")


def test_gram_and_dot_argument_checks():
    c = _codec()
    B, s, pk = case(3, 129)
    with pytest.raises(ValueError, match="no packets"):
        c.gram_sign([])
    with pytest.raises(TypeError, match="sign packets"):
        c.gram_sign([pk[0], object()])
    with pytest.raises(ValueError, match="at most 128"):
        c.gram_sign([pk[0]] * 129)
    with pytest.raises(ValueError, match="at most 128"):
        c.dot_sign([pk[0]] * 129)
    with pytest.raises(ValueError, match="share n"):
        c.gram_sign([pk[0], case(3, 128)[2][0]])
    with pytest.raises(ValueError, match=r"\(m, m\) float64"):
        c.gram_sign(pk, out=torch.empty((3, 3), dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError, match=r"\(m \+ 1,\) float64"):
        c.dot_sign(pk, out=torch.empty(3, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="v must be"):
        c.dot_sign(pk, torch.empty(128, device="cuda"))
    with pytest.raises(ValueError, match="v must be"):
        c.dot_sign(pk, torch.empty(129, dtype=torch.float64, device="cuda"))


# ---- the dot ------------------------------------------------------------------------------------
@pytest.mark.parametrize("m,n", DOT_SHAPES)
def test_dot_exact_inputs_equal_the_model_bit_for_bit(m, n):
    B, s, pk = case(m, n)
    same_bits(dot_call(pk), gm.dot_out(B, s), f"m={m} n={n} v=None")
    v = np.random.default_rng(n + m).integers(-8, 9, n).astype(F)       # every partial sum is exact
    same_bits(dot_call(pk, dev(v)), gm.dot_out(B, s, v), f"m={m} n={n} integer v")


@pytest.mark.parametrize("m,n", DOT_SHAPES)
def test_dot_normal_vector_within_the_summation_bound(m, n):
    B, s, pk = case(m, n)
    v = np.random.default_rng(3 * n + m).standard_normal(n).astype(F)
    vd = dev(v)
    got = dot_call(pk, vd)
    D, bound = gm.dot(B, s, v)
    s64 = s.astype(np.float64)
    err = np.abs(got[:m] - s64 * D)
    tol = s64 * (bound + 2.0 ** -52 * np.abs(D))
    print(f"m={m} n={n}: max err / tol = {np.max(err / np.maximum(tol, 1e-300)):.3g}")
    assert (err <= tol).all(), (err, tol)
    q = gm.dot_out(B, s, v)[m]
    assert abs(got[m] - q) <= sm.sum_bound(n, q) + 2.0 ** -52 * q
    same_bits(dot_call(pk, vd), got, "second call")


def test_dot_non_finite_vector_and_scales():
    m, n = 6, 8193
    B = make_bits(m, n, 9)
    s = make_scales(m, 10)
    s[1], s[4] = np.nan, np.inf
    pk = upload(B, s)
    v = np.random.default_rng(11).integers(-8, 9, n).astype(F)
    for vec in (None, v):
        got = dot_call(pk, None if vec is None else dev(vec))
        assert np.isnan(got[[1, 4]]).all() and not np.isnan(got[[0, 2, 3, 5, 6]]).any()
        same_bits(got, gm.dot_out(B, s, vec), "non-finite scales")
    for bad in (np.nan, np.inf, -np.inf):
        w = v.copy()
        w[n // 2] = bad
        assert np.isnan(dot_call(pk, dev(w))).all(), bad


# ---- against the existing routes ----------------------------------------------------------------
def honest_round(m, n, seed, outliers=()):
    """Clients that share a base pattern with a tenth of the bits flipped each; the outliers send
    the complement of theirs.  Scales in [0.5, 2)."""
    rng = np.random.default_rng(seed)
    base = rng.random(n) < 0.5
    B = np.stack([base ^ (rng.random(n) < 0.1) for _ in range(m)])
    for i in outliers:
        B[i] = ~B[i]
    return B, rng.uniform(0.5, 2.0, m).astype(F)


def test_gram_against_the_dense_float64_product_of_the_decoded_rows():
    c = _codec()
    m, n = 5, 8193
    B, s = honest_round(m, n, 21)
    pk = upload(B, s)
    G = torch.stack([c.decode_sign(p) for p in pk])
    same_bits(host(G), gm.decoded(B, s), "decode_sign")
    dense = host(G.double() @ G.double().T)
    got = gram_call(pk)
    # the dense sum's own rounding bound (Higham); the new value is the correctly rounded one
    assert np.allclose(got, dense, rtol=n * 2.0 ** -52, atol=0.0)


def test_krum_on_sign_packets_returns_the_selected_clients_row():
    from openmsftl_amd import gar
    m, n = 7, 8193
    B, s = honest_round(m, n, 22, outliers=(2, 5))
    pk = upload(B, s)
    K = gm.gram(B, s)
    sel = gar.Krum.select(K, 0.3)
    assert sel not in (2, 5)
    rule = gar.Krum({})
    got = rule.aggregate_packets(pk)
    assert rule.selected == sel
    same_bits(host(got), sm.decode(B[sel], s[sel]), "krum")
    with pytest.raises(TypeError, match="one kind"):
        rule.aggregate_packets([pk[0], object()])


@pytest.mark.parametrize("scheme", ["spectral_gram", "spectral_gram_adaptive", "geometric_median"])
def test_linear_rules_on_sign_packets_fold_their_own_coefficients(scheme):
    from openmsftl_amd import gar
    m, n = 7, 8193
    B, s = honest_round(m, n, 23, outliers=(1, 4))
    pk = upload(B, s)
    K = gm.gram(B, s)
    w = np.full(m, 1.0 / m, F)
    if scheme == "spectral_gram":
        rule = gar.SpectralGram({"rank": 3, "adaptive_rank_th": 0})
        want, S = gar.spectral_coeffs(K, w, n, rank=3, adaptive_rank_th=0)
    elif scheme == "spectral_gram_adaptive":
        rule = gar.SpectralGram({"adaptive_rank_th": 0.9})
        want, S = gar.spectral_coeffs(K, w, n, adaptive_rank_th=0.9, row_sums=gm.dot_out(B, s)[:m])
    else:
        rule = gar.GeometricMedian({})
        want, _ = gar.geometric_median_coeffs(K, w)
    got = rule.aggregate_packets(pk)
    assert np.array_equal(rule.coeffs, want) and rule.carry == 0.0 and rule.excluded == []
    same_bits(host(got), sm.fold(gm.decoded(B, s), rule.coeffs.astype(F)), scheme)
    if scheme.startswith("spectral"):
        assert np.array_equal(rule.Sigma_tracked[-1], S)


def test_centered_clip_on_sign_packets_carries_its_vector_over_two_rounds():
    from openmsftl_amd import gar
    c = _codec()
    m, n = 7, 8193
    rule = gar.CenteredClip({"cclip_tau": 40.0})
    B, s = honest_round(m, n, 24, outliers=(3,))
    got1 = rule.aggregate_packets(upload(B, s))
    _, want = gar.centered_clip_coeffs(gm.gram(B, s), None, 0.0, 40.0, 3)
    assert np.array_equal(rule.coeffs, want) and rule.carry == 0.0
    v1 = sm.fold(gm.decoded(B, s), rule.coeffs.astype(F))
    same_bits(host(got1), v1, "round 1")
    same_bits(host(rule.v), v1, "carried vector")
    B2, s2 = honest_round(m, n, 25, outliers=(0, 6))
    pk2 = upload(B2, s2)
    r = host(c.dot_sign(pk2, rule.v))
    D, bound = gm.dot(B2, s2, v1)
    assert (np.abs(r[:m] - s2 * D) <= s2 * (bound + 2.0 ** -52 * np.abs(D))).all()
    got2 = rule.aggregate_packets(pk2)
    a, want = gar.centered_clip_coeffs(gm.gram(B2, s2), r[:m], float(r[m]), 40.0, 3)
    assert np.array_equal(rule.coeffs, want) and rule.carry == a and a != 0.0
    with np.errstate(all="ignore"):
        start = (v1 * F(a)).astype(F)
    same_bits(host(got2), sm.fold(gm.decoded(B2, s2), rule.coeffs.astype(F), start=start), "round 2")


# ---- the Aggregator -----------------------------------------------------------------------------
def _clients(grads, **cfg):
    from openmsftl_amd import Compression
    return [types.SimpleNamespace(C=Compression(dict({"compression_function": "sign"}, **cfg)), grad=g,
                                  client_id=i) for i, g in enumerate(grads)]


def _agg(scheme="fed_avg", **cfg):
    from openmsftl_amd.aggregation import Aggregator
    return Aggregator(dict({"aggregation_scheme": scheme}, **cfg))


def exact_grads(m, n, seed, nan_client=None):
    """Integer-valued gradients around a common direction (every partial sum of |g| is exact, so
    the device scale is the model's), one of them optionally holding a NaN."""
    rng = np.random.default_rng(seed)
    base = rng.integers(-4, 5, n)
    grads = [(base + rng.integers(-2, 3, n)).astype(F) for _ in range(m)]
    if nan_client is not None:
        grads[nan_client][17] = np.nan
    return grads


def model_round(grads):
    enc = [sm.encode(g) for g in grads]
    B = np.stack([sm.bits(e[0]) for e in enc])
    s = F([e[1] for e in enc])
    return B, s, np.stack([e[3] for e in enc]), gm.gram(B, s)


@pytest.mark.parametrize("scheme", ["krum", "geometric_median", "fed_avg"])
@pytest.mark.parametrize("nan_client", [4, None])
def test_aggregator_sign_gram_routes(scheme, nan_client):
    from openmsftl_amd import gar
    m, n = 6, 8193
    grads = exact_grads(m, n, 31, nan_client)
    B, s, rows, K = model_round(grads)
    assert np.isnan(s[4]) == (nan_client is not None)
    keep = [i for i in range(m) if i != nan_client]
    w = np.full(m, 1.0 / m, F)
    if scheme == "krum":
        sel = gar.Krum.select(K, 0.3)
        assert sel != nan_client
        want = rows[sel]
    elif scheme == "geometric_median":
        coeffs = np.zeros(m)
        coeffs[keep] = gar.geometric_median_coeffs(K[np.ix_(keep, keep)], w[keep])[0]
        want = sm.fold(rows[keep], coeffs.astype(F)[keep])
    else:
        want = sm.fold(rows, w)
    sigma = gar.gram_singular_values(K)
    assert np.isnan(sigma).all() == (nan_client is not None)
    a = _agg(scheme, sign_geometry=True, pc_analysis="gram")
    a.aggregate_grads(_clients(grads))
    assert a.agg_path == "sign-gram" and a.curr_G is None
    same_bits(a.agg_grad, want, f"{scheme} sign-gram")
    assert np.array_equal(a.gar.Sigma_tracked[-1], sigma, equal_nan=True)
    b = _agg(scheme, sign_geometry=True, pc_analysis="gram")
    b.aggregate_wire([cl.C.compress_wire(cl.grad) for cl in _clients(grads)])
    assert b.agg_path == "wire-sign-gram" and b.curr_G is None
    same_bits(b.agg_grad, a.agg_grad, f"{scheme} wire-sign-gram")
    assert np.array_equal(b.gar.Sigma_tracked[-1], sigma, equal_nan=True)
    if scheme == "geometric_median":
        assert a.gar.excluded == b.gar.excluded == ([] if nan_client is None else [nan_client])
        assert np.array_equal(a.gar.coeffs, coeffs)


def test_aggregator_sign_gram_with_error_feedback_over_three_rounds():
    m, n = 4, 8193
    a, b = _agg("krum", sign_geometry=True), _agg()
    ca, cb = (_clients([None] * m, error_feedback=True) for _ in range(2))
    for r in range(3):
        grads = [np.random.default_rng(600 + 10 * r + i).standard_normal(n).astype(F) for i in range(m)]
        for cl in (ca, cb):
            for c, g in zip(cl, grads):
                c.grad = g
        a.aggregate_grads(ca)
        b.aggregate_grads(cb)
        assert (a.agg_path, b.agg_path) == ("sign-gram", "sign")
        for x, y in zip(ca, cb):                                       # each residual advanced once
            same_bits(np.asarray(x.C.get_residual()), np.asarray(y.C.get_residual()), f"round {r} residual")
    with pytest.raises(NotImplementedError, match="device_budget_bytes"):
        _agg("krum", sign_geometry=True, device_budget_bytes=4096).aggregate_grads(ca)
