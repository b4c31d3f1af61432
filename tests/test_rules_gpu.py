"""The three rules that are linear in the rows of G (gar.SpectralGram, GeometricMedian,
CenteredClip) through the Aggregator's "gram" route on an MI355X.

Run:  python -m pytest tests/test_rules_gpu.py -m gpu -q

The round is tests/test_gram_gpu.py's round_clients() (copied): M = 7 clients on N = 3 * 8192 + 5,
'top' at f = 0.25; five clients base + 0.3 noise, client 2 = 5 noise, the last one -3 base.
Bit-level contract: gar.coeffs is the pure coefficient function applied to codec.gram and
codec.dot_dense of the same packets, and agg_grad is the NumPy float32 row-order fold of the
oracle's 'top' rows with coeffs.astype(float32), from +0 or from fl32(a32 * v).
Against the dense float64 oracles (written here) the bound is the float32 fold's,
(M + 1) 2^-24 sum_i |c_i d_i| per coordinate (one more term for a carried vector), plus the
coefficient bound of tests/test_rules_host.py times sum_i |d_i|, with the Gram kernel's own
error c_nz 2^-53 max K_ii per entry in place of the host product's.
"""
import json
import os
import sys
import types

import numpy as np
import pytest

from oracle import compression_oracle as co

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
CH = 8192
N_R = 3 * CH + 5
FRAC = 0.25
TOP_CFG = {"compression_function": "top", "fraction_coordinate": FRAC}
U = 2.0 ** -53
TAU = 100.0
SCHEMES = {
    "spectral_gram": {"aggregation_scheme": "spectral_gram", "adaptive_rank_th": 0.95, "rank": 7},
    "geometric_median": {"aggregation_scheme": "geometric_median"},
    "centered_clip": {"aggregation_scheme": "centered_clip", "cclip_tau": TAU},
}
_MEMO = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from openmsftl_amd import _lib
    assert _lib.load().fc_abi_version() == 4
    yield
    _MEMO.clear()
    torch.cuda.empty_cache()


def memo(key, make):
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


def round_clients():
    """M = 7: five clients base + 0.3 noise, client 2 = 5 noise, the last one -3 base."""
    def make():
        from openmsftl_amd import Compression
        rng = np.random.default_rng(20261020)
        base = rng.standard_normal(N_R)
        grads = []
        for i in range(7):
            noise = rng.standard_normal(N_R)
            g = 5.0 * noise if i == 2 else -3.0 * base if i == 6 else base + 0.3 * noise
            grads.append(g.astype(np.float32))
        rows = [co.compress(TOP_CFG, g) for g in grads]            # the oracle's 'top' rows
        clients = [types.SimpleNamespace(C=Compression(dict(TOP_CFG)), grad=g, client_id=i)
                   for i, g in enumerate(grads)]
        return clients, rows
    return memo("round", make)


def round_packets(clients):
    """The packets gram_round makes of the clients, and their Gram / row sums, recomputed."""
    from openmsftl_amd import codec
    grads = [torch.from_numpy(c.grad).cuda() for c in clients]
    pk = codec.encode_top_batch(grads, round(FRAC * N_R))
    codec.resolve(pk)
    return pk


def fold32(c32, rows, start=None):
    """acc = fl32(acc + fl32(c32_i * row_i)) in row order, from +0 or from ``start``."""
    acc = np.zeros(rows[0].shape[0], np.float32) if start is None else start.astype(np.float32).copy()
    for ci, r in zip(c32, rows):
        acc = np.add(acc, np.multiply(r, np.float32(ci)))
    return acc


def aggregator(scheme, **extra):
    from openmsftl_amd.aggregation import Aggregator
    return Aggregator(dict(SCHEMES[scheme], **extra))


def pure_coeffs(scheme, K, pk, v=None, cfg=None):
    """(a, c) of the pure rule function on the Gram and dot products of the packets."""
    from openmsftl_amd import codec, gar
    cfg = cfg or SCHEMES[scheme]
    M = K.shape[0]
    w = np.full(M, 1.0 / M, np.float32)
    if scheme == "spectral_gram":
        s = codec.dot_dense(pk, None).cpu().numpy()[:M]
        return 0.0, gar.spectral_coeffs(K, w, N_R, rank=cfg.get("rank"),
                                        adaptive_rank_th=cfg.get("adaptive_rank_th"),
                                        drop_top_comp=cfg.get("drop_top_comp", False), row_sums=s)[0]
    if scheme == "geometric_median":
        return 0.0, gar.geometric_median_coeffs(K, w, cfg.get("gm_iters", 100), cfg.get("gm_tol", 1e-12),
                                                cfg.get("gm_nu", 1e-6))[0]
    if v is None:
        return 0.0, gar.centered_clip_coeffs(K, None, 0.0, TAU, 3)[1]
    r = codec.dot_dense(pk, torch.from_numpy(v).cuda()).cpu().numpy()
    return gar.centered_clip_coeffs(K, r[:M], float(r[M]), TAU, 3)


def rng_state():
    """The whole state of np.random: the key words, the position among them (all that a draw of
    fewer than 624 words moves) and the cached Gaussian."""
    name, key, pos, has_gauss, cached = np.random.get_state()
    return name, key.tobytes(), int(pos), int(has_gauss), float(cached)


# ---- the bit-level fold contract -------------------------------------------------------------
@pytest.mark.parametrize("scheme", list(SCHEMES))
def test_bit_level_fold_contract(scheme):
    from openmsftl_amd import codec
    clients, rows = round_clients()
    agg = aggregator(scheme)
    state = rng_state()
    agg.aggregate_grads(clients)
    assert rng_state() == state                                       # draws nothing
    assert agg.agg_path == "gram" and agg.curr_G is None
    assert agg.agg_grad.dtype == np.float32 and agg.agg_grad.shape == (N_R,)
    pk = round_packets(clients)
    K = codec.gram(pk).cpu().numpy()
    a, c = pure_coeffs(scheme, K, pk)
    assert agg.gar.coeffs.dtype == np.float64 and agg.gar.coeffs.tobytes() == c.tobytes()
    assert agg.gar.carry == 0.0 and agg.gar.excluded == []
    want = fold32(c.astype(np.float32), rows)
    assert agg.agg_grad.tobytes() == want.tobytes()
    assert np.all(np.isfinite(agg.agg_grad)) and np.any(agg.agg_grad != 0)


# ---- against the dense float64 oracles -------------------------------------------------------
def dense_weiszfeld(R, alpha, T, nu):
    z = alpha @ R
    nu_abs = nu * np.sqrt(np.max(np.sum(R * R, axis=1)))
    c, seen = alpha.copy(), []
    for _ in range(T):
        dist = np.sqrt(np.sum((R - z[None, :]) ** 2, axis=1))
        seen.append(dist)
        beta = alpha / np.maximum(nu_abs, dist)
        c = beta / np.sum(beta)
        z = c @ R
    return c, z, np.array(seen)


def dense_centered_clip(R, v, tau, T):
    M = R.shape[0]
    z = np.zeros(R.shape[1]) if v is None else v.astype(np.float64).copy()
    a, c, seen = 1.0, np.zeros(M), []
    for _ in range(T):
        dist = np.sqrt(np.sum((R - z[None, :]) ** 2, axis=1))
        seen.append(dist)
        s = np.where(dist > tau, tau / dist, 1.0)
        z = z + (s[:, None] * (R - z[None, :])).sum(axis=0) / M
        a, c = a * (1.0 - s.sum() / M), c * (1.0 - s.sum() / M) + s / M
    return a, c, z, np.array(seen)


def dense_spectral(R, w, rank, th, drop):
    X = R.T
    if not rank or rank > min(X.shape):
        rank = min(X.shape)
    _, S, V = np.linalg.svd(X, full_matrices=False)
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
    return c, c @ R, S, (lo, hi)


def _cnz(R):
    M = R.shape[0]
    return max(int(np.count_nonzero((R[i] != 0) & (R[j] != 0))) for i in range(M) for j in range(i, M))


def iteration_bound(R, T, c_max, d_min, extra=0.0):
    """tests/test_rules_host.py's bound with the Gram kernel's error: |delta c| <= T * 2 *
    ((8 M c_max + 4 c_nz) 2^-53 Kx / d_min^2 + N 2^-53) * c_max, Kx = max K_ii (and |v|^2)."""
    M, N = R.shape
    Kx = max(float(np.max(np.sum(R * R, axis=1))), extra)
    c_max = max(1.0, c_max)
    return T * 2.0 * ((8.0 * (M + 1) * c_max + 4.0 * _cnz(R)) * U * Kx / d_min ** 2 + N * U) * c_max


def spectral_bound(R, kept, w):
    M = R.shape[0]
    lam = np.sort(np.linalg.eigvalsh(R @ R.T))[::-1]
    lo, hi = kept
    inside, outside = lam[lo:hi], np.concatenate([lam[:lo], lam[hi:]])
    floor = 8 * M * U * np.linalg.norm(w)
    if inside.size == 0 or outside.size == 0:
        return floor, np.inf
    gap = float(np.min(np.abs(inside[:, None] - outside[None, :])))
    dK = (M * _cnz(R) * U + M * 2.0 ** -52) * lam[0]
    return 2 * 2 * dK / gap * np.linalg.norm(w) + floor, gap / lam[0]


def assert_close_to_dense(got, z, c, R, cb, what, carry=None):
    """|got - z| <= (M + 1) 2^-24 sum |c_i d_i| + cb sum |d_i| per coordinate (+ the carried term)."""
    M = R.shape[0]
    mag = np.sum(np.abs(c[:, None] * R), axis=0)
    per = cb * np.sum(np.abs(R), axis=0)
    if carry is not None:
        a, v = carry
        mag = mag + np.abs(a * v.astype(np.float64))
        per = per + cb * np.abs(v.astype(np.float64))
        M += 1
    per = per + (M + 1) * 2.0 ** -24 * mag
    err = np.abs(got.astype(np.float64) - z)
    ratio = np.max(err / np.maximum(per, 1e-300)) if np.any(per > 0) else 0.0
    print(f"{what}: max |err| {err.max():.3e}, max err/bound {ratio:.3e}")
    assert np.all(err <= per), what


def test_geometric_median_against_the_dense_oracle():
    clients, rows = round_clients()
    R = np.stack(rows).astype(np.float64)
    T = 20
    alpha = np.full(7, 1.0 / 7, np.float32).astype(np.float64)
    c_w, z, seen = dense_weiszfeld(R, alpha, T, 1e-6)
    assert seen.min() >= 1e-3 * np.sqrt(np.max(np.sum(R * R, axis=1)))       # precondition
    agg = aggregator("geometric_median", gm_iters=T, gm_tol=-1.0)            # no early stop
    agg.aggregate_grads(clients)
    assert agg.gar.iterations == T
    cb = iteration_bound(R, T, float(np.max(np.abs(c_w))), float(seen.min()))
    err = float(np.max(np.abs(agg.gar.coeffs - c_w)))
    print(f"geometric median coefficients {agg.gar.coeffs}: max |err| {err:.3e}, err/bound {err / cb:.3e}")
    assert err <= cb
    assert_close_to_dense(agg.agg_grad, z, c_w, R, cb, "geometric median aggregate")
    plain = aggregator("geometric_median")                                   # the defaults stop early
    plain.aggregate_grads(clients)
    assert 1 < plain.gar.iterations < 100
    assert plain.gar.coeffs[2] < plain.gar.coeffs[0] and plain.gar.coeffs[6] < plain.gar.coeffs[0]


def test_spectral_against_the_dense_oracle_and_the_golden():
    """Against the exact dense-SVD aggregate within the fold bound plus the coefficient bound, and
    against the reference's recorded aggregate within 2 e_ref max|agg_exact| on top; Sigma_tracked
    grows by one per round and holds S within 2 e_ref of the reference's."""
    sys.path.insert(0, GOLDEN)
    try:
        from npz_parts import load_parts
    finally:
        sys.path.remove(GOLDEN)
    arrays = load_parts(GOLDEN, "golden_spectral")
    with open(os.path.join(GOLDEN, "manifest_spectral.json")) as fh:
        man = json.load(fh)
    clients, rows = round_clients()
    R = np.stack(rows).astype(np.float64)
    w = np.full(7, 1.0 / 7, np.float32).astype(np.float64)
    assert len(man["cases"]) == 5
    for name, case in man["cases"].items():
        rank, th, drop = case["rank"], case["adaptive_rank_th"], case["drop_top_comp"]
        agg = aggregator("spectral_gram", rank=rank, adaptive_rank_th=th, drop_top_comp=drop)
        agg.aggregate_grads(clients)
        assert agg.agg_path == "gram" and len(agg.gar.Sigma_tracked) == 1
        c_w, z, S_w, kept = dense_spectral(R, w, rank, th, drop)
        cb, rel_gap = spectral_bound(R, kept, w)
        assert rel_gap >= 1e-3                                                # precondition
        err = float(np.max(np.abs(agg.gar.coeffs - c_w)))
        print(f"{name}: kept {kept}, coefficients max |err| {err:.3e}, err/bound {err / cb:.3e}")
        assert err <= cb
        assert_close_to_dense(agg.agg_grad, z, c_w, R, cb, f"{name} against the dense SVD")
        exact, ref = arrays[f"{name}|agg_exact"], arrays[f"{name}|agg_ref"]
        e_ref, top = case["e_ref"], float(np.max(np.abs(exact)))
        own = 8 * 7 * 7 * U * float(np.max(np.abs(R)))        # the stored float64 reconstruction's own
        per = (8 * 2.0 ** -24 * np.sum(np.abs(c_w[:, None] * R), axis=0)
               + cb * np.sum(np.abs(R), axis=0) + own)
        got = agg.agg_grad.astype(np.float64)
        assert np.all(np.abs(got - exact) <= per), f"{name}: against the golden exact aggregate"
        assert np.all(np.abs(got - ref.astype(np.float64)) <= per + 2 * e_ref * top), \
            f"{name}: against the reference's aggregate"
        S = agg.gar.Sigma_tracked[-1]
        S_ref = arrays[f"{name}|S_ref"]
        assert S.dtype == np.float64 and S.shape == S_ref.shape
        if e_ref > 0:
            assert np.all(np.abs(S - S_ref) <= 2 * e_ref * S_ref), f"{name}: S"
        else:                      # the all-zero aggregate: tests/test_rules_host.py ties this S
            assert np.array_equal(agg.gar.coeffs, np.zeros(7)) and not np.any(agg.agg_grad)
        agg.aggregate_grads(clients)                                          # a second round appends
        assert len(agg.gar.Sigma_tracked) == 2 and agg.gar.Sigma_tracked[1].tobytes() == S.tobytes()


# ---- centered clipping over three rounds ------------------------------------------------------
def test_centered_clip_three_rounds_carry_and_reset(monkeypatch):
    from openmsftl_amd import codec
    clients, rows = round_clients()
    R = np.stack(rows).astype(np.float64)
    calls = []
    real = codec.dot_dense
    monkeypatch.setattr(codec, "dot_dense", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    agg = aggregator("centered_clip")
    pk = round_packets(clients)
    K = codec.gram(pk).cpu().numpy()
    # round 1: the zero start, no dot call, nothing carried
    agg.aggregate_grads(clients)
    assert calls == [] and agg.gar.carry == 0.0
    _, c1 = pure_coeffs("centered_clip", K, pk)
    assert agg.gar.coeffs.tobytes() == c1.tobytes()
    first = agg.agg_grad.copy()
    assert first.tobytes() == fold32(c1.astype(np.float32), rows).tobytes()
    assert agg.gar.v is not None and agg.gar.v.is_cuda and agg.gar.v.dtype == torch.float32
    assert agg.gar.v.cpu().numpy().tobytes() == first.tobytes()
    a_w, c_w, z, seen = dense_centered_clip(R, None, TAU, 3)
    assert np.min(np.abs(seen - TAU)) >= 1e-6 * TAU and seen.min() >= 1e-3 * np.sqrt(np.max(np.diag(R @ R.T)))
    cb = iteration_bound(R, 3, float(np.max(np.abs(c_w))), float(seen.min()))
    assert np.max(np.abs(c1 - c_w)) <= cb
    assert_close_to_dense(first, z, c_w, R, cb, "centered clip, round 1")
    # rounds 2 and 3 carry v
    prev = first
    for rnd in (2, 3):
        n_calls = len(calls)
        agg.aggregate_grads(clients)
        assert len(calls) == n_calls + 1
        a, c = pure_coeffs("centered_clip", K, pk, v=prev)
        calls.pop()                                                   # the test's own dot call
        assert agg.gar.carry == a and agg.gar.coeffs.tobytes() == c.tobytes() and a != 0.0
        start = np.multiply(prev, np.float32(a))                      # fl32(a32 * v)
        want = fold32(c.astype(np.float32), rows, start=start)
        assert agg.agg_grad.tobytes() == want.tobytes(), f"round {rnd}"
        a_w, c_w, z, seen = dense_centered_clip(R, prev, TAU, 3)
        assert np.min(np.abs(seen - TAU)) >= 1e-6 * TAU
        q = float(prev.astype(np.float64) @ prev.astype(np.float64))
        cb = iteration_bound(R, 3, max(float(np.max(np.abs(c_w))), abs(a_w)), float(seen.min()), extra=q)
        assert max(np.max(np.abs(c - c_w)), abs(a - a_w)) <= cb
        assert_close_to_dense(agg.agg_grad, z, c_w, R, cb, f"centered clip, round {rnd}", carry=(a_w, prev))
        prev = agg.agg_grad.copy()
        assert agg.gar.v.cpu().numpy().tobytes() == prev.tobytes()
    assert prev.tobytes() != first.tobytes()
    # reset(): round 1's bits come back
    agg.gar.reset()
    assert agg.gar.v is None
    agg.aggregate_grads(clients)
    assert agg.agg_grad.tobytes() == first.tobytes() and agg.gar.carry == 0.0
    # another length: an error, not a silent reset
    from openmsftl_amd import Compression
    short = [types.SimpleNamespace(C=Compression(dict(TOP_CFG)), grad=c.grad[:CH + 7].copy(), client_id=i)
             for i, c in enumerate(clients)]
    with pytest.raises(ValueError, match="carried vector"):
        agg.aggregate_grads(short)
    assert agg.gar.v.numel() == N_R


# ---- an excluded client -----------------------------------------------------------------------
@pytest.mark.parametrize("scheme", list(SCHEMES))
def test_a_client_with_a_kept_inf_is_excluded(scheme):
    """Client 3's gradient holds an inf, which 'top' keeps: coefficient 0, listed in excluded, and
    the aggregate is the round without that client bit for bit (its weights restricted: 1/7
    each, not renormalised)."""
    from openmsftl_amd import Compression
    clients, _ = round_clients()
    bad = 3
    g = clients[bad].grad.copy()
    g[1234] = np.float32(np.inf)
    poisoned = list(clients)
    poisoned[bad] = types.SimpleNamespace(C=Compression(dict(TOP_CFG)), grad=g, client_id=bad)
    agg = aggregator(scheme)
    agg.aggregate_grads(poisoned)
    assert agg.agg_path == "gram" and agg.gar.excluded == [bad]
    assert agg.gar.coeffs[bad] == 0.0 and np.all(np.isfinite(agg.gar.coeffs))
    assert np.all(np.isfinite(agg.agg_grad)) and agg.agg_grad.dtype == np.float32
    rest = [c for i, c in enumerate(clients) if i != bad]
    ref = aggregator(scheme)
    ref.gar.gradient_weights = np.full(6, np.float32(1.0) / np.float32(7.0), dtype=np.float32)
    assert ref.gar.gradient_weights.tobytes() == np.full(7, 1.0 / 7, np.float32)[:6].tobytes()
    ref.aggregate_grads(rest)
    assert ref.gar.excluded == []
    assert np.delete(agg.gar.coeffs, bad).tobytes() == ref.gar.coeffs.tobytes()
    assert agg.agg_grad.tobytes() == ref.agg_grad.tobytes()


# ---- what stays as it was ---------------------------------------------------------------------
def test_the_two_existing_keys_still_raise_and_gram_analysis_still_appends():
    from openmsftl_amd.aggregation import Aggregator
    clients, _ = round_clients()
    with pytest.raises(NotImplementedError, match="pc_analysis"):
        Aggregator({"aggregation_scheme": "fed_avg", "pc_analysis": True}).aggregate_grads(clients)
    with pytest.raises(NotImplementedError, match="SpectralFedAvg"):
        Aggregator({"aggregation_scheme": "fed_spectral_avg"})
    agg = aggregator("geometric_median", pc_analysis="gram")
    agg.aggregate_grads(clients)
    assert agg.agg_path == "gram" and len(agg.gar.Sigma_tracked) == 1
    assert agg.gar.Sigma_tracked[0].shape == (7,) and np.all(np.diff(agg.gar.Sigma_tracked[0]) <= 0)
    # "spectral_gram" with pc_analysis "gram": two entries per round, the rule's S[:rank] first,
    # then all seven of the whole Gram.  Both come from LAPACK's symmetric eigenvalues of the same
    # K (eigh and eigvalsh), each within a few M 2^-52 lambda_max of the exact ones; through the
    # square root that is lambda_max / s_i per value, and 8 covers the two routines' constants.
    spec = aggregator("spectral_gram", rank=3, adaptive_rank_th=0, pc_analysis="gram")
    for rounds in (1, 2):
        spec.aggregate_grads(clients)
        assert [x.shape for x in spec.gar.Sigma_tracked] == [(3,), (7,)] * rounds
    own, full = spec.gar.Sigma_tracked[2], spec.gar.Sigma_tracked[3]
    assert np.all(np.abs(own - full[:3]) <= 8 * 7 * 2.0 ** -52 * full[0] ** 2 / full[:3])


def test_linear_rule_aggregate_packets_without_a_given_gram():
    """aggregate_packets computes the Gram itself when none is given, and fills a caller's out."""
    from openmsftl_amd import gar
    clients, rows = round_clients()
    pk = round_packets(clients)
    rule = gar.GeometricMedian({})
    out = torch.empty(N_R, dtype=torch.float32, device="cuda")
    assert rule.aggregate_packets(pk, out=out) is out
    via = aggregator("geometric_median")
    via.aggregate_grads(clients)
    assert out.cpu().numpy().tobytes() == via.agg_grad.tobytes()
    assert rule.coeffs.tobytes() == via.gar.coeffs.tobytes()
