"""fc_packets_gram (csrc/fc_gram.hip) and its consumers (codec.gram, gar.Krum, the Aggregator's
"gram" route) on an MI355X.

Run:  python -m pytest tests/test_gram_gpu.py -m gpu -q

Hand-built packets come from oracle/packet_oracle.py's builders: every slot position a packet
does not list holds the poison pair (index 0xFFFF, value NaN), so a read past a count shows up
as NaN in the Gram.  The expected Gram is computed here: rows from po.decode_sparse (the rows
po.decode_packet spreads out), every product in float64 (two float32 multiply exactly) and every
entry summed with math.fsum, which is correctly rounded.

Switch points of the kernel the shapes are built around (names of csrc/fc_gram.hip, not imported):
  kGT = 8           clients per tile: M in {1, 2, T-1, T, T+1, 2T+1, 65, 128}
  kGR * 64 = 256    entries per (client, quarter) held in registers; more take the tail loop
  kGWaves = 8       clients of the stream per round of the workgroup's waves
  n = 6 * 8192 + 2048 + 3: seven chunks, the last one ending three elements into quarter 1.
"""
import math
import types

import numpy as np
import pytest

from oracle import compression_oracle as co
from oracle import packet_oracle as po

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CH, QU = po.CHUNK, po.QUARTER
T = 8
N = 6 * CH + QU + 3
COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 513, 2048)
U = 2.0 ** -53
NEG0 = np.float32(-0.0)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from openmsftl_amd import _lib
    assert _lib.load().fc_abi_version() == 4
    yield
    _DEV.clear()
    _MEMO.clear()
    torch.cuda.empty_cache()


def _codec():
    from openmsftl_amd import codec
    return codec


# ---- builder output -> codec.Packet ----------------------------------------------------------
def _dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a).view(dt).copy()).cuda()


def to_packet(f):
    return _codec().Packet(
        n=f["n"], fmt=f["fmt"], k=int(f["hdr"]["k"]),
        val=_dev(f["val"], np.float32), cnt=_dev(f["cnt"], np.int32),
        hdr=_dev(np.frombuffer(f["hdr"].tobytes(), dtype=np.uint8), np.uint8),
        idx=_dev(f["idx"], np.int16), qoff=_dev(f["qoff"], np.int64))


_DEV, _MEMO = {}, {}


def packets_of(key, fields):
    """Device packets of a list of builder dicts, uploaded once per key."""
    if key not in _DEV:
        _DEV[key] = [to_packet(f) for f in fields]
    return _DEV[key]


def memo(key, make):
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


def gpu_gram(pkts):
    return _codec().gram(pkts).cpu().numpy()


# ---- the expected Gram ------------------------------------------------------------------------
def sparse_rows(fields):
    """Per packet (kept indices, float64 values, finite?) — d_i without spreading it out."""
    rows = []
    for f in fields:
        gidx, x, dz = po.decode_sparse(f, np.float32)
        rows.append((gidx, x.astype(np.float64), bool(np.all(np.isfinite(x)) and np.isfinite(dz))))
    return rows


def oracle_gram(rows):
    """(want, c, absum): want[i][j] = fsum of the exact products, NaN in the rows and columns of
    a client with a non-finite element; c[i][j] the coordinates both rows keep; absum[i][j] the
    sum of the products' magnitudes (the scale of the rounding bound)."""
    m = len(rows)
    want = np.zeros((m, m), np.float64)
    c = np.zeros((m, m), np.int64)
    absum = np.zeros((m, m), np.float64)
    for i in range(m):
        gi, xi, oki = rows[i]
        for j in range(i, m):
            gj, xj, okj = rows[j]
            if not (oki and okj):
                want[i, j] = want[j, i] = np.nan
                continue
            if i == j:
                prod = xi * xi
            else:
                _, ia, ib = np.intersect1d(gi, gj, assume_unique=True, return_indices=True)
                prod = xi[ia] * xj[ib]
            want[i, j] = want[j, i] = math.fsum(prod)
            c[i, j] = c[j, i] = prod.size
            absum[i, j] = absum[j, i] = math.fsum(np.abs(prod))
    return want, c, absum


def dense_rows(dense):
    """sparse_rows' form of dense float32 rows (kept = non-zero coordinates)."""
    out = []
    for r in dense:
        r = np.asarray(r, np.float32)
        gidx = np.nonzero(r)[0]
        out.append((gidx, r[gidx].astype(np.float64), bool(np.all(np.isfinite(r)))))
    return out


def _explain(got, want, limit=6):
    gn, wn = np.isnan(got), np.isnan(want)
    bad = np.argwhere((gn != wn) | (~gn & ~wn & (got.view(np.uint64) != want.view(np.uint64))))
    rows = [f"{len(bad)} of {got.size} entries differ"]
    rows += [f"  [{i},{j}] got {got[i, j]!r} want {want[i, j]!r}" for i, j in bad[:limit]]
    return "\n".join(rows)


def assert_same(got, want, what=""):
    assert po.same_bits(got, want), f"{what}\n{_explain(got, want)}"


def assert_symmetric(g):
    assert po.same_bits(g, np.ascontiguousarray(g.T)), "gram != gram.T"


def assert_within_bound(got, want, c, absum, what=""):
    """|got - want| <= c_ij * 2^-53 * sum_t |d_i[t] d_j[t]|: the worst case of any order of
    summation of exact products against the correctly rounded sum (per entry, not tuned)."""
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    err = np.abs(got[ok] - want[ok])
    bound = c[ok] * U * absum[ok]
    worst = np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0)) if err.size else 0.0
    print(f"{what}: max |err| {err.max() if err.size else 0.0:.3e}, max err/bound {worst:.3e}")
    assert np.all(err <= bound), f"{what}: {int(np.sum(err > bound))} entries above the bound"


# ---- designed supports ------------------------------------------------------------------------
def quarters(n=N):
    """(first element, capacity) of every chunk quarter of a length-n gradient."""
    return [(s, min(QU, n - s)) for s in range(0, n, QU)]


def design_support(i):
    """Client i's kept coordinates: quarter Q holds COUNTS[(i + Q) % 10] of them (at most the
    quarter's capacity), from an offset and with a stride that depend on the client alone.
    Clients i and i + 10 of the same twenty share every coordinate (identical supports), runs of
    different offsets are disjoint or overlap in part, and a full quarter overlaps everything."""
    off = (i % 10) * 150 + (i // 20) * 37
    stride = (1, 3, 5)[(i // 20) % 3]
    out = []
    for Q, (start, cap) in enumerate(quarters()):
        cnt = min(COUNTS[(i + Q) % 10], cap)
        if cap == QU:
            loc = np.sort((off + np.arange(cnt, dtype=np.int64) * stride) % QU)
        else:
            loc = np.arange(cnt, dtype=np.int64)
        out.append(start + loc)
    return np.concatenate(out)


def int_values(rng, size):
    """Small integers of both signs as float32, every zero a -0.0: all sums are exact."""
    v = rng.integers(-8, 9, size=size).astype(np.float32)
    v[v == 0] = NEG0
    return v


def exact_fields(m=128):
    def make():
        out = []
        for i in range(m):
            idx = design_support(i)
            val = int_values(np.random.default_rng([i, 11]), idx.size)
            out.append(po.build_idxval(N, idx, val, thresh=0, codec=po.CODEC_TOP, k=idx.size))
        return out
    return memo("exact", make)


def exact_oracle():
    return memo("exact-oracle", lambda: oracle_gram(sparse_rows(exact_fields())))


def test_design_covers_what_it_claims():
    s = [set(design_support(i).tolist()) for i in (0, 10, 1, 3, 25)]
    assert s[0] == s[1] and s[0] != s[2]                  # identical supports, and others
    per = np.array([[np.sum((design_support(i) >= st) & (design_support(i) < st + cap))
                     for st, cap in quarters()] for i in range(10)])
    assert set(per[:, :24].ravel().tolist()) == set(COUNTS)
    assert per[:, 25].max() == 3 and per[:, 25].min() == 0      # three elements into quarter 1
    q0 = [set((design_support(i) % QU)[design_support(i) < QU].tolist()) for i in range(10)]
    pairs = [(a, b) for a in range(10) for b in range(a + 1, 10) if q0[a] and q0[b]]
    assert any(not (q0[a] & q0[b]) for a, b in pairs), "no disjoint pair"
    assert any((q0[a] & q0[b]) and (q0[a] - q0[b]) and (q0[b] - q0[a]) for a, b in pairs), "no partial overlap"


# ---- exactness --------------------------------------------------------------------------------
@pytest.mark.parametrize("M", [1, 2, T - 1, T, T + 1, 2 * T + 1, 65, 128])
def test_exact_sums_equal_the_oracle_bit_for_bit(M):
    """Small-integer values: every sum is exact, so any order of summation gives the oracle's
    bits.  The first M clients of one set of 128 (the oracle's top-left block)."""
    want, _, _ = exact_oracle()
    assert np.all(np.abs(want) < 2.0 ** 40)
    pk = packets_of("exact", exact_fields())
    got = gpu_gram(pk[:M])
    assert got.shape == (M, M) and got.dtype == np.float64
    assert_same(got, np.ascontiguousarray(want[:M, :M]), f"M={M}")
    assert_symmetric(got)


# ---- rounding, symmetry, determinism ----------------------------------------------------------
def normal_fields(m=2 * T + 1):
    def make():
        out = []
        for i in range(m):
            idx = design_support(i)
            val = np.random.default_rng([i, 13]).standard_normal(idx.size).astype(np.float32)
            out.append(po.build_idxval(N, idx, val, thresh=0, codec=po.CODEC_TOP, k=idx.size))
        return out
    return memo("normal", make)


def test_rounding_within_the_worst_case_of_any_order():
    f = normal_fields()
    want, c, absum = memo("normal-oracle", lambda: oracle_gram(sparse_rows(f)))
    got = gpu_gram(packets_of("normal", f))
    assert_within_bound(got, want, c, absum, f"normal values, M={len(f)}")
    assert np.all(got[c == 0] == 0.0)


def test_symmetric_and_the_same_bits_twice():
    pk = packets_of("normal", normal_fields())
    a = gpu_gram(pk)
    b = gpu_gram(pk)
    assert_symmetric(a)
    assert_same(a, b, "two calls on the same packets")
    out = torch.empty((len(pk), len(pk)), dtype=torch.float64, device="cuda")
    assert _codec().gram(pk, out=out) is out
    assert_same(out.cpu().numpy(), a, "into a caller's tensor")


# ---- slack and the tie cut --------------------------------------------------------------------
TIE = np.float32(1.5)


def slack_fields(i, Ti, nan_at=None):
    """A top-k packet as the sampled encoder leaves it: entries above the k-th magnitude 1.5,
    entries EQUAL to it on both sides of the index cut Ti, and slack below it.  Kept: comp >=
    (key(1.5) << ib | Ti).  Values are multiples of 0.5: every sum exact.  100..400 entries per
    quarter (both sides of the register rounds)."""
    rng = np.random.default_rng([i, 17])
    idx = []
    for start, cap in quarters():
        cnt = min(int(rng.integers(100, 401)), cap)
        idx.append(start + np.sort(rng.choice(cap, size=cnt, replace=False)))
    idx = np.concatenate(idx).astype(np.int64)
    u = rng.random(idx.size)
    mag = rng.choice(np.array([2.0, 2.5, 3.0], np.float32), size=idx.size)
    mag[u < 0.3] = rng.choice(np.array([0.5, 1.0], np.float32), size=int(np.sum(u < 0.3)))
    mag[(u >= 0.3) & (u < 0.5)] = TIE
    val = (mag * rng.choice(np.array([-1.0, 1.0], np.float32), size=idx.size)).astype(np.float32)
    if nan_at is not None:
        val[nan_at] = np.float32(np.nan)
    ib = po.index_bits(N)
    thresh = (int(po.mag_key(np.array([TIE]))[0]) << ib) | int(Ti)
    keep = (np.abs(val) > TIE) | ((np.abs(val) == TIE) & (idx >= Ti)) | np.isnan(val)
    return po.build_idxval(N, idx, val, thresh=thresh, lower=1, codec=po.CODEC_TOP,
                           k=int(keep.sum())), idx, val, keep


SLACK_TI = [3 * CH + QU + 1000, 3 * CH + 2 * QU, 0, N - 1, 5, 2 * CH + 7, 6 * CH + QU + 1,
            CH, 4 * CH + 3 * QU + 2047]


def test_slack_and_tie_cut_only_kept_entries_count():
    assert len(SLACK_TI) == T + 1
    built = [slack_fields(i, Ti) for i, Ti in enumerate(SLACK_TI)]
    fields = [b[0] for b in built]
    clean = []
    for (f, idx, val, keep) in built:
        gk, vk = po.kept_entries(f)
        assert np.array_equal(gk, idx[keep]) and gk.size < idx.size       # slack is listed
        clean.append(po.build_idxval(N, gk, vk, thresh=0, codec=po.CODEC_TOP, k=gk.size))
    f0, idx0, val0, keep0 = built[0]
    ties = np.abs(val0) == TIE
    assert np.any(ties & keep0) and np.any(ties & ~keep0)                 # both sides of the cut
    want, _, _ = oracle_gram(sparse_rows(fields))
    got = gpu_gram([to_packet(f) for f in fields])
    got_clean = gpu_gram([to_packet(f) for f in clean])
    assert_same(got, want, "packets with slack against the oracle")
    assert_same(got, got_clean, "packets with slack against the same packets rebuilt without it")


# ---- codec mix --------------------------------------------------------------------------------
def half_values(rng, size):
    v = (rng.integers(-6, 7, size=size) * 0.5).astype(np.float32)
    v[v == 0] = NEG0
    return v


def mix_fields():
    def make():
        rng = np.random.default_rng(23)
        ib = po.index_bits(N)
        seed, offset = 0xC0FFEE_0000_0042, 9
        gidx = design_support(5)
        comp = (po.philox_keys_at(gidx, seed, offset).astype(np.uint64) << np.uint64(ib)) | gidx.astype(np.uint64)
        philox = po.build_idxval(N, gidx, half_values(rng, gidx.size),
                                 thresh=int(np.sort(comp)[gidx.size // 2]), lower=int(comp.min()),
                                 codec=po.CODEC_RAND, key_mode=po.KEY_PHILOX,
                                 k=gidx.size - gidx.size // 2, seed=seed, offset=offset)
        assert 0 < po.kept_entries(philox)[0].size < gidx.size
        bidx = np.nonzero(rng.random(N) < 0.3)[0]
        biased = po.build_idxval(N, bidx, half_values(rng, bidx.size), thresh=0,
                                 codec=po.CODEC_DROPOUT_BIASED, p=0.3, seed=4)
        uidx = np.nonzero(rng.random(N) < 0.5)[0]            # ~1024 per quarter: the tail loop
        unbiased = po.build_idxval(N, uidx, half_values(rng, uidx.size), thresh=0,
                                   codec=po.CODEC_DROPOUT_UNBIASED, p=0.5, seed=4)
        tops = [slack_fields(40 + i, Ti)[0] for i, Ti in enumerate(SLACK_TI[:6])]
        return [tops[0], philox, tops[1], biased, tops[2], tops[3], unbiased, tops[4], tops[5]]
    return memo("mix", make)


def test_codec_mix_philox_and_dropout_beside_topk():
    f = mix_fields()
    assert len(f) == T + 1
    want, _, _ = oracle_gram(sparse_rows(f))
    assert np.all(np.isfinite(want))
    got = gpu_gram([to_packet(x) for x in f])
    assert_same(got, want, "top-k + Philox rand-k + dropout-biased + dropout-unbiased(p=0.5)")
    assert_symmetric(got)


# ---- the NaN rule -----------------------------------------------------------------------------
def _check_poisoned(fields, bad, what):
    want, _, _ = oracle_gram(sparse_rows(fields))
    got = gpu_gram([to_packet(f) for f in fields])
    m = len(fields)
    good = [i for i in range(m) if i not in bad]
    for b in bad:
        assert np.all(np.isnan(got[b, :])) and np.all(np.isnan(got[:, b])), f"{what}: client {b}"
        assert np.all(np.isnan(want[b, :]))
    rest = gpu_gram([to_packet(fields[i]) for i in good])
    assert np.all(np.isfinite(rest))
    assert_same(np.ascontiguousarray(got[np.ix_(good, good)]), rest, f"{what}: the remaining clients")
    assert_same(got, want, what)


def test_nan_rule_kept_nan_and_kept_inf():
    fields = list(exact_fields()[:T + 1])
    a, b = 2, 6
    # client a: a top-k packet with slack whose kept entries hold a NaN
    fa, idx, val, keep = slack_fields(90, SLACK_TI[0], nan_at=777)
    assert np.isnan(val[777]) and keep[777]
    fields[a] = fa
    # client b: a kept +inf among small integers
    ib_idx = design_support(b)
    vb = int_values(np.random.default_rng([b, 11]), ib_idx.size)
    vb[ib_idx.size // 2] = np.float32(np.inf)
    fields[b] = po.build_idxval(N, ib_idx, vb, thresh=0, codec=po.CODEC_TOP, k=ib_idx.size)
    _check_poisoned(fields, (a, b), "kept NaN in client 2, kept +inf in client 6")


def test_nan_rule_dropout_unbiased_p0_and_overflowing_scale():
    fields = list(exact_fields()[:T + 1])
    idx = design_support(4)
    val = int_values(np.random.default_rng([4, 29]), idx.size)
    fields[4] = po.build_idxval(N, idx, val, thresh=0, codec=po.CODEC_DROPOUT_UNBIASED, p=0.0, seed=4)
    # fl32(fl64(v) / 1e-40) overflows float32 for every non-zero v
    fields[7] = po.build_idxval(N, idx, val, thresh=0, codec=po.CODEC_DROPOUT_UNBIASED, p=1e-40, seed=4)
    _check_poisoned(fields, (4, 7), "dropout-unbiased p = 0 (client 4), overflowing 1/p (client 7)")


# ---- real packets -----------------------------------------------------------------------------
N_R = 3 * CH + 5


def test_real_packets_from_the_batched_encoder():
    codec = _codec()
    k = round(0.25 * N_R)
    rng = np.random.default_rng(41)
    grads = [torch.from_numpy(rng.standard_normal(N_R).astype(np.float32)).cuda() for _ in range(5)]
    pk = codec.encode_top_batch(grads, k)
    dense = [codec.decode(p).cpu().numpy() for p in pk]
    assert all(int(np.count_nonzero(r)) == k for r in dense)
    want, c, absum = oracle_gram(dense_rows(dense))
    got = gpu_gram(pk)
    assert_within_bound(got, want, c, absum, "encode_top_batch packets, M=5")
    assert_symmetric(got)


def test_gram_rejects_what_it_cannot_take():
    codec = _codec()
    pk = packets_of("exact", exact_fields())
    with pytest.raises(ValueError, match="at most 128"):
        codec.gram(pk + pk[:1])
    other = to_packet(po.build_idxval(N_R, np.array([1, 9]), np.float32([1, 2]), thresh=0,
                                      codec=po.CODEC_TOP, k=2))
    with pytest.raises(ValueError, match="share n"):
        codec.gram([pk[0], other])
    g = torch.ones(N_R, dtype=torch.float32, device="cuda")
    bitmap = codec.encode_mask(g, 3, p=0.5, fmt=1)
    with pytest.raises(ValueError, match="idx/val"):
        codec.gram([bitmap])
    with pytest.raises(ValueError, match="no packets"):
        codec.gram([])


# ---- the Aggregator ---------------------------------------------------------------------------
FRAC = 0.25
TOP_CFG = {"compression_function": "top", "fraction_coordinate": FRAC}


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


def test_aggregator_krum_selects_the_oracles_client():
    from openmsftl_amd.aggregation import Aggregator
    clients, rows = round_clients()
    R = np.stack(rows).astype(np.float64)
    M, frac = len(rows), 0.5
    m = int(frac * M)
    dist = np.sqrt(((R[:, None, :] - R[None, :, :]) ** 2).sum(-1))
    scores = np.sort(dist, axis=1)[:, :m].sum(axis=1)
    order = np.argsort(scores, kind="stable")
    gap = (scores[order[1]] - scores[order[0]]) / scores[order[0]]
    print(f"krum oracle scores {scores}, relative gap {gap:.3e}")
    assert gap >= 1e-6                                        # precondition, on the oracle
    want = int(order[0])
    agg = Aggregator({"aggregation_scheme": "krum", "krum_frac": frac})
    agg.aggregate_grads(clients)
    assert agg.agg_path == "gram"
    assert agg.gar.selected == want
    assert np.allclose(agg.gar.scores, scores, rtol=1e-9)
    assert agg.agg_grad.dtype == np.float32
    assert agg.agg_grad.tobytes() == rows[want].tobytes()
    assert agg.curr_G is None and agg.gar.Sigma_tracked == []


def _sigma_check(sig, rows, what, condition_limit=None):
    """Per value |sigma_i - svd_i| <= (M c 2^-53 + M 2^-52) sigma_max^2 / sigma_i, c the largest
    c_ij: the Gram's error and the eigen-solver's, both through the square root."""
    R = np.stack(rows).astype(np.float64)
    want = np.linalg.svd(R, compute_uv=False)
    M = len(rows)
    assert sig.dtype == np.float64 and sig.shape == (M,) and np.all(np.diff(sig) <= 0)
    cond = want[0] / want[-1]
    if condition_limit is not None:
        assert cond <= condition_limit                                # precondition, on the oracle
    c = max(int(np.count_nonzero((R[i] != 0) & (R[j] != 0))) for i in range(M) for j in range(i, M))
    bound = (M * c * U + M * 2.0 ** -52) * want[0] ** 2 / want
    err = np.abs(sig - want)
    print(f"{what}: sigma {sig}, max err/bound {np.max(err / bound):.3e}, condition {cond:.3f}")
    assert np.all(err <= bound), what


def test_aggregator_fedavg_with_gram_analysis():
    """The Krum test's clients: agg_grad equals the "stream" route's bits, and Sigma_tracked holds
    G's singular values within the per-value bound.  These clients' oracle rows have
    sigma_max / sigma_min = 11.07 by construction (five rows share `base`, one is -3 base), so
    the precondition sigma_max / sigma_min <= 10 is asserted on the random round of the next
    test, where it holds; the bound itself carries the factor sigma_max^2 / sigma_i and is
    asserted here unchanged."""
    from openmsftl_amd.aggregation import Aggregator
    clients, rows = round_clients()
    plain = Aggregator({"aggregation_scheme": "fed_avg"})
    plain.aggregate_grads(clients)
    assert plain.agg_path == "stream"
    state = np.random.get_state()
    agg = Aggregator({"aggregation_scheme": "fed_avg", "pc_analysis": "gram"})
    agg.aggregate_grads(clients)
    assert agg.agg_path == "gram"
    assert np.array_equal(np.random.get_state()[1], state[1])        # draws nothing
    assert agg.agg_grad.tobytes() == plain.agg_grad.tobytes()
    assert len(agg.gar.Sigma_tracked) == 1 and plain.gar.Sigma_tracked == []
    sig = agg.gar.Sigma_tracked[-1]
    _sigma_check(sig, rows, "base/noise clients")
    agg.aggregate_grads(clients)                                      # a second round appends
    assert len(agg.gar.Sigma_tracked) == 2
    assert agg.gar.Sigma_tracked[1].tobytes() == sig.tobytes()


def test_aggregator_gram_analysis_on_independent_clients():
    """Seven independent normal gradients, same shape and fraction: sigma_max / sigma_min <= 10
    is asserted on the oracle rows, then the same per-value bound."""
    from openmsftl_amd import Compression
    from openmsftl_amd.aggregation import Aggregator
    rng = np.random.default_rng(20261021)
    grads = [rng.standard_normal(N_R).astype(np.float32) for _ in range(7)]
    rows = [co.compress(TOP_CFG, g) for g in grads]
    clients = [types.SimpleNamespace(C=Compression(dict(TOP_CFG)), grad=g, client_id=i)
               for i, g in enumerate(grads)]
    plain = Aggregator({"aggregation_scheme": "fed_avg"})
    plain.aggregate_grads(clients)
    agg = Aggregator({"aggregation_scheme": "fed_avg", "pc_analysis": "gram"})
    agg.aggregate_grads(clients)
    assert (plain.agg_path, agg.agg_path) == ("stream", "gram")
    assert agg.agg_grad.tobytes() == plain.agg_grad.tobytes()
    _sigma_check(agg.gar.Sigma_tracked[-1], rows, "independent clients", condition_limit=10)


def test_the_two_existing_keys_still_raise():
    from openmsftl_amd.aggregation import Aggregator
    clients, _ = round_clients()
    with pytest.raises(NotImplementedError, match="pc_analysis"):
        Aggregator({"aggregation_scheme": "fed_avg", "pc_analysis": True}).aggregate_grads(clients)
    with pytest.raises(NotImplementedError, match="SpectralFedAvg"):
        Aggregator({"aggregation_scheme": "fed_spectral_avg"})


def test_krum_on_a_dense_G_matches_the_packet_route():
    from openmsftl_amd.gar import Krum
    clients, rows = round_clients()
    G = np.stack(rows)
    gar = Krum({"krum_frac": 0.5})
    out = gar.aggregate(torch.from_numpy(G).cuda())
    host = Krum({"krum_frac": 0.5})
    out_h = host.aggregate(G)
    assert isinstance(out_h, np.ndarray) and gar.selected == host.selected
    assert out.cpu().numpy().tobytes() == G[gar.selected].tobytes() == out_h.tobytes()
    agg_gar = Krum({"krum_frac": 0.5})
    pk = _codec().encode_top_batch([torch.from_numpy(c.grad).cuda() for c in clients],
                                   round(FRAC * N_R))
    got = agg_gar.aggregate_packets(pk)
    assert agg_gar.selected == gar.selected
    assert got.cpu().numpy().tobytes() == G[gar.selected].tobytes()
