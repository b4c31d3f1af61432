"""fc_packets_dot (csrc/fc_dot.hip) through codec.dot_dense on an MI355X.

Run:  python -m pytest tests/test_dot_gpu.py -m gpu -q

Hand-built packets come from oracle/packet_oracle.py's builders, on the geometry and the poison
convention of tests/test_gram_gpu.py: every slot position a packet does not list holds the
poison pair (index 0xFFFF, value NaN), so a read past a count shows up as NaN in the output.
The expected outputs are computed here: rows from po.decode_sparse, every product in float64
(two float32 multiply exactly) and every sum with math.fsum, which is correctly rounded.  Every
sum of the kernel starts from +0.0, so a sum whose terms are all -0.0 is +0.0, as fsum's is.

Switch points of the kernel the shapes are built around (names of csrc/fc_dot.hip, not imported):
  kVTile = 64       clients per workgroup, a second tile from client 64 on: M in {63, 64, 65, 128}
  kVWaves = 8       a wave takes the tile's clients w, w + 8, ...: M in {1, 2, 7, 8, 9}
  kVR * 64 = 256    entries of a (client, chunk) per round of loads: the per-quarter counts below
                    give chunk totals on both sides of 256, 512, ... and empty chunks
  n = 6 * 8192 + 2048 + 3: seven chunks, the last one ending three elements into quarter 1 (the
                    image's float4 loads end inside a vector: n is not a multiple of 4).
Those shapes give every k_dot workgroup ONE chunk and every lane of k_dot_fin at most one part.
The points that depend on n (dot_geom of csrc/fc_capi.hip; tiles = ceil(M / 64), kVSlices = 1024)
have tests of their own at the end of the file, on sparse packets over long vectors:
  slices > 64       a lane of k_dot_fin adds the parts of slices l, l + 64, ... and ORs their
                    flags: 130 chunks (130 slices: lanes 0 and 1 add three parts, the rest two)
  chunks > 1024 / tiles   a workgroup takes cps > 1 chunks: the barrier at the top of the chunk
                    loop and the carry of a client's sum from chunk to chunk.  1024 chunks are the
                    last with cps = 1 for M <= 64 (1024 slices) and give cps = 2 for M = 65;
                    1025 chunks, the last one five elements long, give cps = 2 (513 slices, the
                    last slice one chunk) for M <= 64 and cps = 3 (342 slices, the last slice two
                    chunks) for M = 65.  The poisoned clients there hold their non-finite entry in
                    a chunk that is not the first of its slice for cps = 2 and for cps = 3.
"""
import math

import numpy as np
import pytest

from oracle import packet_oracle as po

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CH, QU = po.CHUNK, po.QUARTER
N = 6 * CH + QU + 3
COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 513, 2048)
MS = [1, 2, 7, 8, 9, 63, 64, 65, 128]
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
    if key not in _DEV:
        _DEV[key] = [to_packet(f) for f in fields]
    return _DEV[key]


def memo(key, make):
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


def gpu_dot(pkts, v=None):
    vt = None if v is None else torch.from_numpy(np.ascontiguousarray(v, np.float32)).cuda()
    out = _codec().dot_dense(pkts, vt)
    assert out.dtype == torch.float64 and tuple(out.shape) == (len(pkts) + 1,)
    return out.cpu().numpy()


# ---- the expected outputs ---------------------------------------------------------------------
def sparse_rows(fields):
    rows = []
    for f in fields:
        gidx, x, dz = po.decode_sparse(f, np.float32)
        rows.append((gidx, x.astype(np.float64), bool(np.all(np.isfinite(x)) and np.isfinite(dz))))
    return rows


def oracle_dot(rows, v, n=N):
    """(want, c, absum): want[i] = fsum of the exact products d_i[t] v[t] (NaN for a client with a
    non-finite element), want[m] = fsum of v's squares (n for v = None); everything NaN when v
    is not finite.  c[i] the entries client i keeps, absum[i] the sum of |d_i[t] v[t]|."""
    m = len(rows)
    want, c, absum = np.zeros(m + 1), np.zeros(m + 1, np.int64), np.zeros(m + 1)
    v64 = None if v is None else np.asarray(v, np.float32).astype(np.float64)
    if v64 is not None and not np.all(np.isfinite(v64)):
        return np.full(m + 1, np.nan), c, absum
    for i, (gi, xi, ok) in enumerate(rows):
        if not ok:
            want[i] = np.nan
            continue
        prod = xi if v64 is None else xi * v64[gi]
        want[i], c[i], absum[i] = math.fsum(prod), prod.size, math.fsum(np.abs(prod))
    if v64 is None:
        want[m] = float(n)
    else:
        want[m] = absum[m] = math.fsum(v64 * v64)
        c[m] = n
    return want, c, absum


def _explain(got, want, limit=6):
    gn, wn = np.isnan(got), np.isnan(want)
    bad = np.nonzero((gn != wn) | (~gn & ~wn & (got.view(np.uint64) != want.view(np.uint64))))[0]
    rows = [f"{len(bad)} of {got.size} outputs differ"]
    rows += [f"  [{i}] got {got[i]!r} want {want[i]!r}" for i in bad[:limit]]
    return "\n".join(rows)


def assert_same(got, want, what=""):
    assert po.same_bits(got, want), f"{what}\n{_explain(got, want)}"


def assert_within_bound(got, want, c, absum, what=""):
    """|got - want| <= c_i * 2^-53 * sum_t |d_i[t] v[t]| (and n * 2^-53 * sum v^2 for the last
    output): the worst case of any order of summation of exact products against the correctly
    rounded sum (per output, not tuned)."""
    assert np.array_equal(np.isnan(got), np.isnan(want)), what
    ok = ~np.isnan(want)
    err, bound = np.abs(got[ok] - want[ok]), c[ok] * U * absum[ok]
    worst = np.max(np.where(bound > 0, err / np.where(bound > 0, bound, 1.0), 0.0))
    print(f"{what}: max |err| {err.max():.3e}, max err/bound {worst:.3e}")
    assert np.all(err <= bound), f"{what}: {int(np.sum(err > bound))} outputs above the bound"


# ---- designed supports (the Gram tests' geometry) ---------------------------------------------
def quarters(n=N):
    return [(s, min(QU, n - s)) for s in range(0, n, QU)]


def design_support(i):
    """Client i's kept coordinates: quarter Q holds COUNTS[(i + Q) % 10] of them (at most the
    quarter's capacity), from an offset and with a stride that depend on the client alone."""
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
    v = rng.integers(-8, 9, size=size).astype(np.float32)
    v[v == 0] = NEG0
    return v


def half_values(rng, size):
    v = (rng.integers(-6, 7, size=size) * 0.5).astype(np.float32)
    v[v == 0] = NEG0
    return v


def half_vector(seed=3):
    """Multiples of 0.5 in [-4, 4], both zeros present."""
    def make():
        v = (np.random.default_rng(seed).integers(-8, 9, size=N) * 0.5).astype(np.float32)
        v[::97][v[::97] == 0] = NEG0
        v[5] = NEG0
        assert np.any(np.signbit(v) & (v == 0)) and np.any(~np.signbit(v) & (v == 0))
        assert v.min() == -4.0 and v.max() == 4.0
        return v
    return memo(("half-v", seed), make)


def exact_fields(m=128):
    def make():
        out = []
        for i in range(m):
            idx = design_support(i)
            val = int_values(np.random.default_rng([i, 11]), idx.size)
            out.append(po.build_idxval(N, idx, val, thresh=0, codec=po.CODEC_TOP, k=idx.size))
        return out
    return memo("exact", make)


def test_design_covers_what_it_claims():
    per = np.array([[np.sum((design_support(i) >= st) & (design_support(i) < st + cap))
                     for st, cap in quarters()] for i in range(10)])
    assert set(per[:, :24].ravel().tolist()) == set(COUNTS)
    assert per[:, 25].max() == 3 and per[:, 25].min() == 0      # three elements into quarter 1
    chunk_tot = per[:, :24].reshape(10, 6, 4).sum(axis=2).ravel()
    assert chunk_tot.min() < 256 < chunk_tot.max() and np.any(chunk_tot > 512) and N % 4 == 3


# ---- exactness --------------------------------------------------------------------------------
@pytest.mark.parametrize("M", MS)
def test_exact_sums_equal_the_oracle_bit_for_bit(M):
    """Small-integer values and a v of multiples of 0.5: every sum is exact, so any order of
    summation gives the oracle's bits.  The first M clients of one set of 128."""
    v = half_vector()
    want, _, _ = memo("exact-oracle", lambda: oracle_dot(sparse_rows(exact_fields()), v))
    assert np.all(np.abs(want) < 2.0 ** 40)
    pk = packets_of("exact", exact_fields())
    got = gpu_dot(pk[:M], v)
    assert_same(got, np.concatenate([want[:M], want[128:]]), f"M={M}")


@pytest.mark.parametrize("M", MS)
def test_row_sums_with_the_all_ones_vector(M):
    want, _, _ = memo("ones-oracle", lambda: oracle_dot(sparse_rows(exact_fields()), None))
    pk = packets_of("exact", exact_fields())
    got = gpu_dot(pk[:M], None)
    assert got[M] == float(N)
    assert_same(got, np.concatenate([want[:M], want[128:]]), f"v = None, M={M}")
    ones = gpu_dot(pk[:M], np.ones(N, np.float32))
    assert_same(ones, got, f"v = ones against v = None, M={M}")


def test_empty_chunks_an_empty_packet_and_a_full_chunk():
    """A client listing two entries (every other chunk empty), one listing nothing at all, one
    whose second chunk lists all 8192 elements (32 full rounds), one keeping the last element."""
    rng = np.random.default_rng(53)
    sup = [np.array([3 * CH + 5, 3 * CH + QU]), np.zeros(0, np.int64), CH + np.arange(CH),
           np.array([0, N - 1])]
    fields = [po.build_idxval(N, s, int_values(rng, s.size), thresh=0, codec=po.CODEC_TOP, k=s.size)
              for s in sup]
    pk = [to_packet(f) for f in fields]
    for v in (half_vector(), None):
        want, _, _ = oracle_dot(sparse_rows(fields), v)
        got = gpu_dot(pk, v)
        assert_same(got, want, "sparse, empty and full clients")
        assert got[1] == 0.0 and not np.signbit(got[1])


# ---- rounding, determinism, out= --------------------------------------------------------------
def normal_fields(m=17):
    def make():
        out = []
        for i in range(m):
            idx = design_support(i)
            val = np.random.default_rng([i, 13]).standard_normal(idx.size).astype(np.float32)
            out.append(po.build_idxval(N, idx, val, thresh=0, codec=po.CODEC_TOP, k=idx.size))
        return out
    return memo("normal", make)


def normal_vector():
    return memo("normal-v", lambda: np.random.default_rng(131).standard_normal(N).astype(np.float32))


def test_rounding_within_the_worst_case_of_any_order():
    f, v = normal_fields(), normal_vector()
    want, c, absum = oracle_dot(sparse_rows(f), v)
    got = gpu_dot(packets_of("normal", f), v)
    assert_within_bound(got, want, c, absum, f"normal values, M={len(f)}")
    want1, c1, absum1 = oracle_dot(sparse_rows(f), None)
    assert_within_bound(gpu_dot(packets_of("normal", f), None), want1, c1, absum1, "normal values, v = None")


def test_the_same_bits_twice_and_into_a_callers_tensor():
    pk, v = packets_of("normal", normal_fields()), normal_vector()
    a, b = gpu_dot(pk, v), gpu_dot(pk, v)
    assert_same(a, b, "two calls on the same inputs")
    vt = torch.from_numpy(v).cuda()
    out = torch.empty(len(pk) + 1, dtype=torch.float64, device="cuda")
    assert _codec().dot_dense(pk, vt, out=out) is out
    assert_same(out.cpu().numpy(), a, "into a caller's tensor")
    with pytest.raises(ValueError, match="out must be"):
        _codec().dot_dense(pk, vt, out=torch.empty(len(pk), dtype=torch.float64, device="cuda"))


# ---- slack and the tie cut --------------------------------------------------------------------
TIE = np.float32(1.5)


def slack_fields(i, Ti, nan_at=None):
    """tests/test_gram_gpu.py's construction: a top-k packet as the sampled encoder leaves it,
    entries above the k-th magnitude 1.5, entries EQUAL to it on both sides of the index cut Ti,
    and slack below it.  Values are multiples of 0.5."""
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
    built = [slack_fields(i, Ti) for i, Ti in enumerate(SLACK_TI)]
    fields, clean = [b[0] for b in built], []
    for (f, idx, val, keep) in built:
        gk, vk = po.kept_entries(f)
        assert np.array_equal(gk, idx[keep]) and gk.size < idx.size       # slack is listed
        clean.append(po.build_idxval(N, gk, vk, thresh=0, codec=po.CODEC_TOP, k=gk.size))
    _, _, val0, keep0 = built[0]
    ties = np.abs(val0) == TIE
    assert np.any(ties & keep0) and np.any(ties & ~keep0)                 # both sides of the cut
    for v in (half_vector(), None):
        want, _, _ = oracle_dot(sparse_rows(fields), v)
        got = gpu_dot([to_packet(f) for f in fields], v)
        got_clean = gpu_dot([to_packet(f) for f in clean], v)
        assert_same(got, want, "packets with slack against the oracle")
        assert_same(got, got_clean, "packets with slack against the same packets rebuilt without it")


# ---- codec mix --------------------------------------------------------------------------------
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
        uidx = np.nonzero(rng.random(N) < 0.5)[0]            # ~4096 per chunk: sixteen rounds
        unbiased = po.build_idxval(N, uidx, half_values(rng, uidx.size), thresh=0,
                                   codec=po.CODEC_DROPOUT_UNBIASED, p=0.5, seed=4)
        tops = [slack_fields(40 + i, Ti)[0] for i, Ti in enumerate(SLACK_TI[:6])]
        return [tops[0], philox, tops[1], biased, tops[2], tops[3], unbiased, tops[4], tops[5]]
    return memo("mix", make)


def test_codec_mix_philox_and_dropout_beside_topk():
    f = mix_fields()
    pk = [to_packet(x) for x in f]
    for v in (half_vector(), None):
        want, _, _ = oracle_dot(sparse_rows(f), v)
        assert np.all(np.isfinite(want))
        assert_same(gpu_dot(pk, v), want, "top-k + Philox rand-k + dropout-biased + dropout-unbiased(p=0.5)")


# ---- the NaN rule -----------------------------------------------------------------------------
def _check_poisoned(fields, bad, what):
    pk = [to_packet(f) for f in fields]
    for v in (half_vector(), None):
        want, _, _ = oracle_dot(sparse_rows(fields), v)
        got = gpu_dot(pk, v)
        m = len(fields)
        for i in range(m):
            assert np.isnan(got[i]) == (i in bad), f"{what}: client {i}"
        assert np.isfinite(got[m])
        assert_same(got, want, what)


def test_nan_rule_kept_nan_and_kept_inf():
    fields = list(exact_fields()[:9])
    a, b = 2, 6
    fa, idx, val, keep = slack_fields(90, SLACK_TI[0], nan_at=777)
    assert np.isnan(val[777]) and keep[777]
    fields[a] = fa
    ib_idx = design_support(b)
    vb = int_values(np.random.default_rng([b, 11]), ib_idx.size)
    vb[ib_idx.size // 2] = np.float32(np.inf)
    fields[b] = po.build_idxval(N, ib_idx, vb, thresh=0, codec=po.CODEC_TOP, k=ib_idx.size)
    _check_poisoned(fields, (a, b), "kept NaN in client 2, kept +inf in client 6")


def test_nan_rule_dropout_unbiased_p0_and_overflowing_scale():
    fields = list(exact_fields()[:9])
    idx = design_support(4)
    val = int_values(np.random.default_rng([4, 29]), idx.size)
    fields[4] = po.build_idxval(N, idx, val, thresh=0, codec=po.CODEC_DROPOUT_UNBIASED, p=0.0, seed=4)
    fields[7] = po.build_idxval(N, idx, val, thresh=0, codec=po.CODEC_DROPOUT_UNBIASED, p=1e-40, seed=4)
    _check_poisoned(fields, (4, 7), "dropout-unbiased p = 0 (client 4), overflowing 1/p (client 7)")


@pytest.mark.parametrize("where,what", [(3 * CH + 77, np.inf), (N - 2, np.nan), (0, -np.inf)])
def test_a_non_finite_v_makes_every_output_nan(where, what):
    """One inf in the middle of v; one NaN in the last, partial quarter (the image's tail)."""
    pk = packets_of("exact", exact_fields())[:9]
    v = half_vector().copy()
    v[where] = np.float32(what)
    assert where < N and (where != N - 2 or where >= 6 * CH + QU)
    got = gpu_dot(pk, v)
    assert got.shape == (10,) and np.all(np.isnan(got))
    v[where] = np.float32(1.0)                                   # and nothing sticks
    assert np.all(np.isfinite(gpu_dot(pk, v)))


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
    rows = [(np.nonzero(r)[0], r[np.nonzero(r)[0]].astype(np.float64), True) for r in dense]
    v = rng.standard_normal(N_R).astype(np.float32)
    for vec in (v, None):
        want, c, absum = oracle_dot(rows, vec, n=N_R)
        assert_within_bound(gpu_dot(pk, vec), want, c, absum, "encode_top_batch packets, M=5")


def test_dot_dense_rejects_what_it_cannot_take():
    codec = _codec()
    pk = packets_of("exact", exact_fields())
    with pytest.raises(ValueError, match="at most 128"):
        codec.dot_dense(pk + pk[:1])
    other = to_packet(po.build_idxval(N_R, np.array([1, 9]), np.float32([1, 2]), thresh=0,
                                      codec=po.CODEC_TOP, k=2))
    with pytest.raises(ValueError, match="share n"):
        codec.dot_dense([pk[0], other])
    g = torch.ones(N_R, dtype=torch.float32, device="cuda")
    bitmap = codec.encode_mask(g, 3, p=0.5, fmt=1)
    with pytest.raises(ValueError, match="idx/val"):
        codec.dot_dense([bitmap])
    with pytest.raises(ValueError, match="no packets"):
        codec.dot_dense([])
    with pytest.raises(ValueError, match="v must be"):
        codec.dot_dense(pk[:2], torch.ones(N, dtype=torch.float64, device="cuda"))
    with pytest.raises(ValueError, match="v must be"):
        codec.dot_dense(pk[:2], torch.ones(N - 1, dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError, match="v must be"):
        codec.dot_dense(pk[:2], torch.ones(N, dtype=torch.float32))


# ---- long vectors: several chunks per workgroup, several parts per lane -----------------------
LONG_NS = [129 * CH + QU + 3, 1024 * CH, 1024 * CH + 5]         # 130, 1024 and 1025 chunks
LONG_COUNTS = (0, 1, 65, 257, 3)


def long_geometry(n, m):
    """(chunks per slice, slices) as dot_geom sets them: restated here so that a test says which
    side of a switch point it stands on, and fails if the kernel's geometry moves away."""
    nch, tiles = po.num_chunks(n), (m + 63) // 64
    cap = min(nch, 1024 // tiles)
    cps = (nch + cap - 1) // cap
    return cps, (nch + cps - 1) // cps


def long_support(n, j):
    """Chunk c holds LONG_COUNTS[(c + j) % 5] entries, spread over its four quarters (stride 29
    from an offset that moves with the chunk); a partial last chunk holds its first elements."""
    out = []
    for c in range(po.num_chunks(n)):
        cap = min(CH, n - c * CH)
        cnt = min(LONG_COUNTS[(c + j) % 5], cap)
        if cap == CH:
            loc = np.sort((c * 131 + j * 517 + np.arange(cnt, dtype=np.int64) * 29) % CH)
        else:
            loc = np.arange(cnt, dtype=np.int64)
        out.append(c * CH + loc)
    return np.concatenate(out)


def late_chunk(n):
    """The last chunk = 5 mod 6: the second chunk of its slice for cps = 2, the third for cps = 3."""
    return 6 * ((po.num_chunks(n) - 1) // 6) - 1


def long_case(n):
    """Three clean clients A, B, C with small-integer values, D = B's entries with +inf in chunk 5,
    E = C's entries with NaN in late_chunk(n); v of multiples of 0.5; the two oracles (once per n)."""
    def make():
        sup = [long_support(n, j) for j in range(3)]
        val = [int_values(np.random.default_rng([j, 61]), s.size) for j, s in enumerate(sup)]
        for j, c, what in ((1, 5, np.inf), (2, late_chunk(n), np.nan)):
            at = np.nonzero(sup[j] // CH == c)[0]
            assert at.size, "the poisoned chunk lists something"
            bad = val[j].copy()
            bad[at[-1]] = np.float32(what)
            sup.append(sup[j])
            val.append(bad)
        chunks = set(np.concatenate(sup[:3]) // CH)
        assert {0, 1, 2, 3, 4, 5}.issubset(chunks) and sup[0].size > 50 * po.num_chunks(n)
        fields = [po.build_idxval(n, s, x, thresh=0, codec=po.CODEC_TOP, k=s.size)
                  for s, x in zip(sup, val)]
        v = (np.random.default_rng([n, 67]).integers(-8, 9, size=n) * 0.5).astype(np.float32)
        v[v == 0] = NEG0
        rows = sparse_rows(fields)
        return fields, v, oracle_dot(rows, v, n=n)[0], oracle_dot(rows, None, n=n)[0]
    return memo(("long", n), make)


def long_clients(n, which):
    """Device packets and the two oracles for the clients named by which (indices into A..E)."""
    fields, v, want_v, want_1 = long_case(n)
    pk = packets_of(("long", n), fields)
    sel = np.asarray(which + [5])
    return [pk[j] for j in which], v, want_v[sel], want_1[sel]


@pytest.mark.parametrize("M", [2, 65])
@pytest.mark.parametrize("n", LONG_NS)
def test_long_vectors_exact_across_chunks_and_parts(n, M):
    """Exact sums (bit-equal to fsum) where a workgroup carries a client's sum over several chunks
    and a lane of the finishing kernel adds several parts.  Clients cycle through A, B, C."""
    cps, slices = long_geometry(n, M)
    nch = po.num_chunks(n)
    assert slices > 64 and (cps > 1) == (nch > 1024 // ((M + 63) // 64))
    pk, v, want_v, want_1 = long_clients(n, [i % 3 for i in range(M)])
    assert np.all(np.isfinite(want_v)) and np.all(np.abs(want_v) < 2.0 ** 40)
    assert_same(gpu_dot(pk, v), want_v, f"n={n} M={M} cps={cps} slices={slices}")
    got = gpu_dot(pk, None)
    assert got[M] == float(n)
    assert_same(got, want_1, f"v = None, n={n} M={M} cps={cps} slices={slices}")


@pytest.mark.parametrize("M", [3, 65])
@pytest.mark.parametrize("n", LONG_NS)
def test_long_vectors_a_late_chunks_non_finite_entry_poisons_its_client_alone(n, M):
    """Client 1 holds +inf in chunk 5 (slice 2 or 1: the first part its lane reads), client M - 1
    holds NaN in late_chunk(n) (the last part its lane reads for cps = 2): neither chunk is the
    first of its slice, and every other client stays exact."""
    cps, _ = long_geometry(n, M)
    assert cps == 1 or (5 % cps != 0 and late_chunk(n) % cps != 0)
    which = [i % 3 for i in range(M)]
    which[1], which[M - 1] = 3, 4
    pk, v, want_v, want_1 = long_clients(n, which)
    for vec, want in ((v, want_v), (None, want_1)):
        got = gpu_dot(pk, vec)
        assert [i for i in range(M + 1) if np.isnan(got[i])] == [1, M - 1]
        assert_same(got, want, f"n={n} M={M} cps={cps}")


def test_long_vectors_rounding_and_a_non_finite_v_in_a_later_chunk():
    """Normal values over 1025 chunks (cps = 2): within the worst case of any order; then one inf
    of v in the second chunk of a slice makes every output NaN."""
    n = LONG_NS[2]
    fields0 = long_case(n)[0]
    rng = np.random.default_rng(71)
    fields = []
    for f in fields0[:2]:
        gidx, _ = po.listed_entries(f)
        fields.append(po.build_idxval(n, gidx, rng.standard_normal(gidx.size).astype(np.float32),
                                      thresh=0, codec=po.CODEC_TOP, k=gidx.size))
    v = rng.standard_normal(n).astype(np.float32)
    pk = [to_packet(f) for f in fields]
    for vec in (v, None):
        want, c, absum = oracle_dot(sparse_rows(fields), vec, n=n)
        assert_within_bound(gpu_dot(pk, vec), want, c, absum, f"normal values, n={n}")
    v[7 * CH + 9] = np.float32(np.inf)
    assert np.all(np.isnan(gpu_dot(pk, v)))
