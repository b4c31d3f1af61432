"""fc_packets_trim (csrc/fc_trim.hip) and its consumers (codec.trimmed_mean, gar.TrimmedMean,
gar.CoordinateMedian, the Aggregator's "gram" route, aggregate_wire) on an MI355X.

Run:  python -m pytest tests/test_trim_gpu.py -m gpu -q

Hand-built packets come from oracle/packet_oracle.py's builders: every slot position a packet
does not list holds the poison pair (index 0xFFFF, value NaN), so a read past a count shows up as
NaN in a column.  The expected aggregate is tests/trim_model.py's on the dense rows
po.decode_packet gives for the same packets.  Every comparison is bit for bit (po.same_bits: the
sign of zero included, NaN positions compare as NaN).

Switch points of the kernel the shapes are built around (csrc/fc_trim.hip, not imported):
  window W = 256 coordinates up to 64 clients, 128 above: M in {64, 65}
  8 waves scatter, client i by wave i % 8: M in {1, 2, 3, 8, 9, 128}
  a window's run of a client is read 64 entries at a time: columns where every client lists, a
    packet that lists every coordinate (a run of W entries: 2 or 4 rounds)
  one workgroup per chunk: n = 5000 (a partial quarter), 8192, 3 * 8192 + 37 (a partial chunk)
"""
import types

import numpy as np
import pytest

import trim_model as tm
from oracle import compression_oracle as co
from oracle import packet_oracle as po

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CH, QU = po.CHUNK, po.QUARTER
F = np.float32
NAN, INF, NEG0 = F(np.nan), F(np.inf), F(-0.0)
NS = (5000, CH, 3 * CH + 37)
N3 = 3 * CH + 37
#: (M, b): the even and odd medians, both windows, the limit, and b = 0 (the plain mean)
MB = [(1, 0), (2, 0), (3, 1), (8, 3), (9, 4), (64, 6), (65, 6), (128, 12), (128, 63), (8, 0), (128, 0)]
#: chunk-local coordinates of the hand-built columns: a window's first and last coordinate for
#: both window sizes, both sides of every quarter boundary and of the chunk boundary
SPOTS = (0, 127, 128, 255, 256, 383, 2047, 2048, 4095, 4096, 4223, 6143, 6144, 8063, 8064, 8191)


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
        _MEMO[key] = make()
    return _MEMO[key]


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


def _explain(got, want, limit=8):
    u = np.uint32
    gn, wn = np.isnan(got), np.isnan(want)
    gu, wu = got.view(u), want.view(u)
    bad = np.nonzero((gn != wn) | (~gn & ~wn & (gu != wu)))[0]
    rows = [f"{bad.size} of {got.size} coordinates differ"]
    rows += [f"  [{j}] chunk {j // CH} local {j % CH}: got {got[j]!r} ({int(gu[j]):#x}) "
             f"want {want[j]!r} ({int(wu[j]):#x})" for j in bad[:limit]]
    return "\n".join(rows)


def assert_same(got, want, what=""):
    if isinstance(got, torch.Tensor):
        got = got.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == want.shape, what
    assert po.same_bits(got, want), f"{what}\n{_explain(got, want)}"


def check(fields, b, what=""):
    """One launch on the packets of the builder dicts against the model on their dense rows."""
    G = np.stack([po.decode_packet(f, np.float32) for f in fields])
    want = tm.trimmed_mean_model(G, b)
    got = _codec().trimmed_mean([to_packet(f) for f in fields], b)
    torch.cuda.synchronize()
    assert_same(got, want, what)
    return got.cpu().numpy(), want, G


# ---- packets from a matrix of listed cells ------------------------------------------------------
def fields_of_cells(V, Lm):
    """One thresh == 0 packet per row: the cells Lm marks are listed with V's value (a listed
    +-0.0 is a kept zero), every other cell is not listed."""
    n = V.shape[1]
    out = []
    for v, l in zip(V, Lm):
        idx = np.nonzero(l)[0]
        out.append(po.build_idxval(n, idx, v[idx], thresh=0, codec=po.CODEC_TOP, k=idx.size))
    return out


def background(M, n, frac, seed):
    rng = np.random.default_rng(seed)
    V = rng.standard_normal((M, n)).astype(F)
    return V, rng.random((M, n)) < frac


def column_kinds(M, b):
    """The hand-built columns for (M, b): name -> (values, listed) of length M, or None when
    (M, b) leaves no room for the column."""
    rng = np.random.default_rng([M, b, 5])
    order = rng.permutation(M)                         # which clients hold the chosen values

    def col(vals):
        """vals on the first clients of ``order``; the other clients list nothing."""
        vals = np.asarray(vals, dtype=F)
        if vals.size > M:
            return None
        v, l = np.zeros(M, F), np.zeros(M, bool)
        v[order[:vals.size]] = vals
        l[order[:vals.size]] = True
        return v, l

    def rnd(c):
        return (rng.standard_normal(max(c, 0)) + F(0.25)).astype(F)

    def signed(c, sign):
        return None if c < 0 else col(sign * (np.abs(rnd(c)) + F(0.5)))

    kinds = {
        "no entry": col([]),
        "every client non-zero": col(rnd(M)),
        "b positives": signed(b, 1), "b-1 positives": signed(b - 1, 1), "b+1 positives": signed(b + 1, 1),
        "b negatives": signed(b, -1), "b-1 negatives": signed(b - 1, -1), "b+1 negatives": signed(b + 1, -1),
        "all equal": col(np.full(M, 1.5)),
        "all equal negative, some": col(np.full((M + 1) // 2, -2.5)),
        "ties across the trim": col(np.concatenate([np.full(b + 1, -1.0), np.full(b + 1, 3.0)])),
        "kept -0.0 only": col(np.full((M + 1) // 2, NEG0)),
        "kept -0.0 in every client": col(np.full(M, NEG0)),
        "kept zeros of both signs": col(np.where(np.arange(M) % 2 == 0, NEG0, F(0.0))),
        "one NaN": col(np.concatenate([[NAN], rnd(min(M - 1, 3))])) if b >= 1 else None,
        "b NaN": col(np.concatenate([np.full(b, NAN), rnd(min(M - b, 2))])),
        "b+1 NaN": col(np.concatenate([np.full(b + 1, NAN), rnd(min(M - b - 1, 2))])),
        "all NaN": col(np.full(M, NAN)),
        "inf and -inf trimmed": col(np.concatenate([[INF, -INF], rnd(min(M - 2, 3))])) if b >= 1 else None,
        "inf and -inf survive": col(np.concatenate([np.full(b + 1, INF), np.full(b + 1, -INF)])),
        "inf survives": col(np.concatenate([np.full(b + 1, INF), rnd(min(M - b - 1, 2))])),
        "-inf, inf and NaN": col(np.concatenate([[NAN, INF, -INF], rnd(min(M - 3, 2))])),
        "denormals": col((np.array([1, -1, 3, 2, -7, 1, 1, 5, -2, 4][:min(M, 10)]) * 1.4e-45).astype(F)),
        "denormals and a zero": col(np.array([1e-45, -0.0, 1e-42, -3e-45][:min(M, 4)], dtype=F)),
    }
    return {k: v for k, v in kinds.items() if v is not None}


def place_columns(V, Lm, b, shift):
    """Write the hand-built columns over the background at SPOTS of every chunk: kind number
    (j + shift + chunk) at spot j.  Returns {coordinate: kind name}."""
    M, n = V.shape
    kinds = column_kinds(M, b)
    names = sorted(kinds)
    placed = {}
    for c in range(po.num_chunks(n)):
        for j, s in enumerate(SPOTS):
            t = c * CH + s
            if t >= n:
                continue
            name = names[(j + shift + c) % len(names)]
            V[:, t], Lm[:, t] = kinds[name]
            placed[t] = name
    for t in (n - 1, n - 2):                           # the last coordinates of a partial chunk
        if t >= 0 and t not in placed:
            name = names[(t + shift) % len(names)]
            V[:, t], Lm[:, t] = kinds[name]
            placed[t] = name
    return placed


def expect_by_kind(name, got, M, b):
    """What the issue pins for a kind of column, beside the model's bits."""
    g = got
    if name in ("no entry", "kept -0.0 only", "kept -0.0 in every client", "kept zeros of both signs"):
        assert g.view(np.uint32) == 0, (name, g)                 # +0.0, never -0.0
    if name == "all equal":
        assert g == F(1.5), (name, g)                            # 1.5 * count is exact
    if name in ("one NaN", "b NaN", "inf and -inf trimmed"):
        assert np.isfinite(g), (name, g)
    if name in ("b+1 NaN", "all NaN", "inf and -inf survive"):
        assert np.isnan(g), (name, g)
    if name == "inf survives":
        assert g == INF, (name, g)


@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("M,b", MB)
def test_shapes_against_the_model(M, b, n):
    V, Lm = background(M, n, 0.1, seed=[M, b, n])
    placed = place_columns(V, Lm, b, shift=0)
    got, want, G = check(fields_of_cells(V, Lm), b, f"M={M} b={b} n={n}")
    for t, name in placed.items():
        expect_by_kind(name, got[t], M, b)
    if b == 0:                                         # the plain mean, rows in ascending order
        acc = np.zeros(n, F)
        with np.errstate(invalid="ignore"):
            for row in np.sort(G, axis=0):
                acc = acc + row
            assert po.same_bits(got, acc / F(M))


@pytest.mark.parametrize("M,b", [(8, 3), (9, 4), (9, 1), (64, 6), (65, 6), (128, 12), (128, 63)])
def test_every_hand_built_column_at_every_spot(M, b):
    """Each launch holds every SPOT of three whole chunks, one kind further on in each; the
    shifts, three apart, move every kind of column over every spot."""
    kinds = column_kinds(M, b)
    seen = set()
    for shift in range(0, len(kinds), 3):
        V, Lm = background(M, N3, 0.1, seed=[M, b, shift])
        placed = place_columns(V, Lm, b, shift)
        got, _, _ = check(fields_of_cells(V, Lm), b, f"M={M} b={b} shift={shift}")
        for t, name in placed.items():
            expect_by_kind(name, got[t], M, b)
            if t % CH in SPOTS and t // CH < 3:
                seen.add((name, t % CH))
    missing = [(k, s) for k in kinds for s in SPOTS if (k, s) not in seen]
    assert not missing, missing[:5]


def test_dense_columns_and_half_full_background():
    """f = 0.5 and f = 1.0 backgrounds: runs longer than one 64-entry round in every window."""
    for M, b, frac in ((16, 3, 0.5), (128, 12, 0.5), (5, 1, 1.0), (65, 32, 1.0), (128, 63, 1.0)):
        V, Lm = background(M, CH + 300, frac, seed=[M, b, 77])
        check(fields_of_cells(V, Lm), b, f"M={M} b={b} f={frac}")


# ---- hand-built packets ---------------------------------------------------------------------------
def slack_packet(n, k, extra, seed):
    """A top-k packet as the sampled encoder leaves it: k kept entries and ``extra`` listed
    ones below T64 that must not count."""
    g = np.random.default_rng(seed).standard_normal(n).astype(F)
    keys = po.mag_key(g)
    T, Lo = po.threshold(keys, k), po.threshold(keys, k + extra)
    idx = np.nonzero(po.comps(keys) >= Lo)[0]
    f = po.build_idxval(n, idx, g[idx], thresh=int(T), lower=int(Lo), codec=po.CODEC_TOP, k=k)
    assert po.kept_entries(f)[0].size == k and idx.size == k + extra
    return f


def philox_packet(n, k, extra, seed):
    """A native rand-k packet: kept by the element's Philox key, not by the value."""
    g = np.random.default_rng(seed).standard_normal(n).astype(F)
    pseed, offset = 0xC0FFEE_0000_0042 + seed, 9
    keys = po.philox_keys_at(np.arange(n), pseed, offset)
    T, Lo = po.threshold(keys, k), po.threshold(keys, k + extra)
    idx = np.nonzero(po.comps(keys) >= Lo)[0]
    f = po.build_idxval(n, idx, g[idx], thresh=int(T), lower=int(Lo), codec=po.CODEC_RAND,
                        key_mode=po.KEY_PHILOX, k=k, seed=pseed, offset=offset)
    assert po.kept_entries(f)[0].size == k and idx.size == k + extra
    return f


def special_packets(n=N3):
    def make():
        rng = np.random.default_rng(31)

        def sparse(frac, drop=None):
            l = rng.random(n) < frac
            if drop is not None:
                l[drop] = False
            idx = np.nonzero(l)[0]
            return idx, rng.standard_normal(idx.size).astype(F)

        out = {}
        idx, val = sparse(0.1, slice(CH + 2 * QU, CH + 3 * QU))
        out["empty quarter"] = po.build_idxval(n, idx, val, thresh=0, codec=po.CODEC_TOP, k=idx.size)
        idx, val = sparse(0.1, slice(CH, 2 * CH))
        out["empty chunk"] = po.build_idxval(n, idx, val, thresh=0, codec=po.CODEC_TOP, k=idx.size)
        val = rng.standard_normal(n).astype(F)
        val[::9], val[4::11] = F(0.0), NEG0                       # listed zeros of both signs
        out["every coordinate"] = po.build_idxval(n, np.arange(n), val, thresh=0, codec=po.CODEC_TOP, k=n)
        out["slack"] = slack_packet(n, n // 10, n // 20, seed=41)
        idx, val = sparse(0.3)
        out["unbiased p=0.3"] = po.build_idxval(n, idx, val, thresh=0, codec=po.CODEC_DROPOUT_UNBIASED,
                                                p=0.3, seed=4)
        out["philox"] = philox_packet(n, n // 10, n // 25, seed=43)
        return out
    return memo(("special", n), make)


@pytest.mark.parametrize("M,b", [(6, 0), (6, 1), (6, 2), (9, 4), (70, 7)])
def test_hand_built_packets(M, b):
    """The six special packets among sparse ones (M > 6), in an order that changes with M."""
    sp = special_packets()
    V, Lm = background(max(M - len(sp), 1), N3, 0.1, seed=[M, 51])
    fields = list(sp.values()) + fields_of_cells(V, Lm)[:M - len(sp)]
    fields = [fields[i] for i in np.random.default_rng(M).permutation(len(fields))][:M]
    assert len(fields) == M
    _, _, G = check(fields, b, f"M={M} b={b}")
    # the specials do what their names say in the rows the model was given
    rows = {k: po.decode_packet(f, np.float32) for k, f in sp.items()}
    assert not rows["empty quarter"][CH + 2 * QU:CH + 3 * QU].any()
    assert not rows["empty chunk"][CH:2 * CH].any()
    assert np.count_nonzero(rows["slack"]) == N3 // 10
    assert np.count_nonzero(rows["philox"]) == N3 // 10
    f = sp["unbiased p=0.3"]
    gidx, val = po.listed_entries(f)
    assert np.array_equal(rows["unbiased p=0.3"][gidx], (val.astype(np.float64) / 0.3).astype(F))


def test_each_special_packet_alone_is_its_decoded_row():
    """M = 1, b = 0: the aggregate is fl32((+0.0 + d[t]) / 1) — the row, with -0.0 made +0.0."""
    for name, f in special_packets().items():
        got, _, G = check([f], 0, name)
        assert po.same_bits(got, G[0] + F(0.0)), name


# ---- whole path and API -----------------------------------------------------------------------------
def real_packets(frac, M=16, n=N3):
    codec = _codec()
    rng = np.random.default_rng([int(frac * 100), M])
    grads = [torch.from_numpy(rng.standard_normal(n).astype(F)).cuda() for _ in range(M)]
    pk = codec.encode_top_batch(grads, round(frac * n))
    codec.resolve(pk)
    return pk


@pytest.mark.parametrize("frac", [0.1, 0.5])
def test_real_packets_against_the_model_on_decoded_rows(frac):
    codec = _codec()
    pk = real_packets(frac)
    G = np.stack([codec.decode(p).cpu().numpy() for p in pk])
    assert all(np.count_nonzero(r) == round(frac * N3) for r in G)
    for b in (1, tm.median_trim(len(pk)), 0):
        assert_same(codec.trimmed_mean(pk, b), tm.trimmed_mean_model(G, b), f"f={frac} b={b}")


def test_determinism_client_order_and_out():
    codec = _codec()
    pk = real_packets(0.1)
    n = pk[0].n
    a = codec.trimmed_mean(pk, 2).cpu().numpy()
    assert codec.trimmed_mean(pk, 2).cpu().numpy().tobytes() == a.tobytes()
    assert codec.trimmed_mean(pk[::-1], 2).cpu().numpy().tobytes() == a.tobytes()
    out = torch.full((n,), 7.0, dtype=torch.float32, device="cuda")
    r = codec.trimmed_mean(pk, 2, out=out)
    assert r is out and out.cpu().numpy().tobytes() == a.tobytes()
    sp = special_packets()
    fields = list(sp.values())
    one = codec.trimmed_mean([to_packet(f) for f in fields], 2).cpu().numpy()
    two = codec.trimmed_mean([to_packet(f) for f in fields[::-1]], 2).cpu().numpy()
    assert po.same_bits(one, two)


def test_codec_value_errors():
    codec = _codec()
    pk = real_packets(0.1)
    for bad in (8, 9, -1, 1.0, None):
        with pytest.raises(ValueError, match="trim"):
            codec.trimmed_mean(pk, bad)
    with pytest.raises(ValueError, match="at most 128"):
        codec.trimmed_mean([pk[0]] * 129, 0)
    with pytest.raises(ValueError, match="no packets"):
        codec.trimmed_mean([], 0)
    n = pk[0].n
    for out in (torch.empty(n, dtype=torch.float64, device="cuda"),
                torch.empty(n + 1, dtype=torch.float32, device="cuda"),
                torch.empty(n + 4, dtype=torch.float32, device="cuda")[1:n + 1],
                torch.empty(n, dtype=torch.float32)):
        with pytest.raises(ValueError, match="out must be"):
            codec.trimmed_mean(pk, 1, out=out)
    other = codec.encode_top_batch([torch.randn(CH, device="cuda")], 10)
    with pytest.raises(ValueError, match="share n"):
        codec.trimmed_mean([pk[0], other[0]], 0)
    f = po.build_idxval(N3, np.arange(5), np.ones(5, F), thresh=0, codec=po.CODEC_TOP, with_qoff=False)
    p = codec.Packet(n=N3, fmt=f["fmt"], k=5, val=_dev(f["val"], np.float32), cnt=_dev(f["cnt"], np.int32),
                     hdr=_dev(np.frombuffer(f["hdr"].tobytes(), dtype=np.uint8), np.uint8),
                     idx=_dev(f["idx"], np.int16), qoff=None)
    with pytest.raises(ValueError, match="quarter offsets"):
        codec.trimmed_mean([p], 0)


N_A, M_A, FRAC_A = 20000, 8, 0.1
TOP_CFG = {"compression_function": "top", "fraction_coordinate": FRAC_A}
SCHEMES = {"trimmed_mean": ({"aggregation_scheme": "trimmed_mean", "trim_count": 2}, 2),
           "trimmed_mean_frac": ({"aggregation_scheme": "trimmed_mean", "trim_frac": 0.25}, 2),
           "coordinate_median": ({"aggregation_scheme": "coordinate_median"}, 3)}


def round_clients():
    """8 clients x 20 000: six near a common base, one scaled noise, one sign-flipped."""
    from openmsftl_amd import Compression

    def make():
        rng = np.random.default_rng(20261020)
        base = rng.standard_normal(N_A)
        grads = []
        for i in range(M_A):
            noise = rng.standard_normal(N_A)
            g = 5.0 * noise if i == 2 else -3.0 * base if i == 6 else base + 0.3 * noise
            grads.append(g.astype(F))
        rows = np.stack([co.compress(TOP_CFG, g) for g in grads])   # the oracle's 'top' rows
        return grads, rows
    grads, rows = memo("round", make)
    clients = [types.SimpleNamespace(C=Compression(dict(TOP_CFG)), grad=g, client_id=i)
               for i, g in enumerate(grads)]
    return clients, rows


@pytest.mark.parametrize("scheme", sorted(SCHEMES))
def test_aggregator_round_and_wire(scheme):
    from openmsftl_amd.aggregation import Aggregator
    cfg, b = SCHEMES[scheme]
    clients, rows = round_clients()
    want = tm.trimmed_mean_model(rows, b)
    agg = Aggregator(dict(cfg))
    agg.aggregate_grads(clients)
    assert agg.agg_path == "gram" and agg.curr_G is None and agg.gar.trim == b
    assert agg.gar.Sigma_tracked == []
    assert_same(agg.agg_grad, want, scheme)
    # pc_analysis "gram": one entry of singular values, the aggregate unchanged
    pc = Aggregator(dict(cfg, pc_analysis="gram"))
    pc.aggregate_grads(clients)
    assert pc.agg_path == "gram" and len(pc.gar.Sigma_tracked) == 1
    S = pc.gar.Sigma_tracked[0]
    assert S.shape == (M_A,) and np.all(np.isfinite(S)) and np.all(np.diff(S) <= 0)
    assert pc.agg_grad.tobytes() == agg.agg_grad.tobytes()
    # the same clients' wire payloads; "wire_fold" leaves the scheme untouched
    payloads = [c.C.compress_wire(c.grad) for c in round_clients()[0]]
    for extra in ({}, {"wire_fold": True}):
        w = Aggregator(dict(cfg, **extra))
        w.aggregate_wire(payloads)
        assert w.agg_path == "wire" and w.gar.trim == b
        assert w.agg_grad.tobytes() == agg.agg_grad.tobytes()
    weighted = Aggregator(dict(cfg))
    weighted.gar.gradient_weights = np.full(M_A, 1.0 / M_A, F)
    with pytest.raises(ValueError, match="gradient_weights"):
        weighted.aggregate_grads(clients)
