"""The packet consumers (k_decode_sparse, k_decode, k_fold_q, k_ef_clear of csrc/fc_decode.hip
and csrc/fc_ef.hip) on HAND-BUILT packets, against the CPU consumer of oracle/packet_oracle.py.

Run on an MI355X:  python -m pytest tests/test_packet_consumers_gpu.py -m gpu -q

Every packet here is well-formed (ascending distinct indices, counts <= 8192, consistent
quarter offsets); every slot position a packet does not list holds a poison pair (index 0xFFFF,
value NaN), so a consumer that reads past a count shows up in the output.  Results are compared
bit for bit, the sign of zero included; NaN positions compare as NaN.

Switch points of k_fold_q the count band is built around (names of csrc/fc_decode.hip, not
imported: the band {0..2048} below stays valid if they are retuned):
  kQR * 64 = 256      entries per (packet, quarter) the fast body's register rounds hold
  kQTail * 64 = 512   above it the wave that owns the quarter takes the slow body (dense_q)
  kQGroup = 3         items per load group, two groups in flight
  kSparseMaxM = 128   idx/val packets per launch (lanes 0..63 -> qo0, 64..127 -> qo1)
  kDecMaxM = 64       bitmap packets per launch
  kSR * kSBlock = kDecR * kDBlock = 1024   slot entries per chunk before the dense-slot loops
  4096 chunks         fc_decode_dense: k_fold_q<false, true> at and above, k_decode_sparse below
"""
import ctypes

import numpy as np
import pytest

from oracle import packet_oracle as po
from oracle import philox as ph

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CH, QU = po.CHUNK, po.QUARTER
NEG0 = np.float32(-0.0)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from openmsftl_amd import _lib
    assert _lib.load().fc_abi_version() == 4
    yield
    _DEV.clear()
    _E_BUF.clear()
    torch.cuda.empty_cache()


def _codec():
    from openmsftl_amd import codec
    return codec


def _L():
    from openmsftl_amd import _lib
    return _lib


# ---- builder output <-> codec.Packet ----------------------------------------------------
def _dev(a, dt):
    return torch.from_numpy(np.ascontiguousarray(a).view(dt).copy()).cuda()


def to_packet(f):
    """A codec.Packet over device copies of the builder's arrays."""
    return _codec().Packet(
        n=f["n"], fmt=f["fmt"], k=int(f["hdr"]["k"]),
        val=_dev(f["val"], np.float32), cnt=_dev(f["cnt"], np.int32),
        hdr=_dev(np.frombuffer(f["hdr"].tobytes(), dtype=np.uint8), np.uint8),
        idx=_dev(f["idx"], np.int16) if f["idx"] is not None else None,
        bitmap=_dev(f["bitmap"], np.int32) if f["bitmap"] is not None else None,
        qoff=_dev(f["qoff"], np.int64) if f["qoff"] is not None else None)


def fields_of(pkt):
    """The builder's dict over host copies of a GPU packet's arrays."""
    host = lambda t, dt: None if t is None else t.cpu().numpy().view(dt)     # noqa: E731
    return {"n": pkt.n, "fmt": pkt.fmt, "idx": host(pkt.idx, np.uint16),
            "val": host(pkt.val, np.float32), "cnt": host(pkt.cnt, np.uint32),
            "qoff": host(pkt.qoff, np.uint64), "bitmap": host(pkt.bitmap, np.uint32),
            "hdr": np.frombuffer(pkt.hdr.cpu().numpy().tobytes(), dtype=po.HDR_DTYPE)[0]}


_DEV = {}


def cached_packet(key, f):
    if key not in _DEV:
        _DEV[key] = to_packet(f)
    return _DEV[key]


def _explain(got, want, limit=8):
    if got.dtype != want.dtype or got.shape != want.shape:
        return f"{got.dtype}{got.shape} against {want.dtype}{want.shape}"
    u = np.dtype(f"<u{got.dtype.itemsize}")
    gn, wn = np.isnan(got), np.isnan(want)
    gu, wu = got.view(u), want.view(u)
    bad = np.nonzero((gn != wn) | (~gn & ~wn & (gu != wu)))[0]
    rows = [f"{bad.size} of {got.size} elements differ"]
    rows += [f"  [{j}] chunk {j // CH} quarter {j % CH // QU}: got {got[j]!r} ({int(gu[j]):#x}) "
             f"want {want[j]!r} ({int(wu[j]):#x})" for j in bad[:limit]]
    return "\n".join(rows)


def assert_same(got, want, what=""):
    if isinstance(got, torch.Tensor):
        got = got.cpu().numpy()
    assert po.same_bits(got, want), f"{what}\n{_explain(got, want)}"


# ---- GPU consumers --------------------------------------------------------------------------
def gpu_decode(pkt, dtype=np.float32):
    t = torch.float64 if np.dtype(dtype) == np.float64 else torch.float32
    return _codec().decode(pkt, dtype=t).cpu().numpy()


def gpu_fold(pkts, w, acc=None):
    codec = _codec()
    if acc is None:
        return codec.decode_accumulate(pkts, w).cpu().numpy()
    out = torch.from_numpy(np.ascontiguousarray(acc, dtype=np.float32).copy()).cuda()
    return codec.decode_accumulate(pkts, w, out=out, continue_sum=True).cpu().numpy()


def gpu_ef_clear(pkt, sentinel):
    """fc_ef_clear through the binding encode_top_ef's fallback chain uses."""
    L = _L()
    res = torch.full((pkt.n,), float(sentinel), dtype=torch.float32, device="cuda")
    v = pkt.view()
    s = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
    L.check(L.load().fc_ef_clear(ctypes.byref(v), pkt.n, res.data_ptr(), s), "fc_ef_clear")
    return res.cpu().numpy()


def partial_sum(n, seed=77):
    """A non-trivial sum to continue: normal values, -0.0, +0.0 and denormals of both signs."""
    a = np.random.default_rng(seed).standard_normal(n).astype(np.float32)
    a[::5] = NEG0
    a[1::7] = np.float32(1e-42)
    a[2::11] = np.float32(-3e-45)
    a[3::13] = np.float32(0.0)
    return a


# ---- designed packets ---------------------------------------------------------------------
# n of parts B, C, D: 6 whole chunks and a last one that ends three elements into quarter 1
N_B = 6 * CH + QU + 3
BAND = [0, 1, 2, 63, 64, 65, 127, 128, 129, 191, 192, 193, 255, 256, 257, 258, 319, 320, 321,
        511, 512, 513, 1023, 1024, 1025, 2047, 2048]
# The whole band in an order whose first four put one chunk's quarters in different bodies
# (empty fast item, inline tail, slow wave, fast); chunks 3..6 take 16 consecutive values of
# it starting at the packet's rotation, so the long quarters move with the packet index.
FULL_ORDER = [0, 257, 513, 64, 256, 512, 1023, 1, 258, 2048, 65, 319, 2047, 127, 320, 1024,
              128, 1025, 2, 321, 511, 63, 129, 191, 192, 193, 255]
# Chunks 0..2 only take counts <= 512: whatever the rotations of a launch, their waves stay in
# the fast body (with and without the inline tail), so the item pipeline is met at every M.
SMALL_ORDER = [255, 256, 257, 258, 0, 1, 2, 63, 511, 512, 64, 65, 127, 128, 129, 191, 192, 193,
               319, 320, 321]
assert sorted(FULL_ORDER) == BAND and sorted(SMALL_ORDER) == [b for b in BAND if b <= 512]


def design_counts(rot):
    """Entry counts per (chunk, quarter) of a 7-chunk packet (before clipping to the last
    chunk's real quarter lengths)."""
    rows = np.zeros((7, 4), dtype=np.int64)
    for s in range(12):
        rows[s // 4, s % 4] = SMALL_ORDER[(s + rot) % len(SMALL_ORDER)]
    for s in range(16):
        rows[3 + s // 4, s % 4] = FULL_ORDER[(s + rot) % len(FULL_ORDER)]
    return rows


def design_entries(n, chunks, rows, rng):
    """Ascending global indices: rows[i][q] random positions in quarter q of chunks[i]."""
    out = [np.zeros(0, dtype=np.int64)]
    for c, row in zip(chunks, rows):
        for q in range(4):
            base = c * CH + q * QU
            qlen = max(0, min(QU, n - base))
            m = min(int(row[q]), qlen)
            if m:
                out.append(base + np.sort(rng.choice(qlen, m, replace=False)).astype(np.int64))
    return np.concatenate(out)


def design_values(rng, m, T, slack, big=0.0):
    """m values around the threshold magnitude T: above it, a `slack` share below it, a
    plateau exactly at it, and -0.0 / +0.0 / +-inf / NaN (both signs) sprinkled in."""
    T = np.float64(np.float32(T))
    u = rng.random(m)
    mag = T * (1.0 + 3.0 * rng.random(m))
    sl = u < slack
    mag[sl] = T * (0.25 + 0.7 * rng.random(int(sl.sum())))
    mag[(u >= slack) & (u < slack + 0.15)] = T
    bg = rng.random(m) < big
    mag[bg] = 1.0 + rng.random(int(bg.sum()))
    v = (mag * rng.choice([-1.0, 1.0], m)).astype(np.float32)
    j = np.arange(m)
    v[j % 97 == 11] = NEG0
    v[j % 101 == 13] = np.inf
    v[j % 103 == 17] = -np.inf
    v[j % 107 == 19] = np.nan
    v[j % 109 == 23] = 0.0
    v.view(np.uint32)[j % 113 == 29] = 0xFFC00001          # a negative NaN with a payload
    return v


def _key(x):
    return int(np.float32(x).view(np.uint32)) & 0x7FFFFFFF


# name -> how the header's threshold is made; Ti = the tie index (global)
DESIGNS = {
    "T_slack0_Ti_qbound": dict(T=1.5, slack=0.0, Ti=3 * CH + 2 * QU),       # on a quarter boundary
    "T_slack5_Ti_mid": dict(T=1.5, slack=0.05, Ti=3 * CH + QU + 1000),      # mid-quarter
    "T_slack50_Ti_first": dict(T=1.5, slack=0.5, Ti=5),                     # ties of later chunks stay
    "T_slack5_Ti_last": dict(T=1.5, slack=0.05, Ti=N_B - 1),               # ties of earlier chunks go
    "denormT": dict(T=1e-42, slack=0.05, Ti=3 * CH + 2 * QU + 700, big=0.3),  # denormal Tf and entries
    "thresh0": dict(T=1.5, slack=0.5, thresh=0),                            # everything listed stays
    "infkey": dict(T=1.5, slack=0.05, key=0x7F800000, Ti=3 * CH + 2 * QU),  # the k-th element is inf
    "nankey": dict(T=1.5, slack=0.05, key=0x7F800001, Ti=2 * CH + 7),       # ... or NaN
    "nothing": dict(T=1.5, slack=0.05, thresh=int(po.NOTHING)),             # k = 0
}
FAST = ["T_slack0_Ti_qbound", "T_slack5_Ti_mid", "T_slack50_Ti_first", "T_slack5_Ti_last",
        "denormT", "thresh0"]                                # k_fold_q does not call these generic
_FIELDS = {}


def design(name, rot, with_qoff=True, rows=None):
    """A top-k-headed packet of N_B elements (cached): counts design_counts(rot) or `rows`."""
    key = (name, rot, with_qoff, None if rows is None else rows.tobytes())
    if key in _FIELDS:
        return _FIELDS[key]
    d = DESIGNS[name]
    rng = np.random.default_rng([list(DESIGNS).index(name), rot, 2024])
    gidx = design_entries(N_B, range(7), design_counts(rot) if rows is None else rows, rng)
    val = design_values(rng, gidx.size, d["T"], d["slack"], d.get("big", 0.0))
    ib = po.index_bits(N_B)
    thresh = d["thresh"] if "thresh" in d else (d.get("key", _key(d["T"])) << ib) | d["Ti"]
    f = po.build_idxval(N_B, gidx, val, thresh=thresh, codec=po.CODEC_TOP, with_qoff=with_qoff)
    kept = po.kept_entries(f)[0].size
    f["hdr"]["k"] = kept
    _FIELDS[key] = f
    return f


def ordinary(i):
    """An everyday top-k packet: 150..205 entries in every quarter (fast body, no tail)."""
    rng = np.random.default_rng([i, 99])
    return design("T_slack5_Ti_mid", 1000 + i, rows=rng.integers(150, 206, size=(7, 4)))


def dpkt(name, rot, with_qoff=True):
    return cached_packet((name, rot, with_qoff), design(name, rot, with_qoff))


def test_designs_cover_what_they_claim():
    """The counts and value classes the parts below rely on are really constructed."""
    rows = design_counts(0)
    assert rows[3].tolist() == [0, 257, 513, 64]            # fast / tail / slow / fast
    assert rows[:3].max() <= 512 and rows[:3].max() > 256   # chunks 0..2: fast body + tail
    seen = set()
    for rot in range(27):
        f = design(FAST[rot % len(FAST)], rot)
        per = f["qoff"]
        seen |= set(design_counts(rot).ravel().tolist())
        assert int(f["cnt"][6]) <= QU + 3 and int(per[6] >> np.uint64(48)) == int(f["cnt"][6])
    assert seen == set(BAND)
    for name in ("T_slack0_Ti_qbound", "T_slack5_Ti_mid", "denormT"):
        f = design(name, 0)
        gi, v = po.listed_entries(f)
        ki = po.kept_entries(f)[0]
        T = np.float32(DESIGNS[name]["T"])
        tie = np.abs(v) == T
        kept = np.isin(gi, ki)
        c3 = gi // CH == 3
        assert (tie & kept & c3).any() and (tie & ~kept & c3).any()      # cut inside chunk 3
        assert (tie & (gi // CH < 3)).any() and not kept[tie & (gi // CH < 3)].any()   # earlier chunks
        assert (tie & (gi // CH > 3)).any() and kept[tie & (gi // CH > 3)].all()       # later chunks
        assert np.isnan(v[kept]).any() and np.isinf(v[kept]).any()       # kept under a finite T
        if DESIGNS[name]["slack"]:
            assert ((np.abs(v) < T) & ~kept).any()
    f = design("thresh0", 0)
    assert (po.kept_entries(f)[1].view(np.uint32) == 0x80000000).any()   # -0.0 entries kept
    assert po.kept_entries(design("nothing", 0))[0].size == 0
    gi, v = po.kept_entries(design("infkey", 0))
    assert np.isinf(v).any() and np.isnan(v).any() and not np.isfinite(v).any()
    assert np.isnan(po.kept_entries(design("nankey", 0))[1]).all()


# =============================================================================================
# A. the builder pinned to the real encoders
# =============================================================================================
A_SIZES = [5, 8191, 8193, 20_011, 100_003]
A_CASES = [(n, "gauss") for n in A_SIZES] + [(20_011, "layered"), (100_003, "layered")]


def _grad(n, kind, seed=0):
    g = np.random.default_rng([n, seed]).standard_normal(n).astype(np.float32)
    if kind == "layered":     # 100x per quarter: a chunk's top-k sits in its first quarter
        g *= (10.0 ** (-2.0 * (np.arange(n) % CH // QU))).astype(np.float32)
    return g


def _listed_pos(cnt):
    cnt = cnt.astype(np.int64)
    chunk = np.repeat(np.arange(cnt.size), cnt)
    return chunk * CH + (np.arange(int(cnt.sum())) - (np.cumsum(cnt) - cnt)[chunk])


def pin(pkt, want, what):
    """The GPU packet equals the CPU-built one: counts, quarter offsets, listed slots of idx
    and val (or the whole bitmap) byte for byte, the header field by field."""
    got = fields_of(pkt)
    assert got["cnt"].tobytes() == want["cnt"].tobytes(), f"{what}: cnt"
    pos = _listed_pos(want["cnt"])
    if want["fmt"] == po.FMT_IDXVAL:
        assert got["qoff"].tobytes() == want["qoff"].tobytes(), f"{what}: qoff"
        assert got["idx"][pos].tobytes() == want["idx"][pos].tobytes(), f"{what}: idx"
    else:
        assert got["bitmap"].tobytes() == want["bitmap"].tobytes(), f"{what}: bitmap"
    assert got["val"][pos].tobytes() == want["val"][pos].tobytes(), f"{what}: val"
    for name in po.HDR_DTYPE.names:
        assert np.array_equal(got["hdr"][name], want["hdr"][name]), \
            f"{what}: header field {name}: {got['hdr'][name]} against {want['hdr'][name]}"


def _pin_topk(pkt, g, k, keys, codec, key_mode=0, seed=0, offset=0, exact=False, what=""):
    idx, _, h = pkt.raw_entries()
    n = g.shape[0]
    T = po.threshold(keys, k)
    c = po.comps(keys)
    assert int(h.thresh) == int(T), f"{what}: T64"
    assert int(h.lower) <= int(h.thresh)
    # L64: exactly the elements with comp >= lower are listed
    np.testing.assert_array_equal(idx.astype(np.int64), np.nonzero(c >= np.uint64(h.lower))[0])
    if exact:
        assert int(h.lower) == int(T) and h.n_entries == k
    want = po.build_idxval(n, idx, g[idx], thresh=int(T), lower=int(h.lower), codec=codec,
                           key_mode=key_mode, k=k, seed=seed, offset=offset,
                           n_definite=h.n_definite, n_cand=h.n_cand)
    pin(pkt, want, what)


def _k_of(n):
    return max(1, round(0.1 * n))


@pytest.mark.parametrize("exact", [False, True])
@pytest.mark.parametrize("n,kind", A_CASES)
def test_A_encode_top(n, kind, exact):
    g = _grad(n, kind)
    k = _k_of(n)
    pkt = _codec().encode_top(torch.from_numpy(g).cuda(), k, exact=exact)
    _pin_topk(pkt, g, k, po.mag_key(g), po.CODEC_TOP, exact=exact, what=f"top n={n} {kind}")


@pytest.mark.parametrize("n,kind", A_CASES)
def test_A_encode_top_batch(n, kind):
    gs = [_grad(n, kind, seed=s) for s in range(3)]
    k = _k_of(n)
    pkts = _codec().encode_top_batch([torch.from_numpy(g).cuda() for g in gs], k)
    for i, (g, p) in enumerate(zip(gs, pkts)):
        _pin_topk(p, g, k, po.mag_key(g), po.CODEC_TOP, what=f"batch[{i}] n={n} {kind}")


@pytest.mark.parametrize("n", A_SIZES)
def test_A_encode_top_philox(n):
    g = _grad(n, "gauss")
    k = _k_of(n)
    seed, offset = 0x1234_5678_9ABC, 7
    pkt = _codec().encode_top(torch.from_numpy(g).cuda(), k, key_mode=po.KEY_PHILOX, seed=seed,
                              offset=offset)
    keys = (ph.element_words(n, seed, offset) >> np.uint32(1)).astype(np.uint32)
    _pin_topk(pkt, g, k, keys, po.CODEC_RAND, po.KEY_PHILOX, seed, offset, what=f"philox n={n}")


def _mask_words(mask):
    n = mask.shape[0]
    bits = np.zeros((n + 31) // 32 * 32, dtype=np.uint8)
    bits[:n] = mask
    return torch.from_numpy(np.packbits(bits, bitorder="little").view(np.int32).copy()).cuda()


MASK_KINDS = ["rand_host", "dropout_biased", "dropout_unbiased"]


def _mask_case(n, kind):
    """(codec, p, seed, offset, host mask or None, the kept elements)."""
    if kind == "rand_host":
        mask = np.zeros(n, dtype=bool)
        mask[np.random.default_rng(n).permutation(n)[: _k_of(n)]] = True
        return po.CODEC_RAND, 0.5, 0, 0, mask, mask
    codec = po.CODEC_DROPOUT_BIASED if kind == "dropout_biased" else po.CODEC_DROPOUT_UNBIASED
    seed, offset = (99, 0) if kind == "dropout_biased" else (0xFEED_0000_0001, 3)
    return codec, 0.3, seed, offset, None, ph.bernoulli_mask(n, 0.3, seed, offset)


@pytest.mark.parametrize("fmt", [po.FMT_IDXVAL, po.FMT_BITMAP])
@pytest.mark.parametrize("kind", MASK_KINDS)
@pytest.mark.parametrize("n,gk", A_CASES)
def test_A_encode_mask(n, gk, kind, fmt):
    g = _grad(n, gk)
    codec, p, seed, offset, host, keep = _mask_case(n, kind)
    pkt = _codec().encode_mask(torch.from_numpy(g).cuda(), codec, p=p, seed=seed, offset=offset,
                               mask_bits=_mask_words(host) if host is not None else None, fmt=fmt)
    idx = pkt.raw_entries()[0].astype(np.int64)
    np.testing.assert_array_equal(idx, np.nonzero(keep)[0])       # the mask, independently
    if fmt == po.FMT_IDXVAL:
        want = po.build_idxval(n, idx, g[idx], thresh=0, codec=codec, p=p, seed=seed, offset=offset)
    else:
        want = po.build_bitmap(n, idx, g[idx], codec=codec, p=p, seed=seed, offset=offset)
    pin(pkt, want, f"mask {kind} fmt={fmt} n={n} {gk}")
    assert_same(gpu_decode(pkt), po.decode_packet(want), "decode of the encoder's packet")


# =============================================================================================
# B. the quarter-count matrix through every idx/val consumer
# =============================================================================================
@pytest.mark.parametrize("rot", [0, 9])
@pytest.mark.parametrize("name", list(DESIGNS))
def test_B_decode(name, rot):
    """k_decode_sparse<false> (float32) and k_decode<IDXVAL, false, true> (float64): chunk
    totals above 1024 run their dense-slot loops."""
    f = design(name, rot)
    assert int(f["cnt"].max()) > 1024
    p = dpkt(name, rot)
    assert_same(gpu_decode(p, np.float32), po.decode_packet(f, np.float32), f"{name} f32")
    assert_same(gpu_decode(p, np.float64), po.decode_packet(f, np.float64), f"{name} f64")


@pytest.mark.parametrize("rot", [0, 9])
@pytest.mark.parametrize("name", list(DESIGNS))
def test_B_fold_one_packet(name, rot):
    """k_fold_q<false> / <true>, M = 1: rot 0 puts the fast body, the inline tail and a slow
    wave side by side in chunk 3; the generic headers send whole workgroups to the slow body."""
    f, p = design(name, rot), dpkt(name, rot)
    for w in (1.0, -1.75):
        assert_same(gpu_fold([p], [w]), po.fold_packets([f], [w]), f"{name} w={w}")
        acc = partial_sum(N_B)
        assert_same(gpu_fold([p], [w], acc), po.fold_packets([f], [w], acc), f"{name} w={w} continue")


@pytest.mark.parametrize("rot", [0, 9])
@pytest.mark.parametrize("name", list(DESIGNS))
def test_B_ef_clear(name, rot):
    """k_ef_clear: +0 exactly at the kept entries, the sentinel untouched elsewhere."""
    f, p = design(name, rot), dpkt(name, rot)
    want = np.full(N_B, np.float32(7.5))
    want[po.kept_entries(f)[0]] = 0.0
    assert_same(gpu_ef_clear(p, 7.5), want, name)


def test_B_long_quarter_in_one_packet_of_many():
    """Nine everyday packets (every quarter 150..205 entries) and one designed packet: each
    long quarter of the launch is long in exactly that one packet."""
    for pos in (0, 4, 9):
        fs = [ordinary(i) for i in range(9)]
        ps = [cached_packet(("ordinary", i), f) for i, f in enumerate(fs)]
        fs.insert(pos, design("T_slack5_Ti_mid", 0))
        ps.insert(pos, dpkt("T_slack5_Ti_mid", 0))
        w = np.random.default_rng(pos).standard_normal(10).astype(np.float32)
        assert_same(gpu_fold(ps, w), po.fold_packets(fs, w), f"designed at {pos}")
        acc = partial_sum(N_B)
        assert_same(gpu_fold(ps, w, acc), po.fold_packets(fs, w, acc), f"designed at {pos}, continue")


def test_B_every_design_in_one_launch():
    """All headers side by side: without the generic ones (fast-body workgroups) and with."""
    for names in (FAST, list(DESIGNS)):
        fs = [design(nm, 2 * i) for i, nm in enumerate(names)]
        ps = [dpkt(nm, 2 * i) for i, nm in enumerate(names)]
        w = np.random.default_rng(len(names)).standard_normal(len(names)).astype(np.float32)
        assert_same(gpu_fold(ps, w), po.fold_packets(fs, w), f"{len(names)} designs")
        acc = partial_sum(N_B)
        assert_same(gpu_fold(ps, w, acc), po.fold_packets(fs, w, acc), f"{len(names)} designs, continue")


@pytest.mark.parametrize("noq", [(0,), (2,), (0, 3, 4), (0, 1, 2, 3, 4, 5)])
def test_B_packets_without_qoff(noq):
    """Views without quarter offsets (whole-chunk scans) among views that have them."""
    fs = [design(FAST[i], i, with_qoff=i not in noq) for i in range(6)]
    ps = [dpkt(FAST[i], i, with_qoff=i not in noq) for i in range(6)]
    w = np.array([1.0, -0.5, 2.0, 0.0, -3.0, 0.25], dtype=np.float32)
    assert_same(gpu_fold(ps, w), po.fold_packets(fs, w), f"no qoff in {noq}")
    acc = partial_sum(N_B)
    assert_same(gpu_fold(ps, w, acc), po.fold_packets(fs, w, acc), f"no qoff in {noq}, continue")
    f0, p0 = fs[noq[0]], ps[noq[0]]
    assert_same(gpu_decode(p0), po.decode_packet(f0), "decode ignores qoff")


@pytest.mark.parametrize("weights", [(1.0,), (-1.0,), (0.0,), (-1.0, 1.0), (-1.0, -2.0)])
def test_continue_onto_negative_zero(weights):
    """Reduced from test_B_fold_one_packet: k_fold_q<true> skips the coordinates a packet drops,
    which is exact for a +0-started sum but left a -0.0 of the caller's acc in place where the
    dense sum gives -0 + fl(+0 * w) = +0 for a weight of positive sign.  acc = -0.0 everywhere,
    packets of one entry each (a -0.0 at element 1, a 2.0 at element 3)."""
    n = 6
    fs = [po.build_idxval(n, [1], [NEG0], thresh=0, codec=po.CODEC_TOP, k=1),
          po.build_idxval(n, [3], [2.0], thresh=0, codec=po.CODEC_TOP, k=1)][: len(weights)]
    ps = [cached_packet(("neg0", i), f) for i, f in enumerate(fs)]
    acc = np.full(n, NEG0)
    want = po.fold_packets(fs, weights, acc)
    if weights == (1.0,):                 # dropped: +0; the kept -0.0 * 1 = -0.0 stays
        assert want.view(np.uint32).tolist() == [0, 0x80000000, 0, 0, 0, 0]
    if weights == (-1.0,):                # dropped: -0 + -0 = -0; kept: -0 + +0 = +0
        assert want.view(np.uint32).tolist() == [0x80000000, 0] + [0x80000000] * 4
    assert_same(gpu_fold(ps, weights, acc), want, f"weights {weights}")


# =============================================================================================
# C. launch shape
# =============================================================================================
C_M = [1, 2, 3, 4, 5, 6, 7, 12, 13, 63, 64, 65, 127, 128, 129, 257]


def c_fields(i):
    """Packet i of a launch: the counts rotate with i (27 rotations, the headers cycling)."""
    rot = i % 27
    return FAST[rot % len(FAST)], rot


def c_weights(M, poison=False):
    w = np.random.default_rng([M, 5]).standard_normal(M).astype(np.float32)
    if M > 1:
        w[1] = 0.0
    if M > 2:
        w[2] = NEG0
    if M > 3:
        w[3] = -abs(w[3])
    if poison:
        w[M // 2] = np.inf
        w[M - 1] = np.nan
    return w


def _c_run(M, poison):
    fs = [design(*c_fields(i)) for i in range(M)]
    ps = [dpkt(*c_fields(i)) for i in range(M)]
    w = c_weights(M, poison)
    assert_same(gpu_fold(ps, w), po.fold_packets(fs, w), f"M={M}")
    acc = partial_sum(N_B, seed=M)
    assert_same(gpu_fold(ps, w, acc), po.fold_packets(fs, w, acc), f"M={M} continue")


@pytest.mark.parametrize("M", C_M)
def test_C_launch_shape(M):
    """Item pipeline (two slots of kQGroup = 3 with the past-the-end re-load), the qo1 half
    (packets 64..127) and the split into launches of 128, on non-uniform packets."""
    _c_run(M, poison=False)


@pytest.mark.parametrize("M", [5, 129])
def test_C_inf_and_nan_weight(M):
    """An inf and a NaN weight: both packets poison what they do not fold."""
    _c_run(M, poison=True)


# =============================================================================================
# D. generic and poisoning packets beside ordinary ones
# =============================================================================================
def odd_packet(kind):
    if kind in _FIELDS:
        return _FIELDS[kind]
    rng = np.random.default_rng([len(kind), 31])
    ib = po.index_bits(N_B)
    if kind == "philox":              # native rand-k: about half the listed entries are slack
        seed, offset = 0xC0FFEE_0000_0042, 9
        gidx = design_entries(N_B, range(7), design_counts(5), rng)
        comp = (po.philox_keys_at(gidx, seed, offset).astype(np.uint64) << np.uint64(ib)) | gidx.astype(np.uint64)
        f = po.build_idxval(N_B, gidx, design_values(rng, gidx.size, 1.5, 0.3),
                            thresh=int(np.sort(comp)[gidx.size // 2]), lower=int(comp.min()),
                            codec=po.CODEC_RAND, key_mode=po.KEY_PHILOX, k=gidx.size - gidx.size // 2,
                            seed=seed, offset=offset)
        assert 0 < po.kept_entries(f)[0].size < gidx.size
    elif kind == "unbiased":          # dropout-unbiased, p = 0.3: ~614 entries per quarter
        gidx = np.nonzero(rng.random(N_B) < 0.3)[0]
        f = po.build_idxval(N_B, gidx, design_values(rng, gidx.size, 1.5, 0.3), thresh=0,
                            codec=po.CODEC_DROPOUT_UNBIASED, p=0.3, seed=4)
    elif kind == "p0":                # dropout-unbiased, p = 0: 0 / 0 at every dropped coordinate
        gidx = design_entries(N_B, range(7), design_counts(9), rng)
        f = po.build_idxval(N_B, gidx, design_values(rng, gidx.size, 1.5, 0.3), thresh=0,
                            codec=po.CODEC_DROPOUT_UNBIASED, p=0.0, seed=4)
    else:
        f = design("infkey", 3)
    _FIELDS[kind] = f
    return f


@pytest.mark.parametrize("pos", [0, 3, 6])
@pytest.mark.parametrize("kind", ["philox", "unbiased", "p0", "infkey"])
def test_D_one_odd_packet(kind, pos):
    """Six top-k packets and one odd one: the launch takes the slow body in every workgroup.
    The same rows folded in up to three calls (top-k rows alone: fast body; the odd packet
    alone) must give the same bits."""
    fs = [design(*c_fields(i)) for i in range(6)]
    ps = [dpkt(*c_fields(i)) for i in range(6)]
    fo = odd_packet(kind)
    fs.insert(pos, fo)
    ps.insert(pos, cached_packet(("odd", kind), fo))
    w = np.random.default_rng([pos, 8]).standard_normal(7).astype(np.float32)
    want = po.fold_packets(fs, w)
    if kind == "p0":
        assert np.isnan(want).mean() > 0.5
    assert_same(gpu_fold(ps, w), want, f"{kind} at {pos}: one launch")
    acc = None
    for lo, hi in ((0, pos), (pos, pos + 1), (pos + 1, 7)):
        if hi > lo:
            acc = gpu_fold(ps[lo:hi], w[lo:hi], acc)
    assert_same(acc, want, f"{kind} at {pos}: split calls")
    part = partial_sum(N_B)
    assert_same(gpu_fold(ps, w, part), po.fold_packets(fs, w, part), f"{kind} at {pos}: continue")


# =============================================================================================
# E. the dense decode at its 4096-chunk dispatch
# =============================================================================================
E_SIZES = {"fold_q_dec": (1 << 25) + 3 * CH + QU + 3,        # 4100 chunks: k_fold_q<false, true>
           "sparse": 4094 * CH + QU + 3}                     # 4095 chunks: k_decode_sparse<false>
_E_BUF = {}


def _e_buffers(n):
    """The packet buffers of one size, poison-filled on the device once; every case rewrites
    the same designed chunks, all others keep cnt = 0."""
    if n not in _E_BUF:
        nch, cap = po.num_chunks(n), po.capacity(n)
        _E_BUF[n] = dict(idx=torch.full((cap,), -1, dtype=torch.int16, device="cuda"),
                         val=torch.full((cap,), float("nan"), dtype=torch.float32, device="cuda"),
                         cnt=torch.zeros(nch, dtype=torch.int32, device="cuda"),
                         qoff=torch.zeros(nch, dtype=torch.int64, device="cuda"))
    return _E_BUF[n]


@pytest.mark.parametrize("case", ["top", "philox", "unbiased", "p0"])
@pytest.mark.parametrize("size", list(E_SIZES))
def test_E_dense_decode_dispatch(size, case):
    n = E_SIZES[size]
    nch = po.num_chunks(n)
    assert (nch >= 4096) == (size == "fold_q_dec")
    chunks = [0, nch // 2, nch - 2, nch - 1]                  # first, middle, last whole, partial
    rows = design_counts(0)[3:7]                              # [0, 257, 513, 64] first
    rng = np.random.default_rng([nch, len(case)])
    gidx = design_entries(n, chunks, rows, rng)
    val = design_values(rng, gidx.size, 1.5, 0.3)
    ib = po.index_bits(n)
    if case == "top":                 # the tie cut mid-quarter in the middle chunk
        f = po.build_idxval(n, gidx, val, thresh=(_key(1.5) << ib) | ((nch // 2) * CH + QU + 1000),
                            codec=po.CODEC_TOP)
    elif case == "philox":
        seed, offset = 0xBEEF_0000_0007, 2
        comp = (po.philox_keys_at(gidx, seed, offset).astype(np.uint64) << np.uint64(ib)) | gidx.astype(np.uint64)
        f = po.build_idxval(n, gidx, val, thresh=int(np.sort(comp)[gidx.size // 2]),
                            lower=int(comp.min()), codec=po.CODEC_RAND, key_mode=po.KEY_PHILOX,
                            seed=seed, offset=offset)
    else:
        f = po.build_idxval(n, gidx, val, thresh=0, codec=po.CODEC_DROPOUT_UNBIASED,
                            p=0.3 if case == "unbiased" else 0.0)
    ki, kx, dz = po.decode_sparse(f, np.float32)
    assert 0 < ki.size and (case in ("unbiased", "p0") or ki.size < gidx.size)
    b = _e_buffers(n)
    for c in chunks:
        sl = slice(c * CH, (c + 1) * CH)
        b["idx"][sl] = _dev(f["idx"][sl], np.int16)
        b["val"][sl] = _dev(f["val"][sl], np.float32)
    ct = torch.tensor(chunks, device="cuda")
    b["cnt"][ct] = _dev(f["cnt"][chunks], np.int32)
    b["qoff"][ct] = _dev(f["qoff"][chunks], np.int64)
    assert int(f["cnt"].sum()) == int(f["cnt"][chunks].sum())
    pkt = _codec().Packet(n=n, fmt=po.FMT_IDXVAL, val=b["val"], cnt=b["cnt"], idx=b["idx"],
                          qoff=b["qoff"], hdr=_dev(np.frombuffer(f["hdr"].tobytes(), dtype=np.uint8), np.uint8))
    got = _codec().decode(pkt)
    exp = torch.full((n,), float(dz), dtype=torch.float32, device="cuda")
    exp[torch.from_numpy(ki).cuda()] = torch.from_numpy(kx).cuda()
    gn, en = got.isnan(), exp.isnan()
    zero = torch.zeros((), dtype=torch.int32, device="cuda")
    same = torch.equal(gn, en) and torch.equal(torch.where(gn, zero, got.view(torch.int32)),
                                               torch.where(en, zero, exp.view(torch.int32)))
    if not same:                      # copy back once, for the message
        assert_same(got, exp.cpu().numpy(), f"{size} {case}")
    if case == "p0":
        assert int(en.sum()) >= n - ki.size


# =============================================================================================
# F. the bitmap fold across launches
# =============================================================================================
F_N = 20_011
F_M = [1, 63, 64, 65, 129]


def _f_hand(i, codec, p, share):
    rng = np.random.default_rng([i, 606])
    gidx = np.nonzero(rng.random(F_N) < share)[0]
    return po.build_bitmap(F_N, gidx, design_values(rng, gidx.size, 1.5, 0.3), codec=codec, p=p,
                           seed=i)


def f_pool():
    """Hand-built and encoder-built dropout bitmap packets (fields, device packet); the last
    two are p = 0 packets (hand-built with entries, encoder-built with none)."""
    if "f_pool" in _DEV:
        return _DEV["f_pool"]
    codec = _codec()
    B, U = po.CODEC_DROPOUT_BIASED, po.CODEC_DROPOUT_UNBIASED
    hand = [_f_hand(0, B, 0.3, 0.3), _f_hand(1, U, 0.3, 0.3), _f_hand(2, B, 0.9, 0.9),
            _f_hand(3, U, 0.5, 0.02)]
    assert int(hand[2]["cnt"].max()) > 1024                       # the dense-slot loop
    pool = [(f, to_packet(f)) for f in hand]
    g = torch.from_numpy(_grad(F_N, "gauss", seed=6)).cuda()
    for c, p, seed in ((B, 0.3, 11), (U, 0.3, 12), (U, 0.7, 13)):
        pk = codec.encode_mask(g, c, p=p, seed=seed, fmt=po.FMT_BITMAP)
        pool.append((fields_of(pk), pk))
    f0 = _f_hand(4, U, 0.0, 0.1)
    pk0 = codec.encode_mask(g, U, p=0.0, seed=14, fmt=po.FMT_BITMAP)
    assert int(fields_of(pk0)["cnt"].sum()) == 0
    pool += [(f0, to_packet(f0)), (fields_of(pk0), pk0)]
    _DEV["f_pool"] = pool
    return pool


def test_F_decode():
    for i, (f, p) in enumerate(f_pool()):
        assert_same(gpu_decode(p, np.float32), po.decode_packet(f, np.float32), f"pool[{i}] f32")
        assert_same(gpu_decode(p, np.float64), po.decode_packet(f, np.float64), f"pool[{i}] f64")


@pytest.mark.parametrize("poison", [False, True])
@pytest.mark.parametrize("M", F_M)
def test_F_bitmap_fold(M, poison):
    """k_decode<FC_FMT_BITMAP, true, false>: launches of at most kDecMaxM = 64 packets."""
    pool = f_pool()
    pick = [pool[i % 7] for i in range(M)]
    if poison:                        # p = 0 packets first, in the middle and last
        for j, src in ((0, 7), (M // 2, 8), (M - 1, 7)):
            pick[j] = pool[src]
    fs, ps = [f for f, _ in pick], [p for _, p in pick]
    w = c_weights(M)
    want = po.fold_packets(fs, w)
    assert not poison or np.isnan(want).mean() > 0.5
    assert_same(gpu_fold(ps, w), want, f"M={M}")
    acc = partial_sum(F_N, seed=M)
    assert_same(gpu_fold(ps, w, acc), po.fold_packets(fs, w, acc), f"M={M} continue")
