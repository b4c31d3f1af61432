"""fc_wire_pack_batch / fc_wire_unpack_batch (csrc/fc_wire.hip) through codec.pack, codec.unpack,
Compression.compress_wire and Aggregator.aggregate_wire on an MI355X.

Run:  python -m pytest tests/test_wire_gpu.py -m gpu -q

Hand-built packets on the geometry and the poison convention of tests/test_dot_gpu.py: n = 6 * 8192
+ 2048 + 3, per-quarter counts from COUNTS, every slot position a packet does not list holds
(0xFFFF, NaN).  The expected bytes come from tests/wire_model.py (oracle.packet_oracle.kept_entries
underneath); everything is compared bit for bit.  Only well-formed packets reach the GPU here:
malformed payloads are the host validator's matter (tests/test_wire_host.py).

Switch points of the kernels (names of csrc/fc_wire.hip, not imported):
  kWWaves = 4        chunks per pack / unpack workgroup: 7 chunks end inside the second workgroup
  kWR * 64 = 256     entries per round of loads: chunk totals on both sides of 256, 512, ...
  kWScanBlock = 1024 chunks per step of the scan, 64 per wave: 130, 1024 and 1025 chunks
"""
import types

import numpy as np
import pytest

import wire_model as wm
from oracle import packet_oracle as po

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CH, QU = po.CHUNK, po.QUARTER
N = 6 * CH + QU + 3
COUNTS = (0, 1, 63, 64, 65, 255, 256, 257, 513, 2048)
TIE = np.float32(1.5)
FILL = 0xA5


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from openmsftl_amd import _lib
    assert _lib.load().fc_abi_version() == 4
    yield
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


_MEMO = {}


def memo(key, make):
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


# ---- the hand-built round ---------------------------------------------------------------------
def quarters(n=N):
    return [(s, min(QU, n - s)) for s in range(0, n, QU)]


def design_support(i):
    """Client i's listed coordinates: quarter Q holds COUNTS[(i + Q) % 10] of them."""
    off = (i % 10) * 150 + (i // 20) * 37
    stride = (1, 3, 5)[(i // 20) % 3]
    out = []
    for Q, (start, cap) in enumerate(quarters()):
        cnt = min(COUNTS[(i + Q) % 10], cap)
        loc = np.sort((off + np.arange(cnt, dtype=np.int64) * stride) % QU) if cap == QU \
            else np.arange(cnt, dtype=np.int64)
        out.append(start + loc)
    return np.concatenate(out)


def half_values(rng, size):
    v = (rng.integers(-6, 7, size=size) * 0.5).astype(np.float32)
    v[v == 0] = np.float32(-0.0)
    return v


def top_with_slack(i, Ti):
    """A top-k packet as the sampled encoder leaves it: entries above the k-th magnitude 1.5,
    entries equal to it on both sides of the index cut Ti, slack below it."""
    rng = np.random.default_rng([i, 17])
    idx = design_support(i)
    u = rng.random(idx.size)
    mag = rng.choice(np.array([2.0, 2.5, 3.0], np.float32), size=idx.size)
    mag[u < 0.3] = rng.choice(np.array([0.5, 1.0], np.float32), size=int(np.sum(u < 0.3)))
    mag[(u >= 0.3) & (u < 0.5)] = TIE
    val = (mag * rng.choice(np.array([-1.0, 1.0], np.float32), size=idx.size)).astype(np.float32)
    thresh = (int(po.mag_key(np.array([TIE]))[0]) << po.index_bits(N)) | int(Ti)
    keep = (np.abs(val) > TIE) | ((np.abs(val) == TIE) & (idx >= Ti))
    return po.build_idxval(N, idx, val, thresh=thresh, lower=1, codec=po.CODEC_TOP, k=int(keep.sum()),
                           n_definite=5, n_cand=9)


def special_values(size):
    """-0.0, +0.0, a quiet and a signalling-pattern NaN with payloads, +-inf, a denormal."""
    v = np.arange(1, size + 1, dtype=np.float32)
    bits = np.array([0x80000000, 0x00000000, 0x7FC12345, 0xFFA00001, 0x7F800000, 0xFF800000,
                     0x00000001], dtype=np.uint32)
    at = np.linspace(0, size - 1, bits.size).astype(np.int64)
    v.view(np.uint32)[at] = bits
    return v


def round_fields():
    """Nine clients: top-k with slack (magnitude keys), native rand-k with slack (Philox keys),
    thresh == 0 mask packets (dropout-biased, rand with a host mask), dropout-unbiased with p, and
    a thresh == 0 packet whose kept values include -0.0, +0.0 and NaNs with payloads."""
    def make():
        rng = np.random.default_rng(23)
        ib = po.index_bits(N)
        tops = [top_with_slack(i, Ti) for i, Ti in
                enumerate([3 * CH + QU + 1000, 0, N - 1, 2 * CH + 7, 6 * CH + QU + 1])]
        seed, offset = 0xC0FFEE_0000_0042, 9
        gidx = design_support(5)
        comp = (po.philox_keys_at(gidx, seed, offset).astype(np.uint64) << np.uint64(ib)) | gidx.astype(np.uint64)
        philox = po.build_idxval(N, gidx, half_values(rng, gidx.size),
                                 thresh=int(np.sort(comp)[gidx.size // 2]), lower=int(comp.min()),
                                 codec=po.CODEC_RAND, key_mode=po.KEY_PHILOX,
                                 k=gidx.size - gidx.size // 2, seed=seed, offset=offset)
        assert 0 < po.kept_entries(philox)[0].size < gidx.size
        bidx = design_support(6)
        biased = po.build_idxval(N, bidx, half_values(rng, bidx.size), thresh=0,
                                 codec=po.CODEC_DROPOUT_BIASED, p=0.3, seed=4)
        uidx = np.nonzero(rng.random(N) < 0.5)[0]
        unbiased = po.build_idxval(N, uidx, half_values(rng, uidx.size), thresh=0,
                                   codec=po.CODEC_DROPOUT_UNBIASED, p=0.5, seed=4)
        sidx = design_support(8)
        special = po.build_idxval(N, sidx, special_values(sidx.size), thresh=0, codec=po.CODEC_RAND)
        out = [tops[0], philox, tops[1], biased, tops[2], unbiased, tops[3], special, tops[4]]
        for f in tops:
            assert po.kept_entries(f)[0].size < po.listed_entries(f)[0].size       # slack is listed
        return out
    return memo("round", make)


def round_packets():
    return memo("round-dev", lambda: [to_packet(f) for f in round_fields()])


def model_bytes():
    return memo("round-model", lambda: [wm.pack(f) for f in round_fields()])


def test_design_covers_what_it_claims():
    per = np.array([[np.sum((design_support(i) >= st) & (design_support(i) < st + cap))
                     for st, cap in quarters()] for i in range(10)])
    assert set(per[:, :24].ravel().tolist()) == set(COUNTS)
    assert per[:, 25].max() == 3
    f = round_fields()
    assert int(f[7]["hdr"]["n_entries"]) == 0 == int(f[3]["hdr"]["n_entries"])     # mask headers
    sizes = {len(b) % 16 for b in model_bytes()}
    assert sizes == {0}
    E = [int(wm.parse(b)["hdr"]["n_entries"]) for b in model_bytes()]
    assert any(e % 8 for e in E) and len(set(E)) > 5                              # pads present


# ---- pack -------------------------------------------------------------------------------------
def test_pack_equals_the_model_byte_for_byte():
    codec = _codec()
    for i, (p, want) in enumerate(zip(round_packets(), model_bytes())):
        w = codec.pack(p)
        assert w.n == N and w.nbytes == len(want) and w.buf.data_ptr() % 16 == 0
        assert w.tobytes() == want, f"client {i}"


@pytest.mark.parametrize("M", [1, 2, 9])
def test_a_batch_in_one_call_equals_the_single_calls(M):
    codec = _codec()
    ws = codec.pack(round_packets()[:M])
    assert isinstance(ws, list) and len(ws) == M
    for i, w in enumerate(ws):
        assert w.tobytes() == model_bytes()[i], f"client {i} of {M}"
    again = codec.pack(round_packets()[:M])
    assert [w.tobytes() for w in again] == [w.tobytes() for w in ws]              # the same bytes twice


def test_entries_sizes_the_buffers_and_too_few_raise():
    codec = _codec()
    from openmsftl_amd import _lib
    pk = round_packets()[:3]
    E = [int(wm.parse(b)["hdr"]["n_entries"]) for b in model_bytes()[:3]]
    ws = codec.pack(pk, entries=E)
    assert [w.buf.numel() for w in ws] == [len(b) for b in model_bytes()[:3]]
    assert [w.tobytes() for w in ws] == model_bytes()[:3]
    with pytest.raises(_lib.FedCodecError, match="status 2"):
        codec.pack(pk, entries=[E[0], E[1] - 8, E[2]])


def test_bytes_past_total_bytes_are_untouched_and_a_short_capacity_overflows():
    codec = _codec()
    from openmsftl_amd import _lib
    pk, want = round_packets()[:3], model_bytes()[:3]
    bufs = [torch.full((len(b) + 512,), FILL, dtype=torch.uint8, device="cuda") for b in want]
    hdrs = codec.pack_into(pk, bufs)
    for h, b, raw in zip(hdrs, bufs, want):
        got = b.cpu().numpy()
        assert h.status == 0 and h.total_bytes == len(raw)
        assert got[: len(raw)].tobytes() == raw
        assert np.all(got[len(raw):] == FILL)
    # one byte short: OVERFLOW, a header that says what is needed, nothing else written
    bufs = [torch.full((len(b) + 512,), FILL, dtype=torch.uint8, device="cuda") for b in want]
    caps = [len(want[0]), len(want[1]) - 1, len(want[2])]
    hdrs = codec.pack_into(pk, bufs, capacities=caps)
    assert [h.status for h in hdrs] == [0, _lib.FC_STATUS_OVERFLOW, 0]
    short = bufs[1].cpu().numpy()
    assert hdrs[1].total_bytes == len(want[1]) and hdrs[1].magic == 0x31574346
    assert hdrs[1].n_entries == int(wm.parse(want[1])["hdr"]["n_entries"])
    assert np.all(short[128:] == FILL)
    for i in (0, 2):
        assert bufs[i].cpu().numpy()[: len(want[i])].tobytes() == want[i]


# ---- the scan's boundaries --------------------------------------------------------------------
LONG_NS = [129 * CH + QU + 3, 1024 * CH, 1024 * CH + 5]             # 130, 1024 and 1025 chunks
LONG_COUNTS = (0, 1, 65, 257, 3)


def long_fields(n, j):
    """Chunk c lists LONG_COUNTS[(c + j) % 5] entries; every third one is slack below thresh."""
    out = []
    for c in range(po.num_chunks(n)):
        cap = min(CH, n - c * CH)
        cnt = min(LONG_COUNTS[(c + j) % 5], cap)
        loc = np.sort((c * 131 + j * 517 + np.arange(cnt, dtype=np.int64) * 29) % CH) if cap == CH \
            else np.arange(cnt, dtype=np.int64)
        out.append(c * CH + loc)
    idx = np.concatenate(out)
    val = np.where(np.arange(idx.size) % 3 == 0, 0.5, 2.0).astype(np.float32)
    thresh = int(po.mag_key(np.float32([1.0]))[0]) << po.index_bits(n)
    return po.build_idxval(n, idx, val, thresh=thresh, lower=1, codec=po.CODEC_TOP,
                           k=int(np.sum(val > 1)))


@pytest.mark.parametrize("n", LONG_NS)
def test_sparse_packets_across_the_scans_steps(n):
    codec = _codec()
    fields = [long_fields(n, j) for j in range(2)]
    want = [wm.pack(f) for f in fields]
    if po.num_chunks(n) == 1025:
        assert n - 1024 * CH == 5 and wm.parse(want[0])["start"][1024] > 0         # a carry crosses
    pk = [to_packet(f) for f in fields]
    ws = codec.pack(pk)
    assert [w.tobytes() for w in ws] == want
    back = codec.unpack(ws)
    for p, q in zip(pk, back):
        assert torch.equal(codec.decode(p).view(torch.int32), codec.decode(q).view(torch.int32))


# ---- unpack -----------------------------------------------------------------------------------
def poisoned(m):
    codec = _codec()
    pk = codec.Packet.alloc_batch(N, m, po.FMT_IDXVAL, torch.device("cuda"))
    for p in pk:
        p.idx.fill_(-1)
        p.val.fill_(float("nan"))
        p.cnt.fill_(-1)
        p.qoff.fill_(-1)
        p.hdr.fill_(0xEE)
    return pk


def unpacked_round():
    def make():
        codec = _codec()
        dst = poisoned(9)
        out = codec.unpack(codec.pack(round_packets()), dst)
        assert all(a is b for a, b in zip(out, dst))
        return out
    return memo("unpacked", make)


def test_unpack_writes_the_kept_entries_and_leaves_poison_elsewhere():
    for i, (p, raw) in enumerate(zip(unpacked_round(), model_bytes())):
        want = wm.unpack(raw)                                        # poison where nothing is listed
        assert p.idx.cpu().numpy().view(np.uint16).tobytes() == want["idx"].tobytes(), i
        got_val = p.val.cpu().numpy()
        assert got_val.view(np.uint32).tobytes() == want["val"].view(np.uint32).tobytes(), i
        assert p.cnt.cpu().numpy().view(np.uint32).tobytes() == want["cnt"].tobytes(), i
        assert p.qoff.cpu().numpy().view(np.uint64).tobytes() == want["qoff"].tobytes(), i
        assert p.hdr.cpu().numpy().tobytes() == want["hdr"].tobytes(), i
        h = p.header()
        assert h.lower == h.thresh and h.status == 0 and h.n_definite == 0 == h.n_cand
        assert h.n_entries == int(want["cnt"].sum()) and p.k == h.k


def test_a_kept_negative_zero_and_nan_payloads_survive():
    raw = _codec().pack(round_packets()[7]).tobytes()
    vals = wm.parse(raw)["val"].view(np.uint32)
    for bits in (0x80000000, 0x00000000, 0x7FC12345, 0xFFA00001, 0x7F800000, 0xFF800000, 0x00000001):
        assert bits in vals, hex(bits)
    assert raw == model_bytes()[7]
    back = unpacked_round()[7]
    src = round_packets()[7]
    assert torch.equal(back.val.view(torch.int32), src.val.view(torch.int32))      # same slots: thresh == 0


def same(a, b):
    return torch.equal(a.contiguous().view(torch.uint8), b.contiguous().view(torch.uint8))


def test_every_consumer_gives_the_same_bits_on_the_unpacked_packets():
    codec = _codec()
    src, dst = round_packets(), unpacked_round()
    for i, (p, q) in enumerate(zip(src, dst)):
        assert same(codec.decode(p), codec.decode(q)), f"decode, client {i}"
    w = [0.25, -1.5, 1.0, 0.125, 3.0, -0.5, 1.0 / 9, 2.0, 0.75]
    assert same(codec.decode_accumulate(src, w), codec.decode_accumulate(dst, w))
    finite = [i for i in range(9) if i != 7]                        # the Gram of client 7 is NaN: compared too
    g0, g1 = codec.gram(src), codec.gram(dst)
    assert torch.equal(torch.isnan(g0), torch.isnan(g1)) and bool(torch.isnan(g0[7]).all())
    assert same(g0[finite][:, finite], g1[finite][:, finite])
    v = torch.from_numpy((np.random.default_rng(3).integers(-8, 9, size=N) * 0.5).astype(np.float32)).cuda()
    for vec in (v, None):
        d0, d1 = codec.dot_dense(src, vec), codec.dot_dense(dst, vec)
        assert torch.equal(torch.isnan(d0), torch.isnan(d1))
        keep = ~torch.isnan(d0)
        assert same(d0[keep], d1[keep]) and int(keep.sum()) == 9


def test_repacking_the_unpacked_packets_gives_the_same_bytes():
    ws = _codec().pack(unpacked_round())                            # sized by one read of the counts
    assert [w.tobytes() for w in ws] == model_bytes()


def test_pack_and_unpack_reject_what_they_cannot_take():
    codec = _codec()
    pk = round_packets()
    with pytest.raises(ValueError, match="no packets"):
        codec.pack([])
    other = to_packet(po.build_idxval(3 * CH + 5, np.array([1, 9]), np.float32([1, 2]), thresh=0,
                                      codec=po.CODEC_TOP, k=2))
    with pytest.raises(ValueError, match="share n"):
        codec.pack([pk[0], other])
    bitmap = codec.encode_mask(torch.ones(3 * CH + 5, dtype=torch.float32, device="cuda"), 3, p=0.5, fmt=1)
    with pytest.raises(ValueError, match="idx/val"):
        codec.pack(bitmap)
    w = codec.pack(pk[0])
    with pytest.raises(ValueError, match="one destination"):
        codec.unpack([w], poisoned(2))
    with pytest.raises(ValueError, match="destination must be"):
        codec.unpack(w, other)


# ---- real encodes -----------------------------------------------------------------------------
N_E, K_E = 100_003, 10_000


def test_sampled_and_exact_encodes_pack_to_the_same_bytes_and_round_trip():
    codec = _codec()
    g = torch.from_numpy(np.random.default_rng(41).standard_normal(N_E).astype(np.float32)).cuda()
    a = codec.encode_top(g, K_E)
    b = codec.encode_top(g, K_E, exact=True)
    ha, hb = a.header(), b.header()
    assert ha.n_entries >= K_E == hb.n_entries
    wa, wb = codec.pack(a), codec.pack(b)
    raw = wa.tobytes()
    assert raw == wb.tobytes() and len(raw) == codec.wire_bytes(N_E, K_E)
    assert int(wm.parse(raw)["hdr"]["n_entries"]) == K_E
    idx, val = po.topk_packet(g.cpu().numpy(), K_E)
    assert raw == wm.from_entries(N_E, idx, val, np.frombuffer(bytes(ha), dtype=po.HDR_DTYPE)[0])
    back = codec.unpack(codec.wire_from_host(raw, n=N_E))
    assert back.k == K_E and same(codec.decode(back), codec.decode(a))
    for data in (np.frombuffer(raw, dtype=np.uint8), torch.frombuffer(bytearray(raw), dtype=torch.uint8)):
        assert codec.wire_from_host(data).tobytes() == raw
    with pytest.raises(ValueError, match="expected"):
        codec.wire_from_host(raw, n=N_E + 1)


# ---- a round from payloads --------------------------------------------------------------------
N_R, FRAC, M_R = 3 * CH + 5, 0.1, 5


def round_grads():
    def make():
        rng = np.random.default_rng(20261020)
        base = rng.standard_normal(N_R)
        return [(base + (0.3 + i) * rng.standard_normal(N_R)).astype(np.float32) for i in range(M_R)]
    return memo("grads", make)


def make_clients(ef=False):
    from openmsftl_amd import Compression
    cfg = {"compression_function": "top", "fraction_coordinate": FRAC}
    if ef:
        cfg["error_feedback"] = True
    return [types.SimpleNamespace(C=Compression(dict(cfg)), grad=g, client_id=i)
            for i, g in enumerate(round_grads())]


def small_budget():
    """A device budget under which plan_group gives fold groups of 2."""
    from openmsftl_amd import _lib, pipeline
    fixed = 6 * 4 * N_R + int(_lib.load().fc_workspace_bytes(N_R))
    budget = fixed + 2 * pipeline.packet_bytes(N_R) + 1
    assert pipeline.plan_group(N_R, M_R, budget) == 2
    return budget


SCHEMES = {"fed_avg": ({"aggregation_scheme": "fed_avg"}, "stream"),
           "krum": ({"aggregation_scheme": "krum", "krum_frac": 0.6}, "gram"),
           "geometric_median": ({"aggregation_scheme": "geometric_median"}, "gram")}


@pytest.mark.parametrize("scheme", sorted(SCHEMES))
def test_aggregate_wire_equals_aggregate_grads(scheme):
    from openmsftl_amd.aggregation import Aggregator
    cfg, route = SCHEMES[scheme]
    cfg = dict(cfg)
    if scheme == "fed_avg":
        cfg["device_budget_bytes"] = small_budget()                 # the fold in groups of 2, 2, 1
    clients = make_clients()
    ref = Aggregator(dict(cfg))
    ref.aggregate_grads(clients)
    assert ref.agg_path == route
    payloads = [c.C.compress_wire(c.grad) for c in make_clients()]
    k = round(FRAC * N_R)
    assert all(isinstance(p, bytes) and len(p) == _codec().wire_bytes(N_R, k) for p in payloads)
    agg = Aggregator(dict(cfg))
    agg.aggregate_wire(payloads)
    assert agg.agg_path == "wire" and agg.curr_G is None
    assert agg.agg_grad.dtype == np.float32 and agg.agg_grad.shape == (N_R,)
    assert agg.agg_grad.tobytes() == ref.agg_grad.tobytes()
    agg.aggregate_wire(payloads, n=N_R)                              # the packets are reused
    assert agg.agg_grad.tobytes() == ref.agg_grad.tobytes()


def test_compress_wire_with_error_feedback_keeps_compress_residuals():
    from openmsftl_amd.aggregation import Aggregator
    cfg = {"aggregation_scheme": "fed_avg", "device_budget_bytes": small_budget()}
    a, b = make_clients(ef=True), make_clients(ef=True)
    ref, agg = Aggregator(dict(cfg)), Aggregator(dict(cfg))
    for rnd in range(2):                                            # the second round adds the residual
        ref.aggregate_grads(a)                                      # compress() per client
        assert ref.agg_path == "dense-fold"
        agg.aggregate_wire([c.C.compress_wire(c.grad) for c in b])
        assert agg.agg_grad.tobytes() == ref.agg_grad.tobytes(), f"round {rnd}"
        for x, y in zip(a, b):
            rx, ry = x.C.get_residual(), y.C.get_residual()         # a tensor after a device input
            rx = rx.cpu().numpy() if isinstance(rx, torch.Tensor) else rx
            assert isinstance(ry, np.ndarray) and ry.shape == (N_R,) and np.any(ry != 0)
            assert rx.tobytes() == ry.tobytes(), f"round {rnd}"
    dense = make_clients()[0].C.compress(round_grads()[0])
    raw = make_clients()[0].C.compress_wire(torch.from_numpy(round_grads()[0]).cuda())
    back = _codec().decode(_codec().unpack(_codec().wire_from_host(raw))).cpu().numpy()
    assert back.tobytes() == dense.tobytes()


def test_aggregate_wire_names_what_it_cannot_do():
    from openmsftl_amd import Compression
    from openmsftl_amd.aggregation import Aggregator
    payloads = [c.C.compress_wire(c.grad) for c in make_clients()[:2]]
    with pytest.raises(NotImplementedError, match="hierarchies"):
        Aggregator({"aggregation_scheme": "fed_avg", "num_hierarchies": 1,
                    "cluster_size_list": [2]}).aggregate_wire(payloads)
    short = Compression({"compression_function": "top", "fraction_coordinate": FRAC}).compress_wire(
        round_grads()[0][: 2 * CH])
    with pytest.raises(NotImplementedError, match="one length"):
        Aggregator({"aggregation_scheme": "fed_avg"}).aggregate_wire(payloads + [short])
    with pytest.raises(NotImplementedError, match="fit device_budget_bytes"):
        Aggregator({"aggregation_scheme": "krum", "device_budget_bytes": 1 << 16}).aggregate_wire(payloads)
    with pytest.raises(NotImplementedError, match="at most 128"):
        Aggregator({"aggregation_scheme": "krum"}).aggregate_wire(payloads * 65)
    with pytest.raises(NotImplementedError, match="'top' only"):
        Compression({"compression_function": "rand"}).compress_wire(round_grads()[0])
