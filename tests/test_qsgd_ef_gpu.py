"""QSGD with error feedback on the GPU: fc_qsgd_encode_ef against the chain of the existing entry
points and the NumPy model (tests/qsgd_ef_model.py over oracle/qsgd_oracle.py), the drop-in
Compression over several rounds, the wire form and the Aggregator's "qsgd" / "wire-qsgd" routes.

Run:  python -m pytest tests/test_qsgd_ef_gpu.py -m gpu -q

Everything is compared byte for byte except the header's norm against NumPy's own float64 sum
(rel 1e-12: the device adds the squares in its own fixed order).  The codes and values of the model
take the DEVICE's norm from the packet header, as tests/test_gpu_parity.py does for the plain codec.
"""
import ctypes
import functools
import types

import numpy as np
import pytest

import qsgd_ef_model as qm
from oracle import qsgd_oracle as qo

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F = np.float32
SENTINEL = 0x5A5A5A5A


def _codec():
    from openmsftl_amd import codec
    return codec


def _dev(x):
    return torch.from_numpy(np.array(x, copy=True)).cuda()           # (the cached inputs are read-only)


@functools.lru_cache(maxsize=None)
def _inputs(n: int):
    """(g, e, a): g as test_qsgd_codes_and_values_match_oracle builds it, a residual of comparable
    magnitude, and their float32 sum made on the host."""
    rng = np.random.default_rng(n)
    scale = 10.0 ** rng.uniform(-4, 1)
    g = (rng.standard_normal(n) * scale).astype(F)
    if n > 10:
        g[:3] = [0.0, -0.0, 1e-40]
    e = (rng.standard_normal(n) * scale * 0.5).astype(F)
    if n > 10:
        e[1:3] = [0.0, -1e-40]                         # -0.0 + +0.0 and a denormal cancellation
    for x in (g, e):
        x.setflags(write=False)
    return g, e, qm.encoded(g, e)


def _guarded_packet(n, bits):
    """A packet whose codes are followed by 64 sentinel words, and a residual buffer followed by 64
    sentinel floats: the encode may write neither."""
    codec = _codec()
    from openmsftl_amd import _lib as L
    words = int(L.load().fc_qsgd_code_words(n, bits))
    cbuf = torch.full((words + 64,), SENTINEL, dtype=torch.int32, device="cuda")
    rbuf = torch.full((n + 64,), SENTINEL, dtype=torch.int32, device="cuda").view(torch.float32)
    pkt = codec.QsgdPacket(cbuf[:words], torch.zeros(L.HDR_BYTES, dtype=torch.uint8, device="cuda"), n, bits)
    return pkt, cbuf, rbuf, words


def _same_but_nan(got: np.ndarray, want: np.ndarray):
    """NaN positions equal, the bits equal elsewhere."""
    gn, wn = np.isnan(got), np.isnan(want)
    assert (gn == wn).all()
    assert got[~gn].tobytes() == want[~wn].tobytes()


def _check_against_chain(g, e, bits, seed, off, oracle=True):
    """One fused call on (g, e) against encode_qsgd / decode_qsgd on a = fl32(g + e) from the host
    (and the NumPy model).  Returns (header, code words, e')."""
    codec = _codec()
    n = g.size
    a = qm.encoded(g, e)
    pkt, cbuf, rbuf, words = _guarded_packet(n, bits)
    gd, ed = _dev(g), (None if e is None else _dev(e))
    got_pkt, res = codec.encode_qsgd(gd, bits, seed=seed, offset=off, packet=pkt, residual=ed,
                                     residual_out=rbuf[:n])
    assert got_pkt is pkt and res.data_ptr() == rbuf.data_ptr()
    chain = codec.encode_qsgd(_dev(a), bits, seed=seed, offset=off)
    hdr = pkt.hdr.cpu().numpy().tobytes()
    assert hdr == chain.hdr.cpu().numpy().tobytes()                    # all 96 bytes
    codes = pkt.codes.cpu().numpy().view(np.uint32)
    assert codes.tobytes() == chain.codes.cpu().numpy()[:words].tobytes()
    assert (cbuf[words:].cpu().numpy().view(np.uint32) == SENTINEL).all()
    assert (rbuf[n:].view(torch.int32).cpu().numpy().view(np.uint32) == SENTINEL).all()
    h = pkt.header()
    assert (h.n, h.k, h.n_entries, h.codec, h.format, h.status, h.key_mode) == (n, bits, n, 5, 2, 0, 1)
    assert (h.seed, h.offset) == (seed, off)
    finite = np.isfinite(a).all()
    if finite:
        assert h.p == pytest.approx(qo.norm64(a), rel=1e-12)            # fp64, reassociated sum
    q = codec.decode_qsgd(pkt).cpu().numpy()
    want_res = qm.residual(a, q)
    got_res = res.cpu().numpy()
    if finite:
        assert got_res.tobytes() == want_res.tobytes()
    else:
        _same_but_nan(got_res, want_res)
    if oracle:
        _, _, mw, mq, me = qm.encode(g, e, bits, seed, off, norm=h.p)
        assert codes.tobytes() == mw.tobytes()
        if finite:
            assert q.tobytes() == mq.tobytes() and got_res.tobytes() == me.tobytes()
    # the inputs are read only
    assert gd.cpu().numpy().tobytes() == g.tobytes()
    assert e is None or ed.cpu().numpy().tobytes() == e.tobytes()
    return h, codes, got_res


# ---- 1. fused equals the chain --------------------------------------------------------------
NS = [1, 3, 7, 8, 9, 255, 256, 257, 511, 512, 513, 4101, 70_001, 3 * 2 ** 20 + 5]


@pytest.mark.parametrize("bits", [1, 2, 3, 6, 7, 14])
@pytest.mark.parametrize("n", NS)
def test_fused_equals_the_chain_and_the_model(n, bits):
    g, e, _ = _inputs(n)
    _check_against_chain(g, e, bits, 1234 + bits, 7)


# ---- 2. past the quantise pass's grid cap ---------------------------------------------------
def test_fused_equals_the_chain_past_the_grid_cap():
    """8192 workgroups of 256 threads cover 2^21 groups of 8: at n = 2^24 + 4099 the grid-stride loop
    of the quantise pass takes a second step."""
    n = 2 ** 24 + 4099
    g, e, _ = _inputs(n)
    _check_against_chain(g, e, 2, 99, 3, oracle=False)


# ---- 3. edge inputs ---------------------------------------------------------------------------
def _raw_encode_ef(g, e, want_out, bits, seed, off):
    """fc_qsgd_encode_ef itself, with NULL where asked: (packet, res_out or None)."""
    codec = _codec()
    from openmsftl_amd import _lib as L
    lib = L.load()
    n = g.numel()
    pkt = codec.QsgdPacket.alloc(n, bits, g.device)
    out = torch.empty(n, dtype=torch.float32, device=g.device) if want_out else None
    ws = torch.zeros(int(lib.fc_qsgd_workspace_bytes()), dtype=torch.uint8, device=g.device)
    ptr = lambda t: ctypes.c_void_p(t.data_ptr()) if t is not None else None      # noqa: E731
    L.check(lib.fc_qsgd_encode_ef(ptr(g), ptr(e), ptr(out), n, bits, seed, off, ptr(pkt.codes),
                                  pkt.codes.numel(), ptr(pkt.hdr), ptr(ws), ws.numel(),
                                  ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)), "fc_qsgd_encode_ef")
    torch.cuda.synchronize()
    return pkt, out


def _bytes(pkt):
    return pkt.hdr.cpu().numpy().tobytes() + pkt.codes.cpu().numpy().tobytes()


@pytest.mark.parametrize("n", [9, 4101])
def test_null_residual_pointers(n):
    codec = _codec()
    g, e, a = _inputs(n)
    g = g.copy()
    g[n // 2] = -0.0
    bits, seed, off = 2, 5, 11
    plain = codec.encode_qsgd(_dev(g), bits, seed=seed, offset=off)
    # res_in NULL, res_out given: a = g itself, so -0.0 keeps its sign bit in the code
    h, codes, res = _check_against_chain(g, None, bits, seed, off)
    assert (int(qo.unpack(codes, n, bits)[n // 2]) >> 3) == 1
    pkt, out = _raw_encode_ef(_dev(g), None, True, bits, seed, off)
    assert _bytes(pkt) == _bytes(plain) and out.cpu().numpy().tobytes() == res.tobytes()
    # with a zero residual the add makes it +0.0
    _, codes0, _ = _check_against_chain(g, np.zeros(n, F), bits, seed, off)
    assert (int(qo.unpack(codes0, n, bits)[n // 2]) >> 3) == 0
    # res_in given, res_out NULL: the packet of a, nothing else written
    pkt, out = _raw_encode_ef(_dev(g), _dev(e), False, bits, seed, off)
    assert out is None
    assert _bytes(pkt) == _bytes(codec.encode_qsgd(_dev(qm.encoded(g, e)), bits, seed=seed, offset=off))
    # both NULL: fc_qsgd_encode
    pkt, out = _raw_encode_ef(_dev(g), None, False, bits, seed, off)
    assert out is None and _bytes(pkt) == _bytes(plain)


@pytest.mark.parametrize("n", [9, 4101])
def test_zero_and_denormal_gradients(n):
    for bits in (2, 14):
        h, codes, res = _check_against_chain(np.zeros(n, F), np.zeros(n, F), bits, 3, 4)
        assert h.p == 0.0 and not codes.any() and res.tobytes() == np.zeros(n, F).tobytes()
        # float32 denormals: s / norm overflows float32, the level takes the fp64 form
        rng = np.random.default_rng(n + bits)
        g = rng.integers(-2000, 2000, n).astype(np.int32)
        e = rng.integers(-500, 500, n).astype(np.int32)
        den = lambda k: (np.abs(k).astype(np.uint32) | (np.uint32(0x80000000) * (k < 0))).view(F)   # noqa: E731
        h, codes, _ = _check_against_chain(den(g), den(e), bits, 3, 4)
        assert 0 < h.p < 2.0 ** bits / np.finfo(F).max and codes.any()


@pytest.mark.parametrize("n", [9, 4101])
def test_one_hot_at_14_bits_never_decodes_to_zero(n):
    codec = _codec()
    g, e = np.zeros(n, F), np.zeros(n, F)
    at = n - 2
    g[at], e[at] = -3.0, 0.25
    a = qm.encoded(g, e)
    gd, ed = _dev(g), _dev(e)
    pkt = codec.QsgdPacket.alloc(n, 14, gd.device)
    out = torch.empty(n, dtype=torch.float32, device="cuda")
    want_q = F(-(2.75 / qo.tau(n, 2.0 ** 14)))
    assert want_q != 0
    for seed in range(50):
        codec.encode_qsgd(gd, 14, seed=seed, offset=seed + 1, packet=pkt, residual=ed, residual_out=out)
        q = codec.decode_qsgd(pkt).cpu().numpy()
        r = out.cpu().numpy()
        assert pkt.header().p == 2.75 and q[at] == want_q, seed
        # (at n = 9 tau is 1 + 3.4e-8 and the float32 value is the norm itself: the residual is 0)
        assert r[at] == F(a[at] - want_q) and np.count_nonzero(q) == 1, seed
        assert not np.delete(r, at).any(), seed


@pytest.mark.parametrize("n", [9, 4101])
@pytest.mark.parametrize("kind", ["nan in g", "nan in e", "inf in g", "-inf in e", "overflow"])
def test_non_finite_inputs_poison_the_residual_as_the_arithmetic_says(n, kind):
    g, e, _ = _inputs(n)
    g, e = g.copy(), e.copy()
    at = n - 3
    if kind == "nan in g":
        g[at] = np.nan
    elif kind == "nan in e":
        e[at] = np.nan
    elif kind == "inf in g":
        g[at] = np.inf
    elif kind == "-inf in e":
        e[at] = -np.inf
    else:
        g[at] = e[at] = F(3e38)
    a = qm.encoded(g, e)
    assert not np.isfinite(a[at])
    for bits in (2, 8):
        h, codes, res = _check_against_chain(g, e, bits, 8, 2)
        assert not np.isfinite(h.p)
        lev = qo.unpack(codes, n, bits) & np.uint32((1 << (qo.width(bits) - 1)) - 1)
        assert int(lev[at]) == 0                                    # NaN (or inf * 0) -> level 0
        assert np.isnan(res[at])


# ---- 4. determinism ---------------------------------------------------------------------------
def test_two_calls_give_the_same_bytes():
    codec = _codec()
    n = 70_001
    g, e, _ = _inputs(n)
    gd, ed = _dev(g), _dev(e)
    runs = []
    for _ in range(2):
        pkt, res = codec.encode_qsgd(gd, 6, seed=4, offset=9, residual=ed)
        runs.append(_bytes(pkt) + res.cpu().numpy().tobytes())
    assert runs[0] == runs[1]
    assert gd.cpu().numpy().tobytes() == g.tobytes() and ed.cpu().numpy().tobytes() == e.tobytes()


def test_encode_qsgd_argument_checks():
    codec = _codec()
    g = _dev(np.ones(64, F))
    with pytest.raises(ValueError, match="residual must have g's length"):
        codec.encode_qsgd(g, 2, residual=_dev(np.ones(65, F)))
    with pytest.raises(ValueError, match="residual_out must have g's length"):
        codec.encode_qsgd(g, 2, residual_out=_dev(np.ones(63, F)))
    from openmsftl_amd._lib import FedCodecError
    with pytest.raises(FedCodecError, match="overlap g"):
        codec.encode_qsgd(g, 2, residual_out=g)
    r = _dev(np.ones(64, F))
    with pytest.raises(FedCodecError, match="overlap res_in"):
        codec.encode_qsgd(g, 2, residual=r, residual_out=r)
    assert isinstance(codec.encode_qsgd(g, 2), codec.QsgdPacket)      # without a residual: as before


# ---- 5. Compression over several rounds -----------------------------------------------------
def _native(bits, **more):
    from openmsftl_amd import Compression
    return Compression(dict({"compression_function": "qsgd", "qsgd": "native", "num_bits": bits,
                             "seed": 21, "error_feedback": True}, **more))


def _twin_header(C, g, bits):
    """The header and codes C's next call will produce, from a second object in C's state."""
    T = _native(bits)
    T._calls = C._calls
    r = C.get_residual()
    if r is not None:
        T.set_residual(r)
    pkt = T._qsgd_packet(g)
    return pkt.header(), pkt.codes.cpu().numpy().view(np.uint32)


def _host(x):
    return x.cpu().numpy() if isinstance(x, torch.Tensor) else np.asarray(x)


@pytest.mark.parametrize("tensor", [False, True], ids=["numpy", "tensor"])
@pytest.mark.parametrize("bits", [2, 8])
def test_compression_rounds_follow_the_model_and_telescope(bits, tensor):
    n, T = 70_001, 6
    rng = np.random.default_rng(bits)
    grads = [(rng.standard_normal(n) * 0.1).astype(F) for _ in range(T)]
    C = _native(bits)
    e = None
    sum_q, sum_g, slack = np.zeros(n), np.zeros(n), np.zeros(n)
    for t, g in enumerate(grads):
        x = _dev(g) if tensor else g
        h, words = _twin_header(C, x, bits)
        assert (h.seed, h.offset) == (21, t + 1)
        q = C.compress(x)
        assert isinstance(q, torch.Tensor) == tensor and q.dtype == (torch.float32 if tensor else F)
        _, _, mw, mq, e = qm.encode(g, e, bits, 21, t + 1, norm=h.p)
        assert words[: mw.size].tobytes() == mw.tobytes()
        assert _host(q).tobytes() == mq.tobytes()
        r = C.get_residual()
        assert isinstance(r, torch.Tensor) == tensor and _host(r).tobytes() == e.tobytes()
        assert _host(x).tobytes() == g.tobytes() and C._calls == t + 1
        sum_q += mq.astype(np.float64)
        sum_g += g.astype(np.float64)
        slack += np.abs(mq.astype(np.float64)) + 2.0 * np.abs(e.astype(np.float64))
    # nothing is lost: two float32 roundings per round and coordinate
    err = np.abs(sum_q + e.astype(np.float64) - sum_g)
    print("telescoping: max err / bound =", float(np.max(err / np.maximum(1.01 * 2.0 ** -24 * slack, 1e-300))))
    assert (err <= 1.01 * 2.0 ** -24 * slack).all()


def test_compression_residual_accessors_and_float64():
    n, bits = 70_001, 2
    rng = np.random.default_rng(3)
    g = rng.standard_normal(n).astype(F)
    C = _native(bits)
    r0 = (0.3 * rng.standard_normal(n)).astype(F)
    C.set_residual(r0)
    h, _ = _twin_header(C, g, bits)
    q = C.compress(g)
    _, _, _, mq, me = qm.encode(g, r0, bits, 21, 1, norm=h.p)
    assert q.tobytes() == mq.tobytes() and C.get_residual().tobytes() == me.tobytes()
    # a length mismatch raises before anything advances
    with pytest.raises(ValueError, match="reset_residual"):
        C.compress(g[:100])
    assert C._calls == 1 and C.get_residual().tobytes() == me.tobytes()
    C.reset_residual()
    assert C.get_residual() is None
    h, _ = _twin_header(C, g[:100], bits)
    q = C.compress(g[:100])
    _, _, _, mq, me = qm.encode(g[:100], None, bits, 21, 2, norm=h.p)
    assert q.tobytes() == mq.tobytes() and C.get_residual().tobytes() == me.tobytes()
    with pytest.raises(TypeError, match="float32"):
        C.set_residual(np.zeros(100, np.float64))
    with pytest.raises(NotImplementedError, match="float32 gradients only"):
        C.compress(np.zeros(100, np.float64))
    assert C._calls == 2
    # an empty gradient: nothing to do, nothing advances
    out = C.compress(np.zeros(0, F))
    assert out.shape == (0,) and out.dtype == F and C._calls == 2


@pytest.mark.parametrize("ef", [False, True], ids=["plain", "error feedback"])
def test_compress_wire_is_the_packed_packet_and_advances_the_same_state(ef):
    codec = _codec()
    n, bits = 70_001, 5
    rng = np.random.default_rng(9)
    A, B = _native(bits, error_feedback=ef), _native(bits, error_feedback=ef)
    for t in range(2):
        g = rng.standard_normal(n).astype(F)
        raw = A.compress_wire(g)
        pkt = B._qsgd_packet(g)
        assert isinstance(raw, bytes) and len(raw) == codec.qsgd_wire_bytes(n, bits) == qm.wire_bytes(n, bits)
        assert raw == codec.pack_qsgd(pkt).cpu().numpy().tobytes()
        h = pkt.header()
        assert (h.seed, h.offset) == (21, t + 1)
        words = pkt.codes.cpu().numpy().view(np.uint32)[: qm.code_words(n, bits)]
        assert raw == qm.pack(n, bits, 21, t + 1, h.p, words)
        assert A._calls == B._calls == t + 1
        if ef:
            assert A.get_residual().tobytes() == B.get_residual().tobytes()
        else:
            assert A.get_residual() is None
    with pytest.raises(ValueError, match="empty gradient"):
        A.compress_wire(np.zeros(0, F))


# ---- 6. the wire form -------------------------------------------------------------------------
@pytest.mark.parametrize("n,bits", [(9, 2), (33, 6), (4101, 1), (70_001, 3), (70_001, 14)])
def test_wire_round_trip(n, bits):
    codec = _codec()
    g, e, a = _inputs(n)
    pkt, _ = codec.encode_qsgd(_dev(g), bits, seed=2, offset=6, residual=_dev(e))
    wire = codec.pack_qsgd(pkt)
    assert wire.is_cuda and wire.dtype == torch.uint8 and wire.numel() == codec.qsgd_wire_bytes(n, bits)
    raw = wire.cpu().numpy().tobytes()
    h = pkt.header()
    words = pkt.codes.cpu().numpy().view(np.uint32)
    assert raw == qm.pack(n, bits, 2, 6, h.p, words[: qm.code_words(n, bits)])       # the pad words are zero
    assert codec.is_qsgd_payload(raw)
    back = codec.qsgd_from_host(wire.cpu(), n)
    assert (back.n, back.bits) == (n, bits) and back.codes.data_ptr() % 16 == 0
    assert back.buf.data_ptr() % 256 == 0 and back.codes.data_ptr() == back.buf.data_ptr() + 128
    assert codec.decode_qsgd(back).cpu().numpy().tobytes() == codec.decode_qsgd(pkt).cpu().numpy().tobytes()
    w = [0.25, 0.5]
    fold = codec.decode_accumulate_qsgd([pkt, pkt], w).cpu().numpy()
    assert codec.decode_accumulate_qsgd([back, codec.qsgd_from_host(raw)], w).cpu().numpy().tobytes() == fold.tobytes()
    # a corrupted payload never reaches the device
    bad = bytearray(raw)
    bad[129 if bits > 6 else 128] |= 0x07 if bits <= 2 else 0x7F      # a level above s
    with pytest.raises(ValueError, match="qsgd wire: the code of element 0 has level"):
        codec.qsgd_from_host(bytes(bad))
    with pytest.raises(ValueError, match="expected"):
        codec.qsgd_from_host(raw, n + 1)
    with pytest.raises(ValueError, match="total_bytes"):
        codec.qsgd_from_host(raw[:-16])


# ---- 7. the routes ------------------------------------------------------------------------------
def _round_clients(grads):
    from openmsftl_amd import Compression
    bits = [2, 5, 12, 2, 5]
    ef = [True, False, True, True, False]
    return [types.SimpleNamespace(
        C=Compression({"compression_function": "qsgd", "qsgd": "native", "num_bits": b, "seed": 40 + i,
                       "error_feedback": f}), grad=g, client_id=i)
        for i, (g, b, f) in enumerate(zip(grads, bits, ef))]


def _state(clients):
    return [(c.C._calls, None if c.C.get_residual() is None else _host(c.C.get_residual()).tobytes())
            for c in clients]


def test_routes_give_equal_bits_and_leave_equal_state():
    from openmsftl_amd.aggregation import Aggregator, qsgd_packet_bytes
    m, n = 5, 70_001
    rng = np.random.default_rng(17)
    w = rng.uniform(0.05, 1.0, m).astype(F)
    budget = 8 * n + 2 * qsgd_packet_bytes(n, 12) + 100               # two packets fit: groups of 2, 2, 1

    def agg(**cfg):
        a = Aggregator(dict({"aggregation_scheme": "fed_avg"}, **cfg))
        a.gar.gradient_weights = w.copy()
        return a
    aggs = {"qsgd": agg(qsgd_packets=True), "dense-fold": agg(), "wire-qsgd": agg(),
            "qsgd, budget": agg(qsgd_packets=True, device_budget_bytes=budget)}
    sets = {}
    for rnd in range(2):
        grads = [rng.standard_normal(n).astype(F) for _ in range(m)]
        if rnd == 0:
            sets = {name: _round_clients(grads) for name in aggs}
        out = {}
        for name, a in aggs.items():
            cl = sets[name]
            for c, g in zip(cl, grads):
                c.grad = g
            if name == "wire-qsgd":
                a.aggregate_wire([c.C.compress_wire(c.grad) for c in cl])
            else:
                a.aggregate_grads(cl)
            assert a.agg_path == name.split(",")[0] and a.curr_G is None
            assert a.agg_grad.dtype == F and a.agg_grad.shape == (n,)
            out[name] = a.agg_grad.tobytes()
        assert len(set(out.values())) == 1, rnd
        states = [_state(sets[name]) for name in aggs]
        assert all(s == states[0] for s in states), rnd
        assert [c for c, _ in states[0]] == [rnd + 1] * m
        assert [r is not None for _, r in states[0]] == [True, False, True, True, False]
        assert aggs["qsgd, budget"].qsgd_groups == 3 and aggs["qsgd"].qsgd_groups == 1
    # a residual of another length: the round fails before any client advances
    cl = sets["qsgd"]
    before = _state(cl)
    cl[3].C.set_residual(np.zeros(n - 1, F))
    before[3] = (before[3][0], np.zeros(n - 1, F).tobytes())
    with pytest.raises(ValueError, match="reset_residual"):
        aggs["qsgd"].aggregate_grads(cl)
    assert _state(cl) == before
