"""The scaled-sign codec (csrc/fc_sign.hip) and its consumers on an MI355X: codec.encode_sign /
decode_sign / fold_sign / vote_sign / pack_sign / sign_from_host, Compression with 'sign' (and
error feedback), gar.SignMajority, the Aggregator's "sign" and "wire-sign" routes.

Run:  python -m pytest tests/test_sign_gpu.py -m gpu -q

The expected values are tests/sign_model.py's.  Every comparison is bit for bit (the sign of zero
included; NaN positions compare as NaN) except the scale of a normal-random gradient, whose
float64 sum the device makes in its own fixed order: it must lie in the model's range around the
true sum (sign_model.scale_range), and everything else is then exact given the packet's own scale.

Switch points of the kernels the shapes are built around (csrc/fc_sign.hip, not imported):
  a word holds 32 bits, a ballot 64, the packet ends on 4 words: n in {31, 32, 33, 63, 64, 65, 127,
    128, 129}
  k_sign_pack: one wave per 256 elements, a 16-byte load per lane, the last one element by element:
    n = 1 (one lane, three elements short), 8191, 8192, 8193, 3 * 8192 + 37
  k_sign_norm: one workgroup per 1024 elements up to 1024 workgroups, two loads in flight per
    thread, the last arriver adds the partials: n = 1,000,003 (977 workgroups, a 3-element tail)
  k_sign_reduce (fold and vote): one wave per 512 coordinates with all sixteen words present, else
    word pairs past the packet read as zero: n = 8193 (a full tile and a one-coordinate tile) and
    3 * 8192 + 37 (the last tile has 37 coordinates in one word pair of four);
    clients are staged 256 at a time: M in {1, 2, 3, 64, 65, 128, 129, 257};
    the vector form reads four clients per load: M = 1, 2, 3, 65, 129, 257 leave a partial four
"""
import types

import numpy as np
import pytest

import sign_model as sm

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F = np.float32
N3 = 3 * 8192 + 37
NS = (1, 31, 32, 33, 63, 64, 65, 127, 128, 129, 8191, 8192, 8193, N3, 1_000_003)
MS = (1, 2, 3, 64, 65, 128, 129, 257)
FOLD_NS = (8193, N3)


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from openmsftl_amd import _lib
    assert _lib.load().fc_abi_version() == 4
    yield
    _MEMO.clear()
    _lib.load().fc_sign_fold_form(-1)
    torch.cuda.empty_cache()


_MEMO = {}


def memo(key, make):
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


def _codec():
    from openmsftl_amd import codec
    return codec


def dev(a):
    return torch.from_numpy(np.array(a)).cuda()


def host(t):
    return t.cpu().numpy()


def assert_same(got, want, what=""):
    """Bit for bit; NaN positions compare as NaN."""
    got, want = np.asarray(got, F), np.asarray(want, F)
    assert got.shape == want.shape, what
    gn, wn = np.isnan(got), np.isnan(want)
    bad = np.nonzero((gn != wn) | (~gn & ~wn & (got.view(np.uint32) != want.view(np.uint32))))[0]
    assert bad.size == 0, (f"{what}: {bad.size} of {got.size} differ, first at {bad[:5]}: "
                           f"got {got[bad[:5]]} want {want[bad[:5]]}")


def exact_input(n, seed):
    """Integers in [-8, 8] with -0.0 among the zeros: every partial sum of |a| is exact."""
    rng = np.random.default_rng(seed)
    g = rng.integers(-8, 9, n).astype(F)
    z = np.nonzero(g == 0)[0]
    g[z[::2]] = F(-0.0)
    if n >= 2:
        g[0], g[n - 1] = F(-0.0), F(0.0)
    return g


def normal_input(n, seed):
    return np.random.default_rng(seed).standard_normal(n).astype(F)


def words_host(pkt):
    return host(pkt.words).view(np.uint32)


def hdr_bytes(pkt):
    return host(pkt.hdr).tobytes()


def check_packet(pkt, a, e2=None, exact=True, what=""):
    """The packet (and e') of the encoded vector a against the model; returns the packet's s."""
    n = a.size
    h = pkt.header()
    s = F(h.p)
    assert np.float64(s) == h.p or np.isnan(h.p)
    if exact:
        assert s.tobytes() == sm.scale(a).tobytes() or (np.isnan(s) and np.isnan(sm.scale(a))), (what, s, sm.scale(a))
    else:
        lo, hi = sm.scale_range(a)
        assert lo <= s <= hi, (what, lo, s, hi)
    assert hdr_bytes(pkt) == sm.header(n, s).tobytes(), what
    w = words_host(pkt)
    assert w.size == sm.sign_words(n)
    assert w.tobytes() == sm.words_of(sm.bits(a)).tobytes(), what
    q = sm.decode(sm.bits(a), s)
    assert_same(host(_codec().decode_sign(pkt)), q, what + " q")
    if e2 is not None:
        assert_same(host(e2), sm.residual(a, q), what + " e'")
    return s


def fresh_packet(n):
    """A packet whose buffers are pre-filled with 0xFF."""
    p = _codec().SignPacket.alloc(n, torch.device("cuda"))
    p.words.fill_(-1)
    p.hdr.fill_(255)
    return p


# ---- encode / decode / residual ---------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
def test_encode_exact_sum_inputs_equal_the_model(n):
    c = _codec()
    g, e = exact_input(n, n), exact_input(n, n + 1)
    pkt, none = c.encode_sign(dev(g), packet=fresh_packet(n))
    assert none is None
    check_packet(pkt, sm.encoded(g), what=f"n={n} no residual")
    out = torch.full((n,), float("nan"), device="cuda")
    pkt, e2 = c.encode_sign(dev(g), dev(e), residual_out=out, packet=fresh_packet(n))
    assert e2 is out
    check_packet(pkt, sm.encoded(g, e), e2, what=f"n={n} residual")
    pkt, e2 = c.encode_sign(dev(g), residual_out=out, packet=fresh_packet(n))       # e' without e
    check_packet(pkt, sm.encoded(g), e2, what=f"n={n} residual_out only")


@pytest.mark.parametrize("n", NS)
def test_encode_normal_inputs_scale_in_range_rest_exact(n):
    c = _codec()
    g, e = normal_input(n, n), normal_input(n, n + 1) * F(0.5)
    pkt, e2 = c.encode_sign(dev(g), dev(e), packet=fresh_packet(n))
    check_packet(pkt, sm.encoded(g, e), e2, exact=False, what=f"n={n}")
    again, e3 = c.encode_sign(dev(g), dev(e), packet=fresh_packet(n))
    assert hdr_bytes(again) == hdr_bytes(pkt) and words_host(again).tobytes() == words_host(pkt).tobytes()
    assert host(e3).tobytes() == host(e2).tobytes()
    check_packet(c.encode_sign(dev(g))[0], g, exact=False, what=f"n={n} no residual")


@pytest.mark.parametrize("case", ["nan", "inf"])
def test_encode_special_values(case):
    n = 8193
    g = normal_input(n, 3)
    neg_nan = np.array([0xFFC00000], np.uint32).view(F)[0]
    pos_nan = np.array([0x7FC00000], np.uint32).view(F)[0]
    g[[1, 64, 8192]] = [-np.inf, np.inf, -np.inf]
    if case == "nan":
        g[[0, 63, 100, 8191]] = [neg_nan, pos_nan, neg_nan, pos_nan]
    g[[5, 6]] = [F(-0.0), np.array([0x80000001], np.uint32).view(F)[0]]       # -0.0, a negative denormal
    pkt, e2 = _codec().encode_sign(dev(g), residual_out=torch.empty(n, device="cuda"), packet=fresh_packet(n))
    s = check_packet(pkt, g, e2, what=case)
    assert np.isnan(s) if case == "nan" else np.isposinf(s)


def test_residual_of_zeros_differs_only_at_minus_zero():
    n = N3
    g = exact_input(n, 11)
    c = _codec()
    plain = words_host(c.encode_sign(dev(g))[0])
    zeros = words_host(c.encode_sign(dev(g), torch.zeros(n, device="cuda"))[0])
    diff = sm.bits_of(plain, n) != sm.bits_of(zeros, n)
    minus_zero = g.view(np.uint32) == 0x80000000
    assert minus_zero.sum() > 100 and (diff == minus_zero).all()


def test_unaligned_input_through_compression():
    from openmsftl_amd import Compression
    n = 8191
    base = dev(exact_input(n + 1, 13))
    view = base[1:]
    assert view.data_ptr() % 16 != 0
    C = Compression({"compression_function": "sign"})
    q = C.compress(view)
    g = host(view)
    assert q.is_cuda and q.dtype == torch.float32
    assert_same(host(q), sm.encode(g)[3], "tensor view")
    qn = C.compress(g)                                                     # the NumPy kind
    assert isinstance(qn, np.ndarray) and qn.dtype == F
    assert_same(qn, sm.encode(g)[3], "numpy")
    assert host(view).tobytes() == g.tobytes()                             # the input untouched
    with pytest.raises(NotImplementedError, match="float32"):
        C.compress(np.zeros(8, np.float64))
    empty = C.compress(np.zeros(0, F))
    assert isinstance(empty, np.ndarray) and empty.shape == (0,) and empty.dtype == F
    assert C.compress(torch.zeros(0, device="cuda")).shape == (0,)
    with pytest.raises(ValueError, match="empty"):
        C.compress_wire(np.zeros(0, F))


# ---- error feedback through Compression -------------------------------------------------------
def _scale_of(q):
    return F(np.abs(q[0]))


def test_error_feedback_five_rounds_against_the_model():
    from openmsftl_amd import Compression
    n = N3
    C = Compression({"compression_function": "sign", "error_feedback": True})
    W = Compression({"compression_function": "sign", "error_feedback": True})
    assert C.get_residual() is None
    e = np.zeros(n, F)
    for r in range(5):
        g = normal_input(n, 100 + r)
        q = C.compress(g)
        a = sm.encoded(g, e)
        s = _scale_of(q)
        lo, hi = sm.scale_range(a)
        assert lo <= s <= hi, (r, lo, s, hi)
        _, _, words, qm, e = sm.encode(g, e, s=s)
        assert_same(q, qm, f"round {r} q")
        got = C.get_residual()
        assert isinstance(got, np.ndarray)
        assert_same(got, e, f"round {r} residual")
        raw = W.compress_wire(g)                                           # the same state, the wire form
        assert raw == sm.pack(n, s, words), f"round {r} wire"
        assert_same(W.get_residual(), e, f"round {r} residual after compress_wire")
    # set / get / reset and the length-change error
    snap = C.get_residual()
    g = normal_input(n, 200)
    q1 = C.compress(g)
    C.set_residual(snap)
    q2 = C.compress(g)
    assert q1.tobytes() == q2.tobytes()
    with pytest.raises(ValueError, match="reset_residual"):
        C.compress(np.zeros(n + 1, F))
    assert_same(C.get_residual(), sm.encode(g, snap, s=_scale_of(q2))[4], "unchanged by the failed call")
    C.reset_residual()
    assert C.get_residual() is None
    q = C.compress(exact_input(n + 1, 7))
    assert_same(q, sm.encode(exact_input(n + 1, 7), np.zeros(n + 1, F))[3], "after reset")
    t = C.compress(dev(exact_input(n + 1, 8)))                             # the tensor kind
    assert t.is_cuda and isinstance(C.get_residual(), torch.Tensor)


# ---- hand-built packets ----------------------------------------------------------------------------
def hand_packet(n, bits, s):
    c = _codec()
    return c.SignPacket(words=dev(sm.words_of(bits).view(np.int32)),
                        hdr=dev(np.frombuffer(sm.header(n, s).tobytes(), dtype=np.uint8)), n=n)


def fold_case(m, n, special=None):
    """(bit rows, scales, weights, decoded rows, packets): client 0 has a zero scale and every bit
    set (its row is -0.0 everywhere: pins the rule for the first row), client 1 a weight of 0."""
    def make():
        rng = np.random.default_rng(1000 * m + n % 997)
        B = rng.integers(0, 2, (m, n)).astype(bool)
        s = (rng.random(m).astype(F) + F(0.25)) * F(0.01)
        w = (rng.random(m).astype(F) + F(0.5)) / F(m)
        B[0], s[0] = True, F(0.0)
        if m > 1:
            w[1] = F(0.0)
        if special == "nan" and m > 2:
            s[2] = F(np.nan)
        if special == "inf" and m > 2:
            s[2] = F(np.inf)                                               # inf * 0 weight elsewhere is fine
        rows = np.stack([sm.decode(B[i], s[i]) for i in range(m)])
        return B, s, w, rows, [hand_packet(n, B[i], s[i]) for i in range(m)]
    return memo(("fold", m, n, special), make)


def both_forms(fn):
    """fn() under every word-loading form: scalar loads, vector loads and v_readlane, a word per lane."""
    from openmsftl_amd import _lib
    lib = _lib.load()
    out = []
    try:
        for form in (0, 1, 2):
            assert lib.fc_sign_fold_form(form) == 0
            out.append(fn())
    finally:
        lib.fc_sign_fold_form(-1)
    return out


@pytest.mark.parametrize("n", FOLD_NS)
@pytest.mark.parametrize("m", MS)
def test_fold_equals_the_dense_fedavg_of_the_decoded_rows(m, n):
    c = _codec()
    B, s, w, rows, pk = fold_case(m, n)
    want = sm.fold(rows, w)
    for got in both_forms(lambda: host(c.fold_sign(pk, w, out=torch.full((n,), float("nan"), device="cuda")))):
        assert_same(got, want, f"M={m} n={n} vs NumPy")
    dense = c.weighted_sum_dense(dev(rows), torch.from_numpy(w))
    assert_same(host(c.fold_sign(pk, w)), host(dense), "vs weighted_sum_dense")
    # a round cut into groups continues to the bits of one call
    for group in (1, 7, 128):
        out = torch.full((n,), float("nan"), device="cuda")
        for s0 in range(0, m, group):
            c.fold_sign(pk[s0:s0 + group], w[s0:s0 + group], out=out, continue_sum=s0 > 0)
        assert_same(host(out), want, f"M={m} n={n} groups of {group}")


@pytest.mark.parametrize("special", ["nan", "inf"])
def test_fold_with_a_non_finite_scale(special):
    c = _codec()
    m, n = 5, 8193
    B, s, w, rows, pk = fold_case(m, n, special)
    want = sm.fold(rows, w)
    assert np.isnan(want).all() if special == "nan" else np.isinf(want).all()
    for got in both_forms(lambda: host(c.fold_sign(pk, w))):
        assert_same(got, want, special)
    assert_same(host(c.weighted_sum_dense(dev(rows), torch.from_numpy(w))), want, special + " dense")


def test_fold_and_vote_argument_checks():
    c = _codec()
    _, _, w, _, pk = fold_case(3, 8193)
    with pytest.raises(ValueError, match="one weight per packet"):
        c.fold_sign(pk, w[:2])
    with pytest.raises(ValueError, match="continue_sum"):
        c.fold_sign(pk, w, continue_sum=True)
    with pytest.raises(ValueError, match="share n"):
        c.fold_sign(pk + fold_case(1, N3)[4], [1.0] * 4)
    with pytest.raises(ValueError, match="no packets"):
        c.vote_sign([], 1.0)
    with pytest.raises(TypeError, match="sign packets"):
        c.vote_sign([object()], 1.0)


# ---- vote --------------------------------------------------------------------------------------
SPOTS = (0, 31, 32, 63, 64, 8191, 8192, -1)


def vote_case(m, n, rot):
    """Random columns, and at SPOTS hand-built ones: all negative, all positive, neg = M // 2 (the
    exact tie at even M) and neg = M // 2 + 1; ``rot`` turns the kinds over the spots."""
    def make():
        rng = np.random.default_rng(77 * m + rot)
        B = rng.integers(0, 2, (m, n)).astype(bool)
        kinds = {}
        for i, spot in enumerate(SPOTS):
            kind = (i + rot) % 4
            neg = (m, 0, m // 2, min(m, m // 2 + 1))[kind]
            col = np.zeros(m, bool)
            col[rng.permutation(m)[:neg]] = True
            B[:, spot] = col
            kinds[spot % n] = neg
        return B, kinds, [hand_packet(n, B[i], F(i + 1)) for i in range(m)]
    return memo(("vote", m, n, rot), make)


@pytest.mark.parametrize("n", FOLD_NS)
@pytest.mark.parametrize("m", MS)
def test_vote_counts_bits(m, n):
    c = _codec()
    eta = F(0.37)
    for rot in range(4):
        B, kinds, pk = vote_case(m, n, rot)
        want = sm.vote(B, eta)
        for spot, neg in kinds.items():
            assert want[spot].tobytes() == (F(-eta) if 2 * neg > m else eta if 2 * neg < m else F(0.0)).tobytes()
        for got in both_forms(lambda: host(c.vote_sign(pk, eta, out=torch.full((n,), float("nan"), device="cuda")))):
            assert_same(got, want, f"M={m} n={n} rot={rot}")
        if rot == 0 and m > 1:                                             # any client order
            assert_same(host(c.vote_sign(pk[::-1], eta)), want, "reversed")


def test_vote_of_five_with_two_flipped_returns_the_honest_signs():
    n = N3
    g = normal_input(n, 21)
    honest = sm.bits(g)
    pk = [hand_packet(n, honest if i < 3 else ~honest, F(1.0 + i)) for i in range(5)]
    got = host(_codec().vote_sign(pk, 0.5))
    assert_same(got, sm.decode(honest, F(0.5)), "honest signs")


# ---- wire and Aggregator -------------------------------------------------------------------------
def test_pack_sign_and_sign_from_host_round_trip():
    c = _codec()
    for n in (1, 33, 129, N3):
        g = exact_input(n, 31 + n)
        pkt, _ = c.encode_sign(dev(g))
        raw = host(c.pack_sign(pkt)).tobytes()
        assert raw == sm.pack(n, sm.scale(g), sm.words_of(sm.bits(g))), n
        back = c.sign_from_host(raw, n)
        assert back.n == n and hdr_bytes(back) == hdr_bytes(pkt)
        assert words_host(back).tobytes() == words_host(pkt).tobytes()
        assert_same(host(c.decode_sign(back)), sm.encode(g)[3], "round trip")
        assert c.sign_from_host(np.frombuffer(raw, np.uint8)).n == n
        bad = bytearray(raw)
        bad[-1] |= 0x80                                                    # a pad bit (or a bit past n)
        before = torch.cuda.memory_allocated()
        with pytest.raises(ValueError, match="sign wire"):
            c.sign_from_host(bytes(bad), n)
        assert torch.cuda.memory_allocated() == before                     # nothing was uploaded
        with pytest.raises(ValueError, match="expected"):
            c.sign_from_host(raw, n + 1)


def _clients(grads, **cfg):
    from openmsftl_amd import Compression
    return [types.SimpleNamespace(C=Compression(dict({"compression_function": "sign"}, **cfg)), grad=g,
                                  client_id=i) for i, g in enumerate(grads)]


def _agg(scheme="fed_avg", **cfg):
    from openmsftl_amd.aggregation import Aggregator
    return Aggregator(dict({"aggregation_scheme": scheme}, **cfg))


def test_aggregate_grads_sign_route_equals_dense_fold_and_the_model():
    m, n = 5, N3
    grads = [exact_input(n, 40 + i) for i in range(m)]
    rows = np.stack([sm.encode(g)[3] for g in grads])
    w = (np.arange(m, dtype=F) + F(1.0)) / F(16.0)
    want = sm.fold(rows, w)
    a = _agg()
    a.gar.gradient_weights = w.copy()
    a.aggregate_grads(_clients(grads))
    assert a.agg_path == "sign" and a.curr_G is None and a.sign_groups == 1
    assert_same(a.agg_grad, want, "sign route vs model")
    b = _agg(sign_packets=False)
    b.gar.gradient_weights = w.copy()
    b.aggregate_grads(_clients(grads))
    assert b.agg_path == "dense-fold"
    assert_same(b.agg_grad, want, "dense-fold vs model")
    # a budget that holds two packets beside the aggregate and one gradient: three fold groups
    from openmsftl_amd.aggregation import sign_packet_bytes
    c = _agg(device_budget_bytes=8 * n + 2 * sign_packet_bytes(n))
    c.gar.gradient_weights = w.copy()
    c.aggregate_grads(_clients(grads))
    assert c.agg_path == "sign" and c.sign_groups == 3
    assert_same(c.agg_grad, want, "three groups")
    # default weights 1 / M, and the wire route on the same clients
    d, e = _agg(), _agg()
    d.aggregate_grads(_clients(grads))
    e.aggregate_wire([cl.C.compress_wire(cl.grad) for cl in _clients(grads)])
    assert e.agg_path == "wire-sign"
    assert_same(d.agg_grad, sm.fold(rows, np.full(m, 1.0 / m, F)), "default weights")
    assert_same(e.agg_grad, d.agg_grad, "wire-sign")
    f = _agg(device_budget_bytes=4 * n + 2 * ((sm.wire_bytes(n) + 255) & ~255))
    f.aggregate_wire([cl.C.compress_wire(cl.grad) for cl in _clients(grads)], n=n)
    assert_same(f.agg_grad, d.agg_grad, "wire-sign in groups")


def test_aggregate_grads_with_error_feedback_over_three_rounds():
    from openmsftl_amd import Compression
    m, n = 4, N3
    a, b, s3 = _agg(), _agg(sign_packets=False), _agg(device_budget_bytes=8 * n + 4096)
    ca, cb, cc = (_clients([None] * m, error_feedback=True) for _ in range(3))
    replay = [Compression({"compression_function": "sign", "error_feedback": True}) for _ in range(m)]
    for r in range(3):
        grads = [normal_input(n, 500 + 10 * r + i) for i in range(m)]
        for cl in (ca, cb, cc):
            for c, g in zip(cl, grads):
                c.grad = g
        a.aggregate_grads(ca)
        b.aggregate_grads(cb)
        s3.aggregate_grads(cc)
        assert (a.agg_path, b.agg_path, s3.agg_path) == ("sign", "dense-fold", "sign") and s3.sign_groups == m
        rows = np.stack([C.compress(g) for C, g in zip(replay, grads)])    # checked against the model above
        want = sm.fold(rows, np.full(m, 1.0 / m, F))
        assert_same(a.agg_grad, want, f"round {r} sign")
        assert_same(b.agg_grad, want, f"round {r} dense-fold")
        assert_same(s3.agg_grad, want, f"round {r} one packet per group")
        for x, y, z, C in zip(ca, cb, cc, replay):                         # each residual advanced once
            assert_same(x.C.get_residual(), C.get_residual(), f"round {r} residual")
            assert_same(host(y.C.get_residual()), C.get_residual(), f"round {r} residual")   # fed a tensor
            assert_same(z.C.get_residual(), C.get_residual(), f"round {r} residual")
    # a client whose residual has another length: the round raises before any residual advances
    before = [c.C.get_residual() for c in ca]
    ca[2].C.set_residual(np.zeros(n + 1, F))
    before[2] = ca[2].C.get_residual()
    with pytest.raises(ValueError, match="reset_residual"):
        a.aggregate_grads(ca)
    for c, e in zip(ca, before):
        assert_same(c.C.get_residual(), e, "no residual advanced")


def test_sign_majority_through_aggregate_grads_and_aggregate_wire():
    m, n = 6, N3
    grads = [exact_input(n, 60 + i) * F(i + 1) for i in range(m)]         # scales 1x .. 6x: still exact sums
    B = np.stack([sm.bits(g) for g in grads])
    scales = [sm.scale(g) for g in grads]
    want = sm.vote(B, sm.majority_eta(scales))
    assert (want == 0).any() and (want > 0).any() and (want < 0).any()
    a = _agg("sign_majority")
    a.aggregate_grads(_clients(grads))
    assert a.agg_path == "sign" and a.gar.eta.tobytes() == sm.majority_eta(scales).tobytes()
    assert_same(a.agg_grad, want, "aggregate_grads")
    b = _agg("sign_majority")
    b.aggregate_wire([cl.C.compress_wire(cl.grad) for cl in _clients(grads)])
    assert b.agg_path == "wire-sign"
    assert_same(b.agg_grad, want, "aggregate_wire")
    c = _agg("sign_majority", majority_scale=0.125)
    c.aggregate_grads(_clients(grads[:5]))
    assert c.gar.eta == F(0.125)
    assert_same(c.agg_grad, sm.vote(B[:5], F(0.125)), "majority_scale")
    # the packets do not fit: the vote needs all of them
    from openmsftl_amd.aggregation import sign_packet_bytes
    small = 8 * n + 3 * sign_packet_bytes(n)
    with pytest.raises(NotImplementedError, match="device_budget_bytes"):
        _agg("sign_majority", device_budget_bytes=small).aggregate_grads(_clients(grads))
    with pytest.raises(NotImplementedError, match="device_budget_bytes"):
        _agg("sign_majority", device_budget_bytes=4 * n + 3 * sign_packet_bytes(n)).aggregate_wire(
            [cl.C.compress_wire(cl.grad) for cl in _clients(grads)])
    # no finite scale
    nan = [np.full(n, np.nan, F)] * 2
    with pytest.raises(ValueError, match="finite scale"):
        _agg("sign_majority").aggregate_grads(_clients(nan))
