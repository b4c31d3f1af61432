"""fc_sign_trim (csrc/fc_sign_trim.hip) and its consumers (codec.trimmed_mean_sign,
gar.CoordinateTrim, the Aggregator's "sign-trim" routes) on an MI355X.

Run:  python -m pytest tests/test_sign_trim_gpu.py -m gpu -q

Packets are built on the host from hand-made bits and scales (sign_model.pack) and uploaded through
the validator (codec.sign_from_host).  Every result is compared BIT FOR BIT (NaN positions as NaN)
with tests/sign_trim_model.py's ``expected``: trim_model.trimmed_mean_model on the rows
sign_model.decode makes.  The order of the float32 adds is part of the definition, so there is
nothing to tolerate.
"""
import types

import numpy as np
import pytest

import sign_geometry_model as gm
import sign_model as sm
import sign_trim_model as stm

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F = np.float32
NS = (1, 31, 32, 33, 127, 128, 129, 8191, 8193)
MS = (1, 2, 3, 4, 63, 64, 65, 127, 128)
BIG = 1_000_003
SENTINEL = -123.0


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from openmsftl_amd import _lib
    assert _lib.load().fc_abi_version() == 4
    yield
    torch.cuda.empty_cache()


def _codec():
    from openmsftl_amd import codec
    return codec


def host(t):
    return t.cpu().numpy()


def same_bits(got, want, what=""):
    """Bit for bit; NaN positions compare as NaN."""
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype == F, what
    gn, wn = np.isnan(got), np.isnan(want)
    bad = np.argwhere((gn != wn) | (~gn & ~wn & (got.view(np.uint32) != want.view(np.uint32))))
    assert bad.size == 0, (f"{what}: {len(bad)} of {got.size} differ, first at {bad[:4].tolist()}: "
                           f"got {[got[tuple(b)] for b in bad[:4]]} want {[want[tuple(b)] for b in bad[:4]]}")


def upload(B, s):
    c = _codec()
    return [c.sign_from_host(raw) for raw in gm.packets(B, s)]


def raw_packets(B, s):
    """Packets made of device tensors directly, past the validator (which refuses a negative
    scale): the words and the canonical header of sign_model."""
    c = _codec()
    n = B.shape[1]
    return [c.SignPacket(words=torch.from_numpy(sm.words_of(b).view(np.int32)).cuda(),
                         hdr=torch.from_numpy(np.frombuffer(sm.header(n, x).tobytes(), np.uint8).copy()).cuda(),
                         n=n) for b, x in zip(B, np.asarray(s, F))]


def trim_call(pk, b):
    """codec.trimmed_mean_sign into a sentinel-filled tensor."""
    out = torch.full((pk[0].n,), SENTINEL, dtype=torch.float32, device="cuda")
    assert _codec().trimmed_mean_sign(pk, b, out=out) is out
    return host(out)


def random_bits(m, n, seed):
    """p = 0.5 rows; client 1 has every bit set and client 2 none (as far as m reaches)."""
    rng = np.random.default_rng(seed)
    B = rng.random((m, n), dtype=F) < 0.5
    if m > 1:
        B[1] = True
    if m > 2:
        B[2] = False
    return B


# ---- shapes -------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
@pytest.mark.parametrize("m", MS)
def test_shapes_equal_the_model_bit_for_bit(m, n):
    rng = np.random.default_rng(1000 * m + n)
    B = random_bits(m, n, 7 * m + n)
    s = stm.SCALES["distinct"](m, rng, 0)
    pk = upload(B, s)
    perm = rng.permutation(m)
    for b in stm.trims(m):
        want = stm.expected(B, s, b)
        got = trim_call(pk, b)
        same_bits(got, want, f"m={m} n={n} b={b}")
        same_bits(trim_call(pk, b), got, f"m={m} n={n} b={b} second call")
        same_bits(trim_call([pk[i] for i in perm], b), got, f"m={m} n={n} b={b} clients permuted")


@pytest.mark.parametrize("m,b", [(3, 1), (128, 31)])
def test_a_million_coordinates(m, b):
    B = random_bits(m, BIG, m)
    s = stm.SCALES["distinct"](m, np.random.default_rng(m), b)
    same_bits(trim_call(upload(B, s), b), stm.expected(B, s, b), f"m={m} n={BIG} b={b}")


# ---- scales and bits ----------------------------------------------------------------------------
def case_bits(m, rng):
    """p = 0.5 columns, all-set columns, all-clear columns and the window's edges (every count of
    negatives from 0 to m), side by side; n is no multiple of 32."""
    B = np.concatenate([rng.random((m, 301)) < 0.5, np.ones((m, 33), bool), np.zeros((m, 33), bool),
                        stm.edge_bits(m, 2 * (m + 1) + 3, rng)], axis=1)
    assert B.shape[1] % 32
    return B


@pytest.mark.parametrize("scales", sorted(stm.SCALES))
@pytest.mark.parametrize("m", [4, 9, 65, 128])
def test_scale_and_bit_cases_equal_the_model_bit_for_bit(m, scales):
    rng = np.random.default_rng(31 * m + len(scales))
    B = case_bits(m, rng)
    for b in stm.trims(m):
        s = stm.SCALES[scales](m, rng, b)
        want = stm.expected(B, s, b)
        same_bits(trim_call(upload(B, s), b), want, f"m={m} b={b} {scales}")
        if scales == "nan_in_b":
            assert not np.isnan(want[:301]).any()                      # b NaNs are all trimmed
        if scales == "nan_in_b_plus_1":
            assert np.isnan(want).all()                                # one survives in every column
        if scales == "mixed_magnitudes" and b == 0 and m in (9, 128):
            # the order of the adds shows: where the +-1e8 cancel, adding by descending magnitude
            # keeps the +-1 that the ascending order loses beside 1e8, so the bits differ (at these
            # two m the drawn scales hold an even count of 1e8, so such columns exist)
            G = stm.decoded(B, s)
            G = np.take_along_axis(G, np.argsort(-np.abs(G), axis=0, kind="stable"), axis=0)
            other = np.zeros(G.shape[1], F)
            for row in G:
                other = np.add(other, row, dtype=F)
            other = np.divide(other, F(m), dtype=F)
            assert (other.view(np.uint32) != want.view(np.uint32)).any()


def test_scales_with_the_sign_bit_set_are_taken_as_they_stand():
    rng = np.random.default_rng(11)
    m = 9
    B = case_bits(m, rng)
    s = stm.SCALES["tie_groups"](m, rng, 0)
    s[[1, 4, 6]] *= F(-1.0)
    s[2], s[7] = F(-0.0), -np.inf
    pk = raw_packets(B, s)
    for b in stm.trims(m):
        same_bits(trim_call(pk, b), stm.expected(B, s, b), f"b={b}")


@pytest.mark.parametrize("m", [1, 2, 7, 8, 64, 65, 127, 128])
def test_median_of_equal_scales_is_the_majority_vote(m):
    c = _codec()
    n, eta = 8193, F(0.375)
    rng = np.random.default_rng(50 + m)
    B = np.concatenate([rng.random((m, n - 2 * (m + 1))) < 0.5, stm.edge_bits(m, 2 * (m + 1), rng)], axis=1)
    pk = upload(B, np.full(m, eta, F))
    got = trim_call(pk, (m - 1) // 2)
    same_bits(got, host(c.vote_sign(pk, float(eta))), f"m={m} against vote_sign")
    same_bits(got, sm.vote(B, eta), f"m={m} against the vote's model")
    if m % 2 == 0:
        tie = B.sum(axis=0) * 2 == m
        assert tie.any() and (got[tie].view(np.uint32) == 0).all()     # a tie gives +0.0


def test_out_is_honoured_and_a_wrong_out_raises():
    c = _codec()
    m, n, b = 5, 129, 1
    B = random_bits(m, n, 3)
    s = stm.SCALES["distinct"](m, np.random.default_rng(4), b)
    pk = upload(B, s)
    want = stm.expected(B, s, b)
    same_bits(host(c.trimmed_mean_sign(pk, b)), want, "allocated out")
    big = torch.full((n + 8,), SENTINEL, dtype=torch.float32, device="cuda")
    base = torch.full((64 + n,), SENTINEL, dtype=torch.float32, device="cuda")
    out = base[64:]                                                    # 256 bytes in: aligned
    assert c.trimmed_mean_sign(pk, b, out=out) is out
    same_bits(host(out), want, "given out")
    assert (host(base[:64]) == F(SENTINEL)).all()
    for bad in (big, base[1:1 + n], torch.empty(n, dtype=torch.float64, device="cuda"),
                torch.empty(n, dtype=torch.float32), torch.empty((n, 2), device="cuda")[:, 0],
                host(out)):
        with pytest.raises(ValueError, match="out must be"):
            c.trimmed_mean_sign(pk, b, out=bad)
    with pytest.raises(ValueError, match=r"2 \* trim"):
        c.trimmed_mean_sign(pk, 3)
    from openmsftl_amd import gar
    rule = gar.CoordinateMedian({})
    same_bits(host(rule.aggregate_packets(pk)), stm.expected(B, s, 2), "CoordinateMedian")
    assert rule.trim == 2


# ---- the Aggregator -----------------------------------------------------------------------------
def _clients(grads, **cfg):
    from openmsftl_amd import Compression
    return [types.SimpleNamespace(C=Compression(dict({"compression_function": "sign"}, **cfg)), grad=g,
                                  client_id=i) for i, g in enumerate(grads)]


def _agg(scheme, **cfg):
    from openmsftl_amd.aggregation import Aggregator
    return Aggregator(dict({"aggregation_scheme": scheme}, **cfg))


RULES = [("trimmed_mean", {"trim_count": 2}, 2), ("coordinate_median", {}, 4)]


def round_grads(m, n, seed):
    rng = np.random.default_rng(seed)
    base = rng.standard_normal(n)
    return [((base + 0.5 * rng.standard_normal(n)) * (1 + i % 3)).astype(F) for i in range(m)]


@pytest.mark.parametrize("scheme,cfg,b", RULES)
def test_aggregator_sign_trim_routes(scheme, cfg, b):
    from openmsftl_amd import gar
    c = _codec()
    m, n = 9, 1000
    grads = round_grads(m, n, 70)
    pk = [c.encode_sign(torch.from_numpy(g).cuda())[0] for g in grads]
    want = host(c.trimmed_mean_sign(pk, b))
    scales = F([p.scale() for p in pk])
    same_bits(want, stm.expected(np.stack([sm.bits(g) for g in grads]), scales, b), "the model")
    sigma = gar.gram_singular_values(host(c.gram_sign(pk)))
    a = _agg(scheme, sign_trim=True, pc_analysis="gram", **cfg)
    a.aggregate_grads(_clients(grads))
    assert a.agg_path == "sign-trim" and a.curr_G is None and a.gar.trim == b
    same_bits(a.agg_grad, want, f"{scheme} sign-trim")
    assert len(a.gar.Sigma_tracked) == 1 and np.array_equal(a.gar.Sigma_tracked[-1], sigma)
    w = _agg(scheme, sign_trim=True, pc_analysis="gram", **cfg)
    w.aggregate_wire([cl.C.compress_wire(cl.grad) for cl in _clients(grads)])
    assert w.agg_path == "wire-sign-trim" and w.curr_G is None and w.gar.trim == b
    same_bits(w.agg_grad, a.agg_grad, f"{scheme} wire-sign-trim")
    assert len(w.gar.Sigma_tracked) == 1 and np.array_equal(w.gar.Sigma_tracked[-1], sigma)
    plain = _agg(scheme, sign_trim=True, **cfg)                        # no Gram matrix without pc_analysis
    plain.aggregate_grads(_clients(grads))
    same_bits(plain.agg_grad, want, f"{scheme} without pc_analysis")
    assert plain.gar.Sigma_tracked == []
    with pytest.raises(NotImplementedError, match="no consumer of sign packets"):
        _agg(scheme, **cfg).aggregate_grads(_clients(grads))           # the key is opt-in


@pytest.mark.parametrize("scheme,cfg,b", RULES)
def test_aggregator_sign_trim_with_error_feedback_over_two_rounds(scheme, cfg, b):
    c = _codec()
    m, n = 9, 1000
    a = _agg(scheme, sign_trim=True, **cfg)
    clients = _clients([None] * m, error_feedback=True)
    res = [torch.zeros(n, dtype=torch.float32, device="cuda") for _ in range(m)]
    for r in range(2):
        grads = round_grads(m, n, 80 + r)
        pk = []
        for i, g in enumerate(grads):                                  # the manual loop
            p, res[i] = c.encode_sign(torch.from_numpy(g).cuda(), res[i])
            pk.append(p)
        for cl, g in zip(clients, grads):
            cl.grad = g
        a.aggregate_grads(clients)
        assert a.agg_path == "sign-trim"
        same_bits(a.agg_grad, host(c.trimmed_mean_sign(pk, b)), f"round {r}")
        for i, cl in enumerate(clients):                               # each residual advanced once
            same_bits(np.asarray(cl.C.get_residual()), host(res[i]), f"round {r} residual {i}")
    with pytest.raises(NotImplementedError, match=r"sign-trim route .*device_budget_bytes"):
        _agg(scheme, sign_trim=True, device_budget_bytes=4096, **cfg).aggregate_grads(clients)
