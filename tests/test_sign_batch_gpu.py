"""The batched scaled-sign encode (fc_sign_encode_batch, codec.encode_sign_batch) and the
Aggregator's "batched_sign_encode" key on an MI355X.

Run:  python -m pytest tests/test_sign_batch_gpu.py -m gpu -q

The oracle everywhere is the lone codec.encode_sign on the same tensors (what there was before):
header (all 96 bytes), words (all fc_sign_words(n), pads included) and the new residual compare
with .tobytes() equality, never with a tolerance.  Inputs come from tests/sign_model.py's kind.

Switch points of the kernels the shapes are built around (csrc/fc_sign.hip, not imported):
  a float4 per lane, a tile of 256 elements per wave, the n % 4 tail elements' bits from the lane
    that owns float4 index n / 4, a tile in which no lane holds a whole float4 (n / 4 a multiple of
    64, n % 4 > 0): n in {1, 3, 4, 5, 255, 256, 257, 259, 1023, 1024, 1027, 8193}
  the grid reaches 1024 workgroups at n = 2^20 and the grid-stride loop starts: n in {2^20,
    2^20 + 1, 2^20 + 4, 2^20 + 259}; a second step for some waves only: 2 * 2^20 + 1028 + 3; the
    two-tiles-in-flight loop with a lone third step: 3 * 2^20 + 1029 + 2
  client = blockIdx.y, a workspace slot per client: m in {1, 2, 3, 65}
"""
import types

import numpy as np
import pytest

import sign_model as sm

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

F = np.float32
M20 = 1 << 20
SMALL_NS = (1, 3, 4, 5, 255, 256, 257, 259, 1023, 1024, 1027, 8193)
LARGE_NS = (M20, M20 + 1, M20 + 4, M20 + 259, 2 * M20 + 1028 + 3, 3 * M20 + 1029 + 2)
SMALL_MS = (1, 2, 3, 65)
COMBOS = ((False, False), (True, False), (False, True), (True, True))       # (res_in, res_out)
CASES = [(n, m) for n in SMALL_NS for m in SMALL_MS] + [(n, 3) for n in LARGE_NS]


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


DEV = "cuda"


def inputs(n, m, seed):
    """m different gradients and residuals of n elements on the device: normal values with -0.0,
    +0.0 and exact cancellations (g + e = +0.0) sprinkled in."""
    gen = torch.Generator(device=DEV).manual_seed(seed)
    g = torch.randn((m, n), device=DEV, generator=gen)
    e = torch.randn((m, n), device=DEV, generator=gen) * 0.5
    g[:, ::7] = -0.0
    e[:, ::14] = 0.0
    e[:, 3::11] = -g[:, 3::11]
    return _rows(g), _rows(e)


def _rows(t):
    """Row tensors with 16-byte aligned storage of their own (a row of an (m, n) block is aligned
    only when 4 n is a multiple of 16)."""
    return [r.clone() for r in t]


def fresh(n, m):
    """m packets whose buffers are pre-filled with 0xFF."""
    out = [_codec().SignPacket.alloc(n, torch.device(DEV)) for _ in range(m)]
    for p in out:
        assert p.words.numel() == sm.sign_words(n)          # blob() compares all of them
        p.words.fill_(-1)
        p.hdr.fill_(255)
    return out


def garbage(n, m):
    return [torch.full((n,), float("nan"), device=DEV) for _ in range(m)]


def blob(packets, res):
    """Everything a call wrote, as bytes per client."""
    return [(p.hdr.cpu().numpy().tobytes(), p.words.cpu().numpy().tobytes(),
             None if res is None else res[i].cpu().numpy().tobytes()) for i, p in enumerate(packets)]


def lone(grads, residuals, want):
    """The oracle: one codec.encode_sign per client."""
    c, n, m = _codec(), grads[0].numel(), len(grads)
    pk, out = fresh(n, m), garbage(n, m) if want else None
    for i in range(m):
        c.encode_sign(grads[i], None if residuals is None else residuals[i],
                      out[i] if want else None, packet=pk[i])
    return blob(pk, out)


def batched(grads, residuals, want, **kw):
    c, n, m = _codec(), grads[0].numel(), len(grads)
    pk = fresh(n, m)
    out = garbage(n, m) if want else None
    got_pk, got_res = c.encode_sign_batch(grads, residuals, out, want_residuals=want, packets=pk, **kw)
    assert [p is q for p, q in zip(got_pk, pk)] == [True] * m
    assert (got_res is None) == (not want)
    if want:
        assert [a is b for a, b in zip(got_res, out)] == [True] * m
    return blob(pk, out)


def assert_blobs(got, want, what):
    assert len(got) == len(want)
    for i, (a, b) in enumerate(zip(got, want)):
        for part, x, y in zip(("header", "words", "residual"), a, b):
            assert x == y, f"{what}: client {i}: {part} differs from the lone call's"


@pytest.mark.parametrize("n,m", CASES)
def test_batch_equals_the_lone_calls_in_all_four_forms(n, m):
    grads, res = inputs(n, m, 100 + n % 1000 + m)
    for res_in, want in COMBOS:
        r = res if res_in else None
        ref = lone(grads, r, want)
        assert_blobs(batched(grads, r, want), ref, f"n={n} m={m} res_in={res_in} res_out={want}")
        # the same cached workspace again: the tickets cleaned themselves
        assert_blobs(batched(grads, r, want), ref, f"n={n} m={m} res_in={res_in} res_out={want} second call")


@pytest.mark.parametrize("n", (1027, M20 + 259))
def test_three_clients_after_sixty_five_on_the_same_workspace(n):
    grads, res = inputs(n, 65, 7 + n % 100)
    for res_in, want in COMBOS:
        batched(grads, res if res_in else None, want)
        r = res[:3] if res_in else None
        assert_blobs(batched(grads[:3], r, want), lone(grads[:3], r, want), f"n={n} m=3 after m=65")


def specials(n):
    neg_nan = np.array([0xFFC00000], np.uint32).view(F)[0]
    pos_nan = np.array([0x7FC00000], np.uint32).view(F)[0]
    den = np.array([0x80000001], np.uint32).view(F)[0]
    spots = (0, 5, 63, 64, 255, 256, n - 1)
    return spots, (neg_nan, pos_nan, F(-np.inf), F(np.inf), F(-0.0), den, neg_nan)


@pytest.mark.parametrize("n", (1027, M20 + 259))
def test_special_values_in_one_client_of_three(n):
    grads, res = inputs(n, 3, 31)
    clean = lone(grads, res, True)
    spots, values = specials(n)
    g1 = grads[1].cpu().numpy()
    for rot in range(2):                         # every value lands on two different spots
        for s, v in zip(spots, values[rot:] + values[:rot]):
            g1[s] = v
        grads[1] = torch.from_numpy(g1).to(DEV)
        res[1][list(spots)] = 0.0                # the add keeps them (and turns -0.0 into +0.0)
        for res_in, want in COMBOS:
            r = res if res_in else None
            ref = lone(grads, r, want)
            got = batched(grads, r, want)
            assert_blobs(got, ref, f"n={n} specials res_in={res_in} res_out={want}")
            if res_in and want:                  # the neighbours' outputs are unaffected
                assert got[0] == clean[0] and got[2] == clean[2]
    # -0.0 without a residual keeps its sign bit; with a zero residual the add clears it
    w_plain = np.frombuffer(batched(grads, None, False)[1][1], np.uint32)
    w_res = np.frombuffer(batched(grads, res, False)[1][1], np.uint32)
    at = [s for s, v in zip(spots, values[1:] + values[:1]) if v.tobytes() == F(-0.0).tobytes()][0]
    assert (w_plain[at // 32] >> (at % 32)) & 1 == 1 and (w_res[at // 32] >> (at % 32)) & 1 == 0


@pytest.mark.parametrize("n", (8193, M20 + 259))
def test_error_feedback_over_four_rounds_swapping_the_buffers(n):
    c, m = _codec(), 3
    e_lone = [torch.zeros(n, device=DEV) for _ in range(m)]
    e_bat = [torch.zeros(n, device=DEV) for _ in range(m)]
    spare = [torch.empty(n, device=DEV) for _ in range(m)]
    for r in range(4):
        grads, _ = inputs(n, m, 900 + 10 * r)
        pk = fresh(n, m)
        new = []
        for i in range(m):
            _, x = c.encode_sign(grads[i], e_lone[i], packet=pk[i])
            new.append(x)
        ref = blob(pk, new)
        e_lone = new
        bp = fresh(n, m)
        _, out = c.encode_sign_batch(grads, e_bat, spare, packets=bp)
        assert_blobs(blob(bp, out), ref, f"n={n} round {r}")
        e_bat, spare = spare, e_bat              # residuals / residuals_out swapped
    for a, b in zip(e_bat, e_lone):
        assert a.cpu().numpy().tobytes() == b.cpu().numpy().tobytes()


def test_validation_raises_before_any_launch():
    c, n, m = _codec(), 1024, 3
    grads, res = inputs(n, m, 1)
    pk = fresh(n, m)
    before = blob(pk, None)

    def bad(match, *a, **kw):
        with pytest.raises(ValueError, match=match):
            c.encode_sign_batch(*a, **kw)
        assert blob(pk, None) == before          # nothing was launched on these packets
    bad("None", grads, [res[0], None, res[2]], packets=pk)
    bad("one per gradient", grads, res[:2], packets=pk)
    bad("elements", grads[:2] + [torch.zeros(n + 4, device=DEV)], packets=pk)
    bad("elements", grads, res[:2] + [torch.zeros(n + 4, device=DEV)], packets=pk)
    bad("overlaps grads", grads, res, [grads[1], torch.empty(n, device=DEV), torch.empty(n, device=DEV)], packets=pk)
    bad("overlaps residuals", grads, res, [torch.empty(n, device=DEV), res[2], torch.empty(n, device=DEV)], packets=pk)
    block = torch.empty(2 * n, device=DEV)
    bad("residuals_out.* overlap", grads, res, [block[:n], block[n - 4:2 * n - 4], torch.empty(n, device=DEV)], packets=pk)
    bad("residuals_out.* overlap", grads, None, [block[:n], block[:n], torch.empty(n, device=DEV)], packets=pk)
    bad("length", grads, packets=[pk[0], c.SignPacket.alloc(n + 32, torch.device(DEV)), pk[2]])
    bad("one per gradient", grads, packets=pk[:2])
    bad("packets.* overlap", grads, packets=[pk[0], pk[0], pk[2]])
    bad("aligned", [grads[0], torch.zeros(n + 1, device=DEV)[1:], grads[2]], packets=pk)
    with pytest.raises(TypeError):
        c.encode_sign_batch([grads[0], grads[1].double(), grads[2]], packets=pk)
    assert blob(pk, None) == before


def test_a_prebuilt_job_table_gives_the_same_bits():
    c, n, m = _codec(), M20 + 259, 3
    grads, res = inputs(n, m, 77)
    for res_in, want in COMBOS:
        r = res if res_in else None
        pk, out = fresh(n, m), garbage(n, m) if want else None
        jobs = c.sign_jobs(grads, pk, r, out)
        assert jobs.is_cuda and jobs.numel() == 48 * m
        for _ in range(2):                       # built once, reused
            c.encode_sign_batch(grads, r, out, want_residuals=want, packets=pk, jobs=jobs)
        assert_blobs(blob(pk, out), batched(grads, r, want), f"jobs res_in={res_in} res_out={want}")


# ---- the Aggregator's key ------------------------------------------------------------------------
def _clients(grads, ef=()):
    from openmsftl_amd import Compression
    return [types.SimpleNamespace(C=Compression({"compression_function": "sign", "error_feedback": i in ef}),
                                  grad=g, client_id=i) for i, g in enumerate(grads)]


def _agg(scheme="fed_avg", **cfg):
    from openmsftl_amd.aggregation import Aggregator
    return Aggregator(dict({"aggregation_scheme": scheme}, **cfg))


def _np_grads(m, n, seed):
    rng = np.random.default_rng(seed)
    return [rng.standard_normal(n).astype(F) for _ in range(m)]


def _residuals(clients):
    return [None if c.C.get_residual() is None else np.asarray(c.C.get_residual()).tobytes() for c in clients]


@pytest.mark.parametrize("budget", ("two per sub-batch", None))
def test_sign_route_with_the_key_equals_the_round_without(budget):
    from openmsftl_amd.aggregation import sign_packet_bytes
    m, n, ef = 5, 8193, (0, 2, 3)
    cfg = {}
    if budget:       # all five packets and the aggregate, and room for two uploaded gradients
        cfg["device_budget_bytes"] = 5 * sign_packet_bytes(n) + 4 * n + 2 * 4 * n
    a, b = _agg(**cfg), _agg(batched_sign_encode=True, **cfg)
    ca, cb = _clients([None] * m, ef), _clients([None] * m, ef)
    for r in range(2):
        for g, x, y in zip(_np_grads(m, n, 40 + r), ca, cb):
            x.grad = y.grad = g
        a.aggregate_grads(ca)
        b.aggregate_grads(cb)
        assert a.agg_path == b.agg_path == "sign" and a.sign_groups == b.sign_groups == 1
        assert b.agg_grad.tobytes() == a.agg_grad.tobytes(), f"round {r}"
        assert _residuals(cb) == _residuals(ca), f"round {r}"
        assert [x is None for x in _residuals(cb)] == [i not in ef for i in range(m)]
        # the clients without error feedback of a sub-batch share one batched call (those with
        # it keep the lone call): sub-batches {0 ef, 1}, {2 ef, 3 ef}, {4}: 1 + 0 + 1; all five: 1
        assert b.sign_encode_calls == (2 if budget else 1) and a.sign_encode_calls == 0


def test_resident_routes_with_the_key():
    m, n, ef = 5, 8193, (1, 4)
    grads = _np_grads(m, n, 9)
    for scheme, key, path in (("krum", {"sign_geometry": True}, "sign-gram"),
                              ("coordinate_median", {"sign_trim": True}, "sign-trim")):
        a, b = _agg(scheme, **key), _agg(scheme, batched_sign_encode=True, **key)
        ca, cb = _clients(grads, ef), _clients(grads, ef)
        a.aggregate_grads(ca)
        b.aggregate_grads(cb)
        assert a.agg_path == b.agg_path == path
        assert b.agg_grad.tobytes() == a.agg_grad.tobytes(), scheme
        assert _residuals(cb) == _residuals(ca), scheme
        assert b.sign_encode_calls == 1 and a.sign_encode_calls == 0


def test_a_bad_residual_raises_with_no_client_advanced():
    m, n = 4, 8193
    b = _agg(batched_sign_encode=True)
    cb = _clients(_np_grads(m, n, 3), ef=range(m))
    b.aggregate_grads(cb)
    cb[2].C.set_residual(np.zeros(n + 1, F))
    before = _residuals(cb)
    with pytest.raises(ValueError, match="reset_residual"):
        b.aggregate_grads(cb)
    assert _residuals(cb) == before
