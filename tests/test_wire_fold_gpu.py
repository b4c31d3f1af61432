"""fc_wire_fold (csrc/fc_wire_fold.hip) through codec.fold_wire and Aggregator.aggregate_wire with
``"wire_fold": True`` on an MI355X.

Run:  python -m pytest tests/test_wire_fold_gpu.py -m gpu -q

The hand-built round of tests/test_wire_gpu.py (its helpers are imported): n = 6 * 8192 + 2048 + 3,
per-quarter counts from COUNTS.  The expected aggregate is oracle.packet_oracle.fold_packets over
tests/wire_model.py's unpack of the same bytes; the second witness is the route the fold replaces,
codec.decode_accumulate(codec.unpack(wires), ...).  Everything is compared bit for bit
(po.same_bits).  Only well-formed payloads reach the GPU, each through codec.wire_from_host.

Switch points of the kernel (names of csrc/fc_decode.hip, whose fold_body both folds run; not
imported):
  64 lanes            quarter counts 63, 64, 65
  kQR * 64 = 256      entries per item of the fast body: 255, 256, 257
  kQTail * 64 = 512   above it the wave takes the slow body: 513 listed, ~360 kept (tail), 2048
  kQGroup = 3         items per load group: batch sizes 1, 2, 64, 65
  kSparseMaxM = 128   packets per launch: batch sizes 128, 129, 130
"""
import numpy as np
import pytest

import test_wire_gpu as twg
import wire_model as wm
from oracle import packet_oracle as po

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

CH, QU = po.CHUNK, po.QUARTER
N = twg.N
WEIGHTS9 = np.float32([0.25, -1.5, 1.0, 0.125, 3.0, -0.5, 1.0 / 9, 2.0, 0.75])

_MEMO = {}


@pytest.fixture(scope="module", autouse=True)
def _gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from openmsftl_amd import _lib
    assert _lib.load().fc_abi_version() == 4
    yield
    _MEMO.clear()
    twg._MEMO.clear()
    torch.cuda.empty_cache()


def memo(key, make):
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


def _codec():
    from openmsftl_amd import codec
    return codec


def upload(payloads, n):
    return [_codec().wire_from_host(raw, n=n) for raw in payloads]          # each one validated


def expected(payloads, weights, acc=None):
    return po.fold_packets([wm.unpack(raw) for raw in payloads], weights, acc)


def host(t):
    return t.cpu().numpy()


def dirty_acc(n, seed):
    """A partial sum that holds -0.0, ordinary values and a NaN."""
    rng = np.random.default_rng(seed)
    acc = (rng.integers(-8, 9, size=n) * 0.25).astype(np.float32)
    acc[::3] = np.float32(-0.0)
    acc[n // 2 + 1] = np.float32(np.nan)
    return acc


def check_round(payloads, weights, n, seed=1):
    """From +0 and continued, against the oracle and against unpack + decode_accumulate."""
    codec = _codec()
    wires = upload(payloads, n)
    w = [float(x) for x in weights]
    got = codec.fold_wire(wires, w)
    want = expected(payloads, weights)
    assert got.dtype == torch.float32 and got.shape == (n,)
    assert po.same_bits(host(got), want)
    pk = codec.unpack(wires)
    assert po.same_bits(host(got), host(codec.decode_accumulate(pk, w)))
    acc = dirty_acc(n, seed)
    out = torch.from_numpy(acc.copy()).cuda()
    back = codec.fold_wire(wires, w, out=out, continue_sum=True)
    assert back is out
    want_c = expected(payloads, weights, acc)
    assert po.same_bits(host(out), want_c)
    out2 = torch.from_numpy(acc.copy()).cuda()
    codec.decode_accumulate(pk, w, out=out2, continue_sum=True)
    assert po.same_bits(host(out), host(out2))
    return want, want_c


def quarter_counts(raw):
    """(nch, 4) kept entries per quarter of a wire payload."""
    q = wm.parse(raw)["qoff"]
    b = np.stack([np.zeros_like(q), q & np.uint64(0xffff), (q >> np.uint64(16)) & np.uint64(0xffff),
                  (q >> np.uint64(32)) & np.uint64(0xffff), q >> np.uint64(48)], axis=1).astype(np.int64)
    return np.diff(b, axis=1)


# ---- 1. the mixed round: the slow body ---------------------------------------------------------
def test_mixed_round_from_zero_and_continued():
    payloads = twg.model_bytes()
    fields = twg.round_fields()
    assert {int(f["hdr"]["codec"]) for f in fields} == {po.CODEC_TOP, po.CODEC_RAND, po.CODEC_DROPOUT_BIASED,
                                                        po.CODEC_DROPOUT_UNBIASED}
    assert any(int(f["hdr"]["key_mode"]) == po.KEY_PHILOX and int(f["hdr"]["thresh"]) for f in fields)
    assert len(set(WEIGHTS9.tolist())) > 5 and (WEIGHTS9 < 0).any()
    starts = np.concatenate([wm.parse(raw)["start"] for raw in payloads])
    assert (starts % 2 == 1).any() and (starts % 8 != 0).any()        # odd and unaligned starts
    want, want_c = check_round(payloads, WEIGHTS9, N)
    acc = dirty_acc(N, 1)
    # the -0.0 fix-up has work to do: a -0.0 of the partial sum that ends as +0
    was = acc.view(np.uint32) == 0x80000000
    assert (was & (want_c.view(np.uint32) == 0)).any()
    assert np.isnan(want).any()


# ---- 2. top-k only: the fast body ---------------------------------------------------------------
def top_payloads():
    return memo("tops", lambda: [twg.model_bytes()[i] for i in (0, 2, 4, 6, 8)])


def test_top_k_only_takes_the_fast_body_and_its_tail():
    payloads = top_payloads()
    for raw in payloads:
        h = wm.parse(raw)["hdr"]["pkt"]
        assert int(h["codec"]) == po.CODEC_TOP and int(h["key_mode"]) == po.KEY_MAGNITUDE
        assert 0 < int(h["thresh"]) >> int(h["index_bits"]) < 0x7F800000
        f = wm.unpack(raw)
        assert po.kept_entries(f)[0].size == po.listed_entries(f)[0].size      # no slack is listed
    per = np.stack([quarter_counts(raw) for raw in payloads])        # (client, chunk, quarter)
    assert (per == 0).any() and ((per >= 1) & (per <= 256)).any()
    assert ((per >= 257) & (per <= 512)).any() and (per > 512).any()
    wave = per.max(axis=0)                                           # what decides a wave's body
    assert (wave <= 256).any()                                       # fast, no tail
    assert ((wave >= 257) & (wave <= 512)).any()                     # fast with the tail loop
    assert (wave > 512).any()                                        # that wave's slow body
    check_round(payloads, np.float32([0.5, -0.75, 1.25, 3.0, 1.0 / 3]), N, seed=2)
    # all weights positive: every -0.0 of the partial sum that a client drops becomes +0
    codec = _codec()
    acc = dirty_acc(N, 3)
    out = torch.from_numpy(acc.copy()).cuda()
    w = np.float32([0.5, 0.75, 1.25, 3.0, 1.0 / 3])
    codec.fold_wire(upload(payloads, N), [float(x) for x in w], out=out, continue_sum=True)
    assert po.same_bits(host(out), expected(payloads, w, acc))


# ---- 2b. packets that keep nothing ---------------------------------------------------------------
def keeps_nothing(thresh):
    return wm.pack(po.build_idxval(N, np.zeros(0, np.int64), np.zeros(0, np.float32), thresh=thresh,
                                   codec=po.CODEC_TOP, k=0))


@pytest.mark.parametrize("thresh", ["select-nothing", "finite"])
def test_packets_with_no_entries_beside_ordinary_top_k(thresh):
    """M = 4: packets 0 and 3 keep nothing (E = 0), 1 and 2 are ordinary top-k.  With kQGroup = 3
    the load groups are (0, 1, 2) and (3, 3, 3): an item with no entries is first in a group, last in
    a group, in the past-the-end reload slots, and a packet of its own, so the fast body's
    unconditional loads of it read the first weight and no byte of its buffer.  A select-nothing
    thresh sends the whole launch to the slow body (its key is above +inf bits); the same round
    under a finite thresh is the one whose waves take the fast body: that needs the whole launch
    non-generic, which the two top-k payloads are (test_top_k_only_... asserts it of them)."""
    ib = po.index_bits(N)
    T = int(po.NOTHING) if thresh == "select-nothing" else int(po.mag_key(np.array([twg.TIE]))[0]) << ib
    empty = keeps_nothing(T)
    h = wm.parse(empty)["hdr"]
    assert int(h["n_entries"]) == 0 and int(h["pkt"]["thresh"]) == T
    assert ((T >> ib) < 0x7F800000) == (thresh == "finite")
    tops = top_payloads()
    payloads = [empty, tops[0], tops[1], empty]
    per = np.stack([quarter_counts(raw) for raw in payloads]).max(axis=0)
    assert (per <= 512).any()                                        # waves that may take the fast body
    check_round(payloads, np.float32([0.5, -0.75, 1.25, 3.0]), N, seed=11)


# ---- 3. the keep rule on wire bytes --------------------------------------------------------------
def listing_slack(f):
    """The wire payload that lists EVERY listed entry of a slotted packet, slack included."""
    gidx, val = po.listed_entries(f)
    return wm.from_entries(f["n"], gidx, val, f["hdr"])


def slack_payloads():
    def make():
        fields = twg.round_fields()
        cut_in_chunk, cut_at_zero, philox = fields[0], fields[2], fields[1]
        ib = po.index_bits(N)
        assert int(cut_in_chunk["hdr"]["thresh"]) & ((1 << ib) - 1) == 3 * CH + QU + 1000
        assert int(cut_at_zero["hdr"]["thresh"]) & ((1 << ib) - 1) == 0
        assert int(philox["hdr"]["key_mode"]) == po.KEY_PHILOX
        out = [listing_slack(f) for f in (cut_in_chunk, cut_at_zero, philox)]
        for raw, f in zip(out, (cut_in_chunk, cut_at_zero, philox)):
            u = wm.unpack(raw)
            listed, kept = po.listed_entries(u), po.kept_entries(u)
            assert 0 < kept[0].size < listed[0].size                 # the payload lists what is dropped
            assert np.array_equal(kept[0], po.kept_entries(f)[0])
        # ties on both sides of the cut, in the chunk that holds it
        u = wm.unpack(out[0])
        gidx, val = po.listed_entries(u)
        tie = np.abs(val) == twg.TIE
        cut = 3 * CH + QU + 1000
        in_chunk = (gidx >= 3 * CH) & (gidx < 4 * CH)
        assert (tie & in_chunk & (gidx < cut)).any() and (tie & in_chunk & (gidx >= cut)).any()
        return out
    return memo("slack", make)


def test_magnitude_key_slack_is_dropped_by_the_fast_body():
    payloads = slack_payloads()[:2]
    per = np.stack([quarter_counts(raw) for raw in payloads]).max(axis=0)
    assert (per <= 512).any() and (per > 512).any()
    check_round(payloads, np.float32([1.5, -0.25]), N, seed=4)


def test_philox_key_slack_and_a_poisoning_packet():
    payloads = list(slack_payloads())
    check_round(payloads, np.float32([1.5, -0.25, 0.5]), N, seed=5)
    rng = np.random.default_rng(9)
    idx = np.sort(rng.choice(N, size=3000, replace=False))
    poison = wm.pack(po.build_idxval(N, idx, twg.half_values(rng, idx.size), thresh=0,
                                     codec=po.CODEC_DROPOUT_UNBIASED, p=0.0, seed=4))
    payloads.insert(1, poison)
    weights = np.float32([1.5, 0.75, -0.25, 0.5])
    want, _ = check_round(payloads, weights, N, seed=6)
    dropped = np.ones(N, bool)
    dropped[idx] = False
    assert np.isnan(want[dropped]).all() and not np.isnan(want[~dropped]).all()


# ---- 4. batch sizes ------------------------------------------------------------------------------
N_B = 2 * CH + 3


def cut_payloads():
    """The five top-k designs cut to N_B, under headers of that length."""
    def make():
        ib = po.index_bits(N_B)
        key = int(po.mag_key(np.array([twg.TIE]))[0])
        out = []
        for j, i in enumerate((0, 2, 4, 6, 8)):
            f = twg.round_fields()[i]
            gidx, val = po.listed_entries(f)
            gidx, val = gidx[gidx < N_B], val[gidx < N_B]
            Ti = min(int(f["hdr"]["thresh"]) & ((1 << po.index_bits(N)) - 1), N_B - 1)
            keep = (np.abs(val) > twg.TIE) | ((np.abs(val) == twg.TIE) & (gidx >= Ti))
            out.append(wm.pack(po.build_idxval(N_B, gidx, val, thresh=(key << ib) | Ti, lower=1,
                                               codec=po.CODEC_TOP, k=int(keep.sum()))))
        return out
    return memo("cut", make)


def cut_state():
    def make():
        payloads = cut_payloads()
        rows = [po.decode_packet(wm.unpack(raw)) for raw in payloads]
        return upload(payloads, N_B), rows
    return memo("cut-dev", make)


@pytest.mark.parametrize("M", [1, 2, 64, 65, 128, 129, 130])
def test_batch_sizes(M):
    from oracle.gar_oracle import sequential_weighted_sum
    codec = _codec()
    wires5, rows5 = cut_state()
    weights = np.float32([((i % 7) - 3) * 0.25 + 0.125 + i / 1024.0 for i in range(M)])
    assert len(set(weights.tolist())) == M
    wires = [wires5[i % 5] for i in range(M)]
    rows = [rows5[i % 5] for i in range(M)]
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        want = sequential_weighted_sum(rows, [np.float32(x) for x in weights])
    got = codec.fold_wire(wires, [float(x) for x in weights])
    assert po.same_bits(host(got), want)
    # continued from the sum of the first rows: the same left-to-right sum
    if M > 1:
        h = M // 2
        out = codec.fold_wire(wires[:h], [float(x) for x in weights[:h]])
        codec.fold_wire(wires[h:], [float(x) for x in weights[h:]], out=out, continue_sum=True)
        assert po.same_bits(host(out), want)


# ---- 5. start beyond 16 bits ---------------------------------------------------------------------
N_S = 9 * CH + 5


def test_a_packet_that_keeps_everything_and_a_sparse_one():
    rng = np.random.default_rng(31)
    full = wm.pack(po.build_idxval(N_S, np.arange(N_S), twg.half_values(rng, N_S), thresh=0,
                                   codec=po.CODEC_RAND))
    w = wm.parse(full)
    assert int(w["start"][8]) == 65536 and int(w["qoff"][7] >> np.uint64(48)) == 8192
    sidx = np.sort(rng.choice(N_S, size=300, replace=False))
    sparse = wm.pack(po.build_idxval(N_S, sidx, twg.half_values(rng, sidx.size), thresh=0,
                                     codec=po.CODEC_TOP, k=sidx.size))
    check_round([full, sparse], np.float32([0.5, -2.0]), N_S, seed=7)
    check_round([sparse, full], np.float32([0.5, 3.0]), N_S, seed=8)


# ---- 6. determinism and the untouched rest -------------------------------------------------------
@pytest.mark.parametrize("n, which", [(N, "mixed"), (N_S, "sparse")])
def test_two_calls_give_the_same_bits_and_the_guards_stay(n, which):
    codec = _codec()
    if which == "mixed":
        payloads, weights = twg.model_bytes(), WEIGHTS9
    else:                                                            # n % 4 == 1: three elements to the boundary
        rng = np.random.default_rng(33)
        sidx = np.sort(rng.choice(n, size=500, replace=False))
        payloads = [wm.pack(po.build_idxval(n, sidx, twg.half_values(rng, sidx.size), thresh=0,
                                            codec=po.CODEC_TOP, k=sidx.size))]
        weights = np.float32([0.75])
        assert n % 4 == 1
    wires = upload(payloads, n)
    w = [float(x) for x in weights]
    pad = 64
    big = torch.full((pad + n + pad,), -1, dtype=torch.int32, device="cuda")
    big.fill_(int(np.uint32(0xA5A5A5A5).view(np.int32)))
    big = big.view(torch.float32)
    guard = host(big).view(np.uint32).copy()
    out = big[pad: pad + n]
    assert out.data_ptr() % 16 == 0
    codec.fold_wire(wires, w, out=out)
    first = host(out).copy()
    after = host(big).view(np.uint32)
    assert np.array_equal(after[:pad], guard[:pad]) and np.array_equal(after[pad + n:], guard[pad + n:])
    assert po.same_bits(first, expected(payloads, weights))
    again = codec.fold_wire(wires, w)
    assert host(again).tobytes() == first.tobytes()                  # byte for byte, NaN payloads included
    with pytest.raises(ValueError, match="out must have n elements"):
        codec.fold_wire(wires, w, out=torch.zeros(n + 4, dtype=torch.float32, device="cuda"))
    with pytest.raises(ValueError, match="continue_sum needs"):
        codec.fold_wire(wires, w, continue_sum=True)


# ---- 7. the Aggregator ---------------------------------------------------------------------------
N_R, FRAC, M_R = twg.N_R, twg.FRAC, twg.M_R


def payload_room():
    size = _codec().wire_bytes(N_R, round(FRAC * N_R))
    return (size + 255) & ~255


def count_folds(monkeypatch):
    codec = _codec()
    calls = []
    real = codec.fold_wire

    def counted(wires, *a, **k):
        calls.append(len(list(wires)))
        return real(wires, *a, **k)
    monkeypatch.setattr(codec, "fold_wire", counted)
    return calls


def test_aggregate_wire_with_wire_fold_equals_aggregate_grads(monkeypatch):
    from openmsftl_amd import aggregation
    from openmsftl_amd.aggregation import Aggregator
    ref = Aggregator({"aggregation_scheme": "fed_avg"})
    ref.aggregate_grads(twg.make_clients())
    assert ref.agg_path == "stream"
    payloads = [c.C.compress_wire(c.grad) for c in twg.make_clients()]
    calls = count_folds(monkeypatch)
    monkeypatch.setattr(_codec(), "unpack", lambda *a, **k: pytest.fail("wire_fold must not unpack"))
    agg = Aggregator({"aggregation_scheme": "fed_avg", "wire_fold": True})
    agg.aggregate_wire(payloads)
    assert agg.agg_path == "wire-fold" and agg.curr_G is None and calls == [M_R]
    assert agg.agg_grad.dtype == np.float32 and agg.agg_grad.shape == (N_R,)
    assert agg.agg_grad.tobytes() == ref.agg_grad.tobytes()
    assert "_wire_packets" not in agg.__dict__ or set(agg.__dict__["_wire_packets"]) <= {"slab"}
    # a budget for two payloads beside the aggregate: groups of 2, 2, 1
    budget = 4 * N_R + 2 * payload_room()
    sizes = [len(p) for p in payloads]
    assert aggregation.wire_fold_groups(sizes, N_R, budget) == [range(0, 2), range(2, 4), range(4, 5)]
    del calls[:]
    small = Aggregator({"aggregation_scheme": "fed_avg", "wire_fold": True, "device_budget_bytes": budget})
    small.aggregate_wire(payloads, n=N_R)
    assert calls == [2, 2, 1] and small.agg_path == "wire-fold"
    assert small.agg_grad.tobytes() == ref.agg_grad.tobytes()
    with pytest.raises(NotImplementedError, match="fit device_budget_bytes"):
        Aggregator({"aggregation_scheme": "fed_avg", "wire_fold": True,
                    "device_budget_bytes": 4 * N_R + payload_room() - 1}).aggregate_wire(payloads)


def test_wire_fold_with_error_feedback_clients_two_rounds():
    from openmsftl_amd.aggregation import Aggregator
    a, b = twg.make_clients(ef=True), twg.make_clients(ef=True)
    ref = Aggregator({"aggregation_scheme": "fed_avg"})
    agg = Aggregator({"aggregation_scheme": "fed_avg", "wire_fold": True,
                      "device_budget_bytes": 4 * N_R + 2 * payload_room()})
    for rnd in range(2):                                             # the second round adds the residual
        ref.aggregate_grads(a)
        agg.aggregate_wire([c.C.compress_wire(c.grad) for c in b])
        assert agg.agg_path == "wire-fold"
        assert agg.agg_grad.tobytes() == ref.agg_grad.tobytes(), f"round {rnd}"


def test_without_the_key_nothing_changes_and_the_gram_family_ignores_it(monkeypatch):
    from openmsftl_amd.aggregation import Aggregator
    payloads = [c.C.compress_wire(c.grad) for c in twg.make_clients()]
    calls = count_folds(monkeypatch)
    folded = Aggregator({"aggregation_scheme": "fed_avg", "wire_fold": True})
    folded.aggregate_wire(payloads)
    for cfg in ({"aggregation_scheme": "fed_avg"}, {"aggregation_scheme": "fed_avg", "wire_fold": False}):
        del calls[:]
        plain = Aggregator(dict(cfg))
        plain.aggregate_wire(payloads)
        assert plain.agg_path == "wire" and calls == []
        assert plain.agg_grad.tobytes() == folded.agg_grad.tobytes()
    del calls[:]
    krum = Aggregator({"aggregation_scheme": "krum", "krum_frac": 0.6, "wire_fold": True})
    krum.aggregate_wire(payloads)
    ref = Aggregator({"aggregation_scheme": "krum", "krum_frac": 0.6})
    ref.aggregate_wire(payloads)
    assert krum.agg_path == "wire" and calls == []
    assert krum.agg_grad.tobytes() == ref.agg_grad.tobytes()
