"""The scaled-sign codec on the host: the model's hand cases, the C ABI of the new entry points,
fc_sign_wire_validate, gar.SignMajority's eta rule and the Aggregator's routing predicates.

Run:  python -m pytest tests/test_sign_host.py -m "not gpu" -q

No GPU is needed: the library loads without one (tests/test_lib_abi.py).  Payloads come from
tests/sign_model.py; one mutation per rule of the validator's list (include/fedcodec.h) must be
rejected with the message of that rule.  The same corpus, and every truncation of the valid
payloads, goes through the stand-alone program tests/payload_validate_main.cc, built with the host
compiler and -fsanitize=address,undefined: the same verdicts and no sanitizer report.
"""
import ctypes
import os
import re
import subprocess
import types

import numpy as np
import pytest

import sign_model as sm
from payload_standalone import run, standalone  # noqa: F401  (standalone: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fedcodec.h")
F = np.float32
NEW = ("fc_sign_words", "fc_sign_workspace_bytes", "fc_sign_encode", "fc_sign_decode",
       "fc_sign_fold", "fc_sign_vote", "fc_sign_wire_validate", "fc_sign_fold_form")


@pytest.fixture(scope="module")
def lib():
    from openmsftl_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


# ---- the model on hand cases --------------------------------------------------------------------
def test_model_bits_go_by_the_ieee_sign_bit():
    neg_nan = np.array([0xFFC00000], np.uint32).view(F)[0]
    pos_nan = np.array([0x7FC00000], np.uint32).view(F)[0]
    den = np.array([0x80000001], np.uint32).view(F)[0]                 # the smallest negative denormal
    a = np.array([-0.0, 0.0, neg_nan, pos_nan, -np.inf, np.inf, den, -den, 1.5, -2.5], F)
    assert list(sm.bits(a)) == [True, False, True, False, True, False, True, False, False, True]
    w = sm.words_of(sm.bits(a))
    assert w.size == 4 and int(w[0]) == 0b1001010101 and not w[1:].any()
    assert list(sm.bits_of(w, a.size)) == list(sm.bits(a))


def test_model_the_add_turns_minus_zero_into_plus_zero():
    g = np.array([-0.0, 0.0, -1.0, 2.0], F)
    assert list(sm.bits(sm.encoded(g))) == [True, False, True, False]
    assert list(sm.bits(sm.encoded(g, np.zeros(4, F)))) == [False, False, True, False]


def test_model_scale_decode_and_residual():
    g = np.array([1.0, -2.0, 3.0, -0.0, 0.0, -6.0], F)
    a, s, w, q, e2 = sm.encode(g)
    assert s == F(2.0) and sm.scale_range(g)[0] <= s <= sm.scale_range(g)[1]
    assert q.tobytes() == np.array([2, -2, 2, -2, 2, -2], F).tobytes()
    assert e2.tobytes() == np.array([-1, 0, 1, 2, -2, -4], F).tobytes()
    assert int(w[0]) == 0b101010
    h = sm.header(g.size, s)
    assert (int(h["n"]), int(h["k"]), int(h["n_entries"])) == (6, 6, 6)
    assert (int(h["codec"]), int(h["format"]), float(h["p"])) == (6, 4, 2.0)
    # non-finite elements: plain IEEE arithmetic
    assert np.isinf(sm.scale(np.array([1.0, np.inf], F))) and np.isnan(sm.scale(np.array([np.nan, np.inf], F)))
    # a denormal survives the float64 sum
    den = np.array([1], np.uint32).view(F)[0]
    assert sm.scale(np.array([den], F)) == den


def test_model_sum_bound_holds_for_numpy_orders():
    rng = np.random.default_rng(5)
    a = rng.standard_normal(100_003).astype(F)
    S, m = sm.true_sum(a), np.abs(a.astype(np.float64))
    b = sm.sum_bound(a.size, S)
    for approx in (float(np.sum(m)), float(np.cumsum(m)[-1]), float(np.sum(m[::-1]))):
        assert abs(approx - S) <= b
    assert 0 < b < 1e-9 * S


def test_model_fold_first_row_rule_and_tie_vote():
    # a zero-scale first client whose bits are all set decodes to -0.0: np.sum starts from +0.0
    rows = np.stack([sm.decode(np.ones(4, bool), F(0.0)), sm.decode(np.array([1, 0, 1, 0], bool), F(0.0))])
    assert rows[0].tobytes() == np.full(4, -0.0, F).tobytes()
    out = sm.fold(rows, np.array([0.5, 0.5], F))
    assert out.tobytes() == np.zeros(4, F).tobytes()
    cont = sm.fold(rows[1:], np.array([0.5], F), start=sm.fold(rows[:1], np.array([0.5], F)))
    assert cont.tobytes() == out.tobytes()
    B = np.array([[1, 1, 0, 0], [1, 0, 1, 0], [1, 0, 0, 0], [1, 1, 1, 0]], bool)       # even M
    v = sm.vote(B, F(0.25))
    assert v.tobytes() == np.array([-0.25, 0.0, 0.0, 0.25], F).tobytes()              # ties are +0.0
    assert sm.vote(B[:3], F(0.25)).tobytes() == np.array([-0.25, 0.25, 0.25, 0.25], F).tobytes()


# ---- the C ABI ----------------------------------------------------------------------------------
def _declarations():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for name, args in re.findall(r"\b(fc_sign_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
        args = args.strip()
        out[name] = 0 if args in ("", "void") else args.count(",") + 1
    return out


def test_new_symbols_are_declared_exported_and_bound(lib):
    from openmsftl_amd import _lib
    decl = _declarations()
    nm = subprocess.run(["nm", "-D", "--defined-only", _lib.LIB_PATH], capture_output=True,
                        text=True, check=True).stdout
    exported = set(re.findall(r"\s[TW]\s+(\S+)", nm))
    for name in NEW:
        assert name in decl and name in exported, name
        assert len(_lib.SIGNATURES[name][1]) == decl[name], name
        getattr(lib, name)
    assert lib.fc_abi_version() == 4
    assert (_lib.FC_CODEC_SIGN, _lib.FC_FMT_SIGN) == (6, 4)
    src = open(HEADER).read()
    assert re.search(r"#define FC_CODEC_SIGN 6\b", src) and re.search(r"#define FC_FMT_SIGN 4\b", src)


def test_sign_words(lib):
    for n, want in ((1, 4), (32, 4), (33, 4), (128, 4), (129, 8)):
        assert lib.fc_sign_words(n) == want == sm.sign_words(n)
    for n in (8191, 8192, 8193, 1_000_003):
        assert lib.fc_sign_words(n) == sm.sign_words(n) and lib.fc_sign_words(n) % 4 == 0
    assert lib.fc_sign_workspace_bytes(1) > 0
    assert lib.fc_sign_workspace_bytes(1 << 27) >= lib.fc_sign_workspace_bytes(1)


def test_argument_errors_do_not_touch_gpu(lib):
    from openmsftl_amd import _lib
    buf = ctypes.create_string_buffer(1 << 14)
    a = (ctypes.addressof(buf) + 15) & ~15
    ws = lib.fc_sign_workspace_bytes(64)
    good = dict(g=a, ri=a + 1024, ro=a + 2048, n=64, words=a + 4096, nw=4, hdr=a + 5120, ws=a + 6144, wsb=ws)

    def enc(**kw):
        p = dict(good, **kw)
        return lib.fc_sign_encode(p["g"], p["ri"], p["ro"], p["n"], p["words"], p["nw"], p["hdr"],
                                  p["ws"], p["wsb"], None)
    err = lambda: lib.fc_last_error()                                  # noqa: E731
    assert enc(g=None) == -1 and b"NULL" in err()
    assert enc(words=None) == -1 and enc(hdr=None) == -1 and enc(ws=None) == -1
    assert enc(n=0) == -1 and b"n=0" in err()
    assert enc(n=1 << 32) == -1
    assert enc(g=a + 4) == -1 and b"aligned" in err()
    assert enc(ri=a + 1028) == -1 and enc(ro=a + 2052) == -1 and enc(words=a + 4100) == -1
    assert enc(nw=3) == -1 and b"n_words" in err()
    assert enc(ro=a) == -1 and b"overlap" in err()                     # e' on g
    assert enc(ro=a + 1024 + 128) == -1 and b"overlap" in err()        # e' on e
    assert enc(wsb=16) == -3 and b"workspace" in err()
    view = _lib.PacketView(bitmap=a, hdr=a + 1024)
    assert lib.fc_sign_decode(None, 64, a, None) == -1
    assert lib.fc_sign_decode(ctypes.byref(view), 64, None, None) == -1
    assert lib.fc_sign_decode(ctypes.byref(view), 0, a + 2048, None) == -1
    assert lib.fc_sign_decode(ctypes.byref(view), 64, a + 2052, None) == -1 and b"aligned" in err()
    assert lib.fc_sign_decode(ctypes.byref(_lib.PacketView(hdr=a)), 64, a + 2048, None) == -1
    for m in (0, -1, 65536):
        assert lib.fc_sign_fold(a, m, 64, a + 2048, 0, None) == -1 and b"m=" in err()
        assert lib.fc_sign_vote(a, m, 64, 1.0, a + 2048, None) == -1 and b"m=" in err()
    assert lib.fc_sign_fold(None, 1, 64, a + 2048, 0, None) == -1
    assert lib.fc_sign_fold(a, 1, 64, None, 0, None) == -1
    assert lib.fc_sign_fold(a, 1, 0, a + 2048, 0, None) == -1
    assert lib.fc_sign_fold(a, 1, 64, a + 2052, 0, None) == -1 and b"aligned" in err()
    assert lib.fc_sign_vote(None, 1, 64, 1.0, a + 2048, None) == -1
    assert lib.fc_sign_vote(a, 1, 64, 1.0, None, None) == -1
    assert lib.fc_sign_vote(a, 1, 1 << 32, 1.0, a + 2048, None) == -1
    assert lib.fc_sign_vote(a, 1, 64, 1.0, a + 2052, None) == -1
    assert lib.fc_sign_wire_validate(None, 0, 0) == -1 and b"NULL" in err()
    assert lib.fc_sign_fold_form(7) == -1 and lib.fc_sign_fold_form(-1) == 0


# ---- the validator ------------------------------------------------------------------------------
N = 3 * 8192 + 5                   # 5 tail bits and three pad words


def validate(lib, raw: bytes, n_expected: int = 0):
    buf = ctypes.create_string_buffer(raw, len(raw))
    rc = lib.fc_sign_wire_validate(ctypes.cast(buf, ctypes.c_void_p), len(raw), n_expected)
    return rc, (lib.fc_last_error() or b"").decode()


def _payload(n, seed=0, s=None):
    rng = np.random.default_rng(seed)
    g = rng.standard_normal(n).astype(F)
    _, sc, w, _, _ = sm.encode(g)
    return sm.pack(n, sc if s is None else s, w)


def accepted_payloads():
    out = {f"n={n}": (_payload(n, n), n) for n in (1, 31, 32, 33, 127, 128, 129, 8192, N)}
    out["zero scale"] = (_payload(65, 1, s=0.0), 65)
    out["inf scale"] = (_payload(65, 2, s=np.inf), 65)
    out["nan scale"] = (_payload(65, 3, s=np.nan), 65)
    out["negative nan scale"] = (_payload(65, 3, s=np.array([0xFFC00000], np.uint32).view(F)[0]), 65)
    out["denormal scale"] = (_payload(65, 4, s=np.array([3], np.uint32).view(F)[0]), 65)
    out["all bits set"] = (sm.pack(64, 1.0, sm.words_of(np.ones(64, bool))), 64)
    return out


def _put(raw: bytes, off: int, value, fmt: str) -> bytes:
    a = bytearray(raw)
    b = np.array([value], dtype=fmt).tobytes()
    a[off: off + len(b)] = b
    return bytes(a)


def mutations():
    """name -> (bytes, n_expected, the message's pattern): one field changed per rule."""
    base, O = _payload(N, 7), sm.OFF
    assert N % 32 == 5 and sm.sign_words(N) - (N + 31) // 32 == 3     # tail bits and three pad words
    words_off = sm.WIRE_HDR_BYTES
    last = words_off + 4 * (N // 32)
    m = {
        "shorter than the header": (base[:127], 0, "shorter than the 128-byte header"),
        "truncated by one byte": (base[:-1], 0, "total_bytes"),
        "one extra byte": (base + b"\0", 0, "total_bytes"),
        "four extra bytes, total_bytes following": (_put(base + b"\0" * 4, O["total_bytes"], len(base) + 4, "<u8"), 0,
                                                    "is not the size of n"),
        "wrong magic": (_put(base, O["magic"], 0x31574346, "<u4"), 0, "bad magic"),
        "wrong version": (_put(base, O["version"], 2, "<u4"), 0, "unsupported version"),
        "reserved bytes": (_put(base, O["zero"] + 12, 1, "<u4"), 0, "reserved bytes"),
        "n = 0": (_put(base, O["pkt.n"], 0, "<u4"), 0, "n = 0"),
        "n_expected mismatch": (base, N + 1, "expected"),
        "codec top": (_put(base, O["pkt.codec"], 1, "<u4"), 0, "codec 1 is not sign"),
        "format idx/val": (_put(base, O["pkt.format"], 0, "<u4"), 0, "format 0 is not sign"),
        "k below n": (_put(base, O["pkt.k"], N - 1, "<u4"), 0, "k = "),
        "n_entries below n": (_put(base, O["pkt.n_entries"], N - 1, "<u4"), 0, "n_entries = "),
        "status retry": (_put(base, O["pkt.status"], 1, "<u4"), 0, "status 1 is not OK"),
        "negative scale": (_put(base, O["pkt.p"], -0.5, "<f8"), 0, "negative"),
        "minus zero scale": (_put(base, O["pkt.p"], -0.0, "<f8"), 0, "negative"),
        "scale not a float32": (_put(base, O["pkt.p"], 0.1, "<f8"), 0, "not a float32"),
        "scale above float32": (_put(base, O["pkt.p"], 1e300, "<f8"), 0, "not a float32"),
        "scale a double denormal": (_put(base, O["pkt.p"], 5e-324, "<f8"), 0, "not a float32"),
        "scale below the float32 denormals": (_put(base, O["pkt.p"], 2.0 ** -150, "<f8"), 0, "not a float32"),
        "scale a half float32 denormal step": (_put(base, O["pkt.p"], 1.5 * 2.0 ** -149, "<f8"), 0, "not a float32"),
        "nan scale with a double's payload": (_put(base, O["pkt.p"], 0x7FF8000000000001, "<u8"), 0, "not a float32"),
        "a bit at n": (_put(base, last, int(np.frombuffer(base, "<u4", 1, last)[0]) | (1 << (N % 32)), "<u4"), 0,
                       "bit at or past n"),
        "the last tail bit": (_put(base, last, int(np.frombuffer(base, "<u4", 1, last)[0]) | (1 << 31), "<u4"), 0,
                              "bit at or past n"),
        "first pad word": (_put(base, last + 4, 1, "<u4"), 0, "pad word"),
        "last pad word": (_put(base, len(base) - 4, 1 << 31, "<u4"), 0, "pad word"),
        "n larger, the same bytes": (_put(_put(_put(base, O["pkt.n"], N + 200, "<u4"), O["pkt.k"], N + 200, "<u4"),
                                           O["pkt.n_entries"], N + 200, "<u4"), 0, "is not the size of n"),
    }
    for f in ("thresh", "lower", "seed", "offset"):
        m[f"{f} not zero"] = (_put(base, O[f"pkt.{f}"], 1, "<u8"), 0, "must be zero")
    for f in ("index_bits", "n_definite", "n_cand", "chunk", "key_mode"):
        m[f"{f} not zero"] = (_put(base, O[f"pkt.{f}"], 1, "<u4"), 0, "must be zero")
    m["reserved[2] not zero"] = (_put(base, O["pkt.reserved"] + 8, 1, "<u4"), 0, "must be zero")
    return m


MUTATIONS = sorted(mutations())


@pytest.mark.parametrize("name", sorted(accepted_payloads()))
def test_validator_accepts_model_payloads(lib, name):
    raw, n = accepted_payloads()[name]
    assert len(raw) == sm.wire_bytes(n) == 128 + 4 * lib.fc_sign_words(n)
    for n_expected in (0, n):
        rc, msg = validate(lib, raw, n_expected)
        assert rc == 0, msg


@pytest.mark.parametrize("name", MUTATIONS)
def test_validator_rejects_each_mutation_with_its_reason(lib, name):
    raw, n_expected, want = mutations()[name]
    rc, msg = validate(lib, raw, n_expected)
    assert rc == -1 and msg.startswith("sign wire: ") and re.search(want, msg), msg


def test_the_two_validators_reject_each_others_bytes(lib):
    raw, n = accepted_payloads()[f"n={N}"]
    buf = ctypes.create_string_buffer(raw, len(raw))
    assert lib.fc_wire_validate(ctypes.cast(buf, ctypes.c_void_p), len(raw), 0) == -1
    assert b"bad magic" in lib.fc_last_error()
    from openmsftl_amd import codec
    with pytest.raises(ValueError, match="bad magic"):
        codec.TOP.check(raw)
    assert codec.is_sign_payload(raw) and not codec.is_sign_payload(b"FCW1" + raw[4:])
    a, h = codec.SIGN.check(raw, n)
    assert int(h.pkt.n) == n and a.size == len(raw)
    with pytest.raises(ValueError, match="expected"):
        codec.SIGN.check(raw, n + 1)


# ---- the same corpus through the sanitized stand-alone program --------------------------------
def test_the_corpus_through_the_sanitized_standalone_program(lib, standalone, tmp_path):
    exe, sanitized = standalone
    corpus = [(name, raw, n) for name, (raw, n) in sorted(accepted_payloads().items())]
    corpus += [(name,) + mutations()[name][:2] for name in MUTATIONS]
    for (name, raw, n_expected), got in zip(corpus, run(exe, ["sign"], tmp_path, corpus)):
        rc, msg = validate(lib, raw, n_expected)
        assert got == ("OK" if rc == 0 else "BAD " + msg), name         # the library's verdict
        if name in mutations():
            assert got.startswith("BAD sign wire: ") and re.search(mutations()[name][2], got), f"{name}: {got}"
        else:
            assert got == "OK", f"{name}: {got}"
    print(f"{len(corpus)} payloads, sanitized build: {sanitized}")


def test_every_truncation_through_the_sanitized_standalone_program(standalone, tmp_path):
    """Each valid payload cut at every length 0 .. size, each prefix in a heap block of exactly its
    length: only the whole payload is accepted and no read leaves a block."""
    exe, sanitized = standalone
    corpus = [(name, raw, 0) for name, (raw, n) in sorted(accepted_payloads().items()) if n <= 8192]
    corpus += [("mutated " + name, mutations()[name][0], 0) for name in MUTATIONS[:6]]
    for (name, raw, _), got in zip(corpus, run(exe, ["sign", "--trunc"], tmp_path, corpus)):
        want = 0 if name.startswith("mutated ") else 1
        assert got == f"TRUNC ok={want} of={len(raw) + 1}", (name, got)
    print(f"{len(corpus)} payloads, sanitized build: {sanitized}")


# ---- gar.SignMajority ---------------------------------------------------------------------------
def test_sign_majority_eta_rule_and_errors():
    from openmsftl_amd.gar import SignMajority
    g = SignMajority({})
    assert g.eta is None and g.majority_scale is None
    for scales in ([0.5], [0.25, 4.0], [0.1, 0.2, 0.7], [0.1, np.inf, 0.3, np.nan, 0.2], [1e-40, 3e38]):
        got = g._eta_of(scales)
        assert isinstance(got, np.float32) and got.tobytes() == sm.majority_eta(scales).tobytes()
    assert g._eta_of([float(F(0.1)), float(F(0.3))]) == F((np.float64(F(0.1)) + np.float64(F(0.3))) / 2)
    for scales in ([], [np.nan], [np.inf, np.nan]):
        with pytest.raises(ValueError, match="finite scale"):
            g._eta_of(scales)
    fixed = SignMajority({"majority_scale": 0.1})
    assert fixed._eta_of([np.nan]) == F(0.1) and isinstance(fixed.majority_scale, np.float32)
    for bad in ("0.1", True, [0.1]):
        with pytest.raises(ValueError, match="majority_scale"):
            SignMajority({"majority_scale": bad})
    with pytest.raises(NotImplementedError, match="dense G"):
        g.aggregate(np.zeros((2, 4), F))
    g.gradient_weights = np.full(2, 0.5, F)
    with pytest.raises(ValueError, match="unweighted"):
        g.aggregate_packets([object(), object()])
    with pytest.raises(TypeError, match="sign packets"):
        SignMajority({}).aggregate_packets([object()])


# ---- the routing predicates on stub clients -----------------------------------------------------
def _clients(m=3, n=100, fn="sign", dtype=F, **cfg):
    from openmsftl_amd import Compression
    return [types.SimpleNamespace(C=Compression(dict({"compression_function": fn}, **cfg)),
                                  grad=np.zeros(n, dtype), client_id=i) for i in range(m)]


def _agg(scheme="fed_avg", **cfg):
    from openmsftl_amd.aggregation import Aggregator
    return Aggregator(dict({"aggregation_scheme": scheme}, **cfg))


def test_sign_route_conditions_on_stub_clients(lib):
    from openmsftl_amd.aggregation import sign_route
    from openmsftl_amd.gar import SignMajority
    assert type(_agg("sign_majority").gar) is SignMajority
    assert sign_route(_agg(), _clients()) is True
    assert sign_route(_agg("sign_majority"), _clients()) is True
    assert sign_route(_agg(), _clients(error_feedback=True)) is True
    # fed_avg outside the conditions: the generic routes take the round
    assert sign_route(_agg(sign_packets=False), _clients()) is False
    assert sign_route(_agg(), _clients(fn="top")) is False
    assert sign_route(_agg(), _clients() + _clients(1, fn="top")) is False
    assert sign_route(_agg(), _clients(dtype=np.float64)) is False
    assert sign_route(_agg(), _clients() + _clients(1, n=101)) is False
    assert sign_route(_agg(), _clients(n=0)) is False
    assert sign_route(_agg(num_hierarchies=1, cluster_size_list=[2]), _clients()) is False
    assert sign_route(_agg(devices=2), _clients()) is False
    a = _agg()
    a.gar.gradient_weights = np.full(3, 1 / 3, np.float64)
    assert sign_route(a, _clients()) is False
    a.gar.gradient_weights = np.full(3, 1 / 3, F)
    assert sign_route(a, _clients()) is True
    stub = _clients()
    stub[1].C = types.SimpleNamespace(compression_function="sign", error_feedback=False)
    assert sign_route(_agg(), stub) is False
    # sign_majority outside the conditions: NotImplementedError naming the condition
    M = "sign_majority"
    for agg, cl, why in (
            (_agg(M), _clients(fn="top"), "every client to compress with 'sign'"),
            (_agg(M), _clients() + _clients(1, fn="full"), "every client to compress with 'sign'"),
            (_agg(M), stub, "drop-in Compression"),
            (_agg(M), _clients(dtype=np.float64), "1-D float32 gradients"),
            (_agg(M), _clients() + _clients(1, n=101), "gradients of one length"),
            (_agg(M), _clients(n=0), "n > 0"),
            (_agg(M, num_hierarchies=1, cluster_size_list=[2]), _clients(), "no hierarchies"),
            (_agg(M, devices=2), _clients(), "one device"),
            (_agg(M, device_budget_bytes=1000), _clients(m=8, n=4096), r"device_budget_bytes \(\d+ > 1000 bytes\)")):
        with pytest.raises(NotImplementedError, match=why):
            sign_route(agg, cl)
    a = _agg(M)
    a.gar.gradient_weights = np.full(3, 1 / 3, F)
    with pytest.raises(ValueError, match="unweighted"):
        sign_route(a, _clients())
    # schemes without a consumer of sign packets
    for agg in (_agg("krum"), _agg("spectral_gram", rank=2, adaptive_rank_th=0), _agg("geometric_median"), _agg("centered_clip", cclip_tau=1.0),
                _agg("trimmed_mean"), _agg("coordinate_median"), _agg(pc_analysis="gram")):
        with pytest.raises(NotImplementedError, match="sign packets"):
            sign_route(agg, _clients())
        with pytest.raises(NotImplementedError, match="sign packets"):
            agg.aggregate_grads(_clients())                            # before a GPU is touched
        assert sign_route(agg, _clients(fn="top")) is False            # their own route's business
    with pytest.raises(NotImplementedError, match="every client to compress with 'sign'"):
        _agg(M).aggregate_grads(_clients(fn="top"))


def test_aggregate_wire_refusals_on_host_bytes(lib):
    """What aggregate_wire refuses before any upload: a mixed round, a scheme without a consumer,
    a corrupted sign payload."""
    raw, n = accepted_payloads()["n=129"]
    import wire_model as wm
    from oracle import packet_oracle as po
    top = wm.pack(po.build_idxval(129, np.array([3]), F([1.0]), thresh=0, codec=po.CODEC_TOP, k=1))
    with pytest.raises(NotImplementedError, match="mixes sign packets"):
        _agg().aggregate_wire([raw, top])
    for scheme in ("krum", "trimmed_mean", "geometric_median"):
        with pytest.raises(NotImplementedError, match="sign packets"):
            _agg(scheme).aggregate_wire([raw, raw])
    with pytest.raises(NotImplementedError, match="sign packets"):
        _agg(pc_analysis="gram").aggregate_wire([raw, raw])
    bad = _put(raw, len(raw) - 4, 1, "<u4")
    for scheme in ("fed_avg", "sign_majority"):
        with pytest.raises(ValueError, match="payload 1: sign wire: pad word"):
            _agg(scheme).aggregate_wire([raw, bad])
    other = accepted_payloads()["n=128"][0]
    with pytest.raises(NotImplementedError, match="one length n"):
        _agg().aggregate_wire([raw, other])
    a = _agg("sign_majority")
    a.gar.gradient_weights = np.full(2, 0.5, F)
    with pytest.raises(ValueError, match="unweighted"):
        a.aggregate_wire([raw, raw])


def test_compression_refusals_without_a_gpu():
    from openmsftl_amd import Compression
    with pytest.raises(NotImplementedError):
        Compression({"compression_function": "sign"}).compress(np.zeros(4, F), layer_wise=True)
    with pytest.raises(NotImplementedError, match="'top' only"):
        Compression({"compression_function": "rand"}).compress_wire(np.zeros(4, F))
    with pytest.raises(NotImplementedError, match="'top' and 'sign'"):
        Compression({"compression_function": "rand", "error_feedback": True}).compress(np.zeros(4, F))
