"""QSGD with error feedback on the host: the model's hand cases, the C ABI of the new entry points,
fc_qsgd_wire_bytes, fc_qsgd_wire_validate, the Compression keys and the Aggregator's routing
predicates.

Run:  python -m pytest tests/test_qsgd_ef_host.py -m "not gpu" -q

No GPU is needed: the library loads without one (tests/test_lib_abi.py).  Payloads come from
tests/qsgd_ef_model.py; one mutation per rule of the validator's list (include/fedcodec.h) must be
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

import qsgd_ef_model as qm
from oracle import qsgd_oracle as qo
from payload_standalone import run, standalone  # noqa: F401  (standalone: a fixture)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = os.path.join(ROOT, "include", "fedcodec.h")
F = np.float32
NEW = ("fc_qsgd_encode_ef", "fc_qsgd_wire_bytes", "fc_qsgd_wire_validate")


@pytest.fixture(scope="module")
def lib():
    from openmsftl_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


# ---- the model on hand cases --------------------------------------------------------------------
def test_model_the_add_turns_minus_zero_into_plus_zero():
    g = np.array([-0.0, 0.0, -1.0, 2.0], F)
    assert list(np.signbit(qm.encoded(g))) == [True, False, True, False]
    assert list(np.signbit(qm.encoded(g, np.zeros(4, F)))) == [False, False, True, False]
    # the sign bit of -0.0 reaches the code only without a residual
    W = qo.width(2)
    c0 = qo.unpack(qm.encode(g, None, 2, 1, 1)[2], 4, 2)
    c1 = qo.unpack(qm.encode(g, np.zeros(4, F), 2, 1, 1)[2], 4, 2)
    assert int(c0[0]) >> (W - 1) == 1 and int(c1[0]) >> (W - 1) == 0


def test_model_a_level_is_clamped_to_s_and_the_residual_follows():
    # a one-hot: s |a| / norm = s exactly, plus a dither in [0, 1): floor gives s, never s + 1
    for bits in (1, 2, 6, 14):
        s = 2 ** bits
        g = np.zeros(9, F)
        g[4] = -3.0
        e = np.zeros(9, F)
        e[4] = 0.5
        a, norm, words, q, e2 = qm.encode(g, e, bits, 7, 3)
        assert norm == 2.5 and a[4] == F(-2.5)
        lev = qo.unpack(words, 9, bits) & np.uint32((1 << (qo.width(bits) - 1)) - 1)
        assert int(lev[4]) == s and not lev[[0, 1, 2, 3, 5, 6, 7, 8]].any()
        want = F(-(2.5 / (s * qo.tau(9, float(s))) * s))
        assert q[4] == want and e2[4] == F(F(-2.5) - want)
        assert e2[[0, 1, 2, 3, 5, 6, 7, 8]].tobytes() == np.zeros(8, F).tobytes()
    # the fp32 product may overshoot s: levels_from_dither clamps, whatever the dither
    lev = qo.levels_from_dither(np.array([np.nextafter(F(1.0), F(2.0))], F), np.array([65535]), 14, 1.0)
    assert int(lev[0]) == 2 ** 14


def test_model_nan_is_level_zero_and_poisons_the_residual():
    g = np.array([1.0, np.nan, -2.0, 0.5], F)
    a, norm, words, q, e2 = qm.encode(g, np.zeros(4, F), 2, 5, 9)
    assert np.isnan(norm)
    lev = qo.unpack(words, 4, 2) & np.uint32(7)
    assert not lev.any()                                   # every level is 0 under a NaN norm
    assert np.isnan(q).all() or (q == 0).all()
    assert np.isnan(e2[1])
    # a NaN in e alone does the same through the add
    a2 = qm.encoded(np.ones(4, F), np.array([0, np.nan, 0, 0], F))
    assert np.isnan(a2[1]) and a2[0] == 1.0


def test_model_wire_layout():
    g = np.arange(1, 10, dtype=F)
    _, norm, words, _, _ = qm.encode(g, None, 6, 3, 4)
    raw = qm.pack(9, 6, 3, 4, norm, words)
    assert len(raw) == qm.wire_bytes(9, 6) == 128 + 16 and words.size == 4
    P = qm.parse(raw)
    assert int(P["hdr"]["magic"]) == 0x31514346 and raw[:4] == b"FCQ1"
    assert (int(P["hdr"]["pkt"]["n"]), int(P["hdr"]["pkt"]["k"]), int(P["hdr"]["pkt"]["codec"])) == (9, 6, 5)
    assert P["words"].tobytes() == words.tobytes()
    assert qm.wire_bytes(9, 2) == 128 + 16 and qm.code_words(9, 2) == 2     # two pad words
    assert qm.wire_bytes(9, 0) == 0 and qm.wire_bytes(9, 15) == 0


# ---- the C ABI ----------------------------------------------------------------------------------
def _declarations():
    src = re.sub(r"/\*.*?\*/", "", open(HEADER).read(), flags=re.S)
    out = {}
    for name, args in re.findall(r"\b(fc_qsgd_[a-z0-9_]+)\s*\(([^;{]*?)\)\s*;", src, flags=re.S):
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
    assert lib.fc_abi_version() == 4                                   # additive: no bump
    assert _lib.QSGD_MAGIC == qm.MAGIC and ctypes.sizeof(_lib.QsgdWireHdr) == 128
    for f, (name, _) in zip(qm.WIRE_HDR.names, _lib.QsgdWireHdr._fields_):
        assert f == name and getattr(_lib.QsgdWireHdr, name).offset == qm.WIRE_HDR.fields[f][1]


@pytest.mark.parametrize("bits", [1, 2, 3, 6, 7, 14])
def test_wire_bytes_against_the_model(lib, bits):
    for n in (1, 7, 8, 9, 31, 32, 33, 4097, 2 ** 32 - 1):
        assert lib.fc_qsgd_wire_bytes(n, bits) == qm.wire_bytes(n, bits), n
        assert lib.fc_qsgd_code_words(n, bits) == qm.code_words(n, bits), n
        assert (lib.fc_qsgd_wire_bytes(n, bits) - 128) % 16 == 0
    for bad in (0, 15, -1):
        assert lib.fc_qsgd_wire_bytes(100, bad) == 0


def test_encode_ef_argument_errors_do_not_touch_gpu(lib):
    buf = ctypes.create_string_buffer(1 << 14)
    a = (ctypes.addressof(buf) + 15) & ~15
    ws = lib.fc_qsgd_workspace_bytes()                    # a size only: every call below fails first
    good = dict(g=a, ri=a + 1024, ro=a + 2048, n=64, bits=2, codes=a + 3072, cw=8, hdr=a + 4096,
                ws=a + 5120, wsb=ws)
    assert lib.fc_qsgd_code_words(64, 2) == 8

    def enc(**kw):
        p = dict(good, **kw)
        return lib.fc_qsgd_encode_ef(p["g"], p["ri"], p["ro"], p["n"], p["bits"], 1, 2, p["codes"],
                                     p["cw"], p["hdr"], p["ws"], p["wsb"], None)
    err = lambda: lib.fc_last_error()                                  # noqa: E731
    assert enc(g=None) == -1 and b"NULL" in err()
    assert enc(codes=None) == -1 and enc(hdr=None) == -1 and enc(ws=None) == -1
    assert enc(bits=0) == -1 and b"bits=0" in err()
    assert enc(bits=15) == -1 and b"bits=15" in err()
    assert enc(n=0) == -1 and b"n=0" in err()
    assert enc(n=1 << 32) == -1
    assert enc(g=a + 4) == -1 and b"aligned" in err()
    assert enc(ri=a + 1028) == -1 and enc(ro=a + 2052) == -1 and enc(codes=a + 3076) == -1
    assert enc(ro=a) == -1 and b"overlap g" in err()                   # e' on g
    assert enc(ro=a + 128) == -1 and b"overlap g" in err()
    assert enc(ro=a + 1024) == -1 and b"overlap res_in" in err()       # e' on e
    assert enc(ro=a + 1024 + 128) == -1 and b"overlap res_in" in err()
    assert enc(ro=a + 1024 - 128) == -1 and b"overlap" in err()
    assert enc(cw=7) == -1 and b"code_words" in err()
    assert enc(bits=14, cw=31) == -1 and b"code_words" in err()
    assert enc(wsb=16) == -3 and b"workspace" in err()
    # every combination of residual pointers reports the same errors first
    for kw in (dict(ri=None), dict(ro=None), dict(ri=None, ro=None)):
        assert enc(n=0, **kw) == -1 and enc(cw=7, **kw) == -1 and enc(wsb=16, **kw) == -3
    assert lib.fc_qsgd_wire_validate(None, 0, 0) == -1 and b"NULL" in err()


# ---- the validator ------------------------------------------------------------------------------
N, BITS = 4099, 2                  # W = 4: a last group of 3 elements, 513 code words, 3 pad words


def validate(lib, raw: bytes, n_expected: int = 0):
    buf = ctypes.create_string_buffer(raw, len(raw))
    rc = lib.fc_qsgd_wire_validate(ctypes.cast(buf, ctypes.c_void_p), len(raw), n_expected)
    return rc, (lib.fc_last_error() or b"").decode()


def _payload(n, bits, seed=0, norm=None, offset=5):
    rng = np.random.default_rng(seed + 100 * bits + n)
    g = rng.standard_normal(n).astype(F)
    _, nm, words, _, _ = qm.encode(g, 0.5 * rng.standard_normal(n).astype(F), bits, seed, offset)
    return qm.pack(n, bits, seed, offset, nm if norm is None else norm, words)


def accepted_payloads():
    out = {f"n={n} bits={b}": (_payload(n, b, n), n) for n in (1, 7, 8, 9, 33, 4099) for b in (1, 2, 6, 14)}
    out["zero norm"] = (qm.pack(65, 2, 0, 0, 0.0, np.zeros(qm.code_words(65, 2), "<u4")), 65)
    out["inf norm"] = (_payload(65, 6, 2, norm=np.inf), 65)
    out["nan norm"] = (_payload(65, 6, 3, norm=np.nan), 65)
    out["negative nan norm"] = (_put(_payload(65, 6, 3), qm.OFF["pkt.p"], 0xFFF8000000000000, "<u8"), 65)
    out["a norm that is no float32"] = (_payload(65, 14, 4, norm=0.1), 65)
    out["a double denormal norm"] = (_payload(65, 14, 4, norm=5e-324), 65)
    out["any seed and offset"] = (qm.pack(8, 1, 2 ** 64 - 1, 2 ** 63 + 5, 1.0, np.zeros(1, "<u4")), 8)
    # every level at s with the sign set: the largest code the encoder writes
    for b in (1, 2, 6, 14):
        W = qo.width(b)
        code = (1 << (W - 1)) | (1 << b)
        word = sum(code << (W * j) for j in range(32 // W))
        out[f"every level s, bits={b}"] = (qm.pack(16, b, 1, 1, 2.0, np.full(qm.code_words(16, b), word, "<u4")), 16)
    return out


def _put(raw: bytes, off: int, value, fmt: str) -> bytes:
    a = bytearray(raw)
    b = np.array([value], dtype=fmt).tobytes()
    a[off: off + len(b)] = b
    return bytes(a)


def _or(raw: bytes, off: int, value: int) -> bytes:
    return _put(raw, off, int(np.frombuffer(raw, "<u4", 1, off)[0]) | value, "<u4")


def mutations():
    """name -> (bytes, n_expected, the message's pattern): one field changed per rule."""
    base, O = _payload(N, BITS, 7), qm.OFF
    assert N % 8 == 3 and qm.code_words(N, BITS) == 513 and qm.wire_words(N, BITS) == 516
    codes = qm.WIRE_HDR_BYTES
    last = codes + 4 * (N // 8)                              # the word of the last (partial) group
    b6 = _payload(33, 6, 1)                                  # W = 8: 5 groups, 10 words, 2 pad words
    b14 = _payload(33, 14, 1)                                # W = 16: 20 words, no pad word
    m = {
        "shorter than the header": (base[:127], 0, "shorter than the 128-byte header"),
        "truncated by one byte": (base[:-1], 0, "total_bytes"),
        "one extra byte": (base + b"\0", 0, "total_bytes"),
        "sixteen extra bytes, total_bytes following": (
            _put(base + b"\0" * 16, O["total_bytes"], len(base) + 16, "<u8"), 0, "is not the size of n"),
        "wrong magic": (_put(base, O["magic"], 0x31534346, "<u4"), 0, "bad magic"),
        "wrong version": (_put(base, O["version"], 2, "<u4"), 0, "unsupported version"),
        "reserved bytes": (_put(base, O["zero"] + 12, 1, "<u4"), 0, "reserved bytes"),
        "n = 0": (_put(base, O["pkt.n"], 0, "<u4"), 0, "n = 0"),
        "n_expected mismatch": (base, N + 1, "expected"),
        "codec top": (_put(base, O["pkt.codec"], 1, "<u4"), 0, "codec 1 is not qsgd"),
        "codec sign": (_put(base, O["pkt.codec"], 6, "<u4"), 0, "codec 6 is not qsgd"),
        "format idx/val": (_put(base, O["pkt.format"], 0, "<u4"), 0, "format 0 is not qsgd"),
        "bits 0": (_put(base, O["pkt.k"], 0, "<u4"), 0, r"k = 0 bits outside \[1, 14\]"),
        "bits 15": (_put(base, O["pkt.k"], 15, "<u4"), 0, r"k = 15 bits outside \[1, 14\]"),
        "n_entries below n": (_put(base, O["pkt.n_entries"], N - 1, "<u4"), 0, "n_entries = "),
        "status retry": (_put(base, O["pkt.status"], 1, "<u4"), 0, "status 1 is not OK"),
        "key_mode magnitude": (_put(base, O["pkt.key_mode"], 0, "<u4"), 0, "key_mode 0 is not philox"),
        "negative norm": (_put(base, O["pkt.p"], -0.5, "<f8"), 0, "negative"),
        "minus zero norm": (_put(base, O["pkt.p"], -0.0, "<f8"), 0, "negative"),
        "minus inf norm": (_put(base, O["pkt.p"], -np.inf, "<f8"), 0, "negative"),
        "bits 6 on a 2-bit payload": (_put(base, O["pkt.k"], 6, "<u4"), 0, "is not the size of n"),
        "n larger, the same bytes": (_put(_put(base, O["pkt.n"], N + 200, "<u4"), O["pkt.n_entries"], N + 200, "<u4"),
                                     0, "is not the size of n"),
        # W = 4 at bits = 2: the level field holds 0..7, s = 4
        "level 5 at bits 2": (_put(base, codes, (int(np.frombuffer(base, "<u4", 1, codes)[0]) & ~0x7) | 5, "<u4"),
                              0, "element 0 has level 5 above s = 4"),
        "level 7 in the last group": (_put(base, last, (int(np.frombuffer(base, "<u4", 1, last)[0]) & ~0x700) | 0x700, "<u4"),
                                      0, f"element {N - 1} has level 7 above s = 4"),
        "level 65 at bits 6": (_put(b6, codes + 5, 65, "u1"), 0, "element 5 has level 65 above s = 64"),
        "level 16385 at bits 14": (_put(b14, codes + 2 * 32, 0x8000 | 16385, "<u2"), 0,
                                   "element 32 has level 16385 above s = 16384"),
        "a code at n": (_or(base, last, 1 << 12), 0, "code at or past n"),
        "a sign bit in the last slot of the last group": (_or(base, last, 1 << 31), 0, "code at or past n"),
        "a code past n at bits 6, second word of the group": (_or(b6, codes + 4 * 9, 1 << 24), 0, "code at or past n"),
        "a code at n at bits 6": (_or(b6, codes + 4 * 8, 1 << 8), 0, "code at or past n"),
        "a code at n at bits 14": (_or(b14, codes + 4 * 16, 1 << 16), 0, "code at or past n"),
        "a code in the last word at bits 14": (_or(b14, codes + 4 * 19, 1), 0, "code at or past n"),
        "first pad word": (_put(base, codes + 4 * 513, 1, "<u4"), 0, "pad word 513"),
        "last pad word": (_put(base, len(base) - 4, 1 << 31, "<u4"), 0, "pad word 515"),
        "pad word at bits 6": (_put(b6, len(b6) - 4, 1, "<u4"), 0, "pad word 11"),
    }
    for f in ("thresh", "lower"):
        m[f"{f} not zero"] = (_put(base, O[f"pkt.{f}"], 1, "<u8"), 0, "must be zero")
    for f in ("index_bits", "n_definite", "n_cand", "chunk"):
        m[f"{f} not zero"] = (_put(base, O[f"pkt.{f}"], 1, "<u4"), 0, "must be zero")
    for i in range(3):
        m[f"reserved[{i}] not zero"] = (_put(base, O["pkt.reserved"] + 4 * i, 1, "<u4"), 0, "must be zero")
    return m


MUTATIONS = sorted(mutations())


@pytest.mark.parametrize("name", sorted(accepted_payloads()))
def test_validator_accepts_model_payloads(lib, name):
    raw, n = accepted_payloads()[name]
    bits = int(qm.parse(raw)["hdr"]["pkt"]["k"])
    assert len(raw) == qm.wire_bytes(n, bits) == lib.fc_qsgd_wire_bytes(n, bits)
    for n_expected in (0, n):
        rc, msg = validate(lib, raw, n_expected)
        assert rc == 0, msg


@pytest.mark.parametrize("name", MUTATIONS)
def test_validator_rejects_each_mutation_with_its_reason(lib, name):
    raw, n_expected, want = mutations()[name]
    rc, msg = validate(lib, raw, n_expected)
    assert rc == -1 and msg.startswith("qsgd wire: ") and re.search(want, msg), msg


@pytest.mark.parametrize("bits", [1, 2, 3, 6, 7, 14])
def test_level_rule_for_every_code_value_and_place(lib, bits):
    """The validator tests two words at a time and walks a pair code by code only for the message:
    every code value (every 5th at W = 16, and the ones around s) in a first, a middle and a last
    place is accepted exactly when its level is at most s."""
    n, W = 40, qo.width(bits)
    s, lmask = 2 ** bits, (1 << (W - 1)) - 1
    words = np.zeros(qm.code_words(n, bits), "<u4")
    values = set(range(0, 1 << W, 5 if W == 16 else 1)) | {s - 1, s, s + 1, (1 << (W - 1)) | s, (1 << (W - 1)) | (s + 1), (1 << W) - 1}
    per = 32 // W
    for el in (0, 19, n - 1):
        for v in sorted(values):
            w = words.copy()
            w[el // per] = v << (W * (el % per))
            rc, msg = validate(lib, qm.pack(n, bits, 0, 0, 1.0, w))
            if (v & lmask) <= s:
                assert rc == 0, (el, v, msg)
            else:
                assert rc == -1 and f"element {el} has level {v & lmask} above s = {s}" in msg, (el, v, msg)


def test_every_truncation_is_rejected(lib):
    for name in ("n=1 bits=1", "n=9 bits=2", "n=33 bits=6", "n=33 bits=14"):
        raw, _ = accepted_payloads()[name]
        for cut in range(len(raw)):
            assert validate(lib, raw[:cut])[0] == -1, (name, cut)
        assert validate(lib, raw)[0] == 0


def test_the_validators_reject_each_others_bytes(lib):
    import sign_model as sm
    import wire_model as wm
    from oracle import packet_oracle as po
    from openmsftl_amd import codec
    raw, n = accepted_payloads()["n=4099 bits=2"]
    buf = ctypes.create_string_buffer(raw, len(raw))
    for fn in (lib.fc_wire_validate, lib.fc_sign_wire_validate):
        assert fn(ctypes.cast(buf, ctypes.c_void_p), len(raw), 0) == -1
        assert b"bad magic" in lib.fc_last_error()
    with pytest.raises(ValueError, match="bad magic"):
        codec.TOP.check(raw)
    with pytest.raises(ValueError, match="bad magic"):
        codec.SIGN.check(raw)
    sign = sm.pack(129, 1.0, sm.words_of(np.ones(129, bool)))
    top = wm.pack(po.build_idxval(129, np.array([3]), F([1.0]), thresh=0, codec=po.CODEC_TOP, k=1))
    for other in (sign, top):
        rc, msg = validate(lib, other)
        assert rc == -1 and "bad magic" in msg
        with pytest.raises(ValueError, match="qsgd wire: bad magic"):
            codec.QSGD.check(other)
        assert not codec.is_qsgd_payload(other)
    assert codec.is_qsgd_payload(raw) and not codec.is_sign_payload(raw)
    assert not codec.is_qsgd_payload(b"FCQ") and not codec.is_qsgd_payload(b"FCS1" + raw[4:])
    a, h = codec.QSGD.check(raw, n)
    assert int(h.pkt.n) == n and int(h.pkt.k) == 2 and a.size == len(raw)
    with pytest.raises(ValueError, match="expected"):
        codec.QSGD.check(raw, n + 1)
    with pytest.raises(ValueError, match="at least 1"):
        codec.QSGD.check(raw, 0)
    assert codec.qsgd_wire_bytes(n, 2) == len(raw)
    with pytest.raises(ValueError, match="bits=15"):
        codec.qsgd_wire_bytes(n, 15)


# ---- the same corpus through the sanitized stand-alone program --------------------------------
def test_the_corpus_through_the_sanitized_standalone_program(lib, standalone, tmp_path):
    exe, sanitized = standalone
    corpus = [(name, raw, n) for name, (raw, n) in sorted(accepted_payloads().items())]
    corpus += [(name,) + mutations()[name][:2] for name in MUTATIONS]
    for (name, raw, n_expected), got in zip(corpus, run(exe, ["qsgd"], tmp_path, corpus)):
        rc, msg = validate(lib, raw, n_expected)
        assert got == ("OK" if rc == 0 else "BAD " + msg), name         # the library's verdict
        if name in mutations():
            assert got.startswith("BAD qsgd wire: ") and re.search(mutations()[name][2], got), f"{name}: {got}"
        else:
            assert got == "OK", f"{name}: {got}"
    print(f"{len(corpus)} payloads, sanitized build: {sanitized}")


def test_every_truncation_through_the_sanitized_standalone_program(standalone, tmp_path):
    """Each valid payload cut at every length 0 .. size, each prefix in a heap block of exactly its
    length: only the whole payload is accepted and no read leaves a block."""
    exe, sanitized = standalone
    corpus = [(name, raw, 0) for name, (raw, n) in sorted(accepted_payloads().items()) if n <= 100]
    corpus += [("mutated " + name, mutations()[name][0], 0) for name in MUTATIONS[:6]]
    for (name, raw, _), got in zip(corpus, run(exe, ["qsgd", "--trunc"], tmp_path, corpus)):
        want = 0 if name.startswith("mutated ") else 1
        assert got == f"TRUNC ok={want} of={len(raw) + 1}", (name, got)
    print(f"{len(corpus)} payloads, sanitized build: {sanitized}")


# ---- Compression --------------------------------------------------------------------------------
NATIVE = {"compression_function": "qsgd", "qsgd": "native"}


def test_compression_keys_without_a_gpu():
    from openmsftl_amd import Compression
    C = Compression(dict(NATIVE, error_feedback=True, num_bits=3))
    assert C.error_feedback is True and C.get_residual() is None and C.num_bits == 3
    # the routing, without a GPU: compress hands the gradient to _qsgd, compress_wire to the packet
    seen = []
    C._qsgd = lambda g: seen.append(("dense", g)) or "q"
    C._qsgd_packet = lambda g: seen.append(("packet", g))
    x0 = np.zeros(4, F)
    assert C.compress(x0) == "q" and seen[0][0] == "dense" and seen[0][1] is x0
    with pytest.raises(ValueError, match="empty gradient"):            # what a None packet means
        C.compress_wire(x0)
    assert len(seen) == 2 and seen[1][0] == "packet" and seen[1][1] is x0
    with pytest.raises(NotImplementedError):
        C.compress(np.zeros(4, F), layer_wise=True)
    # without "qsgd": "native" the codec keeps raising, with or without error feedback
    x = np.ones(8, F)
    for cfg in ({"compression_function": "qsgd"}, {"compression_function": "qsgd", "error_feedback": True},
                {"compression_function": "qsgd", "qsgd": "reference", "error_feedback": True}):
        with pytest.raises(NotImplementedError):
            Compression(cfg).compress(x)
        with pytest.raises(NotImplementedError, match="'top' only"):
            Compression(cfg).compress_wire(x)
    with pytest.raises(NotImplementedError, match="'top' and 'sign' only, and for 'qsgd' with \"qsgd\": \"native\""):
        Compression({"compression_function": "rand", "error_feedback": True}).compress(x)
    with pytest.raises(NotImplementedError, match="native 'qsgd'"):
        Compression({"compression_function": "rand"}).compress_wire(x)


# ---- the routing predicates on stub clients -----------------------------------------------------
def _clients(m=3, n=100, dtype=F, cfg=NATIVE, **more):
    from openmsftl_amd import Compression
    return [types.SimpleNamespace(C=Compression(dict(cfg, **more)), grad=np.zeros(n, dtype), client_id=i)
            for i in range(m)]


def _agg(scheme="fed_avg", **cfg):
    from openmsftl_amd.aggregation import Aggregator
    return Aggregator(dict({"aggregation_scheme": scheme}, **cfg))


def test_qsgd_route_conditions_on_stub_clients(lib):
    from openmsftl_amd.aggregation import qsgd_route, round_route
    on = dict(qsgd_packets=True)
    assert qsgd_route(_agg(**on), _clients()) is True
    assert round_route(_agg(**on), _clients()) == ("qsgd", None)
    assert qsgd_route(_agg(**on), _clients(error_feedback=True)) is True
    mixed = _clients(2, num_bits=2) + _clients(1, num_bits=12, error_feedback=True) + _clients(1, num_bits=1)
    assert qsgd_route(_agg(**on), mixed) is True
    # the key off: today's routing
    assert qsgd_route(_agg(), _clients()) is False and round_route(_agg(), _clients()) is None
    assert qsgd_route(_agg(qsgd_packets=False), _clients()) is False
    # outside the conditions the round goes on down the table
    for agg, cl in (
            (_agg("krum", **on), _clients()),
            (_agg("trimmed_mean", **on), _clients()),
            (_agg("sign_majority", **on), _clients()),
            (_agg(pc_analysis="gram", **on), _clients()),
            (_agg(num_hierarchies=1, cluster_size_list=[2], **on), _clients()),
            (_agg(devices=2, **on), _clients()),
            (_agg(**on), _clients() + _clients(1, cfg={"compression_function": "top"})),
            (_agg(**on), _clients() + _clients(1, cfg={"compression_function": "sign"})),
            (_agg(**on), _clients() + _clients(1, cfg={"compression_function": "qsgd"})),       # not native
            (_agg(**on), _clients(dtype=np.float64)),
            (_agg(**on), _clients() + _clients(1, n=101)),
            (_agg(**on), _clients(n=0)),
            (_agg(**on), _clients(num_bits=0)),
            (_agg(**on), _clients(num_bits=15)),
            (_agg(**on), _clients(num_bits=2.5)),
            (_agg(**on), [])):
        assert qsgd_route(agg, cl) is False
    a = _agg(**on)
    a.gar.gradient_weights = np.full(3, 1 / 3, np.float64)
    assert qsgd_route(a, _clients()) is False
    a.gar.gradient_weights = np.full(3, 1 / 3, F)
    assert qsgd_route(a, _clients()) is True
    stub = _clients()
    stub[1].C = types.SimpleNamespace(compression_function="qsgd", qsgd="native", num_bits=2,
                                      error_feedback=False)
    assert qsgd_route(_agg(**on), stub) is False                      # not the drop-in Compression
    # a round of 'sign' clients keeps its own route with the key set
    sign = _clients(cfg={"compression_function": "sign"})
    assert round_route(_agg(**on), sign) == ("sign", None)


def test_aggregate_wire_refusals_on_host_bytes(lib):
    """What aggregate_wire refuses before any upload: a mixed round, a scheme without a consumer,
    a corrupted payload, payloads of differing n."""
    import sign_model as sm
    import wire_model as wm
    from oracle import packet_oracle as po
    raw, n = accepted_payloads()["n=33 bits=6"]
    sign = sm.pack(33, 1.0, sm.words_of(np.ones(33, bool)))
    top = wm.pack(po.build_idxval(33, np.array([3]), F([1.0]), thresh=0, codec=po.CODEC_TOP, k=1))
    for other in (sign, top):
        for payloads in ([raw, other], [other, raw]):
            with pytest.raises(NotImplementedError, match="mixes QSGD packets"):
                _agg().aggregate_wire(payloads)
    for scheme in ("krum", "trimmed_mean", "geometric_median", "sign_majority"):
        with pytest.raises(NotImplementedError, match="fed_avg for QSGD packets"):
            _agg(scheme).aggregate_wire([raw, raw])
    with pytest.raises(NotImplementedError, match="fed_avg for QSGD packets"):
        _agg(pc_analysis="gram").aggregate_wire([raw, raw])
    with pytest.raises(NotImplementedError, match="no hierarchies"):
        _agg(num_hierarchies=1, cluster_size_list=[2]).aggregate_wire([raw, raw])
    with pytest.raises(NotImplementedError, match="one device"):
        _agg(devices=2).aggregate_wire([raw, raw])
    a = _agg()
    a.gar.gradient_weights = np.full(2, 0.5, np.float64)
    with pytest.raises(NotImplementedError, match="float32 GAR weights"):
        a.aggregate_wire([raw, raw])
    bad = _put(raw, len(raw) - 4, 1, "<u4")
    with pytest.raises(ValueError, match="payload 1: qsgd wire: pad word"):
        _agg().aggregate_wire([raw, bad])
    other_n = accepted_payloads()["n=9 bits=6"][0]
    with pytest.raises(NotImplementedError, match="one length n"):
        _agg().aggregate_wire([raw, other_n])
    with pytest.raises(NotImplementedError, match="one length n"):
        _agg().aggregate_wire([raw, raw], n=34)
