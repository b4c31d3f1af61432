"""The wire format on the host: fc_wire_bytes, fc_wire_validate and codec.wire_from_host.

Run:  python -m pytest tests/test_wire_host.py -m "not gpu" -q

No GPU is needed: the library loads without one (tests/test_lib_abi.py).  Payloads come from
tests/wire_model.py; one mutation per check of the validator's list (include/fedcodec.h) must be
rejected with the message of that check.  The same corpus, and every truncation of small valid
payloads, goes through the stand-alone program tests/payload_validate_main.cc, built with the host
compiler and -fsanitize=address,undefined: the same verdicts and no sanitizer report.
"""
import ctypes
import re

import numpy as np
import pytest

import wire_model as wm
from oracle import packet_oracle as po
from payload_standalone import run, standalone  # noqa: F401  (standalone: a fixture)

CH, QU = po.CHUNK, po.QUARTER
N = 6 * CH + QU + 3
NS = [1, 8191, 8192, 8193, N]
ES = [0, 1, 7, 8, 9]


@pytest.fixture(scope="module")
def lib():
    from openmsftl_amd import build, _lib
    build.build(verbose=False)
    return _lib.load()


def validate(lib, raw: bytes, n_expected: int = 0):
    buf = ctypes.create_string_buffer(raw, len(raw))
    rc = lib.fc_wire_validate(ctypes.cast(buf, ctypes.c_void_p), len(raw), n_expected)
    return rc, (lib.fc_last_error() or b"").decode()


# ---- sizes ------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", NS)
def test_wire_bytes_equals_the_models_size(lib, n):
    prev = 0
    for E in ES:
        if E > n:
            continue
        got = int(lib.fc_wire_bytes(n, E))
        assert got == wm.wire_bytes(n, E) and got % 16 == 0, (n, E)
        assert got >= prev                                         # monotone in E
        prev = got
        gidx = np.arange(E, dtype=np.int64) * (n // max(E, 1)) if E else np.zeros(0, np.int64)
        f = po.build_idxval(n, gidx, np.ones(E, np.float32), thresh=0, codec=po.CODEC_TOP, k=E)
        assert len(wm.pack(f)) == got
    assert lib.fc_wire_bytes(0, 0) == 0 and lib.fc_wire_bytes(1 << 32, 0) == 0


# ---- payloads the validator accepts -----------------------------------------------------------
def base_fields(codec=po.CODEC_TOP, **kw):
    """Chunk 0: a full quarter 1 (2048 entries) and a few in quarters 0 and 3; chunks 1, 3 and 4
    empty; chunk 2 one entry per quarter; chunk 5 three entries; the last chunk (three elements into
    quarter 1) keeps its last element and two others.  E is odd: every section has a pad."""
    idx = np.concatenate([np.array([0, 5, 2047]), QU + np.arange(QU), np.array([3 * QU, CH - 1]),
                          2 * CH + np.array([1, QU + 1, 2 * QU + 1, 3 * QU + 1]),
                          5 * CH + np.array([QU - 1, QU, QU + 5]),
                          6 * CH + np.array([7, QU + 1, QU + 2])]).astype(np.int64)
    val = (np.arange(idx.size) % 17 - 8).astype(np.float32)
    val[val == 0] = np.float32(-0.0)
    kw.setdefault("thresh", 0)
    kw.setdefault("k", idx.size)
    return po.build_idxval(N, idx, val, codec=codec, **kw)


def accepted_payloads():
    out = {"base": (wm.pack(base_fields()), N)}
    out["empty"] = (wm.pack(po.build_idxval(N, np.zeros(0, np.int64), np.zeros(0, np.float32),
                                            thresh=int(po.NOTHING), codec=po.CODEC_TOP, k=0)), N)
    out["n=1"] = (wm.pack(po.build_idxval(1, np.array([0]), np.float32([2.5]), thresh=0,
                                          codec=po.CODEC_TOP, k=1)), 1)
    out["native rand"] = (wm.pack(base_fields(po.CODEC_RAND, key_mode=po.KEY_PHILOX, seed=77, offset=3)), N)
    out["dropout-unbiased"] = (wm.pack(base_fields(po.CODEC_DROPOUT_UNBIASED, p=0.25, seed=4)), N)
    # a top-k packet with slack below thresh: only the kept entries are in the payload
    f = base_fields()
    thresh = (int(po.mag_key(np.float32([3.0]))[0]) << po.index_bits(N)) | 0
    g = po.build_idxval(N, *po.listed_entries(f), thresh=thresh, lower=1, codec=po.CODEC_TOP, k=1)
    assert 0 < po.kept_entries(g)[0].size < po.listed_entries(g)[0].size
    out["top with slack"] = (wm.pack(g), N)
    return out


def test_the_base_payload_covers_what_it_claims():
    w = wm.parse(wm.pack(base_fields()))
    cnt = (w["qoff"] >> np.uint64(48)).astype(np.int64)
    q1 = (w["qoff"] & np.uint64(0xffff)).astype(np.int64)
    q2 = ((w["qoff"] >> np.uint64(16)) & np.uint64(0xffff)).astype(np.int64)
    assert list(cnt == 0) == [False, True, False, True, True, False, False]
    assert q2[0] - q1[0] == QU                                     # a full quarter
    E, L = int(w["hdr"]["n_entries"]), w["layout"]
    assert E == cnt.sum() and E % 2 == 1
    assert L["start"] > L["qoff"] + 8 * 7 and L["idx"] > L["start"] + 4 * 7
    assert L["val"] > L["idx"] + 2 * E and L["total"] > L["val"] + 4 * E
    assert 6 * CH + int(w["idx"][-1]) == N - 1                      # three elements into quarter 1


@pytest.mark.parametrize("name", sorted(accepted_payloads()))
def test_validator_accepts_model_payloads(lib, name):
    raw, n = accepted_payloads()[name]
    for n_expected in (0, n):
        rc, msg = validate(lib, raw, n_expected)
        assert rc == 0, msg


# ---- one mutation per check -------------------------------------------------------------------
def _put(raw: bytes, off: int, value, fmt: str) -> bytes:
    a = bytearray(raw)
    b = np.array([value], dtype=fmt).tobytes()
    a[off: off + len(b)] = b
    return bytes(a)


PKT = 32                                                           # fc_wire_hdr.pkt
OFF = {name: PKT + po.HDR_DTYPE.fields[name][1] for name in po.HDR_DTYPE.names}


def mutations():
    """name -> (payload, n_expected, the message its check gives)."""
    raw = wm.pack(base_fields())
    w = wm.parse(raw)
    L, E = w["layout"], int(w["hdr"]["n_entries"])
    qoff, start = w["qoff"], w["start"]

    def word(q1, q2, q3, cnt):
        return q1 | (q2 << 16) | (q3 << 32) | (cnt << 48)

    q = [int(qoff[0]) >> s & 0xffff for s in (0, 16, 32, 48)]
    last = L["idx"] + 2 * (E - 1)
    m = {
        "shorter than the header": (raw[:127], 0, "shorter than the 128-byte header"),
        "truncated by one byte": (raw[:-1], 0, r"total_bytes \d+ but \d+ bytes given"),
        "one extra byte": (raw + b"\0", 0, r"total_bytes \d+ but \d+ bytes given"),
        "wrong magic": (_put(raw, 0, 0x31574347, "<u4"), 0, "bad magic"),
        "wrong version": (_put(raw, 4, 2, "<u4"), 0, "unsupported version 2"),
        "wrong total_bytes": (_put(raw, 8, len(raw) + 16, "<u8"), 0, r"total_bytes \d+ but \d+ bytes given"),
        "n = 0": (_put(raw, OFF["n"], 0, "<u4"), 0, "n = 0"),
        "n_expected mismatch": (raw, N + 1, rf"n = {N} but {N + 1} expected"),
        "k above n": (_put(raw, OFF["k"], N + 1, "<u4"), 0, "above n"),
        "wrong index_bits": (_put(raw, OFF["index_bits"], 15, "<u4"), 0, "index_bits 15"),
        "wrong chunk": (_put(raw, OFF["chunk"], 4096, "<u4"), 0, "chunk 4096"),
        "bitmap format": (_put(raw, OFF["format"], 1, "<u4"), 0, "format 1 is not idx/val"),
        "codec 0": (_put(raw, OFF["codec"], 0, "<u4"), 0, "codec 0 outside"),
        "codec 5": (_put(raw, OFF["codec"], 5, "<u4"), 0, "codec 5 outside"),
        "key_mode 2": (_put(raw, OFF["key_mode"], 2, "<u4"), 0, "key_mode 2 outside"),
        "status 1": (_put(raw, 28, 1, "<u4"), 0, "status 1 / 0 is not OK"),
        "pkt status 1": (_put(raw, OFF["status"], 1, "<u4"), 0, "status 0 / 1 is not OK"),
        "wrong nch": (_put(raw, 24, 8, "<u4"), 0, "nch 8, 7 chunks"),
        "a wrong start word": (_put(raw, L["start"] + 4 * 3, int(start[3]) + 1, "<u4"), 0,
                               "chunk 3: start .* is not the prefix sum"),
        "start[0] not zero": (_put(raw, L["start"], 1, "<u4"), 0, "chunk 0: start 1 is not the prefix sum 0"),
        "q2 below q1": (_put(raw, L["qoff"], word(q[0], q[0] - 1, q[2], q[3]), "<u8"), 0,
                        "chunk 0: quarter offsets .* out of order"),
        "cnt = 8193": (_put(raw, L["qoff"], word(q[0], q[1], q[2], 8193), "<u8"), 0,
                       "chunk 0: quarter offsets .* count 8193 out of order or above 8192"),
        "two equal indices": (_put(raw, L["idx"] + 2 * 1, 0, "<u2"), 0, "entry 1: index 0 does not ascend"),
        "a descending pair": (_put(raw, L["idx"] + 2 * 2, 3, "<u2"), 0, "entry 2: index 3 does not ascend"),
        "an index in the wrong quarter": (_put(raw, L["idx"] + 2 * 2, 2048, "<u2"), 0,
                                          "entry 2: index 2048 is not in quarter 0"),
        "an index past n in the last chunk": (_put(raw, last, QU + 3, "<u2"), 0,
                                              rf"element {N} is past n = {N}"),
        "pkt.n_entries off by one": (_put(raw, OFF["n_entries"], E + 1, "<u4"), 0,
                                     rf"counts sum to {E}, n_entries {E}, pkt.n_entries {E + 1}"),
        "E off by one": (_put(raw, 16, E + 1, "<u8"), 0,
                         rf"counts sum to {E}, n_entries {E + 1}" if wm.wire_bytes(N, E + 1) == len(raw)
                         else "is not the size of"),
        "E huge": (_put(raw, 16, 1 << 62, "<u8"), 0, "is not the size of"),
    }
    pads = {"qoff": L["qoff"] + 8 * 7, "start": L["start"] + 4 * 7, "idx": L["idx"] + 2 * E,
            "val": L["total"] - 1}
    for name, off in pads.items():
        m[f"a non-zero pad byte after {name}"] = (_put(raw, off, 1, "<u1"), 0,
                                                  rf"pad byte at offset {off} is not zero")
    return m


MUTATIONS = sorted(mutations())


def test_the_mutation_list_covers_the_issue():
    for must in ("truncated by one byte", "one extra byte", "wrong magic", "wrong version",
                 "wrong total_bytes", "wrong nch", "a wrong start word", "q2 below q1", "cnt = 8193",
                 "two equal indices", "a descending pair", "an index in the wrong quarter",
                 "an index past n in the last chunk", "E off by one", "status 1",
                 "a non-zero pad byte after idx", "n_expected mismatch"):
        assert must in MUTATIONS


@pytest.mark.parametrize("name", MUTATIONS)
def test_validator_rejects_each_mutation_with_its_message(lib, name):
    raw, n_expected, want = mutations()[name]
    rc, msg = validate(lib, raw, n_expected)
    assert rc == -1, f"{name}: accepted"
    assert msg.startswith("wire: ") and re.search(want, msg), f"{name}: {msg!r}"


def test_wire_from_host_raises_before_any_device_work(lib, monkeypatch):
    from openmsftl_amd import codec
    import torch

    def no_device(*a, **k):
        raise AssertionError("device work started")
    monkeypatch.setattr(torch.cuda, "current_device", no_device)
    monkeypatch.setattr(torch, "from_numpy", no_device)
    raw, _, want = mutations()["a descending pair"]
    for data in (raw, np.frombuffer(raw, dtype=np.uint8), bytearray(raw)):
        with pytest.raises(ValueError, match=want):
            codec.wire_from_host(data)
    good = wm.pack(base_fields())
    with pytest.raises(ValueError, match="expected"):
        codec.wire_from_host(good, n=N + 1)
    with pytest.raises(TypeError):
        codec.wire_from_host(np.zeros(200, np.float32))
    with pytest.raises(AssertionError, match="device work started"):
        codec.wire_from_host(good, n=N)                              # a valid payload goes on to the copy


# ---- the same corpus through the sanitized stand-alone program --------------------------------
def test_the_corpus_through_the_sanitized_standalone_program(lib, standalone, tmp_path):
    exe, sanitized = standalone
    corpus = [(name, raw, n, None) for name, (raw, n) in sorted(accepted_payloads().items())]
    corpus += [(name,) + mutations()[name] for name in MUTATIONS]
    verdicts = run(exe, ["wire"], tmp_path, corpus)
    for (name, raw, n_expected, want), got in zip(corpus, verdicts):
        rc, msg = validate(lib, raw, n_expected)
        assert got == ("OK" if rc == 0 else "BAD " + msg), name         # the library's verdict
        if want is None:
            assert got == "OK", f"{name}: {got}"
        else:
            assert got.startswith("BAD wire: ") and re.search(want, got), f"{name}: {got}"
    print(f"{len(corpus)} payloads, sanitized build: {sanitized}")


def test_every_truncation_through_the_sanitized_standalone_program(standalone, tmp_path):
    """Each valid payload of n <= 100 cut at every length 0 .. size, each prefix in a heap block of
    exactly its length: only the whole payload is accepted and no read leaves a block."""
    exe, sanitized = standalone
    rng = np.random.default_rng(3)
    corpus = [("n=1", accepted_payloads()["n=1"][0], 0)]
    for n, E in ((1, 0), (7, 3), (64, 64), (100, 0), (100, 1), (100, 37)):
        gidx = np.sort(rng.choice(n, E, replace=False)).astype(np.int64)
        f = po.build_idxval(n, gidx, (np.arange(E) + 1).astype(np.float32), thresh=0, codec=po.CODEC_TOP, k=E)
        corpus.append((f"n={n} E={E}", wm.pack(f), 0))
    for (name, raw, _), got in zip(corpus, run(exe, ["wire", "--trunc"], tmp_path, corpus)):
        assert got == f"TRUNC ok=1 of={len(raw) + 1}", (name, got)
    print(f"{len(corpus)} payloads, sanitized build: {sanitized}")


def test_the_readers_rules_on_the_corpus_through_the_sanitized_program(lib, standalone, tmp_path):
    """wire_accept and wire_clamp (fc_wire_host.h: what k_wire_unpack and the wire fold do with bytes
    nobody validated) on the same corpus, each payload in a heap block of exactly its length: the
    program reads every entry of every clamped range and fails if one leaves [0, E)."""
    exe, sanitized = standalone
    corpus = [(name, raw, n) for name, (raw, n) in sorted(accepted_payloads().items())]
    corpus += [(name, mutations()[name][0], mutations()[name][1] or N) for name in MUTATIONS]
    lines = run(exe, ["wire", "--clamp"], tmp_path, corpus)
    got = dict(zip((name for name, _, _ in corpus), lines))
    for name, raw, n in corpus:
        # every payload: refused, or ranges inside [0, E) (the program checked them and read them)
        assert got[name] == "REJECT" or re.fullmatch(r"ACCEPT E=\d+ exact=[01]", got[name]), (name, got[name])
        if validate(lib, raw, n)[0] == 0:                           # a valid payload: the stored words
            E = int(wm.parse(raw)["hdr"]["n_entries"])
            assert got[name] == f"ACCEPT E={E} exact=1", (name, got[name])
    for name in ("shorter than the header", "truncated by one byte", "wrong magic", "wrong version",
                 "wrong nch", "n = 0", "n_expected mismatch", "E huge"):
        assert got[name] == "REJECT", (name, got[name])
    # a table word the readers take and bend into the packet
    for name in ("cnt = 8193", "q2 below q1"):
        assert got[name].endswith("exact=0"), (name, got[name])
    for name in ("a wrong start word", "start[0] not zero", "one extra byte"):
        assert got[name].startswith("ACCEPT"), (name, got[name])
    print(f"{len(corpus)} payloads, sanitized build: {sanitized}")
