"""NumPy model of QSGD with error feedback and of the QSGD packet's wire form (include/fedcodec.h,
"QSGD with error feedback"), on top of the unchanged oracle/qsgd_oracle.py.  A test model: the
product does not import it.

For a float32 gradient g[n], an optional float32 residual e[n], bits in 1..14 and a Philox key:
  a     = fl32(g + e)               (g itself without a residual)
  codes = qo.encode(a, bits, seed, offset, norm)     norm: ||a||_2 in float64 (the device records
                                                      its own fixed-order sum in the header)
  q     = qo.decode(codes, n, bits, norm)
  e'    = fl32(a - q)
"""
import numpy as np

from oracle import qsgd_oracle as qo

F = np.float32
CODEC_QSGD, FMT_QSGD, KEY_PHILOX = 5, 2, 1
MAGIC, VERSION = 0x31514346, 1                       # "FCQ1"
HDR_BYTES, WIRE_HDR_BYTES = 96, 128

HDR = np.dtype([("thresh", "<u8"), ("lower", "<u8"), ("n", "<u4"), ("k", "<u4"),
                ("n_entries", "<u4"), ("index_bits", "<u4"), ("codec", "<u4"), ("status", "<u4"),
                ("n_definite", "<u4"), ("n_cand", "<u4"), ("seed", "<u8"), ("offset", "<u8"),
                ("p", "<f8"), ("chunk", "<u4"), ("format", "<u4"), ("key_mode", "<u4"),
                ("reserved", "<u4", (3,))])
WIRE_HDR = np.dtype([("magic", "<u4"), ("version", "<u4"), ("total_bytes", "<u8"),
                     ("zero", "<u4", (4,)), ("pkt", HDR)])
assert HDR.itemsize == HDR_BYTES and WIRE_HDR.itemsize == WIRE_HDR_BYTES


def encoded(g, e=None):
    """a: g itself, or fl32(g + e), one IEEE add per element."""
    g = np.asarray(g, F)
    if e is None:
        return g.copy()
    with np.errstate(all="ignore"):
        return (g + np.asarray(e, F)).astype(F)


def residual(a, q):
    """e' = fl32(a - q), one IEEE subtract per element."""
    with np.errstate(all="ignore"):
        return (np.asarray(a, F) - np.asarray(q, F)).astype(F)


def encode(g, e, bits: int, seed: int, offset: int, norm=None):
    """(a, norm, code words, q, e') of one encode; ``norm``: the norm to use instead of norm64(a)
    (the device's header norm)."""
    a = encoded(g, e)
    with np.errstate(all="ignore"):
        norm = qo.norm64(a) if norm is None else float(norm)
        words = qo.encode(a, bits, seed, offset, norm)
        q = qo.decode(words, a.size, bits, norm)
    return a, norm, words, q, residual(a, q)


def code_words(n: int, bits: int) -> int:
    return (n + 7) // 8 * (qo.width(bits) // 4)


def wire_words(n: int, bits: int) -> int:
    return (code_words(n, bits) + 3) // 4 * 4


def wire_bytes(n: int, bits: int) -> int:
    """128 + 4 * (the code words rounded up to a multiple of 4); 0 for bits outside [1, 14]."""
    if not 1 <= bits <= 14:
        return 0
    return WIRE_HDR_BYTES + 4 * wire_words(n, bits)


def header(n: int, bits: int, seed: int, offset: int, norm) -> np.ndarray:
    h = np.zeros((), dtype=HDR)
    h["n"] = h["n_entries"] = n
    h["k"], h["codec"], h["format"], h["key_mode"] = bits, CODEC_QSGD, FMT_QSGD, KEY_PHILOX
    h["seed"], h["offset"], h["p"] = seed, offset, np.float64(norm)
    return h


def pack(n: int, bits: int, seed: int, offset: int, norm, words) -> bytes:
    """The wire form: the 128-byte header, the code words, zero words up to a multiple of 4."""
    words = np.asarray(words, "<u4")
    assert words.size == code_words(n, bits)
    h = np.zeros((), dtype=WIRE_HDR)
    h["magic"], h["version"], h["total_bytes"] = MAGIC, VERSION, wire_bytes(n, bits)
    h["pkt"] = header(n, bits, seed, offset, norm)
    pad = np.zeros(wire_words(n, bits) - words.size, "<u4")
    return h.tobytes() + words.tobytes() + pad.tobytes()


def parse(raw: bytes):
    h = np.frombuffer(raw[:WIRE_HDR_BYTES], dtype=WIRE_HDR)[0]
    return {"hdr": h, "words": np.frombuffer(raw[WIRE_HDR_BYTES:], dtype="<u4")}


#: byte offsets of the wire header's fields (for one-field mutations)
OFF = {"magic": 0, "version": 4, "total_bytes": 8, "zero": 16, "pkt": 32}
OFF.update({f"pkt.{name}": 32 + HDR.fields[name][1] for name in HDR.names})
