"""NumPy restatement of the scaled-sign codec (include/fedcodec.h, "scaled sign with error
feedback"): the encoded vector, the scale, the bits, the decode, the residual, the FedAVG fold, the
majority vote and the wire bytes.  A test model: the product does not import it.

For a float32 gradient g[n] and an optional float32 residual e[n]:
  a  = fl32(g + e)                 (g itself without a residual)
  S  = sum (double)|a|,  s = fl32(S / n)
  b  = the IEEE sign bit of a, bit t % 32 of uint32 word t // 32, sign_words(n) words
  q  = -s where b is set, +s elsewhere;   e' = fl32(a - q)
The device adds the |a| in float64 in an order fixed by n, which this model does not restate.  It
holds instead the true sum (math.fsum) and the rounding bound of ANY order of float64 summation of
n non-negative terms (Higham, Accuracy and Stability of Numerical Algorithms, eq. 4.4 with every
term of one sign): |S^ - S| <= gamma * S, gamma = (n - 1) u / (1 - (n - 1) u), u = 2^-53.
"""
import math

import numpy as np

F = np.float32
CODEC_SIGN, FMT_SIGN = 6, 4
MAGIC, VERSION = 0x31534346, 1                       # "FCS1"
HDR_BYTES, WIRE_HDR_BYTES = 96, 128

HDR = np.dtype([("thresh", "<u8"), ("lower", "<u8"), ("n", "<u4"), ("k", "<u4"),
                ("n_entries", "<u4"), ("index_bits", "<u4"), ("codec", "<u4"), ("status", "<u4"),
                ("n_definite", "<u4"), ("n_cand", "<u4"), ("seed", "<u8"), ("offset", "<u8"),
                ("p", "<f8"), ("chunk", "<u4"), ("format", "<u4"), ("key_mode", "<u4"),
                ("reserved", "<u4", (3,))])
WIRE_HDR = np.dtype([("magic", "<u4"), ("version", "<u4"), ("total_bytes", "<u8"),
                     ("zero", "<u4", (4,)), ("pkt", HDR)])
assert HDR.itemsize == HDR_BYTES and WIRE_HDR.itemsize == WIRE_HDR_BYTES


def sign_words(n: int) -> int:
    """ceil(n / 32) rounded up to a multiple of 4."""
    return ((n + 31) // 32 + 3) // 4 * 4


def encoded(g, e=None):
    """a: g itself, or fl32(g + e), one IEEE add per element."""
    g = np.asarray(g, F)
    if e is None:
        return g.copy()
    with np.errstate(all="ignore"):
        return (g + np.asarray(e, F)).astype(F)


def true_sum(a) -> float:
    """S as the correctly rounded float64 of the exact sum (inf / NaN as IEEE addition gives)."""
    m = np.abs(np.asarray(a, F).astype(np.float64))
    if np.isnan(m).any():
        return math.nan
    if np.isinf(m).any():
        return math.inf
    return math.fsum(m.tolist())


def sum_bound(n: int, S: float) -> float:
    """|S^ - S| of any-order float64 summation of n non-negative terms with true sum S."""
    gam = (n - 1) * 2.0 ** -53
    return gam * S / (1.0 - gam)


def scale(a) -> np.float32:
    """s = fl32(S / n) from the true sum: THE scale when every partial sum is exact."""
    a = np.asarray(a, F)
    with np.errstate(all="ignore"):
        return F(np.float64(true_sum(a)) / np.float64(a.size))


def scale_range(a):
    """(lo, hi): every fl32(x / n) with |x - S| <= sum_bound lies in [lo, hi] (rounding is
    monotone), and a device scale must."""
    a = np.asarray(a, F)
    S = true_sum(a)
    b = sum_bound(a.size, S)
    n = np.float64(a.size)
    return F(np.float64(S - b) / n), F(np.float64(S + b) / n)


def bits(a) -> np.ndarray:
    """b[t]: the IEEE sign bit (-0.0 is negative, a NaN goes by its sign bit)."""
    return (np.asarray(a, F).view(np.uint32) >> np.uint32(31)).astype(bool)


def words_of(b) -> np.ndarray:
    """The uint32 words of n bits: bit t % 32 of word t // 32, tail bits and pad words zero."""
    b = np.asarray(b, bool)
    full = np.zeros(sign_words(b.size) * 32, dtype=bool)
    full[:b.size] = b
    return np.packbits(full, bitorder="little").view("<u4").copy()


def bits_of(words, n: int) -> np.ndarray:
    return np.unpackbits(np.asarray(words, "<u4").view(np.uint8), bitorder="little")[:n].astype(bool)


def decode(b, s) -> np.ndarray:
    """q[t] = b[t] ? -s : +s."""
    s = F(s)
    return np.where(np.asarray(b, bool), F(-s), s).astype(F)


def residual(a, q) -> np.ndarray:
    """e' = fl32(a - q), one IEEE subtract per element."""
    with np.errstate(all="ignore"):
        return (np.asarray(a, F) - np.asarray(q, F)).astype(F)


def encode(g, e=None, s=None):
    """(a, s, words, q, e') of one encode; ``s``: the scale to use instead of the true-sum one."""
    a = encoded(g, e)
    s = scale(a) if s is None else F(s)
    b = bits(a)
    q = decode(b, s)
    return a, s, words_of(b), q, residual(a, q)


def header(n: int, s) -> np.ndarray:
    h = np.zeros((), dtype=HDR)
    h["n"] = h["k"] = h["n_entries"] = n
    h["codec"], h["format"], h["p"] = CODEC_SIGN, FMT_SIGN, np.float64(F(s))
    return h


def fold(rows, weights, start=None) -> np.ndarray:
    """The dense FedAVG of the decoded rows: float32 np.sum(G * w[:, None], axis=0) (row order,
    from +0.0); ``start``: the partial sum the rows continue."""
    G = np.asarray(rows, F)
    w = np.asarray(weights, F)
    with np.errstate(all="ignore"):
        if start is None:
            return np.sum(G * w[:, None], axis=0)
        acc = np.asarray(start, F).copy()
        for r in G * w[:, None]:
            acc = (acc + r).astype(F)
        return acc


def vote(bit_rows, eta) -> np.ndarray:
    """-eta where 2 neg > m, +eta where 2 neg < m, +0.0 on a tie."""
    B = np.asarray(bit_rows, bool)
    m, neg = B.shape[0], B.sum(axis=0, dtype=np.int64)
    eta = F(eta)
    return np.where(2 * neg > m, F(-eta), np.where(2 * neg < m, eta, F(0.0))).astype(F)


def majority_eta(scales) -> np.float32:
    """The default eta: the median of the finite scales in float64, cast to float32."""
    s = np.asarray(scales, np.float64)
    s = s[np.isfinite(s)]
    if s.size == 0:
        raise ValueError("no finite scale")
    return F(np.median(s))


def wire_bytes(n: int) -> int:
    return WIRE_HDR_BYTES + 4 * sign_words(n)


def pack(n: int, s, words) -> bytes:
    """The wire form: the 128-byte header, then the words."""
    words = np.asarray(words, "<u4")
    assert words.size == sign_words(n)
    h = np.zeros((), dtype=WIRE_HDR)
    h["magic"], h["version"], h["total_bytes"] = MAGIC, VERSION, wire_bytes(n)
    h["pkt"] = header(n, s)
    return h.tobytes() + words.tobytes()


def parse(raw: bytes):
    h = np.frombuffer(raw[:WIRE_HDR_BYTES], dtype=WIRE_HDR)[0]
    return {"hdr": h, "words": np.frombuffer(raw[WIRE_HDR_BYTES:], dtype="<u4")}


#: byte offsets of the wire header's fields (for one-field mutations)
OFF = {"magic": 0, "version": 4, "total_bytes": 8, "zero": 16, "pkt": 32}
OFF.update({f"pkt.{name}": 32 + HDR.fields[name][1] for name in HDR.names})
