"""The coordinate-wise trimmed mean of scaled-sign packets (include/fedcodec.h, fc_sign_trim) as
two independent NumPy statements — a helper of tests/test_sign_trim_host.py and
tests/test_sign_trim_gpu.py, not a test.

``expected`` is the definition: ``trim_model.trimmed_mean_model`` (``np.sort`` per column, the ends
dropped, an ascending float32 sum from +0.0, one division) on the rows ``sign_model.decode`` makes.

``walk`` restates what the kernel does instead of sorting: a column holds only ``-|s_i|`` and
``+|s_i|``, so its order is known from the order of the m scales: the negatives first by
descending ``|s_i|``, the positives after them by ascending ``|s_i|``, every NaN last.  The
clients are ranked once (NaN last, ties by client index); per coordinate the bits are walked in
rank order, twice, and a value is added when its position falls inside ``[b, m - b)``.
"""
import numpy as np

import sign_model as sm
from trim_model import trimmed_mean_model

F = np.float32


def decoded(bit_rows, scales) -> np.ndarray:
    """The float32 rows fc_sign_decode makes."""
    B = np.asarray(bit_rows, bool)
    return np.stack([sm.decode(b, s) for b, s in zip(B, np.asarray(scales, F))])


def expected(bit_rows, scales, b: int) -> np.ndarray:
    """The expected column: the sorted model on the decoded rows."""
    return trimmed_mean_model(decoded(bit_rows, scales), b)


def rank_order(scales):
    """(the client indices in rank order, the count of non-NaN scales): by ``|s|`` ascending, +inf
    the largest number, NaN last, ties by client index."""
    s = np.asarray(scales, F)
    nan = np.isnan(s)
    key = np.where(nan, np.uint32(0xFFFFFFFF), np.abs(s).view(np.uint32))
    order = sorted(range(len(s)), key=lambda i: (int(key[i]), i))
    return order, int((~nan).sum())


def walk(bit_rows, scales, b: int) -> np.ndarray:
    """The rank-order walk.  A non-NaN scale with its sign bit set is the client of ``|s|`` with
    every bit flipped (``b ? -s : +s`` as it stands)."""
    B = np.asarray(bit_rows, bool)
    s = np.asarray(scales, F)
    m, n = B.shape
    b = int(b)
    if b < 0 or 2 * b >= m:
        raise ValueError("0 <= b and 2 b < M")
    order, nn = rank_order(s)
    flip = np.signbit(s) & ~np.isnan(s)
    neg = B ^ flip[:, None]                                   # the coordinates that hold -|s_i|
    mag = np.where(np.isnan(s), s, np.abs(s)).astype(F)
    acc = np.zeros(n, dtype=F)                                # +0.0
    pos = np.zeros(n, dtype=np.int64)

    def step(take, v):
        nonlocal acc, pos
        inside = take & (pos >= b) & (pos < m - b)
        with np.errstate(invalid="ignore", over="ignore", under="ignore"):
            acc = np.add(acc, np.where(inside, F(v), F(0.0)), dtype=F)
        pos = pos + take

    for r in range(nn - 1, -1, -1):                           # the negatives, most negative first
        i = order[r]
        step(neg[i], -mag[i])
    for r in range(m):                                        # the positives ascending, then the NaNs
        i = order[r]
        step(~neg[i] if r < nn else np.ones(n, bool), mag[i])
    assert (pos == m).all()
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        return np.divide(acc, F(m - 2 * b), dtype=F)


def trims(m: int):
    """The b values the tests use for m clients: 0, 1, (m - 1) // 4 and the median's."""
    return sorted({b for b in (0, 1, (m - 1) // 4, (m - 1) // 2) if 2 * b < m})


#: the scale cases of the tests: name -> function of (m, rng, b) giving m float32 scales
def _distinct(m, rng, b):
    return (rng.uniform(1.0, 2.0, m) * 2.0 ** rng.integers(-20, 21, m)).astype(F)


def _with(values_at):
    def make(m, rng, b):
        s = _distinct(m, rng, b)
        for i, v in values_at(m, b):
            s[i % m] = v
        return s
    return make


SCALES = {
    "distinct": _distinct,
    "all_equal": lambda m, rng, b: np.full(m, 0.75, F),
    "tie_groups": lambda m, rng, b: F([0.5, 2.0, 1.25])[rng.integers(0, 3, m)],
    "one_zero": _with(lambda m, b: [(m // 2, 0.0)]),
    "all_zero": lambda m, rng, b: np.zeros(m, F),
    "subnormal": _with(lambda m, b: [(0, 1e-42), (m - 1, 3e-45)]),
    "mixed_magnitudes": lambda m, rng, b: F([1e8, 1.0, 1e-8])[rng.integers(0, 3, m)],
    "flt_max": lambda m, rng, b: np.full(m, np.finfo(F).max, F),
    "one_inf": _with(lambda m, b: [(1, np.inf)]),
    "nan_in_one": _with(lambda m, b: [(m // 3, np.nan)]),
    "nan_in_b": _with(lambda m, b: [(2 * i + 1, np.nan) for i in range(b)]),
    "nan_in_b_plus_1": _with(lambda m, b: [(2 * i, np.nan) for i in range(b + 1)]),
}


def edge_bits(m: int, n: int, rng) -> np.ndarray:
    """Bit rows whose column t holds exactly ``t % (m + 1)`` set bits, at random clients: with
    n > m every count of negatives (and so of positives) from 0 to m occurs, the window's edges
    b - 1, b and b + 1 of every b among them."""
    B = np.zeros((m, n), bool)
    for t in range(n):
        B[rng.permutation(m)[: t % (m + 1)], t] = True
    return B
