"""The coordinate-wise trimmed mean's definition (include/fedcodec.h, fc_packets_trim) as a plain
NumPy function — a helper of tests/test_trim_host.py and tests/test_trim_gpu.py, not a test.

Per coordinate: the M values in ``np.sort``'s order (-inf first, -0.0 and +0.0 equal, +inf after
every finite value, every NaN after +inf), the b smallest and the b largest dropped, the other
M - 2b added in ascending order from +0.0 with every add rounded to float32, the sum divided by
float32(M - 2b) in float32.  ``b = (M - 1) // 2`` is the median.
"""
import numpy as np


def trimmed_mean_model(G, b: int) -> np.ndarray:
    G = np.asarray(G)
    if G.ndim != 2 or G.dtype != np.float32:
        raise ValueError("G must be an (M, N) float32 matrix")
    M = G.shape[0]
    b = int(b)
    if b < 0 or 2 * b >= M:
        raise ValueError("0 <= b and 2 b < M")
    S = np.sort(G, axis=0)[b:M - b]
    acc = np.zeros(G.shape[1], dtype=np.float32)             # +0.0
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        for row in S:                                        # ascending, one float32 add per row
            acc = np.add(acc, row, dtype=np.float32)
        return np.divide(acc, np.float32(M - 2 * b), dtype=np.float32)


def median_trim(M: int) -> int:
    return (M - 1) // 2
