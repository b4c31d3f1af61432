"""NumPy / exact-rational restatement of the geometry of scaled-sign packets (include/fedcodec.h,
"The clients' geometry from scaled-sign packets"), on top of tests/sign_model.py.  A test model:
the product does not import it.

With d_i[t] = b_i[t] ? -s_i : +s_i:
  <d_i, d_j> = s_i s_j (n - 2 H_ij),   H_ij = #{t : b_i[t] != b_j[t]}
  <d_i, v>   = s_i D_i,                D_i  = sum_t (b_i[t] ? -v[t] : +v[t])
"""
import math
from fractions import Fraction

import numpy as np

import sign_model as sm

F = np.float32


def pm_matrix(bit_rows) -> np.ndarray:
    """The +-1 float64 matrix of the bit rows (+1 for a clear bit)."""
    return 1.0 - 2.0 * np.asarray(bit_rows, bool).astype(np.float64)


def agreement(bit_rows) -> np.ndarray:
    """n - 2 H as exact int64: the product of the +-1 matrix with its transpose, taken in column
    blocks of 2^16 in float32 (every partial sum is an integer of magnitude <= 2^16: exact) and
    added in int64."""
    B = np.asarray(bit_rows, bool)
    A = np.zeros((B.shape[0], B.shape[0]), np.int64)
    for c in range(0, B.shape[1], 1 << 16):
        P = F(1.0) - F(2.0) * B[:, c:c + (1 << 16)].astype(F)
        A += np.rint(P @ P.T).astype(np.int64)
    return A


def hamming(bit_rows) -> np.ndarray:
    """H_ij, exact integers."""
    B = np.asarray(bit_rows, bool)
    return (B.shape[1] - agreement(B)) // 2


def gram(bit_rows, scales) -> np.ndarray:
    """gram[i][j] = the correctly rounded float64 of s_i s_j (n - 2 H_ij) in exact arithmetic (what
    a single IEEE multiply of the exact s_i s_j by the exact integer gives); NaN rows and columns
    for non-finite scales."""
    s = np.asarray(scales, F)
    A = agreement(bit_rows)
    m = s.size
    out = np.full((m, m), np.nan)
    fr = [Fraction(float(x)) if np.isfinite(x) else None for x in s]
    for i in range(m):
        for j in range(m):
            if fr[i] is not None and fr[j] is not None:
                out[i, j] = float(fr[i] * fr[j] * int(A[i, j]))
    return out


def dot(bit_rows, scales, v=None):
    """(D, bound): the exact D_i (math.fsum, the correctly rounded float64 of the true sum) and the
    bound on |D^_i - D_i| of any order of float64 summation, sign_model.sum_bound(n, sum |v|).
    ``v=None``: the all-ones vector (D_i = n - 2 popcount_i, bound 0)."""
    B = np.asarray(bit_rows, bool)
    n = B.shape[1]
    if v is None:
        return (n - 2 * B.sum(axis=1, dtype=np.int64)).astype(np.float64), 0.0
    v64 = np.asarray(v, F).astype(np.float64)
    D = np.array([math.fsum(np.where(b, -v64, v64).tolist()) for b in B])
    return D, sm.sum_bound(n, math.fsum(np.abs(v64).tolist()))


def dot_out(bit_rows, scales, v=None) -> np.ndarray:
    """[fl64(s_i) * D_i ..., sum v^2] with D_i exact: the expected output where every partial sum
    of the device is exact (integer-valued v, v=None); NaN for a non-finite scale."""
    s = np.asarray(scales, F).astype(np.float64)
    D, _ = dot(bit_rows, scales, v)
    with np.errstate(all="ignore"):
        out = np.where(np.isfinite(s), s * D, np.nan)
    n = np.asarray(bit_rows).shape[1]
    q = float(n) if v is None else math.fsum((np.asarray(v, F).astype(np.float64) ** 2).tolist())
    return np.concatenate([out, [q]])


def decoded(bit_rows, scales) -> np.ndarray:
    """The float32 rows fc_sign_decode makes."""
    return np.stack([sm.decode(b, s) for b, s in zip(np.asarray(bit_rows, bool), np.asarray(scales, F))])


def packets(bit_rows, scales):
    """The wire bytes of each client (sign_model.pack)."""
    B = np.asarray(bit_rows, bool)
    return [sm.pack(B.shape[1], s, sm.words_of(b)) for b, s in zip(B, np.asarray(scales, F))]
