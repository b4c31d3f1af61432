"""NumPy model of the device ``np.random.permutation(n)[:k]`` (openmsftl_amd/csrc/fc_perm.hip).

Stage 1 (the MT19937 outputs) comes from ``oracle.mt19937.outputs``; this module restates what
the kernels do with them, stage by stage, so that the algorithm is pinned against NumPy without
a GPU (tests/test_perm_host.py):

* :func:`parse`: NumPy's shuffle runs ``for i = n-1 .. 1: j = random_interval(i); swap x[i],
  x[j]`` and ``random_interval(i)`` draws outputs w until ``(w & mask(i)) <= i`` (mask(i) the
  smallest 2**b - 1 >= i).  Word q is therefore tested against i = n-1-A(q), A(q) the number of
  accepted words before q.  The words are walked 128 at a time (two per lane): every word is
  tested against the group's first i; its true step is i - p0, p0 <= 127 the number of accepted
  words before it in the group, so the group is exact as it stands when no accepted word has
  (w & mask) > i - 127 and the mask is the same for every step of the group (induction over the
  words); any other group is resolved word by word.  J[i] = w & mask(i) of step i's accepted
  word (the kernel keeps J in draw order, J[n-1-i]).
* :func:`first_k`: x[p] after the shuffle by a walk backwards in time (from step 1 to step
  n-1): at position c and time t the next step above t that touched c is step c itself when
  c > t (the content came from j_c) or the smallest step i > t with j_i == c (it came from
  position i); when there is none the content is the initial x0[c] = c.
* :func:`state_after`: after ``consumed`` outputs from raw offset pos the key is block
  b = (pos + consumed - 1) // 624 of the raw sequence and pos' = pos + consumed - 624 b: the
  block's words are the untempered outputs 624 b - pos .. + 624.
"""
import numpy as np

from oracle import mt19937 as mt

GROUP = 128


def budget(n: int) -> int:
    return 2 * n + 4096


def mask_of(i: int) -> int:
    return (1 << int(i).bit_length()) - 1


def parse(words: np.ndarray, n: int, limit: int = None):
    """(J uint32[n], consumed, slow groups) or (None, None, slow) when ``limit`` words do not
    suffice (the device call's fallback 1)."""
    limit = len(words) if limit is None else limit
    J = np.zeros(n, dtype=np.uint32)
    lanes = np.arange(GROUP)
    i, slow = n - 1, 0
    for qg in range(0, limit, GROUP):
        M = mask_of(i)
        m = (words[qg:qg + GROUP] & np.uint32(M)).astype(np.int64)
        if len(m) == GROUP and qg + GROUP <= limit:
            a0 = m <= i
            p0 = np.cumsum(a0) - a0                       # accepting lanes below
            cnt = int(a0.sum())
            if not np.any(a0 & (m + (GROUP - 1) > i)) and i >= cnt + (M >> 1) + 1:
                J[i - p0[a0]] = m[a0]
                i -= cnt
                continue
        slow += 1
        for l in lanes[:min(GROUP, limit - qg)]:
            ml = int(words[qg + l]) & mask_of(i)
            if ml <= i:
                J[i] = ml
                i -= 1
                if i == 0:
                    return J, qg + int(l) + 1, slow
    return None, None, slow


def first_k(J: np.ndarray, n: int, k: int) -> np.ndarray:
    steps = np.arange(1, n, dtype=np.int64)
    steps = steps[J[1:].astype(np.int64) != steps]        # a self-swap moves nothing
    keys = np.sort(J[steps].astype(np.int64) * n + steps)  # (position, step), ascending
    c = np.arange(k, dtype=np.int64)
    t = np.zeros(k, dtype=np.int64)
    own = c > 0
    t[own] = c[own]
    c[own] = J[c[own]]
    live = np.ones(k, dtype=bool)
    rounds = 0
    while live.any():
        at = np.searchsorted(keys, c[live] * n + t[live], side="right")
        nxt = np.where(at < len(keys), keys[np.minimum(at, len(keys) - 1)], -1) if len(keys) \
            else np.full(at.shape, -1)
        hit = (nxt >= 0) & (nxt // n == c[live])
        ix = np.nonzero(live)[0]
        c[ix[hit]] = t[ix[hit]] = nxt[hit] % n
        live[ix[~hit]] = False
        rounds += 1
    first_k.rounds = rounds
    return c.astype(np.uint32)


def untemper(y: np.ndarray) -> np.ndarray:
    y = np.asarray(y, dtype=np.uint32).copy()
    y ^= y >> np.uint32(18)
    y ^= (y << np.uint32(15)) & np.uint32(0xEFC60000)
    t = y.copy()
    for _ in range(5):
        t = y ^ ((t << np.uint32(7)) & np.uint32(0x9D2C5680))
    y = t
    for _ in range(3):
        t = y ^ (t >> np.uint32(11))
    return t


def state_after(key, pos: int, words: np.ndarray, consumed: int):
    end = pos + consumed
    b = (end - 1) // mt.NW
    if b == 0:
        return np.asarray(key, np.uint32).copy(), end
    q0 = b * mt.NW - pos
    return untemper(words[q0:q0 + mt.NW]), end - b * mt.NW


def permutation(key, pos: int, n: int, k: int, max_words: int = 0):
    """``np.random.permutation(n)[:k]`` from the state (key, pos) -> (idx uint32[k] or None on
    fallback, (key, pos) after, consumed)."""
    if n <= 1:
        return np.arange(k, dtype=np.uint32), (np.asarray(key, np.uint32).copy(), pos), 0
    limit = budget(n) if max_words == 0 or max_words > budget(n) else max_words
    words = mt.outputs(key, pos, limit + mt.NW)
    J, consumed, _ = parse(words, n, limit)
    if J is None:
        return None, (np.asarray(key, np.uint32).copy(), pos), 0
    return first_k(J, n, k), state_after(key, pos, words, consumed), consumed
