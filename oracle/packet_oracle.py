"""CPU restatement of the HIP codec's packet semantics — TEST INFRASTRUCTURE (oracle).

The reference has no wire format (``compression.py:33-37`` returns a dense vector), so the
packet is the build's own.  This module states its rules on the CPU so the GPU packet can
be checked field by field; the selection rule itself is pinned to the reference by
``compression_oracle.topk_indices`` (stable argsort, reversed) — see
``tests/test_oracle_golden.py::test_composite_rule_equals_stable_argsort``.

Composite key (fc_common.h):
  key(x)  = bits(x) & 0x7fffffff, with every NaN mapped to 0x7f800001 (above +inf)
  IB      = index bits = max(1, ceil(log2 N))
  comp(i) = key(g[i]) << IB | i          (unique per element)
  top-k   = the k largest comps  <=>  argsort(|g|, stable)[::-1][:k]
  T64     = the k-th largest comp; selected  <=>  comp >= T64
A packet lists, in ascending index order, every element whose comp >= L64 (a lower bound
found by the sampled bracket, L64 <= T64); the decoder keeps entries with comp >= T64.
"""
from __future__ import annotations

import numpy as np

NAN_KEY = np.uint32(0x7F800001)
NOTHING = np.uint64(1) << np.uint64(63)       # T64 that selects nothing (k == 0)


def index_bits(n: int) -> int:
    return max(1, int(n - 1).bit_length()) if n > 1 else 1


def mag_key(g: np.ndarray) -> np.ndarray:
    u = np.ascontiguousarray(g, dtype=np.float32).view(np.uint32) & np.uint32(0x7FFFFFFF)
    return np.where(u > np.uint32(0x7F800000), NAN_KEY, u).astype(np.uint32)


def comps(keys: np.ndarray) -> np.ndarray:
    n = keys.shape[0]
    ib = np.uint64(index_bits(n))
    return (keys.astype(np.uint64) << ib) | np.arange(n, dtype=np.uint64)


def threshold(keys: np.ndarray, k: int) -> np.uint64:
    """T64 for ``k`` kept coordinates (0 <= k <= N)."""
    n = keys.shape[0]
    if k <= 0:
        return NOTHING
    if k >= n:
        return np.uint64(0)
    c = comps(keys)
    return np.partition(c, n - k)[n - k]


def selected_indices(keys: np.ndarray, k: int) -> np.ndarray:
    """Ascending indices of the k largest comps."""
    t = threshold(keys, k)
    return np.nonzero(comps(keys) >= t)[0].astype(np.uint32)


def topk_packet(g: np.ndarray, k: int):
    """(idx ascending uint32, val float32 bit-copies) of the exact top-k packet."""
    idx = selected_indices(mag_key(g), k)
    return idx, np.ascontiguousarray(g, dtype=np.float32)[idx]


def decode_dense(n: int, idx: np.ndarray, val: np.ndarray) -> np.ndarray:
    out = np.zeros(n, dtype=np.float32)
    out[idx] = val
    return out


# --------------------------------------------------------------------------------------
# The wire format of include/fedcodec.h, stated once on the CPU: a packet BUILDER (every
# field a decoder reads, from a plain list of (index, value) pairs) and a packet CONSUMER
# (the rules of entry_kept / kept_f32 / dropped_f32 in csrc/fc_decode.hip and the row-order
# sum of gar.py:44).  The GPU decoders are fed hand-built packets and compared with the
# consumer; the builder is pinned to the GPU encoders field by field
# (tests/test_packet_consumers_gpu.py part A).
# --------------------------------------------------------------------------------------
CHUNK = 8192
QUARTER = CHUNK // 4
CHUNK_WORDS = CHUNK // 32
CODEC_TOP, CODEC_RAND, CODEC_DROPOUT_BIASED, CODEC_DROPOUT_UNBIASED = 1, 2, 3, 4
KEY_MAGNITUDE, KEY_PHILOX = 0, 1
FMT_IDXVAL, FMT_BITMAP = 0, 1
POISON_IDX = 0xFFFF                      # an unlisted slot: no chunk-local index is this large
POISON_VAL = np.float32(np.nan)          # ... and a folded one shows up in the output

#: fc_packet_hdr (96 bytes, little-endian, no padding)
HDR_DTYPE = np.dtype([("thresh", "<u8"), ("lower", "<u8"), ("n", "<u4"), ("k", "<u4"),
                      ("n_entries", "<u4"), ("index_bits", "<u4"), ("codec", "<u4"),
                      ("status", "<u4"), ("n_definite", "<u4"), ("n_cand", "<u4"),
                      ("seed", "<u8"), ("offset", "<u8"), ("p", "<f8"), ("chunk", "<u4"),
                      ("format", "<u4"), ("key_mode", "<u4"), ("reserved", "<u4", (3,))])
assert HDR_DTYPE.itemsize == 96


def num_chunks(n: int) -> int:
    return (int(n) + CHUNK - 1) // CHUNK


def capacity(n: int) -> int:
    return num_chunks(n) * CHUNK


def _header(n, *, thresh, lower, codec, key_mode, k, seed, offset, p, fmt, n_entries,
            n_definite, n_cand):
    h = np.zeros((), dtype=HDR_DTYPE)
    h["thresh"], h["lower"] = np.uint64(thresh), np.uint64(lower)
    h["n"], h["k"], h["n_entries"] = n, k, n_entries
    h["index_bits"] = index_bits(n)
    h["codec"], h["status"] = codec, 0
    h["n_definite"], h["n_cand"] = n_definite, n_cand
    h["seed"], h["offset"], h["p"] = np.uint64(seed), np.uint64(offset), float(p)
    h["chunk"], h["format"], h["key_mode"] = CHUNK, fmt, key_mode
    return h


def _is_mask_header(codec: int, key_mode: int) -> bool:
    """fc_mask_encode's packets (dropout, rand with a host mask): the static header only."""
    return codec in (CODEC_DROPOUT_BIASED, CODEC_DROPOUT_UNBIASED) or \
        (codec == CODEC_RAND and key_mode == KEY_MAGNITUDE)


def _check_entries(n, idx, val):
    idx = np.asarray(idx, dtype=np.int64).reshape(-1)
    val = np.ascontiguousarray(val, dtype=np.float32).reshape(-1)
    if idx.shape != val.shape:
        raise ValueError("one value per index")
    if idx.size and (idx[0] < 0 or idx[-1] >= n or np.any(np.diff(idx) <= 0)):
        raise ValueError("indices must be ascending, distinct and inside [0, n)")
    return idx, val


def _slots(n, idx):
    """(chunk, chunk-local index, slot position, per-chunk counts) of ascending entries."""
    nch = num_chunks(n)
    c = idx // CHUNK
    cnt = np.bincount(c, minlength=nch).astype(np.int64)
    first = np.cumsum(cnt) - cnt                      # entries before chunk c
    pos = c * CHUNK + (np.arange(idx.size, dtype=np.int64) - first[c])
    return c, idx % CHUNK, pos, cnt


def build_idxval(n, idx, val, *, thresh, lower=0, codec, key_mode=KEY_MAGNITUDE, k=0, seed=0,
                 offset=0, p=0.0, with_qoff=True, fill=(POISON_IDX, POISON_VAL),
                 n_entries=None, n_definite=0, n_cand=0) -> dict:
    """An FC_FMT_IDXVAL packet from ascending, distinct global indices and their values.

    Chunk c's entries sit at ``[c*8192, c*8192 + cnt[c])`` of ``idx`` (uint16, chunk-local) and
    ``val``; every other slot position holds ``fill`` (a poison pair by default);
    ``qoff[c]`` = start of quarter 1 | quarter 2 << 16 | quarter 3 << 32 | cnt << 48.
    Header: what the encoders write — ``n_entries`` is the number of listed entries for the
    top-k / native rand-k encoders and stays 0 in fc_mask_encode's static header;
    ``n_definite`` / ``n_cand`` are encoder diagnostics no decoder reads."""
    n = int(n)
    idx, val = _check_entries(n, idx, val)
    nch, cap = num_chunks(n), capacity(n)
    c, loc, pos, cnt = _slots(n, idx)
    out_idx = np.full(cap, fill[0], dtype=np.uint16)
    out_val = np.full(cap, fill[1], dtype=np.float32)
    out_idx[pos] = loc.astype(np.uint16)
    out_val[pos] = val
    qoff = None
    if with_qoff:
        per = np.bincount(c * 4 + loc // QUARTER, minlength=nch * 4).reshape(nch, 4)
        s1 = per[:, 0]
        s2 = s1 + per[:, 1]
        s3 = s2 + per[:, 2]
        qoff = (s1.astype(np.uint64) | (s2.astype(np.uint64) << np.uint64(16))
                | (s3.astype(np.uint64) << np.uint64(32)) | (cnt.astype(np.uint64) << np.uint64(48)))
    if n_entries is None:
        n_entries = 0 if _is_mask_header(codec, key_mode) else int(idx.size)
    hdr = _header(n, thresh=thresh, lower=lower, codec=codec, key_mode=key_mode, k=k, seed=seed,
                  offset=offset, p=p, fmt=FMT_IDXVAL, n_entries=n_entries,
                  n_definite=n_definite, n_cand=n_cand)
    return {"n": n, "fmt": FMT_IDXVAL, "idx": out_idx, "val": out_val,
            "cnt": cnt.astype(np.uint32), "qoff": qoff, "bitmap": None, "hdr": hdr}


def build_bitmap(n, idx, val, *, codec, p, seed=0, offset=0, fill=POISON_VAL) -> dict:
    """An FC_FMT_BITMAP packet (fc_mask_encode): chunk c's 256 bitmap words at
    ``[c*256, c*256 + 256)`` (bit i % 32 of word i // 32 = element i), its kept values in
    ascending order at ``[c*8192, c*8192 + cnt[c])`` of ``val``; the static mask header."""
    n = int(n)
    idx, val = _check_entries(n, idx, val)
    nch, cap = num_chunks(n), capacity(n)
    _, _, pos, cnt = _slots(n, idx)
    out_val = np.full(cap, fill, dtype=np.float32)
    out_val[pos] = val
    bits = np.zeros(nch * CHUNK, dtype=np.uint8)
    bits[idx] = 1
    bitmap = np.packbits(bits, bitorder="little").view("<u4").copy()
    hdr = _header(n, thresh=0, lower=0, codec=codec, key_mode=KEY_MAGNITUDE, k=0, seed=seed,
                  offset=offset, p=p, fmt=FMT_BITMAP, n_entries=0, n_definite=0, n_cand=0)
    return {"n": n, "fmt": FMT_BITMAP, "idx": None, "val": out_val,
            "cnt": cnt.astype(np.uint32), "qoff": None, "bitmap": bitmap, "hdr": hdr}


def philox_keys_at(idx: np.ndarray, seed: int, offset: int) -> np.ndarray:
    """Native rand-k keys (Philox word >> 1) of the given elements (oracle/philox.py map)."""
    from . import philox as ph
    i = np.asarray(idx, dtype=np.uint64)
    if i.size == 0:
        return np.zeros(0, dtype=np.uint32)
    b = ((i >> np.uint64(8)) << np.uint64(6)) | (i & np.uint64(63))
    w = ph._words(i, b, (i >> np.uint64(6)) & np.uint64(3), int(seed), int(offset))
    return (w >> np.uint32(1)).astype(np.uint32)


def listed_entries(fields: dict):
    """(global index int64 ascending, value float32) of every LISTED entry of a packet
    (work proportional to the entries, not to n)."""
    n, cnt = fields["n"], fields["cnt"].astype(np.int64)
    if cnt.shape != (num_chunks(n),) or np.any(cnt > CHUNK):
        raise ValueError("cnt must hold one count <= 8192 per chunk")
    first = np.cumsum(cnt) - cnt
    chunk = np.repeat(np.arange(cnt.size, dtype=np.int64), cnt)
    pos = chunk * CHUNK + (np.arange(int(cnt.sum()), dtype=np.int64) - first[chunk])
    val = fields["val"][pos]
    if fields["fmt"] == FMT_IDXVAL:
        gidx = chunk * CHUNK + fields["idx"][pos].astype(np.int64)
    else:
        bits = np.unpackbits(fields["bitmap"].view(np.uint8), bitorder="little")
        gidx = np.nonzero(bits[:n])[0].astype(np.int64)
        if not np.array_equal(np.bincount(gidx // CHUNK, minlength=cnt.size), cnt):
            raise ValueError("bitmap population and cnt disagree")
    return gidx, val


def kept_entries(fields: dict):
    """The listed entries a decoder keeps (fc_decode.hip entry_kept): all of them when
    ``thresh == 0`` (and always for the bitmap format), else those with
    ``key << index_bits | index >= thresh``, key = the magnitude key of the VALUE or the
    element's Philox word >> 1."""
    gidx, val = listed_entries(fields)
    h = fields["hdr"]
    thresh = np.uint64(h["thresh"])
    if fields["fmt"] == FMT_BITMAP or thresh == 0:
        return gidx, val
    if int(h["key_mode"]) == KEY_PHILOX:
        key = philox_keys_at(gidx, int(h["seed"]), int(h["offset"]))
    else:
        key = mag_key(val)
    comp = (key.astype(np.uint64) << np.uint64(int(h["index_bits"]))) | gidx.astype(np.uint64)
    keep = comp >= thresh
    return gidx[keep], val[keep]


def decode_sparse(fields: dict, dtype=np.float32):
    """(kept global indices, their decoded values, the value of every other coordinate): kept
    entries carry their value — for dropout-unbiased fl32(fl64(v) / p) (float32 result) or
    fl64(v) / p (float64) — and a dropped coordinate is +0, or NaN (0 / 0) for
    dropout-unbiased with p == 0."""
    dtype = np.dtype(dtype)
    h = fields["hdr"]
    unbiased = int(h["codec"]) == CODEC_DROPOUT_UNBIASED
    p = np.float64(h["p"])
    gidx, val = kept_entries(fields)
    x = val.astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        if unbiased:
            x = x / p
        x = x.astype(dtype)
    return gidx, x, dtype.type(np.nan if (unbiased and p == 0.0) else 0.0)


def decode_packet(fields: dict, dtype=np.float32) -> np.ndarray:
    """The dense vector fc_decode_dense writes (decode_sparse, spread out)."""
    gidx, x, dz = decode_sparse(fields, dtype)
    out = np.full(fields["n"], dz, dtype=np.dtype(dtype))
    out[gidx] = x
    return out


def fold_packets(packets, weights, acc=None) -> np.ndarray:
    """fc_decode_accumulate(_continue) on the CPU: every packet becomes its dense float32 row
    (decode_packet — a dropped coordinate therefore adds fl32(dz * w)) and the rows are summed
    by gar_oracle.sequential_weighted_sum, acc = fl32(acc + fl32(w * x)) in row order from +0.
    With ``acc`` the same two operations continue from it (``acc`` itself is taken as is: a
    -0.0 in it is not first added to +0)."""
    from .gar_oracle import sequential_weighted_sum
    rows = [decode_packet(f, np.float32) for f in packets]
    w = [np.float32(x) for x in weights]
    if len(rows) != len(w):
        raise ValueError("one weight per packet")
    with np.errstate(invalid="ignore", over="ignore", under="ignore"):
        if acc is None:
            return sequential_weighted_sum(rows, w)
        out = np.ascontiguousarray(acc, dtype=np.float32).copy()
        for wi, r in zip(w, rows):
            out = np.add(out, np.multiply(r, wi))
        return out


def same_bits(got: np.ndarray, want: np.ndarray) -> bool:
    """Byte equality (the sign of zero included) with every NaN equal to every NaN."""
    got, want = np.asarray(got), np.asarray(want)
    if got.dtype != want.dtype or got.shape != want.shape:
        return False
    gn, wn = np.isnan(got), np.isnan(want)
    if not np.array_equal(gn, wn):
        return False
    u = np.dtype(f"<u{got.dtype.itemsize}")
    return bool(np.array_equal(got.view(u)[~gn], want.view(u)[~wn]))
