"""NumPy model of the wire format of include/fedcodec.h (csrc/fc_wire_host.h) — TEST INFRASTRUCTURE.

Built on ``oracle.packet_oracle.kept_entries``: the wire packet of a slotted packet holds the
entries the decoders keep, and nothing else of it but a canonical header.

    0     fc_wire_hdr, 128 bytes: magic "FCW1", version 1, total_bytes, n_entries (E), nch,
          status, fc_packet_hdr pkt
    128   uint64 qoff[nch]    quarter 1/2/3 starts | cnt << 48, over the kept entries
          uint32 start[nch]   exclusive prefix sum of the counts
          uint16 idx[E]       chunk-local, ascending inside each chunk
          float  val[E]       the stored values, bit for bit
Little-endian, every section 16-byte aligned, pad bytes zero.
"""
from __future__ import annotations

import numpy as np

from oracle import packet_oracle as po

MAGIC = b"FCW1"
VERSION = 1
HDR_BYTES = 128
WIRE_HDR_DTYPE = np.dtype([("magic", "S4"), ("version", "<u4"), ("total_bytes", "<u8"),
                           ("n_entries", "<u8"), ("nch", "<u4"), ("status", "<u4"),
                           ("pkt", po.HDR_DTYPE)])
assert WIRE_HDR_DTYPE.itemsize == HDR_BYTES


def pad16(x: int) -> int:
    return (int(x) + 15) & ~15


def layout(n: int, entries: int) -> dict:
    """Section offsets and the total size."""
    nch = po.num_chunks(n)
    off_qoff = HDR_BYTES
    off_start = off_qoff + pad16(8 * nch)
    off_idx = off_start + pad16(4 * nch)
    off_val = off_idx + pad16(2 * entries)
    return {"nch": nch, "qoff": off_qoff, "start": off_start, "idx": off_idx, "val": off_val,
            "total": off_val + pad16(4 * entries)}


def wire_bytes(n: int, entries: int) -> int:
    return layout(n, entries)["total"]


def canonical_header(h: np.ndarray, entries: int) -> np.ndarray:
    """pkt of the wire header from a slotted packet's header."""
    o = np.zeros((), dtype=po.HDR_DTYPE)
    for f in ("thresh", "n", "k", "index_bits", "codec", "seed", "offset", "p", "chunk", "format",
              "key_mode"):
        o[f] = h[f]
    o["lower"] = h["thresh"]
    o["n_entries"] = entries
    return o


def from_entries(n: int, gidx, val, hdr: np.ndarray) -> bytes:
    """The wire packet of ascending, distinct kept entries (global index, float32 value) under a
    slotted header ``hdr``."""
    gidx = np.asarray(gidx, dtype=np.int64)
    val = np.ascontiguousarray(val, dtype=np.float32)
    E = int(gidx.size)
    L = layout(n, E)
    nch = L["nch"]
    c, loc = gidx // po.CHUNK, gidx % po.CHUNK
    per = np.bincount(c * 4 + loc // po.QUARTER, minlength=nch * 4).reshape(nch, 4).astype(np.uint64)
    s1 = per[:, 0]
    s2 = s1 + per[:, 1]
    s3 = s2 + per[:, 2]
    cnt = s3 + per[:, 3]
    qoff = s1 | (s2 << np.uint64(16)) | (s3 << np.uint64(32)) | (cnt << np.uint64(48))
    start = (np.cumsum(cnt) - cnt).astype("<u4")
    out = np.zeros(L["total"], dtype=np.uint8)
    wh = np.zeros((), dtype=WIRE_HDR_DTYPE)
    wh["magic"], wh["version"], wh["total_bytes"] = MAGIC, VERSION, L["total"]
    wh["n_entries"], wh["nch"], wh["status"] = E, nch, 0
    wh["pkt"] = canonical_header(hdr, E)
    out[:HDR_BYTES] = np.frombuffer(wh.tobytes(), dtype=np.uint8)
    out[L["qoff"]: L["qoff"] + 8 * nch] = qoff.astype("<u8").view(np.uint8)
    out[L["start"]: L["start"] + 4 * nch] = start.view(np.uint8)
    out[L["idx"]: L["idx"] + 2 * E] = loc.astype("<u2").view(np.uint8)
    out[L["val"]: L["val"] + 4 * E] = val.view(np.uint8)
    return out.tobytes()


def pack(fields: dict) -> bytes:
    """The wire packet of a slotted idx/val packet (``packet_oracle.build_idxval`` fields)."""
    if fields["fmt"] != po.FMT_IDXVAL:
        raise ValueError("only idx/val packets have a wire form")
    gidx, val = po.kept_entries(fields)
    return from_entries(fields["n"], gidx, val, fields["hdr"])


def parse(raw) -> dict:
    """A wire packet's sections as arrays (no validation: for tests that look inside)."""
    a = np.frombuffer(bytes(raw), dtype=np.uint8)
    wh = np.frombuffer(a[:HDR_BYTES].tobytes(), dtype=WIRE_HDR_DTYPE)[0]
    n, E = int(wh["pkt"]["n"]), int(wh["n_entries"])
    L = layout(n, E)
    nch = L["nch"]
    return {"hdr": wh, "layout": L,
            "qoff": a[L["qoff"]: L["qoff"] + 8 * nch].view("<u8"),
            "start": a[L["start"]: L["start"] + 4 * nch].view("<u4"),
            "idx": a[L["idx"]: L["idx"] + 2 * E].view("<u2"),
            "val": a[L["val"]: L["val"] + 4 * E].view("<f4")}


def unpack(raw) -> dict:
    """The slotted packet fc_wire_unpack_batch makes of a well-formed wire packet: the kept
    entries in their slots (poison elsewhere), counts, quarter offsets and the canonical header."""
    w = parse(raw)
    n = int(w["hdr"]["pkt"]["n"])
    cnt = (w["qoff"] >> np.uint64(48)).astype(np.int64)
    chunk = np.repeat(np.arange(cnt.size, dtype=np.int64), cnt)
    gidx = chunk * po.CHUNK + w["idx"].astype(np.int64)
    h = w["hdr"]["pkt"]
    f = po.build_idxval(n, gidx, w["val"], thresh=int(h["thresh"]), lower=int(h["lower"]),
                        codec=int(h["codec"]), key_mode=int(h["key_mode"]), k=int(h["k"]),
                        seed=int(h["seed"]), offset=int(h["offset"]), p=float(h["p"]),
                        n_entries=int(h["n_entries"]))
    assert np.array_equal(f["qoff"], w["qoff"])
    return f
