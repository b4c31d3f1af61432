"""Device-resident codec API over libfedcodec.so (torch tensors in HBM, torch's stream).

    pkt = encode_top(g, k)                 # compression.py:31-37   (one read of g)
    pkt, e2 = encode_top_ef(g, e, k)       # top-k of g + e, e2 = what it dropped (error feedback)
    pkt = encode_rand_philox(g, k, seed)   # compression.py:39-45   native RNG
    pkt = encode_mask(g, codec, p, ...)    # compression.py:47-60 / rand parity
    q   = decode(pkt)                      # the dense vector compress() returns
    agg = decode_accumulate(pkts, w)       # aggregation.py:61-63 + gar.py:44, bit-exact fp32
    gm  = gram(pkts)                       # G @ G.T in float64 straight from the packets
    b   = dot_dense(pkts, v)               # [G @ v, v @ v] in float64 (v=None: row sums, n)
    tm  = trimmed_mean(pkts, b)            # coordinate-wise trimmed mean / median, bit-exact fp32
    w   = pack(pkt); raw = w.tobytes()     # the compact wire form: the kept entries alone
    pkt = unpack(wire_from_host(raw))      # validated host bytes back into a slotted packet
    agg = fold_wire(wires, w)              # decode_accumulate(unpack(wires), w) without the unpack
    pkt, e2 = encode_sign(g, e)            # 1 bit per coordinate and one scale, e2 = a - q
    pkts, _ = encode_sign_batch(grads)     # M clients in one launch, one read of each gradient
    agg = fold_sign(pkts, w)               # FedAVG of sign packets, the dense fold's bits
    v   = vote_sign(pkts, eta)             # majority vote: -eta / +eta / +0.0 per coordinate

Packets live on the GPU in the slotted layout of include/fedcodec.h: chunk c (8192 elements)
lists its entries, ascending, at ``[c*8192, c*8192 + cnt[c])`` of ``idx``/``val`` (or
``bitmap``/``val``); ``idx`` holds the chunk-local index as uint16 (element c*8192 + idx).
Plus per-chunk counts and quarter offsets and a 96-byte device header (``fc_packet_hdr``).
"""
from __future__ import annotations

import bisect
import ctypes
import threading
import warnings
import weakref
from dataclasses import dataclass
from typing import Callable, Optional, Sequence

import numpy as np
import torch

from . import _lib as L

_U32 = torch.int32  # uint32 payloads are stored in int32 tensors (bit-identical)
_U16 = torch.int16  # uint16 chunk-local indices in int16 tensors (bit-identical)


def _vp(t: Optional[torch.Tensor]):
    return ctypes.c_void_p(t.data_ptr()) if t is not None else ctypes.c_void_p(0)


def _stream(device=None):
    return ctypes.c_void_p(torch.cuda.current_stream(device).cuda_stream)


def _require_cuda_f32(g: torch.Tensor, name="g", align: int = 16, dtype=torch.float32):
    if not isinstance(g, torch.Tensor) or not g.is_cuda:
        raise TypeError(f"{name} must be a CUDA (HIP) tensor")
    if g.dtype != dtype:
        raise TypeError(f"{name} must be {dtype} (got {g.dtype})")
    if g.dim() != 1 or not g.is_contiguous():
        raise ValueError(f"{name} must be a contiguous 1-D tensor")
    if g.data_ptr() % align:
        raise ValueError(f"{name} must be {align}-byte aligned")


# ---------------------------------------------------------------------------------------
class Workspace:
    """Per-(device, stream) encoder scratch (self-cleaning after one memset)."""

    _cache: dict = {}

    def __init__(self, n: int, device: torch.device):
        lib = L.load()
        self.n = n
        self.nbytes = int(lib.fc_workspace_bytes(n))
        self.buf = torch.empty(self.nbytes, dtype=torch.uint8, device=device)
        L.check(lib.fc_workspace_init(_vp(self.buf), self.nbytes, _stream(device)),
                "fc_workspace_init")

    @classmethod
    def get(cls, n: int, device: torch.device) -> "Workspace":
        key = (device.index if device.index is not None else torch.cuda.current_device(),
               torch.cuda.current_stream(device).cuda_stream)
        ws = cls._cache.get(key)
        if ws is None or ws.n < n:
            ws = cls(n, device)
            cls._cache[key] = ws
        return ws


@dataclass
class Packet:
    """A compressed gradient resident in HBM (see include/fedcodec.h)."""
    n: int
    fmt: int
    val: torch.Tensor
    cnt: torch.Tensor                      # int32[num_chunks]: entries per chunk slot
    hdr: torch.Tensor                      # uint8[96] (may be a row of a batch tensor)
    idx: Optional[torch.Tensor] = None
    bitmap: Optional[torch.Tensor] = None
    k: int = 0
    qoff: Optional[torch.Tensor] = None    # int64[num_chunks]: quarter offsets (FC_FMT_IDXVAL)
    retried: bool = False                  # encode_top_ef: the exact chain wrote this packet

    @classmethod
    def alloc(cls, n: int, fmt: int, device, hdr: Optional[torch.Tensor] = None,
              k: int = 0) -> "Packet":
        lib = L.load()
        nch = int(lib.fc_num_chunks(n))
        cap = int(lib.fc_packet_capacity(n))
        return cls(n=n, fmt=fmt, k=k,
                   val=torch.empty(cap, dtype=torch.float32, device=device),
                   cnt=torch.empty(nch, dtype=_U32, device=device),
                   hdr=hdr if hdr is not None else torch.empty(L.HDR_BYTES, dtype=torch.uint8,
                                                               device=device),
                   idx=torch.empty(cap, dtype=_U16, device=device) if fmt == L.FC_FMT_IDXVAL else None,
                   bitmap=torch.empty(nch * 256, dtype=_U32, device=device)
                   if fmt == L.FC_FMT_BITMAP else None,
                   qoff=torch.empty(nch, dtype=torch.int64, device=device)
                   if fmt == L.FC_FMT_IDXVAL else None)

    @classmethod
    def alloc_batch(cls, n: int, m: int, fmt: int, device, k: int = 0) -> list:
        """``m`` packets of length n whose fields are the rows of per-field slabs (one (m, cap)
        value tensor, one index tensor, ...): the layout a batch of G's rows would have.  The
        128-client 16 M batched compaction writes them 2-3 % faster than m separate allocations
        (profiles/r05_stagger_probe.jsonl); the packets are ordinary Packet objects."""
        lib = L.load()
        nch = int(lib.fc_num_chunks(n))
        cap = int(lib.fc_packet_capacity(n))
        val = torch.empty((m, cap), dtype=torch.float32, device=device)
        idx = torch.empty((m, cap), dtype=_U16, device=device) if fmt == L.FC_FMT_IDXVAL else None
        bitmap = torch.empty((m, nch * 256), dtype=_U32, device=device) if fmt == L.FC_FMT_BITMAP else None
        cnt = torch.empty((m, nch), dtype=_U32, device=device)
        qoff = torch.empty((m, nch), dtype=torch.int64, device=device) if fmt == L.FC_FMT_IDXVAL else None
        hdr = torch.empty((m, L.HDR_BYTES), dtype=torch.uint8, device=device)
        return [cls(n=n, fmt=fmt, k=k, val=val[i], cnt=cnt[i], hdr=hdr[i],
                    idx=idx[i] if idx is not None else None,
                    bitmap=bitmap[i] if bitmap is not None else None,
                    qoff=qoff[i] if qoff is not None else None) for i in range(m)]

    @property
    def capacity(self) -> int:
        return self.val.numel()

    def release(self) -> None:
        """Drop the reference to the source gradient kept for the exact re-encode (call once
        :func:`resolve` has seen the packet OK), so the gradient's memory can be reused."""
        self._enc = None

    def _decodable(self) -> None:
        if getattr(self, "_dense_only", False):
            raise ValueError("this packet was scratch of compress_top_dense (header format "
                             "FC_FMT_DENSE): it lists no entries; decode the dense q instead")

    def view(self, weight: float = 1.0) -> L.PacketView:
        self._decodable()
        return L.PacketView(idx=self.idx.data_ptr() if self.idx is not None else 0,
                            val=self.val.data_ptr(),
                            bitmap=self.bitmap.data_ptr() if self.bitmap is not None else 0,
                            cnt=self.cnt.data_ptr(), hdr=self.hdr.data_ptr(),
                            qoff=self.qoff.data_ptr() if self.qoff is not None else 0,
                            weight=float(np.float32(weight)), reserved=0)

    def header(self) -> L.PacketHdr:
        """Synchronous D2H read of the device header."""
        raw = self.hdr.cpu().numpy().tobytes()
        return L.PacketHdr.from_buffer_copy(raw)

    def raw_entries(self):
        """(idx uint32 = global element index, val float32, header) of every LISTED entry,
        ascending — includes the sampled-bracket slack (comp < thresh); inspection / test
        helper (synchronises)."""
        self._decodable()
        h = self.header()
        cnt = self.cnt.cpu().numpy().astype(np.int64)
        pos = np.arange(self.capacity, dtype=np.int64)
        listed = (pos % L.FC_CHUNK) < cnt[pos // L.FC_CHUNK]
        val = self.val.cpu().numpy()[listed]
        if self.fmt == L.FC_FMT_IDXVAL:
            local = self.idx.cpu().numpy().view(np.uint16)[listed].astype(np.uint32)
            idx = (pos[listed] // L.FC_CHUNK * L.FC_CHUNK).astype(np.uint32) + local
        else:
            bits = np.unpackbits(self.bitmap.cpu().numpy().view(np.uint8), bitorder="little")
            idx = np.nonzero(bits[: self.n])[0].astype(np.uint32)
        return idx, val, h


def headers(packets: Sequence[Packet]) -> list:
    """Read many device headers with ONE synchronising copy (stacked on the device first)."""
    if not packets:
        return []
    raw = torch.stack([p.hdr for p in packets]).cpu().numpy()
    return [L.PacketHdr.from_buffer_copy(raw[i].tobytes()) for i in range(len(packets))]


# ---------------------------------------------------------------------------------------
def encode_top(g: torch.Tensor, k: int, *, key_mode: int = L.FC_KEY_MAGNITUDE, seed: int = 0,
               offset: int = 0, packet: Optional[Packet] = None,
               check: bool = True, exact: bool = False) -> Packet:
    """Top-k (|g|) or native rand-k (Philox keys) into an idx/val packet.

    ``check=True`` synchronises, reads the header and falls back to the exact device path
    if the sampled bracket missed (FC_STATUS_RETRY_EXACT).  With ``check=False`` call
    :func:`resolve` on the batch later (one sync per batch)."""
    _require_cuda_f32(g)
    lib = L.load()
    n = g.numel()
    if not 0 <= k <= n:
        raise ValueError(f"k={k} outside [0, {n}]")
    ws = Workspace.get(n, g.device)
    if packet is None:
        packet = Packet.alloc(n, L.FC_FMT_IDXVAL, g.device, k=k)
    packet.k = k
    fn = lib.fc_topk_encode_exact if exact else lib.fc_topk_encode
    L.check(fn(_vp(g), n, k, key_mode, seed, offset, _vp(packet.idx), _vp(packet.val),
               packet.capacity, _vp(packet.cnt), _vp(packet.qoff), _vp(packet.hdr), _vp(ws.buf),
               ws.nbytes, _stream(g.device)), "fc_topk_encode")
    packet._enc = (g, k, key_mode, seed, offset)
    packet._dense_only = False
    if check:
        resolve([packet])
    return packet


def _ef_exact(g: torch.Tensor, residual: torch.Tensor, residual_out: torch.Tensor, k: int,
              packet: Packet) -> None:
    """The exact error-feedback chain (include/fedcodec.h): fc_ef_sum, the exact encode of the
    sum held in ``residual_out``, fc_ef_clear.  Also the form for k = 0 and k = n."""
    lib = L.load()
    n = g.numel()
    s = _stream(g.device)
    ws = Workspace.get(n, g.device)
    L.check(lib.fc_ef_sum(_vp(g), _vp(residual), _vp(residual_out), n, s), "fc_ef_sum")
    L.check(lib.fc_topk_encode_exact(_vp(residual_out), n, k, L.FC_KEY_MAGNITUDE, 0, 0,
                                     _vp(packet.idx), _vp(packet.val), packet.capacity,
                                     _vp(packet.cnt), _vp(packet.qoff), _vp(packet.hdr),
                                     _vp(ws.buf), ws.nbytes, s), "fc_topk_encode_exact")
    v = packet.view()
    L.check(lib.fc_ef_clear(ctypes.byref(v), n, _vp(residual_out), s), "fc_ef_clear")


def encode_top_ef(g: torch.Tensor, residual: Optional[torch.Tensor], k: int, *,
                  residual_out: Optional[torch.Tensor] = None, packet: Optional[Packet] = None,
                  check: bool = True, exact: bool = False):
    """Top-k with error feedback (fc_topk_encode_ef): ``a = fl32(g + residual)`` is encoded
    (the packet is exactly ``encode_top(a, k)``'s) and ``residual_out`` becomes ``+0`` at the
    k selected coordinates and ``a`` everywhere else, in one pass over g and the residual.
    Returns ``(packet, residual_out)``.

    ``residual=None`` means zeros.  Neither ``g`` nor ``residual`` is written; ``residual_out``
    (allocated when None) must not share memory with them.  ``check=True`` reads the status
    and, if the sampled bracket missed, runs the exact chain itself (``packet.retried`` tells);
    with ``check=False`` call :func:`resolve` later, until then ``residual_out`` is only valid
    if the header says OK.  ``exact=True``, k = 0 and k = n always take the exact chain."""
    _require_cuda_f32(g)
    n = g.numel()
    if not 0 <= k <= n:
        raise ValueError(f"k={k} outside [0, {n}]")
    if n == 0:
        raise ValueError("empty gradient")
    if residual is None:
        residual = torch.zeros(n, dtype=torch.float32, device=g.device)
    if residual_out is None:
        residual_out = torch.empty(n, dtype=torch.float32, device=g.device)
    for t, name in ((residual, "residual"), (residual_out, "residual_out")):
        _require_cuda_f32(t, name)
        if t.numel() != n or t.device != g.device:
            raise ValueError(f"{name} must have n elements on g's device")
    if packet is None:
        packet = Packet.alloc(n, L.FC_FMT_IDXVAL, g.device, k=k)
    packet.k = k
    packet._enc = ("ef", g, residual, residual_out, k)
    packet._dense_only = False
    packet.retried = False
    if exact or k == 0 or k == n:
        _ef_exact(g, residual, residual_out, k, packet)
        packet.retried = bool(exact)
    else:
        lib = L.load()
        ws = Workspace.get(n, g.device)
        L.check(lib.fc_topk_encode_ef(_vp(g), _vp(residual), _vp(residual_out), n, k,
                                      _vp(packet.idx), _vp(packet.val), packet.capacity,
                                      _vp(packet.cnt), _vp(packet.qoff), _vp(packet.hdr),
                                      _vp(ws.buf), ws.nbytes, _stream(g.device)),
                "fc_topk_encode_ef")
    if check:
        resolve([packet])
    return packet, residual_out


def encode_decode_top(g: torch.Tensor, k: int, *, packet: Optional[Packet] = None,
                      out: Optional[torch.Tensor] = None, check: bool = True):
    """compression.py:31-37 as a packet AND its dense decode (fc_topk_encode_decode): the
    packet fc_topk_encode writes (entries, counts, quarter offsets, header with T64), and
    ``out`` = decode(packet), with the resolve's gather and finish done by the decode launch
    itself (k_fused_mag -> k_beta -> k_decode_res; no gather launch in between).  Returns
    (packet, out).  ``check=False`` skips the status read (call :func:`resolve` and, if it
    re-encoded, :func:`decode` yourself)."""
    _require_cuda_f32(g)
    n = g.numel()
    if not 0 <= k <= n:
        raise ValueError(f"k={k} outside [0, {n}]")
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=g.device)
    _require_cuda_f32(out, "out")
    if out.numel() != n:
        raise ValueError("out must have n elements")
    if packet is None:
        packet = Packet.alloc(n, L.FC_FMT_IDXVAL, g.device, k=k)
    if k == 0 or k >= n:                       # trivial thresholds: the exact engine's packet
        encode_top(g, k, packet=packet, check=check)
        return packet, decode(packet, out=out)
    lib = L.load()
    ws = Workspace.get(n, g.device)
    packet.k = k
    L.check(lib.fc_topk_encode_decode(_vp(g), n, k, _vp(packet.idx), _vp(packet.val),
                                      packet.capacity, _vp(packet.cnt), _vp(packet.qoff),
                                      _vp(packet.hdr), _vp(ws.buf), ws.nbytes, _vp(out),
                                      _stream(g.device)), "fc_topk_encode_decode")
    packet._enc = (g, k, L.FC_KEY_MAGNITUDE, 0, 0)
    packet._dense_only = False
    if check and resolve([packet]):            # bracket missed: exact packet, then decode
        decode(packet, out=out)
    return packet, out


def compress_top_dense(g: torch.Tensor, k: int, out: Optional[torch.Tensor] = None,
                       packet: Optional[Packet] = None, check: bool = True) -> torch.Tensor:
    """compression.py:31-37 on the device, straight to the dense q (fc_topk_encode_dense):
    one pass streams q (the packet buffers are scratch: no entries are written, the header
    says FC_FMT_DENSE), the resolve zeroes the slack.  Same bytes as
    ``decode(encode_top(g, k))``.  ``check=False`` skips the status read (call :func:`resolve`
    — it re-encodes a full packet — + :func:`decode` yourself if the header reports a retry)."""
    _require_cuda_f32(g)
    n = g.numel()
    if not 0 <= k <= n:
        raise ValueError(f"k={k} outside [0, {n}]")
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=g.device)
    _require_cuda_f32(out, "out")
    if out.numel() != n:
        raise ValueError("out must have n elements")
    if packet is None:
        packet = Packet.alloc(n, L.FC_FMT_IDXVAL, g.device, k=k)
    if k == 0 or k >= n:                       # trivial thresholds: packet path
        return decode(encode_top(g, k, packet=packet), out=out)
    lib = L.load()
    ws = Workspace.get(n, g.device)
    packet.k = k
    L.check(lib.fc_topk_encode_dense(_vp(g), n, k, _vp(packet.idx), _vp(packet.val),
                                     packet.capacity, _vp(packet.cnt), _vp(packet.qoff),
                                     _vp(packet.hdr), _vp(ws.buf), ws.nbytes, _vp(out),
                                     _stream(g.device)), "fc_topk_encode_dense")
    packet._enc = (g, k, L.FC_KEY_MAGNITUDE, 0, 0)
    packet._dense_only = True
    if check and resolve([packet]):            # bracket missed: exact packet, then decode
        decode(packet, out=out)
    return out


class BatchWorkspace:
    """Scratch for fc_topk_encode_batch: one encoder state per client (zeroed once)."""

    _cache: dict = {}

    def __init__(self, n: int, m: int, device: torch.device):
        lib = L.load()
        self.n, self.m = n, m
        self.nbytes = int(lib.fc_workspace_bytes_batch(n, m))
        self.buf = torch.empty(self.nbytes, dtype=torch.uint8, device=device)
        L.check(lib.fc_workspace_init(_vp(self.buf), self.nbytes, _stream(device)),
                "fc_workspace_init")

    @classmethod
    def get(cls, n: int, m: int, device: torch.device, slot: int = 0) -> "BatchWorkspace":
        """One workspace per (device, stream, n, slot): ``slot`` = the sub-batch index, so two
        sub-batches dealt to one stream never share encoder state between a SAMPLE part and
        its FINISH part."""
        key = (device.index if device.index is not None else torch.cuda.current_device(),
               torch.cuda.current_stream(device).cuda_stream, n, slot)
        ws = cls._cache.get(key)
        if ws is None or ws.m < m:
            ws = cls(n, m, device)
            cls._cache[key] = ws
        return ws


_SIDE: dict = {}
_MAX_SIDE = 4          # GPU_MAX_HW_QUEUES is 4: more forked streams would share queues
# k_fused_mag / k_fused64 (the lone magnitude encodes) hold workgroups in a bounded in-kernel
# wait; the library orders those launches per device itself (include/fedcodec.h, Concurrency),
# so any stream may issue them.  A graph replay is bracketed by fc_fused_order_begin / _end.


def _side_streams(dev: torch.device, count: int = 2) -> list:
    """Forked streams for :func:`encode_top_batch` sub-batches (created once per device)."""
    key = dev.index if dev.index is not None else torch.cuda.current_device()
    lst = _SIDE.setdefault(key, [])
    while len(lst) < count:
        lst.append(torch.cuda.Stream(device=dev))
    return lst[:count]


def encode_jobs(grads: Sequence[torch.Tensor], packets: Sequence[Packet], seeds=None,
                offsets=None) -> torch.Tensor:
    """Device array of fc_encode_job (build once, reuse while the buffers live)."""
    m = len(grads)
    seeds = seeds if seeds is not None else [0] * m
    offsets = offsets if offsets is not None else [0] * m
    arr = (L.EncodeJob * m)(*[
        L.EncodeJob(g=g.data_ptr(), idx=p.idx.data_ptr(), val=p.val.data_ptr(),
                    cnt=p.cnt.data_ptr(), hdr=p.hdr.data_ptr(), seed=int(s), offset=int(o),
                    qoff=p.qoff.data_ptr() if p.qoff is not None else 0)
        for g, p, s, o in zip(grads, packets, seeds, offsets)])
    host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
    return host.to(grads[0].device)


def encode_top_batch(grads: Sequence[torch.Tensor], k: int, *,
                     key_mode: int = L.FC_KEY_MAGNITUDE, seeds=None, offsets=None,
                     packets: Optional[Sequence[Packet]] = None,
                     jobs: Optional[torch.Tensor] = None, check: bool = True,
                     streams: int = 1, groups: Optional[Sequence[int]] = None,
                     part: int = L.FC_PART_SAMPLE | L.FC_PART_FINISH, fork: bool = True,
                     join: bool = True) -> list:
    """Top-k (or native rand-k) of M equal-length gradients in ONE launch per pipeline stage
    (fc_topk_encode_batch).  Same packets, bit for bit, as M calls of :func:`encode_top`.
    ``jobs``: a prebuilt :func:`encode_jobs` array for these exact grads/packets.
    ``streams``: sub-batches launched on that many forked streams (joined before return),
    free to run concurrently (the batched kernels never wait in-kernel);
    ``groups``: sub-batch sizes (default: ``streams`` equal parts), dealt to the streams in turn.
    Pipelining (bench.py): ``part`` = FC_PART_SAMPLE or FC_PART_FINISH runs one half of the
    pipeline (fc_topk_encode_batch_part; the same ``groups`` / ``streams`` for both halves, so
    each sub-batch's halves share a stream and its own workspace, keyed by the sub-batch index
    even when more sub-batches than streams share one stream); ``fork=False``: the forked
    streams do not wait for the caller's stream first; ``join=False``: the caller's stream does
    not wait for them (the caller orders later work itself)."""
    if not grads:
        raise ValueError("no gradients")
    lib = L.load()
    n, dev = grads[0].numel(), grads[0].device
    # per-tensor checks once per (jobs table, gradient / packet set): a 128-client step spent
    # ~1 ms of host time in them, which shows as GPU idle time when a step is short (16 M).  The
    # table remembers the checked objects by weak reference and compares identity (not id():
    # CPython reuses the ids of collected objects; a per-tensor signature tuple cost ~1.3 ms
    # per 128-client call, which doubled configs[2]'s step)
    def _same(refs, objs):
        return refs is not None and len(refs) == len(objs) and all(r() is o for r, o in zip(refs, objs))
    checked = (jobs is not None and getattr(jobs, "_fc_checked_n", None) == n
               and _same(getattr(jobs, "_fc_grefs", None), grads)
               and (packets is None or _same(getattr(jobs, "_fc_prefs", None), packets)))
    if not checked:
        for g in grads:
            _require_cuda_f32(g)
            if g.numel() != n or g.device != dev:
                raise ValueError("batched gradients must share length and device")
    if not 0 <= k <= n:
        raise ValueError(f"k={k} outside [0, {n}]")
    m = len(grads)
    seeds = seeds if seeds is not None else [0] * m
    offsets = offsets if offsets is not None else [0] * m
    if packets is None:
        packets = [Packet.alloc(n, L.FC_FMT_IDXVAL, dev, k=k) for _ in range(m)]
    if len(packets) != m:
        raise ValueError("one packet per gradient")
    if part != (L.FC_PART_SAMPLE | L.FC_PART_FINISH) and (k == 0 or k == n or n < 2 or check):
        raise ValueError("a partial batch encode needs 0 < k < n and check=False")
    if k == 0 or k == n or n < 2:                    # trivial thresholds: exact engine per client
        return [encode_top(g, k, key_mode=key_mode, seed=s, offset=o, packet=p, check=check)
                for g, p, s, o in zip(grads, packets, seeds, offsets)]
    cap = int(lib.fc_packet_capacity(n))
    for p, g, s, o in zip(packets, grads, seeds, offsets):
        if not checked and (p.capacity < cap or p.fmt != L.FC_FMT_IDXVAL):
            raise ValueError("packet too small or not idx/val")
        p.k = k
        p._enc = (g, k, key_mode, s, o)
        p._dense_only = False
    if jobs is None:
        jobs = encode_jobs(grads, packets, seeds, offsets)
    elif not checked:
        jobs._fc_checked_n = n
        jobs._fc_grefs = [weakref.ref(g) for g in grads]
        jobs._fc_prefs = [weakref.ref(p) for p in packets]
    nside = max(1, min(int(streams), m, _MAX_SIDE))
    if groups is None:
        groups = [(i + 1) * m // nside - i * m // nside for i in range(nside)]
    groups = [int(x) for x in groups]
    if any(x < 1 for x in groups) or sum(groups) != m:
        raise ValueError(f"groups {groups} must be positive sizes summing to {m} clients")
    if nside == 1 or len(groups) == 1:
        ws = BatchWorkspace.get(n, m, dev)
        L.check(lib.fc_topk_encode_batch_part(_vp(jobs), m, n, k, key_mode, packets[0].capacity,
                                              _vp(ws.buf), ws.nbytes, part, _stream(dev)),
                "fc_topk_encode_batch")
    else:
        # Sub-batches on forked streams (group i on stream i % streams), free to overlap.
        # Packets are identical; the caller's stream joins every fork before this returns, so
        # later work (and frees) stay ordered.
        main = torch.cuda.current_stream(dev)
        job_bytes = ctypes.sizeof(L.EncodeJob)
        base = jobs.data_ptr()
        sides = _side_streams(dev, nside)
        if fork:
            ev = torch.cuda.Event()
            ev.record(main)
            for side in sides:
                side.wait_event(ev)
        lo = 0
        for i, size in enumerate(groups):
            side = sides[i % nside]
            with torch.cuda.stream(side):
                ws = BatchWorkspace.get(n, size, dev, slot=i)
                L.check(lib.fc_topk_encode_batch_part(ctypes.c_void_p(base + lo * job_bytes),
                                                      size, n, k, key_mode, packets[0].capacity,
                                                      _vp(ws.buf), ws.nbytes, part, _stream(dev)),
                        "fc_topk_encode_batch")
            lo += size
        if join:
            for side in sides:
                main.wait_stream(side)
    if check:
        resolve(packets)
    return list(packets)


def ef_jobs(residuals: Sequence[torch.Tensor], residuals_out: Sequence[torch.Tensor]) -> torch.Tensor:
    """Device array of fc_ef_job, entry c beside :func:`encode_jobs`' entry c (build once, reuse
    while the buffers live)."""
    arr = (L.EfJob * len(residuals))(*[L.EfJob(res_in=r.data_ptr(), res_out=o.data_ptr())
                                       for r, o in zip(residuals, residuals_out)])
    host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
    return host.to(residuals_out[0].device)


_ef_jobs = ef_jobs        # (encode_top_ef_batch has a keyword of that name)


def encode_top_ef_batch(grads: Sequence[torch.Tensor], residuals: Sequence[Optional[torch.Tensor]],
                        k: int, *, residuals_out: Optional[Sequence[torch.Tensor]] = None,
                        packets: Optional[Sequence[Packet]] = None,
                        jobs: Optional[torch.Tensor] = None,
                        ef_jobs: Optional[torch.Tensor] = None, check: bool = True):
    """:func:`encode_top_ef` for M equal-length gradients in ONE launch per pipeline stage
    (fc_topk_encode_ef_batch): client c's packet and ``residuals_out[c]`` are, bit for bit, what
    ``encode_top_ef(grads[c], residuals[c], k)`` gives.  Returns ``(packets, residuals_out)``.

    A ``None`` entry of ``residuals`` means zeros.  No ``residuals_out[i]`` may overlap any
    gradient, residual or other output of the batch (ValueError before any launch).  ``jobs`` /
    ``ef_jobs``: prebuilt :func:`encode_jobs` / :func:`ef_jobs` tables for these exact buffers.
    ``check=True`` reads the headers once and runs the exact chain for exactly the clients whose
    bracket missed (``packet.retried``); with ``check=False`` call :func:`resolve` later.
    k = 0, k = n and n < 2 loop over :func:`encode_top_ef`."""
    if not grads:
        raise ValueError("no gradients")
    m = len(grads)
    n, dev = grads[0].numel(), grads[0].device
    if len(residuals) != m or (residuals_out is not None and len(residuals_out) != m):
        raise ValueError("one residual and one output per gradient")
    if packets is not None and len(packets) != m:
        raise ValueError("one packet per gradient")
    if n == 0:
        raise ValueError("empty gradient")
    if not 0 <= k <= n:
        raise ValueError(f"k={k} outside [0, {n}]")
    if any(r is None for r in residuals):            # one shared block of zeros (never written)
        zeros = torch.zeros(n, dtype=torch.float32, device=dev)
        residuals = [zeros if r is None else r for r in residuals]
    if residuals_out is None:
        residuals_out = [torch.empty(n, dtype=torch.float32, device=dev) for _ in range(m)]
    for i in range(m):
        for t, name in ((grads[i], "g"), (residuals[i], "residual"),
                        (residuals_out[i], "residual_out")):
            _require_cuda_f32(t, f"{name}[{i}]")
            if t.numel() != n or t.device != dev:
                raise ValueError(f"{name}[{i}] must have {n} elements on {dev}")
    # address ranges on the host: an output against every input and every other output
    nb = 4 * n
    outs = sorted((o.data_ptr(), i) for i, o in enumerate(residuals_out))
    for (a, i), (b, j) in zip(outs, outs[1:]):
        if b < a + nb:
            raise ValueError(f"residuals_out[{i}] and residuals_out[{j}] overlap")
    starts = [a for a, _ in outs]
    for kind, ts in (("grads", grads), ("residuals", residuals)):
        for j, t in enumerate(ts):
            p = t.data_ptr()
            lo = bisect.bisect_right(starts, p - nb)         # first output starting after p - nb
            if lo < m and starts[lo] < p + nb:
                raise ValueError(f"residuals_out[{outs[lo][1]}] overlaps {kind}[{j}]")
    if packets is None:
        packets = [Packet.alloc(n, L.FC_FMT_IDXVAL, dev, k=k) for _ in range(m)]
    if k == 0 or k == n or n < 2:                    # trivial thresholds: the exact chain per client
        for g, r, o, p in zip(grads, residuals, residuals_out, packets):
            encode_top_ef(g, r, k, residual_out=o, packet=p, check=check)
        return list(packets), list(residuals_out)
    lib = L.load()
    cap = int(lib.fc_packet_capacity(n))
    for p, g, r, o in zip(packets, grads, residuals, residuals_out):
        if p.capacity < cap or p.fmt != L.FC_FMT_IDXVAL:
            raise ValueError("packet too small or not idx/val")
        p.k = k
        p._enc = ("ef", g, r, o, k)
        p._dense_only = False
        p.retried = False
    if jobs is None:
        jobs = encode_jobs(grads, packets)
    if ef_jobs is None:
        ef_jobs = _ef_jobs(residuals, residuals_out)
    ws = BatchWorkspace.get(n, m, dev)
    L.check(lib.fc_topk_encode_ef_batch(_vp(jobs), _vp(ef_jobs), m, n, k, packets[0].capacity,
                                        _vp(ws.buf), ws.nbytes, _stream(dev)),
            "fc_topk_encode_ef_batch")
    if check:
        resolve(packets)
    return list(packets), list(residuals_out)


def encode_fold_batch(grads: Sequence[torch.Tensor], k: int, weights, out: torch.Tensor, *,
                      packets: Sequence[Packet], jobs: Optional[torch.Tensor] = None,
                      views: Optional[torch.Tensor] = None, streams: int = 2,
                      status: Optional[tuple] = None) -> "torch.cuda.Event":
    """Batched top-k encode of M gradients AND their packet FedAVG fold (gar.py:44), pipelined:
    sub-batch i is encoded on forked stream i and folded there as soon as it is encoded,
    continuing sub-batch i-1's partial sum (an event orders the folds, so the rows are added
    in G's order: bit-identical to :func:`encode_top_batch` + :func:`decode_accumulate`), while
    sub-batch i+1 encodes on its own stream.  ``out`` holds the aggregate once the
    caller's stream (joined at return) reaches it.  Returns an event recorded once every
    sub-batch is ENCODED (the folds may still run); ``status=(src, dst)``: ``dst.copy_(src)``
    (e.g. the packet headers' status words into pinned host memory) is queued right then, so
    the host can check the statuses while the last fold runs.  No re-encode here: call
    :func:`resolve` and, if it re-encoded anything, fold again (bench.py does)."""
    lib = L.load()
    m = len(grads)
    if m == 0 or len(packets) != m:
        raise ValueError("one packet per gradient, at least one")
    n, dev = grads[0].numel(), grads[0].device
    if not 0 < k < n:
        raise ValueError("encode_fold_batch needs 0 < k < n")
    weights = [float(x) for x in weights]
    if len(weights) != m:
        raise ValueError("one weight per gradient")
    if jobs is None:
        jobs = encode_jobs(grads, packets)
    if views is None:
        views = views_tensor(packets, weights, dev)
    nside = max(1, min(int(streams), m, _MAX_SIDE))
    groups = [(i + 1) * m // nside - i * m // nside for i in range(nside)]
    jb, vb = ctypes.sizeof(L.EncodeJob), ctypes.sizeof(L.PacketView)
    main = torch.cuda.current_stream(dev)
    sides = _side_streams(dev, nside)
    start = torch.cuda.Event()
    start.record(main)
    prev = None
    encoded = []
    lo = 0
    for i, size in enumerate(groups):
        hi = lo + size
        side = sides[i]
        with torch.cuda.stream(side):
            side.wait_event(start)
            ws = BatchWorkspace.get(n, size, dev, slot=i)
            L.check(lib.fc_topk_encode_batch(ctypes.c_void_p(jobs.data_ptr() + lo * jb), size, n,
                                             k, L.FC_KEY_MAGNITUDE, packets[0].capacity,
                                             _vp(ws.buf), ws.nbytes, _stream(dev)),
                    "fc_topk_encode_batch")
            for p, g in zip(packets[lo:hi], grads[lo:hi]):
                p.k = k
                p._enc = (g, k, L.FC_KEY_MAGNITUDE, 0, 0)
            ev = torch.cuda.Event()
            ev.record(side)
            encoded.append(ev)
            if i == len(groups) - 1:                       # every sub-batch is encoded here
                for e in encoded[:-1]:
                    side.wait_event(e)
                if status is not None:
                    status[1].copy_(status[0], non_blocking=True)
                done = torch.cuda.Event()
                done.record(side)
            if prev is not None:
                side.wait_event(prev)                      # folds in G's row order
            fn = lib.fc_decode_accumulate_continue if i else lib.fc_decode_accumulate
            L.check(fn(ctypes.c_void_p(views.data_ptr() + lo * vb), size, L.FC_FMT_IDXVAL, n,
                       _vp(out), _stream(dev)), "fc_decode_accumulate")
            prev = torch.cuda.Event()
            prev.record(side)
        lo = hi
    main.wait_event(prev)
    for side in sides:                                     # later frees stay ordered
        main.wait_stream(side)
    return done


class GraphedCalls:
    """A sequence of codec calls on fixed tensors, captured once into one HIP graph and replayed
    (the hipGraph form of a launch-bound inner loop).  Replays launch the same kernels on the
    same buffers without the host's per-call work and with cheaper kernel boundaries: a lone
    16 M drop-in dense top-k 48.6 -> 45.0 us per call, the packet encode + decode 60.1 -> 56.7 us
    (tools/graph_probe.py, profiles/r05_graph_probe.jsonl).

    ``fn`` issues the calls (``check=False`` throughout: a status check synchronises, which a
    capture cannot; call :func:`resolve` after a replay).  Every tensor ``fn`` touches must stay
    alive at the same address.  The encoder state in the workspaces is self-cleaning, so each
    replay computes what the eager calls would; the workspace is the capture stream's, so do not
    run eager encodes of the same size on that stream concurrently with a replay."""

    def __init__(self, fn, device: Optional[torch.device] = None, warmup: int = 2):
        dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        self.stream = torch.cuda.Stream(dev)
        self.stream.wait_stream(torch.cuda.current_stream(dev))
        with torch.cuda.stream(self.stream):
            for _ in range(warmup):                      # workspaces, packets, first-call setup
                fn()
        self.stream.synchronize()
        self.graph = torch.cuda.CUDAGraph()
        # thread_local: another thread's stream work (e.g. a process group's watchdog polling
        # its events) is not an error during this capture
        with torch.cuda.graph(self.graph, stream=self.stream, capture_error_mode="thread_local"):
            fn()
        torch.cuda.current_stream(dev).wait_stream(self.stream)

    def replay(self) -> None:
        """Launch the captured calls on the current stream, ordered after the device's last
        in-kernel-waiting encode (fc_fused_order_begin / _end: the library's own ordering does
        not see launches inside a graph)."""
        lib = L.load()
        s = _stream(self.stream.device)
        L.check(lib.fc_fused_order_begin(s), "fc_fused_order_begin")
        self.graph.replay()
        L.check(lib.fc_fused_order_end(s), "fc_fused_order_end")


def resolve(packets: Sequence[Packet]) -> int:
    """Re-encode (exact path) every top/rand packet whose sampled bracket missed.
    Returns the number of packets that needed the exact path."""
    lib = L.load()
    redo = 0
    for p, h in zip(packets, headers(packets)):       # one sync for the whole batch
        if h.status == L.FC_STATUS_OK:
            continue
        if h.status != L.FC_STATUS_RETRY_EXACT or getattr(p, "_enc", None) is None:
            raise L.FedCodecError(f"packet status {h.status}")
        if isinstance(p._enc[0], str):                # error feedback: the exact chain on g + e
            _, g, res, res_out, k = p._enc
            _ef_exact(g, res, res_out, k, p)
            redo += 1
            p.retried = True
            h2 = p.header()
            if h2.status != L.FC_STATUS_OK:
                raise L.FedCodecError(f"exact encode status {h2.status}")
            continue
        g, k, key_mode, seed, offset = p._enc
        ws = Workspace.get(g.numel(), g.device)
        L.check(lib.fc_topk_encode_exact(_vp(g), g.numel(), k, key_mode, seed, offset,
                                         _vp(p.idx), _vp(p.val), p.capacity, _vp(p.cnt),
                                         _vp(p.qoff), _vp(p.hdr), _vp(ws.buf), ws.nbytes,
                                         _stream(g.device)), "fc_topk_encode_exact")
        redo += 1
        p._dense_only = False                        # a full packet now
        h2 = p.header()
        if h2.status != L.FC_STATUS_OK:
            raise L.FedCodecError(f"exact encode status {h2.status}")
    return redo


def encode_mask(g: torch.Tensor, codec: int, *, p: float = 0.5,
                mask_bits: Optional[torch.Tensor] = None, seed: int = 0, offset: int = 0,
                fmt: int = L.FC_FMT_BITMAP, packet: Optional[Packet] = None) -> Packet:
    """Mask codecs: dropout-biased / dropout-unbiased (Philox or host mask) and rand-k with a
    host-drawn permutation mask (parity mode).  ``mask_bits``: int32 device tensor, bit i of
    word i//32 = element i."""
    _require_cuda_f32(g)
    lib = L.load()
    n = g.numel()
    ws = Workspace.get(n, g.device)
    if mask_bits is not None and (mask_bits.dtype != _U32 or not mask_bits.is_cuda
                                  or mask_bits.numel() * 32 < n):
        raise ValueError("mask_bits must be an int32 CUDA tensor of ceil(n/32) words")
    if packet is None:
        packet = Packet.alloc(n, fmt, g.device)
    L.check(lib.fc_mask_encode(_vp(g), n, codec, _vp(mask_bits), float(p), seed, offset, fmt,
                               _vp(packet.idx), _vp(packet.val), _vp(packet.bitmap),
                               packet.capacity, _vp(packet.cnt), _vp(packet.qoff),
                               _vp(packet.hdr), _vp(ws.buf), ws.nbytes, _stream(g.device)),
            "fc_mask_encode")
    return packet


def decode(packet: Packet, out: Optional[torch.Tensor] = None,
           dtype: torch.dtype = torch.float32) -> torch.Tensor:
    """Dense reconstruction (the array compress() returns)."""
    lib = L.load()
    dev = packet.val.device
    if out is None:
        out = torch.empty(packet.n, dtype=dtype, device=dev)
    if out.dtype not in (torch.float32, torch.float64) or out.numel() != packet.n:
        raise ValueError("out must be float32/float64 with n elements")
    v = packet.view()
    L.check(lib.fc_decode_dense(ctypes.byref(v), packet.fmt, packet.n, _vp(out),
                                int(out.dtype == torch.float64), _stream(dev)),
            "fc_decode_dense")
    return out


def views_tensor(packets: Sequence[Packet], weights, device) -> torch.Tensor:
    """Device array of fc_packet_view (client order = G row order)."""
    arr = (L.PacketView * len(packets))(*[p.view(w) for p, w in zip(packets, weights)])
    host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
    return host.to(device)


def decode_accumulate(packets: Sequence[Packet], weights, out: Optional[torch.Tensor] = None,
                      views: Optional[torch.Tensor] = None,
                      continue_sum: bool = False) -> torch.Tensor:
    """FedAVG over packets: bit-exact ``np.sum(G * w[:, None], axis=0)`` (gar.py:44).

    ``continue_sum=True`` folds the packets into the partial sum already in ``out`` (rows of
    G that an earlier call, or an earlier rank of the chained reduce, has summed)."""
    lib = L.load()
    if not packets:
        raise ValueError("no packets")
    fmt, n, dev = packets[0].fmt, packets[0].n, packets[0].val.device
    if any(p.fmt != fmt or p.n != n for p in packets):
        raise ValueError("packets must share n and format")
    if out is None:
        if continue_sum:
            raise ValueError("continue_sum needs the partial sum in `out`")
        out = torch.empty(n, dtype=torch.float32, device=dev)
    _require_cuda_f32(out, "out")
    if out.numel() != n:
        raise ValueError("out must have n elements")
    if views is None:
        views = views_tensor(packets, weights, dev)
    fn = lib.fc_decode_accumulate_continue if continue_sum else lib.fc_decode_accumulate
    L.check(fn(_vp(views), len(packets), fmt, n, _vp(out), _stream(dev)),
            "fc_decode_accumulate")
    return out


class GramWorkspace:
    """Per-(device, stream) scratch of :func:`gram` (the partial Grams; needs no zeroing)."""

    _cache: dict = {}

    def __init__(self, nbytes: int, device: torch.device):
        self.nbytes = nbytes
        self.buf = torch.empty(nbytes, dtype=torch.uint8, device=device)

    @classmethod
    def get(cls, n: int, m: int, device: torch.device) -> "GramWorkspace":
        need = int(L.load().fc_gram_workspace_bytes(n, m))
        key = (device.index if device.index is not None else torch.cuda.current_device(),
               torch.cuda.current_stream(device).cuda_stream)
        ws = cls._cache.get(key)
        if ws is None or ws.nbytes < need:
            ws = cls(need, device)
            cls._cache[key] = ws
        return ws


def gram(packets: Sequence[Packet], out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The (m, m) float64 Gram matrix ``G @ G.T`` of the rows :func:`decode` would make of the
    packets, computed straight from them (fc_packets_gram: exact products, float64 sums, a fixed
    order; a client with a non-finite element gets a NaN row and column).  At most
    ``FC_GRAM_MAX_M`` idx/val packets of one length."""
    if not packets:
        raise ValueError("no packets")
    m, n, dev = len(packets), packets[0].n, packets[0].val.device
    if m > L.FC_GRAM_MAX_M:
        raise ValueError(f"gram takes at most {L.FC_GRAM_MAX_M} packets (got {m})")
    _check_idxval_packets(packets)
    lib = L.load()
    if out is None:
        out = torch.empty((m, m), dtype=torch.float64, device=dev)
    if (not isinstance(out, torch.Tensor) or out.dtype != torch.float64 or out.device != dev
            or tuple(out.shape) != (m, m) or not out.is_contiguous() or out.data_ptr() % 16):
        raise ValueError("out must be a contiguous 16-byte aligned (m, m) float64 tensor on the "
                         "packets' device")
    ws = GramWorkspace.get(n, m, dev)
    views = views_tensor(packets, [1.0] * m, dev)
    L.check(lib.fc_packets_gram(_vp(views), m, n, _vp(out), _vp(ws.buf), ws.nbytes, _stream(dev)),
            "fc_packets_gram")
    return out


class DotWorkspace:
    """Per-(device, stream) scratch of :func:`dot_dense` (the partial sums; needs no zeroing)."""

    _cache: dict = {}

    def __init__(self, nbytes: int, device: torch.device):
        self.nbytes = nbytes
        self.buf = torch.empty(nbytes, dtype=torch.uint8, device=device)

    @classmethod
    def get(cls, n: int, m: int, device: torch.device) -> "DotWorkspace":
        need = int(L.load().fc_dot_workspace_bytes(n, m))
        key = (device.index if device.index is not None else torch.cuda.current_device(),
               torch.cuda.current_stream(device).cuda_stream)
        ws = cls._cache.get(key)
        if ws is None or ws.nbytes < need:
            ws = cls(need, device)
            cls._cache[key] = ws
        return ws


def dot_dense(packets: Sequence[Packet], v: Optional[torch.Tensor] = None,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The (m + 1,) float64 tensor ``[G @ v, v @ v]`` of the rows :func:`decode` would make of the
    packets (the rows :func:`gram` uses) and a dense float32 device vector ``v``, computed
    straight from the packets (fc_packets_dot: exact products, float64 sums, a fixed order).
    ``v=None`` is the all-ones vector: the row sums, then ``float(n)``.  A client with a
    non-finite element gets NaN; a non-finite ``v`` makes every output NaN.  At most
    ``FC_GRAM_MAX_M`` idx/val packets of one length."""
    if not packets:
        raise ValueError("no packets")
    m, n, dev = len(packets), packets[0].n, packets[0].val.device
    if m > L.FC_GRAM_MAX_M:
        raise ValueError(f"gram takes at most {L.FC_GRAM_MAX_M} packets (got {m})")
    _check_idxval_packets(packets)
    if v is not None:
        if (not isinstance(v, torch.Tensor) or v.dtype != torch.float32 or v.device != dev
                or v.numel() != n or not v.is_contiguous() or v.data_ptr() % 16):
            raise ValueError("v must be a contiguous 16-byte aligned float32 tensor of n elements "
                             "on the packets' device")
    lib = L.load()
    if out is None:
        out = torch.empty(m + 1, dtype=torch.float64, device=dev)
    if (not isinstance(out, torch.Tensor) or out.dtype != torch.float64 or out.device != dev
            or tuple(out.shape) != (m + 1,) or not out.is_contiguous() or out.data_ptr() % 16):
        raise ValueError("out must be a contiguous 16-byte aligned (m + 1,) float64 tensor on the "
                         "packets' device")
    ws = DotWorkspace.get(n, m, dev)
    views = views_tensor(packets, [1.0] * m, dev)
    L.check(lib.fc_packets_dot(_vp(views), m, n, _vp(v), _vp(out), _vp(ws.buf), ws.nbytes,
                               _stream(dev)), "fc_packets_dot")
    return out


class TrimWorkspace:
    """Per-(device, stream) scratch of :func:`trimmed_mean`, taken only when
    ``fc_trim_workspace_bytes`` is not 0 (needs no zeroing)."""

    _cache: dict = {}

    def __init__(self, nbytes: int, device: torch.device):
        self.nbytes = nbytes
        self.buf = torch.empty(nbytes, dtype=torch.uint8, device=device)

    @classmethod
    def get(cls, n: int, m: int, device: torch.device) -> Optional["TrimWorkspace"]:
        need = int(L.load().fc_trim_workspace_bytes(n, m))
        if need == 0:
            return None
        key = (device.index if device.index is not None else torch.cuda.current_device(),
               torch.cuda.current_stream(device).cuda_stream)
        ws = cls._cache.get(key)
        if ws is None or ws.nbytes < need:
            ws = cls(need, device)
            cls._cache[key] = ws
        return ws


def _check_trim(m: int, trim) -> int:
    """The (m, trim) pairs :func:`trimmed_mean` takes: the checked trim as an int."""
    if m > L.FC_GRAM_MAX_M:
        raise ValueError(f"trimmed_mean takes at most {L.FC_GRAM_MAX_M} packets (got {m})")
    if isinstance(trim, bool) or not isinstance(trim, (int, np.integer)):
        raise ValueError(f"trim must be an integer (got {trim!r})")
    trim = int(trim)
    if trim < 0:
        raise ValueError(f"trim must not be negative (got {trim})")
    if 2 * trim >= m:
        raise ValueError(f"trim={trim} leaves nothing of {m} packets (2 * trim must be < m)")
    return trim


def trimmed_mean(packets: Sequence[Packet], trim: int,
                 out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The (n,) float32 coordinate-wise trimmed mean of the rows :func:`decode` would make of the
    packets (the rows :func:`gram` uses), computed straight from them (fc_packets_trim): per
    coordinate the m values in ``np.sort``'s order, the ``trim`` smallest and largest dropped,
    the rest added in ascending order in float32 from +0.0 and divided by ``float32(m - 2 trim)``.
    ``trim = (m - 1) // 2`` is the coordinate-wise median.  At most ``FC_GRAM_MAX_M`` idx/val
    packets of one length; ``0 <= trim`` and ``2 * trim < m``."""
    if not packets:
        raise ValueError("no packets")
    m, n, dev = len(packets), packets[0].n, packets[0].val.device
    trim = _check_trim(m, trim)
    _check_idxval_packets(packets)
    lib = L.load()
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=dev)
    if (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.device != dev
            or tuple(out.shape) != (n,) or not out.is_contiguous() or out.data_ptr() % 16):
        raise ValueError("out must be a contiguous 16-byte aligned (n,) float32 tensor on the "
                         "packets' device")
    ws = TrimWorkspace.get(n, m, dev)
    views = views_tensor(packets, [1.0] * m, dev)
    L.check(lib.fc_packets_trim(_vp(views), m, n, trim, _vp(out), _vp(ws.buf if ws else None),
                                ws.nbytes if ws else 0, _stream(dev)), "fc_packets_trim")
    return out


# ---- the wire form of idx/val packets (csrc/fc_wire.hip, include/fedcodec.h) ------------------
@dataclass
class WirePacket:
    """One packet as the contiguous byte string a client sends (include/fedcodec.h): the kept
    entries alone.  ``buf`` is a 16-byte aligned uint8 device tensor whose first ``nbytes`` bytes
    are the packet; ``k`` is the header's k (what :func:`unpack` gives ``Packet.k``)."""
    n: int
    buf: torch.Tensor
    nbytes: int
    k: int = 0

    def tobytes(self) -> bytes:
        """The packet's bytes on the host (synchronises)."""
        return self.buf[: self.nbytes].cpu().numpy().tobytes()


class WireWorkspace:
    """Per-(device, stream) scratch of :func:`pack` (counts and prefix sums; needs no zeroing)."""

    _cache: dict = {}

    def __init__(self, nbytes: int, device: torch.device):
        self.nbytes = nbytes
        self.buf = torch.empty(nbytes, dtype=torch.uint8, device=device)

    @classmethod
    def get(cls, n: int, m: int, device: torch.device) -> "WireWorkspace":
        need = int(L.load().fc_wire_workspace_bytes(n, m))
        key = (device.index if device.index is not None else torch.cuda.current_device(),
               torch.cuda.current_stream(device).cuda_stream)
        ws = cls._cache.get(key)
        if ws is None or ws.nbytes < need:
            ws = cls(need, device)
            cls._cache[key] = ws
        return ws


def wire_bytes(n: int, entries: int) -> int:
    """The exact size of a wire packet of length n with ``entries`` kept entries (host)."""
    return int(L.load().fc_wire_bytes(int(n), int(entries)))


def _wire_jobs(buffers: Sequence[torch.Tensor], sizes: Sequence[int], device) -> torch.Tensor:
    arr = (L.WireJob * len(buffers))(*[L.WireJob(wire=b.data_ptr(), bytes=int(s))
                                       for b, s in zip(buffers, sizes)])
    host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
    return host.to(device)


def _check_idxval_packets(packets: Sequence[Packet]):
    """What :func:`gram`, :func:`dot_dense` and :func:`pack` ask of their packets: (n, device)."""
    if not packets:
        raise ValueError("no packets")
    n, dev = packets[0].n, packets[0].val.device
    for p in packets:
        if p.n != n:
            raise ValueError("packets must share n")
        if p.fmt != L.FC_FMT_IDXVAL or p.idx is None or p.qoff is None:
            raise ValueError("gram needs idx/val packets (FC_FMT_IDXVAL) with quarter offsets")
    return n, dev


def _check_wire_buffer(b, device, what: str):
    if (not isinstance(b, torch.Tensor) or b.dtype != torch.uint8 or b.device != device
            or b.dim() != 1 or not b.is_contiguous() or b.data_ptr() % 16
            or b.numel() < L.WIRE_HDR_BYTES):
        raise ValueError(f"{what} must be a contiguous 16-byte aligned uint8 tensor of at least "
                         f"{L.WIRE_HDR_BYTES} bytes on the packets' device")


def pack_into(packets: Sequence[Packet], buffers: Sequence[torch.Tensor],
              capacities: Optional[Sequence[int]] = None) -> list:
    """fc_wire_pack_batch: packet i into ``buffers[i]`` (uint8 device tensors, 16-byte aligned),
    of which at most ``capacities[i]`` bytes (default: all) may be written.  One launch chain for
    the batch, then ONE synchronising read of the m wire headers.  Returns the m ``L.WireHdr``;
    nothing is raised for a status that is not OK (:func:`pack` does that)."""
    n, dev = _check_idxval_packets(packets)
    m = len(packets)
    if len(buffers) != m or (capacities is not None and len(capacities) != m):
        raise ValueError("one buffer (and one capacity) per packet")
    for b in buffers:
        _check_wire_buffer(b, dev, "a wire buffer")
    caps = [b.numel() for b in buffers] if capacities is None else [int(c) for c in capacities]
    if any(not L.WIRE_HDR_BYTES <= c <= b.numel() for c, b in zip(caps, buffers)):
        raise ValueError(f"a capacity must lie between {L.WIRE_HDR_BYTES} and its buffer's size")
    lib = L.load()
    ws = WireWorkspace.get(n, m, dev)
    views = views_tensor(packets, [1.0] * m, dev)
    jobs = _wire_jobs(buffers, caps, dev)
    L.check(lib.fc_wire_pack_batch(_vp(views), _vp(jobs), m, n, _vp(ws.buf), ws.nbytes,
                                   _stream(dev)), "fc_wire_pack_batch")
    raw = torch.stack([b[: L.WIRE_HDR_BYTES] for b in buffers]).cpu().numpy()
    return [L.WireHdr.from_buffer_copy(raw[i].tobytes()) for i in range(m)]


def slab_bytes(nbytes: int) -> int:
    """Bytes rounded up to 256: the room one packet takes in a device slab of several."""
    return (int(nbytes) + 255) & ~255


def pack(packets, entries=None):
    """The wire form of one idx/val packet or of a sequence of them (one launch chain):
    a :class:`WirePacket`, or a list of them.  Only the entries the decoders keep are packed.

    Each buffer is sized for ``entries`` kept entries (an int, or one per packet) when given;
    otherwise for ``Packet.k`` if the packet came from a top-k / native rand-k encode (resolved:
    it keeps exactly k), and otherwise for its listed entries, found by one synchronising read of
    the counts.  Raises ``FedCodecError`` if a wire status is not OK (a source packet that is not
    resolved, ``entries`` too small)."""
    single = isinstance(packets, Packet)
    pk = [packets] if single else list(packets)
    n, dev = _check_idxval_packets(pk)
    m = len(pk)
    if entries is not None:
        ent = [int(entries)] * m if isinstance(entries, (int, np.integer)) else [int(e) for e in entries]
        if len(ent) != m or any(e < 0 for e in ent):
            raise ValueError("entries: one non-negative count, or one per packet")
    else:
        ent = [int(p.k) if hasattr(p, "_enc") else None for p in pk]
        unknown = [i for i, e in enumerate(ent) if e is None]
        if unknown:                                    # listed >= kept: one read for all of them
            tot = torch.stack([pk[i].cnt.sum(dtype=torch.int64) for i in unknown]).cpu().tolist()
            for i, t in zip(unknown, tot):
                ent[i] = int(t)
    lib = L.load()
    caps = [int(lib.fc_wire_bytes(n, min(e, n))) for e in ent]
    offs = np.concatenate([[0], np.cumsum([slab_bytes(c) for c in caps])]).astype(np.int64)
    slab = torch.empty(int(offs[-1]), dtype=torch.uint8, device=dev)
    bufs = [slab[int(offs[i]): int(offs[i]) + caps[i]] for i in range(m)]
    hdrs = pack_into(pk, bufs)
    out = []
    for i, (h, b) in enumerate(zip(hdrs, bufs)):
        if h.status != L.FC_STATUS_OK:
            raise L.FedCodecError(f"wire packet {i}: status {h.status}"
                                  + (f" ({h.n_entries} entries kept, room for {ent[i]})"
                                     if h.status == L.FC_STATUS_OVERFLOW else ""))
        out.append(WirePacket(n=n, buf=b, nbytes=int(h.total_bytes), k=int(h.pkt.k)))
    return out[0] if single else out


def wire_from_host(data, n: Optional[int] = None, device=None) -> WirePacket:
    """Host bytes (``bytes``, a NumPy uint8 array or a CPU uint8 tensor) as a :class:`WirePacket`
    on ``device``: ALWAYS through ``fc_wire_validate`` first (``ValueError`` with the library's
    reason; no device work has started then), then the H2D copy.  ``n``: the length the packet
    must have.  The only way host bytes become a WirePacket."""
    return TOP.upload(*TOP.check(data, n), device)


def _host_bytes(data) -> np.ndarray:
    """Host bytes (``bytes``, a 1-D NumPy uint8 array or a 1-D CPU uint8 tensor) as a contiguous
    uint8 array, without a copy where none is needed."""
    if isinstance(data, torch.Tensor):
        if data.is_cuda or data.dtype != torch.uint8 or data.dim() != 1:
            raise TypeError("data must be bytes, a 1-D NumPy uint8 array or a 1-D CPU uint8 tensor")
        return data.contiguous().numpy()
    if isinstance(data, (bytes, bytearray, memoryview)):
        return np.frombuffer(data, dtype=np.uint8)
    if isinstance(data, np.ndarray) and data.dtype == np.uint8 and data.ndim == 1:
        return np.ascontiguousarray(data)
    raise TypeError("data must be bytes, a 1-D NumPy uint8 array or a 1-D CPU uint8 tensor")


@dataclass(frozen=True)
class PayloadKind:
    """One kind of wire payload (:data:`TOP`, :data:`SIGN`, :data:`QSGD`): what tells it from the
    others on the way from host bytes to a packet on the device."""
    name: str                          # 'top' | 'sign' | 'qsgd'
    magic: Optional[int]               # None: whatever the other kinds do not claim
    validate: str                      # the library's host validator
    hdr: type                          # the ctypes class of the first 128 bytes
    tag: str                           # the library's prefix of every reason
    packet: Callable                   # (device buffer, header, payload bytes) -> the packet object

    def check(self, data, n: Optional[int] = None):
        """The library's validator on host bytes: (the bytes as a uint8 array, their header), or
        ``ValueError`` with the library's reason.  Touches no device."""
        arr = _host_bytes(data)
        if n is not None and int(n) < 1:
            raise ValueError("n must be at least 1")
        lib = L.load()
        rc = getattr(lib, self.validate)(ctypes.c_void_p(arr.ctypes.data), arr.size, int(n) if n else 0)
        if rc != L.FC_OK:
            msg = lib.fc_last_error()
            raise ValueError(msg.decode() if msg else f"{self.tag}: invalid packet")
        return arr, self.hdr.from_buffer_copy(arr[: L.WIRE_HDR_BYTES].tobytes())

    def upload(self, arr: np.ndarray, hdr, device=None, out: Optional[torch.Tensor] = None):
        """The H2D copy of bytes :meth:`check` has passed (into ``out``, a 16-byte aligned uint8
        device tensor of their size, when given); the packet's tensors are views of the copy."""
        dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
        if arr.flags.writeable:
            host = torch.from_numpy(arr)
        else:                                          # e.g. bytes: only ever read, so no host copy
            with warnings.catch_warnings():
                warnings.simplefilter("ignore", UserWarning)
                host = torch.frombuffer(arr, dtype=torch.uint8)
        if out is None:
            buf = host.to(dev)
        else:
            _check_wire_buffer(out, dev, "out")
            if out.numel() != arr.size:
                raise ValueError("out must have the payload's size")
            buf = out.copy_(host)
        return self.packet(buf, hdr, arr.size)


TOP = PayloadKind("top", None, "fc_wire_validate", L.WireHdr, "wire",
                  lambda buf, hdr, nbytes: WirePacket(n=int(hdr.pkt.n), buf=buf, nbytes=nbytes, k=int(hdr.pkt.k)))
SIGN = PayloadKind("sign", L.SIGN_MAGIC, "fc_sign_wire_validate", L.SignWireHdr, "sign wire",
                   lambda buf, hdr, nbytes: SignPacket(words=buf[L.WIRE_HDR_BYTES:].view(_U32),
                                                       hdr=buf[32:L.WIRE_HDR_BYTES], n=int(hdr.pkt.n), buf=buf))
# the codes at byte 128 of the buffer: 16-byte aligned, as the fold needs
QSGD = PayloadKind("qsgd", L.QSGD_MAGIC, "fc_qsgd_wire_validate", L.QsgdWireHdr, "qsgd wire",
                   lambda buf, hdr, nbytes: QsgdPacket(codes=buf[L.WIRE_HDR_BYTES:].view(_U32),
                                                       hdr=buf[32:L.WIRE_HDR_BYTES], n=int(hdr.pkt.n),
                                                       bits=int(hdr.pkt.k), buf=buf))


def kind_of(data) -> PayloadKind:
    """The kind these host bytes claim by their magic, read once: :data:`SIGN`, :data:`QSGD`, or
    :data:`TOP` for anything else (its validator reports a bad magic itself)."""
    arr = _host_bytes(data)
    magic = int(arr[:4].view(np.uint32)[0]) if arr.size >= 4 else None
    return SIGN if magic == SIGN.magic else QSGD if magic == QSGD.magic else TOP


def _pack_fixed(magic: int, hdr: torch.Tensor, words: torch.Tensor, total: int) -> torch.Tensor:
    """The wire form of a sign or QSGD packet as a device uint8 tensor of ``total`` bytes: the 32
    fixed bytes, the device header, the words and zero bytes after them: copies only, no kernel, no
    synchronisation."""
    fixed = np.zeros(32, dtype=np.uint8)
    fixed[:8].view(np.uint32)[:] = (magic, 1)
    fixed[8:16].view(np.uint64)[0] = total
    buf = torch.empty(total, dtype=torch.uint8, device=words.device)
    end = L.WIRE_HDR_BYTES + 4 * words.numel()
    buf[:32].copy_(torch.from_numpy(fixed))
    buf[32:L.WIRE_HDR_BYTES].copy_(hdr)
    buf[L.WIRE_HDR_BYTES:end].copy_(words.view(torch.uint8))
    if end < total:
        buf[end:].zero_()
    return buf


def unpack(wires, packets=None):
    """Wire packets back into ordinary slotted :class:`Packet` objects (fc_wire_unpack_batch, one
    launch for the batch, no synchronisation): freshly allocated, or ``packets`` reused.  Only
    the listed slot positions, the counts, the quarter offsets and the header are written."""
    single = isinstance(wires, WirePacket)
    ws = [wires] if single else list(wires)
    if not ws:
        raise ValueError("no packets")
    n, dev = ws[0].n, ws[0].buf.device
    for w in ws:
        if w.n != n:
            raise ValueError("packets must share n")
        _check_wire_buffer(w.buf, dev, "a wire packet's buffer")
        if not L.WIRE_HDR_BYTES <= w.nbytes <= w.buf.numel():
            raise ValueError("a wire packet's nbytes lies outside its buffer")
    m = len(ws)
    lib = L.load()
    if packets is None:
        pk = Packet.alloc_batch(n, m, L.FC_FMT_IDXVAL, dev)
    else:
        pk = [packets] if isinstance(packets, Packet) else list(packets)
        if len(pk) != m:
            raise ValueError("one destination packet per wire packet")
        cap = int(lib.fc_packet_capacity(n))
        for p in pk:
            if (p.n != n or p.fmt != L.FC_FMT_IDXVAL or p.idx is None or p.qoff is None
                    or p.capacity < cap or p.val.device != dev):
                raise ValueError("a destination must be an idx/val packet of length n with "
                                 "quarter offsets on the wire packets' device")
    for p, w in zip(pk, ws):
        p.k = w.k
        p.__dict__.pop("_enc", None)               # no encode behind it: pack() reads its counts
        p._dense_only = False
        p.retried = False
    views = views_tensor(pk, [1.0] * m, dev)
    jobs = _wire_jobs([w.buf for w in ws], [w.nbytes for w in ws], dev)
    L.check(lib.fc_wire_unpack_batch(_vp(jobs), _vp(views), m, n, _stream(dev)),
            "fc_wire_unpack_batch")
    return pk[0] if single else pk


def fold_wire(wires: Sequence[WirePacket], weights, out: Optional[torch.Tensor] = None,
              continue_sum: bool = False) -> torch.Tensor:
    """FedAVG straight from wire packets (fc_wire_fold): the bits of
    ``decode_accumulate(unpack(wires), weights, ...)`` without the slotted packets in between.
    Each packet's bytes are read once; no synchronisation.

    ``continue_sum=True`` folds the packets into the partial sum already in ``out``."""
    ws = list(wires)
    if not ws:
        raise ValueError("no packets")
    n, dev = ws[0].n, ws[0].buf.device
    if any(w.n != n for w in ws):
        raise ValueError("packets must share n")
    weights = [float(x) for x in weights]
    if len(weights) != len(ws):
        raise ValueError("one weight per packet")
    if out is None and continue_sum:
        raise ValueError("continue_sum needs the partial sum in `out`")
    for w in ws:
        _check_wire_buffer(w.buf, dev, "a wire packet's buffer")
        if not L.WIRE_HDR_BYTES <= w.nbytes <= w.buf.numel():
            raise ValueError("a wire packet's nbytes lies outside its buffer")
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=dev)
    _require_cuda_f32(out, "out")
    if out.numel() != n:
        raise ValueError("out must have n elements")
    lib = L.load()
    jobs = _wire_jobs([w.buf for w in ws], [w.nbytes for w in ws], dev)
    wts = torch.from_numpy(np.asarray(weights, dtype=np.float32)).to(dev)
    L.check(lib.fc_wire_fold(_vp(jobs), _vp(wts), len(ws), n, _vp(out), int(bool(continue_sum)),
                             _stream(dev)), "fc_wire_fold")
    return out


def weighted_sum_dense(rows, weights: torch.Tensor, out: Optional[torch.Tensor] = None,
                       out_dtype: Optional[torch.dtype] = None, continue_sum: bool = False):
    """gar.py:44 on dense device rows (a (M, N) tensor or a list of 1-D tensors).

    float32 rows and float32 weights: fp32 arithmetic (k_wsum).  Anything float64 (rows,
    weights or ``out_dtype``): NumPy's promotion of ``G * w`` to float64, fp64 arithmetic
    (k_wsum64); the result is float64.  ``continue_sum``: ``out`` holds the sum of earlier
    rows and these rows continue it (same bits as one call over all rows)."""
    lib = L.load()
    if isinstance(rows, torch.Tensor):
        rows = list(rows.unbind(0))
    rdt = rows[0].dtype
    if rdt not in (torch.float32, torch.float64) or any(r.dtype != rdt for r in rows):
        raise TypeError("rows must all be float32 or all float64")
    f64 = rdt == torch.float64 or weights.dtype == torch.float64 or out_dtype == torch.float64
    for r in rows:
        _require_cuda_f32(r, "row", align=4 if rdt == torch.float32 else 8, dtype=rdt)
    n, dev = rows[0].numel(), rows[0].device
    if any(r.numel() != n for r in rows):
        raise ValueError("rows must have equal length")
    ptrs = torch.tensor([r.data_ptr() for r in rows], dtype=torch.int64).to(dev)
    odt = torch.float64 if f64 else torch.float32
    if out is None:
        if continue_sum:
            raise ValueError("continue_sum needs the partial sum in `out`")
        out = torch.empty(n, dtype=odt, device=dev)
    if out.dtype != odt or out.numel() != n or not out.is_cuda:
        raise ValueError(f"out must be a CUDA {odt} tensor of {n} elements")
    if f64:
        w = weights.to(device=dev, dtype=torch.float64).contiguous()   # exact for fp32 weights
        L.check(lib.fc_weighted_sum_dense_f64(_vp(ptrs), int(rdt == torch.float64), _vp(w),
                                              len(rows), n, _vp(out), int(continue_sum),
                                              _stream(dev)), "fc_weighted_sum_dense_f64")
        return out
    w = weights.to(device=dev, dtype=torch.float32).contiguous()
    fn = lib.fc_weighted_sum_dense_continue if continue_sum else lib.fc_weighted_sum_dense
    L.check(fn(_vp(ptrs), _vp(w), len(rows), n, _vp(out), _stream(dev)), "fc_weighted_sum_dense")
    return out


def div_scalar(x: torch.Tensor, d: float) -> torch.Tensor:
    """x = fl(x / d) in place, in x's dtype (the count division of np.mean, aggregation.py:91)."""
    lib = L.load()
    if x.dtype == torch.float64:
        _require_cuda_f32(x, "x", align=8, dtype=torch.float64)
        L.check(lib.fc_div_scalar_f64(_vp(x), x.numel(), float(d), _stream(x.device)),
                "fc_div_scalar_f64")
        return x
    _require_cuda_f32(x, "x")
    L.check(lib.fc_div_scalar(_vp(x), x.numel(), ctypes.c_float(d), _stream(x.device)),
            "fc_div_scalar")
    return x


# ---- scaled sign with error feedback (opt-in, no reference counterpart; csrc/fc_sign.hip) ------
@dataclass
class SignPacket:
    """A scaled-sign packet in HBM (include/fedcodec.h): n sign bits, bit ``t % 32`` of word
    ``t // 32``, and the float32 scale in the header's ``p``."""
    words: torch.Tensor          # int32[fc_sign_words(n)] (uint32 payload), 16-byte aligned
    hdr: torch.Tensor            # uint8[HDR_BYTES]
    n: int
    fmt: int = L.FC_FMT_SIGN
    buf: Optional[torch.Tensor] = None     # sign_from_host: the uploaded payload both live in

    @classmethod
    def alloc(cls, n: int, device) -> "SignPacket":
        if n < 1:
            raise ValueError("a sign packet needs n >= 1")
        words = int(L.load().fc_sign_words(n))
        return cls(torch.empty(words, dtype=_U32, device=device),
                   torch.empty(L.HDR_BYTES, dtype=torch.uint8, device=device), n)

    def view(self, weight: float = 1.0) -> L.PacketView:
        return L.PacketView(idx=0, val=0, bitmap=self.words.data_ptr(), cnt=0,
                            hdr=self.hdr.data_ptr(), qoff=0, weight=float(np.float32(weight)),
                            reserved=0)

    def header(self) -> L.PacketHdr:
        """Synchronous D2H read of the device header."""
        return L.PacketHdr.from_buffer_copy(self.hdr.cpu().numpy().tobytes())

    def scale(self) -> np.float32:
        """The packet's scale s (synchronises)."""
        return np.float32(self.header().p)


_SIGN_WS = {}


def _check_sign_packets(packets) -> list:
    pk = list(packets)
    if not pk:
        raise ValueError("no packets")
    if not all(isinstance(p, SignPacket) for p in pk):
        raise TypeError("sign packets expected (codec.encode_sign, codec.sign_from_host)")
    n, dev = pk[0].n, pk[0].words.device
    need = int(L.load().fc_sign_words(n))
    for p in pk:
        if p.n != n or p.words.device != dev:
            raise ValueError("packets must share n and the device")
        if p.words.dtype != _U32 or p.words.numel() < need or p.words.data_ptr() % 16:
            raise ValueError("a sign packet's words must be 16-byte aligned int32[fc_sign_words(n)]")
    return pk


def encode_sign(g: torch.Tensor, residual: Optional[torch.Tensor] = None,
                residual_out: Optional[torch.Tensor] = None, *,
                packet: Optional[SignPacket] = None):
    """The scaled-sign packet of ``a = fl32(g + residual)`` (``a = g`` without a residual):
    ``s = fl32(sum |a| / n)`` in float64 in a fixed order and the sign bits of ``a``
    (fc_sign_encode: a norm pass and a streaming pass, no synchronisation).  With ``residual`` or
    ``residual_out`` given it also writes the new residual ``e' = fl32(a - q)``, ``q = +-s`` (into
    ``residual_out``, which may not overlap ``g`` or ``residual``; allocated when None).
    Returns ``(packet, new residual or None)``."""
    lib = L.load()
    _require_cuda_f32(g)
    n, dev = g.numel(), g.device
    if n < 1:
        raise ValueError("encode_sign needs n >= 1")
    want = residual is not None or residual_out is not None
    for name, t in (("residual", residual), ("residual_out", residual_out)):
        if t is not None:
            _require_cuda_f32(t, name)
            if t.numel() != n or t.device != dev:
                raise ValueError(f"{name} must have g's length and device")
    if want and residual_out is None:
        residual_out = torch.empty(n, dtype=torch.float32, device=dev)
    if packet is None:
        packet = SignPacket.alloc(n, dev)
    elif packet.n != n or packet.words.device != dev:
        raise ValueError("packet must have g's length and device")
    key = (dev.index if dev.index is not None else torch.cuda.current_device(),
           torch.cuda.current_stream(dev).cuda_stream)        # k_sign_norm's ticket: per stream
    ws = _SIGN_WS.get(key)
    if ws is None:
        ws = _SIGN_WS[key] = torch.zeros(int(lib.fc_sign_workspace_bytes(n)), dtype=torch.uint8,
                                         device=dev)
    L.check(lib.fc_sign_encode(_vp(g), _vp(residual), _vp(residual_out), n, _vp(packet.words),
                               packet.words.numel(), _vp(packet.hdr), _vp(ws), ws.numel(),
                               _stream(dev)), "fc_sign_encode")
    return packet, residual_out


_SIGN_BATCH_WS = {}


def sign_jobs(grads: Sequence[torch.Tensor], packets: Sequence[SignPacket],
              residuals: Optional[Sequence[torch.Tensor]] = None,
              residuals_out: Optional[Sequence[torch.Tensor]] = None) -> torch.Tensor:
    """Device array of fc_sign_job for :func:`encode_sign_batch` (build once, reuse while the
    buffers live)."""
    m = len(grads)
    none = [None] * m
    arr = (L.SignJob * m)(*[
        L.SignJob(g=g.data_ptr(), res_in=r.data_ptr() if r is not None else 0,
                  res_out=o.data_ptr() if o is not None else 0, words=p.words.data_ptr(),
                  hdr=p.hdr.data_ptr(), reserved=0)
        for g, p, r, o in zip(grads, packets, residuals or none, residuals_out or none)])
    host = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8)
    return host.to(grads[0].device)


def _disjoint(ranges, what: str) -> None:
    """``ranges``: (start, bytes, index); ValueError when two of them share a byte."""
    ranges = sorted(ranges)
    for (a, la, i), (b, _, j) in zip(ranges, ranges[1:]):
        if b < a + la:
            raise ValueError(f"{what}[{i}] and {what}[{j}] overlap")


def encode_sign_batch(grads: Sequence[torch.Tensor],
                      residuals: Optional[Sequence[torch.Tensor]] = None,
                      residuals_out: Optional[Sequence[torch.Tensor]] = None, *,
                      want_residuals: Optional[bool] = None,
                      packets: Optional[Sequence[SignPacket]] = None,
                      jobs: Optional[torch.Tensor] = None):
    """:func:`encode_sign` for M equal-length gradients in one launch (two when the new residuals
    are written; fc_sign_encode_batch): client c's header, words and ``residuals_out[c]`` are, byte
    for byte, what ``encode_sign(grads[c], residuals[c], residuals_out[c])`` gives.  Returns
    ``(packets, residuals_out or None)``.

    ``residuals`` is None or one tensor per gradient (zeros are not "no residual" for this codec:
    a None entry is a ValueError).  The new residuals are written when ``residuals`` or
    ``residuals_out`` is given, or as ``want_residuals`` says when it is not None; they are
    allocated when missing.  No ``residuals_out[i]`` may overlap any gradient, residual or other
    output of the batch, and the packets' storage is distinct (ValueError before any launch).
    ``jobs``: a prebuilt :func:`sign_jobs` table for these exact buffers."""
    if not grads:
        raise ValueError("no gradients")
    lib = L.load()
    m = len(grads)
    if m > 65535:
        raise ValueError(f"{m} gradients: at most 65535 per call")
    _require_cuda_f32(grads[0], "g[0]")
    n, dev = grads[0].numel(), grads[0].device
    if n < 1:
        raise ValueError("encode_sign_batch needs n >= 1")
    want = want_residuals if want_residuals is not None else (residuals is not None or residuals_out is not None)
    if residuals_out is not None and not want:
        raise ValueError("residuals_out given with want_residuals=False")
    for name, ts in (("residuals", residuals), ("residuals_out", residuals_out), ("packets", packets)):
        if ts is not None and len(ts) != m:
            raise ValueError(f"{name}: one per gradient")
    if residuals is not None and any(r is None for r in residuals):
        raise ValueError("a residual is None: pass residuals=None for a batch without residuals "
                         "(zeros are not 'no residual' for the sign codec)")
    if want and residuals_out is None:
        residuals_out = [torch.empty(n, dtype=torch.float32, device=dev) for _ in range(m)]
    for name, ts in (("g", grads), ("residual", residuals), ("residual_out", residuals_out)):
        for i, t in enumerate(ts or ()):
            _require_cuda_f32(t, f"{name}[{i}]")
            if t.numel() != n or t.device != dev:
                raise ValueError(f"{name}[{i}] must have {n} elements on {dev}")
    nb = 4 * n
    if want:                 # address ranges on the host: an output against every input and output
        outs = sorted((o.data_ptr(), i) for i, o in enumerate(residuals_out))
        _disjoint([(a, nb, i) for a, i in outs], "residuals_out")
        starts = [a for a, _ in outs]
        for kind, ts in (("grads", grads), ("residuals", residuals or ())):
            for j, t in enumerate(ts):
                p = t.data_ptr()
                lo = bisect.bisect_right(starts, p - nb)        # first output starting after p - nb
                if lo < m and starts[lo] < p + nb:
                    raise ValueError(f"residuals_out[{outs[lo][1]}] overlaps {kind}[{j}]")
    if packets is None:
        packets = [SignPacket.alloc(n, dev) for _ in range(m)]
    need = int(lib.fc_sign_words(n))
    for i, p in enumerate(packets):
        if not isinstance(p, SignPacket):
            raise TypeError("sign packets expected (codec.SignPacket.alloc)")
        if p.n != n or p.words.device != dev or p.hdr.device != dev:
            raise ValueError(f"packets[{i}] must have the gradients' length and device")
        if p.words.dtype != _U32 or p.words.numel() < need or p.words.data_ptr() % 16:
            raise ValueError("a sign packet's words must be 16-byte aligned int32[fc_sign_words(n)]")
        if p.hdr.dtype != torch.uint8 or p.hdr.numel() < L.HDR_BYTES or p.hdr.data_ptr() % 8:
            raise ValueError("a sign packet's header must be 8-byte aligned uint8[96]")
    _disjoint([(p.words.data_ptr(), 4 * need, i) for i, p in enumerate(packets)], "packets")
    _disjoint([(p.hdr.data_ptr(), L.HDR_BYTES, i) for i, p in enumerate(packets)], "packets")
    if jobs is None:
        jobs = sign_jobs(grads, packets, residuals, residuals_out if want else None)
    elif (not isinstance(jobs, torch.Tensor) or jobs.device != dev or jobs.dtype != torch.uint8
          or jobs.numel() < m * ctypes.sizeof(L.SignJob) or jobs.data_ptr() % 8):
        raise ValueError("jobs must be the uint8 device table codec.sign_jobs made for these buffers")
    key = (dev.index if dev.index is not None else torch.cuda.current_device(),
           torch.cuda.current_stream(dev).cuda_stream)        # the clients' tickets: per stream
    ws = _SIGN_BATCH_WS.get(key)
    nbytes = int(lib.fc_sign_batch_workspace_bytes(n, m))
    if ws is None or ws.numel() < nbytes:                     # grown to the largest m seen
        ws = _SIGN_BATCH_WS[key] = torch.zeros(nbytes, dtype=torch.uint8, device=dev)
    L.check(lib.fc_sign_encode_batch(_vp(jobs), m, n, int(residuals is not None), int(bool(want)),
                                     _vp(ws), ws.numel(), _stream(dev)), "fc_sign_encode_batch")
    return list(packets), (list(residuals_out) if want else None)


def decode_sign(packet: SignPacket, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The dense ``q = +-s`` of a sign packet (fc_sign_decode)."""
    (packet,) = _check_sign_packets([packet])
    dev = packet.words.device
    if out is None:
        out = torch.empty(packet.n, dtype=torch.float32, device=dev)
    _require_cuda_f32(out, "out")
    if out.numel() != packet.n:
        raise ValueError("out must have n elements")
    v = packet.view()
    L.check(L.load().fc_sign_decode(ctypes.byref(v), packet.n, _vp(out), _stream(dev)),
            "fc_sign_decode")
    return out


def _sign_views(pk, weights, dev) -> torch.Tensor:
    arr = (L.PacketView * len(pk))(*[p.view(float(w)) for p, w in zip(pk, weights)])
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)


def fold_sign(packets: Sequence[SignPacket], weights, out: Optional[torch.Tensor] = None,
              continue_sum: bool = False) -> torch.Tensor:
    """FedAVG straight from sign packets (fc_sign_fold): the bits of :func:`weighted_sum_dense`
    on the rows :func:`decode_sign` gives, reading N/8 bytes per client.  ``continue_sum=True``
    folds into the partial sum already in ``out``."""
    pk = _check_sign_packets(packets)
    weights = [float(x) for x in weights]
    if len(weights) != len(pk):
        raise ValueError("one weight per packet")
    n, dev = pk[0].n, pk[0].words.device
    if out is None:
        if continue_sum:
            raise ValueError("continue_sum needs the partial sum in `out`")
        out = torch.empty(n, dtype=torch.float32, device=dev)
    _require_cuda_f32(out, "out")
    if out.numel() != n:
        raise ValueError("out must have n elements")
    L.check(L.load().fc_sign_fold(_vp(_sign_views(pk, weights, dev)), len(pk), n, _vp(out),
                                  int(bool(continue_sum)), _stream(dev)), "fc_sign_fold")
    return out


def vote_sign(packets: Sequence[SignPacket], eta: float,
              out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The majority vote over sign packets (fc_sign_vote): ``-eta`` where more than half of the
    clients send a set bit, ``+eta`` where fewer do, ``+0.0`` on a tie.  Scales and weights play
    no part."""
    pk = _check_sign_packets(packets)
    n, dev = pk[0].n, pk[0].words.device
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=dev)
    _require_cuda_f32(out, "out")
    if out.numel() != n:
        raise ValueError("out must have n elements")
    L.check(L.load().fc_sign_vote(_vp(_sign_views(pk, [1.0] * len(pk), dev)), len(pk), n,
                                  ctypes.c_float(float(np.float32(eta))), _vp(out), _stream(dev)),
            "fc_sign_vote")
    return out


class SignGramWorkspace:
    """Per-(device, stream) scratch of :func:`gram_sign` (the partial counts; needs no zeroing)."""

    _cache: dict = {}
    _size = "fc_sign_gram_workspace_bytes"

    def __init__(self, nbytes: int, device: torch.device):
        self.nbytes = nbytes
        self.buf = torch.empty(nbytes, dtype=torch.uint8, device=device)

    @classmethod
    def get(cls, n: int, m: int, device: torch.device):
        need = int(getattr(L.load(), cls._size)(n, m))
        key = (device.index if device.index is not None else torch.cuda.current_device(),
               torch.cuda.current_stream(device).cuda_stream)
        ws = cls._cache.get(key)
        if ws is None or ws.nbytes < need:
            ws = cls(need, device)
            cls._cache[key] = ws
        return ws


class SignDotWorkspace(SignGramWorkspace):
    """Per-(device, stream) scratch of :func:`dot_sign` (the partial sums; needs no zeroing)."""

    _cache: dict = {}
    _size = "fc_sign_dot_workspace_bytes"


def _check_sign_round(packets) -> list:
    pk = _check_sign_packets(packets)
    if len(pk) > L.FC_GRAM_MAX_M:
        raise ValueError(f"gram takes at most {L.FC_GRAM_MAX_M} packets (got {len(pk)})")
    return pk


def gram_sign(packets: Sequence[SignPacket], out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The (m, m) float64 Gram matrix ``G @ G.T`` of the rows :func:`decode_sign` would make of
    the packets, computed straight from their bits (fc_sign_gram): ``s_i s_j (n - 2 H_ij)`` with
    ``H_ij`` the exact Hamming distance, one float64 multiply per entry, so every entry is the
    correctly rounded inner product and no order of summation exists; a client with a non-finite
    scale gets a NaN row and column.  At most ``FC_GRAM_MAX_M`` sign packets of one length."""
    pk = _check_sign_round(packets)
    m, n, dev = len(pk), pk[0].n, pk[0].words.device
    if out is None:
        out = torch.empty((m, m), dtype=torch.float64, device=dev)
    if (not isinstance(out, torch.Tensor) or out.dtype != torch.float64 or out.device != dev
            or tuple(out.shape) != (m, m) or not out.is_contiguous() or out.data_ptr() % 16):
        raise ValueError("out must be a contiguous 16-byte aligned (m, m) float64 tensor on the "
                         "packets' device")
    ws = SignGramWorkspace.get(n, m, dev)
    views = _sign_views(pk, [1.0] * m, dev)
    L.check(L.load().fc_sign_gram(_vp(views), m, n, _vp(out), _vp(ws.buf), ws.nbytes, _stream(dev)),
            "fc_sign_gram")
    return out


def dot_sign(packets: Sequence[SignPacket], v: Optional[torch.Tensor] = None,
             out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The (m + 1,) float64 tensor ``[G @ v, v @ v]`` of the rows :func:`decode_sign` would make of
    the packets (the rows :func:`gram_sign` uses) and a dense float32 device vector ``v``, computed
    straight from the bits (fc_sign_dot: float64 sums in a fixed order, then one multiply by the
    scale).  ``v=None`` is the all-ones vector: ``s_i (n - 2 popcount_i)`` exactly, then
    ``float(n)``.  A client with a non-finite scale gets NaN; a non-finite ``v`` makes every output
    NaN.  At most ``FC_GRAM_MAX_M`` sign packets of one length."""
    pk = _check_sign_round(packets)
    m, n, dev = len(pk), pk[0].n, pk[0].words.device
    if v is not None:
        if (not isinstance(v, torch.Tensor) or v.dtype != torch.float32 or v.device != dev
                or v.numel() != n or not v.is_contiguous() or v.data_ptr() % 16):
            raise ValueError("v must be a contiguous 16-byte aligned float32 tensor of n elements "
                             "on the packets' device")
    if out is None:
        out = torch.empty(m + 1, dtype=torch.float64, device=dev)
    if (not isinstance(out, torch.Tensor) or out.dtype != torch.float64 or out.device != dev
            or tuple(out.shape) != (m + 1,) or not out.is_contiguous() or out.data_ptr() % 16):
        raise ValueError("out must be a contiguous 16-byte aligned (m + 1,) float64 tensor on the "
                         "packets' device")
    ws = SignDotWorkspace.get(n, m, dev)
    views = _sign_views(pk, [1.0] * m, dev)
    L.check(L.load().fc_sign_dot(_vp(views), m, n, _vp(v), _vp(out), _vp(ws.buf), ws.nbytes,
                                 _stream(dev)), "fc_sign_dot")
    return out


class SignTrimWorkspace(SignGramWorkspace):
    """Per-(device, stream) scratch of :func:`trimmed_mean_sign`, taken only when
    ``fc_sign_trim_workspace_bytes`` is not 0 (needs no zeroing)."""

    _cache: dict = {}
    _size = "fc_sign_trim_workspace_bytes"


def trimmed_mean_sign(packets: Sequence[SignPacket], trim: int,
                      out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """The (n,) float32 coordinate-wise trimmed mean of the rows :func:`decode_sign` would make of
    the packets, computed straight from their bits (fc_sign_trim): :func:`trimmed_mean`'s
    definition on columns that hold only ``-s_i`` and ``+s_i``, whose ``np.sort`` order follows
    from the order of the scales, so nothing is sorted per coordinate.  ``trim = (m - 1) // 2`` is
    the coordinate-wise median.  A client with a NaN scale is trimmed like a largest value in every
    column.  At most ``FC_GRAM_MAX_M`` sign packets of one length; ``0 <= trim`` and
    ``2 * trim < m``."""
    pk = _check_sign_round(packets)
    m, n, dev = len(pk), pk[0].n, pk[0].words.device
    trim = _check_trim(m, trim)
    lib = L.load()
    if out is None:
        out = torch.empty(n, dtype=torch.float32, device=dev)
    if (not isinstance(out, torch.Tensor) or out.dtype != torch.float32 or out.device != dev
            or tuple(out.shape) != (n,) or not out.is_contiguous() or out.data_ptr() % 16):
        raise ValueError("out must be a contiguous 16-byte aligned (n,) float32 tensor on the "
                         "packets' device")
    ws = SignTrimWorkspace.get(n, m, dev) if int(lib.fc_sign_trim_workspace_bytes(n, m)) else None
    views = _sign_views(pk, [1.0] * m, dev)
    L.check(lib.fc_sign_trim(_vp(views), m, n, trim, _vp(out), _vp(ws.buf if ws else None),
                             ws.nbytes if ws else 0, _stream(dev)), "fc_sign_trim")
    return out


def sign_wire_bytes(n: int) -> int:
    """The size of a sign packet's wire form: 128 + 4 fc_sign_words(n)."""
    return L.WIRE_HDR_BYTES + 4 * int(L.load().fc_sign_words(n))


def pack_sign(packet: SignPacket) -> torch.Tensor:
    """The wire form of a sign packet as a device uint8 tensor (include/fedcodec.h): the 32 fixed
    bytes, the device header and the words, three copies and no kernel, no synchronisation."""
    (packet,) = _check_sign_packets([packet])
    words = int(L.load().fc_sign_words(packet.n))
    total = L.WIRE_HDR_BYTES + 4 * words
    return _pack_fixed(SIGN.magic, packet.hdr, packet.words[:words], total)


def is_sign_payload(data) -> bool:
    """Do these host bytes start with the sign packet's magic?"""
    return kind_of(data) is SIGN


def sign_from_host(data, n: Optional[int] = None, device=None) -> SignPacket:
    """Host bytes as a :class:`SignPacket` on ``device``: ALWAYS through ``fc_sign_wire_validate``
    first (``ValueError`` with the library's reason; no device work has started then), then the
    H2D copy.  ``n``: the length the packet must have."""
    return SIGN.upload(*SIGN.check(data, n), device)


# ---- float64 gradients (attack_models.py:105-106 -> aggregation.py:61) ----------------------
def _f64_status(out: torch.Tensor) -> torch.Tensor:
    """The device status word of ONE output (k_compact64 sets it OK, k_resolve64 raises it to
    RETRY): each output keeps its own, so several unchecked encodes are each resolvable."""
    st = getattr(out, "_fc_f64_status", None)
    if st is None or st.device != out.device:
        st = torch.empty(1, dtype=_U32, device=out.device)
        out._fc_f64_status = st
    return st


def compress_top_dense_f64(g: torch.Tensor, k: int, *, key_mode: int = L.FC_KEY_MAGNITUDE,
                           seed: int = 0, offset: int = 0,
                           out: Optional[torch.Tensor] = None, check: bool = True,
                           exact: bool = False) -> torch.Tensor:
    """compression.py:31-37 ('top') / native 'rand' (PHILOX keys) on a float64 gradient: the
    dense float64 q (same tie rule as fp32).  'top' with 0 < k < n takes the sampled path
    (fc_topk_dense_f64_sampled: one streaming pass); ``check=True`` reads its status (one
    sync) and re-runs a missed bracket exactly; with ``check=False`` call
    :func:`resolve_f64` on the output later (each output has its own status word).  Native rand-k, trivial k and
    ``exact=True``: the exact radix select (fc_topk_dense_f64)."""
    _require_cuda_f32(g, align=8, dtype=torch.float64)
    n = g.numel()
    if not 0 <= k <= n:
        raise ValueError(f"k={k} outside [0, {n}]")
    if out is None:
        out = torch.empty(n, dtype=torch.float64, device=g.device)
    _require_cuda_f32(out, "out", align=8, dtype=torch.float64)
    if out.numel() != n:
        raise ValueError("out must have n elements")
    lib = L.load()
    ws = Workspace.get(n, g.device)
    sampled = (not exact and key_mode == L.FC_KEY_MAGNITUDE and 0 < k < n
               and g.data_ptr() % 16 == 0 and out.data_ptr() % 16 == 0)
    if sampled:
        st = _f64_status(out)
        L.check(lib.fc_topk_dense_f64_sampled(_vp(g), n, k, _vp(out), _vp(ws.buf), ws.nbytes,
                                              _vp(st), _stream(g.device)),
                "fc_topk_dense_f64_sampled")
        out._fc_f64_enc = (g, k)
        if check:
            resolve_f64(out)
        return out
    L.check(lib.fc_topk_dense_f64(_vp(g), n, k, key_mode, seed, offset, _vp(out), _vp(ws.buf),
                                  ws.nbytes, _stream(g.device)), "fc_topk_dense_f64")
    return out


def resolve_f64(out: torch.Tensor) -> int:
    """After a sampled fp64 encode into ``out`` (check=False): if its bracket missed (the
    output's own status word), redo it exactly into ``out``.  Returns 1 if it did, else 0."""
    st = getattr(out, "_fc_f64_status", None)
    if st is None or getattr(out, "_fc_f64_enc", None) is None:
        return 0                                   # not a sampled encode's output
    if int(st.item()) == L.FC_STATUS_OK:
        return 0
    g, k = out._fc_f64_enc
    compress_top_dense_f64(g, k, out=out, exact=True)
    return 1


def mask_dense_f64(g: torch.Tensor, codec: int, *, p: float = 0.5,
                   mask_bits: Optional[torch.Tensor] = None, seed: int = 0, offset: int = 0,
                   out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """'rand' (host permutation mask) and 'dropout-*' on a float64 OR float32 gradient, with
    the reference's float64 arithmetic (g * mask, (g * mask) / p; a float32 g is promoted
    exactly, as NumPy does): fc_mask_dense_f64 / fc_mask_dense_f32.  Result: float64."""
    f32 = isinstance(g, torch.Tensor) and g.dtype == torch.float32
    if f32:
        _require_cuda_f32(g, align=4)
    else:
        _require_cuda_f32(g, align=8, dtype=torch.float64)
    n = g.numel()
    if mask_bits is not None and (mask_bits.dtype != _U32 or not mask_bits.is_cuda
                                  or mask_bits.numel() * 32 < n):
        raise ValueError("mask_bits must be an int32 CUDA tensor of ceil(n/32) words")
    if out is None:
        out = torch.empty(n, dtype=torch.float64, device=g.device)
    _require_cuda_f32(out, "out", align=8, dtype=torch.float64)
    if out.numel() != n:
        raise ValueError("out must have n elements")
    lib = L.load()
    fn = lib.fc_mask_dense_f32 if f32 else lib.fc_mask_dense_f64
    L.check(fn(_vp(g), n, codec, _vp(mask_bits), float(p), seed, offset, _vp(out),
               _stream(g.device)), "fc_mask_dense_f32" if f32 else "fc_mask_dense_f64")
    return out


# ---- QSGD (compression.py:62-74; opt-in, parity unpinned: oracle/qsgd_oracle.py) ----------
@dataclass
class QsgdPacket:
    codes: torch.Tensor          # uint32[fc_qsgd_code_words(n, bits)]
    hdr: torch.Tensor            # uint8[HDR_BYTES]
    n: int
    bits: int
    buf: Optional[torch.Tensor] = None     # qsgd_from_host: the uploaded payload both live in

    @classmethod
    def alloc(cls, n: int, bits: int, device) -> "QsgdPacket":
        lib = L.load()
        words = int(lib.fc_qsgd_code_words(n, bits))
        if words == 0:
            raise ValueError(f"bits={bits} outside [1, 14]")
        return cls(torch.empty(words, dtype=torch.int32, device=device),
                   torch.zeros(L.HDR_BYTES, dtype=torch.uint8, device=device), n, bits)

    def view(self, weight: float = 1.0) -> L.PacketView:
        v = L.PacketView()
        v.idx = self.codes.data_ptr()
        v.hdr = self.hdr.data_ptr()
        v.weight = weight
        return v

    def header(self) -> L.PacketHdr:
        return L.PacketHdr.from_buffer_copy(bytes(self.hdr.cpu().numpy()))


_QSGD_WS = {}


def encode_qsgd(g: torch.Tensor, bits: int, *, seed: int = 0, offset: int = 0,
                packet: Optional[QsgdPacket] = None, residual: Optional[torch.Tensor] = None,
                residual_out: Optional[torch.Tensor] = None):
    """QSGD codes of a device gradient (two streaming passes: ||g||, then quantise).

    With ``residual`` or ``residual_out`` given (error feedback, fc_qsgd_encode_ef) the packet is
    that of ``a = fl32(g + residual)`` (``a = g`` without a residual) and the same two passes also
    write the new residual ``e' = fl32(a - q)``, ``q`` what :func:`decode_qsgd` gives for the packet
    (into ``residual_out``, which may not overlap ``g`` or ``residual``; allocated when None); the
    call then returns ``(packet, new residual)`` as :func:`encode_sign` does.  Without either it
    returns the packet alone."""
    lib = L.load()
    _require_cuda_f32(g)
    n, dev = g.numel(), g.device
    want = residual is not None or residual_out is not None
    for name, t in (("residual", residual), ("residual_out", residual_out)):
        if t is not None:
            _require_cuda_f32(t, name)
            if t.numel() != n or t.device != dev:
                raise ValueError(f"{name} must have g's length and device")
    if want and residual_out is None:
        residual_out = torch.empty(n, dtype=torch.float32, device=dev)
    if packet is None:
        packet = QsgdPacket.alloc(n, bits, dev)
    key = (dev.index if dev.index is not None else torch.cuda.current_device(),
           torch.cuda.current_stream(dev).cuda_stream)        # k_qsgd_norm's ticket: per stream
    ws = _QSGD_WS.get(key)
    if ws is None:
        ws = _QSGD_WS[key] = torch.zeros(int(lib.fc_qsgd_workspace_bytes()), dtype=torch.uint8,
                                         device=dev)
    if want:
        L.check(lib.fc_qsgd_encode_ef(_vp(g), _vp(residual), _vp(residual_out), n, bits, seed, offset,
                                      _vp(packet.codes), packet.codes.numel(), _vp(packet.hdr),
                                      _vp(ws), ws.numel(), _stream(dev)), "fc_qsgd_encode_ef")
        return packet, residual_out
    L.check(lib.fc_qsgd_encode(_vp(g), n, bits, seed, offset, _vp(packet.codes),
                               packet.codes.numel(), _vp(packet.hdr), _vp(ws), ws.numel(),
                               _stream(dev)), "fc_qsgd_encode")
    return packet


def decode_qsgd(packet: QsgdPacket, out: Optional[torch.Tensor] = None) -> torch.Tensor:
    lib = L.load()
    dev = packet.codes.device
    if out is None:
        out = torch.empty(packet.n, dtype=torch.float32, device=dev)
    _require_cuda_f32(out, "out")
    v = packet.view()
    L.check(lib.fc_qsgd_decode(ctypes.byref(v), packet.n, _vp(out), _stream(dev)), "fc_qsgd_decode")
    return out


def decode_accumulate_qsgd(packets: Sequence[QsgdPacket], weights, out: Optional[torch.Tensor] = None,
                           continue_sum: bool = False) -> torch.Tensor:
    """FedAVG over QSGD packets: gar.py:44 on the dense rows they decode to (bit-exact)."""
    lib = L.load()
    if not packets:
        raise ValueError("no packets")
    n, dev = packets[0].n, packets[0].codes.device
    if any(p.n != n for p in packets):
        raise ValueError("packets must share n")
    if out is None:
        if continue_sum:
            raise ValueError("continue_sum needs the partial sum in `out`")
        out = torch.empty(n, dtype=torch.float32, device=dev)
    _require_cuda_f32(out, "out")
    arr = (L.PacketView * len(packets))(*[p.view(float(w)) for p, w in zip(packets, weights)])
    views = torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(dev)
    L.check(lib.fc_qsgd_decode_accumulate(_vp(views), len(packets), n, _vp(out),
                                          int(continue_sum), _stream(dev)),
            "fc_qsgd_decode_accumulate")
    return out


def qsgd_wire_bytes(n: int, bits: int) -> int:
    """The size of a QSGD packet's wire form: 128 + 4 (fc_qsgd_code_words(n, bits) rounded up to a
    multiple of 4); ``ValueError`` for bits outside [1, 14]."""
    total = int(L.load().fc_qsgd_wire_bytes(n, bits))
    if total == 0:
        raise ValueError(f"bits={bits} outside [1, 14]")
    return total


def pack_qsgd(packet: QsgdPacket) -> torch.Tensor:
    """The wire form of a QSGD packet as a device uint8 tensor (include/fedcodec.h): the 32 fixed
    bytes, the device header, the codes and the zero pad words: copies only, no kernel, no
    synchronisation."""
    if not isinstance(packet, QsgdPacket):
        raise TypeError("a QSGD packet expected (codec.encode_qsgd, codec.qsgd_from_host)")
    words = int(L.load().fc_qsgd_code_words(packet.n, packet.bits))
    total = qsgd_wire_bytes(packet.n, packet.bits)
    if packet.codes.numel() < words:
        raise ValueError("the packet's codes are shorter than fc_qsgd_code_words(n, bits)")
    return _pack_fixed(QSGD.magic, packet.hdr, packet.codes[:words], total)


def is_qsgd_payload(data) -> bool:
    """Do these host bytes start with the QSGD packet's magic?"""
    return kind_of(data) is QSGD


def qsgd_from_host(data, n: Optional[int] = None, device=None) -> QsgdPacket:
    """Host bytes as a :class:`QsgdPacket` on ``device``: ALWAYS through ``fc_qsgd_wire_validate``
    first (``ValueError`` with the library's reason; no device work has started then), then one
    H2D copy.  ``n``: the length the packet must have."""
    return QSGD.upload(*QSGD.check(data, n), device)


# ---- NumPy's legacy MT19937 stream on the device (the reference's dropout draws) -------------
class MtPlan:
    """The jump polynomials of gradient length n on one device (fc_mt_plan), for up to
    ``rows`` rows per round; kept per (device, n) and grown on demand."""

    _cache: dict = {}
    _lock = threading.Lock()

    def __init__(self, n: int, rows: int, device: torch.device):
        lib = L.load()
        self.n, self.rows = n, rows
        self.nbytes = int(lib.fc_mt_plan_bytes(n, rows))
        self.buf = torch.empty(self.nbytes, dtype=torch.uint8, device=device)
        L.check(lib.fc_mt_plan(n, rows, _vp(self.buf), self.nbytes, _stream(device)), "fc_mt_plan")

    @classmethod
    def get(cls, n: int, rows: int, device: torch.device) -> "MtPlan":
        key = (device.index if device.index is not None else torch.cuda.current_device(), n)
        with cls._lock:
            p = cls._cache.get(key)
            if p is None or p.rows < rows:
                p = cls(n, max(rows, 2 * p.rows if p is not None else rows), device)
                cls._cache[key] = p
            return p


class MtRound:
    """``rows`` consecutive ``np.random.binomial(1, p_r, (n,))`` draws (compression.py:51, :58)
    generated on the device from the legacy state (key, pos) of ``np.random.get_state()``
    (fc_mt_begin / fc_mt_binomial): row r's mask words equal the host draw's
    ``bitmask_words(mask, n, True)``.  :meth:`end_state` gives the state np.random is left in
    (and whether NumPy would have redrawn somewhere: the caller then draws on the host)."""

    def __init__(self, n: int, rows: int, key: np.ndarray, pos: int,
                 device: Optional[torch.device] = None):
        dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        lib = L.load()
        self.n, self.rows, self.dev = n, rows, dev
        self.plan = MtPlan.get(n, rows, dev)
        self.nbytes = int(lib.fc_mt_workspace_bytes(rows))
        self.ws = torch.empty(self.nbytes, dtype=torch.uint8, device=dev)
        self._key = np.ascontiguousarray(np.asarray(key, dtype=np.uint32))
        if self._key.shape != (624,):
            raise ValueError("an MT19937 key has 624 words")
        with torch.cuda.device(dev):
            L.check(lib.fc_mt_begin(_vp(self.plan.buf), self.plan.nbytes, n, rows,
                                    self._key.ctypes.data_as(ctypes.c_void_p), int(pos),
                                    _vp(self.ws), self.nbytes, _stream(dev)), "fc_mt_begin")
        self._events = []                   # after begin and each row: end_state() waits on them
        self._mark()
        self._begin = (self._events[0], torch.cuda.current_stream(dev))

    def _mark(self) -> None:
        ev = torch.cuda.Event()
        ev.record(torch.cuda.current_stream(self.dev))
        self._events.append(ev)
        if len(self._events) > 8:
            self._events = [e for e in self._events if not e.query()] or self._events[-1:]

    def binomial(self, row: int, p: float, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Row ``row``'s mask as int32 bit words (ceil(n/32)) on the current stream."""
        if out is None:
            out = torch.empty((self.n + 31) // 32, dtype=torch.int32, device=self.dev)
        cur = torch.cuda.current_stream(self.dev)
        if cur != self._begin[1]:           # rows may be drawn on other streams (DeviceRing)
            cur.wait_event(self._begin[0])
        lib = L.load()
        L.check(lib.fc_mt_binomial(_vp(self.plan.buf), self.plan.nbytes, self.n, self.rows, int(row),
                                   float(p), _vp(out), _vp(self.ws), self.nbytes,
                                   _stream(self.dev)), "fc_mt_binomial")
        self._mark()
        return out

    def end_state(self):
        """(key uint32[624], pos, redraw) after the round: waits for begin and every row
        launched so far (the redraw flag covers those rows)."""
        for ev in self._events:
            ev.synchronize()
        raw = self.ws[:624 * 4 + 16].cpu().numpy()
        words = raw.view(np.uint32)
        return words[:624].copy(), int(words[624]), bool(words[625])


def mt_state():
    """np.random's legacy state as (key, pos, has_gauss, gauss); ValueError if not MT19937."""
    st = np.random.get_state()
    if st[0] != "MT19937":
        raise ValueError("np.random is not an MT19937 RandomState")
    return np.asarray(st[1], dtype=np.uint32), int(st[2]), int(st[3]), float(st[4])


def mt_set_state(key: np.ndarray, pos: int, has_gauss: int, gauss: float) -> None:
    np.random.set_state(("MT19937", np.asarray(key, dtype=np.uint32), int(pos), int(has_gauss),
                         float(gauss)))


# ---- np.random.permutation on the device (the reference's 'rand' draws) ------------------------
class PermPlan:
    """The segment jump polynomials of length n on one device (fc_mt_perm_plan), kept per
    (device, n)."""

    _cache: dict = {}
    _lock = threading.Lock()

    def __init__(self, n: int, device: torch.device):
        lib = L.load()
        self.n = n
        self.nbytes = int(lib.fc_mt_perm_plan_bytes(n))
        if self.nbytes == 0:
            raise ValueError(f"n={n} outside [0, 2^31)")
        self.ws_bytes = int(lib.fc_mt_perm_workspace_bytes(n))
        self.buf = torch.empty(self.nbytes, dtype=torch.uint8, device=device)
        with torch.cuda.device(device):
            L.check(lib.fc_mt_perm_plan(n, _vp(self.buf), self.nbytes, _stream(device)),
                    "fc_mt_perm_plan")

    @classmethod
    def get(cls, n: int, device: torch.device) -> "PermPlan":
        key = (device.index if device.index is not None else torch.cuda.current_device(), n)
        with cls._lock:
            p = cls._cache.get(key)
            if p is None:
                p = cls._cache[key] = cls(n, device)
            return p


class PermRound:
    """Consecutive ``np.random.permutation(n)[:k]`` draws (compression.py:43) made on the device
    from the legacy state (key, pos) of ``np.random.get_state()`` (fc_mt_perm_begin /
    fc_mt_permutation).  The state lives in a device block that every call updates in place:
    calls chain in the order they are made, with no host read between them.  :meth:`end_state`
    gives the state np.random is left in and the fallback word (non-zero: a call ran out of its
    word budget or a loop bound; key and pos are then those before that call, the calls from it
    on drew nothing and the caller draws on the host instead)."""

    STATE_BYTES = 2520
    #: the word budget of a call made with ``max_words=0`` (0: the library's 2n + 4096)
    max_words = 0

    def __init__(self, n: int, key: np.ndarray, pos: int, device: Optional[torch.device] = None):
        dev = device if device is not None else torch.device("cuda", torch.cuda.current_device())
        lib = L.load()
        self.n, self.dev = int(n), dev
        self.plan = PermPlan.get(self.n, dev)
        self.nbytes = self.plan.ws_bytes
        self.ws = torch.empty(self.nbytes, dtype=torch.uint8, device=dev)
        self.state = torch.empty(self.STATE_BYTES, dtype=torch.uint8, device=dev)
        self._key = np.ascontiguousarray(np.asarray(key, dtype=np.uint32))
        if self._key.shape != (624,):
            raise ValueError("an MT19937 key has 624 words")
        self._lock = threading.Lock()
        self._home = torch.cuda.current_stream(dev)      # the stream the buffers belong to
        with torch.cuda.device(dev):
            L.check(lib.fc_mt_perm_begin(self._key.ctypes.data_as(ctypes.c_void_p), int(pos),
                                         _vp(self.state), _stream(dev)), "fc_mt_perm_begin")
        self._last = (self._event(self._home), self._home)

    def _event(self, stream) -> torch.cuda.Event:
        ev = torch.cuda.Event()
        ev.record(stream)
        return ev

    def permutation(self, k: int, out_idx: Optional[torch.Tensor] = None,
                    out_mask: Optional[torch.Tensor] = None, max_words: int = 0):
        """The next ``np.random.permutation(n)[:k]`` on the current stream -> (idx, mask):
        ``idx`` int32[k] (the uint32 indices, in NumPy's order) and ``mask`` int32 bit words
        (ceil(n/32), = ``bitmask_words(idx, n, False)``).  With only one of ``out_idx`` /
        ``out_mask`` given only that output is made (the other is None); with neither, both
        are allocated."""
        n, k = self.n, int(k)
        if not 0 <= k <= n:
            raise ValueError(f"k={k} outside [0, n={n}]")
        if out_idx is None and out_mask is None:
            out_idx = torch.empty(k, dtype=torch.int32, device=self.dev)
            out_mask = torch.empty((n + 31) // 32, dtype=torch.int32, device=self.dev)
        for t, size, name in ((out_idx, k, "out_idx"), (out_mask, (n + 31) // 32, "out_mask")):
            if t is not None and (t.dtype != _U32 or not t.is_cuda or not t.is_contiguous()
                                  or t.numel() < size):
                raise ValueError(f"{name} must be a contiguous int32 CUDA tensor of {size} words")
        if n == 0:
            return out_idx, out_mask
        if out_mask is None and k == 0:                  # nothing to write, the draw still runs
            out_mask = torch.empty((n + 31) // 32, dtype=torch.int32, device=self.dev)
        lib = L.load()
        cur = torch.cuda.current_stream(self.dev)
        with self._lock:
            ev, last = self._last
            if cur != last:                              # the state chains across streams
                cur.wait_event(ev)
            if cur != self._home:
                for t in (self.ws, self.state, self.plan.buf):
                    t.record_stream(cur)
            with torch.cuda.device(self.dev):
                L.check(lib.fc_mt_permutation(_vp(self.plan.buf), self.plan.nbytes, n, k,
                                              int(max_words or self.max_words), _vp(self.state),
                                              _vp(out_idx if k else None), _vp(out_mask),
                                              _vp(self.ws), self.nbytes, _stream(self.dev)),
                        "fc_mt_permutation")
            self._last = (self._event(cur), cur)
        return out_idx, out_mask

    def end_state(self):
        """(key uint32[624], pos, fallback, consumed) after the calls made so far
        (synchronises with the last of them)."""
        with self._lock:
            ev = self._last[0]
        ev.synchronize()
        raw = self.state.cpu().numpy()
        words = raw[:2512].view(np.uint32)
        return (words[:624].copy(), int(words[624]), int(words[625]),
                int(raw[2512:2520].view(np.uint64)[0]))

    def rows_done(self) -> int:
        """Calls that completed (synchronises)."""
        with self._lock:
            ev = self._last[0]
        ev.synchronize()
        return int(self.state[2504:2508].cpu().numpy().view(np.uint32)[0])
