"""Drop-in ``Aggregator.aggregate_grads`` (ftl/gradient_aggregation/aggregation.py:19-93) on MI355X.

The reference builds the dense host matrix ``G`` (M x N) row by row from
``client.C.compress(client.grad)`` (aggregation.py:61-63), optionally merges client clusters
(``__merge_gradient``, aggregation.py:80-93, ``num_hierarchies > 0``) and reduces it with the
GAR (gar.py:44).  Here a round takes one route, named by ``agg_path`` afterwards; on all but
"dense" the rows never become a dense matrix.  Every result is bit-exact against the reference
(tests/golden/make_golden_agg.py pins the merge and the sign-of-zero semantics;
tests/test_gpu_parity.py runs both paths), and routes that share clients give the same bits.

``aggregate_grads(clients)``: :func:`round_route` decides on the host, before a GPU is touched, in
the order of the first five rows; the rest is the tail of ``aggregate_grads``.
``aggregate_wire(payloads)`` takes the clients' wire packets (``Compression.compress_wire``;
include/fedcodec.h) instead, validated on the host: the "wire*" rows, each the bits of the row it
names on the same clients.  A round that a scheme or a key claims but whose conditions fail raises
``NotImplementedError`` naming the condition (no silent dense fallback).  "Packet round" below: no
hierarchies, one device, float32 or no GAR weights, 1-D float32 gradients (payloads) of one length.

================  ================================================  ====================  ====================================
``agg_path``      conditions                                        opt-in key            resident on the device
================  ================================================  ====================  ====================================
"sign-gram"       packet round, n > 0, all clients the drop-in      ``sign_geometry``     M sign packets (N/8 bytes each),
                  'sign', M <= 128; krum, spectral_gram,                                  Gram and dot workspaces, 8 M^2
                  geometric_median, centered_clip or fed_avg with                         (:func:`sign_gram_resident_bytes`)
                  ``pc_analysis: "gram"``
"sign-trim"       the same clients; trimmed_mean or                 ``sign_trim``         M sign packets, trim workspace
                  coordinate_median, unweighted                                           (:func:`sign_trim_resident_bytes`)
"gram"            packet round, all clients 'top' without error     the scheme (krum,     M gradients and their 'top' packets,
                  feedback at one fraction with 0 < k < n,          the linear and trim   encode, Gram, dot (and trim)
                  M <= 128 (:func:`gram_wanted`,                    rules), or            workspaces, 8 M^2
                  :func:`gram_route_k`)                             ``pc_analysis:        (:func:`gram_resident_bytes`)
                                                                    "gram"``
"sign"            the "sign-gram" clients; fed_avg (a round         on; off with          fed_avg: a group of sign packets
                  outside the conditions goes on down this          ``sign_packets:       sized by the budget;
                  table) or sign_majority (it is refused,           False`` (fed_avg)     sign_majority: all M
                  unweighted) (:func:`sign_route`)
"qsgd"            packet round, n > 0, fed_avg, all clients the     ``qsgd_packets``      a group of QSGD packets (N W / 8
                  drop-in native 'qsgd' with num_bits in [1, 14]                          bytes each, W = 4 / 8 / 16) sized by
                  (they may differ in bits), with or without error                        the budget, one gradient in flight
                  feedback (:func:`qsgd_route`; a round outside the
                  conditions goes on down this table)
"ef-batch"        packet round, fed_avg, all clients the drop-in    ``batched_error_      groups of <= 64 gradients, residuals
                  'top' with error feedback at one fraction with    feedback``            and packets (:func:`ef_batch_group`)
                  0 < k < n (:func:`ef_batch_k`)
"stream"          a device GAR, float32 gradients and weights,      -                     a bounded ring of gradients and a
                  n > 0, every codec 'full', 'top', 'rand' or                             group of packets per device
                  'dropout-*' without state (:func:`row_plan`);                           (``devices``), within
                  with hierarchies the merged rows go to the GAR                          ``device_budget_bytes``
"dense-fold"      anything else under a device GAR without          -                     one row (:func:`fold_rows`)
                  hierarchies: 'qsgd', error feedback, float64
                  gradients or weights, a codec the reference
                  rejects (it raises at the same row)
"dense"           anything else: hierarchies over such rows, or a   -                     G (M x N)
                  reference GAR (:func:`integration.install`)
"wire"            packet round of 'top' payloads; fed_avg           -                     a group's wire bytes and slotted
                  ("stream"), any M in groups, or a scheme of                             packets; the "gram" schemes: all M
                  "gram", M <= 128                                                        (:func:`wire_resident_bytes`)
"wire-fold"       the same under fed_avg, no slotted packets        ``wire_fold``         a group's wire bytes
                                                                                          (:func:`wire_fold_groups`)
"wire-sign"       packet round of sign payloads; fed_avg in         -                     a group's sign packets;
                  groups or sign_majority ("sign")                                        sign_majority: all M
"wire-sign-gram"  the same, M <= 128, the schemes of "sign-gram"    ``sign_geometry``     as "sign-gram"
"wire-sign-trim"  the same, M <= 128, the schemes of "sign-trim"    ``sign_trim``         as "sign-trim"
"wire-qsgd"       packet round of QSGD payloads; fed_avg in         -                     a group's QSGD packets
                  groups ("qsgd")                                                         (:func:`wire_fold_groups`)
================  ================================================  ====================  ====================================

* ``batched_sign_encode`` (opt-in) names no route: on "sign", "sign-gram" and "sign-trim" it uploads
  the clients in sub-batches (:func:`sign_encode_group`) and encodes those without error feedback
  in one ``codec.encode_sign_batch`` call per sub-batch (:func:`_sign_encode_batched`); the bits,
  the residuals and ``agg_path`` are those of the round without it.
* "stream": the host gradients go through the ring (openmsftl_amd/pipeline.py): H2D, each row made
  on the device (top-k packets, mask packets whose masks are np.random's own draws in row order,
  made on the host or, :data:`DEVICE_MT` / :data:`DEVICE_PERM`, on the device, or the dense
  gradient), every group folded in row order (bit-exact ``np.sum(G * w[:, None], axis=0)``).
  ``aggregation_config["devices"]`` fans the groups out round-robin over several GPUs, the running
  sum hopping between them in group order.  With hierarchies each first-stage cluster mean is the
  streamed fold with weights 1 divided once by the row count; later stages do the same over the
  dense merged rows (:func:`merge_streamed`, :func:`merge_stages`).
* "gram", "sign-gram", "sign-trim" and their wire rows: all of the round's packets resident, then
  :func:`_gram_family`: the M x M float64 Gram matrix straight from the packets
  (``codec.gram`` / ``codec.gram_sign``) and Krum's selection, a linear rule's coefficients and
  fold, or the FedAVG fold ("stream"'s bits); a trim rule runs one kernel over the packets
  (``codec.trimmed_mean`` / ``codec.trimmed_mean_sign``) and needs no Gram matrix.  With
  ``pc_analysis: "gram"`` the singular values of G, ``sqrt(max(eigvalsh(gram), 0))`` descending,
  are appended to ``gar.Sigma_tracked``; unlike the reference's ``randomized_svd`` this draws
  nothing from ``np.random``.  ``pc_analysis: True`` and ``"fed_spectral_avg"`` keep raising.

``aggregate_grads`` is a plain function so that :func:`openmsftl_amd.integration.install` can
bind it onto the REFERENCE ``Aggregator`` class (its ``self.gar`` may then be a reference GAR
with no ``aggregate_packets``: G is then handed over as the host array the reference builds).
Out of the hot path and not rebuilt: ``pc_analysis`` (randomized SVD of G), ``SpectralFedAvg``,
``update_model`` and the RL / DGA aggregators: the device class raises
``NotImplementedError`` for them, the patched reference class keeps its own code for
``pc_analysis``.
"""
from __future__ import annotations

from typing import Dict, List, Optional

import numpy as np
import torch

from . import _lib as L
from . import codec
from .compression import Compression, bitmask_words, kept_count
from .gar import (CenteredClip, CoordinateMedian, CoordinateTrim, FedAvg, GeometricMedian, Krum,
                  LinearRule, SignMajority, SpectralGram, TrimmedMean, gram_singular_values)
from .pipeline import HostFedAvg, MtRedraw, RowCodec, RowPlan


def _cluster_bounds(m: int, cluster_size: int):
    """aggregation.py:82-87: consecutive clusters, the last one absorbs the remainder."""
    num = m // cluster_size
    assert num > 0, "Too small cluter size: {} // {} == 0".format(m, cluster_size)
    bounds = [[i * cluster_size, (i + 1) * cluster_size] for i in range(num)]
    if bounds[-1][1] < m:
        bounds[-1][1] = m
    return bounds


def _merge_log(stage: int, cluster_size: int, bounds) -> None:
    """The reference's progress lines for one merge stage (aggregation.py:71, 88, 90), text and
    order included."""
    print("{}-stage gradient aggregation: cluster size={}".format(stage, cluster_size))
    print("#client clusters: {}".format(len(bounds)))
    for s, e in bounds:
        print("Averaging gradient from the {}-th client to the {}=th".format(s, e))


def _device_of(agg) -> torch.device:
    dev = getattr(agg, "device", None)
    if isinstance(dev, torch.device) and dev.type == "cuda":
        return dev
    return torch.device("cuda", torch.cuda.current_device())


#: default for aggregation_config["devices"] (``integration.install(devices=...)`` sets it):
#: None = the current device only; "all" = every visible GPU of this process
DEFAULT_DEVICES = None


def stream_devices(agg) -> List[torch.device]:
    """The GPUs the streamed path fans out over (one process, one pipeline each):
    ``aggregation_config["devices"]`` = "all" (every visible GPU), a count (the first n) or a
    list of device indices (repeats allowed: tests stand two pipelines on one GPU in for two
    GPUs); absent -> :data:`DEFAULT_DEVICES` (None: the current device).  An aggregator
    constructed with an explicit ``device`` and no ``devices`` key stays on that device."""
    spec = _config(agg).get("devices")
    if spec is None:
        if isinstance(getattr(agg, "device", None), torch.device):
            return [_device_of(agg)]
        spec = DEFAULT_DEVICES
    if spec is None or spec == 1:
        return [_device_of(agg)]
    if spec == "all":
        count = torch.cuda.device_count()
        if count <= 1:
            return [_device_of(agg)]
        return [torch.device("cuda", i) for i in range(count)]
    if isinstance(spec, int):
        if not 1 <= spec <= torch.cuda.device_count():
            raise ValueError(f"devices={spec}: {torch.cuda.device_count()} visible GPU(s)")
        return [torch.device("cuda", i) for i in range(spec)]
    devs = [torch.device("cuda", int(i)) for i in spec]
    if not devs:
        raise ValueError("devices: empty list")
    return devs


def common_top_fraction(clients) -> Optional[float]:
    """The fraction when every client compresses with 'top' at one fraction whose k lies in
    [0, N] (f < 0 / f > 1 keep the reference's slice semantics: generic path), else None."""
    fr = None
    for c in clients:
        C = c.C
        if getattr(C, "compression_function", None) != "top":
            return None
        if getattr(C, "error_feedback", False):      # stateful: only compress() may run it
            return None
        f = C.fraction_coordinates
        if fr is None:
            fr = f
        elif f != fr:
            return None
    n = len(clients[0].grad)
    return fr if 0 <= kept_count(fr, n) <= n else None


_STREAMED = ("full", "top", "rand", "dropout-biased", "dropout-unbiased")


def _streamable(C, n: int) -> bool:
    """Can this client's codec stream (its row made on the device exactly as compress()
    would make it)?  Anything else — 'qsgd', unknown names, an RNG mode or p the drop-in
    would reject — takes the generic path, which raises where the reference raises."""
    fn = getattr(C, "compression_function", None)
    if fn not in _STREAMED:
        return False
    if fn == "full":
        return True
    if getattr(C, "error_feedback", False):
        # a codec with state (the 'top' residual): the streamed paths re-run rows (MtRedraw) and
        # must never see it; the generic path calls compress() exactly once per row, in row order
        return False
    rng = getattr(C, "rng", "numpy")           # a reference Compression draws from np.random
    if rng not in ("numpy", "philox"):
        return False
    if fn in ("top", "rand"):
        f = getattr(C, "fraction_coordinates", None)
        return isinstance(f, (int, float, np.floating, np.integer)) and np.isfinite(f)
    p = getattr(C, "dropout_p", None)
    if not isinstance(p, (int, float, np.floating, np.integer)):
        return False
    return rng == "numpy" or 0.0 <= p <= 1.0


#: draw the reference's np.random dropout masks on the device (np.random's MT19937 stream by
#: jump-ahead, openmsftl_amd/csrc/fc_mt.hip) instead of on the host producer thread
DEVICE_MT = True


def _device_mt_ok(clients) -> bool:
    """Can the round's np.random draws be made on the device?  Only if every host-RNG row is a
    dropout row with p in [0, 1]: 'rand' (np.random.permutation) consumes a data-dependent
    number of draws, and an invalid p must raise at its row (the host path does)."""
    for c in clients:
        C = c.C
        fn = C.compression_function
        if getattr(C, "rng", "numpy") != "numpy":
            continue
        if fn == "rand":
            return False
        if fn in ("dropout-biased", "dropout-unbiased"):
            try:
                p = float(C.dropout_p)
            except (TypeError, ValueError):
                return False
            if not 0.0 <= p <= 1.0:
                return False
    return True


#: draw the reference's np.random.permutation rows on the device (openmsftl_amd/csrc/fc_perm.hip)
#: instead of on the host producer thread.  Opt-in: the default of
#: aggregation_config["device_permutation"] and of :func:`row_plan`'s ``device_perm``
DEVICE_PERM = False


def _device_perm_ok(clients, n: int) -> bool:
    """Can the round's np.random draws be permutations made on the device?  Only if every
    host-RNG row is a 'rand' row (a numpy dropout row in the same round keeps today's host
    plan: the two kinds of draw share one stream) and there is something to draw."""
    rand_rows = 0
    for c in clients:
        C = c.C
        fn = C.compression_function
        if getattr(C, "rng", "numpy") != "numpy":
            continue
        if fn in ("dropout-biased", "dropout-unbiased"):
            return False
        rand_rows += fn == "rand"
    return rand_rows > 0 and 2 <= n < 2 ** 31


def row_plan(clients, n: int, device_mt: Optional[bool] = None,
             device_perm: Optional[bool] = None) -> Optional[RowPlan]:
    """The streamed round's :class:`~openmsftl_amd.pipeline.RowPlan` (aggregation.py:61-63:
    row ix = compress(clients[ix].grad)), or None when some client's codec cannot stream.

    * 'full' -> the gradient itself (a dense row); 'top' -> a top-k packet (k = n: the
      gradient itself; k = 0: nothing kept);
    * 'rand' -> with ``np.random`` (the reference, and the drop-in default) a host mask from
      ``np.random.permutation(n)[:k]`` (compression.py:43); native Philox -> Philox-key top-k;
    * 'dropout-*' -> a host mask from ``np.random.binomial(1, p, (n,))`` (:51/:58), or device
      Bernoulli(p) (Philox); the unbiased 1/p scaling is applied by the fold
      (fl32(fl64(g) / p), compression.py:59-60 then the cast into G, aggregation.py:63).
    Host draws run in row order on the plan's producer thread, exactly the reference's
    consumption of the global RNG; Philox offsets are taken in row order too.  With
    ``device_mt`` (default :data:`DEVICE_MT`) and no host permutation in the round, the dropout
    masks are np.random's own draws made on the device instead (mask_src "mt": row r of the
    round's MtRound, from np.random's state now; :meth:`RowPlan.close` sets the state after).
    With ``device_perm`` (default :data:`DEVICE_PERM`, off) and no numpy dropout row in the
    round, its 'rand' rows are np.random.permutation's own draws made on the device (mask_src
    "perm": draw ``offset`` of the round's PermRound, in row order on one device)."""
    if not all(_streamable(c.C, n) for c in clients):
        return None
    use_mt = (DEVICE_MT if device_mt is None else device_mt) and _device_mt_ok(clients)
    use_perm = (DEVICE_PERM if device_perm is None else device_perm) and _device_perm_ok(clients, n)
    mt_rows = perm_rows = 0
    specs, draws = [], {}
    for i, c in enumerate(clients):
        C = c.C
        fn = C.compression_function
        if fn == "full":
            specs.append(RowCodec("dense"))
            continue
        rng = getattr(C, "rng", "numpy")
        if fn in ("top", "rand"):
            k = kept_count(C.fraction_coordinates, n)
            if fn == "rand" and rng == "numpy" and use_perm:
                specs.append(RowCodec("mask", codec=L.FC_CODEC_RAND, mask_src="perm", k=k,
                                      offset=perm_rows))
                perm_rows += 1
                continue
            if fn == "rand" and rng == "numpy":
                specs.append(RowCodec("mask", codec=L.FC_CODEC_RAND, mask_src="host"))
                draws[i] = (lambda k=k: bitmask_words(np.random.permutation(n)[:k], n, False))
                continue
            key_mode, seed, off = L.FC_KEY_MAGNITUDE, 0, 0
            if fn == "rand":
                key_mode, seed, off = L.FC_KEY_PHILOX, C.seed, C._next_offset()
            if k == n:
                specs.append(RowCodec("dense"))
            elif k == 0:
                specs.append(RowCodec("mask", codec=L.FC_CODEC_RAND, mask_src="none"))
            else:
                specs.append(RowCodec("top", k=k, key_mode=key_mode, seed=seed, offset=off))
            continue
        cid = L.FC_CODEC_DROPOUT_BIASED if fn == "dropout-biased" else L.FC_CODEC_DROPOUT_UNBIASED
        p = float(C.dropout_p)
        if rng == "numpy" and use_mt:
            specs.append(RowCodec("mask", codec=cid, p=p, mask_src="mt", offset=mt_rows))
            mt_rows += 1
        elif rng == "numpy":
            specs.append(RowCodec("mask", codec=cid, p=p, mask_src="host"))
            draws[i] = (lambda p=C.dropout_p: bitmask_words(np.random.binomial(1, p, (n,)), n, True))
        else:
            specs.append(RowCodec("mask", codec=cid, p=p, mask_src="philox", seed=C.seed,
                                  offset=C._next_offset()))
    return RowPlan(n, specs, draws, mt_rows=mt_rows, perm_rows=perm_rows)


#: device bytes the streamed path may hold (gradient ring + packets + aggregates);
#: aggregation_config["device_budget_bytes"] overrides, default a quarter of the free HBM
DEFAULT_BUDGET_FRACTION = 0.25


def _budget(agg, dev: torch.device) -> int:
    b = agg.aggregation_config.get("device_budget_bytes") if hasattr(agg, "aggregation_config") else None
    if b:
        return int(b)
    free, _ = torch.cuda.mem_get_info(dev)
    return int(free * DEFAULT_BUDGET_FRACTION)


def _stream_pipeline(agg, n: int, m: int, devs: List[torch.device]):
    """The aggregator's cached streaming pipeline for length n on ``devs``: one HostFedAvg, or
    a DeviceRing of one HostFedAvg (two packet sets) per device; fold groups sized for the
    per-device budget."""
    from .pipeline import DeviceRing, HostFedAvg, plan_group
    cache = agg.__dict__.setdefault("_host_pipelines", {})
    sets = 1 if len(devs) == 1 else 2
    group = min(plan_group(n, m, _budget(agg, d), sets=sets) for d in devs)
    key = (n, tuple(d.index for d in devs))
    pipe = cache.get(key)
    if pipe is None or pipe.group < group:
        cache.clear()                       # one shape at a time: release the old buffers
        torch.cuda.empty_cache()
        if len(devs) == 1:
            pipe = HostFedAvg(n, group=group, device=devs[0])
        else:
            pipe = DeviceRing([HostFedAvg(n, group=group, device=d, sets=2) for d in devs])
        cache[key] = pipe
    return pipe


def stream_fold(agg, clients, n: int, plan: RowPlan, weights: np.ndarray, dev: torch.device,
                out: Optional[torch.Tensor] = None) -> torch.Tensor:
    """FedAVG of the clients' rows (aggregation.py:61-63 + gar.py:44) streamed from their host
    ``client.grad`` through a bounded H2D ring, each row made on the device as ``plan`` says
    and every group folded in row order (openmsftl_amd/pipeline.py): device memory stays within
    the budget for any client count.  With several devices (:func:`stream_devices`) the
    groups go round-robin to one pipeline per GPU and the running aggregate hops between them
    in group order (pipeline.DeviceRing): the same bits, every GPU's PCIe link busy.  Returns
    the device aggregate (``out`` if given, else on the device that folded the last group)."""
    w = np.asarray(weights, np.float32)
    devs = stream_devices(agg)
    pipe = _stream_pipeline(agg, n, len(clients), devs)
    get = lambda i: clients[i].grad         # noqa: E731
    if isinstance(pipe, HostFedAvg) and (out is None or out.device == pipe.dev):
        return pipe.run(get, len(clients), w, out=out, to_host=False, plan=plan)
    acc = pipe.run(get, len(clients), w, to_host=False, plan=plan)
    if out is None:
        return acc
    out.copy_(acc)
    return out


def merge_streamed(agg, clients, n: int, plan: RowPlan, cluster_size: int,
                   dev: torch.device) -> torch.Tensor:
    """First merge stage straight from the streamed rows (aggregation.py:80-93): each
    cluster's +0-started row-order sum (weights 1), then one fl32 division by its size."""
    bounds = _cluster_bounds(len(clients), cluster_size)
    _merge_log(0, cluster_size, bounds)
    H = torch.empty((len(bounds), n), dtype=torch.float32, device=dev)
    for r, (s, e) in enumerate(bounds):
        row = torch.empty(n, dtype=torch.float32, device=dev)   # 16-B aligned while written
        stream_fold(agg, clients[s:e], n, plan.shifted(s), np.ones(e - s, np.float32), dev, out=row)
        H[r].copy_(codec.div_scalar(row, float(e - s)))
    return H


def merge_stages(G: torch.Tensor, sizes, first_stage: int = 0) -> torch.Tensor:
    """Merge stages over dense device rows (fp32 or fp64 G): +0-started sums (weights 1),
    then / count, in G's dtype (np.mean(G[s:e], axis=0), aggregation.py:91)."""
    for i, cs in enumerate(sizes):
        bounds = _cluster_bounds(G.shape[0], cs)
        _merge_log(first_stage + i, cs, bounds)
        rows = []
        for s, e in bounds:
            r = codec.weighted_sum_dense(G[s:e], torch.ones(e - s, dtype=G.dtype), out_dtype=G.dtype)
            rows.append(codec.div_scalar(r, float(e - s)))
        G = torch.stack(rows)
    return G


def _client_row(C, grad, dev: torch.device):
    """``C.compress(grad)`` (aggregation.py:63) as a device tensor: the drop-in Compression
    gets the gradient on the device (no D2H of its result); another codec object gets the host
    array it expects and its result is copied up."""
    if isinstance(C, Compression) and not isinstance(grad, torch.Tensor):
        a = np.asarray(grad)
        if a.dtype in (np.float32, np.float64) and a.ndim == 1:
            grad = torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    q = C.compress(grad)
    if not isinstance(q, torch.Tensor):
        q = torch.from_numpy(np.ascontiguousarray(q))
    return q


def fold_rows(gar, clients, n: int, tdt: torch.dtype, dev: torch.device) -> torch.Tensor:
    """gar.py:44 over the rows aggregation.py:61-63 would stack, folded one row at a time as
    each client's codec makes it (same NumPy RNG draws, same order; each row cast to G's dtype
    ``tdt`` first, as ``G[ix, :] = q`` does): the +0-started row-order sum in NumPy's promoted
    dtype of G and the GAR's (persisted) weights, without the M x N matrix."""
    gdt = np.float64 if tdt == torch.float64 else np.float32
    w = gar._weights(len(clients), gdt)
    odt = torch.float64 if np.result_type(gdt, w.dtype) == np.float64 else torch.float32
    wt = torch.from_numpy(np.ascontiguousarray(w))
    acc = torch.empty(n, dtype=odt, device=dev)
    row = torch.empty(n, dtype=tdt, device=dev)
    for ix, c in enumerate(clients):
        row.copy_(_client_row(c.C, c.grad, dev))        # G[ix, :] = q (cast to G's dtype)
        codec.weighted_sum_dense([row], wt[ix:ix + 1], out=acc, out_dtype=odt,
                                 continue_sum=ix > 0)
    return acc


# ---- the round conditions, each written once ---------------------------------------------------
# Every check takes ``no``, the function that refuses: a route's own ``_needs(prefix)`` (a
# ``NotImplementedError`` naming the route and the condition), or ``_refused`` where the caller
# answers None / False instead (ef_batch_k, sign_route under fed_avg).
class _Refused(Exception):
    """A round condition that does not hold: only the ``why`` text."""


def _refused(why: str):
    raise _Refused(why)


def _needs(prefix: str):
    def no(why: str):
        raise NotImplementedError(f"{prefix} needs {why}")
    return no


_gram_no = _needs("the gram route (krum / pc_analysis='gram')")
_sign_no = _needs("the sign route (sign packets: fed_avg / sign_majority)")
_sign_gram_no = _needs("the sign-gram route (sign_geometry)")
_sign_trim_no = _needs("the sign-trim route (sign_trim)")
_wire_no = _needs("aggregate_wire")
_qsgd_no = _needs("the qsgd route (qsgd_packets)")


def _config(agg) -> dict:
    return getattr(agg, "aggregation_config", None) or {}


def _no_hierarchies(agg, no) -> None:
    if agg.num_hierarchies != 0:
        no("no hierarchies (num_hierarchies == 0)")


def _one_device(agg, no) -> None:
    if _config(agg).get("devices", DEFAULT_DEVICES) not in (None, 1):
        no("one device")


def _f32_weights(gar, no) -> None:
    w = getattr(gar, "gradient_weights", None)
    if w is not None and np.asarray(w).dtype != np.float32:
        no("float32 GAR weights")


def _drop_in(clients, no) -> None:
    if not all(isinstance(c.C, Compression) for c in clients):
        no("every client to be the drop-in Compression")


def _grad_length(c, n: Optional[int], no) -> int:
    """This client's gradient length; ``n`` is the length of the clients before it."""
    g = np.asarray(c.grad)
    if g.ndim != 1 or g.dtype != np.float32:
        no("1-D float32 gradients")
    if n is not None and g.shape[0] != n:
        no("gradients of one length")
    return g.shape[0]


def _at_most(m: int, what: str, no) -> None:
    if m > L.FC_GRAM_MAX_M:
        no(f"at most {L.FC_GRAM_MAX_M} {what} (got {m})")


def _top_round(clients, error_feedback: bool, no):
    """(n, k) of a round whose clients all compress with 'top', error feedback on for all or for
    none, at one finite fraction with 0 < k < n, on 1-D float32 gradients of one length."""
    n, fr = None, None
    for c in clients:
        C = c.C
        if getattr(C, "compression_function", None) != "top":
            no("every client to compress with 'top'")
        if bool(getattr(C, "error_feedback", False)) != error_feedback:
            no("'top' with error feedback" if error_feedback else "'top' without error feedback")
        n = _grad_length(c, n, no)
        f = C.fraction_coordinates
        if not isinstance(f, (int, float, np.floating, np.integer)) or not np.isfinite(f):
            no("a finite fraction_coordinates")
        if fr is not None and f != fr:
            no("one common fraction_coordinates")
        fr = f
    k = kept_count(fr, n)
    if not 0 < k < n:
        no(f"0 < k < n (k={k}, n={n})")
    return n, k


def _all_sign(clients) -> bool:
    return all(getattr(c.C, "compression_function", None) == "sign" for c in clients)


def _sign_conditions(agg, clients, no, unweighted: bool = False) -> int:
    """n of a round of 'sign' clients that may stay on the device as packets: every client the
    drop-in ``Compression``, no hierarchies, one device, float32 or no weights (``unweighted``: the
    rule's ``ValueError`` for any), 1-D float32 gradients of one length n > 0."""
    _drop_in(clients, no)
    _no_hierarchies(agg, no)
    _one_device(agg, no)
    if unweighted:
        agg.gar._unweighted()
    else:
        _f32_weights(agg.gar, no)
    n = None
    for c in clients:
        n = _grad_length(c, n, no)
    if n == 0:
        no("a gradient length n > 0")
    return n


def _fit(agg, need: int, no, dev: Optional[torch.device] = None, what: str = "packets",
         tail: str = "") -> None:
    """The budget check.  Without ``dev`` (on the host, no GPU touched) only a configured
    ``device_budget_bytes`` is compared; with it :func:`_budget`, whose default reads the free
    memory."""
    configured = _config(agg).get("device_budget_bytes")
    if dev is None and not configured:
        return
    limit = int(configured) if dev is None else _budget(agg, dev)
    if need > limit:
        no(f"the round's {what} to fit device_budget_bytes ({need} > {limit} bytes){tail}")


def _cached(agg, attr: str, key, count: int, make) -> list:
    """``count`` packets from the list ``make(count)`` made, kept at ``agg.<attr>[key]``: made
    again when absent or too short, the lists of other keys released first (one shape at a time;
    a ``"slab"`` stays)."""
    cache = agg.__dict__.setdefault(attr, {})
    packets = cache.get(key)
    if packets is None or len(packets) < count:
        for other in [k for k in cache if k != "slab"]:
            del cache[other]
        packets = cache[key] = make(count)
    return packets[:count]


def _slab_upload(agg, attr: str, upload, part, dev: torch.device) -> list:
    """Validated payloads (``(bytes, header)`` pairs) into the device slab cached at
    ``agg.<attr>["slab"]``, 256-byte aligned each, by ``upload`` (a ``codec.PayloadKind``'s): the
    packets are views of it."""
    cache = agg.__dict__.setdefault(attr, {})
    offs = np.concatenate([[0], np.cumsum([codec.slab_bytes(a.size) for a, _ in part])])
    slab = cache.get("slab")
    if slab is None or slab.device != dev or slab.numel() < int(offs[-1]):
        cache.pop("slab", None)
        slab = cache["slab"] = torch.empty(int(offs[-1]), dtype=torch.uint8, device=dev)
    return [upload(a, h, dev, out=slab[int(o): int(o) + a.size]) for (a, h), o in zip(part, offs)]


#: clients per batched error-feedback encode at most (k_compact_mag1's interleave group)
EF_BATCH_GROUP = 64


def ef_batch_k(agg, clients) -> Optional[int]:
    """k when the round may take the opt-in "ef-batch" route, else None (today's routing):
    ``aggregation_config["batched_error_feedback"]`` is set, the GAR is the device FedAvg with
    float32 (or no) weights, no hierarchies, one device, and EVERY client is the drop-in
    Compression with 'top', error feedback on and one common fraction with 0 < k < n, on 1-D
    float32 gradients of one length.  Touches no GPU."""
    if not _config(agg).get("batched_error_feedback", False) or not clients:
        return None
    if type(agg.gar) is not FedAvg:
        return None
    try:
        _no_hierarchies(agg, _refused)
        _one_device(agg, _refused)                                # multi-GPU rounds: dense-fold
        _f32_weights(agg.gar, _refused)
        _drop_in(clients, _refused)
        return _top_round(clients, True, _refused)[1]
    except _Refused:
        return None


def ef_batch_group(agg, n: int, m: int, dev: torch.device) -> int:
    """Clients per group of the "ef-batch" route: each holds its gradient and spare residual (4N
    each), a reserved packet and an encoder workspace; the aggregate (4N) is held once."""
    from .pipeline import packet_bytes
    per = 8 * n + packet_bytes(n) + int(L.load().fc_workspace_bytes(n))
    fit = (_budget(agg, dev) - 4 * n) // per
    return int(max(1, min(EF_BATCH_GROUP, m, fit)))


def ef_batch_fold(agg, clients, n: int, k: int, weights: np.ndarray, dev: torch.device) -> torch.Tensor:
    """FedAVG of the rows ``compress()`` would make for a round of error-feedback 'top' clients,
    group by group in row order: upload, ONE batched encode (codec.encode_top_ef_batch), one
    resolve, the group's packets folded into the running sum, then the group's residuals
    committed.  A client's residual advances once per round and only after its group resolved."""
    for c in clients:                         # a bad residual raises before anything advances
        c.C._ef_buffers(n, dev, allocate=False)
    m = len(clients)
    gsz = ef_batch_group(agg, n, m, dev)
    packets = _cached(agg, "_ef_batch_packets", (n, dev), gsz,
                      lambda count: codec.Packet.alloc_batch(n, count, L.FC_FMT_IDXVAL, dev, k=k))
    acc = torch.empty(n, dtype=torch.float32, device=dev)
    for gi, s in enumerate(range(0, m, gsz)):
        rows = clients[s:s + gsz]
        grads = [torch.from_numpy(np.ascontiguousarray(c.grad)).to(dev) for c in rows]
        bufs = [c.C._ef_buffers(n, dev) for c in rows]
        pk = packets[:len(rows)]
        codec.encode_top_ef_batch(grads, [b[0] for b in bufs], k,
                                  residuals_out=[b[1] for b in bufs], packets=pk, check=False)
        codec.resolve(pk)
        codec.decode_accumulate(pk, [float(x) for x in weights[s:s + len(rows)]], out=acc,
                                continue_sum=gi > 0)
        for c, (res, new) in zip(rows, bufs):
            c.C._ef_commit(res, new, True)
        for p in pk:
            p.release()
    return acc


#: the rules that are linear in the rows of G (gar.LinearRule): the "gram" route's other GARs
_LINEAR_RULES = (SpectralGram, GeometricMedian, CenteredClip)
#: the coordinate-wise rules (gar.CoordinateTrim): the same route, no Gram matrix needed
_COORD_RULES = (TrimmedMean, CoordinateMedian)


def gram_wanted(agg) -> bool:
    """Does this round take the "gram" route: the device Krum, a linear rule (spectral_gram,
    geometric_median, centered_clip), a coordinate-wise rule (trimmed_mean, coordinate_median),
    or the device FedAvg with
    ``pc_analysis: "gram"`` (a patched reference class keeps its own routing)."""
    gar = getattr(agg, "gar", None)
    if type(gar) in (Krum,) + _LINEAR_RULES + _COORD_RULES:
        return True
    pc = getattr(agg, "analyze_pc", False)
    return isinstance(pc, str) and pc == "gram" and type(gar) is FedAvg


def _trim_ws_bytes(n: int, m: int, gar) -> int:
    """The trim kernel's workspace, for a coordinate-wise rule only (0 for every other GAR)."""
    return int(L.load().fc_trim_workspace_bytes(n, m)) if isinstance(gar, CoordinateTrim) else 0


def gram_resident_bytes(n: int, m: int, gar=None) -> int:
    """Device bytes the "gram" route holds at once: m gradients and their packets, the batched
    encoder's, the Gram kernel's and the dot kernel's workspaces, the aggregate, a carried
    vector (centered_clip) and the Gram matrix; for a coordinate-wise ``gar`` (trimmed_mean,
    coordinate_median) the trim kernel's workspace too."""
    from .pipeline import packet_bytes
    lib = L.load()
    return (m * (4 * n + packet_bytes(n)) + int(lib.fc_workspace_bytes_batch(n, m))
            + int(lib.fc_gram_workspace_bytes(n, m)) + int(lib.fc_dot_workspace_bytes(n, m))
            + 4 * n + 4 * n + 8 * m * m + _trim_ws_bytes(n, m, gar))


def gram_route_k(agg, clients) -> int:
    """k of the round's common 'top' codec when the round meets the "gram" route's conditions;
    otherwise ``NotImplementedError`` naming the condition that fails.  Touches no GPU (the
    budget is checked here only when ``device_budget_bytes`` is configured; :func:`gram_round`
    checks the default budget against the free memory)."""
    no, gar = _gram_no, agg.gar
    if type(gar) not in (FedAvg, Krum) + _LINEAR_RULES + _COORD_RULES:
        no("the device FedAvg or Krum (or spectral_gram / geometric_median / centered_clip / "
           "trimmed_mean / coordinate_median)")
    _no_hierarchies(agg, no)
    _one_device(agg, no)
    if isinstance(gar, CoordinateTrim):
        gar._unweighted()
    _f32_weights(gar, no)
    _at_most(len(clients), "clients", no)
    n, k = _top_round(clients, False, no)
    _fit(agg, gram_resident_bytes(n, len(clients), gar), no)
    return k


def gram_round(agg, clients, n: int, k: int, dev: torch.device) -> torch.Tensor:
    """One round on the "gram" route: upload, one batched 'top' encode, resolve, the packets'
    Gram matrix, then the FedAVG fold in row order (the "stream" route's bits), Krum's selected
    row, a linear rule's fold or a coordinate-wise rule's kernel (which reads the packets alone:
    the Gram matrix is then computed only for ``pc_analysis: "gram"``).  Appends G's singular
    values to ``gar.Sigma_tracked`` for
    ``pc_analysis: "gram"`` (after the entry ``SpectralGram`` appends itself: two per round)."""
    m = len(clients)
    _fit(agg, gram_resident_bytes(n, m, agg.gar), _gram_no, dev)
    pk = _cached(agg, "_gram_packets", (n, dev), m,
                 lambda count: codec.Packet.alloc_batch(n, count, L.FC_FMT_IDXVAL, dev, k=k))
    grads = [torch.from_numpy(np.ascontiguousarray(c.grad)).to(dev) for c in clients]
    codec.encode_top_batch(grads, k, packets=pk, check=False)
    codec.resolve(pk)
    for p in pk:
        p.release()
    del grads
    return _gram_family(agg, agg.gar, pk)


def _gram_family(agg, gar, pk) -> torch.Tensor:
    """The "gram" route's consumers on a round's resident packets (also aggregate_wire's, and
    the "sign-gram" and "sign-trim" routes' on sign packets: ``codec.gram_sign``,
    ``codec.fold_sign`` and, through the coordinate-wise rules, ``codec.trimmed_mean_sign``)."""
    m = len(pk)
    pc = _pc_gram(agg)
    sign = isinstance(pk[0], codec.SignPacket)
    if isinstance(gar, CoordinateTrim):
        out = gar.aggregate_packets(pk)
        gram = (codec.gram_sign(pk) if sign else codec.gram(pk)) if pc else None
    else:
        gram = codec.gram_sign(pk) if sign else codec.gram(pk)
        if isinstance(gar, (Krum, LinearRule)):
            out = gar.aggregate_packets(pk, gram=gram)
        else:
            w = gar._weights(m, np.float32)                         # gar.py:37-42 (persisted)
            fold = codec.fold_sign if sign else codec.decode_accumulate
            out = fold(pk, [float(x) for x in w])
    if pc:
        gar.Sigma_tracked.append(gram_singular_values(gram.cpu().numpy()))
    return out


def _pc_gram(agg) -> bool:
    return getattr(agg, "analyze_pc", False) == "gram"


# ---- rounds of scaled-sign clients: only their N/8-byte packets resident ----------------------
_MAJORITY_TAIL = ": the majority vote reads every packet at once"


def sign_packet_bytes(n: int) -> int:
    """Device bytes of one resident sign packet: its words and header, rounded up to 256."""
    return codec.slab_bytes(4 * int(L.load().fc_sign_words(n)) + L.HDR_BYTES)


def sign_route(agg, clients) -> bool:
    """Does this round take the "sign" route?  True when every client is the drop-in
    ``Compression`` with 'sign', the gradients are 1-D float32 of one length n > 0, there are no
    hierarchies, one device is used and the GAR is the device ``FedAvg`` with float32 or no
    weights (and ``"sign_packets"`` is not False), or ``SignMajority``.  A ``fed_avg`` round
    outside these conditions answers False (the generic routes take it); a ``sign_majority`` round
    outside them raises ``NotImplementedError`` naming the condition, and so does a round of 'sign'
    clients under a scheme that has no consumer of sign packets (Krum, the linear rules, the trim
    rules, ``pc_analysis: "gram"``) unless ``"sign_geometry"`` is set and the scheme is one of
    :func:`sign_geometry_wanted` (then False: :func:`sign_gram_route` decides), or ``"sign_trim"``
    is set and the scheme is a trim rule (:func:`sign_trim_wanted`; then False:
    :func:`sign_trim_route` decides).  Touches no GPU (the budget is checked here only when
    ``device_budget_bytes`` is configured; :func:`sign_round` checks the default budget)."""
    gar = getattr(agg, "gar", None)
    major = type(gar) is SignMajority
    if not _all_sign(clients):
        if major:
            _sign_no("every client to compress with 'sign'")
        return False
    if gram_wanted(agg):
        if sign_geometry_wanted(agg) or sign_trim_wanted(agg):
            return False                       # the "sign-gram" / "sign-trim" route's business
        what = type(gar).__name__ if type(gar) is not FedAvg else "pc_analysis 'gram'"
        raise NotImplementedError(f"{what} has no consumer of sign packets: a round of 'sign' "
                                  "clients takes fed_avg or sign_majority")
    if major:                                  # every failed condition is named
        gar._unweighted()
        n = _sign_conditions(agg, clients, _sign_no)
        _fit(agg, len(clients) * sign_packet_bytes(n) + 8 * n, _sign_no, tail=_MAJORITY_TAIL)
        return True
    if type(gar) is not FedAvg or _config(agg).get("sign_packets", True) is False:
        return False
    try:
        _sign_conditions(agg, clients, _refused)
    except _Refused:
        return False                           # the generic routes take the round
    return True


def _sign_residuals_ready(clients, n: int, dev: torch.device) -> None:
    """Every residual of the round checked before one advances: a bad one raises here."""
    for c in clients:
        if c.C.error_feedback:
            c.C._ef_buffers(n, dev, allocate=False)


#: clients per sub-batch of the batched sign encode, at the most
SIGN_ENCODE_GROUP = 64


def sign_encode_group(agg, n: int, count: int, dev: torch.device) -> int:
    """Clients per sub-batch of ``"batched_sign_encode"``: as many uploaded gradients (4N each) as
    fit in the budget beside what the route counts without the key apart from its one gradient
    in flight (the ``count`` packets and the aggregate), at most ``SIGN_ENCODE_GROUP`` and at
    least one."""
    fit = (_budget(agg, dev) - count * sign_packet_bytes(n) - 4 * n) // (4 * n)
    return int(max(1, min(SIGN_ENCODE_GROUP, count, fit)))


def _sign_encode_batched(agg, part, slots, n: int, dev: torch.device, count: int) -> None:
    """:func:`_sign_encode` under ``aggregation_config["batched_sign_encode"]``: ``part`` in row
    order in sub-batches of :func:`sign_encode_group` clients; a sub-batch is uploaded and its
    clients without error feedback go through ONE ``codec.encode_sign_batch`` call (one read of
    each gradient).  Its error-feedback clients keep the lone ``codec.encode_sign``, each committed
    after its encode was issued: the batched form that also writes the new residuals measured
    slower than the lone calls at 32 x 128 M.  The packets' and residuals'
    bits are those of the lone calls; ``agg.sign_encode_calls`` counts the batched library calls
    of the round."""
    gsz = sign_encode_group(agg, n, count, dev)
    for s in range(0, len(part), gsz):
        rows = list(zip(part[s:s + gsz], slots[s:s + gsz]))
        grads = [torch.from_numpy(np.ascontiguousarray(c.grad)).to(dev) for c, _ in rows]
        plain = [i for i, (c, _) in enumerate(rows) if not c.C.error_feedback]
        if plain:
            codec.encode_sign_batch([grads[i] for i in plain], packets=[rows[i][1] for i in plain])
            agg.sign_encode_calls += 1
        for g, (c, slot) in zip(grads, rows):
            if c.C.error_feedback:
                res, spare = c.C._ef_buffers(n, dev)
                _, new = codec.encode_sign(g, res, residual_out=spare, packet=slot)
                c.C._ef_commit(res, new, True)


def _sign_encode(agg, part, n: int, dev: torch.device, count: int) -> list:
    """``part`` (clients of a round that passed :func:`_sign_residuals_ready`, ``count`` of them
    at the most) uploaded and encoded one at a time (``codec.encode_sign``) into the aggregator's
    ``count`` cached sign packets; returns theirs.  With error feedback a client's residual
    advances exactly once, committed after its encode was issued.
    ``aggregation_config["batched_sign_encode"]`` (opt-in): :func:`_sign_encode_batched`, the
    same bits."""
    slots = _cached(agg, "_sign_packets", (n, dev), count,
                    lambda count: [codec.SignPacket.alloc(n, dev) for _ in range(count)])[:len(part)]
    if _config(agg).get("batched_sign_encode", False):
        _sign_encode_batched(agg, part, slots, n, dev, count)
        return slots
    for c, slot in zip(part, slots):
        g = torch.from_numpy(np.ascontiguousarray(c.grad)).to(dev)
        if c.C.error_feedback:
            res, spare = c.C._ef_buffers(n, dev)
            _, new = codec.encode_sign(g, res, residual_out=spare, packet=slot)
            c.C._ef_commit(res, new, True)
        else:
            codec.encode_sign(g, packet=slot)
    return slots


def sign_round(agg, clients, n: int, dev: torch.device) -> torch.Tensor:
    """One round on the "sign" route.  The clients are uploaded and encoded one at a time
    (:func:`_sign_encode`), so only their N/8-byte packets stay resident.
    ``FedAvg`` folds them in row order in groups sized by the budget, continuing the sum
    (``codec.fold_sign``: the "dense-fold" route's bits); ``SignMajority`` votes over all of them
    and raises ``NotImplementedError`` naming the budget when they do not fit."""
    gar, m = agg.gar, len(clients)
    major = type(gar) is SignMajority
    per = sign_packet_bytes(n)
    if major:
        _fit(agg, m * per + 8 * n, _sign_no, dev, tail=_MAJORITY_TAIL)
        group = m
    else:                                      # beside the aggregate and the gradient in flight
        group = int(max(1, min(m, 65535, (_budget(agg, dev) - 8 * n) // per)))
    _sign_residuals_ready(clients, n, dev)
    w = None if major else gar._weights(m, np.float32)                # gar.py:37-42 (persisted)
    out = torch.empty(n, dtype=torch.float32, device=dev)
    agg.sign_groups = agg.sign_encode_calls = 0
    for s in range(0, m, group):
        pk = _sign_encode(agg, clients[s:s + group], n, dev, group)
        if major:
            gar.aggregate_packets(pk, out=out)
        else:
            codec.fold_sign(pk, [float(x) for x in w[s:s + len(pk)]], out=out, continue_sum=s > 0)
        agg.sign_groups += 1
    return out


def _sign_encode_resident(agg, clients, n: int, dev: torch.device) -> list:
    """The round's clients encoded into sign packets that all stay resident."""
    _sign_residuals_ready(clients, n, dev)
    agg.sign_encode_calls = 0
    return _sign_encode(agg, clients, n, dev, len(clients))


# ---- the opt-in "sign-gram" and "sign-trim" routes: all M sign packets resident ----------------
def sign_geometry_wanted(agg) -> bool:
    """Is ``aggregation_config["sign_geometry"]`` set and the scheme one whose geometry sign
    packets can give: Krum, a linear rule, or the device FedAvg with ``pc_analysis: "gram"``?
    (The coordinate-wise rules need no geometry: their kernel over sign packets is behind
    ``"sign_trim"``, :func:`sign_trim_wanted`.)"""
    return (bool(_config(agg).get("sign_geometry", False)) and gram_wanted(agg)
            and not isinstance(agg.gar, CoordinateTrim))


def sign_trim_wanted(agg) -> bool:
    """Is ``aggregation_config["sign_trim"]`` set and the scheme a coordinate-wise rule
    (trimmed_mean, coordinate_median)?  The key does nothing for any other scheme."""
    return bool(_config(agg).get("sign_trim", False)) and type(getattr(agg, "gar", None)) in _COORD_RULES


def sign_gram_resident_bytes(n: int, m: int, packets_bytes: Optional[int] = None) -> int:
    """Device bytes the "sign-gram" routes hold at once: the m packets (``packets_bytes``: the
    uploaded payloads of ``aggregate_wire``), the aggregate, a carried vector (centered_clip),
    the Gram and dot kernels' workspaces and the Gram matrix."""
    lib = L.load()
    if packets_bytes is None:
        packets_bytes = m * sign_packet_bytes(n)
    return (packets_bytes + 4 * n + 4 * n + int(lib.fc_sign_gram_workspace_bytes(n, m))
            + int(lib.fc_sign_dot_workspace_bytes(n, m)) + 8 * m * m)


def sign_trim_resident_bytes(n: int, m: int, pc: bool = False,
                             packets_bytes: Optional[int] = None) -> int:
    """Device bytes the "sign-trim" routes hold at once: the m packets, the aggregate and the
    gradient in flight (8 n; from payloads, ``packets_bytes`` given, the aggregate alone: 4 n)
    and the trim kernel's workspace; with ``pc`` (``pc_analysis: "gram"``) the Gram kernel's
    workspace and the Gram matrix too."""
    lib = L.load()
    dense = 8 * n if packets_bytes is None else 4 * n
    if packets_bytes is None:
        packets_bytes = m * sign_packet_bytes(n)
    need = packets_bytes + dense + int(lib.fc_sign_trim_workspace_bytes(n, m))
    if pc:
        need += int(lib.fc_sign_gram_workspace_bytes(n, m)) + 8 * m * m
    return need


def _sign_resident_bytes(agg, trim: bool, n: int, m: int, packets_bytes: Optional[int] = None) -> int:
    if trim:
        return sign_trim_resident_bytes(n, m, _pc_gram(agg), packets_bytes)
    return sign_gram_resident_bytes(n, m, packets_bytes)


def _sign_resident_route(agg, clients, trim: bool) -> bool:
    """The conditions both resident routes ask of a round of 'sign' clients: those of
    :func:`_sign_conditions` (``trim``: unweighted), at most ``FC_GRAM_MAX_M`` clients and, when
    ``device_budget_bytes`` is configured, the resident bytes within it."""
    if not _all_sign(clients):
        return False
    no = _sign_trim_no if trim else _sign_gram_no
    n, m = _sign_conditions(agg, clients, no, unweighted=trim), len(clients)
    _at_most(m, "clients", no)
    _fit(agg, _sign_resident_bytes(agg, trim, n, m), no)
    return True


def sign_gram_route(agg, clients) -> bool:
    """Does this round take the "sign-gram" route?  False without the key, under a scheme outside
    :func:`sign_geometry_wanted`, or when not every client compresses with 'sign' (the other
    routes decide).  Otherwise the conditions of :func:`sign_route`, at most ``FC_GRAM_MAX_M``
    clients and, when ``device_budget_bytes`` is configured, the resident bytes within it: each
    failure is a ``NotImplementedError`` naming the condition.  Touches no GPU."""
    return sign_geometry_wanted(agg) and _sign_resident_route(agg, clients, False)


def sign_trim_route(agg, clients) -> bool:
    """Does this round take the "sign-trim" route?  False without the key, under a scheme that is
    no coordinate-wise rule, or when not every client compresses with 'sign' (the other routes
    decide).  Otherwise the conditions of :func:`sign_gram_route`: each failure is a
    ``NotImplementedError`` naming the condition, and a ``gradient_weights`` that is not None is
    the rules' ``ValueError``.  Touches no GPU."""
    return sign_trim_wanted(agg) and _sign_resident_route(agg, clients, True)


def _resident_round(agg, need: int, no, dev: torch.device, packets, what: str = "packets") -> torch.Tensor:
    """One round whose packets all stay resident ("sign-gram", "sign-trim" and aggregate_wire's
    Gram family): the default budget checked on the device, then ``packets()`` (the clients
    encoded, or the payloads uploaded) and the "gram" route's consumers on them."""
    _fit(agg, need, no, dev, what)
    return _gram_family(agg, agg.gar, packets())


def sign_resident_round(agg, clients, n: int, dev: torch.device, trim: bool) -> torch.Tensor:
    """One round on the "sign-gram" (``trim``: the "sign-trim") route: the clients are uploaded and
    encoded one at a time as in :func:`sign_round` (with error feedback each residual advances
    exactly once), all M packets stay resident, then :func:`_gram_family` runs on them: the Gram
    matrix from the bits and the rule, or ``codec.trimmed_mean_sign`` (``codec.gram_sign`` then
    only for ``pc_analysis: "gram"``)."""
    return _resident_round(agg, _sign_resident_bytes(agg, trim, n, len(clients)),
                           _sign_trim_no if trim else _sign_gram_no, dev,
                           lambda: _sign_encode_resident(agg, clients, n, dev))


# ---- rounds of QSGD clients: only their N W / 8-byte packets resident -------------------------
def _qsgd_bits(C) -> Optional[int]:
    """num_bits of a client that compresses with the native 'qsgd' at an integer number of bits in
    [1, 14], else None."""
    if getattr(C, "compression_function", None) != "qsgd" or getattr(C, "qsgd", None) != "native":
        return None
    b = getattr(C, "num_bits", None)
    if isinstance(b, bool) or not isinstance(b, (int, np.integer)) or not 1 <= b <= 14:
        return None
    return int(b)


def qsgd_packet_bytes(n: int, bits: int) -> int:
    """Device bytes of one resident QSGD packet: its codes and header, rounded up to 256."""
    return codec.slab_bytes(4 * int(L.load().fc_qsgd_code_words(n, bits)) + L.HDR_BYTES)


def qsgd_route(agg, clients) -> bool:
    """Does this round take the opt-in "qsgd" route?  True when
    ``aggregation_config["qsgd_packets"]`` is set, every client is the drop-in ``Compression`` with
    the native 'qsgd' at ``num_bits`` in [1, 14] (they may differ in bits, and in error feedback),
    the gradients are 1-D float32 of one length n > 0, there are no hierarchies, one device is used
    and the GAR is the device ``FedAvg`` with float32 or no weights and without
    ``pc_analysis: "gram"``.  A round outside these conditions answers False (the generic routes
    take it, as they take a ``fed_avg`` round of 'sign' clients).  Touches no GPU."""
    if not _config(agg).get("qsgd_packets", False) or not clients:
        return False
    if type(getattr(agg, "gar", None)) is not FedAvg or gram_wanted(agg):
        return False
    try:
        _drop_in(clients, _refused)
        if any(_qsgd_bits(c.C) is None for c in clients):
            _refused("every client to compress with the native 'qsgd' at 1..14 bits")
        _sign_conditions(agg, clients, _refused)      # the packet-round conditions, n > 0
    except _Refused:
        return False
    return True


def _qsgd_fold_group(agg, n: int, m: int, per_packet: int, dev: torch.device) -> int:
    """Packets per fold group: what fits beside the aggregate and the gradient in flight."""
    return int(max(1, min(m, 65535, (_budget(agg, dev) - 8 * n) // per_packet)))


def qsgd_round(agg, clients, n: int, dev: torch.device) -> torch.Tensor:
    """One round on the "qsgd" route.  The clients are uploaded and encoded one at a time into the
    aggregator's cached packets (``codec.encode_qsgd``: fc_qsgd_encode_ef with the client's residual
    buffers under error feedback, fc_qsgd_encode otherwise; each client's Philox offset is taken
    once and its residual is committed after its encode was issued), so only their codes stay
    resident.  They are folded in row order in groups sized by the budget, continuing the sum
    (``codec.decode_accumulate_qsgd``: the "dense-fold" route's bits); ``agg.qsgd_groups`` counts
    the groups."""
    gar, m = agg.gar, len(clients)
    bits = [_qsgd_bits(c.C) for c in clients]
    per = qsgd_packet_bytes(n, max(bits))              # a slot takes any client of the round
    group = _qsgd_fold_group(agg, n, m, per, dev)
    _sign_residuals_ready(clients, n, dev)             # every residual checked before one advances
    w = gar._weights(m, np.float32)                                   # gar.py:37-42 (persisted)
    out = torch.empty(n, dtype=torch.float32, device=dev)
    slots = _cached(agg, "_qsgd_packets", (n, per, dev), group,
                    lambda count: [codec.QsgdPacket.alloc(n, max(bits), dev) for _ in range(count)])
    agg.qsgd_groups = 0
    for s in range(0, m, group):
        pk = slots[:len(clients[s:s + group])]
        for c, b, slot in zip(clients[s:s + group], bits[s:s + group], pk):
            g = torch.from_numpy(np.ascontiguousarray(c.grad)).to(dev)
            C = c.C
            slot.bits = b
            if C.error_feedback:
                res, spare = C._ef_buffers(n, dev)
                _, new = codec.encode_qsgd(g, b, seed=C.seed, offset=C._next_offset(), packet=slot,
                                           residual=res, residual_out=spare)
                C._ef_commit(res, new, True)
            else:
                codec.encode_qsgd(g, b, seed=C.seed, offset=C._next_offset(), packet=slot)
        codec.decode_accumulate_qsgd(pk, [float(x) for x in w[s:s + len(pk)]], out=out,
                                     continue_sum=s > 0)
        agg.qsgd_groups += 1
    return out


def round_route(agg, clients):
    """Which of ``aggregate_grads``' packet routes the round takes, decided on the host (no GPU is
    touched): ``(agg_path, k)`` with ``agg_path`` one of "gram", "sign-gram", "sign-trim", "sign",
    "qsgd" and "ef-batch" (``k``: the common 'top' count of "gram" and "ef-batch", else None), or None
    for the stream / dense tail.  A round that a scheme or an opt-in key claims but whose
    conditions fail raises that route's refusal (no dense fallback).  The predicates are read in
    this order, so a round of 'sign' clients under a scheme without a consumer of sign packets is
    refused before the gram route's own conditions are read."""
    sign = sign_route(agg, clients)
    sign_gram = sign_gram_route(agg, clients)
    sign_trim = sign_trim_route(agg, clients)
    if sign_gram or sign_trim:
        return ("sign-gram" if sign_gram else "sign-trim"), None
    if gram_wanted(agg):
        return "gram", gram_route_k(agg, clients)
    if sign:
        return "sign", None
    if qsgd_route(agg, clients):
        return "qsgd", None
    k = ef_batch_k(agg, clients)
    return None if k is None else ("ef-batch", k)


def aggregate_grads(self, clients: List, input_feature: np.ndarray = None,
                    val_loader=None) -> None:
    """aggregation.py:54-78 on the device: sets ``self.agg_grad`` (host array) and
    ``self.curr_G`` as the reference does."""
    if len(clients) == 0:
        raise Exception('Client List is Empty')
    if self.analyze_pc is True:
        ref = getattr(type(self), "_ref_aggregate_grads", None)
        if ref is not None:                 # patched reference class: its own SVD analysis
            return ref(self, clients, input_feature, val_loader)
        raise NotImplementedError("pc_analysis (randomized SVD of G) is outside the hot path")
    # a packet route, or its refusal, is decided before a GPU is touched (no dense fallback)
    route = round_route(self, clients)
    dev = _device_of(self)
    grad0 = np.asarray(clients[0].grad)
    n = grad0.shape[0]
    if any(np.asarray(c.grad).shape != (n,) for c in clients):
        raise ValueError("client gradients must share one length (aggregation.py:61)")
    if route is not None:
        self.agg_path, k = route
        self.curr_G = None
        if self.agg_path == "gram":
            out = gram_round(self, clients, n, k, dev)
        elif self.agg_path == "sign":
            out = sign_round(self, clients, n, dev)
        elif self.agg_path == "qsgd":               # dense-fold's bits
            out = qsgd_round(self, clients, n, dev)
        elif self.agg_path == "ef-batch":           # dense-fold's bits
            w = self.gar._weights(len(clients), np.float32)         # gar.py:37-42 (persisted)
            out = ef_batch_fold(self, clients, n, k, w, dev)
        else:
            out = sign_resident_round(self, clients, n, dev, trim=self.agg_path == "sign-trim")
        self.agg_grad = out.cpu().numpy()
        return
    device_gar = hasattr(self.gar, "aggregate_packets")
    w = getattr(self.gar, "gradient_weights", None)
    f32_weights = w is None or np.asarray(w).dtype == np.float32
    plan = None
    # stream only when EVERY row is a float32 gradient: a float64 client after a float32 one
    # (RandomGaussian Byzantine noise, attack_models.py:105-118) is compressed in its own dtype
    # and cast into G's float32 row by the generic path, as aggregation.py:63 does
    all_f32 = all(np.asarray(c.grad).dtype == np.float32 for c in clients)
    streamable = device_gar and all_f32 and f32_weights and n > 0
    if streamable:
        # device permutations chain through one device state block: one device only
        want_perm = bool(_config(self).get("device_permutation", DEVICE_PERM))
        plan = row_plan(clients, n, device_perm=want_perm and len(stream_devices(self)) == 1)
    if plan is not None:
        # streamed from the host gradients, G never built (rows live group by group)
        self.agg_path = "stream"
        while True:
            try:
                if self.num_hierarchies > 0:
                    H = merge_streamed(self, clients, n, plan, self.cluster_size_list[0], dev)
                    H = merge_stages(H, self.cluster_size_list[1:], first_stage=1)
                    self.curr_G = H
                    agg = self.gar.aggregate(G=H, client_ids=np.arange(H.shape[0]))
                else:
                    self.curr_G = None
                    w = self.gar._weights(len(clients), np.float32)     # gar.py:37-42 (persisted)
                    agg = stream_fold(self, clients, n, plan, w, dev)
            except BaseException:
                plan.close(wait=False)
                raise
            try:
                plan.close()                # every draw done: the RNG is where the reference leaves it
            except MtRedraw:                # NumPy would redraw somewhere (~2^-52 per element),
                # or a device permutation fell back: the reference's host draws
                plan = row_plan(clients, n, device_mt=False, device_perm=False)
                continue
            break
        self.agg_draws = ("device-mt" if plan.mt_rows else "device-perm" if plan.perm_rows
                          else "host" if plan.draws else None)
    else:
        # generic codec mix / float64: the drop-in Compression per client, in row order; rows
        # take G's dtype (aggregation.py:61-63: G = zeros(..., dtype=clients[0].grad.dtype))
        tdt = torch.float64 if grad0.dtype == np.float64 else torch.float32
        if device_gar and self.num_hierarchies == 0:
            # nothing reads G but the GAR: fold each row as it is made (bounded: one row)
            self.agg_path = "dense-fold"
            self.curr_G = None
            agg = fold_rows(self.gar, clients, n, tdt, dev)
            self.agg_grad = agg.cpu().numpy()
            return
        self.agg_path = "dense"
        G = torch.empty((len(clients), n), dtype=tdt, device=dev)
        for ix, c in enumerate(clients):
            q = c.C.compress(c.grad)
            q = q if isinstance(q, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(q))
            G[ix].copy_(q)                  # implicit cast to G's dtype, as G[ix, :] = q
        if self.num_hierarchies > 0:
            G = merge_stages(G, self.cluster_size_list)
            client_ids = np.arange(G.shape[0])
        else:
            client_ids = np.array([c.client_id for c in clients])
        if device_gar:
            self.curr_G = G
            agg = self.gar.aggregate(G=G, client_ids=client_ids)
        else:                               # a reference GAR: the host G it expects
            self.curr_G = G.cpu().numpy()
            agg = self.gar.aggregate(G=self.curr_G, client_ids=client_ids)
    self.agg_grad = agg.cpu().numpy() if isinstance(agg, torch.Tensor) else agg


def wire_group(agg, n: int, m: int, dev: torch.device) -> int:
    """Payloads per fold group of :func:`aggregate_wire`'s FedAvg: the streamed route's own
    sizing (``pipeline.plan_group`` under :func:`_budget`; a group's wire bytes are smaller than
    the gradients that budget reserves a ring for)."""
    from .pipeline import plan_group
    return plan_group(n, m, _budget(agg, dev))


def wire_resident_bytes(n: int, m: int, wire_total: int, gar=None) -> int:
    """Device bytes :func:`aggregate_wire` holds at once on the Gram family's path: the round's
    wire bytes and unpacked packets, the Gram and dot workspaces, the aggregate, a carried vector
    and the Gram matrix; for a coordinate-wise ``gar`` the trim kernel's workspace too."""
    from .pipeline import packet_bytes
    lib = L.load()
    return (wire_total + m * packet_bytes(n) + int(lib.fc_gram_workspace_bytes(n, m))
            + int(lib.fc_dot_workspace_bytes(n, m)) + 4 * n + 4 * n + 8 * m * m
            + _trim_ws_bytes(n, m, gar))


def wire_fold_groups(sizes, n: int, budget_bytes: int) -> List[range]:
    """The payloads of a ``"wire_fold"`` round cut into consecutive groups, greedily: a group's
    sizes, each rounded up to 256 bytes (its place in the device slab), plus ``4 n`` for the
    aggregate stay within ``budget_bytes``; a group holds at most 65535 payloads (one
    ``fc_wire_fold`` call) and never fewer than one.  A single payload that does not fit raises
    ``NotImplementedError`` naming both numbers.  The aggregate cannot depend on the cut: the sum
    is strictly left to right, and a sum started from +0 never holds -0.0."""
    room = int(budget_bytes) - 4 * int(n)
    groups, first, used = [], 0, 0
    for i, b in enumerate(sizes):
        r = codec.slab_bytes(b)
        if r > room:
            _wire_no(f"payload {i} and the aggregate to fit device_budget_bytes "
                     f"({r + 4 * int(n)} > {int(budget_bytes)} bytes)")
        if i > first and (used + r > room or i - first == 65535):
            groups.append(range(first, i))
            first, used = i, 0
        used += r
    if len(sizes) > first:
        groups.append(range(first, len(sizes)))
    return groups


#: per payload kind: the aggregator's slab cache and codec's FedAVG fold of the uploaded packets
_WIRE_FOLD = {"top": ("_wire_packets", "fold_wire"), "sign": ("_sign_wire", "fold_sign"),
              "qsgd": ("_qsgd_wire", "decode_accumulate_qsgd")}


def _fold_groups(agg, hosts, groups, n: int, dev: torch.device, upload, fold) -> torch.Tensor:
    """aggregate_wire's FedAVG of validated payloads: group by group in row order ``upload`` puts a
    group on the device (its packets) and ``fold`` adds them to the sum, which continues from group
    to group."""
    wts = agg.gar._weights(len(hosts), np.float32)                  # gar.py:37-42 (persisted)
    out = torch.empty(n, dtype=torch.float32, device=dev)
    for gi, g in enumerate(groups):
        fold(upload(hosts[g.start:g.stop]), [float(x) for x in wts[g.start:g.stop]], out=out,
             continue_sum=gi > 0)
    return out


def _validated(payloads, check, n: Optional[int], no):
    """Every payload through ``check`` (a ``codec.PayloadKind``'s) on the host:
    (the ``(bytes, header)`` pairs, their common n).  A bad payload is a ``ValueError`` naming its
    position and the reason."""
    hosts = []
    for i, raw in enumerate(payloads):
        try:
            a, h = check(raw)
        except ValueError as e:
            raise ValueError(f"payload {i}: {e}") from None
        hn = int(h.pkt.n)
        if n is None:
            n = hn
        if hn != int(n):
            no(f"payloads of one length n (payload {i} has n = {hn}, not {int(n)})")
        hosts.append((a, h))
    return hosts, int(n)


def aggregate_wire(self, payloads, n: Optional[int] = None) -> None:
    """A round from the clients' wire packets (``Compression.compress_wire``; include/fedcodec.h)
    instead of their gradients: the "wire*" rows of the module's table.  Every payload is
    validated on the host (``fc_wire_validate`` / ``fc_sign_wire_validate``: ``ValueError`` with
    the payload's position and the reason) and every condition that needs no GPU is checked
    before any of the round reaches it.  Sets ``agg_grad`` (host array), ``agg_path`` and
    ``curr_G = None``.

    * 'top' payloads under ``fed_avg``: any number, folded in row order in groups sized by the
      device budget ("wire": unpacked into slotted packets, :func:`wire_group`; "wire-fold":
      folded as they are, :func:`wire_fold_groups`); bit-equal to the "stream" route of
      ``aggregate_grads`` on the same clients.
    * 'top' payloads under a scheme of :func:`gram_wanted` ("wire", whatever ``"wire_fold"``
      says: those consumers read slotted packets), sign payloads under ``"sign_geometry"``
      ("wire-sign-gram") or ``"sign_trim"`` ("wire-sign-trim"): at most ``FC_GRAM_MAX_M``
      payloads, all resident within the budget, then the "gram" route's consumers
      (:func:`_gram_family`): the bits of ``aggregate_grads``' "gram", "sign-gram" and "sign-trim"
      routes on the same clients.
    * sign payloads under ``fed_avg`` (folded in groups, ``codec.fold_sign``) or ``sign_majority``
      (voted over, all resident): "wire-sign".  Every other scheme refuses sign payloads, and a
      round that mixes the two payload kinds is refused.
    * QSGD payloads (``codec.pack_qsgd``) under ``fed_avg``: validated by
      ``fc_qsgd_wire_validate``, uploaded and folded in groups (``codec.decode_accumulate_qsgd``):
      "wire-qsgd", the bits of ``aggregate_grads``' "qsgd" route on the same clients.  Every other
      scheme refuses them, and so is a round that mixes them with another payload kind.
    Hierarchies, several devices, payloads of differing n and a round that does not fit raise
    ``NotImplementedError`` naming the condition."""
    no = _wire_no
    payloads = list(payloads)
    m = len(payloads)
    if m == 0:
        raise Exception('Client List is Empty')
    if self.analyze_pc is True:
        no("pc_analysis off or 'gram' (the randomized SVD of G is outside the hot path)")
    _no_hierarchies(self, no)
    gar = self.gar
    # ---- one kind of payload ----
    TOP, SIGN, QSGD = codec.TOP, codec.SIGN, codec.QSGD
    kinds = [codec.kind_of(raw) for raw in payloads]
    kind = QSGD if QSGD in kinds else SIGN if SIGN in kinds else TOP
    if any(k is not kind for k in kinds):
        no("payloads of one kind (the round mixes "
           + ("QSGD packets with sign packets or 'top' wire packets)" if kind is QSGD
              else "sign packets and 'top' wire packets)"))
    # ---- the kind's consumers under this scheme; family: all of the round resident ----
    trim = kind is SIGN and sign_trim_wanted(self)
    what, many = "packets", "payloads for the gram route"
    if kind is QSGD:
        family = False
        if type(gar) is not FedAvg or gram_wanted(self):
            no("fed_avg for QSGD packets (sign_majority, Krum, the linear rules, the trim rules and "
               "pc_analysis 'gram' have no consumer of QSGD packets)")
    elif kind is SIGN:
        family = sign_geometry_wanted(self) or trim
        if (type(gar) not in (FedAvg, SignMajority) or gram_wanted(self)) and not family:
            no("fed_avg or sign_majority for sign packets (Krum, the linear rules, the trim rules "
               "and pc_analysis 'gram' have no consumer of sign packets)")
        what, many = "sign packets", "payloads" if trim else "payloads for the sign-gram route"
    else:
        family = gram_wanted(self)
        if not family and type(gar) is not FedAvg:
            no("the device FedAvg, Krum, spectral_gram, geometric_median, centered_clip, trimmed_mean "
               "or coordinate_median")
    family_no = _sign_trim_no if trim else no      # the sign-trim route names its own refusals
    _one_device(self, no)
    if type(gar) is SignMajority or isinstance(gar, CoordinateTrim):
        gar._unweighted()
    _f32_weights(gar, no)
    if family:
        _at_most(m, many, family_no)
    # ---- the host's part: every payload validated, one common n, a configured budget ----
    hosts, n = _validated(payloads, kind.check, n, no)
    if kind is not TOP:
        self.curr_G = None
    if family:
        total = sum(codec.slab_bytes(a.size) for a, _ in hosts)
        need = (_sign_resident_bytes(self, trim, n, m, total) if kind is SIGN
                else wire_resident_bytes(n, m, total, gar))
        _fit(self, need, family_no, what=what)
    # ---- the device's part: a round of 'top' payloads is named once the device is known ----
    if kind is SIGN:
        self.agg_path = "wire-sign" + ("" if not family else "-trim" if trim else "-gram")
    elif kind is QSGD:
        self.agg_path = "wire-qsgd"
    dev = _device_of(self)
    if kind is TOP:
        self.agg_path = "wire"
        self.curr_G = None
    slab, fold = _WIRE_FOLD[kind.name]

    def upload(part):
        """The payloads of one group into one cached device slab (256-byte aligned each)."""
        return _slab_upload(self, slab, kind.upload, part, dev)

    def unpacked(wires):
        return codec.unpack(wires, _cached(
            self, "_wire_packets", (n, dev), len(wires),
            lambda count: codec.Packet.alloc_batch(n, count, L.FC_FMT_IDXVAL, dev)))

    if family:                                                      # all resident: Gram / trim family
        out = _resident_round(self, need, family_no, dev, what=what, packets=lambda: (
            upload(hosts) if kind is SIGN else unpacked(upload(hosts))))
    elif type(gar) is SignMajority:                                 # all resident: the vote
        _fit(self, sum(codec.slab_bytes(a.size) for a, _ in hosts) + 4 * n, no, dev, "sign packets",
             _MAJORITY_TAIL)
        out = torch.empty(n, dtype=torch.float32, device=dev)
        gar.aggregate_packets(upload(hosts), out=out)
    elif kind is TOP and not _config(self).get("wire_fold", False):  # unpacked, then folded
        group = wire_group(self, n, m, dev)
        out = _fold_groups(self, hosts, [range(s, min(s + group, m)) for s in range(0, m, group)], n, dev,
                           lambda part: unpacked(upload(part)), codec.decode_accumulate)
    else:                                                           # folded as they are
        groups = wire_fold_groups([a.size for a, _ in hosts], n, _budget(self, dev))
        if kind is TOP:
            self.agg_path = "wire-fold"
        out = _fold_groups(self, hosts, groups, n, dev, upload, getattr(codec, fold))
        if kind is QSGD:
            self.qsgd_groups = len(groups)
    self.agg_grad = out.cpu().numpy()


class Aggregator:
    """aggregation.py:19-93 — the aggregation hot path of the reference's ``Aggregator``.

    Same constructor, attributes and ``aggregate_grads`` contract; ``agg_grad`` is the host
    NumPy array the server loop reads (server.py:98 -> update_model)."""

    def __init__(self, aggregation_config: Dict, model=None, optimizer=None, clip_val=None,
                 lr_scheduler=None, device: Optional[torch.device] = None):
        self.aggregation_config = aggregation_config
        self.model = model
        self.opt = optimizer
        self.clip_val = clip_val if isinstance(clip_val, float) is True else -1.0
        self.lrs = lr_scheduler
        self.gar = self.__get_gar()
        self.curr_G = None
        self.agg_grad = None
        self.agg_path = None                # the last call's route: a row of the module docstring's tables
        self.agg_draws = None               # streamed np.random draws: "device-mt" | "device-perm" | "host" | None
        self.analyze_pc = self.aggregation_config.get("pc_analysis", False)
        self.num_hierarchies = self.aggregation_config.get("num_hierarchies", 0)
        self.cluster_size_list = self.aggregation_config.get("cluster_size_list", [])
        assert self.num_hierarchies == len(self.cluster_size_list), \
            "Unmatched hierarchial and cluster size list length"
        self.device = device                # None: the current device, resolved per call

    def __get_gar(self):                                                  # aggregation.py:44-52
        scheme = self.aggregation_config["aggregation_scheme"]
        if scheme == "fed_avg":
            return FedAvg(aggregation_config=self.aggregation_config)
        if scheme == "krum":
            return Krum(aggregation_config=self.aggregation_config)
        if scheme == "spectral_gram":
            return SpectralGram(aggregation_config=self.aggregation_config)
        if scheme == "geometric_median":
            return GeometricMedian(aggregation_config=self.aggregation_config)
        if scheme == "centered_clip":
            return CenteredClip(aggregation_config=self.aggregation_config)
        if scheme == "trimmed_mean":
            return TrimmedMean(aggregation_config=self.aggregation_config)
        if scheme == "coordinate_median":
            return CoordinateMedian(aggregation_config=self.aggregation_config)
        if scheme == "sign_majority":
            return SignMajority(aggregation_config=self.aggregation_config)
        if scheme == "fed_spectral_avg":
            raise NotImplementedError("SpectralFedAvg is outside the codec hot path (DESIGN.md §8)")
        raise NotImplementedError

    aggregate_grads = aggregate_grads
    aggregate_wire = aggregate_wire

    def update_model(self):
        raise NotImplementedError("model update is outside the codec hot path (DESIGN.md §8)")


__all__ = ["Aggregator", "Compression", "aggregate_grads", "aggregate_wire"]
