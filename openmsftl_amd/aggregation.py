"""Drop-in ``Aggregator.aggregate_grads`` (ftl/gradient_aggregation/aggregation.py:19-93) on MI355X.

The reference builds the dense host matrix ``G`` (M x N) row by row from
``client.C.compress(client.grad)`` (aggregation.py:61-63), optionally merges client clusters
(``__merge_gradient``, aggregation.py:80-93, ``num_hierarchies > 0``) and reduces it with the
GAR (gar.py:44).  Here the rows never become a dense matrix on the common path:

* when every client's codec is one of compression.py's ('full', 'top', 'rand',
  'dropout-biased', 'dropout-unbiased') on float32 gradients, their host gradients stream
  through a bounded device ring (openmsftl_amd/pipeline.py): H2D, each row made on the device
  (top-k packets, mask packets whose masks are drawn on the host from the global
  ``np.random`` in row order exactly as the reference draws them, or the dense gradient for
  'full'), and every group folded into the FedAVG sum in row order (``fc_decode_accumulate``
  / ``fc_weighted_sum_dense_continue``: bit-exact ``np.sum(G * w[:, None], axis=0)``).  G is
  never built and device memory stays within ``device_budget_bytes`` for any client count.
  ``aggregation_config["devices"]`` (or ``integration.install(devices=...)``) fans the groups
  out round-robin over several GPUs, one pipeline and host thread each, the running sum
  hopping between them in group order; the default is the current device only;
* with hierarchies each first-stage cluster mean is the streamed fold with weights 1 (the
  +0-started row-order sum ``np.mean`` computes) divided once by the row count
  (``fc_div_scalar``); later stages do the same over the dense merged rows
  (``fc_weighted_sum_dense``); the GAR then reduces the merged rows.
* 'qsgd' (opt-in) or a codec the reference rejects, float64 gradients (``RandomGaussian``
  with ``noise_scale == 0``, attack_models.py:105-106) and float64 GAR weights take the
  generic path: the drop-in ``Compression`` per client in row order on the device (same NumPy
  RNG draws as the reference, the same exceptions at the same row), each row cast to G's dtype
  and folded at once into the GAR's sum in NumPy's promoted dtype (``fold_rows``: one row of
  device memory); only a merge (hierarchies) or a host GAR stacks the rows into G.
* opt-in (``aggregation_config["batched_error_feedback"]``): a round whose clients ALL compress
  with 'top' and error feedback takes the "ef-batch" route (:func:`ef_batch_k`,
  :func:`ef_batch_fold`): groups of <= 64 clients encoded by one fc_topk_encode_ef_batch launch
  chain and folded in row order, the same bits as the generic path.

* ``aggregation_scheme: "krum"`` (gar.Krum) and ``aggregation_config["pc_analysis"] = "gram"``
  take the "gram" route (:func:`gram_route_k`, :func:`gram_round`): the whole round's 'top'
  packets resident at once (upload, one batched encode, resolve), their M x M float64 Gram matrix
  straight from the packets (``codec.gram``), then the FedAVG fold (the "stream" route's bits:
  the same encode, the same row-order fold) or Krum's selection.  With ``pc_analysis: "gram"``
  the singular values of G, ``sqrt(max(eigvalsh(gram), 0))`` descending (float64, length M,
  all NaN when the Gram holds NaN), are appended to ``self.gar.Sigma_tracked`` after the
  round.  Unlike the reference's ``randomized_svd`` this draws nothing from ``np.random``, so
  the global RNG stream of a run differs from the reference's by exactly those draws.  The
  string is deliberate: ``pc_analysis: True`` keeps raising on the device class as before.  A
  round that does not meet the route's conditions raises ``NotImplementedError`` naming the
  condition (no silent dense fallback).
* ``aggregation_scheme: "spectral_gram"`` / ``"geometric_median"`` / ``"centered_clip"``
  (gar.LinearRule) take the same route: coefficients from the Gram matrix (and
  ``codec.dot_dense`` for row sums or a carried vector), then the row-order fold of the packets
  with those coefficients.  ``"fed_spectral_avg"`` (the reference's class, with its autoencoder
  branch) keeps raising.
* ``aggregation_scheme: "trimmed_mean"`` / ``"coordinate_median"`` (gar.CoordinateTrim) take the
  same route under the same conditions: one kernel over the resident packets
  (``codec.trimmed_mean``), unweighted (``gradient_weights`` must be None).  The rule needs no
  Gram matrix: it is computed only when ``pc_analysis: "gram"`` asks for the singular values.
* opt-in (``aggregation_config["sign_trim"] = True``): a round whose clients ALL compress with
  'sign' under ``trimmed_mean`` / ``coordinate_median`` takes the "sign-trim" route
  (:func:`sign_trim_route`, :func:`sign_trim_round`): the clients encoded one at a time, all M
  N/8-byte packets resident, then one kernel over their bits (``codec.trimmed_mean_sign``);
  ``aggregate_wire`` takes the same clients' payloads as "wire-sign-trim", the same bits.

* ``Aggregator.aggregate_wire(payloads)`` (:func:`aggregate_wire`) aggregates a round from the
  clients' wire packets (``Compression.compress_wire``; include/fedcodec.h) instead of their
  gradients: validated on the host, uploaded, unpacked into slotted packets, then the fold of
  the "stream" route or the Gram family's ``aggregate_packets``: the same bits, ``agg_path =
  "wire"``.  ``aggregation_config["wire_fold"] = True`` (default off) folds FedAvg straight from
  the uploaded wire bytes instead (``codec.fold_wire``, no slotted packets): the same bits,
  ``agg_path = "wire-fold"``.

``aggregate_grads`` is a plain function so that :func:`openmsftl_amd.integration.install` can
bind it onto the REFERENCE ``Aggregator`` class (its ``self.gar`` may then be a reference GAR
with no ``aggregate_packets``: G is then handed over as the host array the reference builds).

Results are bit-exact against the reference (tests/golden/make_golden_agg.py pins the merge and
the sign-of-zero semantics; tests/test_gpu_parity.py runs both paths).  Out of the hot path and
not rebuilt: ``pc_analysis`` (randomized SVD of G), ``SpectralFedAvg``, ``update_model`` and the
RL / DGA aggregators: the device class raises ``NotImplementedError`` for them,
the patched reference class keeps its own code for ``pc_analysis``.
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
    cfg = getattr(agg, "aggregation_config", None) or {}
    spec = cfg.get("devices")
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


#: clients per batched error-feedback encode at most (k_compact_mag1's interleave group)
EF_BATCH_GROUP = 64


def ef_batch_k(agg, clients) -> Optional[int]:
    """k when the round may take the opt-in "ef-batch" route, else None (today's routing):
    ``aggregation_config["batched_error_feedback"]`` is set, the GAR is the device FedAvg with
    float32 (or no) weights, no hierarchies, one device, and EVERY client is the drop-in
    Compression with 'top', error feedback on and one common fraction with 0 < k < n, on 1-D
    float32 gradients of one length.  Touches no GPU."""
    cfg = getattr(agg, "aggregation_config", None) or {}
    if not cfg.get("batched_error_feedback", False) or not clients:
        return None
    if type(agg.gar) is not FedAvg or agg.num_hierarchies != 0:
        return None
    if cfg.get("devices", DEFAULT_DEVICES) not in (None, 1):      # multi-GPU rounds: dense-fold
        return None
    w = getattr(agg.gar, "gradient_weights", None)
    if w is not None and np.asarray(w).dtype != np.float32:
        return None
    n, fr = None, None
    for c in clients:
        C, g = c.C, np.asarray(c.grad)
        if not isinstance(C, Compression) or C.compression_function != "top" or not C.error_feedback:
            return None
        if g.ndim != 1 or g.dtype != np.float32 or (n is not None and g.shape[0] != n):
            return None
        f = C.fraction_coordinates
        if not isinstance(f, (int, float, np.floating, np.integer)) or not np.isfinite(f):
            return None
        if fr is not None and f != fr:
            return None
        n, fr = g.shape[0], f
    k = kept_count(fr, n)
    return k if 0 < k < n else None


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
    cache = agg.__dict__.setdefault("_ef_batch_packets", {})
    packets = cache.get((n, dev))
    if packets is None or len(packets) < gsz:
        cache.clear()
        packets = cache[(n, dev)] = codec.Packet.alloc_batch(n, gsz, L.FC_FMT_IDXVAL, dev, k=k)
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
    def no(why: str):
        raise NotImplementedError(f"the gram route (krum / pc_analysis='gram') needs {why}")
    cfg = getattr(agg, "aggregation_config", None) or {}
    if type(agg.gar) not in (FedAvg, Krum) + _LINEAR_RULES + _COORD_RULES:
        no("the device FedAvg or Krum (or spectral_gram / geometric_median / centered_clip / "
           "trimmed_mean / coordinate_median)")
    if agg.num_hierarchies != 0:
        no("no hierarchies (num_hierarchies == 0)")
    if cfg.get("devices", DEFAULT_DEVICES) not in (None, 1):
        no("one device")
    w = getattr(agg.gar, "gradient_weights", None)
    if w is not None and isinstance(agg.gar, CoordinateTrim):
        raise ValueError(f"{type(agg.gar).__name__} is unweighted: gradient_weights must be None")
    if w is not None and np.asarray(w).dtype != np.float32:
        no("float32 GAR weights")
    if len(clients) > L.FC_GRAM_MAX_M:
        no(f"at most {L.FC_GRAM_MAX_M} clients (got {len(clients)})")
    n, fr = None, None
    for c in clients:
        C, g = c.C, np.asarray(c.grad)
        if getattr(C, "compression_function", None) != "top":
            no("every client to compress with 'top'")
        if getattr(C, "error_feedback", False):
            no("'top' without error feedback")
        if g.ndim != 1 or g.dtype != np.float32:
            no("1-D float32 gradients")
        if n is not None and g.shape[0] != n:
            no("gradients of one length")
        f = C.fraction_coordinates
        if not isinstance(f, (int, float, np.floating, np.integer)) or not np.isfinite(f):
            no("a finite fraction_coordinates")
        if fr is not None and f != fr:
            no("one common fraction_coordinates")
        n, fr = g.shape[0], f
    k = kept_count(fr, n)
    if not 0 < k < n:
        no(f"0 < k < n (k={k}, n={n})")
    b = cfg.get("device_budget_bytes")
    if b and gram_resident_bytes(n, len(clients), agg.gar) > int(b):
        no(f"the round's packets to fit device_budget_bytes ({gram_resident_bytes(n, len(clients), agg.gar)}"
           f" > {int(b)} bytes)")
    return k


def gram_round(agg, clients, n: int, k: int, dev: torch.device) -> torch.Tensor:
    """One round on the "gram" route: upload, one batched 'top' encode, resolve, the packets'
    Gram matrix, then the FedAVG fold in row order (the "stream" route's bits), Krum's selected
    row, a linear rule's fold or a coordinate-wise rule's kernel (which reads the packets alone:
    the Gram matrix is then computed only for ``pc_analysis: "gram"``).  Appends G's singular
    values to ``gar.Sigma_tracked`` for
    ``pc_analysis: "gram"`` (after the entry ``SpectralGram`` appends itself: two per round)."""
    m = len(clients)
    need = gram_resident_bytes(n, m, agg.gar)
    if need > _budget(agg, dev):
        raise NotImplementedError("the gram route (krum / pc_analysis='gram') needs the round's packets "
                                  f"to fit device_budget_bytes ({need} > {_budget(agg, dev)} bytes)")
    cache = agg.__dict__.setdefault("_gram_packets", {})
    packets = cache.get((n, dev))
    if packets is None or len(packets) < m:
        cache.clear()
        packets = cache[(n, dev)] = codec.Packet.alloc_batch(n, m, L.FC_FMT_IDXVAL, dev, k=k)
    pk = packets[:m]
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
    pc = getattr(agg, "analyze_pc", False) == "gram"
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


# ---- the "sign" route: a round of scaled-sign clients, only their N/8-byte packets resident ----
def _sign_no(why: str):
    raise NotImplementedError(f"the sign route (sign packets: fed_avg / sign_majority) needs {why}")


def sign_packet_bytes(n: int) -> int:
    """Device bytes of one resident sign packet: its words and header, rounded up to 256."""
    return (4 * int(L.load().fc_sign_words(n)) + L.HDR_BYTES + 255) & ~255


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
    cfg = getattr(agg, "aggregation_config", None) or {}
    major = type(gar) is SignMajority
    all_sign = all(getattr(c.C, "compression_function", None) == "sign" for c in clients)
    if not all_sign:
        if major:
            _sign_no("every client to compress with 'sign'")
        return False
    if gram_wanted(agg):
        if sign_geometry_wanted(agg):
            return False                       # the "sign-gram" route's business (sign_gram_route)
        if sign_trim_wanted(agg):
            return False                       # the "sign-trim" route's business (sign_trim_route)
        what = type(gar).__name__ if type(gar) is not FedAvg else "pc_analysis 'gram'"
        raise NotImplementedError(f"{what} has no consumer of sign packets: a round of 'sign' "
                                  "clients takes fed_avg or sign_majority")
    if not major and (type(gar) is not FedAvg or cfg.get("sign_packets", True) is False):
        return False

    def no(why: str):
        if major:
            _sign_no(why)
        return False

    if major and gar.gradient_weights is not None:
        raise ValueError("SignMajority is unweighted: gradient_weights must be None")
    if not all(isinstance(c.C, Compression) for c in clients):
        return no("every client to be the drop-in Compression")
    if agg.num_hierarchies != 0:
        return no("no hierarchies (num_hierarchies == 0)")
    if cfg.get("devices", DEFAULT_DEVICES) not in (None, 1):
        return no("one device")
    w = getattr(gar, "gradient_weights", None)
    if w is not None and np.asarray(w).dtype != np.float32:
        return no("float32 GAR weights")
    n = None
    for c in clients:
        g = np.asarray(c.grad)
        if g.ndim != 1 or g.dtype != np.float32:
            return no("1-D float32 gradients")
        if n is not None and g.shape[0] != n:
            return no("gradients of one length")
        n = g.shape[0]
    if n == 0:
        return no("a gradient length n > 0")
    b = cfg.get("device_budget_bytes")
    if major and b and len(clients) * sign_packet_bytes(n) + 8 * n > int(b):
        _sign_no(f"the round's packets to fit device_budget_bytes "
                 f"({len(clients) * sign_packet_bytes(n) + 8 * n} > {int(b)} bytes): the majority "
                 "vote reads every packet at once")
    return True


def sign_round(agg, clients, n: int, dev: torch.device) -> torch.Tensor:
    """One round on the "sign" route.  The clients are uploaded and encoded one at a time
    (``codec.encode_sign``; with error feedback each client's residual advances exactly once,
    committed after its encode was issued), so only their N/8-byte packets stay resident.
    ``FedAvg`` folds them in row order in groups sized by the budget, continuing the sum
    (``codec.fold_sign``: the "dense-fold" route's bits); ``SignMajority`` votes over all of them
    and raises ``NotImplementedError`` naming the budget when they do not fit."""
    gar, m = agg.gar, len(clients)
    major = type(gar) is SignMajority
    per, budget = sign_packet_bytes(n), _budget(agg, dev)
    room = budget - 8 * n                      # beside the aggregate and the gradient in flight
    if major and m * per > room:
        _sign_no(f"the round's packets to fit device_budget_bytes ({m * per + 8 * n} > {budget} "
                 "bytes): the majority vote reads every packet at once")
    group = m if major else int(max(1, min(m, 65535, room // per)))
    for c in clients:                          # every residual checked before one advances
        if c.C.error_feedback:
            c.C._ef_buffers(n, dev, allocate=False)
    w = None if major else gar._weights(m, np.float32)                # gar.py:37-42 (persisted)
    cache = agg.__dict__.setdefault("_sign_packets", {})
    slots = cache.get((n, dev))
    if slots is None or len(slots) < group:
        cache.clear()
        slots = cache[(n, dev)] = [codec.SignPacket.alloc(n, dev) for _ in range(group)]
    out = torch.empty(n, dtype=torch.float32, device=dev)
    agg.sign_groups = 0
    for s in range(0, m, group):
        part = clients[s:s + group]
        for c, slot in zip(part, slots):
            g = torch.from_numpy(np.ascontiguousarray(c.grad)).to(dev)
            if c.C.error_feedback:
                res, spare = c.C._ef_buffers(n, dev)
                _, new = codec.encode_sign(g, res, residual_out=spare, packet=slot)
                c.C._ef_commit(res, new, True)
            else:
                codec.encode_sign(g, packet=slot)
        pk = slots[:len(part)]
        if major:
            gar.aggregate_packets(pk, out=out)
        else:
            codec.fold_sign(pk, [float(x) for x in w[s:s + len(part)]], out=out, continue_sum=s > 0)
        agg.sign_groups += 1
    return out


# ---- the "sign-gram" route (opt-in): the Gram family's consumers on a round of sign packets ----
def sign_geometry_wanted(agg) -> bool:
    """Is ``aggregation_config["sign_geometry"]`` set and the scheme one whose geometry sign
    packets can give: Krum, a linear rule, or the device FedAvg with ``pc_analysis: "gram"``?
    (The coordinate-wise rules need no geometry: their kernel over sign packets is behind
    ``"sign_trim"``, :func:`sign_trim_wanted`.)"""
    cfg = getattr(agg, "aggregation_config", None) or {}
    return (bool(cfg.get("sign_geometry", False)) and gram_wanted(agg)
            and not isinstance(agg.gar, CoordinateTrim))


def sign_gram_resident_bytes(n: int, m: int, packets_bytes: Optional[int] = None) -> int:
    """Device bytes the "sign-gram" routes hold at once: the m packets (``packets_bytes``: the
    uploaded payloads of ``aggregate_wire``), the aggregate, a carried vector (centered_clip),
    the Gram and dot kernels' workspaces and the Gram matrix."""
    lib = L.load()
    if packets_bytes is None:
        packets_bytes = m * sign_packet_bytes(n)
    return (packets_bytes + 4 * n + 4 * n + int(lib.fc_sign_gram_workspace_bytes(n, m))
            + int(lib.fc_sign_dot_workspace_bytes(n, m)) + 8 * m * m)


def sign_gram_route(agg, clients) -> bool:
    """Does this round take the "sign-gram" route?  False without the key, under a scheme outside
    :func:`sign_geometry_wanted`, or when not every client compresses with 'sign' (the other
    routes decide).  Otherwise the conditions of :func:`sign_route`, at most ``FC_GRAM_MAX_M``
    clients and, when ``device_budget_bytes`` is configured, the resident bytes within it: each
    failure is a ``NotImplementedError`` naming the condition.  Touches no GPU."""
    if not sign_geometry_wanted(agg):
        return False
    if not all(getattr(c.C, "compression_function", None) == "sign" for c in clients):
        return False

    def no(why: str):
        raise NotImplementedError(f"the sign-gram route (sign_geometry) needs {why}")

    cfg = getattr(agg, "aggregation_config", None) or {}
    if not all(isinstance(c.C, Compression) for c in clients):
        no("every client to be the drop-in Compression")
    if agg.num_hierarchies != 0:
        no("no hierarchies (num_hierarchies == 0)")
    if cfg.get("devices", DEFAULT_DEVICES) not in (None, 1):
        no("one device")
    w = getattr(agg.gar, "gradient_weights", None)
    if w is not None and np.asarray(w).dtype != np.float32:
        no("float32 GAR weights")
    n = None
    for c in clients:
        g = np.asarray(c.grad)
        if g.ndim != 1 or g.dtype != np.float32:
            no("1-D float32 gradients")
        if n is not None and g.shape[0] != n:
            no("gradients of one length")
        n = g.shape[0]
    if n == 0:
        no("a gradient length n > 0")
    m = len(clients)
    if m > L.FC_GRAM_MAX_M:
        no(f"at most {L.FC_GRAM_MAX_M} clients (got {m})")
    b = cfg.get("device_budget_bytes")
    if b and sign_gram_resident_bytes(n, m) > int(b):
        no(f"the round's packets to fit device_budget_bytes ({sign_gram_resident_bytes(n, m)} > "
           f"{int(b)} bytes)")
    return True


def sign_gram_round(agg, clients, n: int, dev: torch.device) -> torch.Tensor:
    """One round on the "sign-gram" route: the clients are uploaded and encoded one at a time as
    in :func:`sign_round` (with error feedback each residual advances exactly once), all M packets
    stay resident, then the "gram" route's consumers run on them (:func:`_gram_family`)."""
    m = len(clients)
    need, budget = sign_gram_resident_bytes(n, m), _budget(agg, dev)
    if need > budget:
        raise NotImplementedError("the sign-gram route (sign_geometry) needs the round's packets to "
                                  f"fit device_budget_bytes ({need} > {budget} bytes)")
    return _gram_family(agg, agg.gar, _sign_encode_resident(agg, clients, n, dev))


def _sign_encode_resident(agg, clients, n: int, dev: torch.device) -> list:
    """The round's clients uploaded and encoded one at a time into the aggregator's cached sign
    packets, all M of which stay resident (the "sign-gram" and "sign-trim" routes).  Every
    residual is checked before one advances; each then advances exactly once."""
    m = len(clients)
    for c in clients:                          # every residual checked before one advances
        if c.C.error_feedback:
            c.C._ef_buffers(n, dev, allocate=False)
    cache = agg.__dict__.setdefault("_sign_packets", {})
    slots = cache.get((n, dev))
    if slots is None or len(slots) < m:
        cache.clear()
        slots = cache[(n, dev)] = [codec.SignPacket.alloc(n, dev) for _ in range(m)]
    pk = slots[:m]
    for c, slot in zip(clients, pk):
        g = torch.from_numpy(np.ascontiguousarray(c.grad)).to(dev)
        if c.C.error_feedback:
            res, spare = c.C._ef_buffers(n, dev)
            _, new = codec.encode_sign(g, res, residual_out=spare, packet=slot)
            c.C._ef_commit(res, new, True)
        else:
            codec.encode_sign(g, packet=slot)
    return pk


def _sign_wire_upload(agg, part, dev: torch.device) -> list:
    """Validated sign payloads (``codec._sign_check``'s pairs) into one cached device slab, 256-byte
    aligned each: the packets are views of it."""
    cache = agg.__dict__.setdefault("_sign_wire", {})
    offs = np.concatenate([[0], np.cumsum([(a.size + 255) & ~255 for a, _ in part])])
    slab = cache.get("slab")
    if slab is None or slab.device != dev or slab.numel() < int(offs[-1]):
        cache.pop("slab", None)
        slab = cache["slab"] = torch.empty(int(offs[-1]), dtype=torch.uint8, device=dev)
    return [codec._sign_upload(a, h, dev, out=slab[int(o): int(o) + a.size])
            for (a, h), o in zip(part, offs)]


def sign_wire_gram_round(agg, hosts, n: int, dev: torch.device) -> torch.Tensor:
    """aggregate_wire's round of validated sign payloads under ``sign_geometry``: all uploaded,
    then the "gram" route's consumers on them (:func:`_gram_family`)."""
    total = sum((a.size + 255) & ~255 for a, _ in hosts)
    need, budget = sign_gram_resident_bytes(n, len(hosts), total), _budget(agg, dev)
    if need > budget:
        _wire_no(f"the round's sign packets to fit device_budget_bytes ({need} > {budget} bytes)")
    return _gram_family(agg, agg.gar, _sign_wire_upload(agg, hosts, dev))


# ---- the "sign-trim" route (opt-in): the coordinate-wise rules on a round of sign packets ----
def _sign_trim_no(why: str):
    raise NotImplementedError(f"the sign-trim route (sign_trim) needs {why}")


def sign_trim_wanted(agg) -> bool:
    """Is ``aggregation_config["sign_trim"]`` set and the scheme a coordinate-wise rule
    (trimmed_mean, coordinate_median)?  The key does nothing for any other scheme."""
    cfg = getattr(agg, "aggregation_config", None) or {}
    return bool(cfg.get("sign_trim", False)) and type(getattr(agg, "gar", None)) in _COORD_RULES


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


def _pc_gram(agg) -> bool:
    return getattr(agg, "analyze_pc", False) == "gram"


def sign_trim_route(agg, clients) -> bool:
    """Does this round take the "sign-trim" route?  False without the key, under a scheme that is
    no coordinate-wise rule, or when not every client compresses with 'sign' (the other routes
    decide).  Otherwise the conditions of :func:`sign_gram_route`: each failure is a
    ``NotImplementedError`` naming the condition, and a ``gradient_weights`` that is not None is
    the rules' ``ValueError``.  Touches no GPU."""
    if not sign_trim_wanted(agg):
        return False
    if not all(getattr(c.C, "compression_function", None) == "sign" for c in clients):
        return False
    no = _sign_trim_no
    cfg = getattr(agg, "aggregation_config", None) or {}
    if not all(isinstance(c.C, Compression) for c in clients):
        no("every client to be the drop-in Compression")
    if agg.num_hierarchies != 0:
        no("no hierarchies (num_hierarchies == 0)")
    if cfg.get("devices", DEFAULT_DEVICES) not in (None, 1):
        no("one device")
    if getattr(agg.gar, "gradient_weights", None) is not None:
        raise ValueError(f"{type(agg.gar).__name__} is unweighted: gradient_weights must be None")
    n = None
    for c in clients:
        g = np.asarray(c.grad)
        if g.ndim != 1 or g.dtype != np.float32:
            no("1-D float32 gradients")
        if n is not None and g.shape[0] != n:
            no("gradients of one length")
        n = g.shape[0]
    if n == 0:
        no("a gradient length n > 0")
    m = len(clients)
    if m > L.FC_GRAM_MAX_M:
        no(f"at most {L.FC_GRAM_MAX_M} clients (got {m})")
    b = cfg.get("device_budget_bytes")
    need = sign_trim_resident_bytes(n, m, _pc_gram(agg))
    if b and need > int(b):
        no(f"the round's packets to fit device_budget_bytes ({need} > {int(b)} bytes)")
    return True


def sign_trim_round(agg, clients, n: int, dev: torch.device) -> torch.Tensor:
    """One round on the "sign-trim" route: the clients are uploaded and encoded one at a time as
    in :func:`sign_gram_round` (with error feedback each residual advances exactly once), all M
    packets stay resident, then :func:`_gram_family` runs the rule on them
    (``codec.trimmed_mean_sign``; ``codec.gram_sign`` only for ``pc_analysis: "gram"``)."""
    need, budget = sign_trim_resident_bytes(n, len(clients), _pc_gram(agg)), _budget(agg, dev)
    if need > budget:
        _sign_trim_no(f"the round's packets to fit device_budget_bytes ({need} > {budget} bytes)")
    return _gram_family(agg, agg.gar, _sign_encode_resident(agg, clients, n, dev))


def sign_wire_trim_round(agg, hosts, n: int, dev: torch.device) -> torch.Tensor:
    """aggregate_wire's round of validated sign payloads under ``sign_trim``: all uploaded into
    the cached slab, then :func:`_gram_family` (the bits of :func:`sign_trim_round`)."""
    total = sum((a.size + 255) & ~255 for a, _ in hosts)
    need = sign_trim_resident_bytes(n, len(hosts), _pc_gram(agg), total)
    budget = _budget(agg, dev)
    if need > budget:
        _sign_trim_no(f"the round's sign packets to fit device_budget_bytes ({need} > {budget} bytes)")
    return _gram_family(agg, agg.gar, _sign_wire_upload(agg, hosts, dev))


def sign_wire_round(agg, hosts, n: int, dev: torch.device) -> torch.Tensor:
    """aggregate_wire's round of validated sign payloads (``hosts``: what ``codec._sign_check``
    returned for each): uploaded into one cached device slab and folded in groups
    (:func:`wire_fold_groups`, ``fed_avg``) or voted over, all resident (``sign_majority``)."""
    gar, m = agg.gar, len(hosts)
    sizes = [a.size for a, _ in hosts]
    budget = _budget(agg, dev)
    if type(gar) is SignMajority:
        total = sum((b + 255) & ~255 for b in sizes)
        if total + 4 * n > budget:
            _wire_no(f"the round's sign packets to fit device_budget_bytes ({total + 4 * n} > "
                     f"{budget} bytes): the majority vote reads every packet at once")
        groups = [range(0, m)]
        wts = None
    else:
        groups = wire_fold_groups(sizes, n, budget)
        wts = gar._weights(m, np.float32)                               # gar.py:37-42 (persisted)
    out = torch.empty(n, dtype=torch.float32, device=dev)
    for gi, g in enumerate(groups):
        pk = _sign_wire_upload(agg, hosts[g.start:g.stop], dev)
        if wts is None:
            gar.aggregate_packets(pk, out=out)
        else:
            codec.fold_sign(pk, [float(x) for x in wts[g.start:g.stop]], out=out, continue_sum=gi > 0)
    return out


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
    # Krum / pc_analysis "gram": a round outside the route's conditions raises here, before a
    # GPU is touched (no dense fallback)
    # a round of 'sign' clients: its own route, or NotImplementedError for a scheme without a
    # consumer of sign packets (before the gram route's own conditions are read)
    sign = sign_route(self, clients)
    # opt-in ("sign_geometry"): the Gram family's consumers on a round of sign packets
    sign_gram = sign_gram_route(self, clients)
    # opt-in ("sign_trim"): the coordinate-wise rules on a round of sign packets
    sign_trim = sign_trim_route(self, clients)
    k_gram = (gram_route_k(self, clients)
              if gram_wanted(self) and not sign_gram and not sign_trim else None)
    dev = _device_of(self)
    grad0 = np.asarray(clients[0].grad)
    n = grad0.shape[0]
    if any(np.asarray(c.grad).shape != (n,) for c in clients):
        raise ValueError("client gradients must share one length (aggregation.py:61)")
    if k_gram is not None:
        # the round's packets resident at once, their Gram matrix straight from them
        self.agg_path = "gram"
        self.curr_G = None
        self.agg_grad = gram_round(self, clients, n, k_gram, dev).cpu().numpy()
        return
    if sign_gram:
        # every client a scaled-sign packet, all resident: Gram matrix from the bits, then the rule
        self.agg_path = "sign-gram"
        self.curr_G = None
        self.agg_grad = sign_gram_round(self, clients, n, dev).cpu().numpy()
        return
    if sign_trim:
        # every client a scaled-sign packet, all resident: the trimmed mean straight from the bits
        self.agg_path = "sign-trim"
        self.curr_G = None
        self.agg_grad = sign_trim_round(self, clients, n, dev).cpu().numpy()
        return
    if sign:
        # every client a scaled-sign packet: encoded one at a time, folded or voted from the bits
        self.agg_path = "sign"
        self.curr_G = None
        self.agg_grad = sign_round(self, clients, n, dev).cpu().numpy()
        return
    k_ef = ef_batch_k(self, clients)
    if k_ef is not None:
        # opt-in: a round of error-feedback 'top' clients, batched (dense-fold's bits)
        self.agg_path = "ef-batch"
        self.curr_G = None
        w = self.gar._weights(len(clients), np.float32)             # gar.py:37-42 (persisted)
        self.agg_grad = ef_batch_fold(self, clients, n, k_ef, w, dev).cpu().numpy()
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
        cfg = getattr(self, "aggregation_config", None) or {}
        want_perm = bool(cfg.get("device_permutation", DEVICE_PERM))
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


def _wire_no(why: str):
    raise NotImplementedError(f"aggregate_wire needs {why}")


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
        r = (int(b) + 255) & ~255
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


def aggregate_wire(self, payloads, n: Optional[int] = None) -> None:
    """A round from the clients' wire packets (``Compression.compress_wire``; include/fedcodec.h)
    instead of their gradients: every payload is validated on the host (``fc_wire_validate``, the
    check of ``codec.wire_from_host``: ``ValueError`` with the reason, before any of the round
    reaches the GPU), uploaded, unpacked
    into slotted packets and aggregated.  Sets ``agg_grad`` (host array), ``agg_path = "wire"``
    and ``curr_G = None``.

    * ``fed_avg``: any number of payloads, folded in row order in groups sized by the device
      budget; bit-equal to the "stream" route of ``aggregate_grads`` on the same clients.
      With ``aggregation_config["wire_fold"] = True`` (default ``False``) a group's payloads are
      uploaded and folded as they are (``codec.fold_wire``): no slotted packets are reserved or
      written, the groups are :func:`wire_fold_groups` of the payload sizes, the bits are the
      same and ``agg_path = "wire-fold"``.  The key leaves the Gram family below untouched:
      those consumers read slotted packets, so they still unpack and answer ``"wire"``.
    * ``krum``, ``spectral_gram`` / ``geometric_median`` / ``centered_clip``, ``trimmed_mean`` /
      ``coordinate_median`` and
      ``pc_analysis: "gram"``: at most ``FC_GRAM_MAX_M`` payloads, all resident within the budget;
      ``codec.gram`` then ``gar.aggregate_packets`` exactly as the "gram" route does.
    * payloads that all carry the sign magic (``Compression.compress_wire`` of 'sign' clients):
      validated by ``fc_sign_wire_validate``, uploaded and folded in groups (``fed_avg``,
      ``codec.fold_sign``) or voted over, all resident (``sign_majority``), with ``agg_path =
      "wire-sign"``; the other schemes and a round that mixes the two payload kinds raise.
      With ``aggregation_config["sign_geometry"] = True`` (default absent) ``krum``, the linear
      rules and ``pc_analysis: "gram"`` take such a round too: at most ``FC_GRAM_MAX_M`` payloads,
      all resident, ``codec.gram_sign`` then the "gram" route's consumers, ``agg_path =
      "wire-sign-gram"``, the bits of ``aggregate_grads``' "sign-gram" route on the same clients.
      With ``aggregation_config["sign_trim"] = True`` (default absent) ``trimmed_mean`` and
      ``coordinate_median`` take such a round: at most ``FC_GRAM_MAX_M`` payloads, all resident,
      ``codec.trimmed_mean_sign``, ``agg_path = "wire-sign-trim"``, the bits of
      ``aggregate_grads``' "sign-trim" route on the same clients.
    Hierarchies, payloads of differing n and a round that does not fit raise
    ``NotImplementedError`` naming the condition."""
    no = _wire_no
    payloads = list(payloads)
    m = len(payloads)
    if m == 0:
        raise Exception('Client List is Empty')
    if self.analyze_pc is True:
        no("pc_analysis off or 'gram' (the randomized SVD of G is outside the hot path)")
    if self.num_hierarchies != 0:
        no("no hierarchies (num_hierarchies == 0)")
    gar = self.gar
    cfg = getattr(self, "aggregation_config", None) or {}
    kinds = [codec.is_sign_payload(raw) for raw in payloads]
    if any(kinds):
        # ---- a round of sign payloads: validated on the host, folded or voted ("wire-sign") ----
        if not all(kinds):
            no("payloads of one kind (the round mixes sign packets and 'top' wire packets)")
        geometry = sign_geometry_wanted(self)
        trim = sign_trim_wanted(self)
        if (type(gar) not in (FedAvg, SignMajority) or gram_wanted(self)) and not geometry and not trim:
            no("fed_avg or sign_majority for sign packets (Krum, the linear rules, the trim rules "
               "and pc_analysis 'gram' have no consumer of sign packets)")
        if cfg.get("devices", DEFAULT_DEVICES) not in (None, 1):
            no("one device")
        w = getattr(gar, "gradient_weights", None)
        if w is not None and type(gar) is SignMajority:
            raise ValueError("SignMajority is unweighted: gradient_weights must be None")
        if w is not None and trim:
            raise ValueError(f"{type(gar).__name__} is unweighted: gradient_weights must be None")
        if w is not None and np.asarray(w).dtype != np.float32:
            no("float32 GAR weights")
        if geometry and m > L.FC_GRAM_MAX_M:
            no(f"at most {L.FC_GRAM_MAX_M} payloads for the sign-gram route (got {m})")
        if trim and m > L.FC_GRAM_MAX_M:
            _sign_trim_no(f"at most {L.FC_GRAM_MAX_M} payloads (got {m})")
        hosts = []
        for i, raw in enumerate(payloads):
            try:
                a, h = codec._sign_check(raw)
            except ValueError as e:
                raise ValueError(f"payload {i}: {e}") from None
            hn = int(h.pkt.n)
            if n is None:
                n = hn
            if hn != int(n):
                no(f"payloads of one length n (payload {i} has n = {hn}, not {int(n)})")
            hosts.append((a, h))
        self.curr_G = None
        if geometry:
            # opt-in ("sign_geometry"): all resident, the Gram family's consumers on the bits
            total = sum((a.size + 255) & ~255 for a, _ in hosts)
            b = cfg.get("device_budget_bytes")
            if b and sign_gram_resident_bytes(int(n), m, total) > int(b):
                no(f"the round's sign packets to fit device_budget_bytes "
                   f"({sign_gram_resident_bytes(int(n), m, total)} > {int(b)} bytes)")
            self.agg_path = "wire-sign-gram"
            self.agg_grad = sign_wire_gram_round(self, hosts, int(n), _device_of(self)).cpu().numpy()
            return
        if trim:
            # opt-in ("sign_trim"): all resident, the trimmed mean straight from the bits
            total = sum((a.size + 255) & ~255 for a, _ in hosts)
            b = cfg.get("device_budget_bytes")
            need = sign_trim_resident_bytes(int(n), m, _pc_gram(self), total)
            if b and need > int(b):
                _sign_trim_no(f"the round's sign packets to fit device_budget_bytes ({need} > "
                              f"{int(b)} bytes)")
            self.agg_path = "wire-sign-trim"
            self.agg_grad = sign_wire_trim_round(self, hosts, int(n), _device_of(self)).cpu().numpy()
            return
        self.agg_path = "wire-sign"
        self.agg_grad = sign_wire_round(self, hosts, int(n), _device_of(self)).cpu().numpy()
        return
    family = gram_wanted(self)
    if not family and type(gar) is not FedAvg:
        no("the device FedAvg, Krum, spectral_gram, geometric_median, centered_clip, trimmed_mean "
           "or coordinate_median")
    if cfg.get("devices", DEFAULT_DEVICES) not in (None, 1):
        no("one device")
    w = getattr(gar, "gradient_weights", None)
    if w is not None and isinstance(gar, CoordinateTrim):
        raise ValueError(f"{type(gar).__name__} is unweighted: gradient_weights must be None")
    if w is not None and np.asarray(w).dtype != np.float32:
        no("float32 GAR weights")
    if family and m > L.FC_GRAM_MAX_M:
        no(f"at most {L.FC_GRAM_MAX_M} payloads for the gram route (got {m})")
    # ---- the host's part: every payload validated, one common n ----
    hosts, total = [], 0
    for i, raw in enumerate(payloads):
        try:
            a, h = codec._wire_check(raw)
        except ValueError as e:
            raise ValueError(f"payload {i}: {e}") from None
        hn = int(h.pkt.n)
        if n is None:
            n = hn
        if hn != int(n):
            no(f"payloads of one length n (payload {i} has n = {hn}, not {int(n)})")
        hosts.append((a, h))
        total += (a.size + 255) & ~255
    n = int(n)
    b = cfg.get("device_budget_bytes")
    if family and b and wire_resident_bytes(n, m, total, gar) > int(b):
        no(f"the round's packets to fit device_budget_bytes ({wire_resident_bytes(n, m, total, gar)}"
           f" > {int(b)} bytes)")
    # ---- the device's part ----
    dev = _device_of(self)
    self.agg_path = "wire"
    self.curr_G = None
    cache = self.__dict__.setdefault("_wire_packets", {})

    def packets_for(count: int):
        pk = cache.get((n, dev))
        if pk is None or len(pk) < count:
            for key in [k for k in cache if k != "slab"]:   # one shape at a time
                del cache[key]
            pk = cache[(n, dev)] = codec.Packet.alloc_batch(n, count, L.FC_FMT_IDXVAL, dev)
        return pk[:count]

    def upload(part):
        """The payloads of one group into one cached device slab (256-byte aligned each)."""
        offs = np.concatenate([[0], np.cumsum([(a.size + 255) & ~255 for a, _ in part])])
        slab = cache.get("slab")
        if slab is None or slab.device != dev or slab.numel() < int(offs[-1]):
            cache.pop("slab", None)
            slab = cache["slab"] = torch.empty(int(offs[-1]), dtype=torch.uint8, device=dev)
        return [codec._wire_upload(a, h, dev, out=slab[int(o): int(o) + a.size])
                for (a, h), o in zip(part, offs)]

    if family:
        need = wire_resident_bytes(n, m, total, gar)
        if need > _budget(self, dev):
            no(f"the round's packets to fit device_budget_bytes ({need} > {_budget(self, dev)} bytes)")
        wires = upload(hosts)
        pk = codec.unpack(wires, packets_for(m))
        del wires
        out = _gram_family(self, gar, pk)
    elif cfg.get("wire_fold", False):
        wts = gar._weights(m, np.float32)                           # gar.py:37-42 (persisted)
        groups = wire_fold_groups([a.size for a, _ in hosts], n, _budget(self, dev))
        self.agg_path = "wire-fold"
        out = torch.empty(n, dtype=torch.float32, device=dev)
        for gi, g in enumerate(groups):
            wires = upload(hosts[g.start:g.stop])
            codec.fold_wire(wires, wts[g.start:g.stop], out=out, continue_sum=gi > 0)
            del wires
    else:
        wts = gar._weights(m, np.float32)                           # gar.py:37-42 (persisted)
        group = wire_group(self, n, m, dev)
        out = torch.empty(n, dtype=torch.float32, device=dev)
        for gi, s in enumerate(range(0, m, group)):
            part = hosts[s:s + group]
            wires = upload(part)
            pk = codec.unpack(wires, packets_for(len(part)))
            codec.decode_accumulate(pk, [float(x) for x in wts[s:s + len(part)]], out=out,
                                    continue_sum=gi > 0)
            del wires
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
        self.agg_path = None                # "stream" | "dense-fold" | "dense" | "ef-batch" | "gram" | "sign" | "sign-gram" | "sign-trim" | "wire" | "wire-fold" | "wire-sign" | "wire-sign-gram" | "wire-sign-trim": the last call's path
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
