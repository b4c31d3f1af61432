"""Drop-in FedAVG reduce (ftl/gradient_aggregation/gar.py:11-56) on MI355X.

``FedAvg(aggregation_config).aggregate(G, client_ids)`` keeps the reference's contract —
weights default to ``full(M, 1/M, dtype=G.dtype)``, persist across rounds and are asserted
on M (gar.py:37-42) — and computes ``np.sum(G * w[:, None], axis=0)`` (gar.py:44) in HIP
kernels with the reference's exact operation order (bit-exact):

* float32 G and float32 weights (the configured case): ``k_wsum``, fp32 products and sums;
* float64 G (after ``RandomGaussian`` with ``noise_scale == 0``, attack_models.py:105-106) or
  float64 weights (DGA's softmax / RL estimators set ``gradient_weights``,
  aggregation.py:181-198): NumPy promotes ``G * w`` to float64, so ``k_wsum64`` forms
  ``fl64(double(g) * w)`` and sums in fp64 from +0; the result is float64, as in the reference.

``aggregate_packets`` is the compressed fast path: it consumes device packets directly
(``k_decode_sparse``) so the dense M x N matrix G of aggregation.py:61 is never built; it
takes float32 weights (float64 weights go through the dense path of the Aggregator).

``Krum`` selects one client from the clients' geometry, which it reads from the M x M Gram
matrix alone (``codec.gram`` for packets, a float64 torch product for a dense G);
``gram_singular_values`` gives G's singular values from the same matrix.

``LinearRule`` is the base of the robust rules whose aggregate is linear in the rows of G,
``a * v + sum_i c_i * d_i`` (``v`` an optional dense vector the server carries): the coefficients
come from the Gram matrix ``K = G G^T``, ``b = G v`` and ``|v|^2`` alone (``codec.gram``,
``codec.dot_dense``), through three pure NumPy float64 functions (``spectral_coeffs``,
``geometric_median_coeffs``, ``centered_clip_coeffs``), and the sum is the library's row-order
float32 fold (``codec.decode_accumulate``).  ``SpectralGram`` is the analytic branch of the
reference's ``SpectralFedAvg`` (gar.py:123-134, ``fast_lr_decomposition``) restated on the
Gram, ``GeometricMedian`` the smoothed Weiszfeld iteration (RFA), ``CenteredClip`` centered
clipping (Karimireddy, He, Jaggi, ICML 2021).

``CoordinateTrim`` is the base of the coordinate-wise rules (Yin, Chen, Ramchandran, Bartlett,
ICML 2018), which are not linear in the rows: ``TrimmedMean`` drops the ``b`` smallest and
largest of every coordinate's M values and takes the float32 mean of the rest,
``CoordinateMedian`` is ``b = (M - 1) // 2``.  ``aggregate_packets`` is one kernel over the
packets (``codec.trimmed_mean``): only a column's non-zeros are ordered, no Gram matrix is
needed, no client is excluded as a whole and the rules take no weights.

``SignMajority`` is the majority vote over scaled-sign packets (``codec.vote_sign``); ``FedAvg``'s
``aggregate_packets`` folds such packets with ``codec.fold_sign``.  ``Krum`` and the linear rules
take a list of such packets too: the Gram matrix is then ``codec.gram_sign`` (exact Hamming
distances), ``G v`` is ``codec.dot_sign``, Krum's row is ``codec.decode_sign`` and the fold is
``codec.fold_sign``.  The coordinate-wise rules take them as well (``codec.trimmed_mean_sign``): a
column of such packets holds only ``-s_i`` and ``+s_i``, so its order follows from the order of
the scales and nothing is sorted per coordinate.
"""
from __future__ import annotations

from typing import Dict, Optional, Sequence

import numpy as np
import torch

from . import codec
from ._lib import FC_FMT_SIGN

_NP_OF = {torch.float32: np.float32, torch.float64: np.float64}


def _sign_round(packets) -> bool:
    """Is this a round of sign packets?  A list that mixes packet kinds raises ``TypeError``."""
    kinds = {getattr(p, "fmt", None) == FC_FMT_SIGN for p in packets}
    if len(kinds) > 1:
        raise TypeError("a round's packets must be of one kind (sign packets and idx/val packets "
                        "are mixed)")
    return kinds == {True}


class GAR:
    def __init__(self, aggregation_config: Dict):
        self.aggregation_config = aggregation_config
        self.gradient_weights = None
        self.Sigma_tracked = []
        self.alpha_tracked = []
        self.num_updates = 0

    def aggregate(self, G, client_ids=None):
        self.num_updates += 1

    def _weights(self, m: int, dtype) -> np.ndarray:
        if self.gradient_weights is None:                                  # gar.py:37-40
            self.gradient_weights = np.full(m, fill_value=1.0 / m, dtype=dtype)
        else:                                                              # gar.py:41-42
            assert len(self.gradient_weights) == m
        w = np.asarray(self.gradient_weights)
        if w.dtype not in (np.float32, np.float64):
            raise TypeError(f"gradient_weights must be float32 or float64 (got {w.dtype})")
        return w

    def _unweighted(self) -> None:
        """The check of a rule that takes no weights (CoordinateTrim, SignMajority)."""
        if self.gradient_weights is not None:
            raise ValueError(f"{type(self).__name__} is unweighted: gradient_weights must be None")

    def weighted_average(self, stacked_grad):
        """gar.py:32-46 for an (M, N) float32/float64 G (NumPy array or CUDA tensor).  The
        result has NumPy's promoted dtype of G and the weights; it is a CUDA tensor for a CUDA
        G and a NumPy array otherwise."""
        on_device = isinstance(stacked_grad, torch.Tensor)
        m = int(stacked_grad.shape[0])
        gdt = _NP_OF.get(stacked_grad.dtype) if on_device else stacked_grad.dtype
        if gdt not in (np.float32, np.float64):
            raise TypeError(f"HIP FedAVG handles float32/float64 G (got {stacked_grad.dtype})")
        w = self._weights(m, gdt)
        rdt = np.result_type(gdt, w.dtype)                                 # G * w[:, None]
        if on_device:
            G = stacked_grad
        else:
            G = torch.from_numpy(np.ascontiguousarray(stacked_grad)).cuda()
        out = codec.weighted_sum_dense(G, torch.from_numpy(np.ascontiguousarray(w)),
                                       out_dtype=torch.float64 if rdt == np.float64 else torch.float32)
        return out if on_device else out.cpu().numpy()

    def aggregate_packets(self, packets: Sequence["codec.Packet"], out=None) -> torch.Tensor:
        """FedAVG straight from device packets (no dense G): bit-equal to weighted_average on
        the G the reference would build from the same compressed rows."""
        w = self._weights(len(packets), np.float32)
        if w.dtype != np.float32:
            raise TypeError("aggregate_packets folds with float32 weights; float64 weights "
                            "promote G * w to float64 (use weighted_average on the dense G)")
        if packets and isinstance(packets[0], codec.SignPacket):           # scaled-sign packets
            return codec.fold_sign(packets, [float(x) for x in w], out=out)
        return codec.decode_accumulate(packets, [float(x) for x in w], out=out)


class FedAvg(GAR):
    def __init__(self, aggregation_config):
        GAR.__init__(self, aggregation_config=aggregation_config)

    def aggregate(self, G, client_ids=None):                               # gar.py:53-56
        return self.weighted_average(stacked_grad=G)


def gram_singular_values(gram: np.ndarray) -> np.ndarray:
    """The singular values of G from its Gram matrix ``G @ G.T``: ``sqrt(max(eigvalsh, 0))``,
    descending, float64, on the host.  A Gram that holds NaN gives an all-NaN array.  Draws
    nothing from ``np.random`` (the reference's ``randomized_svd`` does)."""
    g = np.asarray(gram, dtype=np.float64)
    if not np.all(np.isfinite(g)):
        return np.full(g.shape[0], np.nan)
    ev = np.linalg.eigvalsh(g)
    return np.sqrt(np.maximum(ev, 0.0))[::-1].copy()


class Krum(GAR):
    """Krum (Blanchard et al., NeurIPS 2017; the intent of the reference's gar.py:184-212, which
    cannot run there): the client whose summed distance to its nearest clients is smallest.

    Everything comes from the M x M Gram matrix: ``dist[i][j] = sqrt(max(0, G_ii + G_jj -
    2 G_ij))`` in float64; with ``m = int(krum_frac * M)`` (``aggregation_config["krum_frac"]``,
    default 0.3) ``score_i`` is the sum of the m smallest entries of row i, its own 0 diagonal
    included; the first client whose score is strictly below the running minimum (started at
    1e10) is selected.  A NaN score never compares below, so a client with non-finite elements
    is never chosen; if no score is below 1e10 the last client is."""

    def __init__(self, aggregation_config):
        GAR.__init__(self, aggregation_config=aggregation_config)
        self.krum_frac = aggregation_config.get("krum_frac", 0.3)
        self.selected = None
        self.scores = None

    @staticmethod
    def krum_scores(gram, krum_frac: float = 0.3) -> np.ndarray:
        g = np.asarray(gram, dtype=np.float64)
        if g.ndim != 2 or g.shape[0] != g.shape[1] or g.shape[0] == 0:
            raise ValueError("gram must be a non-empty square matrix")
        M = g.shape[0]
        m = int(krum_frac * M)
        d = np.diagonal(g)
        with np.errstate(invalid="ignore"):
            dist = np.sqrt(np.maximum(0.0, d[:, None] + d[None, :] - 2.0 * g))
        near = np.sort(dist, axis=1)[:, :max(m, 0)]           # NaN sorts last
        return np.array([float(np.sum(near[i])) for i in range(M)], dtype=np.float64)

    @staticmethod
    def select(gram, krum_frac: float = 0.3) -> int:
        """Index of the selected client (pure NumPy)."""
        scores = Krum.krum_scores(gram, krum_frac)
        best, idx = 1e10, -1
        for i, s in enumerate(scores):
            if s < best:
                best, idx = s, i
        return idx % len(scores)                               # -1: the last row

    def _pick(self, gram: np.ndarray) -> int:
        self.scores = Krum.krum_scores(gram, self.krum_frac)
        self.selected = Krum.select(gram, self.krum_frac)
        return self.selected

    def aggregate_packets(self, packets: Sequence["codec.Packet"], out=None,
                          gram: Optional[torch.Tensor] = None) -> torch.Tensor:
        """Krum straight from device packets: Gram (codec.gram, codec.gram_sign for sign packets,
        or the one given), selection, then the dense decode of the selected packet."""
        sign = _sign_round(packets)
        if gram is None:
            gram = codec.gram_sign(packets) if sign else codec.gram(packets)
        sel = self._pick(gram.cpu().numpy())
        if sign:
            return codec.decode_sign(packets[sel], out=out)
        return codec.decode(packets[sel], out=out)

    def aggregate(self, G, client_ids=None):
        """The same for a dense (M, N) G (CUDA tensor or host array): ``G.double() @
        G.double().T`` with torch on the device, then row ``selected`` of G."""
        on_device = isinstance(G, torch.Tensor)
        Gd = G if on_device else torch.from_numpy(np.ascontiguousarray(G))
        if not Gd.is_cuda:
            Gd = Gd.cuda()
        G64 = Gd.double()
        sel = self._pick((G64 @ G64.T).cpu().numpy())
        return G[sel]


# ---- rules that are linear in the rows of G: coefficients from the Gram matrix ---------------
def _check_th(adaptive_rank_th) -> None:
    if adaptive_rank_th and not 0 < adaptive_rank_th < 1:      # spectral_aggregation.py:97-99
        raise ValueError("adaptive_rank_th should be between 0 and 1")


def spectral_coeffs(K, w, n: int, rank=None, adaptive_rank_th=None, drop_top_comp: bool = False,
                    row_sums=None):
    """``(c, S)`` with ``c @ G`` the reference's ``weighted_average(fast_lr_decomposition(G))``
    (gar.py:123-134, spectral_aggregation.py:87-130) for the M x n matrix G whose Gram matrix is
    ``K``: the low-rank approximation is ``V_k^T V_k G`` with the rows of ``V`` the eigenvectors of
    K (descending), so the weighted average is ``(V_k^T V_k w) @ G``.  ``S`` are the ``rank``
    leading singular values, ``sqrt(max(eigenvalue, 0))``.  ``row_sums`` (the sums of G's rows) is
    needed with a truthy ``adaptive_rank_th`` only: the reference's total variance is
    ``sum_i (K_ii - s_i^2 / n) / (n - 1)``.  Exact eigenvectors instead of the reference's
    randomized SVD: draws nothing from ``np.random``.  Pure NumPy float64."""
    K = np.asarray(K, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    M = K.shape[0]
    if not rank or rank > min(M, n):
        rank = min(M, n)
    _check_th(adaptive_rank_th)
    lam, Q = np.linalg.eigh(K)
    lam, V = lam[::-1], Q[:, ::-1].T
    S = np.sqrt(np.maximum(lam, 0.0))[:rank].copy()
    V_k = V[:rank]
    if adaptive_rank_th:
        if row_sums is None:
            raise ValueError("adaptive_rank_th needs the row sums of G")
        s = np.asarray(row_sums, dtype=np.float64)
        total_var = float(np.sum((np.diagonal(K) - s * s / n) / (n - 1)))
        cum = np.cumsum(S ** 2 / (n - 1) / total_var)
        ar = int(np.searchsorted(cum, adaptive_rank_th))
        if ar == 0:
            if drop_top_comp:
                ar += 1
            ar += 1
        V_k = V_k[0:ar]
    if drop_top_comp:
        V_k = V_k[1:]
    return V_k.T @ (V_k @ w), S


def geometric_median_coeffs(K, alpha, iters: int = 100, tol: float = 1e-12, nu: float = 1e-6):
    """``(c, iterations)``: the smoothed Weiszfeld iteration for the ``alpha``-weighted geometric
    median of G's rows (RFA: Pillutla, Kakade, Harchaoui), run on the coefficients of the
    iterate ``z = c @ G``: ``|z - g_i|^2 = c.Kc - 2 (Kc)_i + K_ii``.  Starts from ``c = alpha``;
    ``beta_i = alpha_i / max(nu * sqrt(max K_ii), dist_i)``, ``c = beta / sum(beta)``; stops after
    ``iters`` updates or when the objective ``sum alpha_i dist_i`` decreased by less than ``tol``
    relative.  Pure NumPy float64."""
    K = np.asarray(K, dtype=np.float64)
    alpha = np.asarray(alpha, dtype=np.float64)
    d = np.diagonal(K)
    top = float(np.max(d))
    if top == 0.0:
        return alpha.copy(), 0
    nu_abs = nu * np.sqrt(top)
    c, prev, done = alpha.copy(), None, 0
    for _ in range(int(iters)):
        Kc = K @ c
        dist = np.sqrt(np.maximum(0.0, c @ Kc - 2.0 * Kc + d))
        obj = float(alpha @ dist)
        if prev is not None and prev - obj < tol * prev:
            break
        beta = alpha / np.maximum(nu_abs, dist)
        c = beta / np.sum(beta)
        prev, done = obj, done + 1
    return c, done


def centered_clip_coeffs(K, b, q: float, tau: float, iters: int = 3):
    """``(a, c)`` with ``a * v + c @ G`` the result of ``iters`` centered-clipping steps from
    ``v`` (Karimireddy, He, Jaggi, ICML 2021): ``z <- z + mean_i (g_i - z) min(1, tau / |g_i -
    z|)``, run on the coefficients of ``z = a v + c @ G`` with ``b = G v`` and ``q = |v|^2``:
    ``|g_i - z|^2 = K_ii - 2 (a b_i + (Kc)_i) + a^2 q + 2 a c.b + c.Kc``.  ``b=None`` is the zero
    start (b = 0, q = 0).  Pure NumPy float64."""
    K = np.asarray(K, dtype=np.float64)
    M = K.shape[0]
    b = np.zeros(M) if b is None else np.asarray(b, dtype=np.float64)
    d = np.diagonal(K)
    a, c = 1.0, np.zeros(M)
    for _ in range(int(iters)):
        Kc = K @ c
        d2 = d - 2.0 * (a * b + Kc) + (a * a * q + 2.0 * a * (c @ b) + c @ Kc)
        dist = np.sqrt(np.maximum(0.0, d2))
        s = np.where(dist > tau, tau / np.where(dist > tau, dist, 1.0), 1.0)
        S = float(np.sum(s))
        a, c = a * (1.0 - S / M), c * (1.0 - S / M) + s / M
    return a, c


class LinearRule(GAR):
    """A rule whose aggregate is ``carry * v + sum_i coeffs_i * d_i``.  ``aggregate_packets``
    computes the Gram matrix (unless given) and, if the rule needs it, ``codec.dot_dense``; runs
    the rule's pure coefficient function; stores ``coeffs`` (float64, length M), ``carry`` (0.0
    when no vector is carried) and ``excluded``; then folds ``coeffs.astype(float32)`` over the
    non-excluded packets in row order (``codec.decode_accumulate``), from +0 or from
    ``torch.mul(v, float32(carry))``.  The aggregate is float32.  A list of ``codec.SignPacket``
    takes ``codec.gram_sign``, ``codec.dot_sign`` and ``codec.fold_sign`` instead.

    A client whose Gram diagonal is NaN (a non-finite element) is excluded: the rule runs on the
    remaining sub-block, weights restricted (not renormalised), its coefficient is exactly 0
    and its packet is not given to the fold."""

    def __init__(self, aggregation_config):
        GAR.__init__(self, aggregation_config=aggregation_config)
        self.coeffs = None
        self.carry = 0.0
        self.excluded = []

    def aggregate(self, G, client_ids=None):
        raise NotImplementedError(f"{type(self).__name__} reads the clients' geometry from their "
                                  "packets (aggregate_packets, the Aggregator's gram route); a "
                                  "dense G is not taken")

    def _coeffs(self, K, w, packets, keep, n):
        """(coefficients of the kept clients, carry, carried vector or None)."""
        raise NotImplementedError

    def _after(self, agg: torch.Tensor) -> None:
        pass

    @staticmethod
    def _dot(packets, keep, v=None):
        """(b over the kept clients, |v|^2) from codec.dot_dense (codec.dot_sign for sign
        packets), both checked to be finite."""
        r = (codec.dot_sign if _sign_round(packets) else codec.dot_dense)(packets, v).cpu().numpy()
        b, q = r[:len(packets)][keep], float(r[len(packets)])
        if not (np.all(np.isfinite(b)) and np.isfinite(q)):
            raise ValueError("the carried vector holds a non-finite element (G v is not finite)")
        return b, q

    def aggregate_packets(self, packets: Sequence["codec.Packet"], out=None,
                          gram: Optional[torch.Tensor] = None) -> torch.Tensor:
        M = len(packets)
        sign = _sign_round(packets)
        fold = codec.fold_sign if sign else codec.decode_accumulate
        w = self._weights(M, np.float32)
        if w.dtype != np.float32:
            raise TypeError("aggregate_packets folds with float32 weights")
        if gram is None:
            gram = codec.gram_sign(packets) if sign else codec.gram(packets)
        K = gram.cpu().numpy()
        bad = np.isnan(np.diagonal(K))
        keep = np.nonzero(~bad)[0]
        if keep.size == 0:
            raise ValueError("every client holds a non-finite element: nothing to aggregate")
        c_sub, a, v = self._coeffs(K[np.ix_(keep, keep)], w[keep], packets, keep, packets[0].n)
        coeffs = np.zeros(M, dtype=np.float64)
        coeffs[keep] = c_sub
        self.coeffs, self.carry = coeffs, float(a)
        self.excluded = [int(i) for i in np.nonzero(bad)[0]]
        c32 = coeffs.astype(np.float32)
        kept = [packets[i] for i in keep]
        weights = [float(c32[i]) for i in keep]
        if v is None:
            agg = fold(kept, weights, out=out)
        else:
            a32 = float(np.float32(self.carry))
            acc = torch.mul(v, a32) if out is None else torch.mul(v, a32, out=out)
            agg = fold(kept, weights, out=acc, continue_sum=True)
        self._after(agg)
        return agg


class SpectralGram(LinearRule):
    """The analytic branch of the reference's ``SpectralFedAvg`` (``conventional_pca_aggregation``,
    gar.py:123-134): the FedAVG of the rank-truncated G, from the Gram matrix
    (:func:`spectral_coeffs`).  Config keys ``rank``, ``adaptive_rank_th`` (default -1 as in the
    reference, which a truthy value outside (0, 1) makes raise), ``drop_top_comp``.  Appends the
    singular values ``S[:rank]`` to ``Sigma_tracked``; under ``pc_analysis: "gram"`` the
    Aggregator appends all M of the whole Gram after them, two entries per round.  Draws nothing
    from ``np.random``."""

    def __init__(self, aggregation_config):
        LinearRule.__init__(self, aggregation_config=aggregation_config)
        self.rank = aggregation_config.get("rank", None)
        self.adaptive_rank_th = aggregation_config.get("adaptive_rank_th", -1)
        self.drop_top_comp = aggregation_config.get("drop_top_comp", False)
        _check_th(self.adaptive_rank_th)

    def _coeffs(self, K, w, packets, keep, n):
        s = self._dot(packets, keep)[0] if self.adaptive_rank_th else None
        c, S = spectral_coeffs(K, w, n, rank=self.rank, adaptive_rank_th=self.adaptive_rank_th,
                               drop_top_comp=self.drop_top_comp, row_sums=s)
        self.Sigma_tracked.append(S)
        return c, 0.0, None


class GeometricMedian(LinearRule):
    """The geometric median of the clients' rows (:func:`geometric_median_coeffs`).  Config keys
    ``gm_iters`` (100), ``gm_tol`` (1e-12), ``gm_nu`` (1e-6); ``iterations`` holds the count."""

    def __init__(self, aggregation_config):
        LinearRule.__init__(self, aggregation_config=aggregation_config)
        self.gm_iters = aggregation_config.get("gm_iters", 100)
        self.gm_tol = aggregation_config.get("gm_tol", 1e-12)
        self.gm_nu = aggregation_config.get("gm_nu", 1e-6)
        self.iterations = None

    def _coeffs(self, K, w, packets, keep, n):
        c, self.iterations = geometric_median_coeffs(K, w, self.gm_iters, self.gm_tol, self.gm_nu)
        return c, 0.0, None


class CenteredClip(LinearRule):
    """Centered clipping around the previous round's aggregate (:func:`centered_clip_coeffs`).
    Config keys ``cclip_tau`` (required, > 0) and ``cclip_iters`` (3).  ``v`` is the carried
    device float32 vector: None before the first round (the zero start: no dot call) and after
    ``reset()``; a round of another length or device raises instead of resetting it."""

    def __init__(self, aggregation_config):
        LinearRule.__init__(self, aggregation_config=aggregation_config)
        tau = aggregation_config.get("cclip_tau", None)
        if tau is None or isinstance(tau, bool) or not isinstance(tau, (int, float, np.floating, np.integer)) \
                or not tau > 0:
            raise ValueError(f"cclip_tau must be a number > 0 (got {tau!r})")
        self.cclip_tau = float(tau)
        self.cclip_iters = aggregation_config.get("cclip_iters", 3)
        self.v = None

    def reset(self) -> None:
        self.v = None

    def _coeffs(self, K, w, packets, keep, n):
        v = self.v
        if v is None:
            a, c = centered_clip_coeffs(K, None, 0.0, self.cclip_tau, self.cclip_iters)
            return c, 0.0, None
        dev = packets[0].words.device if _sign_round(packets) else packets[0].val.device
        if v.numel() != n or v.device != dev:
            raise ValueError(f"the carried vector has {v.numel()} elements on {v.device}; the round has "
                             f"{n} on {dev} (reset() starts over)")
        b, q = self._dot(packets, keep, v)
        a, c = centered_clip_coeffs(K, b, q, self.cclip_tau, self.cclip_iters)
        return c, a, v

    def _after(self, agg: torch.Tensor) -> None:
        self.v = agg.clone()


# ---- coordinate-wise rules: the trimmed mean and the median of every coordinate --------------
class CoordinateTrim(GAR):
    """A coordinate-wise rule (Yin, Chen, Ramchandran, Bartlett, ICML 2018): per coordinate the M
    clients' values are ordered as ``np.sort`` does, the ``trim`` smallest and largest dropped and
    the float32 mean of the rest taken (``codec.trimmed_mean``: ascending float32 sum from +0.0,
    then one division).  ``aggregate_packets`` reads the packets alone: no dense G and no Gram
    matrix; a list of ``codec.SignPacket`` takes ``codec.trimmed_mean_sign`` instead (a list that
    mixes the two kinds raises ``TypeError``).  ``trim`` holds the count used in the last round.

    The rules are unweighted and exclude no client as a whole: a ``gradient_weights`` that is not
    None raises (a DGA weight vector silently ignored would be a wrong result), and a client with
    a NaN takes part with its other coordinates."""

    def __init__(self, aggregation_config):
        GAR.__init__(self, aggregation_config=aggregation_config)
        self.trim = None

    def _trim_of(self, m: int) -> int:
        """The count b for a round of m clients."""
        raise NotImplementedError

    def aggregate(self, G, client_ids=None):
        raise NotImplementedError(f"{type(self).__name__} reads the clients' geometry from their "
                                  "packets (aggregate_packets, the Aggregator's gram route); a "
                                  "dense G is not taken")

    def aggregate_packets(self, packets: Sequence["codec.Packet"], out=None) -> torch.Tensor:
        self._unweighted()
        sign = _sign_round(packets)
        self.trim = self._trim_of(len(packets))
        if sign:
            return codec.trimmed_mean_sign(packets, self.trim, out=out)
        return codec.trimmed_mean(packets, self.trim, out=out)


class TrimmedMean(CoordinateTrim):
    """The coordinate-wise trimmed mean.  Config keys: ``trim_frac`` (default 0.1) gives
    ``b = int(trim_frac * M)``, or an integer ``trim_count`` gives b itself; both, a negative
    value or ``2 b >= M`` raise ``ValueError``."""

    def __init__(self, aggregation_config):
        CoordinateTrim.__init__(self, aggregation_config=aggregation_config)
        frac = aggregation_config.get("trim_frac", None)
        count = aggregation_config.get("trim_count", None)
        if frac is not None and count is not None:
            raise ValueError("give trim_frac or trim_count, not both")
        if count is not None:
            if isinstance(count, bool) or not isinstance(count, (int, np.integer)):
                raise ValueError(f"trim_count must be an integer (got {count!r})")
            if count < 0:
                raise ValueError(f"trim_count must not be negative (got {count})")
        else:
            frac = 0.1 if frac is None else frac
            if isinstance(frac, bool) or not isinstance(frac, (int, float, np.floating, np.integer)) \
                    or not frac >= 0:
                raise ValueError(f"trim_frac must be a number >= 0 (got {frac!r})")
        self.trim_frac = None if count is not None else float(frac)
        self.trim_count = None if count is None else int(count)

    def _trim_of(self, m: int) -> int:
        key = "trim_frac" if self.trim_count is None else "trim_count"
        b = int(self.trim_frac * m) if self.trim_count is None else self.trim_count
        if 2 * b >= m:
            raise ValueError(f"{key}={getattr(self, key)} trims {b} values at each end of {m} clients: "
                             "nothing is left (2 b must be < M)")
        return b


class CoordinateMedian(CoordinateTrim):
    """The coordinate-wise median: ``b = (M - 1) // 2``, the middle value for odd M and the
    float32 mean of the two middle values for even M."""

    def _trim_of(self, m: int) -> int:
        return (m - 1) // 2


# ---- the majority vote over scaled-sign packets -------------------------------------------------
class SignMajority(GAR):
    """signSGD with majority vote (Bernstein, Zhao, Azizzadenesheli, Anandkumar, ICLR 2019) over
    the clients' scaled-sign packets (``codec.vote_sign``): per coordinate ``-eta`` where more than
    half of the clients send a set sign bit, ``+eta`` where fewer do, ``+0.0`` on a tie.  The
    count is integer arithmetic, so the clients' order does not matter.

    ``eta`` is ``aggregation_config["majority_scale"]`` when given; otherwise the median of the
    clients' finite scales, computed in float64 on the host (``np.median``) and cast to float32
    (no finite scale raises ``ValueError``).  ``eta`` holds the value used in the last round.

    The rule is unweighted: a ``gradient_weights`` that is not None raises, as for the
    coordinate-wise rules.  It reads sign packets alone (``aggregate_packets``, the Aggregator's
    "sign" route): a dense G is not taken."""

    def __init__(self, aggregation_config):
        GAR.__init__(self, aggregation_config=aggregation_config)
        scale = aggregation_config.get("majority_scale", None)
        if scale is not None and (isinstance(scale, bool)
                                  or not isinstance(scale, (int, float, np.floating, np.integer))):
            raise ValueError(f"majority_scale must be a number (got {scale!r})")
        self.majority_scale = None if scale is None else np.float32(scale)
        self.eta = None

    def _eta_of(self, scales) -> np.float32:
        """eta for a round whose clients sent these scales."""
        if self.majority_scale is not None:
            return self.majority_scale
        s = np.asarray(scales, dtype=np.float64)
        s = s[np.isfinite(s)]
        if s.size == 0:
            raise ValueError("sign_majority: no client sent a finite scale (give majority_scale)")
        return np.float32(np.median(s))

    def aggregate(self, G, client_ids=None):
        raise NotImplementedError("SignMajority reads the clients' sign packets (aggregate_packets, "
                                  "the Aggregator's sign route); a dense G is not taken")

    def aggregate_packets(self, packets: Sequence["codec.SignPacket"], out=None) -> torch.Tensor:
        self._unweighted()
        packets = list(packets)
        if not packets or not all(isinstance(p, codec.SignPacket) for p in packets):
            raise TypeError("SignMajority votes over sign packets (codec.encode_sign)")
        scales = ([] if self.majority_scale is not None
                  else [h.p for h in codec.headers(packets)])
        self.eta = self._eta_of(scales)
        return codec.vote_sign(packets, float(self.eta), out=out)
