"""Drop-in for OpenMSFTL's ``ftl.compression.Compression`` (compression.py:8-77), on MI355X.

Same constructor keys and defaults, same ``compress(grad, layer_wise=False)`` contract:
  * 'full'              returns the caller's object itself            (compression.py:27-29)
  * 'top'               fresh array, input dtype, k = round(f*N)      (compression.py:31-37)
  * 'rand'              fresh array, input dtype                      (compression.py:39-45)
  * 'dropout-biased'    float64 result                                (compression.py:47-53)
  * 'dropout-unbiased'  float64 result, fl64(g)/p                     (compression.py:55-60)
  * 'qsgd', unknown names, layer_wise=True -> NotImplementedError at call time (:24,62,76)
  * 'sign'              opt-in, not in the reference: the scaled sign, float32 (:meth:`Compression._sign`)
  * 'qsgd' with ``"qsgd": "native"``  opt-in: the reference's commented formula (:meth:`Compression._qsgd`)
The compute runs in hand-written HIP kernels (libfedcodec.so); there is no CPU fallback.

RNG: by default ('rng': 'numpy') 'rand'/'dropout-*' draw from the process-global legacy
``np.random`` exactly as the reference (same stream consumption, same state afterwards):
'rand' calls ``np.random.permutation`` and only the index set crosses to the GPU (or, with the
opt-in key ``'device_permutation': True``, makes that very draw on the device:
openmsftl_amd/csrc/fc_perm.hip, same indices, same state afterwards); 'dropout-*'
generates ``np.random.binomial``'s own MT19937 variates on the device (jump-ahead from
``np.random.get_state()``, openmsftl_amd/csrc/fc_mt.hip) and sets the state after them.  ``'rng': 'philox'`` draws on the device instead
(Philox4x32-10 keyed by ``'seed'``, counter advanced per call) — no host RNG work, not
stream-identical to the reference (documented in DESIGN.md).

Error feedback (opt-in key ``'error_feedback': True``, 'top', 'sign' and native 'qsgd' on float32
gradients only; the reference keeps no state between calls): the object keeps on the device what its calls so far
dropped and adds it to the next gradient (:meth:`Compression._top_ef`, ``get_residual`` /
``set_residual`` / ``reset_residual``).

Inputs: 1-D float32 NumPy arrays (the reference's `client.grad`, client.py:53) or 1-D
float32 CUDA tensors (device-resident; the result is then a CUDA tensor).  float64 gradients
(what ``RandomGaussian`` with ``noise_scale == 0`` hands over, attack_models.py:105-106) run
on the float64 kernels and return float64, as the reference does; for them 'dropout-*' keeps
the reference's exact g * 0 (including -0.0).

Deliberate, documented deviations:
  * ties in 'top' are broken highest-index-first (= stable argsort reversed); the
    reference's unstable argsort leaves that choice implementation-defined;
  * none for 'dropout-*': the float64 result is g * mask (/ p) byte for byte, -0.0 for a
    dropped negative g included (round 3; it used to write +0.0).
"""
from __future__ import annotations

from typing import Dict

import numpy as np
import torch

from . import _lib as L
from . import codec


#: 'dropout-*' with the numpy RNG: draw np.random.binomial's MT19937 variates on the device
#: (bit-exact, RNG state included; openmsftl_amd/csrc/fc_mt.hip) instead of calling it
DEVICE_MT = True

#: 'rand' with the numpy RNG: draw np.random.permutation(n)[:k] on the device (bit-exact, order
#: and RNG state included; openmsftl_amd/csrc/fc_perm.hip) instead of calling it.  Opt-in: the
#: default of the config key "device_permutation"
DEVICE_PERM = False


def _valid_p(p) -> bool:
    """p the device draws accept: a real number in [0, 1] (NumPy raises for the rest)."""
    try:
        return 0.0 <= float(p) <= 1.0
    except (TypeError, ValueError):
        return False


def kept_count(fraction: float, n: int) -> int:
    """``round(f * N)`` (compression.py:34/42) and the slice semantics of ``idx[:k]``."""
    k = round(fraction * n)
    return len(range(n)[:k])


def bitmask_words(indices_or_mask: np.ndarray, n: int, is_mask: bool) -> np.ndarray:
    """Little-endian bit mask (bit i of word i//32) from an index list or a 0/1 mask."""
    words = (n + 31) // 32
    bits = np.zeros(words * 32, dtype=bool)
    if is_mask:
        bits[:n] = indices_or_mask != 0
    else:
        bits[indices_or_mask] = True
    return np.packbits(bits, bitorder="little").view(np.uint32)


class Compression:
    def __init__(self, compression_config: Dict):
        # compression.py:18-21 — verbatim keys and defaults, no validation
        self.compression_function = compression_config.get("compression_function", 'full')
        self.num_bits = compression_config.get("num_bits", 8)
        self.fraction_coordinates = compression_config.get("fraction_coordinate", 0.5)
        self.dropout_p = compression_config.get("dropout_p", 0.5)
        # extensions (optional keys; defaults = reference behaviour)
        self.rng = compression_config.get("rng", "numpy")
        self.seed = int(compression_config.get("seed", 0))
        self.device = compression_config.get("device", None)
        # 'qsgd': the reference raises NotImplementedError (compression.py:62-64); "native"
        # opts into this build's QSGD (the reference's commented formula, :65-74; num_bits as
        # the reference reads it; Philox keyed by 'seed'; parity unpinned: DESIGN.md §6)
        self.qsgd = compression_config.get("qsgd", None)
        self.device_permutation = bool(compression_config.get("device_permutation", DEVICE_PERM))
        # error feedback for 'top' (opt-in; False = the reference, which keeps no state between
        # calls): see _top_ef
        self.error_feedback = bool(compression_config.get("error_feedback", False))
        self._residual = None              # device float32[n]: what the calls so far dropped
        self._residual_spare = None        # the buffer the next call writes
        self._residual_numpy = True        # kind of the last input (get_residual's return kind)
        self._calls = 0

    # ------------------------------------------------------------------------------------
    def compress(self, grad, layer_wise=False):
        if layer_wise:
            raise NotImplementedError
        fn = self.compression_function
        if fn == 'full':
            return grad
        if fn == 'sign':
            return self._sign(grad)
        if self.error_feedback:
            if fn == 'qsgd' and self.qsgd == 'native':
                return self._qsgd(grad)
            if fn != 'top':
                raise NotImplementedError("error_feedback is built for 'top' and 'sign' only, and "
                                          f"for 'qsgd' with \"qsgd\": \"native\" (got {fn!r})")
            return self._top_ef(grad)
        if fn == 'qsgd' and self.qsgd == 'native':
            return self._qsgd(grad)
        if fn not in ('top', 'rand', 'dropout-biased', 'dropout-unbiased'):
            raise NotImplementedError          # 'qsgd' (:62-64) and unknown names (:76-77)
        L.load()                               # the HIP path is mandatory
        on_device = isinstance(grad, torch.Tensor)
        n = int(grad.shape[0])
        if fn in ('top', 'rand'):
            k = kept_count(self.fraction_coordinates, n)
            host_idx = None
            if fn == 'rand' and self.rng == 'numpy':
                if self.device_permutation and n >= 2:
                    out = self._rand_device(grad, n, k, on_device)
                    if out is not None:
                        return out
                    # the device call fell back (its word budget or a loop bound): NumPy's own
                    # call below, from the same (untouched) state
                host_idx = np.random.permutation(n)[:k]          # compression.py:43
            if n == 0:
                return grad.clone() if on_device else np.zeros_like(grad)
            g = self._to_device(grad)
            if g.dtype == torch.float64:       # float64 kernels (exact radix select / mask)
                if fn == 'top':
                    out = codec.compress_top_dense_f64(g, k)
                elif host_idx is not None:
                    mask = torch.from_numpy(bitmask_words(host_idx, n, False).view(np.int32)).to(g.device)
                    out = codec.mask_dense_f64(g, L.FC_CODEC_RAND, mask_bits=mask)
                else:
                    out = codec.compress_top_dense_f64(g, k, key_mode=L.FC_KEY_PHILOX, seed=self.seed,
                                                       offset=self._next_offset())
                return out if on_device else out.cpu().numpy()
            if fn == 'top':                    # q streamed by the compaction pass itself
                out = codec.compress_top_dense(g, k)
                return out if on_device else out.cpu().numpy()
            if host_idx is not None:
                mask = torch.from_numpy(bitmask_words(host_idx, n, False).view(np.int32)).to(g.device)
                pkt = codec.encode_mask(g, L.FC_CODEC_RAND, mask_bits=mask, fmt=L.FC_FMT_IDXVAL)
            else:
                pkt = codec.encode_top(g, k, key_mode=L.FC_KEY_PHILOX, seed=self.seed,
                                       offset=self._next_offset())
            out = codec.decode(pkt)
            return out if on_device else out.cpu().numpy()
        # dropout-* ---------------------------------------------------------------------
        p = self.dropout_p
        codec_id = L.FC_CODEC_DROPOUT_BIASED if fn == 'dropout-biased' else L.FC_CODEC_DROPOUT_UNBIASED
        host_mask = None
        if self.rng == 'numpy':
            if n > 0 and DEVICE_MT and _valid_p(p):
                # np.random.binomial(1, p, (n,))'s own MT19937 draws, made on the device
                # (fc_mt.hip), np.random left where the call leaves it
                g = self._to_device(grad)
                key, pos, has_gauss, gauss = codec.mt_state()
                R = codec.MtRound(n, 1, key, pos, g.device)
                out = codec.mask_dense_f64(g, codec_id, p=float(p), mask_bits=R.binomial(0, float(p)))
                key, pos, redraw = R.end_state()
                if not redraw:
                    codec.mt_set_state(key, pos, has_gauss, gauss)
                    return out if on_device else out.cpu().numpy()
                # NumPy would redraw one variate (~2^-52 per element): its own call below,
                # from the same (untouched) state
            host_mask = np.random.binomial(1, p, (n,))            # compression.py:51/58
        elif not (0.0 <= p <= 1.0):
            raise ValueError("p < 0, p > 1 or p is NaN")
        if n == 0:
            return (torch.zeros(0, dtype=torch.float64, device=grad.device) if on_device
                    else np.zeros(0, dtype=np.float64))
        g = self._to_device(grad)
        # the dense float64 q = g * mask (/ p) the reference returns, float32 g promoted
        # exactly (-0.0 for dropped negative g, NaN for dropped inf/NaN); the packet form of
        # these codecs is codec.encode_mask (bitmap + kept values) for device folds
        if host_mask is not None:
            mask = torch.from_numpy(bitmask_words(host_mask, n, True).view(np.int32)).to(g.device)
            out = codec.mask_dense_f64(g, codec_id, p=float(p), mask_bits=mask)
        else:
            out = codec.mask_dense_f64(g, codec_id, p=float(p), seed=self.seed,
                                       offset=self._next_offset())
        return out if on_device else out.cpu().numpy()

    # ------------------------------------------------------------------------------------
    def _top_ef(self, grad):
        """'top' with error feedback (config key ``"error_feedback": True``; not in the
        reference): the coordinates this call drops are added to the next call's gradient.

            a = fl32(grad + residual);  q = top-k of a (compression.py:31-37 on a);
            residual = +0 where q took the coordinate, a everywhere else

        in one device pass (codec.encode_top_ef).  Returns q as compress() returns it: a fresh
        array of the input's dtype and kind, the input untouched.  The residual lives on the
        device between calls: 4N bytes per Compression object (one per client, client.py:23),
        8N while a call runs (the new residual is written beside the old one, then the two
        buffers swap).  It advances on EVERY call: a caller that compresses one gradient twice
        per round (DGA does, aggregation.py:188,199 of the reference) must snapshot it with
        :meth:`get_residual` before the first call and :meth:`set_residual` it back before the
        second.  float32 gradients only; the length may not change between calls
        (:meth:`reset_residual` starts over)."""
        on_device = isinstance(grad, torch.Tensor)
        pkt = self._top_ef_packet(grad)
        if pkt is None:                            # an empty gradient
            return grad.clone() if on_device else np.zeros_like(grad)
        out = codec.decode(pkt)
        return out if on_device else out.cpu().numpy()

    def _top_ef_packet(self, grad):
        """The packet behind :meth:`_top_ef` (None for an empty gradient): the residual advances
        here, once per call, whether the caller wants the dense q or the packet's wire form."""
        L.load()
        on_device = isinstance(grad, torch.Tensor)
        g = self._to_device(grad)
        if g.dtype != torch.float32:
            raise NotImplementedError("error_feedback handles float32 gradients only "
                                      f"(got {g.dtype})")
        n = g.numel()
        if n == 0:
            return None
        if g.data_ptr() % 16:
            g = g.clone()
        res = self._residual
        if res is not None and (res.numel() != n or res.device != g.device):
            raise ValueError(f"error_feedback: gradient of {n} elements on {g.device}, residual "
                             f"of {res.numel()} on {res.device} (reset_residual() starts over)")
        if res is None:
            res = torch.zeros(n, dtype=torch.float32, device=g.device)
        spare = self._residual_spare
        if spare is None or spare.numel() != n or spare.device != g.device:
            spare = torch.empty(n, dtype=torch.float32, device=g.device)
        k = kept_count(self.fraction_coordinates, n)
        pkt, new = codec.encode_top_ef(g, res, k, residual_out=spare)
        self._residual, self._residual_spare = new, res
        self._residual_numpy = not on_device
        return pkt

    # ------------------------------------------------------------------------------------
    def _sign(self, grad):
        """'sign' (opt-in, not in the reference): the scaled sign of EF-signSGD (Karimireddy,
        Rebjock, Stich, Jaggi, ICML 2019), 1 bit per coordinate and one float32 scale:

            a = fl32(grad + residual)  (grad itself without error feedback);
            s = fl32(sum |a| / n) in float64;  q = -s where a's sign bit is set, +s elsewhere;
            residual = fl32(a - q)     (with ``"error_feedback": True`` only)

        Returns the dense q as compress() returns it: a fresh float32 array of the input's kind,
        the input untouched.  float32 gradients only.  With error feedback the residual lives on
        the device as :meth:`_top_ef`'s does (the same two buffers, ``get_residual`` /
        ``set_residual`` / ``reset_residual``) and advances on EVERY call.  A non-finite gradient
        makes s inf or NaN and poisons the residual exactly as the arithmetic above says:
        :meth:`reset_residual` starts over."""
        on_device = isinstance(grad, torch.Tensor)
        pkt = self._sign_packet(grad)
        if pkt is None:                            # an empty gradient
            return grad.clone() if on_device else np.zeros_like(grad)
        out = codec.decode_sign(pkt)
        return out if on_device else out.cpu().numpy()

    def _sign_packet(self, grad):
        """The packet behind :meth:`_sign` (None for an empty gradient): with error feedback the
        residual advances here, once per call, whether the caller wants the dense q or the wire
        form."""
        L.load()
        on_device = isinstance(grad, torch.Tensor)
        g = self._to_device(grad)
        n = g.numel()
        if n == 0:
            return None
        if g.dtype != torch.float32:
            raise NotImplementedError(f"'sign' handles float32 gradients only (got {g.dtype})")
        if g.data_ptr() % 16:
            g = g.clone()
        if not self.error_feedback:
            return codec.encode_sign(g)[0]
        res, spare = self._ef_buffers(n, g.device)
        pkt, new = codec.encode_sign(g, res, residual_out=spare)
        self._ef_commit(res, new, not on_device)
        return pkt

    def compress_wire(self, grad) -> bytes:
        """What a client sends instead of the dense ``compress(grad)``: the 'top' packet of a 1-D
        float32 gradient (NumPy array or CUDA tensor) in its wire form (include/fedcodec.h:
        encode, resolve, ``codec.pack``), as ``bytes``; for 'sign' the sign packet's wire form
        (``codec.pack_sign``), for native 'qsgd' the QSGD packet's (``codec.pack_qsgd``; the Philox
        offset advances as ``compress`` advances it).  With ``"error_feedback": True`` the
        packet is :meth:`_top_ef`'s (:meth:`_sign`'s, :meth:`_qsgd`'s) and the residual advances
        exactly as ``compress`` advances it.  ``Aggregator.aggregate_wire`` takes a round of these.  Other
        codecs raise ``NotImplementedError`` (``codec.pack`` itself takes any idx/val packet)."""
        fn = self.compression_function
        if fn == 'sign':
            pkt = self._sign_packet(grad)
            if pkt is None:
                raise ValueError("compress_wire: empty gradient")
            return codec.pack_sign(pkt).cpu().numpy().tobytes()
        if fn == 'qsgd' and self.qsgd == 'native':
            pkt = self._qsgd_packet(grad)
            if pkt is None:
                raise ValueError("compress_wire: empty gradient")
            return codec.pack_qsgd(pkt).cpu().numpy().tobytes()
        if fn != 'top':
            raise NotImplementedError("compress_wire is built for 'top' only, and for 'sign' and "
                                      f"native 'qsgd' (got {fn!r})")
        L.load()
        if self.error_feedback:
            pkt = self._top_ef_packet(grad)
            if pkt is None:
                raise ValueError("compress_wire: empty gradient")
        else:
            g = self._to_device(grad)
            if g.dtype != torch.float32:
                raise NotImplementedError(f"compress_wire handles float32 gradients only (got {g.dtype})")
            n = g.numel()
            if n == 0:
                raise ValueError("compress_wire: empty gradient")
            if g.data_ptr() % 16:
                g = g.clone()
            pkt = codec.encode_top(g, kept_count(self.fraction_coordinates, n))
        return codec.pack(pkt).tobytes()

    # the two hooks of a batch driver (aggregation's "ef-batch" route): the state advances
    # exactly once per round, in _ef_commit, and not at all when the round fails before it
    def _ef_buffers(self, n: int, device: torch.device, allocate: bool = True):
        """``(residual or zeros, spare buffer)`` for a gradient of n elements on ``device``,
        with _top_ef's validation (``allocate=False``: the validation alone); nothing is stored
        until :meth:`_ef_commit`."""
        res = self._residual
        if res is not None and (res.numel() != n or res.device != device):
            raise ValueError(f"error_feedback: gradient of {n} elements on {device}, residual "
                             f"of {res.numel()} on {res.device} (reset_residual() starts over)")
        if not allocate:
            return None
        if res is None:
            res = torch.zeros(n, dtype=torch.float32, device=device)
        spare = self._residual_spare
        if spare is None or spare.numel() != n or spare.device != device:
            spare = torch.empty(n, dtype=torch.float32, device=device)
        return res, spare

    def _ef_commit(self, res: torch.Tensor, new: torch.Tensor, numpy_kind: bool) -> None:
        """``new`` (the spare _ef_buffers handed out, now written) becomes the residual and
        ``res`` the next spare."""
        self._residual, self._residual_spare = new, res
        self._residual_numpy = numpy_kind

    def get_residual(self):
        """A copy of the error-feedback residual, of the kind of the last input (NumPy array or
        CUDA tensor); None before the first call."""
        if self._residual is None:
            return None
        return self._residual.cpu().numpy() if self._residual_numpy else self._residual.clone()

    def set_residual(self, x) -> None:
        """Replace the residual with a copy of ``x`` (1-D float32 NumPy array or tensor)."""
        on_device = isinstance(x, torch.Tensor)
        t = self._to_device(x)
        if t.dtype != torch.float32:
            raise TypeError(f"the residual is float32 (got {t.dtype})")
        if on_device or t.data_ptr() % 16:
            t = t.clone()
        self._residual, self._residual_spare = t, None
        self._residual_numpy = not on_device

    def reset_residual(self) -> None:
        """Forget the residual: the next call starts from zeros (any length)."""
        self._residual = self._residual_spare = None

    def _qsgd(self, grad):
        """compression.py:65-74 (opt-in): dense float32 result of the QSGD codec.

        With ``"error_feedback": True`` (the quantiser divides by tau, E[q] = g / tau: a
        contraction, the form EF-signSGD defines error feedback for):

            a = fl32(grad + residual);  q = QSGD of a;  residual = fl32(a - q)

        in the encode's own two passes (codec.encode_qsgd, fc_qsgd_encode_ef).  The residual lives
        on the device as :meth:`_top_ef`'s does (the same two buffers, ``get_residual`` /
        ``set_residual`` / ``reset_residual``) and advances on EVERY call, as the Philox offset
        does.  float32 gradients only; a non-finite gradient poisons the residual exactly as the
        arithmetic above says."""
        on_device = isinstance(grad, torch.Tensor)
        pkt = self._qsgd_packet(grad)
        if pkt is None:                            # an empty gradient
            return grad.clone() if on_device else np.zeros_like(grad)
        out = codec.decode_qsgd(pkt)
        return out if on_device else out.cpu().numpy()

    def _qsgd_packet(self, grad):
        """The packet behind :meth:`_qsgd` (None for an empty gradient): the Philox offset and,
        with error feedback, the residual advance here, once per call, whether the caller wants
        the dense q or the wire form."""
        L.load()
        on_device = isinstance(grad, torch.Tensor)
        g = self._to_device(grad)
        n = g.numel()
        if n == 0:
            return None
        if not self.error_feedback:
            return codec.encode_qsgd(g, int(self.num_bits), seed=self.seed, offset=self._next_offset())
        if g.dtype != torch.float32:
            raise NotImplementedError("error_feedback handles float32 gradients only "
                                      f"(got {g.dtype})")
        if g.data_ptr() % 16:
            g = g.clone()
        res, spare = self._ef_buffers(n, g.device)
        pkt, new = codec.encode_qsgd(g, int(self.num_bits), seed=self.seed, offset=self._next_offset(),
                                     residual=res, residual_out=spare)
        self._ef_commit(res, new, not on_device)
        return pkt

    def _rand_device(self, grad, n: int, k: int, on_device: bool):
        """'rand' with np.random.permutation(n)[:k] drawn on the device from np.random's state
        (fc_perm.hip), np.random left where the call leaves it; None when the device call fell
        back or the gradient is one the host path rejects (after its draw)."""
        try:
            g = self._to_device(grad)
        except (TypeError, ValueError):
            return None
        key, pos, has_gauss, gauss = codec.mt_state()
        R = codec.PermRound(n, key, pos, g.device)
        _, mask = R.permutation(k, out_mask=torch.empty((n + 31) // 32, dtype=torch.int32,
                                                        device=g.device))
        if g.dtype == torch.float64:
            out = codec.mask_dense_f64(g, L.FC_CODEC_RAND, mask_bits=mask)
        else:
            out = codec.decode(codec.encode_mask(g, L.FC_CODEC_RAND, mask_bits=mask,
                                                 fmt=L.FC_FMT_IDXVAL))
        key, pos, fallback, _ = R.end_state()
        if fallback:
            return None
        codec.mt_set_state(key, pos, has_gauss, gauss)
        return out if on_device else out.cpu().numpy()

    def _next_offset(self) -> int:
        self._calls += 1
        return self._calls

    def _to_device(self, grad) -> torch.Tensor:
        if isinstance(grad, torch.Tensor):
            if grad.dim() != 1:
                raise ValueError("compress expects a 1-D gradient (client.py:53 flat vector)")
            if grad.dtype not in (torch.float32, torch.float64):
                raise TypeError(f"HIP codec handles float32/float64 gradients (got {grad.dtype})")
            return grad.contiguous()
        a = np.asarray(grad)
        if a.ndim != 1:
            raise ValueError("compress expects a 1-D gradient (client.py:53 flat vector)")
        if a.dtype not in (np.float32, np.float64):
            raise TypeError(f"HIP codec handles float32/float64 gradients (got {a.dtype}); "
                            "see DESIGN.md §Scope")
        dev = torch.device(self.device) if self.device else torch.device("cuda")
        return torch.from_numpy(np.ascontiguousarray(a)).to(dev)
