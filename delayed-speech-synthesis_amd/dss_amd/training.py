"""Training the two recurrent models on the GPU: the loops of the reference's train_unidirectional_vad.py:135-219 (the neural
voice-activity detector) and train_bidirectional_model.py:125-191 (the decoder).

The script trains ``UnidirectionalVoiceActivityDetector`` (2 LSTM layers, ``dropout=0.5``) with batch size 1 by truncated
backpropagation through time: a trial is cut into windows of 50 frames (``x.split(50, dim=1)``, the last one the remainder), and
every window is forward from the carried state, ``nn.CrossEntropyLoss``, ``backward()``, ``RMSprop.step()``, ``state.detach()``.
``VadTrainerGPU`` is that window as two hand-written launches (``dss_vad_trainer_window_dev``, csrc/vad_train.hip: one serial
workgroup for forward + backward through time, one launch over all gate rows for the weight gradients and the fused update) and
a trial as one call with no host synchronisation between its windows; ``train_vad`` is the epoch loop over corpora as
``dss_amd.session.session_corpus`` returns them, validating with ``dss_amd.validation.vad_validation`` on a kept inference handle
(``publish``: device to device) and keeping the best weights by ``StoreBestModel``'s rule.

Dropout masks are drawn here, from a seeded ``torch.Generator`` on the host, and handed to the kernels as (T, H) multipliers of 0
or 1 / (1 - p): a run is reproducible from its seed.  This is not torch's own random stream (``nn.LSTM``'s dropout draws inside
MIOpen / ATen); the reference's training is not reproducible across devices either.

The decoder's script trains ``BidirectionalSpeechSynthesisModel`` (2 bidirectional LSTM layers, ``dropout=0.5``) with batch size 1
and no windows: a whole trial (250-1500 frames) is forward from the zero state, ``nn.MSELoss``, ``backward()`` through the trial,
``RMSprop.step()``.  ``DecoderTrainerGPU`` is that trial as seven hand-written launches on one stream
(``dss_dec_trainer_trial_dev``, csrc/dec_train.hip); its masks are (T, 2H), over layer 0's concatenated output
(``decoder_dropout_mask``).  ``train_decoder`` is the epoch loop, validating with ``dss_amd.validation.decoder_validation`` on a kept
``BiLstmDecoderGPU`` and keeping the weights with the lowest validation loss (``StoreBestModel``).

No HDF files, tensorboard, plots, ``torchinfo`` summary or per-epoch ``.npy`` dumps are produced, and the decoder script's
vocoding of validation samples (``AsynchronousSynthesisQueue``) is not part of the loop: ``dss_amd.lpcnet.LPCNetBatch`` vocodes
the ``features`` that ``decoder_validation`` returns."""
from __future__ import annotations

import numpy as np

import ctypes as C

from . import _lib
from . import decoder as _decoder
from . import vad as _vad
from .validation import _state_dict, decoder_validation, trial_bounds, vad_validation

LR, ALPHA, EPS = 1e-4, 0.99, 1e-8          # torch.optim.RMSprop(model.parameters(), lr=0.0001): the script's line 124


def _shapes(c: int, h: int):
    h4 = 4 * h
    return [(h4, c), (h4, h), (h4,), (h4,), (h4, h), (h4, h), (h4,), (h4,), (2, h), (2,)]


def dropout_mask(n_frames: int, hidden_units: int, p: float, generator):
    """(n_frames, H) float32 multipliers of layer 0's output: 0 with probability p, else 1 / (1 - p); None for p == 0."""
    import torch
    if not 0.0 <= p < 1.0:
        raise ValueError("dropout must be in [0, 1)")
    if p == 0.0:
        return None
    keep = torch.rand((int(n_frames), int(hidden_units)), generator=generator, dtype=torch.float32) >= p
    return keep.to(torch.float32) / np.float32(1.0 - p)


class VadTrainerGPU:
    """The trainer of one detector: master parameters, RMSprop square averages and the carried (h, c) live on the device."""

    def __init__(self, module_or_state_dict, max_window: int = 50):
        sd = _state_dict(module_or_state_dict, _vad.fits, "VadTrainerGPU")
        w = [np.ascontiguousarray(sd[k].detach().cpu().numpy() if hasattr(sd[k], "detach") else sd[k], dtype=np.float32) for k in _vad._KEYS]
        h4, c = w[0].shape
        self.C, self.H, self.max_window = int(c), int(h4 // 4), int(max_window)
        self._L = L = _lib.load()
        _lib.check(L.dss_vad_trainer_check(self.C, self.H, self.max_window, 1, 1, 1))
        _lib.require_gpu()
        self._n = int(L.dss_vad_trainer_param_count(self.C, self.H))
        self._h = L.dss_vad_trainer_create(self.C, self.H, self.max_window)
        if not self._h:
            raise MemoryError(L.dss_last_error().decode())
        _lib.check(L.dss_vad_trainer_load(self._h, *[a.ctypes.data for a in w]))

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.dss_vad_trainer_destroy(self._h)
            self._h = None

    # ---- inputs ----
    def _frames(self, x):
        import torch
        x = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
        if x.dtype not in (torch.float64, torch.float32):
            raise TypeError("frames must be float64 or float32")
        if x.dim() != 2 or x.shape[1] != self.C:
            raise ValueError(f"frames must be (T, {self.C})")
        return x.cuda().contiguous()

    @staticmethod
    def _targets(y, n):
        import torch
        y = y.detach().cpu().numpy() if isinstance(y, torch.Tensor) else np.asarray(y)
        y = y.ravel()
        if len(y) != n:
            raise ValueError(f"{n} frames but {len(y)} targets")
        if y.dtype != bool and ((y != 0) & (y != 1)).any():
            raise ValueError("targets must be 0 / 1")
        return torch.from_numpy(np.ascontiguousarray(y, dtype=np.uint8)).cuda()

    def _mask(self, mask, n):
        import torch
        if mask is None:
            return None
        m = mask if isinstance(mask, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(mask))
        if tuple(m.shape) != (n, self.H):
            raise ValueError(f"the mask must be ({n}, {self.H})")
        return m.to(dtype=torch.float32).cuda().contiguous()

    # ---- steps ----
    def window(self, x, y, mask=None, step: bool = True, lr: float = LR, alpha: float = ALPHA, eps: float = EPS) -> float:
        """One window from the carried state: x (T, C) frames, y (T,) 0 / 1 targets, mask (T, H) multipliers or None.  Computes the
        loss and the gradients (``gradients()``), advances the carried state, and applies the RMSprop update if ``step``.
        Returns the loss."""
        import torch
        x = self._frames(x)
        n = int(x.shape[0])
        _lib.check(self._L.dss_vad_trainer_check(self.C, self.H, self.max_window, n, 1, 1))
        y, m = self._targets(y, n), self._mask(mask, n)
        loss = torch.empty((1,), dtype=torch.float64, device=x.device)
        _lib.check(self._L.dss_vad_trainer_window_dev(self._h, x.data_ptr(), int(x.dtype == torch.float64), n, y.data_ptr(),
                                                      m.data_ptr() if m is not None else None, int(bool(step)), float(lr), float(alpha),
                                                      float(eps), loss.data_ptr(), torch.cuda.current_stream().cuda_stream))
        return float(loss.cpu()[0])

    def train_trial(self, x, y, window: int = 50, dropout: float = 0.5, generator=None, masks=None, lr: float = LR,
                    alpha: float = ALPHA, eps: float = EPS):
        """One trial, as the script's lines 146-175: the state starts from zeros, then every window of ``window`` frames (the last
        one the remainder) is stepped, all enqueued in one call.  The dropout masks of the trial are ``masks`` ((len, H)
        multipliers) if given, else drawn with ``dropout_mask(len, H, dropout, generator)``.  Returns the per-window losses
        (float64 array)."""
        import torch
        x = self._frames(x)
        n = int(x.shape[0])
        _lib.check(self._L.dss_vad_trainer_check(self.C, self.H, self.max_window, 1, n, int(window)))
        y = self._targets(y, n)
        m = self._mask(masks if masks is not None else dropout_mask(n, self.H, dropout, generator), n)
        losses = torch.empty((-(-n // int(window)),), dtype=torch.float64, device=x.device)
        _lib.check(self._L.dss_vad_trainer_trial_dev(self._h, x.data_ptr(), int(x.dtype == torch.float64), n, y.data_ptr(),
                                                     m.data_ptr() if m is not None else None, int(window), float(lr), float(alpha),
                                                     float(eps), losses.data_ptr(), torch.cuda.current_stream().cuda_stream))
        return losses.cpu().numpy()

    # ---- what the trainer holds ----
    def _read(self, what: int) -> dict:
        flat = np.empty(self._n, np.float32)
        _lib.check(self._L.dss_vad_trainer_read(self._h, what, flat.ctypes.data))
        out, o = {}, 0
        for k, shp in zip(_vad._KEYS, _shapes(self.C, self.H)):
            cnt = int(np.prod(shp))
            out[k] = flat[o:o + cnt].reshape(shp).copy()
            o += cnt
        return out

    def gradients(self) -> dict:
        """The gradients of the last window, float32 arrays keyed by the torch names."""
        return self._read(1)

    def square_avg(self) -> dict:
        """RMSprop's square averages, keyed by the torch names."""
        return self._read(2)

    def state_dict(self) -> dict:
        """The current parameters as float32 torch tensors: loads into ``UnidirectionalVoiceActivityDetector``."""
        import torch
        return {k: torch.from_numpy(v) for k, v in self._read(0).items()}

    def state(self):
        """The carried (h, c), host float32 arrays [2][H]."""
        h = np.empty((2, self.H), np.float32)
        c = np.empty((2, self.H), np.float32)
        _lib.check(self._L.dss_vad_trainer_state(self._h, h.ctypes.data, c.ctypes.data, 0))
        return h, c

    def set_state(self, h, c):
        h = np.ascontiguousarray(h, dtype=np.float32).reshape(2, self.H)
        c = np.ascontiguousarray(c, dtype=np.float32).reshape(2, self.H)
        _lib.check(self._L.dss_vad_trainer_state(self._h, h.ctypes.data, c.ctypes.data, 1))

    def reset_state(self):
        """Zeros, as at the start of a trial; enqueued on torch's current stream."""
        import torch
        _lib.check(self._L.dss_vad_trainer_reset_state(self._h, torch.cuda.current_stream().cuda_stream))

    def publish(self, detector: "_vad.VadLstmGPU"):
        """Copy the current weights device to device into an inference handle of the same sizes (``VadLstmGPU``)."""
        import torch
        if not isinstance(detector, _vad.VadLstmGPU):
            raise TypeError("publish takes a VadLstmGPU")
        _lib.check(self._L.dss_vad_trainer_publish(self._h, detector._h, torch.cuda.current_stream().cuda_stream))


def _corpus(corpus):
    try:
        return corpus["hga_activity"], corpus["vad_labels"], corpus["trial_ids"]
    except (KeyError, TypeError, IndexError):
        return corpus.hga_activity, corpus.vad_labels, corpus.trial_ids


def train_vad(state_dict, train_corpus, valid_corpus, epochs: int = 8, window: int = 50, dropout: float = 0.5, lr: float = LR,
              seed: int = 0, columns=None, shuffle: bool = True, alpha: float = ALPHA, eps: float = EPS):
    """The script's epoch loop.  ``state_dict`` (or a module) gives the initial weights; a corpus is a mapping (or an object) with
    ``hga_activity`` (N, C), ``vad_labels`` (N,) and ``trial_ids`` (N,), as ``session_corpus`` returns it; ``columns`` is the
    optional channel selection in front of the model (``SelectElectrodesOverSpeechAreas``).

    Per epoch: the training trials in a shuffled order drawn from a generator seeded with ``seed`` (``shuffle=False``: corpus
    order), ``train_trial`` on each with masks from the same generator, then ``publish`` into one kept ``VadLstmGPU`` and
    ``vad_validation`` on the validation corpus.  The best weights are kept when the validation accuracy is strictly greater than
    every one before (``StoreBestModel``).  Returns (best state_dict, history): history[e] has ``train_loss`` (the mean over
    the epoch's windows), ``valid_loss``, ``accuracy``, ``update_steps`` (cumulative) and ``best`` (whether the epoch was kept)."""
    import torch
    from .validation import _corpus_frames
    tr = VadTrainerGPU(state_dict, max_window=window)
    x, ranges = _corpus_frames(*(_corpus(train_corpus)[i] for i in (0, 2)), columns)
    ya = _corpus(train_corpus)[1]
    ya = (ya.detach().cpu().numpy() if isinstance(ya, torch.Tensor) else np.asarray(ya)).ravel()
    if len(ya) != x.shape[0]:
        raise ValueError(f"{x.shape[0]} frames but {len(ya)} labels")
    vx, vy, vid = _corpus(valid_corpus)
    gen = torch.Generator().manual_seed(int(seed))
    detector = _vad.VadLstmGPU(1, state_dict=tr.state_dict())
    best_sd, best_acc, steps, history = None, -np.inf, 0, []
    for _ in range(int(epochs)):
        order = torch.randperm(len(ranges), generator=gen).tolist() if shuffle else list(range(len(ranges)))
        losses = []
        for k in order:
            a, n = ranges[k]
            losses.append(tr.train_trial(x[a:a + n], ya[a:a + n], window=window, dropout=dropout, generator=gen, lr=lr, alpha=alpha, eps=eps))
        losses = np.concatenate(losses) if losses else np.zeros(0)
        steps += len(losses)
        tr.publish(detector)
        v = vad_validation(detector, vx, vy, vid, columns=columns)
        keep = v["accuracy"] > best_acc                     # StoreBestModel.update: strictly greater
        if keep:
            best_acc, best_sd = v["accuracy"], tr.state_dict()
        history.append(dict(train_loss=float(losses.mean()) if len(losses) else float("nan"), valid_loss=v["loss"],
                            accuracy=v["accuracy"], update_steps=steps, best=bool(keep)))
    return (best_sd if best_sd is not None else tr.state_dict()), history



# ---- the decoder -----------------------------------------------------------------------------------------------------------------

def _dec_shapes(c: int, h: int, o: int):
    h4 = 4 * h
    return [shp for cin in (c, 2 * h) for _ in (0, 1) for shp in ((h4, cin), (h4, h), (h4,), (h4,))] + [(o, 2 * h), (o,)]


def decoder_dropout_mask(n_frames: int, hidden_units: int, p: float, generator):
    """(n_frames, 2H) float32 multipliers of layer 0's concatenated output [h_forward | h_backward]: 0 with probability p, else
    1 / (1 - p); None for p == 0."""
    return dropout_mask(n_frames, 2 * int(hidden_units), p, generator)


class DecoderTrainerGPU:
    """The trainer of one decoder: master parameters and RMSprop square averages live on the device."""

    def __init__(self, module_or_state_dict, max_frames: int = 2048):
        sd = _state_dict(module_or_state_dict, _decoder.fits, "DecoderTrainerGPU")
        w = [np.ascontiguousarray(sd[k].detach().cpu().numpy() if hasattr(sd[k], "detach") else sd[k], dtype=np.float32)
             for k in _decoder._KEYS]
        h4, c = w[0].shape
        self.C, self.H, self.O, self.max_frames = int(c), int(h4 // 4), int(w[16].shape[0]), int(max_frames)
        self._L = L = _lib.load()
        _lib.check(L.dss_dec_trainer_check(self.C, self.H, self.O, self.max_frames, 1))
        _lib.require_gpu()
        self._n = int(L.dss_dec_trainer_param_count(self.C, self.H, self.O))
        self._h = L.dss_dec_trainer_create(self.C, self.H, self.O, self.max_frames)
        if not self._h:
            raise MemoryError(L.dss_last_error().decode())
        self._last = 0
        _lib.check(L.dss_dec_trainer_load(self._h, (C.c_void_p * 18)(*[a.ctypes.data for a in w])))

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.dss_dec_trainer_destroy(self._h)
            self._h = None

    # ---- inputs ----
    def _frames(self, x):
        import torch
        x = x if isinstance(x, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(x))
        if x.dtype not in (torch.float64, torch.float32):
            raise TypeError("frames must be float64 or float32")
        if x.dim() != 2 or x.shape[1] != self.C:
            raise ValueError(f"frames must be (T, {self.C})")
        return x.cuda().contiguous()

    def _targets(self, y, n):
        import torch
        y = y if isinstance(y, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(y))
        if tuple(y.shape) != (n, self.O):
            raise ValueError(f"the targets must be ({n}, {self.O})")
        return y.to(dtype=torch.float32).cuda().contiguous()               # y_train.float() (train_bidirectional_model.py:140)

    def _mask(self, mask, n):
        import torch
        if mask is None:
            return None
        m = mask if isinstance(mask, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(mask))
        if tuple(m.shape) != (n, 2 * self.H):
            raise ValueError(f"the mask must be ({n}, {2 * self.H})")
        return m.to(dtype=torch.float32).cuda().contiguous()

    # ---- steps ----
    def trial(self, x, y, mask=None, step: bool = True, lr: float = LR, alpha: float = ALPHA, eps: float = EPS) -> float:
        """One trial from the zero state: x (T, C) frames, y (T, O) targets, mask (T, 2H) multipliers or None.  Computes the loss,
        the features (``features()``) and the gradients (``gradients()``), and applies the RMSprop update if ``step``.  Returns
        the loss."""
        return float(self._trial(x, y, mask, step, lr, alpha, eps).cpu()[0])

    def _trial(self, x, y, mask, step, lr, alpha, eps):
        import torch
        x = self._frames(x)
        n = int(x.shape[0])
        _lib.check(self._L.dss_dec_trainer_check(self.C, self.H, self.O, self.max_frames, n))
        y, m = self._targets(y, n), self._mask(mask, n)
        loss = torch.empty((1,), dtype=torch.float64, device=x.device)
        _lib.check(self._L.dss_dec_trainer_trial_dev(self._h, x.data_ptr(), int(x.dtype == torch.float64), n, y.data_ptr(),
                                                     m.data_ptr() if m is not None else None, int(bool(step)), float(lr), float(alpha),
                                                     float(eps), loss.data_ptr(), torch.cuda.current_stream().cuda_stream))
        self._last = n
        return loss

    def train_trial(self, x, y, dropout: float = 0.5, generator=None, mask=None, lr: float = LR, alpha: float = ALPHA,
                    eps: float = EPS) -> float:
        """One update step, as the script's lines 134-152.  The dropout mask is ``mask`` ((T, 2H) multipliers) if given, else drawn
        with ``decoder_dropout_mask(T, H, dropout, generator)``.  Returns the loss."""
        if mask is None:
            n = int(x.shape[0]) if hasattr(x, "shape") else len(x)
            mask = decoder_dropout_mask(n, self.H, dropout, generator)
        return self.trial(x, y, mask=mask, step=True, lr=lr, alpha=alpha, eps=eps)

    # ---- what the trainer holds ----
    def _read(self, what: int) -> dict:
        flat = np.empty(self._n, np.float32)
        _lib.check(self._L.dss_dec_trainer_read(self._h, what, flat.ctypes.data))
        out, o = {}, 0
        for k, shp in zip(_decoder._KEYS, _dec_shapes(self.C, self.H, self.O)):
            cnt = int(np.prod(shp))
            out[k] = flat[o:o + cnt].reshape(shp).copy()
            o += cnt
        return out

    def gradients(self) -> dict:
        """The gradients of the last trial, float32 arrays keyed by the torch names."""
        return self._read(1)

    def square_avg(self) -> dict:
        """RMSprop's square averages, keyed by the torch names."""
        return self._read(2)

    def state_dict(self) -> dict:
        """The current parameters as float32 torch tensors: loads into ``BidirectionalSpeechSynthesisModel``."""
        import torch
        return {k: torch.from_numpy(v) for k, v in self._read(0).items()}

    def features(self) -> np.ndarray:
        """The float32 (T, O) features the forward half of the last trial computed (with that trial's mask, before its update)."""
        if not self._last:
            raise ValueError("no trial has run on this trainer")
        out = np.empty((self._last, self.O), np.float32)
        _lib.check(self._L.dss_dec_trainer_features(self._h, self._last, out.ctypes.data))
        return out

    def publish(self, decoder: "_decoder.BiLstmDecoderGPU"):
        """Copy the current weights device to device into an inference handle of the same sizes (``BiLstmDecoderGPU``)."""
        import torch
        if not isinstance(decoder, _decoder.BiLstmDecoderGPU):
            raise TypeError("publish takes a BiLstmDecoderGPU")
        _lib.check(self._L.dss_dec_trainer_publish(self._h, decoder._h, torch.cuda.current_stream().cuda_stream))


def _dec_corpus(corpus):
    try:
        return corpus["hga_activity"], corpus["lpc_coefficients"], corpus["trial_ids"]
    except (KeyError, TypeError, IndexError):
        return corpus.hga_activity, corpus.lpc_coefficients, corpus.trial_ids


def train_decoder(state_dict, train_corpus, valid_corpus, epochs: int = 8, dropout: float = 0.5, lr: float = LR, seed: int = 0,
                  columns=None, shuffle: bool = True, alpha: float = ALPHA, eps: float = EPS, max_streams: int = 256):
    """The script's epoch loop.  ``state_dict`` (or a module) gives the initial weights; a corpus is a mapping (or an object) with
    ``hga_activity`` (N, C), ``lpc_coefficients`` (N, O) and ``trial_ids`` (N,): what ``session_corpus`` returns plus the targets;
    ``columns`` is the optional channel selection in front of the model.

    Per epoch: the training trials in a shuffled order drawn from a generator seeded with ``seed`` (``shuffle=False``: corpus
    order), ``train_trial`` on each with a mask from the same generator (the losses stay on the device until the epoch ends), then
    ``publish`` into one kept ``BiLstmDecoderGPU`` (``max_streams`` trials side by side) and ``decoder_validation`` on the
    validation corpus.  The best weights are kept when the validation loss is strictly less than every one before
    (``StoreBestModel``).  Returns (best state_dict, history): history[e] has ``train_loss`` (the mean over the epoch's trials),
    ``valid_loss``, ``update_steps`` (cumulative) and ``best`` (whether the epoch was kept)."""
    import torch
    from .validation import _corpus_frames
    hx, hy, hid = _dec_corpus(train_corpus)
    x, ranges = _corpus_frames(hx, hid, columns)
    vx, vy, vid = _dec_corpus(valid_corpus)
    vranges = trial_bounds(vid.cpu().numpy() if isinstance(vid, torch.Tensor) else vid)
    longest = max([n for _, n in ranges] + [n for _, n in vranges] + [1])
    tr = DecoderTrainerGPU(state_dict, max_frames=longest)
    y = hy if isinstance(hy, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(hy))
    if y.dim() != 2 or y.shape[0] != x.shape[0] or y.shape[1] != tr.O:
        raise ValueError(f"lpc_coefficients must be ({x.shape[0]}, {tr.O})")
    y = y.to(device=x.device, dtype=torch.float32).contiguous()
    gen = torch.Generator().manual_seed(int(seed))
    dec = _decoder.BiLstmDecoderGPU(max(1, min(len(vranges), int(max_streams))), longest, state_dict=tr.state_dict())
    best_sd, best_loss, steps, history = None, np.inf, 0, []
    for _ in range(int(epochs)):
        order = torch.randperm(len(ranges), generator=gen).tolist() if shuffle else list(range(len(ranges)))
        losses = []
        for k in order:
            a, n = ranges[k]
            m = decoder_dropout_mask(n, tr.H, dropout, gen)
            losses.append(tr._trial(x[a:a + n], y[a:a + n], m, True, lr, alpha, eps))
        losses = torch.cat(losses).cpu().numpy() if losses else np.zeros(0)
        steps += len(losses)
        tr.publish(dec)
        v = decoder_validation(dec, vx, vy, vid, columns=columns)
        keep = v["loss"] < best_loss                        # StoreBestModel.update: strictly less
        if keep:
            best_loss, best_sd = v["loss"], tr.state_dict()
        history.append(dict(train_loss=float(losses.mean()) if len(losses) else float("nan"), valid_loss=v["loss"],
                            update_steps=steps, best=bool(keep)))
    return (best_sd if best_sd is not None else tr.state_dict()), history


__all__ = ["VadTrainerGPU", "train_vad", "dropout_mask", "DecoderTrainerGPU", "train_decoder", "decoder_dropout_mask", "trial_bounds",
           "LR", "ALPHA", "EPS"]
