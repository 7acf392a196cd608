"""Training the neural voice-activity detector on the GPU: the loop of the reference's train_unidirectional_vad.py:135-219.

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
MIOpen / ATen); the reference's training is not reproducible across devices either.  No HDF files, tensorboard, plots or
``torchinfo`` summary are produced; the decoder's training (train_bidirectional_model.py) is not part of this package."""
from __future__ import annotations

import numpy as np

from . import _lib
from . import vad as _vad
from .validation import _state_dict, trial_bounds, vad_validation

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


__all__ = ["VadTrainerGPU", "train_vad", "dropout_mask", "trial_bounds", "LR", "ALPHA", "EPS"]
