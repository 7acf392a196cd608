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

``mask_source="device"`` (the epoch loops) or a ``DeviceMaskSource`` in place of the ``torch.Generator`` (the trainers) draws the
masks on the device instead: a stateless counter-based generator (Philox4x32-10; csrc/dropout.hip, Part 14 of include/dss_hip.h),
a mask being a pure function of (seed, draw number, shape, p).  Nothing is drawn on the host, staged or uploaded, and a model's
masks depend neither on the group it trains in nor on its place there.  It is another random stream than the host generator's,
so it is an opt-in: the default stays the host generator, bit for bit.

The decoder's script trains ``BidirectionalSpeechSynthesisModel`` (2 bidirectional LSTM layers, ``dropout=0.5``) with batch size 1
and no windows: a whole trial (250-1500 frames) is forward from the zero state, ``nn.MSELoss``, ``backward()`` through the trial,
``RMSprop.step()``.  ``DecoderTrainerGPU`` is that trial as seven hand-written launches on one stream
(``dss_dec_trainer_trial_dev``, csrc/dec_train.hip); its masks are (T, 2H), over layer 0's concatenated output
(``decoder_dropout_mask``).  ``train_decoder`` is the epoch loop, validating with ``dss_amd.validation.decoder_validation`` on a kept
``BiLstmDecoderGPU`` and keeping the weights with the lowest validation loss (``StoreBestModel``).

``DecoderGroupTrainerGPU`` steps up to 64 decoders of equal sizes in the same seven launches (the model is ``blockIdx.y``; the kernels'
bodies are the single trainer's, so every model's numbers are its bits), and ``train_decoders`` is that many ``train_decoder`` loops
in lock step: the fold loop of train_bidirectional_model.py:65-78 (``leave_one_day_out``, ``join_corpora``), seeds and learning
rates as one run.  ``VadGroupTrainerGPU`` and ``train_vads`` are the same for the detector: up to 64 detectors in one pair of launches
per window, M ``train_vad`` loops in lock step (the day split of train_unidirectional_vad.py:81-93, seeds, learning rates).

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


class _DropoutEntry(C.Structure):
    """``dss_dropout_entry`` of include/dss_hip.h."""
    _fields_ = [("d_mask", C.c_void_p), ("rows", C.c_int), ("width", C.c_int), ("seed", C.c_ulonglong), ("draw", C.c_ulonglong),
                ("p", C.c_float), ("scale", C.c_float)]


DROPOUT_MAX_ENTRIES = 64          # the entries of one launch (Part 14)


def dropout_scale(p: float) -> np.float32:
    """The multiplier of a kept element, float32 1 / (1 - p), in the bits ``dropout_mask`` has always produced (2.0 at p = 0.5)."""
    return np.float32(1.0) / np.float32(1.0 - p)


def _check_p(p):
    if not 0.0 <= p < 1.0:
        raise ValueError("dropout must be in [0, 1)")


def device_dropout_masks(entries):
    """Fill masks from the counter-based generator of Part 14, 64 per launch.  ``entries``: [(out, seed, draw, p)], ``out`` a
    contiguous float32 torch tensor (rows, width) that the mask of (seed, draw, rows, width, p) is written into.  CUDA tensors are
    filled by ``dss_dropout_masks_dev`` on torch's current stream, with no host synchronisation; CPU tensors by the library's
    scalar restatement (``dss_dropout_masks_host``: the same bits, no GPU needed).  One call takes one kind.  Empty tensors are
    skipped."""
    import torch
    L = _lib.load()
    live, cuda = [], None
    for out, seed, draw, p in entries:
        if not (isinstance(out, torch.Tensor) and out.dtype == torch.float32 and out.dim() == 2 and out.is_contiguous()):
            raise ValueError("a mask is written into a contiguous float32 tensor (rows, width)")
        if not (0 <= int(seed) < 2 ** 64 and 0 <= int(draw) < 2 ** 64):
            raise ValueError("seed and draw must be in 0 .. 2**64 - 1")
        if not 0.0 < p < 1.0:
            raise ValueError("a device mask needs 0 < dropout < 1 (dropout 0 is no mask)")
        if cuda is not None and out.is_cuda != cuda:
            raise ValueError("one call fills CUDA masks or CPU masks, not both")
        cuda = out.is_cuda
        if out.numel():
            live.append(_DropoutEntry(out.data_ptr(), int(out.shape[0]), int(out.shape[1]), int(seed), int(draw), float(p), float(dropout_scale(p))))
    if not live:
        return
    stream = None
    if cuda:
        _lib.require_gpu()
        stream = torch.cuda.current_stream().cuda_stream
    for a in range(0, len(live), DROPOUT_MAX_ENTRIES):
        chunk = live[a:a + DROPOUT_MAX_ENTRIES]
        table = (_DropoutEntry * len(chunk))(*chunk)
        _lib.check(L.dss_dropout_masks_dev(table, len(chunk), stream) if cuda else L.dss_dropout_masks_host(table, len(chunk)))


def _packed_masks(requests, device, buf=None):
    """``requests``: [(rows, width, seed, draw, p) or None].  All masks in one buffer, each at a multiple of 4 floats (so that a
    buffer aligned to 16 bytes is written in 16-byte stores), filled by one launch per 64; ``buf`` is reused when it is large
    enough.  Returns ([(rows, width) view or None], the buffer)."""
    import torch
    offsets, total = [], 0
    for r in requests:
        offsets.append(total)
        if r is not None:
            total += -(-(int(r[0]) * int(r[1])) // 4) * 4
    if buf is None or buf.numel() < total:
        buf = torch.empty((total,), dtype=torch.float32, device=device)
    views = [None if r is None else buf[o:o + int(r[0]) * int(r[1])].view(int(r[0]), int(r[1])) for r, o in zip(requests, offsets)]
    device_dropout_masks([(v, r[2], r[3], r[4]) for v, r in zip(views, requests) if r is not None])
    return views, buf


class DeviceMaskSource:
    """The dropout masks of one training run from the counter-based generator of Part 14: ``seed`` (0 <= seed < 2**64) and a
    running ``draw`` number, which starts at 0, goes up by one with every mask and may be set (to resume a run, or to draw a mask
    again).  The trainers take one wherever they take a ``torch.Generator``.  ``device="cpu"`` gives the same bits from the
    library's CPU restatement."""

    def __init__(self, seed: int = 0, device="cuda"):
        seed = int(seed)
        if not 0 <= seed < 2 ** 64:
            raise ValueError("seed must be in 0 .. 2**64 - 1")
        self.seed, self.device, self._draw = seed, device, 0

    @property
    def draw(self) -> int:
        return self._draw

    @draw.setter
    def draw(self, value):
        value = int(value)
        if not 0 <= value < 2 ** 64:
            raise ValueError("draw must be in 0 .. 2**64 - 1")
        self._draw = value

    def take(self, n: int = 1) -> int:
        """Reserve the next n draw numbers; returns the first."""
        first = self._draw
        self.draw = first + int(n)
        return first

    def mask(self, rows: int, width: int, p: float, out=None):
        """The next mask: a (rows, width) float32 tensor on the source's device (``out`` if given: contiguous float32 of that
        shape) of 0 / 1 / (1 - p) multipliers; ``draw`` goes up by one.  None for p == 0, which draws nothing."""
        import torch
        _check_p(p)
        if p == 0.0:
            return None
        rows, width = int(rows), int(width)
        if rows < 0 or width < 0:
            raise ValueError("a mask of negative size")
        if out is None:
            out = torch.empty((rows, width), dtype=torch.float32, device=self.device)
        elif tuple(out.shape) != (rows, width):
            raise ValueError(f"out must be ({rows}, {width})")
        device_dropout_masks([(out, self.seed, self._draw, p)])
        self.take()
        return out

    def masks(self, shapes, p: float):
        """Several masks in one launch (per 64), one draw each in list order: ``shapes`` is [(rows, width) or None]; a None neither
        draws nor advances and gives None.  The masks are slices of one buffer.  [None] * len(shapes) for p == 0."""
        shapes = list(shapes)
        _check_p(p)
        if p == 0.0:
            return [None] * len(shapes)
        requests = [None if s is None else (int(s[0]), int(s[1]), self.seed, self.take(), p) for s in shapes]
        return _packed_masks(requests, self.device)[0]


def dropout_mask(n_frames: int, hidden_units: int, p: float, generator):
    """(n_frames, H) float32 multipliers of layer 0's output: 0 with probability p, else 1 / (1 - p); None for p == 0.  From the
    host generator (a ``torch.Generator`` or None: a CPU tensor), or on the device from a ``DeviceMaskSource``."""
    import torch
    _check_p(p)
    if p == 0.0:
        return None
    if isinstance(generator, DeviceMaskSource):
        return generator.mask(n_frames, hidden_units, p)
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
        multipliers) if given, else drawn with ``dropout_mask(len, H, dropout, generator)``: ``generator`` is a ``torch.Generator``
        (or None) for the host's stream, or a ``DeviceMaskSource``, which draws the mask on the device.  Returns the per-window
        losses (float64 array)."""
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


def _mask_sources(mask_source, seeds):
    """None for "host" (the masks come from the seeded ``torch.Generator`` that draws the permutations), else one
    ``DeviceMaskSource`` per seed."""
    if mask_source == "host":
        return None
    if mask_source != "device":
        raise ValueError(f'mask_source must be "host" or "device", not {mask_source!r}')
    return [DeviceMaskSource(s) for s in seeds]


def train_vad(state_dict, train_corpus, valid_corpus, epochs: int = 8, window: int = 50, dropout: float = 0.5, lr: float = LR,
              seed: int = 0, columns=None, shuffle: bool = True, alpha: float = ALPHA, eps: float = EPS, mask_source: str = "host"):
    """The script's epoch loop.  ``state_dict`` (or a module) gives the initial weights; a corpus is a mapping (or an object) with
    ``hga_activity`` (N, C), ``vad_labels`` (N,) and ``trial_ids`` (N,), as ``session_corpus`` returns it; ``columns`` is the
    optional channel selection in front of the model (``SelectElectrodesOverSpeechAreas``).

    Per epoch: the training trials in a shuffled order drawn from a generator seeded with ``seed`` (``shuffle=False``: corpus
    order), ``train_trial`` on each with masks from the same generator, then ``publish`` into one kept ``VadLstmGPU`` and
    ``vad_validation`` on the validation corpus.  The best weights are kept when the validation accuracy is strictly greater than
    every one before (``StoreBestModel``).  Returns (best state_dict, history): history[e] has ``train_loss`` (the mean over
    the epoch's windows), ``valid_loss``, ``accuracy``, ``update_steps`` (cumulative) and ``best`` (whether the epoch was kept).

    ``mask_source="device"``: the permutations still come from that generator, the masks from ``DeviceMaskSource(seed)``, one
    draw per trial."""
    import torch
    from .validation import _corpus_frames
    src = _mask_sources(mask_source, [seed])
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
            losses.append(tr.train_trial(x[a:a + n], ya[a:a + n], window=window, dropout=dropout, generator=src[0] if src else gen, lr=lr, alpha=alpha,
                                         eps=eps))
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
        with ``decoder_dropout_mask(T, H, dropout, generator)``: ``generator`` is a ``torch.Generator`` (or None) for the host's
        stream, or a ``DeviceMaskSource``, which draws the mask on the device.  Returns the loss."""
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
                  columns=None, shuffle: bool = True, alpha: float = ALPHA, eps: float = EPS, max_streams: int = 256,
                  mask_source: str = "host"):
    """The script's epoch loop.  ``state_dict`` (or a module) gives the initial weights; a corpus is a mapping (or an object) with
    ``hga_activity`` (N, C), ``lpc_coefficients`` (N, O) and ``trial_ids`` (N,): what ``session_corpus`` returns plus the targets;
    ``columns`` is the optional channel selection in front of the model.

    Per epoch: the training trials in a shuffled order drawn from a generator seeded with ``seed`` (``shuffle=False``: corpus
    order), ``train_trial`` on each with a mask from the same generator (the losses stay on the device until the epoch ends), then
    ``publish`` into one kept ``BiLstmDecoderGPU`` (``max_streams`` trials side by side) and ``decoder_validation`` on the
    validation corpus.  The best weights are kept when the validation loss is strictly less than every one before
    (``StoreBestModel``).  Returns (best state_dict, history): history[e] has ``train_loss`` (the mean over the epoch's trials),
    ``valid_loss``, ``update_steps`` (cumulative) and ``best`` (whether the epoch was kept).

    ``mask_source="device"``: the permutations still come from that generator, the masks from ``DeviceMaskSource(seed)``, one
    draw per trial."""
    import torch
    from .validation import _corpus_frames
    src = _mask_sources(mask_source, [seed])
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
            m = decoder_dropout_mask(n, tr.H, dropout, src[0] if src else gen)
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




# ---- several decoders at once ------------------------------------------------------------------------------------------------------

class _GroupTrial(C.Structure):
    """``dss_dec_group_trial`` of include/dss_hip.h."""
    _fields_ = [("d_frames", C.c_void_p), ("T", C.c_int), ("d_targets", C.c_void_p), ("d_mask", C.c_void_p), ("apply_step", C.c_int),
                ("lr", C.c_double), ("alpha", C.c_double), ("eps", C.c_double)]


def _per_model(v, n, what):
    """A scalar for every model, or one entry per model."""
    if np.ndim(v) == 0:
        return [float(v)] * n
    v = list(v)
    if len(v) != n:
        raise ValueError(f"{what}: {len(v)} entries for {n} models")
    return [float(e) for e in v]


def _group_trial_list(group, frames, ranges, models):
    """The arguments of a group's ``forward_trials_torch``, checked: (contiguous frames, first int64, len int32, model int32, sum
    len).  The model indices are left to the library, which names the trial of a bad one."""
    import torch
    from .validation import _ranges
    if frames.dtype not in (torch.float64, torch.float32):
        raise TypeError("frames must be float64 or float32")
    if frames.dim() != 2 or frames.shape[1] != group.C or not frames.is_cuda:
        raise ValueError(f"frames must be a CUDA tensor of shape (N, {group.C})")
    first, length, total = _ranges(group._L, int(frames.shape[0]), ranges)
    model = np.ascontiguousarray(np.asarray(models, dtype=np.int64).ravel())
    if len(model) != len(first):
        raise ValueError(f"{len(model)} model indices for {len(first)} trials")
    if len(model) and (model.min() < -2 ** 31 or model.max() >= 2 ** 31):
        raise ValueError("a model index must fit 32 bits")
    return frames.contiguous(), first, length, model.astype(np.int32), total


class _MaskStage:
    """A group step's host masks on their way to the device: one page-locked buffer and one copy per step.  Two buffers take
    turns, each guarded by an event behind its copy, so filling the next step's masks does not wait for the step in flight."""

    def __init__(self):
        self._stage, self._stage_ev, self._stage_k, self._dev_masks = [None, None], [None, None], 0, None

    def upload(self, host, device):
        """``host``: [(m, float32 CPU tensor)]; returns {m: flat device tensor}."""
        import torch
        total = sum(t.numel() for _, t in host)
        k = self._stage_k
        self._stage_k = 1 - k
        if self._stage_ev[k] is not None:
            self._stage_ev[k].synchronize()
        if self._stage[k] is None or self._stage[k].numel() < total:
            self._stage[k] = torch.empty((total,), dtype=torch.float32).pin_memory()
        if self._dev_masks is None or self._dev_masks.numel() < total:
            self._dev_masks = torch.empty((total,), dtype=torch.float32, device=device)
        out, o = {}, 0
        for m, t in host:
            n = t.numel()
            self._stage[k][o:o + n].copy_(t.reshape(-1))
            out[m] = self._dev_masks[o:o + n]
            o += n
        self._dev_masks[:total].copy_(self._stage[k][:total], non_blocking=True)
        ev = self._stage_ev[k] = self._stage_ev[k] or torch.cuda.Event()
        ev.record()
        return out


class DecoderGroupTrainerGPU:
    """The trainers of M decoders of equal sizes, stepped together: one trial for each model in ONE set of ``DecoderTrainerGPU``'s
    seven launches, with the model as ``blockIdx.y`` (``dss_dec_group_step_dev``, csrc/dec_train.hip), so the serial chains of all
    models run side by side on different compute units.  Every model's numbers are bit for bit those of a ``DecoderTrainerGPU``
    with the same weights given the same trials in the same order.  1 <= M <= 64; more models are more groups."""

    def __init__(self, state_dicts, max_frames: int = 2048):
        state_dicts = list(state_dicts)
        ws = []
        for sd in state_dicts:
            sd = _state_dict(sd, _decoder.fits, "DecoderGroupTrainerGPU")
            ws.append([np.ascontiguousarray(sd[k].detach().cpu().numpy() if hasattr(sd[k], "detach") else sd[k], dtype=np.float32)
                       for k in _decoder._KEYS])
        self._L = L = _lib.load()
        self.M, self.max_frames = len(ws), int(max_frames)
        if not ws:
            _lib.check(L.dss_dec_group_check(0, 1, 1, 1, self.max_frames))
        h4, c = ws[0][0].shape
        self.C, self.H, self.O = int(c), int(h4 // 4), int(ws[0][16].shape[0])
        shapes = [tuple(a.shape) for a in ws[0]]
        for m, w in enumerate(ws):
            if [tuple(a.shape) for a in w] != shapes:
                raise ValueError(f"DecoderGroupTrainerGPU: model {m} has other sizes than model 0 (one group, one size)")
        _lib.check(L.dss_dec_group_check(self.M, self.C, self.H, self.O, self.max_frames))
        _lib.require_gpu()
        self._n = int(L.dss_dec_trainer_param_count(self.C, self.H, self.O))
        self._h = L.dss_dec_group_create(self.M, self.C, self.H, self.O, self.max_frames)
        if not self._h:
            raise MemoryError(L.dss_last_error().decode())
        self._last = [0] * self.M
        self._mask_stage = _MaskStage()
        for m, w in enumerate(ws):
            _lib.check(L.dss_dec_group_load(self._h, m, (C.c_void_p * 18)(*[a.ctypes.data for a in w])))

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.dss_dec_group_destroy(self._h)
            self._h = None

    def __len__(self):
        return self.M

    def _member(self, m):
        m = int(m)
        if not 0 <= m < self.M:
            raise IndexError(f"model {m} of a group of {self.M}")
        return m

    def step(self, xs, ys, masks=None, apply: bool = True, lr=LR, alpha=ALPHA, eps=EPS, losses=None):
        """One step: model m runs the trial ``xs[m]`` (T_m, C) frames / ``ys[m]`` (T_m, O) targets / ``masks[m]`` (T_m, 2H)
        multipliers or None, from the zero state, as ``DecoderTrainerGPU.trial`` would; ``xs[m] is None``: the model sits out and
        nothing of it changes.  All frames of a step have one dtype.  ``lr``, ``alpha``, ``eps``: a scalar or one per model.
        Returns the device tensor of M float64 losses: ``losses`` if given (a CUDA float64 tensor of M entries), else a new one
        filled with NaN; the entries of models that sat out are not written.  Nothing synchronises with the host: steps may be
        enqueued back to back."""
        import torch
        M = self.M
        xs, ys = list(xs), list(ys)
        masks = [None] * M if masks is None else list(masks)
        for what, seq in (("xs", xs), ("ys", ys), ("masks", masks)):
            if len(seq) != M:
                raise ValueError(f"{what}: {len(seq)} entries for {M} models")
        lrs, alphas, epss = (_per_model(v, M, w) for v, w in ((lr, "lr"), (alpha, "alpha"), (eps, "eps")))
        table = (_GroupTrial * M)()
        keep, host_masks, dtype, device = [], [], None, None
        for m in range(M):
            if xs[m] is None:
                continue
            x = xs[m] if isinstance(xs[m], torch.Tensor) else torch.from_numpy(np.ascontiguousarray(xs[m]))
            if x.dtype not in (torch.float64, torch.float32):
                raise TypeError("frames must be float64 or float32")
            if x.dim() != 2 or x.shape[1] != self.C:
                raise ValueError(f"model {m}: frames must be (T, {self.C})")
            if dtype is not None and x.dtype != dtype:
                raise TypeError("the frames of one step must have one dtype")
            dtype = x.dtype
            n = int(x.shape[0])
            if not 1 <= n <= self.max_frames:
                raise ValueError(f"model {m}: a trial of {n} frames: must be 1 .. max_frames = {self.max_frames}")
            x = x.cuda().contiguous()
            device = x.device
            y = ys[m] if isinstance(ys[m], torch.Tensor) else torch.from_numpy(np.ascontiguousarray(ys[m]))
            if tuple(y.shape) != (n, self.O):
                raise ValueError(f"model {m}: the targets must be ({n}, {self.O})")
            y = y.to(dtype=torch.float32).cuda().contiguous()
            k = masks[m]
            if k is not None:
                k = k if isinstance(k, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(k))
                if tuple(k.shape) != (n, 2 * self.H):
                    raise ValueError(f"model {m}: the mask must be ({n}, {2 * self.H})")
                k = k.to(dtype=torch.float32).contiguous()
                if not k.is_cuda:
                    host_masks.append((m, k))
            keep += [x, y, k]
            table[m] = _GroupTrial(x.data_ptr(), n, y.data_ptr(), k.data_ptr() if k is not None and k.is_cuda else None,
                                   int(bool(apply)), lrs[m], alphas[m], epss[m])
        if dtype is None:
            raise ValueError("every model sits out: a step needs at least one trial")
        if host_masks:
            for m, k in self._mask_stage.upload(host_masks, device).items():
                table[m].d_mask = k.data_ptr()
        if losses is None:
            losses = torch.full((M,), float("nan"), dtype=torch.float64, device=device)
        elif not (isinstance(losses, torch.Tensor) and losses.is_cuda and losses.dtype == torch.float64 and losses.is_contiguous()
                  and tuple(losses.shape) == (M,)):
            raise ValueError(f"losses must be a contiguous CUDA float64 tensor of {M} entries")
        _lib.check(self._L.dss_dec_group_step_dev(self._h, table, int(dtype == torch.float64), losses.data_ptr(),
                                                  torch.cuda.current_stream().cuda_stream))
        for m in range(M):
            if table[m].T:
                self._last[m] = int(table[m].T)
        return losses

    # ---- what the group holds, per model ----
    def _read(self, m: int, what: int) -> dict:
        flat = np.empty(self._n, np.float32)
        _lib.check(self._L.dss_dec_group_read(self._h, self._member(m), what, flat.ctypes.data))
        out, o = {}, 0
        for k, shp in zip(_decoder._KEYS, _dec_shapes(self.C, self.H, self.O)):
            cnt = int(np.prod(shp))
            out[k] = flat[o:o + cnt].reshape(shp).copy()
            o += cnt
        return out

    def gradients(self, m: int) -> dict:
        """The gradients of model m's last trial, float32 arrays keyed by the torch names."""
        return self._read(m, 1)

    def square_avg(self, m: int) -> dict:
        """Model m's RMSprop square averages."""
        return self._read(m, 2)

    def state_dict(self, m: int) -> dict:
        """Model m's current parameters as float32 torch tensors."""
        import torch
        return {k: torch.from_numpy(v) for k, v in self._read(m, 0).items()}

    def features(self, m: int) -> np.ndarray:
        """The float32 (T, O) features of the forward half of model m's last trial."""
        m = self._member(m)
        if not self._last[m]:
            raise ValueError(f"no trial has run on model {m}")
        out = np.empty((self._last[m], self.O), np.float32)
        _lib.check(self._L.dss_dec_group_features(self._h, m, self._last[m], out.ctypes.data))
        return out

    def forward_trials_torch(self, frames, ranges, models, max_rows: int = 0):
        """The members' decoders on a trial list in one set of launches (``dss_dec_group_forward_trials_dev``): as
        ``BiLstmDecoderGPU.forward_trials_torch`` with one model index per range -- trial i runs on member ``models[i]``'s current
        weights, in stream order behind the steps enqueued so far, with nothing published and nothing of the members written.
        ``max_rows`` (0: the default) bounds the rows of the two layer buffers; a longer list runs in several sets of launches.
        Returns float32 CUDA features (sum len, n_outputs) in list order, a trial's bits those of a ``BiLstmDecoderGPU`` holding
        that member's weights."""
        import torch
        frames, first, length, model, total = _group_trial_list(self, frames, ranges, models)
        feats = torch.empty((total, self.O), dtype=torch.float32, device=frames.device)
        _lib.check(self._L.dss_dec_group_forward_trials_dev(self._h, frames.data_ptr(), int(frames.dtype == torch.float64), int(frames.shape[0]),
                                                            len(first), first.ctypes.data, length.ctypes.data, model.ctypes.data, int(max_rows),
                                                            feats.data_ptr(), torch.cuda.current_stream().cuda_stream))
        return feats

    def publish(self, m: int, decoder: "_decoder.BiLstmDecoderGPU"):
        """Copy model m's current weights device to device into an inference handle of the same sizes."""
        import torch
        if not isinstance(decoder, _decoder.BiLstmDecoderGPU):
            raise TypeError("publish takes a BiLstmDecoderGPU")
        _lib.check(self._L.dss_dec_group_publish(self._h, self._member(m), decoder._h, torch.cuda.current_stream().cuda_stream))


def lockstep_schedule(orders):
    """The steps of one epoch of several training runs in lock step: ``orders[m]`` is model m's trial order; step k holds every
    model's k-th trial, and None for the models whose trials have run out.  [[trial or None] * M] * max(len(order))."""
    orders = [list(o) for o in orders]
    return [[o[k] if k < len(o) else None for o in orders] for k in range(max([len(o) for o in orders] + [0]))]


def _group_epoch(step, gens, n_trials, lengths, hidden_units, dropout, shuffle, sources=None, mask_fn=None, mask_width=None):
    """One epoch of M runs in lock step.  Model m's generator ``gens[m]`` draws what ``train_decoder``'s generator draws in an
    epoch, in its order: the permutation of its ``n_trials[m]`` trials first, then the mask of each trial as its turn comes
    (``lengths[m][trial]`` frames).  ``step(trials, masks)`` gets, per step, every model's trial index (or None) and mask (or
    None) and returns the step's losses.  Returns ([per step: trials], [per step: what step returned]).

    With ``sources`` (one ``DeviceMaskSource`` per model) the generators draw the permutations only: a step's masks are one entry
    table and one launch into one device buffer, each mask at a multiple of 4 floats, model m's from ``sources[m]``'s next draw (a
    model that sits the step out draws nothing), and ``step`` gets the slices -- nothing is staged or uploaded.  One buffer
    serves every step: the launch that refills it is queued behind the step that read it, on the same stream.

    ``mask_fn(frames, hidden_units, dropout, generator)`` draws a host mask and ``mask_width`` is a device mask's width: the
    decoder's by default (``decoder_dropout_mask``, 2H); the detector's loop passes ``dropout_mask`` and H."""
    import torch
    _check_p(dropout)
    mask_fn = decoder_dropout_mask if mask_fn is None else mask_fn
    mask_width = 2 * int(hidden_units) if mask_width is None else int(mask_width)
    orders = [torch.randperm(n, generator=g).tolist() if shuffle else list(range(n)) for n, g in zip(n_trials, gens)]
    steps, out, buf = lockstep_schedule(orders), [], None
    for trials in steps:
        if sources is None:
            masks = [None if k is None else mask_fn(lengths[m][k], hidden_units, dropout, gens[m]) for m, k in enumerate(trials)]
        elif dropout == 0.0:
            masks = [None] * len(trials)
        else:
            requests = [None if k is None else (lengths[m][k], mask_width, sources[m].seed, sources[m].take(), dropout)
                        for m, k in enumerate(trials)]
            masks, buf = _packed_masks(requests, sources[0].device, buf)
        out.append(step(trials, masks))
    return steps, out


def train_decoders(state_dicts, train_corpora, valid_corpora, epochs: int = 8, dropout: float = 0.5, lr=LR, seeds=None, columns=None,
                   shuffle: bool = True, alpha: float = ALPHA, eps: float = EPS, max_streams: int = 256, mask_source: str = "host",
                   group_validation: bool = False):
    """M ``train_decoder`` loops in lock step on one ``DecoderGroupTrainerGPU``: the folds of train_bidirectional_model.py:65-68,
    seeds or learning rates as one run.  ``state_dicts[m]``, ``train_corpora[m]``, ``valid_corpora[m]`` and ``seeds[m]`` (default
    0 .. M - 1) are model m's arguments of ``train_decoder``; ``lr`` is a scalar or one per model; ``columns`` is shared.

    Model m owns a generator seeded with ``seeds[m]`` that draws its epoch's permutation and then its masks exactly as
    ``train_decoder`` does, and step k of an epoch runs every model's k-th trial, models with fewer trials sitting out the rest of
    the epoch: every model's history and best weights are those of ``train_decoder`` run alone with its seed and corpora, bit
    for bit.  After an epoch each model is published into one kept ``BiLstmDecoderGPU`` and validated on its own corpus.
    Returns [(best state_dict, history)], one pair per model.

    ``mask_source="device"``: the permutations still come from those generators; model m's masks come from
    ``DeviceMaskSource(seeds[m])``, one draw per trial stepped, all masks of a step from one launch -- again what
    ``train_decoder(..., mask_source="device", seed=seeds[m])`` computes alone, bit for bit.

    ``group_validation=True``: the validation corpora go to the device once, before the first epoch (``GroupValidationSet``), and
    an epoch's M publish + validate calls become one ``decoder_validation_group`` call on the trainers' own weights; histories and
    best weights are the same, bit for bit."""
    import torch
    from .validation import GroupValidationSet, _corpus_frames, decoder_validation_group
    state_dicts, train_corpora, valid_corpora = list(state_dicts), list(train_corpora), list(valid_corpora)
    M = len(state_dicts)
    seeds = list(range(M)) if seeds is None else list(seeds)
    for what, seq in (("train_corpora", train_corpora), ("valid_corpora", valid_corpora), ("seeds", seeds)):
        if len(seq) != M:
            raise ValueError(f"{what}: {len(seq)} entries for {M} models")
    lrs = _per_model(lr, M, "lr")
    sources = _mask_sources(mask_source, seeds)
    xs, ys, ranges, valid, longest = [], [], [], [], 1
    for m in range(M):
        hx, hy, hid = _dec_corpus(train_corpora[m])
        x, r = _corpus_frames(hx, hid, columns)
        vx, vy, vid = _dec_corpus(valid_corpora[m])
        vr = trial_bounds(vid.cpu().numpy() if isinstance(vid, torch.Tensor) else vid)
        longest = max([longest] + [n for _, n in r] + [n for _, n in vr])
        xs.append(x); ranges.append(r); valid.append((vx, vy, vid, len(vr)))
        ys.append(hy if isinstance(hy, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(hy)))
    if len({x.dtype for x in xs}) > 1:
        xs = [x.double() for x in xs]
    tr = DecoderGroupTrainerGPU(state_dicts, max_frames=longest)
    for m in range(M):
        if ys[m].dim() != 2 or ys[m].shape[0] != xs[m].shape[0] or ys[m].shape[1] != tr.O:
            raise ValueError(f"model {m}: lpc_coefficients must be ({xs[m].shape[0]}, {tr.O})")
        ys[m] = ys[m].to(device=xs[m].device, dtype=torch.float32).contiguous()
    gens = [torch.Generator().manual_seed(int(s)) for s in seeds]
    dec = _decoder.BiLstmDecoderGPU(max(1, min(max(v[3] for v in valid), int(max_streams))), longest, state_dict=tr.state_dict(0))
    lengths = [[n for _, n in r] for r in ranges]
    vset = GroupValidationSet(valid_corpora, "decoder", columns) if group_validation else None

    def step(trials, masks):
        sl = [None if k is None else slice(ranges[m][k][0], ranges[m][k][0] + ranges[m][k][1]) for m, k in enumerate(trials)]
        return tr.step([None if s is None else xs[m][s] for m, s in enumerate(sl)], [None if s is None else ys[m][s] for m, s in enumerate(sl)],
                       masks, True, lrs, alpha, eps)

    best = [(None, np.inf)] * M
    n_steps, history = [0] * M, [[] for _ in range(M)]
    for _ in range(int(epochs)):
        steps, losses = _group_epoch(step, gens, [len(r) for r in ranges], lengths, tr.H, dropout, shuffle, sources)
        losses = torch.stack(losses).cpu().numpy() if losses else np.zeros((0, M))     # the losses stay on the device until here
        vs = decoder_validation_group(tr, vset) if group_validation else None
        for m in range(M):
            mine = np.array([losses[k, m] for k, trials in enumerate(steps) if trials[m] is not None])
            n_steps[m] += len(mine)
            if group_validation:
                v = vs[m]
            else:
                tr.publish(m, dec)
                vx, vy, vid, _ = valid[m]
                v = decoder_validation(dec, vx, vy, vid, columns=columns)
            keep = v["loss"] < best[m][1]                   # StoreBestModel.update: strictly less
            if keep:
                best[m] = (tr.state_dict(m), v["loss"])
            history[m].append(dict(train_loss=float(mine.mean()) if len(mine) else float("nan"), valid_loss=v["loss"],
                                   update_steps=n_steps[m], best=bool(keep)))
    return [(best[m][0] if best[m][0] is not None else tr.state_dict(m), history[m]) for m in range(M)]


# ---- several detectors at once -----------------------------------------------------------------------------------------------------

class _VadGroupTrial(C.Structure):
    """``dss_vad_group_trial`` of include/dss_hip.h."""
    _fields_ = [("d_frames", C.c_void_p), ("d_targets", C.c_void_p), ("d_mask", C.c_void_p), ("d_losses", C.c_void_p),
                ("lr", C.c_double), ("alpha", C.c_double), ("eps", C.c_double), ("len", C.c_int), ("apply_step", C.c_int)]


class VadGroupTrainerGPU:
    """The trainers of M detectors of equal sizes, stepped together: one window for each model in ONE pair of ``VadTrainerGPU``'s
    launches, with the model as ``blockIdx.y`` (``dss_vad_group_window_dev`` / ``_trial_dev``, csrc/vad_train.hip), so the serial
    workgroups of all models run side by side on different compute units.  Every model's numbers are bit for bit those of a
    ``VadTrainerGPU`` with the same weights given the same windows in the same order.  1 <= M <= 64; more models are more groups."""

    def __init__(self, state_dicts, max_window: int = 50):
        state_dicts = list(state_dicts)
        ws = []
        for sd in state_dicts:
            sd = _state_dict(sd, _vad.fits, "VadGroupTrainerGPU")
            ws.append([np.ascontiguousarray(sd[k].detach().cpu().numpy() if hasattr(sd[k], "detach") else sd[k], dtype=np.float32)
                       for k in _vad._KEYS])
        self._L = L = _lib.load()
        self.M, self.max_window = len(ws), int(max_window)
        if not ws:
            _lib.check(L.dss_vad_group_check(0, 1, 1, self.max_window))
        h4, c = ws[0][0].shape
        self.C, self.H = int(c), int(h4 // 4)
        shapes = [tuple(a.shape) for a in ws[0]]
        for m, w in enumerate(ws):
            if [tuple(a.shape) for a in w] != shapes:
                raise ValueError(f"VadGroupTrainerGPU: model {m} has other sizes than model 0 (one group, one size)")
        _lib.check(L.dss_vad_group_check(self.M, self.C, self.H, self.max_window))
        _lib.require_gpu()
        self._n = int(L.dss_vad_trainer_param_count(self.C, self.H))
        self._h = L.dss_vad_group_create(self.M, self.C, self.H, self.max_window)
        if not self._h:
            raise MemoryError(L.dss_last_error().decode())
        self._mask_stage = _MaskStage()
        for m, w in enumerate(ws):
            _lib.check(L.dss_vad_group_load(self._h, m, *[a.ctypes.data for a in w]))

    def __del__(self):
        if getattr(self, "_h", None):
            self._L.dss_vad_group_destroy(self._h)
            self._h = None

    def __len__(self):
        return self.M

    def _member(self, m):
        m = int(m)
        if not 0 <= m < self.M:
            raise IndexError(f"model {m} of a group of {self.M}")
        return m

    # ---- steps ----
    def _table(self, xs, ys, masks, lr, alpha, eps, longest):
        """The step's entry table from per-model sequences (everything but where the losses go), what must stay alive until the
        call has been enqueued, the frames' dtype and their device."""
        import torch
        M = self.M
        xs, ys = list(xs), list(ys)
        masks = [None] * M if masks is None else list(masks)
        for what, seq in (("xs", xs), ("ys", ys), ("masks", masks)):
            if len(seq) != M:
                raise ValueError(f"{what}: {len(seq)} entries for {M} models")
        lrs, alphas, epss = (_per_model(v, M, w) for v, w in ((lr, "lr"), (alpha, "alpha"), (eps, "eps")))
        table = (_VadGroupTrial * M)()
        keep, host_masks, dtype, device = [], [], None, None
        for m in range(M):
            if xs[m] is None:
                continue
            x = xs[m] if isinstance(xs[m], torch.Tensor) else torch.from_numpy(np.ascontiguousarray(xs[m]))
            if x.dtype not in (torch.float64, torch.float32):
                raise TypeError("frames must be float64 or float32")
            if x.dim() != 2 or x.shape[1] != self.C:
                raise ValueError(f"model {m}: frames must be (T, {self.C})")
            if dtype is not None and x.dtype != dtype:
                raise TypeError("the frames of one step must have one dtype")
            dtype = x.dtype
            n = int(x.shape[0])
            if n < 1 or (longest is not None and n > longest):
                raise ValueError(f"model {m}: {n} frames: must be 1 .. {'any' if longest is None else longest}")
            x = x.cuda().contiguous()
            device = x.device
            y = ys[m]
            if isinstance(y, torch.Tensor) and y.is_cuda and y.dtype == torch.uint8:       # resident labels are taken as they are
                if tuple(y.shape) != (n,):
                    raise ValueError(f"model {m}: {n} frames but targets of shape {tuple(y.shape)}")
                y = y.contiguous()
            else:
                y = VadTrainerGPU._targets(y, n)
            k = masks[m]
            if k is not None:
                k = k if isinstance(k, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(k))
                if tuple(k.shape) != (n, self.H):
                    raise ValueError(f"model {m}: the mask must be ({n}, {self.H})")
                k = k.to(dtype=torch.float32).contiguous()
                if not k.is_cuda:
                    host_masks.append((m, k))
            keep += [x, y, k]
            table[m] = _VadGroupTrial(x.data_ptr(), y.data_ptr(), k.data_ptr() if k is not None and k.is_cuda else None, None,
                                      lrs[m], alphas[m], epss[m], n, 1)
        if dtype is None:
            raise ValueError("every model sits out: a step needs at least one model with frames")
        if host_masks:
            for m, k in self._mask_stage.upload(host_masks, device).items():
                table[m].d_mask = k.data_ptr()
        return table, keep, dtype, device

    def _losses(self, losses, table, columns, device):
        """The (M, columns) float64 device tensor the step writes, new and NaN-filled unless given (``columns`` None: (M,)); every
        taking-part model's entry gets its row."""
        import torch
        shape = (self.M,) if columns is None else (self.M, columns)
        if losses is None:
            losses = torch.full(shape, float("nan"), dtype=torch.float64, device=device)
        elif not (isinstance(losses, torch.Tensor) and losses.is_cuda and losses.dtype == torch.float64 and losses.is_contiguous()
                  and losses.dim() == len(shape) and losses.shape[0] == self.M and (columns is None or losses.shape[1] >= columns)):
            raise ValueError(f"losses must be a contiguous CUDA float64 tensor of {' x '.join(str(s) for s in shape)} entries"
                             + ("" if columns is None else " (or more columns)"))
        row = 8 * (1 if columns is None else int(losses.shape[1]))
        for m in range(self.M):
            if table[m].len:
                table[m].d_losses = losses.data_ptr() + row * m
        return losses

    def window(self, xs, ys, masks=None, step: bool = True, lr=LR, alpha=ALPHA, eps=EPS, losses=None):
        """One window for each model from its carried state, as ``VadTrainerGPU.window``: model m runs ``xs[m]`` (T_m, C) frames
        (T_m <= max_window) / ``ys[m]`` (T_m,) 0 / 1 targets / ``masks[m]`` (T_m, H) multipliers or None; ``xs[m] is None``: the
        model sits out and nothing of it changes.  All frames of a step have one dtype.  ``lr``, ``alpha``, ``eps``: a scalar or one
        per model.  Returns the device tensor of M float64 losses: ``losses`` if given (a CUDA float64 tensor of M entries), else a
        new one filled with NaN; the entries of models that sat out are not written.  Nothing synchronises with the host."""
        import torch
        table, keep, dtype, device = self._table(xs, ys, masks, lr, alpha, eps, self.max_window)
        losses = self._losses(losses, table, None, device)
        for m in range(self.M):
            table[m].apply_step = int(bool(step))
        _lib.check(self._L.dss_vad_group_window_dev(self._h, table, int(dtype == torch.float64), torch.cuda.current_stream().cuda_stream))
        return losses

    def train_trials(self, xs, ys, window: int = 50, masks=None, lr=LR, alpha=ALPHA, eps=EPS, losses=None):
        """One trial for each model, as ``VadTrainerGPU.train_trial`` with given masks: the carried state of every model that takes
        part starts from zeros, then window after window of ``window`` frames (a model's last one the remainder) is stepped for all
        models at once until the longest trial has run out; ``xs[m] is None`` sits out.  ``masks[m]``: (len_m, H) multipliers or
        None.  Returns (losses, counts): the (M, max(counts)) float64 device tensor of per-window losses -- ``losses`` if given (M
        rows, at least that many columns), else new and NaN-filled; row m holds model m's ``counts[m]`` = ceil(len_m / window)
        losses, the rest of it is not written -- and the counts (0 for a model that sat out).  Nothing synchronises with the host:
        trials may be enqueued back to back."""
        import torch
        window = int(window)
        _lib.check(self._L.dss_vad_trainer_check(self.C, self.H, self.max_window, 1, 1, window))
        table, keep, dtype, device = self._table(xs, ys, masks, lr, alpha, eps, None)
        counts = [-(-int(table[m].len) // window) for m in range(self.M)]
        losses = self._losses(losses, table, max(counts), device)
        _lib.check(self._L.dss_vad_group_trial_dev(self._h, table, window, int(dtype == torch.float64),
                                                   torch.cuda.current_stream().cuda_stream))
        return losses, counts

    # ---- what the group holds, per model ----
    def _read(self, m: int, what: int) -> dict:
        flat = np.empty(self._n, np.float32)
        _lib.check(self._L.dss_vad_group_read(self._h, self._member(m), what, flat.ctypes.data))
        out, o = {}, 0
        for k, shp in zip(_vad._KEYS, _shapes(self.C, self.H)):
            cnt = int(np.prod(shp))
            out[k] = flat[o:o + cnt].reshape(shp).copy()
            o += cnt
        return out

    def gradients(self, m: int) -> dict:
        """The gradients of model m's last window, float32 arrays keyed by the torch names."""
        return self._read(m, 1)

    def square_avg(self, m: int) -> dict:
        """Model m's RMSprop square averages."""
        return self._read(m, 2)

    def state_dict(self, m: int) -> dict:
        """Model m's current parameters as float32 torch tensors."""
        import torch
        return {k: torch.from_numpy(v) for k, v in self._read(m, 0).items()}

    def state(self, m: int):
        """Model m's carried (h, c), host float32 arrays [2][H]."""
        h = np.empty((2, self.H), np.float32)
        c = np.empty((2, self.H), np.float32)
        _lib.check(self._L.dss_vad_group_state(self._h, self._member(m), h.ctypes.data, c.ctypes.data, 0))
        return h, c

    def set_state(self, m: int, h, c):
        h = np.ascontiguousarray(h, dtype=np.float32).reshape(2, self.H)
        c = np.ascontiguousarray(c, dtype=np.float32).reshape(2, self.H)
        _lib.check(self._L.dss_vad_group_state(self._h, self._member(m), h.ctypes.data, c.ctypes.data, 1))

    def forward_trials_torch(self, frames, ranges, models, want_logits: bool = False):
        """The members' detectors on a trial list in one launch (``dss_vad_group_forward_trials_dev``): as
        ``VadLstmGPU.forward_trials_torch`` with one model index per range -- trial i runs on member ``models[i]``'s current
        weights, in stream order behind the trials enqueued so far, from the zero state; nothing is published and nothing of the
        members (their carried state included) is written.  Returns int32 CUDA labels (sum len,) [, float32 logits (sum len, 2)]
        in list order, a trial's bits those of a ``VadLstmGPU`` holding that member's weights."""
        import torch
        frames, first, length, model, total = _group_trial_list(self, frames, ranges, models)
        labels = torch.empty((total,), dtype=torch.int32, device=frames.device)
        logits = torch.empty((total, 2), dtype=torch.float32, device=frames.device) if want_logits else None
        _lib.check(self._L.dss_vad_group_forward_trials_dev(self._h, frames.data_ptr(), int(frames.dtype == torch.float64), int(frames.shape[0]),
                                                            len(first), first.ctypes.data, length.ctypes.data, model.ctypes.data,
                                                            labels.data_ptr(), logits.data_ptr() if want_logits else None,
                                                            torch.cuda.current_stream().cuda_stream))
        return (labels, logits) if want_logits else labels

    def publish(self, m: int, detector: "_vad.VadLstmGPU"):
        """Copy model m's current weights device to device into an inference handle of the same sizes (``VadLstmGPU``)."""
        import torch
        if not isinstance(detector, _vad.VadLstmGPU):
            raise TypeError("publish takes a VadLstmGPU")
        _lib.check(self._L.dss_vad_group_publish(self._h, self._member(m), detector._h, torch.cuda.current_stream().cuda_stream))


def train_vads(state_dicts, train_corpora, valid_corpora, epochs: int = 8, window: int = 50, dropout: float = 0.5, lr=LR, seeds=None,
               columns=None, shuffle: bool = True, alpha: float = ALPHA, eps: float = EPS, mask_source: str = "host",
               group_validation: bool = False):
    """M ``train_vad`` loops in lock step on one ``VadGroupTrainerGPU``: the day split of train_unidirectional_vad.py:81-93, seeds
    or learning rates as one run.  ``state_dicts[m]``, ``train_corpora[m]``, ``valid_corpora[m]`` and ``seeds[m]`` (default
    0 .. M - 1) are model m's arguments of ``train_vad``; ``lr`` is a scalar or one per model; ``columns`` is shared.

    Model m owns a generator seeded with ``seeds[m]`` that draws its epoch's permutation and then its masks exactly as
    ``train_vad`` does, and step k of an epoch runs every model's k-th trial (``train_trials``), models with fewer trials sitting
    out the rest of the epoch: every model's history and best weights are those of ``train_vad`` run alone with its seed and
    corpora, bit for bit.  After an epoch each model is published into one kept ``VadLstmGPU`` and validated on its own corpus;
    its weights are kept when its accuracy is strictly greater than every earlier one.  Returns [(best state_dict, history)], one
    pair per model.

    ``mask_source="device"``: the permutations still come from those generators; model m's masks come from
    ``DeviceMaskSource(seeds[m])``, one draw per trial stepped, all masks of a step from one launch -- again what
    ``train_vad(..., mask_source="device", seed=seeds[m])`` computes alone, bit for bit.

    ``group_validation=True``: the validation corpora go to the device once, before the first epoch (``GroupValidationSet``), and
    an epoch's M publish + validate calls become one ``vad_validation_group`` call on the trainers' own weights; histories and
    best weights are the same, bit for bit."""
    import torch
    from .validation import GroupValidationSet, _corpus_frames, vad_validation_group
    state_dicts, train_corpora, valid_corpora = list(state_dicts), list(train_corpora), list(valid_corpora)
    M = len(state_dicts)
    seeds = list(range(M)) if seeds is None else list(seeds)
    for what, seq in (("train_corpora", train_corpora), ("valid_corpora", valid_corpora), ("seeds", seeds)):
        if len(seq) != M:
            raise ValueError(f"{what}: {len(seq)} entries for {M} models")
    lrs = _per_model(lr, M, "lr")
    sources = _mask_sources(mask_source, seeds)
    xs, ys, ranges = [], [], []
    for m in range(M):
        hx, hy, hid = _corpus(train_corpora[m])
        x, r = _corpus_frames(hx, hid, columns)
        ya = (hy.detach().cpu().numpy() if isinstance(hy, torch.Tensor) else np.asarray(hy)).ravel()
        if len(ya) != x.shape[0]:
            raise ValueError(f"model {m}: {x.shape[0]} frames but {len(ya)} labels")
        xs.append(x); ranges.append(r)
        ys.append(VadTrainerGPU._targets(ya, len(ya)))       # checked to be 0 / 1 and resident from here on
    if len({x.dtype for x in xs}) > 1:
        xs = [x.double() for x in xs]
    tr = VadGroupTrainerGPU(state_dicts, max_window=window)
    gens = [torch.Generator().manual_seed(int(s)) for s in seeds]
    detector = _vad.VadLstmGPU(1, state_dict=tr.state_dict(0))
    lengths = [[n for _, n in r] for r in ranges]
    vset = GroupValidationSet(valid_corpora, "vad", columns) if group_validation else None

    def step(trials, masks):
        sl = [None if k is None else slice(ranges[m][k][0], ranges[m][k][0] + ranges[m][k][1]) for m, k in enumerate(trials)]
        return tr.train_trials([None if s is None else xs[m][s] for m, s in enumerate(sl)], [None if s is None else ys[m][s] for m, s in enumerate(sl)],
                               window, masks, lrs, alpha, eps)

    best = [(None, -np.inf)] * M
    n_steps, history = [0] * M, [[] for _ in range(M)]
    for _ in range(int(epochs)):
        steps, out = _group_epoch(step, gens, [len(r) for r in ranges], lengths, tr.H, dropout, shuffle, sources, dropout_mask, tr.H)
        out = [(losses.cpu().numpy(), counts) for losses, counts in out]       # the losses stay on the device until here
        vs = vad_validation_group(tr, vset) if group_validation else None
        for m in range(M):
            mine = [losses[m, :counts[m]] for (losses, counts), trials in zip(out, steps) if trials[m] is not None]
            mine = np.concatenate(mine) if mine else np.zeros(0)
            n_steps[m] += len(mine)
            if group_validation:
                v = vs[m]
            else:
                tr.publish(m, detector)
                vx, vy, vid = _corpus(valid_corpora[m])
                v = vad_validation(detector, vx, vy, vid, columns=columns)
            keep = v["accuracy"] > best[m][1]               # StoreBestModel.update: strictly greater
            if keep:
                best[m] = (tr.state_dict(m), v["accuracy"])
            history[m].append(dict(train_loss=float(mine.mean()) if len(mine) else float("nan"), valid_loss=v["loss"],
                                   accuracy=v["accuracy"], update_steps=n_steps[m], best=bool(keep)))
    return [(best[m][0] if best[m][0] is not None else tr.state_dict(m), history[m]) for m in range(M)]


def leave_one_day_out(days, start_with_day=None):
    """The folds of the reference's ``LeaveOneDayOut().split`` (local/common.py:73-101): the days sorted, rotated so that
    ``start_with_day`` (if given) comes first, then every day in turn as the test day against all the others, in that order.
    Yields (train_days, test_day); ValueError for a ``start_with_day`` that is not among the days."""
    ordered = sorted(days)
    if start_with_day is not None:
        if start_with_day not in ordered:
            raise ValueError(f"start_with_day {start_with_day!r} is not one of the days {ordered}")
        k = ordered.index(start_with_day)
        ordered = ordered[k:] + ordered[:k]
    for k, test_day in enumerate(ordered):
        yield ordered[:k] + ordered[k + 1:], test_day


def join_corpora(corpora):
    """Several corpora (one per recording file, mappings or objects as ``train_decoder`` takes them) as one: ``hga_activity``,
    ``lpc_coefficients``, ``vad_labels`` (where every corpus has them) and ``trial_ids`` concatenated in the given order.

    A trial border is a change of id, so two files that meet with equal ids would lose the border between them: where a file's
    first id equals the last id of what has been joined before it, the whole file's ids are negated.  The borders inside the file
    survive the sign flip, and |id| stays the stimulus code (the reference's ``_squeeze_trial_ids`` takes the absolute value too),
    so ``trial_bounds`` of the result is the per-file bounds laid end to end.  A zero id at such a border cannot be negated and
    raises ValueError, as do corpora whose column counts differ."""
    import torch

    def get(c, k):
        try:
            v = c[k]
        except (KeyError, TypeError, IndexError):
            v = getattr(c, k, None)
        return None if v is None else (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v))

    corpora = list(corpora)
    if not corpora:
        raise ValueError("join_corpora: no corpus given")
    cols = {k: [get(c, k) for c in corpora] for k in ("hga_activity", "lpc_coefficients", "vad_labels", "trial_ids")}
    if any(v is None for v in cols["hga_activity"] + cols["trial_ids"]):
        raise ValueError("join_corpora: every corpus needs hga_activity and trial_ids")
    out, ids, last = {}, [], None
    for f, (x, t) in enumerate(zip(cols["hga_activity"], cols["trial_ids"])):
        t = t.ravel()
        if x.ndim != 2 or len(t) != x.shape[0]:
            raise ValueError(f"join_corpora: corpus {f}: hga_activity must be (N, C) with N trial ids")
        if x.shape[1] != cols["hga_activity"][0].shape[1]:
            raise ValueError(f"join_corpora: corpus {f} has {x.shape[1]} columns of hga_activity, corpus 0 has {cols['hga_activity'][0].shape[1]}")
        if len(t) and last is not None and t[0] == last:
            if t[0] == 0:
                raise ValueError(f"join_corpora: corpus {f} starts with the id 0 its predecessor ends with: the border cannot be kept")
            t = -t
        if len(t):
            last = t[-1]
        ids.append(t)
    out["hga_activity"] = np.concatenate(cols["hga_activity"])
    out["trial_ids"] = np.concatenate(ids)
    for k in ("lpc_coefficients", "vad_labels"):
        have = [v is not None for v in cols[k]]
        if k == "lpc_coefficients" and any(have) and not all(have):
            raise ValueError("join_corpora: some corpora have lpc_coefficients and some do not")
        if not all(have):
            continue
        for f, v in enumerate(cols[k]):
            if len(v) != len(cols["trial_ids"][f].ravel()):
                raise ValueError(f"join_corpora: corpus {f}: {k} has {len(v)} rows for {len(cols['trial_ids'][f].ravel())} trial ids")
            if v.ndim == 2 and v.shape[1] != cols[k][0].shape[1]:
                raise ValueError(f"join_corpora: corpus {f} has {v.shape[1]} columns of {k}, corpus 0 has {cols[k][0].shape[1]}")
        out[k] = np.concatenate(cols[k])
    return out


__all__ = ["VadTrainerGPU", "train_vad", "dropout_mask", "DeviceMaskSource", "device_dropout_masks", "dropout_scale", "DecoderTrainerGPU", "train_decoder", "decoder_dropout_mask", "trial_bounds",
           "DecoderGroupTrainerGPU", "train_decoders", "VadGroupTrainerGPU", "train_vads", "lockstep_schedule", "leave_one_day_out", "join_corpora", "LR", "ALPHA", "EPS"]
