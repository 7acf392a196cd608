"""The validation passes of the reference's two training scripts over a corpus, on the GPU: every trial in one call.

A corpus (``dss_amd.session.session_corpus``, or the reference's HDF containers handed over as arrays) is concatenated arrays --
``hga_activity`` (N, C), ``vad_labels`` (N,), ``lpc_coefficients`` (N, 20) -- cut into trials wherever ``trial_ids`` changes
(``SequentialSpeechTrials``, local/training.py:61-78).  Once per epoch the training scripts run every validation trial through
the model from a fresh state, batch size 1, and score it:

  * ``train_unidirectional_vad.py:181-215``: ``valid_loss`` = the sum over the trials of ``nn.CrossEntropyLoss`` (the mean over a
    trial's frames), ``pred`` = argmax, ``prob`` = softmax[:, 1], accuracy = equal frames over all frames: ``vad_validation``.
  * ``train_bidirectional_model.py:165-188``: the mean over the trials of ``nn.MSELoss`` on a trial: ``decoder_validation``.

Here the model is the hand-written kernel (``VadLstmGPU.forward_trials_torch`` / ``BiLstmDecoderGPU.forward_trials_torch``: all
trials in one launch / one call) and the scores come from one reduction launch (``dss_vad_score_trials_dev`` /
``dss_dec_mse_trials_dev``).  The first argument is a module, a state_dict, or a ``VadLstmGPU`` / ``BiLstmDecoderGPU`` that
already holds the weights: given a module or a state_dict every call creates a handle, uploads the weights and, for the
decoder, allocates the two layer buffers (max_streams x longest trial x 2H floats each); a caller that validates every epoch
keeps one handle and passes it in.  A module that is not the reference's architecture raises: there is no fallback to the module's
own forward.  The training of both models is ``dss_amd.training``.

For M models trained side by side (``DecoderGroupTrainerGPU`` / ``VadGroupTrainerGPU``) the same passes run for all models in one
call on the trainers' own weights: ``GroupValidationSet`` keeps the M corpora on the device as one trial list, and
``decoder_validation_group`` / ``vad_validation_group`` return, per model, what the functions above return for its corpus."""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _lib
from . import decoder as _decoder
from . import vad as _vad


def trial_bounds(trial_ids):
    """[(first, len)] of the trials of a corpus: a new trial starts wherever two consecutive ids differ -- the borders of
    ``SequentialSpeechTrials._find_indices_of_nth_subsequence`` (training.py:66-78), as many as ``_count_trials`` counts."""
    ids = np.asarray(trial_ids).ravel()
    if not len(ids):
        return []
    borders = [0] + (np.where(ids[:-1] != ids[1:])[0] + 1).tolist() + [len(ids)]
    return [(a, b - a) for a, b in zip(borders[:-1], borders[1:])]


def _ranges(L, n_rows: int, ranges):
    """(first int64, len int32, sum len) of [(first, len)], checked by ``dss_trials_check`` against an array of n_rows rows."""
    r = [(int(a), int(b)) for a, b in ranges]
    if any(not -2 ** 31 <= b < 2 ** 31 for _, b in r):
        raise ValueError("a trial's length must fit 32 bits")
    first = np.ascontiguousarray([a for a, _ in r], dtype=np.int64)
    length = np.ascontiguousarray([b for _, b in r], dtype=np.int32)
    total = C.c_longlong(0)
    _lib.check(L.dss_trials_check(int(n_rows), len(r), first.ctypes.data, length.ctypes.data, C.byref(total)))
    return first, length, int(total.value)


def _state_dict(model, fits, what):
    """The float32 state_dict of `model` (a module or a state_dict), after ``fits`` has accepted it."""
    class _Holder:
        def __init__(self, sd):
            self._sd = sd

        def state_dict(self):
            return self._sd

    holder = model if hasattr(model, "state_dict") else _Holder(model)
    if not fits(holder):
        raise ValueError(f"{what}: the model is not the reference's architecture (parameter names, shapes, float32, the kernel's "
                         "sizes); it has to be validated by its own forward, there is no fallback here")
    return holder.state_dict()


def _corpus_frames(hga_activity, trial_ids, columns, device="cuda"):
    """The corpus' frames as a CUDA tensor with the optional channel gather applied (SelectElectrodesOverSpeechAreas, 128 -> 64:
    an index select in front of the model), and its trials."""
    import torch
    x = hga_activity if isinstance(hga_activity, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(hga_activity))
    if x.dim() != 2:
        raise ValueError("hga_activity must be (N, C)")
    ranges = trial_bounds(trial_ids.cpu().numpy() if isinstance(trial_ids, torch.Tensor) else trial_ids)
    if sum(n for _, n in ranges) != x.shape[0]:
        raise ValueError(f"{x.shape[0]} frames but {sum(n for _, n in ranges)} trial ids")
    if x.dtype not in (torch.float64, torch.float32):
        x = x.double()
    x = x.cuda() if device == "cuda" else x.to(device)
    if columns is not None:
        x = x.index_select(1, torch.as_tensor(np.asarray(columns, dtype=np.int64), device=x.device))
    return x.contiguous(), ranges


def vad_validation(model_or_state_dict, hga_activity, vad_labels, trial_ids, columns=None) -> dict:
    """The validation pass of train_unidirectional_vad.py:181-215 on a corpus.  Returns ``loss`` (the sum of the per-trial
    cross-entropies: the script's ``valid_loss``), ``accuracy`` (correct frames / all frames), ``per_trial_loss`` (float64),
    ``per_trial_correct`` (int32), ``pred`` (int32 labels per frame) and ``prob`` (float32 speech probability per frame)."""
    L = _lib.require_gpu()
    k = model_or_state_dict if isinstance(model_or_state_dict, _vad.VadLstmGPU) else None
    sd = None if k is not None else _state_dict(model_or_state_dict, _vad.fits, "vad_validation")
    import torch
    x, ranges = _corpus_frames(hga_activity, trial_ids, columns)
    y = vad_labels.cpu().numpy() if isinstance(vad_labels, torch.Tensor) else np.asarray(vad_labels)
    y = y.ravel()
    if len(y) != x.shape[0]:
        raise ValueError(f"{x.shape[0]} frames but {len(y)} labels")
    if y.dtype != bool and ((y != 0) & (y != 1)).any():
        raise ValueError("vad_labels must be 0 / 1")
    n = len(ranges)
    if not n:
        return dict(loss=0.0, accuracy=float("nan"), per_trial_loss=np.zeros(0), per_trial_correct=np.zeros(0, np.int32),
                    pred=np.zeros(0, np.int32), prob=np.zeros(0, np.float32))
    if k is None:
        k = _vad.VadLstmGPU(1, state_dict=sd)
    pred, logits = k.forward_trials_torch(x, ranges, want_logits=True)
    tg = torch.from_numpy(np.ascontiguousarray(y, dtype=np.uint8)).to(x.device)
    length = np.ascontiguousarray([b for _, b in ranges], dtype=np.int32)
    loss = torch.empty((n,), dtype=torch.float64, device=x.device)
    correct = torch.empty((n,), dtype=torch.int32, device=x.device)
    prob = torch.empty((len(y),), dtype=torch.float32, device=x.device)
    _lib.check(L.dss_vad_score_trials_dev(logits.data_ptr(), pred.data_ptr(), tg.data_ptr(), n, length.ctypes.data, loss.data_ptr(),
                                          correct.data_ptr(), prob.data_ptr(), torch.cuda.current_stream().cuda_stream))
    per_loss, per_correct = loss.cpu().numpy(), correct.cpu().numpy()
    return dict(loss=float(per_loss.sum()), accuracy=float(per_correct.sum()) / len(y), per_trial_loss=per_loss,
                per_trial_correct=per_correct, pred=pred.cpu().numpy(), prob=prob.cpu().numpy())


def decoder_validation(model_or_state_dict, hga_activity, lpc_coefficients, trial_ids, columns=None, max_streams: int = 256) -> dict:
    """The validation pass of train_bidirectional_model.py:165-188 on a corpus.  Returns ``loss`` (the mean of the per-trial
    MSEs: the script's ``final_valid_loss``), ``per_trial_mse`` (float64) and ``features`` (float32 (N, n_outputs)).
    ``max_streams`` is the chunk width of the handle this call creates (trials decoded side by side; its layer buffers take
    2 x max_streams x longest trial x 2H floats); it is ignored when a ``BiLstmDecoderGPU`` is passed in, whose ``max_frames``
    must cover the longest trial."""
    L = _lib.require_gpu()
    k = model_or_state_dict if isinstance(model_or_state_dict, _decoder.BiLstmDecoderGPU) else None
    sd = None if k is not None else _state_dict(model_or_state_dict, _decoder.fits, "decoder_validation")
    import torch
    x, ranges = _corpus_frames(hga_activity, trial_ids, columns)
    t = lpc_coefficients if isinstance(lpc_coefficients, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(lpc_coefficients))
    n = len(ranges)
    n_out = k.O if k is not None else int(sd["regressor.weight"].shape[0])
    if t.dim() != 2 or t.shape[0] != x.shape[0] or t.shape[1] != n_out:
        raise ValueError(f"lpc_coefficients must be ({x.shape[0]}, {n_out})")
    if not n:
        return dict(loss=float("nan"), per_trial_mse=np.zeros(0), features=np.zeros((0, n_out), np.float32))
    t = t.to(device=x.device, dtype=torch.float32).contiguous()            # y_val.float() (train_bidirectional_model.py:171)
    if k is None:
        k = _decoder.BiLstmDecoderGPU(max(1, min(n, int(max_streams))), max(b for _, b in ranges), state_dict=sd)
    feats = k.forward_trials_torch(x, ranges)
    length = np.ascontiguousarray([b for _, b in ranges], dtype=np.int32)
    mse = torch.empty((n,), dtype=torch.float64, device=x.device)
    _lib.check(L.dss_dec_mse_trials_dev(feats.data_ptr(), t.data_ptr(), n_out, n, length.ctypes.data, mse.data_ptr(),
                                        torch.cuda.current_stream().cuda_stream))
    per = mse.cpu().numpy()
    return dict(loss=float(per.mean()), per_trial_mse=per, features=feats.cpu().numpy())


# ---- the validation passes of several models trained side by side, in one call ---------------------------------------------------

def _corpus_arrays(corpus, target_key):
    try:
        return corpus["hga_activity"], corpus[target_key], corpus["trial_ids"]
    except (KeyError, TypeError, IndexError):
        return corpus.hga_activity, getattr(corpus, target_key), corpus.trial_ids


class GroupValidationSet:
    """The validation corpora of the M models of a ``DecoderGroupTrainerGPU`` (``kind="decoder"``) or a ``VadGroupTrainerGPU``
    (``kind="vad"``), resident on the device as ONE trial list: built once before the epoch loop, read by
    ``decoder_validation_group`` / ``vad_validation_group`` after every epoch.  ``corpora[m]`` is model m's corpus (a mapping or
    an object with ``hga_activity``, ``trial_ids`` and ``lpc_coefficients`` / ``vad_labels``) or None for a model that has none;
    ``columns`` is the optional channel gather, applied here once.

    ``frames``: the (sum N, C) CUDA tensor of all models' frames, model after model (float64 as soon as one corpus is not float32);
    ``targets``: float32 (sum N, n_outputs) or uint8 (sum N,) on the device; ``ranges``: [(first, len)] of every trial in rows of
    ``frames``, ``models`` the model of each; ``trials[m]`` / ``rows[m]``: model m's slice of the trial list / of the concatenated
    outputs.  The list is in model order, so a model's outputs are one slice.  ``device`` is where the tensors live; the
    validation functions need "cuda", the default."""

    def __init__(self, corpora, kind: str, columns=None, device="cuda"):
        import torch
        if kind not in ("decoder", "vad"):
            raise ValueError(f'kind must be "decoder" or "vad", not {kind!r}')
        corpora = list(corpora)
        self.kind, self.M = kind, len(corpora)
        self.ranges, self.models, self.trials, self.rows = [], [], [], []
        xs, ts, row0 = [], [], 0
        for m, corpus in enumerate(corpora):
            n0, r0 = len(self.ranges), row0
            if corpus is not None:
                hx, hy, hid = _corpus_arrays(corpus, "lpc_coefficients" if kind == "decoder" else "vad_labels")
                x, r = _corpus_frames(hx, hid, columns, device)
                if kind == "decoder":
                    t = hy if isinstance(hy, torch.Tensor) else torch.from_numpy(np.ascontiguousarray(hy))
                    if t.dim() != 2 or t.shape[0] != x.shape[0]:
                        raise ValueError(f"model {m}: lpc_coefficients must be ({x.shape[0]}, n_outputs)")
                    t = t.to(device=x.device, dtype=torch.float32).contiguous()
                else:
                    y = (hy.cpu().numpy() if isinstance(hy, torch.Tensor) else np.asarray(hy)).ravel()
                    if len(y) != x.shape[0]:
                        raise ValueError(f"model {m}: {x.shape[0]} frames but {len(y)} labels")
                    if y.dtype != bool and ((y != 0) & (y != 1)).any():
                        raise ValueError(f"model {m}: vad_labels must be 0 / 1")
                    t = torch.from_numpy(np.ascontiguousarray(y, dtype=np.uint8)).to(x.device)
                if len(r):
                    xs.append(x); ts.append(t)
                    self.ranges += [(row0 + a, n) for a, n in r]
                    self.models += [m] * len(r)
                    row0 += int(x.shape[0])
            self.trials.append(slice(n0, len(self.ranges)))
            self.rows.append(slice(r0, row0))
        if len({x.dtype for x in xs}) > 1:
            xs = [x.double() for x in xs]
        if len({tuple(x.shape[1:]) for x in xs}) > 1 or len({tuple(t.shape[1:]) for t in ts}) > 1:
            raise ValueError("the corpora of one set must have one number of channels and one number of outputs")
        self.frames = torch.cat(xs).contiguous() if xs else None
        self.targets = torch.cat(ts).contiguous() if ts else None
        self.lengths = np.ascontiguousarray([n for _, n in self.ranges], dtype=np.int32)
        self.n_rows = row0

    def __len__(self):
        return self.M


def _to_host_once(tensors):
    """Device tensors to host arrays of their dtypes through ONE device -> host copy (each starts at a multiple of 8 bytes)."""
    import torch
    parts, spans, o = [], [], 0
    for t in tensors:
        b = t.contiguous().view(-1).view(torch.uint8)
        pad = (-b.numel()) % 8
        parts += [b] + ([torch.zeros((pad,), dtype=torch.uint8, device=b.device)] if pad else [])
        spans.append((o, b.numel()))
        o += b.numel() + pad
    host = torch.cat(parts).cpu().numpy()
    return [host[a:a + n].view(np.dtype(str(t.dtype).replace("torch.", ""))).reshape(tuple(t.shape)) for (a, n), t in zip(spans, tensors)]


def _check_set(group, vset, kind, who):
    if not isinstance(vset, GroupValidationSet) or vset.kind != kind:
        raise TypeError(f'{who} takes a GroupValidationSet of kind "{kind}"')
    if vset.M != len(group):
        raise ValueError(f"{who}: a set of {vset.M} corpora for a group of {len(group)} models")


def decoder_validation_group(group, vset) -> list:
    """``decoder_validation`` for every model of a ``DecoderGroupTrainerGPU`` on its corpus of ``vset`` -- one forward call on the
    members' current weights (no publish, no inference handle), one score call, one device -> host copy.  Returns M dicts with
    ``decoder_validation``'s keys, dtypes and bits; a model without trials gets what that function returns for an empty corpus."""
    import torch
    L = _lib.require_gpu()
    _check_set(group, vset, "decoder", "decoder_validation_group")
    n, O = len(vset.ranges), group.O

    def empty():
        return dict(loss=float("nan"), per_trial_mse=np.zeros(0), features=np.zeros((0, O), np.float32))

    if not n:
        return [empty() for _ in range(vset.M)]
    if vset.targets.shape[1] != O:
        raise ValueError(f"lpc_coefficients must be (N, {O})")
    feats = group.forward_trials_torch(vset.frames, vset.ranges, vset.models)
    mse = torch.empty((n,), dtype=torch.float64, device=feats.device)
    _lib.check(L.dss_dec_mse_trials_dev(feats.data_ptr(), vset.targets.data_ptr(), O, n, vset.lengths.ctypes.data, mse.data_ptr(),
                                        torch.cuda.current_stream().cuda_stream))
    per, features = _to_host_once([mse, feats])
    out = []
    for m in range(vset.M):
        p = per[vset.trials[m]].copy()
        out.append(dict(loss=float(p.mean()), per_trial_mse=p, features=features[vset.rows[m]].copy()) if len(p) else empty())
    return out


def vad_validation_group(group, vset) -> list:
    """``vad_validation`` for every model of a ``VadGroupTrainerGPU`` on its corpus of ``vset`` -- one forward launch on the
    members' current weights (no publish, no inference handle), one score call, one device -> host copy.  Returns M dicts with
    ``vad_validation``'s keys, dtypes and bits; a model without trials gets what that function returns for an empty corpus."""
    import torch
    L = _lib.require_gpu()
    _check_set(group, vset, "vad", "vad_validation_group")
    n = len(vset.ranges)

    def empty():
        return dict(loss=0.0, accuracy=float("nan"), per_trial_loss=np.zeros(0), per_trial_correct=np.zeros(0, np.int32),
                    pred=np.zeros(0, np.int32), prob=np.zeros(0, np.float32))

    if not n:
        return [empty() for _ in range(vset.M)]
    pred, logits = group.forward_trials_torch(vset.frames, vset.ranges, vset.models, want_logits=True)
    loss = torch.empty((n,), dtype=torch.float64, device=pred.device)
    correct = torch.empty((n,), dtype=torch.int32, device=pred.device)
    prob = torch.empty((vset.n_rows,), dtype=torch.float32, device=pred.device)
    _lib.check(L.dss_vad_score_trials_dev(logits.data_ptr(), pred.data_ptr(), vset.targets.data_ptr(), n, vset.lengths.ctypes.data,
                                          loss.data_ptr(), correct.data_ptr(), prob.data_ptr(), torch.cuda.current_stream().cuda_stream))
    per_loss, per_correct, pred_h, prob_h = _to_host_once([loss, correct, pred, prob])
    out = []
    for m in range(vset.M):
        tr, rw = vset.trials[m], vset.rows[m]
        if tr.stop == tr.start:
            out.append(empty())
            continue
        pl, pc = per_loss[tr].copy(), per_correct[tr].copy()
        out.append(dict(loss=float(pl.sum()), accuracy=float(pc.sum()) / (rw.stop - rw.start), per_trial_loss=pl, per_trial_correct=pc,
                        pred=pred_h[rw].copy(), prob=prob_h[rw].copy()))
    return out
