"""The models of a group of trainers over one trial list (Part 17: ``DecoderGroupTrainerGPU.forward_trials_torch``,
``VadGroupTrainerGPU.forward_trials_torch``, ``decoder_validation_group`` / ``vad_validation_group``, ``group_validation=True``)
on the cases of tests/group_validation_cases.py.

The parent's path is the yardstick of the bit tests: a ``BiLstmDecoderGPU`` / ``VadLstmGPU`` loaded with model m's state dict
running ``forward_trials_torch`` on that model's trials alone; every trial's features, labels and logits must equal it bit for
bit.  The float64 test holds every output to ``lstm_reference.bound(scale)``, the project's bound for these kernels.
tests/test_cpu_group_validation.py shows on the float64 reference that another member's weights miss that bound on every trial."""
import ctypes as C
import functools

import numpy as np
import pytest

import decoder_training_reference as D
import group_validation_cases as G
import lstm_reference as R
import vad_training_reference as V

pytestmark = pytest.mark.gpu

TABLES = {"decoder": G.DECODER, "vad": G.DETECTOR}
ENTRIES = [pytest.param(kind, e, id=f"{kind}-{e.name}") for kind, table in TABLES.items() for e in table]
PAD = 3          # rows behind the last output row that hold a sentinel


@pytest.fixture(scope="module")
def T():
    from dss_amd import training
    return training


def _dev(x, f64):
    import torch
    return torch.from_numpy(x if f64 else x.astype(np.float32)).cuda()


@functools.lru_cache(maxsize=None)
def _group(kind, e):
    from dss_amd import training
    sds = G.members(kind, e)
    return training.DecoderGroupTrainerGPU(sds, max_frames=8) if kind == "decoder" else training.VadGroupTrainerGPU(sds, max_window=8)


def _handle(kind, sd, ranges):
    from dss_amd.decoder import BiLstmDecoderGPU
    from dss_amd.vad import VadLstmGPU
    if kind == "vad":
        return VadLstmGPU(1, state_dict=sd)
    return BiLstmDecoderGPU(max(1, min(len(ranges), 256)), max(n for _, n in ranges), state_dict=sd)


@functools.lru_cache(maxsize=None)
def _parent(kind, e):
    """Per trial, in list order, what the parent's path computes: (features,) or (labels, logits), host arrays."""
    x, ranges = G.layout(e)
    xd = _dev(x, e.f64)
    out = [None] * len(ranges)
    for m, idx in G.per_model(e).items():
        if not idx:
            continue
        mine = [ranges[i] for i in idx]
        h = _handle(kind, G.members(kind, e)[m], mine)
        got = h.forward_trials_torch(xd, mine) if kind == "decoder" else h.forward_trials_torch(xd, mine, want_logits=True)
        got = [t.cpu().numpy() for t in (got if isinstance(got, tuple) else (got,))]
        o = 0
        for i in idx:
            out[i] = tuple(a[o:o + e.lengths[i]] for a in got)
            o += e.lengths[i]
    return out


def _raw_call(kind, g, xd, ranges, models, max_rows=0, want_logits=True):
    """The C entry point on outputs with PAD sentinel rows behind them; returns host arrays without the sentinel rows, which are
    checked to be untouched."""
    import torch
    from dss_amd import _lib
    L = _lib.load()
    first = np.ascontiguousarray([a for a, _ in ranges], dtype=np.int64)
    length = np.ascontiguousarray([n for _, n in ranges], dtype=np.int32)
    model = np.ascontiguousarray(models, dtype=np.int32)
    total = int(length.sum())
    st = torch.cuda.current_stream().cuda_stream
    f64 = int(xd.dtype == torch.float64)
    if kind == "decoder":
        feats = torch.full((total + PAD, g.O), float("nan"), dtype=torch.float32, device=xd.device)
        _lib.check(L.dss_dec_group_forward_trials_dev(g._h, xd.data_ptr(), f64, int(xd.shape[0]), len(ranges), first.ctypes.data, length.ctypes.data,
                                                      model.ctypes.data, int(max_rows), feats.data_ptr(), st))
        feats = feats.cpu().numpy()
        assert np.isnan(feats[total:]).all() and not np.isnan(feats[:total]).any()
        return (feats[:total],)
    labels = torch.full((total + PAD,), -7, dtype=torch.int32, device=xd.device)
    logits = torch.full((total + PAD, 2), float("nan"), dtype=torch.float32, device=xd.device)
    _lib.check(L.dss_vad_group_forward_trials_dev(g._h, xd.data_ptr(), f64, int(xd.shape[0]), len(ranges), first.ctypes.data, length.ctypes.data,
                                                  model.ctypes.data, labels.data_ptr(), logits.data_ptr() if want_logits else None, st))
    labels, logits = labels.cpu().numpy(), logits.cpu().numpy()
    assert (labels[total:] == -7).all() and set(np.unique(labels[:total])) <= {0, 1}
    assert np.isnan(logits[total:]).all() and np.isnan(logits[:total]).any() == (not want_logits)
    return (labels[:total], logits[:total]) if want_logits else (labels[:total],)


@functools.lru_cache(maxsize=None)
def _got(kind, e):
    """The group's outputs on the entry, through ``forward_trials_torch``: host arrays in list order."""
    x, ranges = G.layout(e)
    g, xd = _group(kind, e), _dev(x, e.f64)
    if kind == "decoder":
        return (g.forward_trials_torch(xd, ranges, e.models, max_rows=e.max_rows).cpu().numpy(),)
    return tuple(t.cpu().numpy() for t in g.forward_trials_torch(xd, ranges, e.models, want_logits=True))


# ---- 1: bits ---------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind, e", ENTRIES)
def test_every_trial_is_the_single_model_path_bit_for_bit(kind, e):
    x, ranges = G.layout(e)
    got, want, off = _got(kind, e), _parent(kind, e), G.offsets(e)
    assert got[0].dtype == (np.float32 if kind == "decoder" else np.int32) and len(got[0]) == off[-1]
    for i in range(len(ranges)):
        for a, b in zip(got, want[i]):
            assert a.dtype == b.dtype and np.array_equal(a[off[i]:off[i + 1]], b), (e.name, i, e.models[i], e.lengths[i])
    raw = _raw_call(kind, _group(kind, e), _dev(x, e.f64), ranges, e.models, e.max_rows)       # nothing behind the last row is written
    assert all(np.array_equal(a, b) for a, b in zip(raw, got))


def test_detector_labels_do_not_depend_on_the_logits_being_asked_for():
    e = G.by_name(G.DETECTOR, "small")
    x, ranges = G.layout(e)
    g, xd = _group("vad", e), _dev(x, e.f64)
    labels = g.forward_trials_torch(xd, ranges, e.models)
    assert not isinstance(labels, tuple) and np.array_equal(labels.cpu().numpy(), _got("vad", e)[0])
    assert np.array_equal(_raw_call("vad", g, xd, ranges, e.models, want_logits=False)[0], _got("vad", e)[0])


def test_chunked_list_equals_the_list_in_one_set():
    e = G.by_name(G.DECODER, "chunked")
    x, ranges = G.layout(e)
    one = _group("decoder", e).forward_trials_torch(_dev(x, e.f64), ranges, e.models).cpu().numpy()
    assert np.array_equal(one, _got("decoder", e)[0])


# ---- 2: float64 ------------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind, e", ENTRIES)
def test_every_output_is_within_the_bound_of_float64(kind, e):
    got, want, off = _got(kind, e), G.reference(kind, e), G.offsets(e)
    values = got[0] if kind == "decoder" else got[1]
    worst = 0.0
    for i, ref in enumerate(want):
        err = np.abs(values[off[i]:off[i + 1]].astype(np.float64) - ref).max()
        worst = max(worst, err / G.bound(e, e.models[i]))
        assert err <= G.bound(e, e.models[i]), (e.name, i, e.models[i], err)
        if kind == "vad":
            assert np.array_equal(got[0][off[i]:off[i + 1]], (ref[:, 1] > ref[:, 0]).astype(np.int32)), (e.name, i)
    print(f"{kind} {e.name}: largest error / bound {worst:.3f}")


# ---- 3: order changes no bit -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ("decoder", "vad"))
@pytest.mark.parametrize("name", ("small", "width_101_198_1"))
def test_permuting_the_list_permutes_the_outputs(kind, name):
    e = G.by_name(TABLES[kind], name)
    x, ranges = G.layout(e)
    perm = np.random.default_rng(3).permutation(len(ranges))
    g, xd = _group(kind, e), _dev(x, e.f64)
    got = _raw_call(kind, g, xd, [ranges[i] for i in perm], [e.models[i] for i in perm])
    base, off = _got(kind, e), G.offsets(e)
    o = 0
    for i in perm:
        for a, b in zip(got, base):
            assert np.array_equal(a[o:o + e.lengths[i]], b[off[i]:off[i + 1]]), (name, i)
        o += e.lengths[i]


@pytest.mark.parametrize("kind", ("decoder", "vad"))
def test_renumbering_the_members_changes_nothing(kind, T):
    e = G.by_name(TABLES[kind], "small")
    x, ranges = G.layout(e)
    sds = G.members(kind, e)
    place = [2, 0, 1]                                      # member place[m] of the new group holds model m's weights
    moved = [None] * 3
    for m, k in enumerate(place):
        moved[k] = sds[m]
    g = T.DecoderGroupTrainerGPU(moved, max_frames=8) if kind == "decoder" else T.VadGroupTrainerGPU(moved, max_window=8)
    got = _raw_call(kind, g, _dev(x, e.f64), ranges, [place[m] for m in e.models])
    assert all(np.array_equal(a, b) for a, b in zip(got, _got(kind, e)))


@pytest.mark.parametrize("kind", ("decoder", "vad"))
def test_a_member_alone_and_inside_64(kind, T):
    e = G.by_name(TABLES[kind], "capacity")
    x, ranges = G.layout(e)
    base, off, xd = _got(kind, e), G.offsets(e), _dev(x, e.f64)
    for i in (0, 17, len(ranges) - 1):
        sd = G.members(kind, e)[e.models[i]]
        g = T.DecoderGroupTrainerGPU([sd], max_frames=8) if kind == "decoder" else T.VadGroupTrainerGPU([sd], max_window=8)
        got = _raw_call(kind, g, xd, [ranges[i]], [0])
        assert all(np.array_equal(a, b[off[i]:off[i + 1]]) for a, b in zip(got, base)), i


# ---- 4: the members' current weights, nothing published, nothing written ----------------------------------------------------------

def _same(a, b):
    return a.keys() == b.keys() and all(np.array_equal(np.asarray(a[k]), np.asarray(b[k])) for k in a)


def test_decoder_forward_reads_the_weights_behind_two_steps(T):
    import torch
    e = G.by_name(G.DECODER, "small")
    x, ranges = G.layout(e)
    sds = G.members("decoder", e)
    g = T.DecoderGroupTrainerGPU(sds, max_frames=16)
    rng = np.random.default_rng(8)
    xd = _dev(x, False)
    for k in range(2):                                     # enqueued back to back, the forward call right behind them
        n = 9 - 2 * k
        g.step([xd[3 * m + k:3 * m + k + n] for m in range(3)], [rng.standard_normal((n, G.O)).astype(np.float32) for _ in range(3)], lr=1e-2)
    feats = g.forward_trials_torch(xd, ranges, e.models)
    before = [(g.state_dict(m), g.gradients(m), g.square_avg(m), g.features(m)) for m in range(3)]
    assert not _same({k: v.numpy() for k, v in before[0][0].items()}, {k: v.numpy() for k, v in sds[0].items()})      # the steps moved the weights
    again = g.forward_trials_torch(xd, ranges, e.models)
    assert torch.equal(feats, again)
    off = G.offsets(e)
    for m, idx in G.per_model(e).items():
        h = _handle("decoder", sds[m], [ranges[i] for i in idx])
        g.publish(m, h)
        want = h.forward_trials_torch(xd, [ranges[i] for i in idx]).cpu().numpy()
        got = np.concatenate([feats.cpu().numpy()[off[i]:off[i + 1]] for i in idx])
        assert np.array_equal(got, want), m
        after = (g.state_dict(m), g.gradients(m), g.square_avg(m), g.features(m))
        assert all(_same(a, b) for a, b in zip(before[m][:3], after[:3])) and np.array_equal(before[m][3], after[3]), m


def test_detector_forward_reads_the_weights_behind_two_trials(T):
    import torch
    e = G.by_name(G.DETECTOR, "small")
    x, ranges = G.layout(e)
    sds = G.members("vad", e)
    g = T.VadGroupTrainerGPU(sds, max_window=4)
    rng = np.random.default_rng(9)
    xd = _dev(x, False)
    for k in range(2):
        n = 9 - 2 * k
        g.train_trials([xd[3 * m + k:3 * m + k + n] for m in range(3)], [rng.integers(0, 2, n).astype(np.uint8) for _ in range(3)], window=4, lr=1e-2)
    labels, logits = g.forward_trials_torch(xd, ranges, e.models, want_logits=True)
    before = [(g.state_dict(m), g.gradients(m), g.square_avg(m), g.state(m)) for m in range(3)]
    assert any(np.abs(before[m][3][0]).max() > 0 for m in range(3))                    # a carried state that is not the zero state
    l2, z2 = g.forward_trials_torch(xd, ranges, e.models, want_logits=True)
    assert torch.equal(labels, l2) and torch.equal(logits, z2)
    off = G.offsets(e)
    for m, idx in G.per_model(e).items():
        h = _handle("vad", sds[m], None)
        g.publish(m, h)
        wl, wz = (t.cpu().numpy() for t in h.forward_trials_torch(xd, [ranges[i] for i in idx], want_logits=True))
        assert np.array_equal(np.concatenate([labels.cpu().numpy()[off[i]:off[i + 1]] for i in idx]), wl), m
        assert np.array_equal(np.concatenate([logits.cpu().numpy()[off[i]:off[i + 1]] for i in idx]), wz), m
        after = (g.state_dict(m), g.gradients(m), g.square_avg(m), g.state(m))
        assert all(_same(a, b) for a, b in zip(before[m][:3], after[:3])), m
        assert all(np.array_equal(a, b) for a, b in zip(before[m][3], after[3])), m


# ---- 5: the validation dicts -----------------------------------------------------------------------------------------------------

def _corpora(kind, C_raw):
    """Four corpora: trials of 1 .. 9 frames, one model without a corpus, one float64 corpus."""
    rng = np.random.default_rng(12)
    out = []
    for m, lengths in enumerate(([3, 1, 9, 5], None, [4, 4, 7], [2])):
        if lengths is None:
            out.append(None)
            continue
        n = sum(lengths)
        c = dict(hga_activity=R.frames("x2", 1, n, C_raw, 600 + m)[0].astype(np.float64 if m == 2 else np.float32),
                 trial_ids=np.repeat(np.arange(len(lengths)), lengths))
        if kind == "decoder":
            c["lpc_coefficients"] = rng.standard_normal((n, G.O)).astype(np.float32)
        else:
            c["vad_labels"] = np.repeat(rng.integers(0, 2, n // 2 + 1), 2)[:n].astype(np.uint8)
        out.append(c)
    return out


def _assert_dict_equal(got, want):
    assert got.keys() == want.keys()
    for k, w in want.items():
        if isinstance(w, np.ndarray):
            assert got[k].dtype == w.dtype and got[k].shape == w.shape and np.array_equal(got[k], w), k
        else:
            assert type(got[k]) is type(w) and (got[k] == w or (np.isnan(w) and np.isnan(got[k]))), (k, got[k], w)


@pytest.mark.parametrize("kind", ("decoder", "vad"))
def test_group_validation_dicts_are_the_single_model_dicts(kind, T):
    from dss_amd import validation
    e = G.by_name(TABLES[kind], "small")
    cols = [8, 0, 3, 4, 1, 6, 5]                           # 9 raw channels -> the models' 7
    corpora, sds = _corpora(kind, 9), G.members(kind, e) + [G.member_sd(kind, e.H, e.C, 3)]
    g = T.DecoderGroupTrainerGPU(sds, max_frames=8) if kind == "decoder" else T.VadGroupTrainerGPU(sds, max_window=8)
    vset = validation.GroupValidationSet(corpora, kind, columns=cols)
    assert vset.frames.is_cuda and vset.targets.is_cuda and vset.n_rows == 35 and len(vset.ranges) == 8
    got = (validation.decoder_validation_group if kind == "decoder" else validation.vad_validation_group)(g, vset)
    assert len(got) == 4
    single = validation.decoder_validation if kind == "decoder" else validation.vad_validation
    key = "lpc_coefficients" if kind == "decoder" else "vad_labels"
    for m, c in enumerate(corpora):
        if c is None:
            c = dict(hga_activity=np.zeros((0, 9), np.float32), trial_ids=np.zeros(0, np.int64))
            c[key] = np.zeros((0, G.O), np.float32) if kind == "decoder" else np.zeros(0, np.uint8)
        _assert_dict_equal(got[m], single(sds[m], c["hga_activity"], c[key], c["trial_ids"], columns=cols))
    assert len(got[1]["features" if kind == "decoder" else "pred"]) == 0


# ---- 6: the training loops -------------------------------------------------------------------------------------------------------

def _head(corpus, trials, n):
    rows = sum(len(y) for _, y in trials[:n])
    return {k: v[:rows] for k, v in corpus.items()}


def _assert_runs_equal(a, b, keys):
    assert len(a) == len(b)
    for (best_a, hist_a), (best_b, hist_b) in zip(a, b):
        assert hist_a == hist_b, (hist_a, hist_b)
        assert all(np.array_equal(best_a[k].numpy(), best_b[k].numpy()) for k in keys)


def test_train_decoders_with_group_validation_is_the_default_path(T):
    sd, trials, corpus = D.learning_problem()
    L = D.LEARN
    corpora, valid = [_head(corpus, trials, n) for n in (3, 2, 3)], [_head(corpus, trials, 2), corpus, _head(corpus, trials, 1)]
    kw = dict(epochs=2, dropout=L["dropout"], lr=L["lr"], seeds=(11, 12, 13))
    _assert_runs_equal(T.train_decoders([sd] * 3, corpora, valid, group_validation=True, **kw), T.train_decoders([sd] * 3, corpora, valid, **kw), D.KEYS)


def test_train_vads_with_group_validation_is_the_default_path(T):
    sd, trials, corpus = V.learning_problem()
    L = V.LEARN
    sds = [sd, G.member_sd("vad", L["H"], L["C"], 1), sd]
    corpora, valid = [_head(corpus, trials, n) for n in (3, 2, 3)], [_head(corpus, trials, 2), corpus, _head(corpus, trials, 1)]
    kw = dict(epochs=2, window=L["window"], dropout=L["dropout"], lr=L["lr"], seeds=(11, 12, 13))
    _assert_runs_equal(T.train_vads(sds, corpora, valid, group_validation=True, **kw), T.train_vads(sds, corpora, valid, **kw), V.KEYS)


# ---- 7: refusals -----------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("kind", ("decoder", "vad"))
def test_refusals_and_the_empty_list(kind, T):
    import torch
    from dss_amd import _lib
    from dss_amd import decoder as _decoder, vad as _vad
    L = _lib.load()
    e = G.by_name(TABLES[kind], "small")
    x, ranges = G.layout(e)
    g, xd = _group(kind, e), _dev(x, e.f64)
    name = f"dss_{'dec' if kind == 'decoder' else 'vad'}_group_forward_trials_dev"
    for bad in (3, -1):
        with pytest.raises(_lib.DssError, match=f"{name}: trial 1 names model {bad} of a group of 3"):
            g.forward_trials_torch(xd, ranges[:2], [0, bad])
    with pytest.raises(ValueError, match="1 model indices for 2 trials"):
        g.forward_trials_torch(xd, ranges[:2], [0])
    with pytest.raises(_lib.DssError, match="trial 0"):
        g.forward_trials_torch(xd, [(len(x) - 1, 2)], [0])                  # dss_trials_check: runs past the array
    empty = g.forward_trials_torch(xd, [], [])
    if kind == "decoder":
        assert tuple(empty.shape) == (0, G.O) and empty.dtype == torch.float32
        with pytest.raises(_lib.DssError, match="trial 2 has 9 frames, max_rows is 8"):
            g.forward_trials_torch(xd, ranges, e.models, max_rows=8)
    else:
        assert tuple(empty.shape) == (0,) and empty.dtype == torch.int32
        labels, logits = g.forward_trials_torch(xd, [], [], want_logits=True)
        assert tuple(logits.shape) == (0, 2)
    # NULL outputs, and a member without parameters, at the C entry point
    first, length, model = np.zeros(1, np.int64), np.ones(1, np.int32), np.ones(1, np.int32)
    args = (xd.data_ptr(), int(e.f64), int(xd.shape[0]), 1, first.ctypes.data, length.ctypes.data, model.ctypes.data)
    out = torch.zeros((8, G.O), dtype=torch.float32, device=xd.device)
    tail = (0, None, None) if kind == "decoder" else (None, None, None)
    assert getattr(L, name)(g._h, *args, *tail) == -1 and f"{name}: null argument" in L.dss_last_error().decode()
    sd = G.members(kind, e)[0]
    keys = _decoder._KEYS if kind == "decoder" else _vad._KEYS
    w = [np.ascontiguousarray(sd[k].numpy(), dtype=np.float32) for k in keys]
    if kind == "decoder":
        h = L.dss_dec_group_create(2, e.C, e.H, G.O, 8)
        assert h and L.dss_dec_group_load(h, 0, (C.c_void_p * 18)(*[a.ctypes.data for a in w])) == 0
        tail = (0, out.data_ptr(), None)
    else:
        h = L.dss_vad_group_create(2, e.C, e.H, 8)
        assert h and L.dss_vad_group_load(h, 0, *[a.ctypes.data for a in w]) == 0
        tail = (out.data_ptr(), None, None)
    try:
        assert getattr(L, name)(h, *args, *tail) == -1
        assert f"{name}: model 1 has no parameters loaded" in L.dss_last_error().decode()
        model[0] = 0
        assert getattr(L, name)(h, *args, *tail) == 0, L.dss_last_error().decode()       # the loaded member alone is served
        torch.cuda.synchronize()
    finally:
        getattr(L, f"dss_{'dec' if kind == 'decoder' else 'vad'}_group_destroy")(h)
