"""Several decoders trained at once (Part 13 of include/dss_hip.h, dss_amd/training.py) without a GPU: the exported symbols, the
argument checks at both ends of every limit, the fold helper, the join of corpora, the lock-step schedule, and the generator
discipline of ``train_decoders`` (a model's permutation and masks are those ``train_decoder`` draws from the same seed)."""
import os
import re

import numpy as np
import pytest

import decoder_training_reference as D

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ("dss_dec_group_check", "dss_dec_group_create", "dss_dec_group_destroy", "dss_dec_group_load", "dss_dec_group_read",
         "dss_dec_group_features", "dss_dec_group_publish", "dss_dec_group_step_dev")


def test_symbols_are_declared_and_exported():
    from dss_amd import _lib, training
    L = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "dss_hip.h")).read(), flags=re.S)
    for name in NAMES:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(L, name), name
    for name in ("DecoderGroupTrainerGPU", "train_decoders", "leave_one_day_out", "join_corpora", "lockstep_schedule"):
        assert name in training.__all__ and hasattr(training, name), name


def test_trial_struct_matches_the_header():
    """The ctypes mirror of dss_dec_group_trial: the header's fields in the header's order, 64 bytes."""
    import ctypes as C
    from dss_amd.training import _GroupTrial
    text = open(os.path.join(ROOT, "include", "dss_hip.h")).read()
    body = re.search(r"typedef struct \{([^}]*)\} dss_dec_group_trial;", text).group(1)
    fields = re.findall(r"(\w+)\s*(?:,|;)", body)
    assert [n for n, _ in _GroupTrial._fields_] == fields
    assert C.sizeof(_GroupTrial) == 64


@pytest.mark.parametrize("args, ok, reason", [
    ((1, 64, 100, 20, 1500), True, None),
    ((64, 256, 128, 32, 4096), True, None),                # the upper end of every limit
    ((1, 1, 1, 1, 1), True, None),                         # the lower end
    ((0, 64, 100, 20, 1500), False, "0 models"),
    ((65, 64, 100, 20, 1500), False, "65 models"),
    ((-1, 64, 100, 20, 1500), False, "-1 models"),
    ((2, 257, 100, 20, 1500), False, "257 inputs"),
    ((2, 0, 100, 20, 1500), False, "0 inputs"),
    ((2, 64, 129, 20, 1500), False, "129 hidden units"),
    ((2, 64, 0, 20, 1500), False, "0 hidden units"),
    ((2, 64, 100, 33, 1500), False, "33 outputs"),
    ((2, 64, 100, 0, 1500), False, "0 outputs"),
    ((2, 64, 100, 20, 4097), False, "max_frames 4097"),
    ((2, 64, 100, 20, 0), False, "max_frames 0"),
])
def test_group_check_at_both_ends_of_every_limit(args, ok, reason):
    from dss_amd import _lib
    L = _lib.load()
    rc = L.dss_dec_group_check(*args)
    if ok:
        assert rc == 0, L.dss_last_error().decode()
    else:
        assert rc == -1
        assert reason in L.dss_last_error().decode(), L.dss_last_error().decode()


def test_class_refuses_without_a_device_call():
    """Sizes are checked before a device is asked for: 65 models, models of two sizes, no model."""
    import lstm_reference as R
    from dss_amd import _lib, training
    sd = R.decoder_state_dict(6, 5, 1)
    with pytest.raises(_lib.DssError, match="65 models"):
        training.DecoderGroupTrainerGPU([sd] * 65, max_frames=8)
    with pytest.raises(_lib.DssError, match="0 models"):
        training.DecoderGroupTrainerGPU([], max_frames=8)
    with pytest.raises(ValueError, match="other sizes"):
        training.DecoderGroupTrainerGPU([sd, R.decoder_state_dict(8, 5, 1)], max_frames=8)


# ---- the folds ---------------------------------------------------------------------------------------------------------------------

DAYS = ["2022_03_14", "2022_01_20", "2022_02_07", "2021_12_01", "2022_02_21"]


def test_leave_one_day_out():
    from dss_amd.training import leave_one_day_out
    a, b, c, d, e = "2021_12_01", "2022_01_20", "2022_02_07", "2022_02_21", "2022_03_14"
    assert list(leave_one_day_out(DAYS)) == [([b, c, d, e], a), ([a, c, d, e], b), ([a, b, d, e], c), ([a, b, c, e], d), ([a, b, c, d], e)]
    assert list(leave_one_day_out(DAYS, start_with_day=d)) == [([e, a, b, c], d), ([d, a, b, c], e), ([d, e, b, c], a), ([d, e, a, c], b),
                                                               ([d, e, a, b], c)]
    assert list(leave_one_day_out(iter(DAYS), start_with_day=a)) == list(leave_one_day_out(DAYS))
    assert DAYS[0] == "2022_03_14"                         # the input is left as it was
    with pytest.raises(ValueError, match="2020_01_01"):
        list(leave_one_day_out(DAYS, start_with_day="2020_01_01"))
    # the script's nested use (train_bidirectional_model.py:68-70): the validation day out of the training days
    train, test = next(leave_one_day_out(DAYS, start_with_day=c))
    assert (train, test) == ([d, e, a, b], c)
    assert next(leave_one_day_out(train, start_with_day=e)) == ([a, b, d], e)


# ---- joining corpora ---------------------------------------------------------------------------------------------------------------

def _file(ids, C=3, O=2, seed=0, labels=True):
    rng = np.random.default_rng(seed)
    ids = np.asarray(ids)
    out = dict(hga_activity=rng.standard_normal((len(ids), C)), lpc_coefficients=rng.standard_normal((len(ids), O)).astype(np.float32),
               trial_ids=ids)
    if labels:
        out["vad_labels"] = rng.integers(0, 2, len(ids))
    return out


def _laid_end_to_end(files):
    from dss_amd.training import trial_bounds
    want, o = [], 0
    for f in files:
        want += [(a + o, n) for a, n in trial_bounds(f["trial_ids"])]
        o += len(f["trial_ids"])
    return want


@pytest.mark.parametrize("ids", [
    ([3, 3, 5, 5, 5], [7, 7, 2]),                          # different ids at the border
    ([3, 3, 5, 5, 5], [5, 5, 2, 2, 2, 5]),                 # the last id equals the next file's first
    ([4, 4, 9], [9, 9], [9, 1, 1], [1, 1, 1], [-1, 6]),    # a chain: the second file is negated, so the third meets -9 and stays
    ([2, 2], [2, 2], [2, 2]),                              # three one-trial files with the same stimulus
    ([1, -1, 1], [1, 1]),                                  # signs inside a file already mark borders
], ids=str)
def test_join_corpora_keeps_every_border(ids):
    from dss_amd.training import join_corpora, trial_bounds
    files = [_file(t, seed=k) for k, t in enumerate(ids)]
    j = join_corpora(files)
    assert trial_bounds(j["trial_ids"]) == _laid_end_to_end(files)
    assert np.array_equal(np.abs(j["trial_ids"]), np.abs(np.concatenate([np.asarray(t) for t in ids])))
    for k in ("hga_activity", "lpc_coefficients", "vad_labels"):
        assert np.array_equal(j[k], np.concatenate([f[k] for f in files])), k
    assert all(not np.shares_memory(j["trial_ids"], f["trial_ids"]) for f in files)
    assert [list(f["trial_ids"]) for f in files] == [list(t) for t in ids]          # the inputs are left as they were


def test_join_corpora_optional_labels_and_refusals():
    from dss_amd.training import join_corpora
    j = join_corpora([_file([1, 1, 2], labels=False), _file([2, 3])])
    assert "vad_labels" not in j and len(j["trial_ids"]) == 5 and list(j["trial_ids"]) == [1, 1, 2, -2, -3]
    with pytest.raises(ValueError, match="4 columns of hga_activity"):
        join_corpora([_file([1, 1]), _file([2, 2], C=4)])
    with pytest.raises(ValueError, match="3 columns of lpc_coefficients"):
        join_corpora([_file([1, 1]), _file([2, 2], O=3)])
    with pytest.raises(ValueError, match="id 0"):
        join_corpora([_file([1, 0]), _file([0, 2])])
    with pytest.raises(ValueError, match="no corpus"):
        join_corpora([])

    class Obj:                                             # objects with attributes work like mappings
        def __init__(self, d):
            self.__dict__.update(d)
    files = [_file([1, 1, 2]), _file([2, 3])]
    assert np.array_equal(join_corpora([Obj(f) for f in files])["trial_ids"], join_corpora(files)["trial_ids"])


# ---- the schedule and the generators -----------------------------------------------------------------------------------------------

def test_lockstep_schedule():
    from dss_amd.training import lockstep_schedule
    orders = [[2, 0, 1, 3], [1, 0], [], [0, 2, 1]]
    steps = lockstep_schedule(orders)
    assert steps == [[2, 1, None, 0], [0, 0, None, 2], [1, None, None, 1], [3, None, None, None]]
    for m, order in enumerate(orders):                     # every trial exactly once, in the model's own order
        assert [s[m] for s in steps if s[m] is not None] == order
    assert lockstep_schedule([]) == [] and lockstep_schedule([[], []]) == []


@pytest.mark.parametrize("shuffle", (True, False))
def test_generators_draw_what_train_decoder_draws(shuffle):
    """Model m of the lock-step epoch loop is handed, step by step, the trials and the masks that train_decoder's loop (randperm, then
    a mask per trial in that order, epoch after epoch, all from one generator) produces from the same seed.  A stub records what
    the step function is handed; no GPU."""
    import torch
    from dss_amd.training import _group_epoch, decoder_dropout_mask
    H, p, epochs = 5, 0.5, 3
    lengths = [[7, 3, 9, 4, 6, 2], [5, 8, 3, 6, 4], [9, 2, 7, 5]]
    seeds = (11, 12, 13)
    want = []
    for m, seed in enumerate(seeds):                       # train_decoder's loop, lines "order = ..." and "m = decoder_dropout_mask(...)"
        gen, mine = torch.Generator().manual_seed(seed), []
        for _ in range(epochs):
            order = torch.randperm(len(lengths[m]), generator=gen).tolist() if shuffle else list(range(len(lengths[m])))
            mine.append([(k, decoder_dropout_mask(lengths[m][k], H, p, gen)) for k in order])
        want.append(mine)
    gens = [torch.Generator().manual_seed(s) for s in seeds]
    for e in range(epochs):
        seen = [[] for _ in seeds]

        def step(trials, masks):
            for m, (k, mk) in enumerate(zip(trials, masks)):
                assert (k is None) == (mk is None)
                if k is not None:
                    seen[m].append((k, mk))
            return len(seen[0])

        steps, out = _group_epoch(step, gens, [len(n) for n in lengths], lengths, H, p, shuffle)
        assert len(steps) == 6 and out == [1, 2, 3, 4, 5, 6]
        assert [sum(k is not None for k in s) for s in steps] == [3, 3, 3, 3, 2, 1]
        for m in range(3):
            assert [k for k, _ in seen[m]] == [k for k, _ in want[m][e]]
            assert sorted(k for k, _ in seen[m]) == list(range(len(lengths[m])))
            for (_, got), (k, ref) in zip(seen[m], want[m][e]):
                assert got.shape == (lengths[m][k], 2 * H) and torch.equal(got, ref)


def test_learning_masks_are_the_group_loop_s_masks():
    """D.learning_masks -- what the tests of train_decoder pin -- is what the lock-step loop hands model 0 with shuffle off."""
    import torch
    from dss_amd.training import _group_epoch
    _, trials, _ = D.learning_problem()
    want = D.learning_masks(trials)
    gens = [torch.Generator().manual_seed(D.LEARN["seed"]), torch.Generator().manual_seed(5)]
    lengths = [[len(y) for _, y in trials], [len(y) for _, y in trials[:2]]]
    for e in range(D.LEARN["epochs"]):
        got = []
        _group_epoch(lambda t, m: got.append(m[0]), gens, [6, 2], lengths, D.LEARN["H"], D.LEARN["dropout"], False)
        assert all(np.array_equal(g.numpy(), w) for g, w in zip(got, want[e]))
