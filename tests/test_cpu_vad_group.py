"""Several detectors trained at once (Part 15 of include/dss_hip.h, dss_amd/training.py) without a GPU: the exported symbols, the
trial struct against the header, the argument checks at both ends of every limit, what the Python layer refuses before it asks
for a device, and the generator discipline of ``train_vads`` (a model's permutation and masks are those ``train_vad`` draws from
the same seed)."""
import os
import re

import numpy as np
import pytest

import lstm_reference as R
import vad_training_reference as V

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FUNCTIONS = ("dss_vad_group_check", "dss_vad_group_create", "dss_vad_group_destroy", "dss_vad_group_load", "dss_vad_group_read",
             "dss_vad_group_state", "dss_vad_group_publish", "dss_vad_group_window_dev", "dss_vad_group_trial_dev")
TYPES = ("dss_vad_group", "dss_vad_group_trial")           # with the nine functions: the eleven names of Part 15


def _header():
    return open(os.path.join(ROOT, "include", "dss_hip.h")).read()


def test_symbols_are_declared_and_exported():
    from dss_amd import _lib, training
    L = _lib.load()
    text = re.sub(r"/\*.*?\*/", "", _header(), flags=re.S)
    for name in FUNCTIONS:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in _lib.EXPORTED_SYMBOLS and hasattr(L, name), name
    for name in TYPES:
        assert re.search(r"\}\s*%s;|typedef struct %s %s;" % (name, name, name), text), name
    for name in ("VadGroupTrainerGPU", "train_vads"):
        assert name in training.__all__ and hasattr(training, name), name


def test_trial_struct_matches_the_header():
    """The ctypes mirror of dss_vad_group_trial: the header's fields in the header's order, and the 64 bytes of the device-side
    entry (DssVadGroupTrial of csrc/dss_common.h: four pointers, three doubles, two ints)."""
    import ctypes as C
    from dss_amd.training import _VadGroupTrial
    body = re.search(r"typedef struct \{([^}]*)\} dss_vad_group_trial;", _header()).group(1)
    fields = re.findall(r"(\w+)\s*(?:,|;)", body)
    assert [n for n, _ in _VadGroupTrial._fields_] == fields
    assert C.sizeof(_VadGroupTrial) == 4 * C.sizeof(C.c_void_p) + 3 * C.sizeof(C.c_double) + 2 * C.sizeof(C.c_int) == 64
    dev = re.search(r"struct DssVadGroupTrial \{(.*?)\n\};", open(os.path.join(ROOT, "delayed-speech-synthesis_amd", "csrc",
                                                                                 "dss_common.h")).read(), flags=re.S).group(1)
    dev = re.sub(r"//[^\n]*", "", dev)
    assert re.findall(r"(\w+)\s*(?:,|;)", dev) == ["frames", "targets", "mask", "losses", "lr", "alpha", "eps", "len", "apply"]


@pytest.mark.parametrize("args, ok, reason", [
    ((1, 64, 150, 50), True, None),
    ((64, 128, 160, 4096), True, None),                    # the upper end of every limit
    ((1, 1, 1, 1), True, None),                            # the lower end
    ((0, 64, 150, 50), False, "0 models"),
    ((65, 64, 150, 50), False, "65 models"),
    ((-1, 64, 150, 50), False, "-1 models"),
    ((2, 129, 150, 50), False, "129 inputs"),
    ((2, 0, 150, 50), False, "0 inputs"),
    ((2, 64, 161, 50), False, "161 hidden units"),
    ((2, 64, 0, 50), False, "0 hidden units"),
    ((2, 64, 150, 4097), False, "max_window 4097"),
    ((2, 64, 150, 0), False, "max_window 0"),
])
def test_group_check_at_both_ends_of_every_limit(args, ok, reason):
    from dss_amd import _lib
    L = _lib.load()
    rc = L.dss_vad_group_check(*args)
    if ok:
        assert rc == 0, L.dss_last_error().decode()
    else:
        assert rc == -1
        assert reason in L.dss_last_error().decode(), L.dss_last_error().decode()


def test_class_refuses_without_a_device_call():
    """Sizes are checked before a device is asked for: 65 models, models of two sizes, no model, a window beyond the kernels'."""
    from dss_amd import _lib, training
    sd = R.vad_state_dict(6, 5, 1)
    with pytest.raises(_lib.DssError, match="65 models"):
        training.VadGroupTrainerGPU([sd] * 65, max_window=8)
    with pytest.raises(_lib.DssError, match="0 models"):
        training.VadGroupTrainerGPU([], max_window=8)
    with pytest.raises(ValueError, match="other sizes"):
        training.VadGroupTrainerGPU([sd, R.vad_state_dict(8, 5, 1)], max_window=8)
    with pytest.raises(_lib.DssError, match="max_window 4097"):
        training.VadGroupTrainerGPU([sd], max_window=4097)


def test_train_vads_refuses_bad_arguments_without_a_device_call():
    from dss_amd.training import train_vads
    sd, _, corpus = V.learning_problem()
    with pytest.raises(ValueError, match="train_corpora: 1 entries for 2 models"):
        train_vads([sd, sd], [corpus], [corpus, corpus])
    with pytest.raises(ValueError, match="valid_corpora: 3 entries for 2 models"):
        train_vads([sd, sd], [corpus, corpus], [corpus] * 3)
    with pytest.raises(ValueError, match="seeds: 1 entries for 2 models"):
        train_vads([sd, sd], [corpus, corpus], [corpus, corpus], seeds=[4])
    with pytest.raises(ValueError, match="lr: 3 entries for 2 models"):
        train_vads([sd, sd], [corpus, corpus], [corpus, corpus], lr=[1e-3] * 3)
    with pytest.raises(ValueError, match="mask_source"):
        train_vads([sd, sd], [corpus, corpus], [corpus, corpus], mask_source="gpu")


@pytest.mark.parametrize("shuffle", (True, False))
def test_generators_draw_what_train_vad_draws(shuffle):
    """Model m of the lock-step epoch loop, with the detector's mask function and width, is handed step by step the trials and the
    (len, H) masks that train_vad's loop (randperm, then a mask per trial in that order, epoch after epoch, all from one generator)
    produces from the same seed.  A stub records what the step function is handed; no GPU."""
    import torch
    from dss_amd.training import _group_epoch, dropout_mask
    H, p, epochs = 5, 0.5, 3
    lengths = [[7, 3, 9, 4, 6, 2], [5, 8, 3, 6, 4], [9, 2, 7, 5]]
    seeds = (11, 12, 13)
    want = []
    for m, seed in enumerate(seeds):
        gen, mine = torch.Generator().manual_seed(seed), []
        for _ in range(epochs):
            order = torch.randperm(len(lengths[m]), generator=gen).tolist() if shuffle else list(range(len(lengths[m])))
            mine.append([(k, dropout_mask(lengths[m][k], H, p, gen)) for k in order])
        want.append(mine)
    gens = [torch.Generator().manual_seed(s) for s in seeds]
    for e in range(epochs):
        seen = [[] for _ in seeds]

        def step(trials, masks):
            for m, (k, mk) in enumerate(zip(trials, masks)):
                assert (k is None) == (mk is None)
                if k is not None:
                    seen[m].append((k, mk))

        steps, _ = _group_epoch(step, gens, [len(n) for n in lengths], lengths, H, p, shuffle, None, dropout_mask, H)
        assert [sum(k is not None for k in s) for s in steps] == [3, 3, 3, 3, 2, 1]
        for m in range(3):
            assert [k for k, _ in seen[m]] == [k for k, _ in want[m][e]]
            for (_, got), (k, ref) in zip(seen[m], want[m][e]):
                assert got.shape == (lengths[m][k], H) and torch.equal(got, ref)


def test_learning_masks_are_the_group_loop_s_masks():
    """V.learning_masks -- what the tests of train_vad pin -- is what the lock-step loop hands model 0 with shuffle off."""
    import torch
    from dss_amd.training import _group_epoch, dropout_mask
    _, trials, _ = V.learning_problem()
    want = V.learning_masks(trials)
    gens = [torch.Generator().manual_seed(V.LEARN["seed"]), torch.Generator().manual_seed(5)]
    lengths = [[len(y) for _, y in trials], [len(y) for _, y in trials[:2]]]
    for e in range(V.LEARN["epochs"]):
        got = []
        _group_epoch(lambda t, m: got.append(m[0]), gens, [6, 2], lengths, V.LEARN["H"], V.LEARN["dropout"], False, None, dropout_mask,
                     V.LEARN["H"])
        assert all(np.array_equal(g.numpy(), w) for g, w in zip(got, want[e]))
