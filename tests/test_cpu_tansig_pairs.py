"""The table pair of the short activations (csrc/lpcnet_device.h), without a GPU.

* The 1 - y*y table the host builds next to the activation table equals numpy's two separately rounded fp32 operations
  bit for bit, and the y table is the oracle's.
* tools/verify/tansig_exhaustive.c (old and short forms restated in C, -ffp-contract=off) is built and run over every 256th
  bit pattern plus +-64 patterns around each of the 201 index boundaries, around zero and around the clamps; it also
  compares the two-operand sign folds on 2^24 operand pairs.  (Stride 1, all 2^32 patterns, takes a few CPU-minutes: see
  profiles/activation_experiment.md for that run; on the device tests/test_gpu_lpcnet_activations.py visits them all.)"""
import ctypes as C
import os
import shutil
import subprocess

import numpy as np
import pytest

from dss_amd.lpcnet_weights import synthetic_blob

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TANSIG_Y = 208


def _tables():
    from dss_amd import _lib
    L = _lib.load()
    out = (C.c_float * (TANSIG_Y + 201))()
    assert L.dss_selftest_tansig_table(out, TANSIG_Y + 201) == 0, L.dss_last_error().decode()
    return np.array(out, dtype=np.float32)


def test_dy_table_is_two_rounded_fp32_operations(oracle):
    t = _tables()
    y, dy = t[:201], t[TANSIG_Y:]
    want_y = oracle.lpcnet_table(oracle.lpcnet_model(synthetic_blob(0)), 0, 201)
    assert np.array_equal(y.view(np.uint32), want_y.view(np.uint32))
    assert not t[201:TANSIG_Y].any()
    yy = (y * y).astype(np.float32)                                  # rounded to fp32 ...
    want = (np.float32(1) - yy).astype(np.float32)                   # ... before the subtraction
    assert yy.dtype == np.float32 and want.dtype == np.float32
    assert np.array_equal(dy.view(np.uint32), want.view(np.uint32))
    # the fused form (one rounding of 1 - y*y) differs in some entry: the comparison above can tell the two apart
    fused = (1.0 - y.astype(np.float64) ** 2).astype(np.float32)
    assert (fused.view(np.uint32) != want.view(np.uint32)).any()
    assert dy[0] == 1 and (dy >= 0).all() and dy[200] == 0           # (the table's last entries are exactly 1)


def test_table_entry_point_checks_its_arguments():
    from dss_amd import _lib
    L = _lib.load()
    out = (C.c_float * 512)()
    assert L.dss_selftest_tansig_table(out, 201) != 0
    assert L.dss_selftest_tansig_table(None, TANSIG_Y + 201) != 0


def test_verifier_strided_sweep_and_edges(tmp_path):
    cc = shutil.which("gcc") or shutil.which("cc")
    if cc is None:
        pytest.fail("no C compiler: tools/verify/tansig_exhaustive.c cannot be built")
    exe = str(tmp_path / "tansig_exhaustive")
    subprocess.check_call([cc, "-O2", "-ffp-contract=off", "-o", exe, os.path.join(ROOT, "tools", "verify", "tansig_exhaustive.c"), "-lm"])
    p = subprocess.run([exe, "256", "edges"], capture_output=True, text=True)
    print(p.stdout, p.stderr)
    assert p.returncode == 0, p.stdout + p.stderr
    assert "patterns visited: 16777216 (stride 256) + 105006 at the edges; tanh mismatches: 0, sigmoid mismatches: 0, NaN lost: 0" in p.stdout
    assert "2^24 pairs: 0 mismatches" in p.stdout
