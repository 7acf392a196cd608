"""The heap form of the sampling-tree walk of the CU-resident sample kernels (csrc/lpcnet_sample_common.h DSS_TREE_WALK_AT: the
node index carries its level marker, n = n + n + bit(n), 19 scalar instructions) against the prefix form it replaces (24) and a
plain walk over the nodes.

tools/verify/tree_walk_check.c restates both instruction sequences in C, SCC and the six-bit index of s_bitcmp1_b64 included.
Every leaf is spelled on its path with the 248 off-path bits random, a seeded few thousand masks per leaf: all three walks must
return the leaf.  Then fully random masks: all three must agree.  The GPU side is tests/test_gpu_lpcnet_serial_path.py, which
forces every excitation value through the kernels."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_heap_walk_equals_prefix_walk(tmp_path):
    gcc = shutil.which("gcc") or shutil.which("cc")
    if gcc is None:
        pytest.skip("no C compiler")
    exe = str(tmp_path / "tree_walk")
    subprocess.check_call([gcc, "-O2", "-o", exe, os.path.join(ROOT, "tools", "verify", "tree_walk_check.c")])
    out = subprocess.run([exe, "3000", "500000", "7"], capture_output=True, text=True)
    assert out.returncode == 0, out.stdout + out.stderr
    assert "256 x 3000, mismatches: 0;" in out.stdout and "random masks: 500000, mismatches: 0" in out.stdout, out.stdout
