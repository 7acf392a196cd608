"""Static guard (no GPU): every kernel of the built gfx950 code objects keeps subnormals.  The LPCNet parity contract
("Subnormals, the table's ends, Inf / NaN") relies on gradual underflow like the oracle's plain C: the kernel
descriptors must carry float_denorm_mode_32 = 3 and float_denorm_mode_16_64 = 3, and no kernel may change the MODE
register while it runs.  A build flag such as -fgpu-flush-denormals-to-zero shows up here before any GPU is involved;
tests/test_gpu_lpcnet_regimes.py ('tiny') is the dynamic half.

Uses the LLVM tools that ship with ROCm (llvm-objdump unbundles the fat binary and prints the kernel descriptors as
.amdhsa_ directives); skipped with a reason where they are absent."""
import glob
import os
import re
import shutil
import subprocess

import pytest

from dss_amd import build as dss_build


def _objdump():
    for cand in (shutil.which("llvm-objdump"), "/opt/rocm/lib/llvm/bin/llvm-objdump", "/opt/rocm/llvm/bin/llvm-objdump"):
        if cand and os.path.exists(cand):
            return cand
    return None


def test_every_kernel_descriptor_keeps_subnormals(tmp_path):
    tool = _objdump()
    if tool is None:
        pytest.skip("llvm-objdump not found (looked on PATH and under /opt/rocm): cannot read the kernel descriptors")
    if not os.path.exists(dss_build.LIB_PATH):
        pytest.fail("libdss_hip.so is not built: run __graft_entry__.build() first")
    lib = shutil.copy(dss_build.LIB_PATH, tmp_path / "libdss_hip.so")       # the unbundler writes next to its input
    r = subprocess.run([tool, "--offloading", str(lib)], cwd=tmp_path, capture_output=True, text=True)
    objects = sorted(glob.glob(str(tmp_path / "libdss_hip.so.*gfx950*")))
    if r.returncode != 0 or not objects:
        pytest.skip(f"this llvm-objdump cannot unbundle the library (--offloading): rc {r.returncode} {r.stderr.strip()[:200]}")
    assert len(objects) >= sum(s.endswith(".hip") for s in dss_build.SOURCES), objects      # a code object per kernel file
    kernels = {}
    for obj in objects:
        text = subprocess.run([tool, "-d", "--section=.rodata", obj], capture_output=True, text=True, check=True).stdout
        for m in re.finditer(r"\.amdhsa_kernel (\S+)(.*?)\.end_amdhsa_kernel", text, re.S):
            modes = dict(re.findall(r"\.amdhsa_(float_denorm_mode_32|float_denorm_mode_16_64|float_round_mode_32|"
                                    r"float_round_mode_16_64|ieee_mode|dx10_clamp) (\d+)", m.group(2)))
            kernels[m.group(1)] = modes
        code = subprocess.run([tool, "-d", obj], capture_output=True, text=True, check=True).stdout
        changes = re.findall(r"^\s*(s_denorm_mode|s_round_mode|s_setreg\w*)\b.*$", code, re.M)
        assert not changes, (os.path.basename(obj), "kernel code changes the MODE register", changes[:5])
    for family in ("lpcnet_sample_kernel", "lpcnet_sample_pair_kernel", "lpcnet_sample_generic_kernel", "frame_"):
        assert any(family in k for k in kernels), (family, "no such kernel found: the descriptors were not read")
    print(f"{len(kernels)} kernel descriptors in {len(objects)} code objects")
    assert len(kernels) >= 20
    for name, modes in kernels.items():
        assert modes.get("float_denorm_mode_32") == "3" and modes.get("float_denorm_mode_16_64") == "3", (name, modes)
        assert modes.get("float_round_mode_32") == "0" and modes.get("float_round_mode_16_64") == "0", (name, modes)
