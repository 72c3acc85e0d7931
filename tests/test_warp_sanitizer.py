"""The host layer of the temporal warp (csrc/warp.cpp: every argument check of group (AA)) under AddressSanitizer + UBSan, as a
stand-alone CPU program with the kernels' launcher stubbed (tests/san_warp.cpp): each bad word of the spec, NULL, misaligned and
overlapping pointers, the batch, shape and workspace limits are refused before the launcher is reached, and the admitted calls reach it."""
import os
import shutil
import subprocess

import pytest

import util

CSRC = os.path.join(util.ROOT, util.PKG, "csrc")


def test_warp_argument_checks_under_sanitizers(tmp_path):
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "san_warp")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-ffp-contract=off", "-D__HIP_PLATFORM_AMD__",
           "-I/opt/rocm/include", "-I" + os.path.join(util.ROOT, "include"), "-I" + CSRC, os.path.join(util.HERE, "san_warp.cpp"), os.path.join(CSRC, "warp.cpp"), "-o", exe]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "cannot find" in (r.stderr or ""):
        pytest.skip("sanitizer runtime not installed")
    assert r.returncode == 0, r.stderr[-2000:]
    r = subprocess.run([exe], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0 and "mismatches: 0" in r.stdout and "launches: 3" in r.stdout, (r.stdout[-1500:], r.stderr[-3000:])
    assert "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, r.stderr[-3000:]
