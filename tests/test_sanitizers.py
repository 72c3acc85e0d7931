"""Host stage under AddressSanitizer + UBSan and under ThreadSanitizer (CPU build; the GPU pool offers no sanitizers)."""
import os
import re
import shutil
import struct
import subprocess

import pytest

import degenerate_sets
import util

CSRC = os.path.join(util.ROOT, util.PKG, "csrc")
SAN_MAX_POINTS = 20000  # the sanitizer programs leave out the two 4K lattices (331 776 points); the plain host and GPU tests keep them


def _corpus_file(tmp_path, max_points=None):
    """The structured vertex sets of tests/degenerate_sets.py in the form tests/corpus_file.h reads; returns (path, number of sets)."""
    items = list(degenerate_sets.sets(max_points))
    path = str(tmp_path / "corpus.bin")
    with open(path, "wb") as f:
        f.write(struct.pack("<i", len(items)))
        for name, xy in items:
            f.write(struct.pack("<i", len(name)) + name.encode() + struct.pack("<i", len(xy)) + xy.astype("<i4").tobytes())
    return path, len(items)


def _corpus_sets_run(stdout):
    m = re.search(r"^corpus sets: (\d+)", stdout, re.M)
    return int(m.group(1)) if m else -1


@pytest.mark.parametrize("san", ["address,undefined", "thread"])
def test_host_stage_sanitizers(tmp_path, san):
    """... and the structured sets of tests/degenerate_sets.py (all but the two 4K lattices): sequential triangulation against halves,
    quarters and eighths with early and late helpers, and the preparation alone."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "san_host")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-mavx2", "-fsanitize=" + san, "-fno-omit-frame-pointer", "-ffp-contract=off",
           "-I" + os.path.join(util.ROOT, "include"), "-I" + CSRC, "-I" + util.HERE, os.path.join(util.HERE, "san_host.cpp"), os.path.join(CSRC, "host_stage.cpp"),
           "-o", exe, "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "sanitizer" in (r.stderr or "").lower() and "cannot find" in r.stderr:
        pytest.skip("sanitizer runtime not installed")
    assert r.returncode == 0, r.stderr[-2000:]
    corpus, n_sets = _corpus_file(tmp_path, SAN_MAX_POINTS)
    exe = [exe, corpus]
    r = subprocess.run(exe, capture_output=True, text=True, timeout=600)
    if san == "thread" and r.returncode != 0 and "unexpected memory mapping" in r.stderr and shutil.which("setarch"):
        # GCC's ThreadSanitizer runtime does not fit its shadow layout around kernels with more mmap randomisation bits:
        # the same binary again with address randomisation off for this one process (a personality flag, nothing system-wide)
        r = subprocess.run(["setarch", os.uname().machine, "-R"] + exe, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0 and "mismatches: 0" in r.stdout, (r.stdout[-500:], r.stderr[-3000:])
    assert _corpus_sets_run(r.stdout) == n_sets and n_sets >= 580, r.stdout[-500:]


def test_gpu_delaunay_logic_emulated_on_cpu(tmp_path):
    """The device functions of csrc/delaunay_gpu.hip (leaf construction, merge, tree / slot arithmetic) compiled as plain C++ and
    run depth by depth with the nodes of a depth in reversed order, against Delaunay::triangulate, under ASan + UBSan: random sets and the
    structured sets of tests/degenerate_sets.py, each whole in LDS where it fits and cut with subtree limits of 6, 50, 333 and 4000
    vertices (every cut depth from 1 to 6).  Every loop trip of a merge counts against a bound derived from the node's size (emulation
    only): a seam walk that would not end on the GPU fails here with the set's name.  The two 4K lattices (331 776 vertices) are beyond
    both device paths (256 000) and only reported."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "emu_dg")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-mavx2", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-ffp-contract=off", "-x", "c++",
           "-I" + os.path.join(util.ROOT, "include"), "-I" + CSRC, "-I" + util.HERE, os.path.join(util.HERE, "emu_delaunay_gpu.cpp"), os.path.join(CSRC, "host_stage.cpp"),
           "-o", exe, "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "cannot find" in (r.stderr or ""):
        pytest.skip("sanitizer runtime not installed")
    assert r.returncode == 0, r.stderr[-2000:]
    corpus, n_sets = _corpus_file(tmp_path)
    r = subprocess.run([exe, corpus], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "mismatches: 0" in r.stdout and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout[-1500:], r.stderr[-3000:])
    assert _corpus_sets_run(r.stdout) == n_sets and n_sets >= 590 and "beyond both paths: 2)" in r.stdout, r.stdout[-500:]


def test_gpu_vertex_preparation_emulated_on_cpu(tmp_path):
    """The workgroup-cooperative preparation of csrc/delaunay_gpu.hip (dg_prepare in LDS, dg_prepare_global in scratch: bit maps, u16
    rank prefixes, in-place partitions) compiled unchanged and run as one fiber per GPU thread under ASan + UBSan, in buffers of exactly
    the size the launchers request, against Delaunay::kd_ordered_ids: the corner row, negative x on the right side, coincident groups up
    to the limit and beyond, DG_PREP_MAX vertices and one more, a vertex off the bit maps, 4K-sized sets with 1 024 threads; every
    thread of a workgroup must return the same value after the same number of barriers.  And the structured sets of
    tests/degenerate_sets.py that lie on a support lattice (collinear rows and columns, fans, strips, collinear halves, complete
    lattices; sorted, shuffled, at negative x, with coincident points)."""
    if not shutil.which("g++"):
        pytest.skip("no g++")
    exe = str(tmp_path / "emu_prep")
    cmd = ["g++", "-O1", "-g", "-std=c++17", "-mavx2", "-fsanitize=address,undefined", "-fno-omit-frame-pointer", "-ffp-contract=off", "-x", "c++",
           "-I" + os.path.join(util.ROOT, "include"), "-I" + CSRC, "-I" + util.HERE, os.path.join(util.HERE, "emu_dg_prepare.cpp"), os.path.join(CSRC, "host_stage.cpp"),
           "-o", exe, "-lpthread"]
    r = subprocess.run(cmd, capture_output=True, text=True)
    if r.returncode != 0 and "cannot find" in (r.stderr or ""):
        pytest.skip("sanitizer runtime not installed")
    assert r.returncode == 0, r.stderr[-2000:]
    corpus, n_sets = _corpus_file(tmp_path)
    r = subprocess.run([exe, "1", corpus], capture_output=True, text=True, timeout=900)
    assert r.returncode == 0 and "mismatches: 0" in r.stdout and "ERROR: AddressSanitizer" not in r.stderr and "runtime error" not in r.stderr, (r.stdout[-500:], r.stderr[-3000:])
    assert _corpus_sets_run(r.stdout) == n_sets == 592, r.stdout[-500:]
    # every set is accounted for: the ones the preparation is not defined for are counted from the corpus here (rows off the lattice of
    # step 5; more vertices than its 16-bit ids), all others were emulated - in LDS where the bit maps fit, else in global scratch
    sets = list(degenerate_sets.sets())
    off = sum(1 for _, xy in sets if (xy[:, 1] % 5).any())
    large = sum(1 for _, xy in sets if not (xy[:, 1] % 5).any() and len(xy) > 0xFFFF)
    assert (off, large) == (50, 2)
    assert "(in LDS: 462, in global scratch: 78, off the lattice: %d, beyond 65535 vertices: %d)" % (off, large) in r.stdout, r.stdout[-500:]
