"""csrc/edt_core.h as host code: tests/native/edt_core_host.cpp is compiled as a plain executable with the host address
and undefined-behaviour sanitizers (nothing is preloaded) and run on the patterns of surface_cases.py. It runs the three
passes of the distance transform serially, tile by tile as the kernels do, and compares every voxel with a brute force
over all features inside the program: squared distances are exact for integer spacings. It also runs lines of length 1,
2 and the largest extent. An out-of-bounds index in a per-line routine shows here as a sanitizer report before a kernel
runs it.
"""
import os
import shutil
import struct
import subprocess

import pytest

import surface_cases as K

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "native", "edt_core_host.cpp")
INC = os.path.join(REPO, "multimodal-pl_amd", "csrc")

# the brute force is O(V * features): small volumes, among them a 65-wide tile edge, a two-word row and a 129-long line
SHAPES = [(1, 1, 1), (4, 5, 6), (3, 2, 70), (2, 65, 3), (129, 2, 2), (9, 8, 8), (5, 3, 130)]


def _compiler():
    for cxx in (os.environ.get("CXX"), "g++", "clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


def test_three_passes_equal_the_brute_force(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "edt_core_host"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", INC, SRC, "-o", str(exe)], check=True)
    vols = [(K.pattern(p, s), sp) for s in SHAPES for p in K.PATTERNS for sp in K.SPACINGS]
    data = tmp_path / "volumes.bin"
    with open(data, "wb") as f:
        f.write(struct.pack("<i", len(vols)))
        for m, sp in vols:
            f.write(struct.pack("<3i", *m.shape))
            f.write(struct.pack("<3d", *sp))
            f.write(m.tobytes())
    r = subprocess.run([str(exe), str(data)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.strip().endswith("ok") and r.stdout.count("volume ") == len(vols)
    assert r.stdout.count("exact") == len(SHAPES) * len(K.PATTERNS) * len(K.INTEGER_SPACINGS)
