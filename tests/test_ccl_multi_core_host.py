"""The multi-label forms of csrc/ccl_core.h as host code: tests/native/ccl_multi_core_host.cpp is compiled as a plain
executable with the host address and undefined-behaviour sanitizers (nothing is preloaded) and run on the code volumes
of postproc_cases.py. It runs the tile-local phase, the seam unions and the flatten in C order, in reverse order and in
a shuffled order over 8 threads; each run must give, per voxel that takes part, the smallest linear index of its
component among the voxels of its own code (a serial flood fill per code inside the program). A mistake in the
lock-free core shows here, as a wrong root, a sanitizer report or a timeout, before a kernel runs it.
"""
import os
import shutil
import struct
import subprocess

import pytest

import postproc_cases as K

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "native", "ccl_multi_core_host.cpp")
INC = os.path.join(REPO, "multimodal-pl_amd", "csrc")


def _compiler():
    for cxx in (os.environ.get("CXX"), "g++", "clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


def test_multi_label_core_gives_minimum_index_roots_per_code_in_every_order(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "ccl_multi_core_host"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-pthread", "-I", INC, SRC, "-o", str(exe)], check=True)
    vols = K.core_volumes()
    data = tmp_path / "volumes.bin"
    with open(data, "wb") as f:
        f.write(struct.pack("<i", len(vols)))
        for codes, num_labels in vols:
            f.write(struct.pack("<4i", *codes.shape, num_labels))
            f.write(codes.tobytes())
    r = subprocess.run([str(exe), str(data)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.strip().endswith("ok") and r.stdout.count("components") == len(vols)
