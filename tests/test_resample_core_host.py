"""csrc/resample_core.h as host code: tests/native/resample_core_host.cpp is compiled as a plain executable with the host
address and undefined-behaviour sanitizers (nothing is preloaded) and run over the tables and sources of
resample_cases.py: every variant's plan and its inverse, fp32 and int16 sources for the trilinear routine, all four
element types for the nearest one, a 3-channel source, and the exact r = 0.5 case. The program holds each source in a
buffer of exactly its size and compares every voxel with a direct evaluation; one further case carries table entries
outside the source (-7, n + 5), which the clamp has to keep inside the buffer. An offset outside a source shows here as
a sanitizer report before a kernel forms it.
"""
import os
import shutil
import struct
import subprocess

import numpy as np
import pytest

import resample_cases as K
from u3d.data import RS_F32, RS_I16, RS_I32, RS_U8, spacing_plan

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "native", "resample_core_host.cpp")
INC = os.path.join(REPO, "multimodal-pl_amd", "csrc")

CODES = {np.dtype("uint8"): RS_U8, np.dtype("int16"): RS_I16, np.dtype("int32"): RS_I32, np.dtype("float32"): RS_F32}


def _compiler():
    for cxx in (os.environ.get("CXX"), "g++", "clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


def _record(plan, src, hostile=False):
    src = np.ascontiguousarray(src)
    C = src.shape[0] if src.ndim == 4 else 1
    strides, src_n, chan = plan.source_layout()
    assert src.shape[-3:] == plan.src_shape and src.size == C * chan
    out = struct.pack("<3i", CODES[src.dtype], C, int(hostile))
    out += struct.pack("<3i", *src_n) + struct.pack("<3i", *plan.out_shape)
    out += struct.pack("<3q", *strides) + struct.pack("<2q", chan, src.size)
    for a, (i0, frac, near) in enumerate(plan.tables):
        if hostile:
            i0, near = i0.copy(), near.copy()
            i0[0], near[0] = -7, src_n[a] + 5
            i0[-1], near[-1] = src_n[a] + 5, -7
        out += i0.astype("<i4").tobytes() + frac.astype("<f8").tobytes() + near.astype("<i4").tobytes()
    return out + src.tobytes()


def test_core_routines_equal_the_direct_evaluation(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "resample_core_host"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", INC, SRC, "-o", str(exe)], check=True)
    records = []
    for _, shape, affine, pixdim, _ in K.VARIANTS:
        plan = spacing_plan(shape, affine, pixdim)
        inv = plan.inverse()
        records.append(_record(plan, K.image(shape)))
        records.append(_record(plan, K.image_i16(shape)))
        for dt in K.LABEL_DTYPES:
            records.append(_record(plan, K.label(shape).astype(dt)))
        records.append(_record(inv, K.image(inv.src_shape, "probs", 3)))
    shape, zooms, pixdim, _ = K.EXACT
    records.append(_record(spacing_plan(shape, K.affine_for("LPS", zooms), pixdim), K.image_i16(shape)))
    hostile = 0
    for name in ("half_even_clamp", "size1_axis"):
        shape, zooms, pixdim, _ = K.CASES[name]
        for codes, src in (("LPS", K.image(shape)), ("RAS", K.label(shape).astype("uint8"))):
            records.append(_record(spacing_plan(shape, K.affine_for(codes, zooms), pixdim), src, hostile=True))
            hostile += 1
    data = tmp_path / "cases.bin"
    with open(data, "wb") as f:
        f.write(struct.pack("<i", len(records)))
        for r in records:
            f.write(r)
    r = subprocess.run([str(exe), str(data)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.strip().endswith("ok") and r.stdout.count("case ") == len(records)
    assert r.stdout.count(": 0 voxels differ") == len(records) and r.stdout.count("hostile") == hostile
