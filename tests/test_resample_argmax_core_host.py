"""rs::argmax_trilinear of csrc/resample_core.h as host code: tests/native/resample_argmax_core_host.cpp is compiled as a
plain executable with the host address and undefined-behaviour sanitizers (nothing is preloaded) and run over the
inverse plans of resample_cases.py, whole and restricted to a crop of the source, with the scores
resample_cases.image(shape, "probs", C) for C = 1, 2 and 14. Further cases carry a duplicated channel (the lower index
has to win the tie), NaN voxels (the first NaN wins, as in torch.argmax) and a channel-last source (strides that are no
contiguous [C, A0, A1, A2]). The program holds each source in a buffer of exactly its size and compares every voxel
with a direct fp64 evaluation of the contract.
"""
import os
import re
import shutil
import struct
import subprocess

import numpy as np
import pytest

import resample_cases as K
from u3d.data import spacing_plan

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SRC = os.path.join(REPO, "tests", "native", "resample_argmax_core_host.cpp")
INC = os.path.join(REPO, "multimodal-pl_amd", "csrc")


def _compiler():
    for cxx in (os.environ.get("CXX"), "g++", "clang++"):
        if cxx and shutil.which(cxx):
            return shutil.which(cxx)
    return None


def _record(plan, src, channel_last=False):
    """src [C, A0, A1, A2] fp32 with A = plan.src_shape; channel_last stores it as [A0, A1, A2, C]."""
    C = src.shape[0]
    assert src.shape[1:] == plan.src_shape and src.dtype == np.float32
    strides, src_n, chan = plan.source_layout()
    if channel_last:
        src = np.ascontiguousarray(np.moveaxis(src, 0, -1))
        strides, chan = tuple(s * C for s in strides), 1
    out = struct.pack("<i", C) + struct.pack("<3i", *src_n) + struct.pack("<3i", *plan.out_shape)
    out += struct.pack("<3q", *strides) + struct.pack("<2q", chan, src.size)
    for i0, frac, _ in plan.tables:
        out += i0.astype("<i4").tobytes() + frac.astype("<f8").tobytes()
    return out + np.ascontiguousarray(src).tobytes()


def test_argmax_trilinear_equals_the_direct_evaluation(tmp_path):
    cxx = _compiler()
    if cxx is None:
        pytest.skip("no host C++ compiler")
    exe = tmp_path / "resample_argmax_core_host"
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    "-I", INC, SRC, "-o", str(exe)], check=True)
    records, want_ties, want_nans = [], [], []
    for n, (_, shape, affine, pixdim, _) in enumerate(K.VARIANTS):
        inv = spacing_plan(shape, affine, pixdim).inverse()
        for C in (1, 2, 14):
            records.append(_record(inv, K.image(inv.src_shape, "probs", C)))
            want_ties.append(False), want_nans.append(False)
        # a crop of the source: the restricted plan clamps at the crop's border
        origin = tuple(s // 3 for s in inv.src_shape)
        box = tuple(max(1, s - o - s // 4) for s, o in zip(inv.src_shape, origin))
        plan_w, _ = inv.restrict_source(origin, box)
        x = K.image(inv.src_shape, "probs", 14)
        crop = np.ascontiguousarray(x[:, origin[0]:origin[0] + box[0], origin[1]:origin[1] + box[1],
                                      origin[2]:origin[2] + box[2]])
        records.append(_record(plan_w, crop, channel_last=n % 2 == 1))
        want_ties.append(False), want_nans.append(False)
        dup = x.copy()
        dup[9], dup[5] = dup[2], dup[2]                          # three holders of one value: channel 2 wins its ties
        records.append(_record(inv, dup))
        want_ties.append(True), want_nans.append(False)
        records.append(_record(inv, np.stack([x[0], x[0]])))     # C = 2, every voxel a tie
        want_ties.append(True), want_nans.append(False)
        nan = x.copy()
        g = np.random.default_rng([33, n])
        idx = g.integers(0, nan.size, max(4, nan.size // 40))
        nan.reshape(-1)[idx] = np.float32("nan")
        records.append(_record(inv, nan, channel_last=n % 2 == 0))
        want_ties.append(False), want_nans.append(True)
    data = tmp_path / "cases.bin"
    with open(data, "wb") as f:
        f.write(struct.pack("<i", len(records)))
        for r in records:
            f.write(r)
    r = subprocess.run([str(exe), str(data)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert r.stdout.strip().endswith("ok")
    lines = re.findall(r"^case \d+ .*: (\d+) voxels differ, (\d+) ties, (\d+) nans$", r.stdout, re.M)
    assert len(lines) == len(records)
    for (bad, ties, nans), wt, wn in zip(lines, want_ties, want_nans):
        assert int(bad) == 0
        assert (int(ties) > 0) == wt and (int(nans) > 0) == wn, (ties, nans, wt, wn)   # the cases hold what they claim
