"""Generate the G20 atlas-construction fixture by running the REFERENCE's own lines on the CPU (test infrastructure, run
where the reference is present, as tests/golden/gen_golden.py whose shims it imports):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_atlas_build.py

  g20_atlas_build.npz, per case <name> of tests/atlas_build_cases.py::FIXTURES
    <name>_total_shape   preprocess/atlas_gen_mm.py:100-111 (the rounded mean shape)
    <name>_count         the per-label case counts of :114-136
    <name>_sums          catlas as :114-136 leave it, captured before :138 (small integers: stored as uint8, asserted)
    <name>_atlas         the float64 atlas after :138-145 (normalise, gaussian_filter(sigma=3))
    <name>_insum         a checksum of the input volumes

The lines are exec'd with SimpleITK stubbed: ReadImage returns the case's key, GetArrayFromImage its array. Only outputs
are stored: inputs are rebuilt from seeds by tests/atlas_build_cases.py.
"""
import os
import sys
import types

import numpy as np
import scipy.ndimage as ndimage
from scipy.ndimage import gaussian_filter

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_golden as G  # noqa: E402  (reference path + shims)
import atlas_build_cases as BC  # noqa: E402

FNAME = "preprocess/atlas_gen_mm.py"


def run_case(name, out):
    vols = {f"case{i}.nii.gz": v for i, v in enumerate(BC.fixture_volumes(name))}
    sitk = types.SimpleNamespace(ReadImage=lambda key: key, GetArrayFromImage=lambda key: vols[key].copy())
    src_sum = G._ref_lines(FNAME, 100, 136)
    src_fin = G._ref_lines(FNAME, 138, 145)
    assert "total_shape = [int(np.round(s)) for s in total_shape]" in src_sum and "ndimage.zoom(label_mask," in src_sum
    assert "count[label_idx-1] += 1" in src_sum and "gaussian_filter(catlas[i], sigma=3)" in src_fin, \
        "reference lines moved"
    env = {"np": np, "os": os, "sitk": sitk, "ndimage": ndimage, "gaussian_filter": gaussian_filter,
           "training_files": list(vols), "print": lambda *a, **k: None}
    exec(compile(src_sum, FNAME + ":100-136", "exec"), env)
    sums = env["catlas"].copy()
    assert sums.dtype == np.float64 and np.array_equal(sums.astype(np.uint8).astype(np.float64), sums)
    exec(compile(src_fin, FNAME + ":138-145", "exec"), env)
    assert env["catlas"].dtype == np.float64 and list(env["catlas"].shape[1:]) == env["total_shape"]
    out[f"{name}_total_shape"] = np.array(env["total_shape"], dtype=np.int64)
    out[f"{name}_count"] = env["count"].reshape(-1).astype(np.int64)
    out[f"{name}_sums"] = sums.astype(np.uint8)
    out[f"{name}_atlas"] = env["catlas"]
    out[f"{name}_insum"] = np.array(BC.checksum(*vols.values()))


if __name__ == "__main__":
    out = {}
    for name in BC.FIXTURES:
        run_case(name, out)
    G.save("g20_atlas_build.npz", **out)
