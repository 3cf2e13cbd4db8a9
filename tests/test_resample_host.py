"""Host-side contract of the orientation / spacing resampling (no device). The restatement resample_reference.py equals
the engine MONAI calls (torch's grid_sample on CPU float64 tensors, align_corners, border padding) and scipy's
map_coordinates; u3d.data's plans equal the restatement's, integers exactly and floats bit for bit; plans preserve
world positions under all 48 signed axis permutations and an oblique affine, and plan.inverse() undoes the plan; bad
inputs are rejected; the header, the signature table, the Makefile and INTEGRATION.md name the native entry points.
Parity with one MONAI release is not pinned (monai is not installed): the contract is the formulas."""
import inspect
import itertools
import os
import re

import numpy as np
import pytest
import torch
import torch.nn.functional as F
from scipy import ndimage

import resample_cases as K
import resample_reference as R
from conftest import PKG, REPO

ENTRY_POINTS = ["u3d_grid_resample_linear", "u3d_grid_resample_nearest"]


def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def _grid_sample(vol, p, mode):
    """grid_sample of the reoriented float64 volume at the plan's coordinates; a size-1 axis is normalised to 0."""
    v = np.ascontiguousarray(R.reorient(vol, p)).astype(np.float64)
    g = [2.0 * c / (n - 1) - 1.0 if n > 1 else np.zeros_like(c) for c, n in zip(R.coordinates(p), v.shape)]
    G = torch.stack(torch.meshgrid(*(torch.from_numpy(a) for a in g), indexing="ij"), dim=-1)[..., [2, 1, 0]]
    out = F.grid_sample(torch.from_numpy(v)[None, None], G[None], mode=mode, padding_mode="border", align_corners=True)
    return out[0, 0].numpy()


@pytest.mark.parametrize("vid", K.IDS)
def test_restatement_equals_grid_sample_and_map_coordinates(vid):
    _, shape, affine, pixdim, _ = K.VARIANTS[K.IDS.index(vid)]
    fwd = R.plan(shape, affine, pixdim)
    for p in (fwd, R.inverse(fwd)):
        x = K.image(p["src_shape"])
        want = R.sample_linear(x, p)
        tol = 1e-9 * np.abs(x).max()
        gs = _grid_sample(x, p, "bilinear")
        mc = ndimage.map_coordinates(np.ascontiguousarray(R.reorient(x, p)).astype(np.float64),
                                     np.meshgrid(*R.coordinates(p), indexing="ij"), order=1, mode="nearest")
        print(f"{vid}: linear max|d| grid_sample {np.abs(want - gs).max():.2e}, map_coordinates "
              f"{np.abs(want - mc).max():.2e}, bound {tol:.2e}")
        assert want.shape == p["out_shape"] == gs.shape == mc.shape
        assert np.abs(want - gs).max() <= tol and np.abs(want - mc).max() <= tol
        lab = K.label(p["src_shape"])
        near, gn = R.sample_nearest(lab, p), _grid_sample(lab, p, "nearest")
        if p is fwd:
            assert np.array_equal(near, gn)              # half-integer coordinates included (half_coords)
        else:
            # the inverse's coordinates k / r are not this test's subject: grid_sample takes them through
            # 2 c / (n - 1) - 1 and back, which moves c by about 1e-14 n, so its rounding of an exact half (7.5 of
            # 174) is decided by that noise; everywhere else it must agree
            off = [np.abs(c - np.floor(c) - 0.5) > 1e-9 for c in R.coordinates(p)]
            sure = off[0][:, None, None] & off[1][None, :, None] & off[2][None, None, :]
            assert np.array_equal(near[sure], gn[sure]) and sure.any()


def test_half_integer_coordinates_round_to_even():
    shape, zooms, pixdim, _ = K.CASES["half_coords"]
    c = R.coordinates(R.plan(shape, K.affine_for("RAS", zooms), pixdim))
    assert c[0].tolist() == [0, 0.5, 1, 1.5, 2, 2.5, 3] and c[2].tolist() == [0, 2, 4, 5]      # 6 clamps to 5
    assert np.rint(c[0]).tolist() == [0, 0, 1, 2, 2, 2, 3]


def _same_plan(got, want):
    assert got.src_shape == want["src_shape"] and got.out_shape == want["out_shape"]
    assert got.perm == want["perm"] and got.flip == want["flip"]
    assert np.array_equal(np.array(got.scale).view(np.uint64), np.array(want["scale"]).view(np.uint64))
    assert np.array_equal(np.array(got.offset), np.array(want["offset"]))
    assert np.array_equal(got.out_affine.view(np.uint64), want["out_affine"].view(np.uint64))
    for i, (g, w) in enumerate(zip(got.tables, R.tables(want))):
        n = want["src_shape"][want["perm"][i]]
        for a, b, dt in zip(g, w, (np.int32, np.float64, np.int32)):
            assert a.dtype == dt == b.dtype and a.shape == (want["out_shape"][i],)
        assert np.array_equal(g[0], w[0]) and np.array_equal(g[2], w[2])
        assert np.array_equal(g[1].view(np.uint64), w[1].view(np.uint64))
        # the tables' contract with the kernels
        assert g[0].min() >= 0 and g[0].max() <= max(n - 2, 0) and g[2].min() >= 0 and g[2].max() <= n - 1
        assert g[1].min() >= 0 and g[1].max() <= 1


@pytest.mark.parametrize("vid", K.IDS)
def test_plans_equal_the_restatement(vid):
    from u3d.data import axcodes_of, orientation_of, spacing_plan
    _, shape, affine, pixdim, expected = K.VARIANTS[K.IDS.index(vid)]
    want = R.plan(shape, affine, pixdim)
    got = spacing_plan(shape, affine, pixdim)
    assert got.out_shape == expected
    _same_plan(got, want)
    _same_plan(got.inverse(), R.inverse(want))
    assert list(orientation_of(affine)) == R.io_orientation(affine) and axcodes_of(affine) == R.axcodes(affine)
    assert not got.identity
    forced = spacing_plan(shape, affine, pixdim, out_shape=(3, 2, 5))
    _same_plan(forced, R.plan(shape, affine, pixdim, out_shape=(3, 2, 5)))
    kept = spacing_plan(shape, affine, (None, 1.5, None))
    _same_plan(kept, R.plan(shape, affine, (None, 1.5, None)))
    assert kept.scale[0] == 1.0 and kept.out_shape[0] == shape[kept.perm[0]]


def test_axcodes_and_identity():
    from u3d.data import axcodes_of, spacing_plan
    for codes in ("RAS", "LPS", "LAS", "SRA", "IPL") + K.PERMUTED:
        assert axcodes_of(K.affine_for(codes, (0.5, 2.0, 3.0))) == codes
    assert len(set(K.PERMUTED)) == 6
    assert spacing_plan((4, 5, 6), K.affine_for("RAS", (1, 1, 2))).identity
    assert spacing_plan((4, 5, 6), K.affine_for("RAS", (1, 1, 1)), 1).identity                    # a scalar pixdim
    assert spacing_plan((4, 5, 6), K.affine_for("LPS", (3, 1, 2)), (None, None, None), "LPS").identity
    assert not spacing_plan((4, 5, 6), K.affine_for("LAS", (1, 1, 2))).identity
    assert not spacing_plan((4, 5, 6), K.affine_for("RAS", (1, 1, 2)), out_shape=(4, 5, 7)).identity
    p = spacing_plan((4, 5, 6), K.affine_for("SRA", (1, 1, 2)), (1, 1, 2), "SRA")                 # another target
    assert p.identity and axcodes_of(p.out_affine) == "SRA"


def _world_cases():
    g = np.random.default_rng(2711)
    for perm in itertools.permutations(range(3)):
        for signs in itertools.product((0, 1), repeat=3):
            codes = "".join(("LR", "PA", "IS")[w][s] for w, s in zip(perm, signs))
            zooms = g.uniform(0.3, 4.0, 3)
            yield codes, tuple(int(v) for v in g.integers(2, 40, 3)), K.affine_for(codes, zooms, g.uniform(-200, 200, 3))
    yield "oblique", (9, 11, 13), K.oblique_affine((0.8, 1.7, 3.1))


def test_world_positions_are_preserved():
    from u3d.data import axcodes_of, spacing_plan
    g = np.random.default_rng(2712)
    count = 0
    for name, shape, affine in _world_cases():
        plan = spacing_plan(shape, affine)
        ref = R.plan(shape, affine)
        assert axcodes_of(plan.out_affine) == "RAS", name
        inv = plan.inverse()
        n = np.array(plan.out_shape)
        ks = [np.array(c) * (n - 1) for c in itertools.product((0, 1), repeat=3)] + [g.integers(0, n) for _ in range(8)]
        for k in ks:
            j = R.source_index(ref, k)
            out_w = plan.out_affine @ np.append(k, 1.0)
            src_w = affine @ np.append(j, 1.0)
            assert np.abs(out_w - src_w).max() <= 1e-9 * max(1.0, np.abs(src_w).max()), (name, k)
            # u3d's own coordinates, wherever the clamp does not act, agree with the restatement's
            for i in range(3):
                a, c = plan.perm[i], plan.source_coordinate(i, k[i])
                raw = R.raw_coordinate(ref, i, k[i])
                if 0 <= raw <= shape[a] - 1:
                    assert c == raw
            # inverse(plan(k)) == k: the inverse's coordinate of the (real-valued) source index j
            back = [inv.scale[a] * j[a] + inv.offset[a] for a in range(3)]
            assert [inv.perm[a] for a in range(3)] == [plan.perm.index(a) for a in range(3)]
            for a in range(3):
                assert abs(back[a] - k[inv.perm[a]]) <= 1e-9 * max(1.0, abs(k[inv.perm[a]])), (name, k, a)
        assert inv.out_shape == tuple(shape) and inv.src_shape == plan.out_shape
        assert np.array_equal(inv.out_affine, affine) and np.array_equal(inv.src_affine, plan.out_affine)
        count += 1
    assert count == 49


def test_rejected_inputs():
    from u3d import U3DError
    from u3d.data import GridPlan, axcodes_of, preprocess_case, resample_spacing, spacing_plan
    A = K.affine_for("RAS", (1, 1, 2))
    for pixdim in ((1, 0, 2), (1, -1, 2), (1, float("nan"), 2), (float("inf"), 1, 2), (1, 2)):
        with pytest.raises(ValueError):
            spacing_plan((4, 5, 6), A, pixdim)
    singular = A.copy()
    singular[:3, 1] = singular[:3, 0]
    bad = A.copy()
    bad[0, 0] = np.nan
    for aff in (singular, bad, np.zeros((4, 4)), np.eye(3)):
        with pytest.raises(ValueError):
            spacing_plan((4, 5, 6), aff)
        with pytest.raises(ValueError):
            axcodes_of(aff)
    for codes in ("RAX", "RAR", "RA", "RASS"):
        with pytest.raises(ValueError):
            spacing_plan((4, 5, 6), A, axcodes=codes)
    for shape in ((4, 5), (4, 0, 6)):
        with pytest.raises(ValueError):
            spacing_plan(shape, A)
    with pytest.raises(ValueError):
        spacing_plan((4, 5, 6), A, out_shape=(4, 5, 0))
    with pytest.raises(ValueError):
        GridPlan((4, 5, 6), (4, 5, 6), (0, 0, 2), (False,) * 3, (1, 1, 1), (0, 0, 0), A, A)
    with pytest.raises(ValueError):
        GridPlan((4, 5, 6), (4, 5, 6), (0, 1, 2), (False,) * 3, (1, 0, 1), (0, 0, 0), A, A)
    plan = spacing_plan((4, 5, 6), K.affine_for("LPS", (1, 1, 1)))
    x = torch.zeros(4, 5, 6)
    with pytest.raises(U3DError):                                        # no CPU path
        plan.apply(x)
    with pytest.raises(U3DError):
        plan.apply(x.to(torch.uint8), "nearest")
    with pytest.raises(U3DError):
        resample_spacing(x, x, K.affine_for("LPS", (1, 1, 1)))
    with pytest.raises(U3DError):
        preprocess_case(x, x, K.affine_for("LPS", (1, 1, 1)), 100)
    with pytest.raises(ValueError):
        plan.apply(torch.zeros(4, 5, 7))
    with pytest.raises(ValueError):
        plan.apply(x, "cubic")
    with pytest.raises(ValueError):
        resample_spacing(x, torch.zeros(4, 5, 7), K.affine_for("LPS", (1, 1, 1)))


def test_public_signatures():
    from u3d import data
    assert list(inspect.signature(data.spacing_plan).parameters) == ["shape", "affine", "pixdim", "axcodes", "out_shape"]
    sig = inspect.signature(data.resample_spacing)
    assert list(sig.parameters) == ["image", "label", "affine", "pixdim", "axcodes"]
    assert sig.parameters["pixdim"].default == (1, 1, 2) and sig.parameters["axcodes"].default == "RAS"
    assert list(inspect.signature(data.preprocess_case).parameters)[:4] == ["image", "label", "affine", "cid"]
    assert inspect.signature(data.GridPlan.apply).parameters["mode"].default == "linear"
    for name in ("src_shape", "out_shape", "perm", "flip", "scale", "offset", "out_affine", "tables"):
        assert hasattr(data.spacing_plan((4, 5, 6), np.eye(4)), name)


def test_header_signature_table_makefile_and_documents():
    from u3d import _lib
    hdr = _read(REPO, "include", "u3d.h")
    for name in ENTRY_POINTS:
        assert re.search(r"^int " + name + r"\(", hdr, re.M), name
        assert name in _lib._SIGS and name in _lib.exported_symbols()
    assert "min(floor(c), max(n - 2, 0))" in hdr and "a + f (b - a)" in hdr          # the formulas are spelled out
    assert len(_lib._SIGS["u3d_grid_resample_linear"]) == 15 and len(_lib._SIGS["u3d_grid_resample_nearest"]) == 12
    for k, v in (("U8", 0), ("I16", 1), ("I32", 2), ("F32", 3)):
        assert re.search(rf"^#define U3D_RS_{k} {v}$", hdr, re.M)
    mk = _read(PKG, "csrc", "Makefile")
    assert "resample.hip" in re.search(r"^SRCS := (.*)$", mk, re.M).group(1).split()
    assert "resample_core.h" in re.search(r"^build/%\.o: (.*)$", mk, re.M).group(1).split()
    for f in ("resample.hip", "resample_core.h"):
        assert os.path.exists(os.path.join(PKG, "csrc", f))
    doc = _read(REPO, "INTEGRATION.md")
    assert "transforms.py:41-54" in doc
    for name in ENTRY_POINTS:
        assert f"`{name}`" in doc, name
    for name in ("spacing_plan", "resample_spacing", "preprocess_case", "GridPlan"):
        assert name in doc and name in _read(REPO, "README.md"), name
    design = _read(REPO, "DESIGN.md")
    assert re.search(r"^## 27\. ", design, re.M) and "no oracle to pin it to" not in design
