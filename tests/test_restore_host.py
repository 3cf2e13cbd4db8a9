"""Host-side contract of the way back from a prediction to the case's own voxels (no device):
GridPlan.restrict_source's tables and valid ranges against a brute-force evaluation from resample_reference.py's
coordinates, on every inverse plan of resample_cases.VARIANTS and four boxes (the whole grid, an interior box, a box
touching the high border, a box from the low corner) plus a box that no output index reads; its ValueError paths; the
new entry points declared in the header, listed with the declared arity and exported; the argument checks of the
public functions, which have no CPU path."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

import resample_cases as K
import resample_reference as R
from conftest import REPO
from u3d import data

ENTRY_POINTS = ["u3d_grid_resample_argmax", "u3d_ccl_keep_largest", "u3d_ccl_keep_largest_ws_bytes"]


def _boxes(S):
    """name -> (origin, shape) inside a grid of shape S; an axis too short for an interior keeps what it has."""
    return {
        "whole": ((0, 0, 0), tuple(S)),
        "interior": (tuple(min(1, s - 1) for s in S), tuple(max(1, s - 2) for s in S)),
        "high": (tuple(s // 2 for s in S), tuple(s - s // 2 for s in S)),
        "low": ((0, 0, 0), tuple(max(1, s // 2) for s in S)),
    }


def _plans(vid):
    _, shape, affine, pixdim, _ = K.VARIANTS[K.IDS.index(vid)]
    return data.spacing_plan(shape, affine, pixdim).inverse(), R.inverse(R.plan(shape, affine, pixdim))


def _check(inv, rinv, origin, shape):
    plan_w, valid = inv.restrict_source(origin, shape)
    assert plan_w.src_shape == tuple(shape) and plan_w.out_shape == inv.out_shape
    assert plan_w.perm == inv.perm and plan_w.scale == inv.scale and plan_w.flip == (False,) * 3
    rw = dict(rinv, src_shape=tuple(shape),
              offset=tuple(rinv["offset"][i] - origin[rinv["perm"][i]] for i in range(3)))
    for (i0, frac, near), (w0, wf, wn) in zip(plan_w.tables, R.tables(rw)):
        assert np.array_equal(i0, w0) and np.array_equal(frac, wf) and np.array_equal(near, wn)
    empty = False
    for i, c in enumerate(R.coordinates(rinv)):                  # the unrestricted plan's coordinates
        a = rinv["perm"][i]
        near = np.rint(c)
        inside = [k for k in range(len(c)) if origin[a] <= near[k] < origin[a] + shape[a]]
        lo, hi = valid[i]
        assert 0 <= lo <= hi <= len(c)
        assert inside == list(range(lo, hi)), (i, valid[i], inside)
        empty |= not inside
    return empty


@pytest.mark.parametrize("vid", K.IDS)
def test_restrict_source_tables_and_valid_ranges(vid):
    inv, rinv = _plans(vid)
    assert inv.src_shape == rinv["src_shape"] and inv.perm == rinv["perm"]
    for name, (origin, shape) in _boxes(inv.src_shape).items():
        empty = _check(inv, rinv, origin, shape)
        assert not (name == "whole" and empty)
    plan_w, valid = inv.restrict_source((0, 0, 0), inv.src_shape)
    assert valid == tuple((0, n) for n in inv.out_shape)          # the whole grid: everything is valid
    assert all(np.array_equal(a, b) for t, u in zip(plan_w.tables, inv.tables) for a, b in zip(t, u))


def test_a_box_that_no_output_index_reads_gives_an_empty_range():
    """Where the way back thins the grid out (scale 1.5: the nearest indices are 0, 2, 3, 4, 6, ...), a box one voxel
    wide at a skipped index is read by nothing."""
    inv, rinv = _plans("upsample-RAS")
    a = inv.perm[0]
    near = set(inv.tables[0][2].tolist())
    skipped = [j for j in range(inv.src_shape[a]) if j not in near]
    assert skipped, near
    origin, shape = [0, 0, 0], list(inv.src_shape)
    origin[a], shape[a] = skipped[0], 1
    assert _check(inv, rinv, tuple(origin), tuple(shape))
    _, valid = inv.restrict_source(origin, shape)
    assert valid[0] == (0, 0)


def test_valid_comes_from_the_unrestricted_table():
    """rint(c - o) is not rint(c) - o for a half-integer c and an odd o: the restricted plan's own nearest table
    disagrees with the unrestricted one somewhere on these plans, which is why valid is taken from the latter."""
    differ = total = 0
    for vid in K.IDS:
        inv, _ = _plans(vid)
        for origin, shape in _boxes(inv.src_shape).values():
            plan_w, _ = inv.restrict_source(origin, shape)
            for i in range(3):
                o, n = origin[inv.perm[i]], shape[inv.perm[i]]
                near = inv.tables[i][2].astype(np.int64)
                inside = (near >= o) & (near < o + n)
                differ += int(np.count_nonzero((plan_w.tables[i][2] + o != near) & inside))
                total += int(np.count_nonzero(inside))
    print(f"{differ} of {total} nearest indices differ between the restricted and the unrestricted table")
    assert differ > 0


def test_restrict_source_value_errors():
    shape, zooms, pixdim, _ = K.CASES["half_coords"]
    fwd = data.spacing_plan(shape, K.affine_for("LPS", zooms), pixdim)
    assert any(fwd.flip)
    with pytest.raises(ValueError, match="flip"):
        fwd.restrict_source((0, 0, 0), fwd.src_shape)
    inv = fwd.inverse()
    S = inv.src_shape
    for origin, box in (((0, 0, 1), S), ((-1, 0, 0), (1, 1, 1)), ((0, 0, 0), (S[0] + 1, 1, 1)), ((0, 0, 0), (1, 0, 1)),
                        ((0, S[1], 0), (1, 1, 1)), ((0, 0), (1, 1, 1)), ((0, 0, 0), (1, 1))):
        with pytest.raises(ValueError, match="box"):
            inv.restrict_source(origin, box)


def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def _declared_arity(hdr, name):
    m = re.search(r"^(?:int|long long|void) " + name + r"\(([^;]*)\);", hdr, re.M)
    assert m, f"{name} is not declared in u3d.h"
    args = " ".join(m.group(1).split())
    return 0 if args == "void" else args.count(",") + 1


def test_entry_points_are_declared_listed_and_exported():
    from u3d import _lib
    hdr = _read(REPO, "include", "u3d.h")
    h = _lib.lib()
    for name in ENTRY_POINTS:
        assert name in _lib._SIGS and name in _lib.exported_symbols(), name
        assert len(_lib._SIGS[name]) == _declared_arity(hdr, name), name
        assert getattr(h, name) is not None, name
    assert _lib._RESTYPE["u3d_ccl_keep_largest_ws_bytes"] is _lib.L
    assert "#define U3D_KEEP_RECORD 4" in hdr and data.KEEP_REC == 4
    q = _lib.query
    assert q("u3d_ccl_keep_largest_ws_bytes", 0) == -1 and q("u3d_ccl_keep_largest_ws_bytes", 2 ** 31) == -1
    for V in (1, 12345, 2 ** 31 - 1):                             # 8 bytes per voxel and a small table
        assert 8 * V < q("u3d_ccl_keep_largest_ws_bytes", V) <= 8 * V + 8192


def test_public_signatures():
    sig = inspect.signature(data.keep_largest_per_label)
    assert list(sig.parameters) == ["labels", "num_labels", "return_record"]
    assert [p.default for p in list(sig.parameters.values())[1:]] == [13, False]
    sig = inspect.signature(data.restore_prediction)
    assert list(sig.parameters) == ["pred", "info", "cleanup", "num_labels"]
    assert [p.default for p in list(sig.parameters.values())[2:]] == [False, 13]
    assert list(inspect.signature(data.GridPlan.restrict_source).parameters) == ["self", "origin", "shape"]
    sig = inspect.signature(data.GridPlan.apply_argmax)
    assert list(sig.parameters) == ["self", "x", "valid"] and sig.parameters["valid"].default is None


def test_argument_errors_and_no_cpu_path():
    from u3d import U3DError
    shape, zooms, pixdim, _ = K.CASES["half_coords"]
    inv = data.spacing_plan(shape, K.affine_for("LPS", zooms), pixdim).inverse()
    x = torch.zeros((3,) + inv.src_shape)
    for bad in (x[0], x[:, :-1], torch.zeros((257,) + inv.src_shape), x.long()):
        with pytest.raises(ValueError):
            inv.apply_argmax(bad)
    with pytest.raises(U3DError):
        inv.apply_argmax(x)
    lab = torch.zeros((3, 4, 5), dtype=torch.uint8)
    for bad in (lab.float(), lab.bool(), lab[0], lab[None]):
        with pytest.raises(ValueError):
            data.keep_largest_per_label(bad)
    for n in (0, 256):
        with pytest.raises(ValueError):
            data.keep_largest_per_label(lab, num_labels=n)
    with pytest.raises(U3DError):
        data.keep_largest_per_label(lab)
    info = {"plan": inv.inverse(), "origin": (0, 0, 0)}
    with pytest.raises(U3DError):
        data.restore_prediction(torch.zeros((2, 3, 4, 5)), info)
