"""The restatement the GPU tests compare with (surface_reference.py) checked on the host: the distance transform against
an O(V^2) brute force, the surface against a six-neighbour loop, the crop to the union box against the full volume, and
the metrics on two cases worked out by hand."""
import numpy as np
import pytest

import surface_cases as K
import surface_reference as R


def _brute_edt(m, spacing):
    idx = np.argwhere(m != 0).astype(np.float64)
    pts = np.argwhere(np.ones(m.shape, dtype=bool)).astype(np.float64)
    if not len(idx):
        return np.full(m.shape, np.inf)
    s = np.asarray(spacing, dtype=np.float64)
    d2 = (((pts[:, None, :] - idx[None, :, :]) * s) ** 2).sum(-1)
    return np.sqrt(d2.min(1)).reshape(m.shape)


@pytest.mark.parametrize("shape", K.SMALL_SHAPES, ids=str)
def test_edt_ref_is_the_brute_force(shape):
    assert np.prod(shape) <= 600
    for name in K.PATTERNS:
        m = K.pattern(name, shape)
        for sp in K.SPACINGS:
            got, want = R.edt_ref(m, sp), _brute_edt(m, sp)
            assert np.array_equal(np.isinf(got), np.isinf(want)), (name, sp)
            f = np.isfinite(want)
            assert np.allclose(got[f], want[f], rtol=1e-14, atol=0), (name, sp)
            if not m.any():
                assert np.isposinf(got).all()


@pytest.mark.parametrize("shape", [(4, 5, 6), (33, 20, 47)], ids=str)
def test_squared_distances_are_integers_for_integer_spacings(shape):
    for name in K.PATTERNS:
        m = K.pattern(name, shape)
        if not m.any():
            continue
        for sp in K.INTEGER_SPACINGS:
            d2 = R.edt_ref(m, sp) ** 2
            assert np.abs(d2 - np.rint(d2)).max() < 1e-6, (name, sp)


def _surface_loop(m):
    Z, Y, X = m.shape
    out = np.zeros(m.shape, dtype=bool)
    for z in range(Z):
        for y in range(Y):
            for x in range(X):
                if not m[z, y, x]:
                    continue
                for dz, dy, dx in ((1, 0, 0), (-1, 0, 0), (0, 1, 0), (0, -1, 0), (0, 0, 1), (0, 0, -1)):
                    a, b, c = z + dz, y + dy, x + dx
                    if not (0 <= a < Z and 0 <= b < Y and 0 <= c < X) or not m[a, b, c]:
                        out[z, y, x] = True
    return out


@pytest.mark.parametrize("shape", [(1, 1, 1), (1, 4, 7), (5, 6, 7), (3, 9, 4)], ids=str)
def test_surface_ref_is_the_six_neighbour_rule(shape):
    for name in ("none", "all", "checkerboard", "bernoulli0.5", "bernoulli0.95", "gaps"):
        m = K.pattern(name, shape)
        assert np.array_equal(R.surface_ref(m), _surface_loop(m != 0)), name
    lab = K.ellipsoids((9, 10, 11), 3, 5)
    for c in (1, 2, 3):
        assert np.array_equal(R.surface_ref(lab == c), _surface_loop(lab == c))


@pytest.mark.parametrize("spacing", [(1, 1, 1), (2, 1, 1), (0.7, 1.3, 2.5)], ids=str)
def test_crop_to_the_union_box_changes_nothing(spacing):
    pred, gt, nc = K.metric_case("five")
    seen = 0
    for c in range(1, nc + 1):
        a, b = pred == c, gt == c
        if not (a.any() and b.any()):
            continue
        full = R.surface_distances_ref(a, b, spacing)
        crop = R.surface_distances_ref(*K.crop_to_union(a, b), spacing)
        for u, v in zip(full, crop):
            assert u.dtype == np.float64 and u.tobytes() == v.tobytes()
        seen += 1
    assert seen >= 4


def test_metric_cases_hold_what_they_promise():
    pred, gt, nc = K.metric_case("five")
    assert nc == 5 and all((pred == c).any() and (gt == c).any() for c in range(1, 6))
    assert (gt == 2)[0, 0, 0] or (gt == 2)[0].any() and (gt == 2)[:, 0].any() and (gt == 2)[:, :, 0].any()
    pred, gt, nc = K.metric_case("thirteen")
    present = [((pred == c).any(), (gt == c).any()) for c in range(1, 14)]
    assert present[4] == (False, True) and present[6] == (True, False) and present[8] == (False, False)
    assert sum(a and b for a, b in present) >= 8


def test_metrics_of_two_offset_boxes_by_hand():
    """a = a 4^3 box, b = the same box moved by 2 along x, unit spacing. A 4^3 box's surface is 64 - 8 = 56 voxels.
    b's surface holds the faces x = 2 and x = 5 (all of y, z) and the rim voxels for x = 3, 4. A surface voxel of a at x
    (0..3) with (y, z) on the rim is at distance max(0, 2 - x) from b's rim; one with (y, z) interior (4 of the 16, only
    on the faces x = 0 and x = 3) is at 2 (x = 0, to b's face x = 2) or 1 (x = 3: to the rim, the face x = 2 is 1 away
    too). So d_ab: x = 0: 16 voxels at 2; x = 1: 12 at 1; x = 2: 12 at 0; x = 3: 12 at 0 and 4 at 1. By symmetry d_ba is
    the same multiset: 16 twos, 16 ones, 24 zeros."""
    a = np.zeros((8, 8, 12), dtype=bool)
    b = np.zeros_like(a)
    a[2:6, 2:6, 2:6] = True
    b[2:6, 2:6, 4:8] = True
    d_ab, d_ba = R.surface_distances_ref(a, b)
    want = np.array([2.0] * 16 + [1.0] * 16 + [0.0] * 24)
    assert np.array_equal(np.sort(d_ab)[::-1], want) and np.array_equal(np.sort(d_ba)[::-1], want)
    pred, gt = a.astype(np.int64), b.astype(np.int64)
    m = R.metrics_ref(pred, gt, num_class=1, tolerance=1.0)
    assert m[0, 0] == 80 / 112 and m[0, 1] == 2.0 and m[0, 3] == 96 / 112
    assert m[0, 2] == np.percentile(want, 95) == 2.0
    assert R.metrics_ref(pred, gt, num_class=1, tolerance=0.5)[0, 0] == 48 / 112
    # spacing (2, 1, 3): the offset is along x, so the nonzero distances are 3 and 6 or shorter ways round the rim
    m3 = R.metrics_ref(pred, gt, num_class=1, spacing=(2, 1, 3), tolerance=1.0)
    assert m3[0, 1] == 6.0 and m3[0, 0] <= 80 / 112


def test_metrics_with_an_empty_mask():
    pred = np.zeros((4, 5, 6), dtype=np.int64)
    gt = np.zeros_like(pred)
    gt[1:3, 1:3, 1:3] = 1
    pred[0, 0, 0] = 3
    m = R.metrics_ref(pred, gt, num_class=3)
    assert m[0].tolist() == [0.0, np.inf, np.inf, np.inf]          # pred empty
    assert np.isnan(m[1]).all()                                    # both empty
    assert m[2].tolist() == [0.0, np.inf, np.inf, np.inf]          # gt empty
    assert R.class_boxes_ref(pred, gt, 3).tolist() == [[1, 1, 1, 2, 2, 2, 0, 8], [2 ** 31 - 1] * 3 + [-1] * 3 + [0, 0],
                                                       [0, 0, 0, 0, 0, 0, 1, 0]]
