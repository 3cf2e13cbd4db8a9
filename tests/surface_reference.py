"""The surface metrics restated in numpy / scipy fp64: what u3d/surface.py (csrc/edt.hip) is compared with.

Volumes are [Z, Y, X], spacing (sz, sy, sx). The voxel-surface form: a mask's surface is the mask minus its erosion by
the six-neighbour cross (voxels outside the volume are background), distances come from scipy's exact Euclidean distance
transform. One rule is ours: where a mask holds no feature the distance is +inf everywhere (scipy returns meaningless
values there).
"""
import numpy as np
import scipy.ndimage as ndi


def edt_ref(features, spacing=(1, 1, 1)):
    """fp64 distance of every voxel to the nearest nonzero voxel of `features`; +inf everywhere when there is none."""
    f = np.asarray(features) != 0
    if not f.any():
        return np.full(f.shape, np.inf)
    return ndi.distance_transform_edt(~f, sampling=tuple(float(s) for s in spacing))


def surface_ref(mask):
    """bool: the voxels of the mask with at least one of the six face neighbours outside it (or outside the volume)."""
    m = np.asarray(mask) != 0
    return m & ~ndi.binary_erosion(m)


def surface_distances_ref(a, b, spacing=(1, 1, 1)):
    """(d_ab, d_ba) fp64: from each surface voxel of a to the surface of b and back, in C order of the surface voxels."""
    sa, sb = surface_ref(a), surface_ref(b)
    return edt_ref(sb, spacing)[sa], edt_ref(sa, spacing)[sb]


def metrics_from_distances(d_ab, d_ba, tolerance, percentile=95.0):
    """(nsd, hd, hd_percentile, assd) of two non-empty distance sets, and the two within-tolerance counts."""
    n = d_ab.size + d_ba.size
    le_ab, le_ba = int((d_ab <= tolerance).sum()), int((d_ba <= tolerance).sum())
    nsd = (le_ab + le_ba) / n
    hd = max(d_ab.max(), d_ba.max())
    hdp = max(np.percentile(d_ab, percentile), np.percentile(d_ba, percentile))
    assd = (d_ab.sum() + d_ba.sum()) / n
    return (nsd, hd, hdp, assd), (le_ab, le_ba)


def metrics_ref(pred, gt, num_class=13, spacing=(1, 1, 1), tolerance=1.0, percentile=95.0):
    """fp64 [num_class, 4] = (nsd, hd, hd_percentile, assd) of one sample's label maps. Both masks of a class empty:
    NaN; exactly one empty: nsd 0, the rest +inf."""
    pred, gt = np.asarray(pred), np.asarray(gt)
    tol = np.broadcast_to(np.asarray(tolerance, dtype=np.float64), (num_class,))
    out = np.empty((num_class, 4), dtype=np.float64)
    for c in range(1, num_class + 1):
        a, b = pred == c, gt == c
        if not a.any() and not b.any():
            out[c - 1] = np.nan
        elif not a.any() or not b.any():
            out[c - 1] = (0.0, np.inf, np.inf, np.inf)
        else:
            d_ab, d_ba = surface_distances_ref(a, b, spacing)
            out[c - 1] = metrics_from_distances(d_ab, d_ba, tol[c - 1], percentile)[0]
    return out


def class_boxes_ref(pred, gt, num_class):
    """int [num_class, 8]: lo z y x, hi z y x (inclusive) of (pred == c) | (gt == c), voxels of pred == c, of gt == c;
    lo = 2^31 - 1 and hi = -1 for a class in neither."""
    out = np.empty((num_class, 8), dtype=np.int64)
    for c in range(1, num_class + 1):
        a, b = np.asarray(pred) == c, np.asarray(gt) == c
        idx = np.argwhere(a | b)
        if idx.size:
            out[c - 1, :3], out[c - 1, 3:6] = idx.min(0), idx.max(0)
        else:
            out[c - 1, :3], out[c - 1, 3:6] = 2 ** 31 - 1, -1
        out[c - 1, 6], out[c - 1, 7] = a.sum(), b.sum()
    return out
