"""Surface metrics on the device (csrc/edt.hip): an exact 3-D Euclidean distance transform, mask surfaces, and the
boundary metrics multi-organ segmentation is judged by next to Dice. Additive: the reference's evaluate_amos.py reports
overlap counts only.

Volumes are [Z, Y, X] (the dataset's [D, H, W]); ``spacing`` = (sz, sy, sx) in the same order, default (1, 1, 1). After
the reference's Spacingd(pixdim=(1, 1, 2)) and the dataset's transpose the real spacing is (2, 1, 1).

* ``distance_to`` / ``distance_transform_edt``: u3d_edt. Separable, squared distances carried in fp64 with
  w = spacing^2: exact for integer spacings, the root correctly rounded in fp64 and rounded once to fp32. Where there is
  nothing to measure to, the result is +inf (scipy returns meaningless values there).
* ``mask_surface``: the voxels of a mask with a face neighbour outside it (a neighbour outside the volume counts as
  outside): m & ~scipy.ndimage.binary_erosion(m).
* ``surface_distances``, ``surface_metrics``: the voxel-surface form of the metrics, edges by erosion and distances by
  the distance transform, as MONAI's compute_surface_dice and compute_hausdorff_distance document theirs (neither MONAI
  nor DeepMind's surface_distance is installed here: equality with either is not claimed). With a, b the surface voxel
  sets of the prediction and the ground truth, d_ab the distance of each voxel of a to the nearest voxel of b:

  ====== ==========================================================================================================
  NSD    (#{d_ab <= tau} + #{d_ba <= tau}) / (n_a + n_b)
  HD     max(max d_ab, max d_ba)
  HD-p   max(percentile(d_ab, p), percentile(d_ba, p)), numpy's default linear interpolation, in fp64 on the fp32
         distances
  ASSD   (sum d_ab + sum d_ba) / (n_a + n_b)
  ====== ==========================================================================================================

  Both masks of a class empty: all four are NaN. Exactly one empty: NSD is 0, the other three +inf. Every surface voxel
  counts once; the AMOS challenge's scorer weights surface elements by their area, so its NSD differs slightly.

Everything is queued on torch's current stream of the tensors' device. A CPU tensor raises U3DError: no fallback.
"""
import ctypes

import torch

from . import ops
from ._lib import U3DError, call, query
from .data import _mask_u8

CLASS_REC, SURFACE_REC = 8, 5    # U3D_CLASS_RECORD, U3D_SURFACE_RECORD
_DTYPES = {torch.uint8: 0, torch.float32: 1, torch.int32: 2, torch.int64: 3}


def edt_max_extent():
    """The largest extent per axis u3d_edt takes."""
    return int(query("u3d_edt_max_extent"))


def edt_tile():
    """(max_cols, tile_bytes): the min-plus passes solve min(max_cols, largest power of two <= tile_bytes / (8 n))
    adjacent lines of length n per workgroup."""
    t = [ctypes.c_int(0) for _ in range(2)]
    query("u3d_edt_tile", *(ctypes.byref(v) for v in t))
    return tuple(v.value for v in t)


def _volume3(x, what):
    if not torch.is_tensor(x) or x.dim() != 3 or x.numel() == 0:
        raise ValueError(f"{what}: {tuple(getattr(x, 'shape', ()))} must be a non-empty [Z, Y, X] volume")
    ops.require_device(x)
    if x.numel() >= 2 ** 31:
        raise ValueError(f"{what}: {x.numel()} voxels (fewer than 2^31)")


def _spacing(spacing, what):
    if spacing is None:
        return (1.0, 1.0, 1.0)
    try:
        sp = tuple(float(s) for s in spacing)
    except TypeError:
        sp = (float(spacing),) * 3
    if len(sp) != 3 or not all(0 < s < float("inf") for s in sp):
        raise ValueError(f"{what}: spacing {spacing} must be three positive numbers (sz, sy, sx)")
    return sp


def _source(x):
    """A contiguous tensor of a dtype the kernels read in place (uint8, float32, int32, int64)."""
    if x.dtype == torch.bool:
        return x.contiguous().view(torch.uint8)
    if x.dtype not in _DTYPES:
        x = x.float() if x.dtype.is_floating_point else x.long()
    return x.contiguous()


def _edt(m8, spacing, invert, squared):
    Z, Y, X = m8.shape
    big = edt_max_extent()
    if max(Z, Y, X) > big:
        raise ValueError(f"distance transform: {(Z, Y, X)}: at most {big} voxels per axis")
    out = torch.empty((Z, Y, X), dtype=torch.float32, device=m8.device)
    ws = torch.empty(query("u3d_edt_ws_bytes", m8.numel()), dtype=torch.uint8, device=m8.device)
    call("u3d_edt", m8.data_ptr(), Z, Y, X, spacing[0], spacing[1], spacing[2], int(invert), int(squared),
         out.data_ptr(), ws.data_ptr(), ops._stream())
    return out


def distance_to(mask, spacing=(1, 1, 1), squared=False):
    """fp32 [Z, Y, X]: the Euclidean distance (``squared``: its square) of every voxel to the nearest nonzero voxel of
    ``mask`` (any dtype); +inf everywhere when the mask has none."""
    sp = _spacing(spacing, "distance_to")
    _volume3(mask, "distance_to")
    with torch.cuda.device(mask.device):
        return _edt(_mask_u8(mask), sp, False, squared)


def distance_transform_edt(mask, sampling=None, squared=False):
    """scipy.ndimage.distance_transform_edt(mask, sampling) in fp32: the distance of every voxel to the nearest zero
    voxel, 0 on the zeros. Equal to scipy's wherever the mask has a zero; +inf everywhere when it has none."""
    sp = _spacing(sampling, "distance_transform_edt")
    _volume3(mask, "distance_transform_edt")
    with torch.cuda.device(mask.device):
        return _edt(_mask_u8(mask), sp, True, squared)


def _surface(src, value, box):
    """uint8 surface of src == value (None: src != 0) on box = (z0, y0, x0, bz, by, bx); src from _source."""
    Z, Y, X = src.shape
    out = torch.empty(box[3:], dtype=torch.uint8, device=src.device)
    call("u3d_mask_surface", src.data_ptr(), _DTYPES[src.dtype], Z, Y, X, 0.0 if value is None else float(value),
         int(value is None), *box, out.data_ptr(), ops._stream())
    return out


def mask_surface(x, value=None):
    """uint8 [Z, Y, X]: the surface of x == value, or of x != 0 when value is None: the voxels of the mask that have at
    least one of their six face neighbours outside it (or outside the volume)."""
    _volume3(x, "mask_surface")
    with torch.cuda.device(x.device):
        return _surface(_source(x), value, (0, 0, 0) + tuple(x.shape))


def _reduce(surf, dist, tol, rec):
    ws = torch.empty(query("u3d_surface_reduce_ws_bytes"), dtype=torch.uint8, device=surf.device)
    call("u3d_surface_dist_reduce", surf.data_ptr(), dist.data_ptr(), surf.numel(), float(tol), rec.data_ptr(),
         ws.data_ptr(), ops._stream())


def surface_distances(a, b, spacing=(1, 1, 1)):
    """(d_ab, d_ba): fp32 distances from each surface voxel of the mask a to the surface of the mask b and back, in C
    order of the surface voxels. An empty b gives +inf, an empty a an empty tensor."""
    sp = _spacing(spacing, "surface_distances")
    _volume3(a, "surface_distances")
    _volume3(b, "surface_distances")
    if a.shape != b.shape or a.device != b.device:
        raise ValueError(f"surface_distances: a {tuple(a.shape)} on {a.device}, b {tuple(b.shape)} on {b.device}")
    with torch.cuda.device(a.device):
        box = (0, 0, 0) + tuple(a.shape)
        sa, sb = _surface(_source(a), None, box), _surface(_source(b), None, box)
        return _edt(sb, sp, False, False)[sa.bool()], _edt(sa, sp, False, False)[sb.bool()]


def class_boxes(pred, gt, num_class):
    """Device int32 [num_class, 8] for the classes 1..num_class of two label maps [Z, Y, X]: lo z y x, hi z y x
    (inclusive) of (pred == c) | (gt == c) (lo = 2^31 - 1, hi = -1 when empty), voxels of pred == c, of gt == c. One
    launch, no host read."""
    _volume3(pred, "class_boxes")
    _volume3(gt, "class_boxes")
    if pred.shape != gt.shape or pred.device != gt.device:
        raise ValueError(f"class_boxes: pred {tuple(pred.shape)} on {pred.device}, gt {tuple(gt.shape)} on {gt.device}")
    if not 1 <= int(num_class) <= 64:
        raise ValueError(f"class_boxes: num_class={num_class} must be in 1..64")
    with torch.cuda.device(pred.device):
        return _class_boxes(_source(pred), _source(gt), int(num_class))


def _class_boxes(p, g, num_class):
    rec = torch.empty((num_class, CLASS_REC), dtype=torch.int32, device=p.device)
    call("u3d_class_boxes", p.data_ptr(), _DTYPES[p.dtype], g.data_ptr(), _DTYPES[g.dtype], *p.shape, num_class,
         rec.data_ptr(), ops._stream())
    return rec


def _percentile(d, q):
    """numpy.percentile(d, q) (linear interpolation) of a non-empty fp32 device vector, in fp64."""
    return torch.quantile(d.double(), q / 100.0)


def _sample_metrics(p, g, num_class, sp, tol, percentile, out):
    """out fp64 [num_class, 4] of one sample (p, g from _source). One host read, of the class records; torch's boolean
    indexing, which compacts the distances for the percentile, also waits for each set's size."""
    boxes = _class_boxes(p, g, num_class).cpu().tolist()                             # the host read
    nan, inf = float("nan"), float("inf")
    live = [c for c in range(num_class) if boxes[c][6] > 0 and boxes[c][7] > 0]
    # the rows of the classes missing from a map, filled on the host; the others are overwritten below
    out.copy_(torch.tensor([(nan,) * 4 if b[6] == 0 and b[7] == 0 else (0.0, inf, inf, inf) for b in boxes],
                           dtype=torch.float64))
    rec = torch.empty((max(len(live), 1), 2, SURFACE_REC), dtype=torch.float64, device=p.device)
    hdp = torch.empty((max(len(live), 1), 2), dtype=torch.float64, device=p.device)
    for k, c in enumerate(live):
        lo, hi = boxes[c][0:3], boxes[c][3:6]
        box = tuple(lo) + tuple(h - l + 1 for l, h in zip(lo, hi))
        sa, sb = _surface(p, c + 1, box), _surface(g, c + 1, box)
        da, db = _edt(sa, sp, False, False), _edt(sb, sp, False, False)
        _reduce(sa, db, tol[c], rec[k, 0])
        _reduce(sb, da, tol[c], rec[k, 1])
        hdp[k, 0] = _percentile(db[sa.bool()], percentile)
        hdp[k, 1] = _percentile(da[sb.bool()], percentile)
    if live:
        n = rec[:len(live), 0, 0] + rec[:len(live), 1, 0]
        idx = torch.tensor(live, dtype=torch.long, device=p.device)
        res = torch.stack([(rec[:len(live), 0, 3] + rec[:len(live), 1, 3]) / n,
                           torch.maximum(rec[:len(live), 0, 2], rec[:len(live), 1, 2]),
                           torch.maximum(hdp[:len(live), 0], hdp[:len(live), 1]),
                           (rec[:len(live), 0, 1] + rec[:len(live), 1, 1]) / n], dim=1)
        out[idx] = res


def surface_metrics(pred, gt, num_class=13, spacing=(1, 1, 1), tolerance=1.0, percentile=95.0):
    """Device fp32 [S, num_class, 4] = (nsd, hd, hd_percentile, assd) per sample and class 1..num_class (the module
    docstring defines them and the empty cases).

    pred, gt: label maps [S, Z, Y, X] or [Z, Y, X] on the device; pred an integer dtype (the int64 argmax map of
    get_dice), gt the dataset's fp32 labels or an integer dtype. tolerance: a float or a sequence of num_class, in
    spacing units. Per sample: one pass for every class's bounding box and voxel counts (u3d_class_boxes) and one host
    read of them; then, for each class present in both maps, the two surfaces on the box of the union, the two distance
    transforms and two reductions; the percentile by torch device ops on the compacted distances. Cropping to the
    union's box is exact: a mask voxel on a face of the box has a neighbour outside the box that is in neither mask, so
    the surfaces, and with them the distances, are those of the full volume."""
    return surface_metrics_fp64(pred, gt, num_class, spacing, tolerance, percentile).float()


def surface_metrics_fp64(pred, gt, num_class=13, spacing=(1, 1, 1), tolerance=1.0, percentile=95.0):
    """surface_metrics before its fp32 store: device fp64 [S, num_class, 4] (for a caller that averages over the batch
    first, as evaluate_amos.get_surface_scores does)."""
    if not torch.is_tensor(pred) or not torch.is_tensor(gt) or pred.dim() not in (3, 4) or gt.dim() != pred.dim():
        raise ValueError(f"surface_metrics: pred {tuple(getattr(pred, 'shape', ()))}, gt "
                         f"{tuple(getattr(gt, 'shape', ()))} must both be [S, Z, Y, X] or [Z, Y, X]")
    if pred.shape != gt.shape or pred.numel() == 0:
        raise ValueError(f"surface_metrics: pred {tuple(pred.shape)} and gt {tuple(gt.shape)} differ or are empty")
    if pred.dtype.is_floating_point or pred.dtype == torch.bool:
        raise ValueError(f"surface_metrics: pred is {pred.dtype}; it must be an integer label map")
    if not 1 <= int(num_class) <= 64:
        raise ValueError(f"surface_metrics: num_class={num_class} must be in 1..64")
    num_class = int(num_class)
    sp = _spacing(spacing, "surface_metrics")
    try:
        tol = [float(t) for t in tolerance]
    except TypeError:
        tol = [float(tolerance)] * num_class
    if len(tol) != num_class or not all(t == t for t in tol):
        raise ValueError(f"surface_metrics: tolerance must be a number or {num_class} numbers, got {tolerance}")
    if not 0.0 <= float(percentile) <= 100.0:
        raise ValueError(f"surface_metrics: percentile={percentile} must be in [0, 100]")
    ops.require_device(pred, gt)
    if pred.device != gt.device:
        raise ValueError(f"surface_metrics: pred on {pred.device}, gt on {gt.device}")
    if pred.dim() == 3:
        pred, gt = pred[None], gt[None]
    if pred[0].numel() >= 2 ** 31:
        raise ValueError(f"surface_metrics: {pred[0].numel()} voxels per sample (fewer than 2^31)")
    S = pred.shape[0]
    with torch.cuda.device(pred.device):
        out = torch.empty((S, num_class, 4), dtype=torch.float64, device=pred.device)
        p, g = _source(pred), _source(gt)
        for s in range(S):
            _sample_metrics(p[s], g[s], num_class, sp, tol, float(percentile), out[s])
        return out


__all__ = ["U3DError", "class_boxes", "distance_to", "distance_transform_edt", "edt_max_extent", "edt_tile",
           "mask_surface", "surface_distances", "surface_metrics", "surface_metrics_fp64"]
