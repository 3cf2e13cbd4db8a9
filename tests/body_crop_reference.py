"""Host restatement (numpy / scipy, test-only) of the body mask and crop of the reference's preprocess/forward_crop.py
(:37-82 getmaxcomponent / get_body, :148-207 the three crops), with min_filter exposed. It is what the small-shape GPU
tests of u3d.data compare against; test_body_crop_reference.py pins it to the reference's own lines (g21_body_crop.npz)
and to scipy.

Semantics.
* components: face connectivity, numbered 1..n in the C order of each component's first voxel (what
  scipy.ndimage.label(mask) gives; ``label_components`` renumbers explicitly so that the claim is tested, not assumed).
* getmaxcomponent(mask, num_limit, min_filter): labels 1..num_limit-1 only, size >= min_filter, the largest, the
  earliest on a tie, None when none qualifies.
* get_body(vol, t, min_filter): m = vol > t (strict, fp32, NaN false); 2 x 2 x 2 erosion = AND over [z-1..z] x [y-1..y]
  x [x-1..x] with outside false; getmaxcomponent(., 100, min_filter); if None: (vol > fallback t), box erosion 10^3
  (per-axis window offsets -5..4) then box dilation 10^3 (offsets -4..5), outside false.
* the crops: label >= 14 -> 0; x range of the label (margin 1) crops image and label along the LAST axis only; threshold
  by case id; body bounding box with margin 3; the upper half image[:, :, :w // 2 + 10] with min_filter 1e5 and z margin
  5; if (zmax - zmin) - (zmax_up - zmin_up) > 30 and cid > 500 the z slice [zmin_up:zmax_up], in uncropped coordinates,
  is applied to the already z-cropped arrays (the reference's behaviour, kept).
"""
import numpy as np
import scipy.ndimage as ndi

FACE = ndi.generate_binary_structure(3, 1)
ROUTE_COMPONENT, ROUTE_FALLBACK = 0, 1


def label_components(mask):
    """(labels int32, n): face-connected components numbered by their first voxel in C order."""
    lab, n = ndi.label(np.asarray(mask) != 0, structure=FACE)
    flat = lab.reshape(-1)
    vals, first = np.unique(flat, return_index=True)       # first C-order index of every value
    keep = vals > 0
    order = np.argsort(first[keep], kind="stable")
    remap = np.zeros(n + 1, dtype=np.int32)
    remap[vals[keep][order]] = np.arange(1, n + 1, dtype=np.int32)
    return remap[lab], int(n)


def largest_component(mask, num_limit=10, min_filter=1e6):
    lab, n = label_components(mask)
    sizes = np.bincount(lab.reshape(-1), minlength=max(n + 1, num_limit))
    best, bsize = 0, 0
    for i in range(1, num_limit):
        if sizes[i] < min_filter:
            continue
        if sizes[i] > bsize:
            best, bsize = i, int(sizes[i])
    if best == 0:
        return None
    return (lab == best).astype(np.uint8)


def erode2(m):
    """binary_erosion(m, ones((2, 2, 2))): AND over the 8 voxels [z-1..z] x [y-1..y] x [x-1..x], outside false."""
    m = np.asarray(m) != 0
    out = np.zeros_like(m)
    acc = np.ones(tuple(s - 1 for s in m.shape), dtype=bool)
    for dz in (0, 1):
        for dy in (0, 1):
            for dx in (0, 1):
                acc &= m[dz:m.shape[0] - 1 + dz, dy:m.shape[1] - 1 + dy, dx:m.shape[2] - 1 + dx]
    out[1:, 1:, 1:] = acc
    return out


def window_offsets(n, dilate):
    """Per-axis window offsets (lo, hi) of scipy's binary erosion / dilation with a box of size n and origin 0."""
    lo, hi = -(n // 2), n - 1 - n // 2
    return (-hi, -lo) if dilate else (lo, hi)


def window_axis(m, axis, lo, hi, op):
    """AND ("and") / OR ("or") of m over the offsets lo..hi along axis, a voxel outside counting as false."""
    m = np.moveaxis(np.asarray(m) != 0, axis, 0)
    n = m.shape[0]
    out = np.ones_like(m) if op == "and" else np.zeros_like(m)
    for d in range(lo, hi + 1):
        sh = np.zeros_like(m)
        a, b = max(0, -d), min(n, n - d)                   # out index i reads m[i + d]
        if a < b:
            sh[a:b] = m[a + d:b + d]
        out = (out & sh) if op == "and" else (out | sh)
    return np.moveaxis(out, 0, axis)


def box_open(m, n=10):
    for axis in range(3):
        m = window_axis(m, axis, *window_offsets(n, False), "and")
    for axis in range(3):
        m = window_axis(m, axis, *window_offsets(n, True), "or")
    return m


def get_body(vol, threshold_all=-200, min_filter=1e6, fallback_threshold=None):
    """(mask uint8, route)."""
    vol = np.asarray(vol, dtype=np.float32)
    m = erode2(vol > np.float32(threshold_all))
    comp = largest_component(m, 100, min_filter)
    if comp is not None:
        return comp, ROUTE_COMPONENT
    t = threshold_all if fallback_threshold is None else fallback_threshold
    return box_open(vol > np.float32(t)).astype(np.uint8), ROUTE_FALLBACK


def bounding_box(x):
    idx = np.nonzero(np.asarray(x) != 0)
    if idx[0].size == 0:
        raise ValueError("bounding_box: no nonzero voxel")
    return tuple(int(i.min()) for i in idx), tuple(int(i.max()) for i in idx)


def body_threshold(cid):
    if cid in (540, 518):
        return 30000
    return 25 if cid > 410 else -200


def body_crop(image, label, cid, min_filter=1e6, min_filter_up=1e5):
    image = np.asarray(image)
    label = np.array(label, copy=True)
    label[label >= 14] = 0
    sum_before = float(label.astype(np.float64).sum())
    lo, hi = bounding_box(label)
    xmin, xmax = max(0, lo[2] - 1), hi[2] + 1
    image, label = image[:, :, xmin:xmax], label[:, :, xmin:xmax]
    thre = body_threshold(cid)
    mask, route = get_body(image, thre, min_filter)
    blo, bhi = bounding_box(mask)
    size = int(np.count_nonzero(mask))
    zmin, ymin, x0 = (max(0, v - 3) for v in blo)
    zmax, ymax, x1 = (v + 3 for v in bhi)
    image_a, label_a = image[zmin:zmax, ymin:ymax, x0:x1], label[zmin:zmax, ymin:ymax, x0:x1]
    image_up = image[:, :, :image_a.shape[2] // 2 + 10]
    mask_up, route_up = get_body(image_up, thre, min_filter_up)
    ulo, uhi = bounding_box(mask_up)
    zmin_up, zmax_up = max(0, ulo[0] - 5), uhi[0] + 5
    inter_all, inter_up = zmax - zmin, zmax_up - zmin_up
    hand = inter_all - inter_up > 30 and cid > 500
    if hand:
        image_a, label_a, mask = image_a[zmin_up:zmax_up], label_a[zmin_up:zmax_up], mask[zmin_up:zmax_up]
    info = {"label_range": (xmin, xmax), "bbox": (blo, bhi), "bbox_up": (ulo, uhi),
            "size": size,
            "size_up": int(np.count_nonzero(mask_up)), "route": route, "route_up": route_up, "found_hand": bool(hand),
            "inter_all": inter_all, "inter_up": inter_up, "mask": mask, "label_sum_before": sum_before,
            "label_sum_after": float(label_a.astype(np.float64).sum())}
    return image_a, label_a, info
