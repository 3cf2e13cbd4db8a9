"""Shapes, patterns and label maps shared by test_surface_reference.py (host), test_edt_core_host.py (the sanitised
core program), test_gpu_edt.py and test_gpu_surface.py (csrc/edt.hip, u3d.surface). Everything is rebuilt from seeds.
"""
import functools
import zlib

import numpy as np

# csrc/edt_core.h; the GPU tests assert these against u3d_edt_tile / u3d_edt_max_extent
MAX_COLS, TILE_BYTES, MAX_EXTENT = 64, 32768, 2048

SPACINGS = ((1, 1, 1), (2, 1, 1), (1, 1, 2), (3, 2, 1), (0.7, 1.3, 2.5))
INTEGER_SPACINGS = SPACINGS[:4]

BERNOULLI_P = (0.001, 0.05, 0.5, 0.95)
PATTERNS = ("none", "all", "corner", "two_corners", "plane_z0", "gaps", "checkerboard") + tuple(
    f"bernoulli{p}" for p in BERNOULLI_P)


def tile_cols(n):
    """Adjacent lines of length n that one workgroup of the min-plus passes solves together."""
    c = MAX_COLS
    while c > 1 and c * n * 8 > TILE_BYTES:
        c //= 2
    return c


def line_thresholds():
    """The line lengths at which tile_cols changes: 64, 128, ..., 2048 (the last is the largest extent)."""
    return [TILE_BYTES // (8 * c) for c in (64, 32, 16, 8, 4, 2)]


def edt_shapes():
    """Each axis at the lengths around the 64-voxel words of the row pass and the column tile, two odd volumes, the
    lengths around every threshold of tile_cols on the two min-plus axes, and a flat row."""
    shapes = []
    for n in (1, 2, 63, 64, 65, 129, 257):
        shapes += [(n, 3, 5), (3, n, 5), (3, 5, n)]
    shapes += [(17, 17, 17), (33, 20, 47)]
    T = line_thresholds()
    for n in (T[1] - 1, T[1], T[2] - 1, T[2], T[3] - 1, T[3], T[3] + 1, T[4] - 1, T[4], T[4] + 1, T[5] - 1, T[5]):
        shapes += [(n, 2, 3), (2, n, 3)]
    shapes += [(1, 1, 1024), (1, 2, MAX_EXTENT), (1, 1, 1)]
    return shapes


SMALL_SHAPES = ((1, 1, 1), (1, 1, 70), (5, 1, 7), (4, 5, 6), (9, 8, 8), (2, 3, 100))     # <= 600 voxels: brute force


def _seed(name, shape):
    return [zlib.crc32(name.encode())] + list(shape)


def pattern(name, shape):
    """uint8 feature mask [Z, Y, X]."""
    Z, Y, X = shape
    m = np.zeros(shape, dtype=np.uint8)
    if name == "none":
        pass
    elif name == "all":
        m[:] = 1
    elif name == "corner":                      # the longest distances: no search bound short of the line helps
        m[0, 0, 0] = 1
    elif name == "two_corners":                 # ties between the two
        m[0, 0, 0] = m[-1, -1, -1] = 1
    elif name == "plane_z0":
        m[0] = 1
    elif name == "gaps":                        # rows and whole planes without a feature: +inf carried between passes
        g = np.random.default_rng(_seed(name, shape))
        m[:] = g.random(shape) < 0.3
        m[::2] = 0
        m[:, 1::3] = 0
        if Z > 2:
            m[Z // 2:] = 0
    elif name == "checkerboard":
        z, y, x = np.indices(shape)
        m[:] = (z + y + x) % 2 == 0
    elif name.startswith("bernoulli"):
        g = np.random.default_rng(_seed(name, shape))
        m[:] = g.random(shape) < float(name[len("bernoulli"):])
    else:
        raise KeyError(name)
    return m


# ------------------------------------------------------------------------------------------------ label maps
def ellipsoids(shape, num_class, seed, jitter=0.0, border_class=None):
    """int64 label map of num_class overlapping ellipsoids (a later class overwrites an earlier one); `jitter` moves and
    scales each one a little (a prediction of the same anatomy); border_class is pushed against the volume's corner."""
    g = np.random.default_rng(seed)
    gj = np.random.default_rng([seed, 1])
    zz, yy, xx = np.indices(shape).astype(np.float64)
    lab = np.zeros(shape, dtype=np.int64)
    for c in range(1, num_class + 1):
        ctr = np.array([g.uniform(0.25, 0.75) * s for s in shape])
        rad = np.array([g.uniform(0.10, 0.22) * s + 1.5 for s in shape])
        if c == border_class:
            ctr = rad * 0.5
        ctr = ctr + jitter * gj.uniform(-1.5, 1.5, 3)
        rad = rad * (1 + jitter * gj.uniform(-0.15, 0.15, 3))
        lab[((zz - ctr[0]) / rad[0]) ** 2 + ((yy - ctr[1]) / rad[1]) ** 2 + ((xx - ctr[2]) / rad[2]) ** 2 <= 1] = c
    return lab


@functools.lru_cache(maxsize=None)
def metric_case(name):
    """(pred int64, gt int64, num_class): 'five' = (24, 40, 48) with 5 classes, class 2 touching the border; 'thirteen'
    = (40, 50, 60) with 13 classes, class 5 absent from pred, 7 from gt, 9 from both."""
    if name == "five":
        shape, nc, seed = (24, 40, 48), 5, 31
        gt = ellipsoids(shape, nc, seed, 0.0, border_class=2)
        pred = ellipsoids(shape, nc, seed, 1.0, border_class=2)
    elif name == "thirteen":
        shape, nc, seed = (40, 50, 60), 13, 32
        gt = ellipsoids(shape, nc, seed, 0.0)
        pred = ellipsoids(shape, nc, seed, 1.0)
        pred[pred == 5] = 0
        gt[gt == 7] = 0
        pred[pred == 9] = 0
        gt[gt == 9] = 0
    else:
        raise KeyError(name)
    pred.setflags(write=False)
    gt.setflags(write=False)
    return pred, gt, nc


def crop_to_union(a, b):
    """(a, b) cropped to the bounding box of a | b (both bool, not both empty)."""
    idx = np.argwhere(a | b)
    lo, hi = idx.min(0), idx.max(0) + 1
    sl = tuple(slice(l, h) for l, h in zip(lo, hi))
    return a[sl], b[sl]
