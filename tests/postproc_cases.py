"""Multi-label volumes shared by test_ccl_multi_core_host.py (the sanitised core program) and test_gpu_keep_largest.py
(u3d_ccl_keep_largest, u3d.data.keep_largest_per_label), built on the shapes and patterns of body_crop_cases.py with
codes laid over them, and the oracle: scipy.ndimage.label per label, np.bincount and the first maximum. Inputs are
rebuilt from seeds.
"""
import functools

import numpy as np

import body_crop_cases as K

SHAPES = K.label_shapes()
BIG = SHAPES[-1]                       # three tiles on every axis
# one full tile, the seam-straddling extents of one axis at a time, a flat row and the three-tile volume
CORE_SHAPES = [BIG, (K.TILE[0] + 1, 5, 9), (3, 2 * K.TILE[1] + 1, 9), (3, 5, K.TILE[2] + 1), (1, 1, 257)]


def _noise(shape, seed, p, lo, hi, skip=()):
    """Bernoulli(p) voxels holding a code drawn from lo..hi without the codes in skip, 0 elsewhere."""
    g = np.random.default_rng([31, seed] + list(shape))
    pool = np.array([c for c in range(lo, hi + 1) if c not in skip], dtype=np.uint8)
    return np.where(g.random(shape) < p, pool[g.integers(0, pool.size, shape)], 0).astype(np.uint8)


def checker_codes(shape):
    """Every voxel holds code 1 or 2, alternating along every axis: no two face neighbours share a code."""
    z, y, x = np.indices(shape)
    return (1 + (z + y + x) % 2).astype(np.uint8)


def pattern_in_noise(name, shape, code=5, p=0.4):
    """A one-component pattern (serpentine, comb) in one code, Bernoulli noise of the other codes 1..13 around it."""
    m = K.pattern(name, shape)
    return np.where(m != 0, np.uint8(code), _noise(shape, len(name), p, 1, 13, skip=(code,))).astype(np.uint8)


def tie_codes():
    """Label 4: two boxes of 768 voxels each and a smaller one before them; the earlier large box wins. Label 9: one
    box. Shape (12, 20, 70)."""
    c = np.zeros((12, 20, 70), dtype=np.uint8)
    c[0, 0, 0:2] = 4
    c[1:4, 2:6, 3:67] = 4
    c[6:9, 2:6, 3:67] = 4
    c[10, 0, 0:5] = 9
    return c


def crossing_codes():
    """Label 3 crosses three tiles on every axis as one component (a box with its corners cut by other codes), with
    specks of label 3 apart from it; noise of the other codes elsewhere; codes above 13 that must come through."""
    c = _noise(BIG, 7, 0.3, 1, 13, skip=(3,))
    c[1:-1, 1:-1, 2:-2] = 3
    c[1:4, 1:4, 2:6] = 7
    c[0, 0, 0] = c[-1, -1, -1] = c[0, -1, 0] = 3
    c[5, 0, 40:44] = 14
    c[0, 5, 100] = 200
    c[9, 9, 70] = 255
    return c


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (codes uint8 [Z, Y, X], num_labels)."""
    out = {}
    for shape in SHAPES:
        out[f"checker-{shape}"] = (checker_codes(shape), 13)
    for shape in (SHAPES[1], SHAPES[2], BIG):
        for name in ("serpentine", "comb"):
            out[f"{name}-{shape}"] = (pattern_in_noise(name, shape), 13)
    out["tie"] = (tie_codes(), 13)                              # labels other than 4 and 9 are absent
    out["crossing"] = (crossing_codes(), 13)
    out["crossing-one-label"] = (crossing_codes(), 1)           # every code but 1 is above num_labels
    out["noise-one-label"] = (_noise(BIG, 9, 0.5, 1, 3), 1)
    out["background"] = (np.zeros(SHAPES[2], dtype=np.uint8), 13)
    out["dense"] = (_noise((17, 33, 70), 11, 1.0, 1, 4), 13)    # no background, labels 5..13 absent
    for c, _ in out.values():
        c.setflags(write=False)
    return out


def core_volumes():
    """[(codes, num_labels)] for the host program of the lock-free core."""
    out = []
    for shape in CORE_SHAPES:
        out += [(checker_codes(shape), 13), (pattern_in_noise("serpentine", shape), 13),
                (pattern_in_noise("comb", shape), 13), (_noise(shape, 3, 0.6, 1, 3), 2),
                (_noise(shape, 4, 1.0, 1, 2), 13), (np.zeros(shape, dtype=np.uint8), 13)]
    out += [(tie_codes(), 13), (crossing_codes(), 13), (crossing_codes(), 1)]
    return out


@functools.lru_cache(maxsize=None)
def oracle(name):
    """(out uint8, record int32 [num_labels, 4]) from scipy: per label the components of codes == l, their sizes and the
    first maximum (scipy numbers components in the C order of their first voxel)."""
    import scipy.ndimage as ndi
    codes, num_labels = cases()[name]
    out = codes.copy()
    rec = np.zeros((num_labels, 4), dtype=np.int32)
    for l in range(1, num_labels + 1):
        lab, n = ndi.label(codes == l)
        if n == 0:
            rec[l - 1] = (0, 0, 0, -1)
            continue
        sizes = np.bincount(lab.ravel())[1:]
        keep = int(np.argmax(sizes)) + 1                       # the first maximum
        out[(lab != 0) & (lab != keep)] = 0
        rec[l - 1] = (n, int(sizes.sum()), int(sizes[keep - 1]), int(np.flatnonzero(lab.ravel() == keep)[0]))
    out.setflags(write=False)
    rec.setflags(write=False)
    return out, rec
