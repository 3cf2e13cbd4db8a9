"""Cases and inputs shared by test_atlas_build_reference.py (which asserts their conditions on the CPU),
test_gpu_atlas_build.py (which runs csrc/atlas_build.hip and u3d.data.AtlasBuilder on them) and
tests/golden/gen_golden_atlas_build.py (which runs the reference's own lines on the fixture cases for
g20_atlas_build.npz). Inputs are rebuilt from seeds; the fixture holds outputs and a checksum of the inputs.
"""
import functools
import hashlib

import numpy as np

from loss_cases import SLACK  # noqa: F401  (the house's slack)

U = 2.0 ** -24
L_REF = 15                     # the reference's fifteen organs
SIGMA = 3.0                    # gaussian_filter(sigma=3): radius 12

# the kernels' constants (csrc/atlas_build.hip): a change of one shows which case has to move
AB = 256                       # threads per block
AB_GX, AB_GY = 64, 1024        # blocks along an atlas plane / along the slowest atlas axis at most
AB_PB = 1024                   # blocks of the presence pass at most, 16 bytes per thread and trip

# ------------------------------------------------------------------------------------------------ fixture cases
# name -> source shapes [H, W, D] of the training cases of one atlas
FIXTURES = {
    # every atlas axis < 12 < the blur's radius: the reflection wraps more than once. 4 -> 3 holds the exact tie
    # cc = 1.5; axis 2 averages to 4.5 (half to even: 4)
    "small": [(4, 8, 5), (2, 10, 4)],
    # atlas axis 0 = 26 > 2 * 12 + 1; 8 -> 26 and 29 -> 26 lose the last plane
    "wide": [(8, 4, 3), (29, 6, 3), (41, 5, 6)],
}
SHAPES = {"small": (3, 9, 4), "wide": (26, 5, 4)}
ABSENT = 12                    # a label no case of either fixture holds
LONE = 7                       # "small": one voxel of case 0, at an index of axis 0 that 4 -> 3 never reads
LONE_AT = (1, 3, 2)
QUIRK_PAIRS = [(8, 26), (22, 20), (30, 8), (26, 12)]        # (in, out) with the lost last plane


def checksum(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


@functools.lru_cache(maxsize=None)
def fixture_volumes(name):
    """The uint8 label volumes of a fixture case: codes 0..16 without ABSENT (and, in "small", without LONE but for
    the one voxel at LONE_AT of case 0)."""
    pool = [c for c in range(17) if c != ABSENT and not (name == "small" and c == LONE)]
    vols = []
    for i, shp in enumerate(FIXTURES[name]):
        g = np.random.default_rng([20, len(name), i])
        vols.append(np.asarray(pool, dtype=np.uint8)[g.integers(0, len(pool), shp)])
    if name == "small":
        vols[0][LONE_AT] = LONE
    for v in vols:
        v.setflags(write=False)
    return tuple(vols)


# ------------------------------------------------------------------------------------------------ kernel cases
# name -> (source shape, atlas shape): the axis pairs 8 -> 26, 30 -> 8 (lost last plane), 4 -> 3 (tie), 5 -> 1, 1 -> 4,
# 2 -> 7, mixed so that the fastest atlas axis is 26, 7, 3 and 1 long
KERNEL_CASES = {
    "fast26": ((30, 4, 8), (8, 3, 26)),
    "fast7": ((5, 8, 2), (1, 26, 7)),
    "fast3": ((1, 30, 4), (4, 8, 3)),
    "fast1": ((2, 8, 5), (7, 26, 1)),
}
KERNEL_L = [15, 13, 1]
# launch geometry (L = 15): the slowest atlas axis longer than the grid's y, a plane longer than the grid's x
GEOM_CASES = {
    "ystride": ((7, 2, 3), (AB_GY + 6, 2, 3)),
    "xstride": ((3, 50, 41), (2, 130, 131)),
}
ACC_FILL, COUNT_FILL = 3.0, 5

# the presence pass past its grid: more 16-byte words than AB_PB * AB threads, read from a pointer 3 bytes off
# alignment, every label a single voxel: in the scalar head, in the second trip, in the scalar tail, in between
PRESENCE_SHAPE, PRESENCE_ATLAS, PRESENCE_OFFSET = (200, 150, 141), (9, 20, 17), 3
PRESENCE_VOXELS = {1: 0, 3: AB_PB * AB * 16 + 13 + 77, 5: 1234567, 2: 200 * 150 * 141 - 1}   # label -> flat index


@functools.lru_cache(maxsize=None)
def kernel_volume(shape):
    """uint8 codes 0..16 and 255: for every L of KERNEL_L the background, labels, L + 1 and 255."""
    g = np.random.default_rng([21] + list(shape))
    pool = np.asarray(list(range(17)) + [255], dtype=np.uint8)
    v = pool[g.integers(0, len(pool), shape)]
    v.reshape(-1)[-5:] = [0, 255, 2, 14, 16]          # whatever the draw: code 0, 255 and L + 1 for L = 1, 13, 15
    v[0, 0, 0] = 1                                    # and label 1 where every zoom reads (index 0 -> source 0)
    v.setflags(write=False)
    return v


@functools.lru_cache(maxsize=None)
def presence_volume():
    """Background, sparse codes 16 and 255 (never labels), and the single voxels of PRESENCE_VOXELS."""
    g = np.random.default_rng(22)
    n = int(np.prod(PRESENCE_SHAPE))
    v = np.zeros(n, dtype=np.uint8)
    v[g.integers(0, n, 5000)] = 16
    v[g.integers(0, n, 5000)] = 255
    for l, i in PRESENCE_VOXELS.items():
        v[i] = l
    v.setflags(write=False)
    return v.reshape(PRESENCE_SHAPE)


# ------------------------------------------------------------------------------------------------ input dtypes
NOT_LABELS = (257.0, -255.0, 1.5)          # 257 and -255 wrap onto label 1 in a plain uint8 cast, 1.5 truncates onto it


def final_bound(sums, counts):
    """7 u A SLACK per plane (test_gpu_atlas_build.py's docstring), A = the plane's fp64 maximum after normalisation."""
    A = np.array([sums[l].max() / counts[l] if counts[l] > 0 else 0.0 for l in range(sums.shape[0])])
    return 7 * U * A * SLACK
