"""Cases and inputs shared by test_resample_host.py (host), test_resample_core_host.py (the sanitised core program) and
test_gpu_resample.py (csrc/resample.hip, u3d.data). Inputs are rebuilt from seeds.

A case is (shape, zooms, pixdim, expected output shape) of a volume in file index order; ``zooms`` belong to the file
axes. It runs under several source orientations: the file axes run along the world axes named by the codes, so "LPS"
negates the first two columns of the affine and "SRA" permutes them. Under a permuted orientation output axis i reads
the file axis that runs along world axis i, with that axis' zoom; ``expected_shape`` works the size out in exact
rational arithmetic (round half to even).
"""
import functools
import itertools
from fractions import Fraction

import numpy as np

WORLD = {"L": (0, -1), "R": (0, 1), "P": (1, -1), "A": (1, 1), "I": (2, -1), "S": (2, 1)}

# name -> (shape, zooms, pixdim, expected shape under RAS / LPS)
CASES = {
    # (70 - 1) * 5 / 2 + 1 = 173.5 -> 174 (half to even); 173 * 0.4 = 69.2 > 69: the border clamp on the last axis;
    # rows of 174 are longer than two waves
    "half_even_clamp": ((5, 7, 70), (0.7, 0.8, 5.0), (1, 1, 2), (4, 6, 174)),
    "upsample": ((9, 4, 3), (3.0, 3.0, 3.0), (2, 2, 2), (13, 6, 4)),
    "size1_axis": ((6, 1, 66), (1.5, 1.0, 0.75), (1, 1, 2), (8, 1, 25)),
    "half_coords": ((4, 5, 6), (4.0, 2.0, 1.0), (2, 1, 2), (7, 9, 4)),
    "amos_like": ((8, 8, 8), (0.9765625, 0.9765625, 2.5), (1, 1, 2), (8, 8, 10)),
}
PERMUTED_CASE = "half_coords"
# all six assignments of the file axes to the world axes, each with the first and the last file axis reversed
PERMUTED = tuple("".join(("LR", "PA", "IS")[w][1 if i == 1 else 0] for i, w in enumerate(p))
                 for p in itertools.permutations(range(3)))
OBLIQUE_CASE, OBLIQUE_DEG = "amos_like", 10.0
ORIGIN = (-11.5, 23.25, -40.0)

# integer-valued input at r = 0.5: every coordinate is a multiple of 0.5, every value exact in fp64 and fp32
EXACT = ((3, 4, 5), (2.0, 2.0, 2.0), (1, 1, 1), (5, 7, 9))


def affine_for(codes, zooms, origin=ORIGIN):
    """File axis a runs along the world axis of codes[a], towards that code's end, zooms[a] per voxel."""
    A = np.zeros((4, 4), dtype=np.float64)
    for a, c in enumerate(codes):
        w, sign = WORLD[c]
        A[w, a] = sign * zooms[a]
    A[:3, 3] = origin
    A[3, 3] = 1
    return A


def oblique_affine(zooms, deg=OBLIQUE_DEG, origin=ORIGIN):
    """RAS rotated by ``deg`` about the world's third axis."""
    t = np.deg2rad(deg)
    R = np.array([[np.cos(t), -np.sin(t), 0], [np.sin(t), np.cos(t), 0], [0, 0, 1]])
    A = affine_for("RAS", zooms, origin)
    A[:3, :3] = R @ A[:3, :3]
    return A


def expected_shape(shape, zooms, pixdim, codes):
    out = []
    for w in range(3):
        a = [WORLD[c][0] for c in codes].index(w)
        v = Fraction(shape[a] - 1) * Fraction(zooms[a]) / Fraction(pixdim[w]) + 1
        out.append(int(round(v)))                                  # Fraction rounds half to even
    return tuple(out)


def variants():
    """[(id, shape, affine, pixdim, expected shape or None)]"""
    out = []
    for name, (shape, zooms, pixdim, want) in CASES.items():
        for codes in ("RAS", "LPS"):
            assert expected_shape(shape, zooms, pixdim, codes) == want
            out.append((f"{name}-{codes}", shape, affine_for(codes, zooms), pixdim, want))
    shape, zooms, pixdim, _ = CASES[PERMUTED_CASE]
    for codes in PERMUTED:
        out.append((f"{PERMUTED_CASE}-{codes}", shape, affine_for(codes, zooms), pixdim,
                    expected_shape(shape, zooms, pixdim, codes)))
    shape, zooms, pixdim, want = CASES[OBLIQUE_CASE]
    out.append((f"{OBLIQUE_CASE}-oblique", shape, oblique_affine(zooms), pixdim, want))
    return out


VARIANTS = variants()
IDS = [v[0] for v in VARIANTS]


def _seed(name):
    return [27] + [ord(c) for c in name]


@functools.lru_cache(maxsize=None)
def image(shape, name="image", channels=0):
    """fp32 N(0, 300), [A0, A1, A2] or [channels, A0, A1, A2]."""
    g = np.random.default_rng(_seed(name) + list(shape))
    x = (300.0 * g.standard_normal(((channels,) if channels else ()) + tuple(shape))).astype(np.float32)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def image_i16(shape):
    x = np.rint(image(shape)).astype(np.int16)
    x.setflags(write=False)
    return x


@functools.lru_cache(maxsize=None)
def label(shape):
    """label codes 0..13, int64 (the tests cast)."""
    x = np.random.default_rng(_seed("label") + list(shape)).integers(0, 14, tuple(shape))
    x.setflags(write=False)
    return x


LABEL_DTYPES = ("uint8", "int16", "int32", "float32")
