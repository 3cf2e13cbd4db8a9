"""Host restatements of the atlas construction (preprocess/atlas_gen_mm.py:114-145), numpy / scipy in float64, for
test_atlas_build_reference.py (which pins them to the reference's own lines, tests/golden/g20_atlas_build.npz) and
test_gpu_atlas_build.py (which pins csrc/atlas_build.hip and u3d.data.AtlasBuilder to them). No device.
"""
import numpy as np
from scipy import ndimage

from u3d.data import zoom_index

U = 2.0 ** -24


def gather_add(label_u8, shape, L, acc, counts):
    """include/u3d.h's formula of u3d_atlas_build_add, in place: label_u8 [h, w, d] uint8, acc [L, s0, s1, s2],
    counts [L]. One gather of the label codes through the three zoom_index tables, one-hot into the planes; presence
    from the source volume."""
    idx = [zoom_index(n, s) for n, s in zip(label_u8.shape, shape)]
    ok = (idx[0] >= 0)[:, None, None] & (idx[1] >= 0)[None, :, None] & (idx[2] >= 0)[None, None, :]
    codes = label_u8[np.ix_(*(np.maximum(i, 0) for i in idx))]
    for l in range(1, L + 1):
        acc[l - 1] += (ok & (codes == l)).astype(acc.dtype)
        counts[l - 1] += int((label_u8 == l).any())


def gather_sums(volumes, shape, L=15):
    """(sums float64 [L, s0, s1, s2], counts int64 [L]) of a list of uint8 volumes by gather_add."""
    acc, counts = np.zeros((L,) + tuple(shape)), np.zeros(L, dtype=np.int64)
    for v in volumes:
        gather_add(v, shape, L, acc, counts)
    return acc, counts


def zoom_sums(volumes, shape, L=15):
    """The reference's procedure (:121-135) restated: per label a float32 mask, ndimage.zoom(order=0) with the factors
    shape / mask.shape, summed where the mask is not empty."""
    acc, counts = np.zeros((L,) + tuple(shape)), np.zeros(L, dtype=np.int64)
    for v in volumes:
        for l in range(1, L + 1):
            mask = (v == l).astype(np.float32)
            if mask.sum() > 0:
                resized = ndimage.zoom(mask, [s / n for s, n in zip(shape, mask.shape)], order=0)
                assert resized.shape == tuple(shape)
                acc[l - 1] += resized
                counts[l - 1] += 1
    return acc, counts


def normalized(sums, counts):
    """sums / counts per plane in float64; zeros where counts == 0."""
    out = np.zeros_like(sums, dtype=np.float64)
    for l in range(sums.shape[0]):
        if counts[l] > 0:
            out[l] = sums[l] / float(counts[l])
    return out


def finish(sums, counts, sigma=3.0):
    """:138-145 restated: plane / count, then gaussian_filter(sigma), skipped for a label no case has. float64."""
    out = normalized(sums, counts)
    for l in range(sums.shape[0]):
        if counts[l] > 0 and sigma:
            out[l] = ndimage.gaussian_filter(out[l], sigma=sigma)
    return out


def canonical_u8(a):
    """AtlasBuilder.add's rule: a value that is an integer in 0..255 keeps its code, everything else is background."""
    a = np.asarray(a)
    with np.errstate(invalid="ignore"):
        ok = (a >= 0) & (a <= 255) & (a == np.floor(a))
    return np.where(ok, a, 0).astype(np.uint8)
