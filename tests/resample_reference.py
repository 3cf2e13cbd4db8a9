"""numpy float64 restatement of the orientation / spacing resampling (u3d.data.GridPlan, csrc/resample.hip), written
apart from u3d.data: MONAI's Orientationd + Spacingd with Spacing's defaults as the reference's
preprocess/transforms.py:41-54 calls them.

* ``plan``: the output grid and the per-axis source coordinates from shape, affine, pixdim and axcodes.
* ``sample_linear`` / ``sample_nearest``: the sampling the way MONAI performs it: the volume is reoriented first
  (transpose, then reversed axes), then sampled at the per-axis coordinates with border clamping, trilinear
  (axis 2, then 1, then 0, a + f (b - a)) or nearest (rint: half to even). Nothing here knows the kernels' tables.
* ``tables``: the tables the kernels read, restated from the coordinates.

test_resample_host.py pins the two sampling functions to torch's grid_sample and scipy's map_coordinates.
"""
import numpy as np

CODES = {"L": (0, -1), "R": (0, 1), "P": (1, -1), "A": (1, 1), "I": (2, -1), "S": (2, 1)}


def io_orientation(affine):
    """nibabel's algorithm: [(world axis, sign)] per index axis."""
    rzs = np.asarray(affine, dtype=np.float64)[:3, :3]
    zooms = np.sqrt(np.sum(rzs * rzs, axis=0))
    zooms[zooms == 0] = 1
    rs = rzs / zooms
    P, S, Qs = np.linalg.svd(rs, full_matrices=False)
    keep = S > S.max() * 3 * np.finfo(np.float64).eps
    R = P[:, keep] @ Qs[keep]
    ornt = []
    for ax in range(3):
        o = int(np.argmax(np.abs(R[:, ax])))
        ornt.append((o, 1 if R[o, ax] > 0 else -1))
        R[o, :] = 0
    return ornt


def axcodes(affine):
    inv = {v: k for k, v in CODES.items()}
    return "".join(inv[t] for t in io_orientation(affine))


def plan(shape, affine, pixdim=(1, 1, 2), codes="RAS", out_shape=None):
    """dict: src_shape, out_shape, perm, flip, scale, offset, src_affine, out_affine."""
    affine = np.asarray(affine, dtype=np.float64)
    src = io_orientation(affine)
    perm, flip = [], []
    for c in codes:
        w, sign = CODES[c]
        ax = [o for o, _ in src].index(w)
        perm.append(ax)
        flip.append(src[ax][1] != sign)
    M = np.zeros((4, 4))
    M[3, 3] = 1
    for i in range(3):
        M[perm[i], i] = -1 if flip[i] else 1
        M[perm[i], 3] = shape[perm[i]] - 1 if flip[i] else 0
    re = affine @ M
    out_affine = re.copy()
    scale, n_out = [], []
    for i in range(3):
        n = shape[perm[i]]
        s = np.sqrt(np.sum(re[:3, i] * re[:3, i]))
        p = s if pixdim[i] is None else np.float64(pixdim[i])
        r = p / s
        scale.append(float(r))
        n_out.append(int(np.round((n - 1) * s / p + 1)))
        out_affine[:3, i] = re[:3, i] * r
    if out_shape is not None:
        n_out = list(out_shape)
    return {"src_shape": tuple(shape), "out_shape": tuple(n_out), "perm": tuple(perm), "flip": tuple(flip),
            "scale": tuple(scale), "offset": (0.0, 0.0, 0.0), "src_affine": affine, "out_affine": out_affine}


def inverse(p):
    """The plan from p's output grid back onto p's source grid."""
    perm, scale, offset = [0] * 3, [0.0] * 3, [0.0] * 3
    for i in range(3):
        a = p["perm"][i]
        n = p["src_shape"][a]
        se, oe = p["scale"][i], p["offset"][i]
        if p["flip"][i]:
            se, oe = -se, (n - 1) - oe
        perm[a], scale[a], offset[a] = i, 1.0 / se, 0.0 - oe / se
    return {"src_shape": p["out_shape"], "out_shape": p["src_shape"], "perm": tuple(perm), "flip": (False,) * 3,
            "scale": tuple(scale), "offset": tuple(offset), "src_affine": p["out_affine"], "out_affine": p["src_affine"]}


def raw_coordinate(p, i, k):
    """Unclamped coordinate along axis i of the reoriented source."""
    return np.float64(p["scale"][i]) * np.asarray(k, dtype=np.float64) + np.float64(p["offset"][i])


def coordinates(p):
    """Per output axis the clamped coordinates along the reoriented source axis, float64 [n_out]."""
    out = []
    for i in range(3):
        n = p["src_shape"][p["perm"][i]]
        out.append(np.clip(raw_coordinate(p, i, np.arange(p["out_shape"][i])), 0.0, float(n - 1)))
    return out


def source_index(p, k):
    """The unclamped source index (file order, float64 [3]) of the output index k: the world-preservation tests."""
    j = np.zeros(3)
    for i in range(3):
        a = p["perm"][i]
        c = raw_coordinate(p, i, k[i])
        j[a] = (p["src_shape"][a] - 1) - c if p["flip"][i] else c
    return j


def reorient(vol, p):
    """[..., A0, A1, A2] -> the reoriented volume: transposed by perm, then reversed along the flipped axes."""
    lead = vol.ndim - 3
    v = np.transpose(vol, tuple(range(lead)) + tuple(lead + a for a in p["perm"]))
    for i in range(3):
        if p["flip"][i]:
            v = np.flip(v, axis=lead + i)
    return v


def sample_linear(vol, p):
    """float64 [..., n0, n1, n2]."""
    v = reorient(np.asarray(vol), p).astype(np.float64)
    cs = coordinates(p)
    for axis in (2, 1, 0):
        ax = v.ndim - 3 + axis
        n, c = v.shape[ax], cs[axis]
        i0 = np.minimum(np.floor(c), max(n - 2, 0)).astype(np.int64)
        i1 = np.minimum(i0 + 1, n - 1)
        f = (c - i0).reshape([-1 if d == ax else 1 for d in range(v.ndim)])
        a, b = np.take(v, i0, axis=ax), np.take(v, i1, axis=ax)
        v = a + f * (b - a)
    return v


def sample_nearest(vol, p):
    v = reorient(np.asarray(vol), p)
    cs = coordinates(p)
    for axis in (2, 1, 0):
        v = np.take(v, np.rint(cs[axis]).astype(np.int64), axis=v.ndim - 3 + axis)
    return np.ascontiguousarray(v)


def tables(p):
    """Per output axis (i0 int32, frac float64, near int32) in indices of the source axis as stored."""
    out = []
    for i, c in enumerate(coordinates(p)):
        n = p["src_shape"][p["perm"][i]]
        j0 = np.minimum(np.floor(c), max(n - 2, 0))
        j1 = np.minimum(j0 + 1, n - 1)
        f, near = c - j0, np.rint(c)
        if p["flip"][i]:
            out.append(((n - 1 - j1).astype(np.int32), 1.0 - f, (n - 1 - near).astype(np.int32)))
        else:
            out.append((j0.astype(np.int32), f, near.astype(np.int32)))
    return out


def ulp32(x):
    """The spacing of fp32 at |x| (towards larger magnitudes), as float64."""
    x = np.abs(np.asarray(x, dtype=np.float32))
    return (np.nextafter(x, np.float32(np.inf)) - x).astype(np.float64)
