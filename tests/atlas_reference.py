"""fp64 / integer references of csrc/atlas.hip, device-agnostic torch and numpy (test infrastructure):

  nearest_index / atlas_crop_ref   u3d_atlas_crop: the formula of include/u3d.h in integers
  getitem_atlas_ref                MOTSDataset.py:357-392's atlas lines (F.interpolate on a float64 CPU tensor, pad_image2,
                                   crop, transpose) restated with torch / numpy calls
  select_probs_ref                 u3d_select_probs_fwd / _bwd in fp64, with the magnitudes the bounds need
  dice_atlas_ref                   u3d_dice_metric_atlas: the reference's lines evaluate_amos.py:144-151 in fp64 on the
                                   fp32 inputs, integer counts, dice_score / senc_score / spec_score from the counts
"""
import types

import numpy as np
import torch

F64 = torch.float64
U = 2.0 ** -24
GATE = float(np.float32(0.15))      # the reference adds the Python scalar 0.15 to a float32 tensor: 0.15 rounded to fp32


def nearest_index(i, n_in, n_out):
    """Source index of output index i: floor(i * in / out) in integers, clamped to in - 1."""
    return min((int(i) * int(n_in)) // int(n_out), int(n_in) - 1)


def atlas_crop_ref(atlas, image_shape, offsets, crop):
    """atlas [C, Ah, Aw, Ad] numpy -> [C, cd, ch, cw]: include/u3d.h's formula, element by index tables."""
    C, Ah, Aw, Ad = atlas.shape
    Ih, Iw, Id = image_shape
    b0, c0, a0 = offsets
    ch, cw, cd = crop
    ys, xs, zs = b0 + np.arange(ch), c0 + np.arange(cw), a0 + np.arange(cd)
    sy = np.array([nearest_index(y, Ah, Ih) if y < Ih else 0 for y in ys])
    sx = np.array([nearest_index(x, Aw, Iw) if x < Iw else 0 for x in xs])
    sz = np.array([nearest_index(z, Ad, Id) if z < Id else 0 for z in zs])
    inside = (zs < Id)[:, None, None] & (ys < Ih)[None, :, None] & (xs < Iw)[None, None, :]
    out = atlas[:, sy[None, :, None], sx[None, None, :], sz[:, None, None]]     # [C, cd, ch, cw]
    return np.where(inside[None], out, 0).astype(atlas.dtype)


def interpolate_f64(atlas, image_shape):
    """MOTSDataset.py:357: nn.functional.interpolate(torch.tensor(atlas).unsqueeze(0), image.shape).numpy()[0] with the
    float64 atlas the reference loads (mode 'nearest' on the CPU)."""
    t = torch.from_numpy(np.asarray(atlas, dtype=np.float64))
    return torch.nn.functional.interpolate(t.unsqueeze(0), tuple(int(v) for v in image_shape)).numpy()[0]


def getitem_atlas_ref(atlas, image_shape, crop_size, usage, rng):
    """The atlas side of AMOSDataSet_newatlas.__getitem__ (:357, :372, :377-385, :392); crop_size (d, h, w); draws from
    rng.randint in the reference's order b, c, a. Returns (catlas [C, D, H, W] float64, (b, c, a))."""
    cd, ch, cw = crop_size
    cat = interpolate_f64(atlas, image_shape)
    miss = [max(0, t - s) for t, s in zip((ch + 5, cw + 5, cd + 5), cat.shape[1:])]
    cat = np.pad(cat, ((0, 0), (0, miss[0]), (0, miss[1]), (0, miss[2])), "constant")
    b = c = a = 0
    if usage == "train":
        b = rng.randint(cat.shape[1] - ch)
        c = rng.randint(cat.shape[2] - cw)
        a = rng.randint(cat.shape[3] - cd)
        cat = cat[:, b:b + ch, c:c + cw, a:a + cd]
    return cat.transpose((0, 3, 1, 2)), (int(b), int(c), int(a))


# ------------------------------------------------------------------------------------------------ organ / atlas pairs
def select_probs_ref(lg, first, index, atlas=None, gout=None):
    """lg [C, V] fp32 logits (any device), index: list of ints, atlas [A, V] or None, gout [K, nch, V] or None.
    out [K, nch, V] fp64 (the atlas channel the atlas's own values); with gout: dl [C, V] = p (G - sum_j p_j G_j),
    G_c = sum of gout[k, 0] over first + index[k] == c, plus the magnitudes of the bound (atlas_cases.select_bounds)."""
    x = lg.to(F64)
    C, V = x.shape
    xm = x - x.max(0, keepdim=True).values
    p = torch.softmax(x, 0)
    K, nch = len(index), 1 if atlas is None else 2
    cls = torch.tensor([first + i for i in index], dtype=torch.long, device=lg.device)
    out = torch.zeros((K, nch, V), dtype=F64, device=lg.device)
    if K:
        out[:, 0] = p[cls]
        if atlas is not None:
            out[:, 1] = atlas.to(F64)[torch.tensor(list(index), dtype=torch.long, device=lg.device)]
    r = types.SimpleNamespace(out=out, p=p, x=xm, cls=cls)
    if gout is not None and K:
        g0 = gout.to(F64)[:, 0]
        G = torch.zeros_like(p).index_add_(0, cls, g0)
        r.G, r.G_abs = G, torch.zeros_like(p).index_add_(0, cls, g0.abs())
        r.ndup = torch.zeros(C, dtype=F64, device=lg.device).index_add_(0, cls, torch.ones(K, dtype=F64, device=lg.device))
        r.dot = (G * p).sum(0, keepdim=True)
        r.gp_abs = (G * p).abs().sum(0, keepdim=True)
        r.dl = p * (G - r.dot)
    return r


# ------------------------------------------------------------------------------------------------ atlas-gated Dice
def gate_margin(lg, atlas, ncls):
    """p + 0.15 - (1 - a) in fp64 from the fp32 inputs: lg [S, V, C], atlas [S, A, V] -> [S, ncls, V]."""
    p = torch.softmax(lg.to(F64), 2)[:, :, 1:ncls + 1].permute(0, 2, 1)
    return p + GATE - (1.0 - atlas.to(F64)[:, :ncls])


def dice_atlas_ref(lg, lab, atlas, ncls):
    """lg [S, V, C], lab [S, V], atlas [S, A, V]: counts [S, ncls, 3] int64 = (sum cpred & t, sum cpred, sum t), metrics
    [ncls, 3] fp64 = (dice, sensitivity, precision) averaged over samples as the reference's helpers, argmax [S, V]."""
    S, V, C = lg.shape
    m = gate_margin(lg, atlas, ncls)
    cpred = m > 0
    t = lab[:, None, :] == torch.arange(1, ncls + 1, device=lg.device, dtype=lab.dtype)[None, :, None]
    counts = torch.stack([(cpred & t).sum(2), cpred.sum(2), t.sum(2)], 2).to(torch.int64)
    c = counts.to(F64)
    metrics = torch.stack([(2 * c[..., 0] / (c[..., 1] + c[..., 2] + 1)).mean(0), (c[..., 0] / (c[..., 2] + 1)).mean(0),
                           (c[..., 0] / (c[..., 1] + 1)).mean(0)], 1)
    return types.SimpleNamespace(counts=counts, metrics=metrics, argmax=lg.to(F64).argmax(2), margin=m,
                                 share=cpred.to(F64).mean((0, 2)))
