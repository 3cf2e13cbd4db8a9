"""The configuration behind tests/golden/g18_eam.npz, shared by its generator (which runs the reference on the CPU in
fp64) and by the tests (which run the native models): unet3D_with_eam, unet3D_with_eam_baseline and unet3D_with_feam
at 1 x 1 x 32^3, layers [1, 2, 2, 2, 2], 14 classes, weight_std=True, weights / input / class tokens from
oracle.weights_recipe.

norm3 of every EAM is then scaled by Q_GAIN. A recipe EAM has scale q.k of unit variance over the voxels, a softmax
close to uniform whose backward is a small term; scaling the class tokens cannot change that, because norm3
normalises them (and every later level's token) first, so its affine is scaled instead: the generator asserts that the
softmax is peaked (max_n P >= 8 / N on at least half the rows of every level) and that leaving out the softmax backward
moves |d eam84.q.weight| by far more than the tests' tolerance. Q_GAIN = 1.5 is the first step of 0.5 at which that
holds (at 1.0 only 21 % of eam84's rows reach 8 / N; at 1.5, 75 %). CM_GAIN weighs the projection on cm against the
maps' (every level's cm but the last also reaches the loss through the next level's maps).
"""
import numpy as np
import torch

try:
    from oracle.weights_recipe import apply_recipe, input_volume
except ImportError:   # the generator has oracle/ itself on the path: the reference's modules own the top-level names
    from weights_recipe import apply_recipe, input_volume

NC = 14
LAYERS = [1, 2, 2, 2, 2]
SHAPE = (1, 1, 32, 32, 32)
X_SEED = 80
Q_GAIN = 1.5
CM_GAIN = 1.0
SAMPLE_N = 4096
MODELS = {"eam": ("unet3D_with_eam", {}), "base": ("unet3D_with_eam_baseline", {}), "feam": ("unet3D_with_feam", {})}
EAMS = {"eam": ("eam84", "eam42", "eam21"), "base": ("eam84", "eam42"), "feam": ("eam84", "eam42", "eam21")}


def build(module, tag, **kw):
    """The model ``tag`` of ``module`` (the reference's unet3D or the package's) with the fixture's weights."""
    m = getattr(module, MODELS[tag][0])(LAYERS, num_classes=NC, weight_std=True, **kw)
    apply_recipe(m, seed=0)
    with torch.no_grad():
        for e in EAMS[tag]:
            getattr(m, e).norm3.weight.mul_(Q_GAIN)
            getattr(m, e).norm3.bias.mul_(Q_GAIN)
    return m


def x_volume():
    return torch.from_numpy(input_volume(SHAPE, seed=X_SEED, kind="normal"))


def projections(tag, shapes):
    """Seeded output projections, one per output in the order (logits, cm if any, maps...)."""
    rng = np.random.default_rng([180, sorted(MODELS).index(tag)])
    return [torch.from_numpy(rng.standard_normal(s).astype(np.float32)) for s in shapes]


def loss_of(tag, logits, cm, att):
    outs = [logits] + ([cm] if cm is not None else []) + list(att)
    ups = projections(tag, [tuple(t.shape) for t in outs])
    gains = [1.0] + ([CM_GAIN] if cm is not None else []) + [1.0] * len(att)
    return sum(g * (t * u.to(t)).sum() for t, u, g in zip(outs, ups, gains))


def sample_index(numel, *key):
    return np.random.default_rng([181, *key]).integers(0, numel, size=SAMPLE_N)


def label_mask():
    """A label volume for unet3D_with_feam's token renewal: classes 3 and 7 absent, class 5 only in the upper half."""
    lab = np.random.default_rng([182, 0]).integers(0, NC, size=SHAPE)
    lab[np.isin(lab, [3, 7])] = 0
    lab[:, :, :16][lab[:, :, :16] == 5] = 0
    return torch.from_numpy(lab.astype(np.float32))


def grad_summary(model, n_sample=16):
    """Per parameter: the gradient's fp64 norm (-1: no gradient) and seeded sampled entries, in named_parameters order."""
    names, norms, idx_all, val_all = [], [], [], []
    for i, (k, p) in enumerate(model.named_parameters()):
        idx = np.random.default_rng([1234, i]).integers(0, p.numel(), size=n_sample)
        names.append(k)
        idx_all.append(idx)
        if p.grad is None:
            norms.append(-1.0)
            val_all.append(np.zeros(n_sample))
            continue
        g = p.grad.detach().reshape(-1).double().cpu()
        norms.append(g.norm().item())
        val_all.append(g[torch.from_numpy(idx)].numpy())
    return np.array(names), np.array(norms), np.stack(idx_all), np.stack(val_all)
