"""fp64 restatement of the deep-supervision loss (reference losses.py:119-129 with EDiceLoss_partial(uce=False),
loss_partial.py:24-57, 71-99) and its gradient, in torch on the CPU: what the fused kernels are measured against.
Pinned to the reference's own outputs by tests/test_deepsup_reference.py.

The nearest index is torch's CPU kernel's, taken in fp32 as there: identity when out == in, else
min((int)floorf(i * scale), in - 1) with scale = (float)in / out.
"""
import numpy as np
import torch


def nearest_index(out, inn):
    if out == inn:
        return torch.arange(out)
    scale = np.float32(inn) / np.float32(out)
    idx = np.floor(np.arange(out, dtype=np.float32) * scale).astype(np.int64)
    return torch.from_numpy(np.minimum(idx, inn - 1))


def nearest_target(target, size):
    """target fp32 [S, 1, D, H, W] (or [S, D, H, W]) -> [S, d, h, w], F.interpolate(mode='nearest')."""
    t = target[:, 0] if target.dim() == 5 else target
    ia, ib, ie = (nearest_index(o, i) for o, i in zip(size, t.shape[1:]))
    return t[:, ia][:, :, ib][:, :, :, ie]


def deepsup_loss(deep, target, weights, level_weights=(0.125, 0.25, 0.5, 1.0), grad_out=1.0):
    """deep: [S, C, d, h, w] logits per level; target fp32 labels; weights [C] (= mask[0][:C]).
    Returns (loss, [level losses], [d loss * grad_out / d deep_l]) in fp64."""
    w = torch.as_tensor(weights).double()
    xs = [d.detach().double().requires_grad_(True) for d in deep]
    levels = []
    for x in xs:
        C = x.shape[1]
        p = torch.softmax(x, 1)
        t = nearest_target(target.float(), x.shape[2:])
        onehot = torch.stack([(t == c) for c in range(C)], 1).double()
        inter, z, y = (p * onehot).sum((0, 2, 3, 4)), (p * p).sum((0, 2, 3, 4)), onehot.sum((0, 2, 3, 4))
        dice = 1.0 - (2.0 * inter + 1e-5) / (z + y + 1e-5)
        levels.append((dice * w[:C]).sum() / C)
    loss = sum(lv * lw for lv, lw in zip(levels, level_weights))
    grads = torch.autograd.grad(loss * grad_out, xs, allow_unused=True)
    grads = [g if g is not None else torch.zeros_like(x) for g, x in zip(grads, xs)]
    return loss.detach(), [lv.detach() for lv in levels], grads
