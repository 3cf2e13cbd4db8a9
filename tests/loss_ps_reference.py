"""fp64 restatement of the per-sample supervision losses (csrc/loss_ps.hip and the _ps kernels of csrc/deepsup.hip):
the partial-label soft Dice + BCE with one weight row per sample, forward and backward, and its per-level
deep-supervision form. Built on loss_reference.partial_probs (the probabilities, t_c and the BCE element are exactly
those of loss_reference.py) and on deepsup_reference's nearest map; pinned to torch's autograd and, for equal rows, to
loss_reference.partial_loss_ref by test_loss_ps_reference.py.

logits [S, V, C], labels [S, V], weights w [S, C] (any floats):
    m_sc = [w_sc != 0],  n_c = sum_s m_sc,  w^_c = sum_s w_sc / n_c (0 when n_c = 0)
    per-sample sums I_sc, Z_sc, Y_sc, B_sc (unmasked), pooled X_c = sum_s m_sc X_sc (s ascending)
    d_c = 1 - (2 I_c + 1e-5) / (Z_c + Y_c + 1e-5)
    loss = sum_c w^_c d_c / C + [uce] sum_{c: n_c > 0} w^_c B_c / (n_c V)
    dL/dp_svc = m_sc (t a_c + p b_c + kb_c (p - t) / max((1 - p) p, 1e-12)),  a_c = -2 / den_c w^_c / C g,
    b_c = 2 num_c / den_c^2 w^_c / C g,  kb_c = w^_c / (n_c V) g;  then the softmax / sigmoid / identity Jacobian.
"""
from types import SimpleNamespace as NS

import torch

import deepsup_reference as DR
import loss_reference as R
from loss_reference import F64, MODE_SIGMOID, MODE_SOFTMAX, SMOOTH, _d


def pool_weights(weights):
    """w [S, C] -> m [S, C] (0 / 1 fp64), n [C], w^ [C]."""
    w = _d(weights)
    m = (w != 0).double()
    n = m.sum(0)
    what = torch.where(n > 0, w.sum(0) / n.clamp(min=1), torch.zeros_like(n))
    return w, m, n, what


def partial_loss_ps_value(lg, labels, weights, mode, uce):
    """The forward alone on an fp64 lg [S, V, C] (differentiable): NS(loss, sums_ps [S, C, 4], pooled [C, 5], d [C],
    pr = partial_probs of the flat [S V, C] logits, hit, bce (flat), m, n, what)."""
    S, V, C = lg.shape
    assert uce in (0, 1)
    w, m, n, what = pool_weights(weights)
    cls = torch.arange(C, dtype=F64, device=lg.device)
    hit = _d(labels).reshape(S * V, 1) == cls[None, :]
    pr = R.partial_probs(lg.reshape(S * V, C), mode)
    p = pr.p
    ps = lambda x: x.reshape(S, V, C).sum(1)                                    # noqa: E731
    I, Z, Y = ps(p * hit), ps(p * p), ps(hit.double())
    bce = None
    B = torch.zeros(S, C, dtype=F64, device=lg.device)
    if uce == 1:
        bce = -torch.where(hit, pr.logp.clamp(min=-100.0), pr.logq.clamp(min=-100.0))
        B = ps(bce)
    sums_ps = torch.stack([I, Z, Y, B], 2)                                      # [S, C, 4]
    X = torch.zeros(C, 4, dtype=F64, device=lg.device)
    for s in range(S):                                                          # s ascending
        X = X + m[s][:, None] * sums_ps[s]
    d = 1 - (2 * X[:, 0] + SMOOTH) / (X[:, 1] + X[:, 2] + SMOOTH)
    loss = (what * d).sum() / C
    if uce == 1:
        loss = loss + torch.where(n > 0, what * X[:, 3] / (n.clamp(min=1) * V), torch.zeros_like(n)).sum()
    return NS(loss=loss, sums_ps=sums_ps, pooled=torch.cat([X, n[:, None]], 1), d=d, pr=pr, hit=hit, bce=bce, w=w, m=m,
              n=n, what=what)


def partial_loss_ps_ref(logits, labels, weights, mode, uce, grad_out=None, pooled=None):
    """logits [S, V, C], labels [S, V], weights [S, C] as stored. The forward (partial_loss_ps_value) and, with
    grad_out, dl [S V, C] = grad_out * d loss / d logits formed from `pooled` [C, >= 3] (default: the reference's
    own). The fields loss_cases.loss_bwd_bounds reads are there, flat over [S V, C], with the coefficients a, b, kb
    expanded per voxel (0 where the voxel's sample does not supervise the class); sums = the pooled (I, Z, Y, B)."""
    with torch.no_grad():
        lg = _d(logits)
        S, V, C = lg.shape
        f = partial_loss_ps_value(lg, labels, weights, mode, uce)
        f.sums = f.pooled[:, :4]
        f.bce_abs_ps = (f.bce.abs().reshape(S, V, C).sum(1) if f.bce is not None
                        else torch.zeros(S, C, dtype=F64, device=lg.device))
        if grad_out is None:
            return f
        go = float(grad_out)
        X = f.pooled if pooled is None else _d(pooled)
        num, den = 2 * X[:, 0] + SMOOTH, X[:, 1] + X[:, 2] + SMOOTH
        scale = f.what / C * go
        a_c, b_c = -2 / den * scale, 2 * num / (den * den) * scale
        kb_c = (torch.where(f.n > 0, f.what / (f.n.clamp(min=1) * V), torch.zeros_like(f.n)) * go if uce == 1
                else torch.zeros_like(f.what))
        f.a_c, f.b_c, f.kb_c = a_c, b_c, kb_c
        per_voxel = lambda k: (f.m * k[None, :])[:, None, :].expand(S, V, C).reshape(S * V, C)   # noqa: E731
        f.a, f.b, f.kb = per_voxel(a_c), per_voxel(b_c), per_voxel(kb_c)
        p, q, t = f.pr.p, f.pr.q, f.hit.double()
        f.g1 = t * f.a + p * f.b
        f.g2 = f.kb * (p - t) / (q * p).clamp(min=1e-12) if uce == 1 else torch.zeros_like(p)
        f.g = f.g1 + f.g2
        f.gp_abs = (f.g * p).abs().sum(1, keepdim=True)
        if mode == MODE_SOFTMAX:
            f.dot = (f.g * p).sum(1, keepdim=True)
            r = p * (f.g - f.dot)
        elif mode == MODE_SIGMOID:
            r = f.g * q * p
        else:
            r = f.g
        f.r0, f.ce, f.dl = r, None, r
        return f


# ------------------------------------------------------------------------------------------------ deep supervision
def deepsup_ps_value(xs, target, weights, level_weights):
    """xs: fp64 [S, C, d, h, w] logits per level (differentiable); target fp32 labels [S, 1, D, H, W] or [S, D, H, W];
    weights [S, C]. Per level the pooling rule with uce 0 on the nearest-resized target.
    NS(loss, levels [L], sums_ps [L][S, C, 4], pooled [L][C, 5])."""
    w, m, n, what = pool_weights(weights)
    levels, sums_ps, pooled = [], [], []
    for x in xs:
        S, C = x.shape[:2]
        p = torch.softmax(x, 1)
        t = DR.nearest_target(target.float(), x.shape[2:])
        onehot = torch.stack([(t == c) for c in range(C)], 1).double()
        I, Z, Y = (p * onehot).sum((2, 3, 4)), (p * p).sum((2, 3, 4)), onehot.sum((2, 3, 4))      # [S, C]
        sp = torch.stack([I, Z, Y, torch.zeros_like(I)], 2)
        X = torch.zeros(C, 4, dtype=F64)
        for s in range(S):
            X = X + m[s][:, None] * sp[s]
        d = 1 - (2 * X[:, 0] + SMOOTH) / (X[:, 1] + X[:, 2] + SMOOTH)
        levels.append((what * d).sum() / C)
        sums_ps.append(sp)
        pooled.append(torch.cat([X, n[:, None]], 1))
    loss = sum(lv * lw for lv, lw in zip(levels, level_weights))
    return NS(loss=loss, levels=levels, sums_ps=sums_ps, pooled=pooled)


def deepsup_ps_loss(deep, target, weights, level_weights=(0.125, 0.25, 0.5, 1.0), grad_out=1.0):
    """As deepsup_reference.deepsup_loss with weights [S, C]: (loss, [level losses], [d loss * grad_out / d deep_l],
    the forward's NS) in fp64 on the CPU; the gradients by autograd of this forward."""
    xs = [d.detach().double().cpu().requires_grad_(True) for d in deep]
    f = deepsup_ps_value(xs, target.detach().cpu(), torch.as_tensor(weights).detach().cpu(), level_weights)
    grads = torch.autograd.grad(f.loss * grad_out, xs, allow_unused=True)
    grads = [g if g is not None else torch.zeros_like(x) for g, x in zip(grads, xs)]
    f.sums_ps = [s.detach() for s in f.sums_ps]
    f.pooled = [s.detach() for s in f.pooled]
    return f.loss.detach(), [lv.detach() for lv in f.levels], grads, f
