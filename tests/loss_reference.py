"""fp64 restatements of csrc/loss.hip and csrc/consist.hip: the partial-label soft Dice + BCE / cross entropy
(EDiceLoss_partial, EDiceLoss_full) forward and backward, the hard Dice metrics (get_dice, get_dice2), the partial-label
target, the consistency branch of get_loss and EDiceLoss_full2. They are the independent references of test_gpu_loss.py
and are themselves pinned to oracle.ref_cpu and to torch's autograd by test_loss_reference.py.

All of them are plain torch on whatever device the operands live on, take the flat layouts of the C entry points
(include/u3d.h) as they are stored and compute in fp64. Next to each result they return the per-voxel intermediates
and abs-sums from which the GPU tests build their rounding bounds (loss_cases.py).

Partial loss, logits [nvox, C], labels [nvox] (floats; a label that equals no class index simply never hits):
    p = softmax / sigmoid / identity (mode 1 / 0 / 2),  t_c = [label == c]
    sums[c] = (sum p t, sum p^2, sum t, sum bce),  d_c = 1 - (2 I + 1e-5) / (Z + Y + 1e-5)
    uce 1: bce = -(t max(log p, -100) + (1 - t) max(log(1 - p), -100)),  loss = sum_c w_c d_c / C + sum_c w_c B_c / nvox
    uce 2: bce = -t log p (cross entropy, unweighted, unclamped),         loss = sum_c w_c d_c / C + sum_c B_c / nvox
    dL/dp_c = t a_c + p b_c + kb_c (p - t) / max((1 - p) p, 1e-12) (torch's BCELoss backward), a = -2 / den * w / C,
    b = 2 num / den^2 * w / C, kb = w / nvox; then the softmax / sigmoid Jacobian; uce 2 adds (p - t) / nvox in the
    voxels whose label is a class.
    1 - p is formed as (sum of the other classes' exponentials) / s, so it keeps its precision as p -> 1.
    round_p_to_fp32 rounds p to fp32 before everything else, as PyTorch's fp32 softmax hands it to BCELoss: p == 1
    then really occurs, with log(1 - p) = -inf clamped to -100 and (1 - p) p clamped to 1e-12.
Consistency (batch 1), organ g active when label_t[g] == 0, t = softmax(refine[g])[1], confident when t > 1 - confi or
t < confi; maps = the natt attention maps, then softmax(logits)[g + 1]; map number idx takes [0.125, 0.25, 0.5, 1][idx]
and a sigmoid unless idx == 3 (the reference's enumerate over attns + [softmax map], losses.py:159-172): so with
natt < 3 the softmax map takes weights[natt] and a sigmoid. Results are stored by slot (k = 0..2 attention, 3 softmax).
"""
from types import SimpleNamespace as NS

import torch

U = 2.0 ** -24      # unit roundoff of fp32
F64 = torch.float64
MODE_SIGMOID, MODE_SOFTMAX, MODE_IDENTITY = 0, 1, 2
CONSIST_W = (0.125, 0.25, 0.5, 1.0)
SMOOTH = 1e-5


def _d(t):
    return t.detach().to(F64)


def f32(x):
    """A Python float rounded to fp32, as a C float argument arrives."""
    return float(torch.tensor(x, dtype=torch.float32).double())


# ------------------------------------------------------------------------------------------------ partial loss
def partial_probs(lg, mode, round_p_to_fp32=False):
    """lg fp64 [nvox, C] -> p, q = 1 - p, log p, log(1 - p), and for the softmax x = lg - max, s = sum exp(x)."""
    x = s = None
    if mode == MODE_SOFTMAX:
        x = lg - lg.max(1, keepdim=True).values
        e = torch.exp(x)
        s = e.sum(1, keepdim=True)
        p = e / s
        am = x.argmax(1, keepdim=True)
        rest = e.scatter(1, am, 0.0).sum(1, keepdim=True)      # the leading class's 1 - p without cancellation
        oth = (s - e).scatter(1, am, rest)
        q = oth / s
        logp, logq = x - torch.log(s), torch.log(oth) - torch.log(s)
    elif mode == MODE_SIGMOID:
        p, q = torch.sigmoid(lg), torch.sigmoid(-lg)
        logp, logq = torch.nn.functional.logsigmoid(lg), torch.nn.functional.logsigmoid(-lg)
    else:
        p, q = lg, 1 - lg
        logp, logq = torch.log(p), torch.log(q)
    if round_p_to_fp32:
        p = p.float().double()
        q = 1 - p
        logp, logq = torch.log(p), torch.log(q)
    return NS(p=p, q=q, logp=logp, logq=logq, x=x, s=s)


def partial_loss_value(lg, labels, weights, mode, uce, round_p_to_fp32=False):
    """The forward alone on an fp64 lg (differentiable): NS(loss, sums [C, 4], d [C], pr = partial_probs, hit, bce)."""
    nvox, C = lg.shape
    w = _d(weights)
    cls = torch.arange(C, dtype=F64, device=lg.device)
    hit = _d(labels)[:, None] == cls[None, :]
    pr = partial_probs(lg, mode, round_p_to_fp32)
    p = pr.p
    I, Z, Y = (p * hit).sum(0), (p * p).sum(0), hit.double().sum(0)
    bce = None
    B = torch.zeros(C, dtype=F64, device=lg.device)
    if uce == 1:
        bce = -torch.where(hit, pr.logp.clamp(min=-100.0), pr.logq.clamp(min=-100.0))
        B = bce.sum(0)
    elif uce == 2:
        bce = torch.where(hit, -pr.logp, torch.zeros_like(p))
        B = bce.sum(0)
    d = 1 - (2 * I + SMOOTH) / (Z + Y + SMOOTH)
    loss = (d * w).sum() / C
    if uce == 1:
        loss = loss + (B / nvox * w).sum()
    elif uce == 2:
        loss = loss + B.sum() / nvox
    return NS(loss=loss, sums=torch.stack([I, Z, Y, B], 1), d=d, pr=pr, hit=hit, bce=bce)


def partial_loss_ref(logits, labels, weights, mode, uce, grad_out=None, round_p_to_fp32=False, sums=None):
    """logits [nvox, C], labels [nvox], weights [C] as stored. Returns the forward (partial_loss_value) and, with
    grad_out, dl [nvox, C] = grad_out * d loss / d logits formed from `sums` (default: the reference's own), with the
    intermediates g = dL/dp, g1 = its Dice part, g2 = its BCE part, gp_abs = sum_c |g_c p_c|, ce = the uce 2 term,
    and the coefficients a, b, kb [C]."""
    with torch.no_grad():
        lg = _d(logits)
        nvox, C = lg.shape
        f = partial_loss_value(lg, labels, weights, mode, uce, round_p_to_fp32)
        f.bce_abs = f.bce.abs().sum(0) if f.bce is not None else torch.zeros(C, dtype=F64, device=lg.device)
        if grad_out is None:
            return f
        w, go = _d(weights), float(grad_out)
        S4 = f.sums if sums is None else _d(sums)
        I, Z, Y = S4[:, 0], S4[:, 1], S4[:, 2]
        num, den = 2 * I + SMOOTH, Z + Y + SMOOTH
        scale = w / C * go
        f.a, f.b = -2 / den * scale, 2 * num / (den * den) * scale
        f.kb = w / nvox * go if uce == 1 else torch.full_like(w, go / nvox) if uce == 2 else torch.zeros_like(w)
        p, q, t = f.pr.p, f.pr.q, f.hit.double()
        f.g1 = t * f.a + p * f.b
        f.g2 = f.kb * (p - t) / (q * p).clamp(min=1e-12) if uce == 1 else torch.zeros_like(p)
        g = f.g1 + f.g2
        f.g = g
        f.gp_abs = (g * p).abs().sum(1, keepdim=True)
        if mode == MODE_SOFTMAX:
            f.dot = (g * p).sum(1, keepdim=True)
            r = p * (g - f.dot)
        elif mode == MODE_SIGMOID:
            r = g * q * p
        else:
            r = g
        f.r0 = r
        f.ce = f.kb * (p - t) * f.hit.any(1, keepdim=True) if uce == 2 else None   # no label, no cross-entropy term
        f.dl = r + f.ce if uce == 2 else r
        return f


# ------------------------------------------------------------------------------------------------ Dice metrics
def _ratios(cnt):
    """cnt [S, n, 3] fp64 (TP, P, T) -> [n, 3]: dice, sensitivity, precision with the reference's + 1, mean over S."""
    tp, pp, tt = cnt[..., 0], cnt[..., 1], cnt[..., 2]
    return torch.stack([2 * tp / (pp + tt + 1), tp / (tt + 1), tp / (pp + 1)], -1).mean(0)


def dice_metric_ref(logits, labels, num_class):
    """logits [S, V, C], labels [S, V] -> argmax [S, V] int64 (first maximum on ties), counts [S, num_class, 3] int64
    (TP, P, T) for l = 1..num_class, metrics [num_class, 3] fp64. A non-integer label matches no class."""
    lg, lab = _d(logits), _d(labels)
    idx = torch.arange(lg.shape[2], device=lg.device).expand_as(lg)
    am = torch.where(lg == lg.max(2, keepdim=True).values, idx, lg.shape[2]).amin(2)    # the first maximal index
    cls = torch.arange(1, num_class + 1, device=lg.device)
    P = am[..., None] == cls
    T = lab[..., None] == cls.double()
    cnt = torch.stack([(P & T).sum(1), P.sum(1), T.sum(1)], -1)
    return NS(argmax=am, counts=cnt, metrics=_ratios(cnt.double()))


def dice_binary_ref(refine, rsn, rsc, rsv, nt, V, labels):
    """refine: flat storage read with element strides (organ rsn, class rsc, voxel rsv); labels [V]. Organ l's
    prediction argmax == 1 (channel 1 strictly above channel 0) against labels == l + 1."""
    flat, lab = _d(refine).reshape(-1), _d(labels)
    g = torch.arange(nt, device=flat.device)[:, None] * rsn + torch.arange(V, device=flat.device)[None, :] * rsv
    r0, r1 = flat[g], flat[g + rsc]
    am = (r1 > r0).long()
    T = lab[None, :] == torch.arange(1, nt + 1, device=flat.device, dtype=F64)[:, None]
    P = am == 1
    cnt = torch.stack([(P & T).sum(1), P.sum(1), T.sum(1)], -1)          # [nt, 3]
    return NS(argmax=am, counts=cnt, metrics=_ratios(cnt.double()[None]), gap=(r1 - r0).abs())


# ------------------------------------------------------------------------------------------------ partial target
def partial_target_ref(labels, mask, mask_stride, M, lmin, lmax):
    """labels [S, V]; mask int64 flat, row s at s * mask_stride (0: one row for all), M entries per row: every label l
    in [lmin, lmax] with l < M and mask[s][l] == 0 becomes 0."""
    lab = labels.detach().clone()
    S = lab.shape[0]
    for s in range(S):
        row = mask.reshape(-1)[s * mask_stride: s * mask_stride + M]
        for l in range(lmin, min(lmax, M - 1) + 1):
            if int(row[l]) == 0:
                lab[s][lab[s] == float(l)] = 0
    return lab


# ------------------------------------------------------------------------------------------------ consistency
def _gather(flat, idx):
    return flat.reshape(-1)[idx]


def consistency_value(atts, logits_vc, r0, r1, label_t, confi, weight_feature):
    """Differentiable core on fp64 operands: atts = list of [nt, V] attention logits, logits_vc [V, C], r0 / r1 [nt, V]
    the refiner's two channels. NS(aux, dice [nt, 4], coef [nt, 4, 2], per-voxel intermediates)."""
    natt = len(atts)
    nt, V = r0.shape
    dev = r0.device
    t = torch.softmax(torch.stack([r0, r1], 0), 0)[1]
    hi, lo = f32(1.0 - f32(confi)), f32(confi)
    conf = (t > hi) | (t < lo)
    active = _d(label_t) == 0
    on = (conf & active[:, None]).double()                                   # [nt, V]
    p = torch.softmax(logits_vc, 1)                                          # [V, C]
    pm = p[:, 1:nt + 1].t()                                                  # [nt, V]
    sup = int((~active).sum())
    maps, wts, sig = [], [], []
    for k in range(3):
        if k < natt:
            maps.append(torch.sigmoid(atts[k]))
            wts.append(CONSIST_W[k])
            sig.append(True)
        else:
            maps.append(None)
            wts.append(0.0)
            sig.append(False)
    sig.append(natt != 3)
    maps.append(torch.sigmoid(pm) if natt != 3 else pm)
    wts.append(CONSIST_W[natt])
    wf = f32(weight_feature)
    Y = (t * t * on).sum(1)
    z = torch.zeros(nt, dtype=F64, device=dev)
    dice, cA, cB, Is, Zs, cs = [], [], [], [], [], []
    aux = torch.zeros((), dtype=F64, device=dev)
    for k in range(4):
        if maps[k] is None:
            for lst in (dice, cA, cB, Is, Zs, cs):
                lst.append(z)
            continue
        s = maps[k]
        I, Z = (s * t * on).sum(1), (s * s * on).sum(1)
        den, num = Z + Y + SMOOTH, 2 * I + SMOOTH
        d = (1 - num / den) * active
        c = active.double() * wts[k] * wf / (nt - sup) if nt > sup else z
        aux = aux + (d * c).sum()
        dice.append(d), cA.append(c * 2 / den), cB.append(c * 2 * num / (den * den)), Is.append(I), Zs.append(Z)
        cs.append(c)
    st = lambda l: torch.stack(l, 1)                                          # noqa: E731
    return NS(aux=aux, dice=st(dice), coef=torch.stack([st(cA), st(cB)], 2), I=st(Is), Z=st(Zs), Y=Y, c=st(cs),
              t=t, on=on, p=p, pm=pm, maps=maps, sig=sig, natt=natt, active=active, sup=sup)


def consistency_ref(atts, logits_vc, r0, r1, label_t, confi, weight_feature, grad_out=None, coef=None):
    """Forward as consistency_value; with grad_out the backward from `coef` [nt, 4, 2] (default: the reference's own):
    datt [natt][nt, V] and dlogits [V, C], plus gp [V, C] = d aux / d softmax(logits) and its per-voxel parts."""
    with torch.no_grad():
        atts = [_d(a) for a in atts]
        lg, r0, r1 = _d(logits_vc), _d(r0), _d(r1)
        f = consistency_value(atts, lg, r0, r1, label_t, confi, weight_feature)
        if grad_out is None:
            return f
        go = float(grad_out)
        cf = f.coef if coef is None else _d(coef)
        nt, V = r0.shape
        C = lg.shape[1]
        f.datt, f.inner = [], []
        for k in range(f.natt):
            s = f.maps[k]
            inner = cf[:, k, 1:2] * s - cf[:, k, 0:1] * f.t
            f.inner.append(inner)
            f.datt.append(go * inner * s * (1 - s) * f.on)
        s = f.maps[3]
        inner = cf[:, 3, 1:2] * s - cf[:, 3, 0:1] * f.t
        gpm = go * inner * f.on
        if f.sig[3]:
            gpm = gpm * s * (1 - s)
        f.inner3 = inner
        gp = torch.zeros(V, C, dtype=F64, device=lg.device)
        gp[:, 1:nt + 1] = gpm.t()
        f.gp = gp
        f.dot = (gp * f.p).sum(1, keepdim=True)
        f.gpp_abs = (gp * f.p).abs().sum(1, keepdim=True)
        f.dl = f.p * (gp - f.dot)
        f.coef_used = cf
        return f


# ------------------------------------------------------------------------------------------------ EDiceLoss_full2
def full2_value(x, t, m, sigmoid, uce):
    """Differentiable core, fp64 x, t, m [V] (m None = all ones): NS(loss, I, Z, Y, bce [V] or None, s, on)."""
    on = torch.ones_like(t) if m is None else (m != 0).double()
    s = torch.sigmoid(x) if sigmoid else x
    I, Z, Y = (s * t * on).sum(), (s * s * on).sum(), (t * t * on).sum()
    num, den = 2 * I + SMOOTH, Z + Y + SMOOTH
    loss = 1 - num / den
    bce = None
    if uce:
        ls = torch.nn.functional.logsigmoid            # = max(x, 0) - x t + log1p(exp(-|x|)), smooth at 0
        bce = -(t * ls(x) + (1 - t) * ls(-x))
        loss = loss + bce.sum() / x.numel()
    return NS(loss=loss, I=I, Z=Z, Y=Y, num=num, den=den, bce=bce, s=s, on=on)


def full2_ref(x, t, m, sigmoid, uce, grad_out=None, coef=None):
    """Forward, coef = (2 / den, 2 num / den^2, uce / V), and with grad_out dx [V] from `coef` (default: its own)."""
    with torch.no_grad():
        x, t = _d(x), _d(t)
        m = None if m is None else _d(m)
        f = full2_value(x, t, m, sigmoid, uce)
        V = x.numel()
        f.coef = torch.stack([2 / f.den, 2 * f.num / (f.den * f.den),
                              torch.tensor((1.0 / V) if uce else 0.0, dtype=F64, device=x.device)])
        if grad_out is None:
            return f
        A, B, cb = (_d(coef) if coef is not None else f.coef).tolist()
        go = float(grad_out)
        sg = torch.sigmoid(x)
        f.sg = sg
        f.dbce = cb * (sg - t)
        f.ds = (B * f.s - A * t) * f.on
        f.dd = f.ds * f.s * (1 - f.s) if sigmoid else f.ds
        f.dx = go * (f.dbce + f.dd)
        return f
