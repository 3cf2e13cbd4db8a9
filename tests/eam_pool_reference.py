"""fp64 restatement of the EAM class message (csrc/eam_pool.hip, u3d.feam.eam_pool_op): attention pooling of one decoder
level against the class tokens, forward and backward. It is the independent reference of test_gpu_eam_pool.py and is
itself pinned to torch autograd of a literal softmax(q k^T scale) @ v attention by test_eam_pool_reference.py.

h = 4 heads, hd = c / h, scale = hd^-0.5; head i owns channels i hd .. (i + 1) hd - 1; Wk = kv.weight[:c],
Wv = kv.weight[c:]; xhat_n = LayerNorm-normalised voxel (eps 1e-5, biased variance); u_n = xhat_n g2 + b2; the rows
r = i nt + t run over (head, token).

    token side, before   z = LN3(tok) g3 + b3,  q = z Wq^T,  A[r] = q[t, head i] Wk[head i, :]             A [h nt, c]
    voxel side           S[r, n] = A[r] . u_n,  att[t, n] = 1/h sum_i S[i nt + t, n]
                         P[r, .] = softmax_n(scale S[r, .]),  Yhat[r] = sum_n P[r, n] xhat_n
    token side, after    Y = Yhat g2 + b2,  O[t, head i] = Wv[head i, :] . Y[i nt + t],  cm = proj(LN2(O)) + O
    voxel side backward  D[r] = dYhat[r] . Yhat[r],  dP = dYhat[r] . xhat_n,  dS = scale P (dP - D) + gatt[t, n] / h
                         dl_n = sum_r dS[r, n] A[r],  dxhat_n = sum_r P[r, n] dYhat[r] + g2 dl_n,  dx = LN backward
                         dA[r] = sum_n dS[r, n] u_n,  dg2 = sum_n dl_n xhat_n,  db2 = sum_n dl_n

The voxel side is written out by hand, forward and backward; the two token sides are a few [<= 16, <= 128] products
whose backward is torch's own (they are torch operations on the device too). Everything takes the operands as they
are stored (fp32, or bf16 upcast exactly) and computes in fp64; next to each result come the per-voxel intermediates
and the sums of absolute values of the terms that make it up, from which the GPU test builds its rounding bounds.
"""
from types import SimpleNamespace as NS

import torch
import torch.nn.functional as F

from heads_reference import F64, LN_EPS, U, _d, ln_ref  # noqa: F401

HEADS = 4


def token_before(tok, g3, b3, wq, wk, heads=HEADS):
    """tok [nt, c] -> A [heads nt, c] (differentiable torch, the caller's dtype)."""
    c = tok.shape[1]
    hd = c // heads
    q = F.layer_norm(tok, (c,), g3, b3, LN_EPS) @ wq.t()
    return torch.cat([q[:, i * hd:(i + 1) * hd] @ wk[i * hd:(i + 1) * hd] for i in range(heads)], 0)


def token_after(yhat, g2, b2, wv, pw, pb, heads=HEADS):
    """Yhat [heads nt, c] -> cm [nt, c] (differentiable torch)."""
    c = yhat.shape[1]
    hd, nt = c // heads, yhat.shape[0] // heads
    y = yhat * g2 + b2
    o = torch.cat([y[i * nt:(i + 1) * nt] @ wv[i * hd:(i + 1) * hd].t() for i in range(heads)], 1)
    return F.linear(F.layer_norm(o, (c,), g2, b2, LN_EPS), pw, pb) + o


def pool_fwd_ref(x, g2, b2, A, scale, heads=HEADS):
    """x [v, c], A [R, c] -> att [nt, v], Yhat [R, c], the softmax statistics m = max_n scale S and l = sum_n
    exp(scale S - m), and the intermediates ln, u, S, P with S_abs = |A| . |u| and Y_abs = sum_n P |xhat|."""
    g2, b2, A = _d(g2), _d(b2), _d(A)
    ln = ln_ref(x)
    u = ln.xhat * g2 + b2
    S = A @ u.t()
    nt = A.shape[0] // heads
    m = (scale * S).max(1).values
    E = torch.exp(scale * S - m[:, None])
    l = E.sum(1)
    P = E / l[:, None]
    return NS(ln=ln, u=u, S=S, S_abs=A.abs() @ u.abs().t(), att=S.reshape(heads, nt, -1).mean(0),
              att_abs=S.abs().reshape(heads, nt, -1).mean(0), m=m, l=l, P=P, yhat=P @ ln.xhat, y_abs=P @ ln.xhat.abs())


def pool_bwd_ref(x, g2, b2, A, scale, m, l, dyhat, D, gatt, heads=HEADS):
    """Backward of the voxel side from the operands as stored: the softmax statistics (m, l), dYhat [R, c] with its
    D [R] (or both None) and gatt [nt, v] (or None) -> dx [v, c], dA [R, c], dg2, db2 [c]; the intermediates ln, u, S,
    P, dP, dS, dl, dxh, m1, m2; the block sums PS = sum_n dS xhat, Gs = sum_n dS; and the abs-sums of each."""
    g2, b2, A, m, l = map(_d, (g2, b2, A, m, l))
    v, c = x.shape
    R = A.shape[0]
    dy = _d(dyhat) if dyhat is not None else torch.zeros(R, c, dtype=F64)
    D = _d(D) if D is not None else torch.zeros(R, dtype=F64)
    ga = _d(gatt).repeat(heads, 1) / heads if gatt is not None else torch.zeros(R, v, dtype=F64)
    ln = ln_ref(x)
    u = ln.xhat * g2 + b2
    S = A @ u.t()
    P = torch.exp(scale * S - m[:, None]) / l[:, None]
    dP = dy @ ln.xhat.t()
    dS = scale * P * (dP - D[:, None]) + ga
    dl = dS.t() @ A
    dxh = P.t() @ dy + g2 * dl
    m1 = dxh.sum(1, keepdim=True) / c
    m2 = (dxh * ln.xhat).sum(1, keepdim=True) / c
    PS, Gs = dS @ ln.xhat, dS.sum(1)
    return NS(dx=ln.rstd * (dxh - m1 - ln.xhat * m2), dA=g2 * PS + b2 * Gs[:, None], dg2=(A * PS).sum(0),
              db2=(A * Gs[:, None]).sum(0), dg2_direct=(dl * ln.xhat).sum(0), db2_direct=dl.sum(0),
              ln=ln, u=u, S=S, S_abs=A.abs() @ u.abs().t(), P=P, dP=dP, dP_abs=dy.abs() @ ln.xhat.abs().t(), dPD=dP - D[:, None],
              dS=dS, dl=dl, dl_abs=dS.abs().t() @ A.abs(), dxh=dxh, dxh_abs=P.t() @ dy.abs() + g2.abs() * (dS.abs().t() @ A.abs()),
              m1=m1, m2=m2, PS=PS, Gs=Gs, PS_abs=dS.abs() @ ln.xhat.abs(), Gs_abs=dS.abs().sum(1), dy=dy, D=D)


def eam_ref(x, tok, p, gcm=None, gatt=None, heads=HEADS):
    """The whole EAM by the folded math: x [v, c], tok [nt, c], p = dict(kv, q, proj_w, proj_b, g2, b2, g3, b3) ->
    cm [nt, c], att [nt, v] and, given gcm and / or gatt, the gradients of sum(cm gcm) + sum(att gatt) with respect
    to x, tok and every entry of p (dict `grad`)."""
    x, tok = _d(x), _d(tok)
    p = {k: _d(t) for k, t in p.items()}
    c = x.shape[1]
    scale = (c // heads) ** -0.5
    tl = {k: p[k].clone().requires_grad_(True) for k in ("g3", "b3", "q", "kv")}
    tokl = tok.clone().requires_grad_(True)
    A = token_before(tokl, tl["g3"], tl["b3"], tl["q"], tl["kv"][:c], heads)
    f = pool_fwd_ref(x, p["g2"], p["b2"], A, scale, heads)
    al = {k: p[k].clone().requires_grad_(True) for k in ("g2", "b2", "kv", "proj_w", "proj_b")}
    yl = f.yhat.clone().requires_grad_(True)
    cm = token_after(yl, al["g2"], al["b2"], al["kv"][c:], al["proj_w"], al["proj_b"], heads)
    out = NS(cm=cm.detach(), att=f.att, fwd=f, A=A.detach())
    if gcm is None and gatt is None:
        return out
    grad = {k: torch.zeros_like(t) for k, t in p.items()}
    dy = D = None
    if gcm is not None:
        gs = torch.autograd.grad(cm, [yl] + list(al.values()), _d(gcm))
        dy = gs[0]
        D = (dy * f.yhat).sum(1)
        for k, g in zip(al, gs[1:]):
            grad[k] += g
    b = pool_bwd_ref(x, p["g2"], p["b2"], A, scale, f.m, f.l, dy, D, gatt, heads)
    grad["g2"] += b.dg2
    grad["b2"] += b.db2
    gs = torch.autograd.grad(A, [tokl] + list(tl.values()), b.dA)
    for k, g in zip(tl, gs[1:]):
        grad[k] += g
    grad["tok"], grad["x"] = gs[0], b.dx
    out.grad, out.bwd = grad, b
    return out
