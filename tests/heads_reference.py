"""fp64 restatements of the two model heads on top of the trunk: the EAM attention branch (csrc/eam.hip: token side,
forward, backward, parameter backward) and the DynConv 8,8,2 head (csrc/dynhead.hip: controller, per-voxel MLP, their
backwards). They are the independent references of test_gpu_eam.py and test_gpu_dynhead.py, and are themselves pinned
to oracle.ref_cpu.eam_attn / oracle.ref_cpu.unet3d_dyn_forward and torch's autograd by test_heads_reference.py.

All of them take the operands as they are stored (fp32, or bf16 upcast exactly) and compute in fp64. Next to each
result they return the sums of the absolute values of the terms that make it up (the same formula on |operands|) and
the per-voxel intermediates, from which the GPU tests build their rounding bounds.

EAM (eps = 1e-5, biased variance), x [n, v, c], token [nt, c]:
    zhat = LN(tok), z = zhat g3 + b3, q = z Wq^T, M = inv_h q Wk                               (token side)
    xhat = (x - mean) rstd,   att[n, t, v] = sum_c M[t, c] (xhat g2 + b2)[c]                   (forward)
    dl = sum_t g[t] M[t], dxh = dl g2, dx = rstd (dxh - mean_c(dxh) - xhat mean_c(dxh xhat))   (backward)
    dM[t, c] = g2[c] sum_v g[t] xhat[c] + b2[c] sum_v g[t], dg2 = sum_v dl xhat, db2 = sum_v dl
    dq = inv_h dM Wk^T, dz = dq Wq, dWq = dq^T z, dWk = inv_h q^T dM (rows 0..c-1 of dkv [2c, c]; the rest 0),
    dg3 = sum_t dz zhat, db3 = sum_t dz                                                        (parameter backward)
Dynamic head, params[162] = [W1 8x8 | W2 8x8 | W3 2x8 | b1 8 | b2 8 | b3 2] ([out][in]):
    params = Wc cat(feat, onehot(task, 7)) + bc
    a1 = W1 h + b1, r1 = relu(a1), a2 = W2 r1 + b2, r2 = relu(a2), out = W3 r2 + b3
"""
from types import SimpleNamespace as NS

import torch

U = 2.0 ** -24      # unit roundoff of fp32
LN_EPS = 1e-5
F64 = torch.float64


def _d(t):
    return t.detach().to(F64)


def ln_ref(x):
    """Per-row LayerNorm statistics of x [..., c]: mean, rstd, xhat and the sums sum|x|, sum|x - mean|, sum (x - mean)^2."""
    x = _d(x)
    c = x.shape[-1]
    mean = x.sum(-1, keepdim=True) / c
    d = x - mean
    s2 = (d * d).sum(-1, keepdim=True)
    rstd = 1.0 / torch.sqrt(s2 / c + LN_EPS)
    return NS(mean=mean, rstd=rstd, xhat=d * rstd, d=d, sabs=x.abs().sum(-1, keepdim=True),
              s1=d.abs().sum(-1, keepdim=True), s2=s2)


# ------------------------------------------------------------------------------------------------ EAM token side
def eam_token_ref(tok, g3, b3, wq, wk, inv_h):
    """tok [nt, c], wq [c, c], wk [c, c] (rows 0..c-1 of kv.weight) -> zhat, q, M [nt, c] and z, the LN statistics of
    the tokens (ln) and q_abs = |z| |Wq|^T, M_abs = inv_h |q| |Wk|."""
    g3, b3, wq, wk = _d(g3), _d(b3), _d(wq), _d(wk)
    ln = ln_ref(tok)
    z = ln.xhat * g3 + b3
    q = z @ wq.t()
    M = inv_h * (q @ wk)
    return NS(zhat=ln.xhat, z=z, q=q, M=M, ln=ln, q_abs=z.abs() @ wq.abs().t(), M_abs=inv_h * (q.abs() @ wk.abs()))


def eam_param_bwd_ref(dM, zhat, q, g3, b3, wq, wk, inv_h):
    """dM, zhat, q [nt, c] as stored -> dWq [c, c], dkv [2c, c], dg3, db3 [c]; dq, dz, z and each one's abs-sum."""
    dM, zhat, q, g3, b3, wq, wk = map(_d, (dM, zhat, q, g3, b3, wq, wk))
    c = dM.shape[1]
    z = zhat * g3 + b3
    dq = inv_h * (dM @ wk.t())
    dz = dq @ wq
    dkv = torch.zeros((2 * c, c), dtype=F64)
    dkv[:c] = inv_h * (q.t() @ dM)
    return NS(dq=dq, dz=dz, z=z, dwq=dq.t() @ z, dkv=dkv, dg3=(dz * zhat).sum(0), db3=dz.sum(0),
              dq_abs=inv_h * (dM.abs() @ wk.abs().t()), dz_abs=dq.abs() @ wq.abs(),
              dwq_abs=dq.abs().t() @ z.abs(), dkv_abs=inv_h * (q.abs().t() @ dM.abs()),
              dg3_abs=(dz * zhat).abs().sum(0), db3_abs=dz.abs().sum(0))


# ------------------------------------------------------------------------------------------------ EAM voxel side
def eam_fwd_ref(x, g2, b2, M, chunk=1 << 16):
    """x [n, v, c], M [nt, c] -> att [n, nt, v]; att_abs = rstd sum_c |A_tc| |x_c - mean| with A = M g2 (same shape);
    a0_abs [nt] = sum_c |M_tc b2_c|; A_abs [nt] = sum_c |A_tc|; and the per-voxel LN sums mean, rstd, sabs, s1, s2
    ([n, v]). Walks the voxels in chunks, so the largest case needs no full-size fp64 copy of x."""
    g2, b2, M = _d(g2), _d(b2), _d(M)
    n, v, c = x.shape
    A = M * g2
    a0 = M @ b2
    flat = x.reshape(n * v, c)
    att, att_abs, stats = [], [], {k: [] for k in ("mean", "rstd", "sabs", "s1", "s2")}
    for i in range(0, n * v, chunk):
        ln = ln_ref(flat[i:i + chunk])
        att.append((ln.rstd * (ln.d @ A.t()) + a0).t())
        att_abs.append((ln.rstd * (ln.d.abs() @ A.abs().t())).t())
        for k in stats:
            stats[k].append(getattr(ln, k)[:, 0])

    def maps(parts):  # [nt, n*v] -> [n, nt, v]
        return torch.cat(parts, 1).reshape(-1, n, v).permute(1, 0, 2).contiguous()
    return NS(att=maps(att), att_abs=maps(att_abs), a0_abs=(M * b2).abs().sum(1), A_abs=A.abs().sum(1),
              **{k: torch.cat(p).reshape(n, v) for k, p in stats.items()})


def eam_bwd_ref(x, g2, b2, M, gout):
    """x [n, v, c], gout [n, nt, v] -> dx [n, v, c], dM [nt, c], dg2, db2 [c], with the per-voxel intermediates
    (ln, dl, dxh, m1, m2 and dl_abs = sum_t |g_t M_tc|) and the abs-sums of the four reductions:
    P = sum_v g xhat (P_abs), Gs = sum_v g (Gs_abs), dg2_abs, db2_abs."""
    g2, b2, M = _d(g2), _d(b2), _d(M)
    n, v, c = x.shape
    g = _d(gout).permute(0, 2, 1).reshape(n * v, -1)          # [nv, nt]
    ln = ln_ref(x.reshape(n * v, c))
    dl = g @ M
    dxh = dl * g2
    m1 = dxh.sum(1, keepdim=True) / c
    m2 = (dxh * ln.xhat).sum(1, keepdim=True) / c
    dx = ln.rstd * (dxh - m1 - ln.xhat * m2)
    P, Gs = g.t() @ ln.xhat, g.sum(0)
    return NS(dx=dx.reshape(n, v, c), dM=g2 * P + b2 * Gs[:, None], dg2=(dl * ln.xhat).sum(0), db2=dl.sum(0),
              ln=ln, g=g, dl=dl, dl_abs=g.abs() @ M.abs(), dxh=dxh, m1=m1, m2=m2, P=P, Gs=Gs,
              P_abs=g.abs().t() @ ln.xhat.abs(), Gs_abs=g.abs().sum(0), dg2_abs=(dl * ln.xhat).abs().sum(0),
              db2_abs=dl.abs().sum(0))


# ------------------------------------------------------------------------------------------------ dynamic head
def split_params(p):
    """params [n, 162] -> W1 [n, 8, 8], W2 [n, 8, 8], W3 [n, 2, 8], b1 [n, 8], b2 [n, 8], b3 [n, 2]."""
    n = p.shape[0]
    return (p[:, 0:64].reshape(n, 8, 8), p[:, 64:128].reshape(n, 8, 8), p[:, 128:144].reshape(n, 2, 8),
            p[:, 144:152], p[:, 152:160], p[:, 160:162])


def join_params(w1, w2, w3, b1, b2, b3):
    n = w1.shape[0]
    return torch.cat([w1.reshape(n, 64), w2.reshape(n, 64), w3.reshape(n, 16), b1, b2, b3], 1)


def controller_ref(feat, task, w, b, kt=7):
    """feat [n, kf], task [n] (int), w [m, kf + kt], b [m] -> params [n, m] and the abs-sum of its terms."""
    feat, w, b = _d(feat), _d(w), _d(b)
    x = torch.cat([feat, torch.nn.functional.one_hot(task.long(), kt).to(F64)], 1)
    return NS(params=x @ w.t() + b, abs=x.abs() @ w.abs().t() + b.abs(), x=x)


def _lin(w, b, x):        # [n, o, k], [n, o], [n, v, k] -> [n, v, o]
    return torch.einsum("nok,nvk->nvo", w, x) + b[:, None, :]


def dynhead_fwd_ref(h, params):
    """h [n, v, 8], params [n, 162] -> out [n, v, 2], the pre-activations a1, a2 and r1, r2, and the abs-sums of the
    three layers a1_abs, a2_abs, out_abs (|b| + |W| |input|)."""
    h, p = _d(h), _d(params)
    w1, w2, w3, b1, b2, b3 = split_params(p)
    a1 = _lin(w1, b1, h)
    r1 = a1.clamp(min=0)
    a2 = _lin(w2, b2, r1)
    r2 = a2.clamp(min=0)
    return NS(out=_lin(w3, b3, r2), a1=a1, r1=r1, a2=a2, r2=r2, h=h, a1_abs=_lin(w1.abs(), b1.abs(), h.abs()),
              a2_abs=_lin(w2.abs(), b2.abs(), r1), out_abs=_lin(w3.abs(), b3.abs(), r2))


def dynhead_bwd_ref(h, params, dout):
    """-> dh [n, v, 8], dparams [n, 162] (layout of params) with its abs-sum dparams_abs, and per voxel: the forward
    (fwd), da2, da1 (gradients of the pre-activations) and the abs-sums dr2_abs, dr1_abs, dh_abs of the products that
    make up dr2 = W3^T d, dr1 = W2^T da2 and dh = W1^T da1 (each on the abs-sum of the one before)."""
    f = dynhead_fwd_ref(h, params)
    d = _d(dout)
    w1, w2, w3, _, _, _ = split_params(_d(params))
    k1, k2 = (f.a1 > 0).to(F64), (f.a2 > 0).to(F64)
    dr2 = torch.einsum("nok,nvo->nvk", w3, d)
    dr2_abs = torch.einsum("nok,nvo->nvk", w3.abs(), d.abs())
    da2 = dr2 * k2
    dr1 = torch.einsum("nok,nvo->nvk", w2, da2)
    dr1_abs = torch.einsum("nok,nvo->nvk", w2.abs(), dr2_abs * k2)
    da1 = dr1 * k1
    dh = torch.einsum("nok,nvo->nvk", w1, da1)
    dh_abs = torch.einsum("nok,nvo->nvk", w1.abs(), dr1_abs * k1)

    def outer(a, b):      # sum_v a[n, v, o] b[n, v, k] -> [n, o, k]
        return torch.einsum("nvo,nvk->nok", a, b)
    dparams = join_params(outer(da1, f.h), outer(da2, f.r1), outer(d, f.r2), da1.sum(1), da2.sum(1), d.sum(1))
    dabs = join_params(outer(da1.abs(), f.h.abs()), outer(da2.abs(), f.r1), outer(d.abs(), f.r2), da1.abs().sum(1),
                       da2.abs().sum(1), d.abs().sum(1))
    return NS(dh=dh, dparams=dparams, dparams_abs=dabs, fwd=f, d=d, k1=k1, k2=k2, da1=da1, da2=da2, dr2_abs=dr2_abs,
              dr1_abs=dr1_abs, dh_abs=dh_abs, dh_abs1=torch.einsum("nok,nvo->nvk", w1.abs(), da1.abs()))


def controller_bwd_ref(feat, task, w, dparams, v, kt=7):
    """-> dW [m, kf + kt], db [m], dA [n, kf] = dfeat / v (the value every one of the v bottleneck voxels receives) and
    the abs-sums of each."""
    feat, w, dy = _d(feat), _d(w), _d(dparams)
    kf = feat.shape[1]
    x = torch.cat([feat, torch.nn.functional.one_hot(task.long(), kt).to(F64)], 1)
    return NS(dw=dy.t() @ x, db=dy.sum(0), dA=(dy @ w[:, :kf]) / v, dw_abs=dy.abs().t() @ x.abs(),
              db_abs=dy.abs().sum(0), dA_abs=(dy.abs() @ w[:, :kf].abs()) / v)
