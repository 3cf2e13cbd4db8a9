"""fp64 restatements of the trunk's edge kernels, on the SAME operands the kernels read: the trilinear x2 upsample and
its adjoint (csrc/upsample.hip), the stem convolution and its weight gradient (stem.hip), the streaming classifier head
with its data gradient, bias partials and GroupNorm-backward partials (head.hip), and the helpers of misc.hip. The
reference test_gpu_trunk_edge.py compares those kernels against; pinned to torch (F.interpolate and its autograd,
conv3d autograd, group_norm autograd) and to oracle/ref_cpu.py by test_trunk_edge_reference.py. CPU only: nothing here
imports the GPU package. The convolution references, decode_pf, prologue_ref and the bound functions are those of
conv_reference.py.

Every function returns the value and its absolute-sum companion S (the same operation on the absolute operands).

Upsample.  Per axis the dense weight matrix U_n [2n, n] of the documented source-index rule (upsample.hip:4-5):
src = max(0, (o + .5) / 2 - .5), i0 = floor(src), i1 = i0 + (i0 < n - 1), l1 = src - i0, l0 = 1 - l1; U[o, i0] += l0,
U[o, i1] += l1, so both weights fall on one input when n = 1 or at the far face. Forward y = (U_d x U_h x U_w) x
(+ skip); backward the transpose (+ prev). Every weight is non-negative (0, .25, .75 or 1, exact in every format), so
S is the same operator on |x|.

Head.  The backward reference reads the FORWARD pack's weights and dy.to(bf16) (round-to-nearest-even: what the kernel's
conversion must produce), never the data-gradient pack, so a wrong transpose in pd shows. GroupNorm partials: per
(sample, channel) sum g and sum g xhat with g = [pre > 0] dA, pre = x0 sc + sh, xhat = (x0 - mean) rstd, all in fp64 from
the handed fp32 statistics; a voxel with |pre| <= E (conv_reference.py's bound on the fp32 prologue's error) may take
the other side of the ReLU test in the kernel, and adds |dA| (|dA xhat|) to the bound D of the sums it feeds.
"""
import torch

from conv_reference import BF, U32, conv_fwd_ref, conv_wgrad_ref, nd


# ------------------------------------------------------------------------------------------------- upsample
def up_matrix(n):
    """U_n [2n, n] fp64: the weights of output o onto the inputs along one axis."""
    U = torch.zeros((2 * n, n), dtype=torch.float64)
    for o in range(2 * n):
        src = max(0.0, (o + 0.5) * 0.5 - 0.5)
        i0 = int(src)
        i1 = i0 + (1 if i0 < n - 1 else 0)
        l1 = src - i0
        U[o, i0] += 1.0 - l1
        U[o, i1] += l1
    return U


def upsample_fwd_ref(x, skip=None):
    """x [n,d,h,w,c], skip [n,2d,2h,2w,c] or None (any float dtype: the stored values). Returns (y, S) fp64."""
    _, d, h, w, _ = x.shape
    Ud, Uh, Uw = up_matrix(d), up_matrix(h), up_matrix(w)
    f = lambda t: torch.einsum("ad,bh,cw,ndhwk->nabck", Ud, Uh, Uw, t)
    y, s = f(x.double()), f(x.double().abs())
    if skip is not None:
        y, s = y + skip.double(), s + skip.double().abs()
    return y, s


def upsample_bwd_ref(dy, prev=None):
    """dy [n,2d,2h,2w,c], prev [n,d,h,w,c] or None (accumulate). Returns (dx, S) fp64."""
    d, h, w = (e // 2 for e in dy.shape[1:4])
    Ud, Uh, Uw = up_matrix(d), up_matrix(h), up_matrix(w)
    f = lambda t: torch.einsum("ad,bh,cw,nabck->ndhwk", Ud, Uh, Uw, t)
    dx, s = f(dy.double()), f(dy.double().abs())
    if prev is not None:
        dx, s = dx + prev.double(), s + prev.double().abs()
    return dx, s


# ------------------------------------------------------------------------------------------------- stem
def stem_operand(x_ncdhw, bf16_operand):
    """The stem's input as the kernel multiplies it: NDHWC fp64 of the fp32 volume, or of x.to(bf16) (RNE) for the
    matrix-core kernels (stem1_mfma_kernel, stem_wgrad_mfma_kernel)."""
    x = x_ncdhw.to(BF) if bf16_operand else x_ncdhw
    return nd(x.double())


def stem_fwd_ref(a, wq, stride):
    """a [n,d,h,w,cin] fp64 (stem_operand), wq = decode_pf(pf, cout, cin, 3). Returns (y, S) NDHWC."""
    return conv_fwd_ref(a, wq, 3, stride)


def stem_wgrad_ref(a, dy, stride):
    """a [n,d,h,w,cin] fp64, dy [n,od,oh,ow,cout] (the stored values). Returns (dw, S) as [27][cout][cin]."""
    return conv_wgrad_ref(a, dy.double(), 3, stride)


# ------------------------------------------------------------------------------------------------- head
def head_fwd_ref(a, wq, bias=None, a_delta=None):
    """a [n,v,cin] fp64 (the prologue's activations or x.double()), wq = decode_pf(pf, cout, cin, 1), bias [cout] or
    None. Returns (y, S) [n,v,cout], or (y, S, D) with a_delta."""
    v5 = lambda t: None if t is None else t[:, :, None, None, :]
    out = conv_fwd_ref(v5(a), wq, 1, 1, None, None if bias is None else bias.double(), a_delta=v5(a_delta))
    return tuple(t[:, :, 0, 0, :] for t in out)


def head_bwd_ref(dy, wq):
    """dy fp32 [rows, cout], wq = decode_pf(pf, cout, cin, 1) (the FORWARD pack). Returns (dA, S) fp64 [rows, cin], the
    bf16 image of dy [rows, round8(cout)] with zero padding columns, and (column sums, their absolute sums) of the
    fp32 dy."""
    rows, cout = dy.shape
    w2 = wq.reshape(wq.shape[0], wq.shape[1])
    dyb = torch.zeros((rows, (cout + 7) // 8 * 8), dtype=BF)
    dyb[:, :cout] = dy.to(BF)
    q = dyb[:, :cout].double()
    return q @ w2, q.abs() @ w2.abs(), dyb, (dy.double().sum(0), dy.double().abs().sum(0))


def head_gn_parts_ref(x0, dA, stats, gamma, beta, G):
    """x0 [n,v,c] bf16, dA [n,v,c] (the kernel's stored bf16 data gradient), stats [n,G,2] fp32 (mean, rstd).
    Returns (P, S, D, share): P [n,c,2] = (sum g, sum g xhat), S its absolute sums, D the ambiguity term and the
    ambiguous share of the voxels."""
    n, c = x0.shape[0], x0.shape[-1]
    xs, da = x0.double(), dA.double()
    gi = torch.arange(c) // (c // G)
    st = stats.double().cpu()
    mean, rstd = st[:, gi, 0][:, None], st[:, gi, 1][:, None]              # [n, 1, c]
    sc = rstd * gamma.double().cpu()
    sh = beta.double().cpu() - mean * sc
    xsc = xs * sc
    pre = xsc + sh
    E = U32 * (3 * xsc.abs() + 2 * (mean * sc).abs() + 2 * sh.abs())
    amb = pre.abs() <= E
    xhat = (xs - mean) * rstd
    g = torch.where(pre > 0, da, torch.zeros_like(da))
    P = torch.stack((g.sum(1), (g * xhat).sum(1)), -1)
    S = torch.stack((g.abs().sum(1), (g * xhat).abs().sum(1)), -1)
    D = torch.stack(((amb * da.abs()).sum(1), (amb * (da * xhat).abs()).sum(1)), -1)
    return P, S, D, amb.double().mean().item()


# ------------------------------------------------------------------------------------------------- helpers
def add_ref(y, x):
    """(y + x, |y| + |x|) in fp64."""
    return y.double() + x.double(), y.double().abs() + x.double().abs()


def channel_sum_ref(x, prev=None):
    """x [rows, c]; prev [c] fp32 or None. Returns (column sums (+ prev), absolute sums) fp64."""
    s, a = x.double().sum(0), x.double().abs().sum(0)
    if prev is not None:
        s, a = s + prev.double(), a + prev.double().abs()
    return s, a


def cast_ref(x, dtype, cout):
    """x [rows, cin] -> [rows, cout] of dtype: x.to(dtype) (round-to-nearest-even) and zero padding columns."""
    y = torch.zeros((x.shape[0], cout), dtype=dtype)
    y[:, :x.shape[1]] = x.to(dtype)
    return y
