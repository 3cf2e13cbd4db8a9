"""fp64 restatement of the convolutions (forward, data gradient, weight gradient) and of the GroupNorm + ReLU prologue,
on NDHWC tensors and on the SAME rounded operands the kernels read: the reference test_gpu_conv.py compares every
convolution kernel against, pinned to torch autograd, oracle/ref_cpu.py and the golden vectors by
test_conv_reference.py. CPU only: nothing here imports the GPU package.

Operands.  Activations are x.to(dt).double(); the weights are decoded from the FORWARD pack pf [k^3][cout_p][cin_p]
(decode_pf) exactly as test_gpu_bf16.py decodes them. The data-gradient reference never reads the data-gradient pack
pd, so a wrong flip or transpose in pd shows.

Every function returns the value and its absolute-sum companion S: the same operation on |a|, |w|, |dy| (+ |res|,
+ |bias|), i.e. the sum of the absolute values of the terms behind each element.

Prologue.  prologue_ref evaluates v = relu(x * sc + sh), sc = rstd * gamma, sh = beta - mean * sc, in fp64 from the
fp32 statistics the kernel is handed, and rounds v to dt. The kernels evaluate the same expression in fp32, so their v
is off by at most

    E = 2^-24 (3 |x sc| + 2 |mean sc| + 2 |sh|)

(one rounding each of sc, mean * sc, beta - mean * sc and of the product and the sum, or of their fma). In bf16 an
activation is AMBIGUOUS when v lies within max(2^-12 spacing(v), E) of a bf16 rounding boundary or within
max(2^-20, E) of the ReLU zero: there the kernel may legitimately round the other way. No ambiguous activation is
excluded from any comparison; instead each contributes

    delta = spacing(a) + 2 E        (one whole bf16 spacing: the neighbouring value; 2^-8 |a| <= spacing(a) <= 2^-7 |a|)

times |w| (or |dy|) to the bound of the outputs it feeds: one more conv3d over delta (the *_ref functions take it as
``a_delta``). In fp32 no activation is rounded to a coarser grid: every activation carries delta = E + 2^-24 |v|.

Bounds (bound_store, bound_accum), per element:
  bf16 store   2^-8 |ref|: round-to-nearest-even to 8 significand bits is off by at most half a spacing, 2^-9 |v| at
               the top of a binade and 2^-8 |v| just above a power of two (test_gpu_groupnorm.py derives it)
  fp32 chain   (L + 1) 2^-24 S: L fp32 additions on the longest chain to one output, S the absolute sum
"""
import torch
import torch.nn.functional as F

BF, F32 = torch.bfloat16, torch.float32
U32 = 2.0 ** -24          # fp32 unit roundoff
MAX_AMBIGUOUS = 1e-3      # the cap on the ambiguous share of a case's activations (a condition, asserted on the CPU)


def cl(t):
    """NDHWC -> NCDHW."""
    return t.permute(0, 4, 1, 2, 3)


def nd(t):
    """NCDHW -> NDHWC."""
    return t.permute(0, 2, 3, 4, 1)


def out_dim(d, k, s):
    return (d + 2 * (k // 2) - k) // s + 1


def decode_pf(pf, cout, cin, k):
    """The forward pack [k^3][cout_p][cin_p] -> fp64 [cout][cin][k][k][k] (the values the kernels multiply)."""
    return pf.float().cpu()[:, :cout, :cin].permute(1, 2, 0).reshape(cout, cin, k, k, k).double()


def conv_fwd_ref(a, w, k, stride, res=None, bias=None, a_delta=None):
    """a [n,d,h,w,cin], w [cout,cin,k,k,k], res [n,od,oh,ow,cout], bias [cout], all fp64. Returns (y, S) NDHWC, or
    (y, S, D) with a_delta: D = conv(a_delta, |w|), the ambiguity term."""
    p = k // 2
    y = nd(F.conv3d(cl(a), w, stride=stride, padding=p))
    s = nd(F.conv3d(cl(a.abs()), w.abs(), stride=stride, padding=p))
    if res is not None:
        y, s = y + res, s + res.abs()
    if bias is not None:
        y, s = y + bias, s + bias.abs()
    if a_delta is None:
        return y, s
    return y, s, nd(F.conv3d(cl(a_delta), w.abs(), stride=stride, padding=p))


def conv_dgrad_ref(dy, w, in_shape, k, stride):
    """dy [n,od,oh,ow,cout], w [cout,cin,k,k,k] (decoded from the FORWARD pack), in_shape = (n, d, h, w). Returns
    (dx, S) [n,d,h,w,cin]."""
    n, d, h, w_ = in_shape
    shape = (n, w.shape[1], d, h, w_)
    p = k // 2
    dx = torch.nn.grad.conv3d_input(shape, w, cl(dy), stride=stride, padding=p)
    s = torch.nn.grad.conv3d_input(shape, w.abs(), cl(dy.abs()), stride=stride, padding=p)
    return nd(dx), nd(s)


def conv_wgrad_ref(a, dy, k, stride, a_delta=None):
    """a [n,d,h,w,cin], dy [n,od,oh,ow,cout]. Returns (dw, S) as [k^3][cout][cin] (the slab layout), or (dw, S, D) with
    a_delta: D = the weight gradient of (a_delta, |dy|)."""
    cin, cout = a.shape[-1], dy.shape[-1]
    shape = (cout, cin, k, k, k)
    p = k // 2

    def wg(aa, gg):
        g = torch.nn.grad.conv3d_weight(cl(aa), shape, cl(gg), stride=stride, padding=p)
        return g.reshape(cout, cin, k ** 3).permute(2, 0, 1)
    out = (wg(a, dy), wg(a.abs(), dy.abs()))
    return out if a_delta is None else out + (wg(a_delta, dy.abs()),)


def _spacing(v, dt):
    """(spacing of dt's grid at |v|, whether |v| is a power of two), fp64; spacing 0 at 0."""
    bits = 8 if dt == BF else 24
    m, e = torch.frexp(v.abs())                                     # |v| = m 2^e, m in [0.5, 1)
    sp = torch.where(v != 0, torch.pow(2.0, (e - bits).double()), torch.zeros_like(v))
    return sp, m == 0.5


def prologue_ref(x, stats, gamma, beta, G, dt):
    """x [n,...,c] (any float dtype; taken as x.to(dt)), stats [n,G,2] fp32 (mean, rstd), gamma / beta [c] fp32.
    Returns (a, mask, delta): a = relu(gn(x)) evaluated in fp64 and rounded to dt (fp64 tensor, x's shape), the
    ambiguity mask (bool; all False for fp32) and delta, the per-activation term of the module docstring (0 where
    the mask is clear in bf16)."""
    n, c = x.shape[0], x.shape[-1]
    xs = x.to(dt).double()
    g = torch.arange(c) // (c // G)
    st = stats.double().cpu()
    mean, rstd = st[:, g, 0], st[:, g, 1]                             # [n, c]
    sc = rstd * gamma.double().cpu()[None]
    sh = beta.double().cpu()[None] - mean * sc
    view = (n,) + (1,) * (x.dim() - 2) + (c,)
    xsc = xs * sc.view(view)
    pre = xsc + sh.view(view)
    v = pre.clamp_min(0)
    a = v.to(dt).double()
    E = U32 * (3 * xsc.abs() + (2 * (mean * sc).abs() + 2 * sh.abs()).view(view))
    if dt != BF:
        return a, torch.zeros_like(a, dtype=torch.bool), E + U32 * v
    sp, pow2 = _spacing(a, dt)
    # v rounds to a from [a - lo, a + sp / 2]; below a power of two the grid is twice as fine, so lo = sp / 4 there
    lo = torch.where(pow2, sp / 4, sp / 2)
    dist = torch.minimum((v - (a - lo)).abs(), (v - (a + sp / 2)).abs())
    win = torch.maximum(2.0 ** -12 * sp, E)
    mask = ((dist <= win) & (v > 0)) | (pre.abs() <= torch.maximum(torch.full_like(E, 2.0 ** -20), E))
    delta = torch.where(mask, torch.maximum(sp, _spacing(v + E, dt)[0]) + 2 * E, torch.zeros_like(E))
    return a, mask, delta


def bound_store(ref, dt):
    """The final rounding of a stored value: 2^-8 |ref| in bf16, nothing more than the chain's last rounding in fp32."""
    return 2.0 ** -8 * ref.abs() if dt == BF else torch.zeros_like(ref)


def bound_accum(S, L):
    """L fp32 additions on the longest chain over terms whose absolute values sum to S."""
    return (L + 1) * U32 * S
