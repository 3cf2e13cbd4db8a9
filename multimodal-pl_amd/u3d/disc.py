"""Style discriminators on the native 4^3 / stride-2 conv + LeakyReLU kernels (csrc/disc.hip).

Reference unet3D.py:1832-1849 (get_style_discriminator_output), :1852-1905 (deep_style_discriminator_output) and
:1907-1947 (norm_style_discriminator_output), driven by train_amos_atlas_final.py:320-379: two forwards (generator
pass with frozen parameters, discriminator pass with detached inputs) are alive before either backward, so every
activation a backward needs is a tensor owned by its call; only split-K / slab workspaces (consumed inside one call,
in stream order) are shared.

The conv chain is one autograd Function whose inputs include the parameters: parameter gradients come back as
returned gradients, so .grad accumulation, zero_grad and torch.optim.Adam work untouched. It returns the last conv's
NDHWC fp32 activation; AdaptiveAvgPool3d(1) + Reshape + Linear (a few voxels per sample) stay torch device ops.
"""
import weakref

import torch

from . import ops
from ._lib import U3DError, call, query
from .ops import WS, _ptr, _stream, dt_code
from .trunk import compute_dtype

SLOPE = 0.2
MAX_CLASSES = 4

# ------------------------------------------------------------------------------------------ weight packs
_PACKS = {}  # (kind, data_ptr, shape, dtype) -> ((autograd version, WEIGHT_GEN), weakref of the parameter, pack)
PACK_STATS = {"hit": 0, "miss": 0}


def _cached(kind, w, dtype, make):
    """Pack of parameter ``w``, reused while the parameter is unchanged: keyed as the trunk's no_grad pack cache is
    (ops._pack_key), by pointer and autograd version, so the optimizer's in-place step invalidates it. The entry also
    remembers which tensor it was made from: another parameter that later lands on the same address is a miss."""
    key = (kind, w.data_ptr(), tuple(w.shape), dtype)
    stamp = (w._version, ops.WEIGHT_GEN[0])
    hit = _PACKS.get(key)
    if hit is not None and hit[0] == stamp and hit[1]() is w:
        PACK_STATS["hit"] += 1
        return hit[2]
    PACK_STATS["miss"] += 1
    for k in [k for k, v in _PACKS.items() if v[1]() is None]:  # packs of parameters that are gone
        del _PACKS[k]
    with torch.no_grad():
        pk = make(w.detach())
    _PACKS[key] = (stamp, weakref.ref(w), pk)
    return pk


def pack_conv_fwd(w, dtype):
    """[cout][cin][4][4][4] fp32 -> [64][cin / 8][cout][8] (the forward's B operand: 8 consecutive ci per lane)."""
    cout, cin = w.shape[0], w.shape[1]
    return w.reshape(cout, cin // 8, 8, 64).permute(3, 1, 0, 2).contiguous().to(dtype)


def pack_conv_dgrad(w, dtype):
    """[cout][cin][4][4][4] fp32 -> [64][cout / 8][cin][8] (the data gradient's B operand: 8 consecutive co)."""
    cout, cin = w.shape[0], w.shape[1]
    return w.reshape(cout // 8, 8, cin, 64).permute(3, 0, 2, 1).contiguous().to(dtype)


def pack_first(w):
    """[cout][C][4][4][4] fp32 -> fp32 [64][C][cout]."""
    cout, c = w.shape[0], w.shape[1]
    return w.reshape(cout, c, 64).permute(2, 1, 0).contiguous()


def pack_side(w):
    """[C][1][3][3][3] fp32 -> fp32 [27][C]."""
    return w.reshape(w.shape[0], 27).t().contiguous()


# ------------------------------------------------------------------------------------------ kernels
class View:
    """Channels [off, off + c) of an NDHWC tensor [n, d, h, w, pitch]."""

    def __init__(self, t, off, c):
        self.t, self.off, self.c = t, off, c
        self.pitch = t.shape[4]

    @property
    def dims(self):
        return tuple(self.t.shape[1:4])

    @property
    def n(self):
        return self.t.shape[0]

    def args(self):
        return (_ptr(self.t), self.pitch, self.off)


def _ws(nbytes, device):
    return WS.get(max(int(nbytes), 256), device, ops.Slot.DISC)


def conv_fwd(x, wpk, bias, y):
    n, (d, h, w) = x.n, x.dims
    dt = dt_code(x.t.dtype)
    splits = query("u3d_disc_conv_fwd_splits", n, d, h, w, x.c, y.c)
    ws = _ws(query("u3d_disc_conv_fwd_ws_bytes", n, d, h, w, y.c, splits), x.t.device) if splits > 1 else None
    call("u3d_disc_conv_fwd", dt, *x.args(), n, d, h, w, x.c, _ptr(wpk), _ptr(bias), *y.args(), y.c, splits, _ptr(ws),
         _stream())


def conv_dgrad(dy, y, wpk, dx):
    n, (d, h, w) = dx.n, dx.dims
    call("u3d_disc_conv_dgrad", dt_code(dx.t.dtype), *dy.args(), *y.args(), n, d, h, w, dx.c, y.c, _ptr(wpk), *dx.args(),
         _stream())


def conv_wgrad(x, dy, y, dw):
    n, (d, h, w) = x.n, x.dims
    splits = query("u3d_disc_conv_wgrad_splits", n, d, h, w, x.c, y.c)
    ws = _ws(query("u3d_disc_conv_wgrad_ws_bytes", x.c, y.c, splits), x.t.device)
    call("u3d_disc_conv_wgrad", dt_code(x.t.dtype), *x.args(), *dy.args(), *y.args(), n, d, h, w, x.c, y.c, splits,
         _ptr(ws), _ptr(dw), _stream())


def bias_grad(dy, y, db):
    m = y.n * y.dims[0] * y.dims[1] * y.dims[2]
    ws = _ws(query("u3d_disc_bias_grad_ws_bytes", m, y.c), y.t.device)
    call("u3d_disc_bias_grad", dt_code(y.t.dtype), *dy.args(), *y.args(), m, y.c, _ptr(ws), _ptr(db), _stream())


def first_fwd(x, w1, bias, y):
    n, c, d, h, w = x.shape
    call("u3d_disc_first_fwd", dt_code(y.t.dtype), _ptr(x), n, c, d, h, w, _ptr(w1), _ptr(bias), *y.args(), y.c,
         _stream())


def first_dgrad(dy, y, w1, dx):
    n, c, d, h, w = dx.shape
    call("u3d_disc_first_dgrad", dt_code(y.t.dtype), *dy.args(), *y.args(), n, c, d, h, w, y.c, _ptr(w1), _ptr(dx),
         _stream())


def first_wgrad(x, dy, y, dw):
    n, c, d, h, w = x.shape
    ws = _ws(query("u3d_disc_first_wgrad_ws_bytes", n, d, h, w, c, y.c), x.device)
    call("u3d_disc_first_wgrad", dt_code(y.t.dtype), _ptr(x), *dy.args(), *y.args(), n, c, d, h, w, y.c, _ptr(ws),
         _ptr(dw), _stream())


def side_fwd(f, wsd, bias, y):
    n, _, d, h, w = f.shape
    call("u3d_disc_side_fwd", dt_code(y.t.dtype), _ptr(f), n, d, h, w, _ptr(wsd), _ptr(bias), *y.args(), y.c, _stream())


def side_dgrad(dy, y, wsd, df):
    n, _, d, h, w = df.shape
    call("u3d_disc_side_dgrad", dt_code(y.t.dtype), *dy.args(), *y.args(), n, d, h, w, y.c, _ptr(wsd), _ptr(df),
         _stream())


def side_wgrad(f, dy, y, dw):
    n, _, d, h, w = f.shape
    ws = _ws(query("u3d_disc_side_wgrad_ws_bytes", n, d, h, w, y.c), f.device)
    call("u3d_disc_side_wgrad", dt_code(y.t.dtype), _ptr(f), *dy.args(), *y.args(), n, d, h, w, y.c, _ptr(ws), _ptr(dw),
         _stream())


# ------------------------------------------------------------------------------------------ the conv chain
def chain_dims(dims, layers=6):
    """Spatial dims after each of the stride-2 convs: out = floor(n / 2), every input dim >= 2."""
    out = []
    for i in range(layers):
        if min(dims) < 2:
            raise U3DError(f"u3d: discriminator input too small: conv {i + 1} of {layers} would see {tuple(dims)}; every "
                           f"spatial dim must be >= {2 ** layers} (out = floor(n / 2), n >= 2 at every layer)")
        dims = tuple(v // 2 for v in dims)
        out.append(dims)
    return out


def check_config(num_classes, ndf):
    if not (isinstance(ndf, int) and ndf > 0 and ndf % 32 == 0):
        raise U3DError(f"u3d: discriminator ndf must be a positive multiple of 32 (got {ndf})")
    if not (isinstance(num_classes, int) and 1 <= num_classes <= MAX_CLASSES):
        raise U3DError(f"u3d: discriminator num_classes must be in 1..{MAX_CLASSES} (got {num_classes})")


class _ChainFn(torch.autograd.Function):
    """x_in [B, C, D, H, W] (+ the three side maps) -> the sixth conv's activation, fp32 NDHWC [B, d, h, w, 8 ndf].
    params: (w, b) of the six convs, then (w, b) of min_block1..3 when deep."""

    @staticmethod
    def forward(ctx, deep, dtype, x_in, f1, f2, f3, *params):
        # f1 / f2 / f3: the maps at block1 / block2 / block3 output resolution (f_m[2], f_m[1], f_m[0])
        B = x_in.shape[0]
        dev = x_in.device
        convs = [(params[2 * i], params[2 * i + 1]) for i in range(6)]
        sides = [(params[12 + 2 * i], params[13 + 2 * i]) for i in range(3)] if deep else []
        fmaps = [f1, f2, f3] if deep else []
        dims = chain_dims(tuple(x_in.shape[2:]))
        couts = [w.shape[0] for w, _ in convs]
        ctx.deep, ctx.dtype, ctx.empty = deep, dtype, B == 0
        ctx.x_in, ctx.fmaps, ctx.convs, ctx.sides = x_in, fmaps, convs, sides
        # the backward reads the inputs and repacks the weights: what autograd's saved-tensor check would guard
        ctx.versions = [t._version for t in (x_in, *fmaps, *params)]
        if B == 0:  # an empty flist: nothing to launch
            ctx.out_shape = (0, *dims[5], couts[5])
            return torch.empty(ctx.out_shape, dtype=torch.float32, device=dev)
        # buffers: layer i's output is channels [0, cout_i) of bufs[i]; a side conv fills the upper half
        bufs, ys = [], []
        for i in range(6):
            pitch = couts[i] * 2 if (deep and i < 3) else couts[i]
            bufs.append(torch.empty((B, *dims[i], pitch), dtype=dtype, device=dev))
            ys.append(View(bufs[i], 0, couts[i]))
        w1 = _cached("first", convs[0][0], torch.float32, pack_first)
        first_fwd(x_in, w1, convs[0][1], ys[0])
        xin = []  # the input view of conv i (i >= 1)
        for i in range(1, 6):
            if deep and i <= 3:
                c = couts[i - 1]
                wsd = _cached("side", sides[i - 1][0], torch.float32, pack_side)
                side_fwd(fmaps[i - 1], wsd, sides[i - 1][1], View(bufs[i - 1], c, c))
                xv = View(bufs[i - 1], 0, 2 * c)
            else:
                xv = ys[i - 1]
            xin.append(xv)
            wpk = _cached("fwd", convs[i][0], dtype, lambda w: pack_conv_fwd(w, dtype))
            conv_fwd(xv, wpk, convs[i][1], ys[i])
        ctx.bufs, ctx.ys, ctx.xin = bufs, ys, xin
        return bufs[5].float() if dtype != torch.float32 else bufs[5].clone()

    @staticmethod
    def backward(ctx, g):
        deep, dtype = ctx.deep, ctx.dtype
        convs, sides, fmaps, x_in = ctx.convs, ctx.sides, ctx.fmaps, ctx.x_in
        live = (x_in, *fmaps, *[t for wb in convs for t in wb], *[t for wb in sides for t in wb])
        for k, (t, v) in enumerate(zip(live, ctx.versions)):
            if t._version != v:
                raise RuntimeError("u3d: a tensor needed by the discriminator's backward (input or parameter "
                                   f"{k} of the conv chain) was modified in place after the forward: it is at "
                                   f"version {t._version}, expected {v}. Run the backward before the optimizer step")
        need = ctx.needs_input_grad
        need_x = need[2]
        need_f = [need[3 + i] for i in range(3)] if deep else [False] * 3
        need_p = need[6:]
        grads = [None] * len(need_p)
        if ctx.empty:
            gx = torch.zeros_like(x_in) if need_x else None
            gf = [torch.zeros_like(fmaps[i]) if need_f[i] else None for i in range(3)] if deep else [None] * 3
            for k, p in enumerate(list(sum(convs, ())) + list(sum(sides, ()))):
                if need_p[k]:
                    grads[k] = torch.zeros_like(p)
            return (None, None, gx, *gf, *grads)
        bufs, ys, xin = ctx.bufs, ctx.ys, ctx.xin
        dev = x_in.device
        g = g.to(dtype).contiguous()
        dy = View(g, 0, g.shape[4])
        gf = [None] * 3
        gx = None
        for i in range(5, 0, -1):
            w, b = convs[i]
            y, xv = ys[i], xin[i - 1]
            if need_p[2 * i]:
                grads[2 * i] = torch.empty_like(w)
                conv_wgrad(xv, dy, y, grads[2 * i])
            if need_p[2 * i + 1]:
                grads[2 * i + 1] = torch.empty_like(b)
                bias_grad(dy, y, grads[2 * i + 1])
            side = deep and i <= 3
            side_need = side and (need_f[i - 1] or need_p[12 + 2 * (i - 1)] or need_p[13 + 2 * (i - 1)])
            # the gradient is needed below this conv when anything under it wants one
            below = (need_x or any(need_p[:2 * i]) or any(need_f[:i - 1])
                     or (deep and any(need_p[12:12 + 2 * min(i - 1, 3)])))
            if not (below or side_need):
                return (None, None, gx, *gf, *grads)
            dxt = torch.empty_like(xv.t)
            conv_dgrad(dy, y, _cached("dgrad", w, dtype, lambda t: pack_conv_dgrad(t, dtype)), View(dxt, 0, xv.c))
            if side:
                c = ys[i - 1].c
                sy, sdy = View(bufs[i - 1], c, c), View(dxt, c, c)
                sw, sb = sides[i - 1]
                k = 12 + 2 * (i - 1)
                if need_p[k]:
                    grads[k] = torch.empty_like(sw)
                    side_wgrad(fmaps[i - 1], sdy, sy, grads[k])
                if need_p[k + 1]:
                    grads[k + 1] = torch.empty_like(sb)
                    bias_grad(sdy, sy, grads[k + 1])
                if need_f[i - 1]:
                    gf[i - 1] = torch.empty_like(fmaps[i - 1])
                    side_dgrad(sdy, sy, _cached("side", sw, torch.float32, pack_side), gf[i - 1])
            dy = View(dxt, 0, ys[i - 1].c)
        w, b = convs[0]
        if need_p[0]:
            grads[0] = torch.empty_like(w)
            first_wgrad(x_in, dy, ys[0], grads[0])
        if need_p[1]:
            grads[1] = torch.empty_like(b)
            bias_grad(dy, ys[0], grads[1])
        if need_x:
            gx = torch.empty_like(x_in)
            first_dgrad(dy, ys[0], _cached("first", w, torch.float32, pack_first), gx)
        return (None, None, gx, *gf, *grads)


def _prep(t):
    ops.require_device(t)
    if t.dtype != torch.float32 or not t.is_contiguous():
        t = t.float().contiguous()
    return t


def run_chain(x_in, f_m, conv_params, side_params, num_classes, ndf, dtype=None):
    """The six convs (+ the three side convs when ``f_m`` is given) -> fp32 NDHWC [B, d, h, w, 8 ndf].
    conv_params / side_params: [(weight, bias)] in layer order (side: min_block1, 2, 3)."""
    check_config(num_classes, ndf)
    dtype = compute_dtype(dtype)
    if not isinstance(x_in, torch.Tensor) or x_in.dim() != 5:
        raise U3DError("u3d: discriminator input must be a [B, num_classes, D, H, W] tensor")
    if x_in.shape[1] != num_classes:
        raise U3DError(f"u3d: discriminator input has {x_in.shape[1]} channels, the module was built for {num_classes}")
    dims = chain_dims(tuple(x_in.shape[2:]))
    deep = f_m is not None
    fs = [None, None, None]
    if deep:
        if not isinstance(f_m, (list, tuple)) or len(f_m) != 3:
            raise U3DError("u3d: deep_style_discriminator_output needs f_m = [map at block3's, block2's, block1's "
                           "output resolution]")
        for i in range(3):  # fs[i] feeds min_block(i + 1)
            f = f_m[2 - i]
            want = (x_in.shape[0], 1, *dims[i])
            if not isinstance(f, torch.Tensor) or tuple(f.shape) != want:
                got = tuple(f.shape) if isinstance(f, torch.Tensor) else type(f).__name__
                raise U3DError(f"u3d: f_m[{2 - i}] must be {want} (block{i + 1}'s output resolution), got {got}")
            fs[i] = f
    x_in = _prep(x_in)
    fs = [None if f is None else _prep(f) for f in fs]
    params = [t for wb in conv_params for t in wb] + [t for wb in (side_params if deep else []) for t in wb]
    ops.require_device(*params)
    return _ChainFn.apply(deep, dtype, x_in, *fs, *params)


def pool_linear(feat, weight, bias):
    """AdaptiveAvgPool3d(1) + Reshape + Linear on the fp32 NDHWC activation (unet3D.py:1886-1888), in fp32."""
    with torch.autocast("cuda", enabled=False):
        pooled = feat.mean(dim=(1, 2, 3))
        return torch.nn.functional.linear(pooled, weight, bias)
