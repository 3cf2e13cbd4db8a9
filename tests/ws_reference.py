"""fp64 restatements of the weight path every trunk conv takes once per step: weight standardisation (unet3D.py:21-26),
the packs the implicit-GEMM kernels read, the standardisation backward in closed form, and one step of torch.optim.SGD.
They are the independent references of test_gpu_wstd.py and of the step-wise checks of test_gpu_optim.py, and are
themselves pinned to oracle.ref_cpu.ws_weight, torch's autograd and torch.optim.SGD by test_ws_reference.py.

All of them take the fp32 operands as they are stored and compute in fp64.

    mean_r = sum_i w_ri / K        c = w - mean        sd_r = sqrt(sum_i c_ri^2 / (K - 1) + 1e-12)        W^ = c / sd
    F1_r = sum_i G_ri / K          F2_r = sum_i G_ri W^_ri / (K - 1)
    dW = (G - F1 - W^ * F2) / sd                       (autograd of sum(W^ * G) through mean and sd)
"""
from collections import namedtuple

import numpy as np
import torch

U = 2.0 ** -24  # unit roundoff of fp32

# (cout, cin, k, standardise), each for the branch of csrc/wprep.hip / csrc/wstd.hip it enters
SHAPES = [(32, 1, 3, True),     # stem: K = 27, scalar stats and stage, cin = 1
          (16, 3, 3, True),     # cin % 4 != 0, K = 81
          (24, 40, 3, True),    # cout no multiple of 16; second ci tile with 8 valid columns; 256 % 40 != 0: gather branch
          (48, 32, 3, True),    # cout_p = 64: a half-empty tile row
          (32, 32, 3, True),    # row kernel, 4 elements per thread
          (32, 64, 3, True),    # 8
          (32, 128, 3, True),   # 16
          (64, 256, 3, True),   # 28; K = 6912, the longest row on the vector stats path
          (40, 320, 3, True),   # 56; K = 8640: stats by the scalar walk because of length
          (8, 544, 3, True),    # K = 14688 > 56 * 256: the chunked kernel by routing, not by option
          (64, 64, 1, True),    # k = 1, standardised
          (8, 32, 1, False),    # k = 1, unstandardised head
          (2, 8, 1, False)]     # k = 1, unstandardised head
LONG = (8, 544, 3, True)
ROW_MAX_K = 56 * 256            # longest row of wstd_grad_row_kernel

WsBwdRef = namedtuple("WsBwdRef", "dw F1 F2 A1 A2")


def round32(c):
    return (c + 31) // 32 * 32


def ws_ref(w):
    """W^ (w's shape), per-row mean and per-row sd (each [cout]) of the stored values of w, in fp64."""
    wd = w.double()
    rows = wd.reshape(w.shape[0], -1)
    K = rows.shape[1]
    mean = rows.sum(1) / K
    c = rows - mean[:, None]
    sd = torch.sqrt((c * c).sum(1) / max(K - 1, 1) + 1e-12)
    return (c / sd[:, None]).reshape(w.shape), mean, sd


def pack_fwd(wh, pad=0.0):
    """[cout, cin, k, k, k] -> the forward pack [k^3][cout_p][cin_p], pf[t, co, ci] = wh[co, ci, t]; cout_p and cin_p
    round up to 32 and the padding holds ``pad``. This is the layout of a weight-gradient slab too."""
    cout, cin = wh.shape[:2]
    k3 = wh[0, 0].numel()
    out = torch.full((k3, round32(cout), round32(cin)), pad, dtype=wh.dtype)
    out[:, :cout, :cin] = wh.reshape(cout, cin, k3).permute(2, 0, 1)
    return out


def pack_dgrad(wh, pad=0.0):
    """The data-gradient pack [k^3][cin_p][cout_p]: the (0, 2, 1) transpose of the forward pack."""
    return pack_fwd(wh, pad).permute(0, 2, 1).contiguous()


def unpack(pf, shape):
    """A forward pack / slab [k^3][cout_p][cin_p] back in parameter order [cout, cin, k, k, k] (padding dropped)."""
    cout, cin = shape[:2]
    return pf[:, :cout, :cin].permute(1, 2, 0).reshape(shape).contiguous()


def ws_bwd_ref(w, G, standardise=True):
    """dW for the upstream gradient G (fp64, parameter order: the sum of the slabs), and the per-row quantities
    ([cout, 1, 1, 1, 1]) the error bounds need: F1 = mean(G), F2 = sum(G W^) / (K - 1), A1 = sum|G|, A2 = sum|G W^|.
    Without standardisation dW = G and F1 = F2 = 0."""
    G = G.double()
    cout = w.shape[0]
    K = w[0].numel()
    col = (cout,) + (1,) * (w.dim() - 1)
    rows = G.reshape(cout, -1)
    A1 = rows.abs().sum(1).reshape(col)
    if not standardise:
        z = torch.zeros(col, dtype=torch.float64)
        return WsBwdRef(G.clone(), z, z, A1, (rows * w.double().reshape(cout, -1)).abs().sum(1).reshape(col))
    wh, _, sd = ws_ref(w)
    gw = rows * wh.reshape(cout, -1)
    F1 = (rows.sum(1) / K).reshape(col)
    F2 = (gw.sum(1) / max(K - 1, 1)).reshape(col)
    dw = (G - F1 - wh * F2) / sd.reshape(col)
    return WsBwdRef(dw, F1, F2, A1, gw.abs().sum(1).reshape(col))


def f32(x):
    """The fp32 value a C float argument carries, as a Python float."""
    return float(np.float32(x))


def sgd_ref(p, g, buf, lr, momentum=0.0, dampening=0.0, wd=0.0, nesterov=False, maximize=False, init=False):
    """One step of torch.optim.SGD's rule in fp64 on the stored values of p, g and buf, with the hyper-parameters as the
    fp32 values the kernel is handed (1 - dampening formed in fp32, as the kernel forms it). ``init``: the first step
    of a parameter, where the momentum buffer becomes d_p itself. Returns (p', buf'); buf' is None without momentum."""
    lr, momentum, wd = f32(lr), f32(momentum), f32(wd)
    omd = float(np.float32(1.0) - np.float32(dampening))
    p, g = p.double(), g.double()
    if maximize:
        g = -g
    d = g + wd * p if wd != 0.0 else g
    b = None
    if momentum != 0.0:
        b = d.clone() if init else momentum * buf.double() + omd * d
        d = d + momentum * b if nesterov else b
    return p - lr * d, b
