"""fp64 restatement of the backward of relu(group_norm(x)) on NDHWC tensors: the independent reference the GroupNorm
kernel tests (test_gpu_groupnorm.py) compare against, pinned to torch's autograd by test_gn_reference.py.

The statistics are operands: the helper takes the [n][G][2] (mean, rstd) tensor it is handed, so a backward test
does not fail for a rounding of the statistics (with mean 300 an fp32 mean alone moves dgamma by ~4e-5).

    pre = (x - mu) * rs * gamma + beta        m = pre > 0        g = m * dA        xhat = (x - mu) * rs
    dbeta_c = sum_{n,v} g                      dgamma_c = sum_{n,v} g * xhat
    per (n, group), M = v * cpg:   a = sum gamma_c g / M,   b = sum gamma_c g xhat / M
    dx = rs * (gamma * g - a - xhat * b)

The relu mask is discontinuous: wherever |pre| < TIE the helper zeroes dA (returned as ``da``; the tests feed THAT dA
to the kernel), so a kernel whose fp32 pre lands on the other side of zero computes the same sums and the same dx, and
no entry is left out of the comparison. ``share`` is the fraction so zeroed; the tests require it to stay <= MAX_SHARE.
"""
from collections import namedtuple

import torch

TIE = 1e-4
MAX_SHARE = 1e-3

# (n, c, dims, groups), each for a branch of the kernels (test_gn_reference.py checks the geometry claims)
SMALL = [(2, 32, (6, 8, 12), 16),    # two reduction blocks, the second ragged (bf16; fp32: three)
         (1, 24, (5, 7, 9), 8),      # 3 / 6 chunks per voxel: the serial branch of block_channel_reduce, 510 apply threads
         (1, 40, (3, 5, 7), 8),      # 5 / 10 chunks per voxel
         (8, 256, (2, 2, 3), 16),    # n * c == GN_PAIRS_MAX: four rounds of 512 pairs in the combine
         (3, 128, (5, 7, 9), 16),    # the general case
         (1, 8, (3, 5, 7), 8),       # one channel per group, one chunk per voxel in bf16
         (2, 256, (1, 1, 2), 16)]    # fewer voxels than voxel lanes
LARGE = (1, 32, (50, 66, 80), 16)       # ~230 blocks > 8 * spl = 128: a second latency round in combine_channels
LARGE_PAIR = (2, 32, (60, 62, 58), 16)  # n * v >= 409 600: gn_bwd2's apply takes 16 vectors per thread

GnBwdRef = namedtuple("GnBwdRef", "dx dgamma dbeta abs_dgamma abs_dbeta da share")


def per_channel(t, c):
    """[n, G] per-group values -> [n, 1, c] per channel (fp64)."""
    n, G = t.shape
    return t.double().repeat_interleave(c // G, dim=1).reshape(n, 1, c)


def zero_ties(pre, da):
    """da with zeros where |pre| < TIE (same dtype and shape as da), and the share of entries zeroed."""
    tie = pre.abs() < TIE
    return da.masked_fill(tie.reshape(da.shape), 0), tie.double().mean().item()


def gn_relu_bwd_ref(x, da, stats, gamma, beta, groups, sums=None):
    """x, da: [n, ..., c] (any float dtype: taken as the fp64 of the stored values); stats [n, G, 2]; gamma, beta [c].
    sums: optional (s1, s2), each [n, c] fp64: per-(n, channel) sums of g and g * xhat supplied by the caller instead
    of those of da and x (the kernels that finish the backward from another kernel's partial sums).
    Returns GnBwdRef: dx (fp64, x's shape), dgamma / dbeta [c], the sums of |terms| behind them, the tie-cleaned dA
    (da's dtype) and the share of entries zeroed."""
    n, c = x.shape[0], x.shape[-1]
    xs = x.double().reshape(n, -1, c)
    v = xs.shape[1]
    cpg = c // groups
    mu = per_channel(stats[..., 0], c)
    rs = per_channel(stats[..., 1], c)
    ga, be = gamma.double().reshape(1, 1, c), beta.double().reshape(1, 1, c)
    xhat = (xs - mu) * rs
    pre = xhat * ga + be
    da_clean, share = zero_ties(pre, da)
    g = torch.where(pre > 0, da_clean.double().reshape(n, -1, c), torch.zeros_like(pre))
    gx = g * xhat
    if sums is None:
        s1, s2 = g.sum(1), gx.sum(1)                                    # [n, c]
        abs1, abs2 = g.abs().sum((0, 1)), gx.abs().sum((0, 1))
    else:
        s1, s2 = sums[0].double(), sums[1].double()
        abs1 = abs2 = None
    M = float(v * cpg)
    a = (s1 * ga[0]).reshape(n, groups, cpg).sum(-1) / M               # [n, G]
    b = (s2 * ga[0]).reshape(n, groups, cpg).sum(-1) / M
    dx = rs * (ga * g - per_channel(a, c) - xhat * per_channel(b, c))
    return GnBwdRef(dx.reshape(x.shape), s2.sum(0), s1.sum(0), abs2, abs1, da_clean, share)


def reduce_geom(n, c, v, elsize, max_blocks=256):
    """The reduction geometry of csrc/groupnorm.hip (make_geom; GN_MAXBLK default 256) restated, so the tests can say
    which branch a shape takes: 16-byte chunks per voxel, voxel lanes of the 512-thread block, voxels per block and
    blocks per sample."""
    vec = 16 // elsize
    chn = c // vec
    vlanes = max(1, 512 // chn)
    nb = min(max_blocks, max(16, (v * n * c * elsize) >> 16))
    want = max(vlanes * 4, -(-v * n // nb))
    vpb = -(-want // vlanes) * vlanes
    return dict(chn=chn, vlanes=vlanes, vpb=vpb, nblk=-(-v // vpb))


def exact_stats(x, groups, eps=1e-5):
    """fp64 (mean, rstd) [n, G, 2] of the stored values of x ([n, ..., c]), and the per-group standard deviation."""
    n, c = x.shape[0], x.shape[-1]
    xg = x.double().reshape(n, -1, groups, c // groups).permute(0, 2, 1, 3).reshape(n, groups, -1)
    mean = xg.mean(-1)
    var = xg.var(-1, unbiased=False)
    return torch.stack([mean, (var + eps).rsqrt()], -1), var.sqrt()
