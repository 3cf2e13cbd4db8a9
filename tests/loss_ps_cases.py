"""Cases, inputs and rounding bounds of the per-sample supervision loss kernels (csrc/loss_ps.hip), shared by
test_loss_ps_reference.py (CPU) and test_gpu_loss_ps.py. The derivation of the bounds is in test_gpu_loss_ps.py's
docstring. Inputs, the probability error model (p_err) and the backward's bound (loss_bwd_bounds) are loss_cases'.
"""
import functools
import math

import torch

import loss_cases as K
import loss_reference as R
from loss_cases import IDENT, SIG, SOFT, U

# the kernels' constants (csrc/loss_ps.hip): a change of one shows which case has to move
PT = 256                      # threads per block; voxels per block and trip of every kernel but the lane-pair forward
PS_FWD_NB = 512               # blocks of loss_ps_partial_kernel over all samples at most
PS_PAIR_NB, PAIR_VOX = 1280, 128   # the same for loss_ps_partial16_pair_kernel; its voxels per block and trip
PS_BWD_NB = 1024              # blocks of loss_ps_bwd_kernel over all samples at most
PS_CMAX = 32
PS_MAXS = 65535
U64 = 2.0 ** -53
F64 = torch.float64

MODES = [(SOFT, 0), (SOFT, 1), (SIG, 0), (SIG, 1), (IDENT, 0), (IDENT, 1)]
CLASSES = K.CLASSES                                   # 2, 5, 8, 14, 16, 32
SMALL_SV = [(1, 1), (2, 5), (3, 255), (3, 256), (3, 257), (2, 693)]
KINDS = ["mixed", "zero_row", "all_zero", "disjoint", "equal"]
# a CT row of the AMOS supervision table (one organ annotated) and an MRI row (nothing annotated)
CT_ROW = [0, 0, 0, 1, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0]
MRI_ROW = [0] * 15


def blocks(S, V, budget, vox):
    """Blocks per sample (ps_blocks): the budget shared by the samples, at least one, no more than V needs."""
    return max(1, min(budget // S, -(-V // vox)))


def is_pair(C, mode, uce):
    return C == 16 and mode == SOFT and uce == 1


def fwd_blocks(S, V, C, mode, uce):
    return blocks(S, V, PS_PAIR_NB, PAIR_VOX) if is_pair(C, mode, uce) else blocks(S, V, PS_FWD_NB, PT)


def workspace_bytes(S, V, C):
    nb = max(blocks(S, V, PS_FWD_NB, PT), blocks(S, V, PS_PAIR_NB, PAIR_VOX) if C == 16 else 0)
    return S * nb * 4 * C * 4


# one trip of the grid covers, per sample, blocks * voxels per block; the multi-trip cases exceed that by 300
S_MULTI = 2
FWD_MULTI_V = (PS_FWD_NB // S_MULTI) * PT + 300            # generic forward (C = 5): a second trip for 300 voxels
FWD_MULTI_PAIR_V = (PS_PAIR_NB // S_MULTI) * PAIR_VOX + 300   # lane-pair forward (C = 16, softmax, uce 1)
BWD_MULTI_V = (PS_BWD_NB // S_MULTI) * PT + 300
# (S, V, C, mode, uce, kind[, dtype])
FWD_MULTI = [(S_MULTI, FWD_MULTI_V, 5, SOFT, 1, "mixed"), (S_MULTI, FWD_MULTI_PAIR_V, 16, SOFT, 1, "mixed")]
BWD_MULTI = [(S_MULTI, BWD_MULTI_V, 16, SOFT, 1, "mixed", torch.float32),     # the pipelined path
             (S_MULTI, BWD_MULTI_V, 2, SIG, 1, "mixed", torch.bfloat16)]     # the generic loop


def kinds_for(S, V):
    """Every mask kind where there is more than one sample and at the sizes around a block; 'mixed' everywhere."""
    return KINDS if (S, V) in ((3, 257), (2, 693)) else ["mixed"]


def case_id(case):
    return K.case_id(case)


def make_weights(kind, S, C, seed=0):
    """[S, C] fp32 on the CPU. mixed: rows differ, values in [0.5, 1.5] with zeros (every sample keeps a class, a
    class is left to nobody when C > 3); zero_row: mixed with sample S - 1 all zero; all_zero; disjoint: class c
    supervised by sample c % S alone; equal: one mixed row for every sample."""
    gen = torch.Generator().manual_seed(4242 + 131 * S + 7 * C + seed)
    w = 0.5 + torch.rand(S, C, generator=gen)
    if kind == "all_zero":
        return torch.zeros(S, C)
    if kind == "disjoint":
        own = (torch.arange(C)[None, :] % S) == torch.arange(S)[:, None]
        return w * own
    if kind == "equal":
        row = w[0].clone()
        row[1::3] = 0.0
        return row[None, :].expand(S, C).contiguous()
    for s in range(S):
        w[s, (s + 1)::3] = 0.0
    if C > 3:
        w[:, 3] = 0.0                       # a class nobody supervises: n_c = 0
    if kind == "zero_row":
        w[S - 1] = 0.0
    return w


@functools.lru_cache(maxsize=8)
def ps_inputs(case):
    """loss_cases.loss_inputs' logits and labels (regular regime, special labels included) reshaped to [S, V, C] and
    [S, V], with the [S, C] weights of the case's kind."""
    S, V, C, mode, uce, kind = case[:6]
    lg, lab, _ = K.loss_inputs((S, V, C, mode, uce, "reg"))
    return lg.reshape(S, V, C), lab.reshape(S, V), make_weights(kind, S, C)


def depth(V, nbx, vox):
    """fp32 additions one sum goes through: the thread's trips, 6 wave levels (5 in the lane-pair kernel), 4 waves."""
    return math.ceil(V / (nbx * vox)) + 10


def sample_sum_bounds(ref, s, S, V, mode, uce, D):
    """Bounds of sums_ps[s] [C, 4] (loss_cases.loss_fwd_bounds' sums, for one sample's voxels and depth D)."""
    C = ref.sums_ps.shape[1]
    ep, ee, es = K.p_err(ref, mode, C)
    sl = slice(s * V, (s + 1) * V)
    pr, hit = ref.pr, ref.hit[sl]
    p = pr.p[sl]
    ep_s = ep[sl]
    I, Z, Y, B = ref.sums_ps[s].unbind(1)
    dI = D * U * I + (p * hit * ep_s).sum(0)
    dZ = D * U * Z + (2 * p * p * ep_s).sum(0)
    dY = torch.zeros_like(Y)
    dB = torch.zeros_like(B)
    if uce == 1:
        logp, logq = pr.logp[sl], pr.logq[sl]
        if mode == SOFT:
            x, lns, es_s, ee_s = pr.x[sl], torch.log(pr.s[sl]), es[sl], ee[sl]
            dls = 4 * U * lns + es_s
            e_hit = U * x.abs() + dls + U * logp.abs()
            q = pr.q[sl].clamp(min=1e-300)
            e_non = (es_s + p * ee_s) / q + U + 4 * U * (logq + lns).abs() + dls + U * logq.abs()
        else:
            e_hit = ep_s + 2 * U * logp.abs()
            e_non = ep_s * p / pr.q[sl].clamp(min=1e-300) + 4 * U * logq.abs()
        bce = ref.bce[sl]
        el = torch.where(bce == 100.0, torch.zeros_like(p), torch.where(hit, e_hit, e_non))
        dB = D * U * ref.bce_abs_ps[s] + el.sum(0)
    return torch.stack([dI, dZ, dY, dB], 1)


def fwd_bounds(ref, S, V, mode, uce, nbx, vox):
    """(bounds of sums_ps [S, C, 4], of pooled[:, :4] [C, 4], of the loss)."""
    C = ref.sums_ps.shape[1]
    D = depth(V, nbx, vox)
    bs = torch.stack([sample_sum_bounds(ref, s, S, V, mode, uce, D) for s in range(S)])
    X = ref.pooled[:, :4]
    bp = (ref.m[:, :, None] * bs).sum(0) + S * U64 * X.abs()          # S fp64 adds on top of the samples' errors
    I, Z, Y, B = X.unbind(1)
    dI, dZ, dY, dB = bp.unbind(1)
    num, den = 2 * I + R.SMOOTH, Z + Y + R.SMOOTH
    ratio = num / den
    dd = 2 * dI / den + ratio * (dZ + dY) / den + U * ratio + U * ref.d.abs()
    what = ref.what.abs()
    rw = (S + 2) * U64                                                 # w^_c: S fp64 adds and a division
    bl = (what * (dd + rw * ref.d.abs())).sum() / C
    if uce == 1:
        nV = ref.n.clamp(min=1) * V
        on = (ref.n > 0).double()
        bl = bl + (on * what * (dB + (U + rw + 2 * U64) * B.abs()) / nV).sum()   # 1 / (n_c V): a product, a division
    bl = bl + U * ref.loss.abs()
    return bs, bp, bl


def bwd_bounds(ref, mode, uce, S, out_bf16=False, dpooled=None):
    """Bound of dl [S V, C]: loss_cases.loss_bwd_bounds on the per-voxel coefficient tables (a, b, kb are formed in
    fp64 and rounded once to fp32, as in loss.hip), plus the fp64 roundings of w^_c and 1 / (n_c V), which sit far
    below u: (S + 6) 2^-53 of every term."""
    br = K.loss_bwd_bounds(ref, mode, uce, out_bf16=out_bf16, dsums=dpooled)
    return br + (S + 6) * U64 * K.grad_magnitude(ref, mode)
