"""Cases, inputs and rounding bounds shared by test_loss_reference.py (which asserts the input conditions on the CPU)
and test_gpu_loss.py (which runs the kernels of csrc/loss.hip and csrc/consist.hip on them). The derivation of every
bound is in test_gpu_loss.py's docstring; the functions here are device-agnostic like loss_reference.py.
"""
import functools
import math

import torch

import loss_reference as R
from loss_reference import U

# the kernels' constants (csrc/loss.hip, csrc/consist.hip): a change of one shows which case has to move
LT = 256                 # threads per block, voxels per block of every kernel but the lane-pair forward
U3D_LOSS_NB = 512        # blocks of loss_partial_kernel at most
LP_NB, LP_VOX = 1280, 128   # blocks of loss_partial16_pair_kernel at most, voxels per block
BWD_NB = 8192            # blocks of loss_bwd_kernel at most
DICE_NB = 1024           # blocks per sample / organ of the two Dice count kernels at most
PT_NB = 4096             # blocks of partial_target_kernel at most
CS_BLOCKS = 128          # blocks per organ of consist_fwd_kernel, blocks of full2_fwd_kernel at most
CS_BWD_NB = 2048         # blocks of consist_bwd_kernel and full2_bwd_kernel at most
CS_MAPS = 4
SLACK = 1 + 2.0 ** -10
UB = 2.0 ** -8           # unit roundoff of a bf16 store
TIGHT = 2.0 ** -12       # regular-regime inputs keep every bound below this share of what it covers
F64 = torch.float64

SIG, SOFT, IDENT = R.MODE_SIGMOID, R.MODE_SOFTMAX, R.MODE_IDENTITY
MODES = [(SOFT, 0), (SOFT, 1), (SOFT, 2), (SIG, 0), (SIG, 1), (IDENT, 0), (IDENT, 1)]   # (softmax, uce) of u3d.h
CLASSES = [2, 5, 8, 14, 16, 32]          # 5 and 32: the guarded 32-wide fallback of U3D_NC_DISPATCH
SMALL_SV = [(1, 1), (1, 5), (1, 255), (1, 256), (1, 257), (2, 7 * 9 * 11)]   # (S, V); the last crosses a sample mid-block
FWD_MULTI = 2 * LP_NB * LP_VOX + 77      # 2-3 trips of the pair kernel, 2-3 of the generic one, with a tail
BWD_MULTI = BWD_NB * LT + 300            # a second trip for the first 300 voxels only
assert FWD_MULTI > 2 * U3D_LOSS_NB * LT and FWD_MULTI % LT and FWD_MULTI % LP_VOX

# (S, V, C, mode, uce, kind); kind: "reg", "zero_w" (all weights 0), "absent" (class C - 1 never a label, p ~ 1e-13)
LOSS_SMALL = [(s, v, c, m, u, "reg") for c in CLASSES for (m, u) in MODES for (s, v) in SMALL_SV]
LOSS_SPECIAL = [(2, 693, 16, SOFT, 1, "zero_w"), (1, 257, 5, SIG, 1, "zero_w"),
                (2, 693, 16, SOFT, 1, "absent"), (2, 693, 5, SOFT, 0, "absent")]
LOSS_FWD_MULTI = [(1, FWD_MULTI, 16, SOFT, 1, "reg"), (1, FWD_MULTI, 5, SOFT, 1, "reg")]
LOSS_BWD_MULTI = [(1, BWD_MULTI, 16, SOFT, 1, "reg", torch.float32),     # the pipelined path
                  (1, BWD_MULTI, 2, SOFT, 1, "reg", torch.bfloat16)]    # the generic loop
LOSS_SAT = [(1, 300, 2), (1, 300, 16)]   # (S, V, C): softmax + BCE, one class ahead by >= 40 everywhere
GRAD_OUT = 0.75


def case_id(case):
    return "-".join(str(a).replace("torch.", "") for a in case)


# ------------------------------------------------------------------------------------------------ partial loss inputs
@functools.lru_cache(maxsize=8)
def loss_inputs(case):
    """fp32 logits [nvox, C], labels [nvox], weights [C] on the CPU. Regular regime: logits randn * 2 plus a per-class
    offset in [-1, 1] (identity mode: their sigmoid, a probability); randn * 1 at C = 2, where the gap between the two
    logits is the whole story and randn * 2 put the gradient's bound at 1.2e-2 of what it covers (2^-12 is asked).
    Labels are class indices with, where the case is long enough, one label >= C, one negative and one non-integer;
    weights in [0.5, 1.5] with zeros."""
    S, V, C, mode, uce, kind = case[:6]
    nvox = S * V
    gen = torch.Generator().manual_seed(1000 * C + 10 * mode + uce + nvox % 997)
    off = torch.rand(C, generator=gen) * 2 - 1
    lg = torch.randn(nvox, C, generator=gen) * (1 if C == 2 else 2) + off
    hi = C - 1 if kind == "absent" else C
    lab = torch.randint(0, hi, (nvox,), generator=gen).float()
    if kind == "absent":
        lg[:, C - 1] -= 30.0
    if nvox >= 5:
        lab[1], lab[2], lab[3] = float(C + 1), -1.0, 0.5
    if mode == IDENT:
        lg = torch.sigmoid(lg)
    w = 0.5 + torch.rand(C, generator=gen)
    w[1::3] = 0.0
    if kind == "zero_w":
        w.zero_()
    return lg.contiguous(), lab, w


@functools.lru_cache(maxsize=None)
def sat_inputs(case):
    """Saturated softmax + BCE: in every voxel one class leads every other by 40..80, in hit and in non-hit positions
    (labels cycle over the classes and the specials); voxel 7's gap is above 110, where exp2 gives 0 and fp32 p == 0."""
    S, V, C = case
    nvox = S * V
    gen = torch.Generator().manual_seed(77 + C)
    lg = torch.randn(nvox, C, generator=gen)
    lead = torch.arange(nvox) % C
    lg[torch.arange(nvox), lead] += 45.0 + 30.0 * torch.rand(nvox, generator=gen)
    lg[7, lead[7]] += 80.0
    lab = ((torch.arange(nvox) // C) % (C + 1)).float()      # every (lead, label) pair, and label C (no class)
    lab[5] = 0.5
    w = 0.5 + torch.rand(C, generator=gen)
    return lg.contiguous(), lab, w, lead


# ------------------------------------------------------------------------------------------------ partial loss bounds
def p_err(ref, mode, C, round_p=False):
    """Relative error of the kernel's p [nvox, C] (ep), of its e = exp2 (ee) and of its s = sum e (es)."""
    if mode == SOFT:
        ee = (3 * ref.pr.x.abs() + 2) * U
        es = (C - 1) * U + (ref.pr.p * ee).sum(1, keepdim=True)
        ep = ee + es + 3 * U
    elif mode == SIG:
        ee = es = None
        ep = torch.full_like(ref.pr.p, 5 * U)
    else:
        ee = es = None
        ep = torch.zeros_like(ref.pr.p)
    if round_p:
        ep = ep + U
    return ep, ee, es


def fwd_depth(nvox, pair):
    nb = min(LP_NB, -(-nvox // LP_VOX)) if pair else min(U3D_LOSS_NB, -(-nvox // LT))
    return math.ceil(nvox / (nb * (LP_VOX if pair else LT))) + 10


def loss_fwd_bounds(ref, weights, mode, uce, nvox, pair=False, round_p=False):
    """Bounds of sums [C, 4] and of the loss for one forward; ref = partial_loss_ref's result."""
    C = ref.sums.shape[0]
    D = fwd_depth(nvox, pair)
    ep, ee, es = p_err(ref, mode, C, round_p)
    pr, hit = ref.pr, ref.hit
    p = pr.p
    I, Z, Y, B = ref.sums.unbind(1)
    dI = D * U * I + (p * hit * ep).sum(0)
    dZ = D * U * Z + (2 * p * p * ep).sum(0)
    dY = torch.zeros_like(Y)
    dB = torch.zeros_like(B)
    if uce:
        rp = U if round_p else 0.0
        if mode == SOFT:
            lns = torch.log(pr.s)
            dls = 4 * U * lns + es
            e_hit = U * pr.x.abs() + dls + U * pr.logp.abs() + rp
            if uce == 1:
                q = pr.q.clamp(min=1e-300)
                e_non = (es + p * ee) / q + U + 4 * U * (pr.logq + lns).abs() + dls + U * pr.logq.abs() + rp * p / q
        else:
            e_hit = ep + 2 * U * pr.logp.abs()
            e_non = ep * p / pr.q.clamp(min=1e-300) + 4 * U * pr.logq.abs()
        if uce == 1:
            clamped = ref.bce == 100.0          # both sides clamp: the cases keep every log well away from -100
            el = torch.where(clamped, torch.zeros_like(p), torch.where(hit, e_hit, e_non))
        else:
            el = torch.where(hit, e_hit, torch.zeros_like(p))
        dB = D * U * ref.bce_abs + el.sum(0)
    w = weights.double().to(p.device)
    num, den = 2 * I + R.SMOOTH, Z + Y + R.SMOOTH
    ratio = num / den
    dratio = 2 * dI / den + ratio * (dZ + dY) / den
    dd = dratio + U * ratio + U * ref.d.abs()
    bl = (w * dd).sum() / C
    if uce == 1:
        bl = bl + (w * (dB + U * B.abs()) / nvox).sum()
    elif uce == 2:
        bl = bl + dB.sum() / nvox
    bl = bl + U * ref.loss.abs()
    return torch.stack([dI, dZ, dY, dB], 1), bl, dict(den=den, num=num)


def loss_bwd_bounds(ref, mode, uce, out_bf16=False, round_p=False, dsums=None):
    """Bound of dl [nvox, C]. dsums [C, 4]: the error of the sums the kernel was fed (None: the reference's own)."""
    C = ref.sums.shape[0]
    ep, _, _ = p_err(ref, mode, C, round_p)
    p, q, t = ref.pr.p, ref.pr.q, ref.hit.double()
    a, b, kb = ref.a.abs(), ref.b.abs(), ref.kb.abs()
    ra = torch.full_like(a, U)
    rb = torch.full_like(b, U)
    if dsums is not None:
        I, Z, Y = ref.sums[:, 0], ref.sums[:, 1], ref.sums[:, 2]
        num, den = 2 * I + R.SMOOTH, Z + Y + R.SMOOTH
        dden = (dsums[:, 1] + dsums[:, 2]) / den
        ra = ra + dden
        rb = rb + 2 * dsums[:, 0] / num + 2 * dden
    dg = t * a * ra + p * b * (ep + rb + 2 * U) + U * ref.g1.abs()
    if uce == 1:
        qs = q.clamp(min=1e-300)
        qp = q * p
        open_ = (qp > 1e-12).double()                 # the clamp of (1 - p) p: below it the product's error is cut off
        pmt = (p - t).abs().clamp(min=1e-300)
        e2 = p * ep / pmt + open_ * (p * ep / qs + ep) + 8 * U
        dg = dg + ref.g2.abs() * e2 + U * ref.g.abs()
    if mode == SOFT:
        gp = (ref.g * p).abs()
        ddot = (dg * p + gp * ep).sum(1, keepdim=True) + C * U * ref.gp_abs
        br = ref.r0.abs() * (ep + 2 * U) + p * (dg + ddot)
    elif mode == SIG:
        br = dg * q * p + ref.r0.abs() * (p * ep / q.clamp(min=1e-300) + ep + 3 * U)
    else:
        br = dg
    if uce == 2:
        br = br + kb * (p * ep + U * (p - t).abs()) + 2 * U * ref.ce.abs() + U * ref.dl.abs()
    if out_bf16:
        br = br + UB * (ref.dl.abs() + br)
    return br


def grad_magnitude(ref, mode):
    """What a gradient element's bound is measured against in the regular regime: the abs-sum of its terms."""
    p = ref.pr.p
    if mode == SOFT:
        m = p * (ref.g.abs() + ref.gp_abs)
    elif mode == SIG:
        m = ref.g.abs() * ref.pr.q * p
    else:
        m = ref.g.abs()
    return m + (ref.ce.abs() if ref.ce is not None else 0)


# ------------------------------------------------------------------------------------------------ Dice metric
# (S, V, C, num_class); logits are multiples of 1/8 with deliberate ties
DICE_CASES = [(1, 1, 2, 1), (3, 255, 14, 13), (1, 257, 16, 13), (3, 257, 5, 4), (3, 257, 5, 2), (1, 257, 2, 1),
              (1, DICE_NB * LT + 300, 16, 15), (3, DICE_NB * LT + 300, 5, 3)]
DICE2_CASES = [(1, 1), (13, 255), (64, 257), (13, DICE_NB * LT + 300)]   # (nt, V)


@functools.lru_cache(maxsize=4)
def dice_inputs(case):
    S, V, C, ncls = case
    gen = torch.Generator().manual_seed(S + V + 31 * C + ncls)
    lg = torch.randint(-40, 41, (S, V, C), generator=gen).float() / 8
    tie = torch.arange(V) % 3 == 0                      # every third voxel: the first two maxima tie
    if C >= 3:
        top = lg.max(2, keepdim=True).values
        lg[:, tie, 2:3] = top[:, tie]
        lg[:, tie, 1:2] = torch.where(torch.arange(int(tie.sum()))[None, :, None] % 2 == 0, top[:, tie], lg[:, tie, 1:2])
    else:
        lg[:, tie, 1] = lg[:, tie, 0]
    lab = torch.randint(0, C, (S, V), generator=gen).float()
    if V >= 5:
        lab[:, 1], lab[:, 2], lab[:, 3] = float(ncls + 1), -1.0, 1.5
    return lg.contiguous(), lab


@functools.lru_cache(maxsize=4)
def dice2_inputs(case):
    """The refiner's output [nt, 2, V] (NCDHW-contiguous), multiples of 1/8 with ties, and one label volume [V]."""
    nt, V = case
    gen = torch.Generator().manual_seed(nt + V)
    ref = torch.randint(-40, 41, (nt, 2, V), generator=gen).float() / 8
    tie = torch.arange(V) % 4 == 0
    ref[:, 1, tie] = ref[:, 0, tie]
    lab = torch.randint(0, nt + 2, (V,), generator=gen).float()
    if V >= 5:
        lab[1], lab[2] = -1.0, 1.5
    return ref.contiguous(), lab


def metric_bound(metrics, S):
    """int -> float conversions (exact below 2^24, else one rounding each), a division, S adds and the division by S."""
    return (S + 5) * U * metrics.abs()


# ------------------------------------------------------------------------------------------------ partial target
# (S, V, M, mask_stride, lmin, lmax)
PT_CASES = [(3, 257, 14, 14, 1, 13), (3, 257, 14, 0, 1, 13), (2, 300, 9, 9, 1, 13), (1, 1, 14, 14, 1, 13),
            (3, 77, 16, 16, 2, 5), (3, (PT_NB * LT + 700) // 3, 14, 14, 1, 13)]


@functools.lru_cache(maxsize=4)
def pt_inputs(case):
    S, V, M, stride, lmin, lmax = case
    gen = torch.Generator().manual_seed(V + M + stride)
    lab = torch.randint(0, 16, (S, V), generator=gen).float()
    if V >= 5:
        lab[:, 1], lab[:, 2] = 3.5, -2.0
    rows = S if stride else 1
    mask = torch.randint(0, 2, (rows, M), generator=gen).long() * torch.randint(1, 4, (rows, M), generator=gen)
    for r in range(rows):
        mask[r, (r + 1) % M] = 0            # every row drops a label the others may keep
    return lab, mask.contiguous()


# ------------------------------------------------------------------------------------------------ consistency
CONFI, WF = 0.10, 0.1
CS_V2 = CS_BLOCKS * LT + 77
# (V, C, nt, natt, pattern); pattern: "mixed", "none" (all unsupervised), "all" (all supervised)
CONSIST_CASES = [(1, 3, 2, 3, "none"), (1, 3, 2, 0, "none"),
                 (300, 3, 2, 3, "mixed"), (300, 3, 2, 2, "mixed"), (300, 3, 2, 1, "none"), (300, 3, 2, 0, "mixed"),
                 (300, 14, 13, 3, "mixed"), (300, 14, 13, 2, "mixed"), (300, 14, 13, 1, "mixed"),
                 (300, 14, 13, 0, "none"), (300, 16, 15, 3, "none"), (300, 16, 15, 2, "mixed"),
                 (300, 16, 9, 3, "mixed"), (300, 16, 9, 1, "mixed"),          # nt < C - 1
                 (300, 14, 13, 3, "all"), (300, 14, 13, 2, "all"),
                 (CS_V2, 14, 13, 3, "mixed"), (CS_V2, 14, 13, 2, "mixed"), (CS_V2, 3, 2, 0, "none")]
CONSIST_BWD_EXTRA = [(CS_BWD_NB * LT + 5, 3, 2, 2, "mixed"), (CS_BWD_NB * LT + 5, 14, 13, 3, "mixed")]


@functools.lru_cache(maxsize=4)
def consist_inputs(case):
    """Storage as the wrappers pass it: logits NDHWC [V, C] (voxel stride C, class stride 1), refiner NDHWC [nt, V, 2]
    (organ 2 V, class 1, voxel 2), attention maps NCDHW [nt, V]. Refiner logits are multiples of 1/4; the last
    unsupervised organ (when there are at least two) has no confident voxel."""
    V, C, nt, natt, pattern = case
    gen = torch.Generator().manual_seed(V % 1009 + 17 * C + 3 * nt + natt)
    lg = torch.randn(V, C, generator=gen) * 2 + (torch.rand(C, generator=gen) * 2 - 1)
    ref = torch.randint(-24, 25, (nt, V, 2), generator=gen).float() / 4
    atts = [torch.randn(nt, V, generator=gen) * 2 for _ in range(natt)]
    if pattern == "none":
        lt = torch.zeros(nt)
    elif pattern == "all":
        lt = torch.ones(nt)
    else:
        lt = (torch.arange(nt) % 3 == 1).float()
        if nt == 2:
            lt = torch.tensor([1.0, 0.0])
    un = [g for g in range(nt) if lt[g] == 0]
    if len(un) >= 2:
        ref[un[-1]] = torch.randint(-4, 5, (V, 2), generator=gen).float() / 4 * 0.5   # |r1 - r0| <= 2: never confident
        ref[un[-1]] = (ref[un[-1]] * 4).round() / 4
    return lg.contiguous(), ref.contiguous(), atts, lt


def sig_err(x, s):
    """Relative error of sigm(x) = 1 / (1 + __expf(-x)) given an exact x: the product x log2(e) rounds twice (constant,
    product), exp2 to 1 ulp, so e is off by (2 |x| + 2) u; that enters s by the factor 1 - s; the sum and the
    division round once each (+ slack u)."""
    return ((2 * x.abs() + 2) * (1 - s) + 3) * U


def consist_errs(ref, atts, lg, r0, r1):
    """Per-voxel relative errors: et of t [nt, V], ep of softmax(logits) [V, C], and (value, relative error) per slot."""
    et = ((r1 - r0).abs() + 5) * U
    x = lg - lg.max(1, keepdim=True).values
    ee = (x.abs() + 2) * U
    es = (lg.shape[1] - 1) * U + (ref.p * ee).sum(1, keepdim=True)
    ep = ee + es + 3 * U
    nt = r0.shape[0]
    epm = ep[:, 1:nt + 1].t()
    slot = []
    for k in range(ref.natt):
        slot.append(sig_err(atts[k], ref.maps[k]))
    slot += [None] * (3 - ref.natt)
    if ref.sig[3]:
        s = ref.maps[3]
        slot.append((1 - s) * ref.pm * epm + sig_err(ref.pm, s))
    else:
        slot.append(epm)
    return et, ep, slot


def finalize_errs(I, Z, Y, dI, dZ, dY):
    """fp32 finalize of a soft Dice from fp64 sums: den = Z + Y + 1e-5, num = 2 I + 1e-5 (three conversions, two
    adds each, the constants' own rounding); relative errors of num, den and num / den, absolute error of d."""
    num, den = 2 * I + R.SMOOTH, Z + Y + R.SMOOTH
    rden = (dZ + dY) / den + 4 * U
    rnum = 2 * dI / num + 3 * U
    ratio = num / den
    dd = ratio * (rnum + rden + U) + U * (1 - ratio).abs()
    return rnum, rden, dd


def consist_fwd_bounds(ref, atts, lg, r0, r1, V):
    D = math.ceil(V / (CS_BLOCKS * LT)) + 1
    et, ep, slot = consist_errs(ref, atts, lg, r0, r1)
    t, on = ref.t, ref.on
    dY = D * U * ref.Y + (2 * t * t * et * on).sum(1)
    nt = t.shape[0]
    b_dice = torch.zeros(nt, 4, dtype=F64, device=t.device)
    b_coef = torch.zeros(nt, 4, 2, dtype=F64, device=t.device)
    b_aux = torch.zeros((), dtype=F64, device=t.device)
    dc_abs = (ref.dice * ref.c).abs()
    for k in range(4):
        if ref.maps[k] is None:
            continue
        s = ref.maps[k]
        dI = D * U * ref.I[:, k] + (s * t * (slot[k] + et) * on).sum(1)
        dZ = D * U * ref.Z[:, k] + (2 * s * s * slot[k] * on).sum(1)
        rnum, rden, dd = finalize_errs(ref.I[:, k], ref.Z[:, k], ref.Y, dI, dZ, dY)
        act = ref.active.double()
        b_dice[:, k] = dd * act
        b_coef[:, k, 0] = ref.coef[:, k, 0].abs() * (2 * U + rden + 2 * U)
        b_coef[:, k, 1] = ref.coef[:, k, 1].abs() * (2 * U + rnum + 2 * rden + 4 * U)
        b_aux = b_aux + (dd * act * ref.c[:, k]).sum()
    b_aux = b_aux + (7 + nt) * U * dc_abs.sum() + U * ref.aux.abs()
    return b_dice, b_coef, b_aux


def consist_bwd_bounds(ref, atts, lg, r0, r1, go):
    """The kernel is fed the reference's coef rounded to fp32 (one rounding u each)."""
    et, ep, slot = consist_errs(ref, atts, lg, r0, r1)
    t, on, cf = ref.t, ref.on, ref.coef_used.abs()
    g = abs(go)

    def inner_err(k, s, es):
        return cf[:, k, 1:2] * s * (es + 2 * U) + cf[:, k, 0:1] * t * (et + 2 * U)

    b_att = []
    for k in range(ref.natt):
        s = ref.maps[k]
        ie = inner_err(k, s, slot[k]) + U * ref.inner[k].abs()
        b_att.append((ie * s * (1 - s) * g + ref.datt[k].abs() * (slot[k] * (1 + s / (1 - s)) + 5 * U)) * on)
    s = ref.maps[3]
    ie = inner_err(3, s, slot[3]) + U * ref.inner3.abs()
    nt = t.shape[0]
    gpm = ref.gp[:, 1:nt + 1].t().abs()
    if ref.sig[3]:
        dgp = (ie * s * (1 - s) * g + gpm * (slot[3] * (1 + s / (1 - s)) + 5 * U)) * on
    else:
        dgp = (ie * g + 2 * U * gpm) * on
    dg = torch.zeros_like(ref.gp)
    dg[:, 1:nt + 1] = dgp.t()
    C = lg.shape[1]
    ddot = (dg * ref.p + (ref.gp * ref.p).abs() * ep).sum(1, keepdim=True) + C * U * ref.gpp_abs
    b_dl = ref.dl.abs() * (ep + 2 * U) + ref.p * (dg + ddot)
    return b_att, b_dl


# ------------------------------------------------------------------------------------------------ EDiceLoss_full2
FULL2_V = [1, 257, CS_BLOCKS * LT + 9, CS_BWD_NB * LT + 9]
FULL2_MASKS = ["null", "some", "zeros"]
FULL2_CASES = [(v, sg, uce, m) for v in FULL2_V[:3] for sg in (0, 1) for uce in (0, 1) for m in ("null", "some")] \
    + [(257, 1, 1, "zeros"), (257, 0, 0, "zeros"), (FULL2_V[3], 1, 1, "some"), (FULL2_V[3], 0, 0, "null")]


@functools.lru_cache(maxsize=4)
def full2_inputs(case):
    """x up to |x| = 30 when it goes through the sigmoid (a probability-like value in [0, 1] otherwise), t a soft
    target in [0, 1], m a 0/1 mask or None."""
    V, sg, uce, mk = case
    gen = torch.Generator().manual_seed(V % 1013 + 2 * sg + uce)
    x = torch.randn(V, generator=gen) * 4
    if V >= 5:
        x[1], x[2], x[3] = 30.0, -30.0, 0.0
    if not sg:
        x = torch.sigmoid(x)
    t = torch.rand(V, generator=gen)
    if V >= 5:
        t[4] = 0.0
    m = None if mk == "null" else torch.zeros(V) if mk == "zeros" else (torch.rand(V, generator=gen) < 0.7).float()
    return x, t, m


def full2_fwd_bounds(ref, x, t, sg, uce, V):
    x, t = x.double(), t.double()
    D = math.ceil(V / (min(CS_BLOCKS, -(-V // LT)) * LT)) + 1
    es = sig_err(x, ref.s) if sg else torch.zeros_like(x)
    on = ref.on
    dI = D * U * ref.I.abs() + (ref.s * t * es * on).abs().sum()
    dZ = D * U * ref.Z + (2 * ref.s * ref.s * es * on).sum()
    dY = D * U * ref.Y
    rnum, rden, dd = finalize_errs(ref.I, ref.Z, ref.Y, dI, dZ, dY)
    bl = dd
    if uce:
        lp = torch.log1p(torch.exp(-x.abs()))
        el = U * (x * t).abs() + U * (x.clamp(min=0) - x * t).abs() + 6 * U * lp + U * ref.bce.abs()
        dB = D * U * ref.bce.abs().sum() + el.sum()
        bl = bl + dB / V + U * ref.bce.sum().abs() / V
    bl = bl + U * ref.loss.abs()
    b_coef = torch.stack([ref.coef[0].abs() * (rden + 2 * U), ref.coef[1].abs() * (rnum + 2 * rden + 4 * U),
                          ref.coef[2].abs() * 2 * U])
    return bl, b_coef


def full2_bwd_bounds(ref, x, t, sg, go, coef):
    x, t = x.double(), t.double()
    A, B, cb = (abs(float(c)) for c in coef)
    esg = sig_err(x, ref.sg)
    b = cb * (ref.sg * esg + U * (ref.sg - t).abs()) + 2 * U * ref.dbce.abs()
    es = esg if sg else torch.zeros_like(x)
    s = ref.s
    dds = (B * s.abs() * (es + 2 * U) + A * t * 2 * U + U * ref.ds.abs()) * ref.on
    if sg:
        dds = dds * s * (1 - s) + ref.dd.abs() * (es * (1 + s / (1 - s)) + 3 * U)
    b = b + dds + U * (ref.dbce + ref.dd).abs()
    return abs(go) * b + U * ref.dx.abs()
