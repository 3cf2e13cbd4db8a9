"""csrc/loss.hip and csrc/consist.hip kernel by kernel against the fp64 references of loss_reference.py:
u3d_partial_loss_fwd (loss_partial_kernel<2|8|14|16|32>, loss_partial16_pair_kernel, loss_combine_kernel,
loss_final_kernel), u3d_partial_loss_bwd (loss_bwd_kernel<NC, float|bf16>), u3d_dice_metric (dice_count_kernel,
dice_final_kernel), u3d_dice_metric_binary (dice_binary_count_kernel), u3d_partial_target, u3d_consistency_fwd / _bwd
(consist_fwd_kernel, consist_finalize_kernel, consist_bwd_kernel) and u3d_edice_full2_fwd / _bwd (full2_*). The C entry
points are called through u3d._lib on buffers the test allocates: outputs and workspaces pre-filled with NaN, every
workspace of exactly the advertised size and followed by a guard block that must come back unchanged. Every element is
compared. Cases, inputs and the bound functions live in loss_cases.py (the kernels' constants are named at its top),
and test_loss_reference.py asserts the cases' input conditions on the CPU.

Bounds: worst-case counts of the fp32 roundings in the code, u = 2^-24 (2^-8 for a bf16 store), times magnitudes of the
fp64 reference only, all inflated by 1 + 2^-10. The hardware exp2 / log / rcp are taken at the 1 ulp = 2 u the code's
comments claim, libm's expf / logf at 1 ulp and log1pf at 2 ulp.

softmax   x = lg - m rounds once (u |x|), x log2(e) twice (the constant, the product): e = exp2(..) is off by
          ee = (3 |x| + 2) u; s = sum e by es = (C - 1) u + sum_c p_c ee_c; p = e rcp(s) by ep = ee + es + 3 u.
          sigmoid 1 / (1 + expf(-x)): ep = 5 u. identity: ep = 0. (saturated cases: + u, the reference's own fp32 p.)
sums      D = ceil(nvox / (blocks * voxels per block)) fmas per thread + 6 wave + 4 block levels, then fp64:
          dI = D u I + sum t p ep,  dZ = D u Z + sum 2 p^2 ep,  Y is a sum of ones: exact.
BCE       ls = log2(s) ln2: dls = 4 u ln s + es. hit: lq = x - ls: u |x| + dls + u |lq|. non-hit: lq = ln(s - e_c) - ls,
          where s - e_c cancels: relative (es + p ee) / (1 - p) + u, about (C + 1) u / (1 - p); then 4 u |ln(s - e_c)|
          + dls + u |lq|. sigmoid / identity (bce_elem): ep + 2 u |log p|, ep p / (1 - p) + 4 u |log(1 - p)|.
          An element the reference clamps at 100 is clamped by the kernel too (the cases keep logs away from -100): 0.
          dB = D u sum|bce| + sum of these. Under uce 0 the kernel writes sums[c][3] = 0, as u3d.h says.
loss      loss_final_kernel: ratio = (2 I + 1e-5) / (Z + Y + 1e-5) in fp64, rounded to fp32, subtracted from 1:
          dd = 2 dI / den + ratio (dZ + dY) / den + u ratio + u |d|; the BCE mean rounds to fp32 (uce 1): (dB + u B) / n;
          loss <= sum_c w_c dd_c / C + sum_c w_c (..) + u |loss|. All weights zero: exactly 0.
backward  a, b, kb are formed in fp64 and rounded once (u each). When the kernel's own forward sums are fed, their
          errors enter through den and den^2: a by (dZ + dY) / den, b by 2 dI / num + 2 (dZ + dY) / den.
          g1 = t a + p b: t |a| ra + p |b| (ep + rb + 2 u) + u |g1|.
          g2 = kb (p - t) rcp(max((1 - p) p, 1e-12)): relative p ep / |p - t| + [p ep / (1 - p) + ep] + 8 u, the
          bracket only while the clamp is open (max is 1-Lipschitz, so the bound holds across the clamp).
          dot = sum g p: ddot = sum (dg p + |g p| ep) + C u sum |g p|;  r = p (g - dot): |r| (ep + 2 u) + p (dg + ddot).
          sigmoid: r = g (1 - p) p: dg (1 - p) p + |r| (p ep / (1 - p) + ep + 3 u). identity: dg.
          uce 2 adds kb (p - onehot): kb (p ep + u |p - t|) + 2 u |..| + u |result|. bf16: + 2^-8 (|result| + bound).
metrics   counts and argmax are exact. dice_final_kernel: conversions, a division, S adds, / S: (S + 5) u |metric|.
consist   t = e1 / (e0 + e1) with libm expf: et = (|r1 - r0| + 5) u. sigm(x) = 1 / (1 + __expf(-x)): the argument
          x log2(e) rounds twice, so e is off by (2 |x| + 2) u and s by ((2 |x| + 2) (1 - s) + 3) u =: esig, growing
          with |x|. softmax_row with libm expf: ee = (|x| + 2) u, ep as above. The softmax map through a sigmoid
          (natt < 3): (1 - s) p ep + esig(p). Per thread D = ceil(V / (128 * 256)) + 1 fmas in fp32, the rest fp64:
          dY = D u Y + sum 2 t^2 et, dI = D u I + sum s t (esig + et), dZ = D u Z + sum 2 s^2 esig.
          finalize in fp32: den by (dZ + dY) / den + 4 u, num by 2 dI / num + 3 u, d = 1 - num / den by
          ratio (rnum + rden + u) + u |d|; c = w_k wf / (nt - sup): 2 u; coef A by rden + 4 u, B by rnum + 2 rden + 6 u;
          aux by sum dd c + (7 + nt) u sum |d c| + u |aux|.
          backward (fed the reference's coef rounded to fp32): inner = cB s - cA t: cB s (esig + 2 u) + cA t (et + 2 u)
          + u |inner|; times s (1 - s): esig (1 + s / (1 - s)) + 5 u; dlogits as the loss backward's softmax line.
full2     as consist with x exact; the BCE element max(x, 0) - x t + log1pf(expf(-|x|)): u |x t| + u |max - x t|
          + 6 u log1p(..) + u |element|; coef[2] = 1 / (float) V: 2 u.

Every test prints its worst error as a share of the bound ("SHARE <family> <value>") before asserting.
"""
import pytest
import torch

import loss_cases as K
import loss_reference as R
from loss_cases import (BWD_NB, CS_BLOCKS, CS_BWD_NB, DICE_NB, LP_NB, LP_VOX, LT, PT_NB, SLACK, U3D_LOSS_NB,  # noqa: F401
                        SOFT)

pytestmark = pytest.mark.gpu

f32, f64, bf16, i64 = torch.float32, torch.float64, torch.bfloat16, torch.int64
GUARD = 256           # bytes after each workspace
GUARD_BYTE = 0xA5


def _share(name, err, bound):
    """max err / bound (an entry with a zero bound must have no error); printed, then returned for the assertion."""
    err, bound = torch.as_tensor(err), torch.as_tensor(bound)
    assert bool(torch.isfinite(err).all()), f"{name}: an element was not written or is not finite"
    zero = bound == 0
    assert not bool((err[zero] != 0).any()), f"{name}: error where the bound is 0"
    s = (err[~zero] / bound[~zero]).max().item() if bool((~zero).any()) else 0.0
    print(f"SHARE {name} {s:.4f}")
    return s


def _L():
    from u3d import _lib as L
    return L


def _stream():
    from u3d.ops import _stream as s
    return s()


def _nan(shape, dtype, dev):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


def _ws(nbytes, dev):
    """A workspace of exactly nbytes of NaN bit patterns followed by a guard block; returns (tensor, check)."""
    buf = torch.full((nbytes + GUARD,), 0xFF, dtype=torch.uint8, device=dev)
    buf[nbytes:] = GUARD_BYTE

    def check():
        assert bool((buf[nbytes:] == GUARD_BYTE).all()), "the kernel wrote past its workspace"
    return buf, check


def _ptr(t):
    return None if t is None else t.data_ptr()


# ------------------------------------------------------------------------------------------------ partial loss
def _fwd(dev, lg, lab, w, S, V, C, mode, uce):
    L = _L()
    nvox = S * V
    nbytes = L.query("u3d_loss_workspace_bytes", S, V, C)
    nb = min(U3D_LOSS_NB, -(-nvox // LT))
    assert nbytes == max(nb, min(LP_NB, -(-nvox // LP_VOX)) if C == 16 else 0) * 4 * C * 4
    ws, check = _ws(nbytes, dev)
    sums, loss = _nan((C, 4), f64, dev), _nan((1,), f32, dev)
    L.call("u3d_partial_loss_fwd", lg.data_ptr(), lab.data_ptr(), S, V, C, mode, w.data_ptr(), uce, sums.data_ptr(),
           loss.data_ptr(), ws.data_ptr(), _stream())
    torch.cuda.synchronize()
    check()
    return sums, loss


def _bwd(dev, lg, lab, w, S, V, C, mode, uce, sums, dtype):
    go = torch.tensor([K.GRAD_OUT], dtype=f32, device=dev)
    dl = _nan((S * V, C), dtype, dev)
    _L().call("u3d_partial_loss_bwd", _L().BF16 if dtype == bf16 else _L().F32, lg.data_ptr(), lab.data_ptr(), S, V, C,
              mode, w.data_ptr(), uce, sums.data_ptr(), go.data_ptr(), dl.data_ptr(), _stream())
    torch.cuda.synchronize()
    return dl.double()


def _check_fwd(tag, dev, dlg, dlab, dw, case, ref, pair, round_p=False):
    S, V, C, mode, uce = case[:5]
    sums, loss = _fwd(dev, dlg, dlab, dw, S, V, C, mode, uce)
    bs, bl, _ = K.loss_fwd_bounds(ref, dw, mode, uce, S * V, pair=pair, round_p=round_p)
    for k, nm in enumerate(("I", "Z", "Y", "bce")):
        assert _share(f"loss-sum-{nm} {tag}", (sums[:, k] - ref.sums[:, k]).abs(), SLACK * bs[:, k]) <= 1
    assert _share(f"loss-fwd {tag}", (loss.double() - ref.loss).abs(), SLACK * bl.reshape(1)) <= 1
    return sums, loss, bs


def _pair_settings(C, mode, uce):
    return (1, 0) if (C == 16 and mode == SOFT and uce == 1) else (None,)


def _with_pair(setting):
    import contextlib
    from u3d import ops
    return contextlib.nullcontext() if setting is None else ops.option("LOSS_PAIR", setting)


def _run_loss_case(dev, case, dtypes=(f32, bf16), own_sums=False):
    S, V, C, mode, uce = case[:5]
    lg, lab, w = K.loss_inputs(case[:6])
    dlg, dlab, dw = lg.to(dev), lab.to(dev), w.to(dev)
    ref = R.partial_loss_ref(dlg, dlab, dw, mode, uce, grad_out=K.GRAD_OUT)
    tag = K.case_id(case[:6])
    out = None
    for setting in _pair_settings(C, mode, uce):
        with _with_pair(setting):
            out = _check_fwd(f"{tag} pair={setting}", dev, dlg, dlab, dw, case, ref, pair=bool(setting))
    for dtype in dtypes:
        dl = _bwd(dev, dlg, dlab, dw, S, V, C, mode, uce, ref.sums.contiguous(), dtype)
        bound = K.loss_bwd_bounds(ref, mode, uce, out_bf16=dtype == bf16)
        assert _share(f"loss-bwd {tag} {str(dtype)[6:]}", (dl - ref.dl).abs(), SLACK * bound) <= 1
    if own_sums:      # as the model runs it: the backward on the forward's own sums
        sums, _, bs = out
        dl = _bwd(dev, dlg, dlab, dw, S, V, C, mode, uce, sums, f32)
        bound = K.loss_bwd_bounds(ref, mode, uce, dsums=SLACK * bs)
        assert _share(f"loss-bwd-own-sums {tag}", (dl - ref.dl).abs(), SLACK * bound) <= 1
    return ref, out


@pytest.mark.parametrize("C", K.CLASSES)
@pytest.mark.parametrize("mode,uce", K.MODES, ids=lambda m: str(m))
def test_partial_loss_small(gpu, C, mode, uce):
    for case in K.LOSS_SMALL:
        if case[2:5] == (C, mode, uce):
            _run_loss_case(gpu, case, own_sums=case[:2] == (2, 693))


@pytest.mark.parametrize("case", K.LOSS_SPECIAL, ids=K.case_id)
def test_partial_loss_special(gpu, case):
    ref, (sums, loss, _) = _run_loss_case(gpu, case)
    if case[5] == "zero_w":
        assert loss.item() == 0.0
    else:
        C = case[2]
        den = sums[C - 1, 1] + sums[C - 1, 2] + 1e-5
        assert abs(den.item() / 1e-5 - 1) < 1e-6


@pytest.mark.parametrize("case", K.LOSS_FWD_MULTI, ids=K.case_id)
def test_partial_loss_fwd_multi_trip(gpu, case):
    """Two to three trips of the grid-stride loops of loss_partial16_pair_kernel and loss_partial_kernel, with a tail."""
    S, V, C, mode, uce = case[:5]
    assert S * V > 2 * LP_NB * LP_VOX and S * V > 2 * U3D_LOSS_NB * LT
    lg, lab, w = K.loss_inputs(case)
    dlg, dlab, dw = lg.to(gpu), lab.to(gpu), w.to(gpu)
    ref = R.partial_loss_ref(dlg, dlab, dw, mode, uce)
    for setting in _pair_settings(C, mode, uce):
        with _with_pair(setting):
            _check_fwd(f"{K.case_id(case)} pair={setting}", gpu, dlg, dlab, dw, case, ref, pair=bool(setting))


@pytest.mark.parametrize("case", K.LOSS_BWD_MULTI, ids=K.case_id)
def test_partial_loss_bwd_multi_trip(gpu, case):
    """A second trip of loss_bwd_kernel's grid-stride loop: the prefetch of v + stride and its clamped index."""
    S, V, C, mode, uce, _, dtype = case
    assert S * V > BWD_NB * LT and (S * V) % LT
    lg, lab, w = K.loss_inputs(case[:6])
    dlg, dlab, dw = lg.to(gpu), lab.to(gpu), w.to(gpu)
    ref = R.partial_loss_ref(dlg, dlab, dw, mode, uce, grad_out=K.GRAD_OUT)
    dl = _bwd(gpu, dlg, dlab, dw, S, V, C, mode, uce, ref.sums.contiguous(), dtype)
    bound = K.loss_bwd_bounds(ref, mode, uce, out_bf16=dtype == bf16)
    err = (dl - ref.dl).abs()
    assert _share(f"loss-bwd-multi {K.case_id(case)} second trip", err[BWD_NB * LT:], SLACK * bound[BWD_NB * LT:]) <= 1
    assert _share(f"loss-bwd-multi {K.case_id(case)}", err, SLACK * bound) <= 1


@pytest.mark.parametrize("case", K.LOSS_SAT, ids=K.case_id)
def test_partial_loss_saturated(gpu, case):
    """p == 1 in fp32: log(1 - p) = ln(s - e_c) - ln s has s - e_c == 0 and must clamp at -100, the backward's
    (1 - p) p at 1e-12; the reference rounds its probabilities to fp32 as PyTorch's softmax does."""
    S, V, C = case
    lg, lab, w, lead = K.sat_inputs(case)
    dlg, dlab, dw = lg.to(gpu), lab.to(gpu), w.to(gpu)
    ref = R.partial_loss_ref(dlg, dlab, dw, SOFT, 1, grad_out=K.GRAD_OUT, round_p_to_fp32=True)
    full = (S, V, C, SOFT, 1)
    for setting in _pair_settings(C, SOFT, 1):
        with _with_pair(setting):
            sums, loss, _ = _check_fwd(f"sat {K.case_id(case)} pair={setting}", gpu, dlg, dlab, dw, full, ref,
                                       pair=bool(setting), round_p=True)
        assert bool(torch.isfinite(sums).all()) and bool(torch.isfinite(loss).all())
        nclamp = (ref.bce == 100).sum(0)
        assert bool((nclamp > 0).all()) and bool((sums[:, 3] >= 100 * nclamp).all())      # the -100 clamp shows
    for dtype in (f32, bf16):
        dl = _bwd(gpu, dlg, dlab, dw, S, V, C, SOFT, 1, ref.sums.contiguous(), dtype)
        assert bool(torch.isfinite(dl).all())
        bound = K.loss_bwd_bounds(ref, SOFT, 1, out_bf16=dtype == bf16, round_p=True)
        assert _share(f"sat-bwd {K.case_id(case)} {str(dtype)[6:]}", (dl - ref.dl).abs(), SLACK * bound) <= 1


# ------------------------------------------------------------------------------------------------ Dice metrics
@pytest.mark.parametrize("want_argmax", [True, False], ids=["argmax", "no-argmax"])
@pytest.mark.parametrize("case", K.DICE_CASES, ids=K.case_id)
def test_dice_metric(gpu, case, want_argmax):
    S, V, C, ncls = case
    lg, lab = K.dice_inputs(case)
    dlg, dlab = lg.to(gpu), lab.to(gpu)
    ref = R.dice_metric_ref(dlg, dlab, ncls)
    counts = torch.full((S, ncls, 3), -7, dtype=i64, device=gpu)
    metrics = _nan((ncls, 3), f32, gpu)
    am = torch.full((S, V), -7, dtype=i64, device=gpu) if want_argmax else None
    _L().call("u3d_dice_metric", dlg.data_ptr(), dlab.data_ptr(), S, V, C, ncls, counts.data_ptr(), metrics.data_ptr(),
              _ptr(am), _stream())
    torch.cuda.synchronize()
    assert torch.equal(counts, ref.counts)
    if want_argmax:
        assert torch.equal(am, ref.argmax)
    assert _share(f"dice-metric {K.case_id(case)}", (metrics.double() - ref.metrics).abs(),
                  SLACK * K.metric_bound(ref.metrics, S)) <= 1


@pytest.mark.parametrize("layout", ["ncdhw", "ndhwc-view"])
@pytest.mark.parametrize("case", K.DICE2_CASES, ids=K.case_id)
def test_dice_metric_binary(gpu, case, layout):
    nt, V = case
    rf, lab = K.dice2_inputs(case)
    if layout == "ncdhw":
        store, (rsn, rsc, rsv) = rf.to(gpu), (2 * V, V, 1)
    else:
        store, (rsn, rsc, rsv) = rf.permute(0, 2, 1).contiguous().to(gpu), (2 * V, 1, 2)
    dlab = lab.to(gpu)
    ref = R.dice_binary_ref(store, rsn, rsc, rsv, nt, V, dlab)
    counts = torch.full((nt, 3), -7, dtype=i64, device=gpu)
    metrics = _nan((nt, 3), f32, gpu)
    for am in (torch.full((nt, V), -7, dtype=i64, device=gpu), None):
        _L().call("u3d_dice_metric_binary", store.data_ptr(), nt, V, rsn, rsc, rsv, dlab.data_ptr(), counts.data_ptr(),
                  metrics.data_ptr(), _ptr(am), _stream())
        torch.cuda.synchronize()
        assert torch.equal(counts, ref.counts)
        assert am is None or torch.equal(am, ref.argmax)
        assert _share(f"dice-binary {K.case_id(case)} {layout}", (metrics.double() - ref.metrics).abs(),
                      SLACK * K.metric_bound(ref.metrics, 1)) <= 1


# ------------------------------------------------------------------------------------------------ partial target
@pytest.mark.parametrize("case", K.PT_CASES, ids=K.case_id)
def test_partial_target(gpu, case):
    S, V, M, stride, lmin, lmax = case
    assert case != K.PT_CASES[-1] or S * V > PT_NB * LT
    lab, mask = K.pt_inputs(case)
    want = R.partial_target_ref(lab, mask, stride, M, lmin, lmax)
    dlab, dmask = lab.to(gpu), mask.to(gpu)
    out = _nan((S, V), f32, gpu)
    _L().call("u3d_partial_target", dlab.data_ptr(), S, V, dmask.data_ptr(), stride, M, lmin, lmax, out.data_ptr(),
              _stream())
    torch.cuda.synchronize()
    assert torch.equal(out.cpu().view(torch.int32), want.view(torch.int32))
    print("SHARE partial-target 0.0000")


# ------------------------------------------------------------------------------------------------ consistency
def _consist_dev(dev, case):
    lg, rf, atts, lt = K.consist_inputs(case)
    return lg.to(dev), rf.to(dev), [a.to(dev) for a in atts], lt.to(dev)


def _consist_args(dlg, drf, datts, dlt, case):
    V, C, nt, natt, _ = case
    ap = [a.data_ptr() for a in datts] + [None] * (3 - natt)
    # attention maps NCDHW [nt, V]; logits NDHWC [V, C]; refiner NDHWC [nt, V, 2]
    return (ap[0], ap[1], ap[2], natt, V, 1, dlg.data_ptr(), C, 1, C, drf.data_ptr(), 2 * V, 1, 2, dlt.data_ptr(), nt, V,
            K.CONFI)


def _run_consist(dev, case, forward=True):
    V, C, nt, natt, pattern = case
    L = _L()
    dlg, drf, datts, dlt = _consist_dev(dev, case)
    r0, r1 = drf[:, :, 0].double(), drf[:, :, 1].double()
    a64 = [a.double() for a in datts]
    ref = R.consistency_ref(datts, dlg, r0, r1, dlt, K.CONFI, K.WF, grad_out=K.GRAD_OUT)
    tag = K.case_id(case)
    args = _consist_args(dlg, drf, datts, dlt, case)
    if forward:
        nbytes = L.query("u3d_consistency_ws_bytes", nt)
        assert nbytes == nt * CS_BLOCKS * 9 * 8 + nt * 4 * 3 * 4 + 256
        ws, check = _ws(nbytes, dev)
        aux, dice, coef = _nan((1,), f32, dev), _nan((nt, 4), f32, dev), _nan((nt, 4, 2), f32, dev)
        L.call("u3d_consistency_fwd", *args, K.WF, aux.data_ptr(), dice.data_ptr(), coef.data_ptr(), ws.data_ptr(),
               _stream())
        torch.cuda.synchronize()
        check()
        b_dice, b_coef, b_aux = K.consist_fwd_bounds(ref, a64, dlg.double(), r0, r1, V)
        if pattern == "all":    # nt - sup == 0: nothing is active, everything exactly 0 and finite
            assert aux.item() == 0.0 and bool((dice == 0).all()) and bool((coef == 0).all())
        assert _share(f"consist-aux {tag}", (aux.double() - ref.aux).abs(), SLACK * b_aux.reshape(1)) <= 1
        assert _share(f"consist-dice {tag}", (dice.double() - ref.dice).abs(), SLACK * b_dice) <= 1
        assert _share(f"consist-coef {tag}", (coef.double() - ref.coef).abs(), SLACK * b_coef) <= 1
    coef32 = ref.coef.float().contiguous()
    rb = R.consistency_ref(datts, dlg, r0, r1, dlt, K.CONFI, K.WF, grad_out=K.GRAD_OUT, coef=coef32)
    go = torch.tensor([K.GRAD_OUT], dtype=f32, device=dev)
    datt = [_nan((nt, V), f32, dev) for _ in range(natt)]
    dp = [d.data_ptr() for d in datt] + [None] * (3 - natt)
    dl = _nan((V, C), f32, dev)
    L.call("u3d_consistency_bwd", *args, coef32.data_ptr(), go.data_ptr(), dp[0], dp[1], dp[2], dl.data_ptr(), _stream())
    torch.cuda.synchronize()
    b_att, b_dl = K.consist_bwd_bounds(rb, a64, dlg.double(), r0, r1, K.GRAD_OUT)
    for k in range(natt):
        assert _share(f"consist-datt{k} {tag}", (datt[k].double() - rb.datt[k]).abs(), SLACK * b_att[k]) <= 1
    assert _share(f"consist-dlogits {tag}", (dl.double() - rb.dl).abs(), SLACK * b_dl) <= 1


@pytest.mark.parametrize("case", K.CONSIST_CASES, ids=K.case_id)
def test_consistency(gpu, case):
    _run_consist(gpu, case)


@pytest.mark.parametrize("case", K.CONSIST_BWD_EXTRA, ids=K.case_id)
def test_consistency_bwd_multi_trip(gpu, case):
    assert case[0] > CS_BWD_NB * LT
    _run_consist(gpu, case, forward=False)


def test_get_loss_two_attention_maps_matches_oracle(gpu):
    """End to end: loss_functions.losses.get_loss with two attention maps (use_cm with one entry off) against
    oracle.ref_cpu.get_loss_consistency: the softmax map takes weights[2] and a sigmoid."""
    import oracle.ref_cpu as O
    from loss_functions.losses import get_loss
    C, nt, D, H, W = 14, 13, 4, 5, 6
    gen = torch.Generator().manual_seed(3)
    out = torch.randn(1, C, D, H, W, generator=gen) * 2
    tgt = torch.randint(0, C, (1, 1, D, H, W), generator=gen).float()
    atts = [torch.randn(1, nt, D, H, W, generator=gen) * 2 for _ in range(2)]
    rfo = torch.randint(-24, 25, (nt, 2, D, H, W), generator=gen).float() / 4
    label_t = [float(g % 3 == 1) for g in range(nt)]
    mask = [torch.ones(C)]
    want = O.get_loss_consistency(out.double(), tgt.double(), [m.double() for m in mask], [a.double() for a in atts],
                                  rfo.double(), label_t)
    leaf = out.to(gpu).requires_grad_(True)
    got, _ = get_loss(leaf, None, [], tgt.to(gpu), mask=[m.to(gpu) for m in mask], attns=[a.to(gpu) for a in atts],
                      refine_output=rfo.to(gpu), label_t=label_t)
    got.backward()
    torch.cuda.synchronize()
    print(f"SHARE get-loss-natt2 {abs(got.item() - want.item()) / (1e-5 * abs(want.item())):.4f}")
    assert abs(got.item() - want.item()) <= 1e-5 * abs(want.item())      # fp32 sums of 120 voxels against fp64
    assert bool(torch.isfinite(leaf.grad).all())


# ------------------------------------------------------------------------------------------------ EDiceLoss_full2
@pytest.mark.parametrize("case", K.FULL2_CASES, ids=K.case_id)
def test_edice_full2(gpu, case):
    V, sg, uce, mk = case
    L = _L()
    x, t, m = K.full2_inputs(case)
    dx_, dt_, dm_ = x.to(gpu), t.to(gpu), None if m is None else m.to(gpu)
    ref = R.full2_ref(dx_, dt_, dm_, sg, uce)
    ws, check = _ws(CS_BLOCKS * 4 * 8, gpu)
    loss, coef = _nan((1,), f32, gpu), _nan((3,), f32, gpu)
    L.call("u3d_edice_full2_fwd", dx_.data_ptr(), dt_.data_ptr(), _ptr(dm_), V, sg, uce, loss.data_ptr(),
           coef.data_ptr(), ws.data_ptr(), _stream())
    torch.cuda.synchronize()
    check()
    tag = K.case_id(case)
    bl, b_coef = K.full2_fwd_bounds(ref, dx_, dt_, sg, uce, V)
    assert _share(f"full2-loss {tag}", (loss.double() - ref.loss).abs(), SLACK * bl.reshape(1)) <= 1
    assert _share(f"full2-coef {tag}", (coef.double() - ref.coef).abs(), SLACK * b_coef) <= 1
    coef32 = ref.coef.float().contiguous()
    rb = R.full2_ref(dx_, dt_, dm_, sg, uce, grad_out=K.GRAD_OUT, coef=coef32)
    go = torch.tensor([K.GRAD_OUT], dtype=f32, device=gpu)
    dx = _nan((V,), f32, gpu)
    L.call("u3d_edice_full2_bwd", dx_.data_ptr(), dt_.data_ptr(), _ptr(dm_), V, sg, coef32.data_ptr(), go.data_ptr(),
           dx.data_ptr(), _stream())
    torch.cuda.synchronize()
    bound = K.full2_bwd_bounds(rb, dx_, dt_, sg, K.GRAD_OUT, coef32.double())
    assert _share(f"full2-bwd {tag}", (dx.double() - rb.dx).abs(), SLACK * bound) <= 1
