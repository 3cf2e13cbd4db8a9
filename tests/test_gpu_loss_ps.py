"""csrc/loss_ps.hip and the _ps kernels of csrc/deepsup.hip against the fp64 references of loss_ps_reference.py:
u3d_partial_loss_ps_fwd (loss_ps_partial_kernel<2|8|14|16|32>, loss_ps_partial16_pair_kernel, loss_ps_combine_kernel,
loss_ps_final_kernel), u3d_partial_loss_ps_bwd (loss_ps_bwd_kernel<NC, float|bf16>), u3d_deepsup_loss_ps_fwd / _bwd,
and the Python wiring (EDiceLoss_partial(per_sample=True), Engine.train_step, GraphedStep). As test_gpu_loss.py: the
C entry points are called on NaN-prefilled outputs with exact-size workspaces followed by a guard block, every element
is compared, every test prints its worst error as a share of the bound ("SHARE <family> <value>") before asserting.
Cases, inputs and the bound functions live in loss_ps_cases.py (the kernels' grid constants are named at its top).

Bounds: the method at the head of test_gpu_loss.py (worst-case counts of the fp32 roundings in the code, u = 2^-24,
2^-8 for a bf16 store, times magnitudes of the fp64 reference only, inflated by 1 + 2^-10), applied to the new code.
The per-voxel arithmetic of loss_ps.hip is loss.hip's, so the probability errors (ep, ee, es), the BCE element errors
and the backward's per-voxel bound are loss_cases' functions by import. What differs:

sums_ps   one sample's V voxels over its own blocks: D = ceil(V / (blocks per sample * voxels per block)) + 10 fp32
          additions per sum (the thread's trips, the wave tree, the block's 4 waves), then fp64:
          dI_s = D u I_s + sum_v t p ep,  dZ_s = D u Z_s + sum_v 2 p^2 ep,  Y_s exact,  dB_s = D u sum|bce| + sum el.
pooled    X_c = sum_s m_sc X_sc in fp64, s ascending: dX_c = sum_s m_sc dX_sc + S 2^-53 |X_c|; n_c is exact.
loss      d_c as loss_final_kernel (the ratio in fp64, rounded to fp32, subtracted from 1):
          dd = 2 dI / den + ratio (dZ + dY) / den + u ratio + u |d|.  w^_c = sum_s w_sc / n_c in fp64: (S + 2) 2^-53.
          The BCE mean B_c / (n_c V) is rounded to fp32 (u) after a product and a division in fp64 (2 2^-53).
          loss <= sum_c w^_c (dd_c + rw |d_c|) / C + sum_{n_c > 0} w^_c (dB_c + (u + rw + 2^-52) |B_c|) / (n_c V) + u |loss|.
          All rows zero: every w^_c is 0 and every d_c finite, so the loss is exactly 0.
backward  a, b, kb are formed in fp64 from the pooled sums, w^_c and 1 / (n_c V), and rounded once to fp32 (u each),
          as loss.hip's; the fp64 roundings of w^_c and n_c V add (S + 6) 2^-53 of the gradient's magnitude. A class the
          sample does not supervise has a = b = kb = 0 exactly, so its g_c is exactly 0; a sample that supervises no
          class is written as zeros. Fed the kernel's own pooled sums, their errors enter as in test_gpu_loss.py.
equal     against u3d_partial_loss_fwd / _bwd on the same inputs: each side within its own bound of the same fp64
          value, so the two differ by at most the sum of the two bounds.
deepsup   soft Dice of at most 4096 voxels per sample and level: D = 1 + 10 additions, ep <= (3 |x| + 2 + C + 3) u
          with |x| <= 20: sums_ps and pooled within 2^-16 relative, losses within 2^-15; gradients by the rule of
          test_gpu_deepsup_loss.py (rtol 1e-3, atol 1e-4 max|ref|), equal rows against the batch entry points by its
          fused-against-composed rule (value rtol 1e-5, gradients rtol 1e-4 with atol 1e-6 max|ref|: the partial sums
          are taken in another order).
"""
import argparse
import ctypes
import sys

import numpy as np
import pytest
import torch

import deepsup_cases as DC
import loss_cases as K
import loss_ps_cases as P
import loss_ps_reference as PR
import loss_reference as R
from loss_cases import SLACK, SOFT

pytestmark = pytest.mark.gpu

f32, f64, bf16 = torch.float32, torch.float64, torch.bfloat16
GUARD = 256
GUARD_BYTE = 0xA5


def _share(name, err, bound):
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
    buf = torch.full((nbytes + GUARD,), 0xFF, dtype=torch.uint8, device=dev)
    buf[nbytes:] = GUARD_BYTE

    def check():
        assert bool((buf[nbytes:] == GUARD_BYTE).all()), "the kernel wrote past its workspace"
    return buf, check


def _fwd(dev, lg, lab, w, S, V, C, mode, uce):
    L = _L()
    nbytes = L.query("u3d_loss_ps_workspace_bytes", S, V, C)
    assert nbytes == P.workspace_bytes(S, V, C)
    ws, check = _ws(nbytes, dev)
    sums_ps, pooled, loss = _nan((S, C, 4), f64, dev), _nan((C, 5), f64, dev), _nan((1,), f32, dev)
    L.call("u3d_partial_loss_ps_fwd", lg.data_ptr(), lab.data_ptr(), S, V, C, mode, w.data_ptr(), uce,
           sums_ps.data_ptr(), pooled.data_ptr(), loss.data_ptr(), ws.data_ptr(), _stream())
    torch.cuda.synchronize()
    check()
    return sums_ps, pooled, loss


def _bwd(dev, lg, lab, w, S, V, C, mode, uce, pooled, dtype):
    go = torch.tensor([K.GRAD_OUT], dtype=f32, device=dev)
    dl = _nan((S * V, C), dtype, dev)
    _L().call("u3d_partial_loss_ps_bwd", _L().BF16 if dtype == bf16 else _L().F32, lg.data_ptr(), lab.data_ptr(), S, V,
              C, mode, w.data_ptr(), uce, pooled.data_ptr(), go.data_ptr(), dl.data_ptr(), _stream())
    torch.cuda.synchronize()
    return dl


def _check_fwd(tag, dev, dlg, dlab, dw, case, ref):
    S, V, C, mode, uce = case[:5]
    sums_ps, pooled, loss = _fwd(dev, dlg, dlab, dw, S, V, C, mode, uce)
    nbx = P.fwd_blocks(S, V, C, mode, uce)
    bs, bp, bl = P.fwd_bounds(ref, S, V, mode, uce, nbx, P.PAIR_VOX if P.is_pair(C, mode, uce) else P.PT)
    for k, nm in enumerate(("I", "Z", "Y", "bce")):
        assert _share(f"ps-sum-{nm} {tag}", (sums_ps[:, :, k] - ref.sums_ps[:, :, k]).abs(), SLACK * bs[:, :, k]) <= 1
        assert _share(f"ps-pooled-{nm} {tag}", (pooled[:, k] - ref.pooled[:, k]).abs(), SLACK * bp[:, k]) <= 1
    assert torch.equal(pooled[:, 4], ref.pooled[:, 4]), "n_c"
    assert _share(f"ps-fwd {tag}", (loss.double() - ref.loss).abs(), SLACK * bl.reshape(1)) <= 1
    return sums_ps, pooled, loss, bp, bl


def _check_kind(tag, case, ref, dw, loss, dls):
    """The properties of the mask kinds, on top of the comparison with the reference."""
    S, V, C, mode, uce, kind = case[:6]
    if kind == "all_zero":
        assert loss.item() == 0.0 and loss.view(torch.int32).item() == 0, "all rows zero: the loss is bitwise 0"
    zero_rows = [s for s in range(S) if not bool((dw[s] != 0).any())]
    if kind in ("zero_row", "all_zero", "ct_mri"):
        assert zero_rows
    for dl in dls:
        for s in zero_rows:
            blk = dl[s * V:(s + 1) * V]
            bits = blk.view(torch.int16 if blk.dtype == bf16 else torch.int32)
            assert bool((bits == 0).all()), f"{tag}: sample {s} has a zero row, its dlogits must be bitwise 0"
    if kind == "disjoint":
        assert bool((ref.n == 1).all())


def _run_case(dev, case, dtypes=(f32, bf16), own=False, forward=True):
    S, V, C, mode, uce, kind = case[:6]
    lg, lab, w = P.ps_inputs(case[:6])
    dlg, dlab, dw = lg.to(dev).contiguous(), lab.to(dev).contiguous(), w.to(dev).contiguous()
    ref = PR.partial_loss_ps_ref(dlg, dlab, dw, mode, uce, grad_out=K.GRAD_OUT)
    tag = P.case_id(case[:6])
    out = _check_fwd(tag, dev, dlg, dlab, dw, case, ref) if forward else None
    dls = []
    rp = ref.pooled.contiguous()
    for dtype in dtypes:
        dl = _bwd(dev, dlg, dlab, dw, S, V, C, mode, uce, rp, dtype)
        bound = P.bwd_bounds(ref, mode, uce, S, out_bf16=dtype == bf16)
        assert _share(f"ps-bwd {tag} {str(dtype)[6:]}", (dl.double() - ref.dl).abs(), SLACK * bound) <= 1
        dls.append(dl)
    if own and forward:    # as the model runs it: the backward on the forward's own pooled sums
        _, pooled, _, bp, _ = out
        dl = _bwd(dev, dlg, dlab, dw, S, V, C, mode, uce, pooled, f32)
        bound = P.bwd_bounds(ref, mode, uce, S, dpooled=SLACK * bp)
        assert _share(f"ps-bwd-own-pooled {tag}", (dl.double() - ref.dl).abs(), SLACK * bound) <= 1
        dls.append(dl)
    if forward:
        _check_kind(tag, case, ref, dw, out[2], dls)
    return ref, out, dls, (dlg, dlab, dw)


def _pair_default():
    from u3d import ops
    return ops.option("LOSS_PAIR", 1)


def _check_equal(dev, case, ref, out, dls, tensors):
    """Equal rows against the batch kernels of loss.hip, run here on the same inputs with the one row."""
    S, V, C, mode, uce = case[:5]
    dlg, dlab, dw = tensors
    L = _L()
    tag = P.case_id(case[:6])
    row = dw[0].contiguous()
    pair = C == 16 and mode == SOFT and uce == 1
    refb = R.partial_loss_ref(dlg.reshape(S * V, C), dlab.reshape(-1), row, mode, uce, grad_out=K.GRAD_OUT)
    ws, check = _ws(L.query("u3d_loss_workspace_bytes", S, V, C), dev)
    sums, loss_b = _nan((C, 4), f64, dev), _nan((1,), f32, dev)
    with _pair_default():
        L.call("u3d_partial_loss_fwd", dlg.data_ptr(), dlab.data_ptr(), S, V, C, mode, row.data_ptr(), uce,
               sums.data_ptr(), loss_b.data_ptr(), ws.data_ptr(), _stream())
    torch.cuda.synchronize()
    check()
    bsb, blb, _ = K.loss_fwd_bounds(refb, row, mode, uce, S * V, pair=pair)
    _, pooled, loss, bp, bl = out
    # every sample supervises the classes the row keeps: pooled = the batch sums there, 0 where the row is 0
    keep = (row != 0).double()[:, None]
    assert _share(f"ps-equal-pooled {tag}", (pooled[:, :4] - keep * sums).abs(), SLACK * (bp + keep * bsb)) <= 1
    assert _share(f"ps-equal-loss {tag}", (loss.double() - loss_b.double()).abs(), SLACK * (bl + blb).reshape(1)) <= 1
    go = torch.tensor([K.GRAD_OUT], dtype=f32, device=dev)
    dlb = _nan((S * V, C), f32, dev)
    L.call("u3d_partial_loss_bwd", L.F32, dlg.data_ptr(), dlab.data_ptr(), S, V, C, mode, row.data_ptr(), uce,
           refb.sums.contiguous().data_ptr(), go.data_ptr(), dlb.data_ptr(), _stream())
    torch.cuda.synchronize()
    bound = P.bwd_bounds(ref, mode, uce, S) + K.loss_bwd_bounds(refb, mode, uce)
    assert _share(f"ps-equal-bwd {tag}", (dls[0].double() - dlb.double()).abs(), SLACK * bound) <= 1
    # and the reference itself: equal rows are the batch loss with that row
    assert abs(ref.loss.item() - refb.loss.item()) <= 1e-12 * max(1.0, abs(refb.loss.item()))


@pytest.mark.parametrize("C", P.CLASSES)
@pytest.mark.parametrize("mode,uce", P.MODES, ids=lambda m: str(m))
def test_partial_loss_ps_small(gpu, C, mode, uce):
    for (S, V) in P.SMALL_SV:
        for kind in P.kinds_for(S, V):
            case = (S, V, C, mode, uce, kind)
            ref, out, dls, tensors = _run_case(gpu, case, own=(S, V) == (2, 693))
            if kind == "equal":
                _check_equal(gpu, case, ref, out, dls, tensors)


def test_partial_loss_ps_ct_mri_pair(gpu):
    """A CT case that annotates one organ next to an MRI case that annotates none (C = 14), in both orders: the MRI
    patch gets no gradient at all and enters no sum, the CT patch is trained as if alone."""
    S, V, C = 2, 693, 14
    for order in ((P.CT_ROW, P.MRI_ROW), (P.MRI_ROW, P.CT_ROW)):
        lg, lab, _ = P.ps_inputs((S, V, C, SOFT, 1, "mixed"))
        w = torch.tensor(order, dtype=f32)[:, :C]
        dlg, dlab, dw = lg.to(gpu).contiguous(), lab.to(gpu).contiguous(), w.to(gpu).contiguous()
        ref = PR.partial_loss_ps_ref(dlg, dlab, dw, SOFT, 1, grad_out=K.GRAD_OUT)
        case = (S, V, C, SOFT, 1, "ct_mri")
        tag = f"ct-mri {'ct-first' if order[0] is P.CT_ROW else 'mri-first'}"
        _, pooled, loss, bp, _ = _check_fwd(tag, gpu, dlg, dlab, dw, case, ref)
        dls = []
        for dtype in (f32, bf16):
            dl = _bwd(gpu, dlg, dlab, dw, S, V, C, SOFT, 1, pooled, dtype)
            bound = P.bwd_bounds(ref, SOFT, 1, S, out_bf16=dtype == bf16, dpooled=SLACK * bp)
            assert _share(f"ps-bwd {tag} {str(dtype)[6:]}", (dl.double() - ref.dl).abs(), SLACK * bound) <= 1
            dls.append(dl)
        _check_kind(tag, case, ref, dw, loss, dls)
        ct = 0 if order[0] is P.CT_ROW else 1
        assert loss.item() > 0 and bool((dls[0][ct * V:(ct + 1) * V] != 0).any())
        # the CT sample alone (S = 1) is the same loss: single supervisor, n_c = 1, the BCE mean over V
        alone = PR.partial_loss_ps_ref(dlg[ct:ct + 1], dlab[ct:ct + 1], dw[ct:ct + 1], SOFT, 1)
        assert abs(alone.loss.item() - ref.loss.item()) <= 1e-12


@pytest.mark.parametrize("case", P.FWD_MULTI, ids=P.case_id)
def test_partial_loss_ps_fwd_multi_trip(gpu, case):
    """A second trip of the forward's per-sample grid-stride loop for 300 voxels (generic and lane-pair kernel)."""
    S, V, C, mode, uce, kind = case
    nbx = P.fwd_blocks(S, V, C, mode, uce)
    vox = P.PAIR_VOX if P.is_pair(C, mode, uce) else P.PT
    assert V == nbx * vox + 300
    lg, lab, w = P.ps_inputs(case)
    dlg, dlab, dw = lg.to(gpu).contiguous(), lab.to(gpu).contiguous(), w.to(gpu).contiguous()
    ref = PR.partial_loss_ps_ref(dlg, dlab, dw, mode, uce)
    _check_fwd(P.case_id(case), gpu, dlg, dlab, dw, case, ref)


@pytest.mark.parametrize("case", P.BWD_MULTI, ids=P.case_id)
def test_partial_loss_ps_bwd_multi_trip(gpu, case):
    """A second trip of loss_ps_bwd_kernel's per-sample loop: the prefetch of v + stride and its clamped index."""
    S, V, C, mode, uce, kind, dtype = case
    nbx = P.blocks(S, V, P.PS_BWD_NB, P.PT)
    assert V == nbx * P.PT + 300
    lg, lab, w = P.ps_inputs(case[:6])
    dlg, dlab, dw = lg.to(gpu).contiguous(), lab.to(gpu).contiguous(), w.to(gpu).contiguous()
    ref = PR.partial_loss_ps_ref(dlg, dlab, dw, mode, uce, grad_out=K.GRAD_OUT)
    dl = _bwd(gpu, dlg, dlab, dw, S, V, C, mode, uce, ref.pooled.contiguous(), dtype)
    bound = P.bwd_bounds(ref, mode, uce, S, out_bf16=dtype == bf16)
    err = (dl.double() - ref.dl).abs()
    tail = torch.cat([torch.arange(s * V + nbx * P.PT, (s + 1) * V, device=gpu) for s in range(S)])
    assert _share(f"ps-bwd-multi {P.case_id(case)} second trip", err[tail], SLACK * bound[tail]) <= 1
    assert _share(f"ps-bwd-multi {P.case_id(case)}", err, SLACK * bound) <= 1


def test_partial_loss_ps_rejections(gpu):
    L = _L()
    S, V, C = 2, 5, 16
    lg, lab = torch.zeros(S, V, C, device=gpu), torch.zeros(S, V, device=gpu)
    w = torch.ones(S, C, device=gpu)
    sums_ps, pooled, loss = _nan((S, C, 4), f64, gpu), _nan((C, 5), f64, gpu), _nan((1,), f32, gpu)
    ws, _ = _ws(L.query("u3d_loss_ps_workspace_bytes", S, V, C), gpu)
    go, dl = torch.ones(1, device=gpu), _nan((S * V, C), f32, gpu)

    def fwd(**kw):
        a = dict(lg=lg.data_ptr(), lab=lab.data_ptr(), S=S, C=C, w=w.data_ptr(), uce=1, pooled=pooled.data_ptr())
        a.update(kw)
        return L.lib().u3d_partial_loss_ps_fwd(a["lg"], a["lab"], a["S"], V, a["C"], 1, a["w"], a["uce"],
                                               sums_ps.data_ptr(), a["pooled"], loss.data_ptr(), ws.data_ptr(),
                                               _stream())

    def bwd(**kw):
        a = dict(lg=lg.data_ptr(), S=S, C=C, uce=1, pooled=pooled.data_ptr())
        a.update(kw)
        return L.lib().u3d_partial_loss_ps_bwd(L.F32, a["lg"], lab.data_ptr(), a["S"], V, a["C"], 1, w.data_ptr(),
                                               a["uce"], a["pooled"], go.data_ptr(), dl.data_ptr(), _stream())

    EINVAL = 1                                   # U3D_EINVAL (include/u3d.h)
    for f in (fwd, bwd):
        assert f(uce=2) == EINVAL                # the cross entropy is unweighted: no per-sample form
        assert b"uce" in L.lib().u3d_last_error()
        assert f(lg=None) == EINVAL and b"null pointer" in L.lib().u3d_last_error()
        assert f(pooled=None) == EINVAL
        assert f(C=P.PS_CMAX + 1) == EINVAL
        assert f(S=P.PS_MAXS + 1) == EINVAL and b"samples" in L.lib().u3d_last_error()
    torch.cuda.synchronize()
    assert bool(torch.isnan(loss).all()) and bool(torch.isnan(dl).all())       # nothing was launched
    with pytest.raises(L.U3DError):
        from u3d import loss as UL
        UL.partial_loss(lg.permute(0, 2, 1).reshape(S, C, V, 1, 1), lab.reshape(S, V, 1, 1), w, uce=2)


# ------------------------------------------------------------------------------------------------ deep supervision
# id: (S, target extent, level extents)
DS_GEOM = {"D": (2, (16, 16, 16), DC.GEOM["D"][1]),
           "odd3": (3, (10, 6, 5), [(3, 2, 2), (5, 3, 3), (10, 6, 5)])}
DS_C = 14
DS_GO = 0.75


def _ds_inputs(name, kind):
    S, sp, levels = DS_GEOM[name]
    g = torch.Generator().manual_seed(900 + len(name))
    deep = [torch.randn((S, DS_C) + tuple(lv), generator=g) * 2 for lv in levels]
    target = torch.randint(0, DS_C, (S, 1) + tuple(sp), generator=g).float()
    kind = {"mixed": "mixed", "zero_row": "zero_row", "equal": "equal"}[kind]
    return deep, target, P.make_weights(kind, S, DS_C, seed=5)


def _ds_call(gpu, deep, target, w, ps):
    """The C entry points on NDHWC copies: (loss, level_loss, sums, pooled | None, dlogits [L] NDHWC)."""
    L = _L()
    lgs = [d.to(gpu).permute(0, 2, 3, 4, 1).contiguous() for d in deep]
    tgt = target.to(gpu)[:, 0].contiguous()
    S, (D, H, W), nl, C = tgt.shape[0], tgt.shape[1:], len(lgs), DS_C
    ptrs = (ctypes.c_void_p * nl)(*[t.data_ptr() for t in lgs])
    dims = (ctypes.c_int * (3 * nl))(*[int(n) for t in lgs for n in t.shape[1:4]])
    lw = (ctypes.c_float * nl)(*DC.LEVEL_WEIGHTS[:nl])
    dw = w.to(gpu).contiguous()
    level_loss, loss = _nan((nl,), f32, gpu), _nan((1,), f32, gpu)
    go = torch.tensor([DS_GO], dtype=f32, device=gpu)
    dls = [_nan(tuple(t.shape), f32, gpu) for t in lgs]
    dptrs = (ctypes.c_void_p * nl)(*[t.data_ptr() for t in dls])
    if ps:
        nbytes = L.query("u3d_deepsup_loss_ps_workspace_bytes", nl, C, S)
        assert nbytes == S * nl * 256 * 3 * C * 4
        ws, check = _ws(nbytes, gpu)
        sums, pooled = _nan((nl, S, C, 4), f64, gpu), _nan((nl, C, 5), f64, gpu)
        L.call("u3d_deepsup_loss_ps_fwd", nl, ptrs, dims, lw, tgt.data_ptr(), S, D, H, W, C, dw.data_ptr(),
               sums.data_ptr(), pooled.data_ptr(), level_loss.data_ptr(), loss.data_ptr(), ws.data_ptr(), _stream())
        torch.cuda.synchronize()
        check()
        L.call("u3d_deepsup_loss_ps_bwd", nl, ptrs, dims, lw, tgt.data_ptr(), S, D, H, W, C, dw.data_ptr(),
               pooled.data_ptr(), go.data_ptr(), dptrs, _stream())
    else:
        ws, check = _ws(L.query("u3d_deepsup_loss_workspace_bytes", nl, C), gpu)
        sums, pooled = _nan((nl, C, 4), f64, gpu), None
        L.call("u3d_deepsup_loss_fwd", nl, ptrs, dims, lw, tgt.data_ptr(), S, D, H, W, C, dw.data_ptr(),
               sums.data_ptr(), level_loss.data_ptr(), loss.data_ptr(), ws.data_ptr(), _stream())
        torch.cuda.synchronize()
        check()
        L.call("u3d_deepsup_loss_bwd", nl, ptrs, dims, lw, tgt.data_ptr(), S, D, H, W, C, dw.data_ptr(),
               sums.data_ptr(), go.data_ptr(), dptrs, _stream())
    torch.cuda.synchronize()
    return loss, level_loss, sums, pooled, dls


@pytest.mark.parametrize("kind", ["mixed", "zero_row", "equal"])
@pytest.mark.parametrize("name", sorted(DS_GEOM))
def test_deepsup_ps(gpu, name, kind):
    deep, target, w = _ds_inputs(name, kind)
    S = target.shape[0]
    nl = len(deep)
    ref_loss, ref_levels, ref_grads, f = PR.deepsup_ps_loss(deep, target, w, DC.LEVEL_WEIGHTS[:nl], grad_out=DS_GO)
    loss, level_loss, sums, pooled, dls = _ds_call(gpu, deep, target, w, ps=True)
    tag = f"{name} {kind}"
    for l in range(nl):
        rs, rp = f.sums_ps[l], f.pooled[l]
        assert _share(f"ds-ps-sums {tag} level {l}", (sums[l].cpu() - rs).abs(), 2.0 ** -16 * rs.abs()) <= 1
        assert _share(f"ds-ps-pooled {tag} level {l}", (pooled[l].cpu()[:, :4] - rp[:, :4]).abs(),
                      2.0 ** -16 * rp[:, :4].abs()) <= 1
        assert torch.equal(pooled[l].cpu()[:, 4], rp[:, 4])
        assert _share(f"ds-ps-level {tag} level {l}", (level_loss[l].double().cpu() - ref_levels[l]).abs().reshape(1),
                      2.0 ** -15 * ref_levels[l].abs().reshape(1)) <= 1
    assert _share(f"ds-ps-loss {tag}", (loss.double().cpu() - ref_loss).abs().reshape(1),
                  2.0 ** -15 * ref_loss.abs().reshape(1)) <= 1
    for l, (dl, rg) in enumerate(zip(dls, ref_grads)):
        got = dl.permute(0, 4, 1, 2, 3).cpu().double().numpy()
        assert np.isfinite(got).all()
        r = rg.numpy()
        print(f"{tag} level {l}: max|err| {np.abs(got - r).max():.3e}  max|ref| {np.abs(r).max():.3e}")
        np.testing.assert_allclose(got, r, rtol=1e-3, atol=1e-4 * np.abs(r).max(), err_msg=f"{tag} level {l}")
        if kind == "zero_row":
            assert bool((dl[S - 1].view(torch.int32) == 0).all()), "the zero row's dlogits must be bitwise 0"
            assert bool((dl[0] != 0).any())
    if kind == "equal":      # against the existing entry points with the one row
        loss_b, level_b, sums_b, _, dls_b = _ds_call(gpu, deep, target, w[0], ps=False)
        np.testing.assert_allclose(loss.item(), loss_b.item(), rtol=1e-5)
        np.testing.assert_allclose(level_loss.cpu().numpy(), level_b.cpu().numpy(), rtol=1e-5)
        keep = (w[0] != 0).double()[None, :, None]
        np.testing.assert_allclose(pooled.cpu()[:, :, :4].numpy(), (keep * sums_b.cpu()).numpy(), rtol=1e-5)
        for l, (a, b) in enumerate(zip(dls, dls_b)):
            a, b = a.cpu().double().numpy(), b.cpu().double().numpy()
            np.testing.assert_allclose(a, b, rtol=1e-4, atol=1e-6 * np.abs(b).max(), err_msg=f"{tag} level {l}")


def test_deepsup_ps_python_entry(gpu):
    """u3d.loss.deep_supervision_loss(per_sample=True) and get_loss's deep_out term: the C call's values, NCDHW views of
    NDHWC gradients."""
    from u3d.loss import deep_supervision_loss
    deep, target, w = _ds_inputs("D", "mixed")
    xs = [d.to(gpu).requires_grad_(True) for d in deep]
    loss = deep_supervision_loss(xs, target.to(gpu), [r for r in w.to(gpu)], per_sample=True)
    grads = torch.autograd.grad(loss * DS_GO, xs)
    want_loss, _, _, _, want = _ds_call(gpu, deep, target, w, ps=True)
    assert torch.equal(loss.reshape(1), want_loss)
    for g_, dl in zip(grads, want):
        assert torch.equal(g_.permute(0, 2, 3, 4, 1), dl)
    with pytest.raises(ValueError):
        deep_supervision_loss(xs, target.to(gpu), [w[0].to(gpu)], per_sample=True)


# ------------------------------------------------------------------------------------------------ wiring
def _model(gpu, seed=0):
    import unet3D
    torch.manual_seed(seed)
    return unet3D.unet3D_baseline([1, 2, 2, 2, 2], 16, True).to(gpu).train()


def _batch(gpu, seed=5, s=16):
    g = torch.Generator().manual_seed(seed)
    x = (torch.rand((2, 1, s, s, s), generator=g) * 2 - 1).to(gpu)
    lab = torch.randint(0, 16, (2, 1, s, s, s), generator=g).float().to(gpu)
    rows = (torch.rand(2, 16, generator=g) < 0.6).long()
    rows[0, 0], rows[1, 0], rows[0, 2], rows[1, 2] = 1, 1, 1, 0
    return x, lab, rows.to(gpu)


def test_module_gradient_is_formed_by_the_ps_kernel(gpu):
    from loss_functions.loss_partial import EDiceLoss_partial
    from u3d import ops
    from u3d.loss import DeferredLossGrad, ndhwc_view, sample_weights
    m = _model(gpu, 1)
    x, lab, rows = _batch(gpu)
    assert not torch.equal(rows[0], rows[1])
    lg, _, _ = m(x)
    loss = EDiceLoss_partial(16, per_sample=True)(lg, lab[:, 0], mask=[rows[0], rows[1]])
    (gl,) = torch.autograd.grad(loss, lg)
    assert type(gl) is torch.Tensor and not isinstance(gl, DeferredLossGrad)
    lgv = ndhwc_view(lg.detach())
    w = sample_weights(rows, 2, 16, gpu)
    want_loss, _, pooled = ops.partial_loss_ps_fwd(lgv, lab[:, 0].contiguous(), w, True, True)
    ref = ops.partial_loss_ps_bwd(lgv, lab[:, 0].contiguous(), w, pooled, torch.ones(1, device=gpu), True, True)
    assert torch.equal(loss.reshape(1), want_loss)
    assert torch.equal(gl.permute(0, 2, 3, 4, 1), ref)


def _engine(monkeypatch):
    import engine
    monkeypatch.setattr(sys, "argv", ["x"])
    return engine.Engine(custom_parser=argparse.ArgumentParser())


def test_engine_train_step_per_sample(gpu, monkeypatch):
    e = _engine(monkeypatch)
    m = _model(gpu)
    opt = torch.optim.SGD(m.parameters(), lr=1e-2, momentum=0.9)
    x, lab, rows = _batch(gpu)
    before = [p.detach().clone() for p in m.parameters()]
    loss = e.train_step(m, opt, x, lab, [rows[0], rows[1]], per_sample=True)
    torch.cuda.synchronize()
    assert bool(torch.isfinite(loss)) and loss.item() > 0
    assert any(not torch.equal(a, b) for a, b in zip(before, m.parameters()))
    with pytest.raises(ValueError):
        e.train_step(m, opt, x, lab, [rows[0]], per_sample=True)


def test_graphed_step_per_sample_with_device_mask(gpu, monkeypatch):
    from u3d.graph import GraphedStep
    e = _engine(monkeypatch)
    batches = [_batch(gpu, seed) for seed in (5, 6, 7)]

    def run(graphed):
        m = _model(gpu)
        opt = torch.optim.SGD(m.parameters(), lr=1e-2, momentum=0.9)
        x, lab, rows = (t.clone() for t in batches[0])

        def step():
            return e.train_step(m, opt, x, lab, rows, per_sample=True)
        losses = []
        if graphed:
            g = GraphedStep(step, (x, lab, rows), warmup=2, optimizer=opt)
            for b in batches[1:]:
                losses.append(g(*b).item())
        else:
            for _ in range(2):
                step()
            for b in batches[1:]:
                for dst, src in zip((x, lab, rows), b):
                    dst.copy_(src)
                losses.append(step().item())
        torch.cuda.synchronize()
        return losses

    eager, replay = run(False), run(True)
    assert all(np.isfinite(v) for v in replay)
    assert replay == pytest.approx(eager, rel=1e-6, abs=1e-7)
