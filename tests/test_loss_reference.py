"""loss_reference.py pinned to what already exists, on the CPU: its values against oracle.ref_cpu (edice_partial,
edice_full, edice_full2, get_loss_consistency minus its edice_partial term, get_dice, get_dice2, partial_target), its
gradients against torch's autograd of the same restatement in fp64, and the input conditions of every case of
test_gpu_loss.py (loss_cases.py), so that a GPU case cannot hide an error behind its own inputs:

  * regular-regime logits keep every bound tight: each Dice-sum and BCE-sum bound is at most 2^-12 of the abs-sum it
    covers, and so is the loss's; a gradient element's own relative error grows like 1 / (1 - p) in any fp32 evaluation
    of BCE on a softmax, so the gradient bounds are measured in aggregate, sum of bounds against the sum of the
    abs-sums of the terms (loss_cases.grad_magnitude). The class that the "absent" cases remove has sums ~ 1e-13 per
    voxel by construction; its BCE sum is exempt and the loss's bound carries it.
  * saturated cases: the leading gap is 40..85 or above 105 in every voxel, every class leads somewhere as a hit and
    as a non-hit, fp32 p == 1 and p == 0 occur, and both clamps (-100, 1e-12) are active;
  * Dice-metric logits are multiples of 1/8 (equal or at least 1/8 apart within a voxel), with ties present;
  * the consistency refiner's 2-class softmax stays 2^-10 away from confi and 1 - confi in every voxel.
"""
import numpy as np
import pytest
import torch

import oracle.ref_cpu as O
import loss_cases as K
import loss_reference as R

F64 = torch.float64


def _close(a, b, tol, what=""):
    a, b = torch.as_tensor(a, dtype=F64), torch.as_tensor(b, dtype=F64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    err = (a - b).abs().max().item() if a.numel() else 0.0
    assert err <= tol * max(1.0, b.abs().max().item() if b.numel() else 1.0), (what, err)


# ------------------------------------------------------------------------------------------------ values vs the oracle
@pytest.mark.parametrize("C", [2, 5, 16])
@pytest.mark.parametrize("mode,uce", [(K.SOFT, 0), (K.SOFT, 1), (K.SIG, 0), (K.SIG, 1)])
def test_partial_loss_matches_oracle(C, mode, uce):
    S, D, H, W = 2, 3, 4, 5
    lg, lab, w = K.loss_inputs((S, D * H * W, C, mode, uce, "reg"))
    ref = R.partial_loss_ref(lg, lab, w, mode, uce)
    x = lg.reshape(S, D, H, W, C).permute(0, 4, 1, 2, 3).double()
    want = O.edice_partial(x, lab.reshape(S, D, H, W).double(), mask=[w.double()], soft_max=mode == K.SOFT, uce=bool(uce))
    _close(ref.loss, want, 1e-5, "edice_partial")          # the oracle's BCE runs on fp32 probabilities


@pytest.mark.parametrize("C", [2, 14])
@pytest.mark.parametrize("mode,uce", [(K.SOFT, 2), (K.SOFT, 0), (K.SIG, 0)])
def test_full_loss_matches_oracle(C, mode, uce):
    S, D, H, W = 2, 3, 4, 5
    lg, lab, _ = K.loss_inputs((S, D * H * W, C, mode, uce, "reg"))
    lab = lab.round().clamp(0, C - 1)                      # nn.CrossEntropyLoss wants class indices
    ref = R.partial_loss_ref(lg, lab, torch.ones(C), mode, uce)
    x = lg.reshape(S, D, H, W, C).permute(0, 4, 1, 2, 3).double()
    want = O.edice_full(x, lab.reshape(S, D, H, W), logits="softmax" if mode == K.SOFT else "sigmoid", uce=uce == 2)
    _close(ref.loss, want, 1e-5, "edice_full")


@pytest.mark.parametrize("case", [(2, 60, 5, 4), (3, 257, 14, 13), (1, 257, 2, 1)], ids=K.case_id)
def test_dice_metric_matches_oracle(case):
    S, V, C, ncls = case
    lg, lab = K.dice_inputs(case)
    ref = R.dice_metric_ref(lg, lab, ncls)
    d, se, sp = O.get_dice(lg.permute(0, 2, 1).reshape(S, C, V, 1, 1).double(), lab.reshape(S, V, 1, 1), num_class=ncls)
    _close(ref.metrics, np.stack([d, se, sp], 1), 1e-12, "get_dice")


@pytest.mark.parametrize("case", K.DICE2_CASES[:3], ids=K.case_id)
def test_dice_binary_matches_oracle(case):
    nt, V = case
    ref_l, lab = K.dice2_inputs(case)
    ref = R.dice_binary_ref(ref_l, 2 * V, V, 1, nt, V, lab)
    d, se, sp, am = O.get_dice2(ref_l.reshape(nt, 2, V, 1, 1).double(), lab.reshape(1, V, 1, 1), num_class=nt)
    _close(ref.metrics, np.stack([d, se, sp], 1), 1e-12, "get_dice2")
    assert torch.equal(ref.argmax, am.reshape(nt, V))
    ndhwc = ref_l.permute(0, 2, 1).contiguous()            # the same values behind the other layout's strides
    alt = R.dice_binary_ref(ndhwc, 2 * V, 1, 2, nt, V, lab)
    assert torch.equal(alt.counts, ref.counts) and torch.equal(alt.argmax, ref.argmax)


def test_partial_target_matches_oracle():
    case = (3, 257, 14, 14, 1, 13)
    lab, mask = K.pt_inputs(case)
    got = R.partial_target_ref(lab, mask, 14, 14, 1, 13)
    for s in range(3):
        assert np.array_equal(got[s].numpy(), O.partial_target(lab[s].numpy(), mask[s].numpy()))
    one = R.partial_target_ref(lab, mask[:1].contiguous(), 0, 14, 1, 13)
    for s in range(3):
        assert np.array_equal(one[s].numpy(), O.partial_target(lab[s].numpy(), mask[0].numpy()))
    assert not torch.equal(got, lab)


def _consist_split(case):
    lg, rf, atts, lt = K.consist_inputs(case)
    return lg, rf[:, :, 0].contiguous(), rf[:, :, 1].contiguous(), atts, lt


@pytest.mark.parametrize("case", [c for c in K.CONSIST_CASES if c[0] == 300 and c[2] == c[1] - 1 and c[4] != "all"],
                         ids=K.case_id)
def test_consistency_matches_oracle(case):
    V, C, nt, natt, _ = case
    lg, r0, r1, atts, lt = _consist_split(case)
    ref = R.consistency_ref(atts, lg, r0, r1, lt, K.CONFI, K.WF)
    sp = (V, 1, 1)
    out = lg.t().reshape(1, C, *sp).double()
    tgt = torch.zeros(1, 1, *sp, dtype=F64)
    rfo = torch.stack([r0, r1], 1).reshape(nt, 2, *sp).double()
    aa = [a.reshape(1, nt, *sp).double() for a in atts]
    full = O.get_loss_consistency(out, tgt, None, aa, rfo, lt.tolist(), confi_=K.CONFI, weight_feature=K.WF)
    want = full - O.edice_partial(out, tgt.squeeze(1), mask=None)
    _close(ref.aux, want, 2e-6, "get_loss_consistency - edice_partial")   # fp32(0.1) weight, fp32 BCE in the oracle
    if natt < 3:       # the softmax map is map number natt: weights[natt] and a sigmoid, not weight 1 as is
        g = int((lt == 0).nonzero()[0])
        p1 = torch.softmax(rfo[g], 0)[1].reshape(-1)
        conf = ((p1 > 0.9) | (p1 < 0.1)).reshape(1, 1, *sp).double()
        s = torch.softmax(out, 1)[:, g + 1:g + 2]
        one = O.edice_full2(s, p1.reshape(1, *sp), uce=False, sigmoid=True, mask=conf)
        _close(ref.dice[g, 3], one, 1e-6, "softmax map through a sigmoid")
        assert abs(ref.c[g, 3].item() - R.CONSIST_W[natt] * R.f32(K.WF) / (nt - ref.sup)) < 1e-15


@pytest.mark.parametrize("case", [(257, sg, uce, m) for sg in (0, 1) for uce in (0, 1) for m in ("null", "some")],
                         ids=K.case_id)
def test_full2_matches_oracle(case):
    V, sg, uce, _ = case
    x, t, m = K.full2_inputs(case)
    ref = R.full2_ref(x, t, m, sg, uce)
    want = O.edice_full2(x.reshape(1, 1, V).double(), t.reshape(1, V).double(), uce=bool(uce),
                         mask=None if m is None else m.reshape(1, 1, V), sigmoid=bool(sg))
    _close(ref.loss, want, 1e-6, "edice_full2")


# ------------------------------------------------------------------------------------------------ gradients vs autograd
@pytest.mark.parametrize("C", [2, 5])
@pytest.mark.parametrize("mode,uce", K.MODES)
def test_partial_loss_grad_matches_autograd(C, mode, uce):
    lg, lab, w = K.loss_inputs((1, 257, C, mode, uce, "reg"))
    ref = R.partial_loss_ref(lg, lab, w, mode, uce, grad_out=K.GRAD_OUT)
    leaf = lg.double().requires_grad_(True)
    (R.partial_loss_value(leaf, lab, w, mode, uce).loss * K.GRAD_OUT).backward()
    assert (ref.dl - leaf.grad).abs().max().item() <= 1e-12 * leaf.grad.abs().max().item()


@pytest.mark.parametrize("natt", [0, 1, 2, 3])
def test_consistency_grad_matches_autograd(natt):
    lg, r0, r1, atts, lt = _consist_split((300, 14, 13, natt, "mixed"))
    ref = R.consistency_ref(atts, lg, r0, r1, lt, K.CONFI, K.WF, grad_out=K.GRAD_OUT)
    leaves = [a.double().requires_grad_(True) for a in atts]
    ll = lg.double().requires_grad_(True)
    (R.consistency_value(leaves, ll, r0.double(), r1.double(), lt, K.CONFI, K.WF).aux * K.GRAD_OUT).backward()
    for got, leaf in zip(ref.datt + [ref.dl], leaves + [ll]):
        assert (got - leaf.grad).abs().max().item() <= 1e-12 * leaf.grad.abs().max().item()


@pytest.mark.parametrize("case", [(257, sg, uce, m) for sg in (0, 1) for uce in (0, 1) for m in ("null", "some")],
                         ids=K.case_id)
def test_full2_grad_matches_autograd(case):
    V, sg, uce, _ = case
    x, t, m = K.full2_inputs(case)
    ref = R.full2_ref(x, t, m, sg, uce, grad_out=K.GRAD_OUT)
    leaf = x.double().requires_grad_(True)
    (R.full2_value(leaf, t.double(), None if m is None else m.double(), sg, uce).loss * K.GRAD_OUT).backward()
    assert (ref.dx - leaf.grad).abs().max().item() <= 1e-12 * leaf.grad.abs().max().item()


# ------------------------------------------------------------------------------------------------ conditions
def _tight(bound, mag, what):
    ok = bound <= K.TIGHT * mag
    assert bool(ok.all()), (what, (bound / mag.clamp(min=1e-300))[~ok].max().item())


def _loss_conditions(case, bf16=False):
    S, V, C, mode, uce, kind = case[:6]
    nvox = S * V
    lg, lab, w = K.loss_inputs(case[:6])
    assert lg.shape == (nvox, C) and lab.shape == (nvox,)
    ref = R.partial_loss_ref(lg, lab, w, mode, uce, grad_out=K.GRAD_OUT)
    if nvox >= 5:
        assert (lab >= C).any() and (lab < 0).any() and (lab != lab.round()).any()
    assert kind == "zero_w" or ((w == 0).any() and (w > 0).any())
    bs, bl, _ = K.loss_fwd_bounds(ref, w, mode, uce, nvox, pair=C == 16 and mode == K.SOFT and uce == 1)
    keep = torch.ones(C, dtype=torch.bool)
    if kind == "absent":
        assert ref.sums[C - 1, 2] == 0 and ref.sums[C - 1, 1] < 1e-20 * nvox
        assert abs((ref.sums[C - 1, 1] + ref.sums[C - 1, 2] + 1e-5) / 1e-5 - 1) < 1e-6      # den ~ 1e-5
        keep[C - 1] = False
    if nvox >= 255:      # (a class's sums over one or five voxels can be all but empty: there the loss's bound speaks)
        _tight(bs[:, 0], ref.sums[:, 0], "I")
        _tight(bs[:, 1][keep], ref.sums[:, 1][keep], "Z")
        _tight(bs[:, 3][keep], ref.bce_abs[keep], "BCE")
    if kind == "zero_w":
        assert ref.loss == 0 and bl == 0
    else:
        _tight(bl.reshape(1), ref.loss.abs().reshape(1), "loss")
        br = K.loss_bwd_bounds(ref, mode, uce)
        _tight(br.sum().reshape(1), K.grad_magnitude(ref, mode).sum().reshape(1), "gradient")
        assert bool(torch.isfinite(br).all())
    return ref


@pytest.mark.parametrize("C", K.CLASSES)
@pytest.mark.parametrize("mode,uce", K.MODES)
def test_small_loss_case_conditions(C, mode, uce):
    for case in K.LOSS_SMALL:
        if case[2:5] == (C, mode, uce):
            _loss_conditions(case)


@pytest.mark.parametrize("case", K.LOSS_SPECIAL + K.LOSS_FWD_MULTI + K.LOSS_BWD_MULTI, ids=K.case_id)
def test_large_loss_case_conditions(case):
    _loss_conditions(case)


@pytest.mark.parametrize("case", K.LOSS_SAT, ids=K.case_id)
def test_saturated_case_conditions(case):
    S, V, C = case
    lg, lab, w, lead = K.sat_inputs(case)
    top2 = lg.double().topk(2, 1).values
    gap = top2[:, 0] - top2[:, 1]
    assert gap.min() >= 40 and not ((gap > 85) & (gap < 105)).any() and gap[7] > 110
    assert torch.exp(-gap).max() * C < 2.0 ** -26            # fp32: s == e_lead == 1, so s - e_lead == 0 exactly
    ref = R.partial_loss_ref(lg, lab, w, K.SOFT, 1, grad_out=K.GRAD_OUT, round_p_to_fp32=True)
    exact = R.partial_loss_ref(lg, lab, w, K.SOFT, 1)
    p = ref.pr.p
    idx = torch.arange(S * V)
    assert (p[idx, lead] == 1).all() and (p[7].sum() == 1)
    for c in range(C):                                       # every class leads as a hit and as a non-hit
        assert ((lead == c) & (lab == c)).any() and ((lead == c) & (lab != c)).any()
    lead_nonhit = lab != lead.float()
    assert (ref.bce[idx, lead][lead_nonhit] == 100).all()    # the -100 clamp where fp32 has p == 1 ...
    assert (exact.bce[idx, lead][lead_nonhit & (gap < 85)] < 90).all()   # ... which the exact probabilities do not reach
    assert (ref.bce[7] == 100).sum() >= 1
    assert ((ref.pr.q * p) < 1e-12).all()                    # the 1e-12 clamp is active everywhere
    assert bool(torch.isfinite(ref.dl).all()) and bool(torch.isfinite(ref.loss))
    bs, bl, _ = K.loss_fwd_bounds(ref, w, K.SOFT, 1, S * V, pair=C == 16, round_p=True)
    assert bool(torch.isfinite(bs).all()) and bool(torch.isfinite(bl))
    assert bool(torch.isfinite(K.loss_bwd_bounds(ref, K.SOFT, 1, round_p=True)).all())


@pytest.mark.parametrize("case", K.DICE_CASES, ids=K.case_id)
def test_dice_case_conditions(case):
    S, V, C, ncls = case
    lg, lab = K.dice_inputs(case)
    assert lg.shape == (S, V, C) and torch.equal(lg * 8, (lg * 8).round()) and lg.abs().max() <= 5
    srt = lg.sort(2).values
    d = srt[..., 1:] - srt[..., :-1]
    assert bool(((d == 0) | (d >= 0.125)).all())
    if V >= 3:
        top2 = lg.topk(2, 2).values
        assert (top2[..., 0] == top2[..., 1]).any()          # deliberate ties at the maximum
    if V >= 5:
        assert (lab > ncls).any() and (lab != lab.round()).any() and (lab < 0).any()
    assert ncls <= C - 1
    ref = R.dice_metric_ref(lg, lab, ncls)
    assert V < 255 or ref.counts[..., 0].sum() > 0


@pytest.mark.parametrize("case", K.DICE2_CASES, ids=K.case_id)
def test_dice_binary_case_conditions(case):
    nt, V = case
    rf, lab = K.dice2_inputs(case)
    assert torch.equal(rf * 8, (rf * 8).round())
    gap = (rf[:, 1] - rf[:, 0]).abs()
    assert bool(((gap == 0) | (gap >= 0.125)).all()) and (V < 4 or (gap == 0).any())


@pytest.mark.parametrize("case", K.PT_CASES, ids=K.case_id)
def test_partial_target_case_conditions(case):
    S, V, M, stride, lmin, lmax = case
    lab, mask = K.pt_inputs(case)
    out = R.partial_target_ref(lab, mask, stride, M, lmin, lmax)
    assert V == 1 or not torch.equal(out, lab)
    keep = (lab < lmin) | (lab > min(lmax, M - 1)) | (lab != lab.round())
    assert torch.equal(out[keep], lab[keep])                 # labels outside the range or non-integer pass through


@pytest.mark.parametrize("case", K.CONSIST_CASES + K.CONSIST_BWD_EXTRA, ids=K.case_id)
def test_consistency_case_conditions(case):
    V, C, nt, natt, pattern = case
    lg, r0, r1, atts, lt = _consist_split(case)
    assert torch.equal(r0 * 4, (r0 * 4).round()) and torch.equal(r1 * 4, (r1 * 4).round())
    ref = R.consistency_ref(atts, lg, r0, r1, lt, K.CONFI, K.WF, grad_out=K.GRAD_OUT)
    for thr in (K.CONFI, 1 - K.CONFI):
        assert ((ref.t - thr).abs() >= 2.0 ** -10).all()     # the mask is the same in fp32 and fp64
    if pattern == "all":
        assert ref.sup == nt and ref.aux == 0 and (ref.coef == 0).all() and (ref.dl == 0).all()
        return
    assert ref.sup < nt and (V < 300 or ref.aux > 0)
    un = [g for g in range(nt) if lt[g] == 0]
    if len(un) >= 2:                                         # one organ without a confident voxel: d = 0
        assert ref.on[un[-1]].sum() == 0 and (ref.dice[un[-1]] == 0).all()
    if V >= 300:
        assert ref.on[un[0]].sum() > 0 and (ref.on[un[0]] == 0).any()
    b_dice, b_coef, b_aux = K.consist_fwd_bounds(ref, [a.double() for a in atts], lg.double(), r0.double(), r1.double(), V)
    if V >= 300:
        _tight(b_aux.reshape(1), ref.aux.abs().reshape(1), "aux")
    b_att, b_dl = K.consist_bwd_bounds(ref, [a.double() for a in atts], lg.double(), r0.double(), r1.double(), K.GRAD_OUT)
    assert all(bool(torch.isfinite(b).all()) for b in b_att + [b_dl, b_dice, b_coef])


@pytest.mark.parametrize("case", K.FULL2_CASES, ids=K.case_id)
def test_full2_case_conditions(case):
    V, sg, uce, mk = case
    x, t, m = K.full2_inputs(case)
    assert V < 5 or not sg or x.abs().max() == 30
    assert (t >= 0).all() and (t <= 1).all()
    ref = R.full2_ref(x, t, m, sg, uce, grad_out=K.GRAD_OUT)
    if mk == "zeros":
        assert ref.I == 0 and ref.Z == 0 and ref.Y == 0
    bl, b_coef = K.full2_fwd_bounds(ref, x, t, sg, uce, V)
    assert bool(torch.isfinite(bl)) and bool(torch.isfinite(b_coef).all())
    if V >= 257 and (uce or mk != "zeros"):
        _tight(bl.reshape(1), ref.loss.abs().reshape(1), "full2 loss")
    assert bool(torch.isfinite(K.full2_bwd_bounds(ref, x, t, sg, K.GRAD_OUT, ref.coef)).all())
