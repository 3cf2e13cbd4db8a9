"""loss_ps_reference.py (the fp64 restatement the per-sample loss kernels are held to) pinned on the CPU: its gradient
against torch's autograd of its own forward, equal rows against loss_reference.partial_loss_ref, the zero-row, all-zero
and single-supervisor properties, the deep-supervision form against deepsup_reference; and the host side of the
feature: u3d.loss.sample_weights, the per_sample keyword of the loss modules, get_loss and Engine.train_step, the input
conditions of loss_ps_cases.py."""
import inspect

import pytest
import torch

import deepsup_reference as DR
import loss_cases as K
import loss_ps_cases as P
import loss_ps_reference as PR
import loss_reference as R
from loss_cases import IDENT, SIG, SOFT

F64 = torch.float64
CASES = [(S, V, C, m, u, kind) for (S, V) in [(2, 5), (3, 257)] for C in (2, 5, 16) for (m, u) in P.MODES
         for kind in P.KINDS if (S, V) == (3, 257) or kind == "mixed"]


def _autograd(lg, lab, w, mode, uce, go):
    x = lg.double().requires_grad_(True)
    f = PR.partial_loss_ps_value(x, lab, w, mode, uce)
    (g,) = torch.autograd.grad(f.loss * go, x)
    return g.reshape(-1, lg.shape[2])


@pytest.mark.parametrize("case", CASES, ids=P.case_id)
def test_reference_gradient_is_autograd_of_its_forward(case):
    S, V, C, mode, uce, kind = case
    lg, lab, w = P.ps_inputs(case)
    ref = PR.partial_loss_ps_ref(lg, lab, w, mode, uce, grad_out=K.GRAD_OUT)
    want = _autograd(lg, lab, w, mode, uce, K.GRAD_OUT)
    scale = want.abs().max().item() + 1e-300
    assert (ref.dl - want).abs().max().item() <= 1e-11 * max(scale, 1e-6)
    if kind == "all_zero":
        assert ref.loss.item() == 0.0 and not bool(ref.dl.any())


@pytest.mark.parametrize("mode,uce", P.MODES, ids=str)
@pytest.mark.parametrize("S,V,C", [(1, 257, 5), (3, 257, 16), (2, 693, 14)])
def test_equal_rows_are_the_batch_loss(S, V, C, mode, uce):
    """Float weights with zeros, the same row for every sample: value, sums and dl of loss_reference.partial_loss_ref."""
    lg, lab, w = P.ps_inputs((S, V, C, mode, uce, "equal"))
    assert bool((w[0] == 0).any()) and bool((w[0] != 0).any()) and bool((w == w[0]).all())
    ref = PR.partial_loss_ps_ref(lg, lab, w, mode, uce, grad_out=K.GRAD_OUT)
    want = R.partial_loss_ref(lg.reshape(S * V, C), lab.reshape(-1), w[0], mode, uce, grad_out=K.GRAD_OUT)
    rnd = 64 * 2.0 ** -53
    assert abs(ref.loss.item() - want.loss.item()) <= rnd * abs(want.loss.item())
    keep = (w[0] != 0).double()[:, None]
    assert bool(((ref.pooled[:, :4] - keep * want.sums).abs() <= rnd * want.sums.abs()).all())
    assert bool(((ref.sums_ps.sum(0) - want.sums).abs() <= rnd * want.sums.abs()).all())
    assert bool(((ref.dl - want.dl).abs() <= rnd * K.grad_magnitude(want, mode)).all())


@pytest.mark.parametrize("mode,uce", [(SOFT, 1), (SIG, 1), (IDENT, 0)], ids=str)
def test_zero_row_all_zero_and_single_supervisor(mode, uce):
    S, V, C = 3, 257, 8
    lg, lab, w = P.ps_inputs((S, V, C, mode, uce, "zero_row"))
    assert not bool(w[S - 1].any()) and bool(w[:S - 1].any(1).all())
    ref = PR.partial_loss_ps_ref(lg, lab, w, mode, uce, grad_out=K.GRAD_OUT)
    assert not bool(ref.dl[(S - 1) * V:].any()) and bool(ref.dl[:(S - 1) * V].any())
    # the zero row enters no pooled sum: dropping the sample changes nothing
    two = PR.partial_loss_ps_ref(lg[:S - 1], lab[:S - 1], w[:S - 1], mode, uce, grad_out=K.GRAD_OUT)
    assert abs(two.loss.item() - ref.loss.item()) <= 1e-14 and torch.equal(two.pooled, ref.pooled)
    assert (two.dl - ref.dl[:(S - 1) * V]).abs().max().item() <= 1e-15
    # all rows zero
    zero = PR.partial_loss_ps_ref(lg, lab, torch.zeros(S, C), mode, uce, grad_out=K.GRAD_OUT)
    assert zero.loss.item() == 0.0 and not bool(zero.dl.any()) and not bool(zero.pooled.any())
    # single supervisor: class c's terms are those of its one sample alone, the BCE mean over V
    lg, lab, w = P.ps_inputs((S, V, C, mode, uce, "disjoint"))
    ref = PR.partial_loss_ps_ref(lg, lab, w, mode, uce, grad_out=K.GRAD_OUT)
    assert bool((ref.n == 1).all())
    total = 0.0
    for s in range(S):
        one = R.partial_loss_ref(lg[s], lab[s], w[s], mode, uce, grad_out=K.GRAD_OUT)     # nvox = V, weights 0 elsewhere
        total += one.loss.item()
        own = w[s] != 0
        assert bool(((ref.pooled[own, :4] - one.sums[own]).abs() <= 1e-12 * one.sums[own].abs()).all())
        assert (ref.dl[s * V:(s + 1) * V] - one.dl).abs().max().item() <= 1e-14
    assert abs(total - ref.loss.item()) <= 1e-13


def test_deepsup_reference_equal_rows_and_autograd():
    g = torch.Generator().manual_seed(3)
    S, C, sp, levels = 3, 14, (10, 6, 5), [(3, 2, 2), (5, 3, 3), (10, 6, 5)]
    deep = [torch.randn((S, C) + lv, generator=g) * 2 for lv in levels]
    target = torch.randint(0, C, (S, 1) + sp, generator=g).float()
    w = P.make_weights("equal", S, C)
    loss, levels_, grads, f = PR.deepsup_ps_loss(deep, target, w)
    want_loss, want_levels, want_grads = DR.deepsup_loss(deep, target, w[0].double(), (0.125, 0.25, 0.5))
    assert abs(loss.item() - want_loss.item()) <= 1e-13
    for a, b in zip(grads, want_grads):
        assert (a - b).abs().max().item() <= 1e-14
    w = P.make_weights("zero_row", S, C)
    loss, _, grads, f = PR.deepsup_ps_loss(deep, target, w)
    assert all(not bool(gr[S - 1].any()) and bool(gr[0].any()) for gr in grads)
    assert all(torch.equal(p[:, 4], (w != 0).double().sum(0)) for p in f.pooled)


def test_cases_cover_what_they_claim():
    for kind in P.KINDS:
        for S, C in [(2, 2), (3, 5), (2, 16), (3, 32)]:
            w = P.make_weights(kind, S, C)
            n = (w != 0).sum(0)
            assert w.shape == (S, C) and w.dtype == torch.float32
            if kind == "mixed":
                assert not bool((w == w[0]).all()) and bool((w == 0).any()) and bool(w.any(1).all())
                assert bool(((w == 0) | ((w >= 0.5) & (w <= 1.5))).all())
                assert C <= 3 or bool((n == 0).any())
            elif kind == "zero_row":
                assert not bool(w[S - 1].any()) and bool(w[:S - 1].any())
            elif kind == "all_zero":
                assert not bool(w.any())
            elif kind == "disjoint":
                assert bool((n == 1).all())
            else:
                assert bool((w == w[0]).all()) and bool((w[0] == 0).any()) and bool(w[0].any())
    # the multi-trip cases exceed one trip of the per-sample grid by 300 voxels
    for (S, V, C, mode, uce, _) in P.FWD_MULTI:
        vox = P.PAIR_VOX if P.is_pair(C, mode, uce) else P.PT
        assert V == P.fwd_blocks(S, V, C, mode, uce) * vox + 300
    assert P.is_pair(*P.FWD_MULTI[1][2:5]) and not P.is_pair(*P.FWD_MULTI[0][2:5])
    for (S, V, *_r) in P.BWD_MULTI:
        assert V == P.blocks(S, V, P.PS_BWD_NB, P.PT) * P.PT + 300
    assert len(P.CT_ROW) == 15 and sum(P.CT_ROW) == 1 and not any(P.MRI_ROW)


def test_sample_weights_shapes_and_errors():
    from u3d.loss import class_weights, sample_weights
    dev = torch.device("cpu")
    rows = [[1, 0, 1, 1, 0], torch.tensor([0, 0, 2, 0, 1])]
    w = sample_weights(rows, 2, 4, dev)
    assert w.shape == (2, 4) and w.dtype == torch.float32 and w.is_contiguous()
    assert w.tolist() == [[1, 0, 1, 1], [0, 0, 2, 0]]
    t = torch.tensor([[1, 0, 1, 1, 0], [0, 0, 2, 0, 1]])
    assert torch.equal(sample_weights(t, 2, 4, dev), w)
    assert torch.equal(sample_weights(t.float() * 0.5, 2, 5, dev), t.float() * 0.5)
    assert torch.equal(sample_weights(None, 3, 4, dev), torch.ones(3, 4))
    with pytest.raises(IndexError):
        sample_weights(rows, 2, 6, dev)
    with pytest.raises(IndexError):
        sample_weights(t, 2, 6, dev)
    with pytest.raises(ValueError):
        sample_weights(rows, 3, 4, dev)
    with pytest.raises(ValueError):
        sample_weights(t, 1, 4, dev)
    with pytest.raises(ValueError):
        sample_weights(t[0], 2, 4, dev)
    # class_weights is untouched: mask[0] only
    assert class_weights(rows, 4, dev).tolist() == [1, 0, 1, 1]


def test_per_sample_keyword_reaches_every_layer():
    import engine
    from loss_functions.loss_partial import DiceLoss, EDiceLoss_partial
    from loss_functions.losses import get_loss
    from u3d import _lib
    from u3d import loss as UL
    assert EDiceLoss_partial(16, per_sample=True).per_sample is True
    assert EDiceLoss_partial(16).per_sample is False
    for fn in (get_loss, UL.deep_supervision_loss, engine.Engine.train_step, DiceLoss.forward):
        assert inspect.signature(fn).parameters["per_sample"].default is False
    # accepted all the way down: what fails on CPU tensors is the device check, not the keyword or the mask's shape
    out, tgt = torch.zeros(2, 4, 2, 2, 2), torch.zeros(2, 1, 2, 2, 2)
    with pytest.raises(_lib.U3DError, match="ROCm device"):
        get_loss(out, 0, [], tgt, mask=[[1, 1, 0, 1], [0, 0, 0, 0]], per_sample=True)
    with pytest.raises(ValueError):
        get_loss(out, 0, [], tgt, mask=[[1, 1, 0, 1]], per_sample=True)
    for name in ("u3d_loss_ps_workspace_bytes", "u3d_partial_loss_ps_fwd", "u3d_partial_loss_ps_bwd",
                 "u3d_deepsup_loss_ps_workspace_bytes", "u3d_deepsup_loss_ps_fwd", "u3d_deepsup_loss_ps_bwd"):
        assert name in _lib.exported_symbols()
