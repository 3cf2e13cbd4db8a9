"""The fused multi-level deep-supervision loss (u3d.loss.deep_supervision_loss, csrc/deepsup.hip) and get_loss's
deep_out branch on the device.

Against the fp64 restatement (tests/deepsup_reference.py) and the reference's G16 outputs: value rtol 1e-4, gradients
rtol 1e-3 with atol 1e-4 * max|ref| (the G9 rule). Against the composed form (F.interpolate + partial_loss per level,
the same softmax and coefficient code): value rtol 1e-5, gradients rtol 1e-4. Layout, repeat and graph-replay
comparisons are bitwise."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import deepsup_cases as DC
import deepsup_reference as DR
from conftest import golden

pytestmark = pytest.mark.gpu

LW = DC.LEVEL_WEIGHTS
A_LV, B_LV, D_LV = (DC.GEOM[t][1] for t in "ABD")

# id: (C, S, target extent, level extents, mask kind, grad_out)
CASES = {
    "geomA_c14": (14, 1, (16, 16, 8), A_LV, "mix", 1.0),
    "geomB_c14_L4": (14, 1, (20, 12, 10), B_LV, "mix", 1.0),        # 105 and 300 voxels: no multiple of 256
    "geomD_c14_s2": (14, 2, (16, 16, 16), D_LV, "mix", 1.0),
    "c2_s2": (2, 2, (16, 16, 16), D_LV, "ones", 1.0),
    "c16_s1_L4": (16, 1, (20, 12, 10), B_LV, "mix", 1.0),
    "c16_s2_L1": (16, 2, (16, 16, 8), [(8, 8, 4)], "mix", 1.0),
    "c8_s2": (8, 2, (12, 10, 6), [(3, 5, 2), (12, 10, 6)], "mix", 1.0),
    "c5_generic": (5, 2, (10, 9, 7), [(3, 4, 2), (5, 9, 3)], "mix", 1.0),   # the C <= 32 fallback, odd extents
    "c32_generic": (32, 1, (8, 8, 8), [(4, 4, 4)], "mix", 1.0),
    "tiny_8_voxels_L1": (14, 1, (16, 16, 16), [(2, 2, 2)], "mix", 1.0),      # less than one wave
    "grad_out": (14, 2, (16, 16, 8), A_LV, "mix", -2.5),
    "zero_mask": (14, 1, (16, 16, 8), A_LV, "zero", 1.0),
    # more voxels in a level than one pass of the forward's (65536) and the backward's (524288) grids covers
    "grid_stride": (2, 1, (96, 96, 64), [(96, 96, 64), (12, 12, 8)], "ones", 1.0),
}


def _inputs(name):
    C, S, sp, levels, mk, go = CASES[name]
    g = torch.Generator().manual_seed(sorted(CASES).index(name) + 100)
    deep = [torch.randn((S, C) + tuple(lv), generator=g) * 2 for lv in levels]
    target = torch.randint(0, C, (S, 1) + tuple(sp), generator=g).float()
    if mk == "ones":
        mask = torch.ones(C, dtype=torch.long)
    elif mk == "zero":
        mask = torch.zeros(C, dtype=torch.long)
    else:
        mask = (torch.rand(C, generator=g) < 0.6).long()
        mask[0], mask[1] = 1, 0
    return deep, target, mask, go


_REF = {}


def _reference(name):
    """fp64 restatement of a case, computed once and shared."""
    if name not in _REF:
        deep, target, mask, go = _inputs(name)
        _REF[name] = DR.deepsup_loss(deep, target, mask.double(), LW[:len(deep)], grad_out=go)
    return _REF[name]


def _fused(deep, target, mask, gpu, go=1.0, ndhwc=False, level_weights=LW):
    from u3d.loss import deep_supervision_loss
    if ndhwc:   # NCDHW-shaped views over NDHWC storage, as the native heads return them
        xs = [d.to(gpu).permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3).requires_grad_(True) for d in deep]
    else:
        xs = [d.to(gpu).contiguous().requires_grad_(True) for d in deep]
    loss = deep_supervision_loss(xs, target.to(gpu), [mask.to(gpu)], level_weights)
    # autograd.grad hands back the operation's own gradient tensors (.grad of a leaf would be re-laid to the leaf)
    return loss.detach(), list(torch.autograd.grad(loss * go, xs))


def _check_grads(got, ref, what, rtol=1e-3, atol_rel=1e-4):
    assert len(got) == len(ref)
    for i, (a, r) in enumerate(zip(got, ref)):
        r = np.asarray(r.numpy() if torch.is_tensor(r) else r, np.float64)
        a = a.detach().cpu().double().numpy()
        assert a.shape == r.shape
        print(f"{what} level {i}: max|err| {np.abs(a - r).max():.3e}  max|ref| {np.abs(r).max():.3e}")
        np.testing.assert_allclose(a, r, rtol=rtol, atol=atol_rel * np.abs(r).max(), err_msg=f"{what} level {i}")


@pytest.mark.parametrize("name", sorted(CASES))
def test_fused_vs_fp64_restatement(gpu, name):
    deep, target, mask, go = _inputs(name)
    ref_loss, _, ref_grads = _reference(name)
    loss, grads = _fused(deep, target, mask, gpu, go)
    print(f"{name}: loss {loss.item():.8f} ref {ref_loss.item():.8f}")
    if CASES[name][4] == "zero":
        assert loss.item() == 0.0 and all(g.abs().max().item() == 0.0 for g in grads)
    np.testing.assert_allclose(loss.item(), ref_loss.item(), rtol=1e-4)
    _check_grads(grads, ref_grads, name)
    for g_, d in zip(grads, deep):   # NCDHW-shaped views over NDHWC storage
        assert g_.shape == d.shape and g_.permute(0, 2, 3, 4, 1).is_contiguous()


def test_vanishing_class(gpu):
    """Case D's class 9 sits at odd source indices only: no level sees it (sum t = 0 at every level), its Dice term
    is 1 - 1e-5 / (sum p^2 + 1e-5); a kernel that read a neighbouring source voxel would count it."""
    g = golden("g16_deepsup.npz")
    inp = DC.case_inputs("D")
    deep, target = [torch.from_numpy(d) for d in inp["deep"]], torch.from_numpy(inp["labels"])
    assert (target == DC.VANISHING).any()
    only = torch.zeros(15, dtype=torch.long)
    only[DC.VANISHING] = 1
    ref_loss, ref_levels, ref_grads = DR.deepsup_loss(deep, target, only[:DC.C].double(), LW[:3])
    assert all(abs(v.item() * DC.C - 1.0) < 1e-3 for v in ref_levels)   # each level: (1 - ~0) / C
    loss, grads = _fused(deep, target, only, gpu)
    np.testing.assert_allclose(loss.item(), ref_loss.item(), rtol=1e-4)
    _check_grads(grads, ref_grads, "vanishing")
    loss, grads = _fused(deep, target, torch.from_numpy(inp["mask"]), gpu)
    np.testing.assert_allclose(loss.item(), float(g["D_value"]), rtol=1e-4)
    _check_grads(grads, [g[f"D_ddeep{i}"] for i in range(3)], "D vs reference")
    loss, grads = _fused(deep, target, torch.zeros(15, dtype=torch.long), gpu)
    assert loss.item() == 0.0 == float(g["Dzero_value"]) and all(x.abs().max().item() == 0.0 for x in grads)


def _sampled(t, tag, i):
    flat = t.detach().reshape(-1).cpu()
    return flat[torch.from_numpy(DC.sample_index(flat.numel(), ord(tag), i))].double().numpy()


@pytest.mark.parametrize("tag", ["A", "B"])
def test_get_loss_consistency_branch_vs_reference(gpu, tag):
    """Fixture cases A / B: the reference's get_loss with deep_out in the consistency branch — value and the
    gradients w.r.t. the logits, every deep map and every attention map."""
    from loss_functions.losses import get_loss
    g = golden("g16_deepsup.npz")
    inp = DC.case_inputs(tag)
    dev = lambda a, grad=False: torch.from_numpy(a).to(gpu).requires_grad_(grad)  # noqa: E731
    lg, deep, att = dev(inp["logits"], True), [dev(d, True) for d in inp["deep"]], [dev(a, True) for a in inp["att"]]
    attl = list(att)
    v, conf = get_loss(lg, 0, deep, dev(inp["labels"]), [dev(inp["mask"])], None, attl, dev(inp["refine"]),
                       dev(inp["label_t"]), weight_feature=DC.WEIGHT_FEATURE)
    assert conf == 0.10 and len(attl) == 3
    v.backward()
    print(f"{tag}: value {v.item():.7f} ref {float(g[f'{tag}_value']):.7f} (without deep_out "
          f"{float(g[f'{tag}_value_nodeep']):.7f})")
    np.testing.assert_allclose(v.item(), float(g[f"{tag}_value"]), rtol=1e-4)
    _check_grads([lg.grad], [g[f"{tag}_dlogits"]], f"{tag} dlogits")
    _check_grads([d.grad for d in deep], [g[f"{tag}_ddeep{i}"] for i in range(len(deep))], f"{tag} ddeep")
    for i, a in enumerate(att):
        ref = g[f"{tag}_datt{i}_val"]
        np.testing.assert_allclose(_sampled(a.grad, tag, i), ref, rtol=1e-3, atol=1e-4 * np.abs(ref).max())
        np.testing.assert_allclose(a.grad.double().norm().item(), float(g[f"{tag}_datt{i}_norm"]), rtol=1e-3)


def test_get_loss_pretrain_branch_discards_deep_term(gpu):
    """Fixture case C: with refine_output=None the reference returns dice_loss alone; the deep maps get no gradient."""
    from loss_functions.losses import get_loss
    g = golden("g16_deepsup.npz")
    inp = DC.case_inputs("A")
    dev = lambda a, grad=False: torch.from_numpy(a).to(gpu).requires_grad_(grad)  # noqa: E731
    lg, deep = dev(inp["logits"], True), [dev(d, True) for d in inp["deep"]]
    v, conf = get_loss(lg, 0, deep, dev(inp["labels"]), [dev(inp["mask"])])
    v0, _ = get_loss(lg, 0, [], dev(inp["labels"]), [dev(inp["mask"])])
    assert conf == 0.10 and v.item() == v0.item()
    np.testing.assert_allclose(v.item(), float(g["C_value"]), rtol=1e-4)
    v.backward()
    assert all(d.grad is None for d in deep) and g["C_deep_grad_none"].tolist() == [1, 1, 1]
    _check_grads([lg.grad], [g["C_dlogits"]], "C dlogits")


def _composed(deep, target, mask, gpu, go=1.0):
    """The form the fused operation replaces: a nearest resize and a partial_loss (soft Dice only) per level."""
    from u3d import loss as L
    xs = [d.to(gpu).contiguous().requires_grad_(True) for d in deep]
    t = target.to(gpu)
    w = L.class_weights([mask.to(gpu)], xs[0].shape[1], gpu)
    total = 0.0
    for x, lw in zip(xs, LW):
        ct = F.interpolate(t, x.shape[2:], mode="nearest").squeeze(1)
        total = total + L.partial_loss(x, ct, w, mode=L.MODE_SOFTMAX, uce=False) * lw
    (total * go).backward()
    return total.detach(), [x.grad for x in xs]


@pytest.mark.parametrize("name", ["geomA_c14", "geomB_c14_L4", "geomD_c14_s2", "c16_s1_L4", "c2_s2", "grad_out"])
def test_fused_equals_composed(gpu, name):
    deep, target, mask, go = _inputs(name)
    la, ga = _fused(deep, target, mask, gpu, go)
    lb, gb = _composed(deep, target, mask, gpu, go)
    print(f"{name}: fused {la.item():.8f} composed {lb.item():.8f}")
    np.testing.assert_allclose(la.item(), lb.item(), rtol=1e-5)
    for i, (a, b) in enumerate(zip(ga, gb)):
        a, b = a.cpu().double().numpy(), b.cpu().double().numpy()
        nz = b != 0
        print(f"  level {i}: max rel diff {(np.abs(a - b)[nz] / np.abs(b)[nz]).max() if nz.any() else 0.0:.3e}")
        np.testing.assert_allclose(a, b, rtol=1e-4, atol=0, err_msg=f"{name} level {i}")


@pytest.mark.parametrize("name", ["geomB_c14_L4", "c16_s2_L1", "c5_generic"])
def test_ncdhw_and_ndhwc_storage_give_identical_results(gpu, name):
    deep, target, mask, go = _inputs(name)
    la, ga = _fused(deep, target, mask, gpu, go, ndhwc=False)
    lb, gb = _fused(deep, target, mask, gpu, go, ndhwc=True)
    assert torch.equal(la, lb)
    for a, b in zip(ga, gb):
        assert torch.equal(a, b)


def test_two_runs_are_bitwise_equal(gpu):
    deep, target, mask, go = _inputs("grid_stride")
    la, ga = _fused(deep, target, mask, gpu, go)
    lb, gb = _fused(deep, target, mask, gpu, go)
    assert torch.equal(la, lb) and all(torch.equal(a, b) for a, b in zip(ga, gb))
    deep, target, mask, go = _inputs("geomB_c14_L4")
    la, ga = _fused(deep, target, mask, gpu, go)
    lb, gb = _fused(deep, target, mask, gpu, go)
    assert torch.equal(la, lb) and all(torch.equal(a, b) for a, b in zip(ga, gb))


def test_custom_level_weights(gpu):
    deep, target, mask, _ = _inputs("geomA_c14")
    lw = (0.3, 0.7, 1.9)
    ref_loss, _, ref_grads = DR.deepsup_loss(deep, target, mask.double(), lw)
    loss, grads = _fused(deep, target, mask, gpu, level_weights=lw)
    np.testing.assert_allclose(loss.item(), ref_loss.item(), rtol=1e-4)
    _check_grads(grads, ref_grads, "custom weights")


def test_forward_and_backward_replay_in_a_graph(gpu):
    """Captured once (no host to device copies: pointers and extents ride in the kernel arguments), replayed on new
    inputs: bitwise the eager result."""
    from u3d.graph import GraphedStep
    from u3d.loss import deep_supervision_loss
    batches = []
    for seed in (1, 2, 3):
        g = torch.Generator().manual_seed(seed)
        deep = [(torch.randn((2, 14) + lv, generator=g) * 2).to(gpu) for lv in B_LV]
        target = torch.randint(0, 14, (2, 1, 20, 12, 10), generator=g).float().to(gpu)
        mask = (torch.rand(14, generator=g) < 0.7).long().to(gpu)
        batches.append((*deep, target, mask))

    def make_step(deep, target, mask):
        def step():
            loss = deep_supervision_loss(deep, target, [mask])
            grads = torch.autograd.grad(loss * 0.5, deep)
            return torch.cat([loss.reshape(1)] + [x.reshape(-1) for x in grads])
        return step

    static = [t.clone() for t in batches[0]]
    for t in static[:4]:
        t.requires_grad_(True)
    gs = GraphedStep(make_step(static[:4], static[4], static[5]), tuple(static), warmup=2)
    for b in batches[1:]:
        with torch.no_grad():
            got = gs(*b).clone()
        eager_in = [t.clone().requires_grad_(True) for t in b[:4]]
        want = make_step(eager_in, b[4], b[5])()
        torch.cuda.synchronize()
        assert torch.equal(got, want)
