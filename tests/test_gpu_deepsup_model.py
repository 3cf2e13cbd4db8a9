"""unet3D_with_deepsup on the native path against the reference's G16 model fixture (batch 2: new ground for the deep
heads). fp32 parity mode: deep maps and sampled logits <= 1e-3 max-abs, parameter-gradient norms rtol 2e-3, sampled
gradient entries within 0.1 x the parameter's gradient RMS, eval logits equal to train logits within
the fixture's own difference + 1e-5. One bf16 autocast training step with the deep-supervision loss runs, eagerly and
under u3d.graph.GraphedStep (same losses and weights, rel 1e-6)."""
import numpy as np
import pytest
import torch

import deepsup_cases as DC
from conftest import golden
from oracle.weights_recipe import apply_recipe, input_volume

pytestmark = pytest.mark.gpu
NC = DC.C


def _model(gpu, **kw):
    import unet3D
    m = unet3D.unet3D_with_deepsup([1, 2, 2, 2, 2], num_classes=NC, weight_std=True, **kw)
    apply_recipe(m, seed=0)
    return m.to(gpu).train()


def _x(gpu):
    shape, seed = DC.MODEL_INPUT
    return torch.from_numpy(input_volume(shape, seed=seed, kind="normal")).to(gpu)


def test_deepsup_forward_backward_vs_golden(gpu):
    g = golden("g16_deepsup_model.npz")
    m, x = _model(gpu), _x(gpu)
    np.testing.assert_allclose(x.double().abs().sum().item(), float(g["x_sum"]), rtol=1e-12)
    logits, deep = m(x, None)
    assert logits.shape == (2, NC, 32, 32, 32) and [tuple(d.shape[2:]) for d in deep] == [(4,) * 3, (8,) * 3, (16,) * 3]
    for i, d in enumerate(deep):
        err = np.abs(d.detach().cpu().numpy() - g[f"deep{i}"]).max()
        print(f"deep{i}: max-abs err {err:.3e}")
        assert err < 1e-3, (i, err)
        assert d.permute(0, 2, 3, 4, 1).is_contiguous()   # NCDHW view of NDHWC storage: the loss reads it in place
    flat = logits.detach().reshape(-1).cpu()
    got = flat[torch.from_numpy(DC.sample_index(flat.numel(), 0))].numpy()
    assert np.abs(got - g["logits_val"]).max() < 1e-3
    np.testing.assert_allclose(flat.double().sum().item(), float(g["logits_sum"]), rtol=0, atol=1e-3 * flat.numel() ** 0.5)
    outs = [logits] + list(deep)
    ups = DC.model_projections([tuple(t.shape) for t in outs])
    sum((t * torch.from_numpy(u).to(gpu)).sum() for t, u in zip(outs, ups)).backward()
    named = dict(m.named_parameters())
    assert list(named) == [str(k) for k in g["gnames"]]
    rows = []
    for i, k in enumerate(g["gnames"]):
        gr = named[str(k)].grad.double().reshape(-1).cpu()
        rms = g["gnorm"][i] / gr.numel() ** 0.5
        err = np.abs(gr[torch.from_numpy(g["gidx"][i])].numpy() - g["gval"][i]).max()
        rows.append((abs(gr.norm().item() - g["gnorm"][i]) / g["gnorm"][i], err / rms, gr.norm().item(), i, str(k)))
    for r in sorted(rows, reverse=True)[:5]:
        print("grad norm rel err %.3e  entry err / rms %.3e  %s" % (r[0], r[1], r[4]))
    print("worst entry err / rms %.3e" % max(r[1] for r in rows))
    for _, erel, gn, i, k in rows:
        np.testing.assert_allclose(gn, g["gnorm"][i], rtol=2e-3, atol=1e-5, err_msg=k)
        assert erel <= 0.1, (k, erel)


def test_deepsup_eval_returns_logits_only(gpu):
    g = golden("g16_deepsup_model.npz")
    m, x = _model(gpu), _x(gpu)
    with torch.no_grad():
        train_logits, deep = m(x, None)
        y = m.eval()(x, None)
    assert torch.is_tensor(y) and y.shape == (2, NC, 32, 32, 32) and len(deep) == 3
    assert (y - train_logits).abs().max().item() <= float(g["eval_minus_train"]) + 1e-5


def test_deepsup_ema_and_no_grad_paths(gpu):
    """ema=True detaches the parameters (no autograd graph, as feam3); torch.no_grad gives the same values."""
    x = _x(gpu)
    logits, deep = _model(gpu, ema=True)(x, None)
    assert not logits.requires_grad and not any(d.requires_grad for d in deep)
    m = _model(gpu)
    with torch.no_grad():
        lg2, deep2 = m(x, None)
    assert torch.equal(logits, lg2) and all(torch.equal(a, b) for a, b in zip(deep, deep2))
    lg3, deep3 = m(x, None)
    assert lg3.requires_grad and all(d.requires_grad for d in deep3)
    assert (lg3.detach() - lg2).abs().max().item() < 1e-4   # the recording forward may route convs differently


def _train_setup(gpu):
    from loss_functions.loss_partial import EDiceLoss_partial
    m = _model(gpu)
    opt = torch.optim.SGD(m.parameters(), lr=1e-2, momentum=0.9, weight_decay=1e-4)
    g = torch.Generator().manual_seed(7)
    bs = []
    for _ in range(3):
        x = (torch.rand((2, 1, 32, 32, 32), generator=g) * 2 - 1).to(gpu)
        lab = torch.randint(0, NC, (2, 1, 32, 32, 32), generator=g).float().to(gpu)
        mask = (torch.rand(NC, generator=g) < 0.7).long().to(gpu)
        bs.append((x, lab, mask))
    return m, opt, EDiceLoss_partial(NC), bs


def _make_step(m, opt, crit, x, t, mk):
    from u3d.loss import deep_supervision_loss

    def step():
        opt.zero_grad(set_to_none=True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            lg, deep = m(x, None)
        loss = crit(lg, t.squeeze(1), mask=[mk]) + deep_supervision_loss(deep, t, [mk])
        loss.backward()
        opt.step()
        return loss
    return step


def test_bf16_training_step_with_deep_supervision(gpu):
    m, opt, crit, bs = _train_setup(gpu)
    x, t, mk = bs[0]
    from u3d.loss import deep_supervision_loss
    opt.zero_grad(set_to_none=True)
    with torch.autocast("cuda", dtype=torch.bfloat16):
        lg, deep = m(x, None)
    main, aux = crit(lg, t.squeeze(1), mask=[mk]), deep_supervision_loss(deep, t, [mk])
    (main + aux).backward()
    assert torch.isfinite(main).item() and torch.isfinite(aux).item() and aux.item() > 0
    for n, p in m.named_parameters():
        assert p.grad is not None and torch.isfinite(p.grad).all(), n
    assert m.deepout1[2].weight.grad.abs().max().item() > 0


def test_graphed_deepsup_step_matches_eager(gpu):
    from u3d.graph import GraphedStep
    mA, oA, cA, bs = _train_setup(gpu)
    xA, tA, kA = (t.clone() for t in bs[0])
    stepA = _make_step(mA, oA, cA, xA, tA, kA)
    for _ in range(3):
        stepA()
    lossA = []
    for b in bs[1:]:
        for dst, src in zip((xA, tA, kA), b):
            dst.copy_(src)
        lossA.append(stepA().item())
    mB, oB, cB, _ = _train_setup(gpu)
    xB, tB, kB = (t.clone() for t in bs[0])
    g = GraphedStep(_make_step(mB, oB, cB, xB, tB, kB), (xB, tB, kB), warmup=3, optimizer=oB)
    lossB = [g(*b).item() for b in bs[1:]]
    torch.cuda.synchronize()
    assert lossA == pytest.approx(lossB, rel=1e-6, abs=1e-7)
    for (n, pa), (_, pb) in zip(mA.named_parameters(), mB.named_parameters()):
        torch.testing.assert_close(pa, pb, rtol=1e-6, atol=1e-7, msg=n)
