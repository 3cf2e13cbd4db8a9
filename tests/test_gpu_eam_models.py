"""unet3D_with_eam, unet3D_with_eam_baseline and unet3D_with_feam on the native path (u3d.feam, eam_pool.hip / eam.hip) at
32^3 against tests/golden/g18_eam.npz, the reference's own fp64 run of the configuration in tests/eam_cases.py. fp32
parity mode, the project's bounds: logits <= 1e-3 max-abs, cm and the attention maps <= 1e-3 max(1, max |ref|),
parameter-gradient norms rtol 2e-3 / atol 1e-5, sampled gradient entries within ENTRY_TOL = 0.1 of the parameter's
gradient RMS (test_gpu_parity.py's bound and its reason: single entries of a trunk gradient are ill-conditioned, a
permuted or flipped gradient moves them by ~1.4 RMS), renewed tokens <= 1e-5. The fixture's softmax is peaked and its
backward carries 98 % of d eam84.q.weight (asserted by the generator), so a wrong softmax backward cannot pass the
gradient comparison.

bf16 compute: cm and the maps of the bf16 run against the fp64 fixture within the project's 8e-2 norm-wise figure
(test_gpu_feam3.py); measured on an MI355X: BF16_MEASURED below."""
import numpy as np
import pytest
import torch

import eam_cases as EC
from conftest import golden

pytestmark = pytest.mark.gpu
ENTRY_TOL = 0.1
BF16_MEASURED = "unet3D_with_eam: cm 4.7e-2, maps 4.5e-2 (4^3) / 7.1e-2 (8^3) / 5.7e-2 (16^3, sampled)"


def _model(gpu, tag, **kw):
    import unet3D
    return EC.build(unet3D, tag, **kw).to(gpu).train()


def _x(gpu):
    return EC.x_volume().to(gpu)


def _forward(m, tag, x, mask=None):
    if tag == "feam":
        logits, att = m(x, torch.zeros(EC.SHAPE, device=x.device) if mask is None else mask)
        return logits, None, att
    return m(x, None)


def _close(name, got, ref):
    ref = np.asarray(ref)
    err = np.abs(np.asarray(got, dtype=np.float64) - ref).max()
    bound = 1e-3 * max(1.0, np.abs(ref).max())
    print(f"{name}: err {err:.3e}, bound {bound:.3e}")
    assert err <= bound, (name, err, bound)


def _check_outputs(g, tag, logits, cm, att):
    flat = logits.detach().reshape(-1).cpu()
    err = np.abs(flat[torch.from_numpy(EC.sample_index(flat.numel(), 0))].double().numpy() - g[f"{tag}_logits_val"]).max()
    assert err <= 1e-3, ("logits", err)
    assert abs(flat.double().sum().item() - float(g[f"{tag}_logits_sum"])) <= 1e-3 * flat.numel() ** 0.5
    if tag != "feam":
        assert cm.shape == g[f"{tag}_cm"].shape
        _close(f"{tag} cm", cm.detach().cpu().numpy(), g[f"{tag}_cm"])
    assert len(att) == int(g[f"{tag}_natt"])
    for i, a in enumerate(att):
        a = a.detach().cpu()
        if f"{tag}_att{i}" in g.files:
            assert a.shape == g[f"{tag}_att{i}"].shape
            _close(f"{tag} att{i}", a.numpy(), g[f"{tag}_att{i}"])
        else:
            val = a.reshape(-1)[torch.from_numpy(EC.sample_index(a.numel(), 1, i))].numpy()
            err = np.abs(val.astype(np.float64) - g[f"{tag}_att{i}_val"]).max()
            assert err <= 1e-3 * max(1.0, float(g[f"{tag}_att{i}_max"])), (i, err)


def _check_grads(g, tag, m):
    names, norms, gidx, gval = EC.grad_summary(m)
    assert names.tolist() == g[f"{tag}_gnames"].tolist()
    worst, worst_entry, worst_lit, bad = 0.0, (0.0, ""), (0.0, ""), []
    for i, k in enumerate(names):
        ref = float(g[f"{tag}_gnorm"][i])
        if ref < 0:
            assert norms[i] < 0, f"{k}: a gradient where the reference has none"
            continue
        assert norms[i] >= 0, f"{k}: no gradient"
        assert abs(norms[i] - ref) <= 2e-3 * ref + 1e-5, (k, norms[i], ref)
        assert (gidx[i] == g[f"{tag}_gidx"][i]).all()
        want = g[f"{tag}_gval"][i]
        err = np.abs(gval[i] - want)
        rms = ref / dict(m.named_parameters())[k].numel() ** 0.5
        worst_entry = max(worst_entry, (float(err.max() / rms) if rms > 0 else 0.0, k))
        worst_lit = max(worst_lit, (float((err / (2e-3 * np.abs(want) + 1e-5)).max()), k))
        if rms > 0 and err.max() > ENTRY_TOL * rms:
            bad.append((k, float(err.max() / rms)))
        worst = max(worst, abs(norms[i] / ref - 1) if ref > 0 else 0.0)
    print(f"{tag}: worst gradient-norm deviation {worst:.3e}; worst sampled entry {worst_entry[0]:.3e} x RMS "
          f"({worst_entry[1]}); entry by entry at rtol 2e-3 / atol 1e-5 the worst is {worst_lit[0]:.1f} x that "
          f"({worst_lit[1]})")
    assert not bad, f"sampled gradient entries off by more than {ENTRY_TOL} x RMS: {bad}"


@pytest.mark.parametrize("tag", ["eam", "base", "feam"])
def test_forward_backward_vs_reference_fixture(gpu, tag):
    g = golden("g18_eam.npz")
    m = _model(gpu, tag)
    logits, cm, att = _forward(m, tag, _x(gpu))
    _check_outputs(g, tag, logits, cm, att)
    EC.loss_of(tag, logits, cm, att).backward()
    torch.cuda.synchronize()
    _check_grads(g, tag, m)
    idx = g[f"{tag}_gnames"].tolist()
    if tag != "feam":   # the halves of the EAM that only the class message reaches, and the class token itself
        c84 = 128
        for k in ("eam84.proj.weight", "eam84.proj.bias", "class_token", "linear84_2_42.weight"):
            assert float(dict(m.named_parameters())[k].grad.double().norm()) > 0, k
        vhalf = m.eam84.kv.weight.grad[c84:].double().norm().item()
        assert vhalf > 1e-3 * float(g[f"{tag}_gnorm"][idx.index("eam84.kv.weight")])
    else:               # the tokens are detached and proj is past the discarded class message
        for k in ("eam84.proj.weight", "class_token1"):
            assert dict(m.named_parameters())[k].grad is None


@pytest.mark.parametrize("tag", ["eam", "base", "feam"])
def test_eval_returns_the_train_logits(gpu, tag):
    m = _model(gpu, tag)
    x = _x(gpu)
    with torch.no_grad():
        train = _forward(m, tag, x)[0]
        ev = m.eval()(x, None)
    assert isinstance(ev, torch.Tensor) and torch.equal(ev, train)


def test_no_grad_train_forward_matches_the_recorded_one(gpu):
    g = golden("g18_eam.npz")
    m = _model(gpu, "eam")
    with torch.no_grad():
        logits, cm, att = m(_x(gpu), None)
    _check_outputs(g, "eam", logits, cm, att)


@pytest.mark.parametrize("tag", ["eam", "base", "feam"])
def test_batch_of_two_raises(gpu, tag):
    m = _model(gpu, tag)
    x = torch.zeros(2, 1, 16, 16, 16, device=gpu)
    with pytest.raises(RuntimeError, match="is invalid for input of size"):
        _forward(m, tag, x, torch.zeros(2, 1, 16, 16, 16, device=gpu))


def test_use_cm_gating(gpu):
    g = golden("g18_eam.npz")
    x = _x(gpu)
    with pytest.raises(UnboundLocalError):
        _model(gpu, "eam", use_cm=[False, True, True])(x, None)
    assert isinstance(_model(gpu, "eam", use_cm=[False, True, True]).eval()(x, None), torch.Tensor)
    with torch.no_grad():
        logits, cm, att = _model(gpu, "eam", use_cm=[True, False, True])(x, None)   # the third level needs the second
        assert len(att) == 1 and cm.shape == (1, EC.NC, 128)
        _close("att0", att[0].cpu().numpy(), g["eam_att0"])
        logits, att = _model(gpu, "feam", use_cm=[True, False, True])(x, torch.zeros(EC.SHAPE, device=gpu))
        assert len(att) == 1


def test_logits_only_loss_leaves_the_eam_parameters_without_gradient(gpu):
    m = _model(gpu, "eam")
    logits, cm, att = m(_x(gpu), None)
    logits.square().mean().backward()
    for k, p in m.named_parameters():
        if k.startswith(("eam", "linear", "class_token")):
            assert p.grad is None, k
        else:
            assert p.grad is not None, k


def test_bf16_compute_stays_within_the_norm_wise_figure(gpu):
    g = golden("g18_eam.npz")
    m = _model(gpu, "eam")
    m.compute_dtype = torch.bfloat16
    with torch.no_grad():
        logits, cm, att = m(_x(gpu), None)

    def rel(got, ref):
        return float(np.linalg.norm(got.double().cpu().numpy() - ref) / np.linalg.norm(ref))
    figs = [rel(cm, g["eam_cm"])] + [rel(att[i], g[f"eam_att{i}"]) for i in range(2)]
    flat = att[2].reshape(-1).cpu()[torch.from_numpy(EC.sample_index(att[2].numel(), 1, 2))]
    figs.append(rel(flat, g["eam_att2_val"]))
    print("bf16 norm-wise errors (cm, maps):", " ".join(f"{f:.3e}" for f in figs))
    assert max(figs) <= 8e-2, figs


def test_feam_renews_its_tokens_in_the_forward(gpu):
    g = golden("g18_eam.npz")
    m = _model(gpu, "feam", ema=True)
    mask = EC.label_mask().to(gpu)
    before = m.class_token1.detach().clone()
    logits, att = m(_x(gpu), mask)
    assert len(att) == 3
    for k in (1, 2, 3):
        err = (getattr(m, f"class_token{k}").detach().cpu().double().numpy() - g[f"feam_renew_tok{k}"])
        assert np.abs(err).max() <= 1e-5, (k, np.abs(err).max())
    assert not torch.equal(before, m.class_token1.detach())
    for i, a in enumerate(att):     # the maps are taken against the renewed tokens
        val = a.reshape(-1).cpu()[torch.from_numpy(EC.sample_index(a.numel(), 2, i))].double().numpy()
        ref = g[f"feam_renew_att{i}_val"]
        assert np.abs(val - ref).max() <= 1e-3 * max(1.0, np.abs(ref).max())


def test_feam_labelled_mask_with_grad_requiring_tokens_raises(gpu):
    g = golden("g18_eam.npz")
    assert int(g["feam_labelled_grad_raises"]) == 1
    m = _model(gpu, "feam")
    with pytest.raises(RuntimeError, match="in-place operation"):
        m(_x(gpu), EC.label_mask().to(gpu))
    with pytest.raises(AttributeError):
        m(_x(gpu), None)
