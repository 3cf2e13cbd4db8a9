"""Generate the G18 fixture by running the REFERENCE's unet3D_with_eam, unet3D_with_eam_baseline and unet3D_with_feam on
the CPU in fp64 (test infrastructure, run where the reference is present, as tests/golden/gen_golden.py whose shims
it imports):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_eam.py

The configuration is tests/eam_cases.py's. Only outputs are stored (g18_eam.npz): parameter names and shapes; sampled
logits; cm and the attention maps (the 16^3 map sampled); parameter-gradient norms and seeded sampled entries under the
random output projections of eam_cases.loss_of, which include one on cm; for unet3D_with_feam the renewed tokens
(ema=True, labelled mask) and a gradient case with a mask that holds no label.

Asserted here, so that the fixture can tell a wrong softmax backward from a right one: at every level of every model
max_n P >= 8 / N on at least half of the (head, token) rows; and with the softmax detached in eam84 (its backward term
scale P (dP - D) left out) |d eam84.q.weight| moves by more than 100 x the tests' gradient tolerance.
"""
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_golden as G  # noqa: E402  (reference imports + shims, oracle/ on the path)
import eam_cases as EC  # noqa: E402

GRAD_RTOL = 2e-3  # the model tests' bound on gradient norms


class _DetachedSoftmax(torch.nn.Module):
    def forward(self, x):
        return torch.softmax(x, -1).detach()


def _peaked(m, tag, rec):
    """Hooks on every EAM: record max_n softmax(scale attn) per row from the module's own outputs."""
    hooks = []
    for e in EC.EAMS[tag]:
        mod = getattr(m, e)

        def hook(mod_, inp, outp, e=e):
            attn = outp[1].detach()                     # [1, heads, nt, N]
            p = torch.softmax(attn * mod_.scale, -1)
            rec[e] = (p.max(-1).values.reshape(-1), attn.shape[-1])
        hooks.append(mod.register_forward_hook(hook))
    return hooks


def _run(tag, out, detach_softmax=False, **kw):
    m = EC.build(G.R, tag, **kw).double().train()
    if detach_softmax:
        m.eam84.softmax = _DetachedSoftmax()
    rec = {}
    hooks = _peaked(m, tag, rec)
    x = EC.x_volume().double()
    if tag == "feam":
        logits, att = m(x, torch.zeros(EC.SHAPE, dtype=torch.float64))    # no label: no token is renewed
        cm = None
    else:
        logits, cm, att = m(x, None)
    for h in hooks:
        h.remove()
    EC.loss_of(tag, logits, cm, att).backward()
    if detach_softmax:
        return m
    for e, (pmax, n) in rec.items():
        share = (pmax >= 8.0 / n).double().mean().item()
        print(f"{tag} {e}: N = {n}, rows with max P >= 8/N: {share:.2f}, median max P {pmax.median().item():.3f}")
        assert share >= 0.5, (tag, e, share)
    out[f"{tag}_pnames"] = np.array([k for k, _ in m.named_parameters()])
    out[f"{tag}_pshapes"] = np.array([",".join(str(s) for s in p.shape) for _, p in m.named_parameters()])
    flat = logits.detach().reshape(-1)
    out[f"{tag}_logits_val"] = flat[torch.from_numpy(EC.sample_index(flat.numel(), 0))].numpy()
    out[f"{tag}_logits_sum"] = flat.sum().numpy()
    if cm is not None:
        out[f"{tag}_cm"] = cm.detach().numpy()
    for i, a in enumerate(att):
        a = a.detach()
        if a.numel() > 4 * EC.SAMPLE_N:
            out[f"{tag}_att{i}_val"] = a.reshape(-1)[torch.from_numpy(EC.sample_index(a.numel(), 1, i))].numpy()
            out[f"{tag}_att{i}_max"] = a.abs().max().numpy()
        else:
            out[f"{tag}_att{i}"] = a.numpy()
    out[f"{tag}_natt"] = np.array(len(att))
    names, norms, gidx, gval = EC.grad_summary(m)
    out[f"{tag}_gnames"], out[f"{tag}_gnorm"], out[f"{tag}_gidx"], out[f"{tag}_gval"] = names, norms, gidx, gval
    m.eval()
    with torch.no_grad():
        ev = m(x, None)
    out[f"{tag}_eval_minus_train"] = (ev - logits.detach()).abs().max().numpy()
    return m


def _softmax_backward_matters(out):
    full = _run("eam", {})
    cut = _run("eam", {}, detach_softmax=True)
    a, b = full.eam84.q.weight.grad, cut.eam84.q.weight.grad
    move = ((a - b).norm() / a.norm()).item()
    print(f"eam84.q.weight: |grad| {a.norm().item():.4e}, without the softmax backward off by {move:.3f} of it")
    assert abs(b.norm().item() / a.norm().item() - 1) > 100 * GRAD_RTOL, (a.norm(), b.norm())
    out["eam_q84_without_softmax_bwd"] = np.array(b.norm().item())


def _feam_renewal(out):
    m = EC.build(G.R, "feam", ema=True).double().train()
    mask = EC.label_mask().double()
    with torch.no_grad():
        logits, att = m(EC.x_volume().double(), mask)
    for k in (1, 2, 3):
        out[f"feam_renew_tok{k}"] = getattr(m, f"class_token{k}").detach().numpy()
    for i, a in enumerate(att):
        a = a.detach()
        out[f"feam_renew_att{i}_val"] = a.reshape(-1)[torch.from_numpy(EC.sample_index(a.numel(), 2, i))].numpy()
    m2 = EC.build(G.R, "feam").double().train()
    try:
        m2(EC.x_volume().double(), mask)
        out["feam_labelled_grad_raises"] = np.array(0)
    except RuntimeError:
        out["feam_labelled_grad_raises"] = np.array(1)


if __name__ == "__main__":
    out = {}
    for tag in ("eam", "base", "feam"):
        _run(tag, out)
    _softmax_backward_matters(out)
    _feam_renewal(out)
    G.save("g18_eam.npz", **out)
