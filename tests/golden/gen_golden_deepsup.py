"""Generate the G16 deep-supervision fixtures by running the REFERENCE on the CPU (test infrastructure, run where
the reference is present, as tests/golden/gen_golden.py whose shims it imports):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_deepsup.py

  g16_deepsup.npz        get_loss with deep_out (losses.py:107-182): cases A-D of tests/deepsup_cases.py
  g16_deepsup_model.npz  unet3D_with_deepsup (unet3D.py:280-429), train forward + backward, eval

Only outputs are stored: the inputs are rebuilt from seeds by tests/deepsup_cases.py (their checksum is stored), and
the attention-map gradients of cases A / B are stored as N_SAMPLE seeded entries + the fp64 norm per map (the full
maps would take the two files past the size a committed file may have; the model lives in its own file for the
same reason).
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_golden as G  # noqa: E402  (reference imports + shims, oracle/weights_recipe on the path)
import deepsup_cases as DC  # noqa: E402
from loss_functions import losses as RL  # noqa: E402  (the reference's)
from weights_recipe import apply_recipe, input_volume  # noqa: E402


def _t(a, grad=False):
    return torch.from_numpy(a).clone().requires_grad_(grad)


def _deep_term(deep, labels, mask):
    """The reference's own blocks per level (losses.py:121-129): (sum_l w_l * level_l, [level_l])."""
    levels = [G.RLP.EDiceLoss_partial(DC.C)(l, F.interpolate(labels, l.shape[2:], mode="nearest").float().squeeze(1),
                                            soft_max=True, mask=mask, uce=False) for l in deep]
    return sum(v * w for v, w in zip(levels, DC.LEVEL_WEIGHTS)), levels


def consistency_case(tag, out):
    inp = DC.case_inputs(tag)
    lg, deep = _t(inp["logits"], True), [_t(d, True) for d in inp["deep"]]
    att = [_t(a, True) for a in inp["att"]]
    lab, mask = _t(inp["labels"]), [_t(inp["mask"])]
    ref, label_t = _t(inp["refine"]), _t(inp["label_t"])
    attl = list(att)
    v, _ = RL.get_loss(lg, 0, deep, lab, mask, None, attl, ref, label_t, weight_feature=DC.WEIGHT_FEATURE)
    assert len(attl) == 3
    v.backward()
    with torch.no_grad():
        v0, _ = RL.get_loss(lg, 0, [], lab, mask, None, list(att), ref, label_t, weight_feature=DC.WEIGHT_FEATURE)
        vd, levels = _deep_term(deep, lab, mask)
    assert abs(float(v0) + float(vd) - float(v.detach())) < 1e-5 * abs(float(v.detach())), (v0, vd, v)
    out[f"{tag}_insum"] = DC.checksum(inp)
    out[f"{tag}_value"], out[f"{tag}_value_nodeep"] = v.detach().numpy(), v0.numpy()
    out[f"{tag}_deep_value"], out[f"{tag}_levels"] = vd.numpy(), np.array([float(x) for x in levels], np.float32)
    out[f"{tag}_dlogits"] = lg.grad.numpy()
    for i, d in enumerate(deep):
        out[f"{tag}_ddeep{i}"] = d.grad.numpy()
    for i, a in enumerate(att):
        flat = a.grad.reshape(-1)
        out[f"{tag}_datt{i}_val"] = flat[torch.from_numpy(DC.sample_index(flat.numel(), ord(tag), i))].numpy()
        out[f"{tag}_datt{i}_norm"] = flat.double().norm().numpy()


def pretrain_case(out):
    inp = DC.case_inputs("A")
    lg, deep = _t(inp["logits"], True), [_t(d, True) for d in inp["deep"]]
    lab, mask = _t(inp["labels"]), [_t(inp["mask"])]
    v, _ = RL.get_loss(lg, 0, deep, lab, mask)
    v.backward()
    with torch.no_grad():
        v0, _ = RL.get_loss(lg, 0, [], lab, mask)
    out["C_value"], out["C_value_nodeep"] = v.detach().numpy(), v0.numpy()
    out["C_deep_grad_none"] = np.array([int(d.grad is None) for d in deep])
    out["C_dlogits"] = lg.grad.numpy()


def batch2_case(out):
    inp = DC.case_inputs("D")
    lab = _t(inp["labels"])
    for l in inp["deep"]:   # the construction holds: the class is in the target and in no resized target
        assert (lab == DC.VANISHING).any() and not (F.interpolate(lab, l.shape[2:], mode="nearest") == DC.VANISHING).any()
    out["D_insum"] = DC.checksum(inp)
    for tag, mvec in (("D", inp["mask"]), ("Dzero", np.zeros(15, np.int64))):
        deep = [_t(d, True) for d in inp["deep"]]
        v, levels = _deep_term(deep, lab, [_t(mvec)])
        v.backward()
        out[f"{tag}_value"], out[f"{tag}_levels"] = v.detach().numpy(), np.array([float(x) for x in levels], np.float32)
        for i, d in enumerate(deep):
            out[f"{tag}_ddeep{i}"] = d.grad.numpy()


def model_fixture():
    shape, seed = DC.MODEL_INPUT
    m = G.R.unet3D_with_deepsup([1, 2, 2, 2, 2], DC.C, weight_std=True)
    apply_recipe(m, seed=0)
    m.train()
    x = torch.from_numpy(input_volume(shape, seed=seed, kind="normal"))
    logits, deep = m(x, None)
    outs = [logits] + list(deep)
    ups = DC.model_projections([tuple(t.shape) for t in outs])
    sum((t * torch.from_numpy(u)).sum() for t, u in zip(outs, ups)).backward()
    names, norms, gidx, gval = G.grad_summary(m)
    flat = logits.detach().reshape(-1)
    idx = DC.sample_index(flat.numel(), 0)
    out = {"keys": np.array(list(m.state_dict().keys())), "gnames": names, "gnorm": norms, "gidx": gidx, "gval": gval,
           "logits_val": flat[torch.from_numpy(idx)].numpy(), "logits_sum": flat.double().sum().numpy(),
           "x_sum": np.abs(x.double().numpy()).sum()}
    for i, d in enumerate(deep):
        out[f"deep{i}"] = d.detach().numpy()
    m.eval()
    with torch.no_grad():
        out["eval_minus_train"] = (m(x, None) - logits.detach()).abs().max().numpy()
    G.save("g16_deepsup_model.npz", **out)


if __name__ == "__main__":
    out = {}
    consistency_case("A", out)
    consistency_case("B", out)
    pretrain_case(out)
    batch2_case(out)
    G.save("g16_deepsup.npz", **out)
    model_fixture()
