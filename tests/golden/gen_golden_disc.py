"""Generate the G17 style-discriminator fixtures by running the REFERENCE on the CPU (test infrastructure, run where
the reference is present, as tests/golden/gen_golden.py whose shims it imports):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_disc.py

  g17_disc.npz        M1-M3 (logits, parameter / input / f_m gradient summaries), M5 (keys, shapes, default-initialised
                      parameters after torch.manual_seed(0)), M6 (the reference at B = 0)
  g17_disc_step.npz   M4, the driver's step pattern (train_amos_atlas_final.py:320-379) on the deep discriminator

M1-M4 run the reference's modules in fp64 (module.double(), the float32 inputs and weights widened exactly): the
fixture then does not depend on the order in which a CPU sums fp32 products (thread count, vector width), which moves
an fp32 weight-gradient entry by a few 1e-6 of the largest one between machines, and the fp64 restatement
tests/disc_reference.py can be pinned to it at 1e-6 anywhere. The native tests' bounds (1e-3 and up) are far above
the reference's own fp32 rounding.

Only outputs are stored: inputs and weights are rebuilt from seeds by tests/disc_cases.py (their checksum is
stored); gradients are stored as fp64 norms plus seeded sampled entries (the three 256 -> 256 4^3 weights are 4.2 M
floats each).
"""
import hashlib
import os
import sys

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_golden as G  # noqa: E402  (reference imports + shims)
import disc_cases as DC  # noqa: E402
from loss_functions import losses as RL  # noqa: E402  (the reference's)

LOGIT_TOL = 1e-3  # the model tests' bound on the logits, relative to max |logit|


def _build(kind):
    return getattr(G.R, DC.KINDS[kind])(DC.NUM_CLASSES, DC.NDF)


def _inputs(tag, grad):
    inp = DC.case_inputs(tag)
    x = torch.from_numpy(inp["x"]).double().requires_grad_(grad)
    f_m = [torch.from_numpy(f).double().requires_grad_(grad) for f in inp.get("f_m", [])]
    return inp, x, f_m


def _assert_samples_differ(logits):
    """A kernel that ignored its input must fail: different samples' logits differ by > 100 x the tolerance."""
    lg = logits.detach().double()
    tol = LOGIT_TOL * lg.abs().max()
    for a in range(lg.shape[0]):
        for b in range(a + 1, lg.shape[0]):
            assert (lg[a] - lg[b]).abs().max() > 100 * tol, (a, b, lg)


def model_case(tag, out):
    kind = DC.GEOM[tag][0]
    m = _build(kind)
    w = DC.fill(m)
    m.double().train()
    inp, x, f_m = _inputs(tag, True)
    logits = m(x, f_m) if kind == "deep" else m(x)
    if logits.shape[0] > 1:
        _assert_samples_differ(logits)
    (logits * torch.from_numpy(DC.projection(tag, tuple(logits.shape))).double()).sum().backward()
    out[f"{tag}_insum"] = DC.checksum(inp, w)
    out[f"{tag}_logits"] = logits.detach().numpy()
    names, norms, gidx, gval = DC.grad_summary([(k, p.grad) for k, p in m.named_parameters()])
    out[f"{tag}_gnames"], out[f"{tag}_gnorm"], out[f"{tag}_gidx"], out[f"{tag}_gval"] = names, norms, gidx, gval
    out[f"{tag}_dx_norm"], out[f"{tag}_dx_val"] = DC.tensor_summary(x.grad, int(tag[1]), 0)
    for i, f in enumerate(f_m):
        out[f"{tag}_df{i}_norm"], out[f"{tag}_df{i}_val"] = DC.tensor_summary(f.grad, int(tag[1]), 1 + i)


def step_case(out):
    """train_amos_atlas_final.py:326-377 with the reference's own module and losses: both forwards, then both
    backwards. (The reference's bce_loss moves its label with .to(y_pred.get_device()), which is -1 on the CPU; its
    body is SmoothCrossEntropyLoss()(y_pred, constant label), called here directly with the same label.)"""
    tag = "M4"
    m = _build("deep")
    w = DC.fill(m)
    m.double().train()
    inp, x, f_m = _inputs(tag, True)
    flist, clist = DC.FLIST, list(range(x.shape[0]))
    label_t = torch.tensor(DC.LABEL_T)
    for p in m.parameters():
        p.requires_grad = False
    d_output = m(x[flist], [f[flist] for f in f_m])
    loss_d = RL.SmoothCrossEntropyLoss()(d_output, torch.full((d_output.shape[0],), 1, dtype=torch.long))
    for p in m.parameters():
        p.requires_grad = True
    d_output_ = m(x.detach()[clist], [f.detach()[clist] for f in f_m])
    loss_d_ = RL.SmoothCrossEntropyLoss()(d_output_, label_t[clist])
    _assert_samples_differ(d_output_)
    (loss_d * 0.01).backward()
    out["M4_gen_pgrad_none"] = np.array([int(p.grad is None) for p in m.parameters()])
    loss_d_.backward()
    out["M4_insum"] = DC.checksum(inp, w)
    out["M4_gen_logits"], out["M4_dis_logits"] = d_output.detach().numpy(), d_output_.detach().numpy()
    out["M4_loss_d"], out["M4_loss_d_"] = loss_d.detach().numpy(), loss_d_.detach().numpy()
    names, norms, gidx, gval = DC.grad_summary([(k, p.grad) for k, p in m.named_parameters()])
    out["M4_gnames"], out["M4_gnorm"], out["M4_gidx"], out["M4_gval"] = names, norms, gidx, gval
    out["M4_dx_norm"], out["M4_dx_val"] = DC.tensor_summary(x.grad, 4, 0)
    for i, f in enumerate(f_m):
        out[f"M4_df{i}_norm"], out[f"M4_df{i}_val"] = DC.tensor_summary(f.grad, 4, 1 + i)
    # rows outside flist get no gradient
    rest = [i for i in clist if i not in flist]
    out["M4_dx_rest_absmax"] = x.grad[rest].abs().max().numpy()


def init_case(out):
    for kind in DC.KINDS:
        torch.manual_seed(0)
        m = _build(kind)
        sd = m.state_dict()
        out[f"M5_{kind}_keys"] = np.array(list(sd.keys()))
        out[f"M5_{kind}_shapes"] = np.array([",".join(str(v) for v in t.shape) for t in sd.values()])
        out[f"M5_{kind}_abssum"] = np.array([t.double().abs().sum().item() for t in sd.values()])
        h = hashlib.sha256()
        for t in sd.values():
            h.update(t.contiguous().numpy().tobytes())
        out[f"M5_{kind}_sha256"] = np.array(h.hexdigest())


def _state(g):
    return 0 if g is None else (1 if float(g.abs().sum()) == 0.0 else 2)


def empty_case(out):
    """What the reference module does at B = 0 on the CPU: 0 = gradient None, 1 = all zeros, 2 = non-zero."""
    for kind in ("norm", "deep"):
        m = _build(kind)
        DC.fill(m)
        dims = (64, 64, 64)
        x = torch.zeros((0, DC.NUM_CLASSES) + dims, requires_grad=True)
        f_m = [torch.zeros((0, 1) + DC.halve(dims, 3 - i), requires_grad=True) for i in range(3)]
        try:
            o = m(x, f_m) if kind == "deep" else m(x)
            out[f"M6_{kind}_fwd_ok"], out[f"M6_{kind}_shape"] = np.array(1), np.array(o.shape)
        except Exception as e:  # noqa: BLE001
            out[f"M6_{kind}_fwd_ok"], out[f"M6_{kind}_error"] = np.array(0), np.array(type(e).__name__)
            continue
        try:
            o.sum().backward()
            out[f"M6_{kind}_bwd_ok"] = np.array(1)
            out[f"M6_{kind}_pgrad"] = np.array([_state(p.grad) for p in m.parameters()])
            out[f"M6_{kind}_xgrad"] = np.array([_state(x.grad)] + ([_state(f.grad) for f in f_m] if kind == "deep" else []))
        except Exception as e:  # noqa: BLE001
            out[f"M6_{kind}_bwd_ok"], out[f"M6_{kind}_error"] = np.array(0), np.array(type(e).__name__)


if __name__ == "__main__":
    out = {}
    for tag in ("M1", "M2", "M3"):
        model_case(tag, out)
    init_case(out)
    empty_case(out)
    G.save("g17_disc.npz", **out)
    out = {}
    step_case(out)
    G.save("g17_disc_step.npz", **out)
