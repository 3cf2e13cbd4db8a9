"""The native style discriminators end to end against the G17 fixtures (the reference's CPU outputs), fp32 mode, with
the bounds the project uses for G1-G3 and G8: logits max-abs <= 1e-3 max|logit|; every parameter-gradient norm rtol
2e-3 and sampled entries <= 0.1 x the parameter's gradient RMS; input / f_m gradient norms and samples likewise.
M4 replays the driver's step (train_amos_atlas_final.py:326-377): two live graphs, frozen parameters, detached inputs.
bf16 under autocast is measured against the torch restatement under autocast (DESIGN §10 convention)."""
import numpy as np
import pytest
import torch

import disc_cases as DC
import disc_reference as DR
from conftest import golden

pytestmark = pytest.mark.gpu


def _native(kind, gpu):
    import unet3D
    m = getattr(unet3D, DC.KINDS[kind])(DC.NUM_CLASSES, DC.NDF)
    w = DC.fill(m)
    return m.to(gpu).train(), w


def _inputs(tag, gpu, grad=True):
    inp = DC.case_inputs(tag)
    x = torch.from_numpy(inp["x"]).to(gpu).requires_grad_(grad)
    f_m = [torch.from_numpy(f).to(gpu).requires_grad_(grad) for f in inp.get("f_m", [])]
    return inp, x, f_m


def _check_logits(got, want, what):
    want = np.asarray(want, np.float64)
    err = np.abs(got.detach().double().cpu().numpy() - want).max()
    print(f"{what}: logits max-abs error {err:.3e}, max |logit| {np.abs(want).max():.3e}")
    assert err <= 1e-3 * np.abs(want).max(), (what, err)


def _check_param_grads(m, g, tag):
    names, norms, gidx, gval = DC.grad_summary([(k, p.grad) for k, p in m.named_parameters()])
    assert list(names) == [str(n) for n in g[f"{tag}_gnames"]]
    np.testing.assert_array_equal(gidx, g[f"{tag}_gidx"])
    numel = dict((k, p.numel()) for k, p in m.named_parameters())
    for i, k in enumerate(names):
        want = float(g[f"{tag}_gnorm"][i])
        rms = want / np.sqrt(numel[str(k)])
        e = np.abs(gval[i] - g[f"{tag}_gval"][i]).max()
        print(f"{tag} {k}: grad norm {norms[i]:.6e} (fixture {want:.6e}), sampled max error / rms {e / rms:.3e}")
        assert abs(norms[i] - want) <= 2e-3 * want, (tag, k, norms[i], want)
        assert e <= 0.1 * rms, (tag, k, e, rms)


def _check_tensor_grad(t, g, tag, key, *skey):
    norm, val = DC.tensor_summary(t.grad, *skey)
    want = float(g[f"{tag}_{key}_norm"])
    rms = want / np.sqrt(t.numel())
    e = np.abs(val - g[f"{tag}_{key}_val"]).max()
    print(f"{tag} {key}: grad norm {norm:.6e} (fixture {want:.6e}), sampled max error / rms {e / rms:.3e}")
    assert abs(norm - want) <= 2e-3 * want, (tag, key, norm, want)
    assert e <= 0.1 * rms, (tag, key, e, rms)


@pytest.mark.parametrize("tag", ["M1", "M2", "M3"])
def test_model_fp32_against_fixture(gpu, tag):
    g = golden("g17_disc.npz")
    kind = DC.GEOM[tag][0]
    m, w = _native(kind, gpu)
    inp, x, f_m = _inputs(tag, gpu)
    assert DC.checksum(inp, w) == pytest.approx(float(g[f"{tag}_insum"]), rel=1e-12)
    lg = m(x, f_m) if kind == "deep" else m(x)
    assert lg.shape == g[f"{tag}_logits"].shape and lg.dtype == torch.float32
    _check_logits(lg, g[f"{tag}_logits"], tag)
    (lg * torch.from_numpy(DC.projection(tag, tuple(lg.shape))).to(gpu)).sum().backward()
    _check_param_grads(m, g, tag)
    _check_tensor_grad(x, g, tag, "dx", int(tag[1]), 0)
    for i, f in enumerate(f_m):
        _check_tensor_grad(f, g, tag, f"df{i}", int(tag[1]), 1 + i)


def test_non_contiguous_input_is_made_contiguous(gpu):
    g = golden("g17_disc.npz")
    m, _ = _native("norm", gpu)
    _, x, _ = _inputs("M1", gpu, grad=False)
    xt = x.permute(0, 1, 4, 2, 3).contiguous().permute(0, 1, 3, 4, 2)
    assert not xt.is_contiguous()
    with torch.no_grad():
        _check_logits(m(xt), g["M1_logits"], "M1 non-contiguous")


def test_m4_driver_step(gpu):
    from loss_functions.losses import SmoothCrossEntropyLoss, bce_loss
    g = golden("g17_disc_step.npz")
    m, w = _native("deep", gpu)
    inp, x, f_m = _inputs("M4", gpu)
    assert DC.checksum(inp, w) == pytest.approx(float(g["M4_insum"]), rel=1e-12)
    flist, clist = DC.FLIST, list(range(x.shape[0]))
    label_t = torch.tensor(DC.LABEL_T)
    opt = torch.optim.Adam(m.parameters(), lr=1e-4)
    opt.zero_grad()
    for p in m.parameters():
        p.requires_grad = False
    d_output = m(x[flist], [f[flist] for f in f_m])
    loss_d = bce_loss(d_output, 1)
    first = d_output.detach().clone()
    for p in m.parameters():
        p.requires_grad = True
    d_output_ = m(x.detach()[clist], [f.detach()[clist] for f in f_m])
    loss_d_ = SmoothCrossEntropyLoss()(d_output_, label_t[clist].to(gpu))
    # both forwards before either backward: the second did not disturb the first graph's result
    assert torch.equal(d_output.detach(), first)
    _check_logits(d_output, g["M4_gen_logits"], "M4 generator pass")
    _check_logits(d_output_, g["M4_dis_logits"], "M4 discriminator pass")
    assert float(loss_d.detach()) == pytest.approx(float(g["M4_loss_d"]), rel=1e-3)
    assert float(loss_d_.detach()) == pytest.approx(float(g["M4_loss_d_"]), rel=1e-3)
    (loss_d * 0.01).backward()
    # the generator pass leaves parameter .grad untouched (None in the reference: fixture)
    assert bool(g["M4_gen_pgrad_none"].all())
    assert all(p.grad is None for p in m.parameters())
    _check_tensor_grad(x, g, "M4", "dx", 4, 0)
    for i, f in enumerate(f_m):
        _check_tensor_grad(f, g, "M4", f"df{i}", 4, 1 + i)
    rest = [i for i in clist if i not in flist]
    assert float(x.grad[rest].abs().max()) == float(g["M4_dx_rest_absmax"]) == 0.0
    xg = x.grad.clone()
    loss_d_.backward()
    _check_param_grads(m, g, "M4")
    assert torch.equal(x.grad, xg)   # detached inputs: the discriminator pass sends nothing back
    # the driver's Adam step writes the parameters in place: the cached weight packs must follow
    with torch.no_grad():
        from u3d import disc
        before = m(x.detach()[clist], [f.detach()[clist] for f in f_m])
        stats = dict(disc.PACK_STATS)
        again = m(x.detach()[clist], [f.detach()[clist] for f in f_m])
        assert disc.PACK_STATS["miss"] == stats["miss"] and disc.PACK_STATS["hit"] > stats["hit"]  # packs reused
        assert torch.equal(before, again) and torch.equal(before, d_output_.detach())
        opt.step()
        after = m(x.detach()[clist], [f.detach()[clist] for f in f_m])
    assert not torch.equal(before, after)
    ref = DR.DeepDisc(DC.NUM_CLASSES, DC.NDF)
    ref.load_state_dict({k: v.cpu() for k, v in m.state_dict().items()})
    with torch.no_grad():
        want = ref.double()(x.detach().cpu().double(), [f.detach().cpu().double() for f in f_m])
    _check_logits(after, want.numpy(), "M4 after the Adam step")


@pytest.mark.parametrize("kind", ["norm", "deep"])
def test_m6_empty_batch(gpu, kind):
    """B = 0 (an empty flist): the reference module raises in its forward on the CPU (fixture M6: fwd_ok = 0); the
    native module returns an empty [0, 2] attached to the graph, and its backward yields zero gradients."""
    g = golden("g17_disc.npz")
    assert int(g[f"M6_{kind}_fwd_ok"]) == 0 and str(g[f"M6_{kind}_error"]) == "RuntimeError"
    m, _ = _native(kind, gpu)
    x = torch.zeros((0, DC.NUM_CLASSES, 64, 64, 64), device=gpu, requires_grad=True)
    f_m = [torch.zeros((0, 1) + DC.halve((64, 64, 64), 3 - i), device=gpu, requires_grad=True) for i in range(3)]
    out = m(x, f_m) if kind == "deep" else m(x)
    assert out.shape == (0, 2) and out.requires_grad
    out.sum().backward()
    assert x.grad is not None and x.grad.shape == x.shape
    for p in m.parameters():
        assert p.grad is None or float(p.grad.abs().sum()) == 0.0
    if kind == "deep":
        assert all(f.grad is None or f.grad.numel() == 0 for f in f_m)


def test_seq_discriminator_matches_restatement(gpu):
    """get_style_discriminator_output: the same six-conv chain with Linear(8 ndf, 1), against the fp64 restatement.
    Gradients are held to the norm bound of the fixture tests (rtol 2e-3), not to an entry-wise one: a LeakyReLU
    pre-activation that fp32 puts on the other side of zero moves every gradient below it (on M1's volume one
    block3 pre-activation is 3.9e-7 and flips; with the native run's own masks the fp64 backward agrees to 2e-6)."""
    m, _ = _native("seq", gpu)
    ref = DR.SeqDisc(DC.NUM_CLASSES, DC.NDF)
    DC.fill(ref)
    _, x, _ = _inputs("M1", gpu)
    out = m(x)
    assert out.shape == (2, 1)
    xr = x.detach().cpu().double().requires_grad_(True)
    want = ref.double()(xr)
    _check_logits(out, want.detach().numpy(), "seq")
    out.sum().backward()
    want.sum().backward()
    pairs = [(k, p.grad, q.grad) for (k, p), (_, q) in zip(m.named_parameters(), ref.named_parameters())]
    for k, got, ref_g in pairs + [("dx", x.grad, xr.grad)]:
        a, b = got.double().cpu().norm().item(), ref_g.norm().item()
        print(f"seq {k}: grad norm {a:.6e} (fp64 {b:.6e})")
        assert abs(a - b) <= 2e-3 * b, (k, a, b)


def test_bf16_autocast_m2_against_torch_yardstick(gpu):
    """bf16 operands, fp32 accumulation under torch.autocast: the native error against the fp64 CPU result must be
    <= 1.5 x the error of the torch restatement under autocast on the same device (MIOpen convs) + 1e-2, rel L2."""
    ref = DR.DeepDisc(DC.NUM_CLASSES, DC.NDF)
    DC.fill(ref)
    inp = DC.case_inputs("M2")

    def run(mod, device, dtype, autocast):
        x = torch.from_numpy(inp["x"]).to(device).to(dtype).requires_grad_(True)
        f_m = [torch.from_numpy(f).to(device).to(dtype).requires_grad_(True) for f in inp["f_m"]]
        with torch.autocast("cuda", torch.bfloat16, enabled=autocast):
            lg = mod(x, f_m)
        proj = torch.from_numpy(DC.projection("M2", tuple(lg.shape))).to(device).to(lg.dtype)
        (lg * proj).sum().backward()
        grads = {k: p.grad.detach().double().cpu() for k, p in mod.named_parameters()}
        grads.update({f"df{i}": f.grad.detach().double().cpu() for i, f in enumerate(f_m)})
        return lg.detach().double().cpu(), x.grad.double().cpu(), grads

    want = run(ref.double(), "cpu", torch.float64, False)
    yard_mod = DR.DeepDisc(DC.NUM_CLASSES, DC.NDF)
    DC.fill(yard_mod)
    yard = run(yard_mod.to(gpu), gpu, torch.float32, True)
    m, _ = _native("deep", gpu)
    got = run(m, gpu, torch.float32, True)

    def rel(a, b):
        return ((a - b).norm() / b.norm()).item()

    pairs = [("logits", rel(got[0], want[0]), rel(yard[0], want[0])), ("dx", rel(got[1], want[1]), rel(yard[1], want[1]))]
    pairs += [(k, rel(got[2][k], want[2][k]), rel(yard[2][k], want[2][k])) for k in want[2]]
    for what, e_native, e_yard in pairs:
        print(f"bf16 M2 {what}: native rel L2 {e_native:.3e}, torch autocast yardstick {e_yard:.3e}")
    for what, e_native, e_yard in pairs:
        assert e_native <= 1.5 * e_yard + 1e-2, (what, e_native, e_yard)


def test_in_place_change_between_forward_and_backward_raises(gpu):
    """The backward reads the inputs and repacks the weights from the parameters: an in-place write after the forward
    (an optimizer step before the backward) must raise, as autograd's saved-tensor check would, not use new values."""
    m, _ = _native("norm", gpu)
    _, x, _ = _inputs("M1", gpu)
    out = m(x[:1])
    with torch.no_grad():
        m.block2[0].weight.mul_(0.5)
    with pytest.raises(RuntimeError, match="modified in place"):
        out.sum().backward()
