"""tests/disc_reference.py is the yardstick of the discriminator kernel tests, so it is pinned itself: the three modules
in fp64 against the G17 fixtures (the reference's modules run in fp64) at 1e-6 — logits, every parameter-gradient norm and
sampled entry, the input and f_m gradients — and the space-to-depth / parity-class identities the kernels are built on
against F.conv3d and its autograd in fp64."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import disc_cases as DC
import disc_reference as DR
from conftest import golden

RTOL = 1e-6


def _rel(a, b):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    return np.abs(a - b).max() / max(np.abs(b).max(), 1e-30)


def _run(tag, dtype):
    kind = DC.GEOM[tag][0]
    m = DR.KINDS[kind](DC.NUM_CLASSES, DC.NDF)
    w = DC.fill(m)
    m.to(dtype)
    inp = DC.case_inputs(tag)
    x = torch.from_numpy(inp["x"]).to(dtype).requires_grad_(True)
    f_m = [torch.from_numpy(f).to(dtype).requires_grad_(True) for f in inp.get("f_m", [])]
    lg = m(x, f_m) if kind == "deep" else m(x)
    (lg * torch.from_numpy(DC.projection(tag, tuple(lg.shape))).to(dtype)).sum().backward()
    return m, inp, w, x, f_m, lg


@pytest.fixture(scope="module")
def runs():
    """fp64 forward + backward of M1-M3 through the restatement, once."""
    return {tag: _run(tag, torch.float64) for tag in ("M1", "M2", "M3")}


@pytest.mark.parametrize("tag", ["M1", "M2", "M3"])
def test_restatement_matches_fixture(runs, tag):
    g = golden("g17_disc.npz")
    m, inp, w, x, f_m, lg = runs[tag]
    assert DC.checksum(inp, w) == pytest.approx(float(g[f"{tag}_insum"]), rel=1e-12)
    assert _rel(lg.detach().numpy(), g[f"{tag}_logits"]) < RTOL
    names, norms, gidx, gval = DC.grad_summary([(k, p.grad) for k, p in m.named_parameters()])
    assert list(names) == [str(n) for n in g[f"{tag}_gnames"]]
    np.testing.assert_array_equal(gidx, g[f"{tag}_gidx"])
    np.testing.assert_allclose(norms, g[f"{tag}_gnorm"], rtol=RTOL)
    for i in range(len(names)):
        want = g[f"{tag}_gval"][i]
        assert np.abs(gval[i] - want).max() <= RTOL * np.abs(want).max(), names[i]
    for key, t in [("dx", x)] + [(f"df{i}", f) for i, f in enumerate(f_m)]:
        norm, val = DC.tensor_summary(t.grad, int(tag[1]), 0 if key == "dx" else 1 + int(key[2]))
        want = g[f"{tag}_{key}_val"]
        assert norm == pytest.approx(float(g[f"{tag}_{key}_norm"]), rel=RTOL)
        assert np.abs(val - want).max() <= RTOL * np.abs(want).max(), key


def test_fixture_samples_reach_different_logits():
    g = golden("g17_disc.npz")
    for tag in ("M1", "M2"):
        lg = g[f"{tag}_logits"].astype(np.float64)
        assert np.abs(lg[0] - lg[1]).max() > 100 * 1e-3 * np.abs(lg).max()


@pytest.mark.parametrize("dims", [(6, 10, 12), (5, 9, 7), (2, 2, 2), (4, 7, 3)])
def test_space_to_depth_identity(dims):
    rng = torch.Generator().manual_seed(3)
    x = torch.randn((2, 3) + dims, dtype=torch.float64, generator=rng)
    w = torch.randn((5, 3, 4, 4, 4), dtype=torch.float64, generator=rng)
    want = F.conv3d(x, w, stride=2, padding=1)
    got = DR.conv4_s2d(x, w)
    assert got.shape == want.shape == (2, 5) + tuple(v // 2 for v in dims)
    assert (got - want).abs().max() < 1e-12


@pytest.mark.parametrize("dims", [(6, 10, 12), (5, 9, 7), (2, 2, 2), (4, 7, 3)])
def test_parity_class_data_gradient_identity(dims):
    rng = torch.Generator().manual_seed(4)
    x = torch.randn((2, 3) + dims, dtype=torch.float64, generator=rng).requires_grad_(True)
    w = torch.randn((5, 3, 4, 4, 4), dtype=torch.float64, generator=rng)
    y = F.conv3d(x, w, stride=2, padding=1)
    g = torch.randn(y.shape, dtype=torch.float64, generator=rng)
    (y * g).sum().backward()
    got = DR.dgrad_parity(g, w, dims)
    assert (got - x.grad).abs().max() < 1e-12


def test_lrelu_grad_from_stored_output_matches_autograd():
    pre = torch.tensor([-2.0, -0.0, 0.0, 1e-30, 3.0], dtype=torch.float64, requires_grad=True)
    y = F.leaky_relu(pre, DR.SLOPE)
    dy = torch.tensor([1.0, 2.0, 3.0, 4.0, 5.0], dtype=torch.float64)
    (y * dy).sum().backward()
    assert torch.equal(DR.lrelu_grad(dy, y.detach()), pre.grad)
