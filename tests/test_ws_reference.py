"""The fp64 references of the weight path (ws_reference.py) against what they restate: oracle.ref_cpu.ws_weight in
fp64, torch's autograd of sum(ws_weight(w) * G), and torch.optim.SGD on fp64 CPU tensors, at the shapes of
test_gpu_wstd.py. The formulas are the same mathematics; only the order of fp64 operations
differs."""
import numpy as np
import pytest
import torch

import oracle.ref_cpu as O
from ws_reference import SHAPES, f32, pack_dgrad, pack_fwd, sgd_ref, unpack, ws_bwd_ref, ws_ref

SMALL = SHAPES  # weight-sized: all of them are small on a CPU as well
SGD_KW = [dict(momentum=0.9, weight_decay=1e-4), dict(momentum=0.0),
          dict(momentum=0.8, dampening=0.1, weight_decay=1e-3),
          dict(momentum=0.9, nesterov=True), dict(momentum=0.5, maximize=True)]   # those of test_gpu_optim.py


def _omd(dampening):
    return float(np.float32(1.0) - np.float32(dampening))


def _weight(cout, cin, k, seed):
    gen = torch.Generator().manual_seed(seed)
    w = 0.1 * torch.randn(cout, cin, k, k, k, generator=gen) + 0.02
    return w, gen


@pytest.mark.parametrize("cout,cin,k,std", SMALL, ids=str)
def test_ws_ref_matches_oracle(cout, cin, k, std):
    w, _ = _weight(cout, cin, k, 5 + cout + cin)
    wh, mean, sd = ws_ref(w)
    want = O.ws_weight(w.double())
    assert (wh - want).abs().max().item() <= 1e-12 * want.abs().max().item()
    rows = w.double().reshape(cout, -1)
    assert (mean - rows.mean(1)).abs().max().item() <= 1e-12 * rows.abs().max().item()
    sd_want = torch.sqrt(torch.var(rows - rows.mean(1, keepdim=True), dim=1) + 1e-12)
    assert ((sd - sd_want).abs() <= 1e-12 * sd_want).all()


@pytest.mark.parametrize("cout,cin,k,std", SMALL, ids=str)
def test_ws_bwd_ref_matches_autograd(cout, cin, k, std):
    w, gen = _weight(cout, cin, k, 9 + cout + cin)
    wh, _, _ = ws_ref(w)
    G = (0.7 * wh + 0.3 + 0.5 * torch.randn(w.shape, generator=gen)).float().double()
    ref = ws_bwd_ref(w, G, std)
    wa = w.double().requires_grad_(True)
    ((O.ws_weight(wa) if std else wa) * G).sum().backward()
    assert (ref.dw - wa.grad).abs().max().item() <= 1e-10 * wa.grad.abs().max().item()
    K = cin * k ** 3
    rows, whr = G.reshape(cout, -1), (wh if std else w.double()).reshape(cout, -1)
    assert torch.equal(ref.A1.flatten(), rows.abs().sum(1))
    assert (ref.A2.flatten() - (rows * whr).abs().sum(1)).abs().max().item() <= 1e-12 * ref.A2.max().item()
    if std:   # the sums of |terms| bound the sums themselves
        assert bool((ref.F1.abs() * K <= ref.A1 * (1 + 1e-12)).all())
        assert bool((ref.F2.abs() * (K - 1) <= ref.A2 * (1 + 1e-12)).all())


@pytest.mark.parametrize("cout,cin,k,std", SMALL, ids=str)
def test_packs(cout, cin, k, std):
    w, _ = _weight(cout, cin, k, 1)
    pf, pd = pack_fwd(w), pack_dgrad(w)
    k3, cp, cip = k ** 3, (cout + 31) // 32 * 32, (cin + 31) // 32 * 32
    assert pf.shape == (k3, cp, cip) and pd.shape == (k3, cip, cp)
    assert torch.equal(pd, pf.transpose(1, 2))
    for t, co, ci in ((0, 0, 0), (k3 - 1, cout - 1, cin - 1), (k3 // 2, cout // 2, cin // 3)):
        assert pf[t, co, ci] == w.reshape(cout, cin, k3)[co, ci, t]
    assert not pf[:, cout:].any() and not pf[:, :, cin:].any() and (pf != 0).sum() == (w != 0).sum()  # zero padding
    assert torch.equal(unpack(pf, w.shape), w)
    assert bool((pack_fwd(w, pad=7.0)[:, cout:] == 7).all()) and bool((pack_fwd(w, pad=7.0)[:, :, cin:] == 7).all())


@pytest.mark.parametrize("kw", SGD_KW, ids=str)
def test_sgd_ref_matches_torch(kw):
    """torch.optim.SGD is handed the values the kernel's float arguments carry: fp32 roundings of lr, momentum and
    weight_decay, and the dampening d' with 1 - d' == fp32(1 - fp32(dampening)) exactly (1 - x is exact in fp64 for
    x in [0.5, 1], both ways)."""
    gen = torch.Generator().manual_seed(11)
    shapes = [(32, 1, 3, 3, 3), (7,), (5, 3)]
    ps = [torch.randn(s, generator=gen) for s in shapes]
    ta = [torch.nn.Parameter(p.double()) for p in ps]
    lr = 0.05
    tkw = {a: (f32(v) if a in ("momentum", "weight_decay") else v) for a, v in kw.items()}
    if "dampening" in kw:
        tkw["dampening"] = 1.0 - _omd(kw["dampening"])
    opt = torch.optim.SGD(ta, lr=f32(lr), **tkw)
    mine = [(p.double(), None) for p in ps]
    for it in range(3):
        if it == 2:
            lr = 0.01
            opt.param_groups[0]["lr"] = f32(lr)
        gs = [torch.randn(s, generator=gen) for s in shapes]
        for a, g in zip(ta, gs):
            a.grad = g.double()
        opt.step()
        mine = [sgd_ref(p, g, b, lr, kw.get("momentum", 0.0), kw.get("dampening", 0.0), kw.get("weight_decay", 0.0),
                        kw.get("nesterov", False), kw.get("maximize", False), init=it == 0)
                for (p, b), g in zip(mine, gs)]
        for a, (p, b) in zip(ta, mine):
            assert (p - a.detach()).abs().max().item() <= 1e-12 * a.detach().abs().max().item()
            tb = opt.state[a].get("momentum_buffer")
            assert (tb is None) == (b is None)
            if b is not None:
                assert (b - tb).abs().max().item() <= 1e-12 * tb.abs().max().item()
