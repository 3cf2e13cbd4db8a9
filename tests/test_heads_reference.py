"""The fp64 references of the EAM and dynamic heads (heads_reference.py) against independent statements of the same
mathematics, in fp64 with torch's autograd:

  * oracle.ref_cpu.eam_attn(...).mean(1): the full multi-head q k^T form of the reference model, so agreement also
    proves the head-mean folding M = (1/h) q Wk; F.layer_norm for the per-voxel side with M as a leaf (dM);
  * oracle.ref_cpu.unet3d_dyn_forward from its GAP onwards (one-hot concatenation, controller conv, split_with_sizes,
    grouped F.conv3d heads), with the trunk, precls and the GAP's GroupNorm replaced by tensors the test supplies.

Tolerance: both sides are fp64 (unit roundoff 2^-53 = 1.1e-16) and differ only in the order of operations. The
longest sums here have 263 terms (controller) or v * c <= 100 * 128 products (the EAM reductions); a worst-case chain
of 12800 roundings is 1.4e-12 of the abs-sum, random-walk growth sqrt(12800) ~ 113 roundings is 1.3e-14. RTOL = 1e-12
of the largest magnitude of the quantity compared sits between the two (the equal-channel voxel, whose rstd is 316,
multiplies the rounding of its mean, which is why the random-walk figure alone is not taken), and 6e4 times below the
2^-24 the GPU tests resolve. Each comparison prints its figure ("RELERR <name> <value>"); the largest is 2.7e-14.
"""
import pytest
import torch
import torch.nn.functional as F

import oracle.ref_cpu as O
import heads_reference as R

RTOL = 1e-12
F64 = torch.float64


def _close(name, got, want):
    scale = want.abs().max().item()
    err = (got - want).abs().max().item()
    assert got.shape == want.shape, name
    print(f"RELERR {name} {err / max(scale, 1e-300):.2e}")
    assert err <= RTOL * max(scale, 1e-300), f"{name}: {err:.3e} vs {RTOL * scale:.3e}"


def _eam_inputs(n, v, c, nt, seed):
    gen = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=gen)                                    # noqa: E731
    x = (r(n, v, c) + 0.3).double()
    x[0, v // 2] = 0.7                                                              # a voxel of equal channels
    return dict(x=x, tok=r(nt, c).double(), g2=(0.5 + r(c).abs()).double(), b2=r(c).double(),
                g3=(0.5 + r(c).abs()).double(), b3=r(c).double(), wq=(r(c, c) / c ** 0.5).double(),
                kv=(r(2 * c, c) / c ** 0.5).double(), gout=r(n, nt, v).double())


EAM_CASES = [(1, 64, 128, 13), (1, 3, 32, 13), (1, 77, 32, 1), (2, 100, 64, 16), (1, 9, 24, 3)]


@pytest.mark.parametrize("n,v,c,nt", EAM_CASES, ids=str)
def test_eam_refs_match_oracle(n, v, c, nt):
    heads = 4
    I = _eam_inputs(n, v, c, nt, 3 + v + c)
    leaf = {k: I[k].clone().requires_grad_(True) for k in ("x", "g2", "b2", "g3", "b3", "wq", "kv")}
    P = {"e.norm2.weight": leaf["g2"], "e.norm2.bias": leaf["b2"], "e.norm3.weight": leaf["g3"],
         "e.norm3.bias": leaf["b3"], "e.q.weight": leaf["wq"], "e.kv.weight": leaf["kv"]}
    # the attention is per voxel, so the n samples run as one sequence of n * v (the oracle, like the model, takes B = 1)
    att = O.eam_attn(P, "e.", leaf["x"].reshape(1, n * v, c), I["tok"].reshape(1, nt, c), heads).mean(1)
    att = att.reshape(nt, n, v).permute(1, 0, 2)
    (att * I["gout"]).sum().backward()

    wk = I["kv"][:c]
    tk = R.eam_token_ref(I["tok"], I["g3"], I["b3"], I["wq"], wk, 1.0 / heads)
    _close("zhat", tk.zhat, F.layer_norm(I["tok"], (c,), None, None, 1e-5))
    _close("q", tk.q, F.linear(F.layer_norm(I["tok"], (c,), I["g3"], I["b3"], 1e-5), I["wq"]))
    fw = R.eam_fwd_ref(I["x"], I["g2"], I["b2"], tk.M, chunk=37)                     # several chunks, the last partial
    _close("att", fw.att, att.detach())
    bw = R.eam_bwd_ref(I["x"], I["g2"], I["b2"], tk.M, I["gout"])
    _close("dx", bw.dx, leaf["x"].grad)
    _close("dg2", bw.dg2, leaf["g2"].grad)
    _close("db2", bw.db2, leaf["b2"].grad)
    # dM with M as a leaf of the per-voxel side alone
    Ml = tk.M.clone().requires_grad_(True)
    xn = F.layer_norm(I["x"], (c,), I["g2"], I["b2"], 1e-5)
    (torch.einsum("tc,nvc->ntv", Ml, xn) * I["gout"]).sum().backward()
    _close("dM", bw.dM, Ml.grad)
    pb = R.eam_param_bwd_ref(bw.dM, tk.zhat, tk.q, I["g3"], I["b3"], I["wq"], wk, 1.0 / heads)
    _close("dWq", pb.dwq, leaf["wq"].grad)
    _close("dkv", pb.dkv, leaf["kv"].grad)
    assert not pb.dkv[c:].any() and not leaf["kv"].grad[c:].any()
    _close("dg3", pb.dg3, leaf["g3"].grad)
    _close("db3", pb.db3, leaf["b3"].grad)
    # the abs-sums bound the sums they belong to, and are the same formulas on |operands|
    one = 1 + 1e-12
    assert bool((tk.q.abs() <= tk.q_abs * one).all()) and bool((tk.M.abs() <= tk.M_abs * one).all())
    assert bool(((fw.att - (tk.M @ I["b2"])[None, :, None]).abs() <= fw.att_abs * one + 1e-13).all())
    assert bool((bw.dl.abs() <= bw.dl_abs * one).all())
    for a, b in ((bw.P, bw.P_abs), (bw.Gs, bw.Gs_abs), (bw.dg2, bw.dg2_abs), (bw.db2, bw.db2_abs), (pb.dq, pb.dq_abs),
                 (pb.dz, pb.dz_abs), (pb.dwq, pb.dwq_abs), (pb.dkv[:c], pb.dkv_abs), (pb.dg3, pb.dg3_abs),
                 (pb.db3, pb.db3_abs)):
        assert bool((a.abs() <= b * one).all())
    _close("a0_abs", fw.a0_abs, (tk.M * I["b2"]).abs().sum(1))
    eq = fw.s2[0, v // 2].item()
    assert eq <= 1e-28 and abs(fw.rstd[0, v // 2].item() * 1e-5 ** 0.5 - 1) < 1e-12   # the equal-channel voxel: rstd = 1/sqrt(eps)


DYN_CASES = [(1, 1, 1), (1, 255, 8), (2, 257, 72), (3, 1000, 1)]


@pytest.mark.parametrize("n,v,vb", DYN_CASES, ids=str)
def test_dyn_refs_match_oracle(monkeypatch, n, v, vb):
    gen = torch.Generator().manual_seed(17 + v)
    r = lambda *s: torch.randn(*s, generator=gen).double()                           # noqa: E731
    task = torch.tensor([(2 * i + v) % 7 for i in range(n)])
    bott = r(n, 256, vb, 1, 1).requires_grad_(True)            # the GAP input; its mean over the voxels is feat
    hd = r(n, 8, v, 1, 1).requires_grad_(True)                 # precls_conv's output, NCDHW
    wc = (r(162, 263, 1, 1, 1) / 8).requires_grad_(True)
    bc = r(162).requires_grad_(True)
    monkeypatch.setattr(O, "trunk", lambda P, x, ws=True: (None, bott))
    monkeypatch.setattr(O, "gn_relu", lambda x, groups, gamma, beta: x)
    monkeypatch.setattr(O, "precls", lambda P, y, groups: hd)
    P = {"GAP.0.weight": None, "GAP.0.bias": None, "controller.weight": wc, "controller.bias": bc}
    out = O.unet3d_dyn_forward(P, torch.zeros(n, 1, 1, 1, 1), task)                  # [n, 2, v, 1, 1]
    dout = r(n, 2, v, 1, 1)
    (out * dout).sum().backward()

    feat = bott.detach().mean(dim=(2, 3, 4))
    h = hd.detach().reshape(n, 8, v).permute(0, 2, 1)          # [n, v, 8]
    d = dout.reshape(n, 2, v).permute(0, 2, 1)
    w2d = wc.detach().reshape(162, 263)
    ct = R.controller_ref(feat, task, w2d, bc.detach())
    fw = R.dynhead_fwd_ref(h, ct.params)
    _close("out", fw.out, out.detach().reshape(n, 2, v).permute(0, 2, 1))
    bw = R.dynhead_bwd_ref(h, ct.params, d)
    _close("dh", bw.dh, hd.grad.reshape(n, 8, v).permute(0, 2, 1))
    cb = R.controller_bwd_ref(feat, task, w2d, bw.dparams, vb)
    _close("dWc", cb.dw, wc.grad.reshape(162, 263))
    _close("dbc", cb.db, bc.grad)
    _close("dA", cb.dA[:, :, None].expand(n, 256, vb), bott.grad.reshape(n, 256, vb))
    # dparams itself: autograd with params as the leaf of the heads alone
    pl = ct.params.clone().requires_grad_(True)
    w1, w2, w3, b1, b2, b3 = R.split_params(pl)
    a = F.relu(torch.einsum("nok,nvk->nvo", w1, h) + b1[:, None])
    a = F.relu(torch.einsum("nok,nvk->nvo", w2, a) + b2[:, None])
    ((torch.einsum("nok,nvk->nvo", w3, a) + b3[:, None]) * d).sum().backward()
    _close("dparams", bw.dparams, pl.grad)
    one = 1 + 1e-12
    for a_, b_ in ((ct.params, ct.abs), (fw.a1, fw.a1_abs), (fw.a2, fw.a2_abs), (fw.out, fw.out_abs),
                   (bw.dparams, bw.dparams_abs), (bw.dh, bw.dh_abs1), (bw.dh_abs1, bw.dh_abs), (cb.dw, cb.dw_abs),
                   (cb.db, cb.db_abs), (cb.dA, cb.dA_abs)):
        assert bool((a_.abs() <= b_ * one).all())
    assert torch.equal(R.join_params(*R.split_params(ct.params)), ct.params)
