"""eam_pool_reference.py (the folded fp64 statement of the EAM class message that test_gpu_eam_pool.py measures the
kernels against) pinned on the CPU to torch autograd of the attention as it is usually written: LayerNorm, a kv
projection of every voxel, per-head softmax(q k^T scale) @ v, proj(norm2(.)) + residual. cm, the head-mean score map
and every gradient (x, token, kv, q, proj, norm2, norm3) agree to 1e-10 of the tensor's largest magnitude in fp64, for
a gradient on cm alone, on the map alone and on both."""
import pytest
import torch
import torch.nn.functional as F

import eam_pool_reference as R

F64 = torch.float64
CASES = [(32, 500, 13), (128, 64, 14), (64, 100, 16), (32, 3, 1)]     # (c, voxels, tokens)
RTOL = 1e-10


def _operands(c, v, nt):
    gen = torch.Generator().manual_seed(c + 3 * v + nt)
    r = lambda *s: torch.randn(*s, generator=gen, dtype=F64)           # noqa: E731
    p = dict(kv=r(2 * c, c) / c ** 0.5, q=r(c, c) / c ** 0.5, proj_w=r(c, c) / c ** 0.5, proj_b=0.3 * r(c),
             g2=0.4 + 1.6 * torch.rand(c, generator=gen, dtype=F64), b2=0.5 + 0.8 * r(c),
             g3=0.4 + 1.6 * torch.rand(c, generator=gen, dtype=F64), b3=0.5 + 0.8 * r(c))
    return r(v, c) + 0.5 * r(v, 1), 3.0 * r(nt, c), p, r(nt, c), r(nt, v)


def _direct(x, tok, p, heads=4):
    v, c = x.shape
    nt, hd = tok.shape[0], c // heads
    xn = F.layer_norm(x, (c,), p["g2"], p["b2"], 1e-5)
    tn = F.layer_norm(tok, (c,), p["g3"], p["b3"], 1e-5)
    kv = (xn @ p["kv"].t()).reshape(v, 2, heads, hd).permute(1, 2, 0, 3)
    k, val = kv[0], kv[1]                                             # [heads, v, hd]
    q = (tn @ p["q"].t()).reshape(nt, heads, hd).permute(1, 0, 2)     # [heads, nt, hd]
    attn = q @ k.transpose(-2, -1)                                    # [heads, nt, v]
    o = (torch.softmax(attn * hd ** -0.5, -1) @ val).transpose(0, 1).reshape(nt, c)
    return F.linear(F.layer_norm(o, (c,), p["g2"], p["b2"], 1e-5), p["proj_w"], p["proj_b"]) + o, attn.mean(0), attn


def _close(name, got, want, ref=None):
    """ref: the magnitude the error is measured against, where the value itself is a cancelled sum."""
    err = (got - want).abs().max().item()
    ref = want.abs().max().item() if ref is None else ref
    assert err <= RTOL * ref, f"{name}: {err:.3e} against max |ref| {ref:.3e}"


@pytest.mark.parametrize("mode", ["cm", "att", "both"])
@pytest.mark.parametrize("c,v,nt", CASES, ids=str)
def test_folded_math_matches_direct_attention(c, v, nt, mode):
    x, tok, p, gcm, gatt = _operands(c, v, nt)
    gcm = gcm if mode != "att" else None
    gatt = gatt if mode != "cm" else None
    ref = R.eam_ref(x, tok, p, gcm, gatt)
    leaves = {k: t.clone().requires_grad_(True) for k, t in dict(p, x=x, tok=tok).items()}
    cm, att, attn = _direct(leaves["x"], leaves["tok"], {k: leaves[k] for k in p})
    if v > 8:   # the softmax is far from uniform, so its backward carries weight
        pmax = torch.softmax(attn * (c // 4) ** -0.5, -1).max(-1).values
        assert (pmax >= 8.0 / v).double().mean() >= 0.5
    _close("cm", ref.cm, cm.detach())
    _close("att", ref.att, att.detach())
    loss = (cm * gcm).sum() if gcm is not None else 0
    loss = loss + ((att * gatt).sum() if gatt is not None else 0)
    loss.backward()
    for k, leaf in leaves.items():
        want = leaf.grad if leaf.grad is not None else torch.zeros_like(leaf)
        if mode == "att" and k in ("proj_w", "proj_b"):
            assert not bool(ref.grad[k].any()) and not bool(want.any())
            continue
        _close("d" + k, ref.grad[k], want)
    # the two statements of the norm2 gradients of the voxel side (per voxel, and from the block sums) are one
    # (sum_n dS = 0 row by row when only cm carries a gradient: db2 of the voxel side is then a sum that cancels)
    b = ref.bwd
    _close("dg2 forms", b.dg2, b.dg2_direct, (ref.A.abs() * b.PS_abs).sum(0).max().item())
    _close("db2 forms", b.db2, b.db2_direct, (ref.A.abs() * b.Gs_abs[:, None]).sum(0).max().item())


def test_reference_intermediates_are_consistent():
    x, tok, p, gcm, gatt = _operands(64, 100, 16)
    ref = R.eam_ref(x, tok, p, gcm, gatt)
    f, b = ref.fwd, ref.bwd
    assert torch.allclose(f.P.sum(1), torch.ones(64, dtype=F64), rtol=0, atol=1e-13)
    assert torch.equal(f.P, b.P) and torch.equal(f.S, b.S)
    assert bool((f.S.abs() <= f.S_abs * (1 + 1e-12)).all()) and bool((b.dP.abs() <= b.dP_abs * (1 + 1e-12)).all())
    assert bool((b.PS.abs() <= b.PS_abs * (1 + 1e-12)).all()) and bool((b.dxh.abs() <= b.dxh_abs * (1 + 1e-12)).all())
