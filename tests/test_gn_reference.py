"""The fp64 GroupNorm+ReLU backward reference of the GPU tests (gn_reference.py) against torch's own autograd of
relu(group_norm(x)) in fp64, at the small shapes of test_gpu_groupnorm.py. Fed fp64-exact statistics the two agree to
1e-10 relative (the formulas are the same mathematics; only the order of fp64 operations differs)."""
import pytest
import torch
import torch.nn.functional as F

from gn_reference import (LARGE, LARGE_PAIR, MAX_SHARE, SMALL, TIE, exact_stats, gn_relu_bwd_ref, reduce_geom,
                          zero_ties)


def _inputs(n, c, dims, seed):
    torch.manual_seed(seed)
    x = (1.5 * torch.randn((n,) + dims + (c,)) + 0.3).double()
    da = torch.randn(x.shape).double()
    return x, da, (1 + 0.1 * torch.randn(c)).double(), (0.1 * torch.randn(c)).double()


@pytest.mark.parametrize("n,c,dims,G", SMALL)
def test_reference_matches_autograd_fp64(n, c, dims, G):
    x, da, ga, be = _inputs(n, c, dims, 17 + c)
    st, _ = exact_stats(x, G)
    ref = gn_relu_bwd_ref(x, da, st, ga, be, G)
    assert ref.share <= MAX_SHARE
    xa, gaa, bea = (t.clone().requires_grad_(True) for t in (x, ga, be))
    y = F.relu(F.group_norm(xa.movedim(-1, 1), G, gaa, bea, eps=1e-5))
    y.backward(ref.da.movedim(-1, 1))                       # the tie-cleaned dA: the mask no longer matters there
    for got, want in ((ref.dx, xa.grad), (ref.dgamma, gaa.grad), (ref.dbeta, bea.grad)):
        assert (got - want).abs().max().item() <= 1e-10 * want.abs().max().item()
    # the sums of |terms| bound the sums themselves, and handing the helper its own sums changes nothing
    assert bool((ref.dgamma.abs() <= ref.abs_dgamma * (1 + 1e-12)).all())
    assert bool((ref.dbeta.abs() <= ref.abs_dbeta * (1 + 1e-12)).all())
    xs = x.reshape(n, -1, c)
    mu = st[..., 0].repeat_interleave(c // G, dim=1)[:, None]
    rs = st[..., 1].repeat_interleave(c // G, dim=1)[:, None]
    xhat = (xs - mu) * rs
    g = torch.where(xhat * ga + be > 0, ref.da.reshape(n, -1, c), torch.zeros(()).double())
    again = gn_relu_bwd_ref(x, da, st, ga, be, G, sums=(g.sum(1), (g * xhat).sum(1)))
    assert (again.dx - ref.dx).abs().max().item() <= 1e-12 * ref.dx.abs().max().item()


def test_reference_takes_the_statistics_it_is_handed():
    """fp32-rounded statistics are operands: with them dx is no longer group_norm's exact gradient, so the documented
    formula is checked directly at one element with plain Python sums; and the tie handling zeroes exactly the entries
    with |pre| < TIE."""
    n, c, dims, G = 2, 32, (3, 4, 5), 16
    x, da, ga, be = _inputs(n, c, dims, 3)
    st = exact_stats(x, G)[0].float()
    ref = gn_relu_bwd_ref(x, da, st, ga, be, G)
    cpg, v = c // G, 3 * 4 * 5
    nn, ch, vox = 1, 13, 37
    gr = ch // cpg
    mu, rs = st[nn, gr, 0].double(), st[nn, gr, 1].double()
    xs, ds = x.reshape(n, v, c), ref.da.reshape(n, v, c)
    a = b = 0.0
    for k in range(gr * cpg, (gr + 1) * cpg):
        xh = (xs[nn, :, k] - mu) * rs
        gk = torch.where(xh * ga[k] + be[k] > 0, ds[nn, :, k], torch.zeros(()).double())
        a += (ga[k] * gk).sum().item() / (v * cpg)
        b += (ga[k] * gk * xh).sum().item() / (v * cpg)
    xh = ((xs[nn, vox, ch] - mu) * rs).item()
    gg = ds[nn, vox, ch].item() if xh * ga[ch].item() + be[ch].item() > 0 else 0.0
    want = rs.item() * (ga[ch].item() * gg - a - xh * b)
    assert abs(ref.dx.reshape(n, v, c)[nn, vox, ch].item() - want) <= 1e-12 * max(1.0, abs(want))
    pre = torch.tensor([[-2e-4, -5e-5, 0.0, 5e-5, 2e-4]]).double()
    cleaned, share = zero_ties(pre, torch.ones(1, 5))
    assert cleaned.tolist() == [[1.0, 0.0, 0.0, 0.0, 1.0]] and abs(share - 0.6) < 1e-12 and TIE == 1e-4


def test_shapes_reach_the_branches_they_are_named_for():
    """The geometry claims beside the shapes of gn_reference.py, from the restated make_geom (bf16 = 2, fp32 = 4 bytes)."""
    vox = lambda dims: dims[0] * dims[1] * dims[2]  # noqa: E731
    n, c, dims, _ = SMALL[0]
    g = reduce_geom(n, c, vox(dims), 2)
    assert g["nblk"] == 2 and vox(dims) % g["vpb"] != 0                  # two blocks, the second ragged
    assert reduce_geom(n, c, vox(dims), 4)["nblk"] == 3
    for (n, c, dims, _), chunks in ((SMALL[1], (3, 6)), (SMALL[2], (5, 10))):
        for es, chn in zip((2, 4), chunks):
            g = reduce_geom(n, c, vox(dims), es)
            assert g["chn"] == chn and 64 % chn != 0                     # the serial branch of block_channel_reduce
    assert 512 // 3 * 3 == 510                                           # the apply's thread count at 3 chunks
    assert SMALL[3][0] * SMALL[3][1] == 2048                             # GN_PAIRS_MAX
    assert reduce_geom(1, 8, 105, 2)["chn"] == 1
    n, c, dims, _ = SMALL[6]
    assert vox(dims) < min(reduce_geom(n, c, vox(dims), es)["vlanes"] for es in (2, 4))
    n, c, dims, _ = LARGE
    spl = 512 // (n * c)
    assert reduce_geom(n, c, vox(dims), 2)["nblk"] == 230 and reduce_geom(n, c, vox(dims), 4)["nblk"] == 243
    assert 8 * spl == 128
    n, c, dims, _ = LARGE_PAIR
    v = vox(dims)
    assert n * v >= 409600 and v < 1 << 24
    for es in (2, 4):  # gn_bwd2_launch: U3D_GN2_APV = 16 vectors per apply thread where that leaves >= 200 blocks
        chn = c * es // 16
        athr = 512 // chn * chn
        assert n * -(-v * chn // (16 * athr)) >= 200
