"""Pins tests/trunk_edge_reference.py (the fp64 restatements test_gpu_trunk_edge.py compares the stem, head, upsample
and helper kernels against) to torch in fp64 (F.interpolate and its autograd, conv3d / group_norm autograd) and to
oracle/ref_cpu.py, and asserts on the CPU the conditions of every row of tests/trunk_edge_cases.py: the kernel it
reaches, the tile / block / split edge it is there for, and, for every row with a GroupNorm prologue, an ambiguous
share <= 1e-3 under the exact statistics."""
import pytest
import torch
import torch.nn.functional as F

import conv_reference as cr
import trunk_edge_cases as tc
import trunk_edge_reference as tr
from conv_reference import BF, F32, cl, nd
from gn_reference import exact_stats
from oracle import ref_cpu as O


def _gen(seed):
    return torch.Generator().manual_seed(seed)


# ------------------------------------------------------------------------------------------------- the restatements
@pytest.mark.parametrize("dims", [(1, 1, 1), (1, 3, 2), (7, 1, 4), (5, 7, 9), (2, 2, 2)])
def test_upsample_refs_match_interpolate_and_autograd(dims):
    g = _gen(sum(dims))
    n, c = 2, 3
    x = torch.randn((n,) + dims + (c,), generator=g, dtype=torch.float64)
    big = (n,) + tuple(2 * e for e in dims) + (c,)
    skip, dy = (torch.randn(big, generator=g, dtype=torch.float64) for _ in range(2))
    prev = torch.randn(x.shape, generator=g, dtype=torch.float64)
    xr = cl(x).clone().requires_grad_(True)
    up = F.interpolate(xr, scale_factor=2, mode="trilinear")
    y, S = tr.upsample_fwd_ref(x, skip)
    torch.testing.assert_close(y, nd(up.detach()) + skip, rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(tr.upsample_fwd_ref(x)[0], nd(O.upsample2x(cl(x))), rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(S, tr.upsample_fwd_ref(x.abs(), skip.abs())[0], rtol=0, atol=0)
    up.backward(cl(dy))
    dx, Sx = tr.upsample_bwd_ref(dy, prev)
    torch.testing.assert_close(dx, nd(xr.grad) + prev, rtol=1e-13, atol=1e-13)
    torch.testing.assert_close(Sx, tr.upsample_bwd_ref(dy.abs(), prev.abs())[0], rtol=0, atol=0)
    assert bool((S >= y.abs() * (1 - 1e-12)).all()) and bool((Sx >= dx.abs() * (1 - 1e-12)).all())


def test_up_matrix_rule():
    assert tr.up_matrix(1).tolist() == [[1.0], [1.0]]                      # n = 1: both weights on the one input
    U = tr.up_matrix(3)
    assert U.tolist() == [[1, 0, 0], [.75, .25, 0], [.25, .75, 0], [0, .75, .25], [0, .25, .75], [0, 0, 1]]
    for n in (1, 2, 5, 9):                                                 # rows sum to 1; an input feeds <= 4 outputs
        U = tr.up_matrix(n)
        assert bool((U.sum(1) == 1).all()) and int((U != 0).sum(0).max()) <= 4 and bool((U >= 0).all())


@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("dims", [(1, 5, 7), (4, 1, 9), (3, 4, 1), (5, 7, 9)])
def test_stem_refs_match_autograd_fp64(stride, dims):
    g = _gen(stride + sum(dims))
    n, cin, cout = 2, 3, 5
    x = torch.randn((n, cin) + dims, generator=g)                          # fp32 NCDHW, as the model hands it over
    w = torch.randn((cout, cin, 3, 3, 3), generator=g, dtype=torch.float64)
    xr, wr = x.double().requires_grad_(True), w.clone().requires_grad_(True)
    y = F.conv3d(xr, wr, None, stride, 1)
    dy = torch.randn(nd(y).shape, generator=g, dtype=torch.float64)
    ref, S = tr.stem_fwd_ref(tr.stem_operand(x, False), w, stride)
    torch.testing.assert_close(ref, nd(y.detach()), rtol=1e-12, atol=1e-12)
    y.backward(cl(dy))
    dw, Sw = tr.stem_wgrad_ref(tr.stem_operand(x, False), dy, stride)
    torch.testing.assert_close(dw, wr.grad.reshape(cout, cin, 27).permute(2, 0, 1), rtol=1e-12, atol=1e-12)
    assert bool((S >= ref.abs() * (1 - 1e-12)).all()) and bool((Sw >= dw.abs() * (1 - 1e-12)).all())
    assert torch.equal(tr.stem_operand(x, True), nd(x.to(BF).double()))    # the matrix-core kernels' operand


def test_head_refs_match_autograd_fp64():
    g = _gen(5)
    n, v, cin, cout, G = 3, 37, 32, 13, 8
    x = (torch.randn((n, v, cin), generator=g) * 1.5 + 0.3).to(BF)
    ga, be = 1 + 0.1 * torch.randn(cin, generator=g), 0.1 * torch.randn(cin, generator=g)
    w = (0.2 * torch.randn((cout, cin, 1, 1, 1), generator=g)).to(BF).double()
    bias = torch.randn(cout, generator=g)
    dy = torch.randn((n * v, cout), generator=g)
    st = exact_stats(x, G)[0]
    # forward from unrounded activations: the conv + bias alone
    a = torch.randn((n, v, cin), generator=g, dtype=torch.float64)
    y, S = tr.head_fwd_ref(a, w, bias)
    torch.testing.assert_close(y, a @ w.reshape(cout, cin).T + bias.double(), rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(S, a.abs() @ w.reshape(cout, cin).abs().T + bias.double().abs(), rtol=1e-12, atol=0)
    dl = torch.rand(a.shape, generator=g, dtype=torch.float64)
    torch.testing.assert_close(tr.head_fwd_ref(a, w, bias, dl)[2], dl @ w.reshape(cout, cin).abs().T, rtol=1e-12, atol=0)
    # backward: bf16 dy times the forward weights; zero padding columns; column sums of the fp32 dy
    dA, SA, dyb, (cs, csa) = tr.head_bwd_ref(dy, w)
    assert dyb.shape == (n * v, 16) and dyb.dtype == BF and torch.count_nonzero(dyb[:, cout:]) == 0
    assert torch.equal(dyb[:, :cout], dy.to(BF))
    ar = a.reshape(n * v, cin).clone().requires_grad_(True)
    (ar @ w.reshape(cout, cin).T).backward(dy.to(BF).double())
    torch.testing.assert_close(dA, ar.grad, rtol=1e-12, atol=1e-12)
    torch.testing.assert_close(cs, dy.double().sum(0), rtol=0, atol=0)
    assert bool((SA >= dA.abs() * (1 - 1e-12)).all()) and bool((csa >= cs.abs()).all())
    # GroupNorm partials: summed over the samples they are d / d beta and d / d gamma of relu(group_norm(x))
    dAb = torch.randn((n, v, cin), generator=g).to(BF)
    P, Sp, D, share = tr.head_gn_parts_ref(x, dAb, st.float(), ga, be, G)
    xr = x.double().permute(0, 2, 1).clone()
    gar, ber = ga.double().requires_grad_(True), be.double().requires_grad_(True)
    F.relu(F.group_norm(xr, G, gar, ber, 1e-5)).backward(dAb.double().permute(0, 2, 1))
    torch.testing.assert_close(P[..., 0].sum(0), ber.grad, rtol=1e-5, atol=1e-5)     # (fp32 statistics handed over)
    torch.testing.assert_close(P[..., 1].sum(0), gar.grad, rtol=1e-5, atol=1e-5)
    assert share <= cr.MAX_AMBIGUOUS and bool((Sp >= P.abs() * (1 - 1e-12)).all()) and bool((D >= 0).all())
    # an input on the ReLU zero is ambiguous and carries its |dA| (|dA xhat|) into D
    x1, st1 = torch.zeros((1, 4, 8)).to(BF), torch.tensor([[[0.0, 1.0]] * 8])
    d1 = torch.ones((1, 4, 8)).to(BF)
    P1, _, D1, sh1 = tr.head_gn_parts_ref(x1, d1, st1, torch.ones(8), torch.zeros(8), 8)
    assert sh1 == 1.0 and bool((D1[..., 0] == 4).all()) and bool((P1 == 0).all())


def test_helper_refs():
    g = _gen(9)
    x = torch.randn((11, 5), generator=g)
    y, S = tr.add_ref(x.to(BF), x)
    assert torch.equal(y, x.to(BF).double() + x.double()) and bool((S >= y.abs()).all())
    s, a = tr.channel_sum_ref(x, x[0])
    torch.testing.assert_close(s, x.double().sum(0) + x[0].double(), rtol=0, atol=0)
    assert bool((a >= s.abs()).all())
    k = tr.cast_ref(x, BF, 8)
    assert k.dtype == BF and torch.equal(k[:, :5], x.to(BF)) and torch.count_nonzero(k[:, 5:]) == 0


# ------------------------------------------------------------------------------------------------- the rows
def test_upsample_rows_reach_every_kernel_and_edge():
    kern = {(tc.dtn(c.dt), tc.up_fwd_kernel(c)[0]) for c in tc.UP_FWD}
    assert kern == {("fp32", "one4"), ("fp32", "one1"), ("bf16", "one8"), ("bf16", "one1"), ("bf16", "quad")}
    for k in kern:                                                         # each with and without the skip
        assert {c.skip for c in tc.UP_FWD if (tc.dtn(c.dt), tc.up_fwd_kernel(c)[0]) == k} == {False, True}
    assert {c.c for c in tc.UP_FWD if c.dt == F32 and tc.up_vec(c.dt, c.c) == 1} == {2, 3}
    assert {c.c for c in tc.UP_FWD if c.dt == BF and tc.up_vec(c.dt, c.c) == 1} == {4}
    for k in ("one4", "one8", "quad"):
        dims = {c.dims for c in tc.UP_FWD if tc.up_fwd_kernel(c)[0] == k}
        assert {(1, 1, 1), (7, 1, 4), (5, 7, 9)} <= dims
        assert any(c.n == 3 for c in tc.UP_FWD if tc.up_fwd_kernel(c)[0] == k)
    assert any(c.dims == (1, 3, 2) for c in tc.UP_FWD)
    quad = [tc.up_fwd_kernel(c) for c in tc.UP_FWD if tc.up_fwd_kernel(c)[0] == "quad"]
    assert ("quad", 20, 64) in quad and ("quad", 320, 256) in quad         # a block not full; a ragged second block
    assert any(t > 256 for k, t, _ in map(tc.up_fwd_kernel, tc.UP_FWD) if k in ("one4", "one8"))
    kb = {(tc.dtn(c.dt), tc.up_bwd_kernel(c), c.accum) for c in tc.UP_BWD}
    assert kb == {(d, k, a) for d, ks in (("fp32", ("blk", "row4", "row1")), ("bf16", ("blk", "row8", "row1")))
                  for k in ks for a in (False, True)}
    for k in ("blk", "row4", "row8"):
        dims = {c.dims for c in tc.UP_BWD if tc.up_bwd_kernel(c) == k}
        assert {(1, 1, 1), (1, 3, 2), (7, 1, 4), (5, 7, 9)} <= dims          # odd d and h: the half-empty row pair
    assert {c.c for c in tc.UP_BWD if tc.up_bwd_kernel(c) == "row1"} == {2, 3}
    assert tc.UP_FWD_L(tc.UP_FWD[0]) == 6 and tc.UP_FWD_L(tc.UP_FWD[1]) == 7 and tc.UP_BWD_L(tc.UP_BWD[0]) == 20


def test_stem_rows_reach_every_kernel_and_edge():
    routes = {(tc.dtn(c.dt), tc.stem_fwd_kernel(c), dict(c.opts).get("STEM1", 1)) for c in tc.STEM_FWD if c.cin == 1}
    assert routes == {("fp32", "stem1_fwd", 1), ("bf16", "stem1_fwd", 1), ("bf16", "stem1_mfma", 1),
                      ("fp32", "stem_fwd", 0), ("bf16", "stem_fwd", 0)}
    for r in routes:
        rows = [c for c in tc.STEM_FWD if c.cin == 1 and (tc.dtn(c.dt), tc.stem_fwd_kernel(c),
                                                           dict(c.opts).get("STEM1", 1)) == r]
        assert {(1, 5, 7), (4, 1, 9), (3, 4, 1)} <= {c.dims for c in rows}
        assert {6, 33, 70} <= {c.dims[2] for c in rows}
        for c in rows:
            tot = c.n * c.dims[0] * c.dims[1] * c.dims[2]
            assert tot % 64 != 0
        assert any(c.n == 3 and c.n * c.dims[0] * c.dims[1] * c.dims[2] > 256 for c in rows)
    gen = [c for c in tc.STEM_FWD if c.cin > 1]
    assert all(tc.stem_fwd_kernel(c) == "stem_fwd" for c in gen)
    assert {c.cin for c in gen} == {2, 3, 4} and {c.cout for c in gen} == {8, 24, 32, 40}
    assert {(c.dt, c.stride) for c in gen} == {(d, s) for d in (F32, BF) for s in (1, 2)}
    assert all(e % 2 == 1 for c in gen for e in c.dims)
    assert all((c.dims[0] * c.dims[1] * c.dims[2]) % 256 == 0 for c in tc.STEM_STATS)
    assert {dict(c.opts)["STEM_MFMA"] for c in tc.STEM_STATS} == {0, 1}
    valu = [c for c in tc.STEM_WGRAD if not tc.stem_wgrad_mfma(c)]
    mfma = [c for c in tc.STEM_WGRAD if tc.stem_wgrad_mfma(c)]
    assert {(c.cin, c.cout) for c in valu} >= {(1, 8), (2, 32), (3, 24), (4, 16)}
    assert {(c.dt, c.stride) for c in valu} == {(d, s) for d in (F32, BF) for s in (1, 2)}
    assert {c.nsplit for c in valu} == {1, 3, 7}
    empty = 0
    for c in valu:
        od, oh, ow = tc.stem_out_dims(c)
        total = c.n * od * oh * ow
        vps = tc.cdiv(total, c.nsplit)
        assert vps % 64 != 0 and tc.stem_wgrad_L(c) == tc.cdiv(vps, 64) * 64
        assert 27 * c.cin * c.cout <= 8 * 256
        empty += c.nsplit > tc.cdiv(total, 64) and tc.cdiv(total, vps) < c.nsplit
    assert empty >= 1                                                      # more splits than 64-voxel chunks
    assert {c.dims[2] for c in mfma} == {32, 64}
    assert any(c.dims[0] % 4 for c in mfma) and any(c.dims[1] % 8 for c in mfma)
    assert any(c.dims[0] == 1 for c in mfma) and any(c.dims[1] == 1 for c in mfma)
    rel = set()
    for c in mfma:
        nb = tc.stem_bricks(c)
        per = tc.cdiv(nb, c.nsplit)
        rel.add(("eq" if c.nsplit == nb else "below" if c.nsplit < nb else "above", tc.cdiv(nb, per) < c.nsplit))
        assert tc.stem_wgrad_L(c) == 128 * per + 8
    assert {r for r, _ in rel} == {"eq", "below", "above"} and ("below", True) in rel and ("above", True) in rel


def test_head_rows_reach_every_path():
    f = tc.HEAD_FWD
    assert {c.cin for c in f} == {16, 32, 48, 64} and {c.cout for c in f} == {2, 8, 13, 16, 24, 32}
    paths = {(tc.head_fwd_tr(c), c.gn, c.bias) for c in f}
    assert paths == {(t, g, b) for t in (False, True) for g in (False, True) for b in (False, True)}
    assert any(c.cout % 8 == 0 and not tc.head_fwd_tr(c) and dict(c.opts).get("HEAD_TR", 1) == 0 for c in f)
    assert any(c.n * c.cin > tc.HD_GMAX and c.gn and c.cout % 8 == 0 and not tc.head_fwd_tr(c) for c in f)
    assert any(c.n * c.v < 32 for c in f) and any(c.n == 3 and c.v % 32 != 0 for c in f)
    assert {tc.head_fwd_tr(c) for c in f if dict(c.opts).get("HEAD_NB") == 1} == {False, True}
    assert all(tc.head_blocks(c.n * c.v, c.opts) == 1 and c.n * c.v > 4 * 32 for c in f if dict(c.opts).get("HEAD_NB") == 1)
    b = tc.HEAD_BWD
    assert {c.cin for c in b} == {8, 16, 24, 32, 64} and {c.cout for c in b} == {2, 8, 13, 16, 24, 32}
    assert {dict(c.opts)["HEAD_TR"] for c in b} == {0, 1} and any(c.rows % 32 for c in b) and any(c.rows < 32 for c in b)
    assert tc.head_colsum_L(1000, 1) == 8 + 9 and tc.head_colsum_L(303, 3) == 1 + 9
    g = tc.HEAD_GN
    assert {c.n for c in g} == {1, 3} and {c.v for c in g} == {32, 224} and {c.fused for c in g} == {False, True}
    assert {tc.head_gn_bps(c) for c in g if c.v == 224} == {1, 2} and all(c.v % 32 == 0 for c in g)
    assert tc.head_gn_L(tc.HeadG(1, 224, False, (("HEAD_GN_NB", 1),))) == 2 + 9


@pytest.mark.parametrize("c", [c for c in tc.HEAD_FWD if c.gn] + tc.HEAD_GN, ids=tc.case_id)
def test_head_rows_ambiguous_share(c):
    """With the exact statistics (handed over in fp32) the seeds leave <= 1e-3 of the prologue's activations, and of
    the backward's ReLU tests, ambiguous; the GPU test asserts it again with the statistics the kernel is handed."""
    I = tc.head_inputs(c)
    st = exact_stats(I["x"], tc.HEAD_G)[0].float()
    if isinstance(c, tc.HeadG):
        dA = torch.ones(I["x"].shape).to(BF)
        share = tr.head_gn_parts_ref(I["x"], dA, st, I["gamma"], I["beta"], tc.HEAD_G)[3]
    else:
        share = cr.prologue_ref(I["x"], st, I["gamma"], I["beta"], tc.HEAD_G, BF)[1].double().mean().item()
    assert share <= cr.MAX_AMBIGUOUS, share


def test_helper_rows():
    assert {(c.dt, c.numel) for c in tc.ADD} >= {(d, n) for d in (F32, BF) for n in (1, 3, 8, 1027)}
    big = [c for c in tc.ADD if c.numel // (8 if c.dt == BF else 4) > tc.ADD_GRID]
    assert len(big) == 1 and big[0].numel % 4 != 0                         # the loop runs twice, then the tail kernel
    assert {c.c for c in tc.CHSUM} == {1, 2, 3, 16, 48, 100, 256} and {c.rows for c in tc.CHSUM} == {1, 5, 1000, 70001}
    assert {(c.dt, c.accum) for c in tc.CHSUM} == {(d, a) for d in (F32, BF) for a in (False, True)}
    assert any(256 % c.c for c in tc.CHSUM) and any(tc.chsum_geom(c.rows, c.c)[0] > 256 for c in tc.CHSUM)
    assert tc.chsum_geom(70001, 100) == (1015, 69, 2) and tc.chsum_L(tc.ChSum(F32, 70001, 100, True)) == 35 + 2 + 2
    assert {(c.dti, c.dto) for c in tc.CAST} == {(a, b) for a in (F32, BF) for b in (F32, BF)}
    assert any(c.cout == c.cin for c in tc.CAST) and any(c.cout > c.cin for c in tc.CAST) and any(c.rows == 0 for c in tc.CAST)
