"""The stem (csrc/stem.hip), the streaming classifier head (head.hip), the trilinear x2 upsample (upsample.hip) and the
helpers of misc.hip against the fp64 restatements of tests/trunk_edge_reference.py on the SAME operands the kernels
read. One launch and one CPU reference per row of tests/trunk_edge_cases.py (test_trunk_edge_reference.py pins the
restatements and asserts the rows' conditions on the CPU). The C entry points are called through u3d._lib.call with the
argument lists of u3d/ops.py, on buffers the test allocates (gpu_buffers.Bufs): every output and workspace is
pre-filled with NaN bit patterns (or holds the values an accumulating launch starts from), has exactly the advertised
size and is followed by a guard block that must come back unchanged; zeroed counter words must come back zero. Every
element is compared; none is excluded.

BOUNDS, per element, each from the arithmetic and none from a measured result:

  |got - ref| <= store + (L + 1) 2^-24 S + D

  store   2^-8 |ref| for a bf16 result, 0 for fp32 (conv_reference.py).
  chain   S = the absolute sum, L = the fp32 roundings on the longest chain to one output of THAT kernel, restated next
          to the rows in trunk_edge_cases.py:
            upsample forward   upsample.hip:59-60 (up_fwd_kernel) and :149-152 (up_fwd_quad_kernel): the nested lerp
                               rounds a product and a sum on each of three levels (the weights 0, .25, .75, 1 are
                               exact): 6, + 1 for the skip (:63, :155)
            upsample backward  upsample.hip:274-283 / :307-317 (up_bwd_kernel), :386-402 (up_bwd_blk_kernel): <= 4 w taps
                               by fmaf into ``part``, then <= 16 (od, oh) rows by fmaf into ``acc`` (wd * wh is exact):
                               20 (at most 4^3 taps), + 1 where it accumulates (:292, :324, :419)
            stem VALU forward  stem.hip:42 (stem_fwd_kernel), :125 (stem1_fwd_kernel): one fmaf per tap and input
                               channel: 27 cin. Operands: the fp32 input and the pack's weights
            stem1_mfma_kernel  stem.hip:254: one 16x16x32 instruction: 32. Operands: x.to(bf16) (:230 pack_bf16x2)
            stem VALU wgrad    stem.hip:334, :364 (stem_wgrad_kernel): a slab is one fmaf chain over the split's
                               vps = ceil(total / nsplit) voxels staged 64 at a time: vps padded to 64. fp32 x, stored dy
            stem MFMA wgrad    stem.hip:479-499, :517 (stem_wgrad_mfma_kernel): 8 k-steps of depth 16 per brick and wave
                               over per = ceil(bricks / nsplit) bricks, + 8 for the cross-wave sum: 128 per + 8.
                               Operands: x.to(bf16) (:495), bf16 dy. The test sums the slabs in fp64
            head forward       head.hip:105 / :155, :119 / :161: cin / 16 instructions of depth 16, then the bias:
                               round_up(cin, 32) + 1. Output fp32
            head dA            head.hip:223-224 / :249-250, :400-401: two instructions of depth 16: 32; bf16 store
            bias partials      head.hip:212 / :390, :268 / :492, :280 / :504: a lane adds one row per tile its wave
                               visits, 5 shuffle steps, 4 waves; the blocks' rows are summed in fp64 (+ 1 for the fused
                               form's rounding of the last block's fp64 sum, :521)
            GroupNorm partials head.hip:436-437, :466-468, :483: the same chain over the v / 32 tiles of one sample's
                               4 bps waves; the second sum's terms carry the two roundings of (x - mean) * rstd: + 2
            channel_sum        misc.hip:39, :45, :56-60: rows per lane chain, + lanes, + the rounding of the fp64
                               total to fp32 (+ 1 where it accumulates)
            add_inplace        misc.hip:17, :25: one fp32 add, then the store rounding
            cast               the store rounding alone: BITWISE x.to(dtype) with exact zero padding
          The bf16 image of dy (head_bwd, head_loss_bwd_gn) is compared BITWISE with dy.to(bf16), padding columns included.
  D       the ambiguity term. Head forward: conv_reference.prologue_ref's delta times |w|. GroupNorm partials: a voxel
          whose pre-ReLU value lies within the fp32 prologue's error E of zero adds |dA| (|dA xhat|). The ambiguous share
          is <= 1e-3, asserted for every such row on the CPU (exact statistics) and here (the handed statistics).

KERNELS of the four files and the test that pins each (occupy_kernel, a diagnostic, is not covered):
  up_fwd_kernel<float,4>, <float,1>, <bf16,8>, <bf16,1>   test_upsample_fwd_vs_fp64 (fp32 c % 4 == 0 / c = 2, 3; bf16
                              UP_QUAD0 / c = 4)
  up_fwd_quad_kernel<0>       test_upsample_fwd_vs_fp64[bf16-* without UP_QUAD0]; its statistics forms <2..16> pinned
                              bitwise / by test_gpu_epi_stats.py::test_upsample_epilogue_stats
  up_bwd_kernel<*,4|8|1>      test_upsample_bwd_vs_fp64[*_UP_BWD_BLK0]
  up_bwd_blk_kernel           test_upsample_bwd_vs_fp64[*_UP_BWD_BLK1]
  stem_fwd_kernel             test_stem_fwd_vs_fp64[c2.., c3.., c4.. and *_STEM10]
  stem1_wtab_kernel, stem1_fwd_kernel<float>, <bf16>   test_stem_fwd_vs_fp64[fp32-n*c1x32-*, bf16-*_STEM_MFMA0]
  stem1_fwd_kernel<bf16,true>, stem1_mfma_kernel<true>  test_stem1_fwd_stats_vs_fp64
  stem1_mfma_kernel<false>    test_stem_fwd_vs_fp64[bf16-n*c1x32-*-s1]
  stem_wgrad_kernel           test_stem_wgrad_vs_fp64 (every row but the bf16 1 -> 32 rows with w % 32 == 0)
  stem_wgrad_mfma_kernel      test_stem_wgrad_vs_fp64[bf16-n*c1x32-*x32-* / *x64-*]
  head_fwd_kernel<KS,true|false>  test_head_fwd_vs_fp64 (KS = cin / 16 = 1..4; the report names the path)
  head_bwd_kernel             test_head_bwd_vs_fp64 (both HEAD_TR)
  head_loss_bwd_kernel<true>  test_head_loss_bwd_gn_vs_fp64; <false> pinned bitwise to partial_loss_bwd + head_bwd by
                              test_gpu_head_loss.py::test_head_loss_bwd_bitwise
  add_kernel, add_tail_kernel test_add_inplace_vs_fp64
  chsum_partial, chsum_final  test_channel_sum_vs_fp64
  cast_kernel (four pairs)    test_cast_bitwise

FOUND by this pass: nothing; every row met its bound at the first run.

WORST measured share of each bound (MI355X, for review only, never a bound; every test prints its own before it
asserts). bf16 results come close to 1 at elements just above a power of two, as derived:
  upsample2x_add bf16 0.996 fp32 0.390; upsample2x_bwd bf16 0.995 fp32 0.128; stem_fwd bf16 0.994 fp32 0.126;
  stem1_fwd_stats output 0.990 (mean err 8e-10 of scale, rstd 6e-8 relative); stem_wgrad VALU 0.025 MFMA 0.004; head_fwd
  transposed 0.054 untransposed 0.057; head_bwd dA 0.994 dbias 0.117; head_loss_bwd_gn dA 0.993 dbias 0.082 fused dbias
  0.075 sum g 0.026 sum g xhat 0.158; add_inplace bf16 0.996 fp32 0.500; channel_sum bf16 0.103 fp32 0.181; the bf16 dy
  images and cast: 0 elements differ.

MUTANTS (scratch builds, nothing committed; each stays inside its buffers): the new tests that fail, with the number
of failing rows, and after the bar the tests of test_gpu_bf16.py, test_gpu_upsample_blk.py, test_gpu_epi_stats.py,
test_gpu_head_loss.py, test_gpu_head_oracle.py and test_gpu_parity.py that fail (the rest of those files passed):
  upsample: far-face i1 not clamped to i0 (taken from i0 - 1, in bounds)
                                       upsample_fwd 26, upsample_bwd 36 | 28: quad bitwise 4, blocked bitwise 16, golden 1,
                                       bf16_gn_bwd_and_upsample 1, whole-model parity 6
  quad kernel: output (1, 1) of the quad with its neighbour's w weights
                                       upsample_fwd 10 | 5: quad bitwise 3, bf16_gn_bwd_and_upsample 1, bf16 parity 1
  backward gather without the 2i + 2 tap (both kernels)
                                       upsample_bwd 36 | 4: golden 1, whole-model parity 3; the bitwise tests pass
  stem1_fwd_kernel: zw == w read from the next row instead of the zero padding
                                       stem_fwd 12, stem1_fwd_stats 1 | 12: packed bitwise 4, fp32 packed 3, parity 5
  stem1_mfma_kernel: tap 26 dropped from the A fragment
                                       stem_fwd 3, stem1_fwd_stats 1 | 10 (test_gpu_bf16 stem tests 9, parity 1)
  stem_wgrad_kernel: the last voxel of every split dropped
                                       stem_wgrad 20 | 1: test_bf16_stem_wgrad (one of its cases)
  head forward: bias omitted on the untransposed path
                                       head_fwd 13 | 4: test_head_fwd_bwd 1, transposed bitwise 3
  head_bwd: the padding columns of the bf16 dy hold neighbouring values, not zeros
                                       head_bwd 10 | all pass
  head_bwd: truncation instead of round-to-nearest-even in the dy conversion
                                       head_bwd 24 | 10: test_head_fwd_bwd 4, head-loss bitwise 6
  chsum_partial: the last lane group skipped where c does not divide 256
                                       channel_sum 8 | all pass
  add_tail_kernel: the last element skipped
                                       add_inplace 7 | all pass
"""
import pytest
import torch

import conv_reference as cr
import trunk_edge_cases as tc
import trunk_edge_reference as tr
from conv_reference import BF, F32
from gn_reference import exact_stats
from gpu_buffers import Bufs, opts, ptr

pytestmark = pytest.mark.gpu


def _report(name, got, ref, bound):
    d = (got - ref).abs()
    ok = torch.isfinite(got).all().item()
    worst = (d / bound.clamp_min(1e-300)).max().item() if ok and d.numel() else (0.0 if ok else float("inf"))
    print(f"{name}: worst |got - ref| / bound = {worst:.3f} (max |d| {d.max().item() if d.numel() else 0:.3e})")
    assert ok, f"{name}: non-finite (unwritten?) elements"
    assert not bool(((bound == 0) & (ref != 0)).any()), f"{name}: a zero bound where the reference is not zero"
    assert bool((d <= bound).all()), (name, worst)


def _bits(t):
    return t.contiguous().view(torch.int16 if t.dtype == BF else torch.int32)


# ------------------------------------------------------------------------------------------------- upsample
@pytest.mark.parametrize("c", tc.UP_FWD, ids=tc.case_id)
def test_upsample_fwd_vs_fp64(gpu, c):
    from u3d import ops
    from u3d._lib import call
    I = tc.up_inputs(c)
    d, h, w = c.dims
    x, skip = I["x"].to(gpu), (I["skip"].to(gpu) if c.skip else None)
    B = Bufs(gpu)
    with opts(c.opts):
        y = B.nan((c.n, 2 * d, 2 * h, 2 * w, c.c), c.dt)
        call("u3d_upsample2x_add", ops.dt_code(c.dt), x.data_ptr(), c.n, c.c, d, h, w, ptr(skip), y.data_ptr(),
             ops._stream())
        got = y.double().cpu()
    B.check()
    ref, S = tr.upsample_fwd_ref(I["x"], I["skip"] if c.skip else None)
    _report("upsample2x_add " + tc.case_id(c), got, ref, cr.bound_store(ref, c.dt) + cr.bound_accum(S, tc.UP_FWD_L(c)))


@pytest.mark.parametrize("c", tc.UP_BWD, ids=tc.case_id)
def test_upsample_bwd_vs_fp64(gpu, c):
    from u3d import ops
    from u3d._lib import call
    I = tc.up_inputs(c)
    d, h, w = c.dims
    dy = I["dy"].to(gpu)
    B = Bufs(gpu)
    with opts(c.opts):
        dx = B.of(I["prev"].to(gpu)) if c.accum else B.nan((c.n, d, h, w, c.c), c.dt)
        call("u3d_upsample2x_bwd", ops.dt_code(c.dt), dy.data_ptr(), c.n, c.c, d, h, w, dx.data_ptr(), int(c.accum),
             ops._stream())
        got = dx.double().cpu()
    B.check()
    ref, S = tr.upsample_bwd_ref(I["dy"], I["prev"] if c.accum else None)
    _report("upsample2x_bwd " + tc.case_id(c), got, ref, cr.bound_store(ref, c.dt) + cr.bound_accum(S, tc.UP_BWD_L(c)))


# ------------------------------------------------------------------------------------------------- stem
@pytest.mark.parametrize("c", tc.STEM_FWD, ids=tc.case_id)
def test_stem_fwd_vs_fp64(gpu, c):
    from u3d import ops
    from u3d._lib import call
    I = tc.stem_inputs(c)
    x = I["x"].to(gpu)
    pf, _, _ = ops.wstd_fwd(I["w"].to(gpu), c.dt, True, need_dgrad=False)
    wq = cr.decode_pf(pf, c.cout, c.cin, 3)
    B = Bufs(gpu)
    with opts(c.opts):
        y = B.nan((c.n,) + tc.stem_out_dims(c) + (c.cout,), c.dt)
        call("u3d_stem_fwd", ops.dt_code(c.dt), x.data_ptr(), c.n, c.cin, *c.dims, pf.data_ptr(), c.cout, c.stride,
             y.data_ptr(), B.ws(ops.STEM_WS_BYTES), ops._stream())
        got = y.double().cpu()
    B.check()
    ref, S = tr.stem_fwd_ref(tr.stem_operand(I["x"], tc.stem_fwd_kernel(c) == "stem1_mfma"), wq, c.stride)
    _report("stem_fwd " + tc.case_id(c), got, ref, cr.bound_store(ref, c.dt) + cr.bound_accum(S, tc.stem_fwd_L(c)))


@pytest.mark.parametrize("c", tc.STEM_STATS, ids=tc.case_id)
def test_stem1_fwd_stats_vs_fp64(gpu, c):
    """The output under the bound of the plain launch; the statistics against the fp64 statistics of the stored output
    under the bound test_gpu_epi_stats.py derives (mean within 1e-4 of the output scale, rstd within 5e-4 relative)."""
    from u3d import ops
    from u3d._lib import call, query
    I = tc.stem_inputs(c)
    x = I["x"].to(gpu)
    pf, _, _ = ops.wstd_fwd(I["w"].to(gpu), BF, True, need_dgrad=False)
    wq = cr.decode_pf(pf, 32, 1, 3)
    B = Bufs(gpu)
    mfma = dict(c.opts)["STEM_MFMA"] != 0
    with opts(c.opts):
        nws = query("u3d_stem1_stats_ws_floats", c.n, *c.dims)
        assert nws == c.n * (c.dims[0] * c.dims[1] * c.dims[2] // 256) * 32
        y, stats = B.nan((c.n,) + c.dims + (32,), BF), B.nan((c.n, 16, 2), F32)
        call("u3d_stem1_fwd_stats", x.data_ptr(), c.n, *c.dims, pf.data_ptr(), y.data_ptr(), B.ws(ops.STEM_WS_BYTES),
             B.ws(4 * nws), stats.data_ptr(), ops._stream())
        ys, got_st = y.cpu(), stats.double().cpu()
    B.check()
    ref, S = tr.stem_fwd_ref(tr.stem_operand(I["x"], mfma), wq, 1)
    _report("stem1_fwd_stats " + tc.case_id(c), ys.double(), ref,
            cr.bound_store(ref, BF) + cr.bound_accum(S, 32 if mfma else 27))
    st = exact_stats(ys, 16)[0]
    scale = ys.float().abs().max().item()
    dm = (got_st[..., 0] - st[..., 0]).abs().max().item()
    dr = ((got_st[..., 1] - st[..., 1]).abs() / st[..., 1]).max().item()
    print(f"stem1_fwd_stats {tc.case_id(c)}: mean err {dm / scale:.2e} of scale, rstd rel err {dr:.2e}")
    assert bool(torch.isfinite(got_st).all()) and dm < 1e-4 * scale and dr < 5e-4


@pytest.mark.parametrize("c", tc.STEM_WGRAD, ids=tc.case_id)
def test_stem_wgrad_vs_fp64(gpu, c):
    from u3d import ops
    from u3d._lib import call
    I = tc.stem_inputs(c)
    x, dy = I["x"].to(gpu), I["dy"].to(gpu)
    cop, cip = (c.cout + 31) // 32 * 32, 32
    mfma = tc.stem_wgrad_mfma(c)
    B = Bufs(gpu)
    part = B.nan((c.nsplit, 27, cop, cip), F32)
    call("u3d_stem_wgrad", ops.dt_code(c.dt), dy.data_ptr(), x.data_ptr(), c.n, c.cin, *c.dims, c.cout, c.stride,
         part.data_ptr(), c.nsplit, ops._stream())
    got_all = part.double().cpu()
    B.check()
    ref, S = tr.stem_wgrad_ref(tr.stem_operand(I["x"], mfma), I["dy"], c.stride)
    L = tc.stem_wgrad_L(c)
    _report(f"stem_wgrad {tc.case_id(c)} ({'mfma' if mfma else 'valu'}, L = {L})", got_all.sum(0)[:, :c.cout, :c.cin], ref,
            cr.bound_accum(S, L))
    # the slabs' contract: exact zeros in the padded co rows and ci columns, and in the slabs of splits without voxels
    assert torch.count_nonzero(got_all[:, :, c.cout:, :]) == 0 and torch.count_nonzero(got_all[:, :, :, c.cin:]) == 0
    if mfma:
        used = tc.cdiv(tc.stem_bricks(c), tc.cdiv(tc.stem_bricks(c), c.nsplit))
    else:
        od, oh, ow = tc.stem_out_dims(c)
        total = c.n * od * oh * ow
        used = tc.cdiv(total, tc.cdiv(total, c.nsplit))
    assert torch.count_nonzero(got_all[used:]) == 0


# ------------------------------------------------------------------------------------------------- head
def _head_pack(I, gpu, need_dgrad):
    from u3d import ops
    cout, cin = I["w"].shape[:2]
    pf, pd, _ = ops.wstd_fwd(I["w"].to(gpu), BF, False, need_dgrad=need_dgrad)
    return pf, pd, cr.decode_pf(pf, cout, cin, 1)


@pytest.mark.parametrize("c", tc.HEAD_FWD, ids=tc.case_id)
def test_head_fwd_vs_fp64(gpu, c):
    from u3d import ops
    from u3d._lib import call
    I = tc.head_inputs(c)
    T = {k: v.to(gpu) for k, v in I.items()}
    pf, _, wq = _head_pack(I, gpu, False)
    G = tc.HEAD_G
    if c.gn:
        if c.n * c.cin <= tc.HD_GMAX:
            st = ops.gn_stats(T["x"].view(c.n, c.v, 1, 1, c.cin), G)
        else:   # u3d_gn_stats serves n * c <= 2048 only: hand the fp64 statistics over, rounded to fp32
            st = exact_stats(I["x"], G)[0].float().to(gpu)
        a, mask, delta = cr.prologue_ref(I["x"], st.cpu(), I["gamma"], I["beta"], G, BF)
        share = mask.double().mean().item()
        assert share <= cr.MAX_AMBIGUOUS, f"ambiguous share {share:.2e} of the prologue's activations"
        gn = (st.data_ptr(), T["gamma"].data_ptr(), T["beta"].data_ptr(), G)
    else:
        a, delta, gn = I["x"].double(), None, (None, None, None, 0)
    B = Bufs(gpu)
    with opts(c.opts):
        y = B.nan((c.n, c.v, c.cout), F32)
        call("u3d_head_fwd", T["x"].data_ptr(), c.n, c.v, c.cin, pf.data_ptr(), c.cout,
             T["bias"].data_ptr() if c.bias else None, *gn, y.data_ptr(), ops._stream())
        got = y.double().cpu()
    B.check()
    ref, S, *D = tr.head_fwd_ref(a, wq, I["bias"] if c.bias else None, delta)
    _report(f"head_fwd {tc.case_id(c)} ({'tr' if tc.head_fwd_tr(c) else 'untr'})", got, ref,
            cr.bound_accum(S, tc.HEAD_FWD_L(c)) + (D[0] if D else 0))


def _check_head_bwd(name, dy32, wq, dA, dyb, dbp_sum, L_bias):
    """dA, the whole bf16 image of dy (padding columns included, bitwise) and the bias gradient against head_bwd_ref."""
    refA, SA, dyb_ref, (cs, csa) = tr.head_bwd_ref(dy32, wq)
    _report(name + " dA", dA.double(), refA, cr.bound_store(refA, BF) + cr.bound_accum(SA, tc.HEAD_DA_L))
    wrong = (_bits(dyb) != _bits(dyb_ref)).sum().item()
    print(f"{name} dy bf16: {wrong} of {dyb_ref.numel()} elements differ from dy.to(bf16) + zero padding")
    assert dyb.shape == dyb_ref.shape and wrong == 0
    _report(name + " dbias", dbp_sum, cs, cr.bound_accum(csa, L_bias))


@pytest.mark.parametrize("c", tc.HEAD_BWD, ids=tc.case_id)
def test_head_bwd_vs_fp64(gpu, c):
    from u3d import ops
    from u3d._lib import call, query
    I = tc.head_inputs(c)
    dy = I["dy"].to(gpu)
    _, pd, wq = _head_pack(I, gpu, True)
    B = Bufs(gpu)
    with opts(c.opts):
        nb = query("u3d_head_bwd_blocks", c.rows)
        assert nb == tc.head_blocks(c.rows, c.opts)
        dA, dyb = B.nan((c.rows, c.cin), BF), B.nan((c.rows, (c.cout + 7) // 8 * 8), BF)
        dbp = B.nan((nb, c.cout), F32)
        call("u3d_head_bwd", dy.data_ptr(), c.rows, c.cout, pd.data_ptr(), c.cin, dA.data_ptr(), dyb.data_ptr(),
             dbp.data_ptr(), ops._stream())
        dA, dyb, dbp = dA.cpu(), dyb.cpu(), dbp.double().cpu()
    B.check()
    _check_head_bwd("head_bwd " + tc.case_id(c), I["dy"], wq, dA, dyb, dbp.sum(0), tc.head_colsum_L(c.rows, nb))


@pytest.mark.parametrize("c", tc.HEAD_GN, ids=tc.case_id)
def test_head_loss_bwd_gn_vs_fp64(gpu, c):
    """dy is formed in registers from the logits; its fp32 value is u3d_partial_loss_bwd's (pinned by test_gpu_loss.py;
    test_gpu_head_loss.py ties the two bitwise), so dA, the bf16 dy and the bias gradient meet the references of the
    plain form on that dy. The GroupNorm partials are compared on the kernel's own stored dA, pinned just before."""
    from u3d import ops
    from u3d._lib import call, query
    I = tc.head_inputs(c)
    T = {k: v.to(gpu) for k, v in I.items()}
    n, v, cin, C, G = c.n, c.v, 32, 16, tc.HEAD_G
    pf, pd, wq = _head_pack(I, gpu, True)
    x5 = T["x"].view(n, v, 1, 1, cin)
    st = ops.gn_stats(x5, G)
    lg = ops.head_fwd(x5, pf, C, T["bias"], (st, T["gamma"], T["beta"], G)).view(n, v, C)
    _, sums = ops.partial_loss_fwd(lg, T["lab"], T["wt"], True, True)
    go = torch.ones(1, device=gpu)
    dl = ops.partial_loss_bwd(lg, T["lab"], T["wt"], sums, go).cpu().view(n * v, C)
    B = Bufs(gpu)
    with opts(c.opts):
        bps = query("u3d_head_loss_bwd_gn_bps", n, v, cin)
        assert bps == tc.head_gn_bps(c)
        dA, dyb = B.nan((n, v, cin), BF), B.nan((n, v, C), BF)
        dbp, parts = B.nan((n * bps, C), F32), B.nan((n, bps, cin, 2), F32)
        dbias = B.nan((C,), F32) if c.fused else None
        call("u3d_head_loss_bwd_gn", lg.data_ptr(), T["lab"].data_ptr(), n, v, C, T["wt"].data_ptr(), sums.data_ptr(),
             go.data_ptr(), pd.data_ptr(), cin, dA.data_ptr(), dyb.data_ptr(), dbp.data_ptr(), T["x"].data_ptr(),
             st.data_ptr(), T["gamma"].data_ptr(), T["beta"].data_ptr(), G, parts.data_ptr(), ptr(dbias),
             B.zeros(4) if c.fused else None, ops._stream())
        dA, dyb, dbp, parts = dA.cpu(), dyb.cpu(), dbp.double().cpu(), parts.double().cpu()
        dbias = dbias.double().cpu() if c.fused else None
    B.check()
    name, L = "head_loss_bwd_gn " + tc.case_id(c), tc.head_gn_L(c)
    _check_head_bwd(name, dl, wq, dA.view(n * v, cin), dyb.view(n * v, C), dbp.sum(0), L)
    if c.fused:   # the last block's fp64 sum of the partial rows, rounded once to fp32
        _, _, _, (cs, csa) = tr.head_bwd_ref(dl, wq)
        _report(name + " fused dbias", dbias, cs, cr.bound_accum(csa, L + 1))
    P, S, D, share = tr.head_gn_parts_ref(I["x"], dA, st.cpu(), I["gamma"], I["beta"], G)
    assert share <= cr.MAX_AMBIGUOUS, f"ambiguous share {share:.2e} of the ReLU tests"
    got = parts.sum(1)
    _report(name + " sum g", got[..., 0], P[..., 0], cr.bound_accum(S[..., 0], L) + D[..., 0])
    _report(name + " sum g xhat", got[..., 1], P[..., 1], cr.bound_accum(S[..., 1], L + 2) + D[..., 1])


# ------------------------------------------------------------------------------------------------- helpers
@pytest.mark.parametrize("c", tc.ADD, ids=tc.case_id)
def test_add_inplace_vs_fp64(gpu, c):
    from u3d import ops
    from u3d._lib import call
    I = tc.helper_inputs(c)
    B = Bufs(gpu)
    y, x = B.of(I["y"].to(gpu)), I["x"].to(gpu)
    call("u3d_add_inplace", ops.dt_code(c.dt), y.data_ptr(), x.data_ptr(), c.numel, ops._stream())
    got = y.double().cpu()
    B.check()
    ref, S = tr.add_ref(I["y"], I["x"])
    _report("add_inplace " + tc.case_id(c), got, ref, cr.bound_store(ref, c.dt) + cr.bound_accum(S, tc.ADD_L))


@pytest.mark.parametrize("c", tc.CHSUM, ids=tc.case_id)
def test_channel_sum_vs_fp64(gpu, c):
    from u3d import ops
    from u3d._lib import call, query
    I = tc.helper_inputs(c)
    x = I["x"].to(gpu)
    B = Bufs(gpu)
    nbytes = query("u3d_channel_sum_workspace_bytes", c.rows, c.c)
    assert nbytes == tc.chsum_geom(c.rows, c.c)[0] * c.c * 4
    out = B.of(I["prev"].to(gpu)) if c.accum else B.nan((c.c,), F32)
    call("u3d_channel_sum", ops.dt_code(c.dt), x.data_ptr(), c.rows, c.c, out.data_ptr(), int(c.accum), B.ws(nbytes),
         ops._stream())
    got = out.double().cpu()
    B.check()
    ref, S = tr.channel_sum_ref(I["x"], I["prev"] if c.accum else None)
    _report("channel_sum " + tc.case_id(c), got, ref, cr.bound_accum(S, tc.chsum_L(c)))


@pytest.mark.parametrize("c", tc.CAST, ids=tc.case_id)
def test_cast_bitwise(gpu, c):
    """The store rounding alone: bitwise x.to(dtype) (round-to-nearest-even) with exact zeros in the padding channels."""
    from u3d import ops
    from u3d._lib import call
    I = tc.helper_inputs(c)
    x = I["x"].to(gpu) if c.rows else torch.zeros(1, dtype=c.dti, device=gpu)   # (rows = 0: any valid pointer)
    B = Bufs(gpu)
    y = B.nan((c.rows, c.cout), c.dto)
    yp = y.data_ptr() if c.rows else B.all[-1][0].data_ptr()                   # (an empty view has no pointer of its own)
    call("u3d_cast", ops.dt_code(c.dti), x.data_ptr(), ops.dt_code(c.dto), yp, c.rows, c.cin, c.cout,
         ops._stream())
    got = y.cpu()
    B.check()
    ref = tr.cast_ref(I["x"], c.dto, c.cout)
    wrong = (_bits(got) != _bits(ref)).sum().item()
    print(f"cast {tc.case_id(c)}: {wrong} of {ref.numel()} elements differ")
    assert got.shape == ref.shape and wrong == 0
