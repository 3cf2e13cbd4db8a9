"""The convolution kernels, family by family, against the fp64 restatement of tests/conv_reference.py on the SAME rounded
operands: csrc/conv.hip, conv_ring.hip, conv_brick.hip, conv_brick_gen.hip, conv_small*.h/.hip, conv_s2.hip,
dgrad_s2.hip, conv1x1.hip, wgrad_ring*.h/.hip and wgrad_brick*.h/.hip. One launch and one CPU reference per row of
tests/conv_cases.py (test_conv_reference.py asserts the rows' conditions on the CPU). The C entry points are called
through u3d._lib.call with the argument lists of u3d/ops.py, on buffers the test allocates: every output and workspace
is pre-filled with NaN bit patterns, has exactly the advertised size and is followed by a guard block that must come
back unchanged; zeroed counter words must come back zero. Every element is compared; none is excluded.

Out of scope here: the stem (stem.hip), the streaming head (head.hip), the upsample kernels and the helpers of misc.hip
are pinned the same way by test_gpu_trunk_edge.py; the fused forms are pinned BITWISE to the plain launches tested here
(see the table below).

BOUNDS, per element, each from the arithmetic and none from a measured result:

  |got - ref| <= store + (L + 1) 2^-24 S + D

  store   the roundings of the stored value. A bf16 output: 2^-8 |ref| (conv_reference.py). The ring, conv32_brick,
          both generic brick kernels and the unsplit small-volume kernel round the convolution c to bf16 FIRST and add
          the bf16 residual to that (conv_ring.hip:421-443 pack_bf16x2 then a[e] += c[e]; conv_brick.hip:194-208;
          conv_brick_gen.hip:258-276 and :685-704; conv_small_body.h:509-530), as the unfused bf16 `out + residual` of the
          model does: two roundings, 2^-8 (1 + 2^-8) |ref - res| + 2^-8 |ref|. The implicit GEMM and the small-volume
          combine add the residual in fp32 (conv.hip:291, :540, :766; conv_small_body.h:376-384; conv_small.hip:44-50):
          one rounding.
          fp32 outputs and weight-gradient slabs: nothing beyond the chain's own roundings.
  chain   S = the absolute sum; L = the fp32 additions on the longest chain to one output of THAT kernel. Every forward /
          data-gradient kernel keeps one fp32 accumulator per output (and per contraction split) and feeds it matrix
          instructions whose depth divides the padded contraction, so with cx_p = the contracted channels rounded up to
          32, L = k^3 cx_p + slabs + 2 (the slabs' sum, the residual, the bias), which is the term count plus the slab
          count:
            conv32_ring_kernel        conv_ring.hip:523   16x16x32 bf16, 27 steps of 32 channels, no split
            conv32_brick_kernel       conv_brick.hip:179  32x32x16 bf16, 54 steps (tap, k16 half), no split
            convg_brick_kernel        conv_brick_gen.hip:206  32x32x16, chunks of 32 channels x 27 taps, no split
            convg_pbrick_kernel       conv_brick_gen.hip:575  the same chain per unit
            conv_small_kernel         conv_small_body.h:256   32x32x16 over the split's chunks; slabs summed in fixed
                                      order by the tile's last workgroup (:372-375) or small_reduce_kernel
                                      (conv_small.hip:43): + nks <= slabs
            dgrad_s2_kernel           dgrad_s2.hip:161    32x32x16, <= 8 taps x cout_p per parity class (<= 27 cout_p)
            conv_s2_ring_kernel       conv_s2.hip:258-265 16x16x32, 27 taps x 32 channels
            igemm_bf16_kernel         conv.hip:473        32x32x16, K stages of 32 / 64 channels
            igemm_kernel              conv.hip:80 / :102  32x32x16 bf16, 32x32x2 fp32 (an fp32 fma per term)
            splitk_reduce_kernel      conv.hip:755-756    bias, then the nsplit slabs in order: + nsplit <= slabs
            conv1x1_kernel            conv1x1.hip:135     32x32x16, cx_p terms
          A weight-gradient slab is one accumulator chain over the voxels of its plane range / bricks / chunk, padded
          to the instruction depth, and the test sums the slabs in fp64: L = the voxels of one slab, restated from each
          launcher's split in conv_cases.wgrad_slab_terms (wgrad_ring.hip:259 and :375, wgrad_ring_body.h:378 / :401,
          wgrad_brick_body.h:274 / :300 and wb_geom (:69), wgrad_brick.hip:170 and :286, conv.hip:704 / :712 and
          :1014), + 8 for a cross-wave combine of the 8 waves.
  D       the ambiguity term of conv_reference.prologue_ref: activations whose fp64 value lies within the fp32
          prologue's own error of a bf16 rounding boundary or of the ReLU zero may round the other way; each feeds
          spacing(a) + 2E times |w| (|dy|) into the bound of the outputs it touches (the neighbouring bf16 value is one
          whole spacing away, up to 2^-7 |a|; 2^-8 |a| is the half spacing). The share is <= 1e-3, asserted for every
          row on the CPU (exact statistics) and here (the statistics the kernel is handed).

KERNELS of the ten files and the test that pins each:
  conv32_ring_kernel         test_fwd_dgrad_vs_fp64[conv32_ring-*, conv32_ring_q-*]; its epilogue-statistics, xn,
                             fused-finalize and GroupNorm-backward forms pinned bitwise by test_gpu_bf16.py::
                             test_ring_epilogue_gn_stats_match_stats_pass, test_gpu_ring_xn.py, test_gpu_epi_stats.py,
                             test_gpu_gnfused.py and test_gpu_fullsize.py::test_ring_work_queue_matches_static_schedule
  ring_gn_finalize_kernel, ring_gn_finalize_q_kernel   statistics only: pinned by test_gpu_epi_stats.py and
                             test_gpu_fullsize.py (out of scope here)
  conv32_brick_kernel        test_fwd_dgrad_vs_fp64[conv32_brick-*]
  convg_brick_kernel         test_fwd_dgrad_vs_fp64[convg_brick-*-CONVG_PERSIST0]
  convg_pbrick_kernel        test_fwd_dgrad_vs_fp64[convg_brick-*-CONVG_PERSIST1]; statistics / GroupNorm-backward forms
                             pinned bitwise by test_gpu_pbrick.py and test_gpu_gnfused_brick.py
  pbrick_gn_finalize_kernel  statistics only: test_gpu_pbrick.py (out of scope here)
  conv_small_kernel          test_fwd_dgrad_vs_fp64[conv_small2-*, conv_small-*]; the statistics, dgrad_gn and backward-
                             pair forms pinned bitwise by test_gpu_gnfused_small.py and test_gpu_small_pair.py
  small_reduce_kernel        test_fwd_dgrad_vs_fp64[conv_small-*] (rows with slabs > 1)
  dgrad_s2_kernel            test_fwd_dgrad_vs_fp64[conv_dgrad_s2-*]
  conv_s2_ring_kernel        test_fwd_dgrad_vs_fp64[conv_s2_ring-*]; its statistics against test_gpu_s2ring.py
  igemm_kernel               test_fwd_dgrad_vs_fp64[conv_fwd-*-fp32-*, conv_dgrad-*-fp32-*]
  igemm_bf16_kernel          test_fwd_dgrad_vs_fp64[conv_fwd-*-bf16-*, conv_dgrad-*-bf16-*]
  splitk_reduce_kernel       the conv_fwd / conv_dgrad rows with -m<slabs>
  wgrad_kernel               test_wgrad_vs_fp64[conv_wgrad-*]
  conv1x1_kernel             test_fwd_dgrad_vs_fp64[conv1x1-*]
  wgrad_ring_kernel          test_wgrad_vs_fp64[conv_wgrad_ring-*-12x12-*, *-12x24-*] (12 x 12 and 12 x 24 plane tiles)
  wgrad_ring_dma_kernel      test_wgrad_vs_fp64[conv_wgrad_ring-*] (16 x 16 plane tiles: every other extent)
  wgrad_brick_kernel         test_wgrad_vs_fp64[conv_wgrad_brick-*]
  wgrad1_kernel              test_wgrad_vs_fp64[conv_wgrad1-*]

FOUND by this pass: wgrad_brick_kernel and wgrad1_kernel applied the prologue to the zero chunks of the cin_p padding
with the coefficients of channel cin - 1 (gn_coef8 clamps), so with relu(sh) > 0 there the slabs' padded ci columns
held sum(dy) relu(sh) instead of the zeros u3d_conv_wgrad's contract names (include/u3d.h). wstd_bwd reads [:cout, :cin]
only, so no gradient was wrong. Fixed in the kernels (coefficients of padding chunks zeroed); the rows' last channel
has beta = 0.75 so that the defect shows at every seed (conv_cases.make_inputs).

WORST measured share of each bound (MI355X, for review only, never a bound; every test prints its own before it
asserts). bf16 outputs come close to 1 at elements just above a power of two, as derived:
  conv1x1 fwd 0.994 dgrad 0.993; conv32_ring fwd 0.926 dgrad 0.927; conv32_ring_q fwd 0.934 dgrad 0.924; conv32_brick
  fwd 0.927 dgrad 0.937; convg_brick fwd 0.891 dgrad 0.913; conv_small2 fwd 0.923 dgrad 0.912; conv_small fwd 0.925 dgrad
  0.917; conv_dgrad_s2 0.940; conv_s2_ring 0.919; conv_fwd bf16 0.992 fp32 0.056; conv_dgrad bf16 0.971 fp32 0.047;
  conv_wgrad bf16 0.019 fp32 0.050; conv_wgrad1 0.003; conv_wgrad_ring 0.774 and conv_wgrad_brick 0.983 (rows behind a
  prologue where an ambiguous activation rounded the other way: the D term; <= 0.03 without a prologue).

MUTANTS (scratch builds, nothing committed): the new tests that fail (F = test_fwd_dgrad_vs_fp64, W = test_wgrad_vs_fp64,
by entry point, with the number of failing rows) and, after the bar, whether test_gpu_bf16.py::test_bf16_conv_* /
test_gpu_conv1x1.py / test_ws_conv_fwd_bwd_vs_golden still pass:
  the prologue on the cin_p padding (the parent)          W[conv_wgrad_brick] 4, W[conv_wgrad1] 1 | all pass
  ring: halo column right of the volume read from the next row (all channels; one 8-channel piece of one halo row)
                                                          F[conv32_ring] 20, F[conv32_ring_q] 13 | fwd 12, dgrad 12 fail
  small: one (tap, 16-channel step) skipped; one voxel's 8 products; one product
                                                          F[conv_small2] 29 / 29 / 28, F[conv_small] 16 | 32 / 32 / 30 fail
  gemm: the tail split-K slab left unsummed               F[conv_fwd] 6, F[conv_dgrad] 2 (the -m rows) | 54 fail
  taps 0 and 1 swapped in the pd pack                     F, every data-gradient entry, 74 rows | dgrad 102 fail
  s2: one parity class's +1 offset dropped                F[conv_dgrad_s2] 16 | dgrad 30 fail
  weight-gradient ring: the last plane of a range skipped W[conv_wgrad_ring] 6 (the WR_WGS and target rows) | all pass
  prologue on the halo's out-of-volume zeros (small, weight-gradient brick)
                                                          F[conv_small2] 9, F[conv_small] 5, W[conv_wgrad_brick] 14 | 15 fail
  conv1x1: truncation instead of round-to-nearest         F[conv1x1] 22 | all pass
  implicit-GEMM weight gradient: the last voxel of a split dropped
                                                          W[conv_wgrad] 10 | wgrad 17, golden 5 fail
"""
import ctypes

import pytest
import torch

import conv_cases as cc
import conv_reference as cr
from conv_reference import BF, F32
from gpu_buffers import Bufs as _Bufs, opts as _opts, ptr as _ptr

pytestmark = pytest.mark.gpu

TWO_ROUNDINGS = ("u3d_conv32_ring", "u3d_conv32_ring_q", "u3d_conv32_brick", "u3d_convg_brick")


def _operands(c, dev):
    """The row's inputs on the device, the packs from the weight-standardisation kernel, the statistics from
    u3d_gn_stats (both pinned by earlier passes) and the fp64 operands of the reference decoded from what the kernel reads."""
    from u3d import ops
    I = cc.make_inputs(c)
    T = {k: v.to(dev) for k, v in I.items()}
    pf, pd, _ = ops.wstd_fwd(T["w"], c.dt, True, need_dgrad=c.dir == "dgrad")
    T["pf"], T["pd"] = pf, pd
    wq = cr.decode_pf(pf, c.cout, c.cin, c.k)
    G = cc.groups(c.cin)
    if c.gn:
        T["st"] = ops.gn_stats(T["x"], G)
        a, mask, delta = cr.prologue_ref(I["x"], T["st"].cpu(), I["gamma"], I["beta"], G, c.dt)
        share = mask.double().mean().item()
        assert share <= cr.MAX_AMBIGUOUS, f"ambiguous share {share:.2e} of the prologue's activations"
        T["gn"] = (T["st"], T["gamma"], T["beta"], G)
    else:
        a, delta = I["x"].double(), None
        T["gn"] = (None, None, None, 0)
    return I, T, wq, a, delta


def _launch(c, T, B):
    """One launch of the row's entry point into NaN-filled buffers; returns the output tensor."""
    from u3d import ops
    from u3d._lib import call, query
    n, (d, h, w) = c.n, c.dims
    od, oh, ow = cc.out_dims(c)
    st, ga, be, G = T["gn"]
    gn = (_ptr(st), _ptr(ga), _ptr(be), G)
    fwd = c.dir == "fwd"
    res = T["res"] if c.res else None
    s = ops._stream()
    e = c.entry
    dtc = ops.dt_code(c.dt)
    if fwd:
        src, wpk, cx, cy = T["x"], T["pf"], c.cin, c.cout
        out = B.nan((n, od, oh, ow, cy), F32 if c.out_f32 else c.dt)
    else:
        src, wpk, cx, cy = T["dy"], T["pd"], c.cout, c.cin
        out = B.nan((n, d, h, w, cy), c.dt)
    flip = 0 if fwd else 1
    if e in ("u3d_conv32_ring", "u3d_conv32_brick"):
        call(e, flip, src.data_ptr(), n, d, h, w, wpk.data_ptr(), *gn, _ptr(res), out.data_ptr(), s)
    elif e == "u3d_conv32_ring_q":
        q = B.zeros(query("u3d_conv32_ring_q_queue_bytes", n, d, h, w))
        call(e, flip, src.data_ptr(), n, d, h, w, wpk.data_ptr(), *gn, _ptr(res), out.data_ptr(), None, q, s)
    elif e == "u3d_convg_brick":
        call(e, flip, src.data_ptr(), n, cx, d, h, w, wpk.data_ptr(), cy, *gn, _ptr(res), out.data_ptr(), s)
    elif e in ("u3d_conv_small", "u3d_conv_small2"):
        nb = c.slabs * n * d * h * w * cy * 4
        args = (flip, src.data_ptr(), n, cx, d, h, w, wpk.data_ptr(), cy, *gn, _ptr(res), out.data_ptr(), B.ws(nb), nb)
        if e == "u3d_conv_small":
            call(e, *args, s)
        else:
            made = ctypes.c_int(0)
            cnt = B.zeros(query("u3d_conv_small_cnt_bytes", n, d, h, w, cy))
            call(e, *args, cnt, None, None, ctypes.addressof(made), s)
            assert made.value == 0                                      # no statistics asked for
    elif e == "u3d_conv_dgrad_s2":
        call(e, src.data_ptr(), n, cx, wpk.data_ptr(), cy, d, h, w, out.data_ptr(), s)
    elif e == "u3d_conv_s2_ring":
        assert query("u3d_conv_s2_ring_ok", n, cx, d, h, w, cy) == 1
        sp = B.ws(4 * query("u3d_conv_s2_ring_ws_floats", n, d, h, w))
        stats = B.nan((n, 16, 2), F32)
        call(e, src.data_ptr(), n, d, h, w, wpk.data_ptr(), *gn, out.data_ptr(), sp, stats.data_ptr(), B.zeros(4), s)
        assert bool(torch.isfinite(stats).all())
    elif e == "u3d_conv_fwd":
        if c.gn and c.dt == BF and cx >= ops.GN_MATERIALIZE_MIN_C:   # as ops.conv_fwd: relu(gn(x)) materialised once
            src = ops.gn_apply(src, st, ga, be, G)
            gn = (None, None, None, 0)
        nb = c.slabs * n * od * oh * ow * cy * 4
        call(e, dtc, src.data_ptr(), n, cx, d, h, w, wpk.data_ptr(), cy, c.k, c.stride, *gn, _ptr(res),
             _ptr(T["bias"]) if c.bias else None, out.data_ptr(), int(c.out_f32), B.ws(nb), nb, s)
    elif e == "u3d_conv_dgrad":
        mq = d * h * w if c.stride == 1 else (d // 2) * (h // 2) * (w // 2)   # a launch per parity class at stride 2
        nb = c.slabs * n * mq * cy * 4
        call(e, dtc, src.data_ptr(), n, cx, wpk.data_ptr(), cy, d, h, w, c.k, c.stride, out.data_ptr(), B.ws(nb), nb, s)
    elif e == "u3d_conv1x1":
        sd, sh_, sw = (d, h, w)                                         # (data gradient: stride 1, dy's extents)
        call(e, src.data_ptr(), n, cx, sd, sh_, sw, wpk.data_ptr(), wpk.shape[-1], cy, c.stride if fwd else 1, *gn,
             out.data_ptr(), s)
    else:
        raise AssertionError(e)
    return out


def _report(name, got, ref, bound):
    d = (got - ref).abs()
    ok = torch.isfinite(got).all().item()
    worst = (d / bound.clamp_min(1e-300)).max().item() if ok else float("inf")
    print(f"{name}: worst |got - ref| / bound = {worst:.3f} (max |d| {d.max().item():.3e}, max |ref| "
          f"{ref.abs().max().item():.3e})")
    assert ok, f"{name}: non-finite (unwritten?) elements"
    assert not bool(((bound == 0) & (ref != 0)).any()), f"{name}: a zero bound where the reference is not zero"
    assert bool((d <= bound).all()), (name, worst)


@pytest.mark.parametrize("c", cc.FWD_DGRAD, ids=cc.case_id)
def test_fwd_dgrad_vs_fp64(gpu, c):
    I, T, wq, a, delta = _operands(c, gpu)
    B = _Bufs(gpu)
    with _opts(c.opts):
        out = _launch(c, T, B)
        got = out.double().cpu()
    B.check()
    L = cc.chain_len(c, max(1, c.slabs))
    if c.dir == "fwd":
        res = I["res"].double() if c.res else None
        ref, S, *D = cr.conv_fwd_ref(a, wq, c.k, c.stride, res, I["bias"].double() if c.bias else None, a_delta=delta)
        bound = cr.bound_store(ref, F32 if c.out_f32 else c.dt) + cr.bound_accum(S, L) + (D[0] if D else 0)
        unsplit_small = c.family == "small" and (cc.round32(c.cin) == 32 or c.slabs < 2)
        if c.res and c.dt == BF and (c.entry in TWO_ROUNDINGS or unsplit_small):
            bound = bound + 2.0 ** -8 * (1 + 2.0 ** -8) * (ref - res).abs()      # the conv rounded before the add
    else:
        ref, S = cr.conv_dgrad_ref(I["dy"].double(), wq, (c.n,) + c.dims, c.k, c.stride)
        bound = cr.bound_store(ref, c.dt) + cr.bound_accum(S, L)
        if c.k == 1 and c.stride == 2:       # a 1^3 stride-2 conv reads the even voxels only: exact zeros elsewhere
            even = torch.zeros(got.shape[1:4], dtype=torch.bool)
            even[::2, ::2, ::2] = True
            assert torch.count_nonzero(got[:, ~even]) == 0
            assert bool((bound[:, ~even] == 0).all())
    _report(cc.case_id(c), got, ref, bound)


@pytest.mark.parametrize("c", cc.WGRAD, ids=cc.case_id)
def test_wgrad_vs_fp64(gpu, c):
    from u3d import ops
    from u3d._lib import call, query
    I, T, wq, a, delta = _operands(c, gpu)
    B = _Bufs(gpu)
    n, (d, h, w) = c.n, c.dims
    st, ga, be, G = T["gn"]
    gn = (_ptr(st), _ptr(ga), _ptr(be), G)
    cop, cip = cc.round32(c.cout), cc.round32(c.cin)
    with _opts(c.opts):
        s = ops._stream()
        if c.entry == "u3d_conv_wgrad_ring":
            ns = (query("u3d_conv_wgrad_ring_splits", n, c.cin, d, h, w, c.cout) if c.mode == "splits" else
                  query("u3d_conv_wgrad_ring_splits_target", n, c.cin, d, h, w, c.cout, ops.WGRAD_Q_WGS))
            part = B.nan((ns, 27, cop, cip), F32)
            call(c.entry, T["dy"].data_ptr(), T["x"].data_ptr(), n, c.cin, d, h, w, c.cout, *gn, part.data_ptr(), ns, s)
        elif c.entry in ("u3d_conv_wgrad_brick", "u3d_conv_wgrad1"):
            ns = query(c.entry + "_splits", n, c.cin, d, h, w, c.cout, c.stride)
            part = B.nan((ns, c.k ** 3, cop, cip), F32)
            call(c.entry, T["dy"].data_ptr(), T["x"].data_ptr(), n, c.cin, d, h, w, c.cout, c.stride, *gn,
                 part.data_ptr(), ns, s)
        else:
            ns = c.slabs
            part = B.nan((ns, c.k ** 3, cop, cip), F32)
            call(c.entry, ops.dt_code(c.dt), T["dy"].data_ptr(), T["x"].data_ptr(), n, c.cin, d, h, w, c.cout, c.k,
                 c.stride, *gn, part.data_ptr(), ns, s)
        got_all = part.double().cpu()
    got = got_all.sum(0)[:, :c.cout, :c.cin]
    ref, S, *D = cr.conv_wgrad_ref(a, I["dy"].double(), c.k, c.stride, a_delta=delta)
    L = cc.wgrad_slab_terms(c, ns) + 8
    bound = cr.bound_accum(S, L) + (D[0] if D else 0)
    pad = max(got_all[:, :, c.cout:, :].abs().max().item() if cop > c.cout else 0.0,
              got_all[:, :, :, c.cin:].abs().max().item() if cip > c.cin else 0.0)
    print(f"{cc.case_id(c)}: {ns} slabs, L = {L}, max |padding entry| = {pad}")
    _report(cc.case_id(c), got, ref, bound)          # (prints the worst share, then asserts finite and within bound)
    B.check()
    # the slabs' contract (include/u3d.h): the rows / columns past cout / cin hold exact zeros
    assert torch.count_nonzero(got_all[:, :, c.cout:, :]) == 0 and torch.count_nonzero(got_all[:, :, :, c.cin:]) == 0


@pytest.mark.parametrize("dt,k,dims", cc.ODD_S2, ids=lambda v: str(v).split(".")[-1])
def test_gemm_s2_dgrad_odd_extent_raises_and_writes_nothing(gpu, dt, k, dims):
    """u3d_conv_dgrad at stride 2 serves even extents only (parity classes of d / 2 x h / 2 x w / 2): an odd extent
    must raise, not skip voxels, and must leave dx untouched."""
    from u3d import ops
    from u3d._lib import U3DError, call
    n, cin, cout = 1, 32, 64
    od = tuple(cr.out_dim(v, k, 2) for v in dims)
    g = torch.Generator().manual_seed(5)
    dy = torch.randn((n,) + od + (cout,), generator=g).to(dt).to(gpu)
    pf, pd, _ = ops.wstd_fwd(torch.randn((cout, cin, k, k, k), generator=g).to(gpu), dt, True)
    B = _Bufs(gpu)
    dx = B.nan((n,) + dims + (cin,), dt)
    with pytest.raises(U3DError):
        call("u3d_conv_dgrad", ops.dt_code(dt), dy.data_ptr(), n, cout, pd.data_ptr(), cin, *dims, k, 2, dx.data_ptr(),
             None, 0, ops._stream())
    torch.cuda.synchronize()
    B.check()
    assert bool((B.all[0][0][:B.all[0][1]] == 0xFF).all()), "dx written before the launcher refused the shape"
