"""The GroupNorm kernels (csrc/groupnorm.hip, and the dynamic head's u3d_gn_relu_mean) one by one against fp64 on the
SAME rounded operands (x.to(dt).double()), so the differences are the kernels' fp32 arithmetic and, in bf16, the
final rounding of dx. The backward reference is tests/gn_reference.py (pinned to torch autograd in
test_gn_reference.py); it takes the fp32 statistics the kernel is handed as operands, and the kernels are fed the dA
it cleaned of relu sign ties (share <= 0.1 %, asserted), so no entry is excluded from any comparison.

Bounds (each from the arithmetic, none from a measured result):
  statistics  |mean - ref| <= 2^-23 |ref| + 1e-5 sigma_ref (fp32 rounding of the stored value + the margin of
              test_gpu_bf16.py); |rstd - ref| / ref <= 1e-5 (test_gpu_bf16.py:172-174)
  dx fp32     <= 1e-5 max|ref| (the bound of test_block_gn_fwd_bwd_vs_oracle)
  dx bf16     |dx - ref| <= 2^-8 |ref| + 1e-5 max|ref|: store16<bf16> (common.h) packs with pack_bf16x2, a
              __builtin_convertvector to __bf16 = v_cvt_pk_bf16_f32, round-to-nearest-even (as from_f<bf16>'s
              __float2bfloat16). bf16 keeps 8 significand bits, so the stored value is within half a spacing of the fp32
              result: 2^-9 |v| at the top of a binade, 2^-8 |v| just above a power of two. The bound is that worst case
              plus the fp32 term, so elements near a power of two come close to it (measured up to 0.99 of the bound)
  dgamma, dbeta  <= 1e-5 sum|terms| (fp64 sum of the absolute values of what was added): the fp32 chains are a
              per-thread walk of <= ~16 voxels, a 6-step shuffle tree and 8 LDS rows; everything after is fp64
  parts       dgamma, dbeta <= 1e-6 sum|parts|: fp64 sums, one fp32 rounding
Every test prints its worst figure as a fraction of its bound before it asserts."""
import functools

import pytest
import torch

from gn_reference import LARGE, LARGE_PAIR, MAX_SHARE, SMALL, exact_stats, gn_relu_bwd_ref, per_channel, zero_ties

pytestmark = pytest.mark.gpu

DTS = [torch.bfloat16, torch.float32]
BF, F32 = torch.bfloat16, torch.float32


def _ids(v):
    if isinstance(v, torch.dtype):
        return str(v).split(".")[-1]
    if isinstance(v, tuple) and len(v) == 4 and isinstance(v[2], tuple):   # (n, c, dims, groups)
        return f"n{v[0]}c{v[1]}_{'x'.join(map(str, v[2]))}_g{v[3]}"
    if isinstance(v, tuple):
        return "x".join(str(i) for i in v)
    return None


def _randn(seed, *shape, dev="cuda:0"):
    """Seeded CPU normal numbers moved to the device: the same inputs on every machine, so the share of relu sign ties
    the reference zeroes is a property of the test, not of a device's generator."""
    return torch.randn(shape, generator=torch.Generator().manual_seed(seed)).to(dev)


@functools.lru_cache(maxsize=4)
def _inputs(n, c, dims, dt, dist="default", dev="cuda:0"):
    """(x, dA, gamma, beta) on the device; x and dA in dt. Cached: the tests of one shape share them (read-only)."""
    seed = 7 * c + n + sum(dims)
    r = _randn(seed, n, *dims, c, dev=dev)
    x = {"default": 1.5 * r + 0.3, "mean300": 0.5 * r + 300, "plus8": r + 8}[dist].to(dt)
    da = _randn(seed + 1, n, *dims, c, dev=dev).to(dt)
    return x, da, 1 + 0.1 * _randn(seed + 2, c, dev=dev), 0.1 * _randn(seed + 3, c, dev=dev)


def _check_dx(name, dx, ref, dt, scale=None):
    scale = ref.abs().max().item() if scale is None else scale
    d = (dx.double() - ref).abs()
    bound = 1e-5 * scale + (2.0 ** -8 * ref.abs() if dt == BF else 0)
    worst = (d / bound).max().item()
    print(f"{name}: worst |dx - ref| / bound = {worst:.3f} (max|d| {d.max().item():.3e}, scale {scale:.3e})")
    assert torch.isfinite(dx.double()).all() and worst <= 1.0, (name, worst)


def _check_sum(name, got, ref, abs_terms, tol=1e-5):
    d = (got.double() - ref).abs()
    bound = tol * abs_terms.double()
    worst = (d / bound.clamp_min(1e-300)).max().item()       # (a channel whose every term is masked: 0 <= 0)
    print(f"{name}: worst |sum - ref| / ({tol:g} sum|terms|) = {worst:.3f}")
    assert torch.isfinite(got).all() and bool((d <= bound).all()), (name, worst)


# ----------------------------------------------------------------------------------------------- statistics
STAT_CASES = ([(s, dt, "default") for s in SMALL + [LARGE] for dt in DTS]
              + [(s, F32, "mean300") for s in SMALL + [LARGE]]   # an unshifted fp32 sum of squares loses the variance
              + [(s, BF, "plus8") for s in SMALL + [LARGE]]
              + [(s, dt, "const") for s in SMALL for dt in DTS])


@pytest.mark.parametrize("shape,dt,dist", STAT_CASES, ids=_ids)
def test_gn_stats_vs_fp64(gpu, shape, dt, dist):
    """u3d_gn_stats against the fp64 mean and rsqrt(var + 1e-5) of the stored values. ``const``: one (sample, group)
    overwritten with 2.5: mean 2.5 exactly (the shifted sums are all zero) and rstd 1 / sqrt(1e-5)."""
    from u3d import ops
    n, c, dims, G = shape
    x = _inputs(n, c, dims, dt, "default" if dist == "const" else dist)[0]
    cn, cg, cpg = n - 1, G // 2, c // G
    if dist == "const":
        x = x.clone()
        x[cn, ..., cg * cpg:(cg + 1) * cpg] = 2.5
    st = ops.gn_stats(x, G).double()
    ref, sigma = exact_stats(x, G)
    dm = (st[..., 0] - ref[..., 0]).abs()
    bm = 2.0 ** -23 * ref[..., 0].abs() + 1e-5 * sigma
    dr = (st[..., 1] - ref[..., 1]).abs() / ref[..., 1]
    if dist == "const":
        assert st[cn, cg, 0].item() == 2.5
        assert abs(st[cn, cg, 1].item() * 1e-5 ** 0.5 - 1) <= 1e-5
        bm[cn, cg] = 1.0                                       # (asserted exactly above; sigma_ref is 0 there)
    print(f"gn_stats: mean worst {(dm / bm).max().item():.3f} of bound, rstd worst rel {dr.max().item():.3e}")
    assert bool((dm <= bm).all()), (dm / bm).max().item()
    assert dr.max().item() <= 1e-5


# ----------------------------------------------------------------------------------------------- gn_bwd
MODES = [(False, False), (True, False), (False, True), (True, True), (False, None)]  # (accumulate, acc_params / None)
BWD_CASES = ([(s, dt, "default", m) for s in SMALL for dt in DTS for m in MODES]
             + [(LARGE, dt, "default", m) for dt in DTS for m in (MODES[0], MODES[3])]
             + [(s, BF, "plus8", MODES[3]) for s in (SMALL[0], SMALL[4])])


@pytest.mark.parametrize("shape,dt,dist,mode", BWD_CASES, ids=_ids)
def test_gn_bwd_vs_fp64(gpu, shape, dt, dist, mode):
    """u3d_gn_bwd (partial pass + last-block combine + apply): dx fresh and accumulated onto randn, dgamma / dbeta fresh,
    accumulated onto preloaded values, and absent (None)."""
    from u3d import ops
    n, c, dims, G = shape
    acc, accp = mode
    x, da, ga, be = _inputs(n, c, dims, dt, dist)
    st = ops.gn_stats(x, G)
    ref = gn_relu_bwd_ref(x, da, st, ga, be, G)
    assert ref.share <= MAX_SHARE
    base = _randn(5, *x.shape).to(dt)
    pg, pb = _randn(6, c), _randn(7, c)
    dx = base.clone() if acc else torch.full_like(x, float("nan"))
    dg, db = (None, None) if accp is None else (pg.clone(), pb.clone())
    out = ops.gn_bwd(ref.da, x, st, ga, be, G, dx=dx, accumulate=acc, dgamma=dg, dbeta=db, acc_params=bool(accp))
    assert out is dx
    _check_dx("gn_bwd", dx, ref.dx + (base.double() if acc else 0), dt)
    if accp is not None:
        _check_sum("dgamma", dg, ref.dgamma + (pg.double() if accp else 0), ref.abs_dgamma + (pg.abs() if accp else 0))
        _check_sum("dbeta", db, ref.dbeta + (pb.double() if accp else 0), ref.abs_dbeta + (pb.abs() if accp else 0))


# ----------------------------------------------------------------------------------------------- gn_bwd2
S2_SHAPES = [(2, 32, (7, 9, 11), 16), (1, 64, (8, 8, 8), 16), (3, 128, (5, 7, 9), 16), (1, 256, (4, 6, 3), 16),
             (1, 24, (5, 6, 7), 8), LARGE_PAIR]
BWD2_CASES = ([(s, dt, False, acc) for s in SMALL + [LARGE_PAIR] for dt in DTS for acc in (False, True)]
              + [(s, dt, True, acc) for s in S2_SHAPES for dt in DTS for acc in (False, True)])


def _second_set(n, c, dims, dt, compact, dev="cuda:0"):
    """(gamma2, beta2, dA2 at full resolution); compact: dA2 is nonzero at the even voxels only."""
    g2, b2 = 1 + 0.1 * _randn(21 + c, c, dev=dev), 0.1 * _randn(22 + c, c, dev=dev)
    if not compact:
        return g2, b2, _randn(23 + c, n, *dims, c, dev=dev).to(dt)
    od = tuple((d - 1) // 2 + 1 for d in dims)
    da2 = torch.zeros((n,) + dims + (c,), dtype=dt, device=dev)
    da2[:, ::2, ::2, ::2] = _randn(23 + c, n, *od, c, dev=dev).to(dt)  # the reference's expansion: plain indexing
    return g2, b2, da2


@pytest.mark.parametrize("shape,dt,compact,acc", BWD2_CASES, ids=_ids)
def test_gn_bwd2_vs_sum_of_two_fp64(gpu, shape, dt, compact, acc):
    """u3d_gn_bwd2 / u3d_gn_bwd2_s2 (two GN+ReLU consumers of x, same statistics) against the SUM of two reference
    backwards with (gamma1, beta1, dA1) and (gamma2, beta2, dA2). compact: dA2 is given at the stride-2 resolution;
    the reference expands it to the even voxels with plain indexing. Odd and mixed dims walk crd_of / crd_add over
    ragged rows; LARGE_PAIR takes 16 vectors per apply thread and large non-cubic voxel strides."""
    from u3d import ops
    n, c, dims, G = shape
    x, da1, g1, b1 = _inputs(n, c, dims, dt)
    g2, b2, da2 = _second_set(n, c, dims, dt, compact)
    st = ops.gn_stats(x, G)
    r1 = gn_relu_bwd_ref(x, da1, st, g1, b1, G)
    r2 = gn_relu_bwd_ref(x, da2, st, g2, b2, G)
    assert r1.share <= MAX_SHARE and r2.share <= MAX_SHARE
    base = _randn(5, *x.shape).to(dt)
    dx = base.clone() if acc else torch.full_like(x, float("nan"))
    dps = [(torch.full((c,), float("nan"), device=gpu), torch.full((c,), float("nan"), device=gpu)) for _ in range(2)]
    da2k = r2.da[:, ::2, ::2, ::2].contiguous() if compact else r2.da
    ops.gn_bwd2(r1.da, da2k, x, st, (g1, b1), (g2, b2), G, dx=dx, accumulate=acc, dparams1=dps[0], dparams2=dps[1],
                da2_s2=compact)
    _check_dx("gn_bwd2", dx, r1.dx + r2.dx + (base.double() if acc else 0), dt)
    for k, (r, (dg, db)) in enumerate(zip((r1, r2), dps)):
        _check_sum(f"dgamma{k + 1}", dg, r.dgamma, r.abs_dgamma)
        _check_sum(f"dbeta{k + 1}", db, r.dbeta, r.abs_dbeta)


# ----------------------------------------------------------------------------------------------- gn_bwd_parts
# (n, c, nparts): 32 pairs -> 32 slices of the 1024 threads... spl = 1024 / (n c): 16 at (2, 32), 128 at (1, 8)
PARTS_CASES = ([(2, 32, k) for k in (1, 15, 16, 17, 127, 128, 129, 300)]   # around spl and 8 * spl = 128, and a tail
               + [(1, 8, 5), (1, 8, 1000)]        # fewer parts than slices; many 8-deep rounds
               + [(3, 24, 50)]                    # 72 pairs, 1024 % 72 != 0: idle tail threads
               + [(8, 256, 9)])                   # 2048 pairs > 1024 threads: two p0 rounds


@pytest.mark.parametrize("acc", [False, True])
@pytest.mark.parametrize("n,c,nparts", PARTS_CASES)
def test_gn_bwd_parts_synthetic_partials(gpu, n, c, nparts, acc):
    """u3d_gn_bwd_parts (gn_bwd_parts_finalize + apply, bf16) with partials unrelated to dA and x: the kernel only sums
    them, so a_g, b_g come from the fp64 sums of the parts, dbeta / dgamma are those sums, and dx follows the formula."""
    from u3d import ops
    dims = (2, 2, 3) if n * c == 2048 else (3, 5, 7)
    G = 16 if c % 16 == 0 else 8
    x, da, ga, be = _inputs(n, c, dims, BF)
    parts = _randn(nparts, n, nparts, c, 2)
    st = ops.gn_stats(x, G)
    pd = parts.double()
    ref = gn_relu_bwd_ref(x, da, st, ga, be, G, sums=(pd[..., 0].sum(1), pd[..., 1].sum(1)))
    assert ref.share <= MAX_SHARE
    base = _randn(5, *x.shape).to(BF)
    pg, pb = _randn(6, c), _randn(7, c)
    dx = base.clone() if acc else torch.full_like(x, float("nan"))
    dg, db = pg.clone(), pb.clone()
    ops.gn_bwd_parts(ref.da, x, parts, st, ga, be, G, dx=dx, accumulate=acc, dgamma=dg, dbeta=db, acc_params=acc)
    _check_dx("gn_bwd_parts", dx, ref.dx + (base.double() if acc else 0), BF)
    ab = pd.abs().sum((0, 1))                                              # [c, 2]
    _check_sum("dgamma", dg, ref.dgamma + (pg.double() if acc else 0), ab[:, 1] + (pg.abs() if acc else 0), 1e-6)
    _check_sum("dbeta", db, ref.dbeta + (pb.double() if acc else 0), ab[:, 0] + (pb.abs() if acc else 0), 1e-6)


# ----------------------------------------------------------------------------------------------- gn_bwd_apply_coef
@pytest.mark.parametrize("acc", [False, True])
@pytest.mark.parametrize("shape", SMALL + [LARGE], ids=_ids)
def test_gn_bwd_apply_coef_synthetic(gpu, shape, acc):
    """u3d_gn_bwd_apply_coef (bf16) with random coefficients [n, 5, c]: dx (+)= c2 (x c0 + c1 > 0 ? dA : 0) + c3 x + c4.
    The terms may cancel, so the fp32 part of the bound is 1e-5 max(|c2 dA| + |c3 x| + |c4|)."""
    from u3d import ops
    n, c, dims, G = shape
    x, da, _, _ = _inputs(n, c, dims, BF)
    coef = _randn(3 + c, n, 5, c)
    cd = coef.double().reshape(n, 5, *([1] * len(dims)), c)
    xd = x.double()
    pre = xd * cd[:, 0] + cd[:, 1]
    da_clean, share = zero_ties(pre, da)
    assert share <= MAX_SHARE
    dd = da_clean.double()
    ref = cd[:, 2] * torch.where(pre > 0, dd, torch.zeros_like(dd)) + cd[:, 3] * xd + cd[:, 4]
    scale = ((cd[:, 2] * dd).abs() + (cd[:, 3] * xd).abs() + cd[:, 4].abs()).max().item()
    base = _randn(5, *x.shape).to(BF)
    dx = base.clone() if acc else torch.full_like(x, float("nan"))
    ops.gn_bwd_apply_coef(da_clean, x, coef, G, dx=dx, accumulate=acc)
    _check_dx("gn_bwd_apply_coef", dx, ref + (base.double() if acc else 0), BF, scale=scale)


# ----------------------------------------------------------------------------------------------- gn_relu_mean
@pytest.mark.parametrize("dt", DTS, ids=_ids)
@pytest.mark.parametrize("dims", [(1, 1, 1), (3, 4, 6), (6, 6, 6)], ids=_ids)
@pytest.mark.parametrize("n", [1, 2])
def test_gn_relu_mean_vs_fp64(gpu, n, dims, dt):
    """u3d_gn_relu_mean, the dynamic head's GAP (u3d/dynhead.py): feat[n, c] = mean_v relu(GN(16, 256)(x)), v = 1, 72,
    216. relu is continuous: no tie handling. Bound 1e-5 of the mean |pre| over the tensor (one fp32 fma per element from
    fp32 scale / shift, fp64 sums, one fp32 rounding of the result)."""
    from u3d import ops
    from u3d._lib import call
    c, G = 256, 16
    x, _, ga, be = _inputs(n, c, dims, dt)
    st = ops.gn_stats(x, G)
    v = x.numel() // (n * c)
    feat = torch.full((n, c), float("nan"), device=gpu)
    call("u3d_gn_relu_mean", ops.dt_code(dt), x.data_ptr(), n, c, v, G, st.data_ptr(), ga.data_ptr(), be.data_ptr(),
         feat.data_ptr(), ops._stream())
    pre = (x.double().reshape(n, v, c) - per_channel(st[..., 0], c)) * per_channel(st[..., 1], c) * ga.double() + be.double()
    ref = pre.clamp_min(0).mean(1)
    bound = 1e-5 * pre.abs().mean().item()
    d = (feat.double() - ref).abs().max().item()
    print(f"gn_relu_mean: max |d| {d:.3e} = {d / bound:.3f} of the bound")
    assert torch.isfinite(feat).all() and d <= bound


# ----------------------------------------------------------------------------------------------- U3D_S2_NORM_ONCE
def _run_block(gpu, cin, cout, xin, up, norm_once, materialize=True):
    """One stride-2 NoBottleneck (GN + 1^3 downsample) forward + backward under bf16 autocast; returns the output,
    x.grad, the parameter gradients, and how the stride-2 3^3 conv ran: gn_apply calls seen by the tape and by
    conv_fwd, and whether its weight gradient read the materialised operand (gn is None)."""
    import unet3D
    from oracle.weights_recipe import apply_recipe
    from u3d import ops
    ds = torch.nn.Sequential(torch.nn.GroupNorm(16, cin), torch.nn.ReLU(True),
                             unet3D.conv3x3x3(cin, cout, (1, 1, 1), (2, 2, 2), 0, weight_std=True))
    blk = unet3D.NoBottleneck(cin, cout, (2, 2, 2), downsample=ds, weight_std=True)
    apply_recipe(blk, seed=3)
    blk = blk.to(gpu)
    seen = {"gn_apply": 0, "fwd_s2_gn": [], "wgrad_s2_gn": []}
    saved = (ops.S2_NORM_ONCE, ops.GN_MATERIALIZE_BYTES, ops.gn_apply, ops.conv_wgrad, ops.conv_fwd)

    def gn_apply(*a, **k):
        seen["gn_apply"] += 1
        return saved[2](*a, **k)

    def conv_wgrad(dy, x, k, stride, gn=None, brick=None):
        if k == 3 and stride == 2:
            seen["wgrad_s2_gn"].append(gn is not None)
        return saved[3](dy, x, k, stride, gn, brick)

    def conv_fwd(x, wpk, cout_, k, stride, gn=None, *a, **kw):
        if k == 3 and stride == 2:
            seen["fwd_s2_gn"].append(gn is not None)
        return saved[4](x, wpk, cout_, k, stride, gn, *a, **kw)

    ops.S2_NORM_ONCE, ops.gn_apply, ops.conv_wgrad, ops.conv_fwd = norm_once, gn_apply, conv_wgrad, conv_fwd
    if not materialize:
        ops.GN_MATERIALIZE_BYTES = 0
    try:
        x = xin.clone().requires_grad_(True)
        with torch.autocast("cuda", dtype=torch.bfloat16):
            y = blk(x)
        (y * up).sum().backward()
        torch.cuda.synchronize()
    finally:
        ops.S2_NORM_ONCE, ops.GN_MATERIALIZE_BYTES, ops.gn_apply, ops.conv_wgrad, ops.conv_fwd = saved
    return y.detach(), x.grad, {k: p.grad for k, p in blk.named_parameters()}, seen


@pytest.mark.parametrize("cin,cout", [(64, 128), (128, 256)])
def test_s2_norm_once_on_equals_off_bitwise(gpu, cin, cout):
    """U3D_S2_NORM_ONCE (default on: relu(gn(x)) materialised once by u3d_gn_apply ahead of every cin >= 64 stride-2
    3^3 conv and reused by its weight gradient) against off, where the implicit GEMM's prologue (conv.hip
    build_gn_table + the staging) and the brick weight gradient's prologue (gn_coef8 + gn_relu8) normalise on the fly.
    As read from the code, all of them form relu(fma(x, sc, sh)) from sc = rstd * gamma, sh = beta - mean * sc in fp32 and
    round to bf16 once (gn_relu8 rounds before the relu, which commutes with a sign-preserving rounding), so the block
    output, x.grad and every parameter gradient are asserted BITWISE equal, in both off forms: the routing's own
    (conv_fwd materialises small cin >= 64 activations itself, GN_MATERIALIZE_BYTES) and the prologue proper
    (GN_MATERIALIZE_BYTES = 0). The counters prove which branch ran: a silent fallback cannot pass."""
    xin = _randn(cin, 2, cin, 8, 12, 10) * 1.5 + 0.3
    up = _randn(cout, 2, cout, 4, 6, 5)
    on = _run_block(gpu, cin, cout, xin, up, True)
    assert on[3] == {"gn_apply": 1, "fwd_s2_gn": [False], "wgrad_s2_gn": [False]}, on[3]
    for materialize in (True, False):
        off = _run_block(gpu, cin, cout, xin, up, False, materialize)
        assert off[3] == {"gn_apply": int(materialize), "fwd_s2_gn": [True], "wgrad_s2_gn": [True]}, off[3]
        diffs = {"y": (on[0] - off[0]).abs().max().item(), "dx": (on[1] - off[1]).abs().max().item()}
        diffs.update({k: (on[2][k] - off[2][k]).abs().max().item() for k in on[2]})
        print(f"S2_NORM_ONCE on vs off (materialize={materialize}): max |diff| {diffs}")
        assert torch.equal(on[0], off[0]) and torch.equal(on[1], off[1]), diffs
        assert set(on[2]) == set(off[2]) and len(on[2]) == 9
        for k in on[2]:
            assert on[2][k] is not None and torch.equal(on[2][k], off[2][k]), (k, diffs[k])
