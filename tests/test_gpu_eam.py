"""csrc/eam.hip kernel by kernel against the fp64 references of heads_reference.py (EAM) and against fp64
F.interpolate / oracle.ref_cpu.renew_token: u3d_eam_prep, u3d_eam_attn_fwd, u3d_eam_attn_bwd (+ its reduce kernel),
u3d_eam_param_bwd, u3d_upsample_trilinear (+ _bwd) and u3d_renew_token. The C entry points are called through
u3d._lib, as u3d/feam.py calls them, on buffers the test allocates and pre-fills with NaN (outputs, `part`, `dq_ws`,
`dz_ws`, the trilinear `ws`), so an element a kernel leaves out cannot pass. Every element is compared.

Sizes follow the kernels' constants: EAM_TV = 64 voxels per backward tile, BWD_BLOCKS = 256 workgroups at most in
eam_attn_bwd_kernel, FWD_BLOCKS = 2048 blocks of 256 threads in eam_attn_fwd_kernel, TRI_BLOCKS = 8192 blocks of 256
threads in the up_tri_* kernels, RT_CHUNK = 256 voxels per renew_token chunk. A change of one of them shows here which
case has to move.

Bounds: worst-case counts of the fp32 roundings in the code, u = 2^-24, times magnitudes of the fp64 reference only
(values and abs-sums), all inflated by 1 + 2^-10 for the second-order terms. c channels, CS = c / 4, x~ = x - mean.

LayerNorm of a row whose sum takes K roundings (forward K = c: c - 1 adds, one division; backward K = CS + 2: CS - 1
adds, two shuffle adds, one division; token side K = 9: an 8-level tree, one division):
  dmean = K u sum|x| / c,   dd_i = u |x~_i| + dmean                    (the subtraction rounds once)
  e_v   = (2 sum|x~| dd + sum dd^2) / (sum x~^2 + c eps) + (K + 2) u     (squares and their sum K, / c, + eps)
  e_r   = e_v / 2 + 3 u                                                 (rsqrtf: 1 ulp = 2 u, and slack u)
  dxhat = |xhat| (2 u + e_r) + rstd dmean
  The row of equal channels has x~ = 0, rstd = 1 / sqrt(eps): the rstd dmean term and the sum dd^2 term carry it.
forward   |att - ref| <= (c + 3) u att_abs + e_r att_abs + rstd dmean sum_c|A_tc| + (c + 1) u sum_c|M_tc b2_c|
          att_abs = rstd sum_c |A_tc| |x~_c|: A = M g2 rounds once, the fma chain c times, the subtraction and the last
          fma once each; a0 = M b2 is a chain of c fmas, rounded once more by that last fma. The same for bf16 input.
dx        ddxh = (nt + 1) u |g2| sum_t|g_t M_tc| =: (nt + 1) u DXA     (nt fmas, one product)
          dm1  = ((CS + 2) u sum_c|dxh| + sum_c ddxh) / c                (CS - 1 + 2 adds, one division)
          dm2  = ((CS + 3) u sum_c|dxh xhat| + sum_c ddxh |xhat| + sum_c |dxh| dxhat) / c   (CS fmas, 2 adds, / c)
          |dx - ref| <= rstd (ddxh + dm1 + |xhat| dm2 + |m2| dxhat + (4 u + e_r) (|dxh| + |m1| + |xhat m2|))
          accumulate: + u |prev + ref|; bf16 store: + 2^-8 (|result| + the bound so far): bf16 keeps 8 significant
          bits, so round-to-nearest moves a value by up to half of 2^-7 of it (2^-9 would be a 9-bit format; the
          kernel's stores reach 1.98 of it, as a correct rounding must).
dM        L = 64 * ceil(tiles / workgroups) fmas carried in registers across a workgroup's tiles, no tree, stored once:
          dP = (L + 1) u P_abs + sum_v |g_t| dxhat,  dGs = (L + 1) u Gs_abs;  the cross-block sum and g2 P + b2 Gs
          are fp64: |dM - ref| <= |g2| dP + |b2| dGs + u |ref|
dg2, db2  (L + 1) u abs-sum + nt u sum_v DLA |xhat| (db2: sum_v DLA) + sum_v |dl| dxhat (dg2 only) + u |ref|
          (+ u |prev + ref| with acc_params), DLA = sum_t |g_t M_tc|
token     q: c u q_abs + (|g3| dzhat + u |z|) |Wq|^T;  M: inv_h ((c + 1) u |q| |Wk| + dq |Wk|)
param bwd dq: (c + 1) u dq_abs;  dz: c u dz_abs + ddq |Wq|;  dkv: (nt + 2) u dkv_abs;
          dWq: (nt + 2) u dWq_abs + ddq^T |z|;  dg3: nt u dg3_abs + sum_t ddz |zhat|;  db3: nt u db3_abs + sum_t ddz
          (accumulate: + u |prev + ref| each)
trilinear s a power of two, so the interpolation weights are exact in fp32. forward: six roundings deep (product, sum,
          per axis): 6 u interp(|x|). backward: three gather passes of at most 2 s terms with a weight that may be a
          rounded sum of two: 3 (2 s + 1) u bwd(|dy|) (+ u |prev + ref| when accumulating).
renew     partials of at most RT_CHUNK fp32 adds, an fp64 combine rounded once, then tok (1 - a) + mean a in fp32:
          a (RT_CHUNK + 1) u mean|x| + 4 u (|tok| (1 - a) + a |mean|)

Every test prints its worst error as a share of the bound ("SHARE <family> <value>") before asserting.
"""
import functools
import math

import pytest
import torch
import torch.nn.functional as F

import oracle.ref_cpu as O
import heads_reference as R
from heads_reference import U

pytestmark = pytest.mark.gpu

EAM_TV, BWD_BLOCKS, FWD_BLOCKS, TRI_BLOCKS, RT_CHUNK = 64, 256, 2048, 8192, 256
SLACK = 1 + 2.0 ** -10
INV_H = 0.25           # 1 / num_heads, exact in fp32
UB = 2.0 ** -8         # unit roundoff of bf16 (8 significant bits)
f32, bf16 = torch.float32, torch.bfloat16

SMALL = [(1, 64, 128, 13, f32),      # the model's own x8 level: one full tile
         (1, 3, 32, 13, f32),        # fewer voxels than one tile
         (1, 3, 32, 13, bf16),
         (1, 77, 32, 1, f32),        # tail tile, nt = 1 (rows t >= nt of GL stay stale)
         (2, 100, 64, 16, f32),      # nt = EAM_NT, the tile 64..127 straddles the sample boundary at 100
         (2, 100, 64, 16, bf16)]
FWD_CASES = SMALL + [(1, FWD_BLOCKS * 256 + 300, 32, 13, bf16)]             # the grid-stride loop of the forward
BWD_CASES = SMALL + [(1, 2 * BWD_BLOCKS * EAM_TV + 37, 32, 13, f32),         # every workgroup 2-3 tiles, with tail
                     (1, 2 * BWD_BLOCKS * EAM_TV + 37, 32, 13, bf16),
                     (1, BWD_BLOCKS * EAM_TV + 5 * EAM_TV + 1, 128, 13, bf16)]  # NPAIR = 8; some workgroups 2 tiles
TOKEN_CASES = [(13, 128), (13, 64), (13, 32), (1, 32), (16, 256), (3, 24)]   # c = 256 fills the block, 24 idles lanes


def _id(case):
    return "-".join(str(a).replace("torch.", "") for a in case)


def _share(name, err, bound):
    """max err / bound (an entry with a zero bound must have no error); printed, then returned for the assertion."""
    assert bool(torch.isfinite(err).all()), f"{name}: an element was not written"
    zero = bound == 0
    assert not bool((err[zero] != 0).any()), f"{name}: error where the bound is 0"
    s = (err[~zero] / bound[~zero]).max().item() if bool((~zero).any()) else 0.0
    print(f"SHARE {name} {s:.4f}")
    return s


def _L():
    from u3d import _lib as L
    return L


def _stream():
    from u3d.ops import _stream as s
    return s()


def _nan(shape, dtype, dev):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


def _dt(dtype):
    return _L().BF16 if dtype == bf16 else _L().F32


def _ln_err(ln, c, K):
    """(dmean, e_r) of the docstring from the LN sums (sabs, s1, s2) of heads_reference.ln_ref; K: roundings of the mean."""
    dmean = K * U * ln.sabs / c
    sdd = U * ln.s2 + dmean * ln.s1                                    # sum |x~| dd
    sdd2 = U * U * ln.s2 + 2 * U * dmean * ln.s1 + c * dmean * dmean   # sum dd^2
    e_v = (2 * sdd + sdd2) / (ln.s2 + c * R.LN_EPS) + (K + 2) * U
    e_r = e_v / 2 + 3 * U
    return dmean, e_r


# ------------------------------------------------------------------------------------------------ cases
@functools.lru_cache(maxsize=None)
def _token(nt, c):
    """Token-side operands (fp32) and their fp64 reference, built once."""
    gen = torch.Generator().manual_seed(1000 * nt + c)
    r = lambda *s: torch.randn(*s, generator=gen)                      # noqa: E731
    tok = r(nt, c) + 0.2
    g3, b3 = 0.4 + 1.6 * torch.rand(c, generator=gen), 0.5 + 0.8 * r(c)
    wq, kv = r(c, c) / c ** 0.5, r(2 * c, c) / c ** 0.5
    ref = R.eam_token_ref(tok, g3, b3, wq, kv[:c], INV_H)
    return dict(tok=tok, g3=g3, b3=b3, wq=wq, kv=kv, ref=ref, dM=r(nt, c), prev=[r(c, c), r(2 * c, c), r(c), r(c)])


@functools.lru_cache(maxsize=None)
def _case(case):
    """Voxel-side operands as stored; M is the fp32 rounding of the reference token side's."""
    n, v, c, nt, dtype = case
    gen = torch.Generator().manual_seed(v + 7 * c + nt)
    r = lambda *s: torch.randn(*s, generator=gen)                      # noqa: E731
    x = r(n, v, c) + 0.5 * r(n, v, 1)              # per-voxel channel standard deviation 1, a mean of its own
    x[0, min(1, v - 1)] = 0.7                      # one voxel of equal channels: xhat = 0, rstd = 1 / sqrt(eps)
    x = x.to(dtype)
    sign = torch.where(torch.rand(c, generator=gen) < 0.5, -1.0, 1.0)
    g2 = sign * (0.4 + 1.6 * torch.rand(c, generator=gen))
    b2 = 0.5 + 0.8 * r(c)
    M = _token(nt, c)["ref"].M.float()
    return dict(x=x, g2=g2, b2=b2, M=M, gout=r(n, nt, v), prev_dx=r(n, v, c).to(dtype), prev_g=r(c), prev_b=r(c))


@functools.lru_cache(maxsize=None)
def _fwd_ref(case):
    I = _case(case)
    return R.eam_fwd_ref(I["x"], I["g2"], I["b2"], I["M"])


@functools.lru_cache(maxsize=None)
def _bwd_ref(case):
    I = _case(case)
    return R.eam_bwd_ref(I["x"], I["g2"], I["b2"], I["M"], I["gout"])


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("case", FWD_CASES, ids=_id)
def test_attn_fwd(gpu, case):
    n, v, c, nt, dtype = case
    I, ref = _case(case), _fwd_ref(case)
    x, g2, b2, M = (I[k].to(gpu) for k in ("x", "g2", "b2", "M"))
    out = _nan((n, nt, v), f32, gpu)
    _L().call("u3d_eam_attn_fwd", _dt(dtype), x.data_ptr(), n, v, c, g2.data_ptr(), b2.data_ptr(), M.data_ptr(), nt,
              out.data_ptr(), _stream())
    torch.cuda.synchronize()
    ln = R.NS(sabs=ref.sabs, s1=ref.s1, s2=ref.s2)
    dmean, e_r = _ln_err(ln, c, c)
    bound = ((c + 3) * U + e_r[:, None]) * ref.att_abs + (ref.rstd * dmean)[:, None] * ref.A_abs[None, :, None] \
        + (c + 1) * U * ref.a0_abs[None, :, None]
    assert _share(f"eam-fwd {_id(case)}", (out.cpu().double() - ref.att).abs(), SLACK * bound) <= 1


# ------------------------------------------------------------------------------------------------ backward
def _bwd_bounds(case, ref, I):
    n, v, c, nt, dtype = case
    ln, cs = ref.ln, c // 4
    g2, b2 = I["g2"].double().abs(), I["b2"].double().abs()
    dmean, e_r = _ln_err(ln, c, cs + 2)
    xh = ln.xhat.abs()
    dxhat = xh * (2 * U + e_r) + ln.rstd * dmean
    dxa = g2 * ref.dl_abs
    ddxh = (nt + 1) * U * dxa
    sum_c = lambda t: t.sum(1, keepdim=True)                           # noqa: E731
    dm1 = ((cs + 2) * U * sum_c(ref.dxh.abs()) + sum_c(ddxh)) / c
    dm2 = ((cs + 3) * U * sum_c((ref.dxh * ln.xhat).abs()) + sum_c(ddxh * xh) + sum_c(ref.dxh.abs() * dxhat)) / c
    T = ref.dxh.abs() + ref.m1.abs() + (ln.xhat * ref.m2).abs()
    b_dx = ln.rstd * (ddxh + dm1 + xh * dm2 + ref.m2.abs() * dxhat + (4 * U + e_r) * T)
    ntile = (n * v + EAM_TV - 1) // EAM_TV
    L = EAM_TV * math.ceil(ntile / min(BWD_BLOCKS, ntile))
    ga = ref.g.abs()
    dP = (L + 1) * U * ref.P_abs + ga.t() @ dxhat
    dGs = (L + 1) * U * ref.Gs_abs
    b_dm = g2 * dP + b2 * dGs[:, None] + U * ref.dM.abs()
    b_dg2 = (L + 1) * U * ref.dg2_abs + nt * U * (ref.dl_abs * xh).sum(0) + (ref.dl.abs() * dxhat).sum(0) \
        + U * ref.dg2.abs()
    b_db2 = (L + 1) * U * ref.db2_abs + nt * U * ref.dl_abs.sum(0) + U * ref.db2.abs()
    return b_dx.reshape(n, v, c), b_dm, b_dg2, b_db2


@pytest.mark.parametrize("case", BWD_CASES, ids=_id)
def test_attn_bwd(gpu, case):
    n, v, c, nt, dtype = case
    L = _L()
    I, ref = _case(case), _bwd_ref(case)
    x, g2, b2, M, gout = (I[k].to(gpu) for k in ("x", "g2", "b2", "M", "gout"))
    nblk = L.query("u3d_eam_attn_bwd_blocks", n, v)
    assert nblk == min(BWD_BLOCKS, (n * v + EAM_TV - 1) // EAM_TV)
    npart = L.query("u3d_eam_attn_bwd_part_floats", n, v, c, nt)
    assert npart == nblk * (nt * c + nt + 2 * c)
    b_dx, b_dm, b_dg2, b_db2 = _bwd_bounds(case, ref, I)
    tag = _id(case)
    for acc, accp in ((0, 0), (1, 0), (0, 1), (1, 1)):
        runs = []
        for _ in range(2):                          # twice: the kernels promise a fixed summation order
            dx = I["prev_dx"].to(gpu) if acc else _nan((n, v, c), dtype, gpu)
            dg2 = I["prev_g"].to(gpu) if accp else _nan((c,), f32, gpu)
            db2 = I["prev_b"].to(gpu) if accp else _nan((c,), f32, gpu)
            dM, part = _nan((nt, c), f32, gpu), _nan((npart,), f32, gpu)   # exactly the floats the query names
            L.call("u3d_eam_attn_bwd", _dt(dtype), x.data_ptr(), n, v, c, g2.data_ptr(), b2.data_ptr(), M.data_ptr(),
                   nt, gout.data_ptr(), dx.data_ptr(), acc, part.data_ptr(), dM.data_ptr(), dg2.data_ptr(),
                   db2.data_ptr(), accp, _stream())
            torch.cuda.synchronize()
            assert bool(torch.isfinite(part).all()), "a float of part was not written"
            runs.append([t.cpu() for t in (dx, dM, dg2, db2)])
        for a, b in zip(*runs):
            assert torch.equal(a.view(torch.int16 if a.dtype == bf16 else torch.int32),
                               b.view(torch.int16 if b.dtype == bf16 else torch.int32)), "not deterministic"
        dx, dM, dg2, db2 = (t.double() for t in runs[0])
        mode = f"acc{acc}{accp} {tag}"
        want = ref.dx + (I["prev_dx"].double() if acc else 0)
        bd = b_dx + (U * want.abs() if acc else 0)
        if dtype == bf16:
            bd = bd + UB * (want.abs() + bd)
        assert _share(f"eam-dx {mode}", (dx - want).abs(), SLACK * bd) <= 1
        assert _share(f"eam-dM {mode}", (dM - ref.dM).abs(), SLACK * b_dm) <= 1
        for nm, got, r_, b_, prev in (("dg2", dg2, ref.dg2, b_dg2, I["prev_g"]), ("db2", db2, ref.db2, b_db2, I["prev_b"])):
            w_ = r_ + (prev.double() if accp else 0)
            assert _share(f"eam-{nm} {mode}", (got - w_).abs(), SLACK * (b_ + (U * w_.abs() if accp else 0))) <= 1


# ------------------------------------------------------------------------------------------------ token side
def _token_bounds(I):
    ref, c = I["ref"], I["tok"].shape[1]
    g3, wq, wk = I["g3"].double().abs(), I["wq"].double().abs(), I["kv"][:c].double().abs()
    dmean, e_r = _ln_err(ref.ln, c, 9)
    dzhat = ref.zhat.abs() * (2 * U + e_r) + ref.ln.rstd * dmean
    dz = g3 * dzhat + U * ref.z.abs()
    dq = c * U * ref.q_abs + dz @ wq.t()
    dM = INV_H * ((c + 1) * U * (ref.q.abs() @ wk) + dq @ wk)
    return dzhat, dq, dM


@pytest.mark.parametrize("nt,c", TOKEN_CASES, ids=str)
def test_eam_prep(gpu, nt, c):
    I = _token(nt, c)
    tok, g3, b3, wq, kv = (I[k].to(gpu) for k in ("tok", "g3", "b3", "wq", "kv"))
    zhat, q, M = (_nan((nt, c), f32, gpu) for _ in range(3))
    _L().call("u3d_eam_prep", tok.data_ptr(), nt, c, g3.data_ptr(), b3.data_ptr(), wq.data_ptr(), kv.data_ptr(), INV_H,
              zhat.data_ptr(), q.data_ptr(), M.data_ptr(), _stream())
    torch.cuda.synchronize()
    ref = I["ref"]
    for nm, got, want, b in zip(("zhat", "q", "M"), (zhat, q, M), (ref.zhat, ref.q, ref.M), _token_bounds(I)):
        assert _share(f"eam-prep-{nm} ({nt}, {c})", (got.cpu().double() - want).abs(), SLACK * b) <= 1


@pytest.mark.parametrize("acc", [0, 1], ids=["write", "accumulate"])
@pytest.mark.parametrize("nt,c", TOKEN_CASES, ids=str)
def test_eam_param_bwd(gpu, nt, c, acc):
    I = _token(nt, c)
    zhat, q = I["ref"].zhat.float(), I["ref"].q.float()        # as the forward stores them
    wk = I["kv"][:c]
    ref = R.eam_param_bwd_ref(I["dM"], zhat, q, I["g3"], I["b3"], I["wq"], wk, INV_H)
    dev = [t.to(gpu) for t in (I["dM"], zhat, I["g3"], I["b3"], I["wq"], I["kv"], q)]
    dq_ws, dz_ws = _nan((nt, c), f32, gpu), _nan((nt, c), f32, gpu)
    outs = [p.to(gpu) for p in I["prev"]] if acc else [_nan(p.shape, f32, gpu) for p in I["prev"]]
    _L().call("u3d_eam_param_bwd", dev[0].data_ptr(), nt, c, dev[1].data_ptr(), dev[2].data_ptr(), dev[3].data_ptr(),
              dev[4].data_ptr(), dev[5].data_ptr(), dev[6].data_ptr(), INV_H, dq_ws.data_ptr(), dz_ws.data_ptr(),
              outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(), acc, _stream())
    torch.cuda.synchronize()
    wqa = I["wq"].double().abs()
    ddq = (c + 1) * U * ref.dq_abs
    ddz = c * U * ref.dz_abs + ddq @ wqa
    bounds = [(nt + 2) * U * ref.dwq_abs + ddq.t() @ ref.z.abs(),
              torch.cat([(nt + 2) * U * ref.dkv_abs, torch.zeros(c, c, dtype=torch.float64)]),
              nt * U * ref.dg3_abs + (ddz * zhat.double().abs()).sum(0), nt * U * ref.db3_abs + ddz.sum(0)]
    tag = f"({nt}, {c}) acc{acc}"
    assert _share(f"eam-dq {tag}", (dq_ws.cpu().double() - ref.dq).abs(), SLACK * ddq) <= 1
    assert _share(f"eam-dz {tag}", (dz_ws.cpu().double() - ref.dz).abs(), SLACK * ddz) <= 1
    dkv = outs[1].cpu()
    if acc:   # the unused v half of kv.weight's gradient is not touched
        assert torch.equal(dkv[c:].view(torch.int32), I["prev"][1][c:].view(torch.int32)), "dkv rows c..2c-1 changed"
    else:
        assert bool((dkv[c:] == 0).all()), "dkv rows c..2c-1 are not zero"
    for nm, got, want, b, prev in zip(("dWq", "dkv", "dg3", "db3"), outs, (ref.dwq, ref.dkv, ref.dg3, ref.db3), bounds,
                                      I["prev"]):
        w_ = want + (prev.double() if acc else 0)
        if acc:
            b = b + U * w_.abs()
            if nm == "dkv":
                b[c:] = 0
        assert _share(f"eam-{nm} {tag}", (got.cpu().double() - w_).abs(), SLACK * b) <= 1


# ------------------------------------------------------------------------------------------------ trilinear x s
TRI_CASES = [(2, 1, 5, 6, 4), (2, 5, 1, 6, 4), (2, 5, 6, 1, 4),   # an axis of 1: i1 clamps to i0 everywhere on it
             (2, 1, 1, 3, 2),       # the same in the scalar forward (w s = 6)
             (3, 16, 19, 18, 8),    # vector forward (w s % 4 == 0): 8 404 992 outputs > 4 * 256 * TRI_BLOCKS
             (4, 52, 51, 51, 2)]    # scalar forward (w s = 102): 4 328 064 outputs > 256 * TRI_BLOCKS; the first axis
#                                     pass of the backward has 2 164 032 elements > 256 * TRI_BLOCKS


@functools.lru_cache(maxsize=None)
def _tri(case, backward):
    nc, d, h, w, s = case
    gen = torch.Generator().manual_seed(nc + d + h + w + s)
    x = torch.randn(1, nc, d, h, w, generator=gen)
    up = lambda t: F.interpolate(t, scale_factor=s, mode="trilinear")   # noqa: E731
    out = dict(x=x, y=up(x.double()), y_abs=up(x.double().abs()))
    if backward:
        dy, prev = torch.randn(out["y"].shape, generator=gen), torch.randn(x.shape, generator=gen)
        for key, t in (("dx", dy.double()), ("dx_abs", dy.double().abs())):
            leaf = torch.zeros(x.shape, dtype=torch.float64, requires_grad=True)
            (up(leaf) * t).sum().backward()
            out[key] = leaf.grad
        out.update(dy=dy, prev=prev)
    return out


@pytest.mark.parametrize("case", TRI_CASES, ids=str)
def test_trilinear_fwd(gpu, case):
    nc, d, h, w, s = case
    assert nc * d * h * w * s ** 3 // (4 if w * s % 4 == 0 else 1) > 256 * TRI_BLOCKS or d * h * w < 64
    I = _tri(case, False)
    y = _nan(I["y"].shape, f32, gpu)
    x = I["x"].to(gpu)
    _L().call("u3d_upsample_trilinear", x.data_ptr(), nc, d, h, w, s, y.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert _share(f"tri-fwd {case}", (y.cpu().double() - I["y"]).abs(), SLACK * 6 * U * I["y_abs"]) <= 1


@pytest.mark.parametrize("acc", [0, 1], ids=["write", "accumulate"])
@pytest.mark.parametrize("case", [c for c in TRI_CASES if c[4] != 8], ids=str)
def test_trilinear_bwd(gpu, case, acc):
    nc, d, h, w, s = case
    I = _tri(case, True)
    nws = _L().query("u3d_upsample_trilinear_bwd_ws_floats", nc, d, h, w, s)
    assert nws == nc * d * s * h * w * (s + 1)
    ws = _nan((nws,), f32, gpu)
    dx = I["prev"].to(gpu) if acc else _nan(I["x"].shape, f32, gpu)
    dy = I["dy"].to(gpu)
    _L().call("u3d_upsample_trilinear_bwd", dy.data_ptr(), nc, d, h, w, s, dx.data_ptr(), acc, ws.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(ws).all()), "a float of the workspace was not written"
    want = I["dx"] + (I["prev"].double() if acc else 0)
    bound = 3 * (2 * s + 1) * U * I["dx_abs"] + (U * want.abs() if acc else 0)
    assert _share(f"tri-bwd {case} acc{acc}", (dx.cpu().double() - want).abs(), SLACK * bound) <= 1


# ------------------------------------------------------------------------------------------------ renew_token
RT_D, RT_H, RT_W, RT_C, RT_NCLS, RT_ALPHA = 5, 7, 9, 80, 5, 0.25   # 315 voxels = RT_CHUNK + 59; 5 * 80 pairs > 256 threads
RT_TAIL0 = 300                                                     # first voxel of the class that lives in the last chunk


@functools.lru_cache(maxsize=None)
def _renew(kind, dtype):
    """kind "tail": labels at the feature's size, class 3 only in voxels >= RT_CHUNK (the partial second chunk), class
    2 across the chunk boundary. kind "vanish": the same labels on a mask of twice the size, plus class 4 on odd mask
    coordinates only, which the nearest resize (source = 2 * destination) never reads."""
    v = RT_D * RT_H * RT_W
    gen = torch.Generator().manual_seed(5)
    lab = torch.zeros(v)
    assert v % RT_CHUNK != 0 and RT_TAIL0 >= RT_CHUNK and RT_TAIL0 + 11 <= v
    lab[0:200:3], lab[200:290], lab[RT_TAIL0:RT_TAIL0 + 11] = 1, 2, 3
    lab = lab.reshape(1, 1, RT_D, RT_H, RT_W)
    if kind == "vanish":
        lab = lab.repeat_interleave(2, 2).repeat_interleave(2, 3).repeat_interleave(2, 4)
        lab[0, 0, 1, 1, 1] = lab[0, 0, 3, 5, 7] = lab[0, 0, 9, 13, 17] = 4
    x = (torch.randn(1, v, RT_C, generator=gen) + 0.3).to(dtype)                 # stored [n, v, c]
    tok = torch.randn(RT_NCLS - 1, RT_C, generator=gen)
    feat = x.double().permute(0, 2, 1).reshape(1, RT_C, RT_D, RT_H, RT_W)
    new = O.renew_token([tok.double().clone()], [feat], lab.double(), RT_NCLS, RT_ALPHA)[0]
    mabs = O.renew_token([torch.zeros(tok.shape, dtype=torch.float64)], [feat.abs()], lab.double(), RT_NCLS, 1.0)[0]
    return dict(x=x, tok=tok, lab=lab, new=new, mabs=mabs)


@pytest.mark.parametrize("layout", ["ndhwc-view", "ncdhw"])
@pytest.mark.parametrize("dtype", [f32, bf16], ids=["f32", "bf16"])
@pytest.mark.parametrize("kind", ["tail", "vanish"])
def test_renew_token(gpu, kind, dtype, layout):
    I = _renew(kind, dtype)
    v = RT_D * RT_H * RT_W
    x = I["x"].to(gpu)
    sv, sc = RT_C, 1
    if layout == "ncdhw":
        x, sv, sc = x.permute(0, 2, 1).contiguous(), 1, v
    tok, mask = I["tok"].to(gpu), I["lab"].to(gpu)
    md, mh, mw = I["lab"].shape[2:]
    ws = torch.full((_L().query("u3d_renew_token_ws_bytes", 1, RT_D, RT_H, RT_W, RT_NCLS, RT_C),), 255,
                    dtype=torch.uint8, device=gpu)
    _L().call("u3d_renew_token", _dt(dtype), x.data_ptr(), sv, sc, 1, RT_D, RT_H, RT_W, RT_C, mask.data_ptr(), md, mh,
              mw, RT_NCLS, RT_NCLS - 1, RT_ALPHA, tok.data_ptr(), ws.data_ptr(), _stream())
    torch.cuda.synchronize()
    got, old = tok.cpu(), I["tok"]
    assert torch.equal(got[3].view(torch.int32), old[3].view(torch.int32)), "the token of a class without voxels changed"
    assert not torch.equal(got[2], old[2])
    mean_abs = (I["new"] - old.double() * (1 - RT_ALPHA)).abs()                  # a |mean|
    bound = RT_ALPHA * (RT_CHUNK + 1) * U * I["mabs"] + 4 * U * (old.double().abs() * (1 - RT_ALPHA) + mean_abs)
    assert _share(f"renew {kind} {layout}", (got.double() - I["new"]).abs()[:3], SLACK * bound[:3]) <= 1
