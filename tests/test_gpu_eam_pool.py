"""csrc/eam_pool.hip kernel by kernel against the fp64 reference of eam_pool_reference.py: u3d_eam_pool_fwd (the tile
kernel and its block-order combine) and u3d_eam_pool_bwd (the tile kernel and its two combines), called through
u3d._lib as u3d/feam.py calls them, on buffers the test allocates and pre-fills with NaN (outputs and `part`), so an
element a kernel leaves out cannot pass. Every element is compared.

Sizes follow the kernels' constants: EP_TV = 64 voxels per tile, EP_BLOCKS = 256 workgroups at most, workgroup b takes
tiles b, b + grid, ...; so v = 2 EP_BLOCKS EP_TV + 37 gives 513 tiles: workgroup 0 takes three (the last one the 37-voxel
tail), every other one two. A change of one of the constants shows here which case has to move.

Bounds: worst-case counts of the fp32 roundings in the code, u = 2^-24, times magnitudes of the fp64 reference only
(values and abs-sums), all inflated by 1 + 2^-10 for the second-order terms. c channels, CS = c / 4, R = 4 nt rows,
T = ceil(tiles / workgroups) tiles per workgroup, L = 64 T.

xhat      as test_gpu_eam.py (K = CS + 2 roundings of the mean): ex = |xhat| (2 u + e_r) + rstd dmean
S         u_n = fma(xhat, g2, b2) rounds once, then a chain of c fmas:
          dS = (c + 1) u S_abs + sum_c |A_rc g2_c| ex_c,   S_abs = sum_c |A_rc| |u_c|
att       0.25 ((S0 + S1) + (S2 + S3)): every score passes two adds: 0.25 (sum_i dS_i + 2 u sum_i |S_i|)
exponent  es = |scale| dS + u |scale S| (the product; a contracted fma rounds less). An argument of expf is a
          difference of two such values or of two maxima and rounds once: EA u with EA = 104, because below -104 expf
          gives 0 or a subnormal and the term is lost with an absolute error <= 2^-126 (FLOOR), which is added.
          The device expf's own relative error over [-104, 0] is EXP_ERR (below).
forward   a voxel's weight e^(s - M) is made of T + 1 expf calls at most (its own, one rescale per later tile of its
          workgroup, the combine's) and, on the way into l, of a 6-level shuffle tree, T fmas, the combine's product
          and the rounding of l: a_n = expm1(es_n + (T + 1) (EA u + EXP_ERR) + (T + 8) u). With abar = sum_n P_n a_n
          the normalised weight is off by errP = P (a + abar) / (1 - abar) + FLOOR.
          Yhat: 64 fmas and one rescale product per tile, then the combine's product, two roundings and the division:
          |Yhat - ref| <= errP |xhat| + P ex + (65 T + 4) u Y_abs
          stat: M is the maximum of the computed exponents: |M - ref| <= max_n es_n + u |ref|; l is compared as
          l e^(M - m_ref) against l_ref: relative error <= (abar + es_max + EA u + EXP_ERR) / (1 - abar).
backward  P = expf(scale s - M) / l from the stored (M, l): a_n = expm1(es_n + EA u + EXP_ERR) + 3 u (1 / l, two products),
          errP = P a + FLOOR.  dP: c fmas: ddP = c u dP_abs + |dYhat| ex.
          dS = fma(gatt, 0.25, scale P (dP - D)): ddS = |scale| ((errP + 3 u P) |dP - D| + P (ddP + u |dP - D|)) + u |dS|
          dxhat: two chains of R fmas and the closing fma: ddxh = (R + 1) u dxh_abs + |g2| (ddS^T |A|) + errP^T |dYhat|
          dx: the LayerNorm backward of test_gpu_eam.py from ddxh (accumulate: + u |prev + ref|; bf16 store: + 2^-8
          (|result| + the bound so far)).
          block sums: L fmas carried in registers, stored once: dPS = (L + 1) u PS_abs + ddS |xhat| + |dS| ex,
          dGs = (L + 1) u Gs_abs + sum_n ddS. The combines sum in fp64 and round once per product and per result:
          dA: |g2| dPS + |b2| dGs + u |ref|;  dg2: sum_r |A| dPS + u sum_r |A PS| + u |ref|;  db2 the same with Gs
          (acc_params: + u |prev + ref|).

EXP_ERR: the ROCm tree holds no accuracy table for the device library's expf, so it was measured once on an MI355X
over [-104, 0] (2^24 points, half on a regular grid, half random; a stand-alone program built with the library's
flags) against fp64: largest relative error in the normal range MEASURED_EXP_ERR = 8.409e-8 = 1.41 u (at x = -42.93;
expf(0) = 1 exactly; in the subnormal range the absolute error stayed at 1.4e-45, one subnormal step). The bound uses
EXP_ERR = twice that, 1.682e-7.

The forced-rescale cases (online softmax: a branch that random data does not take) scale rows of A until scale S
passes +-200, where an fp32 exp without the running maximum overflows (88.7), and put the row maximum (a) in the first
tile, (b) in the last tile of the last workgroup, (c) rising tile by tile; two voxels in different workgroups' ranges
carry the same spiked feature, so each holds P ~ 1/2 and a combine that drops or mis-scales a block's partial fails.

Every test prints its worst error as a share of the bound ("SHARE <family> <value>") before asserting.
"""
import functools
import math

import pytest
import torch

import eam_pool_reference as R
from heads_reference import U

pytestmark = pytest.mark.gpu

EP_TV, EP_BLOCKS, HEADS = 64, 256, 4
SLACK = 1 + 2.0 ** -10
UB = 2.0 ** -8            # unit roundoff of bf16 (8 significant bits)
EA = 104.0                # |argument| of an expf whose result is not lost
FLOOR = 2.0 ** -125
MEASURED_EXP_ERR = 8.409090e-08
EXP_ERR = 2 * MEASURED_EXP_ERR
f32, bf16 = torch.float32, torch.bfloat16
F64 = torch.float64
BIG = 2 * EP_BLOCKS * EP_TV + 37

CASES = [(64, 128, 14, f32, "plain"),        # the model's own x8 level at 32^3: one full tile
         (3, 32, 13, f32, "plain"),          # fewer voxels than one tile
         (3, 32, 13, bf16, "plain"),
         (EP_TV + 1, 32, 13, f32, "plain"),  # one tile + 1: the second workgroup holds one voxel
         (77, 32, 1, f32, "plain"),          # nt = 1: 4 rows of 64
         (100, 64, 16, f32, "plain"),        # nt = 16: every row
         (100, 64, 16, bf16, "plain"),
         (BIG, 32, 13, f32, "plain"),        # every workgroup 2-3 tiles, with a tail
         (BIG, 32, 13, bf16, "plain"),
         (EP_BLOCKS * EP_TV + 5 * EP_TV + 1, 128, 13, bf16, "plain"),   # c = 128; some workgroups two tiles
         (BIG, 32, 13, f32, "first"),        # forced rescale (a), (b), (c)
         (BIG, 32, 13, f32, "last"),
         (BIG, 32, 13, f32, "rising")]
# the two voxels of the spiked feature: tile 0 (workgroup 0) and tile 300 (workgroup 44); tile 100 (workgroup 100) and
# tile 511, the last tile of the last workgroup; tile 511 and tile 512, workgroup 0's third
SPIKES = {"first": (5, 300 * EP_TV + 7), "last": (100 * EP_TV + 9, 511 * EP_TV + 3),
          "rising": (511 * EP_TV + 3, 512 * EP_TV + 30)}


def _id(case):
    return "-".join(str(a).replace("torch.", "") for a in case)


def _share(name, err, bound):
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


def _bits(t):
    return t.view(torch.int16 if t.dtype == bf16 else torch.int32)


def _tiles(v):
    ntile = (v + EP_TV - 1) // EP_TV
    nblk = min(EP_BLOCKS, ntile)
    return ntile, nblk, math.ceil(ntile / nblk)


def _ln_err(ln, c, K):
    """(dmean, e_r) of test_gpu_eam.py's docstring from the LN sums of heads_reference.ln_ref."""
    dmean = K * U * ln.sabs / c
    sdd = U * ln.s2 + dmean * ln.s1
    sdd2 = U * U * ln.s2 + 2 * U * dmean * ln.s1 + c * dmean * dmean
    e_v = (2 * sdd + sdd2) / (ln.s2 + c * R.LN_EPS) + (K + 2) * U
    return dmean, e_v / 2 + 3 * U


# ------------------------------------------------------------------------------------------------ cases
@functools.lru_cache(maxsize=None)
def _case(case):
    """Operands as stored, and the fp64 forward and backward references (built once per case)."""
    v, c, nt, dtype, kind = case
    rows = HEADS * nt
    scale = (c // HEADS) ** -0.5
    gen = torch.Generator().manual_seed(v + 7 * c + nt + len(kind))
    r = lambda *s: torch.randn(*s, generator=gen)                      # noqa: E731
    x = r(v, c) + 0.5 * r(v, 1)
    x[min(1, v - 1)] = 0.7                        # one voxel of equal channels: xhat = 0, rstd = 1 / sqrt(eps)
    sign = torch.where(torch.rand(c, generator=gen) < 0.5, -1.0, 1.0)
    g2 = sign * (0.4 + 1.6 * torch.rand(c, generator=gen))
    b2 = 0.5 + 0.8 * r(c)
    A = r(rows, c) * (2.0 / (scale * c ** 0.5))   # scale S of a few units: a softmax far from uniform
    if kind != "plain":
        dvec = r(c)
        if kind == "rising":
            x = x + torch.linspace(0, 1, v)[:, None] * dvec
        s0, s1 = SPIKES[kind]
        x[s0] = x[s1] = r(c) * 0.1 + 6.0 * dvec   # the same spiked feature in two workgroups' ranges
        A[:rows // 2] = (60.0 / (scale * c ** 0.5)) * dvec * sign + 0.1 * A[:rows // 2]
    x = x.to(dtype)
    fwd = R.pool_fwd_ref(x, g2, b2, A, scale)
    if kind != "plain":
        sc = scale * fwd.S
        assert sc.max() > 200 and sc.min() < -200
        s0, s1 = SPIKES[kind]
        assert bool((fwd.P[:rows // 2, s0] > 0.4).all()) and bool((fwd.P[:rows // 2, s1] > 0.4).all())
        assert s0 // EP_TV % EP_BLOCKS != s1 // EP_TV % EP_BLOCKS
        if kind == "rising":                      # workgroup 0's tiles 0, 256, 512: the maximum of row 0 rises each time
            tm = [sc[0, t * EP_TV:(t + 1) * EP_TV].max().item() for t in (0, EP_BLOCKS, 2 * EP_BLOCKS)]
            assert tm[0] < tm[1] < tm[2]
        else:
            assert (sc[0].argmax().item() in SPIKES[kind])
    dy, gatt = r(rows, c), r(nt, v)
    stat = torch.cat([fwd.m, fwd.l]).float()      # as the forward stores them
    D = (dy.double() * fwd.yhat).sum(1).float()
    bwd = {}
    for mode in ("both", "dy", "gatt"):
        bwd[mode] = R.pool_bwd_ref(x, g2, b2, A, scale, stat[:rows], stat[rows:], dy if mode != "gatt" else None,
                                   D if mode != "gatt" else None, gatt if mode != "dy" else None)
    return dict(x=x, g2=g2, b2=b2, A=A, scale=scale, fwd=fwd, bwd=bwd, dy=dy, gatt=gatt, stat=stat, D=D,
                prev_dx=r(v, c).to(dtype), prev_g=r(c), prev_b=r(c))


def _score_err(case, I, ref):
    """ex [v, c], e_r [v, 1] and the exponent error es [R, v] of the docstring."""
    v, c, nt, dtype, kind = case
    ln = ref.ln
    dmean, e_r = _ln_err(ln, c, c // 4 + 2)
    ex = ln.xhat.abs() * (2 * U + e_r) + ln.rstd * dmean
    Aa, g2a = I["A"].double().abs(), I["g2"].double().abs()
    dS = (c + 1) * U * ref.S_abs + (Aa * g2a) @ ex.t()
    es = abs(I["scale"]) * dS + U * (I["scale"] * ref.S).abs()
    return ex, e_r, dS, es


# ------------------------------------------------------------------------------------------------ forward
@pytest.mark.parametrize("case", CASES, ids=_id)
def test_pool_fwd(gpu, case):
    v, c, nt, dtype, kind = case
    L = _L()
    I = _case(case)
    ref = I["fwd"]
    rows = HEADS * nt
    ntile, nblk, T = _tiles(v)
    assert L.query("u3d_eam_pool_blocks", v) == nblk
    npart = L.query("u3d_eam_pool_part_floats", v, c, nt)
    assert npart == nblk * rows * (c + 2) + 2 * rows * c
    x, g2, b2, A = (I[k].to(gpu) for k in ("x", "g2", "b2", "A"))
    runs = []
    for with_att in (1, 1, 0):                      # twice with the map (bitwise equal), once without it
        att, yhat, stat = _nan((nt, v), f32, gpu), _nan((rows, c), f32, gpu), _nan((2 * rows,), f32, gpu)
        part = _nan((npart,), f32, gpu)
        L.call("u3d_eam_pool_fwd", _dt(dtype), x.data_ptr(), 1, v, c, g2.data_ptr(), b2.data_ptr(), A.data_ptr(), nt,
               HEADS, I["scale"], att.data_ptr() if with_att else 0, yhat.data_ptr(), stat.data_ptr(), part.data_ptr(),
               _stream())
        torch.cuda.synchronize()
        assert bool(torch.isfinite(part[:nblk * rows * (c + 2)]).all()), "a float of part was not written"
        runs.append([t.cpu() for t in (att, yhat, stat)])
    for a, b in zip(runs[0], runs[1]):
        assert torch.equal(_bits(a), _bits(b)), "not deterministic"
    assert bool(torch.isnan(runs[2][0]).all()), "att written although absent"
    assert torch.equal(_bits(runs[2][1]), _bits(runs[0][1])) and torch.equal(_bits(runs[2][2]), _bits(runs[0][2]))
    att, yhat, stat = (t.double() for t in runs[0])
    ex, e_r, dS, es = _score_err(case, I, ref)
    tag = _id(case)
    b_att = 0.25 * (dS.reshape(HEADS, nt, v).sum(0) + 2 * U * ref.S.abs().reshape(HEADS, nt, v).sum(0))
    assert _share(f"pool-att {tag}", (att - ref.att).abs(), SLACK * b_att) <= 1
    a = torch.expm1(es + (T + 1) * (EA * U + EXP_ERR) + (T + 8) * U)
    abar = (ref.P * a).sum(1, keepdim=True) + v * FLOOR
    assert abar.max() < 0.5
    errP = ref.P * (a + abar) / (1 - abar) + FLOOR
    b_y = errP @ ref.ln.xhat.abs() + ref.P @ ex + (65 * T + 4) * U * ref.y_abs
    assert _share(f"pool-yhat {tag}", (yhat - ref.yhat).abs(), SLACK * b_y) <= 1
    es_max = es.max(1).values
    assert _share(f"pool-m {tag}", (stat[:rows] - ref.m).abs(), SLACK * (es_max + U * ref.m.abs())) <= 1
    l_at_ref = stat[rows:] * torch.exp(stat[:rows] - ref.m)
    b_l = ref.l * (abar[:, 0] + es_max + EA * U + EXP_ERR) / (1 - abar[:, 0])
    assert _share(f"pool-l {tag}", (l_at_ref - ref.l).abs(), SLACK * b_l) <= 1


# ------------------------------------------------------------------------------------------------ backward
def _bwd_bounds(case, I, ref):
    v, c, nt, dtype, kind = case
    rows, cs = HEADS * nt, c // 4
    ntile, nblk, T = _tiles(v)
    ln = ref.ln
    xh = ln.xhat.abs()
    ex, e_r, _, es = _score_err(case, I, ref)
    Aa, g2a, b2a = I["A"].double().abs(), I["g2"].double().abs(), I["b2"].double().abs()
    sc = abs(I["scale"])
    errP = ref.P * (torch.expm1(es + EA * U + EXP_ERR) + 3 * U) + FLOOR
    ddP = c * U * ref.dP_abs + ref.dy.abs() @ ex.t()
    PD = ref.dPD.abs()
    ddS = sc * ((errP + 3 * U * ref.P) * PD + ref.P * (ddP + U * PD)) + U * ref.dS.abs()
    ddxh = (rows + 1) * U * ref.dxh_abs + g2a * (ddS.t() @ Aa) + errP.t() @ ref.dy.abs()
    sum_c = lambda t: t.sum(1, keepdim=True)                           # noqa: E731
    dm1 = ((cs + 2) * U * sum_c(ref.dxh.abs()) + sum_c(ddxh)) / c
    dm2 = ((cs + 3) * U * sum_c((ref.dxh * ln.xhat).abs()) + sum_c(ddxh * xh) + sum_c(ref.dxh.abs() * ex)) / c
    Tm = ref.dxh.abs() + ref.m1.abs() + (ln.xhat * ref.m2).abs()
    b_dx = ln.rstd * (ddxh + dm1 + xh * dm2 + ref.m2.abs() * ex + (4 * U + e_r) * Tm)
    Lc = EP_TV * T
    dPS = (Lc + 1) * U * ref.PS_abs + ddS @ xh + ref.dS.abs() @ ex
    dGs = (Lc + 1) * U * ref.Gs_abs + ddS.sum(1)
    A = I["A"].double()
    b_dA = g2a * dPS + b2a * dGs[:, None] + U * ref.dA.abs()
    b_dg2 = (Aa * dPS).sum(0) + U * (A * ref.PS).abs().sum(0) + U * ref.dg2.abs()
    b_db2 = (Aa * dGs[:, None]).sum(0) + U * (A * ref.Gs[:, None]).abs().sum(0) + U * ref.db2.abs()
    return b_dx, b_dA, b_dg2, b_db2


BWD_CASES = [(case, mode) for case in CASES for mode in ("both", "dy", "gatt")
             if mode == "both" or (case[4] == "plain" and case[0] < BIG)]   # dYhat only / gatt only: the small cases


@pytest.mark.parametrize("case,mode", BWD_CASES, ids=lambda a: a if isinstance(a, str) else _id(a))
def test_pool_bwd(gpu, case, mode):
    v, c, nt, dtype, kind = case
    L = _L()
    I = _case(case)
    ref = I["bwd"][mode]
    rows = HEADS * nt
    _, nblk, _ = _tiles(v)
    npart = L.query("u3d_eam_pool_part_floats", v, c, nt)
    x, g2, b2, A, stat, dy, D, gatt = (I[k].to(gpu) for k in ("x", "g2", "b2", "A", "stat", "dy", "D", "gatt"))
    p_dy, p_D = (dy.data_ptr(), D.data_ptr()) if mode != "gatt" else (0, 0)
    p_ga = gatt.data_ptr() if mode != "dy" else 0
    b_dx, b_dA, b_dg2, b_db2 = _bwd_bounds(case, I, ref)
    tag = f"{mode} {_id(case)}"
    for acc, accp in ((0, 0), (1, 1)) if mode == "both" else ((0, 0),):
        runs = []
        for _ in range(2):                          # twice: the kernels promise a fixed summation order
            dx = I["prev_dx"].to(gpu) if acc else _nan((v, c), dtype, gpu)
            dg2 = I["prev_g"].to(gpu) if accp else _nan((c,), f32, gpu)
            db2 = I["prev_b"].to(gpu) if accp else _nan((c,), f32, gpu)
            dA, part = _nan((rows, c), f32, gpu), _nan((npart,), f32, gpu)
            L.call("u3d_eam_pool_bwd", _dt(dtype), x.data_ptr(), 1, v, c, g2.data_ptr(), b2.data_ptr(), A.data_ptr(),
                   nt, HEADS, I["scale"], stat.data_ptr(), p_dy, p_D, p_ga, dx.data_ptr(), acc, part.data_ptr(),
                   dA.data_ptr(), dg2.data_ptr(), db2.data_ptr(), accp, _stream())
            torch.cuda.synchronize()
            used = torch.cat([part[b * rows * (c + 2):b * rows * (c + 2) + rows * c + rows] for b in range(nblk)]
                             + [part[nblk * rows * (c + 2):]])
            assert bool(torch.isfinite(used).all()), "a float of part was not written"
            runs.append([t.cpu() for t in (dx, dA, dg2, db2)])
        for a, b in zip(*runs):
            assert torch.equal(_bits(a), _bits(b)), "not deterministic"
        dx, dA, dg2, db2 = (t.double() for t in runs[0])
        m_ = f"acc{acc}{accp} {tag}"
        want = ref.dx + (I["prev_dx"].double() if acc else 0)
        bd = b_dx + (U * want.abs() if acc else 0)
        if dtype == bf16:
            bd = bd + UB * (want.abs() + bd)
        assert _share(f"pool-dx {m_}", (dx - want).abs(), SLACK * bd) <= 1
        assert _share(f"pool-dA {m_}", (dA - ref.dA).abs(), SLACK * b_dA) <= 1
        for nm, got, r_, b_, prev in (("dg2", dg2, ref.dg2, b_dg2, I["prev_g"]), ("db2", db2, ref.db2, b_db2, I["prev_b"])):
            w_ = r_ + (prev.double() if accp else 0)
            assert _share(f"pool-{nm} {m_}", (got - w_).abs(), SLACK * (b_ + (U * w_.abs() if accp else 0))) <= 1


# ------------------------------------------------------------------------------------------------ contract
def test_workspace_does_not_grow_past_the_block_cap(gpu):
    q = lambda v: _L().query("u3d_eam_pool_part_floats", v, 32, 16)     # noqa: E731
    cap = EP_BLOCKS * EP_TV
    assert q(10 * cap) == q(100 * cap) == EP_BLOCKS * 64 * 34 + 2 * 64 * 32
    assert _L().query("u3d_eam_pool_blocks", 100 * cap) == EP_BLOCKS


def test_batch_of_two_is_an_error(gpu):
    from u3d._lib import U3DError
    t = torch.zeros(4096, device=gpu)
    p = t.data_ptr()
    with pytest.raises(U3DError, match="n = 2"):
        _L().call("u3d_eam_pool_fwd", _L().F32, p, 2, 3, 32, p, p, p, 13, HEADS, 1.0, p, p, p, p, _stream())
    with pytest.raises(U3DError, match="n = 2"):
        _L().call("u3d_eam_pool_bwd", _L().F32, p, 2, 3, 32, p, p, p, 13, HEADS, 1.0, p, p, p, p, p, 0, p, p, p, p, 0,
                  _stream())
