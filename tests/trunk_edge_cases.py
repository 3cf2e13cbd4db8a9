"""The case tables of test_gpu_trunk_edge.py: one row per launch of an entry point of csrc/upsample.hip, stem.hip,
head.hip and misc.hip, with the seeded CPU inputs, the kernel each row reaches (the launchers' dispatch restated) and the
length L of the fp32 chain behind each row's bound, restated from the kernels next to the rows. CPU only
(test_trunk_edge_reference.py asserts every row's conditions without a GPU).

Shapes are the smallest that still reach each path: extents of 1, odd extents, n = 3, rows that end ragged inside a
wave / block / tile, both sides of every dispatch threshold.
"""
import zlib
from collections import namedtuple

import torch

from conv_reference import BF, F32, out_dim

cdiv = lambda a, b: -(-a // b)
dtn = lambda dt: "bf16" if dt == BF else "fp32"
_o = lambda opts: "".join(f"_{k}{v}" for k, v in opts)
_x = lambda dims: "x".join(map(str, dims))


def gen(case, salt=0):
    """The row's seeded CPU generator: the same bits on every machine."""
    return torch.Generator().manual_seed((zlib.crc32(case_id(case).encode()) + salt) & 0x7FFFFFFF)


def case_id(c):
    return c.id if hasattr(c, "id") else ID[type(c).__name__](c)


# =============================================================================================== upsample
UpF = namedtuple("UpF", "dt n c dims skip opts")
UpB = namedtuple("UpB", "dt n c dims accum opts")


def up_vec(dt, c):
    """Channels per thread: 16-byte vectors where c allows, else the scalar instantiation (upsample.hip:444-445)."""
    v = 8 if dt == BF else 4
    return v if c % v == 0 else 1


def up_fwd_kernel(c):
    """(kernel, threads per row, block) of u3d_upsample2x_add (upsample.hip:449-463)."""
    vec = up_vec(c.dt, c.c)
    w = c.dims[2]
    if c.dt == BF and vec == 8 and dict(c.opts).get("UP_QUAD", 1) != 0:
        tpr = w * (c.c // 8)                                      # up_quad_shape (upsample.hip:431-435)
        return "quad", tpr, (cdiv(tpr, 64) * 64 if tpr <= 256 else 256)
    return f"one{vec}", 2 * w * (c.c // vec), 256


def up_bwd_kernel(c):
    """u3d_upsample2x_bwd (upsample.hip:513-528): the 2 x 2-row kernel only for 16-byte vectors and UP_BWD_BLK = 1."""
    vec = up_vec(c.dt, c.c)
    return "blk" if vec > 1 and dict(c.opts)["UP_BWD_BLK"] == 1 else f"row{vec}"


# L: the nested three-level lerp (upsample.hip:59-60 / :149-152) rounds a product and a sum per level (the weights are
# exact; fewer where the compiler contracts to fma): 6, plus the skip add (:63 / :155)
UP_FWD_L = lambda c: 6 + int(c.skip)
# the gather (upsample.hip:274-283, :307-317, :386-402): <= 4 w taps through fmaf into ``part``, then <= 4 x 4 (od, oh)
# rows through fmaf into ``acc`` (wd * wh is exact): 20, plus the accumulate add (:292, :324, :419); 4^3 taps at most
UP_BWD_L = lambda c: 4 + 16 + int(c.accum)


def _up_rows():
    f, b = [], []
    F = lambda dt, n, c, dims, opts=(): [f.append(UpF(dt, n, c, dims, sk, tuple(opts))) for sk in (False, True)]
    for dims, n, c4 in [((1, 1, 1), 1, 4), ((7, 1, 4), 2, 4), ((5, 7, 9), 3, 8), ((1, 2, 40), 1, 16)]:
        F(F32, n, c4, dims)                                        # fp32 VEC 4; (1, 2, 40) x 16: 320 threads per row
    F(F32, 1, 2, (1, 3, 2))                                        # fp32 scalar
    F(F32, 3, 3, (5, 7, 9))
    q0 = (("UP_QUAD", 0),)
    for dims, n, c8 in [((1, 1, 1), 1, 8), ((7, 1, 4), 2, 8), ((5, 7, 9), 3, 16), ((1, 2, 40), 1, 64)]:
        F(BF, n, c8, dims, q0)                                     # bf16 one-output VEC 8; the last: 640 threads per row
    F(BF, 1, 4, (1, 3, 2))                                         # bf16 scalar
    F(BF, 3, 4, (3, 5, 7))
    for dims, n, c8 in [((1, 1, 1), 1, 8), ((1, 3, 2), 1, 16), ((7, 1, 4), 2, 8), ((5, 7, 9), 3, 16),
                        ((2, 3, 5), 2, 32),                        # w c / 8 = 20: one 64-thread block, not full
                        ((1, 2, 40), 1, 64)]:                      # 320 threads: a full block and a ragged second one
        F(BF, n, c8, dims)
    for blk in (0, 1):
        o = (("UP_BWD_BLK", blk),)
        for dt in (F32, BF):
            v = 8 if dt == BF else 4
            for accum in (False, True):
                for dims, n, c in [((1, 1, 1), 1, v), ((1, 3, 2), 1, v), ((7, 1, 4), 2, v), ((5, 7, 9), 3, 2 * v)]:
                    b.append(UpB(dt, n, c, dims, accum, o))
            b.append(UpB(dt, 2, 8 * v, (2, 3, 40), True, o))       # 320 threads per row
    o = (("UP_BWD_BLK", 0),)
    for dt in (F32, BF):
        for accum in (False, True):                                # scalar: the one-row kernel only
            b.append(UpB(dt, 1, 2, (1, 3, 2), accum, o))
            b.append(UpB(dt, 3, 3, (5, 7, 9), accum, o))
    return f, b


# =============================================================================================== stem
StemF = namedtuple("StemF", "dt n cin cout dims stride opts")
StemS = namedtuple("StemS", "n dims opts")
StemW = namedtuple("StemW", "dt n cin cout dims stride nsplit")
SM_BD, SM_BH, SM_BW = 4, 8, 32                                     # stem.hip:387-389: the weight gradient's bricks


def stem_fwd_kernel(c):
    """The kernel u3d_stem_fwd launches (stem.hip:563-590) and whether it multiplies x.to(bf16)."""
    o = dict(c.opts)
    if c.cin == 1 and c.stride == 1 and c.cout == 32 and o.get("STEM1", 1) != 0:
        if c.dt == BF and o.get("STEM_MFMA", 1) != 0:
            return "stem1_mfma"
        return "stem1_fwd"
    return "stem_fwd"


def stem_fwd_L(c):
    """stem1_mfma_kernel: one 16x16x32 instruction per output (stem.hip:254): 32. The VALU kernels: one fmaf per tap
    and input channel into one accumulator (stem.hip:42, :125): 27 cin."""
    return 32 if stem_fwd_kernel(c) == "stem1_mfma" else 27 * c.cin


def stem_out_dims(c):
    return tuple(out_dim(e, 3, c.stride) for e in c.dims)


def stem_wgrad_mfma(c):
    """stem_mfma_ok (stem.hip:593-595)."""
    return c.dt == BF and c.cin == 1 and c.cout == 32 and c.stride == 1 and c.dims[2] % SM_BW == 0


def stem_bricks(c):
    d, h, w = c.dims
    return c.n * cdiv(d, SM_BD) * cdiv(h, SM_BH) * (w // SM_BW)


def stem_wgrad_L(c):
    """VALU (stem.hip:334, :364): a slab is one fmaf chain over its split's vps = ceil(total / nsplit) voxels, staged 64
    at a time (zeros past the end): vps padded to 64. MFMA (stem.hip:479-499, :517): a wave runs SM_NV / 16 / 8 = 8
    k-steps of depth 16 per brick over its split's per = ceil(bricks / nsplit) bricks, then the 8 waves are summed: 128
    per + 8. The test sums the slabs in fp64."""
    if stem_wgrad_mfma(c):
        return cdiv(stem_bricks(c), c.nsplit) * (SM_BD * SM_BH * SM_BW // 16 // 8) * 16 + 8
    od, oh, ow = stem_out_dims(c)
    return cdiv(cdiv(c.n * od * oh * ow, c.nsplit), 64) * 64


def _stem_rows():
    f, w = [], []
    routes = [(F32, ()), (BF, (("STEM_MFMA", 0),)), (BF, ()), (F32, (("STEM1", 0),)), (BF, (("STEM1", 0),))]
    # extents of 1 along each axis in turn; w = 6, 33, 70 with n d h w no multiple of 64: waves and blocks straddle samples
    shapes = [(1, (1, 5, 7)), (1, (4, 1, 9)), (1, (3, 4, 1)), (3, (3, 5, 6)), (3, (2, 3, 33)), (3, (2, 2, 70))]
    for dt, o in routes:
        for n, dims in shapes:
            f.append(StemF(dt, n, 1, 32, dims, 1, o))
    for dt in (F32, BF):                                           # the generic kernel: both store paths, two co0 chunks
        for stride in (1, 2):
            for cin, cout in [(2, 8), (3, 24), (4, 32), (2, 40), (4, 40)]:
                f.append(StemF(dt, 2, cin, cout, (5, 7, 9), stride, ()))
    s = [StemS(3, (4, 8, 8), (("STEM_MFMA", m),)) for m in (0, 1)]
    i = 0
    for dt in (F32, BF):
        for stride in (1, 2):
            for cin, cout in [(1, 8), (2, 32), (3, 24), (4, 16)]:
                w.append(StemW(dt, 2, cin, cout, (5, 7, 9), stride, (1, 3, 7)[i % 3]))
                i += 1
        w.append(StemW(dt, 1, 2, 32, (1, 2, 5), 1, 7))            # 10 voxels in 7 splits of 2: two splits are empty
        w.append(StemW(dt, 3, 1, 32, (3, 5, 33), 1, 3))           # conv1's channels through the VALU kernel (w % 32 != 0)
    # the matrix-core kernel: 16 bricks in 16 / 3 / 5 (4 launched, one zero-filled) / 20 (16 launched) splits; d % 4, h % 8
    for n, dims, ns in [(2, (5, 9, 64), 16), (2, (5, 9, 64), 3), (2, (5, 9, 64), 5), (2, (5, 9, 64), 20),
                        (1, (1, 8, 64), 2), (1, (4, 1, 32), 1), (3, (5, 8, 32), 4), (1, (4, 5, 32), 1)]:
        w.append(StemW(BF, n, 1, 32, dims, 1, ns))
    return f, s, w


# =============================================================================================== head
HeadF = namedtuple("HeadF", "n v cin cout gn bias opts salt")
HeadB = namedtuple("HeadB", "rows cin cout opts")
HeadG = namedtuple("HeadG", "n v fused opts")
HD_GMAX = 2048                                                     # head.hip:25
HEAD_G = 8                                                         # GroupNorm groups of the head rows


def head_blocks(rows, opts):
    """head_blocks (head.hip:528-530)."""
    return min(dict(opts).get("HEAD_NB", 768), max(1, (rows + 127) // 128))


def head_fwd_tr(c):
    """The transposed forward (head.hip:550)."""
    return c.cout % 8 == 0 and dict(c.opts).get("HEAD_TR", 1) != 0 and (not c.gn or c.n * c.cin <= HD_GMAX)


# cin / 16 instructions of depth 16 into one accumulator, then the bias (head.hip:105 / :155, :119 / :161); the issue's
# round_up(cin, 32) + 1 covers it
HEAD_FWD_L = lambda c: cdiv(c.cin, 32) * 32 + 1
HEAD_DA_L = 32                                                     # two instructions of depth 16 (head.hip:223-224 / :249-250)


def head_colsum_L(rows, nb):
    """Bias partials of one block (head.hip:212, :268, :280): a lane adds one row per tile its wave visits, then 5
    shuffle steps over the 32 lanes, then the 4 waves. The test sums the blocks' rows in fp64."""
    return cdiv(cdiv(rows, 32), 4 * nb) + 5 + 4


def head_gn_bps(c):
    """u3d_head_loss_bwd_gn_bps (head.hip:600-605)."""
    return max(1, min(dict(c.opts).get("HEAD_GN_NB", 512), (c.n * c.v + 127) // 128) // c.n)


def head_gn_L(c):
    """GroupNorm partials of one block (head.hip:436-437, :466-468, :483): a lane adds one voxel per tile its wave visits
    (v / 32 tiles over 4 bps waves), 5 shuffle steps, 4 waves; the second sum's terms carry the two roundings of
    (x - mean) * rstd: + 2. The bias partials run the same chain."""
    return cdiv(c.v // 32, 4 * head_gn_bps(c)) + 5 + 4


def _head_rows():
    f, b, g = [], [], []
    H = lambda n, v, cin, cout, gn=True, bias=True, opts=(), salt=0: f.append(
        HeadF(n, v, cin, cout, gn, bias, tuple(opts), salt))
    for cin, cout in [(16, 2), (16, 16), (32, 8), (32, 13), (32, 16), (48, 24), (48, 13), (64, 32), (64, 2), (16, 32),
                      (64, 8)]:
        H(3, 101, cin, cout)                                       # 303 rows: tiles straddle samples, the last is ragged
    for gn, bias in [(False, True), (True, False), (False, False)]:
        H(3, 101, 32, 16, gn, bias)
        H(3, 101, 48, 13, gn, bias)
    H(3, 101, 64, 32, False, True)
    t0 = (("HEAD_TR", 0),)
    for cin, cout in [(32, 16), (64, 32), (16, 8), (48, 24)]:
        H(3, 101, cin, cout, opts=t0)
    H(3, 101, 32, 16, False, False, opts=t0)
    H(2, 5, 32, 16)                                                # n v < 32
    H(2, 5, 32, 13)
    H(65, 6, 32, 16)                                               # n cin = 2080 > HD_GMAX: untransposed behind GroupNorm
    H(65, 6, 32, 16, gn=False)                                     # ... and transposed without it
    for o in ((("HEAD_NB", 1),), (("HEAD_NB", 1), ("HEAD_TR", 0))):
        H(3, 101, 32, 16, opts=o)                                  # one block walks every tile
    H(3, 101, 32, 13, opts=(("HEAD_NB", 1),))
    for tr in (1, 0):
        o = (("HEAD_TR", tr),)
        for cin, cout in [(8, 2), (16, 8), (24, 13), (32, 16), (64, 24), (64, 32), (32, 2), (8, 32), (24, 16), (16, 13)]:
            b.append(HeadB(303, cin, cout, o))
        b.append(HeadB(10, 32, 13, o))
        b.append(HeadB(1000, 32, 16, o + (("HEAD_NB", 1),)))       # one block: a wave visits 8 tiles
    for fused in (False, True):
        for n, v, o in [(1, 32, ()), (3, 32, ()), (1, 224, ()), (3, 224, ()), (1, 224, (("HEAD_GN_NB", 1),)),
                        (3, 224, (("HEAD_GN_NB", 1),))]:
            g.append(HeadG(n, v, fused, o))
    return f, b, g


# =============================================================================================== helpers
Add = namedtuple("Add", "dt numel")
ChSum = namedtuple("ChSum", "dt rows c accum")
Cast = namedtuple("Cast", "dti dto rows cin cout")
ADD_GRID = 8192 * 256                                              # misc.hip:82: vectors one sweep of the grid covers


def chsum_geom(rows, c):
    """chsum_blocks (misc.hip:63-68): (blocks, rows per block, row lanes)."""
    lanes = 256 // c
    rpb = max(lanes * 4, (rows + 1023) // 1024)
    return cdiv(rows, rpb), rpb, lanes


def chsum_L(c):
    """chsum_partial (misc.hip:39, :45): a lane adds every lanes-th row of its block, then one thread adds the lanes;
    chsum_final (:56-60) sums the blocks in fp64 and rounds once to fp32, and once more where it accumulates."""
    _, rpb, lanes = chsum_geom(c.rows, c.c)
    return cdiv(min(rpb, c.rows), lanes) + lanes + 1 + int(c.accum)


ADD_L = 1                                                          # one fp32 add (misc.hip:17, :25), then the store


def _helper_rows():
    a = [Add(dt, n) for dt in (F32, BF) for n in (1, 3, 8, 1027)]
    a.append(Add(F32, ADD_GRID * 4 + 1027))                        # the grid-stride loop runs twice (the one large row)
    s, i = [], 0
    for c in (1, 2, 3, 16, 48, 100, 256):
        for rows in (1, 5, 1000, 70001):
            s.append(ChSum((F32, BF)[i % 2], rows, c, (i // 2) % 2 == 1))
            i += 1
        i += 1
    k = [Cast(di, do, rows, cin, cout) for di in (F32, BF) for do in (F32, BF)
         for rows, cin, cout in [(37, 5, 5), (3001, 3, 32), (0, 4, 8)]]
    return a, s, k


UP_FWD, UP_BWD = _up_rows()
STEM_FWD, STEM_STATS, STEM_WGRAD = _stem_rows()
HEAD_FWD, HEAD_BWD, HEAD_GN = _head_rows()
ADD, CHSUM, CAST = _helper_rows()

ID = {
    "UpF": lambda c: f"{dtn(c.dt)}-n{c.n}c{c.c}-{_x(c.dims)}{'-skip' if c.skip else ''}{_o(c.opts)}",
    "UpB": lambda c: f"{dtn(c.dt)}-n{c.n}c{c.c}-{_x(c.dims)}{'-acc' if c.accum else ''}{_o(c.opts)}",
    "StemF": lambda c: f"{dtn(c.dt)}-n{c.n}c{c.cin}x{c.cout}-{_x(c.dims)}-s{c.stride}{_o(c.opts)}",
    "StemS": lambda c: f"n{c.n}-{_x(c.dims)}{_o(c.opts)}",
    "StemW": lambda c: f"{dtn(c.dt)}-n{c.n}c{c.cin}x{c.cout}-{_x(c.dims)}-s{c.stride}-ns{c.nsplit}",
    "HeadF": lambda c: (f"n{c.n}v{c.v}c{c.cin}x{c.cout}{'-G' if c.gn else ''}{'-B' if c.bias else ''}{_o(c.opts)}"),
    "HeadB": lambda c: f"r{c.rows}c{c.cin}x{c.cout}{_o(c.opts)}",
    "HeadG": lambda c: f"n{c.n}v{c.v}{'-dbias' if c.fused else ''}{_o(c.opts)}",
    "Add": lambda c: f"{dtn(c.dt)}-{c.numel}",
    "ChSum": lambda c: f"{dtn(c.dt)}-r{c.rows}c{c.c}{'-acc' if c.accum else ''}",
    "Cast": lambda c: f"{dtn(c.dti)}-{dtn(c.dto)}-r{c.rows}c{c.cin}x{c.cout}",
}
ALL = (UP_FWD, UP_BWD, STEM_FWD, STEM_STATS, STEM_WGRAD, HEAD_FWD, HEAD_BWD, HEAD_GN, ADD, CHSUM, CAST)
for _t in ALL:
    assert len({case_id(c) for c in _t}) == len(_t), "duplicate case ids"


# =============================================================================================== inputs
def _randn(g, *shape):
    return torch.randn(shape, generator=g)


def up_inputs(c):
    g = gen(c)
    d, h, w = c.dims
    big = (c.n, 2 * d, 2 * h, 2 * w, c.c)
    if isinstance(c, UpF):
        return {"x": _randn(g, c.n, d, h, w, c.c).to(c.dt), "skip": _randn(g, *big).to(c.dt)}
    return {"dy": _randn(g, *big).to(c.dt), "prev": _randn(g, c.n, d, h, w, c.c).to(c.dt)}


def stem_inputs(c):
    """x fp32 NCDHW, w [cout,cin,3,3,3], dy [n,od,oh,ow,cout] in the row's dtype."""
    g = gen(c)
    if isinstance(c, StemS):
        return {"x": _randn(g, c.n, 1, *c.dims) + 0.5, "w": _randn(g, 32, 1, 3, 3, 3)}
    I = {"x": _randn(g, c.n, c.cin, *c.dims) * 1.5 + 0.3, "w": _randn(g, c.cout, c.cin, 3, 3, 3)}
    I["dy"] = _randn(g, c.n, *stem_out_dims(c), c.cout).to(c.dt)
    return I


def head_inputs(c):
    """HeadF: x bf16 [n,v,cin], w [cout,cin,1,1,1], gamma / beta [cin], bias [cout]. HeadB: dy fp32 [rows,cout], w.
    HeadG: x0 bf16 [n,v,32], w [16,32,1,1,1], gamma, beta, bias, labels [n,v] in 0..15, class weights [16]."""
    if isinstance(c, HeadB):
        g = gen(c)
        return {"dy": _randn(g, c.rows, c.cout), "w": 0.2 * _randn(g, c.cout, c.cin, 1, 1, 1)}
    g = gen(c, getattr(c, "salt", 0))
    cin, cout = (32, 16) if isinstance(c, HeadG) else (c.cin, c.cout)
    I = {"x": (_randn(g, c.n, c.v, cin) * 1.5 + 0.3).to(BF), "w": 0.2 * _randn(g, cout, cin, 1, 1, 1),
         "gamma": 1 + 0.1 * _randn(g, cin), "beta": 0.1 * _randn(g, cin), "bias": 0.1 * _randn(g, cout)}
    if isinstance(c, HeadG):
        I["lab"] = torch.randint(0, 16, (c.n, c.v), generator=g).float()
        I["wt"] = (torch.rand(16, generator=g) < 0.7).float()
        I["wt"][0] = 1.0
    return I


def helper_inputs(c):
    g = gen(c)
    if isinstance(c, Add):
        return {"y": _randn(g, c.numel).to(c.dt), "x": _randn(g, c.numel).to(c.dt)}
    if isinstance(c, ChSum):
        return {"x": (_randn(g, c.rows, c.c) + 0.25).to(c.dt), "prev": _randn(g, c.c)}
    return {"x": (_randn(g, max(c.rows, 1), c.cin) * 3).to(c.dti)[:c.rows]}
