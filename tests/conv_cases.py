"""The case table of test_gpu_conv.py: one row per launch of a convolution entry point, with the seeded CPU inputs and
the length of the fp32 chain behind each row's bound. CPU only (test_conv_reference.py asserts every row's conditions
without a GPU: it lies inside its family's own predicate, its routing mark is true, its ambiguous share is <= 1e-3 and
no bound is zero where the reference is not).

A row names the C entry point it launches (``entry``), the family of ops.ROUTES (or the weight-gradient family) that
entry belongs to, the direction (fwd / dgrad / wgrad), and the conv: dt, n, cin -> cout (the FORWARD conv's channels,
also for dgrad / wgrad), dims = the forward conv's INPUT extents, k, stride. ``routed``: True = production-routed
(ops.conv_route / ops.wgrad_route with the default flags picks this family for this conv); False = forced (reached
through ``route=``, a module flag or a library option, restored afterwards). ``opts``: library options (csrc/common.h)
set around the launch. ``slabs``: the split-K workspace handed to the launcher holds exactly this many slabs.

Extents are the smallest that still cross each tile edge (exact / one under / one over), channels shrink before edges.
Tile sizes, from the sources: ring32 8 x 32 output tiles per plane (conv_ring.hip RG_BH, RG_BW); conv32_brick 2 x 8 x 32;
generic brick 4 x 8 x 16 x 64 / 32 channels (conv_brick_gen.hip GB_BD, GB_BH, GB_BW); small: bricks of <= 256 voxels that
divide the volume evenly, contraction split in 32-channel chunks (conv_small_body.h sc_plan); dgrad_s2: eight parity
classes per launch; conv_s2: 8 x 16 output tiles (S2_OH, S2_OW); gemm: 128 / 256-row M tiles, 32 / 64 / 128-wide N tiles,
32- or 64-channel K stages, split-K slabs (conv.hip launch_igemm); weight-gradient ring 16 x 16, 12 x 12 or 12 x 24 plane
tiles (wgrad_ring_body.h wr_geom), bricks 3 (2) x 8 x 16 at stride 1 and 3 (2) x 4 x 8 output voxels at stride 2
(wgrad_brick.hip brick_dims), wgrad1 chunks of 512 voxels (W1_NV), u3d_conv_wgrad slabs of voxels rounded up to 32.

Out of scope (the next pass; see test_gpu_conv.py): the stem, the streaming head, the upsample kernels and the fused
forms that are pinned bitwise to the plain launches.
"""
import zlib
from collections import namedtuple

import torch

from conv_reference import BF, F32, out_dim

Case = namedtuple("Case", "family entry dir dt n cin cout dims k stride gn res bias out_f32 routed opts slabs mode")


DEFAULT_OPTS = {"CONVG_PERSIST": 1, "WGRAD_BD": 3, "WB_S2BD": 3, "WB_S2CO64": 1}  # (csrc/runtime.cpp's defaults)


def forced_by_opts(opts):
    """Whether a row sets a library option to something other than its default: then it is a forced row."""
    return any(DEFAULT_OPTS.get(k) != v for k, v in opts)


def C(family, entry, dir, n, cin, cout, dims, k=3, stride=1, dt=BF, gn=False, res=False, bias=False, out_f32=False,
      routed=False, opts=(), slabs=0, mode=""):
    opts = tuple(sorted(dict(opts).items()))
    return Case(family, entry, dir, dt, n, cin, cout, tuple(dims), k, stride, gn, res, bias, out_f32,
                routed and not forced_by_opts(opts), opts, slabs, mode)


def case_id(c):
    dtn = "bf16" if c.dt == BF else "fp32"
    flags = "".join(f for f, on in (("G", c.gn), ("R", c.res), ("B", c.bias), ("F", c.out_f32)) if on)
    opts = "".join(f"_{k}{v}" for k, v in c.opts)
    return (f"{c.entry[4:]}-{c.dir}-{dtn}-n{c.n}c{c.cin}x{c.cout}-{'x'.join(map(str, c.dims))}-k{c.k}s{c.stride}"
            + (f"-{flags}" if flags else "") + (f"-m{c.slabs}" if c.slabs else "") + (f"-{c.mode}" if c.mode else "")
            + opts)


def groups(cin):
    return 16 if cin % 16 == 0 else 8


def round32(c):
    return (c + 31) // 32 * 32


def out_dims(c):
    return tuple(out_dim(d, c.k, c.stride) for d in c.dims)


# ----------------------------------------------------------------------------------------------- inputs
def _randn(gen, *shape):
    return torch.randn(shape, generator=gen)


def make_inputs(c):
    """Seeded CPU inputs of a row (the operand distributions of test_gpu_bf16._case), the same bits on every machine:
    x [n,d,h,w,cin] and dy / res [n,od,oh,ow,cout] in the row's dtype, w [cout,cin,k,k,k], gamma, beta, bias fp32."""
    gen = torch.Generator().manual_seed(zlib.crc32(case_id(c).encode()) & 0x7FFFFFFF)
    od = out_dims(c)
    I = {"x": (_randn(gen, c.n, *c.dims, c.cin) * 1.5 + 0.3).to(c.dt),
         "w": _randn(gen, c.cout, c.cin, c.k, c.k, c.k),
         "gamma": 1 + 0.1 * _randn(gen, c.cin), "beta": 0.1 * _randn(gen, c.cin),
         "dy": _randn(gen, c.n, *od, c.cout).to(c.dt),
         "res": _randn(gen, c.n, *od, c.cout).to(c.dt),
         "bias": _randn(gen, c.cout)}
    # the last channel's shift sh = beta - mean * sc is positive in every row: a prologue applied where the operand
    # is zero padding (a halo voxel outside the volume, a channel of the cin_p padding, whose coefficients the kernels
    # clamp to channel cin - 1) then yields relu(sh) > 0 instead of 0 and shows, whatever the seed
    I["beta"][-1] = 0.75
    return I


# ----------------------------------------------------------------------------------------------- chain lengths
def chain_len(c, slabs=1):
    """L of a forward / data-gradient row: the fp32 additions on the longest chain to one output. Every kernel keeps ONE
    fp32 accumulator per output and contraction split and feeds it MFMAs of depth 16 or 32 (2 in fp32) over the padded
    contraction, so the chain is the (padded) term count k^3 * cx_p of the split, then the slabs' sum, the residual and
    the bias: L = k^3 cx_p + slabs + 2 (test_gpu_conv.py lists the line per kernel). cx = the channels contracted."""
    cx = c.cin if c.dir == "fwd" else c.cout
    return c.k ** 3 * round32(cx) + slabs + 2


def wgrad_slab_terms(c, ns):
    """L of a weight-gradient row: the voxels one slab sums (each slab is one accumulator chain over its voxels, padded
    to the MFMA depth; the test sums the slabs in fp64), from the launcher's own split of the volume into ns slabs."""
    n = c.n
    d, h, w = c.dims
    od, oh, ow = out_dims(c)
    cd = lambda a, b: -(-a // b)
    if c.entry == "u3d_conv_wgrad_ring":        # wgrad_ring.hip:375 per = ceil(planes / nsplit) plane tiles of ph x pw
        ph = pw = 16
        if dict(c.opts).get("WR_TILE16", 0) == 0 and w % 16 != 0 and w % 12 == 0 and h % 12 == 0:
            ph, pw = 12, (24 if w % 24 == 0 else 12)
        planes = n * cd(h, ph) * cd(w, pw) * d
        return cd(planes, ns) * (-(-ph * pw // 32) * 32)
    if c.entry == "u3d_conv_wgrad_brick":       # wgrad_brick_body.h wb_geom: per_split = ceil(bricks / nsplit)
        o = dict(c.opts)
        if c.stride == 1:
            bd, bh, bw = (2 if o.get("WGRAD_BD", 3) == 2 else 3), 8, 16
        else:
            bd, bh, bw = (2 if o.get("WB_S2BD", 3) == 2 else 3), 4, 8
        nb = n * cd(od, bd) * cd(oh, bh) * cd(ow, bw)
        return cd(nb, ns) * bd * bh * bw
    if c.entry == "u3d_conv_wgrad1":            # wgrad_brick.hip:286 per_split = ceil(chunks / nsplit) * 512
        return cd(cd(n * od * oh * ow, 512), ns) * 512
    vps = cd(n * od * oh * ow, ns)              # conv.hip:1014 vps rounded up to 32
    return cd(vps, 32) * 32


# ----------------------------------------------------------------------------------------------- the table
def _ring32():
    rows = []
    dims = [(1, (1, 1, 1)), (1, (3, 8, 32)), (1, (4, 7, 31)), (1, (5, 9, 33)), (3, (9, 5, 70)),
            (8, (33, 16, 16))]                   # the last: PER2 of test_gpu_fullsize.py (a workgroup walks two ranges)
    for n, d in dims:                            # the same rows through the static ring and its work-stealing form
        for entry, routed in (("u3d_conv32_ring", True), ("u3d_conv32_ring_q", False)):
            rows.append(C("ring32", entry, "fwd", n, 32, 32, d, gn=True, res=True, routed=routed))
            rows.append(C("ring32", entry, "fwd", n, 32, 32, d, routed=routed))
            rows.append(C("ring32", entry, "dgrad", n, 32, 32, d, routed=routed))
            if d in (dims[3][1], dims[4][1]):    # prologue only, residual only
                rows.append(C("ring32", entry, "fwd", n, 32, 32, d, gn=True, routed=routed))
                rows.append(C("ring32", entry, "fwd", n, 32, 32, d, res=True, routed=routed))
    # 2 x 8 x 32 bricks, w % 32 == 0, n <= 16: exact, one over / under in d and h, two bricks in w, a PER2 row
    for i, (n, d) in enumerate([(1, (2, 8, 32)), (1, (3, 9, 32)), (1, (1, 7, 32)), (3, (5, 7, 64)), (8, (40, 8, 32))]):
        rows.append(C("ring32", "u3d_conv32_brick", "fwd", n, 32, 32, d, gn=True, res=True))
        rows.append(C("ring32", "u3d_conv32_brick", "fwd", n, 32, 32, d))
        rows.append(C("ring32", "u3d_conv32_brick", "dgrad", n, 32, 32, d))
        if i in (1, 3):
            rows.append(C("ring32", "u3d_conv32_brick", "fwd", n, 32, 32, d, gn=True))
            rows.append(C("ring32", "u3d_conv32_brick", "fwd", n, 32, 32, d, res=True))
    return rows


def _brick():
    rows = []
    chans = [(24, 24), (40, 48), (64, 128), (128, 64), (256, 256)]
    dims = [(4, 8, 16), (3, 7, 15), (5, 9, 17), (1, 1, 1)]
    i = 0
    for ci, co in chans:
        for d in dims:
            n = 1 if i % 2 else 3
            pf, pg = i % 2, (i // 2 + i) % 2    # one-shot / persistent alternate over channels, dims and directions
            rows.append(C("brick", "u3d_convg_brick", "fwd", n, ci, co, d, gn=True, res=True, opts={"CONVG_PERSIST": pf}))
            rows.append(C("brick", "u3d_convg_brick", "dgrad", n, ci, co, d, opts={"CONVG_PERSIST": pg}))
            i += 1
    for pers in (0, 1):
        rows.append(C("brick", "u3d_convg_brick", "fwd", 3, 40, 48, (5, 9, 17), opts={"CONVG_PERSIST": pers}))
        rows.append(C("brick", "u3d_convg_brick", "fwd", 1, 64, 128, (3, 7, 15), gn=True, opts={"CONVG_PERSIST": pers}))
        rows.append(C("brick", "u3d_convg_brick", "fwd", 1, 128, 64, (5, 9, 17), res=True, opts={"CONVG_PERSIST": pers}))
        rows.append(C("brick", "u3d_convg_brick", "fwd", 3, 24, 24, (3, 7, 15), gn=True, res=True,
                      opts={"CONVG_PERSIST": pers}))
        rows.append(C("brick", "u3d_convg_brick", "dgrad", 3, 256, 256, (3, 7, 15), opts={"CONVG_PERSIST": pers}))
        rows.append(C("brick", "u3d_convg_brick", "dgrad", 1, 40, 48, (5, 9, 17), opts={"CONVG_PERSIST": pers}))
    # production-routed: >= 128 workgroups, more voxels than the small family takes (8-wide persistent bricks: w = 24)
    rows.append(C("brick", "u3d_convg_brick", "fwd", 2, 64, 128, (16, 16, 32), gn=True, res=True, routed=True))
    rows.append(C("brick", "u3d_convg_brick", "dgrad", 2, 128, 64, (16, 16, 32), routed=True))
    rows.append(C("brick", "u3d_convg_brick", "fwd", 2, 64, 128, (14, 17, 24), gn=True, routed=True))
    return rows


def _small():
    rows = []
    chans = [(24, 24), (128, 256), (256, 256)]
    dims = [(2, (12, 12, 12)), (1, (6, 6, 6)), (1, (1, 1, 1)), (1, (5, 7, 9))]
    i = 0
    for ci, co in chans:
        for n, d in dims:
            full = i % 2 == 0
            rows.append(C("small", "u3d_conv_small2", "fwd", n, ci, co, d, gn=full, res=full, routed=True, slabs=8))
            rows.append(C("small", "u3d_conv_small2", "dgrad", n, ci, co, d, routed=True, slabs=8))
            if d in ((12, 12, 12), (5, 7, 9)):  # SMALL_FUSE off: u3d_conv_small + small_reduce_kernel
                rows.append(C("small", "u3d_conv_small", "fwd", n, ci, co, d, gn=not full, res=not full, slabs=8))
                rows.append(C("small", "u3d_conv_small", "dgrad", n, ci, co, d, slabs=8))
            i += 1
    # a split count that does not divide the contraction: 8 chunks of 32 channels over 3 workgroups (3 + 3 + 2), 5 over 2
    for entry in ("u3d_conv_small2", "u3d_conv_small"):
        r = entry == "u3d_conv_small2"
        rows.append(C("small", entry, "fwd", 1, 256, 256, (6, 6, 6), gn=True, res=True, routed=r, slabs=3))
        rows.append(C("small", entry, "dgrad", 1, 256, 256, (6, 6, 6), routed=r, slabs=3))
        rows.append(C("small", entry, "fwd", 1, 160, 64, (5, 7, 9), gn=True, routed=r, slabs=2))
        rows.append(C("small", entry, "dgrad", 1, 64, 160, (5, 7, 9), routed=r, slabs=2))
    # no workspace: the whole contraction in one workgroup
    rows.append(C("small", "u3d_conv_small2", "fwd", 1, 128, 256, (6, 6, 6), gn=True, res=True, routed=True, slabs=0))
    return rows


def _s2():
    rows = []
    dims = [(1, 1, 1), (2, 2, 2), (7, 9, 11), (12, 16, 34), (6, 6, 6)]
    chans = [(32, 64), (64, 128), (40, 48), (256, 256)]
    i = 0
    for ci, co in chans:
        for d in dims:
            rows.append(C("s2", "u3d_conv_dgrad_s2", "dgrad", 1 + i % 2, ci, co, d, stride=2, routed=True))
            i += 1
    # stride-2 ring forward (32 -> 64 behind a prologue, 8 x 16 output tiles): output (2, 8, 16) exact from an even
    # and an odd input, (., 7, 15) one under, (., 9, 17) one over, one voxel; n = 3
    for n, d in [(1, (1, 1, 1)), (1, (4, 16, 32)), (3, (3, 15, 31)), (1, (4, 14, 30)), (3, (2, 13, 29)),
                 (1, (5, 17, 33)), (2, (7, 18, 34))]:
        rows.append(C("gemm", "u3d_conv_s2_ring", "fwd", n, 32, 64, d, stride=2, gn=True))
    return rows


def _gemm():
    rows = []
    g = lambda *a, **k: rows.append(C("gemm", *a, **k))
    for dt in (F32, BF):
        p32 = dt == F32                          # every fp32 conv is production-routed to the implicit GEMM
        # k x stride x direction at odd extents (stride 2 data gradients need even ones); N tile 32 in bf16 (small
        # volumes narrow to it, conv.hip:784-785), 32 / 64 in fp32
        g("u3d_conv_fwd", "fwd", 2, 32, 24, (5, 7, 9), k=3, stride=1, dt=dt, gn=True, res=True, routed=p32)
        g("u3d_conv_fwd", "fwd", 1, 32, 64, (7, 9, 11), k=3, stride=2, dt=dt, gn=True, routed=True)
        g("u3d_conv_fwd", "fwd", 2, 64, 48, (5, 7, 9), k=1, stride=1, dt=dt, gn=True, routed=p32)
        g("u3d_conv_fwd", "fwd", 1, 96, 128, (7, 9, 11), k=1, stride=2, dt=dt, gn=True, routed=p32)
        g("u3d_conv_dgrad", "dgrad", 2, 24, 32, (5, 7, 9), k=3, stride=1, dt=dt, routed=p32)
        g("u3d_conv_dgrad", "dgrad", 1, 64, 96, (5, 7, 9), k=1, stride=1, dt=dt, routed=p32)
        # stride-2 3^3 data gradient: eight parity classes (1, 2, 4 and 8 taps)
        g("u3d_conv_dgrad", "dgrad", 2, 32, 64, (6, 8, 10), k=3, stride=2, dt=dt, routed=p32)
        g("u3d_conv_dgrad", "dgrad", 1, 64, 40, (2, 2, 2), k=3, stride=2, dt=dt, routed=p32)
        # stride-2 1^3 data gradient: the odd voxels exactly zero
        g("u3d_conv_dgrad", "dgrad", 2, 32, 64, (8, 6, 10), k=1, stride=2, dt=dt, routed=True)
        g("u3d_conv_dgrad", "dgrad", 1, 256, 256, (4, 6, 2), k=1, stride=2, dt=dt, routed=True)
        # bias / fp32 output / residual epilogues, unsplit and through the split-K reduce kernel
        g("u3d_conv_fwd", "fwd", 2, 32, 16, (5, 7, 9), k=1, dt=dt, gn=True, bias=True, out_f32=True, routed=True)
        g("u3d_conv_fwd", "fwd", 1, 64, 64, (4, 5, 6), k=3, dt=dt, res=True, bias=True, routed=True, slabs=8)
        g("u3d_conv_fwd", "fwd", 1, 64, 16, (4, 5, 6), k=3, dt=dt, bias=True, out_f32=True, routed=True, slabs=8)
        # split-K forced: 27 K-steps (cin_p 64 in bf16 64-channel stages, cin_p 32 in fp32) in 8 splits of 4: the eighth
        # has none; in 4 splits of 7: the last is short; the data gradient likewise
        ck = 32 if p32 else 64
        g("u3d_conv_fwd", "fwd", 1, ck, 64, (5, 6, 7), k=3, dt=dt, gn=True, res=True, routed=p32, slabs=8,
          opts={"IGEMM_NS": 8})
        g("u3d_conv_fwd", "fwd", 2, ck, 40, (3, 5, 9), k=3, dt=dt, routed=p32, slabs=4, opts={"IGEMM_NS": 4})
        g("u3d_conv_dgrad", "dgrad", 1, 48, ck, (5, 6, 7), k=3, dt=dt, routed=p32, slabs=8, opts={"IGEMM_NS": 8})
        g("u3d_conv_dgrad", "dgrad", 1, 48, ck, (4, 6, 8), k=3, stride=2, dt=dt, routed=p32, slabs=8,
          opts={"IGEMM_NS": 8})
        # prologue in the K loop at 64 channels (fp32 keeps it there; bf16 materialises relu(gn(x)) from 64 channels)
        g("u3d_conv_fwd", "fwd", 2, 128, 64, (3, 5, 7), k=3, stride=2, dt=dt, gn=True, routed=True, slabs=8)
    # bf16 N tile 128 (IGEMM_AUTO off: the narrowing for small volumes would halve it), 32- and 64-channel K stages
    g("u3d_conv_fwd", "fwd", 1, 32, 128, (5, 7, 9), k=3, gn=True, res=True, opts={"IGEMM_AUTO": 0})
    g("u3d_conv_fwd", "fwd", 1, 64, 160, (5, 7, 9), k=3, stride=2, gn=True, routed=True, opts={"IGEMM_AUTO": 0})
    g("u3d_conv_dgrad", "dgrad", 1, 128, 96, (5, 7, 9), k=3, opts={"IGEMM_AUTO": 0})
    # bf16 128-row M tile with the 64-wide N tile (cout_p 64; the form of the mid-size stride-2 layers), both K stages
    g("u3d_conv_fwd", "fwd", 1, 32, 64, (7, 9, 11), k=3, stride=2, gn=True, opts={"IGEMM_AUTO": 0})
    g("u3d_conv_fwd", "fwd", 2, 64, 64, (5, 7, 9), k=3, gn=True, res=True, opts={"IGEMM_AUTO": 0})
    g("u3d_conv_dgrad", "dgrad", 1, 64, 32, (5, 7, 9), k=3, opts={"IGEMM_AUTO": 0})
    g("u3d_conv_dgrad", "dgrad", 2, 40, 64, (4, 6, 8), k=3, stride=2, opts={"IGEMM_AUTO": 0})
    # the 256-row M tile: cdiv(Mq, 256) * cdiv(cout, 64) * n >= 256 (the one large row)
    g("u3d_conv_fwd", "fwd", 2, 32, 64, (64, 64, 64), k=3, stride=2, gn=True, routed=True)
    return rows


def _conv1x1():
    rows = []
    dims = [(5, 7, 9), (4, 6, 8), (1, 2, 3), (3, 5, 33)]  # (one voxel per group leaves GroupNorm nothing to normalise)
    i = 0
    for cx in (8, 24, 256):
        for cy in (8, 24, 256):
            d = dims[i % 4]
            rows.append(C("conv1x1", "u3d_conv1x1", "fwd", 1 + 2 * (i % 2), cx, cy, d, k=1, stride=1, gn=True, routed=True))
            rows.append(C("conv1x1", "u3d_conv1x1", "fwd", 3 - 2 * (i % 2), cx, cy, dims[(i + 1) % 4], k=1, stride=2,
                          gn=i % 3 != 0, routed=True))
            i += 1
    for cx, cy in [(8, 24), (256, 8), (24, 256), (64, 32)]:
        rows.append(C("conv1x1", "u3d_conv1x1", "dgrad", 3, cx, cy, (5, 7, 9), k=1, stride=1, routed=True))
    return rows


def _wgrad():
    rows = []
    # the ring: h, w in {8, 12, 16, 17, 33}; d in {1, 2, 5}; n = 3: a plane range crosses a sample
    dims = [(1, 8, 8), (2, 12, 12), (5, 16, 16), (2, 17, 33), (1, 33, 17), (2, 12, 24), (5, 8, 17), (2, 16, 12),
            (5, 33, 8), (1, 17, 12)]
    chans = [(32, 32), (64, 32), (128, 256)]
    for i, d in enumerate(dims):
        ci, co = chans[i % 3]
        rows.append(C("wgrad_ring", "u3d_conv_wgrad_ring", "wgrad", 3, ci, co, d, gn=True, routed=True, mode="splits"))
        ci, co = chans[(i + 1) % 3]
        rows.append(C("wgrad_ring", "u3d_conv_wgrad_ring", "wgrad", 3, ci, co, d, gn=i % 2 == 1, mode="target"))
        ci, co = chans[(i + 2) % 3]
        rows.append(C("wgrad_ring", "u3d_conv_wgrad_ring", "wgrad", 1 + i % 2, ci, co, d, routed=True, mode="splits"))
    # cin_p / cout_p padding behind the prologue (the slabs' padded rows and columns hold exact zeros)
    rows.append(C("wgrad_ring", "u3d_conv_wgrad_ring", "wgrad", 3, 40, 48, (2, 17, 12), gn=True, routed=True, mode="splits"))
    rows.append(C("wgrad_ring", "u3d_conv_wgrad_ring", "wgrad", 1, 24, 8, (2, 12, 12), gn=True, routed=True, mode="splits"))
    # one slab per two plane tiles (WR_WGS small): a range of several planes that crosses a sample
    rows.append(C("wgrad_ring", "u3d_conv_wgrad_ring", "wgrad", 3, 32, 32, (5, 17, 33), gn=True, routed=True,
                  mode="splits", opts={"WR_WGS": 7}))
    rows.append(C("wgrad_ring", "u3d_conv_wgrad_ring", "wgrad", 3, 64, 32, (5, 12, 24), gn=True, routed=True,
                  mode="splits", opts={"WR_WGS": 8}))
    # halo bricks, stride 1 (h or w < 8 in production) and 2: odd extents, 2- and 3-plane bricks, 1 / 2 co tiles, 40 -> 48
    for ci, co, n, d in [(40, 48, 1, (5, 7, 9)), (32, 64, 3, (7, 9, 11)), (64, 128, 2, (6, 10, 14))]:
        for bd in (2, 3):
            rows.append(C("wgrad_brick", "u3d_conv_wgrad_brick", "wgrad", n, ci, co, d, stride=1, gn=True,
                          routed=min(d[1:]) < 8, opts={"WGRAD_BD": bd}))
            for nco in (0, 1):
                rows.append(C("wgrad_brick", "u3d_conv_wgrad_brick", "wgrad", n, ci, co, d, stride=2, gn=bd == 3,
                              routed=True, opts={"WB_S2BD": bd, "WB_S2CO64": nco}))
    rows.append(C("wgrad_brick", "u3d_conv_wgrad_brick", "wgrad", 3, 32, 32, (9, 5, 17), gn=True, routed=True,
                  opts={"WB_WGS": 3}))                          # several bricks per slab, slabs that cross samples
    rows.append(C("wgrad_brick", "u3d_conv_wgrad_brick", "wgrad", 3, 32, 64, (9, 10, 17), stride=2, gn=True,
                  routed=True, opts={"WB_WGS": 3}))
    # the 1^3 kernel, stride 1 and 2 (512-voxel chunks)
    for n, ci, co, d, s in [(2, 32, 16, (8, 10, 12), 1), (2, 32, 64, (8, 10, 12), 2), (1, 64, 128, (6, 6, 7), 2),
                            (1, 32, 8, (5, 7, 9), 1), (3, 40, 48, (5, 7, 9), 2), (1, 256, 256, (1, 1, 1), 1)]:
        rows.append(C("wgrad1", "u3d_conv_wgrad1", "wgrad", n, ci, co, d, k=1, stride=s, gn=True, routed=True))
        rows.append(C("wgrad1", "u3d_conv_wgrad1", "wgrad", n, ci, co, d, k=1, stride=s, routed=True))
    # the implicit-GEMM weight gradient, fp32 and bf16, k 1 / 3, stride 1 / 2; slabs = the split count handed over:
    # 7 slabs over 630 voxels (96 per slab, the last 54), 5 over 100 (32 per slab: the fifth has none)
    for dt in (F32, BF):
        p32 = dt == F32
        rows.append(C("wgrad_gemm", "u3d_conv_wgrad", "wgrad", 2, 32, 48, (5, 7, 9), k=3, dt=dt, gn=True, routed=p32, slabs=7))
        rows.append(C("wgrad_gemm", "u3d_conv_wgrad", "wgrad", 2, 40, 32, (5, 7, 9), k=1, dt=dt, gn=True, routed=p32, slabs=7))
        rows.append(C("wgrad_gemm", "u3d_conv_wgrad", "wgrad", 1, 64, 32, (7, 9, 11), k=3, stride=2, dt=dt, routed=p32, slabs=3))
        rows.append(C("wgrad_gemm", "u3d_conv_wgrad", "wgrad", 1, 32, 64, (7, 9, 11), k=1, stride=2, dt=dt, routed=p32, slabs=1))
        rows.append(C("wgrad_gemm", "u3d_conv_wgrad", "wgrad", 1, 32, 32, (4, 5, 5), k=3, dt=dt, gn=True, routed=p32, slabs=5))
    return rows


CASES = _ring32() + _brick() + _small() + _s2() + _gemm() + _conv1x1() + _wgrad()
assert len({case_id(c) for c in CASES}) == len(CASES), "duplicate case ids"
FWD_DGRAD = [c for c in CASES if c.dir != "wgrad"]
WGRAD = [c for c in CASES if c.dir == "wgrad"]
# (dtype, k, dims): a stride-2 data gradient of the implicit GEMM at an odd extent must raise and write nothing
ODD_S2 = [(BF, 3, (5, 6, 8)), (F32, 3, (6, 7, 8)), (BF, 1, (6, 6, 7)), (F32, 1, (5, 7, 9))]
