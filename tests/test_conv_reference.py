"""Pins tests/conv_reference.py (the fp64 restatement test_gpu_conv.py compares the convolution kernels against) to torch
autograd in fp64, to oracle/ref_cpu.py and to the golden vectors, and asserts on the CPU the conditions of every row of
tests/conv_cases.py: it lies inside its family's own predicate, its routing mark is true, the ambiguous share of its
prologue is <= 1e-3, no bound is zero where the reference is not, and its inputs come from seeded CPU generators."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import conv_cases as cc
import conv_reference as cr
from conftest import golden
from conv_reference import BF, F32, cl, nd
from gn_reference import exact_stats
from oracle import ref_cpu as O

def _gen(seed):
    return torch.Generator().manual_seed(seed)


@pytest.mark.parametrize("k", [1, 3])
@pytest.mark.parametrize("stride", [1, 2])
@pytest.mark.parametrize("dims", [(5, 7, 9), (4, 6, 8), (1, 1, 1), (2, 5, 8)])
def test_refs_match_autograd_fp64(k, stride, dims):
    g = _gen(7 * k + stride + sum(dims))
    n, cin, cout = 2, 5, 7
    a = torch.randn((n,) + dims + (cin,), generator=g, dtype=torch.float64)
    w = torch.randn((cout, cin, k, k, k), generator=g, dtype=torch.float64)
    od = tuple(cr.out_dim(d, k, stride) for d in dims)
    res = torch.randn((n,) + od + (cout,), generator=g, dtype=torch.float64)
    bias = torch.randn(cout, generator=g, dtype=torch.float64)
    dy = torch.randn((n,) + od + (cout,), generator=g, dtype=torch.float64)
    ax, wx = cl(a).clone().requires_grad_(True), w.clone().requires_grad_(True)
    y = F.conv3d(ax, wx, bias, stride, k // 2)
    ref, S = cr.conv_fwd_ref(a, w, k, stride, res, bias)
    torch.testing.assert_close(ref, nd(y.detach()) + res, rtol=1e-12, atol=1e-12)
    assert bool((S >= ref.abs() * (1 - 1e-12)).all())                  # the absolute sum dominates the value
    y.backward(cl(dy))
    dx, Sx = cr.conv_dgrad_ref(dy, w, (n,) + dims, k, stride)
    torch.testing.assert_close(dx, nd(ax.grad), rtol=1e-12, atol=1e-12)
    dw, Sw = cr.conv_wgrad_ref(a, dy, k, stride)
    torch.testing.assert_close(dw, wx.grad.reshape(cout, cin, k ** 3).permute(2, 0, 1), rtol=1e-12, atol=1e-12)
    assert bool((Sx >= dx.abs() * (1 - 1e-12)).all()) and bool((Sw >= dw.abs() * (1 - 1e-12)).all())
    # the absolute sums are the same operations on the absolute operands
    torch.testing.assert_close(Sx, cr.conv_dgrad_ref(dy.abs(), w.abs(), (n,) + dims, k, stride)[0], rtol=1e-12, atol=0)
    torch.testing.assert_close(Sw, cr.conv_wgrad_ref(a.abs(), dy.abs(), k, stride)[0], rtol=1e-12, atol=0)
    # the ambiguity term is linear in a_delta
    dl = torch.rand(a.shape, generator=g, dtype=torch.float64)
    torch.testing.assert_close(cr.conv_fwd_ref(a, w, k, stride, a_delta=dl)[2],
                               cr.conv_fwd_ref(dl, w.abs(), k, stride)[0], rtol=1e-12, atol=0)
    torch.testing.assert_close(cr.conv_wgrad_ref(a, dy, k, stride, a_delta=dl)[2],
                               cr.conv_wgrad_ref(dl, dy.abs(), k, stride)[0], rtol=1e-12, atol=0)


@pytest.mark.parametrize("tag,s", [("c3s1", 1), ("c3s2", 2), ("c1s2", 2), ("c3s1b", 1), ("c1s1", 1)])
def test_refs_match_oracle_and_golden(tag, s):
    g = golden("g4_ops.npz")
    x, w, up = (torch.from_numpy(g[f"{tag}_{v}"]) for v in ("x", "w", "up"))
    k = w.shape[2]
    wr = w.clone().requires_grad_(True)
    wst = O.ws_weight(wr)
    y, _ = cr.conv_fwd_ref(nd(x).double(), wst.detach().double(), k, s)
    np.testing.assert_allclose(cl(y).numpy(), O.conv(x, w, s).numpy(), atol=1e-4)  # (the oracle runs in fp32)
    np.testing.assert_allclose(cl(y).numpy(), g[f"{tag}_y"], atol=1e-4)
    dx, _ = cr.conv_dgrad_ref(nd(up).double(), wst.detach().double(), (x.shape[0],) + tuple(x.shape[2:]), k, s)
    np.testing.assert_allclose(cl(dx).numpy(), g[f"{tag}_dx"], atol=1e-4)
    dw, _ = cr.conv_wgrad_ref(nd(x).double(), nd(up).double(), k, s)      # d / d W_hat; through the standardisation:
    wst.backward(dw.permute(1, 2, 0).reshape(w.shape).float())
    np.testing.assert_allclose(wr.grad.numpy(), g[f"{tag}_dw"], atol=1e-3, rtol=1e-4)


def test_decode_pf_inverts_the_pack_layout():
    w = torch.randn(24, 40, 3, 3, 3, generator=_gen(3))
    pf = torch.zeros(27, 32, 64)
    pf[:, :24, :40] = w.reshape(24, 40, 27).permute(2, 0, 1)
    assert torch.equal(cr.decode_pf(pf, 24, 40, 3), w.double())


@pytest.mark.parametrize("dt", [BF, F32])
@pytest.mark.parametrize("n,c,dims,G", [(2, 32, (4, 5, 6), 16), (1, 24, (3, 5, 7), 8), (3, 256, (2, 2, 3), 16)])
def test_prologue_ref_equals_gn_forward(dt, n, c, dims, G):
    """prologue_ref against relu(F.group_norm) in fp64 from the exact statistics (gn_reference.exact_stats; handed
    over in fp32, so to fp32 resolution), and its mask / delta against the fp32 evaluation a kernel runs."""
    g = _gen(c + n)
    x = (torch.randn((n,) + dims + (c,), generator=g) * 1.5 + 0.3).to(dt)
    ga, be = 1 + 0.1 * torch.randn(c, generator=g), 0.1 * torch.randn(c, generator=g)
    st = exact_stats(x, G)[0].float()
    a, mask, delta = cr.prologue_ref(x, st, ga, be, G, dt)
    ref = nd(F.relu(F.group_norm(cl(x.double()), G, ga.double(), be.double(), 1e-5)))
    tol = 2.0 ** -8 if dt == BF else 1e-5                              # (one rounding to bf16)
    assert bool(((a - ref).abs() <= tol * ref.abs() + 1e-5).all())
    assert mask.double().mean().item() <= cr.MAX_AMBIGUOUS
    # the fp32 prologue (the expression of test_gpu_bf16._act_ref): wherever it rounds otherwise, the mask is set,
    # and it never moves further than delta
    gi = torch.arange(c) // (c // G)
    sc = st[:, gi, 1] * ga[None]
    sh = be[None] - st[:, gi, 0] * sc
    v = (n, 1, 1, 1, c)
    for af in (torch.clamp_min(torch.addcmul(sh.view(v), x.float(), sc.view(v)), 0),
               torch.clamp_min(x.float() * sc.view(v) + sh.view(v), 0)):
        af = af.to(dt).double()
        if dt == BF:
            assert not bool(((af != a) & ~mask).any())
        assert bool(((af - a).abs() <= delta).all())


def test_bf16_spacing_and_boundaries():
    v = torch.tensor([1.0, 1.5, 1.9921875, 2.0, 0.75, 3.0], dtype=torch.float64)
    sp, p2 = cr._spacing(v, BF)
    assert sp.tolist() == [2.0 ** -7, 2.0 ** -7, 2.0 ** -7, 2.0 ** -6, 2.0 ** -8, 2.0 ** -6]
    assert p2.tolist() == [True, False, False, True, False, False]


# ------------------------------------------------------------------------------------------------ the case table
def _predicate(c):
    """The applicability test of the row's own kernel (u3d.ops predicates and the launchers' REQUIREs)."""
    from u3d import ops
    n, (d, h, w) = c.n, c.dims
    bf = c.dt == BF
    cx, cy = (c.cin, c.cout) if c.dir == "fwd" else (c.cout, c.cin)
    shape = (n, d, h, w)
    if c.entry in ("u3d_conv32_ring", "u3d_conv32_ring_q"):
        return ops._use_conv32(c.dt, cx, cy, c.k, c.stride, n, w) and not (c.dir == "dgrad" and (c.gn or c.res))
    if c.entry == "u3d_conv32_brick":
        old = ops.CONV32_FN
        ops.CONV32_FN = "u3d_conv32_brick"
        try:
            return ops._use_conv32(c.dt, cx, cy, c.k, c.stride, n, w)
        finally:
            ops.CONV32_FN = old
    if c.entry == "u3d_convg_brick":
        old = ops.BRICK_MIN_WG
        ops.BRICK_MIN_WG = 0 if not c.routed else old
        try:
            return ops._use_gen_brick(c.dt, cx, cy, c.k, c.stride, shape)
        finally:
            ops.BRICK_MIN_WG = old
    if c.entry in ("u3d_conv_small", "u3d_conv_small2"):
        return ops._use_small(c.dt, cx, cy, c.k, c.stride, shape) and not (c.dir == "dgrad" and (c.gn or c.res))
    if c.entry == "u3d_conv_dgrad_s2":
        return bf and c.k == 3 and c.stride == 2 and c.cin % 8 == 0 and c.cout % 8 == 0 and c.dir == "dgrad"
    if c.entry == "u3d_conv_s2_ring":  # conv_s2.hip s2_geom
        return bf and c.gn and (c.cin, c.cout, c.k, c.stride) == (32, 64, 3, 2) and n * 16 <= 512 and not c.res
    if c.entry == "u3d_conv_fwd":
        return c.k in (1, 3) and c.stride in (1, 2) and c.cin % 8 == 0 and not (c.out_f32 and c.res) \
            and (not c.gn or c.cin <= 256)
    if c.entry == "u3d_conv_dgrad":
        return c.cout % 8 == 0 and (c.stride == 1 or all(v % 2 == 0 for v in c.dims)) and not (c.gn or c.res or c.bias)
    if c.entry == "u3d_conv1x1":
        return ops._use_conv1x1(c.dt, cx, cy, c.k, n) and (c.dir == "fwd" or c.stride == 1) and not (c.res or c.bias)
    if c.entry == "u3d_conv_wgrad_ring":
        return bf and c.k == 3 and c.stride == 1 and min(h, w) >= ops.RING_WGRAD_MIN_HW
    if c.entry == "u3d_conv_wgrad_brick":
        return bf and c.k == 3 and c.cin % 8 == 0 and c.cout % 8 == 0
    if c.entry == "u3d_conv_wgrad1":
        return bf and c.k == 1 and c.cin % 8 == 0 and c.cout % 8 == 0
    if c.entry == "u3d_conv_wgrad":
        return c.cin % 8 == 0 and c.cout % 8 == 0 and c.slabs >= 1 and (not c.gn or c.cin <= 256)
    return False


def _production_route(c):
    from u3d import ops
    n, (d, h, w) = c.n, c.dims
    shape = (n, d, h, w)
    if c.dir == "wgrad":
        x = torch.empty((n, d, h, w, c.cin), dtype=c.dt, device="meta")
        dy = torch.empty((n,) + cc.out_dims(c) + (c.cout,), dtype=c.dt, device="meta")
        r = ops.wgrad_route(dy, x, c.k, c.stride)
        return {"ring": "wgrad_ring", "brick": "wgrad1" if c.k == 1 else "wgrad_brick", "gemm": "wgrad_gemm"}[r]
    el = 2 if c.dt == BF else 4
    if c.dir == "fwd":
        return ops.conv_route(c.dt, c.cin, c.cout, c.k, c.stride, shape, n * d * h * w * c.cin * el, False,
                              True if c.res else None, True if c.bias else None, c.out_f32)
    od = cc.out_dims(c)
    return ops.conv_route(c.dt, c.cout, c.cin, c.k, c.stride, shape, n * od[0] * od[1] * od[2] * c.cout * el, True)


FORCED_FORMS = ("u3d_conv_s2_ring", "u3d_conv32_ring_q", "u3d_conv_small", "u3d_conv32_brick")


@pytest.mark.parametrize("c", cc.CASES, ids=cc.case_id)
def test_case_is_inside_its_kernels_contract_and_marked_right(c):
    assert c.cin % cc.groups(c.cin) == 0
    assert _predicate(c), "the row lies outside its kernel's contract"
    if c.entry in FORCED_FORMS or c.mode == "target" or cc.forced_by_opts(c.opts):   # another schedule of a family the route names: reached through a flag only
        assert not c.routed
    else:
        assert (_production_route(c) == c.family) == c.routed, (_production_route(c), c.family, c.routed)
    if c.dims == (64, 64, 64):                               # the 256-row M tile's condition (conv.hip:807)
        od = cc.out_dims(c)
        assert -(-od[0] * od[1] * od[2] // 256) * -(-c.cout // 64) * c.n >= 256
    else:
        assert c.n * c.dims[0] * c.dims[1] * c.dims[2] * max(c.cin, c.cout) <= 2 * 64 ** 3 * 32


def _cpu_operands(c):
    """The row's operands on the CPU: the weights standardised by the oracle and rounded to the row's dtype (the GPU
    test decodes the kernel's own pack instead), the statistics exact and rounded to fp32."""
    I = cc.make_inputs(c)
    wq = O.ws_weight(I["w"]).to(c.dt).double()
    if not c.gn:
        return I, wq, I["x"].double(), None, None
    G = cc.groups(c.cin)
    a, mask, delta = cr.prologue_ref(I["x"], exact_stats(I["x"], G)[0].float(), I["gamma"], I["beta"], G, c.dt)
    return I, wq, a, mask, delta


@pytest.mark.parametrize("c", cc.CASES, ids=cc.case_id)
def test_case_conditions(c):
    I, wq, a, mask, delta = _cpu_operands(c)
    again = cc.make_inputs(c)
    assert all(torch.equal(I[k], again[k]) for k in I)                  # seeded CPU generators: the same bits
    if mask is not None:
        share = mask.double().mean().item()
        assert share <= cr.MAX_AMBIGUOUS, share
    if c.dir == "fwd":
        out = cr.conv_fwd_ref(a, wq, c.k, c.stride, I["res"].double() if c.res else None,
                              I["bias"].double() if c.bias else None, a_delta=delta)
        L = cc.chain_len(c, max(1, c.slabs))
    elif c.dir == "dgrad":
        out = cr.conv_dgrad_ref(I["dy"].double(), wq, (c.n,) + c.dims, c.k, c.stride)
        L = cc.chain_len(c, max(1, c.slabs))
    else:
        out = cr.conv_wgrad_ref(a, I["dy"].double(), c.k, c.stride, a_delta=delta)
        L = cc.wgrad_slab_terms(c, max(1, c.slabs))
    ref, S = out[0], out[1]
    out_bf = c.dt == BF and not c.out_f32 and c.dir != "wgrad"
    bound = cr.bound_store(ref, BF if out_bf else F32) + cr.bound_accum(S, L) + (out[2] if len(out) > 2 else 0)
    assert L >= 1 and torch.isfinite(bound).all()
    assert not bool(((bound == 0) & (ref != 0)).any())
    assert bool((S >= ref.abs() * (1 - 1e-9)).all())
