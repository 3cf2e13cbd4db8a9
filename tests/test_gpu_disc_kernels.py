"""The discriminator kernels (csrc/disc.hip), entry point by entry point, against the fp64 restatement
tests/disc_reference.py on the same (bf16-rounded, in bf16 mode) operands: the project's bf16 convention, DESIGN §5.

Bounds: bf16 outputs max error <= 1e-2 max|y| and rel L2 <= 4e-3 per sample; weight / bias
gradients entry-wise <= 2e-3 max|dW| and rel L2 <= 1e-3; fp32 mode rel L2 <= 1e-5 (outputs), 1e-4 (weight gradients).
Shapes: the smallest at which each mechanism can go wrong (odd dims, taps in the padding, several workgroups, K-split).
"""
import math

import pytest
import torch
import torch.nn.functional as F

import disc_reference as DR

pytestmark = pytest.mark.gpu

DTYPES = [torch.bfloat16, torch.float32]
# (n, cin, cout, input dims)
CONV_CASES = [
    (2, 32, 64, (6, 10, 12)),
    (1, 64, 64, (5, 9, 7)),      # odd dims: the last plane is reached by tap 3 only
    (3, 32, 32, (2, 2, 2)),      # -> 1^3: nearly every tap in the padding
    (2, 64, 64, (8, 16, 16)),    # several workgroups per sample, several partial-sum blocks
    (2, 128, 128, (4, 4, 4)),    # K-split, the driver's tail
    (2, 256, 256, (4, 4, 4)),
    (2, 256, 256, (2, 6, 6)),    # -> 1 x 3 x 3, K = 16384
]
_CACHE = {}


def rnd(t, dtype):
    """fp64 tensor holding values representable in dtype."""
    return t.to(dtype).double()


def nd(t):
    return t.permute(0, 2, 3, 4, 1).contiguous()


def ncdhw(t):
    return t.permute(0, 4, 1, 2, 3)


def conv_ref(n, cin, cout, dims, dtype):
    """fp64 reference of one inner conv layer, forward and backward, computed once per case."""
    key = ("conv", n, cin, cout, dims, dtype)
    if key in _CACHE:
        return _CACHE[key]
    g = torch.Generator().manual_seed(1000 + cin + cout + sum(dims))
    x = rnd(torch.randn((n, cin) + dims, generator=g, dtype=torch.float64), dtype).requires_grad_(True)
    w = rnd(torch.randn((cout, cin, 4, 4, 4), generator=g, dtype=torch.float64) * math.sqrt(2 / (1.04 * cin * 64)),
            dtype).requires_grad_(True)
    b = (0.1 * torch.randn(cout, generator=g)).double()
    pre = F.conv3d(x, w, b, stride=2, padding=1)
    y = F.leaky_relu(pre, DR.SLOPE).detach()
    ys = rnd(y, dtype)                      # the stored output the backward reads
    ys.view(-1)[::7] = 0.0                  # y exactly 0 takes the slope
    dy = rnd(torch.randn(y.shape, generator=g, dtype=torch.float64), dtype)
    gg = DR.lrelu_grad(dy, ys)
    (pre * gg).sum().backward()
    r = dict(x=x.detach(), w=w.detach(), b=b, y=y, ys=ys, dy=dy, dx=x.grad, dw=w.grad, db=gg.sum(dim=(0, 2, 3, 4)))
    _CACHE[key] = r
    return r


def check_out(got, want, dtype, what):
    """got / want NCDHW-shaped (sample first); the bf16 / fp32 output bounds, per sample."""
    got, want = got.double().cpu(), want.double()
    for s in range(want.shape[0]):
        e = got[s] - want[s]
        rel = (e.norm() / want[s].norm().clamp_min(1e-30)).item()
        mx = (e.abs().max() / want[s].abs().max().clamp_min(1e-30)).item()
        print(f"{what} sample {s}: rel L2 {rel:.3e}, max err / max {mx:.3e}")
        if dtype == torch.bfloat16:
            assert mx <= 1e-2 and rel <= 4e-3, (what, s, rel, mx)
        else:
            assert rel <= 1e-5, (what, s, rel)


def check_wgrad(got, want, dtype, what):
    got, want = got.double().cpu(), want.double()
    e = got - want
    rel = (e.norm() / want.norm().clamp_min(1e-30)).item()
    mx = (e.abs().max() / want.abs().max().clamp_min(1e-30)).item()
    print(f"{what}: rel L2 {rel:.3e}, max err / max {mx:.3e}")
    if dtype == torch.bfloat16:
        assert mx <= 2e-3 and rel <= 1e-3, (what, rel, mx)
    else:
        assert rel <= 1e-4, (what, rel)


def dev(t, dtype, gpu):
    return t.to(dtype).to(gpu).contiguous()


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: f"n{c[0]}_{c[1]}to{c[2]}_{'x'.join(map(str, c[3]))}")
def test_conv_forward(gpu, case, dtype):
    from u3d import disc
    n, cin, cout, dims = case
    r = conv_ref(n, cin, cout, dims, dtype)
    x = dev(nd(r["x"]), dtype, gpu)
    y = torch.empty((n, *[v // 2 for v in dims], cout), dtype=dtype, device=gpu)
    disc.conv_fwd(disc.View(x, 0, cin), disc.pack_conv_fwd(dev(r["w"], torch.float32, gpu), dtype),
                  dev(r["b"], torch.float32, gpu), disc.View(y, 0, cout))
    check_out(ncdhw(y), r["y"], dtype, "conv_fwd")


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: f"n{c[0]}_{c[1]}to{c[2]}_{'x'.join(map(str, c[3]))}")
def test_conv_backward(gpu, case, dtype):
    """Data gradient with the LeakyReLU mask from the stored y (zeros included), weight and bias gradients, and the
    parameter gradients bitwise equal across two runs."""
    from u3d import disc
    n, cin, cout, dims = case
    r = conv_ref(n, cin, cout, dims, dtype)
    x, ys, dy = (dev(nd(r[k]), dtype, gpu) for k in ("x", "ys", "dy"))
    xv, yv, dyv = disc.View(x, 0, cin), disc.View(ys, 0, cout), disc.View(dy, 0, cout)
    dx = torch.full_like(x, float("nan"))
    disc.conv_dgrad(dyv, yv, disc.pack_conv_dgrad(dev(r["w"], torch.float32, gpu), dtype), disc.View(dx, 0, cin))
    check_out(ncdhw(dx), r["dx"], dtype, "conv_dgrad")
    runs = []
    for _ in range(2):
        dw = torch.full((cout, cin, 4, 4, 4), float("nan"), device=gpu)
        db = torch.full((cout,), float("nan"), device=gpu)
        disc.conv_wgrad(xv, dyv, yv, dw)
        disc.bias_grad(dyv, yv, db)
        runs.append((dw, db))
    check_wgrad(runs[0][0], r["dw"], dtype, "conv_wgrad")
    check_wgrad(runs[0][1], r["db"], dtype, "bias_grad")
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
def test_channel_offset_and_pitch(gpu, dtype):
    """The forward writes the upper half of a 2C buffer whose lower half holds a sentinel; the backward reads dy / y
    from upper halves, reads x from a lower half and writes dx into a lower half: the sentinels survive."""
    from u3d import disc
    n, cin, cout, dims = CONV_CASES[0]
    r = conv_ref(n, cin, cout, dims, dtype)
    S = 77.0
    w32 = dev(r["w"], torch.float32, gpu)
    xbuf = torch.full((n, *dims, 2 * cin), S, dtype=dtype, device=gpu)
    xbuf[..., :cin] = dev(nd(r["x"]), dtype, gpu)
    odims = [v // 2 for v in dims]
    ybuf = torch.full((n, *odims, 2 * cout), S, dtype=dtype, device=gpu)
    disc.conv_fwd(disc.View(xbuf, 0, cin), disc.pack_conv_fwd(w32, dtype), dev(r["b"], torch.float32, gpu),
                  disc.View(ybuf, cout, cout))
    assert bool((ybuf[..., :cout] == S).all())
    check_out(ncdhw(ybuf[..., cout:]), r["y"], dtype, "conv_fwd upper half")
    ybuf[..., cout:] = dev(nd(r["ys"]), dtype, gpu)
    dybuf = torch.full_like(ybuf, S)
    dybuf[..., cout:] = dev(nd(r["dy"]), dtype, gpu)
    dxbuf = torch.full((n, *dims, 2 * cin), S, dtype=dtype, device=gpu)
    yv, dyv = disc.View(ybuf, cout, cout), disc.View(dybuf, cout, cout)
    disc.conv_dgrad(dyv, yv, disc.pack_conv_dgrad(w32, dtype), disc.View(dxbuf, 0, cin))
    assert bool((dxbuf[..., cin:] == S).all())
    check_out(ncdhw(dxbuf[..., :cin]), r["dx"], dtype, "conv_dgrad lower half")
    dw = torch.empty((cout, cin, 4, 4, 4), device=gpu)
    db = torch.empty((cout,), device=gpu)
    disc.conv_wgrad(disc.View(xbuf, 0, cin), dyv, yv, dw)
    disc.bias_grad(dyv, yv, db)
    check_wgrad(dw, r["dw"], dtype, "conv_wgrad from views")
    check_wgrad(db, r["db"], dtype, "bias_grad from views")


def first_ref(C, dims, dtype):
    key = ("first", C, dims, dtype)
    if key in _CACHE:
        return _CACHE[key]
    n, cout = 2, 32
    g = torch.Generator().manual_seed(2000 + C + sum(dims))
    x = torch.randn((n, C) + dims, generator=g).double().requires_grad_(True)         # fp32 input, read as is
    w = (torch.randn((cout, C, 4, 4, 4), generator=g) * math.sqrt(2 / (1.04 * C * 64))).double().requires_grad_(True)
    b = (0.1 * torch.randn(cout, generator=g)).double()
    pre = F.conv3d(x, w, b, stride=2, padding=1)
    y = F.leaky_relu(pre, DR.SLOPE).detach()
    ys = rnd(y, dtype)
    ys.view(-1)[::5] = 0.0
    dy = rnd(torch.randn(y.shape, generator=g, dtype=torch.float64), dtype)
    gg = DR.lrelu_grad(dy, ys)
    (pre * gg).sum().backward()
    r = dict(x=x.detach(), w=w.detach(), b=b, y=y, ys=ys, dy=dy, dx=x.grad, dw=w.grad, db=gg.sum(dim=(0, 2, 3, 4)))
    _CACHE[key] = r
    return r


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("dims", [(6, 8, 10), (5, 7, 9)], ids=["6x8x10", "5x7x9"])
@pytest.mark.parametrize("C", [1, 2, 4])
def test_first_layer(gpu, C, dims, dtype):
    from u3d import disc
    r = first_ref(C, dims, dtype)
    n, cout = 2, 32
    x = dev(r["x"], torch.float32, gpu)
    w32 = dev(r["w"], torch.float32, gpu)
    w1 = disc.pack_first(w32)
    S = 55.0
    ybuf = torch.full((n, *[v // 2 for v in dims], 2 * cout), S, dtype=dtype, device=gpu)
    disc.first_fwd(x, w1, dev(r["b"], torch.float32, gpu), disc.View(ybuf, 0, cout))
    assert bool((ybuf[..., cout:] == S).all())
    check_out(ncdhw(ybuf[..., :cout]), r["y"], dtype, "first_fwd")
    ys, dy = dev(nd(r["ys"]), dtype, gpu), dev(nd(r["dy"]), dtype, gpu)
    yv, dyv = disc.View(ys, 0, cout), disc.View(dy, 0, cout)
    dx = torch.full_like(x, float("nan"))
    disc.first_dgrad(dyv, yv, w1, dx)
    check_out(dx, r["dx"], dtype, "first_dgrad")
    runs = []
    for _ in range(2):
        dw = torch.full((cout, C, 4, 4, 4), float("nan"), device=gpu)
        db = torch.full((cout,), float("nan"), device=gpu)
        disc.first_wgrad(x, dyv, yv, dw)
        disc.bias_grad(dyv, yv, db)
        runs.append((dw, db))
    check_wgrad(runs[0][0], r["dw"], dtype, "first_wgrad")
    check_wgrad(runs[0][1], r["db"], dtype, "first bias_grad")
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def side_ref(C, dims, dtype):
    key = ("side", C, dims, dtype)
    if key in _CACHE:
        return _CACHE[key]
    n = 2
    g = torch.Generator().manual_seed(3000 + C + sum(dims))
    f = torch.randn((n, 1) + dims, generator=g).double().requires_grad_(True)
    w = (torch.randn((C, 1, 3, 3, 3), generator=g) * math.sqrt(2 / (1.04 * 27))).double().requires_grad_(True)
    b = (0.1 * torch.randn(C, generator=g)).double()
    pre = F.conv3d(f, w, b, stride=1, padding=1)
    y = F.leaky_relu(pre, DR.SLOPE).detach()
    ys = rnd(y, dtype)
    ys.view(-1)[::5] = 0.0
    dy = rnd(torch.randn(y.shape, generator=g, dtype=torch.float64), dtype)
    gg = DR.lrelu_grad(dy, ys)
    (pre * gg).sum().backward()
    r = dict(f=f.detach(), w=w.detach(), b=b, y=y, ys=ys, dy=dy, df=f.grad, dw=w.grad, db=gg.sum(dim=(0, 2, 3, 4)))
    _CACHE[key] = r
    return r


@pytest.mark.parametrize("dtype", DTYPES, ids=["bf16", "fp32"])
@pytest.mark.parametrize("dims", [(3, 5, 7), (8, 8, 8)], ids=["3x5x7", "8x8x8"])
@pytest.mark.parametrize("C", [32, 128])
def test_side_conv(gpu, C, dims, dtype):
    """Forward into the upper channel half of the shared buffer (the lower half's sentinel survives), data gradient to
    the one-channel map, weight and bias gradients from the upper half of a gradient buffer."""
    from u3d import disc
    r = side_ref(C, dims, dtype)
    n = 2
    f = dev(r["f"], torch.float32, gpu)
    wsd = disc.pack_side(dev(r["w"], torch.float32, gpu))
    S = 33.0
    ybuf = torch.full((n, *dims, 2 * C), S, dtype=dtype, device=gpu)
    disc.side_fwd(f, wsd, dev(r["b"], torch.float32, gpu), disc.View(ybuf, C, C))
    assert bool((ybuf[..., :C] == S).all())
    check_out(ncdhw(ybuf[..., C:]), r["y"], dtype, "side_fwd")
    ybuf[..., C:] = dev(nd(r["ys"]), dtype, gpu)
    dybuf = torch.full_like(ybuf, S)
    dybuf[..., C:] = dev(nd(r["dy"]), dtype, gpu)
    yv, dyv = disc.View(ybuf, C, C), disc.View(dybuf, C, C)
    df = torch.full_like(f, float("nan"))
    disc.side_dgrad(dyv, yv, wsd, df)
    check_out(df, r["df"], dtype, "side_dgrad")
    runs = []
    for _ in range(2):
        dw = torch.full((C, 1, 3, 3, 3), float("nan"), device=gpu)
        db = torch.full((C,), float("nan"), device=gpu)
        disc.side_wgrad(f, dyv, yv, dw)
        disc.bias_grad(dyv, yv, db)
        runs.append((dw, db))
    check_wgrad(runs[0][0], r["dw"], dtype, "side_wgrad")
    check_wgrad(runs[0][1], r["db"], dtype, "side bias_grad")
    assert torch.equal(runs[0][0], runs[1][0]) and torch.equal(runs[0][1], runs[1][1])


def test_bad_views_and_sizes_raise(gpu):
    from u3d import U3DError, disc
    x = torch.zeros((1, 2, 2, 2, 48), dtype=torch.bfloat16, device=gpu)
    y = torch.zeros((1, 1, 1, 1, 32), dtype=torch.bfloat16, device=gpu)
    w = torch.zeros((64, 4, 32, 8), dtype=torch.bfloat16, device=gpu)
    b = torch.zeros(32, device=gpu)
    with pytest.raises(U3DError, match="multiples of 32"):
        disc.conv_fwd(disc.View(x, 0, 48), w, b, disc.View(y, 0, 32))
    x = torch.zeros((1, 1, 2, 2, 32), dtype=torch.bfloat16, device=gpu)
    with pytest.raises(U3DError, match=">= 2"):
        disc.conv_fwd(disc.View(x, 0, 32), w, b, disc.View(y, 0, 32))
