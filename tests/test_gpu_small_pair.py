"""The 12^3 / 6^3 backward pair (u3d_conv_small_bwd_pair, ops.conv_bwd_pair_small): the data gradient of
conv(relu(gn(x))) with its GroupNorm-backward partials and finalize, and the same conv's weight gradient, as two
sub-grids of one launch. Both halves run the bodies of the separate kernels with the same geometry and split counts, so
every output is BITWISE what ops.conv_wgrad + ops.conv_dgrad_gn write; the tests hold it to that, to an fp64 reference
(which would catch both forms being wrong alike), under graph replay, and in a whole training step.
Reference: autograd of NoBottleneck's relu(gn(x)) -> conv3x3x3 (unet3D.py:44-73)."""
import pytest
import torch

pytestmark = pytest.mark.gpu

SHAPES = [  # n, d, h, w, cin (x, dA), cout (dy), groups, x offset
    (2, 12, 12, 12, 256, 256, 16, 0.0),   # the main 12^3 case
    (2, 12, 12, 12, 256, 128, 16, 0.0),   # cin != cout, as in x8_resb.0.conv1
    (2, 12, 12, 12, 128, 128, 16, 0.0),   # 16 weight-gradient tiles x 16 splits
    (2, 6, 6, 6, 256, 256, 16, 0.0),      # the 6^3 case (brick weight gradient)
    (1, 12, 12, 12, 256, 256, 16, 30.0),  # n = 1, |mean| / std ~ 40
    (2, 6, 6, 6, 128, 256, 16, 0.0),      # brick path with cin != cout
]
_ids = lambda c: "x".join(map(str, c[:4])) + f"_c{c[4]}-{c[5]}_g{c[6]}_o{c[7]:g}"  # noqa: E731
_CACHE = {}


def _setup(gpu, n, d, h, w, cin, cout, groups, off):
    """Operands of one case (made once, never written): x, dy, the forward / data-gradient packs, the GroupNorm."""
    key = (n, d, h, w, cin, cout, groups, off)
    if key not in _CACHE:
        from u3d import ops
        torch.manual_seed(7)
        x = (torch.randn((n, d, h, w, cin), device=gpu) * 0.8 + 0.2 + off).to(torch.bfloat16)
        dy = (torch.randn((n, d, h, w, cout), device=gpu) * 0.3).to(torch.bfloat16)
        wt = torch.randn((cout, cin, 3, 3, 3), device=gpu) * 0.05
        (pf, pd, st), = ops.wstd_fwd_batch([(wt, True, True)], torch.bfloat16)
        if n * cin <= 2048:
            st = ops.gn_stats(x, groups)
        else:  # (past u3d_gn_stats' n * c limit: the same (mean, rstd) table from torch)
            xg = x.double().reshape(n, -1, groups, cin // groups).permute(0, 2, 1, 3).reshape(n, groups, -1)
            st = torch.stack((xg.mean(-1), (xg.var(-1, unbiased=False) + 1e-5).rsqrt()), -1).float().contiguous()
        gn = (st, 1 + 0.1 * torch.randn(cin, device=gpu), 0.1 * torch.randn(cin, device=gpu), groups)
        _CACHE[key] = (x, dy, pf, pd, gn)
    return _CACHE[key]


def _poison(gpu, x, dy, ns=32):
    """NaN where the next launches' outputs and scratch will be: the split-K slabs and the GroupNorm-backward partial
    rows (workspaces), and freshly freed blocks of the output sizes (torch.empty takes the caching allocator's last
    freed block of a size). The arrival counters stay zero."""
    from u3d import ops
    n, d, h, w, cin = x.shape
    cout = dy.shape[-1]
    for slot in (4, ops.SMALL_GB_SLOT):
        b = ops.WS.buf.get((gpu, slot))
        if b is not None:
            b.fill_(0xFF)  # fp32 NaN
    junk = [torch.full((n, d, h, w, cin), float("nan"), dtype=torch.bfloat16, device=gpu),
            torch.full((n, 5, cin), float("nan"), device=gpu),
            torch.full((ns, 27, ops.round32(cout), ops.round32(cin)), float("nan"), device=gpu)]
    del junk


def _separate(gpu, x, dy, pd, gn):
    from u3d import ops
    cin = x.shape[-1]
    dg, db = torch.full((cin,), 7.0, device=gpu), torch.full((cin,), 7.0, device=gpu)
    on = ops.SMALL_BWD_PAIR
    ops.SMALL_BWD_PAIR = False
    try:
        part, ns = ops.conv_wgrad(dy, x, 3, 1, gn)
        _poison(gpu, x, dy, ns)
        part, ns = ops.conv_wgrad(dy, x, 3, 1, gn)
        r = ops.conv_dgrad_gn(dy, pd, cin, x, 3, 1, gn, dgb=lambda: (dg, db))
    finally:
        ops.SMALL_BWD_PAIR = on
    assert r is not None and isinstance(r[1], tuple) and r[1][0] == "coef", "the fused small data gradient did not run"
    return part, ns, r[0], r[1][1], dg, db


def _paired(gpu, x, dy, pd, gn, ns):
    from u3d import ops
    cin = x.shape[-1]
    dg, db = torch.full((cin,), 7.0, device=gpu), torch.full((cin,), 7.0, device=gpu)
    _poison(gpu, x, dy, ns)
    on = ops.SMALL_BWD_PAIR
    ops.SMALL_BWD_PAIR = True
    try:
        r = ops.conv_bwd_pair_small(dy, pd, x, 3, 1, gn, dgb=lambda: (dg, db))
    finally:
        ops.SMALL_BWD_PAIR = on
    assert r is not None, "the pair declined"
    part, ns2, da, parts = r
    assert parts[0] == "coef"
    return part, ns2, da, parts[1], dg, db


@pytest.mark.parametrize("case", SHAPES, ids=_ids)
def test_pair_bitwise_separate(gpu, case):
    x, dy, _, pd, gn = _setup(gpu, *case)
    sep = _separate(gpu, x, dy, pd, gn)
    runs = [_paired(gpu, x, dy, pd, gn, sep[1]) for _ in range(2)]
    torch.cuda.synchronize()
    names = ("slabs", "ns", "dA", "coef", "dgamma", "dbeta")
    for got in runs:
        assert got[1] == sep[1], f"ns {got[1]} vs {sep[1]}"
        assert tuple(got[0].shape) == tuple(sep[0].shape)
        for nm, a, b in zip(names, got, sep):
            if nm != "ns":
                assert not torch.isnan(a.float()).any(), f"{nm}: NaN left"
                assert torch.equal(a, b), f"{nm}: pair differs from the separate launches"
    for nm, a, b in zip(names, runs[0], runs[1]):
        if nm != "ns":
            assert torch.equal(a, b), f"{nm}: second run differs (arrival counters not left at zero?)"


def _declined(gpu, case):
    """The pair returns None without asking for the dgamma / dbeta destinations; the separate path still works."""
    from u3d import ops
    x, dy, _, pd, gn = _setup(gpu, *case)
    asked = []
    assert ops.conv_bwd_pair_small(dy, pd, x, 3, 1, gn, dgb=lambda: asked.append(1)) is None
    assert not asked
    n, d, h, w, cin = x.shape
    part, ns = ops.conv_wgrad(dy, x, 3, 1, gn)
    da = ops.conv_dgrad(dy, pd, cin, (n, d, h, w), 3, 1)
    torch.cuda.synchronize()
    assert ns >= 1 and torch.isfinite(part).all() and torch.isfinite(da.float()).all()
    return x, dy, pd, gn


def test_pair_declines_dma_ring_shape(gpu):
    """8-wide planes: the weight gradient is the 16 x 16 LDS-DMA ring, not one of the pair's two kernels."""
    from u3d import ops
    x, dy, pd, gn = _declined(gpu, (3, 8, 8, 8, 64, 64, 8, 0.0))
    cin = x.shape[-1]
    dg, db = torch.full((cin,), 7.0, device=gpu), torch.full((cin,), 7.0, device=gpu)
    r = ops.conv_dgrad_gn(dy, pd, cin, x, 3, 1, gn, dgb=lambda: (dg, db))  # the fused data gradient alone still runs
    assert r is not None and r[1][0] == "coef" and not (dg == 7.0).any()


def test_pair_declines_finalize_limit(gpu):
    """n * cin * 2 > 8192: the data gradient's in-launch finalize does not fit its LDS table."""
    _declined(gpu, (17, 2, 2, 2, 256, 32, 16, 0.0))


def test_pair_declines_collective_in_flight(gpu):
    from u3d import ops
    assert not ops.COLLECTIVE_IN_FLIGHT[0]
    ops.COLLECTIVE_IN_FLIGHT[0] = True
    try:
        _declined(gpu, SHAPES[0])
    finally:
        ops.COLLECTIVE_IN_FLIGHT[0] = False
    x, dy, _, pd, gn = _setup(gpu, *SHAPES[0])
    assert _paired(gpu, x, dy, pd, gn, 1) is not None  # and runs again once the latch is clear


def _fp64_backward(x, dy, pf, gn):
    """fp64 dA [n, d, h, w, cin] and dW [27, cout, cin] of y = conv3x3x3(A), A = bf16(relu(gn(x))) as the kernels'
    prologue forms it, from the bf16-rounded operands: 27 shifted fp64 matrix products on the device."""
    st, ga, be, G = gn
    n, d, h, w, cin = x.shape
    cout = dy.shape[-1]
    grp = torch.arange(cin, device=x.device) // (cin // G)
    sc = st[:, grp, 1] * ga[None]
    sh = be[None] - st[:, grp, 0] * sc
    a = torch.clamp_min(torch.addcmul(sh.view(n, 1, 1, 1, cin), x.float(), sc.view(n, 1, 1, 1, cin)), 0)
    a = a.to(torch.bfloat16).double()
    apad = torch.zeros((n, d + 2, h + 2, w + 2, cin), dtype=torch.float64, device=x.device)
    apad[:, 1:-1, 1:-1, 1:-1] = a
    dapad = torch.zeros_like(apad)
    dy2 = dy.double().reshape(-1, cout)
    wq = pf[:, :cout, :cin].double()  # [27][cout][cin], tap t = (td * 3 + th) * 3 + tw
    dw = torch.empty((27, cout, cin), dtype=torch.float64, device=x.device)
    for t in range(27):
        td, th, tw = t // 9, (t // 3) % 3, t % 3
        win = (slice(None), slice(td, td + d), slice(th, th + h), slice(tw, tw + w))
        dw[t] = dy2.t() @ apad[win].reshape(-1, cin)
        dapad[win] += (dy2 @ wq[t]).view(n, d, h, w, cin)
    return dapad[:, 1:-1, 1:-1, 1:-1], dw


@pytest.mark.parametrize("case", [SHAPES[0], SHAPES[3]], ids=_ids)
def test_pair_against_fp64(gpu, case):
    """Tolerances of tests/test_gpu_fullsize.py for these kinds: the bf16 data gradient per (sample, d) plane
    max |err| <= 1e-2 x the plane's max and rel L2 <= 4e-3; the fp32 weight gradient max |err| <= 2e-3 x max |dW| and
    rel L2 <= 1e-3."""
    x, dy, pf, pd, gn = _setup(gpu, *case)
    cin, cout = x.shape[-1], dy.shape[-1]
    part, ns, da, _, _, _ = _paired(gpu, x, dy, pd, gn, 32)
    ref_da, ref_dw = _fp64_backward(x, dy, pf, gn)
    got = da.double()
    err = (got - ref_da).abs().amax(dim=(2, 3, 4))
    scale = ref_da.abs().amax(dim=(2, 3, 4)).clamp_min(1e-30)
    worst, rel2 = (err / scale).max().item(), ((got - ref_da).norm() / ref_da.norm()).item()
    print(f"dA: worst plane {worst:.3e}, rel L2 {rel2:.3e}")
    assert worst <= 1e-2, f"dA: worst plane max-err / plane max = {worst:.3e}"
    assert rel2 <= 4e-3, f"dA: relative L2 {rel2:.3e}"
    dw = part.double().sum(0)[:, :cout, :cin]
    emax = ((dw - ref_dw).abs().max() / ref_dw.abs().max()).item()
    el2 = ((dw - ref_dw).norm() / ref_dw.norm()).item()
    print(f"dW: max {emax:.3e}, rel L2 {el2:.3e}")
    assert emax <= 2e-3, f"dW: max |err| / max |dW| = {emax:.3e}"
    assert el2 <= 1e-3, f"dW: relative L2 {el2:.3e}"


def test_pair_graph_replay(gpu):
    """One captured pair launch replayed three times on NaN-refilled outputs: each replay bitwise the eager result."""
    from u3d import ops
    x, dy, _, pd, gn = _setup(gpu, *SHAPES[0])
    cin = x.shape[-1]
    eager = _paired(gpu, x, dy, pd, gn, 32)  # (also sizes every workspace before the capture)
    dg, db = torch.full((cin,), 7.0, device=gpu), torch.full((cin,), 7.0, device=gpu)
    torch.cuda.synchronize()
    g = torch.cuda.CUDAGraph()
    with torch.cuda.graph(g):
        r = ops.conv_bwd_pair_small(dy, pd, x, 3, 1, gn, dgb=lambda: (dg, db))
    assert r is not None
    part, ns, da, (_, coef) = r
    assert ns == eager[1]
    for _ in range(3):
        for t in (part, da, coef):
            t.fill_(float("nan"))
        dg.fill_(7.0)
        db.fill_(7.0)
        g.replay()
        torch.cuda.synchronize()
        for nm, a, b in zip(("slabs", "dA", "coef", "dgamma", "dbeta"), (part, da, coef, dg, db),
                            (eager[0], eager[2], eager[3], eager[4], eager[5])):
            assert torch.equal(a, b), f"{nm}: replay differs from the eager launch"


def test_pair_whole_step(gpu):
    """unet3D_baseline at 2 x 1 x 48^3 under bf16 autocast (12^3 at 128 channels, 6^3 at 256): loss and every
    parameter gradient identical with the pair on and off, and the pair ran."""
    import unet3D
    from loss_functions.loss_partial import EDiceLoss_partial
    from u3d import ops

    torch.manual_seed(3)
    m = unet3D.unet3D_baseline([1, 2, 2, 2, 2], num_classes=16, weight_std=True).to(gpu).train()
    crit = EDiceLoss_partial(16)
    gen = torch.Generator().manual_seed(11)
    x = (torch.rand((2, 1, 48, 48, 48), generator=gen) * 2 - 1).to(gpu)
    lab = torch.randint(0, 16, (2, 48, 48, 48), generator=gen).float().to(gpu)
    mask = (torch.rand(16, generator=gen) < 0.7).long().to(gpu)

    def step(on):
        for p in m.parameters():
            p.grad = None
        keep = ops.SMALL_BWD_PAIR
        ops.SMALL_BWD_PAIR = on
        calls0 = ops.PAIR_CALLS[0]
        try:
            with torch.autocast("cuda", dtype=torch.bfloat16):
                lg, _, _ = m(x)
            loss = crit(lg, lab, mask=[mask])
            loss.backward()
        finally:
            ops.SMALL_BWD_PAIR = keep
        torch.cuda.synchronize()
        return loss.detach().clone(), {k: p.grad.clone() for k, p in m.named_parameters() if p.grad is not None}, \
            ops.PAIR_CALLS[0] - calls0

    loss1, g1, c1 = step(True)
    loss0, g0, c0 = step(False)
    assert c0 == 0 and c1 >= 6, f"pair launches: {c1} with the switch on, {c0} off"
    assert torch.equal(loss1, loss0)
    assert g1.keys() == g0.keys() and len(g1) > 0
    for k in g1:
        assert torch.equal(g1[k], g0[k]), f"{k}: gradient differs between the pair and the separate launches"
