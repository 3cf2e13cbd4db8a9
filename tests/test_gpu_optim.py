"""u3d.optim.SGD (one fused launch per 48 tensors) against torch.optim.SGD: same update rule, momentum buffer
initialisation, weight decay, nesterov/dampening/maximize variants, LR changes between steps, state_dict keys."""
import pytest
import torch

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("kw", [dict(momentum=0.9, weight_decay=1e-4), dict(momentum=0.0),
                                dict(momentum=0.8, dampening=0.1, weight_decay=1e-3),
                                dict(momentum=0.9, nesterov=True), dict(momentum=0.5, maximize=True)])
def test_sgd_matches_torch(gpu, kw):
    from u3d.optim import SGD
    torch.manual_seed(0)
    shapes = [(32, 1, 3, 3, 3), (32,), (7,), (256, 256, 3, 3, 3), (5, 3)] + [(3,)] * 60   # > 48 tensors
    pa = [torch.randn(s, device=gpu) for s in shapes]
    pb = [p.clone() for p in pa]
    pa = [torch.nn.Parameter(p) for p in pa]
    pb = [torch.nn.Parameter(p) for p in pb]
    oa = torch.optim.SGD(pa, lr=0.05, **kw)
    ob = SGD(pb, lr=0.05, **kw)
    for it in range(4):
        for a, b in zip(pa, pb):
            g = torch.randn_like(a)
            a.grad, b.grad = g.clone(), g.clone()
        if it == 2:
            oa.param_groups[0]["lr"] = ob.param_groups[0]["lr"] = 0.01
        oa.step()
        ob.step()
    for a, b in zip(pa, pb):
        torch.testing.assert_close(b, a, rtol=1e-5, atol=1e-6)
    sa, sb = oa.state_dict()["state"], ob.state_dict()["state"]
    assert set(sa) == set(sb) and all(set(sa[k]) == set(sb[k]) for k in sa)


# ---------------------------------------------------------------------------------------------------------------------
# sgd_kernel step by step against the fp64 restatement of torch.optim.SGD's rule (ws_reference.sgd_ref). Each step is
# compared with the reference started from the kernel's OWN previous p and buf, so errors do not compound. With
# u = 2^-24, D = |g| + wd |p| and Bn = momentum |buf| + |1 - dampening| D (buf = 0 on a parameter's first step):
#     |buf' - ref| <= 4u Bn                  |p' - ref| <= u |ref| + 8u lr ((1 + momentum) Bn + D)
# (worst-case counts of the kernel's fp32 roundings: three fused multiply-adds and one product on the way to buf', two
# more on the way to p'). Every check prints its worst error as a share of the bound before asserting.
KWS = [dict(momentum=0.9, weight_decay=1e-4), dict(momentum=0.0), dict(momentum=0.8, dampening=0.1, weight_decay=1e-3),
       dict(momentum=0.9, nesterov=True), dict(momentum=0.5, maximize=True)]
U = 2.0 ** -24
SENT = 31337.0


def _check_sgd_step(tag, p0, g, b0, p1, b1, lr, kw, init):
    """p0, b0: before the step (b0 None: no momentum; ignored when init); p1, b1: what the kernel left."""
    import numpy as np
    from ws_reference import f32, sgd_ref
    mom, damp, wd = (kw.get(k, 0.0) for k in ("momentum", "dampening", "weight_decay"))
    p0, g = p0.detach().double().cpu(), g.double().cpu()
    bz = torch.zeros_like(p0) if (init or b0 is None) else b0.double().cpu()
    rp, rb = sgd_ref(p0, g, bz, lr, mom, damp, wd, kw.get("nesterov", False), kw.get("maximize", False), init)
    D = g.abs() + f32(wd) * p0.abs()
    Bn = f32(mom) * bz.abs() + abs(float(np.float32(1.0) - np.float32(damp))) * D
    shares = {}
    if mom != 0:
        assert bool(torch.isfinite(b1).all()), tag
        eb, bb = (b1.double().cpu() - rb).abs(), 4 * U * Bn
        assert not bool((eb[bb == 0] != 0).any())
        shares["buf"] = (eb[bb > 0] / bb[bb > 0]).max().item() if bool((bb > 0).any()) else 0.0
    ep = (p1.detach().double().cpu() - rp).abs()
    bp = U * rp.abs() + 8 * U * f32(lr) * ((1 + f32(mom)) * Bn + D)
    assert bool(torch.isfinite(ep).all()), tag
    assert not bool((ep[bp == 0] != 0).any())
    shares["p"] = (ep[bp > 0] / bp[bp > 0]).max().item() if bool((bp > 0).any()) else 0.0
    for k, v in shares.items():
        print(f"SHARE sgd-{k} {tag} {v:.4f}")
        assert v <= 1, (tag, k, v)


@pytest.mark.parametrize("kw", KWS, ids=str)
def test_sgd_stepwise_fp64(gpu, kw):
    from u3d.optim import SGD
    torch.manual_seed(1)
    shapes = [(32, 1, 3, 3, 3), (7,), (64, 64, 3, 3, 3), (5, 3), (4 * 4 * 256 + 1,)]
    ps = [torch.nn.Parameter(torch.randn(s).to(gpu)) for s in shapes]
    opt = SGD(ps, lr=0.05, **kw)
    for it in range(3):
        if it == 2:
            opt.param_groups[0]["lr"] = 0.01
        before = [(p.detach().clone(), None if it == 0 or not kw["momentum"]
                   else opt.state[p]["momentum_buffer"].clone()) for p in ps]
        for p in ps:
            p.grad = torch.randn(p.shape).to(gpu)
        opt.step()
        torch.cuda.synchronize()
        for p, (p0, b0) in zip(ps, before):
            _check_sgd_step(f"step{it}", p0, p.grad, b0, p, opt.state[p].get("momentum_buffer"),
                            opt.param_groups[0]["lr"], kw, it == 0)


def _views(n, gpu, offs=(1, 2, 3), fill=None):
    """p, g, buf as views ``offs`` floats into flat buffers with sentinels either side."""
    out = []
    for i, off in enumerate(offs):
        flat = torch.full((n + 8,), SENT + i, device=gpu)
        v = flat[off:off + n]
        v.copy_(torch.randn(n)) if fill is None or i < 2 else v.fill_(fill)
        out.append((flat, v, off))
    return out


def _sentinels_ok(views, n):
    return all(bool((flat[:off] == SENT + i).all()) and bool((flat[off + n:] == SENT + i).all())
               for i, (flat, _, off) in enumerate(views))


LENGTHS = [1, 3, 4, 5, 7, 4099, 4 * 4 * 256 + 1]   # the last: a second block with a 1-element tail


@pytest.mark.parametrize("kw", KWS, ids=str)
def test_sgd_misaligned_views(gpu, kw):
    """p, grad and (through a pre-seeded state) momentum_buffer 1, 2 and 3 floats into flat buffers, as the DDP bucket
    views sit: the scalar branch of sgd_kernel. Same bounds; the floats either side of every view untouched."""
    from u3d.optim import SGD
    torch.manual_seed(2)
    views = [_views(n, gpu) for n in LENGTHS]
    ps = [torch.nn.Parameter(v[0][1]) for v in views]
    assert all(p.data_ptr() == v[0][1].data_ptr() and p.data_ptr() % 16 == 4 for p, v in zip(ps, views))
    opt = SGD(ps, lr=0.05, **kw)
    for p, v in zip(ps, views):
        p.grad = v[1][1]
        if kw["momentum"]:
            opt.state[p]["momentum_buffer"] = v[2][1]
    for it in range(2):
        before = [(p.detach().clone(), v[2][1].clone() if kw["momentum"] else None) for p, v in zip(ps, views)]
        opt.step()
        torch.cuda.synchronize()
        for n, p, v, (p0, b0) in zip(LENGTHS, ps, views, before):
            assert p.data_ptr() == v[0][1].data_ptr()
            if kw["momentum"]:
                assert opt.state[p]["momentum_buffer"].data_ptr() == v[2][1].data_ptr()
            _check_sgd_step(f"views n={n}", p0, v[1][1], b0, v[0][1], v[2][1] if kw["momentum"] else None, 0.05, kw,
                            False)
            assert _sentinels_ok(v if kw["momentum"] else v[:2], n), f"n={n}: a float outside a view changed"
            v[1][1].copy_(torch.randn(n))


@pytest.mark.parametrize("offs", [(1, 2, 3), (0, 0, 0), (0, 0, 1)], ids=str)
@pytest.mark.parametrize("kw", [KWS[0], KWS[2], KWS[3]], ids=str)
def test_sgd_first_step_scalar_paths(gpu, kw, offs):
    """A parameter's first step (init = 1) through the C entry point, with the momentum buffer pre-filled with NaN: on
    a first step the buffer is write-only, on the scalar branch (misaligned views, the tail of a length that is no
    multiple of 4) as on the vector one."""
    import ctypes
    from u3d import _lib
    from u3d.ops import _stream
    torch.manual_seed(3)
    lr = torch.full((1,), 0.05, device=gpu)
    views = [_views(n, gpu, offs, fill=float("nan")) for n in LENGTHS]
    before = [v[0][1].clone() for v in views]
    descs = [_lib.SgdDesc(v[0][1].data_ptr(), v[1][1].data_ptr(), v[2][1].data_ptr(), n)
             for n, v in zip(LENGTHS, views)]
    arr = (_lib.SgdDesc * len(descs))(*descs)
    _lib.call("u3d_sgd_step", ctypes.addressof(arr), len(descs), lr.data_ptr(), kw["momentum"],
              kw.get("dampening", 0.0), kw.get("weight_decay", 0.0), int(kw.get("nesterov", False)),
              int(kw.get("maximize", False)), 1, _stream())
    torch.cuda.synchronize()
    for n, v, p0 in zip(LENGTHS, views, before):
        _check_sgd_step(f"first n={n} offs={offs}", p0, v[1][1], None, v[0][1], v[2][1], 0.05, kw, True)
        assert _sentinels_ok(v, n), f"n={n}: a float outside a view changed"


@pytest.mark.parametrize("kw", [KWS[0], KWS[2]], ids=str)
def test_sgd_late_and_empty_parameters(gpu, kw):
    """50 parameters get their first .grad at step 2, next to 50 that have stepped before: one step() then issues
    init = 1 and init = 0 launches, each in two batches of <= 48. One parameter on each side has zero elements."""
    from u3d.optim import SGD
    torch.manual_seed(4)
    shapes = [(3,)] * 24 + [(0,)] + [(5, 3)] * 24 + [(4 * 4 * 256 + 1,)]
    early = [torch.randn(s, device=gpu) for s in shapes]
    late = [torch.randn(s, device=gpu) for s in shapes]
    pa = [torch.nn.Parameter(p.clone()) for p in early + late]
    pb = [torch.nn.Parameter(p.clone()) for p in early + late]
    ne = len(early)
    assert ne > 48
    oa, ob = torch.optim.SGD(pa, lr=0.05, **kw), SGD(pb, lr=0.05, **kw)
    for it in range(3):
        live = range(ne) if it == 0 else range(2 * ne)
        before = {}
        for i in live:
            g = torch.randn_like(pa[i])
            pa[i].grad, pb[i].grad = g.clone(), g.clone()
            b = ob.state[pb[i]].get("momentum_buffer")
            before[i] = (pb[i].detach().clone(), None if b is None else b.clone(), b is None)
        oa.step()
        ob.step()
        torch.cuda.synchronize()
        for i in live:
            p0, b0, init = before[i]
            if pb[i].numel():
                _check_sgd_step(f"late step{it}", p0, pb[i].grad, b0, pb[i], ob.state[pb[i]]["momentum_buffer"], 0.05,
                                kw, init)
    for a, b in zip(pa, pb):
        torch.testing.assert_close(b, a, rtol=1e-5, atol=1e-6)
    sa, sb = oa.state_dict()["state"], ob.state_dict()["state"]
    assert set(sa) == set(sb) and all(set(sa[k]) == set(sb[k]) for k in sa)
