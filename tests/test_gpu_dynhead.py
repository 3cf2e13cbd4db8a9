"""csrc/dynhead.hip kernel by kernel against the fp64 references of heads_reference.py: u3d_dyn_controller,
u3d_dynhead_fwd, u3d_dynhead_bwd (+ its reduce kernel) and u3d_dyn_controller_bwd (u3d_gn_relu_mean is pinned in
test_gpu_groupnorm.py). The C entry points are called through u3d._lib, as u3d/dynhead.py calls them, on buffers the
test allocates and pre-fills with NaN (outputs and `part`), so an element a kernel leaves out cannot pass. Every
element is compared.

Sizes follow the launchers' constants: FWD_BLOCKS = 2048 and BWD_BLOCKS = 512 blocks of 256 threads per sample in
dynhead_fwd_kernel / dynhead_bwd_kernel; above 256 * that many voxels a thread walks several voxels and, in the
backward, carries its 162 gradient accumulators across them.

Bounds: worst-case counts of the fp32 roundings in the code, u = 2^-24, times magnitudes of the fp64 reference only
(values and abs-sums), inflated by 1 + 2^-10 for the second-order terms.

controller  a chain of kf fmas on the bias and one add for the one-hot column: (kf + 1) u (|b| + sum|w x|)
forward     da1 = 8 u a1_abs, da2 = 8 u a2_abs + |W2| da1, dout = 8 u out_abs + |W3| da2   (8 fmas on the bias a layer;
            relu is 1-Lipschitz; x_abs = |b| + |W| |input|)
ReLU kinks  the kernel's relu mask and autograd's agree only if no pre-activation changes sign under rounding. The
            inputs are built so that |a1| > 4 da1 and |a2| > 4 da2 everywhere (voxels that miss it are redrawn from the
            same generator until none is left); the test asserts it and excludes nothing.
dh          dr2 = fma(W3_0k, d0, W3_1k d1): 2 u dr2_abs. dr1: 8 fmas on it: 10 u dr1_abs. dh: 8 fmas on that:
            |dh - ref| <= 8 u |W1|^T |da1| + 10 u |W1|^T (mask1 dr1_abs)
dparams     K = ceil(v / (256 blocks)) fmas per thread + 6 shuffle levels + 3 adds over the waves + 1 store; the
            cross-block sum is fp64, rounded once (inside the + 1): K u abs-sum + sum_v of the terms' own errors
            (dda1 |h|; dda2 r1 + |da2| da1; |d| da2; dda1; dda2; none for b3), dda2 = 2 u mask2 dr2_abs,
            dda1 = 10 u mask1 dr1_abs.
            A sample whose b1 is -100 has every layer-1 unit dead: the bounds of its dh and its W1 / b1 / W2 gradients
            are 0, so those must be exactly 0, while its b3 gradient keeps the full bound.
ctrl bwd    dW, db: n u abs-sum (+ u |prev + ref| when accumulating). dA: 162 fmas and a division,
            163 u sum|w dy| / v, for bf16 + 2^-8 (|ref| + that) (8 significant bits: round-to-nearest moves a value by
            up to 2^-8 of it); the v voxels of a sample hold the same bits.

Every test prints its worst error as a share of the bound ("SHARE <family> <value>") before asserting.
"""
import functools
import math

import pytest
import torch

import heads_reference as R
from heads_reference import U

pytestmark = pytest.mark.gpu

FWD_BLOCKS, BWD_BLOCKS = 2048, 512
KF, KT, M = 256, 7, 162
SLACK = 1 + 2.0 ** -10
f32, bf16 = torch.float32, torch.bfloat16

HEAD_CASES = [(1, 1), (1, 255), (2, 257), (3, 1000),
              (2, BWD_BLOCKS * 256 + 300)]          # backward grid-stride: the threads of 300 voxels walk two of them
FWD_ONLY = [(1, FWD_BLOCKS * 256 + 300)]            # forward grid-stride
DEAD = 1                                            # the sample with b1 = -100 (cases with n > 1)


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


def _fwd_err(f, params):
    """(da1, da2, dout) of the docstring from a heads_reference.dynhead_fwd_ref result."""
    _, w2, w3, _, _, _ = R.split_params(params.double())
    da1 = 8 * U * f.a1_abs
    da2 = 8 * U * f.a2_abs + torch.einsum("nok,nvk->nvo", w2.abs(), da1)
    return da1, da2, 8 * U * f.out_abs + torch.einsum("nok,nvk->nvo", w3.abs(), da2)


@functools.lru_cache(maxsize=None)
def _case(n, v):
    """params, h, dout (fp32) with every pre-activation clear of 0 by 4 rounding bounds, and the fp64 forward."""
    gen = torch.Generator().manual_seed(31 * n + v)
    r = lambda *s: torch.randn(*s, generator=gen)                      # noqa: E731
    params = R.join_params(1.2 * r(n, 8, 8) / 8 ** 0.5, 1.2 * r(n, 8, 8) / 8 ** 0.5, r(n, 2, 8) / 8 ** 0.5,
                           0.3 * r(n, 8), 0.3 * r(n, 8), r(n, 2)).contiguous()
    if n > 1:
        params[DEAD, 144:152] = -100.0
    h = r(n, v, 8)
    for _ in range(50):
        f = R.dynhead_fwd_ref(h, params)
        da1, da2, _ = _fwd_err(f, params)
        bad = ((f.a1.abs() <= 4 * da1) | (f.a2.abs() <= 4 * da2)).any(2)
        if not bool(bad.any()):
            break
        h[bad] = r(int(bad.sum()), 8)
    return dict(params=params, h=h, dout=r(n, v, 2), fwd=f)


@functools.lru_cache(maxsize=None)
def _bwd_ref(n, v):
    I = _case(n, v)
    return R.dynhead_bwd_ref(I["h"], I["params"], I["dout"])


# ------------------------------------------------------------------------------------------------ controller
@pytest.mark.parametrize("tasks", [(3,), (0, 1, 2), (4, 5, 6)], ids=str)
def test_controller(gpu, tasks):
    n = len(tasks)
    gen = torch.Generator().manual_seed(sum(tasks))
    feat = torch.randn(n, KF, generator=gen).abs()
    w, b = torch.randn(M, KF + KT, generator=gen) / 16, torch.randn(M, generator=gen)
    task = torch.tensor(tasks, dtype=torch.int64)
    ref = R.controller_ref(feat, task, w, b, KT)
    out = _nan((n, M), f32, gpu)
    dev = [t.to(gpu) for t in (feat, task, w, b)]
    _L().call("u3d_dyn_controller", dev[0].data_ptr(), n, KF, dev[1].data_ptr(), KT, dev[2].data_ptr(),
              dev[3].data_ptr(), M, out.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert _share(f"dyn-controller {tasks}", (out.cpu().double() - ref.params).abs(), SLACK * (KF + 1) * U * ref.abs) <= 1


# ------------------------------------------------------------------------------------------------ heads
def _assert_margin(I):
    f = I["fwd"]
    da1, da2, _ = _fwd_err(f, I["params"])
    assert bool((f.a1.abs() > 4 * da1).all()) and bool((f.a2.abs() > 4 * da2).all()), "a pre-activation near 0"


@pytest.mark.parametrize("n,v", HEAD_CASES + FWD_ONLY, ids=str)
def test_dynhead_fwd(gpu, n, v):
    I = _case(n, v)
    _assert_margin(I)
    out = _nan((n, v, 2), f32, gpu)
    h, p = I["h"].to(gpu), I["params"].to(gpu)
    _L().call("u3d_dynhead_fwd", h.data_ptr(), p.data_ptr(), n, v, out.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert _share(f"dyn-fwd ({n}, {v})", (out.cpu().double() - I["fwd"].out).abs(),
                  SLACK * _fwd_err(I["fwd"], I["params"])[2]) <= 1


@pytest.mark.parametrize("n,v", HEAD_CASES, ids=str)
def test_dynhead_bwd(gpu, n, v):
    L = _L()
    I, ref = _case(n, v), _bwd_ref(n, v)
    _assert_margin(I)
    nb = L.query("u3d_dynhead_bwd_blocks", v)
    assert nb == min(BWD_BLOCKS, (v + 255) // 256)
    dh, part, dp = _nan((n, v, 8), f32, gpu), _nan((n, nb, M), f32, gpu), _nan((n, M), f32, gpu)
    h, p, d = I["h"].to(gpu), I["params"].to(gpu), I["dout"].to(gpu)
    L.call("u3d_dynhead_bwd", h.data_ptr(), p.data_ptr(), d.data_ptr(), n, v, dh.data_ptr(), part.data_ptr(),
           dp.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert bool(torch.isfinite(part).all()), "a float of part was not written"
    f = ref.fwd
    da1, da2, _ = _fwd_err(f, I["params"])
    b_dh = 8 * U * ref.dh_abs1 + 10 * U * ref.dh_abs
    dh, dp = dh.cpu().double(), dp.cpu().double()
    assert _share(f"dyn-dh ({n}, {v})", (dh - ref.dh).abs(), SLACK * b_dh) <= 1
    K = math.ceil(v / (256 * nb)) + 6 + 3 + 1
    dda2, dda1 = 2 * U * ref.k2 * ref.dr2_abs, 10 * U * ref.k1 * ref.dr1_abs
    outer = lambda a, b: torch.einsum("nvo,nvk->nok", a, b)             # noqa: E731
    terms = R.join_params(outer(dda1, f.h.abs()), outer(dda2, f.r1) + outer(ref.da2.abs(), ref.k1 * da1),
                          outer(ref.d.abs(), ref.k2 * da2), dda1.sum(1), dda2.sum(1), torch.zeros(n, 2, dtype=torch.float64))
    b_dp = K * U * ref.dparams_abs + terms
    assert _share(f"dyn-dparams ({n}, {v})", (dp - ref.dparams).abs(), SLACK * b_dp) <= 1
    if n > 1:   # the dead sample: exact zeros where nothing flows, an exact bound on b3 where everything does
        assert not dh[DEAD].any() and not dp[DEAD, :128].any() and not dp[DEAD, 144:152].any()
        assert bool((b_dp[DEAD, 160:] > 0).all()) and bool((ref.dparams[DEAD, 160:] != 0).all())
        assert _share(f"dyn-db3-dead ({n}, {v})", (dp - ref.dparams).abs()[DEAD, 160:], SLACK * b_dp[DEAD, 160:]) <= 1


# ------------------------------------------------------------------------------------------------ controller backward
@pytest.mark.parametrize("acc", [0, 1], ids=["write", "accumulate"])
@pytest.mark.parametrize("dtype", [f32, bf16], ids=["f32", "bf16"])
@pytest.mark.parametrize("v", [1, 72])
@pytest.mark.parametrize("n", [1, 2, 3])
def test_controller_bwd(gpu, n, v, dtype, acc):
    L = _L()
    gen = torch.Generator().manual_seed(10 * n + v)
    r = lambda *s: torch.randn(*s, generator=gen)                      # noqa: E731
    feat, w, dy = r(n, KF).abs(), r(M, KF + KT) / 16, r(n, M)
    pw, pb = r(M, KF + KT), r(M)
    task = torch.tensor([(3 * i + n) % KT for i in range(n)], dtype=torch.int64)
    ref = R.controller_bwd_ref(feat, task, w, dy, v, KT)
    dw = pw.to(gpu) if acc else _nan((M, KF + KT), f32, gpu)
    db = pb.to(gpu) if acc else _nan((M,), f32, gpu)
    dA = _nan((n, v, KF), dtype, gpu)
    dev = [t.to(gpu) for t in (feat, task, w, dy)]
    L.call("u3d_dyn_controller_bwd", L.BF16 if dtype == bf16 else L.F32, dev[0].data_ptr(), n, KF, dev[1].data_ptr(),
           KT, dev[2].data_ptr(), dev[3].data_ptr(), M, dw.data_ptr(), db.data_ptr(), acc, v, dA.data_ptr(), _stream())
    torch.cuda.synchronize()
    tag = f"n{n} v{v} {'bf16' if dtype == bf16 else 'f32'} acc{acc}"
    for nm, got, want, a, prev in (("dW", dw, ref.dw, ref.dw_abs, pw), ("db", db, ref.db, ref.db_abs, pb)):
        w_ = want + (prev.double() if acc else 0)
        bound = n * U * a + (U * w_.abs() if acc else 0)
        assert _share(f"dyn-ctrl-{nm} {tag}", (got.cpu().double() - w_).abs(), SLACK * bound) <= 1
    dA = dA.cpu()
    assert bool(torch.isfinite(dA.float()).all())
    assert bool((dA == dA[:, :1]).all()), "the voxels of a sample differ"
    bound = (M + 1) * U * ref.dA_abs
    if dtype == bf16:
        bound = bound + 2.0 ** -8 * (ref.dA.abs() + bound)
    assert _share(f"dyn-ctrl-dA {tag}", (dA.double() - ref.dA[:, None, :]).abs(),
                  (SLACK * bound)[:, None, :].expand(n, v, KF)) <= 1
