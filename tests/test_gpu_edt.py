"""csrc/edt.hip through u3d.surface and the C entry point: the exact 3-D Euclidean distance transform against scipy's
(surface_reference.edt_ref, fp64). Shapes and patterns live in surface_cases.py: every axis at the lengths around the
64-voxel words of the row pass and the column tile of the min-plus passes, the line lengths around every threshold of the
tile's column count, the largest extent.

Bounds. With integer spacings the squared distance is an integer formed exactly in fp64, so the squared output equals
rint(edt_ref^2) rounded to fp32, bit for bit, and the distance is the correctly rounded fp64 root rounded once to fp32,
against scipy's fp64 root: |got - want| <= 2^-23 |want|, one fp32 ulp. With the non-integer spacing the kernel's fp64
sum of w d^2 and scipy's sum of (d s)^2 differ by a few fp64 ulps before the fp32 rounding: the same one-ulp bound holds
for both outputs. +inf exactly where the restatement has it."""
import functools

import numpy as np
import pytest
import torch

import surface_cases as K
import surface_reference as R
from u3d import surface

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23


def _L():
    from u3d import _lib as L
    return L


def _stream():
    from u3d.ops import _stream as s
    return s()


def _dev(a, gpu):
    return torch.from_numpy(np.array(a, order="C")).to(gpu)             # a copy: the cached cases are read-only


@functools.lru_cache(maxsize=None)
def _case(name, shape, spacing):
    m = K.pattern(name, shape)
    want = R.edt_ref(m, spacing)
    m.setflags(write=False)
    want.setflags(write=False)
    return m, want


def _check(got, want, what):
    """fp32 `got` against fp64 `want`: +inf in the same places, one fp32 ulp elsewhere."""
    got = got.astype(np.float64)
    inf = np.isposinf(want)
    assert np.array_equal(np.isposinf(got), inf), what
    err = np.abs(got[~inf] - want[~inf])
    bound = ULP * np.abs(want[~inf])
    worst = float((err - bound).max()) if err.size else 0.0
    assert (err <= bound).all(), (what, worst)


def test_constants_are_the_ones_the_shapes_straddle(gpu):
    assert surface.edt_tile() == (K.MAX_COLS, K.TILE_BYTES) and surface.edt_max_extent() == K.MAX_EXTENT


@pytest.mark.parametrize("shape", K.edt_shapes(), ids=str)
def test_edt_is_scipys(gpu, shape):
    for name in K.PATTERNS:
        md = _dev(K.pattern(name, shape), gpu)
        for sp in K.SPACINGS:
            m, want = _case(name, shape, sp)
            d = surface.distance_to(md, sp).cpu().numpy()
            d2 = surface.distance_to(md, sp, squared=True).cpu().numpy()
            assert d.dtype == np.float32 and d.shape == shape
            _check(d, want, (name, sp, "distance"))
            if sp in K.INTEGER_SPACINGS:
                w2 = np.rint(want ** 2)               # the integer; fp32 holds it up to 2^24, beyond that its rounding
                assert np.array_equal(d2, w2.astype(np.float32)), (name, sp, "squared")
                assert np.array_equal(d, np.sqrt(w2).astype(np.float32)), (name, sp, "root")
            else:
                _check(d2, want ** 2, (name, sp, "squared"))
            if not m.any():
                assert np.isposinf(d).all() and np.isposinf(d2).all()


@pytest.mark.parametrize("shape", [(33, 20, 47), (3, 65, 5), (129, 3, 5)], ids=str)
def test_invert_is_the_complement_and_scipys_function(gpu, shape):
    import scipy.ndimage as ndi
    for name in ("bernoulli0.5", "bernoulli0.95", "gaps", "all", "none"):
        m = K.pattern(name, shape)
        for sp in ((1, 1, 1), (2, 1, 1), (0.7, 1.3, 2.5)):
            a = surface.distance_transform_edt(_dev(m, gpu), sampling=sp)
            b = surface.distance_to(_dev(1 - m, gpu), sp)
            assert torch.equal(a, b), (name, sp)
            if (m == 0).any():
                _check(a.cpu().numpy(), ndi.distance_transform_edt(m, sampling=sp), (name, sp))
            else:
                assert torch.isposinf(a).all()
    a = surface.distance_transform_edt(_dev(K.pattern("bernoulli0.5", shape), gpu))       # sampling=None
    assert torch.equal(a, surface.distance_to(_dev(1 - K.pattern("bernoulli0.5", shape), gpu)))


@pytest.mark.parametrize("dtype", [torch.bool, torch.int64, torch.float32, torch.int16])
def test_any_dtype_nonzero_is_a_feature(gpu, dtype):
    shape = (9, 10, 70)
    g = np.random.default_rng(41)
    vals = np.array([0, 0, 0, 0, 1, -3, 256], dtype=np.float64)[g.integers(0, 7, shape)]
    t = torch.from_numpy(vals).to(gpu)
    t = (t != 0) if dtype == torch.bool else t.to(dtype)
    _check(surface.distance_to(t).cpu().numpy(), R.edt_ref(vals), dtype)
    tp = t.permute(2, 1, 0)                                              # not contiguous
    _check(surface.distance_to(tp).cpu().numpy(), R.edt_ref(vals.transpose(2, 1, 0)), dtype)


def test_two_runs_are_bit_equal_whatever_the_workspace_holds(gpu):
    """The C entry point on a workspace and an output filled with 0xFF, then 0x00: the same bits."""
    shape, sp = (33, 20, 47), (0.7, 1.3, 2.5)
    m, want = _case("bernoulli0.05", shape, sp)
    md = _dev(m, gpu)
    outs = []
    for fill in (0xFF, 0x00):
        ws = torch.full((_L().query("u3d_edt_ws_bytes", m.size),), fill, dtype=torch.uint8, device=gpu)
        out = torch.full(shape, -7.0, dtype=torch.float32, device=gpu)
        _L().call("u3d_edt", md.data_ptr(), *shape, *[float(s) for s in sp], 0, 0, out.data_ptr(), ws.data_ptr(),
                  _stream())
        outs.append(out.cpu().numpy())
    assert outs[0].tobytes() == outs[1].tobytes()
    _check(outs[0], want, "entry point")
    assert outs[0].tobytes() == surface.distance_to(md, sp).cpu().numpy().tobytes()


def test_bad_arguments_are_refused_by_the_entry_point(gpu):
    """Shape arguments only: the checks come before any pointer is used or anything is launched."""
    from u3d._lib import U3DError
    small = torch.zeros(64, dtype=torch.int32, device=gpu)
    p = small.data_ptr()
    big = K.MAX_EXTENT + 1
    for shape in ((big, 1, 1), (1, big, 1), (1, 1, big)):
        with pytest.raises(U3DError, match="per axis"):
            _L().call("u3d_edt", p, *shape, 1.0, 1.0, 1.0, 0, 0, p, p, _stream())
    with pytest.raises(U3DError, match="2\\^31"):
        _L().call("u3d_edt", p, 2048, 1024, 1024, 1.0, 1.0, 1.0, 0, 0, p, p, _stream())
    with pytest.raises(U3DError):
        _L().call("u3d_edt", p, 0, 4, 4, 1.0, 1.0, 1.0, 0, 0, p, p, _stream())
    with pytest.raises(U3DError, match="spacing"):
        _L().call("u3d_edt", p, 2, 2, 2, 1.0, 0.0, 1.0, 0, 0, p, p, _stream())
    for args in ((None, p, p), (p, None, p), (p, p, None)):
        with pytest.raises(U3DError, match="null"):
            _L().call("u3d_edt", args[0], 2, 2, 2, 1.0, 1.0, 1.0, 0, 0, args[1], args[2], _stream())
    with pytest.raises(ValueError):
        surface.distance_to(torch.zeros((1, 1, big), dtype=torch.uint8, device=gpu))
    assert int(small.sum().item()) == 0                                  # nothing ran on the 256 bytes
