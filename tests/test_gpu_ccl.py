"""csrc/ccl.hip through u3d.data and the C entry points: 3-D connected components against scipy.ndimage.label, the
getmaxcomponent rule against body_crop_reference.py, the mask helpers against scipy. Everything is integer or boolean:
every comparison is exact, of every voxel. Shapes and patterns live in body_crop_cases.py (their properties are asserted
on the CPU by test_body_crop_reference.py); the shapes straddle the labelling tile's seams on every axis."""
import numpy as np
import pytest
import scipy.ndimage as ndi
import torch

import body_crop_cases as K
import body_crop_reference as R
from u3d.data import bounding_box, ccl_tile, label_components, largest_component

pytestmark = pytest.mark.gpu


def _L():
    from u3d import _lib as L
    return L


def _stream():
    from u3d.ops import _stream as s
    return s()


def _dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def test_tile_is_the_one_the_shapes_straddle(gpu):
    assert ccl_tile() == K.TILE


# ------------------------------------------------------------------------------------------------ labelling
@pytest.mark.parametrize("shape", K.label_shapes(), ids=str)
@pytest.mark.parametrize("name", K.PATTERNS)
def test_label_components_is_scipys(gpu, name, shape):
    m = K.pattern(name, shape)
    want, wn = ndi.label(m)
    lab, n = label_components(_dev(m, gpu))
    assert lab.dtype == torch.int32 and tuple(lab.shape) == shape
    assert n == wn
    assert np.array_equal(lab.cpu().numpy(), want)


@pytest.mark.parametrize("value", [0, 1])
def test_single_voxel(gpu, value):
    lab, n = label_components(torch.full((1, 1, 1), value, dtype=torch.uint8, device=gpu))
    assert n == value and lab.cpu().tolist() == [[[value]]]


def test_percolation_threshold_volume(gpu):
    m = K.pattern("bernoulli0.31", K.PERCOLATION_SHAPE)
    want, wn = ndi.label(m)
    lab, n = label_components(_dev(m, gpu))
    assert n == wn and np.array_equal(lab.cpu().numpy(), want)


def test_result_ignores_stale_workspace_and_output(gpu):
    """The C entry point on a workspace and an output filled with 0xFF, twice: the same labels, scipy's."""
    shape = K.label_shapes()[-1]
    m = K.pattern("bernoulli0.31", shape)
    want, wn = ndi.label(m)
    md = _dev(m, gpu)
    for fill in (0xFF, 0x00):
        ws = torch.full((_L().query("u3d_ccl_ws_bytes", m.size),), fill, dtype=torch.uint8, device=gpu)
        lab = torch.full(shape, -7, dtype=torch.int32, device=gpu)
        n = torch.full((1,), -7, dtype=torch.int32, device=gpu)
        _L().call("u3d_ccl_label", md.data_ptr(), *shape, lab.data_ptr(), n.data_ptr(), ws.data_ptr(), _stream())
        assert int(n.item()) == wn and np.array_equal(lab.cpu().numpy(), want)


@pytest.mark.parametrize("dtype", [torch.bool, torch.int64, torch.float32, torch.float64, torch.int16])
def test_any_dtype_nonzero_is_foreground(gpu, dtype):
    shape = (9, 10, 70)
    g = np.random.default_rng(27)
    vals = np.array([0, 0, 1, -3, 256, 7], dtype=np.float64)[g.integers(0, 6, shape)]
    t = torch.from_numpy(vals).to(gpu)
    if dtype.is_floating_point:
        t = t.to(dtype)
        t[0, 0, 0], vals[0, 0, 0] = float("nan"), 1.0            # NaN != 0
        t[0, 0, 2], vals[0, 0, 2] = 0.25, 1.0
    else:
        t = (t != 0) if dtype == torch.bool else t.to(dtype)
    want, wn = ndi.label(vals != 0)
    lab, n = label_components(t)
    assert n == wn and np.array_equal(lab.cpu().numpy(), want)


def test_non_contiguous_mask(gpu):
    m = K.pattern("bernoulli0.5", (17, 33, 70))
    t = _dev(m, gpu).permute(2, 1, 0)
    want, wn = ndi.label(m.transpose(2, 1, 0))
    lab, n = label_components(t)
    assert n == wn and np.array_equal(lab.cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------ getmaxcomponent
@pytest.mark.parametrize("name", list(K.largest_cases()))
def test_largest_component(gpu, name):
    m, num_limit, min_filter = K.largest_cases()[name]
    want = R.largest_component(m, num_limit, min_filter)
    got = largest_component(_dev(m, gpu), num_limit, min_filter)
    if want is None:
        assert got is None
    else:
        assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)


def test_largest_component_defaults_on_a_tortuous_mask(gpu):
    m = K.pattern("bernoulli0.31", K.PERCOLATION_SHAPE)
    for num_limit, min_filter in ((10, 1e6), (100, 20.0), (1024, 300.0)):
        want = R.largest_component(m, num_limit, min_filter)
        got = largest_component(_dev(m, gpu), num_limit, min_filter)
        assert (got is None) == (want is None)
        if want is not None:
            assert np.array_equal(got.cpu().numpy(), want)


def test_select_record(gpu):
    """The record of u3d_ccl_select: found, label, size, the inclusive bounding box, n."""
    m, num_limit, min_filter = K.largest_cases()["tie"]
    lab, n = label_components(_dev(m, gpu))
    nd = torch.tensor([n], dtype=torch.int32, device=gpu)
    out = torch.full(m.shape, 9, dtype=torch.uint8, device=gpu)
    rec = torch.full((12,), -5, dtype=torch.int32, device=gpu)
    ws = torch.full((_L().query("u3d_ccl_select_ws_bytes"),), 0xFF, dtype=torch.uint8, device=gpu)
    _L().call("u3d_ccl_select", lab.data_ptr(), *m.shape, nd.data_ptr(), num_limit, min_filter, out.data_ptr(),
              rec.data_ptr(), ws.data_ptr(), _stream())
    assert rec.cpu().tolist() == [1, 2, 768, 1, 2, 3, 3, 5, 66, 4, 0, 0]
    _L().call("u3d_ccl_select", lab.data_ptr(), *m.shape, nd.data_ptr(), num_limit, 1e6, out.data_ptr(),
              rec.data_ptr(), ws.data_ptr(), _stream())
    assert rec.cpu().tolist() == [0, 0, 0] + [2 ** 31 - 1] * 3 + [-1] * 3 + [4, 0, 0] and not out.any().item()


# ------------------------------------------------------------------------------------------------ mask helpers
def _threshold(vol, t, erode, gpu, gate=None):
    v = _dev(vol, gpu)
    out = torch.full(vol.shape, 9, dtype=torch.uint8, device=gpu)
    _L().call("u3d_body_threshold", v.data_ptr(), *vol.shape, float(t), erode, out.data_ptr(),
              gate.data_ptr() if gate is not None else None, _stream())
    return out.cpu().numpy()


@pytest.mark.parametrize("shape", [(1, 5, 70), (5, 1, 70), (5, 6, 1), (2, 2, 2), (9, 17, 129), (7, 9, 65)], ids=str)
def test_threshold_and_erosion_are_scipys(gpu, shape):
    g = np.random.default_rng([28] + list(shape))
    vol = (g.standard_normal(shape) * 100 - 120).astype(np.float32)
    vol.reshape(-1)[g.integers(0, vol.size, max(1, vol.size // 50))] = np.float32(-200)      # exactly the threshold
    vol.reshape(-1)[g.integers(0, vol.size, max(1, vol.size // 50))] = np.float32("nan")
    m = vol > np.float32(-200)
    assert np.array_equal(_threshold(vol, -200, 0, gpu), m.astype(np.uint8))
    want = ndi.binary_erosion(m, structure=np.ones((2, 2, 2)))
    got = _threshold(vol, -200, 1, gpu)
    assert np.array_equal(got, want.astype(np.uint8))
    assert not got[0].any() and not got[:, 0].any() and not got[:, :, 0].any()


def _window3(m, lo, hi, op, gpu):
    cur = _dev(m.astype(np.uint8), gpu)
    Z, Y, X = m.shape
    for outer, n, inner in ((1, Z, Y * X), (Z, Y, X), (Z * Y, X, 1)):
        nxt = torch.full(m.shape, 9, dtype=torch.uint8, device=gpu)
        _L().call("u3d_mask_window_axis", cur.data_ptr(), nxt.data_ptr(), outer, n, inner, lo, hi, op, None, _stream())
        cur = nxt
    return cur.cpu().numpy().astype(bool)


@pytest.mark.parametrize("shape", [(4, 9, 10), (10, 10, 10), (11, 23, 70), (30, 9, 31)], ids=str)
def test_box_erosion_and_dilation_are_scipys(gpu, shape):
    g = np.random.default_rng([29] + list(shape))
    s = np.ones((10, 10, 10))
    m = g.random(shape) < 0.985
    assert np.array_equal(_window3(m, -5, 4, 0, gpu), ndi.binary_erosion(m, structure=s))
    sparse = g.random(shape) < 0.002
    sparse[0, 0, 0] = sparse[-1, -1, -1] = True
    assert np.array_equal(_window3(sparse, -4, 5, 1, gpu), ndi.binary_dilation(sparse, structure=s))
    full = np.ones(shape, dtype=bool)                            # the border alone erodes
    assert np.array_equal(_window3(full, -5, 4, 0, gpu), ndi.binary_erosion(full, structure=s))


def test_gate_turns_the_helpers_off(gpu):
    vol = np.full((3, 4, 5), 7.0, dtype=np.float32)
    for g, want in ((0, 1), (1, 9)):
        gate = torch.tensor([g], dtype=torch.int32, device=gpu)
        assert (_threshold(vol, 0.0, 0, gpu, gate) == want).all()


@pytest.mark.parametrize("dtype", [torch.uint8, torch.float32, torch.int32, torch.float64, torch.bool])
def test_bounding_box(gpu, dtype):
    shape = (9, 17, 140)
    x = np.zeros(shape, dtype=np.float64)
    x[2, 5, 130], x[7, 3, 4], x[4, 16, 64] = 3, -1, 2
    t = torch.from_numpy(x).to(gpu).to(dtype)
    assert bounding_box(t) == R.bounding_box(x) == ((2, 3, 4), (7, 16, 130))
    with pytest.raises(ValueError):
        bounding_box(torch.zeros(shape, dtype=dtype, device=gpu))


def test_bounding_box_counts_nan(gpu):
    t = torch.zeros((2, 3, 4), device=gpu)
    t[1, 2, 3] = float("nan")
    assert bounding_box(t) == ((1, 2, 3), (1, 2, 3))


# ------------------------------------------------------------------------------------------------ errors
def test_cpu_tensor_is_refused():
    from u3d._lib import U3DError
    for f in (label_components, largest_component, bounding_box):
        with pytest.raises(U3DError):
            f(torch.ones((2, 3, 4), dtype=torch.uint8))


def test_non_3d_is_a_value_error(gpu):
    for f in (label_components, largest_component, bounding_box):
        for shape in ((4, 5), (1, 2, 3, 4), (0, 3, 4)):
            with pytest.raises(ValueError):
                f(torch.ones(shape, dtype=torch.uint8, device=gpu))


def test_two_to_the_31_voxels_are_refused_by_the_entry_point(gpu):
    """Shape arguments only: the check comes before any pointer is used, nothing of that size is allocated."""
    from u3d._lib import U3DError
    assert _L().query("u3d_ccl_ws_bytes", 2 ** 31) == -1 and _L().query("u3d_ccl_ws_bytes", 2 ** 31 - 1) > 0
    small = torch.zeros(64, dtype=torch.int32, device=gpu)
    p = small.data_ptr()
    with pytest.raises(U3DError, match="2\\^31"):
        _L().call("u3d_ccl_label", p, 2048, 1024, 1024, p, p, p, _stream())
    with pytest.raises(U3DError, match="2\\^31"):
        _L().call("u3d_ccl_select", p, 2048, 1024, 1024, p, 10, 1.0, p, p, p, _stream())
    with pytest.raises(U3DError):
        _L().call("u3d_ccl_select", p, 2, 2, 2, p, 1025, 1.0, p, p, p, _stream())
