"""u3d_ccl_keep_largest through u3d.data.keep_largest_per_label and the C entry point: per label the largest
face-connected component, in one labelling of the whole code map, against scipy.ndimage.label(x == l), np.bincount and
the first maximum per label (postproc_cases.oracle). Everything is integer: the output and the whole record are compared
exactly, out of place and in place. The cases (postproc_cases.py) lay codes over the shapes and patterns of
body_crop_cases.py, whose shapes straddle the labelling tile's seams on every axis."""
import numpy as np
import pytest
import torch

import body_crop_cases as BK
import postproc_cases as K
from u3d import data

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
    assert data.ccl_tile() == BK.TILE


@pytest.mark.parametrize("name", list(K.cases()))
def test_keep_largest_is_scipys_per_label(gpu, name):
    codes, num_labels = K.cases()[name]
    want, wrec = K.oracle(name)
    x = _dev(codes, gpu)
    out, rec = data.keep_largest_per_label(x, num_labels, return_record=True)
    assert out.dtype == torch.uint8 and tuple(out.shape) == codes.shape and out.data_ptr() != x.data_ptr()
    assert rec.dtype == torch.int32 and tuple(rec.shape) == (num_labels, 4)
    assert np.array_equal(x.cpu().numpy(), codes)                                  # the input is left alone
    assert np.array_equal(rec.cpu().numpy(), wrec), (rec.cpu().numpy(), wrec)
    assert np.array_equal(out.cpu().numpy(), want)
    assert torch.equal(data.keep_largest_per_label(x, num_labels), out)
    # in place through the entry point, on a workspace and a record filled with 0xFF and then with zeros
    for fill in (0xFF, 0x00):
        buf = _dev(codes, gpu)
        ws = torch.full((_L().query("u3d_ccl_keep_largest_ws_bytes", codes.size),), fill, dtype=torch.uint8, device=gpu)
        r = torch.full((num_labels, 4), -7 if fill else 0, dtype=torch.int32, device=gpu)
        _L().call("u3d_ccl_keep_largest", buf.data_ptr(), *codes.shape, num_labels, buf.data_ptr(), r.data_ptr(),
                  ws.data_ptr(), _stream())
        assert np.array_equal(buf.cpu().numpy(), want) and np.array_equal(r.cpu().numpy(), wrec), fill


@pytest.mark.parametrize("dtype", [torch.int16, torch.int32, torch.int64])
def test_integer_dtypes_come_back_as_they_came(gpu, dtype):
    codes, num_labels = K.cases()["crossing"]
    want, _ = K.oracle("crossing")
    out = data.keep_largest_per_label(_dev(codes, gpu).to(dtype), num_labels)
    assert out.dtype == dtype and np.array_equal(out.cpu().numpy(), want.astype(out.cpu().numpy().dtype))
    t = _dev(codes, gpu).to(dtype).permute(2, 1, 0)                                # a non-contiguous view
    import scipy.ndimage as ndi
    got = data.keep_largest_per_label(t, 3).cpu().numpy()
    ct = codes.transpose(2, 1, 0)
    for l in (1, 2, 3):
        lab, n = ndi.label(ct == l)
        sizes = np.bincount(lab.ravel())[1:]
        assert np.array_equal(got == l, lab == int(np.argmax(sizes)) + 1), l
    assert np.array_equal(got[ct > 3], ct[ct > 3])


@pytest.mark.parametrize("name", ["plain", "tie", "hidden"])
def test_one_label_on_a_mask_is_largest_component(gpu, name):
    """A binary mask as label 1: the kept component is the one largest_component picks when it looks at every
    component (num_limit above their number, no size filter)."""
    m, _, _ = BK.largest_cases()[name]
    x = _dev(m, gpu)
    want = data.largest_component(x, num_limit=1024, min_filter=0)
    out, rec = data.keep_largest_per_label(x, 1, return_record=True)
    assert want is not None and torch.equal(out, want)
    assert int(rec[0, 0]) < 1023 and int(rec[0, 2]) == int(want.sum())


@pytest.mark.parametrize("pattern", ["bernoulli0.31", "serpentine", "ones"])
def test_one_label_on_the_patterns_is_largest_component(gpu, pattern):
    m = BK.pattern(pattern, (5, 7, 300))
    x = _dev(m, gpu)
    out, rec = data.keep_largest_per_label(x, 1, return_record=True)
    assert int(rec[0, 0]) < 1023                                                   # largest_component sees them all
    assert torch.equal(out, data.largest_component(x, num_limit=1024, min_filter=0))


def test_bad_arguments(gpu):
    from u3d._lib import U3DError
    assert _L().query("u3d_ccl_keep_largest_ws_bytes", 2 ** 31) == -1
    small = torch.zeros(4096, dtype=torch.int32, device=gpu)
    p = small.data_ptr()
    with pytest.raises(U3DError, match="2\\^31"):
        _L().call("u3d_ccl_keep_largest", p, 2048, 1024, 1024, 13, p, p, p, _stream())
    for n in (0, 256, -1):
        with pytest.raises(U3DError, match="num_labels"):
            _L().call("u3d_ccl_keep_largest", p, 2, 2, 2, n, p, p, p, _stream())
    for args in ((None, 2, 2, 2, 13, p, p, p), (p, 2, 2, 2, 13, None, p, p), (p, 2, 2, 2, 13, p, None, p),
                 (p, 2, 2, 2, 13, p, p, None), (p, 0, 2, 2, 13, p, p, p)):
        with pytest.raises(U3DError):
            _L().call("u3d_ccl_keep_largest", *args, _stream())
    torch.cuda.synchronize()
    assert not small.any().item()
