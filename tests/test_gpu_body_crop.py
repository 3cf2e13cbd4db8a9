"""u3d.data.get_body and body_crop (the body mask and crops of the reference's preprocess/forward_crop.py) on the
device: small shapes with min_filter overrides against the host restatement body_crop_reference.py (both get_body
routes, both outcomes of the hand test), and the cases of tests/golden/g21_body_crop.npz, made by the reference's own
lines, with its default filters. Masks, bounding boxes and sizes are exact; image_a and label_a are slices, so they are
bit-equal to the restatement's."""
import numpy as np
import pytest
import torch

import body_crop_cases as K
import body_crop_reference as R
from conftest import golden
from u3d.data import ROUTE_COMPONENT, ROUTE_FALLBACK, body_crop, body_threshold, get_body

pytestmark = pytest.mark.gpu


def _dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _bits(a):
    a = a.cpu().numpy() if isinstance(a, torch.Tensor) else np.asarray(a)
    return np.ascontiguousarray(a).view(np.uint32 if a.dtype == np.float32 else a.dtype)


@pytest.mark.parametrize("name", list(K.SMALL))
def test_get_body_small(gpu, name):
    cid, mf, mfu, _ = K.SMALL[name]
    _, img, _ = K.case_inputs(name)
    t = R.body_threshold(cid)
    for vol, f in ((img, mf), (img[:, :, :img.shape[2] // 2 + 3], mfu)):
        want, _ = R.get_body(vol, t, f)
        got = get_body(_dev(vol, gpu), t, f)
        assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), want)


def test_get_body_fallback_threshold(gpu):
    """The fallback's own threshold (the reference's global) may differ from the component search's."""
    _, img, _ = K.case_inputs("fallback_first")
    want, route = R.get_body(img, 25, 1e6, fallback_threshold=190.0)
    assert route == R.ROUTE_FALLBACK
    got = get_body(_dev(img, gpu), 25, 1e6, fallback_threshold=190.0)
    assert np.array_equal(got.cpu().numpy(), want)
    assert not np.array_equal(want, R.get_body(img, 25, 1e6)[0])


def _compare(got, want):
    image_a, label_a, info = got
    w_image, w_label, w = want
    assert tuple(image_a.shape) == w_image.shape and tuple(label_a.shape) == w_label.shape
    assert np.array_equal(_bits(image_a), _bits(w_image)) and np.array_equal(_bits(label_a), _bits(w_label))
    for k in ("label_range", "bbox", "bbox_up", "size", "size_up", "route", "route_up", "inter_all", "inter_up",
              "found_hand"):
        assert info[k] == w[k], (k, info[k], w[k])
    assert np.array_equal(info["mask"].cpu().numpy(), w["mask"])
    assert float(info["label_sum_before"]) == w["label_sum_before"]
    assert float(info["label_sum_after"]) == w["label_sum_after"]


@pytest.mark.parametrize("name", list(K.SMALL))
def test_body_crop_small(gpu, name):
    cid, mf, mfu, _ = K.SMALL[name]
    _, img, lab = K.case_inputs(name)
    want = R.body_crop(img, lab, cid, mf, mfu)
    di, dl = _dev(img, gpu), _dev(lab, gpu)
    got = body_crop(di, dl, cid, mf, mfu)
    _compare(got, want)
    assert np.array_equal(_bits(dl), _bits(lab)), "the caller's label is left as it was"
    assert got[0].data_ptr() >= di.data_ptr() and got[0].data_ptr() < di.data_ptr() + di.numel() * 4, "image_a is a view"
    assert (ROUTE_COMPONENT, ROUTE_FALLBACK) == (R.ROUTE_COMPONENT, R.ROUTE_FALLBACK)


@pytest.mark.parametrize("name", list(K.FIXTURES))
def test_body_crop_reference_fixture(gpu, name):
    g = golden("g21_body_crop.npz")
    cid, img, lab = K.case_inputs(name)
    assert str(g[f"{name}_insum"]) == K.checksum(img, lab), "the inputs moved: regenerate the fixture"
    image_a, label_a, info = body_crop(_dev(img, gpu), _dev(lab, gpu), cid)
    assert np.array_equal(np.array(info["bbox"]), g[f"{name}_bbox"])
    assert np.array_equal(np.array(info["bbox_up"]), g[f"{name}_bbox_up"])
    assert (info["size"], info["size_up"]) == (int(g[f"{name}_size"]), int(g[f"{name}_size_up"]))
    assert (info["route"], info["route_up"]) == (int(g[f"{name}_route"]), int(g[f"{name}_route_up"]))
    assert [info["inter_all"], info["inter_up"], int(info["found_hand"])] == g[f"{name}_inter"].tolist()
    assert [list(image_a.shape), list(label_a.shape), list(info["mask"].shape)] == g[f"{name}_shapes"].tolist()
    assert np.array_equal(np.packbits(info["mask"].cpu().numpy() != 0), g[f"{name}_mask_bits"])
    assert [K.checksum(image_a.cpu().numpy()), K.checksum(label_a.cpu().numpy())] == g[f"{name}_sha"].tolist()
    sums = g[f"{name}_sums"]
    assert float(info["label_sum_after"]) == sums[1] and float(info["label_sum_before"]) == sums[2]


def test_thresholds():
    assert [body_threshold(c) for c in (1, 410, 411, 500, 518, 540, 600)] == [-200, -200, 25, 25, 30000, 30000, 25]


def test_errors(gpu):
    from u3d._lib import U3DError
    cid, mf, mfu, _ = K.SMALL["nohand_extent"]
    _, img, lab = K.case_inputs("nohand_extent")
    di, dl = _dev(img, gpu), _dev(lab, gpu)
    with pytest.raises(U3DError):
        body_crop(torch.from_numpy(img.copy()), torch.from_numpy(lab.copy()), cid, mf, mfu)
    with pytest.raises(U3DError):
        get_body(torch.from_numpy(img.copy()))
    with pytest.raises(ValueError):
        get_body(di[0])
    with pytest.raises(ValueError):
        body_crop(di[None], dl[None], cid, mf, mfu)
    with pytest.raises(ValueError):
        body_crop(di, dl[:, :, 1:], cid, mf, mfu)
    with pytest.raises(ValueError):                      # only codes >= 14: empty once they are cleared
        body_crop(di, torch.where(dl >= 14, dl, torch.zeros_like(dl)), cid, mf, mfu)
    with pytest.raises(ValueError):                      # nothing above the threshold: both routes come out empty
        body_crop(torch.zeros_like(di), dl, cid, mf, mfu)
