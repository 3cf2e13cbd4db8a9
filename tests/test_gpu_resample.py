"""u3d.data.GridPlan.apply, resample_spacing and preprocess_case (csrc/resample.hip) on the device against the float64
restatement resample_reference.py, on the cases of resample_cases.py (every case as RAS and LPS, one under all six axis
permutations, one oblique).

Bounds. Trilinear: the kernel interpolates in fp64 and rounds once, so it is within 1 fp32 ulp of the restatement
rounded to fp32 (the fp64 evaluation error, about 1e-16 of the taps' magnitude, is far below half an fp32 ulp; only a
double rounding can move the last bit); bit-equal where every coordinate and value is exact (integer input at
r = 0.5) and on the identity plan, which returns its input. Nearest: exactly equal, every element type. Channels are
independent: channel c of a multi-channel call equals the single-channel call bit for bit."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import body_crop_cases as BK
import body_crop_reference as BR
import resample_cases as K
import resample_reference as R
from u3d import data
from u3d._lib import lib

pytestmark = pytest.mark.gpu


def _dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


@functools.lru_cache(maxsize=None)
def _plans(vid):
    _, shape, affine, pixdim, _ = K.VARIANTS[K.IDS.index(vid)]
    return data.spacing_plan(shape, affine, pixdim), R.plan(shape, affine, pixdim)


@functools.lru_cache(maxsize=None)
def _linear_reference(vid, inverse=False):
    _, ref = _plans(vid)
    if inverse:
        ref = R.inverse(ref)
        return R.sample_linear(K.image(ref["src_shape"], "probs", 3), ref)
    return R.sample_linear(K.image(ref["src_shape"]), ref), R.sample_linear(K.image_i16(ref["src_shape"]), ref)


def _within_one_ulp(got, want, what):
    got = got.cpu().numpy()
    assert got.dtype == np.float32 and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    w32 = want.astype(np.float32)
    nan = np.isnan(w32)                      # a NaN voxel of the source reaches the same outputs: the taps are the same
    assert np.array_equal(np.isnan(got), nan), what
    got, w32 = np.where(nan, np.float32(0), got), np.where(nan, np.float32(0), w32)
    ulps = np.abs(got.astype(np.float64) - w32.astype(np.float64)) / R.ulp32(w32)
    print(f"{what}: max {ulps.max():.3f} ulp, {np.count_nonzero(ulps)} of {ulps.size} voxels differ")
    assert ulps.max() <= 1.0, what


@pytest.mark.parametrize("vid", K.IDS)
def test_linear(gpu, vid):
    plan, ref = _plans(vid)
    want_f32, want_i16 = _linear_reference(vid)
    shape = ref["src_shape"]
    _within_one_ulp(plan.apply(_dev(K.image(shape), gpu)), want_f32, f"{vid} fp32")
    _within_one_ulp(plan.apply(_dev(K.image_i16(shape), gpu), "linear"), want_i16, f"{vid} int16")


@pytest.mark.parametrize("vid", K.IDS)
def test_nearest(gpu, vid):
    plan, ref = _plans(vid)
    lab = K.label(ref["src_shape"])
    want = R.sample_nearest(lab, ref)
    for dt in K.LABEL_DTYPES:
        got = plan.apply(_dev(lab.astype(dt), gpu), "nearest").cpu().numpy()
        assert got.dtype == np.dtype(dt) and np.array_equal(got, want.astype(dt)), (vid, dt)
    x = K.image(ref["src_shape"])                                  # arbitrary fp32 bits are copied, not converted
    got = plan.apply(_dev(x, gpu), "nearest").cpu().numpy()
    assert np.array_equal(got.view(np.uint32), R.sample_nearest(x, ref).view(np.uint32))


@pytest.mark.parametrize("vid", K.IDS)
def test_inverse_three_channels(gpu, vid):
    plan, ref = _plans(vid)
    inv, rinv = plan.inverse(), R.inverse(ref)
    x = K.image(rinv["src_shape"], "probs", 3)
    dx = _dev(x, gpu)
    got = inv.apply(dx)
    assert tuple(got.shape) == (3,) + ref["src_shape"]
    _within_one_ulp(got, _linear_reference(vid, True), f"{vid} inverse, 3 channels")
    near = inv.apply(dx, "nearest")
    assert np.array_equal(near.cpu().numpy().view(np.uint32), R.sample_nearest(x, rinv).view(np.uint32))
    for c in range(3):
        assert torch.equal(inv.apply(dx[c]).view(torch.int32), got[c].view(torch.int32)), (vid, c)
        assert torch.equal(inv.apply(dx[c], "nearest").view(torch.int32), near[c].view(torch.int32)), (vid, c)


def test_identity_and_exact_coordinates(gpu):
    ident = data.spacing_plan((4, 5, 6), K.affine_for("RAS", (1, 1, 2)))
    for x in (_dev(K.image((4, 5, 6)), gpu), _dev(K.image_i16((4, 5, 6)), gpu), _dev(K.image((4, 5, 6), "probs", 3), gpu)):
        assert ident.identity and ident.apply(x) is x and ident.apply(x, "nearest") is x
    shape, zooms, pixdim, expected = K.EXACT
    for codes in ("RAS", "LPS", K.PERMUTED[3]):
        affine = K.affine_for(codes, zooms)
        plan, ref = data.spacing_plan(shape, affine, pixdim), R.plan(shape, affine, pixdim)
        assert sorted(plan.out_shape) == sorted(expected) and plan.scale == (0.5, 0.5, 0.5)
        x = K.image_i16(shape)
        want = R.sample_linear(x, ref)
        assert np.array_equal(want, np.round(want * 8) / 8)                   # the case is exact: multiples of 1 / 8
        for src in (x, x.astype(np.float32)):
            got = plan.apply(_dev(src, gpu)).cpu().numpy()
            assert np.array_equal(got.view(np.uint32), want.astype(np.float32).view(np.uint32)), codes


@functools.lru_cache(maxsize=None)
def _case():
    """A body_crop case read as an LPS file with voxels of 0.8 x 1 x 1.6 mm: both axes 0 and 2 shrink by 0.8."""
    cid, mf, mfu, _ = BK.SMALL["hand"]
    _, img, lab = BK.case_inputs("hand")
    affine = K.affine_for("LPS", (0.8, 1.0, 1.6))
    ref = R.plan(img.shape, affine)
    r_img = R.sample_linear(img, ref).astype(np.float32)
    r_lab = R.sample_nearest(lab, ref)
    return cid, mf / 2, mfu / 2, img, lab, affine, ref, r_img, r_lab, BR.body_crop(r_img, r_lab, cid, mf / 2, mfu / 2)


def test_resample_spacing(gpu):
    cid, mf, mfu, img, lab, affine, ref, r_img, r_lab, _ = _case()
    got_img, got_lab, out_affine, plan = data.resample_spacing(_dev(img, gpu), _dev(lab, gpu), affine)
    assert tuple(got_img.shape) == ref["out_shape"] == tuple(got_lab.shape) == plan.out_shape
    assert np.array_equal(out_affine, ref["out_affine"]) and data.axcodes_of(out_affine) == "RAS"
    assert got_lab.dtype == torch.float32 and np.array_equal(got_lab.cpu().numpy(), r_lab)
    _within_one_ulp(got_img, R.sample_linear(img, ref), "resample_spacing image")
    i16 = np.rint(np.nan_to_num(img)).astype(np.int16)                       # raw CT as stored
    got16 = data.resample_spacing(_dev(i16, gpu), _dev(lab.astype(np.uint8), gpu), affine)
    assert got16[0].dtype == torch.float32 and got16[1].dtype == torch.uint8
    _within_one_ulp(got16[0], R.sample_linear(i16, ref), "resample_spacing int16 image")
    assert np.array_equal(got16[1].cpu().numpy(), r_lab.astype(np.uint8))


def test_preprocess_case(gpu):
    cid, mf, mfu, img, lab, affine, ref, r_img, r_lab, want = _case()
    w_image, w_label, w = want
    image_a, label_a, info = data.preprocess_case(_dev(img, gpu), _dev(lab, gpu), affine, cid, min_filter=mf,
                                                  min_filter_up=mfu)
    assert tuple(image_a.shape) == w_image.shape and tuple(label_a.shape) == w_label.shape
    assert np.array_equal(label_a.cpu().numpy(), w_label)
    _within_one_ulp(image_a, w_image.astype(np.float64), "preprocess_case image")
    for k in ("label_range", "bbox", "bbox_up", "size", "size_up", "route", "route_up", "inter_all", "inter_up",
              "found_hand"):
        assert info[k] == w[k], (k, info[k], w[k])
    assert np.array_equal(info["mask"].cpu().numpy(), w["mask"])
    assert float(info["label_sum_before"]) == w["label_sum_before"]
    assert float(info["label_sum_after"]) == w["label_sum_after"]
    assert np.array_equal(info["affine"], ref["out_affine"]) and info["spacing"] == (1, 1, 2)
    assert info["plan"].out_shape == ref["out_shape"] and info["plan"].inverse().out_shape == img.shape


def test_bad_arguments_launch_nothing(gpu):
    """U3D_EINVAL (1) for every argument the entry points can judge, before anything is queued: the output keeps its
    sentinel."""
    shape, zooms, pixdim, _ = K.CASES["half_coords"]
    plan = data.spacing_plan(shape, K.affine_for("LPS", zooms), pixdim)
    src = _dev(K.image(shape), gpu)
    tabs = plan._device_tables(src.device)
    out = torch.full(plan.out_shape, -7.0, dtype=torch.float32, device=gpu)
    st, sn, chan = plan.source_layout()
    A3, L3 = ctypes.c_int * 3, ctypes.c_longlong * 3
    h = lib()

    def args(**kw):
        a = dict(src=src.data_ptr(), dtype=data.RS_F32, C=1, stride=L3(*st), chan=chan, src_n=A3(*sn),
                 n_out=A3(*plan.out_shape), t0=tabs[0][0].data_ptr(), t1=tabs[1][0].data_ptr(), t2=tabs[2][0].data_ptr(),
                 f0=tabs[0][1].data_ptr(), f1=tabs[1][1].data_ptr(), f2=tabs[2][1].data_ptr(), out=out.data_ptr())
        a.update(kw)
        return a

    def linear(**kw):
        a = args(**kw)
        return h.u3d_grid_resample_linear(a["src"], a["dtype"], a["C"], a["stride"], a["chan"], a["src_n"], a["n_out"],
                                          a["t0"], a["t1"], a["t2"], a["f0"], a["f1"], a["f2"], a["out"], None)

    def nearest(**kw):
        a = args(**kw)
        return h.u3d_grid_resample_nearest(a["src"], a["dtype"], a["C"], a["stride"], a["chan"], a["src_n"], a["n_out"],
                                           a["t0"], a["t1"], a["t2"], a["out"], None)

    bad = [dict(src=None), dict(out=None), dict(C=0), dict(C=-1), dict(chan=-1), dict(stride=None), dict(src_n=None),
           dict(n_out=None), dict(n_out=A3(7, 0, 4)), dict(n_out=A3(65536, 65536, 1)), dict(src_n=A3(4, 5, 0)),
           dict(stride=L3(30, 0, 1)), dict(stride=L3(-30, 6, 1)), dict(t1=None), dict(dtype=7), dict(dtype=-1)]
    for kw in bad:
        assert linear(**kw) == 1, kw
        assert nearest(**kw) == 1, kw
    for kw in (dict(f2=None), dict(dtype=data.RS_U8), dict(dtype=data.RS_I32)):      # linear reads fp32 or int16 only
        assert linear(**kw) == 1, kw
    assert b"grid_resample" in h.u3d_last_error()
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    assert linear() == 0                                                             # the same arguments, unbroken
    torch.cuda.synchronize()
    assert bool((out != -7.0).all())
    with pytest.raises(ValueError):
        plan.apply(src.double(), "nearest")
    with pytest.raises(ValueError):
        plan.apply(src[:, :, :5])
