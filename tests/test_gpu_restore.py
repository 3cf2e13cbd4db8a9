"""The way back from the network's output to a label map on the case's own voxels, on the device:
GridPlan.apply_argmax (u3d_grid_resample_argmax), body_crop's origin / input_shape and restore_prediction, on the inverse
plans of resample_cases.VARIANTS restricted to four boxes each (the whole resampled grid, an interior box, a box touching
the high border, a box from the low corner; the largest volume is 5 x 7 x 174). Inputs are
resample_cases.image(box shape, "probs", C).

Everything is compared exactly. The fused kernel evaluates each channel with the routine the linear kernel uses and
rounds it as that kernel does, so it equals the argmax over the linear kernel's output bit for bit, ties and NaNs
included. Against the numpy float64 restatement the argmax can only differ where fp32 rounding reorders the two largest
channels; the test asserts first that no voxel's two largest values are within 2 fp32 ulp of each other (so rounding
each to fp32, half an ulp at most, cannot reorder them), and then compares every voxel."""
import ctypes
import functools

import numpy as np
import pytest
import torch

import body_crop_cases as BK
import resample_cases as K
import resample_reference as R
from u3d import data
from u3d._lib import lib

pytestmark = pytest.mark.gpu

CHANNELS = (1, 2, 14)
BOXES = ("whole", "interior", "high", "low")


def _dev(a, gpu):
    return torch.from_numpy(np.ascontiguousarray(a)).to(gpu)


def _box(S, name):
    """(origin, shape) inside a grid of shape S; an axis too short for an interior keeps what it has."""
    return {"whole": ((0, 0, 0), tuple(S)),
            "interior": (tuple(min(1, s - 1) for s in S), tuple(max(1, s - 2) for s in S)),
            "high": (tuple(s // 2 for s in S), tuple(s - s // 2 for s in S)),
            "low": ((0, 0, 0), tuple(max(1, s // 2) for s in S))}[name]


@functools.lru_cache(maxsize=None)
def _plans(vid):
    _, shape, affine, pixdim, _ = K.VARIANTS[K.IDS.index(vid)]
    return data.spacing_plan(shape, affine, pixdim).inverse(), R.inverse(R.plan(shape, affine, pixdim))


@functools.lru_cache(maxsize=None)
def _restricted(vid, box):
    """(plan_w, valid, reference plan of the crop, mask of the valid output voxels)."""
    inv, rinv = _plans(vid)
    origin, shape = _box(inv.src_shape, box)
    plan_w, valid = inv.restrict_source(origin, shape)
    rw = dict(rinv, src_shape=shape, offset=tuple(rinv["offset"][i] - origin[rinv["perm"][i]] for i in range(3)))
    mask = np.ones(inv.out_shape, dtype=bool)
    for i, (lo, hi) in enumerate(valid):
        k = np.arange(inv.out_shape[i])
        mask &= ((k >= lo) & (k < hi)).reshape([-1 if d == i else 1 for d in range(3)])
    mask.setflags(write=False)
    return plan_w, valid, rw, mask


def _composed(plan_w, mask, x):
    """The path the fused kernel replaces: the C resampled volumes, their argmax, the mask."""
    lin = plan_w.apply(x, "linear")
    assert lin.dtype == torch.float32
    am = lin.argmax(0).to(torch.uint8)
    return torch.where(torch.from_numpy(mask).to(x.device), am, torch.zeros_like(am))


@pytest.mark.parametrize("vid", K.IDS)
def test_apply_argmax_is_the_argmax_of_the_linear_kernel(gpu, vid):
    for box in BOXES:
        plan_w, valid, _, mask = _restricted(vid, box)
        for C in CHANNELS:
            x = _dev(K.image(plan_w.src_shape, "probs", C), gpu)
            want = _composed(plan_w, mask, x)
            got = plan_w.apply_argmax(x, valid)
            assert got.dtype == torch.uint8 and tuple(got.shape) == plan_w.out_shape
            assert torch.equal(got, want), (vid, box, C)
            # a permuted view of a channel-last tensor: read through its strides, no copy
            view = x.permute(1, 2, 3, 0).contiguous().permute(3, 0, 1, 2)
            assert view.shape == x.shape and (C == 1 or min(plan_w.src_shape) == 1 or not view.is_contiguous())
            assert torch.equal(plan_w.apply_argmax(view, valid), want), (vid, box, C, "view")
        if box == "whole":                                        # valid=None: everything is valid
            assert mask.all() and torch.equal(plan_w.apply_argmax(x), want)


@functools.lru_cache(maxsize=None)
def _restatement(vid, box, C):
    """(argmax of the float64 restatement masked by valid, voxels whose two largest values are within 2 fp32 ulp)."""
    plan_w, valid, rw, mask = _restricted(vid, box)
    v = R.sample_linear(K.image(plan_w.src_shape, "probs", C), rw)
    close = 0
    if C > 1:
        top = np.sort(v, axis=0)[-2:]
        close = int(np.count_nonzero((top[1] - top[0] <= 2 * R.ulp32(np.maximum(np.abs(top[0]), np.abs(top[1])))) & mask))
    return np.where(mask, np.argmax(v, axis=0), 0).astype(np.uint8), close, int(mask.sum())


@pytest.mark.parametrize("vid", K.IDS)
def test_apply_argmax_is_the_float64_restatement(gpu, vid):
    voxels = 0
    for box in BOXES:
        plan_w, valid, _, _ = _restricted(vid, box)
        for C in CHANNELS:
            want, close, n = _restatement(vid, box, C)
            assert close == 0, (vid, box, C, close)               # the precondition: no voxel is exempt below
            got = plan_w.apply_argmax(_dev(K.image(plan_w.src_shape, "probs", C), gpu), valid)
            assert np.array_equal(got.cpu().numpy(), want), (vid, box, C)
            voxels += n
    print(f"{vid}: {voxels} valid voxels compared, none within 2 ulp")


@pytest.mark.parametrize("vid", ["half_even_clamp-LPS", "half_coords-" + K.PERMUTED[3], "amos_like-oblique"])
def test_ties_and_nans_follow_torch_argmax(gpu, vid):
    plan_w, valid, _, mask = _restricted(vid, "interior")
    x = K.image(plan_w.src_shape, "probs", 14).copy()
    x[9], x[5] = x[2], x[2]                                        # three holders of one value
    dup = _dev(x, gpu)
    got = plan_w.apply_argmax(dup, valid)
    assert torch.equal(got, _composed(plan_w, mask, dup))
    assert int((got == 2).sum()) > 0 and int((got == 5).sum()) == 0 and int((got == 9).sum()) == 0
    two = torch.stack([dup[0], dup[0]])
    assert int(plan_w.apply_argmax(two, valid).sum()) == 0         # every voxel a tie: channel 0
    g = np.random.default_rng([35, K.IDS.index(vid)])
    x = K.image(plan_w.src_shape, "probs", 14).copy()
    x.reshape(-1)[g.integers(0, x.size, max(4, x.size // 150))] = np.float32("nan")
    for c in (3, 7):                                               # two channels that are often NaN together
        x[c][g.random(x.shape[1:]) < 0.15] = np.float32("nan")
    nan = _dev(x, gpu)
    lin = plan_w.apply(nan, "linear")
    hit = torch.isnan(lin).any(0) & torch.from_numpy(mask).to(gpu)
    assert int(hit.sum()) > 0 and int(torch.isnan(lin).sum(0).max()) > 1          # some voxels hold several NaNs
    got = plan_w.apply_argmax(nan, valid)
    assert torch.equal(got, _composed(plan_w, mask, nan))
    first_nan = torch.isnan(lin).to(torch.uint8).argmax(0).to(torch.uint8)         # the first NaN wins
    assert torch.equal(got[hit], first_nan[hit])


def test_identity_plan_pastes_the_channel_argmax_into_the_box(gpu):
    shape = (6, 9, 70)
    ident = data.spacing_plan(shape, K.affine_for("RAS", (1, 1, 2)))
    assert ident.identity and ident.inverse().identity
    for origin, box in (((0, 0, 0), shape), ((1, 2, 3), (4, 5, 66)), ((2, 0, 69), (4, 9, 1))):
        pred = _dev(K.image(box, "probs", 14), gpu)
        got = data.restore_prediction(pred, {"plan": ident, "origin": origin})
        want = torch.zeros(shape, dtype=torch.uint8, device=gpu)
        want[tuple(slice(o, o + s) for o, s in zip(origin, box))] = pred.argmax(0).to(torch.uint8)
        assert got.dtype == torch.uint8 and torch.equal(got, want), (origin, box)
    x = _dev(K.image(shape, "probs", 3), gpu)
    assert torch.equal(ident.apply_argmax(x), x.argmax(0).to(torch.uint8))
    assert torch.equal(ident.apply_argmax(x.double()), x.argmax(0).to(torch.uint8))  # other float dtypes are cast


@pytest.mark.parametrize("vid", K.IDS)
def test_label_map_goes_through_the_nearest_kernel(gpu, vid):
    _, shape, affine, pixdim, _ = K.VARIANTS[K.IDS.index(vid)]
    plan = data.spacing_plan(shape, affine, pixdim)
    rinv = _plans(vid)[1]
    for box in BOXES:
        origin, bshape = _box(plan.out_shape, box)
        lab = K.label(bshape)
        padded = np.zeros(plan.out_shape, dtype=np.uint8)
        padded[tuple(slice(o, o + s) for o, s in zip(origin, bshape))] = lab
        want = R.sample_nearest(padded, rinv)
        for dt in (torch.uint8, torch.int16, torch.int32, torch.int64):
            got = data.restore_prediction(_dev(lab, gpu).to(dt), {"plan": plan, "origin": origin})
            assert got.dtype == torch.uint8 and tuple(got.shape) == plan.src_shape
            assert np.array_equal(got.cpu().numpy(), want), (vid, box, dt)


@pytest.mark.parametrize("name", list(BK.SMALL))
def test_body_crop_records_where_the_crop_sits(gpu, name):
    cid, mf, mfu, _ = BK.SMALL[name]
    _, img, lab = BK.case_inputs(name)
    image, label = _dev(img, gpu), _dev(lab, gpu)
    image_a, label_a, info = data.body_crop(image, label, cid, mf, mfu)
    o = info["origin"]
    assert info["input_shape"] == img.shape and len(o) == 3 and all(isinstance(v, int) for v in o)
    box = tuple(slice(a, a + n) for a, n in zip(o, image_a.shape))
    assert all(a >= 0 and a + n <= s for a, n, s in zip(o, image_a.shape, img.shape))
    assert torch.equal(image_a.view(torch.int32), image[box].view(torch.int32))    # bits: the NaN voxel too
    cleared = torch.where(label >= 14, torch.zeros_like(label), label)
    assert torch.equal(label_a, cleared[box])
    assert (name in ("hand", "fallback_both_hand")) == info["found_hand"]


@functools.lru_cache(maxsize=None)
def _case():
    """The preprocess_case case of test_gpu_resample.py: a body_crop case read as an LPS file with voxels of
    0.8 x 1 x 1.6 mm."""
    cid, mf, mfu, _ = BK.SMALL["hand"]
    _, img, lab = BK.case_inputs("hand")
    return cid, mf / 2, mfu / 2, img, lab, K.affine_for("LPS", (0.8, 1.0, 1.6))


def test_preprocess_case_origin_and_restore_end_to_end(gpu):
    cid, mf, mfu, img, lab, affine = _case()
    image, label = _dev(img, gpu), _dev(lab, gpu)
    image_a, label_a, info = data.preprocess_case(image, label, affine, cid, min_filter=mf, min_filter_up=mfu)
    plan, o = info["plan"], info["origin"]
    assert info["input_shape"] == plan.out_shape
    box = tuple(slice(a, a + n) for a, n in zip(o, image_a.shape))
    resampled = plan.apply(image, "linear")
    assert torch.equal(image_a.view(torch.int32), resampled[box].view(torch.int32))
    # scores on image_a's grid -> a label map on the file's own voxels, against the composed device path
    logits = _dev(K.image(tuple(image_a.shape), "probs", 14), gpu)
    plan_w, valid = plan.inverse().restrict_source(o, image_a.shape)
    mask = torch.ones(plan.src_shape, dtype=torch.bool, device=gpu)
    for i, (lo, hi) in enumerate(valid):
        k = torch.arange(plan.src_shape[i], device=gpu)
        mask &= ((k >= lo) & (k < hi)).reshape([-1 if d == i else 1 for d in range(3)])
    print(f"origin {o}, crop {tuple(image_a.shape)} of {plan.out_shape}: {int(mask.sum())} of {mask.numel()} voxels valid")
    assert int(mask.sum()) > 0
    am = plan_w.apply(logits, "linear").argmax(0).to(torch.uint8)
    want = torch.where(mask, am, torch.zeros_like(am))
    got = data.restore_prediction(logits, info)
    assert got.dtype == torch.uint8 and tuple(got.shape) == img.shape and torch.equal(got, want)
    # a permuted view, as a channel-last network output would arrive
    view = logits.permute(1, 2, 3, 0).contiguous().permute(3, 0, 1, 2)
    assert torch.equal(data.restore_prediction(view, info), want)
    clean, rec = data.keep_largest_per_label(want, 13, return_record=True)
    assert torch.equal(data.restore_prediction(logits, info, cleanup=True), clean)
    assert int((clean != want).sum()) > 0 and bool((clean[clean != want] == 0).all())   # noise: many specks go
    # the label map route: label_a back onto the file's voxels equals the nearest kernel on the padded map
    lab8 = label_a.to(torch.uint8)
    padded = torch.zeros(plan.out_shape, dtype=torch.uint8, device=gpu)
    padded[box] = lab8
    back = data.restore_prediction(lab8, info)
    assert torch.equal(back, plan.inverse().apply(padded, "nearest")) and tuple(back.shape) == img.shape


def test_bad_arguments_launch_nothing(gpu):
    """U3D_EINVAL (1) for every argument the entry point can judge, before anything is queued: the output keeps its
    sentinel."""
    shape, zooms, pixdim, _ = K.CASES["half_coords"]
    inv = data.spacing_plan(shape, K.affine_for("LPS", zooms), pixdim).inverse()
    src = _dev(K.image(inv.src_shape, "probs", 2), gpu)
    tabs = inv._device_tables(src.device)
    out = torch.full(inv.out_shape, 77, dtype=torch.uint8, device=gpu)
    st, sn, chan = inv.source_layout()
    A3, L3 = ctypes.c_int * 3, ctypes.c_longlong * 3
    h = lib()

    def run(**kw):
        a = dict(src=src.data_ptr(), C=2, stride=L3(*st), chan=chan, src_n=A3(*sn), n_out=A3(*inv.out_shape),
                 t0=tabs[0][0].data_ptr(), t1=tabs[1][0].data_ptr(), t2=tabs[2][0].data_ptr(),
                 f0=tabs[0][1].data_ptr(), f1=tabs[1][1].data_ptr(), f2=tabs[2][1].data_ptr(),
                 lo=A3(0, 0, 0), hi=A3(*inv.out_shape), out=out.data_ptr())
        a.update(kw)
        return h.u3d_grid_resample_argmax(a["src"], a["C"], a["stride"], a["chan"], a["src_n"], a["n_out"], a["t0"],
                                          a["t1"], a["t2"], a["f0"], a["f1"], a["f2"], a["lo"], a["hi"], a["out"], None)

    for kw in (dict(src=None), dict(out=None), dict(C=0), dict(C=257), dict(chan=-1), dict(stride=None),
               dict(src_n=None), dict(n_out=None), dict(n_out=A3(7, 0, 4)), dict(src_n=A3(4, 5, 0)),
               dict(stride=L3(30, 0, 1)), dict(t1=None), dict(f2=None), dict(lo=None), dict(hi=None)):
        assert run(**kw) == 1, kw
    assert b"grid_resample_argmax" in h.u3d_last_error()
    torch.cuda.synchronize()
    assert bool((out == 77).all())
    assert run(lo=A3(0, 0, 0), hi=A3(0, 0, 0)) == 0                # an empty range: zeros, nothing read
    torch.cuda.synchronize()
    assert bool((out == 0).all())
    assert run() == 0
    torch.cuda.synchronize()
    assert torch.equal(out, inv.apply(src, "linear").argmax(0).to(torch.uint8))
