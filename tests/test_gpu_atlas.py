"""csrc/atlas.hip kernel by kernel: u3d_atlas_crop (atlas_crop_kernel) against the reference's own lines
(tests/golden/g19_atlas.npz) and against crop_transpose of the float64-CPU-resized atlas; u3d_select_probs_fwd / _bwd
(select_probs_fwd_kernel<NC>, select_probs_bwd_kernel<NC>) and u3d_dice_metric_atlas (dice_atlas_count_kernel<NC> +
loss.hip's dice_final_kernel) against the fp64 references of atlas_reference.py. The C entry points are called through
u3d._lib on buffers the test allocates, outputs pre-filled with NaN (integers with -7), and every element is compared;
the Python entry points (u3d.data, utils, evaluate_amos) are then checked against the same references. Cases, inputs and
bound functions live in atlas_cases.py; test_atlas_reference.py asserts the cases' input conditions on the CPU.

Bounds: worst-case counts of the fp32 roundings in the code, u = 2^-24, times magnitudes of the fp64 reference only, all
inflated by SLACK = 1 + 2^-10 (the conventions of test_gpu_loss.py, whose lines are quoted).

crop      a gather: bit-exact. The source index is an integer expression; nothing rounds.
softmax   (test_gpu_loss.py's "softmax" line in its libm form, as its "consist" line takes it for softmax_row)
          x = lg - m rounds once (u |x|) and libm expf is taken at 1 ulp = 2 u: e is off by ee = (|x| + 2) u;
          s = sum e by es = (C - 1) u + sum_c p_c ee_c; p = e / s, the division taken like the rcp-and-multiply of that
          line: ep = ee + es + 3 u. out[k][0] = p[first + index[k]]: |err| <= p ep.
atlas     out[k][1] is a copy: bit-exact.
gradient  (the "dot / r" part of the "backward" line) G_c sums the rows of class c in ascending k in fp32:
          dG = (rows - 1) u sum |g|, 0 without duplicates. dot = sum_c G_c p_c by C fmas:
          ddot = sum (dG p + |G p| ep) + C u sum |G p|;  r = p (G - dot): |r| (ep + 2 u) + p (dG + ddot).
gated     under the cases' condition (every fp64 margin |p + 0.15 - (1 - a)| >= 1e-3, about 1000 x the fp32 error of
          the two sides) the gate, hence every count, is exact; the argmax is exact (top-2 logit gap > 1e-5).
metrics   dice_final_kernel, test_gpu_loss.py's "metrics" line: (S + 5) u |metric|. Against the fixture (the
          reference's own fp32 ratios from the same counts) twice that: each side rounds on its own.
sum       the end-to-end check: autograd adds the loss gradient and the pair gradient in fp32, one rounding:
          u |g_loss + g_pairs|.

Every test prints its worst error as a share of the bound ("SHARE <family> <value>") before asserting.
"""
import ctypes

import numpy as np
import pytest
import torch

import atlas_cases as K
import atlas_reference as R
from atlas_cases import SLACK, U
from conftest import golden

pytestmark = pytest.mark.gpu

f32, f64, i64 = torch.float32, torch.float64, torch.int64


def _share(name, err, bound):
    err, bound = torch.as_tensor(err), torch.as_tensor(bound)
    assert bool(torch.isfinite(err).all()), f"{name}: an element was not written or is not finite"
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


def _nan(shape, dev, dtype=f32):
    return torch.full(shape, float("nan"), dtype=dtype, device=dev)


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


# ------------------------------------------------------------------------------------------------ resize-in-crop
def _out_hw(tag):
    _, ishape, (cd, ch, cw), usage, _ = K.CROP_CASES[tag]
    return (ch, cw, cd) if usage == "train" else K.padded_shape(ishape, (cd, ch, cw))


@pytest.mark.parametrize("tag", list(K.CROP_CASES))
def test_atlas_crop_kernel_vs_fixture(gpu, tag):
    g = golden("g19_atlas.npz")
    ashape, ishape, crop, usage, seed = K.CROP_CASES[tag]
    atlas, _, _ = K.crop_inputs(tag)
    want = torch.from_numpy(g[f"crop_{tag}_catlas"])
    b, c, a = [int(v) for v in g[f"crop_{tag}_draws"]] if usage == "train" else (0, 0, 0)
    ch, cw, cd = _out_hw(tag)
    da = torch.from_numpy(atlas.astype(np.float32)).to(gpu)        # k / 64: the cast is exact
    out = _nan((ashape[0], cd, ch, cw), gpu)
    _L().call("u3d_atlas_crop", da.data_ptr(), *ashape, *ishape, b, c, a, ch, cw, cd, out.data_ptr(), _stream())
    torch.cuda.synchronize()
    assert out.shape == want.shape and torch.equal(_bits(out), _bits(want))
    if usage == "valid":
        assert all(bool((z == 0).all()) for z in (out[:, ishape[2]:], out[:, :, ishape[0]:], out[..., ishape[1]:]))
    print(f"SHARE atlas-crop {tag} 0.0000")


@pytest.mark.parametrize("dtype", [np.float64, np.float32], ids=["atlas-f64", "atlas-f32"])
@pytest.mark.parametrize("tag", list(K.CROP_CASES))
def test_crop_patch_with_raw_atlas(gpu, tag, dtype):
    """crop_patch(atlas=raw) draws and returns what crop_patch(catlas=the float64-CPU-resized atlas) does, bit for bit,
    and its atlas output is the fixture's (MOTSDataset.py:357-392 on the float64 atlas)."""
    from u3d import data
    g = golden("g19_atlas.npz")
    ashape, ishape, crop, usage, seed = K.CROP_CASES[tag]
    atlas, image, label = K.crop_inputs(tag)
    dimg = torch.from_numpy(image.astype(np.float32)).to(gpu)
    dlab = torch.from_numpy(label.astype(np.float32)).to(gpu)
    resized = torch.from_numpy(R.interpolate_f64(atlas, ishape).astype(np.float32)).to(gpu)
    assert tuple(resized.shape) == tuple(int(v) for v in g[f"crop_{tag}_resized_shape"])

    class Rec:
        def __init__(self):
            self.rs, self.draws = np.random.RandomState(seed), []

        def randint(self, *a):
            self.draws.append(int(self.rs.randint(*a)))
            return self.draws[-1]
    r0, r1 = Rec(), Rec()
    wi, wl, wc = data.crop_patch(dimg, dlab, resized, K.NAME, crop, usage=usage, rng=r0)
    gi, gl, gc = data.crop_patch(dimg, dlab, None, K.NAME, crop, usage=usage, rng=r1,
                                 atlas=torch.from_numpy(atlas.astype(dtype)).to(gpu))
    assert r0.draws == r1.draws == g[f"crop_{tag}_draws"].tolist()
    for got, want in ((gi, wi), (gl, wl), (gc, wc)):
        assert got.shape == want.shape and got.dtype == f32 and torch.equal(_bits(got), _bits(want))
    assert torch.equal(_bits(gc), _bits(torch.from_numpy(g[f"crop_{tag}_catlas"])))
    off = tuple(r1.draws) if usage == "train" else (0, 0, 0)
    direct = data.atlas_crop(torch.from_numpy(atlas).to(gpu), ishape, off, _out_hw(tag))
    assert torch.equal(_bits(direct), _bits(data.crop_transpose(resized, off, _out_hw(tag))))


# ------------------------------------------------------------------------------------------------ organ / atlas pairs
def _strides(lg):
    from u3d.loss import _voxel_strides
    t, (_, lsc, lsv) = _voxel_strides(lg, 2)
    assert t.data_ptr() == lg.data_ptr()          # read in place: no copy for either layout
    return lsc, lsv


@pytest.mark.parametrize("layout", K.LAYOUTS)
@pytest.mark.parametrize("geom", K.PAIR_GEOM, ids=K.case_id)
def test_select_probs_kernels(gpu, geom, layout):
    C, sp, first, with_atlas = geom
    lg, atlas = K.pair_inputs(geom)
    n, V = C - first, sp[0] * sp[1] * sp[2]
    dlg = K.as_layout(lg, layout, gpu)
    lsc, lsv = _strides(dlg)
    assert V == 1 or (lsc, lsv) == ((V, 1) if layout == "ncdhw" else (1, C))   # (one voxel: either stride serves)
    dat = atlas.reshape(n, V).to(gpu) if with_atlas else None
    flat = dlg.reshape(C, V) if layout == "ncdhw" else dlg.permute(0, 2, 3, 4, 1).reshape(V, C).t()
    for name, index in K.pair_indices(n).items():
        if not index:
            continue                                  # the empty list never reaches the library (the wrapper's test)
        Kn, nch = len(index), 2 if with_atlas else 1
        gout = K.pair_grad(Kn, nch, sp, 5 + Kn).reshape(Kn, nch, V).to(gpu)
        ref = R.select_probs_ref(flat, first, index, dat, gout)
        b_out, b_dl = K.select_bounds(ref)
        idx = (ctypes.c_int * Kn)(*index)
        out = _nan((Kn, nch, V), gpu)
        _L().call("u3d_select_probs_fwd", dlg.data_ptr(), lsc, lsv, C, V, first, idx, Kn,
                  dat.data_ptr() if with_atlas else None, n if with_atlas else 0, out.data_ptr(), _stream())
        dl = K.as_layout(torch.full(lg.shape, float("nan")), layout, gpu)
        _L().call("u3d_select_probs_bwd", dlg.data_ptr(), lsc, lsv, C, V, first, idx, Kn, gout.data_ptr(), nch,
                  dl.data_ptr(), _stream())
        torch.cuda.synchronize()
        tag = f"{K.case_id(geom)} {layout} {name}"
        assert _share(f"select-fwd {tag}", (out[:, 0].double() - ref.out[:, 0]).abs(), SLACK * b_out) <= 1
        if with_atlas:
            assert torch.equal(_bits(out[:, 1]), _bits(dat[index]))
        assert dl.stride() == dlg.stride()
        assert _share(f"select-bwd {tag}", (dl.reshape(C, V).double() - ref.dl).abs(), SLACK * b_dl) <= 1


@pytest.mark.parametrize("layout", K.LAYOUTS)
def test_pair_helpers_vs_driver_expression(gpu, layout):
    """utils.organ_atlas_pairs / attention_pairs against the driver's torch lines on the device: values within the
    forward bound of the fp64 reference, the atlas channel bit-exact, gradients through autograd within the backward
    bound and in the logits' own strides; empty index, tensor index, negative index, float64 atlas."""
    import utils
    geom = K.PAIR_GEOM[0]
    C, sp, first, _ = geom
    lg, atlas = K.pair_inputs(geom)
    V, n = sp[0] * sp[1] * sp[2], C - 1
    dat = atlas.to(gpu)
    for name, index in K.pair_indices(n).items():
        x = K.as_layout(lg, layout, gpu).requires_grad_(True)
        got = utils.organ_atlas_pairs(x, dat, index)
        assert got.shape == (len(index), 2) + sp and got.dtype == f32 and got.is_contiguous()
        if not index:
            assert got.numel() == 0 and not got.requires_grad
            continue
        want = torch.cat([torch.softmax(x.detach().double(), 1)[0, 1:].unsqueeze(1), dat.double().unsqueeze(1)], 1)[index]
        gout = K.pair_grad(len(index), 2, sp, 5 + len(index)).to(gpu)
        flat = x.detach().reshape(C, V) if layout == "ncdhw" else x.detach().permute(0, 2, 3, 4, 1).reshape(V, C).t()
        ref = R.select_probs_ref(flat, 1, index, dat.reshape(n, V), gout.reshape(len(index), 2, V))
        b_out, b_dl = K.select_bounds(ref)
        assert (ref.out.reshape(want.shape) - want).abs().max().item() < 1e-14     # the driver's lines, in fp64
        assert _share(f"pairs-fwd {layout} {name}", (got[:, 0].double() - want[:, 0]).abs().reshape(len(index), V),
                      SLACK * b_out) <= 1
        assert torch.equal(_bits(got[:, 1]), _bits(dat[index]))
        (got * gout).sum().backward()
        assert x.grad.stride() == x.stride()
        assert _share(f"pairs-bwd {layout} {name}", (x.grad.reshape(C, V).double() - ref.dl).abs(), SLACK * b_dl) <= 1
    x = K.as_layout(lg, layout, gpu)
    a = utils.organ_atlas_pairs(x, dat, [2, 12, 5])
    assert torch.equal(a, utils.organ_atlas_pairs(x, dat.double(), torch.tensor([2, -1, 5])))
    assert not a.requires_grad
    d2 = dat.clone().requires_grad_(True)                       # the atlas gets no gradient
    utils.organ_atlas_pairs(K.as_layout(lg, layout, gpu).requires_grad_(True), d2, [1]).sum().backward()
    assert d2.grad is None
    with pytest.raises(IndexError):
        utils.organ_atlas_pairs(x, dat, [13])
    with pytest.raises(RuntimeError):
        utils.organ_atlas_pairs(x, dat[:12], [0])
    # attention maps: 13 organ channels at a reduced resolution, first = 0, one channel
    ag = K.PAIR_GEOM[2]
    att, _ = K.pair_inputs(ag)
    xa = K.as_layout(att, layout, gpu).requires_grad_(True)
    index = K.pair_indices(13)["dup"]
    got = utils.attention_pairs(xa, index)
    want = torch.softmax(xa.detach().double(), 1)[0][index].unsqueeze(1)
    Va = ag[1][0] * ag[1][1] * ag[1][2]
    flat = xa.detach().reshape(13, Va) if layout == "ncdhw" else xa.detach().permute(0, 2, 3, 4, 1).reshape(Va, 13).t()
    gout = K.pair_grad(len(index), 1, ag[1], 3).to(gpu)
    ref = R.select_probs_ref(flat, 0, index, None, gout.reshape(len(index), 1, Va))
    b_out, b_dl = K.select_bounds(ref)
    assert got.shape == want.shape
    assert _share(f"attention-fwd {layout}", (got.double() - want).abs().reshape(len(index), Va), SLACK * b_out) <= 1
    (got * gout).sum().backward()
    assert _share(f"attention-bwd {layout}", (xa.grad.reshape(13, Va).double() - ref.dl).abs(), SLACK * b_dl) <= 1
    assert utils.attention_pairs(xa, []).shape == (0, 1) + ag[1]


@pytest.mark.parametrize("layout", K.LAYOUTS)
def test_loss_and_pairs_one_backward(gpu, layout):
    """logits.requires_grad, EDiceLoss_partial(14) plus a weighted sum of organ_atlas_pairs, one backward(): the
    gradient is the sum of the two gradients taken separately (one fp32 add per element)."""
    import utils
    from loss_functions.loss_partial import EDiceLoss_partial
    geom = K.PAIR_GEOM[0]
    C, sp, _, _ = geom
    lg, atlas = K.pair_inputs(geom)
    assert (1, C) + sp == (1, 14, 6, 10, 12)
    gen = torch.Generator().manual_seed(11)
    labels = torch.randint(0, C, (1,) + sp, generator=gen).float().to(gpu)
    index = K.pair_indices(C - 1)["dup"]
    w = torch.randn((len(index), 2) + sp, generator=gen).to(gpu)
    dat = atlas.to(gpu)
    crit = EDiceLoss_partial(C)

    def grad(use_loss, use_pairs):
        x = K.as_layout(lg, layout, gpu).requires_grad_(True)
        total = 0
        if use_loss:
            total = total + crit(x, labels)
        if use_pairs:
            total = total + (utils.organ_atlas_pairs(x, dat, index) * w).sum()
        total.backward()
        if not use_loss:
            assert x.grad.stride() == x.stride()
        return x.grad.double()
    both, g_loss, g_pairs = grad(True, True), grad(True, False), grad(False, True)
    assert g_loss.abs().max().item() > 0 and g_pairs.abs().max().item() > 0
    want = g_loss + g_pairs
    assert _share(f"loss+pairs {layout}", (both - want).abs(), SLACK * U * want.abs()) <= 1


# ------------------------------------------------------------------------------------------------ atlas-gated Dice
@pytest.mark.parametrize("want_argmax", [True, False], ids=["argmax", "no-argmax"])
@pytest.mark.parametrize("case", K.DICE_CASES, ids=K.case_id)
def test_dice_metric_atlas_kernel(gpu, case, want_argmax):
    S, C, ncls, sp = case
    lg, lab, atlas = (t.to(gpu) for t in K.dice_flat(case))
    V, A = lg.shape[1], atlas.shape[1]
    ref = R.dice_atlas_ref(lg, lab, atlas, ncls)
    assert ref.margin.abs().min().item() >= K.MARGIN
    counts = torch.full((S, ncls, 3), -7, dtype=i64, device=gpu)
    metrics = _nan((ncls, 3), gpu)
    am = torch.full((S, V), -7, dtype=i64, device=gpu) if want_argmax else None
    _L().call("u3d_dice_metric_atlas", lg.data_ptr(), lab.data_ptr(), atlas.data_ptr(), A, S, V, C, ncls,
              counts.data_ptr(), metrics.data_ptr(), am.data_ptr() if want_argmax else None, _stream())
    torch.cuda.synchronize()
    assert torch.equal(counts, ref.counts)
    if want_argmax:
        assert torch.equal(am, ref.argmax)
    assert _share(f"dice-atlas {K.case_id(case)}", (metrics.double() - ref.metrics).abs(),
                  SLACK * K.metric_bound(ref.metrics, S)) <= 1


@pytest.mark.parametrize("case", K.DICE_FIXTURE, ids=K.case_id)
def test_get_dice_with_atlas_vs_reference_fixture(gpu, case):
    import evaluate_amos
    g = golden("g19_atlas.npz")
    S, C, ncls, sp = case
    preds, lab, atlas = (t.to(gpu) for t in K.dice_inputs(case))
    key = "dice_" + K.case_id(case)
    want = torch.from_numpy(np.stack([g[f"{key}_dice"], g[f"{key}_senc"], g[f"{key}_spec"]], 1)).to(gpu)
    ref = R.dice_atlas_ref(*(t.to(gpu) for t in K.dice_flat(case)), ncls)
    for fn, at in ((evaluate_amos.get_dice, atlas), (evaluate_amos.get_dice, atlas.double()),
                   (evaluate_amos.get_dice2, atlas)):
        if fn is evaluate_amos.get_dice2 and C == 2:
            continue
        dices, senc, spec, am = fn(preds, lab, 1, at, num_class=ncls)
        assert len(dices) == len(senc) == len(spec) == ncls and all(d.dim() == 0 for d in dices)
        got = torch.stack([torch.stack(dices), torch.stack(senc), torch.stack(spec)], 1).double()
        bound = SLACK * K.metric_bound(ref.metrics, S)
        assert _share(f"get_dice-atlas {K.case_id(case)}", (got - ref.metrics).abs(), bound) <= 1
        assert _share(f"get_dice-atlas-fixture {K.case_id(case)}", (got - want).abs(), 2 * bound) <= 1
        assert am.shape == (S,) + sp and torch.equal(am.cpu(), torch.from_numpy(g[f"{key}_argmax"].astype(np.int64)))
    plain = evaluate_amos.get_dice(preds, lab, 1, num_class=ncls)
    assert torch.equal(plain[3], am)                      # the same argmax map as the atlas=None branch


def test_get_dice2_with_atlas_on_refiner_layout_raises_like_the_reference(gpu):
    import evaluate_amos
    ref_out = torch.zeros(13, 2, 2, 3, 4, device=gpu)
    with pytest.raises(IndexError):       # preds_r[:, l + 1] at l = 1 on 2 channels
        evaluate_amos.get_dice2(ref_out, torch.zeros(1, 2, 3, 4, device=gpu), 1,
                                torch.zeros(13, 13, 2, 3, 4, device=gpu), num_class=13)
