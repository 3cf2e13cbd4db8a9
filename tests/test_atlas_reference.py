"""The references of atlas_reference.py against the reference's own outputs (tests/golden/g19_atlas.npz, written by
tests/golden/gen_golden_atlas.py), the nearest-index sweep, and the input conditions of every case of atlas_cases.py that
test_gpu_atlas.py relies on. No device."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import atlas_cases as K
import atlas_reference as R
from atlas_reference import U
from conftest import golden

F64 = torch.float64


# ------------------------------------------------------------------------------------------------ resize-in-crop
def _draws(tag):
    return [int(v) for v in golden("g19_atlas.npz")[f"crop_{tag}_draws"]]


@pytest.mark.parametrize("tag", list(K.CROP_CASES))
def test_crop_references_reproduce_fixture(tag):
    g = golden("g19_atlas.npz")
    ashape, ishape, crop, usage, seed = K.CROP_CASES[tag]
    atlas, image, label = K.crop_inputs(tag)
    assert K.checksum(atlas, image, label) == str(g[f"crop_{tag}_insum"])
    want = g[f"crop_{tag}_catlas"]
    assert want.dtype == np.float32
    got, (b, c, a) = R.getitem_atlas_ref(atlas, ishape, crop, usage, np.random.RandomState(seed))
    assert ([b, c, a] if usage == "train" else []) == _draws(tag)
    assert got.dtype == np.float64 and np.array_equal(got, want.astype(np.float64))
    cd, ch, cw = crop
    out_hw = (ch, cw, cd) if usage == "train" else K.padded_shape(ishape, crop)
    mine = R.atlas_crop_ref(atlas, ishape, (b, c, a), out_hw)
    assert mine.shape == want.shape and np.array_equal(mine, want.astype(np.float64))


@pytest.mark.parametrize("tag", list(K.CROP_CASES))
def test_crop_case_conditions(tag):
    ashape, ishape, crop, usage, seed = K.CROP_CASES[tag]
    atlas, _, _ = K.crop_inputs(tag)
    cd, ch, cw = crop
    ph, pw, pd = K.padded_shape(ishape, crop)
    if tag.startswith("f32trap"):
        assert usage == "valid"      # the output covers the whole padded volume
        # the float32 formula reads another source row inside the volume, and the rows differ: a kernel using it fails
        ax = [(i, ashape[1], ishape[0]) for i in range(ishape[0])]
        bad = [i for i, n_in, n_out in ax if K.f32_index(i, n_in, n_out) != R.nearest_index(i, n_in, n_out)]
        assert 41 in bad and K.f32_index(41, 2, 82) == 0 and R.nearest_index(41, 2, 82) == 1
        assert not np.array_equal(atlas[:, 0], atlas[:, 1])
        wrong = atlas[:, [K.f32_index(i, 2, 82) for i in range(82)]]
        right = atlas[:, [R.nearest_index(i, 2, 82) for i in range(82)]]
        assert not np.array_equal(wrong, right)
        return
    assert ishape == K.IMAGE and pd > ishape[2] and (ph, pw) == ishape[:2]        # only D is padded
    rel = [np.sign(a - i) for a, i in zip(ashape[1:], ishape)]                   # atlas vs image per axis (H, W, D)
    assert rel == {"up": [-1, -1, -1], "mixed": [1, -1, 1], "eqdbl": [0, -1, 0]}[tag.split("_")[0]]
    if tag.startswith("eqdbl"):
        assert ishape[1] == 2 * ashape[2]
    if usage == "train":
        b, c, a = _draws(tag)
        assert 0 <= b < ph - ch and 0 <= c < pw - cw and 0 <= a < pd - cd
    assert len(np.unique(atlas)) > 32                                             # values tell the voxels apart


def test_nearest_index_sweep():
    """torch's CPU nearest resize of a float64 tensor takes source index (i * in) // out for every pair of the sweep
    (sizes up to 700 -> 1200); the float32 formula that a float32 or device interpolate takes does not."""
    ins = list(range(1, 41)) + [47, 64, 100, 128, 160, 255, 256, 300, 511, 512, 700]
    outs = list(range(1, 131)) + [160, 192, 200, 256, 300, 320, 511, 512, 513, 640, 700, 999, 1024, 1200]
    pairs = f32_bad = 0
    for n_in in ins:
        src = torch.arange(n_in, dtype=F64).reshape(1, 1, n_in)
        for n_out in outs:
            got = F.interpolate(src, size=n_out).reshape(-1).to(torch.int64)
            i = torch.arange(n_out, dtype=torch.int64)
            want = torch.clamp((i * n_in) // n_out, max=n_in - 1)
            assert torch.equal(got, want), (n_in, n_out)
            scale = np.float32(n_in) / np.float32(n_out)
            f32 = np.minimum(np.floor(np.arange(n_out, dtype=np.float32) * scale).astype(np.int64), n_in - 1)
            f32_bad += int(not np.array_equal(f32, want.numpy()))
            pairs += 1
    assert pairs == len(ins) * len(outs) and pairs > 7000
    assert f32_bad > 0 and K.f32_index(41, 2, 82) == 0 and R.nearest_index(41, 2, 82) == 1
    print(f"nearest-index sweep: {pairs} pairs, the float32 formula differs in {f32_bad}")


# ------------------------------------------------------------------------------------------------ atlas-gated Dice
@pytest.mark.parametrize("case", K.DICE_CASES, ids=K.case_id)
def test_dice_case_conditions(case):
    S, C, ncls, sp = case
    lg, lab, atlas = K.dice_flat(case)
    V = lg.shape[1]
    assert atlas.shape[1] >= ncls and ncls <= C - 1 and atlas.dtype == torch.float32
    ref = R.dice_atlas_ref(lg, lab, atlas, ncls)
    mm = ref.margin.abs().min().item()
    print(f"gated-dice {K.case_id(case)}: min margin {mm:.3e}, shares {ref.share.min().item():.3f} .. "
          f"{ref.share.max().item():.3f}")
    assert mm >= K.MARGIN          # far above the fp32 error of p + 0.15 and 1 - a (about 1e-6): the counts are exact
    if S * V >= 255:               # (a lone voxel's share is 0 or 1)
        assert K.SHARE[0] <= ref.share.min().item() and ref.share.max().item() <= K.SHARE[1]
        assert bool((ref.counts[..., 2].sum(0) > 0).all())       # every organ is labelled somewhere
    top = lg.double().topk(2, dim=2).values
    assert (top[..., 0] - top[..., 1]).min().item() > 1e-5        # the argmax is not a matter of rounding
    if case == K.DICE_TRIP[0]:
        assert V > K.AT_DICE_NB * K.AT and V % K.AT


@pytest.mark.parametrize("case", K.DICE_FIXTURE, ids=K.case_id)
def test_dice_reference_reproduces_fixture(case):
    """The reference's get_dice(preds, labels, 1, atlas) computes fp32 ratios from exact counts: within the 'metrics'
    line's (S + 5) u of the fp64 ratios; the argmax map equal."""
    g = golden("g19_atlas.npz")
    S, C, ncls, sp = case
    preds, lab, atlas = K.dice_inputs(case)
    key = "dice_" + K.case_id(case)
    assert K.checksum(preds.numpy(), lab.numpy(), atlas.numpy()) == str(g[f"{key}_insum"])
    ref = R.dice_atlas_ref(*K.dice_flat(case), ncls)
    want = torch.from_numpy(np.stack([g[f"{key}_dice"], g[f"{key}_senc"], g[f"{key}_spec"]], 1))
    assert want.shape == (ncls, 3)
    assert bool(((ref.metrics - want).abs() <= K.SLACK * K.metric_bound(ref.metrics, S)).all())
    assert torch.equal(ref.argmax.reshape(S, *sp), torch.from_numpy(g[f"{key}_argmax"].astype(np.int64)))


# ------------------------------------------------------------------------------------------------ organ / atlas pairs
@pytest.mark.parametrize("geom", K.PAIR_GEOM, ids=K.case_id)
def test_pair_reference_vs_torch_fp64(geom):
    """select_probs_ref's forward is the driver's expression and its backward formula is autograd's, in fp64."""
    C, sp, first, with_atlas = geom
    lg, atlas = K.pair_inputs(geom)
    n = C - first
    lists = K.pair_indices(n)
    assert len(set(lists["dup"])) < len(lists["dup"]) and lists["empty"] == [] and lists["all"] == list(range(n))
    assert sorted(lists["subset"]) != lists["subset"] or len(lists["subset"]) < 3
    for name, index in lists.items():
        x = lg.double().requires_grad_(True)
        pr = torch.softmax(x, 1)[0, first:]
        if with_atlas:
            want = torch.cat([pr.unsqueeze(1), atlas.double().unsqueeze(1)], 1)[index]
        else:
            want = pr[index].unsqueeze(1)
        K_ = len(index)
        gout = K.pair_grad(K_, want.shape[1], sp, 5 + K_) if K_ else None
        ref = R.select_probs_ref(lg.reshape(C, -1), first, index, None if atlas is None else atlas.reshape(n, -1),
                                 None if gout is None else gout.reshape(K_, want.shape[1], -1))
        assert ref.out.shape[0] == K_ and torch.equal(ref.out.reshape(want.shape), want.detach())
        if K_:
            (want * gout.double()).sum().backward()
            err = (ref.dl.reshape(x.shape) - x.grad).abs().max().item()
            assert err <= 1e-15 * max(1.0, x.grad.abs().max().item()), (name, err)
            b_out, b_dl = K.select_bounds(ref)
            # regular regime: the bounds stay a small multiple of u of what they cover
            assert (b_out / ref.out[:, 0]).max().item() < 64 * U
            scale = ref.p * (ref.G_abs + ref.gp_abs)
            assert (b_dl / scale.clamp(min=1e-300)).max().item() < 256 * U
