"""csrc/atlas_build.hip and u3d.data.AtlasBuilder against the host restatements of atlas_build_reference.py and the
reference's own lines (tests/golden/g20_atlas_build.npz). The C entry points are called through u3d._lib on buffers the
test allocates: acc pre-filled with 3.0 and counts with 5, so that "+=" and the untouched elements both show, and every
element is compared. Cases and inputs live in atlas_build_cases.py; test_atlas_build_reference.py asserts their
conditions on the CPU.

Bounds.
sums      small integers in fp32, a gather through integer tables: bit-exact, whatever the launch geometry and the
          order of the calls.
counts    integers: exact.
normalise (float)((double)acc / count): one rounding, u = 2^-24 relative.
final     per plane 7 u A SLACK against the float64 fixture, A = the plane's fp64 maximum after normalisation,
          SLACK = 1 + 2^-10: one rounding in the normalise, then per blur pass (three of them) one for the fp32 weights
          (each weight fl32(w) = w (1 + d), |d| <= u, against a sum of |x| w <= A) and one for the fp32 store; the
          blur is a convex combination up to those roundings, so nothing exceeds A; the fp64 accumulation of 25 terms
          (25 * 2^-53) sits inside SLACK. A label no case has: exactly zero.

Every bounded test prints its worst error as a share of the bound ("SHARE <family> <value>") before asserting.
"""
import functools

import numpy as np
import pytest
import torch

import atlas_build_cases as K
import atlas_build_reference as R
import atlas_reference as AR
from conftest import golden

pytestmark = pytest.mark.gpu

f32, i32 = torch.float32, torch.int32


def _L():
    from u3d import _lib as L
    return L


def _stream():
    from u3d.ops import _stream as s
    return s()


def _bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


def _tables(src, dst, dev):
    from u3d.data import zoom_index
    return [torch.from_numpy(zoom_index(n, s)).to(dev) for n, s in zip(src, dst)]


def _run_add(label_dev, src, dst, L, dev):
    """u3d_atlas_build_add on pre-filled buffers; (acc, counts) on the host."""
    idx = _tables(src, dst, dev)
    acc = torch.full((L,) + tuple(dst), K.ACC_FILL, dtype=f32, device=dev)
    counts = torch.full((L,), K.COUNT_FILL, dtype=i32, device=dev)
    ws = torch.full((_L().query("u3d_atlas_build_ws_bytes"),), 0xFF, dtype=torch.uint8, device=dev)   # dirty on entry
    _L().call("u3d_atlas_build_add", label_dev.data_ptr(), *src, *(t.data_ptr() for t in idx), L, *dst, acc.data_ptr(),
              counts.data_ptr(), ws.data_ptr(), _stream())
    torch.cuda.synchronize()
    return acc.cpu().numpy(), counts.cpu().numpy()


def _want_add(vol, dst, L):
    acc = np.full((L,) + tuple(dst), K.ACC_FILL, dtype=np.float32)
    counts = np.full(L, K.COUNT_FILL, dtype=np.int32)
    R.gather_add(vol, dst, L, acc, counts)
    return acc, counts


@pytest.mark.parametrize("L", K.KERNEL_L)
@pytest.mark.parametrize("name", list(K.KERNEL_CASES))
def test_add_kernel_vs_restatement(gpu, name, L):
    src, dst = K.KERNEL_CASES[name]
    vol = K.kernel_volume(src)
    acc, counts = _run_add(torch.from_numpy(vol.copy()).to(gpu), src, dst, L, gpu)
    wa, wc = _want_add(vol, dst, L)
    assert np.array_equal(acc.view(np.int32), wa.view(np.int32)) and np.array_equal(counts, wc)
    print(f"SHARE atlas-build-add {name} L={L} 0.0000")


@pytest.mark.parametrize("name", list(K.GEOM_CASES))
def test_add_kernel_past_its_grid(gpu, name):
    src, dst = K.GEOM_CASES[name]
    vol = K.kernel_volume(src)
    acc, counts = _run_add(torch.from_numpy(vol.copy()).to(gpu), src, dst, 15, gpu)
    wa, wc = _want_add(vol, dst, 15)
    assert np.array_equal(acc.view(np.int32), wa.view(np.int32)) and np.array_equal(counts, wc)


def test_presence_pass_unaligned_and_past_its_grid(gpu):
    vol = K.presence_volume()
    buf = torch.zeros(vol.size + 64, dtype=torch.uint8, device=gpu)
    assert buf.data_ptr() % 16 == 0
    lab = buf[K.PRESENCE_OFFSET:K.PRESENCE_OFFSET + vol.size]
    lab.copy_(torch.from_numpy(vol.reshape(-1).copy()))
    assert lab.data_ptr() % 16 == K.PRESENCE_OFFSET
    acc, counts = _run_add(lab, K.PRESENCE_SHAPE, K.PRESENCE_ATLAS, 15, gpu)
    wa, wc = _want_add(vol, K.PRESENCE_ATLAS, 15)
    assert np.array_equal(counts, wc) and np.array_equal(acc.view(np.int32), wa.view(np.int32))
    assert sorted(np.nonzero(counts - K.COUNT_FILL)[0] + 1) == sorted(K.PRESENCE_VOXELS)


def test_normalize_kernel(gpu):
    L, V = 5, 2 * K.AB + 3
    g = np.random.default_rng(23)
    acc = g.integers(0, 40, (L, V)).astype(np.float32)
    counts = np.array([3, 0, 7, 1, 39], dtype=np.int32)
    acc[1] = 9.0                                   # a plane without a count is written as zeros whatever it holds
    out = torch.full((L, V), float("nan"), dtype=f32, device=gpu)
    dacc, dcounts = torch.from_numpy(acc).to(gpu), torch.from_numpy(counts).to(gpu)
    _L().call("u3d_atlas_build_normalize", dacc.data_ptr(), dcounts.data_ptr(), L, V, out.data_ptr(), _stream())
    torch.cuda.synchronize()
    want = R.normalized(acc.astype(np.float64), counts).astype(np.float32)      # one rounding of the fp64 quotient
    assert np.array_equal(out.cpu().numpy().view(np.int32), want.view(np.int32))
    assert not out[1].any() and bool(torch.isfinite(out).all())


# ------------------------------------------------------------------------------------------------ AtlasBuilder
@functools.lru_cache(maxsize=None)
def _built(name, reverse=False):
    """(builder, finish()) over a fixture's cases on the device, built once."""
    from u3d.data import AtlasBuilder
    dev = torch.device("cuda:0")
    vols = K.fixture_volumes(name)
    b = AtlasBuilder(K.SHAPES[name], K.L_REF, dev)
    for v in (reversed(vols) if reverse else vols):
        b.add(torch.from_numpy(v.copy()).to(dev))
    return b, b.finish(K.SIGMA)


def _check_final(tag, got, g, name):
    sums, counts = g[f"{name}_sums"].astype(np.float64), g[f"{name}_count"]
    want = g[f"{name}_atlas"]
    assert got.dtype == f32 and tuple(got.shape) == want.shape and got.is_contiguous()
    bound = K.final_bound(sums, counts)
    err = np.abs(got.cpu().numpy().astype(np.float64) - want).reshape(want.shape[0], -1).max(1)
    assert np.isfinite(err).all()
    assert not err[bound == 0].any(), f"{tag}: error where the bound is 0"
    share = float((err[bound > 0] / bound[bound > 0]).max())
    print(f"SHARE {tag} {share:.4f}")
    assert share <= 1


@pytest.mark.parametrize("name", list(K.FIXTURES))
def test_builder_vs_reference_fixture(gpu, name):
    g = golden("g20_atlas_build.npz")
    b, atlas = _built(name)
    assert b.acc.dtype == f32 and b.counts.dtype == i32 and b.acc.device == gpu
    assert np.array_equal(b.acc.cpu().numpy(), g[f"{name}_sums"].astype(np.float32))
    assert np.array_equal(b.counts.cpu().numpy(), g[f"{name}_count"])
    _check_final(f"atlas-build-final {name}", atlas, g, name)
    plain = b.finish(sigma=None).cpu().numpy()           # the normalised sums: one rounding of the fp64 quotient
    want = R.normalized(g[f"{name}_sums"].astype(np.float64), g[f"{name}_count"]).astype(np.float32)
    assert np.array_equal(plain.view(np.int32), want.view(np.int32))
    # a label no case has: its plane is exactly zero and finite, with and without the blur
    z = atlas[K.ABSENT - 1]
    assert g[f"{name}_count"][K.ABSENT - 1] == 0 and bool(torch.isfinite(atlas).all()) and not bool(z.any())
    assert not plain[K.ABSENT - 1].any()


@pytest.mark.parametrize("name", list(K.FIXTURES))
def test_build_atlas_picks_the_shape(gpu, name):
    from u3d.data import build_atlas
    g = golden("g20_atlas_build.npz")
    vols = [torch.from_numpy(v.copy()).to(gpu) for v in K.fixture_volumes(name)]
    atlas = build_atlas(iter(vols))
    assert tuple(atlas.shape) == (15,) + tuple(int(v) for v in g[f"{name}_total_shape"])
    assert torch.equal(_bits(atlas), _bits(_built(name)[1]))
    _check_final(f"build_atlas {name}", atlas, g, name)
    assert torch.equal(_bits(build_atlas(vols, shape=K.SHAPES[name], num_labels=13)), _bits(atlas[:13]))


def test_finish_leaves_the_builder_usable(gpu):
    from u3d.data import AtlasBuilder
    vols = [torch.from_numpy(v.copy()).to(gpu) for v in K.fixture_volumes("small")]
    b = AtlasBuilder(K.SHAPES["small"], device=gpu)
    b.add(vols[0])
    first = b.finish()
    assert first.data_ptr() != b.acc.data_ptr()
    b.add(vols[1])
    assert torch.equal(_bits(b.acc), _bits(_built("small")[0].acc))
    assert torch.equal(_bits(b.finish()), _bits(_built("small")[1]))
    merged = AtlasBuilder(K.SHAPES["small"], device=gpu)                     # partial builders merge by addition
    parts = [AtlasBuilder(K.SHAPES["small"], device=gpu).add(v) for v in vols]
    for p in parts:
        merged.acc += p.acc
        merged.counts += p.counts
    assert torch.equal(_bits(merged.finish()), _bits(_built("small")[1]))


@pytest.mark.parametrize("dtype", [torch.int16, torch.int32, torch.int64, torch.float32, torch.float64],
                         ids=lambda d: str(d).replace("torch.", ""))
def test_input_dtypes_do_not_wrap(gpu, dtype):
    """257, -255 and (floats) 1.5 in place of background voxels: the result is the canonical uint8 input's."""
    from u3d.data import AtlasBuilder
    name = "small"
    want_b, _ = _built(name)
    b = AtlasBuilder(K.SHAPES[name], device=gpu)
    planted = 0
    for v in K.fixture_volumes(name):
        a = v.astype(np.float64)
        zeros = np.argwhere(v == 0)
        bad = [x for x in K.NOT_LABELS if dtype.is_floating_point or x == int(x)]
        assert len(zeros) >= len(bad)
        for pos, x in zip(zeros, bad):
            a[tuple(pos)] = x
            planted += 1
        t = torch.from_numpy(a).to(dtype)
        assert np.array_equal(R.canonical_u8(t.numpy()), v)
        b.add(t.to(gpu))
    assert planted >= 4
    assert torch.equal(_bits(b.acc), _bits(want_b.acc)) and torch.equal(b.counts, want_b.counts)
    # label 1's plane would have gained the wrapped voxels: the comparison above is on it too
    assert bool(want_b.acc[0].any())


@pytest.mark.parametrize("name", list(K.FIXTURES))
def test_case_order_does_not_matter(gpu, name):
    fwd, rev = _built(name), _built(name, True)
    assert torch.equal(_bits(fwd[0].acc), _bits(rev[0].acc)) and torch.equal(fwd[0].counts, rev[0].counts)
    assert torch.equal(_bits(fwd[1]), _bits(rev[1]))


def test_finish_feeds_atlas_crop(gpu):
    """finish()'s tensor goes straight into atlas_crop / crop_patch(atlas=): the same bits as the host restatement of
    atlas_crop on a host copy of it."""
    from u3d import data
    _, atlas = _built("wide")
    image_shape, offsets, crop = (20, 30, 12), (3, 5, 1), (12, 16, 8)
    got = data.atlas_crop(atlas[:13], image_shape, offsets, crop)
    host = atlas[:13].cpu().numpy().copy()
    want = AR.atlas_crop_ref(host, image_shape, offsets, crop)
    assert got.shape == want.shape and np.array_equal(got.cpu().numpy().view(np.int32),
                                                      want.astype(np.float32).view(np.int32))
    again = data.atlas_crop(torch.from_numpy(host).to(gpu), image_shape, offsets, crop)
    assert torch.equal(_bits(got), _bits(again))
    img = torch.zeros(image_shape, device=gpu)
    _, _, cat = data.crop_patch(img, img, None, "0007", (8, 12, 16), usage="valid", atlas=atlas[:13])
    assert cat.shape[0] == 13 and bool(cat.any())
