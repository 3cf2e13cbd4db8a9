"""The restatements of atlas_build_reference.py against the reference's own lines (tests/golden/g20_atlas_build.npz,
written by tests/golden/gen_golden_atlas_build.py) and against the per-label ndimage.zoom procedure, and the input
conditions of the cases of atlas_build_cases.py that test_gpu_atlas_build.py relies on. No device."""
import numpy as np
import pytest

import atlas_build_cases as K
import atlas_build_reference as R
from conftest import golden
from u3d.data import average_shape, zoom_index


@pytest.mark.parametrize("name", list(K.FIXTURES))
def test_restatement_reproduces_fixture_and_zoom_procedure(name):
    """The gather through zoom_index equals the per-label ndimage.zoom sums and the reference's, exactly; the float64
    finish equals the reference's atlas exactly (the same scipy calls on the same sums)."""
    g = golden("g20_atlas_build.npz")
    vols = K.fixture_volumes(name)
    assert K.checksum(*vols) == str(g[f"{name}_insum"])
    shape = tuple(int(v) for v in g[f"{name}_total_shape"])
    assert shape == K.SHAPES[name] == average_shape([v.shape for v in vols])
    sums, counts = R.gather_sums(vols, shape, K.L_REF)
    zs, zc = R.zoom_sums(vols, shape, K.L_REF)
    assert np.array_equal(sums, zs) and np.array_equal(counts, zc)
    assert g[f"{name}_sums"].dtype == np.uint8 and g[f"{name}_atlas"].dtype == np.float64
    assert np.array_equal(sums, g[f"{name}_sums"].astype(np.float64))
    assert np.array_equal(counts, g[f"{name}_count"])
    assert np.array_equal(R.finish(sums, counts, K.SIGMA), g[f"{name}_atlas"])


def test_fixture_case_conditions():
    g = golden("g20_atlas_build.npz")
    radius = int(4.0 * K.SIGMA + 0.5)
    assert radius == 12
    assert max(K.SHAPES["small"]) < radius                    # the blur's reflection wraps on every axis
    assert max(K.SHAPES["wide"]) >= 2 * radius + 2            # and one axis holds the whole kernel
    # lost last plane: at least one (in, out) axis pair of the fixture, and every named pair
    lost = [(v.shape[a], K.SHAPES[n][a]) for n in K.FIXTURES for v in K.fixture_volumes(n) for a in range(3)
            if zoom_index(v.shape[a], K.SHAPES[n][a])[-1] < 0]
    assert (8, 26) in lost and (29, 26) in lost
    for n_in, n_out in K.QUIRK_PAIRS:
        t = zoom_index(n_in, n_out)
        assert t[-1] == -1 and (t[:-1] >= 0).all(), (n_in, n_out)
    # the lost plane is visible in the reference's sums: nothing arrives in the last plane of axis 0 from two of the
    # three cases of "wide", so no voxel there exceeds 1
    assert g["wide_sums"].sum(0)[-1].max() <= 1 < g["wide_sums"].sum(0)[:-1].max()
    # an exact tie: 4 -> 3, cc = 1.5 -> source 2 (floor(cc + 0.5)); rint would give 2 as well, floor(cc) 1
    assert zoom_index(4, 3).tolist() == [0, 2, 3] and 1 * ((4 - 1) / (3 - 1)) == 1.5
    assert K.FIXTURES["small"][0][0] == 4 and K.SHAPES["small"][0] == 3
    # an axis whose mean ends in .5, rounded half to even (half up would give 5)
    d = [s[2] for s in K.FIXTURES["small"]]
    assert sum(d) / len(d) == 4.5 and K.SHAPES["small"][2] == 4
    for name in K.FIXTURES:
        vols = K.fixture_volumes(name)
        assert all(v.dtype == np.uint8 for v in vols)
        assert not any((v == K.ABSENT).any() for v in vols) and g[f"{name}_count"][K.ABSENT - 1] == 0
        assert not g[f"{name}_atlas"][K.ABSENT - 1].any()
        assert any((v == 0).any() for v in vols) and any((v == 16).any() for v in vols)       # codes 0 and 16
        present = [l for l in range(1, 16) if g[f"{name}_count"][l - 1] > 0]
        assert present == [l for l in range(1, 16) if l != K.ABSENT]
    # a label present in a source but absent after its zoom: it counts, and its plane stays empty
    v0 = K.fixture_volumes("small")[0]
    assert int((v0 == K.LONE).sum()) == 1 and v0[K.LONE_AT] == K.LONE
    assert K.LONE_AT[0] not in zoom_index(4, 3).tolist()
    assert not any((v == K.LONE).any() for v in K.fixture_volumes("small")[1:])
    assert g["small_count"][K.LONE - 1] == 1 and not g["small_sums"][K.LONE - 1].any()
    assert not g["small_atlas"][K.LONE - 1].any()
    # the case order matters to nothing, the counts differ between labels (a plane / the wrong count would show)
    assert len(set(g["small_count"].tolist())) >= 3


@pytest.mark.parametrize("name", list(K.KERNEL_CASES) + list(K.GEOM_CASES))
def test_kernel_case_conditions(name):
    src, dst = (K.KERNEL_CASES | K.GEOM_CASES)[name]
    v = K.kernel_volume(src)
    for L in K.KERNEL_L:
        for code in (0, L + 1, 255):
            assert (v == code).any(), (name, L, code)
        # on the pre-filled buffers both "+=" and the untouched elements show, in the sums and in the counts
        acc, cnt = np.full((L,) + dst, K.ACC_FILL), np.full(L, K.COUNT_FILL)
        R.gather_add(v, dst, L, acc, cnt)
        assert (acc == K.ACC_FILL).any() and (acc == K.ACC_FILL + 1).any() and acc.max() == K.ACC_FILL + 1
        assert (cnt == K.COUNT_FILL + 1).any()
    if name in K.KERNEL_CASES:
        pairs = {(a, b) for s, d in K.KERNEL_CASES.values() for a, b in zip(s, d)}
        assert pairs == {(8, 26), (30, 8), (4, 3), (5, 1), (1, 4), (2, 7)}
        assert sorted(d[2] for _, d in K.KERNEL_CASES.values()) == [1, 3, 7, 26]
        assert dst[0] * dst[1] * dst[2] > 0
    if name == "ystride":
        assert dst[0] > K.AB_GY
    if name == "xstride":
        assert dst[1] * dst[2] > K.AB_GX * K.AB and (dst[1] * dst[2]) % K.AB
    # the restatement equals the zoom procedure on these shapes too
    a, c = R.gather_sums([v], dst, 15)
    za, zc = R.zoom_sums([v], dst, 15)
    assert np.array_equal(a, za) and np.array_equal(c, zc)


def test_presence_case_conditions():
    v = K.presence_volume()
    n = v.size
    head = 16 - K.PRESENCE_OFFSET                             # bytes before the first aligned 16-byte word
    words = (n - head) // 16
    assert words > K.AB_PB * K.AB and (n - head) % 16         # a second trip, and a scalar tail
    idx = K.PRESENCE_VOXELS
    assert idx[1] < head and (idx[3] - head) // 16 >= K.AB_PB * K.AB and idx[2] >= head + words * 16
    assert head <= idx[5] < head + K.AB_PB * K.AB * 16
    flat = v.reshape(-1)
    for l in range(1, 16):
        assert int((flat == l).sum()) == (1 if l in idx else 0)
    assert (flat == 16).any() and (flat == 255).any()
    # the gather of this case loses labels (it shrinks): presence must come from the source
    a, c = R.gather_sums([v], K.PRESENCE_ATLAS, 15)
    assert sorted(np.nonzero(c)[0] + 1) == sorted(idx) and any(not a[l - 1].any() for l in idx)


def test_canonical_u8():
    a = np.array([0.0, 1.0, 15.0, 255.0, 256.0, 257.0, -255.0, -1.0, 1.5, np.nan, np.inf])
    assert R.canonical_u8(a).tolist() == [0, 1, 15, 255, 0, 0, 0, 0, 0, 0, 0]
    for bad in K.NOT_LABELS:     # what a plain cast would make of them
        assert np.array([bad]).astype(np.int64).astype(np.uint8)[0] == 1
    assert R.canonical_u8(np.array([257, -255, 3], dtype=np.int16)).tolist() == [0, 0, 3]
