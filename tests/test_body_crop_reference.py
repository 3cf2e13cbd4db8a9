"""body_crop_reference.py (the host restatement the GPU tests compare against) pinned to the reference's own lines
(tests/golden/g21_body_crop.npz) and to scipy, and the stated property of every labelling pattern of
body_crop_cases.py. No GPU."""
import numpy as np
import pytest
import scipy.ndimage as ndi

import body_crop_cases as K
import body_crop_reference as R
from conftest import golden


@pytest.fixture(scope="module")
def g21():
    return golden("g21_body_crop.npz")


# ------------------------------------------------------------------------------------------------ the fixture
@pytest.mark.parametrize("name", list(K.FIXTURES))
def test_restatement_reproduces_fixture(g21, name):
    cid, img, lab = K.case_inputs(name)
    assert str(g21[f"{name}_insum"]) == K.checksum(img, lab), "the inputs moved: regenerate the fixture"
    image_a, label_a, info = R.body_crop(img, lab, cid)
    assert np.array_equal(np.array(info["bbox"]), g21[f"{name}_bbox"])
    assert np.array_equal(np.array(info["bbox_up"]), g21[f"{name}_bbox_up"])
    assert (info["size"], info["size_up"]) == (int(g21[f"{name}_size"]), int(g21[f"{name}_size_up"]))
    assert (info["route"], info["route_up"]) == (int(g21[f"{name}_route"]), int(g21[f"{name}_route_up"]))
    assert [info["inter_all"], info["inter_up"], int(info["found_hand"])] == g21[f"{name}_inter"].tolist()
    assert [list(image_a.shape), list(label_a.shape), list(info["mask"].shape)] == g21[f"{name}_shapes"].tolist()
    assert np.array_equal(np.packbits(info["mask"] != 0), g21[f"{name}_mask_bits"])
    assert [K.checksum(image_a), K.checksum(label_a)] == g21[f"{name}_sha"].tolist()
    sums = g21[f"{name}_sums"]
    assert np.nansum(image_a.astype(np.float64)) == sums[0]
    assert info["label_sum_after"] == sums[1] and info["label_sum_before"] == sums[2]


def test_fixture_covers_the_routes(g21):
    routes = {n: (int(g21[f"{n}_route"]), int(g21[f"{n}_route_up"]), int(g21[f"{n}_inter"][2])) for n in K.FIXTURES}
    assert routes["mri_hand"] == (0, 0, 1)                    # both calls find a component, the hand branch
    assert routes["ct_fallback"][:2] == (1, 0) and routes["ct_fallback"][2] == 0 and K.FIXTURES["ct_fallback"][0] <= 410
    assert routes["special_both_fallback"] == (1, 1, 1)
    assert (K.case_inputs("ct_fallback")[2] >= 14).any()      # codes >= 14 in a label


# ------------------------------------------------------------------------------------------------ labelling
@pytest.mark.parametrize("shape", K.label_shapes() + [(1, 1, 1)], ids=str)
@pytest.mark.parametrize("name", K.PATTERNS)
def test_labelling_is_scipys_and_patterns_hold(name, shape):
    m = K.pattern(name, shape)
    lab, n = R.label_components(m)
    want, wn = ndi.label(m)                                   # default structure: faces; numbered by first voxel
    assert n == wn and np.array_equal(lab, want)
    fg = int(np.count_nonzero(m))
    if name == "zeros":
        assert n == 0
    elif name in ("ones", "serpentine", "comb"):
        assert n == 1 and fg > 0
    elif name == "checkerboard":
        assert n == fg
    elif name in ("edge", "corner") and K.boxes_separable(shape, name):
        assert n == 2
        assert ndi.label(m, structure=np.ones((3, 3, 3)))[1] == 1    # they do touch, diagonally


def test_percolation_case_is_tortuous():
    m = K.pattern("bernoulli0.31", K.PERCOLATION_SHAPE)
    lab, n = R.label_components(m)
    assert 9000 < n < 13000 and np.bincount(lab.reshape(-1))[1:].max() > 1000


# ------------------------------------------------------------------------------------------------ getmaxcomponent
def test_largest_component_cases():
    c = K.largest_cases()
    got = {k: R.largest_component(*v) for k, v in c.items()}
    assert int(got["plain"].sum()) == 8 * 12 * 64
    assert int(got["tie"].sum()) == 768 and got["tie"][1:4].any() and not got["tie"][6:9].any()
    assert int(got["hidden"].sum()) == 1 and int(got["hidden_found"].sum()) == 8 * 16 * 66
    assert got["none"] is None
    assert int(got["fractional"].sum()) == 8 * 12 * 64
    assert int(got["fractional_cut"].sum()) == 12
    assert int(got["exact"].sum()) == 12


# ------------------------------------------------------------------------------------------------ masks
@pytest.mark.parametrize("shape", [(1, 5, 6), (5, 1, 6), (5, 6, 1), (2, 2, 2), (7, 9, 11)])
def test_erode2_is_scipys(shape):
    g = np.random.default_rng([25] + list(shape))
    m = g.random(shape) < 0.85
    assert np.array_equal(R.erode2(m), ndi.binary_erosion(m, structure=np.ones((2, 2, 2))))


@pytest.mark.parametrize("shape", [(4, 9, 10), (10, 10, 10), (11, 23, 31)])
def test_box_windows_are_scipys(shape):
    g = np.random.default_rng([26] + list(shape))
    m = g.random(shape) < 0.97
    s = np.ones((10, 10, 10))
    er = m
    for ax in range(3):
        er = R.window_axis(er, ax, -5, 4, "and")
    assert np.array_equal(er, ndi.binary_erosion(m, structure=s))
    sparse = g.random(shape) < 0.002
    di = sparse
    for ax in range(3):
        di = R.window_axis(di, ax, -4, 5, "or")
    assert np.array_equal(di, ndi.binary_dilation(sparse, structure=s))
    assert R.window_offsets(10, False) == (-5, 4) and R.window_offsets(10, True) == (-4, 5)


def test_window_offsets_distinguished_from_their_mirror():
    """A single voxel / a single hole off centre: the mirrored offsets give another answer, scipy gives ours."""
    s = np.ones((10, 10, 10))
    m = np.zeros((1, 1, 30), dtype=bool)
    m[0, 0, 12] = True
    s1 = np.ones((1, 1, 10))
    ours = R.window_axis(m, 2, -4, 5, "or")
    assert np.array_equal(ours, ndi.binary_dilation(m, structure=s1))
    assert not np.array_equal(R.window_axis(m, 2, -5, 4, "or"), ours)
    run = np.zeros((1, 1, 30), dtype=bool)
    run[0, 0, 5:17] = True
    ours = R.window_axis(run, 2, -5, 4, "and")
    assert np.array_equal(ours, ndi.binary_erosion(run, structure=s1)) and ours.sum() == 3
    assert not np.array_equal(R.window_axis(run, 2, -4, 5, "and"), ours)
    assert s.shape == (10, 10, 10)
    for n in (3, 4, 7):
        sn = np.ones((1, 1, n))
        assert np.array_equal(R.window_axis(run, 2, *R.window_offsets(n, False), "and"), ndi.binary_erosion(run, structure=sn))
        assert np.array_equal(R.window_axis(m, 2, *R.window_offsets(n, True), "or"), ndi.binary_dilation(m, structure=sn))


def test_threshold_is_strict_and_nan_is_background():
    v = np.array([[[np.nan, -200.0, -199.99, 5.0]]], dtype=np.float32)
    assert (v > np.float32(-200)).tolist() == [[[False, False, True, True]]]
    assert [R.body_threshold(c) for c in (1, 410, 411, 500, 518, 540, 600)] == [-200, -200, 25, 25, 30000, 30000, 25]


@pytest.mark.parametrize("name", list(K.SMALL))
def test_small_cases_take_their_routes(name):
    cid, mf, mfu, _ = K.SMALL[name]
    _, img, lab = K.case_inputs(name)
    _, _, info = R.body_crop(img, lab, cid, mf, mfu)
    want = {"hand": (0, 0, True), "nohand_cid": (0, 0, False), "nohand_extent": (0, 0, False),
            "fallback_first": (1, 0, False), "fallback_both_hand": (1, 1, True)}[name]
    assert (info["route"], info["route_up"], info["found_hand"]) == want
    if name == "nohand_cid":
        assert info["inter_all"] - info["inter_up"] > 30       # only the case id keeps the branch from firing


def test_empty_inputs_raise():
    _, img, lab = K.case_inputs("nohand_extent")
    with pytest.raises(ValueError):
        R.body_crop(img, np.where(lab >= 14, lab, 0), 600, 2000.0, 500.0)      # only codes >= 14: empty once cleared
    with pytest.raises(ValueError):
        R.body_crop(np.zeros_like(img), lab, 600, 2000.0, 500.0)               # nothing above the threshold
