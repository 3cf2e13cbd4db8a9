"""u3d.surface and evaluate_amos.get_surface_scores on the device against surface_reference.py (numpy / scipy fp64):
mask surfaces and class boxes exactly, surface distances to one fp32 ulp (exactly for integer spacings), the metrics as
follows. With integer spacings the squared distances are integers, so d <= tau has no near-ties: the NSD counts, and with
them the NSD (one fp64 division rounded to fp32), are exact; HD is the largest distance, exact. HD95 and ASSD are within
2^-22 relative: one fp32 ulp (2^-23) per distance and the fp32 store. With the non-integer spacing the test first asserts
that no reference distance lies within 2^-20 relative of tau (a condition on the inputs), then the same."""
import functools

import numpy as np
import pytest
import torch

import surface_cases as K
import surface_reference as R
from u3d import surface

pytestmark = pytest.mark.gpu

ULP = 2.0 ** -23
NONINT = (0.7, 1.3, 2.5)
NONINT_TAU = 2.2


def _L():
    from u3d import _lib as L
    return L


def _stream():
    from u3d.ops import _stream as s
    return s()


def _dev(a, gpu):
    return torch.from_numpy(np.array(a, order="C")).to(gpu)             # a copy: the cached cases are read-only


# ------------------------------------------------------------------------------------------------ surfaces
@pytest.mark.parametrize("dtype", [torch.uint8, torch.int32, torch.int64, torch.float32, torch.bool, torch.int16])
def test_mask_surface_on_every_dtype(gpu, dtype):
    for shape in ((1, 1, 1), (5, 6, 7), (9, 17, 130)):
        for name in ("none", "all", "bernoulli0.5", "bernoulli0.95", "checkerboard"):
            m = K.pattern(name, shape)
            got = surface.mask_surface(_dev(m, gpu).to(dtype))
            assert got.dtype == torch.uint8 and tuple(got.shape) == shape
            assert np.array_equal(got.cpu().numpy(), R.surface_ref(m).astype(np.uint8)), (shape, name)


@pytest.mark.parametrize("dtype", [torch.uint8, torch.int32, torch.int64, torch.float32])
def test_mask_surface_of_a_class_value(gpu, dtype):
    lab = K.ellipsoids((20, 24, 70), 5, 7, border_class=3)
    t = _dev(lab, gpu).to(dtype)
    for c in (0, 1, 3, 5, 6):
        want = R.surface_ref(lab == c).astype(np.uint8)
        assert np.array_equal(surface.mask_surface(t, value=c).cpu().numpy(), want), c
    if dtype == torch.float32:
        t[2, 3, 4] = float("nan")
        t[2, 3, 5] = 1.5
        lab = lab.copy()
        lab[2, 3, 4] = lab[2, 3, 5] = -1                                 # neither equals any class
        assert np.array_equal(surface.mask_surface(t, value=1).cpu().numpy(), R.surface_ref(lab == 1).astype(np.uint8))
        assert np.array_equal(surface.mask_surface(t).cpu().numpy(), R.surface_ref(lab != 0).astype(np.uint8))


def test_mask_surface_on_boxes_touching_every_face(gpu):
    """The C entry point on a box: the surface is that of the whole volume, cut to the box."""
    shape = (9, 10, 70)
    lab = K.pattern("bernoulli0.95", shape).astype(np.int32) * 4
    want = R.surface_ref(lab == 4).astype(np.uint8)
    t = _dev(lab, gpu)
    for z0, y0, x0, bz, by, bx in ((0, 0, 0, 9, 10, 70), (0, 2, 3, 4, 5, 60), (5, 0, 3, 4, 5, 60), (2, 5, 0, 4, 5, 66),
                                   (2, 3, 5, 7, 7, 65), (3, 3, 3, 1, 1, 1), (8, 9, 69, 1, 1, 1), (0, 0, 0, 1, 10, 1)):
        out = torch.full((bz, by, bx), 9, dtype=torch.uint8, device=gpu)
        _L().call("u3d_mask_surface", t.data_ptr(), 2, *shape, 4.0, 0, z0, y0, x0, bz, by, bx, out.data_ptr(), _stream())
        assert np.array_equal(out.cpu().numpy(), want[z0:z0 + bz, y0:y0 + by, x0:x0 + bx]), (z0, y0, x0)
    from u3d._lib import U3DError
    p = t.data_ptr()
    for box in ((0, 0, 0, 10, 10, 70), (1, 0, 0, 9, 10, 70), (0, 0, 66, 1, 1, 5), (-1, 0, 0, 1, 1, 1), (0, 0, 0, 0, 1, 1)):
        with pytest.raises(U3DError, match="box"):
            _L().call("u3d_mask_surface", p, 2, *shape, 4.0, 0, *box, p, _stream())
    with pytest.raises(U3DError, match="dtype"):
        _L().call("u3d_mask_surface", p, 4, *shape, 4.0, 0, 0, 0, 0, 1, 1, 1, p, _stream())
    with pytest.raises(U3DError, match="null"):
        _L().call("u3d_mask_surface", p, 2, *shape, 4.0, 0, 0, 0, 0, 1, 1, 1, None, _stream())


# ------------------------------------------------------------------------------------------------ class boxes
@pytest.mark.parametrize("pdt,gdt", [(torch.int64, torch.float32), (torch.int32, torch.int64),
                                     (torch.uint8, torch.uint8), (torch.int64, torch.int32)])
def test_class_boxes_are_numpys(gpu, pdt, gdt):
    pred, gt, nc = K.metric_case("thirteen")                             # 5 absent from pred, 7 from gt, 9 from both
    want = R.class_boxes_ref(pred, gt, nc)
    assert want[4, 6] == 0 < want[4, 7] and want[6, 7] == 0 < want[6, 6] and want[8, 6] == want[8, 7] == 0
    got = surface.class_boxes(_dev(pred, gpu).to(pdt), _dev(gt, gpu).to(gdt), nc)
    assert got.dtype == torch.int32 and np.array_equal(got.cpu().numpy(), want)
    # classes beyond num_class, and values that are no class, belong to no box
    got = surface.class_boxes(_dev(pred, gpu).to(pdt), _dev(gt, gpu).to(gdt), 4)
    assert np.array_equal(got.cpu().numpy(), want[:4])


def test_class_boxes_on_a_wide_row_and_odd_values(gpu):
    shape = (3, 5, 300)
    g = np.random.default_rng(43)
    pred = g.integers(0, 4, shape).astype(np.int64)
    gt = g.integers(0, 4, shape).astype(np.float32)
    pred[0, 0, 0], pred[0, 0, 1] = -1, 2 ** 40 + 1
    gt[0, 0, 0], gt[0, 0, 1], gt[0, 0, 2] = np.nan, 1.5, -2.0
    got = surface.class_boxes(_dev(pred, gpu), _dev(gt, gpu), 3)
    assert np.array_equal(got.cpu().numpy(), R.class_boxes_ref(pred, gt, 3))
    from u3d._lib import U3DError
    p = got.data_ptr()
    with pytest.raises(U3DError, match="num_class"):
        _L().call("u3d_class_boxes", p, 3, p, 1, 2, 2, 2, 65, p, _stream())
    with pytest.raises(U3DError, match="2\\^31"):
        _L().call("u3d_class_boxes", p, 3, p, 1, 2048, 1024, 1024, 3, p, _stream())


# ------------------------------------------------------------------------------------------------ surface distances
def _one_ulp(got, want, exact_squares):
    got = got.astype(np.float64)
    assert got.shape == want.shape
    assert (np.abs(got - want) <= ULP * np.abs(want)).all()
    if exact_squares:
        assert np.array_equal(got, np.sqrt(np.rint(want ** 2)).astype(np.float32).astype(np.float64))


@pytest.mark.parametrize("spacing", [(1, 1, 1), (2, 1, 1), (3, 2, 1), NONINT], ids=str)
def test_surface_distances(gpu, spacing):
    pred, gt, nc = K.metric_case("five")
    for c in (1, 2, 4):
        a, b = pred == c, gt == c
        want = R.surface_distances_ref(a, b, spacing)
        got = surface.surface_distances(_dev(a, gpu), _dev(b, gpu), spacing)
        for u, v in zip(got, want):
            assert u.dtype == torch.float32 and u.dim() == 1
            _one_ulp(u.cpu().numpy(), v, spacing != NONINT)             # same length, same (C) order
    a = _dev(pred == 1, gpu)
    none = torch.zeros_like(a)
    d_ab, d_ba = surface.surface_distances(a, none, spacing)
    assert d_ba.numel() == 0 and d_ab.numel() == int(R.surface_ref(pred == 1).sum()) and torch.isposinf(d_ab).all()


def test_reduce_entry_point(gpu):
    """u3d_surface_dist_reduce against numpy on a volume of more than one block per wave round, and on an empty set."""
    g = np.random.default_rng(44)
    V = 70001
    surf = (g.random(V) < 0.3).astype(np.uint8)
    dist = (g.random(V) * 9).astype(np.float32)
    dist[g.integers(0, V, 50)] = np.float32(2.5)
    sel = dist[surf != 0].astype(np.float64)
    ws = torch.full((_L().query("u3d_surface_reduce_ws_bytes"),), 0xFF, dtype=torch.uint8, device=gpu)
    rec = torch.full((5,), -3.0, dtype=torch.float64, device=gpu)
    sd, dd = _dev(surf, gpu), _dev(dist, gpu)
    _L().call("u3d_surface_dist_reduce", sd.data_ptr(), dd.data_ptr(), V, 2.5, rec.data_ptr(), ws.data_ptr(), _stream())
    r = rec.cpu().numpy()
    assert r[0] == sel.size and r[2] == sel.max() and r[3] == (sel <= 2.5).sum() and r[4] == sel.min()
    assert abs(r[1] - sel.sum()) <= 1e-12 * sel.sum()
    again = torch.empty_like(rec)
    _L().call("u3d_surface_dist_reduce", sd.data_ptr(), dd.data_ptr(), V, 2.5, again.data_ptr(), ws.data_ptr(), _stream())
    assert again.cpu().numpy().tobytes() == r.tobytes()                  # fixed order
    sd.zero_()
    _L().call("u3d_surface_dist_reduce", sd.data_ptr(), dd.data_ptr(), V, 2.5, rec.data_ptr(), ws.data_ptr(), _stream())
    assert rec.cpu().tolist() == [0.0, 0.0, -np.inf, 0.0, np.inf]


# ------------------------------------------------------------------------------------------------ metrics
@functools.lru_cache(maxsize=None)
def _distances(case, spacing):
    """Per class the two reference distance sets: None where both masks are empty, () where exactly one is."""
    pred, gt, nc = K.metric_case(case)
    dists = []
    for c in range(1, nc + 1):
        a, b = pred == c, gt == c
        if a.any() and b.any():
            dists.append(R.surface_distances_ref(a, b, spacing))
        else:
            dists.append(() if a.any() or b.any() else None)
    return dists


def _reference(case, spacing, tau):
    """fp64 [nc, 4] metrics (the distances are computed once per case and spacing), and the distance sets."""
    dists = _distances(case, spacing)
    want = np.empty((len(dists), 4))
    for c, d in enumerate(dists):
        if d is None:
            want[c] = np.nan
        elif not d:
            want[c] = (0.0, np.inf, np.inf, np.inf)
        else:
            want[c] = R.metrics_from_distances(d[0], d[1], tau)[0]
    return want, dists


def _assert_metrics(got, want, what):
    """got fp32 [nc, 4] against want fp64: NSD and HD exact (the fp32 rounding of the reference), HD95 and ASSD within
    2^-22 relative; NaN and inf in the same places."""
    got64 = got.astype(np.float64)
    assert np.array_equal(np.isnan(got64), np.isnan(want)), what
    assert np.array_equal(np.isposinf(got64), np.isposinf(want)), what
    f = np.isfinite(want).all(axis=1)
    assert np.array_equal(got[f, 0], want[f, 0].astype(np.float32)), (what, "nsd")
    assert np.array_equal(got[f, 1], want[f, 1].astype(np.float32)), (what, "hd")
    for k, name in ((2, "hd95"), (3, "assd")):
        err = np.abs(got64[f, k] - want[f, k])
        assert (err <= 2.0 ** -22 * np.abs(want[f, k])).all(), (what, name, float(err.max()))
    assert (got[~f & ~np.isnan(want[:, 0]), 0] == 0).all()               # exactly one mask empty: NSD 0


@pytest.mark.parametrize("case", ["five", "thirteen"])
@pytest.mark.parametrize("spacing", [(1, 1, 1), (2, 1, 1)], ids=str)
def test_surface_metrics_integer_spacings(gpu, case, spacing):
    pred, gt, nc = K.metric_case(case)
    pd, gd = _dev(pred, gpu), _dev(gt, gpu).float()
    keep = (pd.clone(), gd.clone())
    for tau in (1.0, 1.5, 3.0):
        want, _ = _reference(case, spacing, tau)
        got = surface.surface_metrics(pd, gd, num_class=nc, spacing=spacing, tolerance=tau)
        assert got.dtype == torch.float32 and tuple(got.shape) == (1, nc, 4) and got.device == pd.device
        _assert_metrics(got[0].cpu().numpy(), want, (case, spacing, tau))
    assert torch.equal(pd, keep[0]) and torch.equal(gd, keep[1])         # the caller's tensors are left unchanged
    if case == "thirteen":
        w = _reference(case, spacing, 1.0)[0]
        assert np.isnan(w[8]).all() and np.isposinf(w[4, 1:]).all() and np.isposinf(w[6, 1:]).all()
        assert w[4, 0] == 0 and w[6, 0] == 0


@pytest.mark.parametrize("case", ["five", "thirteen"])
def test_surface_metrics_non_integer_spacing(gpu, case):
    pred, gt, nc = K.metric_case(case)
    want, dists = _reference(case, NONINT, NONINT_TAU)
    assert np.array_equal(want, R.metrics_ref(pred, gt, nc, NONINT, NONINT_TAU), equal_nan=True)
    for d in dists:                                                      # a condition on the inputs, not on the code
        if d:
            for v in d:
                assert (np.abs(v - NONINT_TAU) > 2.0 ** -20 * NONINT_TAU).all()
    got = surface.surface_metrics(_dev(pred, gpu), _dev(gt, gpu), num_class=nc, spacing=NONINT, tolerance=NONINT_TAU)
    _assert_metrics(got[0].cpu().numpy(), want, (case, NONINT))


def test_surface_metrics_batch_per_class_tolerance_and_percentile(gpu):
    """S = 2 (the second sample is the first with pred and gt exchanged and class 1 removed from its pred), a tolerance
    per class, another percentile, int32 ground truth."""
    pred, gt, nc = K.metric_case("five")
    p2, g2 = gt.copy(), pred.copy()
    p2[p2 == 1] = 0
    tol = [1.0, 2.0, 0.5, 3.0, 1.5]
    P = _dev(np.stack([pred, p2]), gpu)
    G = _dev(np.stack([gt, g2]).astype(np.int32), gpu)
    got = surface.surface_metrics(P, G, num_class=nc, spacing=(2, 1, 1), tolerance=tol, percentile=50.0).cpu().numpy()
    assert got.shape == (2, nc, 4)
    for s, (a, b) in enumerate(((pred, gt), (p2, g2))):
        _assert_metrics(got[s], R.metrics_ref(a, b, nc, (2, 1, 1), tol, 50.0), ("batch", s))
    assert got[1, 0].tolist() == [0.0, np.inf, np.inf, np.inf]
    one = surface.surface_metrics(P[0], G[0], num_class=nc, spacing=(2, 1, 1), tolerance=tol, percentile=50.0)
    assert np.array_equal(one.cpu().numpy()[0], got[0], equal_nan=True)  # [Z, Y, X] is a batch of one


def test_empty_mask_rules(gpu):
    pred = torch.zeros((4, 5, 6), dtype=torch.int64, device=gpu)
    gt = torch.zeros((4, 5, 6), dtype=torch.float32, device=gpu)
    gt[1:3, 1:3, 1:3] = 1
    pred[0, 0, 0] = 3
    pred[1:3, 1:3, 1:4] = 4
    gt[1:3, 1:3, 3:5] = 4
    got = surface.surface_metrics(pred, gt, num_class=4)[0].cpu().numpy()
    assert got[0].tolist() == [0.0, np.inf, np.inf, np.inf] and got[2].tolist() == [0.0, np.inf, np.inf, np.inf]
    assert np.isnan(got[1]).all() and np.isfinite(got[3]).all()
    _assert_metrics(got, R.metrics_ref(pred.cpu().numpy(), gt.cpu().numpy(), 4), "empty rules")
    nothing = surface.surface_metrics(torch.zeros_like(pred), torch.zeros_like(gt), num_class=2)
    assert torch.isnan(nothing).all()


# ------------------------------------------------------------------------------------------------ evaluate_amos
def test_get_surface_scores(gpu):
    import evaluate_amos
    pred, gt, nc = K.metric_case("five")
    p2, g2 = gt.copy(), pred.copy()
    P = np.stack([pred, p2])
    G = np.stack([gt, g2])
    am = _dev(P, gpu)
    labels = _dev(G.astype(np.float32), gpu)[:, None]                    # [S, 1, D, H, W]
    g = torch.Generator(device="cpu").manual_seed(45)
    logits = torch.randn((2, nc + 1) + pred.shape, generator=g).to(gpu)
    logits.scatter_(1, am[:, None], 10.0)                                # the argmax of the logits is the label map
    keep = (logits.clone(), labels.clone(), am.clone())
    tau, sp = 1.5, (2, 1, 1)
    want = np.stack([R.metrics_ref(a, b, nc, sp, tau) for a, b in ((pred, gt), (p2, g2))]).mean(axis=0)
    from_map = evaluate_amos.get_surface_scores(am, labels, 0, num_class=nc, spacing=sp, tolerance=tau)
    from_logits = evaluate_amos.get_surface_scores(logits, labels, 0, num_class=nc, spacing=sp, tolerance=tau)
    flat = evaluate_amos.get_surface_scores(am, labels[:, 0], 0, num_class=nc, spacing=sp, tolerance=tau)
    assert torch.equal(from_logits[3], am) and from_logits[3].dtype == torch.int64 and from_map[3] is am
    for res in (from_map, from_logits, flat):
        nsd, hd95, assd, _ = res
        assert len(nsd) == len(hd95) == len(assd) == nc
        assert all(v.dim() == 0 and v.is_cuda and v.dtype == torch.float32 for v in nsd + hd95 + assd)
        # the batch mean is taken in fp64 before the one fp32 store: the bounds of surface_metrics hold
        assert [float(x) for x in nsd] == want[:, 0].astype(np.float32).tolist()
        for k, vals in ((2, hd95), (3, assd)):
            v = np.array([float(x) for x in vals])
            assert (np.abs(v - want[:, k]) <= 2.0 ** -22 * np.abs(want[:, k])).all(), k
    for a, b in zip(from_map[:3], from_logits[:3]):
        assert [float(x) for x in a] == [float(x) for x in b]
    assert torch.equal(logits, keep[0]) and torch.equal(labels, keep[1]) and torch.equal(am, keep[2])
    # inf and NaN propagate through the batch mean
    am2 = am.clone()
    am2[0][am2[0] == 2] = 0
    lab2 = labels.clone()
    lab2[lab2 == 5] = 0
    am2[am2 == 5] = 0
    nsd, hd95, assd, _ = evaluate_amos.get_surface_scores(am2, lab2, 0, num_class=nc)
    assert float(nsd[1]) < 1 and np.isposinf(float(hd95[1])) and np.isposinf(float(assd[1]))
    assert np.isnan(float(nsd[4])) and np.isnan(float(hd95[4])) and np.isnan(float(assd[4]))
