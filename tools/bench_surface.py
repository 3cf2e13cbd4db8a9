"""Distance transform and surface metrics timing (csrc/edt.hip, u3d.surface) on a 128 x 256 x 256 volume, next to the
scipy restatement (tests/surface_reference.py) on this machine's CPU.

  edt              u3d_edt (three launches), ms by device events, median of --reps after a warm-up, on two masks: Bernoulli
                   0.5 (every search ends after a step or two) and the surface of an ellipsoid (sparse features: long
                   searches, rows and planes without a feature). Next to each: the bytes the three passes move (mask 1 B
                   read and 8 B written; 8 + 8 in place; 8 read and 4 written = 37 B per voxel), the 5 B per voxel any
                   implementation has to move, both over 8 TB/s, and scipy.ndimage.distance_transform_edt's seconds.
  surface_metrics  the whole call (host read included) on a synthetic 13-organ pair of label maps of that size, and the
                   restatement's seconds (per class: crop to the union's box, two erosions, two transforms, the metrics).

Writes --out/surface.json and prints it as one JSON line.

    python tools/bench_surface.py [--out profiles] [--reps 7] [--shape 128 256 256] [--no-scipy]
"""
import argparse
import json
import os
import sys
import time

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [os.path.join(REPO, "multimodal-pl_amd"), REPO]
import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM = 8e12


def timed(fn, reps):
    ms = []
    for _ in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1))
    return float(np.median(ms[1:])), float(min(ms[1:])), float(max(ms[1:]))      # the first run warms up


def organs(shape, num_class, dev, seed, jitter):
    """int64 label map of num_class overlapping ellipsoids; jitter > 0: each moved and scaled a little."""
    g = np.random.default_rng(seed)
    gj = np.random.default_rng([seed, 1])
    zz = torch.arange(shape[0], device=dev).view(-1, 1, 1).double()
    yy = torch.arange(shape[1], device=dev).view(1, -1, 1).double()
    xx = torch.arange(shape[2], device=dev).view(1, 1, -1).double()
    lab = torch.zeros(shape, dtype=torch.int64, device=dev)
    for c in range(1, num_class + 1):
        ctr = np.array([g.uniform(0.25, 0.75) * s for s in shape])
        rad = np.array([g.uniform(0.08, 0.18) * s + 2 for s in shape])
        ctr = ctr + jitter * gj.uniform(-2.5, 2.5, 3)
        rad = rad * (1 + jitter * gj.uniform(-0.1, 0.1, 3))
        inside = ((zz - ctr[0]) / rad[0]) ** 2 + ((yy - ctr[1]) / rad[1]) ** 2 + ((xx - ctr[2]) / rad[2]) ** 2 <= 1
        lab[inside] = c
    return lab


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(REPO, "profiles"))
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--shape", type=int, nargs=3, default=[128, 256, 256])
    p.add_argument("--no-scipy", action="store_true")
    a = p.parse_args()
    from u3d import ops, surface
    from u3d._lib import call, query
    dev = torch.device("cuda:0")
    shape = tuple(a.shape)
    Z, Y, X = shape
    V = Z * Y * X
    spacing = (2.0, 1.0, 1.0)
    s = ops._stream()
    gen = torch.Generator(device=dev).manual_seed(0)
    ell = organs(shape, 1, dev, 3, 0.0)
    masks = {"bernoulli0.5": (torch.rand(shape, device=dev, generator=gen) < 0.5).to(torch.uint8),
             "ellipsoid_surface": surface.mask_surface(ell)}
    out = torch.empty(shape, dtype=torch.float32, device=dev)
    ws = torch.empty(query("u3d_edt_ws_bytes", V), dtype=torch.uint8, device=dev)
    res = {"metric": "distance transform and surface metrics, %d x %d x %d (%d voxels), spacing %s" % (Z, Y, X, V, spacing),
           "shape": list(shape), "voxels": V, "reps": a.reps, "spacing": list(spacing), "edt": {},
           "source": "tools/bench_surface.py, MI355X, device events, median of reps after one warm-up"}
    if not a.no_scipy:
        sys.path.insert(0, os.path.join(REPO, "tests"))
        import surface_cases as K
        import surface_reference as R
    for name, m in masks.items():
        fn = lambda: call("u3d_edt", m.data_ptr(), Z, Y, X, *spacing, 0, 0, out.data_ptr(), ws.data_ptr(), s)  # noqa: E731
        med, lo, hi = timed(fn, a.reps)
        row = {"ms_median": med, "ms_min": lo, "ms_max": hi, "features": int(m.sum().item()),
               "bytes_moved": 37 * V, "moved_floor_ms_at_8TBps": 37 * V / HBM * 1e3,
               "bytes_least": 5 * V, "least_floor_ms_at_8TBps": 5 * V / HBM * 1e3}
        if not a.no_scipy:
            hm = m.cpu().numpy()
            t0 = time.perf_counter()
            want = R.edt_ref(hm, spacing)
            row["scipy_s"] = time.perf_counter() - t0
            got = out.cpu().numpy().astype(np.float64)
            row["max_rel_err_vs_scipy"] = float((np.abs(got - want) / np.maximum(want, 1e-30)).max())
        res["edt"][name] = row
    nc = 13
    gt = organs(shape, nc, dev, 5, 0.0)
    pred = organs(shape, nc, dev, 5, 1.0)
    gtf = gt.float()
    got = {}

    def metrics():
        got["m"] = surface.surface_metrics(pred, gtf, num_class=nc, spacing=spacing, tolerance=1.0)

    med, lo, hi = timed(metrics, a.reps)
    boxes = surface.class_boxes(pred, gtf, nc).cpu().numpy()
    box_vox = int(np.prod(np.maximum(boxes[:, 3:6] - boxes[:, 0:3] + 1, 0), axis=1).sum())
    res["surface_metrics"] = {"ms_median": med, "ms_min": lo, "ms_max": hi, "num_class": nc,
                              "box_voxels_all_classes": box_vox,
                              "voxels_pred": boxes[:, 6].tolist(), "voxels_gt": boxes[:, 7].tolist(),
                              # class boxes: pred 8 B + gt 4 B read; per box voxel: two surfaces (8 + 4 read, 2 written),
                              # two transforms (37 each), two reductions (5 each)
                              "bytes_moved": 12 * V + box_vox * (14 + 74 + 10)}
    res["surface_metrics"]["moved_floor_ms_at_8TBps"] = res["surface_metrics"]["bytes_moved"] / HBM * 1e3
    if not a.no_scipy:
        hp, hg = pred.cpu().numpy(), gt.cpu().numpy()
        t0 = time.perf_counter()
        want = np.empty((nc, 4))
        for c in range(1, nc + 1):
            ca, cb = hp == c, hg == c
            if ca.any() and cb.any():
                want[c - 1] = R.metrics_from_distances(*R.surface_distances_ref(*K.crop_to_union(ca, cb), spacing), 1.0)[0]
            else:
                want[c - 1] = np.nan if not (ca.any() or cb.any()) else (0.0, np.inf, np.inf, np.inf)
        res["surface_metrics"]["scipy_s"] = time.perf_counter() - t0
        res["surface_metrics"]["scipy_note"] = ("same machine's CPU, one thread, each class cropped to its union box "
                                                "first (26 transforms of the full volume would take 26 x the edt row)")
        g = got["m"][0].cpu().numpy().astype(np.float64)
        f = np.isfinite(want)
        res["surface_metrics"]["max_rel_err_vs_scipy"] = float((np.abs(g[f] - want[f]) / np.maximum(want[f], 1e-30)).max())
        for k, key in ((0, "nsd"), (2, "hd95"), (3, "assd")):   # a class missing from a map: null
            res["surface_metrics"][key] = [float(v) if np.isfinite(v) else None for v in g[:, k]]
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "surface.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
