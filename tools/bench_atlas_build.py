"""Atlas construction timing: u3d.data.AtlasBuilder over synthetic label volumes of varying shape near 512 x 512 x 100
(the mean shape is the atlas shape, as atlas_gen_mm.py:100-111 takes it), next to the scipy restatement of the same
lines on this machine's CPU.

  add      ms per AtlasBuilder.add (device events; canonical uint8 input: presence pass, finalize, gather) and the
           achieved GB/s against the traffic model 1 B gathered + 8 B read-modify-write per atlas voxel, on volumes
           with an independent random code per voxel and on volumes of constant 16 x 16 x 8 cells
  finish   ms per AtlasBuilder.finish(sigma=3): normalise + three blur passes over all 15 planes
  scipy    seconds for ONE case: fifteen ndimage.zoom(label == l, order=0) calls (atlas_gen_mm.py:126-135), and for one
           organ's float64 gaussian_filter(sigma=3) (:144), one thread as the reference runs them

Writes --out/atlas_build.json and prints it as one JSON line.

    python tools/bench_atlas_build.py [--out profiles] [--cases 20]
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

L = 15


def shapes(n, seed=0):
    g = np.random.default_rng(seed)
    return [(int(g.integers(448, 577)), int(g.integers(448, 577)), int(g.integers(70, 131))) for _ in range(n)]


def blobs(s, dev, gen):
    """A label volume of constant 16 x 16 x 8 cells (spatially coherent codes, as a segmentation's are)."""
    cells = [(s[0] + 15) // 16, (s[1] + 15) // 16, (s[2] + 7) // 8]
    low = torch.randint(0, 17, cells, dtype=torch.uint8, device=dev, generator=gen)
    full = low.repeat_interleave(16, 0).repeat_interleave(16, 1).repeat_interleave(8, 2)
    return full[:s[0], :s[1], :s[2]].contiguous()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(REPO, "profiles"))
    p.add_argument("--cases", type=int, default=20)
    p.add_argument("--no-scipy", action="store_true")
    a = p.parse_args()
    from u3d import data
    dev = torch.device("cuda:0")
    shp = shapes(a.cases)
    atlas_shape = data.average_shape(shp)
    V = atlas_shape[0] * atlas_shape[1] * atlas_shape[2]
    gen = torch.Generator(device=dev).manual_seed(0)
    builder = data.AtlasBuilder(atlas_shape, L, dev)
    warm = torch.randint(0, 17, shp[0], dtype=torch.uint8, device=dev, generator=gen)
    for _ in range(2):                       # warm-up: module load, index tables of the first shape
        builder.add(warm)
    builder.acc.zero_()
    builder.counts.zero_()
    add_ms, blob_ms, first = [], [], None
    for s in shp:
        lab = torch.randint(0, 17, s, dtype=torch.uint8, device=dev, generator=gen)
        first = lab if first is None else first
        builder._table(s[0], atlas_shape[0]), builder._table(s[1], atlas_shape[1]), builder._table(s[2], atlas_shape[2])
        for dst, vol in ((add_ms, lab), (blob_ms, blobs(s, dev, gen))):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            builder.add(vol)
            e1.record()
            e1.synchronize()
            dst.append(e0.elapsed_time(e1))
    assert int(builder.counts.min()) == 2 * a.cases
    fin_ms = []
    for _ in range(3):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        atlas = builder.finish(3.0)
        e1.record()
        e1.synchronize()
        fin_ms.append(e0.elapsed_time(e1))
        del atlas
    add_med = float(np.median(add_ms))
    res = {"metric": "atlas construction, %d synthetic uint8 cases near 512 x 512 x 100, 15 labels" % a.cases,
           "atlas_shape": list(atlas_shape), "atlas_voxels": V,
           "add_ms_median": add_med, "add_ms_min": float(min(add_ms)), "add_ms_max": float(max(add_ms)),
           "add_traffic_model_bytes": 9 * V, "add_gbps_model": 9 * V / (add_med * 1e-3) / 1e9,
           "add_blobs_ms_median": float(np.median(blob_ms)),
           "add_blobs_gbps_model": 9 * V / (float(np.median(blob_ms)) * 1e-3) / 1e9,
           "add_note": "add_ms: an independent random code per voxel, the worst case for the per-label planes (a wave's "
                       "64 voxels scatter over 15 planes); add_blobs: constant 16 x 16 x 8 cells, as organs are",
           "finish_ms_median": float(np.median(fin_ms)), "finish_ms_first": float(fin_ms[0]),
           "source": "tools/bench_atlas_build.py, MI355X, device events"}
    if not a.no_scipy:
        from scipy import ndimage
        lab = first.cpu().numpy()
        t0 = time.perf_counter()
        one = None
        for l in range(1, L + 1):
            mask = (lab == l).astype(np.float32)
            if mask.sum() > 0:
                one = ndimage.zoom(mask, [t / n for t, n in zip(atlas_shape, mask.shape)], order=0)
        t1 = time.perf_counter()
        ndimage.gaussian_filter(one.astype(np.float64), sigma=3)
        t2 = time.perf_counter()
        res["scipy_zoom_one_case_15_labels_s"] = t1 - t0
        res["scipy_gaussian_filter_one_organ_s"] = t2 - t1
        res["scipy_note"] = "same machine's CPU, the reference's calls; its finish runs the filter once per organ"
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "atlas_build.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
