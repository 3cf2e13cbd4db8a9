"""Body mask and crop timing: u3d.data.get_body / body_crop (csrc/ccl.hip) on a synthetic fp32 volume near
400 x 400 x 250 (an elliptic torso with two arms, a table-like slab under it, noise and bright specks), next to the
host restatement of the same lines (scipy: threshold, 2 x 2 x 2 erosion, label, sizes, bounding box) on this machine's
CPU.

  passes   ms per C entry point (device events, median of --reps): threshold + erosion, the labelling (six launches),
           the selection (sizes, pick, mask + bounding box), one box-opening (threshold + six window passes + bounding
           box, ungated), the label range; next to each the bytes it has to move and that / 8 TB/s as the floor
  get_body, body_crop   ms for the whole calls, host reads included
  scipy    seconds for the restatement's get_body on the same volume, one thread

Writes --out/body_crop.json and prints it as one JSON line.

    python tools/bench_body_crop.py [--out profiles] [--reps 7] [--shape 250 400 400]
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


def volume(shape, dev, seed=0):
    """CT-like: air -1000, torso and arms 40, a table slab 200 apart from the body, noise sd 30, bright specks."""
    Z, Y, X = shape
    gen = torch.Generator(device=dev).manual_seed(seed)
    z = torch.arange(Z, device=dev).view(Z, 1, 1).float()
    y = torch.arange(Y, device=dev).view(1, Y, 1).float()
    x = torch.arange(X, device=dev).view(1, 1, X).float()
    torso = ((y - 0.45 * Y) / (0.28 * Y)) ** 2 + ((x - 0.5 * X) / (0.36 * X)) ** 2 < 1
    torso = torso & (z >= 0.04 * Z) & (z < 0.96 * Z)
    arms = (((y - 0.45 * Y) / (0.07 * Y)) ** 2 + (((x - 0.5 * X).abs() - 0.40 * X) / (0.06 * X)) ** 2 < 1) & (z < 0.8 * Z)
    slab = (y >= 0.80 * Y) & (y < 0.84 * Y) & (x >= 0.1 * X) & (x < 0.9 * X)
    vol = torch.full(shape, -1000.0, device=dev)
    vol = torch.where(torso | arms, torch.full_like(vol, 40.0), vol)
    vol = torch.where(slab.expand(shape), torch.full_like(vol, 200.0), vol)
    vol += 30.0 * torch.randn(shape, device=dev, generator=gen)
    specks = torch.rand(shape, device=dev, generator=gen) < 2e-5
    vol = torch.where(specks, torch.full_like(vol, 500.0), vol)
    lab = torch.zeros(shape, device=dev)
    lab[int(0.2 * Z):int(0.8 * Z), int(0.3 * Y):int(0.6 * Y), int(0.05 * X):int(0.95 * X)] = \
        torch.randint(0, 14, (int(0.8 * Z) - int(0.2 * Z), int(0.6 * Y) - int(0.3 * Y), int(0.95 * X) - int(0.05 * X)),
                      device=dev, generator=gen).float()
    return vol.contiguous(), lab


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


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(REPO, "profiles"))
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--shape", type=int, nargs=3, default=[250, 400, 400])
    p.add_argument("--no-scipy", action="store_true")
    a = p.parse_args()
    from u3d import data, ops
    from u3d._lib import call, query
    dev = torch.device("cuda:0")
    shape = tuple(a.shape)
    Z, Y, X = shape
    V = Z * Y * X
    vol, lab = volume(shape, dev)
    s = ops._stream()
    u8 = lambda: torch.empty(shape, dtype=torch.uint8, device=dev)  # noqa: E731
    m, out, tmp = u8(), u8(), u8()
    labels = torch.empty(shape, dtype=torch.int32, device=dev)
    n = torch.empty(1, dtype=torch.int32, device=dev)
    rec = torch.empty(data.REC_LEN, dtype=torch.int32, device=dev)
    ws = torch.empty(query("u3d_ccl_ws_bytes", V), dtype=torch.uint8, device=dev)
    ws2 = torch.empty(query("u3d_ccl_select_ws_bytes"), dtype=torch.uint8, device=dev)

    def opening():
        call("u3d_body_threshold", vol.data_ptr(), Z, Y, X, -200.0, 0, m.data_ptr(), None, s)
        cur, nxt = m, tmp
        for op, (lo, hi) in ((0, (-5, 4)), (1, (-4, 5))):
            for outer, nn, inner in ((1, Z, Y * X), (Z, Y, X), (Z * Y, X, 1)):
                call("u3d_mask_window_axis", cur.data_ptr(), nxt.data_ptr(), outer, nn, inner, lo, hi, op, None, s)
                cur, nxt = nxt, (out if nxt is tmp else tmp)
        call("u3d_nonzero_bbox", cur.data_ptr(), 0, Z, Y, X, rec.data_ptr(), 0, None, s)

    passes = {
        # name: (callable, bytes moved at least)
        "threshold_erode": (lambda: call("u3d_body_threshold", vol.data_ptr(), Z, Y, X, -200.0, 1, m.data_ptr(), None, s),
                            5 * V),
        # mask 1 B read, parents 4 B written; flatten 4 + 4; rank 4 read; relabel 4 read + 4 written (+ root gathers)
        "label": (lambda: call("u3d_ccl_label", m.data_ptr(), Z, Y, X, labels.data_ptr(), n.data_ptr(), ws.data_ptr(), s),
                  25 * V),
        # sizes 4 B read; mask + box 4 B read, 1 B written
        "select": (lambda: call("u3d_ccl_select", labels.data_ptr(), Z, Y, X, n.data_ptr(), 100, 1e6, out.data_ptr(),
                                rec.data_ptr(), ws2.data_ptr(), s), 9 * V),
        "opening_fallback": (opening, (5 + 6 * 2 + 1) * V),
        "label_range": (lambda: call("u3d_nonzero_bbox", lab.data_ptr(), 1, Z, Y, X, rec.data_ptr(), 0, None, s), 4 * V),
    }
    res = {"metric": "body mask and crop, synthetic fp32 volume %d x %d x %d (%d voxels)" % (Z, Y, X, V),
           "shape": list(shape), "voxels": V, "reps": a.reps, "passes": {},
           "source": "tools/bench_body_crop.py, MI355X, device events, median of reps after one warm-up"}
    for name, (fn, nbytes) in passes.items():
        med, lo, hi = timed(fn, a.reps)
        res["passes"][name] = {"ms_median": med, "ms_min": lo, "ms_max": hi, "bytes": nbytes,
                               "floor_ms_at_8TBps": nbytes / HBM * 1e3}
    passes["select"][0]()
    r = rec.cpu().tolist()                       # the selection's record on the full volume
    res["components"] = int(n.item())
    res["get_body_ms"] = timed(lambda: data.get_body(vol), a.reps)[0]
    res["get_body_fallback_ms"] = timed(lambda: data.get_body(vol, min_filter=1e9), a.reps)[0]
    info = {}

    def crop():
        info.update(data.body_crop(vol, lab, 100)[2])

    res["body_crop_ms"] = timed(crop, a.reps)[0]
    res["body_size"], res["body_route"], res["body_bbox"] = info["size"], info["route"], [list(v) for v in info["bbox"]]
    res["select_record"] = r
    if not a.no_scipy:
        sys.path.insert(0, os.path.join(REPO, "tests"))
        import scipy.ndimage as ndi
        import body_crop_reference as R
        hv = vol.cpu().numpy()
        t0 = time.perf_counter()
        er = R.erode2(hv > np.float32(-200))
        t1 = time.perf_counter()
        hl, hn = ndi.label(er)
        t2 = time.perf_counter()
        sizes = np.bincount(hl.reshape(-1), minlength=100)[:100]
        best = int(np.argmax(sizes[1:])) + 1
        hm = hl == best
        t3 = time.perf_counter()
        idx = np.nonzero(hm)
        box = [[int(i.min()) for i in idx], [int(i.max()) for i in idx]]
        t4 = time.perf_counter()
        res["scipy"] = {"threshold_erode_s": t1 - t0, "label_s": t2 - t1, "sizes_mask_s": t3 - t2, "bbox_s": t4 - t3,
                        "get_body_s": t4 - t0, "threads": 1, "components": int(hn),
                        "note": "same machine's CPU, numpy / scipy.ndimage, one thread; the reference's own "
                                "getmaxcomponent sums the label image twice per candidate label on top of this"}
        res["scipy"]["bbox"], res["scipy"]["size"] = box, int(hm.sum())
        res["scipy_agrees"] = bool(hn == res["components"] and r[2] == int(hm.sum()) and [r[3:6], r[6:9]] == box)
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "body_crop.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
