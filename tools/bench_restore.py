"""Timing and peak memory of the way back from the network's output to a label map on the case's own voxels
(u3d.data.restore_prediction, keep_largest_per_label; csrc/resample.hip, csrc/ccl.hip) next to the paths they replace.

The case: a 512 x 512 x 120 file stored LPS at 0.8 x 0.8 x 2.5 mm, resampled to RAS (1, 1, 2) mm (410 x 410 x 150); the
prediction is 14 channels on a 400 x 400 x 100 crop of that grid.

  restore            restore_prediction(scores [14, 400, 400, 100] contiguous): one fused kernel, uint8 out
  restore_view       the same scores stored as the network leaves them, [14, 100, 400, 400], passed as a permuted view
                     (no copy: output axis 2 then reads the source's slowest axis)
  composed           what it replaces: plan_w.apply(scores, "linear") (14 fp32 volumes on the file's grid), torch.argmax
                     (int64), the cast to uint8 and the mask of the voxels outside the crop
  keep_largest       keep_largest_per_label on a 512 x 512 x 120 label map of 13 organs with specks around them
  thirteen_labellings  what it replaces: per label largest_component(x == l, num_limit=1024, min_filter=0) and torch.where
                     (one labelling, one selection and one host read per label)

Per call: ms (device events around --calls back-to-back calls, median over --reps after a warm-up round; the sources
rotate over buffers whose sum exceeds the Infinity Cache), the peak of torch.cuda.max_memory_allocated above what was
allocated before the call, the bytes the kernels have to move and those over 6.3 TB/s as the floor. The outputs of the
paired paths are compared and the result recorded.

Writes --out/restore.json and prints it as one JSON line.

    python tools/bench_restore.py [--out profiles] [--reps 5] [--calls 8]
"""
import argparse
import json
import os
import sys

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [os.path.join(REPO, "multimodal-pl_amd"), REPO]
import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_ACHIEVABLE = 6.3e12
FILE_SHAPE, ZOOMS, CODES = (512, 512, 120), (0.8, 0.8, 2.5), "LPS"
CROP, CROP_ORIGIN, CHANNELS = (400, 400, 100), (5, 6, 20), 14


def timed(fn, reps, calls):
    ms = []
    for _ in range(reps + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for i in range(calls):
            fn(i)
        e1.record()
        e1.synchronize()
        ms.append(e0.elapsed_time(e1) / calls)
    return float(np.median(ms[1:])), float(min(ms[1:])), float(max(ms[1:]))      # the first round warms up


def peak_bytes(fn):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    out = fn(0)
    torch.cuda.synchronize()
    peak = torch.cuda.max_memory_allocated() - base
    del out
    return int(peak)


def affine_for(codes, zooms):
    world = {"L": (0, -1), "R": (0, 1), "P": (1, -1), "A": (1, 1), "I": (2, -1), "S": (2, 1)}
    A = np.zeros((4, 4))
    for a, c in enumerate(codes):
        A[world[c][0], a] = world[c][1] * zooms[a]
    A[3, 3] = 1
    return A


def organs(shape, dev, gen):
    """uint8 label map: 13 ellipsoids on a 4 x 4 lattice of the first two axes, and 40 specks of 2 x 2 x 2 per label."""
    z, y, x = (torch.arange(n, device=dev, dtype=torch.float32) for n in shape)
    lab = torch.zeros(shape, dtype=torch.uint8, device=dev)
    for l in range(1, 14):
        cz, cy, cx = (0.5 + (l - 1) // 4) * shape[0] / 4, (0.5 + (l - 1) % 4) * shape[1] / 4, shape[2] / 2
        r = (shape[0] / 10, shape[1] / 10, shape[2] / 3)
        d = ((z - cz) / r[0])[:, None, None] ** 2 + ((y - cy) / r[1])[None, :, None] ** 2 + \
            ((x - cx) / r[2])[None, None, :] ** 2
        lab[d <= 1] = l
        for _ in range(40):
            p = [int(torch.randint(0, n - 2, (1,), device=dev, generator=gen)) for n in shape]
            lab[p[0]:p[0] + 2, p[1]:p[1] + 2, p[2]:p[2] + 2] = l
    return lab


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(REPO, "profiles"))
    p.add_argument("--reps", type=int, default=5)
    p.add_argument("--calls", type=int, default=8)
    a = p.parse_args()
    from u3d import data
    dev = torch.device("cuda:0")
    gen = torch.Generator(device=dev).manual_seed(0)
    plan = data.spacing_plan(FILE_SHAPE, affine_for(CODES, ZOOMS))
    info = {"plan": plan, "origin": CROP_ORIGIN}
    assert all(o + n <= s for o, n, s in zip(CROP_ORIGIN, CROP, plan.out_shape)), plan.out_shape
    plan_w, valid = plan.inverse().restrict_source(CROP_ORIGIN, CROP)
    V_src, V_out = CHANNELS * int(np.prod(CROP)), int(np.prod(FILE_SHAPE))
    tables = sum(n * (4 + 8) for n in FILE_SHAPE)
    res = {"metric": "restore_prediction and keep_largest_per_label, 14 x %d x %d x %d scores on a crop of the (1, 1, 2) mm "
                     "grid %s back to a %d x %d x %d %s file" % (CROP + (list(plan.out_shape),) + FILE_SHAPE + (CODES,)),
           "reps": a.reps, "calls_per_rep": a.calls, "valid": [list(v) for v in valid], "calls": {},
           "source": "tools/bench_restore.py, MI355X, device events around back-to-back calls, median of reps after one "
                     "warm-up round; sources rotate over the copies; peak = torch.cuda.max_memory_allocated above the "
                     "allocation before the call"}

    # ---- the scores back onto the file's voxels
    scores = [torch.randn((CHANNELS,) + CROP, device=dev, generator=gen) for _ in range(2)]       # 2 x 896 MB
    mask = torch.ones(FILE_SHAPE, dtype=torch.bool, device=dev)
    for i, (lo, hi) in enumerate(valid):
        k = torch.arange(FILE_SHAPE[i], device=dev)
        mask &= ((k >= lo) & (k < hi)).reshape([-1 if d == i else 1 for d in range(3)])

    def composed(i):
        am = plan_w.apply(scores[i % 2], "linear").argmax(0).to(torch.uint8)
        return torch.where(mask, am, torch.zeros_like(am))

    fused = lambda i: data.restore_prediction(scores[i % 2], info)  # noqa: E731
    res["restore_equals_composed"] = bool(torch.equal(fused(0), composed(0)))
    calls = {"restore": (fused, 4 * V_src + V_out + tables),
             "composed": (composed, 4 * V_src + 4 * CHANNELS * V_out      # the linear kernel
                          + 4 * CHANNELS * V_out + 8 * V_out              # argmax
                          + 8 * V_out + V_out                             # cast
                          + 3 * V_out)}                                   # where
    for name, (fn, nbytes) in calls.items():
        med, lo, hi = timed(fn, a.reps, a.calls)
        res["calls"][name] = {"ms_median": med, "ms_min": lo, "ms_max": hi, "peak_bytes": peak_bytes(fn),
                              "bytes": nbytes, "floor_ms_at_6.3TBps": nbytes / HBM_ACHIEVABLE * 1e3,
                              "achieved_TBps": nbytes / (med * 1e-3) / 1e12}
    want = fused(0)
    views = [s.permute(0, 3, 1, 2).contiguous().permute(0, 2, 3, 1) for s in scores]              # stored [14, 100, 400, 400]
    del scores
    torch.cuda.empty_cache()
    scores = views
    assert not scores[0].is_contiguous() and tuple(scores[0].shape) == (CHANNELS,) + CROP
    res["restore_view_equals_restore"] = bool(torch.equal(fused(0), want))
    med, lo, hi = timed(fused, a.reps, a.calls)
    nbytes = calls["restore"][1]
    res["calls"]["restore_view"] = {"ms_median": med, "ms_min": lo, "ms_max": hi, "peak_bytes": peak_bytes(fused),
                                    "bytes": nbytes, "floor_ms_at_6.3TBps": nbytes / HBM_ACHIEVABLE * 1e3,
                                    "achieved_TBps": nbytes / (med * 1e-3) / 1e12}
    del scores, views, mask, want
    torch.cuda.empty_cache()

    # ---- the per-organ cleanup
    lab = organs(FILE_SHAPE, dev, gen)
    labs = [lab.clone() for _ in range(10)]                                                       # 10 x 31 MB
    zero = torch.zeros((), dtype=torch.uint8, device=dev)

    def thirteen(i):
        x = labs[i % len(labs)]
        out = x.clone()
        for l in range(1, 14):
            m = x == l
            keep = data.largest_component(m, num_limit=1024, min_filter=0)
            if keep is not None:
                out = torch.where(m & (keep == 0), zero, out)
        return out

    one = lambda i: data.keep_largest_per_label(labs[i % len(labs)], 13)  # noqa: E731
    got, rec = data.keep_largest_per_label(lab, 13, return_record=True)
    res["keep_largest_equals_thirteen_labellings"] = bool(torch.equal(got, thirteen(0)))
    res["keep_largest_record"] = rec.cpu().tolist()
    # codes 1, parents 4 + sizes 4 written; parents read and written, sizes added; parents + sizes of the roots read;
    # codes + parents read, codes written
    kbytes = V_out * (1 + 8 + 8 + 4 + 4 + 1 + 4 + 1)
    # per label: the mask written and read, parents 4 written, read and written, labels 4 written twice and read twice,
    # the selection's pass and its mask, the two wheres
    tbytes = 13 * V_out * (1 + 1 + 1 + 4 + 8 + 16 + 4 + 1 + 5)
    for name, (fn, nbytes) in {"keep_largest": (one, kbytes), "thirteen_labellings": (thirteen, tbytes)}.items():
        med, lo, hi = timed(fn, a.reps, max(1, a.calls // 2))
        res["calls"][name] = {"ms_median": med, "ms_min": lo, "ms_max": hi, "peak_bytes": peak_bytes(fn),
                              "bytes": nbytes, "floor_ms_at_6.3TBps": nbytes / HBM_ACHIEVABLE * 1e3,
                              "achieved_TBps": nbytes / (med * 1e-3) / 1e12}
    c = res["calls"]
    res["composed_over_restore"] = c["composed"]["ms_median"] / c["restore"]["ms_median"]
    res["composed_over_restore_view"] = c["composed"]["ms_median"] / c["restore_view"]["ms_median"]
    res["thirteen_over_keep_largest"] = c["thirteen_labellings"]["ms_median"] / c["keep_largest"]["ms_median"]
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "restore.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
