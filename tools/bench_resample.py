"""Orientation / spacing resampling timing: u3d.data.GridPlan.apply (csrc/resample.hip) on an AMOS-like CT case, raw
int16 512 x 512 x 100 at 0.75 x 0.75 x 5 mm resampled to (1, 1, 2) mm (384 x 384 x 248), the image trilinear and the
uint8 label nearest, next to torch.nn.functional.grid_sample on the same device producing the same fp32 image from an
fp32 copy of the source and a [.., 3] fp32 grid: what a user would run today (its image agrees with the kernel's to
fp32 rounding of the normalised grid; the largest difference is recorded).

  unpermuted   the file is RAS already: the source's contiguous axis is output axis 2 (the case the kernel is shaped for)
  permuted     the same volume stored as [100, 512, 512] with codes "SAR": output axis 2 reads the source's slowest axis

Per variant and call: ms (device events around --calls back-to-back calls, median over --reps after a warm-up round;
the sources rotate over --copies buffers whose sum exceeds the Infinity Cache, so a call does not find its source
resident from the call before), the bytes the call has to move (source once, output once, tables) and that over
8 TB/s as the floor.

Writes --out/resample.json and prints it as one JSON line.

    python tools/bench_resample.py [--out profiles] [--reps 7] [--calls 20] [--shape 512 512 100]
"""
import argparse
import json
import os
import sys

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [os.path.join(REPO, "multimodal-pl_amd"), REPO]
import numpy as np  # noqa: E402
import torch  # noqa: E402

HBM_PEAK, HBM_ACHIEVABLE = 8e12, 6.3e12
ZOOMS = (0.75, 0.75, 5.0)


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


def affine_for(codes, zooms):
    world = {"L": (0, -1), "R": (0, 1), "P": (1, -1), "A": (1, 1), "I": (2, -1), "S": (2, 1)}
    A = np.zeros((4, 4))
    for a, c in enumerate(codes):
        A[world[c][0], a] = world[c][1] * zooms[a]
    A[3, 3] = 1
    return A


def grid_for(plan, dev):
    """The normalised fp32 grid [1, n0, n1, n2, 3] that makes grid_sample, reading the volume as stored, produce the
    plan's output: component x (y, z) addresses file axis 2 (1, 0), so it carries the coordinates of the output axis
    that reads that file axis. (No flips: the bench's affines have none.)"""
    assert not any(plan.flip)
    g = []
    for i in range(3):
        n = plan.src_shape[plan.perm[i]]
        c = plan.source_coordinate(i, np.arange(plan.out_shape[i]))
        g.append(torch.from_numpy(2.0 * c / max(n - 1, 1) - 1.0).float().to(dev))
    mesh = torch.meshgrid(*g, indexing="ij")
    return torch.stack([mesh[plan.perm.index(a)] for a in (2, 1, 0)], dim=-1)[None].contiguous()


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(REPO, "profiles"))
    p.add_argument("--reps", type=int, default=7)
    p.add_argument("--calls", type=int, default=20)
    p.add_argument("--copies", type=int, default=6)
    p.add_argument("--shape", type=int, nargs=3, default=[512, 512, 100])
    a = p.parse_args()
    from u3d import data
    dev = torch.device("cuda:0")
    shape = tuple(a.shape)
    gen = torch.Generator(device=dev).manual_seed(0)
    ras_img = (300.0 * torch.randn(shape, device=dev, generator=gen)).round().clamp(-1024, 3000).to(torch.int16)
    ras_lab = torch.randint(0, 14, shape, device=dev, generator=gen).to(torch.uint8)
    res = {"metric": "orientation / spacing resampling, int16 %d x %d x %d at %s mm to (1, 1, 2) mm" % (shape + (ZOOMS,)),
           "reps": a.reps, "calls_per_rep": a.calls, "source_copies": a.copies, "variants": {},
           "source": "tools/bench_resample.py, MI355X, device events around back-to-back calls, median of reps after one "
                     "warm-up round; sources rotate over the copies"}
    for name, codes, order in (("unpermuted", "RAS", (0, 1, 2)), ("permuted", "SAR", (2, 1, 0))):
        img = ras_img.permute(order).contiguous()
        lab = ras_lab.permute(order).contiguous()
        zooms = tuple(ZOOMS[o] for o in order)
        plan = data.spacing_plan(img.shape, affine_for(codes, zooms))
        imgs = [img.clone() for _ in range(a.copies)]
        labs = [lab.clone() for _ in range(a.copies)]
        V_in, V_out = img.numel(), int(np.prod(plan.out_shape))
        tables = sum(n * (4 + 8) for n in plan.out_shape)
        v = {"codes": codes, "src_shape": list(img.shape), "out_shape": list(plan.out_shape), "perm": list(plan.perm),
             "calls": {}}
        calls = {
            "image_linear_int16": (lambda i: plan.apply(imgs[i % a.copies], "linear"), 2 * V_in + 4 * V_out + tables),
            "label_nearest_uint8": (lambda i: plan.apply(labs[i % a.copies], "nearest"), V_in + V_out + tables),
        }
        fimgs = [x.float() for x in imgs]
        grid = grid_for(plan, dev)
        f5 = [x[None, None] for x in fimgs]
        gs = lambda i: torch.nn.functional.grid_sample(f5[i % a.copies], grid, mode="bilinear",  # noqa: E731
                                                       padding_mode="border", align_corners=True)
        calls["image_linear_fp32"] = (lambda i: plan.apply(fimgs[i % a.copies], "linear"), 4 * V_in + 4 * V_out + tables)
        calls["grid_sample_fp32"] = (gs, 4 * V_in + 4 * V_out + 12 * V_out)
        for cname, (fn, nbytes) in calls.items():
            med, lo, hi = timed(fn, a.reps, a.calls)
            v["calls"][cname] = {"ms_median": med, "ms_min": lo, "ms_max": hi, "bytes": nbytes,
                                 "floor_ms_at_8TBps": nbytes / HBM_PEAK * 1e3,
                                 "floor_ms_at_6.3TBps": nbytes / HBM_ACHIEVABLE * 1e3,
                                 "achieved_TBps": nbytes / (med * 1e-3) / 1e12}
        ours = plan.apply(fimgs[0], "linear")
        theirs = gs(0)[0, 0]
        v["max_abs_diff_vs_grid_sample"] = float((ours - theirs).abs().max())
        v["grid_sample_over_kernel_fp32"] = v["calls"]["grid_sample_fp32"]["ms_median"] / \
            v["calls"]["image_linear_fp32"]["ms_median"]
        v["grid_sample_over_kernel_int16"] = v["calls"]["grid_sample_fp32"]["ms_median"] / \
            v["calls"]["image_linear_int16"]["ms_median"]
        v["case_ms_image_plus_label"] = v["calls"]["image_linear_int16"]["ms_median"] + \
            v["calls"]["label_nearest_uint8"]["ms_median"]
        res["variants"][name] = v
        del imgs, labs, fimgs, f5, grid
        torch.cuda.empty_cache()
    os.makedirs(a.out, exist_ok=True)
    with open(os.path.join(a.out, "resample.json"), "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
