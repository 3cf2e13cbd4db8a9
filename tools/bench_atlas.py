"""Atlas path timing: the three kernels of csrc/atlas.hip at the training patch (64 x 192 x 192 from a 13 x 128 x 256 x
256 atlas and a 512 x 512 x 160 image), each next to the ATen composition it replaces, in the same run:

  crop    u3d.data.atlas_crop                      vs  device F.interpolate (nearest) to the image + crop_transpose
          (+ peak device memory of each; the device interpolate is the float32 formula, timed only)
  pairs   utils.organ_atlas_pairs, forward and     vs  cat([softmax(preds, 1)[0, 1:].unsqueeze(1), catlas.unsqueeze(1)],
          forward + backward                           1)[index].float() and its autograd backward
  dice    evaluate_amos.get_dice(..., atlas)       vs  the reference's Python loop (evaluate_amos.py:144-151) on the device

Times are device events around `--iters` calls after `--warmup`, alternating the two sides. Writes one JSON per kernel
into --out and prints them as one JSON line.

    python tools/bench_atlas.py [--out profiles] [--iters 20]
"""
import argparse
import json
import os
import sys

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [os.path.join(REPO, "multimodal-pl_amd"), REPO]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

PATCH = (64, 192, 192)          # (d, h, w)
IMAGE = (512, 512, 160)         # [H, W, D]
ATLAS = (13, 128, 256, 256)
OFFSETS = (101, 57, 33)         # (b, c, a)


def timed(fns, iters, warmup):
    """ms per call of each fn, the calls of the different fns alternating inside one window each."""
    for _ in range(warmup):
        for f in fns:
            f()
    torch.cuda.synchronize()
    total = [0.0] * len(fns)
    for _ in range(iters):
        for i, f in enumerate(fns):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            f()
            b.record()
            b.synchronize()
            total[i] += a.elapsed_time(b)
    return [t / iters for t in total]


def peak_mb(f):
    torch.cuda.synchronize()
    torch.cuda.empty_cache()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    f()
    torch.cuda.synchronize()
    return (torch.cuda.max_memory_allocated() - base) / 2 ** 20


def bench_crop(dev, iters, warmup):
    from u3d import data
    g = torch.Generator().manual_seed(0)
    atlas = torch.rand(ATLAS, generator=g).to(dev)
    cd, ch, cw = PATCH
    crop = (ch, cw, cd)

    def native():
        return data.atlas_crop(atlas, IMAGE, OFFSETS, crop)

    def aten():
        return data.crop_transpose(F.interpolate(atlas.unsqueeze(0), IMAGE)[0], OFFSETS, crop)
    n_ms, a_ms = timed([native, aten], iters, warmup)
    mism = int((native() != aten()).sum())
    return {"metric": "atlas crop ms per call (13 x 64 x 192 x 192 from a 13 x 128 x 256 x 256 atlas, image 512 x 512 x 160)",
            "native_ms": n_ms, "aten_interpolate_crop_ms": a_ms, "native_peak_mb": peak_mb(native),
            "aten_peak_mb": peak_mb(aten), "atlas_mb": atlas.numel() * 4 / 2 ** 20,
            "elements_differing_from_float32_device_interpolate": mism}


def bench_pairs(dev, iters, warmup):
    import utils
    g = torch.Generator().manual_seed(1)
    logits = torch.randn((1, 14) + PATCH, generator=g).to(dev).requires_grad_(True)
    catlas = torch.rand((13,) + PATCH, generator=g).to(dev)
    res = {"metric": "organ / atlas pairs ms per call at 1 x 14 x 64 x 192 x 192"}
    for name, index in (("flist6", [0, 2, 3, 7, 8, 11]), ("clist13", list(range(13)))):
        w = torch.randn((len(index), 2) + PATCH, generator=g).to(dev)

        def native():
            return utils.organ_atlas_pairs(logits, catlas, index)

        def aten():
            return torch.cat([torch.softmax(logits, 1)[0, 1:].unsqueeze(1), catlas.unsqueeze(1)], 1)[index].float()

        def both(f):
            def run():
                logits.grad = None
                (f() * w).sum().backward()
            return run
        with torch.no_grad():
            nf, af = timed([native, aten], iters, warmup)
        nb, ab = timed([both(native), both(aten)], iters, warmup)
        res[name] = {"native_fwd_ms": nf, "aten_fwd_ms": af, "native_fwd_bwd_ms": nb, "aten_fwd_bwd_ms": ab,
                     "max_abs_diff_fwd": float((native() - aten()).abs().max())}
    res["note"] = "fwd_bwd includes the weighted sum that feeds the backward on both sides"
    return res


def bench_dice(dev, iters, warmup):
    import evaluate_amos as E
    g = torch.Generator().manual_seed(2)
    preds = (torch.randn((1, 14) + PATCH, generator=g) * 2).to(dev)
    labels = torch.randint(0, 14, (1,) + PATCH, generator=g).float().to(dev)
    atlas = torch.rand((1, 13) + PATCH, generator=g).to(dev)

    def native():
        return E.get_dice(preds, labels, 1, atlas)

    def loop():      # evaluate_amos.py:130-151 of the reference, on the device
        pr = F.softmax(preds, dim=1)
        am = torch.argmax(pr, dim=1)
        d, s, p = [], [], []
        for l in range(13):
            cpred = (pr[:, l + 1] + 0.15) > (1 - atlas[:, l])
            d.append(E.dice_score(cpred, labels == (l + 1)))
            s.append(E.senc_score(cpred, labels == (l + 1)))
            p.append(E.spec_score(cpred, labels == (l + 1)))
        return d, s, p, am
    n_ms, a_ms = timed([native, loop], iters, warmup)
    a, b = native(), loop()
    diff = max(abs(float(x) - float(y)) for k in range(3) for x, y in zip(a[k], b[k]))
    return {"metric": "atlas-gated Dice ms per call at 1 x 14 x 64 x 192 x 192, 13 organs", "native_ms": n_ms,
            "aten_python_loop_ms": a_ms, "max_abs_metric_diff": diff, "argmax_equal": bool(torch.equal(a[3], b[3]))}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--out", default=os.path.join(REPO, "profiles"))
    p.add_argument("--iters", type=int, default=20)
    p.add_argument("--warmup", type=int, default=3)
    a = p.parse_args()
    dev = torch.device("cuda:0")
    os.makedirs(a.out, exist_ok=True)
    allres = {}
    for name, fn in (("atlas_crop", bench_crop), ("atlas_pairs", bench_pairs), ("atlas_dice", bench_dice)):
        r = fn(dev, a.iters, a.warmup)
        r["source"] = "tools/bench_atlas.py, MI355X, device events, %d calls after %d warm-up" % (a.iters, a.warmup)
        with open(os.path.join(a.out, f"{name}_bench.json"), "w") as f:
            json.dump(r, f, indent=1)
            f.write("\n")
        allres[name] = r
        torch.cuda.empty_cache()
    print(json.dumps(allres))


if __name__ == "__main__":
    main()
