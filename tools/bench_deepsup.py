"""Deep-supervision loss, forward + backward: the fused multi-level operation (u3d.loss.deep_supervision_loss, two
launches + one) against the composed form it replaces (per level a nearest resize of the target, partial_loss
forward and backward: three resized targets and about a dozen launches). Shapes: the levels of the feam3 bench patch,
1 x 14 x (8x24x24, 16x48x48, 32x96x96) logits (NDHWC storage, as the native heads return them), target 64x192x192.

Device events around each call, a warm-up of both forms, the two forms alternating in one run; per form the median
and the spread over the rounds (each round = ``--inner`` calls between one event pair, so the host's launch rate is
inside the figure, as it is inside a training step). Writes one JSON line to stdout and, with --out, to a file."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [os.path.join(REPO, "multimodal-pl_amd"), REPO]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--target", type=int, nargs=3, default=[64, 192, 192])
    p.add_argument("--batch", type=int, default=1)
    p.add_argument("--classes", type=int, default=14)
    p.add_argument("--rounds", type=int, default=30)
    p.add_argument("--inner", type=int, default=20)
    p.add_argument("--warmup", type=int, default=20)
    p.add_argument("--out", default=None)
    a = p.parse_args()
    from u3d import loss as L
    dev = torch.device("cuda:0")
    S, C, sp = a.batch, a.classes, tuple(a.target)
    g = torch.Generator().manual_seed(0)
    levels = [tuple(n // r for n in sp) for r in (8, 4, 2)]
    deep = [(torch.randn((S,) + lv + (C,), generator=g) * 2).to(dev).permute(0, 4, 1, 2, 3).requires_grad_(True)
            for lv in levels]
    target = torch.randint(0, C, (S, 1) + sp, generator=g).float().to(dev)
    mvec = torch.tensor([1, 1, 1, 1, 1, 0, 1, 1, 0, 1, 1, 1, 1, 1, 0], dtype=torch.int64, device=dev)
    w = L.class_weights([mvec], C, dev)

    def fused():
        loss = L.deep_supervision_loss(deep, target, [mvec])
        return loss, torch.autograd.grad(loss, deep)

    def composed():
        loss = 0.0
        for x, lw in zip(deep, L.DEEP_WEIGHTS):
            ct = F.interpolate(target, x.shape[2:], mode="nearest").squeeze(1)
            loss = loss + L.partial_loss(x, ct, w, mode=L.MODE_SOFTMAX, uce=False) * lw
        return loss, torch.autograd.grad(loss, deep)

    forms = {"fused": fused, "composed": composed}
    for _ in range(a.warmup):
        for f in forms.values():
            f()
    torch.cuda.synchronize()
    (lf, gf), (lc, gc) = fused(), composed()
    diff = max(((x - y).abs().max() / y.abs().max()).item() for x, y in zip(gf, gc))
    times = {k: [] for k in forms}
    for _ in range(a.rounds):
        for k, f in forms.items():   # alternating
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(a.inner):
                f()
            e1.record()
            e1.synchronize()
            times[k].append(e0.elapsed_time(e1) * 1e3 / a.inner)
    res = {"metric": "deep-supervision loss fwd+bwd, us per call (device events, host launches included)",
           "levels": [list(lv) for lv in levels], "target": list(sp), "batch": S, "classes": C,
           "rounds": a.rounds, "inner": a.inner, "loss_fused": lf.item(), "loss_composed": lc.item(),
           "grad_max_rel_diff": diff}
    for k, v in times.items():
        res[f"{k}_us_median"] = statistics.median(v)
        res[f"{k}_us_min"], res[f"{k}_us_max"] = min(v), max(v)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
