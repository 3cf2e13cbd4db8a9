"""Style discriminator at the driver's shape (train_amos_atlas_final.py:320-379): deep_style_discriminator_output on
13 x 2 x 64 x 192 x 192 with the 32x96x96 / 16x48x48 / 8x24x24 maps, bf16 under autocast. Two timed operations:
  generator pass       forward + data gradient, parameters frozen
  discriminator pass   forward + all parameter gradients, inputs detached
The native module against the torch restatement (tests/disc_reference.py DeepDisc, MIOpen convs) under the same
autocast, the two alternating in one run on the same inputs; medians over the rounds, device events around each call,
host launches included. With --layers, each native kernel of the five inner convs is also timed on its own
(median of 3) with the fraction of the measured bf16 MFMA peak (profiles/r01e_peaks.json: 1950.9 TFLOP/s), beside the
same layer through torch (conv + LeakyReLU under autocast, its data and weight gradients by autograd).
Writes one JSON line to stdout and, with --out, to a file."""
import argparse
import json
import os
import statistics
import sys

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [os.path.join(REPO, "multimodal-pl_amd"), os.path.join(REPO, "tests"), REPO]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

PEAK_BF16_TFLOPS = 1950.9


def timed(fn):
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    fn()
    e1.record()
    e1.synchronize()
    return e0.elapsed_time(e1)


def layer_times(m, x, f_m, reps=3):
    """ms of each inner-conv kernel of the native deep module at this shape, bf16."""
    from u3d import disc
    dt = torch.bfloat16
    B, dev = x.shape[0], x.device
    ndf = m.ndf
    dims = disc.chain_dims(tuple(x.shape[2:]))
    convs = [m.block2[0], m.block3[0], m.block4[0], m.block4[2], m.block4[4]]
    out = []
    for j, c in enumerate(convs):
        i = j + 1
        cin, cout = c.in_channels, c.out_channels
        xin = torch.randn((B, *dims[i - 1], cin), device=dev).to(dt)
        y = torch.empty((B, *dims[i], cout), dtype=dt, device=dev)
        dy = torch.randn(y.shape, device=dev).to(dt)
        dx = torch.empty_like(xin)
        dw = torch.empty_like(c.weight)
        wf, wd = disc.pack_conv_fwd(c.weight.detach(), dt), disc.pack_conv_dgrad(c.weight.detach(), dt)
        xv, yv, dyv, dxv = (disc.View(t, 0, t.shape[4]) for t in (xin, y, dy, dx))
        ops = {"fwd": lambda: disc.conv_fwd(xv, wf, c.bias.detach(), yv),
               "dgrad": lambda: disc.conv_dgrad(dyv, yv, wd, dxv),
               "wgrad": lambda: disc.conv_wgrad(xv, dyv, yv, dw)}
        m_out = B * dims[i][0] * dims[i][1] * dims[i][2]
        gflop = 2.0 * m_out * 64 * cin * cout / 1e9
        row = {"layer": f"{cin}->{cout} @ {'x'.join(map(str, dims[i - 1]))}", "gflop": gflop}
        for k, f in ops.items():
            f()
            ms = statistics.median(timed(f) for _ in range(reps))
            row[f"{k}_ms"] = ms
            row[f"{k}_peak_fraction"] = gflop / ms / PEAK_BF16_TFLOPS
        # the same layer through torch (MIOpen) under autocast: conv + LeakyReLU, and its two gradients by autograd
        xt = xin.permute(0, 4, 1, 2, 3).contiguous().requires_grad_(True)
        wt, bt = c.weight.detach().clone().requires_grad_(True), c.bias.detach()
        dyt = dy.permute(0, 4, 1, 2, 3).contiguous()

        def t_fwd():
            with torch.autocast("cuda", torch.bfloat16):
                return F.leaky_relu(F.conv3d(xt, wt, bt, stride=2, padding=1), 0.2)

        yt = t_fwd()
        tops = {"fwd": t_fwd, "dgrad": lambda: torch.autograd.grad(yt, xt, dyt, retain_graph=True),
                "wgrad": lambda: torch.autograd.grad(yt, wt, dyt, retain_graph=True)}
        for k, f in tops.items():
            f()
            row[f"torch_{k}_ms"] = statistics.median(timed(f) for _ in range(reps))
        out.append(row)
    return out


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--organs", type=int, default=13)
    p.add_argument("--patch", type=int, nargs=3, default=[64, 192, 192])
    p.add_argument("--rounds", type=int, default=5)
    p.add_argument("--warmup", type=int, default=1)
    p.add_argument("--layers", action="store_true")
    p.add_argument("--out", default=None)
    a = p.parse_args()
    import disc_reference as DR
    import unet3D
    dev = torch.device("cuda:0")
    B, sp = a.organs, tuple(a.patch)
    g = torch.Generator().manual_seed(0)
    x = torch.rand((B, 2) + sp, generator=g).to(dev)
    f_m = [torch.rand((B, 1) + tuple(v // r for v in sp), generator=g).to(dev) for r in (8, 4, 2)]
    torch.manual_seed(0)
    native = unet3D.deep_style_discriminator_output(2).to(dev).train()
    yard = DR.DeepDisc(2).to(dev).train()
    yard.load_state_dict(native.state_dict())

    def gen_pass(m):
        for q in m.parameters():
            q.requires_grad = False
        xi = x.clone().requires_grad_(True)
        fi = [f.clone().requires_grad_(True) for f in f_m]
        with torch.autocast("cuda", torch.bfloat16):
            out = m(xi, fi)
        out.float().sum().backward()
        return out.detach()

    def dis_pass(m):
        for q in m.parameters():
            q.requires_grad = True
            q.grad = None
        with torch.autocast("cuda", torch.bfloat16):
            out = m(x, f_m)
        out.float().sum().backward()
        return out.detach()

    forms = {"native_gen": lambda: gen_pass(native), "torch_gen": lambda: gen_pass(yard),
             "native_dis": lambda: dis_pass(native), "torch_dis": lambda: dis_pass(yard)}
    for _ in range(a.warmup):
        for f in forms.values():
            f()
    torch.cuda.synchronize()
    on, ot = forms["native_dis"]().float(), forms["torch_dis"]().float()
    times = {k: [] for k in forms}
    for _ in range(a.rounds):
        for k, f in forms.items():   # alternating
            times[k].append(timed(f))
    res = {"metric": "deep_style_discriminator_output, bf16 autocast, ms per pass (device events, host launches included)",
           "organs": B, "patch": list(sp), "rounds": a.rounds,
           "logits_rel_diff_native_vs_torch": ((on - ot).norm() / ot.norm()).item()}
    for k, v in times.items():
        res[f"{k}_ms_median"] = statistics.median(v)
        res[f"{k}_ms_min"], res[f"{k}_ms_max"] = min(v), max(v)
    if a.layers:
        res["layers"] = layer_times(native, x, f_m)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
