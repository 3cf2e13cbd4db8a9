"""What the driver does with its discriminator, against the drop-in modules, with seeded tensors in place of the
model's outputs: construction (train_amos_atlas_final.py:123-129) and one step's discriminator part (:320-379) — a
fresh Adam, the generator pass with frozen parameters over flist, the discriminator pass with detached inputs over
clist, both backwards after both forwards, the optimizer step. Both branches of args.deep_up are run. One JSON line.

    python tools/replay_disc_step.py [--patch 64 96 96] [--organs 13]
"""
import argparse
import json
import os
import sys

REPO = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path[:0] = [os.path.join(REPO, "multimodal-pl_amd"), REPO]
import torch  # noqa: E402
import torch.optim as optim  # noqa: E402


def step(deep_up, organs, patch, device, weight_gan=0.01):
    """One step's discriminator part. deep_up selects the driver's branch: True builds the norm discriminator and
    feeds it the organ probabilities + atlas only (level weight 1), False builds the deep one and adds the three
    attention maps."""
    import unet3D
    from loss_functions.losses import SmoothCrossEntropyLoss, bce_loss
    g = torch.Generator().manual_seed(1)
    torch.manual_seed(0)
    ctor = unet3D.norm_style_discriminator_output if deep_up else unet3D.deep_style_discriminator_output
    d_style = ctor(num_classes=2).to(device).train()
    # seeded stand-ins for the model's outputs: class logits, the atlas prior, the three attention logit maps
    logits = torch.randn((1, 1 + organs) + patch, generator=g).to(device).requires_grad_(True)
    catlas = torch.rand((organs,) + patch, generator=g).to(device)
    attns = [torch.randn((1, organs) + tuple(v // r for v in patch), generator=g).to(device).requires_grad_(True)
             for r in (8, 4, 2)]
    label_t = (torch.rand(organs, generator=g) > 0.5).long()
    flist = [i for i in range(organs) if label_t[i] == 0][: max(1, organs // 2)]
    clist = list(range(organs))
    from utils import attention_pairs, organ_atlas_pairs

    def call(idx, detach):
        # [len(idx), 2, D, H, W]: the organs' probabilities and atlas maps (driver :337 / :345 / :355 / :365)
        x_in = organ_atlas_pairs(logits.detach() if detach else logits, catlas, idx)
        if deep_up:
            return d_style(x_in)
        return d_style(x_in, [attention_pairs(a.detach() if detach else a, idx) for a in attns])

    opt = optim.Adam(d_style.parameters(), lr=1e-4)
    opt.zero_grad()
    for q in d_style.parameters():          # generator pass: the discriminator is frozen
        q.requires_grad = False
    loss_d = bce_loss(call(flist, detach=False), 1)
    for q in d_style.parameters():          # discriminator pass: nothing flows back to the generator
        q.requires_grad = True
    out = call(clist, detach=True)
    loss_d_ = SmoothCrossEntropyLoss()(out, label_t[clist].to(out.device))
    (loss_d * weight_gan).backward()        # both forwards are alive here
    assert all(q.grad is None for q in d_style.parameters())
    loss_d_.backward()
    before = [q.detach().clone() for q in d_style.parameters()]
    opt.step()
    moved = sum(int(not torch.equal(a, q.detach())) for a, q in zip(before, d_style.parameters()))
    torch.cuda.synchronize()
    return {"deep_up": deep_up, "loss_d": float(loss_d.detach()), "loss_d_": float(loss_d_.detach()),
            "logits_grad_norm": float(logits.grad.norm()),
            "attn_grad_norms": [float(a.grad.norm()) if a.grad is not None else None for a in attns],
            "param_grads_finite": all(bool(torch.isfinite(q.grad).all()) for q in d_style.parameters()),
            "parameters_moved_by_adam": moved, "parameters": len(before), "flist": len(flist), "clist": len(clist)}


def main():
    p = argparse.ArgumentParser()
    p.add_argument("--organs", type=int, default=13)
    p.add_argument("--patch", type=int, nargs=3, default=[64, 96, 96])
    a = p.parse_args()
    dev = torch.device("cuda:0")
    print(json.dumps({"patch": a.patch, "organs": a.organs,
                      "steps": [step(d, a.organs, tuple(a.patch), dev) for d in (False, True)]}))


if __name__ == "__main__":
    main()
