"""UNet3D (DynConv 8,8,2) on the native executor, forward and backward: trunk + GAP + controller + per-sample
dynamic heads (reference unet3D.py:1659-1664, 1688-1732, 1734-1806).

Forward: trunk -> precls_conv (8 channels, fp32) ; GAP = mean_v relu(GN(16,256)(bottleneck)) ; params =
controller(cat(GAP, onehot(task, 7))) ; logits = 8->8->8->2 MLP per voxel with each sample's own params.
Backward: three closures at the end of the tape, so they replay first, seeded by trunk.TapeFn with the logits'
gradient: dynamic-head backward (dh + 162 parameter grads per sample), controller backward (dW, db, and the GAP's dA
broadcast = AdaptiveAvgPool3d backward), GAP GroupNorm backward into the bottleneck gradient; then the trunk's own
closures with the head gradient. Every value is a libu3d kernel.
"""
import torch

from . import ops, trunk


def _dyn_forward(tape, cfg, x, task_id):
    P = tape.P
    f, bott = tape.trunk(x, cfg)
    head = tape.head(f, cfg)                       # Act: [n, d, h, w, 8] fp32 (precls_conv)
    n, d, h, w, _ = head.t.shape
    v = d * h * w
    b = bott.t
    vb = b.numel() // (n * 256)
    st = tape.stats(bott, 16)
    gw, gb = P["GAP.0.weight"], P["GAP.0.bias"]
    feat = torch.empty((n, 256), dtype=torch.float32, device=x.device)
    ops.call("u3d_gn_relu_mean", ops.dt_code(b.dtype), b.data_ptr(), n, 256, vb, 16, st.data_ptr(), gw.data_ptr(),
             gb.data_ptr(), feat.data_ptr(), ops._stream())
    task = task_id.to(device=x.device, dtype=torch.int64).contiguous()
    params = torch.empty((n, 162), dtype=torch.float32, device=x.device)
    wc = P["controller.weight"].reshape(162, 263).contiguous()
    ops.call("u3d_dyn_controller", feat.data_ptr(), n, 256, task.data_ptr(), 7, wc.data_ptr(),
             P["controller.bias"].data_ptr(), 162, params.data_ptr(), ops._stream())
    out = trunk.Act(torch.empty((n, d, h, w, 2), dtype=torch.float32, device=x.device))
    ops.call("u3d_dynhead_fwd", head.t.data_ptr(), params.data_ptr(), n, v, out.t.data_ptr(), ops._stream())
    if tape.record:
        new = lambda *s: torch.empty(s, dtype=torch.float32, device=x.device)  # noqa: E731
        mid = {}  # what one stage hands the next: dparams [n, 162], then the GAP's dA

        def dynhead_bwd():  # dh [n, v, 8] (the precls head's gradient) and the per-sample parameter gradients
            head.grad, mid["dparams"] = new(*head.t.shape), new(n, 162)
            part = new(n, ops.query("u3d_dynhead_bwd_blocks", v), 162)
            ops.call("u3d_dynhead_bwd", head.t.data_ptr(), params.data_ptr(), out.grad.data_ptr(), n, v,
                     head.grad.data_ptr(), part.data_ptr(), mid["dparams"].data_ptr(), ops._stream())

        def controller_bwd():  # dW, db; dfeat -> GAP dA broadcast over the bottleneck voxels
            dwc = tape.grad_out("controller.weight", P["controller.weight"])
            dbc = tape.grad_out("controller.bias", P["controller.bias"])
            mid["dA"] = torch.empty_like(b)
            ops.call("u3d_dyn_controller_bwd", ops.dt_code(b.dtype), feat.data_ptr(), n, 256, task.data_ptr(), 7,
                     wc.data_ptr(), mid.pop("dparams").data_ptr(), 162, dwc.data_ptr(), dbc.data_ptr(), 0, vb,
                     mid["dA"].data_ptr(), ops._stream())
            tape.grad_done("controller.weight")
            tape.grad_done("controller.bias")

        def gap_bwd():  # GAP GroupNorm + ReLU backward into the bottleneck (fusionConv output) gradient
            dg, dbb = tape.grad_out("GAP.0.weight", gw), tape.grad_out("GAP.0.bias", gb)
            bott.grad = ops.gn_bwd(mid.pop("dA"), b, st, gw, gb, 16, dgamma=dg, dbeta=dbb)
            tape.grad_done("GAP.0.weight")
            tape.grad_done("GAP.0.bias")

        tape.ops += [gap_bwd, controller_bwd, dynhead_bwd]  # appended last and replayed in reverse: before the trunk's
    return out, {}


def run_unet3d(model, x, task_id):
    return trunk.run_model(lambda tape, x: _dyn_forward(tape, model._u3d_cfg, x, task_id), x,
                           list(model.named_parameters()), getattr(model, "compute_dtype", None))[0]
