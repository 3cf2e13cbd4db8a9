"""Autograd wrapper to run one sub-module (a weight-standardised conv, a NoBottleneck block) on the native
executor when a caller uses that module on its own, outside the full trunk. Kept apart from trunk.TapeFn: it alone
differentiates with respect to its input (an NCDHW activation, not the input volume), sets the tape's
standardisation itself and never reports to a DDP sink."""
import torch

from . import ops
from .trunk import Act, Tape, compute_dtype, ncdhw, ndhwc_grad


class _SubFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, builder, dtype, std, names, x, *tensors):
        tape = Tape(dict(zip(names, tensors)), dtype, record=True)
        tape.std = std
        xa = Act(ndhwc_grad(x, dtype))
        out = builder(tape, xa)
        ctx.tape, ctx.xa, ctx.out, ctx.names = tape, xa, out, names
        return ncdhw(out.t).float()

    @staticmethod
    def backward(ctx, g):
        tape = ctx.tape
        tape.backward(ctx.out, ndhwc_grad(g, ctx.out.t.dtype))
        dx = ctx.xa.grad
        dx = ncdhw(dx.float()) if dx is not None else None
        grads = [tape.pgrad.get(n) for n in ctx.names]
        return (*[None] * (len(ctx.needs_input_grad) - len(grads) - 1), dx, *grads)


def run(builder, x, named_params, std=True, dtype=None):
    """x: NCDHW fp32 device tensor; builder(tape, act) -> Act. Returns NCDHW fp32."""
    ops.require_device(x)
    dtype = compute_dtype(dtype)
    names = [n for n, _ in named_params]
    tensors = [p for _, p in named_params]
    return _SubFn.apply(builder, dtype, std, names, x, *tensors)
