#!/usr/bin/env python3
"""Launch trace of the u3d dispatcher on the host: which library entry points a training step (or a single conv
wrapper) calls, with which scalar arguments, and which workspace slots it asks for. Nothing is launched: the tensors
live on the ``meta`` device, ``ops.call`` is replaced by a recorder, and only the library's host-side size / split
queries run. Two trees route identically exactly when their traces are equal.

  tools/route_trace.py --write tests/route_trace_expected.json   expected digests (from the tree that is the reference)
  tools/route_trace.py --check tests/route_trace_expected.json   compare this tree against them
  tools/route_trace.py --dump DIR                                full traces, one JSON per configuration (for diffing)

One trace entry per library call: ["call", entry point, [args]] with every int / long / float argument verbatim and
every pointer argument as 0 (null) or 1; one entry per workspace request: ["ws", slot, bytes].
"""
import argparse
import contextlib
import ctypes
import hashlib
import json
import os
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "multimodal-pl_amd")]

import torch  # noqa: E402

from u3d import _lib, ops, trunk  # noqa: E402
from u3d.loss import DeferredLossGrad  # noqa: E402

# entry points whose ``made`` out-flag (the argument before the stream) the dispatcher reads back
_MADE = ("u3d_conv_small2", "u3d_conv_small_dgrad_gn", "u3d_conv_small_bwd_pair")


def library_built():
    return os.path.exists(_lib.LIB_PATH)


@contextlib.contextmanager
def recording():
    """Yields the trace list while ops.call / ops.WS.get record instead of running."""
    trace = []

    def call(name, *args):
        sig = _lib._SIGS[name]
        assert len(sig) == len(args), (name, len(sig), len(args))
        trace.append(["call", name, [int(a is not None) if t is _lib.P else a for t, a in zip(sig, args)]])
        if name in _MADE:
            ctypes.c_int.from_address(args[-2]).value = 1
        return 0

    def ws_get(nbytes, device, slot=0):
        trace.append(["ws", getattr(slot, "value", slot), int(nbytes)])
        return torch.empty(max(int(nbytes), 256), dtype=torch.uint8, device="meta")

    saved = {n: getattr(ops, n) for n in ("call", "_stream", "require_device")}
    ops.call, ops._stream, ops.require_device = call, (lambda: 0), (lambda *ts: None)
    ops.WS.get = ws_get
    try:
        yield trace
    finally:
        del ops.WS.get
        for n, v in saved.items():
            setattr(ops, n, v)


@contextlib.contextmanager
def flags(**kw):
    """Module flags of u3d.ops set for the duration (CONVG_PERSIST: the library option)."""
    with contextlib.ExitStack() as es:
        if "CONVG_PERSIST" in kw:
            es.enter_context(ops.option("CONVG_PERSIST", kw.pop("CONVG_PERSIST")))
        saved = {n: getattr(ops, n) for n in kw}
        for n, v in kw.items():
            setattr(ops, n, v)
        try:
            yield
        finally:
            for n, v in saved.items():
                setattr(ops, n, v)


FLAG_SETS = {
    "collective": dict(COLLECTIVE_IN_FLIGHT=[True]),
    "fused_finalize": dict(FUSED_FINALIZE=True),
    "ring_queue": dict(RING_QUEUE=True),
    "ring_xn": dict(RING_XN=True),
    "small_fuse_off": dict(SMALL_FUSE=False),
    "conv32_brick": dict(CONV32_FN="u3d_conv32_brick"),
    "convg_persist_off": dict(CONVG_PERSIST=0),
    # the flags that steer the backward forms of a conv on the tape (ops.conv_bwd, Tape.gn_conv)
    "gn_pairs_off": dict(GN_BWD_PAIRS=False),
    "small_pair_off": dict(SMALL_BWD_PAIR=False),
    "s2_compact_off": dict(S2_COMPACT=False),
    "s2_norm_once_off": dict(S2_NORM_ONCE=False),
    "gn_bwd_fused_off": dict(GN_BWD_FUSED=False),
    "gn_bwd_fused_brick_off": dict(GN_BWD_FUSED_BRICK=False),
    "small_gb_off": dict(SMALL_GB=False),
    "head_gn_parts_off": dict(HEAD_GN_PARTS=False),
    "head_dbias_off": dict(HEAD_DBIAS_FUSED=False),
    "eager_slab_sum": dict(EAGER_SLAB_SUM=True),
    "wgrad_queue": dict(WGRAD_QUEUE=True),
    "ring_wgrad_off": dict(USE_RING_WGRAD=False),
    "brick_wgrad_off": dict(USE_BRICK_WGRAD=False),
    "collective_fused_finalize": dict(COLLECTIVE_IN_FLIGHT=[True], FUSED_FINALIZE=True),  # (the tolerant DDP step)
    "collective_small_pair_off": dict(COLLECTIVE_IN_FLIGHT=[True], SMALL_BWD_PAIR=False),
}


def meta(shape, dtype=torch.float32):
    return torch.empty(tuple(shape), dtype=dtype, device="meta")


# ------------------------------------------------------------------------------------------ whole trunk steps
def _model(name):
    import unet3D
    with torch.device("meta"):
        if name == "unet3D":
            return unet3D.unet3D([1, 2, 2, 2, 2], 16)
        if name == "baseline":
            return unet3D.unet3D_baseline([1, 2, 2, 2, 2], num_classes=16, weight_std=True)
        return unet3D.unet3D_g([1, 2, 2, 2, 2], num_classes=3, weight_std=True)


def trunk_step(model, shape, dtype, record=True, plain_grad=False):
    """Tape.trunk + Tape.head (+ Tape.backward) of ``model`` on a meta input [n, d, h, w]. ``plain_grad``: the loss
    gradient reaches the head formed (an fp32 tensor), as from any loss but the partial-label one."""
    m = _model(model)
    n, d, h, w = shape
    cin = m.conv0.weight.shape[1] if hasattr(m, "conv0") else m.conv1.weight.shape[1]
    tape = trunk.Tape(dict(m._trunk_params()), dtype, record=record)
    f, _ = tape.trunk(meta((n, cin, d, h, w)), m._u3d_cfg)
    lg = tape.head(f, m._u3d_cfg)
    if not record:
        return
    y = lg.t
    if getattr(tape, "head_out", None) is lg and not plain_grad:  # the loss gradient handed to the streaming head unformed
        payload = (y, meta(y.shape[:-1]), meta((y.shape[-1],)), meta((y.shape[-1], 4), torch.float64), meta((1,)))
        g = DeferredLossGrad((y.shape, y.stride(), y.dtype, y.device), None, payload, None)
    else:
        g = meta(y.shape)
    tape.backward(lg, g)


TRUNK_INPUTS = {
    "bf16_2x96": ((2, 96, 96, 96), torch.bfloat16),
    "bf16_1x32": ((1, 32, 32, 32), torch.bfloat16),
    "bf16_2x64x48x80": ((2, 64, 48, 80), torch.bfloat16),  # (no multiple of 32: the conv0 model's skips do not line up)
    "bf16_2x64x96x128": ((2, 64, 96, 128), torch.bfloat16),
    "fp32_1x32": ((1, 32, 32, 32), torch.float32),
}
MODELS = ("unet3D", "baseline", "unet3D_g")


# ------------------------------------------------------------------------------------------ whole model steps
L5 = [1, 2, 2, 2, 2]
MODEL_TAGS = {   # tag -> (constructor on the unet3D module, what forward takes after the input volume)
    "unet3D": (lambda u: u.unet3D(L5, 16, True), "task"),
    "feam3": (lambda u: u.unet3D_with_feam3(L5, 16, True, deep_up=False), None),
    "feam3_up": (lambda u: u.unet3D_with_feam3(L5, 16, True, deep_up=True), None),
    "feam2_ema": (lambda u: u.unet3D_with_feam2(L5, 16, True, ema=True), "mask"),  # (train mode renews the tokens)
    "deepsup": (lambda u: u.unet3D_with_deepsup(L5, 16, True), None),
    "eam": (lambda u: u.unet3D_with_eam(L5, 16, True), None),
    "eam_baseline": (lambda u: u.unet3D_with_eam_baseline(L5, 16, True), None),
    "feam": (lambda u: u.unet3D_with_feam(L5, 16, True), "no_label"),
}
MODEL_INPUTS = ("bf16_1x32", "fp32_1x32")


def _flat(outs):
    if torch.is_tensor(outs):
        return [outs]
    return [t for o in outs if o is not None for t in _flat(o)]


def model_step(tag, shape, dtype, train=True):
    """model.forward of a whole model class on a meta input [n, d, h, w], through the autograd Function, and (train)
    torch.autograd.backward with a gradient on every differentiable output. The pack cache is off: its test asks
    torch about stream capture, which needs a device."""
    import unet3D
    make, extra = MODEL_TAGS[tag]
    with torch.device("meta"):
        m = make(unet3D)
    m.compute_dtype = dtype
    m.train(train)
    n, d, h, w = shape
    args = [meta((n, 1, d, h, w))]
    if extra == "task":
        args.append(meta((n,), torch.int64))
    elif extra == "mask":
        args.append(meta((n, 1, d, h, w)))
    elif extra == "no_label":  # read on the host (feam.labels_reach): a real tensor, all background
        args.append(torch.zeros((n, 1, d, h, w)))
    with flags(PACK_CACHE_OK=[False]), torch.set_grad_enabled(train):
        outs = [t for t in _flat(m(*args)) if t.requires_grad]
        if outs:
            torch.autograd.backward(outs, [meta(t.shape, t.dtype) for t in outs])


# ------------------------------------------------------------------------------------------ tape pieces
def _conv_params(P, key, cin, cout, k, gn_key=None, bias=False):
    P[key + ".weight"] = meta((cout, cin, k, k, k))
    if bias:
        P[key + ".bias"] = meta((cout,))
    if gn_key is not None:
        P[gn_key + ".weight"], P[gn_key + ".bias"] = meta((cin,)), meta((cin,))


def tape_piece(build, cin, edge, gdtype=torch.bfloat16, n=2):
    """One piece of the tape, forward and backward, on a meta Act [n, edge^3, cin]: build(P) fills the parameters and
    returns the function (tape, act) -> output Act; the gradient handed in has ``gdtype``."""
    P = {}
    fwd = build(P)
    tape = trunk.Tape(P, torch.bfloat16, record=True)
    out = fwd(tape, trunk.Act(meta((n, edge, edge, edge, cin), torch.bfloat16)))
    tape.backward(out, meta(out.t.shape, gdtype))


def _block(cin, cout, stride, down):
    def build(P):
        _conv_params(P, "b.conv1", cin, cout, 3, "b.gn1")
        _conv_params(P, "b.conv2", cout, cout, 3, "b.gn2")
        if down:
            _conv_params(P, "b.downsample.2", cin, cout, 1, "b.downsample.0")
        return lambda tape, x: tape.block(x, "b.", stride, 16)
    return build


def _lone_conv(c):  # no GroupNorm in front: unet3D.Conv3d on its own (subgraph), the conv0 model's conv1
    def build(P):
        _conv_params(P, "c", c, c, 3)
        return lambda tape, x: tape.gn_conv(x, "c", 3, 1)
    return build


def _deep_head(cin):  # a feam.Level's deep head (feam._feam3_forward); cin 32 / 64 run the streaming head, 128 the implicit GEMM
    def build(P):
        _conv_params(P, "deepout.2", cin, 16, 1, "deepout.0", bias=True)
        return lambda tape, x: tape.gn_conv(x, "deepout.2", 1, 1, gn_key="deepout.0", G=16, bias=True, out_f32=True,
                                            standardize=False)
    return build


TAPE_EDGES = (12, 48)  # 2 x 12^3: the small family; 2 x 48^3: the ring (32 -> 32) and the brick
TAPE_PIECES = {
    "block_down_s2": (_block(32, 64, 2, True), 32, torch.bfloat16),
    "block_down_s1": (_block(64, 32, 1, True), 64, torch.bfloat16),
    "block_32": (_block(32, 32, 1, False), 32, torch.bfloat16),
    "block_64": (_block(64, 64, 1, False), 64, torch.bfloat16),
    "conv_no_gn_32": (_lone_conv(32), 32, torch.bfloat16),
    "conv_no_gn_64": (_lone_conv(64), 64, torch.bfloat16),
    "deep_head_32": (_deep_head(32), 32, torch.float32),
    "deep_head_128": (_deep_head(128), 128, torch.float32),
}


# ------------------------------------------------------------------------------------------ single wrappers
CHANNELS = ((32, 32), (32, 64), (64, 64), (64, 128), (128, 128), (256, 256), (16, 8))
EDGES = (6, 12, 24, 48, 96)
BATCHES = (1, 2, 17)
KS = ((3, 1), (3, 2), (1, 1), (1, 2))


def _gn(n, c, G=16):
    return (meta((n, G, 2)), meta((c,)), meta((c,)), G)


def _attempt(trace, label, fn):
    """One wrapper call: its library calls follow the label; an exception is recorded as its type."""
    trace.append(["case", label])
    try:
        fn()
    except Exception as e:  # noqa: BLE001 (what the tree rejects is part of its routing)
        trace.append(["raised", type(e).__name__])


def direct_calls(trace, cin, cout, k, stride, shape, dtype=torch.bfloat16):
    """Every conv wrapper of u3d.ops once for one conv (cin -> cout, k^3, stride) on the input volume ``shape``."""
    n, d, h, w = shape
    oshape = (n,) + tuple(ops.out_dim(v, k, stride) for v in (d, h, w))
    x, dy = meta(shape + (cin,), dtype), meta(oshape + (cout,), dtype)
    res = meta(oshape + (cout,), dtype)
    pf = meta((k ** 3, ops.round32(cout), ops.round32(cin)), dtype)
    pd = meta((k ** 3, ops.round32(cin), ops.round32(cout)), dtype)
    gn, bias = _gn(n, cin), meta((cout,))
    dgb = lambda: (meta((cin,)), meta((cin,)))  # noqa: E731
    tag = f"{cin}->{cout} k{k}s{stride} {n}x{d}x{h}x{w}"
    A = lambda what, fn: _attempt(trace, f"{what} {tag}", fn)  # noqa: E731
    A("fwd", lambda: ops.conv_fwd(x, pf, cout, k, stride))
    A("fwd gn", lambda: ops.conv_fwd(x, pf, cout, k, stride, gn))
    A("fwd gn res", lambda: ops.conv_fwd(x, pf, cout, k, stride, gn, res))
    A("fwd gn bias f32", lambda: ops.conv_fwd(x, pf, cout, k, stride, gn, None, bias, True))
    A("fwd_stats", lambda: ops.conv_fwd_stats(x, pf, cout, k, stride))
    A("fwd_stats res", lambda: ops.conv_fwd_stats(x, pf, cout, k, stride, None, res))
    A("fwd_stats gn", lambda: ops.conv_fwd_stats(x, pf, cout, k, stride, gn))
    A("fwd_stats gn res", lambda: ops.conv_fwd_stats(x, pf, cout, k, stride, gn, res))
    A("dgrad", lambda: ops.conv_dgrad(dy, pd, cin, shape, k, stride))
    A("dgrad_gn", lambda: _shape_of(trace, ops.conv_dgrad_gn(dy, pd, cin, x, k, stride, gn)))
    A("dgrad_gn dgb", lambda: _shape_of(trace, ops.conv_dgrad_gn(dy, pd, cin, x, k, stride, gn, dgb)))
    A("bwd_pair", lambda: _shape_of(trace, ops.conv_bwd_pair_small(dy, pd, x, k, stride, gn, dgb)))
    A("wgrad", lambda: ops.conv_wgrad(dy, x, k, stride))
    A("wgrad gn", lambda: ops.conv_wgrad(dy, x, k, stride, gn))


def _shape_of(trace, r):
    """What a fused form returned: None (declined) or the kind of its GroupNorm-backward hand-off."""
    if r is None:
        trace.append(["ret", None])
    else:
        parts = r[-1]
        trace.append(["ret", "coef" if isinstance(parts, tuple) else list(parts.shape)])


def direct_grid(trace, channels=CHANNELS, ks=KS, dtype=torch.bfloat16, edges=EDGES, batches=BATCHES):
    for cin, cout in channels:
        for k, stride in ks:
            for e in edges:
                for n in batches:
                    direct_calls(trace, cin, cout, k, stride, (n, e, e, e), dtype)


def beyond_2gib(trace):
    """The two stride-2 data gradients of test_stride2_dgrad_beyond_2gib_routes_to_the_64bit_kernel (and every other
    wrapper on those operands)."""
    direct_calls(trace, 32, 64, 3, 2, (2, 96, 1024, 1024))
    direct_calls(trace, 32, 64, 3, 2, (2, 48, 128, 128))
    direct_calls(trace, 32, 32, 3, 1, (2, 64, 1024, 1024))  # a 32 -> 32 ring operand of 4 GiB: past its 32-bit offsets


# ------------------------------------------------------------------------------------------ configurations
def configs():
    """name -> function(trace) for every recorded configuration."""
    out = {}
    for m in MODELS:
        for iname, (shape, dtype) in TRUNK_INPUTS.items():
            out[f"trunk/{m}/{iname}"] = lambda t, m=m, s=shape, dt=dtype: trunk_step(m, s, dt)
        for fname, kw in FLAG_SETS.items():
            def run(t, m=m, kw=kw):
                with flags(**kw):
                    trunk_step(m, (2, 96, 96, 96), torch.bfloat16)
            out[f"trunk/{m}/bf16_2x96/{fname}"] = run
        out[f"trunk/{m}/bf16_2x96/inference"] = lambda t, m=m: trunk_step(m, (2, 96, 96, 96), torch.bfloat16, False)
    out["trunk/baseline/bf16_2x96/plain_grad"] = lambda t: trunk_step("baseline", (2, 96, 96, 96), torch.bfloat16,
                                                                      plain_grad=True)
    for tag in MODEL_TAGS:
        for iname in MODEL_INPUTS:
            shape, dtype = TRUNK_INPUTS[iname]
            out[f"model/{tag}/{iname}"] = lambda t, g=tag, s=shape, dt=dtype: model_step(g, s, dt)
        out[f"model/{tag}/bf16_1x32/inference"] = lambda t, g=tag: model_step(g, (1, 32, 32, 32), torch.bfloat16, False)
    for pname, (build, cin, gdtype) in TAPE_PIECES.items():
        for e in TAPE_EDGES:
            out[f"tape/{pname}/{e}"] = lambda t, b=build, c=cin, e=e, g=gdtype: tape_piece(b, c, e, g)
    for cin, cout in CHANNELS:
        for k, stride in KS:
            out[f"direct/{cin}-{cout}/k{k}s{stride}"] = \
                lambda t, c=(cin, cout), ks=(k, stride): direct_grid(t, (c,), (ks,))
    out["direct/beyond_2gib"] = beyond_2gib
    out["direct/fp32"] = lambda t: direct_grid(t, dtype=torch.float32, edges=(6, 24, 96), batches=(1, 2))
    for fname, kw in FLAG_SETS.items():
        def run(t, kw=kw):
            with flags(**kw):
                direct_grid(t, edges=(6, 12, 24, 96), batches=(2, 17))
        out[f"direct/flags/{fname}"] = run
    return out


def run_config(fn):
    with recording() as trace:
        _attempt(trace, "config", lambda: fn(trace))
    return trace


def digest(trace):
    counts = {}
    for e in trace:
        if e[0] == "call":
            counts[e[1]] = counts.get(e[1], 0) + 1
    blob = json.dumps(trace, separators=(",", ":")).encode()
    return {"sha256": hashlib.sha256(blob).hexdigest(), "entries": len(trace), "calls": dict(sorted(counts.items()))}


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--write", metavar="JSON")
    ap.add_argument("--check", metavar="JSON")
    ap.add_argument("--dump", metavar="DIR")
    ap.add_argument("--only", metavar="SUBSTR", help="configurations whose name contains this")
    a = ap.parse_args()
    want = json.load(open(a.check)) if a.check else None
    got, bad = {}, []
    for name, fn in configs().items():
        if a.only and a.only not in name:
            continue
        trace = run_config(fn)
        got[name] = digest(trace)
        if a.dump:
            path = os.path.join(a.dump, name.replace("/", "__") + ".json")
            os.makedirs(a.dump, exist_ok=True)
            with open(path, "w") as f:
                f.write("\n".join(json.dumps(e, separators=(",", ":")) for e in trace) + "\n")
        if want is not None and want.get(name) != got[name]:
            bad.append(name)
    if a.write:
        with open(a.write, "w") as f:
            json.dump(got, f, indent=0, sort_keys=True, separators=(",", ":"))
            f.write("\n")
    if want is not None:
        print(f"{len(got) - len(bad)} of {len(got)} configurations match" + ("; differ: " + ", ".join(bad) if bad else ""))
        return 1 if bad else 0
    print(f"{len(got)} configurations, {sum(g['entries'] for g in got.values())} trace entries")
    return 0


if __name__ == "__main__":
    sys.exit(main())
