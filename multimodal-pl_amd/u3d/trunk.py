"""Native executor for the reference U-Net trunks (unet3D.py): forward records a tape of backward closures,
backward replays it in reverse. Every value is produced by a libu3d kernel; torch provides memory and the
stream. Activations live NDHWC in the compute dtype (fp32 parity mode or bf16 fast mode) with fp32 master
weights; weight standardisation is re-applied from the fp32 master each step (unet3D.py:21-26).

Graph (reference unet3D.forward :1734-1806 / unet3D_baseline.forward :663-718 / unet3D_g.forward :1568-1623):
  stem conv1 (or conv0 s2 -> conv1) -> layer0..4 (NoBottleneck :40-73) -> fusionConv (GN,ReLU,1^3)
  -> 4 x [trilinear x2 + skip -> x{8,4,2,1}_resb] -> precls_conv (GN,ReLU,1^3+bias) [-> x2 upsample (unet3D_g)]

Every model class of unet3D.py reaches autograd through one Function, TapeFn, and one runner, run_model: a model is a
builder (tape, x) -> outputs (run_trunk here, dynhead._dyn_forward, feam._feam3_forward, feam._eam_forward), and what
differs between models is what their builders append to the tape.
"""
from dataclasses import dataclass
from functools import partial

import torch

from . import ops
from .loss import DeferredLossGrad


@dataclass(frozen=True)
class TrunkCfg:
    layers: tuple = (1, 2, 2, 2, 2)
    groups: int = 16          # GroupNorm groups inside NoBottleneck / downsample
    fusion_groups: int = 16
    head_groups: int = 16
    conv0: bool = False       # unet3D_g: stride-2 stem conv0 then a plain conv1
    final_up: bool = False    # unet3D_g: x2 trilinear upsample of the logits
    weight_std: bool = True


class Act:
    """An NDHWC activation, its cached GroupNorm statistics and its accumulated gradient."""
    __slots__ = ("t", "stats", "grad", "gn_pend")

    def __init__(self, t):
        self.t = t
        self.stats = {}
        self.grad = None
        self.gn_pend = None  # the parked (dA, gn, key, compact) of a block's downsample GN (Tape.prologue_bwd)


class Tape:
    def __init__(self, params, dtype, record):
        self.P = params
        self.dtype = dtype
        self.record = record
        self.packs = {}
        self.pgrad = {}
        self.ops = []
        self.sink = None
        self.std = True
        self.pending = []   # weight grads waiting for the batched standardisation backward
        self.head_out = None            # the Act of a 16-class streaming head (conv_fwd_form)
        self.offer_head_link = False    # the builder lets the loss hand its gradient to that head unformed (TapeFn)

    @classmethod
    def recording(cls, names, tensors, dtype):
        """A recording tape over the named parameters for one model step (TapeFn), attached to the current DDP sink."""
        from .ddp import current_sink
        tape = cls(dict(zip(names, tensors)), dtype, record=True)
        tape.sink = current_sink()
        if tape.sink is not None:
            tape.sink.begin()
        return tape

    def finish(self, names):
        """After backward(): the parameter gradients in ``names`` order (None where the sink assigned .grad itself)."""
        if self.sink is None:
            return [self.pgrad.get(n) for n in names]
        self.sink.finish()
        return self.sink.returned(names, [self.pgrad.get(n) for n in names])

    def prepack(self, plan):
        """Standardise + pack every conv weight of ``plan`` [(key, standardize, need_dgrad)] in one launch."""
        todo = [(k, s, d and self.record) for k, s, d in plan if k not in self.packs and k + ".weight" in self.P]
        res = ops.wstd_fwd_batch([(self.P[k + ".weight"], s, d) for k, s, d in todo], self.dtype)
        for (k, _, _), r in zip(todo, res):
            self.packs[k] = r

    def conv_plan(self, cfg):
        """The convs trunk()/head() run: (key, standardize, need_dgrad). Absent keys are skipped."""
        std = cfg.weight_std
        plan = [("conv0", std, False), ("conv1", std, True)] if cfg.conv0 else [("conv1", std, False)]
        blocks = [f"layer{i}.{b}." for i in range(5) for b in range(cfg.layers[i])]
        blocks += [n + ".0." for n in ("x8_resb", "x4_resb", "x2_resb", "x1_resb")]
        for pre in blocks:
            plan += [(pre + c, std, True) for c in ("conv1", "downsample.2", "conv2")]
        plan += [("fusionConv.2", std, True), ("precls_conv.2", False, True)]
        plan += [(f"deepout{k}.2", False, True) for k in (1, 2, 3)]  # unet3D_with_feam3 deep supervision
        return plan

    def pend_wgrad(self, part, ns, W, st, std, name):
        self.pending.append((part, ns, W, st, std, self.grad_out(name, W), False, name))
        if self.sink is not None:
            self.sink.note_pending(name)  # sets sink.flush_due when the parked gradients complete a DDP bucket

    def flush_wgrads(self):
        """Slab sum + standardisation backward of the pending weight gradients, in one batched launch pair.
        Batched at the end of the backward (or at a DDP bucket boundary): flushing after every conv measured
        7.33 vs 6.61 ms/step (r03, gpurun_out/r03i/flush), the per-conv launches cost more than the Infinity Cache
        residency of the slabs saves; a side-stream flush measured 7.93 vs 7.83 (round 2)."""
        if not self.pending:
            return
        ops.wstd_bwd_batch([p[:7] for p in self.pending])
        names = [p[7] for p in self.pending]
        self.pending = []
        for n in names:
            self.grad_done(n)

    # ------------------------------------------------------------------ helpers
    def packed(self, key, standardize, need_dgrad=True):
        if key not in self.packs:
            self.packs[key] = ops.wstd_fwd(self.P[key + ".weight"], self.dtype, standardize,
                                           need_dgrad and self.record)
        return self.packs[key]

    def stats(self, act, G):
        if G not in act.stats:
            act.stats[G] = ops.gn_stats(act.t, G)
        return act.stats[G]

    def acc_grad(self, act, g):
        if act.grad is None:
            act.grad = g
        else:
            ops.add_(act.grad, g)

    def grad_out(self, name, like):
        """Destination of a parameter gradient: a DDP bucket view when data-parallel, else a fresh tensor."""
        t = self.sink.out(name) if self.sink is not None else None
        if t is None:
            t = torch.empty_like(like)
        self.pgrad[name] = t
        return t

    def grad_done(self, name):
        if self.sink is not None:
            self.sink.done(name)

    # ------------------------------------------------------------------ ops
    def stem(self, x, key, stride):
        """conv with cin <= 4 from the fp32 NCDHW input volume (unet3D.py:1632 / :1514)."""
        W = self.P[key + ".weight"]
        pf, _, st = self.packed(key, self.std, need_dgrad=False)
        y, st16 = ops.stem_fwd_stats(x, pf, W.shape[0], stride, self.dtype)
        out = Act(y)
        if st16 is not None:
            out.stats[16] = st16  # GroupNorm(16) statistics from the conv1 epilogue (layer0's gn1 / gn2 read them)
        if self.record:
            def bwd():
                if out.grad is None:
                    return
                part, ns = ops.stem_wgrad(out.grad, x, stride)
                self.pend_wgrad(part, ns, W, st, self.std, key + ".weight")
            self.ops.append(bwd)
        return out

    def conv_fwd_form(self, x, pf, cout, k, stride, gn, res, b, out_f32, head):
        """gn_conv's forward in the form that serves it: (output Act, xn). xn: relu(gn(x)) where the forward stored it,
        the weight gradient's operand (no GN prologue there)."""
        st16 = xn = None
        if head:  # precls_conv: streaming MFMA head (head.hip)
            y = ops.head_fwd(x, pf, cout, b, gn)
        elif b is not None or out_f32:  # (the plain conv only)
            y = ops.conv_fwd(x, pf, cout, k, stride, gn, res, b, out_f32)
        elif self.record and ops.ring_xn_ok(x, cout, k, stride, gn):
            y, st16, xn = ops.conv_fwd_stats_xn(x, pf, cout, k, stride, gn, res)
        elif res is None and ops.s2_normalise_once(x, x.shape[-1], cout, k, stride, gn):
            # stride-2 3^3 conv on the implicit GEMM: relu(gn(x)) materialised once (the GEMM's prologue normalised
            # every gathered element, 27/8 times per input element) and reused by the weight gradient
            xn = ops.gn_apply(x, *gn)
            y, st16 = ops.conv_fwd_stats(xn, pf, cout, k, stride, None)
        elif gn is not None and ops.epilogue_stats_cout(cout):
            y, st16 = ops.conv_fwd_stats(x, pf, cout, k, stride, gn, res)
        else:
            y = ops.conv_fwd(x, pf, cout, k, stride, gn, res)
        out = Act(y)
        if head and cout == 16:
            self.head_out = out  # the partial loss may hand its gradient to this head unformed (TapeFn)
        if st16 is not None:
            out.stats[16] = st16  # GroupNorm(16) statistics from the conv epilogue (consumed by the next GN)
        return out, xn

    def gn_conv(self, x, key, k, stride, gn_key=None, G=0, residual=None, bias=False, out_f32=False,
                standardize=None, park=False):
        """conv(relu(gn(x))) [+ residual] [+ bias] — Conv3d/conv3x3x3 :16-35 behind GN+ReLU :44-53. ``park``: this GN's
        backward waits for the next conv's on the same x (block)."""
        std = self.std if standardize is None else standardize
        W = self.P[key + ".weight"]
        cout, cin = W.shape[0], W.shape[1]
        pf, pd, st = self.packed(key, std)
        gn = (self.stats(x, G), self.P[gn_key + ".weight"], self.P[gn_key + ".bias"], G) if gn_key is not None else None
        b = self.P[key + ".bias"] if bias else None
        head = out_f32 and residual is None and ops.use_head(x.t.dtype, cin, cout, k, stride)
        out, xn = self.conv_fwd_form(x.t, pf, cout, k, stride, gn, residual.t if residual is not None else None, b,
                                     out_f32, head)
        if self.record:
            def dgb():  # the GroupNorm's parameter-gradient destinations, for a launch that writes them itself
                return self.grad_out(gn_key + ".weight", gn[1]), self.grad_out(gn_key + ".bias", gn[2])

            def bwd():
                dy = out.grad
                if dy is None:
                    return self.settle_parked(x, G)
                alone = gn is not None and not park and not x.gn_pend  # this GN's backward runs by itself: fusable
                dyT, dA, parts = self.output_side(dy, out.t, x.t, pd, gn if alone else None, key, b, residual, head)
                r = ops.conv_bwd(dyT, pd, x.t, cout, k, stride, gn, dgb, xn, want_da=dA is None, fuse_gn=alone,
                                 compact=park and gn is not None,
                                 wgrad_done=partial(self.pend_wgrad, W=W, st=st, std=std, name=key + ".weight"))
                dA, parts, compact = r if dA is None else (dA, parts, False)  # (the head's pass produced dA already)
                self.prologue_bwd(x, dA, parts, gn, gn_key, G, park, compact)
            self.ops.append(bwd)
        return out

    def settle_parked(self, x, G):
        """No gradient reached a conv whose partner parked its GN backward on x: that one runs alone after all."""
        if x.gn_pend:
            dA2, gn2, key2, s2c = x.gn_pend.pop()
            self.gn_bwd_one(x, ops.expand_s2(dA2, x.t.shape[:4]) if s2c else dA2, gn2, key2, G)

    def output_side(self, dy, y, x, pd, gn, key, b, residual, head):
        """Output side of a conv's backward -> (dyT, dA, parts): the bias gradient, the residual's share and dy as the
        GEMM operand; on the streaming head one pass over the fp32 dlogits that also produces dA, and for ``gn`` (the
        prologue GroupNorm, where its backward runs by itself) may take that backward's partials."""
        if not head:
            if b is not None:
                ops.channel_sum(dy, out=self.grad_out(key + ".bias", b))
                self.grad_done(key + ".bias")
            if residual is not None:
                self.acc_grad(residual, dy)
            return ops.cast(dy, self.dtype, pad_to=8), None, None  # channels padded to 8 (2-class head)
        cin = x.shape[-1]
        db = self.grad_out(key + ".bias", b) if b is not None else None
        parts = None
        if not isinstance(dy, DeferredLossGrad):
            dA, dyT = ops.head_bwd(dy, pd, cin, dbias=db)
        else:  # the loss gradient formed inside the head's pass
            lg, lab, wt, sums, go = dy.payload
            assert lg.data_ptr() == y.data_ptr() and lg.shape == y.shape, "deferred loss gradient: not this head's logits"
            if gn is not None and ops.head_gn_parts_ok(lg, x, cin, gn):  # (no partial pass over dA)
                dA, dyT, parts = ops.head_loss_bwd(lg, lab, wt, sums, go, pd, cin, dbias=db, x0=x, gn=gn)
            else:
                dA, dyT = ops.head_loss_bwd(lg, lab, wt, sums, go, pd, cin, dbias=db)
        if b is not None:
            self.grad_done(key + ".bias")
        return dyT, dA, parts

    def prologue_bwd(self, x, dA, parts, gn, gn_key, G, park, compact):
        """The backward of a conv's GN + ReLU prologue from dA. A block's gn1 and downsample GN read x with the same
        statistics: the downsample's (``park``; ``compact``: its dA is at the conv's output resolution) waits on x for
        gn1's, which runs next in the reversed tape and takes both in one pass."""
        if gn is None:
            self.acc_grad(x, dA)
        elif park:
            x.gn_pend = [(dA, gn, gn_key, compact)]
        elif x.gn_pend:
            dA2, gn2, key2, s2c2 = x.gn_pend.pop()
            dps = [(self.grad_out(k_ + ".weight", g_[1]), self.grad_out(k_ + ".bias", g_[2]))
                   for k_, g_ in ((gn_key, gn), (key2, gn2))]
            x.grad = ops.gn_bwd2(dA, dA2, x.t, gn[0], (gn[1], gn[2]), (gn2[1], gn2[2]), G, dx=x.grad,
                                 accumulate=x.grad is not None, dparams1=dps[0], dparams2=dps[1], da2_s2=s2c2)
            for k_ in (gn_key, key2):
                self.grad_done(k_ + ".weight")
                self.grad_done(k_ + ".bias")
        else:
            self.gn_bwd_one(x, dA, gn, gn_key, G, parts)

    def gn_bwd_one(self, x, dA, gn, gn_key, G, parts=None):
        acc = dict(dx=x.grad, accumulate=x.grad is not None)
        if isinstance(parts, tuple) and parts[0] == "coef":  # partials, finalize and dgamma / dbeta done in the dgrad
            x.grad = ops.gn_bwd_apply_coef(dA, x.t, parts[1], G, **acc)
        else:
            acc.update(dgamma=self.grad_out(gn_key + ".weight", gn[1]), dbeta=self.grad_out(gn_key + ".bias", gn[2]))
            if parts is not None:  # partial sums already taken by the data-gradient ring (ops.conv_dgrad_gn)
                x.grad = ops.gn_bwd_parts(dA, x.t, parts, gn[0], gn[1], gn[2], G, **acc)
            else:
                x.grad = ops.gn_bwd(dA, x.t, gn[0], gn[1], gn[2], G, **acc)
        self.grad_done(gn_key + ".weight")
        self.grad_done(gn_key + ".bias")

    def up_add(self, x, skip, stats=False):
        """upsamplex2 (trilinear, align_corners=False) + skip, unet3D.py:1646 / :1764-1783. ``stats``: the output feeds
        GroupNorm(16)s (a decoder block): take its statistics from the upsample's epilogue."""
        sk = skip.t if skip is not None else None
        y, st16 = ops.upsample2x_add_stats(x.t, sk) if stats else (ops.upsample2x_add(x.t, sk), None)
        out = Act(y)
        if st16 is not None:
            out.stats[16] = st16
        if self.record:
            def bwd():
                dy = out.grad
                if dy is None:
                    return
                if skip is not None:
                    self.acc_grad(skip, dy)
                x.grad = ops.upsample2x_bwd(dy, tuple(x.t.shape), dx=x.grad, accumulate=x.grad is not None)
            self.ops.append(bwd)
        return out

    def block(self, x, pre, stride, G):
        """NoBottleneck.forward, unet3D.py:56-73."""
        h = self.gn_conv(x, pre + "conv1", 3, stride, gn_key=pre + "gn1", G=G)
        if pre + "downsample.2.weight" in self.P:  # its GN backward runs paired with gn1's (prologue_bwd)
            r = self.gn_conv(x, pre + "downsample.2", 1, stride, gn_key=pre + "downsample.0", G=G,
                             park=ops.GN_BWD_PAIRS)
        else:
            r = x
        return self.gn_conv(h, pre + "conv2", 3, 1, gn_key=pre + "gn2", G=G, residual=r)

    # ------------------------------------------------------------------ graph
    def trunk(self, x, cfg):
        self.std = cfg.weight_std
        self.prepack(self.conv_plan(cfg))
        if cfg.conv0:
            t = self.stem(x, "conv0", 2)
            t = self.gn_conv(t, "conv1", 3, 1)
        else:
            t = self.stem(x, "conv1", 1)
        skips = []
        for i in range(5):
            for b in range(cfg.layers[i]):
                stride = 2 if (i > 0 and b == 0) else 1
                t = self.block(t, f"layer{i}.{b}.", stride, cfg.groups)
            skips.append(t)
        f = self.gn_conv(t, "fusionConv.2", 1, 1, gn_key="fusionConv.0", G=cfg.fusion_groups)
        bott = f
        self.dec = []  # decoder features after x8/x4/x2/x1_resb (unet3D_with_feam3 heads read the first three)
        for name, s in zip(["x8_resb", "x4_resb", "x2_resb", "x1_resb"], [skips[3], skips[2], skips[1], skips[0]]):
            u = self.up_add(f, s, stats=cfg.groups == 16)
            f = self.block(u, name + ".0.", 1, cfg.groups)
            self.dec.append(f)
        return f, bott

    def head(self, f, cfg):
        lg = self.gn_conv(f, "precls_conv.2", 1, 1, gn_key="precls_conv.0", G=cfg.head_groups, bias=True,
                          out_f32=True, standardize=False)
        if cfg.final_up:
            lg = self.up_add(lg, None)
        return lg

    def backward(self, out_act, grad):
        out_act.grad = grad
        for fn in reversed(self.ops):
            fn()
            if self.sink is not None and self.sink.flush_due:
                self.sink.flush_due = False
                self.flush_wgrads()
        self.flush_wgrads()
        self.ops = []


def compute_dtype(explicit=None):
    """bf16 under torch.autocast('cuda') (the reference's --FP16 amp path), fp32 otherwise."""
    if explicit is not None:
        return explicit
    if torch.is_autocast_enabled("cuda"):
        return torch.bfloat16
    return torch.float32


def ndhwc_grad(g, dtype=torch.float32):
    """An NCDHW gradient from autograd as the tape reads it: contiguous NDHWC in ``dtype``."""
    return g.permute(0, 2, 3, 4, 1).to(dtype).contiguous()


def ncdhw(t):
    return t.permute(0, 4, 1, 2, 3)


# How a builder's output crosses the autograd boundary: kind -> (what autograd sees of it, its incoming gradient in
# the form the tape reads; None: not differentiable).
NDHWC, NCDHW, TOKEN, STORED = "ndhwc", "ncdhw", "token", "stored"
CROSS = {
    NDHWC: (lambda a: ncdhw(a.t), ndhwc_grad),                             # an NDHWC Act: logits, deep maps
    NCDHW: (lambda a: a.t, lambda g: g.contiguous()),                      # an NCDHW fp32 Act: attention maps
    TOKEN: (lambda k: k.t.unsqueeze(0), lambda g: g.squeeze(0).float()),   # a feam.Tok [nt, C]: the class message
    STORED: (ncdhw, None),                                                 # a detached tensor: feature_stored
}


def wants_grad(tensors):
    return torch.is_grad_enabled() and any(p.requires_grad for p in tensors)


class TapeFn(torch.autograd.Function):
    """The one Function between autograd and a whole model step. ``build(tape, x)`` runs the forward on a recording
    tape and returns its outputs [(kind, value)], the primary one (NDHWC: what seeds the tape's replay) first."""

    @staticmethod
    def forward(ctx, build, dtype, names, x, *tensors):
        ctx.set_materialize_grads(False)  # an output no loss reads arrives as None and costs nothing
        tape = Tape.recording(names, tensors, dtype)
        outs = build(tape, x)
        ctx.tape, ctx.outs, ctx.names = tape, outs, names
        seen = [CROSS[kind][0](v) for kind, v in outs]
        ctx.mark_non_differentiable(*[t for t, (kind, _) in zip(seen, outs) if CROSS[kind][1] is None])
        # The partial loss may hand its gradient back unformed (loss.DeferredLossGrad) where the logits come straight
        # from the streaming head, and only to the models whose builder offers it (run_trunk). Offering it to the
        # feam / eam / deepsup models would change their launches (ops.head_loss_bwd for ops.head_bwd): a performance
        # change for a pull request of its own.
        ctx.link = None
        if tape.offer_head_link and tape.head_out is outs[0][1]:
            ctx.link = seen[0]._u3d_head_link = object()
        return tuple(seen)

    @staticmethod
    def backward(ctx, g, *grads):
        tape, outs = ctx.tape, ctx.outs
        for (kind, v), gv in zip(outs[1:], grads):
            if CROSS[kind][1] is not None:
                v.grad = CROSS[kind][1](gv) if gv is not None else None
        out = outs[0][1]
        if isinstance(g, DeferredLossGrad):
            if not (ctx.link is not None and g.link is ctx.link and g.unformed()):
                g = ndhwc_grad(g.materialize())  # (else: to the head's backward as is, ops.head_loss_bwd)
        elif g is None:  # no loss reads the primary output
            g = torch.zeros(out.t.shape, dtype=torch.float32, device=out.t.device)
        else:
            g = ndhwc_grad(g)
        tape.backward(out, g)
        pg = tape.finish(ctx.names)
        ctx.tape = ctx.outs = None
        return (*[None] * (len(ctx.needs_input_grad) - len(pg)), *pg)


def run_model(build, x, named_params, dtype=None, grad=True):
    """One model step on the native executor. ``build(tape, x)`` -> (primary output Act, {name: (kind, [values])});
    returns (the primary output NCDHW, {name: [tensors]}). Records under autograd when a parameter asks for a gradient
    (``grad`` false: never, an eval forward), else runs the same builder on a tape that records nothing."""
    ops.require_device(x)
    dtype = compute_dtype(dtype)
    if x.dtype != torch.float32 or not x.is_contiguous():
        x = x.float().contiguous()
    names = [n for n, _ in named_params]
    tensors = [p for _, p in named_params]
    sizes = {}

    def flat(tape, x):
        out, groups = build(tape, x)
        sizes.update((name, len(vs)) for name, (_, vs) in groups.items())
        return [(NDHWC, out)] + [(kind, v) for kind, vs in groups.values() for v in vs]

    if grad and wants_grad(tensors):
        seen = TapeFn.apply(flat, dtype, names, x, *tensors)
    else:
        with torch.no_grad():
            seen = [CROSS[kind][0](v) for kind, v in flat(Tape(dict(zip(names, tensors)), dtype, record=False), x)]
    rest = iter(seen[1:])
    return seen[0], {name: [next(rest) for _ in range(n)] for name, n in sizes.items()}


def run_trunk(cfg, x, named_params, dtype=None):
    """Forward the trunk + classification head. Returns NCDHW-shaped fp32 logits (NDHWC storage)."""
    def build(tape, x):
        f, _ = tape.trunk(x, cfg)
        tape.offer_head_link = True  # these logits may take the partial loss's gradient unformed (TapeFn)
        return tape.head(f, cfg), {}
    return run_model(build, x, named_params, dtype)[0]
