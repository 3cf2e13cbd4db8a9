"""The decoder-level heads of the feam / eam / deepsup models on the native executor (reference unet3D.py:938-1190),
forward and backward. The models run through trunk.run_model / trunk.TapeFn like every other; this module holds their
builders and the tape ops those use.

_feam3_forward: the shared trunk tape (conv1 .. x1_resb, precls_conv), plus at each of the x8 / x4 / x2 decoder levels
what the model's Level record asks for, in this order:
  * deepout{1,2,3} = GN(16) -> ReLU -> Conv3d 1^3 + bias (:969-993, same fused GN-prologue conv as precls_conv);
  * a detached copy of the feature (feature_stored, :1129);
  * renew_token (:1051-1068): u3d_renew_token on the feature, in place on the device class token;
  * the EAM attention map against the detached class token (:1131-1175): u3d_eam_prep (token side: LN3, q, M) and
    u3d_eam_attn_fwd (per-voxel LN2 + Nt x C GEMV, written NCDHW), x8/x4/x2 trilinear-upsampled to full size when
    deep_up (u3d_upsample_trilinear).
Each unet3D class states its own three Levels (unet3D_with_feam3 / _feam2 / _deepsup / _feam). Backward: every output
gradient that autograd hands in (unused outputs arrive as None and cost nothing) is pushed through the same kernels'
backward (u3d_upsample_trilinear_bwd, u3d_eam_attn_bwd, u3d_eam_param_bwd, the 1^3 head backward) by the closures the
ops recorded, accumulated into the decoder features' gradients, then the trunk's closures replay.

_eam_forward: unet3D_with_eam / unet3D_with_eam_baseline (:431-582, :1370-1504) run the whole EAM (eam_pool_op: the
score map and the class message cm, u3d_eam_pool_fwd / _bwd) in a cascade down the decoder, each level's cm through a
Linear the next level's token.
"""
from dataclasses import dataclass

import torch
import torch.nn.functional as F

from . import ops, trunk

EAM_KEYS = ("eam84", "eam42", "eam21")
UP_SCALE = (8, 4, 2)   # upsamplex4 / upsamplex3 / upsamplex2 for deep_up (:1138, :1156, :1175)
NUM_HEADS = 4          # EAM(dim, num_heads=4) (:975, :985, :996)


def _eam_shape_error(n, v, c):
    """The reference's kv reshape uses the token's batch of 1 (unet3D.py:189, :198): B > 1 fails there."""
    return RuntimeError(f"shape '[1, {v}, 2, {NUM_HEADS}, {c // NUM_HEADS}]' is invalid for input of size "
                        f"{n * v * 2 * c}")


def upsample_trilinear(x, s):
    """NCDHW fp32 [n, c, d, h, w] -> [n, c, sd, sh, sw] (nn.Upsample(scale_factor=s, mode='trilinear'))."""
    n, c, d, h, w = x.shape
    y = torch.empty((n, c, d * s, h * s, w * s), dtype=torch.float32, device=x.device)
    ops.call("u3d_upsample_trilinear", x.data_ptr(), n * c, d, h, w, s, y.data_ptr(), ops._stream())
    return y


def upsample_trilinear_bwd(dy, in_shape, s):
    n, c, d, h, w = in_shape
    if dy.dtype != torch.float32 or not dy.is_contiguous():
        dy = dy.float().contiguous()
    dx = torch.empty(in_shape, dtype=torch.float32, device=dy.device)
    ws = torch.empty(ops.query("u3d_upsample_trilinear_bwd_ws_floats", n * c, d, h, w, s), dtype=torch.float32,
                     device=dy.device)
    ops.call("u3d_upsample_trilinear_bwd", dy.data_ptr(), n * c, d, h, w, s, dx.data_ptr(), 0, ws.data_ptr(),
         ops._stream())
    return dx


def eam_op(tape, f, key, token, up):
    """EAM attention map of decoder feature ``f`` (Act, NDHWC) against ``token`` [nt, C] -> Act holding the NCDHW
    fp32 map [n, nt, d, h, w] (upsampled x``up`` when up > 1). Records its backward on the tape."""
    P = tape.P
    x = f.t
    n, d, h, w, c = x.shape
    v = d * h * w
    if n != 1:
        raise _eam_shape_error(n, v, c)
    nt = token.shape[0]
    dev = x.device
    tok = token.detach().float().contiguous()
    wk = P[key + ".kv.weight"]            # [2c, c]: rows 0..c-1 = k (kv reshape (2, heads, c/heads), :198-199)
    wq = P[key + ".q.weight"]
    g2, b2 = P[key + ".norm2.weight"], P[key + ".norm2.bias"]
    g3, b3 = P[key + ".norm3.weight"], P[key + ".norm3.bias"]
    zhat, q, M = (torch.empty((nt, c), dtype=torch.float32, device=dev) for _ in range(3))
    inv_h = 1.0 / NUM_HEADS
    st = ops._stream()
    ops.call("u3d_eam_prep", tok.data_ptr(), nt, c, g3.data_ptr(), b3.data_ptr(), wq.data_ptr(), wk.data_ptr(), inv_h,
         zhat.data_ptr(), q.data_ptr(), M.data_ptr(), st)
    att = torch.empty((n, nt, d, h, w), dtype=torch.float32, device=dev)
    ops.call("u3d_eam_attn_fwd", ops.dt_code(x.dtype), x.data_ptr(), n, v, c, g2.data_ptr(), b2.data_ptr(),
             M.data_ptr(), nt, att.data_ptr(), st)
    out = trunk.Act(upsample_trilinear(att, up) if up > 1 else att)
    if tape.record:
        def bwd():
            g = out.grad
            if g is None:
                return
            g = upsample_trilinear_bwd(g, tuple(att.shape), up) if up > 1 else g.float().contiguous()
            part = torch.empty(ops.query("u3d_eam_attn_bwd_part_floats", n, v, c, nt), dtype=torch.float32, device=dev)
            dM = torch.empty((nt, c), dtype=torch.float32, device=dev)
            dg2 = tape.grad_out(key + ".norm2.weight", g2)
            db2 = tape.grad_out(key + ".norm2.bias", b2)
            acc = f.grad is not None
            dx = f.grad if acc else torch.empty_like(x)
            s = ops._stream()
            ops.call("u3d_eam_attn_bwd", ops.dt_code(x.dtype), x.data_ptr(), n, v, c, g2.data_ptr(), b2.data_ptr(),
                 M.data_ptr(), nt, g.data_ptr(), dx.data_ptr(), int(acc), part.data_ptr(), dM.data_ptr(),
                 dg2.data_ptr(), db2.data_ptr(), 0, s)
            f.grad = dx
            dwq = tape.grad_out(key + ".q.weight", wq)
            dkv = tape.grad_out(key + ".kv.weight", wk)
            dg3 = tape.grad_out(key + ".norm3.weight", g3)
            db3 = tape.grad_out(key + ".norm3.bias", b3)
            dq_ws, dz_ws = torch.empty((nt, c), dtype=torch.float32, device=dev), torch.empty_like(dM)
            ops.call("u3d_eam_param_bwd", dM.data_ptr(), nt, c, zhat.data_ptr(), g3.data_ptr(), b3.data_ptr(),
                 wq.data_ptr(), wk.data_ptr(), q.data_ptr(), inv_h, dq_ws.data_ptr(), dz_ws.data_ptr(),
                 dwq.data_ptr(), dkv.data_ptr(), dg3.data_ptr(), db3.data_ptr(), 0, s)
            for nm in (".norm2.weight", ".norm2.bias", ".q.weight", ".kv.weight", ".norm3.weight", ".norm3.bias"):
                tape.grad_done(key + nm)
        tape.ops.append(bwd)
    return out


class Tok:
    """A token-side value [nt, c] (fp32, outside autograd) and its accumulated gradient: the class token, a level's
    class message, the Linear that hands it to the next level."""
    __slots__ = ("t", "grad")

    def __init__(self, t):
        self.t = t
        self.grad = None

    def acc(self, g):
        self.grad = g if self.grad is None else self.grad + g


def _pool_before(tok, g3, b3, wq, wk):
    """Token side before the voxel pass: z = LN3(tok), q = z Wq^T, A[i nt + t] = q[t, head i] Wk[head i, :]."""
    c = tok.shape[1]
    hd = c // NUM_HEADS
    q = F.layer_norm(tok, (c,), g3, b3, 1e-5) @ wq.t()
    return torch.cat([q[:, i * hd:(i + 1) * hd] @ wk[i * hd:(i + 1) * hd] for i in range(NUM_HEADS)], 0)


def _pool_after(yhat, g2, b2, wv, pw, pb):
    """Token side after it: Y = Yhat g2 + b2 (the softmax sums to 1), O[t, head i] = Wv[head i, :] . Y[i nt + t],
    cm = proj(norm2(O)) + O (norm2 a second time, unet3D.py:206)."""
    c = yhat.shape[1]
    hd, nt = c // NUM_HEADS, yhat.shape[0] // NUM_HEADS
    y = yhat * g2 + b2
    o = torch.cat([y[i * nt:(i + 1) * nt] @ wv[i * hd:(i + 1) * hd].t() for i in range(NUM_HEADS)], 1)
    return F.linear(F.layer_norm(o, (c,), g2, b2, 1e-5), pw, pb) + o


def _leaves(*ts):
    return [t.detach().requires_grad_(True) for t in ts]


def _param_grads(tape, named):
    """Hand finished parameter gradients [(name, parameter, gradient)] to the tape (a DDP bucket view or a tensor)."""
    for name, p, g in named:
        tape.grad_out(name, p).copy_(g)
        tape.grad_done(name)


def eam_pool_op(tape, f, key, tok):
    """The whole EAM (unet3D.py:186-212) of decoder feature ``f`` (Act, NDHWC, batch 1) against ``tok`` (Tok [nt, C],
    not detached) -> (Act holding the head-mean score map [1, nt, d, h, w], NCDHW fp32; Tok holding the class message
    cm [nt, C]). The voxel side is u3d_eam_pool_fwd / _bwd: scores, softmax over all voxels and the pooling in one pass
    over the feature, no k / v projection formed. The token side (<= 16 x 128: LN3, q, A before; Y, O, proj(norm2) +
    residual after) is torch device operations, differentiated inside the backward closure by a local graph."""
    P = tape.P
    x = f.t
    n, d, h, w, c = x.shape
    v = d * h * w
    if n != 1:
        raise _eam_shape_error(n, v, c)
    nt = tok.t.shape[0]
    rows = NUM_HEADS * nt
    scale = float((c // NUM_HEADS) ** -0.5)
    dev = x.device
    names = [key + s for s in (".kv.weight", ".q.weight", ".proj.weight", ".proj.bias", ".norm2.weight", ".norm2.bias",
                               ".norm3.weight", ".norm3.bias")]
    kv, wq, pw, pb, g2, b2, g3, b3 = (P[nm] for nm in names)
    new = lambda *s: torch.empty(s, dtype=torch.float32, device=dev)   # noqa: E731
    with torch.no_grad():
        A = _pool_before(tok.t, g3, b3, wq, kv[:c]).contiguous()
    att, yhat, stat = new(n, nt, d, h, w), new(rows, c), new(2 * rows)
    npart = ops.query("u3d_eam_pool_part_floats", v, c, nt)
    ops.call("u3d_eam_pool_fwd", ops.dt_code(x.dtype), x.data_ptr(), n, v, c, g2.data_ptr(), b2.data_ptr(),
             A.data_ptr(), nt, NUM_HEADS, scale, att.data_ptr(), yhat.data_ptr(), stat.data_ptr(),
             new(npart).data_ptr(), ops._stream())
    with torch.no_grad():
        cm = Tok(_pool_after(yhat, g2, b2, kv[c:], pw, pb))
    out = trunk.Act(att)
    if tape.record:
        def bwd():
            gatt, gcm = out.grad, cm.grad
            if gatt is None and gcm is None:
                return
            pg = {}
            dy = dd = None
            if gcm is not None:      # cm -> dYhat and the token-side halves of norm2, kv (v rows), proj
                with torch.enable_grad():
                    lv = _leaves(yhat, g2, b2, kv, pw, pb)
                    gs = torch.autograd.grad(_pool_after(lv[0], lv[1], lv[2], lv[3][c:], lv[4], lv[5]), lv, gcm)
                dy = gs[0].contiguous()
                dd = (dy * yhat).sum(1)
                pg.update(zip((names[4], names[5], names[0], names[2], names[3]), gs[1:]))
            if gatt is not None:
                gatt = gatt.float().contiguous()
            dA, dg2, db2 = new(rows, c), new(c), new(c)
            acc = f.grad is not None
            dx = f.grad if acc else torch.empty_like(x)
            ptr = lambda t: t.data_ptr() if t is not None else 0       # noqa: E731
            ops.call("u3d_eam_pool_bwd", ops.dt_code(x.dtype), x.data_ptr(), n, v, c, g2.data_ptr(), b2.data_ptr(),
                 A.data_ptr(), nt, NUM_HEADS, scale, stat.data_ptr(), ptr(dy), ptr(dd), ptr(gatt), dx.data_ptr(),
                 int(acc), new(npart).data_ptr(), dA.data_ptr(), dg2.data_ptr(), db2.data_ptr(), 0, ops._stream())
            f.grad = dx
            with torch.enable_grad():  # dA -> the token, norm3, q and the k rows of kv
                lv = _leaves(tok.t, g3, b3, wq, kv)
                gs = torch.autograd.grad(_pool_before(lv[0], lv[1], lv[2], lv[3], lv[4][:c]), lv, dA)
            tok.acc(gs[0])
            for nm, g in ((names[4], dg2), (names[5], db2), (names[6], gs[1]), (names[7], gs[2]), (names[1], gs[3]),
                          (names[0], gs[4])):
                pg[nm] = pg[nm] + g if nm in pg else g
            _param_grads(tape, [(nm, P[nm], g) for nm, g in pg.items()])
        tape.ops.append(bwd)
    return out, cm


def tok_linear(tape, tok, key):
    """nn.Linear on a class message (linear84_2_42 / linear42_2_21, unet3D.py:552, :564): Tok [nt, cin] -> Tok [nt, cout]."""
    W, b = tape.P[key + ".weight"], tape.P[key + ".bias"]
    with torch.no_grad():
        out = Tok(torch.addmm(b, tok.t, W.t()))
    if tape.record:
        def bwd():
            g = out.grad
            if g is None:
                return
            _param_grads(tape, [(key + ".weight", W, g.t() @ tok.t), (key + ".bias", b, g.sum(0))])
            tok.acc(g @ W)
        tape.ops.append(bwd)
    return out


EAM_LINEAR_KEYS = ("linear84_2_42", "linear42_2_21")


def _eam_forward(tape, cfg, x, gates):
    """unet3D_with_eam / _eam_baseline (unet3D.py:508-582, :1440-1504): the trunk, then the cascade of EAMs down the
    decoder, each level's class message through a Linear the next level's token. gates[k]: level k runs (the
    reference's cumulative use_cm tests; () in eval: the trunk and the logits head alone). Returns the logits Act and
    the outputs {cm: the last level's Tok, if a level ran; atten: the map Acts}."""
    root = None
    if gates and gates[0]:
        root = Tok(tape.P["class_token"].detach())
        if tape.record:
            def bwd():   # recorded first, so it runs last: every level has added its share by then
                if root.grad is not None:
                    _param_grads(tape, [("class_token", tape.P["class_token"], root.grad)])
            tape.ops.append(bwd)
    f, _ = tape.trunk(x, cfg)
    lg = tape.head(f, cfg)
    cm, att = None, []
    for k, on in enumerate(gates):
        if not on:
            break
        tok = root if k == 0 else tok_linear(tape, cm, EAM_LINEAR_KEYS[k - 1])
        a, cm = eam_pool_op(tape, tape.dec[k], EAM_KEYS[k], tok)
        att.append(a)
    return lg, {"cm": (trunk.TOKEN, [cm] if cm is not None else []), "atten": (trunk.NCDHW, att)}


def run_eam(model, x, gates):
    """model: unet3D.unet3D_with_eam / unet3D_with_eam_baseline. train: (logits, cm [1, nt, C] or None, atten_map);
    eval: logits (the EAMs are not run)."""
    gates = tuple(bool(g) for g in gates) if model.training else ()
    lg, outs = trunk.run_model(lambda tape, x: _eam_forward(tape, model._u3d_cfg, x, gates), x,
                               list(model.named_parameters()), getattr(model, "compute_dtype", None),
                               grad=model.training)
    if not model.training:
        return lg
    return lg, outs["cm"][0] if outs["cm"] else None, outs["atten"]


@dataclass(frozen=True)
class Level:
    """What a model does with the decoder feature after x8 / x4 / x2_resb, in the order it happens there."""
    deep: bool = False     # the deep-supervision head deepout{1,2,3} (unet3D.py:969-993)
    store: bool = False    # a detached copy of the feature (feature_stored, :1129)
    renew: tuple = None    # (mask, classes, alpha): ``token`` updated in place from the feature first (:869-878)
    token: object = None   # the level's class token [classes - 1, C]
    attend: bool = False   # the EAM attention map against the detached token (:1131-1175)
    up: int = 1            # the map trilinear-upsampled by this factor (deep_up)


def _feam3_forward(tape, cfg, x, levels):
    """The trunk, the logits head and, per decoder level, what its Level asks for (none in eval). Returns the logits
    Act and the outputs {atten, deep, stored}."""
    f, _ = tape.trunk(x, cfg)
    lg = tape.head(f, cfg)
    att, deep, feats = [], [], []
    for k, lv in enumerate(levels):
        fk = tape.dec[k]
        if lv.deep:
            deep.append(tape.gn_conv(fk, f"deepout{k + 1}.2", 1, 1, gn_key=f"deepout{k + 1}.0", G=16, bias=True,
                                     out_f32=True, standardize=False))
        if lv.store:
            feats.append(fk.t.detach().clone())
        if lv.renew is not None:
            renew_token([lv.token], [trunk.ncdhw(fk.t)], *lv.renew)
        if lv.attend:
            att.append(eam_op(tape, fk, EAM_KEYS[k], lv.token, lv.up))
    return lg, {"atten": (trunk.NCDHW, att), "deep": (trunk.NDHWC, deep), "stored": (trunk.STORED, feats)}


def labels_reach(mask, sizes, ncls):
    """True when a label 1..ncls of ``mask`` [n, 1, D, H, W] survives the nearest resize to one of ``sizes``: the
    condition under which the reference's in-forward token renewal writes a token (unet3D.py:1301-1308). One host
    synchronisation; callers ask only where the answer decides between an error and a gradient run."""
    valid = ((mask >= 1) & (mask <= ncls) & (mask == mask.floor())).float()
    return any(bool(F.interpolate(valid, s, mode="nearest").any()) for s in sizes)


def run_feam3(model, x, levels):
    """model: unet3D.unet3D_with_feam3 / _feam2 / _deepsup / _feam, ``levels`` its three Levels (x8, x4, x2). Returns
    train: (logits, atten_map, deep_map, feature_stored), each list as long as the levels make it; eval: logits."""
    ops.require_device(x)
    named = list(model.named_parameters())
    if not model.training:
        levels = ()
    elif any(lv.renew is not None for lv in levels) and trunk.wants_grad([p for _, p in named]):
        raise RuntimeError("a leaf Variable that requires grad is being used in an in-place operation.")
    lg, outs = trunk.run_model(lambda tape, x: _feam3_forward(tape, model._u3d_cfg, x, levels), x, named,
                               getattr(model, "compute_dtype", None), grad=model.training)
    if not model.training:
        return lg
    return lg, outs["atten"], outs["deep"], outs["stored"]


def renew_token(tokens, features, mask, num_classes, alpha):
    """u3d_renew_token per level (unet3D.py:1051-1068). tokens: device fp32 [nc-1, C] tensors, updated in place."""
    mask = mask.float().contiguous()
    ops.require_device(mask, *tokens)
    n, _, md, mh, mw = mask.shape
    for tok, feat in zip(tokens, features):
        nb, c, d, h, w = feat.shape
        if nb != n:
            raise RuntimeError(f"renew_token: feature batch {nb} != mask batch {n}")
        v = d * h * w
        st = feat.stride()
        if st[1] == 1 and st[4] == c and st[0] == v * c:       # NCDHW view of NDHWC storage (our features)
            sv, sc = c, 1
        elif feat.is_contiguous():                           # plain NCDHW
            sv, sc = 1, v
        else:
            feat = feat.contiguous()
            sv, sc = 1, v
        if feat.dtype not in (torch.float32, torch.bfloat16):
            feat = feat.float()
        ops.require_device(feat)
        ws = ops.WS.get(ops.query("u3d_renew_token_ws_bytes", n, d, h, w, num_classes, c), feat.device,
                        ops.Slot.RENEW_TOKEN)
        ops.call("u3d_renew_token", ops.dt_code(feat.dtype), feat.data_ptr(), sv, sc, n, d, h, w, c, mask.data_ptr(),
             md, mh, mw, num_classes, tok.shape[0], float(alpha), tok.data_ptr(), ws.data_ptr(), ops._stream())
