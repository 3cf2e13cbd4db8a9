"""Autograd Function for the fused partial-label Dice + BCE loss (reference loss_partial.py:59-99)."""
import ctypes

import torch
from torch.utils import _pytree as pytree

from . import ops

MODE_SIGMOID, MODE_SOFTMAX, MODE_IDENTITY = 0, 1, 2


def ndhwc_view(x):
    """[S, C, D, H, W] -> NDHWC-contiguous [S, D, H, W, C] (free when x came from the native head)."""
    y = x.permute(0, 2, 3, 4, 1)
    return y if y.is_contiguous() else y.contiguous()


def class_weights(mask, C, device):
    """mask[0] of the reference (only the first sample's supervision vector is used, loss_partial.py:87)."""
    if mask is None:
        return torch.ones(C, dtype=torch.float32, device=device)
    w = mask[0]
    if not torch.is_tensor(w):
        w = torch.tensor(w)
    if w.numel() < C:
        raise IndexError(f"index {w.numel()} is out of bounds for dimension 0 with size {w.numel()} "
                         f"(mask[0] shorter than the {C} classes, as the reference's weight[i] would fail)")
    return w.reshape(-1)[:C].to(device=device, dtype=torch.float32)


def sample_weights(mask, S, C, device):
    """One supervision row per sample: [S, C] fp32 for the per-sample losses (DESIGN.md "Per-sample supervision").
    mask: a list of S rows (lists or tensors) or a tensor [S, >= C]; None = all ones. A tensor that already lives on
    the device is sliced and cast there without a host read, so a captured step can feed it from a static tensor.
    A row count other than S is a ValueError, rows shorter than C an IndexError (as class_weights)."""
    if mask is None:
        return torch.ones((S, C), dtype=torch.float32, device=device)
    if torch.is_tensor(mask):
        if mask.dim() != 2:
            raise ValueError(f"sample_weights: a [S, >= C] tensor or a list of S rows expected, got {tuple(mask.shape)}")
        rows = mask
    else:
        rows = list(mask)
        if len(rows) != S:
            raise ValueError(f"sample_weights: {len(rows)} mask rows for a batch of {S}")
        rows = [r if torch.is_tensor(r) else torch.tensor(r) for r in rows]
        for r in rows:
            if r.numel() < C:
                raise IndexError(f"index {r.numel()} is out of bounds for dimension 0 with size {r.numel()} "
                                 f"(a mask row shorter than the {C} classes)")
        rows = torch.stack([r.reshape(-1)[:C].to(device=device, dtype=torch.float32) for r in rows])
    if rows.shape[0] != S:
        raise ValueError(f"sample_weights: {rows.shape[0]} mask rows for a batch of {S}")
    if rows.shape[1] < C:
        raise IndexError(f"index {rows.shape[1]} is out of bounds for dimension 1 with size {rows.shape[1]} "
                         f"(mask rows shorter than the {C} classes)")
    return rows[:, :C].to(device=device, dtype=torch.float32).contiguous()


class DeferredLossGrad(torch.Tensor):
    """The partial loss's gradient w.r.t. the trunk's logits, handed back unformed when the logits came straight from
    the streaming head (trunk.TapeFn tags them): the trunk's backward passes it to the head, whose backward forms the
    loss gradient in registers (ops.head_loss_bwd) — the fp32 dlogits tensor (113 MB at 2 x 96^3 x 16) is never
    written or read. Anything else that touches it (a hook, torch.autograd.grad on the logits, a sum with another
    gradient) goes through __torch_dispatch__, which forms the real gradient first (ops.partial_loss_bwd): every
    reader sees the same values as without the hand-off."""

    @staticmethod
    def __new__(cls, like, make, payload, link):
        shape, stride, dtype, device = like
        r = torch.Tensor._make_wrapper_subclass(cls, shape, strides=stride, dtype=dtype, device=device)
        r._make, r.payload, r.link, r._real = make, payload, link, None
        return r

    def unformed(self):
        return self._real is None

    def materialize(self):
        if self._real is None:
            self._real = self._make()
            self.payload = None
        return self._real

    __torch_function__ = torch._C._disabled_torch_function_impl

    @classmethod
    def __torch_dispatch__(cls, func, types, args=(), kwargs=None):
        def real(t):
            return t.materialize() if isinstance(t, DeferredLossGrad) else t
        return func(*pytree.tree_map(real, args), **pytree.tree_map(real, kwargs or {}))

    def __repr__(self):
        return f"DeferredLossGrad(shape={tuple(self.shape)}, formed={self._real is not None})"


class _PartialLossFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, target, weights, mode, uce):
        lg = ndhwc_view(logits.float())
        lab = target.float().contiguous()
        loss, sums = ops.partial_loss_fwd(lg, lab, weights, mode, uce)
        ctx.save_for_backward(lg, lab, weights, sums)
        ctx.mode, ctx.uce = mode, uce
        link = getattr(logits, "_u3d_head_link", None)
        ctx.link = (link if ops.HEAD_LOSS_FUSED and link is not None and mode == MODE_SOFTMAX and int(uce) == 1
                    and lg.shape[-1] == 16 and lg.dtype == torch.float32 else None)
        ctx.like = (tuple(logits.shape), tuple(logits.stride()), logits.dtype, logits.device)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        lg, lab, weights, sums = ctx.saved_tensors
        go = g.reshape(1).float().contiguous()
        mode, uce = ctx.mode, ctx.uce

        def form():
            return ops.partial_loss_bwd(lg, lab, weights, sums, go, mode, uce).permute(0, 4, 1, 2, 3)
        if ctx.link is not None:
            return DeferredLossGrad(ctx.like, form, (lg, lab, weights, sums, go), ctx.link), None, None, None, None
        return form(), None, None, None, None


class _PartialLossPsFn(torch.autograd.Function):
    """The partial loss with one supervision row per sample (weights [S, C], ops.partial_loss_ps_fwd/_bwd)."""

    @staticmethod
    def forward(ctx, logits, target, weights, mode, uce):
        lg = ndhwc_view(logits.float())
        lab = target.float().contiguous()
        loss, _, pooled = ops.partial_loss_ps_fwd(lg, lab, weights, mode, uce)
        ctx.save_for_backward(lg, lab, weights, pooled)
        ctx.mode, ctx.uce = mode, uce
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        lg, lab, weights, pooled = ctx.saved_tensors
        go = g.reshape(1).float().contiguous()
        # The streaming head's deferred hand-off (DeferredLossGrad, ops.head_loss_bwd) is declined on purpose, even
        # when the logits carry a _u3d_head_link: the fused head + loss backward forms the batch loss's gradient from
        # one weight row. The gradient here always comes from the per-sample backward kernel; porting the hand-off
        # is a performance change of its own.
        dl = ops.partial_loss_ps_bwd(lg, lab, weights, pooled, go, ctx.mode, ctx.uce)
        return dl.permute(0, 4, 1, 2, 3), None, None, None, None


def partial_loss(logits, target, weights, mode=MODE_SOFTMAX, uce=True):
    """weights [C]: the batch loss (the reference's mask[0] for every sample). weights [S, C] (sample_weights): the
    per-sample loss; uce must then be 0 or 1."""
    ops.require_device(logits, target)
    if target.shape[0] != logits.shape[0] or target.numel() * logits.shape[1] != logits.numel():
        raise AssertionError(f"predict {tuple(logits.shape)} & target {tuple(target.shape)} shape do not match")
    if weights.dim() == 2:
        if tuple(weights.shape) != (logits.shape[0], logits.shape[1]):
            raise ValueError(f"partial_loss: per-sample weights {tuple(weights.shape)} for logits "
                             f"{tuple(logits.shape)}: [S, C] expected")
        return _PartialLossPsFn.apply(logits, target, weights.float().contiguous(), mode, uce)
    return _PartialLossFn.apply(logits, target, weights, mode, uce)


# ------------------------------------------------------------------ deep supervision (losses.py:119-129)
DEEP_WEIGHTS = (0.125, 0.25, 0.5, 1.0)   # losses.py:116


def _deepsup_host_args(lgs, level_weights):
    """The per-level host arrays of u3d_deepsup_loss_fwd/_bwd (read during the call only)."""
    L = len(lgs)
    ptrs = (ctypes.c_void_p * L)(*[t.data_ptr() for t in lgs])
    dims = (ctypes.c_int * (3 * L))(*[int(n) for t in lgs for n in t.shape[1:4]])
    lw = (ctypes.c_float * L)(*[float(w) for w in level_weights])
    return ptrs, dims, lw


class _DeepSupFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, target, weights, level_weights, *deep):
        lgs = [ndhwc_view(l.float()) for l in deep]
        tgt = target.float().contiguous()
        L, (S, C) = len(lgs), (lgs[0].shape[0], lgs[0].shape[-1])
        D, H, W = tgt.shape[-3:]
        dev = tgt.device
        sums = torch.empty((L, C, 4), dtype=torch.float64, device=dev)
        level_loss = torch.empty(L, dtype=torch.float32, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        ws = ops.WS.get(_lib_query("u3d_deepsup_loss_workspace_bytes", L, C), dev, ops.Slot.DEEPSUP)
        ptrs, dims, lw = _deepsup_host_args(lgs, level_weights)
        ops.call("u3d_deepsup_loss_fwd", L, ptrs, dims, lw, tgt.data_ptr(), S, D, H, W, C, weights.data_ptr(),
                 sums.data_ptr(), level_loss.data_ptr(), loss.data_ptr(), ws.data_ptr(), ops._stream())
        ctx.save_for_backward(tgt, weights, sums, *lgs)
        ctx.level_weights = tuple(level_weights)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        tgt, weights, sums, *lgs = ctx.saved_tensors
        L, (S, C) = len(lgs), (lgs[0].shape[0], lgs[0].shape[-1])
        D, H, W = tgt.shape[-3:]
        go = g.reshape(1).float().contiguous()
        dls = [torch.empty_like(t) for t in lgs]
        ptrs, dims, lw = _deepsup_host_args(lgs, ctx.level_weights)
        dptrs = (ctypes.c_void_p * L)(*[t.data_ptr() for t in dls])
        ops.call("u3d_deepsup_loss_bwd", L, ptrs, dims, lw, tgt.data_ptr(), S, D, H, W, C, weights.data_ptr(),
                 sums.data_ptr(), go.data_ptr(), dptrs, ops._stream())
        # NCDHW-shaped views over NDHWC storage: what the native heads' backward takes without a copy
        return (None, None, None, *[d.permute(0, 4, 1, 2, 3) for d in dls])


class _DeepSupPsFn(torch.autograd.Function):
    """_DeepSupFn with one supervision row per sample (weights [S, C], u3d_deepsup_loss_ps_fwd/_bwd)."""

    @staticmethod
    def forward(ctx, target, weights, level_weights, *deep):
        lgs = [ndhwc_view(l.float()) for l in deep]
        tgt = target.float().contiguous()
        L, (S, C) = len(lgs), (lgs[0].shape[0], lgs[0].shape[-1])
        D, H, W = tgt.shape[-3:]
        dev = tgt.device
        sums_ps = torch.empty((L, S, C, 4), dtype=torch.float64, device=dev)
        pooled = torch.empty((L, C, 5), dtype=torch.float64, device=dev)
        level_loss = torch.empty(L, dtype=torch.float32, device=dev)
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        ws = ops.WS.get(_lib_query("u3d_deepsup_loss_ps_workspace_bytes", L, C, S), dev, ops.Slot.DEEPSUP_PS)
        ptrs, dims, lw = _deepsup_host_args(lgs, level_weights)
        ops.call("u3d_deepsup_loss_ps_fwd", L, ptrs, dims, lw, tgt.data_ptr(), S, D, H, W, C, weights.data_ptr(),
                 sums_ps.data_ptr(), pooled.data_ptr(), level_loss.data_ptr(), loss.data_ptr(), ws.data_ptr(),
                 ops._stream())
        ctx.save_for_backward(tgt, weights, pooled, *lgs)
        ctx.level_weights = tuple(level_weights)
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        tgt, weights, pooled, *lgs = ctx.saved_tensors
        L, (S, C) = len(lgs), (lgs[0].shape[0], lgs[0].shape[-1])
        D, H, W = tgt.shape[-3:]
        go = g.reshape(1).float().contiguous()
        dls = [torch.empty_like(t) for t in lgs]
        ptrs, dims, lw = _deepsup_host_args(lgs, ctx.level_weights)
        dptrs = (ctypes.c_void_p * L)(*[t.data_ptr() for t in dls])
        ops.call("u3d_deepsup_loss_ps_bwd", L, ptrs, dims, lw, tgt.data_ptr(), S, D, H, W, C, weights.data_ptr(),
                 pooled.data_ptr(), go.data_ptr(), dptrs, ops._stream())
        return (None, None, None, *[d.permute(0, 4, 1, 2, 3) for d in dls])


def deep_supervision_loss(deep_out, target, mask=None, level_weights=DEEP_WEIGHTS, per_sample=False):
    """get_loss's deep-supervision term (losses.py:119-129): sum over the levels of level_weights[idx] *
    EDiceLoss_partial(C)(l, F.interpolate(target, l.shape[2:], mode='nearest').squeeze(1), soft_max=True, mask=mask,
    uce=False), as one fused multi-level pass each way (u3d_deepsup_loss_fwd/_bwd; the resized targets are never
    built). deep_out: [S, C, d, h, w] logits per level (NCDHW views of NDHWC storage, as the native heads return, are
    read in place; plain NCDHW costs one copy); target [S, 1, D, H, W] (or [S, D, H, W]). More levels than weights
    raise IndexError (weights[idx]), a level with another C or batch AssertionError, as the reference.
    per_sample: ``mask`` holds one row per sample (sample_weights) and every level pools its sums over the samples
    that supervise the class; the default weights the whole batch with mask[0], as the reference."""
    deep_out = list(deep_out)
    if len(deep_out) == 0:
        raise ValueError("deep_supervision_loss: no levels")
    C = deep_out[0].shape[1]
    check_deep_levels(deep_out, target, C, len(level_weights))
    ops.require_device(target, *deep_out)
    fn = _DeepSupPsFn if per_sample else _DeepSupFn
    w = sample_weights(mask, target.shape[0], C, target.device) if per_sample else class_weights(mask, C, target.device)
    return fn.apply(target[:, 0] if target.dim() == 5 else target, w,
                    tuple(float(x) for x in level_weights[:len(deep_out)]), *deep_out)


def check_deep_levels(deep_out, target, C, n_weights=len(DEEP_WEIGHTS)):
    """The failures of the reference's loop over the levels (losses.py:121-129), in its order: a level past the
    weights list is an IndexError (weights[idx]); a level whose class count or batch differs from the one-hot
    target's is DiceLoss's AssertionError (loss_partial.py:46)."""
    if target.dim() not in (4, 5) or (target.dim() == 5 and target.shape[1] != 1):
        raise AssertionError(f"target {tuple(target.shape)}: [S, 1, D, H, W] labels expected")
    for idx, l in enumerate(deep_out):
        if l.dim() != 5 or l.shape[0] != target.shape[0] or l.shape[1] != C:
            raise AssertionError(f"predict {tuple(l.shape)} & target {(target.shape[0], C) + tuple(l.shape[2:])} "
                                 "shape do not match")
        if idx >= n_weights:
            raise IndexError("list index out of range")


# ------------------------------------------------------------------ consistency branch (losses.py:131-178)
def _voxel_strides(t, lead):
    """Element strides (lead dims..., voxel) of a [*lead, D, H, W] view whose spatial dims are voxel-linear
    (NCDHW or an NCDHW view of NDHWC storage); otherwise a contiguous copy is made."""
    st, sh = t.stride(), t.shape
    d = len(st) - 3
    if st[d + 1] == sh[d + 2] * st[d + 2] and st[d] == sh[d + 1] * st[d + 1]:
        return t, [st[i] for i in range(lead)] + [st[d + 2]]
    t = t.contiguous()
    return t, [t.stride(i) for i in range(lead)] + [1]


def _consist_args(logits, atts, refine, label_t):
    lg, (_, lsc, lsv) = _voxel_strides(logits.float(), 2)
    ref, (rsn, rsc, rsv) = _voxel_strides(refine.detach().float(), 2)
    aa = []
    asc = asv = 0
    for a in atts:
        a2, (_, asc, asv) = _voxel_strides(a.float(), 2)
        aa.append(a2)
    lt = label_t.to(device=logits.device, dtype=torch.float32).contiguous()
    return lg, lsv, lsc, ref, rsn, rsc, rsv, aa, asc, asv, lt


class _ConsistFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, refine, label_t, weight_feature, confi, *atts):
        lg, lsv, lsc, ref, rsn, rsc, rsv, aa, asc, asv, lt = _consist_args(logits, atts, refine, label_t)
        C, nt = lg.shape[1], lt.numel()
        V = lg.numel() // C
        dev = logits.device
        ptr = [a.data_ptr() for a in aa] + [None] * (3 - len(aa))
        aux = torch.empty(1, dtype=torch.float32, device=dev)
        dice = torch.empty((nt, 4), dtype=torch.float32, device=dev)
        coef = torch.empty((nt, 4, 2), dtype=torch.float32, device=dev)
        ws = ops.WS.get(_lib_query("u3d_consistency_ws_bytes", nt), dev, ops.Slot.CONSISTENCY)
        ops.call("u3d_consistency_fwd", ptr[0], ptr[1], ptr[2], len(aa), asc, asv, lg.data_ptr(), lsv, lsc, C,
                 ref.data_ptr(), rsn, rsc, rsv, lt.data_ptr(), nt, V, float(confi), float(weight_feature),
                 aux.data_ptr(), dice.data_ptr(), coef.data_ptr(), ws.data_ptr(), ops._stream())
        ctx.save_for_backward(lg, ref, lt, coef, *aa)
        ctx.geo = (lsv, lsc, C, rsn, rsc, rsv, nt, V, asc, asv, float(confi), tuple(logits.shape))
        ctx.dice = dice
        return aux.reshape(())

    @staticmethod
    def backward(ctx, g):
        lg, ref, lt, coef, *aa = ctx.saved_tensors
        lsv, lsc, C, rsn, rsc, rsv, nt, V, asc, asv, confi, shape = ctx.geo
        dev = lg.device
        go = g.reshape(1).float().contiguous()
        datt = [torch.empty(a.shape, dtype=torch.float32, device=dev) for a in aa]
        dp = [d.data_ptr() for d in datt] + [None] * (3 - len(aa))
        ap = [a.data_ptr() for a in aa] + [None] * (3 - len(aa))
        n, _, D, H, W = shape
        dl = torch.empty((n, D, H, W, C), dtype=torch.float32, device=dev)
        ops.call("u3d_consistency_bwd", ap[0], ap[1], ap[2], len(aa), asc, asv, lg.data_ptr(), lsv, lsc, C,
                 ref.data_ptr(), rsn, rsc, rsv, lt.data_ptr(), nt, V, confi, coef.data_ptr(), go.data_ptr(),
                 dp[0], dp[1], dp[2], dl.data_ptr(), ops._stream())
        return (dl.permute(0, 4, 1, 2, 3), None, None, None, None, *datt)


def _lib_query(name, *a):
    from ._lib import query
    return query(name, *a)


def consistency_aux(logits, attns, refine, label_t, weight_feature, confi=0.10):
    """aux term of get_loss's refiner branch (losses.py:158-174): one fused pass over the voxels per organ.
    As the reference enumerates ``attns + [softmax(output)[:, 1:]]``, with fewer than three attention maps the softmax
    map is map number ``len(attns)``: it takes ``weights[len(attns)]`` and a sigmoid like the attention maps."""
    ops.require_device(logits, refine, *attns)
    if logits.shape[0] != 1:
        raise IndexError("get_loss consistency: the reference indexes the maps with a [1, 1, ...] mask "
                         "(losses.py:167-169), batch must be 1")
    if len(attns) > 3:
        raise ValueError("at most 3 attention maps (unet3D_with_feam3)")
    sp = tuple(logits.shape[2:])
    for a in attns:
        if tuple(a.shape[2:]) != sp:
            raise IndexError(f"The shape of the mask {sp} does not match the shape of the indexed tensor "
                             f"{tuple(a.shape[2:])} (the reference needs deep_up=True maps, losses.py:167-169)")
    return _ConsistFn.apply(logits, refine, label_t, weight_feature, confi, *attns)


# ------------------------------------------- refiner / discriminator inputs (train_amos_atlas_final.py:277-365)
SELECT_CMAX, SELECT_KMAX = 32, 64   # csrc/atlas.hip: classes, selected organs


class _SelectProbsFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, logits, atlas, index, first):
        lg, (_, lsc, lsv) = _voxel_strides(logits.float(), 2)
        C = lg.shape[1]
        D, H, W = lg.shape[2:]
        V = D * H * W
        K, nch = len(index), 1 if atlas is None else 2
        idx = (ctypes.c_int * K)(*index)
        out = torch.empty((K, nch, D, H, W), dtype=torch.float32, device=lg.device)
        ops.call("u3d_select_probs_fwd", lg.data_ptr(), lsc, lsv, C, V, first, idx, K,
                 atlas.data_ptr() if atlas is not None else None, atlas.shape[0] if atlas is not None else 0,
                 out.data_ptr(), ops._stream())
        ctx.save_for_backward(lg)
        ctx.geo = (lsc, lsv, C, V, first, tuple(index), nch)
        return out

    @staticmethod
    def backward(ctx, g):
        (lg,) = ctx.saved_tensors
        lsc, lsv, C, V, first, index, nch = ctx.geo
        K = len(index)
        idx = (ctypes.c_int * K)(*index)
        go = g.float().contiguous()
        # the logits' own shape and strides (NCDHW, or an NCDHW view of NDHWC storage): autograd sums it with the loss
        # gradient of the same logits without a layout copy
        dl = torch.empty_strided(lg.shape, lg.stride(), dtype=torch.float32, device=lg.device)
        ops.call("u3d_select_probs_bwd", lg.data_ptr(), lsc, lsv, C, V, first, idx, K, go.data_ptr(), nch,
                 dl.data_ptr(), ops._stream())
        return dl, None, None, None


def select_probs(logits, index, atlas=None, first=0):
    """out[k, 0] = softmax(logits, 1)[0, first + index[k]] and, with an atlas [A, D, H, W], out[k, 1] = atlas[index[k]]:
    [K, 1 | 2, D, H, W] fp32, one pass (u3d_select_probs_fwd), with the gradient of channel 0 back to the logits
    (u3d_select_probs_bwd; the atlas gets none). logits [1, C, D, H, W], NCDHW or the native head's NCDHW view of
    NDHWC storage, read in place. index: ints (list, tuple, tensor), duplicates allowed, negative values count from
    the end as in tensor[index]; an empty index returns an empty tensor without a launch."""
    ops.require_device(logits, *([atlas] if atlas is not None else []))
    if logits.dim() != 5 or logits.shape[0] != 1:
        raise ValueError(f"select_probs: logits {tuple(logits.shape)} must be one sample [1, C, D, H, W]")
    C, sp = logits.shape[1], tuple(logits.shape[2:])
    if torch.is_tensor(index):
        if index.dtype == torch.bool:
            index = index.nonzero().reshape(-1)
        index = index.reshape(-1).tolist()
    n = C - first
    if atlas is not None:
        if atlas.dim() != 4 or tuple(atlas.shape[1:]) != sp:
            raise RuntimeError(f"select_probs: atlas {tuple(atlas.shape)} vs the logits' volume {sp} (torch.cat needs "
                               "equal sizes)")
        if atlas.shape[0] != n:
            raise RuntimeError(f"select_probs: {n} organ maps and {atlas.shape[0]} atlas channels (torch.cat needs "
                               "equal sizes)")
        atlas = atlas.detach().float().contiguous()
    idx = []
    for i in index:
        i = int(i)
        if not -n <= i < n:
            raise IndexError(f"index {i} is out of bounds for dimension 0 with size {n}")
        idx.append(i % n)
    if C > SELECT_CMAX or len(idx) > SELECT_KMAX or first not in (0, 1):
        from ._lib import U3DError
        raise U3DError(f"select_probs: C = {C} (at most {SELECT_CMAX}), {len(idx)} selected (at most {SELECT_KMAX}), "
                       f"first = {first} (0 or 1)")
    if not idx:
        return torch.empty((0, 1 if atlas is None else 2) + sp, dtype=torch.float32, device=logits.device)
    return _SelectProbsFn.apply(logits, atlas, tuple(idx), int(first))


class _Full2Fn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, t, m, sigmoid, uce):
        xc, tc = x.float().contiguous(), t.float().contiguous()
        mc = m.float().contiguous() if m is not None else None
        V = xc.numel()
        loss = torch.empty(1, dtype=torch.float32, device=x.device)
        coef = torch.empty(3, dtype=torch.float32, device=x.device)
        ws = ops.WS.get(128 * 4 * 8, x.device, ops.Slot.EDICE)
        ops.call("u3d_edice_full2_fwd", xc.data_ptr(), tc.data_ptr(), mc.data_ptr() if mc is not None else None, V,
                 int(sigmoid), int(uce), loss.data_ptr(), coef.data_ptr(), ws.data_ptr(), ops._stream())
        ctx.save_for_backward(xc, tc, coef, *( [mc] if mc is not None else []))
        ctx.sigmoid, ctx.has_m, ctx.shape = sigmoid, mc is not None, x.shape
        return loss.reshape(())

    @staticmethod
    def backward(ctx, g):
        xc, tc, coef, *mm = ctx.saved_tensors
        dx = torch.empty_like(xc)
        ops.call("u3d_edice_full2_bwd", xc.data_ptr(), tc.data_ptr(), mm[0].data_ptr() if mm else None, xc.numel(),
                 int(ctx.sigmoid), coef.data_ptr(), g.reshape(1).float().contiguous().data_ptr(), dx.data_ptr(),
                 ops._stream())
        return dx.reshape(ctx.shape), None, None, None, None


def edice_full2(inputs, target, uce=True, mask=None, sigmoid=True):
    ops.require_device(inputs, target)
    if inputs.numel() != target.numel() or (mask is not None and mask.numel() != target.numel()):
        raise IndexError(f"EDiceLoss_full2: inputs {tuple(inputs.shape)}, target {tuple(target.shape)}, mask "
                         f"{None if mask is None else tuple(mask.shape)} must cover the same voxels")
    return _Full2Fn.apply(inputs, target, mask, bool(sigmoid), bool(uce))
