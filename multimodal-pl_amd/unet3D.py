"""Drop-in replacement for the reference ``unet3D`` module (TThuraya/multimodal-PL unet3D.py).

Same class / factory names, constructor signatures, forward signatures, return tuples and state_dict keys
(checkpoints interchange: the fp32 NCDHW parameters ARE the reference parameters). The forward of every
trunk model runs on the MI355X-native executor (u3d.trunk -> libu3d.so HIP kernels); there is no CPU
path: calling a model on CPU tensors raises U3DError.

Precision: fp32 by default (parity mode); under ``torch.autocast('cuda')`` (the reference's --FP16 path)
activations are bf16 with fp32 accumulation and fp32 master weights.
"""
import torch
import torch.nn as nn

from u3d import subgraph, trunk
from u3d._lib import U3DError

affine_par = True
in_place = True


class Conv3d(nn.Conv3d):
    """Weight-standardised Conv3d, reference unet3D.py:16-27."""

    def __init__(self, in_channels, out_channels, kernel_size, stride=(1, 1, 1), padding=(0, 0, 0),
                 dilation=(1, 1, 1), groups=1, bias=False):
        super().__init__(in_channels, out_channels, kernel_size, stride, padding, dilation, groups, bias)

    def forward(self, x):
        return _conv_module_forward(self, x, standardize=True)


def _conv_module_forward(m, x, standardize):
    k, s, p = m.kernel_size[0], m.stride[0], m.padding[0]
    if (m.kernel_size != (k, k, k) or m.stride != (s, s, s) or k not in (1, 3) or s not in (1, 2)
            or m.padding != (k // 2,) * 3 or m.groups != 1 or m.dilation != (1, 1, 1) or m.bias is not None
            or m.in_channels % 8 != 0):
        raise U3DError(f"u3d: Conv3d k={m.kernel_size} s={m.stride} p={m.padding} cin={m.in_channels} "
                       "is outside the native path")

    def build(tape, xa):
        return tape.gn_conv(xa, "c", k, s, standardize=standardize)

    return subgraph.run(build, x, [("c.weight", m.weight)], std=standardize)


def conv3x3x3(in_planes, out_planes, kernel_size=(3, 3, 3), stride=(1, 1, 1), padding=1, dilation=1, bias=False,
              weight_std=False):
    """Reference unet3D.py:30-35."""
    if weight_std:
        return Conv3d(in_planes, out_planes, kernel_size=kernel_size, stride=stride, padding=padding,
                      dilation=dilation, bias=bias)
    return nn.Conv3d(in_planes, out_planes, kernel_size=kernel_size, stride=stride, padding=padding,
                     dilation=dilation, bias=bias)


class NoBottleneck(nn.Module):
    """Pre-activation residual block, reference unet3D.py:40-73 (same submodule names)."""

    def __init__(self, inplanes, planes, stride=1, dilation=1, downsample=None, fist_dilation=1, multi_grid=1,
                 weight_std=False, group=16):
        super().__init__()
        self.weight_std = weight_std
        self.gn1 = nn.GroupNorm(group, inplanes)
        self.conv1 = conv3x3x3(inplanes, planes, kernel_size=(3, 3, 3), stride=stride, padding=(1, 1, 1),
                               dilation=dilation * multi_grid, bias=False, weight_std=self.weight_std)
        self.relu = nn.ReLU(inplace=in_place)
        self.gn2 = nn.GroupNorm(group, planes)
        self.conv2 = conv3x3x3(planes, planes, kernel_size=(3, 3, 3), stride=1, padding=(1, 1, 1),
                               dilation=dilation * multi_grid, bias=False, weight_std=self.weight_std)
        self.downsample = downsample
        self.dilation = dilation
        self.stride = stride
        self.group = group

    def forward(self, x):
        s = self.stride if isinstance(self.stride, int) else self.stride[0]
        G = self.group

        def build(tape, xa):
            return tape.block(xa, "", s, G)

        return subgraph.run(build, x, list(self.named_parameters()), std=self.weight_std)


def _make_layer(model, block, inplanes, planes, blocks, stride=(1, 1, 1), dilation=1, multi_grid=1, group=16,
                ds_group=16):
    """Shared _make_layer (reference :1666-1686 / :1538-1564)."""
    downsample = None
    if stride[0] != 1 or stride[1] != 1 or stride[2] != 1 or inplanes != planes:
        downsample = nn.Sequential(
            nn.GroupNorm(ds_group, inplanes),
            nn.ReLU(inplace=in_place),
            conv3x3x3(inplanes, planes, kernel_size=(1, 1, 1), stride=stride, padding=0, weight_std=model.weight_std),
        )
    layers = []
    gm = lambda index, grids: grids[index % len(grids)] if isinstance(grids, tuple) else 1  # noqa: E731
    layers.append(block(inplanes, planes, stride, dilation=dilation, downsample=downsample,
                        multi_grid=gm(0, multi_grid), weight_std=model.weight_std, group=group))
    for i in range(1, blocks):
        layers.append(block(planes, planes, dilation=dilation, multi_grid=gm(i, multi_grid),
                            weight_std=model.weight_std, group=group))
    return nn.Sequential(*layers)


def _head(groups, cin, ncls):
    return nn.Sequential(nn.GroupNorm(groups, cin), nn.ReLU(inplace=in_place), nn.Conv3d(cin, ncls, kernel_size=1))


class _TrunkMixin:
    """Builds the conv1 / layer0-4 / fusionConv / decoder / precls_conv modules with reference names."""

    def _build_trunk(self, in_channel, f, layers, group, fusion_group, head_group, ncls, conv0=False, up48=False,
                     deep=False, eams=0, linears=0):
        """Every trunk class's modules in the reference's registration (and construction) order. What a class has
        after x8 / x4 / x2_resb: a deep-supervision head deepout{1,2,3} (``deep``), an EAM (the first ``eams`` levels),
        the Linear that hands the class message down a level (the first ``linears``). ``up48``: the x4 / x8 upsamplers
        of deep_up, registered before the decoder (:964-965)."""
        if conv0:
            self.conv0 = conv3x3x3(in_channel, f, stride=[2, 2, 2], weight_std=self.weight_std)
            self.conv1 = conv3x3x3(f, f, stride=[1, 1, 1], weight_std=self.weight_std)
        else:
            self.conv1 = conv3x3x3(in_channel, f, stride=[1, 1, 1], weight_std=self.weight_std)
        mk = lambda cin, cout, n, s: _make_layer(self, NoBottleneck, cin, cout, n, stride=s, group=group,  # noqa
                                                 ds_group=group)
        self.layer0 = mk(f, f, layers[0], (1, 1, 1))
        self.layer1 = mk(f, 2 * f, layers[1], (2, 2, 2))
        self.layer2 = mk(2 * f, 4 * f, layers[2], (2, 2, 2))
        self.layer3 = mk(4 * f, 8 * f, layers[3], (2, 2, 2))
        self.layer4 = mk(8 * f, 8 * f, layers[4], (2, 2, 2))
        self.fusionConv = nn.Sequential(
            nn.GroupNorm(fusion_group, 8 * f),
            nn.ReLU(inplace=in_place),
            conv3x3x3(8 * f, 8 * f, kernel_size=(1, 1, 1), padding=(0, 0, 0), weight_std=self.weight_std),
        )
        self.upsamplex2 = nn.Upsample(scale_factor=2, mode="trilinear")
        if up48:
            self.upsamplex3 = nn.Upsample(scale_factor=4, mode="trilinear")
            self.upsamplex4 = nn.Upsample(scale_factor=8, mode="trilinear")
        for k, (name, cin, cout) in enumerate((("x8_resb", 8 * f, 4 * f), ("x4_resb", 4 * f, 2 * f),
                                               ("x2_resb", 2 * f, f))):
            setattr(self, name, mk(cin, cout, 1, (1, 1, 1)))
            if deep:
                setattr(self, f"deepout{k + 1}", _head(16, cout, ncls))
            if k < eams:
                setattr(self, ("eam84", "eam42", "eam21")[k], EAM(cout, input_resolution=None, num_heads=4))
            if k < linears:
                setattr(self, ("linear84_2_42", "linear42_2_21")[k], nn.Linear(cout, cout // 2))
        self.x1_resb = mk(f, f, 1, (1, 1, 1))
        self.precls_conv = _head(head_group, f, ncls)
        self._u3d_cfg = trunk.TrunkCfg(layers=tuple(layers), groups=group, fusion_groups=fusion_group,
                                       head_groups=head_group, conv0=conv0, final_up=conv0,
                                       weight_std=bool(self.weight_std))

    def _ema_detach(self, ema):
        if ema:
            for param in self.parameters():
                param.detach_()

    def _tokens_to(self, dev):
        """The three class tokens, moved to ``dev`` where they are plain tensors."""
        self.class_token1 = self.class_token1.to(dev)
        self.class_token2 = self.class_token2.to(dev)
        self.class_token3 = self.class_token3.to(dev)
        return [self.class_token1, self.class_token2, self.class_token3]

    def _trunk_params(self):
        return [(n, p) for n, p in self.named_parameters()
                if not n.startswith(("GAP.", "controller."))]

    def _run(self, x):
        return trunk.run_trunk(self._u3d_cfg, x, self._trunk_params(), getattr(self, "compute_dtype", None))


class unet3D_baseline(_TrunkMixin, nn.Module):
    """Reference unet3D.py:584-718. forward(input, mask=None) -> train: (logits, [], []); eval: logits."""

    def __init__(self, layers, num_classes=12, weight_std=False, ema=False, use_cm=[True, True, True],  # noqa: B006
                 deep_up=False):
        super().__init__()
        self.inplanes = 128
        self.weight_std = weight_std
        self.num_classes = num_classes
        self.use_cm = use_cm
        self.alpha = 0.01
        self.deep_up = deep_up
        self._build_trunk(1, 32, layers, 16, 16, 16, num_classes)
        self.upsamplex3 = nn.Upsample(scale_factor=4, mode="trilinear")
        self.upsamplex4 = nn.Upsample(scale_factor=8, mode="trilinear")
        self._ema_detach(ema)

    def forward(self, input, mask=None):
        logits = self._run(input)
        if self.training:
            return logits, [], []
        return logits


class unet3D_g(_TrunkMixin, nn.Module):
    """Reference unet3D.py:1507-1623 (the refiner / light variant): stride-2 conv0, GN(4) blocks,
    GN(init/2) fusion, GN(init/4) head, final x2 upsample of the logits."""

    def __init__(self, layers, num_classes=3, weight_std=False, in_channel=2, init_filter=32):
        super().__init__()
        self.inplanes = 128
        self.weight_std = weight_std
        self.init_filter = init_filter
        self._build_trunk(in_channel, init_filter, layers, 4, init_filter // 2, init_filter // 4, num_classes,
                          conv0=True)

    def forward(self, input, _=None):
        return self._run(input)


class unet3D(_TrunkMixin, nn.Module):
    """Reference unet3D.py:1625-1806: trunk + DynConv 8,8,2 head conditioned on the task id."""

    def __init__(self, layers, num_classes=3, weight_std=False, in_channel=1, init_filter=32):
        super().__init__()
        self.inplanes = 128
        self.weight_std = weight_std
        self.init_filter = init_filter
        self._build_trunk(in_channel, init_filter, layers, 16, 16, 16, 8)
        self.GAP = nn.Sequential(nn.GroupNorm(16, 256), nn.ReLU(inplace=in_place), torch.nn.AdaptiveAvgPool3d((1, 1, 1)))
        self.controller = nn.Conv3d(256 + 7, 162, kernel_size=1, stride=1, padding=0)

    def forward(self, input, task_id):
        from u3d import dynhead
        return dynhead.run_unet3d(self, input, task_id)


def UNet3D(num_classes=1, weight_std=False):
    """Reference factory unet3D.py:1808-1811."""
    print("Using DynConv 8,8,2")
    return unet3D([1, 2, 2, 2, 2], num_classes, weight_std)


def _next_row(name, row):
    def ctor(*a, **k):
        raise NotImplementedError(f"{name}: method-specific head, SURVEY.md §8(f) row {row} — not built in this round")
    ctor.__name__ = name
    return ctor


class EAM(nn.Module):
    """Reference unet3D.py:142-212 (same parameters: kv, q, proj, norm2, norm3). Inside unet3D_with_feam3 / _feam2 /
    _feam its attention map runs natively (u3d.feam.eam_op: only ``attn`` is used there, :1134), inside
    unet3D_with_eam / _eam_baseline the whole module does (u3d.feam.eam_pool_op); called on its own it raises."""

    def __init__(self, dim, input_resolution, num_heads, mlp_ratio=4., qkv_bias=True, qk_scale=None, drop=0.,
                 attn_drop=0., drop_path=0., norm_layer=nn.LayerNorm, upsample=None, use_checkpoint=False):
        super().__init__()
        self.dim = dim
        self.input_resolution = input_resolution
        self.use_checkpoint = use_checkpoint
        self.num_heads = num_heads
        head_dim = dim // num_heads
        self.scale = qk_scale or head_dim ** -0.5
        self.kv = nn.Linear(dim, dim * 2, bias=False)
        self.q = nn.Linear(dim, dim, bias=False)
        self.softmax = nn.Softmax(dim=-1)
        self.proj = nn.Linear(dim, dim)
        self.norm2 = norm_layer(dim)
        self.norm3 = norm_layer(dim)

    def forward(self, x, modality_token):
        raise U3DError("EAM: the native path runs it inside unet3D_with_feam3 (u3d.feam); standalone use is not "
                       "on the hot path")


class unet3D_with_feam3(_TrunkMixin, nn.Module):
    """Reference unet3D.py:938-1190 (the model train_amos_atlas_final.py:118 trains): the trunk + deep-supervision
    heads deepout1-3 + EAM attention maps against EMA class tokens. forward(input, mask=None) -> train:
    (logits, atten_map[<=3], deep_map[3], feature_stored[3]); eval: logits. Batch 1 when use_cm (the reference's
    EAM reshapes with the token's batch of 1 and raises otherwise)."""

    def __init__(self, layers, num_classes=12, weight_std=False, ema=False, use_cm=[True, True, True],  # noqa: B006
                 deep_up=False):
        self.inplanes = 128
        self.weight_std = weight_std
        self.num_classes = num_classes
        self.use_cm = use_cm
        self.alpha = 0.01
        self.deep_up = deep_up
        super().__init__()
        self._build_trunk(1, 32, layers, 16, 16, 16, num_classes, up48=True, deep=True, eams=3)
        # class tokens: plain tensors (not parameters / buffers, so not in the state_dict), :1016-1021
        self.class_token1 = torch.randn(num_classes - 1, 128)
        self.class_token2 = torch.randn(num_classes - 1, 64)
        self.class_token3 = torch.randn(num_classes - 1, 32)
        self._ema_detach(ema)

    def renew_token(self, features, mask):
        """EMA update of the class tokens from the stored features (:1051-1068), on the device."""
        from u3d import feam
        feam.renew_token(self._tokens_to(mask.device), features, mask, self.num_classes, self.alpha)

    def _levels(self, tokens, renew=None):
        """Per decoder level: the deep head, the stored feature, the map where use_cm (full size if deep_up)."""
        from u3d import feam
        return [feam.Level(deep=True, store=True, renew=renew, token=tokens[k], attend=bool(self.use_cm[k]),
                           up=feam.UP_SCALE[k] if self.deep_up else 1) for k in range(3)]

    def forward(self, input, mask=None):
        from u3d import feam
        return feam.run_feam3(self, input, self._levels(self._tokens_to(input.device)))


class unet3D_with_feam2(unet3D_with_feam3):
    """Reference unet3D.py:721-936 — the model evaluate_amos.py:571 builds. Same modules as unet3D_with_feam3; the
    class tokens are nn.Parameters (in the state_dict, registered last, :788-793) updated INSIDE forward in train
    mode (each level before its attention). forward(input, mask=None) -> train: (logits, atten_map, deep_map);
    eval: logits. As in the reference, a train-mode forward with a mask updates the tokens in place, which
    autograd refuses while they require grad (it works with ema=True), and mask=None fails at ``(mask == l+1)``."""

    def __init__(self, layers, num_classes=12, weight_std=False, ema=False, use_cm=[True, True, True],  # noqa: B006
                 deep_up=False):
        super().__init__(layers, num_classes, weight_std, False, use_cm, deep_up)
        self.class_token1 = nn.Parameter(torch.randn(num_classes - 1, 128))
        self.class_token2 = nn.Parameter(torch.randn(num_classes - 1, 64))
        self.class_token3 = nn.Parameter(torch.randn(num_classes - 1, 32))
        self._ema_detach(ema)

    def forward(self, input, mask=None):
        from u3d import feam
        if self.training and mask is None:
            raise AttributeError("'bool' object has no attribute 'sum'")  # (None == l+1).sum(), unet3D.py:870
        tokens = [self.class_token1, self.class_token2, self.class_token3]
        outs = feam.run_feam3(self, input, self._levels(tokens, (mask, self.num_classes, self.alpha)))
        return outs[:3] if self.training else outs


class unet3D_with_deepsup(_TrunkMixin, nn.Module):
    """Reference unet3D.py:280-429: the trunk + the three deep-supervision heads deepout1-3 (GN(16), ReLU, 1^3 conv +
    bias on the x8 / x4 / x2 decoder features), no EAM and no class tokens. forward(input, ids) -> train: (logits,
    [deep x8, deep x4, deep x2]); eval: logits (the heads are not run). ``ids`` is unused, as in the reference; any
    batch size. The deep maps are trained by losses.get_loss(..., deep_out=...) / u3d.loss.deep_supervision_loss."""

    def __init__(self, layers, num_classes=12, weight_std=False, ema=False, use_cm=[True, True, True]):  # noqa: B006
        self.inplanes = 128
        self.weight_std = weight_std
        self.num_classes = num_classes
        self.use_cm = use_cm
        super().__init__()
        self._build_trunk(1, 32, layers, 16, 16, 16, num_classes, deep=True)
        self._ema_detach(ema)

    def forward(self, input, ids=None):
        from u3d import feam
        outs = feam.run_feam3(self, input, [feam.Level(deep=True)] * 3)
        return (outs[0], outs[2]) if self.training else outs


def _cascade(use_cm, n):
    """The reference's cumulative tests: level k runs when use_cm[0] .. use_cm[k] all hold (unet3D.py:536, 551, 563)."""
    return [all(bool(u) for u in use_cm[:k + 1]) for k in range(n)]


class unet3D_with_eam(_TrunkMixin, nn.Module):
    """Reference unet3D.py:431-582 (the model evaluate_amos.py:574 builds): the trunk + a cascade of whole EAMs. The
    class token [num_classes, 128] is a Parameter and is not detached; each level's class message cm goes through a
    Linear and is the next level's token. forward(input, task_id) -> train: (logits, cm [1, num_classes, C of the last
    level run], atten_map); eval: logits (the EAMs are not run). Batch 1, as the reference's EAM reshape demands;
    with use_cm[0] false a train forward fails as the reference's does, on the cm it never made."""
    EAMS = 3   # eam84 -> linear84_2_42 -> eam42 -> linear42_2_21 -> eam21 (:439-475)

    def __init__(self, layers, num_classes=12, weight_std=False, ema=False, use_cm=[True, True, True]):  # noqa: B006
        self.inplanes = 128
        self.weight_std = weight_std
        self.num_classes = num_classes
        self.use_cm = use_cm
        super().__init__()
        self._build_trunk(1, 32, layers, 16, 16, 16, num_classes, eams=self.EAMS, linears=self.EAMS - 1)
        self.class_token = nn.Parameter(torch.randn(num_classes, 128))
        self._ema_detach(ema)

    def _gates(self):
        return _cascade(self.use_cm, 3)

    def forward(self, input, task_id=None):
        from u3d import feam
        gates = self._gates()
        if self.training and not gates[0]:
            feam.ops.require_device(input)
            raise UnboundLocalError("local variable 'cm' referenced before assignment")  # unet3D.py:580
        return feam.run_eam(self, input, gates)


class unet3D_with_eam_baseline(unet3D_with_eam):
    """Reference unet3D.py:1370-1504: two EAM levels (eam84 -> linear84_2_42 -> eam42), always on; cm is eam42's."""
    EAMS = 2

    def __init__(self, layers, num_classes=12, weight_std=False):
        super().__init__(layers, num_classes, weight_std)

    def _gates(self):
        return [True, True]


class unet3D_with_feam(_TrunkMixin, nn.Module):
    """Reference unet3D.py:1193-1367: the trunk + EAM attention maps against Parameter class tokens that a train
    forward renews from the labelled voxels (13 classes, factor 0.01) before each level's attention; no deep heads.
    forward(input, mask=None) -> train: (logits, atten_map); eval: logits. The maps exist only in training, under the
    reference's cumulative use_cm tests. As there, a label that reaches a level while the tokens require grad is an
    in-place write autograd refuses (it works with ema=True, or with a mask that holds no label), and mask=None fails
    at ``(mask == l+1)``."""
    RENEW_CLASSES, ALPHA = 13, 0.01

    def __init__(self, layers, num_classes=12, weight_std=False, ema=False, use_cm=[True, True, True]):  # noqa: B006
        self.inplanes = 128
        self.weight_std = weight_std
        self.num_classes = num_classes
        self.use_cm = use_cm
        self.deep_up = False
        super().__init__()
        self._build_trunk(1, 32, layers, 16, 16, 16, num_classes, eams=3)
        self.class_token1 = nn.Parameter(torch.randn(num_classes - 1, 128))
        self.class_token2 = nn.Parameter(torch.randn(num_classes - 1, 64))
        self.class_token3 = nn.Parameter(torch.randn(num_classes - 1, 32))
        self._ema_detach(ema)

    def forward(self, input, mask=None):
        from u3d import feam
        feam.ops.require_device(input)
        renew = None
        if self.training:
            if mask is None:
                raise AttributeError("'bool' object has no attribute 'sum'")  # (None == l+1).sum(), unet3D.py:1302
            feam.ops.require_device(mask)
            renew = (mask, self.RENEW_CLASSES, self.ALPHA)
            if trunk.wants_grad(self.parameters()):
                sizes = [tuple(s // f for s in input.shape[2:]) for f in (8, 4, 2)]
                if feam.labels_reach(mask, sizes, self.RENEW_CLASSES):
                    raise RuntimeError("a leaf Variable that requires grad is being used in an in-place operation.")
                renew = None   # no label reaches a level: the renewal writes nothing
        tokens = [self.class_token1, self.class_token2, self.class_token3]
        levels = [feam.Level(renew=renew, token=t, attend=g) for t, g in zip(tokens, _cascade(self.use_cm, 3))]
        outs = feam.run_feam3(self, input, levels)
        return outs[:2] if self.training else outs


# get_style_discriminator (a (2, 3, 2) conv) is not built by the driver: SURVEY.md §2, out of scope.
get_style_discriminator = _next_row("get_style_discriminator", "out-of-scope")


class Reshape(nn.Module):
    """Reference unet3D.py:1825-1830."""

    def forward(self, x):
        return x.view(x.shape[0], -1)


def _lrelu():
    return nn.LeakyReLU(negative_slope=0.2, inplace=True)


def _disc_conv(cin, cout):
    return nn.Conv3d(cin, cout, kernel_size=4, stride=2, padding=1)


def _disc_tail(cin, ndf, out_features):
    """block4 of the two discriminator classes / the back of get_style_discriminator_output: three 4^3 stride-2 convs,
    pool, reshape, linear (reference unet3D.py:1879-1889), at the reference's Sequential indices."""
    return [_disc_conv(cin, ndf * 8), _lrelu(), _disc_conv(ndf * 8, ndf * 8), _lrelu(), _disc_conv(ndf * 8, ndf * 8),
            _lrelu(), nn.AdaptiveAvgPool3d(1), Reshape(), nn.Linear(ndf * 8, out_features)]


def _wb(conv):
    return conv.weight, conv.bias


class _StyleDiscriminatorOutput(nn.Sequential):
    """What get_style_discriminator_output returns (reference unet3D.py:1832-1849): the reference's nn.Sequential, same
    indices and state_dict keys, with the forward on the native kernels (u3d.disc)."""

    def __init__(self, num_classes, ndf):
        from u3d import disc
        disc.check_config(num_classes, ndf)
        super().__init__(_disc_conv(num_classes, ndf), _lrelu(), _disc_conv(ndf, ndf * 2), _lrelu(),
                         _disc_conv(ndf * 2, ndf * 4), _lrelu(), *_disc_tail(ndf * 4, ndf, 1))
        self.num_classes, self.ndf = num_classes, ndf

    def forward(self, x_in):
        from u3d import disc
        feat = disc.run_chain(x_in, None, [_wb(self[i]) for i in (0, 2, 4, 6, 8, 10)], None, self.num_classes, self.ndf)
        return disc.pool_linear(feat, self[14].weight, self[14].bias)


def get_style_discriminator_output(num_classes, ndf=32):
    """Reference unet3D.py:1832-1849. forward(x_in [B, num_classes, D, H, W]) -> [B, 1]."""
    return _StyleDiscriminatorOutput(num_classes, ndf)


class deep_style_discriminator_output(nn.Module):
    """Reference unet3D.py:1852-1905 (train_amos_atlas_final.py:124): forward(x_in, f_m) -> [B, 2]; f_m[2] / f_m[1] /
    f_m[0] are one-channel maps at block1's / block2's / block3's output resolution. The side convs write the upper
    channel half of the buffer the next block reads: the reference's torch.cat is never materialised."""

    def __init__(self, num_classes, ndf=32):
        from u3d import disc
        disc.check_config(num_classes, ndf)
        super().__init__()
        self.ndf = ndf
        self._num_classes = num_classes
        self.block1 = nn.Sequential(_disc_conv(num_classes, ndf), _lrelu())
        self.min_block1 = nn.Sequential(nn.Conv3d(1, ndf, kernel_size=3, stride=1, padding=1), _lrelu())
        self.block2 = nn.Sequential(_disc_conv(ndf * 2, ndf * 2), _lrelu())
        self.min_block2 = nn.Sequential(nn.Conv3d(1, ndf * 2, kernel_size=3, stride=1, padding=1), _lrelu())
        self.block3 = nn.Sequential(_disc_conv(ndf * 4, ndf * 4), _lrelu())
        self.min_block3 = nn.Sequential(nn.Conv3d(1, ndf * 4, kernel_size=3, stride=1, padding=1), _lrelu())
        self.block4 = nn.Sequential(*_disc_tail(ndf * 8, ndf, 2))

    def forward(self, x_in, f_m):
        from u3d import disc
        b4 = self.block4
        convs = [_wb(self.block1[0]), _wb(self.block2[0]), _wb(self.block3[0]), _wb(b4[0]), _wb(b4[2]), _wb(b4[4])]
        sides = [_wb(self.min_block1[0]), _wb(self.min_block2[0]), _wb(self.min_block3[0])]
        feat = disc.run_chain(x_in, f_m, convs, sides, self._num_classes, self.ndf)
        return disc.pool_linear(feat, b4[8].weight, b4[8].bias)


class norm_style_discriminator_output(nn.Module):
    """Reference unet3D.py:1907-1947 (train_amos_atlas_final.py:126): forward(x_in) -> [B, 2]."""

    def __init__(self, num_classes, ndf=32):
        from u3d import disc
        disc.check_config(num_classes, ndf)
        super().__init__()
        self.ndf = ndf
        self._num_classes = num_classes
        self.block1 = nn.Sequential(_disc_conv(num_classes, ndf), _lrelu())
        self.block2 = nn.Sequential(_disc_conv(ndf, ndf * 2), _lrelu())
        self.block3 = nn.Sequential(_disc_conv(ndf * 2, ndf * 4), _lrelu())
        self.block4 = nn.Sequential(*_disc_tail(ndf * 4, ndf, 2))

    def forward(self, x_in):
        from u3d import disc
        b4 = self.block4
        convs = [_wb(self.block1[0]), _wb(self.block2[0]), _wb(self.block3[0]), _wb(b4[0]), _wb(b4[2]), _wb(b4[4])]
        feat = disc.run_chain(x_in, None, convs, None, self._num_classes, self.ndf)
        return disc.pool_linear(feat, b4[8].weight, b4[8].bias)
