"""Plain-torch restatement of the style discriminators' layer ops and of the three modules, written here in the manner
of tests/gn_reference.py: the yardstick of the kernel tests (in fp64 on the CPU) and of the bf16 model test (on the GPU
under autocast). Pinned to the G17 fixtures by tests/test_disc_reference.py.

Layer ops (x NCDHW):
  conv4   4^3 / stride 2 / pad 1 conv + bias + LeakyReLU(0.2)
  side3   3^3 / stride 1 / pad 1 conv (1 -> C) + bias + LeakyReLU(0.2)
and the two identities the kernels are built on:
  conv4_s2d      the 4^3 / s2 / p1 conv as a 2^3-tap stride-1 conv over the space-to-depth(2) view of the padded input:
                 out[o] = sum_{a, b in {0, 1}} w[2a + b] xp[2 (o + a) + b] per dimension
  dgrad_parity   its data gradient as 8 parity classes, each a dense 2^3-tap conv over dy: even inputs x = 2q take
                 taps 1 and 3 from o = q and o = q - 1, odd inputs x = 2q + 1 taps 0 and 2 from o = q + 1 and o = q
"""
import itertools

import torch
import torch.nn.functional as F

SLOPE = 0.2


def conv4(x, w, b, act=True):
    y = F.conv3d(x, w, b, stride=2, padding=1)
    return F.leaky_relu(y, SLOPE) if act else y


def side3(f, w, b, act=True):
    y = F.conv3d(f, w, b, stride=1, padding=1)
    return F.leaky_relu(y, SLOPE) if act else y


def lrelu_grad(dy, y):
    """dy * lrelu'(pre) from the stored post-activation output: sign(y) = sign(pre) because the slope is positive."""
    return dy * torch.where(y > 0, torch.ones_like(y), torch.full_like(y, SLOPE))


def conv4_s2d(x, w):
    """The stride-2 conv (no bias, no activation) by the space-to-depth identity."""
    n, c, d, h, wd = x.shape
    do, ho, wo = d // 2, h // 2, wd // 2
    xp = F.pad(x, (1, 1, 1, 1, 1, 1))
    xp = xp[:, :, :2 * (do + 1), :2 * (ho + 1), :2 * (wo + 1)]
    # s2d: [n, c, do + 1, 2, ho + 1, 2, wo + 1, 2] -> channels (c, bd, bh, bw)
    v = xp.reshape(n, c, do + 1, 2, ho + 1, 2, wo + 1, 2).permute(0, 1, 3, 5, 7, 2, 4, 6)
    v = v.reshape(n, c * 8, do + 1, ho + 1, wo + 1)
    # w[co, ci, 2 ad + bd, 2 ah + bh, 2 aw + bw] -> [co, (ci, bd, bh, bw), ad, ah, aw]
    co = w.shape[0]
    w2 = w.reshape(co, c, 2, 2, 2, 2, 2, 2).permute(0, 1, 3, 5, 7, 2, 4, 6).reshape(co, c * 8, 2, 2, 2)
    return F.conv3d(v, w2)


def dgrad_parity(g, w, in_dims):
    """Data gradient of the stride-2 conv from g = d loss / d (pre-activation) [n, co, do, ho, wo], by parity classes."""
    n, co = g.shape[:2]
    ci = w.shape[1]
    odims = g.shape[2:]
    dx = g.new_zeros((n, ci) + tuple(in_dims))
    gp = F.pad(g, (1, 1, 1, 1, 1, 1))  # index o + 1
    for par in itertools.product((0, 1), repeat=3):
        q = [(in_dims[a] - par[a] + 1) // 2 for a in range(3)]  # number of inputs x = 2 q + p < in_dims
        if min(q) <= 0:
            continue
        acc = g.new_zeros((n, ci, *q))
        for t in itertools.product((0, 1), repeat=3):
            k = [(2 - 2 * t[a]) if par[a] else (1 + 2 * t[a]) for a in range(3)]
            off = [t[a] if par[a] else -t[a] for a in range(3)]  # o = q + off
            sl = []
            for a in range(3):
                # o ranges over off .. off + q - 1; rows beyond the padded extent are out of the output: zeros
                lo = off[a] + 1
                idx = torch.arange(lo, lo + q[a])
                idx = torch.where(idx <= odims[a] + 1, idx, torch.zeros_like(idx))  # 0 = a padding row
                sl.append(idx)
            gs = gp[:, :, sl[0]][:, :, :, sl[1]][:, :, :, :, sl[2]]
            acc = acc + torch.einsum("nodhw,oi->nidhw", gs, w[:, :, k[0], k[1], k[2]])
        dx[:, :, par[0]::2, par[1]::2, par[2]::2] = acc
    return dx


# ------------------------------------------------------------------------------------------ the three modules
class _Base(torch.nn.Module):
    """Parameters at the reference's state_dict keys (Sequential indices), so tests/disc_cases.fill and a reference
    checkpoint load into it."""

    def _tail(self, cin, ndf, out_features):
        nn = torch.nn
        return nn.Sequential(nn.Conv3d(cin, ndf * 8, 4, 2, 1), nn.Identity(), nn.Conv3d(ndf * 8, ndf * 8, 4, 2, 1),
                             nn.Identity(), nn.Conv3d(ndf * 8, ndf * 8, 4, 2, 1), nn.Identity(), nn.Identity(),
                             nn.Identity(), nn.Linear(ndf * 8, out_features))

    @staticmethod
    def _c4(m, x):
        return conv4(x, m.weight, m.bias)

    @staticmethod
    def _run_tail(t, x):
        for i in (0, 2, 4):
            x = conv4(x, t[i].weight, t[i].bias)
        return F.linear(x.mean(dim=(2, 3, 4)), t[8].weight, t[8].bias)


class NormDisc(_Base):
    def __init__(self, num_classes, ndf=32):
        super().__init__()
        nn = torch.nn
        self.block1 = nn.Sequential(nn.Conv3d(num_classes, ndf, 4, 2, 1))
        self.block2 = nn.Sequential(nn.Conv3d(ndf, ndf * 2, 4, 2, 1))
        self.block3 = nn.Sequential(nn.Conv3d(ndf * 2, ndf * 4, 4, 2, 1))
        self.block4 = self._tail(ndf * 4, ndf, 2)

    def forward(self, x):
        for b in (self.block1, self.block2, self.block3):
            x = self._c4(b[0], x)
        return self._run_tail(self.block4, x)


class DeepDisc(_Base):
    def __init__(self, num_classes, ndf=32):
        super().__init__()
        nn = torch.nn
        self.block1 = nn.Sequential(nn.Conv3d(num_classes, ndf, 4, 2, 1))
        self.min_block1 = nn.Sequential(nn.Conv3d(1, ndf, 3, 1, 1))
        self.block2 = nn.Sequential(nn.Conv3d(ndf * 2, ndf * 2, 4, 2, 1))
        self.min_block2 = nn.Sequential(nn.Conv3d(1, ndf * 2, 3, 1, 1))
        self.block3 = nn.Sequential(nn.Conv3d(ndf * 4, ndf * 4, 4, 2, 1))
        self.min_block3 = nn.Sequential(nn.Conv3d(1, ndf * 4, 3, 1, 1))
        self.block4 = self._tail(ndf * 8, ndf, 2)

    def forward(self, x, f_m):
        x = self._c4(self.block1[0], x)
        x = torch.cat([x, side3(f_m[2], self.min_block1[0].weight, self.min_block1[0].bias)], 1)
        x = self._c4(self.block2[0], x)
        x = torch.cat([x, side3(f_m[1], self.min_block2[0].weight, self.min_block2[0].bias)], 1)
        x = self._c4(self.block3[0], x)
        x = torch.cat([x, side3(f_m[0], self.min_block3[0].weight, self.min_block3[0].bias)], 1)
        return self._run_tail(self.block4, x)


class SeqDisc(torch.nn.Sequential):
    def __init__(self, num_classes, ndf=32):
        nn = torch.nn
        chans = [num_classes, ndf, ndf * 2, ndf * 4, ndf * 8, ndf * 8, ndf * 8]
        mods = []
        for i in range(6):
            mods += [nn.Conv3d(chans[i], chans[i + 1], 4, 2, 1), nn.Identity()]
        super().__init__(*mods, nn.Identity(), nn.Identity(), nn.Linear(ndf * 8, 1))

    def forward(self, x):
        for i in range(0, 12, 2):
            x = conv4(x, self[i].weight, self[i].bias)
        return F.linear(x.mean(dim=(2, 3, 4)), self[14].weight, self[14].bias)


KINDS = {"norm": NormDisc, "deep": DeepDisc, "seq": SeqDisc}
