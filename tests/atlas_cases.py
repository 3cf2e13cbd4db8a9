"""Cases, inputs and rounding bounds shared by test_atlas_reference.py (which asserts the input conditions on the CPU),
test_gpu_atlas.py (which runs the kernels of csrc/atlas.hip on them) and tests/golden/gen_golden_atlas.py (which runs
the reference on them for g19_atlas.npz). Inputs are rebuilt from seeds; the fixture holds outputs and a checksum of
the inputs. The derivation of the bounds is in test_gpu_atlas.py's docstring.
"""
import functools
import hashlib

import numpy as np
import torch

import atlas_reference as R
from atlas_reference import U
from loss_cases import SLACK, metric_bound  # noqa: F401  (the house's slack and its "metrics" line)

# the kernels' constants (csrc/atlas.hip): a change of one shows which case has to move
AT = 256                 # threads per block = voxels per block
AT_DICE_NB = 1024        # blocks per sample of dice_atlas_count_kernel at most (the other kernels do not cap their grid)
CMAX, KMAX = 32, 64
F64 = torch.float64

# ------------------------------------------------------------------------------------------------ resize-in-crop
CROP = (8, 12, 16)                  # (d, h, w) as the dataset stores them
IMAGE = (20, 30, 12)                # [H, W, D]: D is padded to crop_d + 5 = 13, offsets from the seeded draws
ATLASES = {"up": (13, 6, 10, 7),            # all axes up
           "mixed": (13, 24, 16, 40),       # down / up / down
           "eqdbl": (13, 20, 15, 12)}       # equal / double / equal
# tag -> (atlas shape, image shape, crop (d, h, w), usage, seed of the draws)
CROP_CASES = {f"{k}_{u}": (shp, IMAGE, CROP, u, 190 + i) for i, (k, shp) in enumerate(ATLASES.items())
              for u in ("train", "valid")}
# the float32 index formula floorf(i * (float)in / out) gives another source row here (in = 2, out = 82: i = 41);
# usage "valid": offsets 0, the output is the whole padded volume
CROP_CASES["f32trap_valid"] = ((2, 2, 3, 2), (82, 5, 94), CROP, "valid", 199)
NAME = "0007"                       # a CT case id: the image goes through the clip, no statistics


def case_id(case):
    return "-".join(str(a).replace("torch.", "").replace(" ", "") for a in case)


@functools.lru_cache(maxsize=None)
def crop_inputs(tag):
    """(atlas float64 [C, Ah, Aw, Ad] with values k / 64 as a probability map quantised for the fixture's size, image
    int16 [H, W, D], label uint8 [H, W, D]) as the dataset reads them."""
    ashape, ishape = CROP_CASES[tag][:2]
    g = np.random.default_rng([19, sum(ord(c) for c in tag)])
    atlas = g.integers(0, 65, ashape).astype(np.float64) / 64.0
    image = g.integers(-1100, 1400, ishape).astype(np.int16)
    label = g.integers(0, 14, ishape).astype(np.uint8)
    return atlas, image, label


def padded_shape(ishape, crop):
    cd, ch, cw = crop
    return max(ishape[0], ch + 5), max(ishape[1], cw + 5), max(ishape[2], cd + 5)


def f32_index(i, n_in, n_out):
    """What a float32 / device nearest interpolate computes: floorf(i * (float)in / out), the scale rounded to fp32."""
    scale = np.float32(n_in) / np.float32(n_out)
    return min(int(np.floor(np.float32(i) * scale)), n_in - 1)


def checksum(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


# ------------------------------------------------------------------------------------------------ atlas-gated Dice
MARGIN, MOVE = 1e-3, 4e-3
SHARE = (0.1, 0.9)
DICE_SEED = 7
# (S, C, num_class, (D, H, W))
DICE_MAIN = [(2, 14, 13, (6, 10, 12)), (1, 16, 13, (5, 7, 9)), (2, 3, 2, (4, 4, 17))]
DICE_SMALL = [(2, 3, 2, (1, 1, v)) for v in (1, 255, 257)]          # a lone voxel, one short of a block, one past it
DICE_TRIP = [(1, 3, 2, (1, 1, AT_DICE_NB * AT + 300))]              # one trip past the grid's cap, with a tail
DICE_CASES = DICE_MAIN + DICE_SMALL + DICE_TRIP
DICE_FIXTURE = DICE_MAIN + DICE_SMALL                               # what g19 records the reference's get_dice on


@functools.lru_cache(maxsize=None)
def dice_inputs(case):
    """preds [S, C, D, H, W] fp32 = randn * 2 + a per-class offset in [-1, 1], labels [S, D, H, W] class indices (with
    a label above num_class, a negative one and a non-integer where the case is long enough), atlas [S, A >= num_class,
    D, H, W] fp32 = U(0, 1) and then the condition: wherever the fp64 margin |p + 0.15 - (1 - a)| is below
    MARGIN the atlas value moves MOVE away from the threshold (the margin is re-evaluated on the stored fp32 value)."""
    S, C, ncls, sp = case
    V = sp[0] * sp[1] * sp[2]
    gen = torch.Generator().manual_seed(DICE_SEED + 1000 * C + V % 997 + S)
    off = torch.rand(C, generator=gen) * 2 - 1
    lg = torch.randn(S, V, C, generator=gen) * 2 + off
    lab = torch.randint(0, C, (S, V), generator=gen).float()
    if V >= 5:
        lab[:, 1], lab[:, 2], lab[:, 3] = float(ncls + 1), -1.0, 1.5
    A = ncls + 1 if C == 3 else ncls        # one atlas channel more than organs at C = 3: it must be ignored
    atlas = torch.rand(S, A, V, generator=gen)
    for _ in range(2):      # the move is 4 x the margin: one pass settles it, the second proves it
        m = R.gate_margin(lg, atlas, ncls)
        near = m.abs() < MARGIN
        step = torch.where(m >= 0, torch.tensor(MOVE, dtype=F64), torch.tensor(-MOVE, dtype=F64))
        a64 = atlas.double()
        a64[:, :ncls] = torch.where(near, a64[:, :ncls] + step, a64[:, :ncls])
        atlas = a64.float()
    preds = lg.permute(0, 2, 1).reshape(S, C, *sp).contiguous()
    return preds, lab.reshape(S, *sp), atlas.reshape(S, A, *sp)


def dice_flat(case):
    """(lg [S, V, C], lab [S, V], atlas [S, A, V]) views of dice_inputs for the references."""
    preds, lab, atlas = dice_inputs(case)
    S, C = preds.shape[:2]
    return preds.reshape(S, C, -1).permute(0, 2, 1).contiguous(), lab.reshape(S, -1), atlas.reshape(S, atlas.shape[1], -1)


# ------------------------------------------------------------------------------------------------ organ / atlas pairs
# (C, (D, H, W), first, with_atlas): the driver's two forms at both sizes, then the block edges
PAIR_GEOM = [(14, (6, 10, 12), 1, True), (14, (6, 10, 12), 0, False), (13, (3, 5, 6), 0, False), (13, (3, 5, 6), 1, True)] \
    + [(14, (1, 1, v), 1, True) for v in (1, 255, 257)]
LAYOUTS = ["ncdhw", "ndhwc-view"]


def pair_indices(n):
    """Index lists over n organs: one organ, all, a shuffled subset, one with a duplicate (three times the same organ
    and a pair), empty."""
    rs = np.random.RandomState(n)
    sub = [int(v) for v in rs.permutation(n)[: max(2, n // 2)]]
    return {"one": [n // 3], "all": list(range(n)), "subset": sub, "dup": [n - 1, 0, n - 1, 2 % n, n - 1, 0], "empty": []}


@functools.lru_cache(maxsize=None)
def pair_inputs(geom):
    """logits [1, C, D, H, W] fp32 (randn * 2 + per-class offset), atlas [C - first, D, H, W] fp32 U(0, 1) or None."""
    C, sp, first, with_atlas = geom
    gen = torch.Generator().manual_seed(31 * C + sp[0] * sp[1] * sp[2] + first)
    lg = torch.randn(1, C, *sp, generator=gen) * 2 + (torch.rand(C, generator=gen) * 2 - 1).reshape(1, C, 1, 1, 1)
    atlas = torch.rand(C - first, *sp, generator=gen) if with_atlas else None
    return lg, atlas


def pair_grad(K, nch, sp, seed):
    gen = torch.Generator().manual_seed(seed)
    return torch.randn(K, nch, *sp, generator=gen)


def as_layout(lg, layout, dev):
    """The logits on the device as NCDHW-contiguous or as the native head's NCDHW view of NDHWC storage."""
    if layout == "ncdhw":
        return lg.to(dev).contiguous()
    return lg.to(dev).permute(0, 2, 3, 4, 1).contiguous().permute(0, 4, 1, 2, 3)


def softmax_err(ref):
    """Relative error ep [C, V] of the kernel's p (softmax_strided: libm expf, a true division)."""
    C = ref.p.shape[0]
    ee = (ref.x.abs() + 2) * U
    es = (C - 1) * U + (ref.p * ee).sum(0, keepdim=True)
    return ee + es + 3 * U


def select_bounds(ref):
    """(bound of out[:, 0] [K, V], bound of dl [C, V] or None)."""
    ep = softmax_err(ref)
    b_out = (ref.p * ep)[ref.cls]
    if not hasattr(ref, "dl"):
        return b_out, None
    C = ref.p.shape[0]
    dG = (ref.ndup - 1).clamp(min=0)[:, None] * U * ref.G_abs
    ddot = (dG * ref.p + (ref.G * ref.p).abs() * ep).sum(0, keepdim=True) + C * U * ref.gp_abs
    return b_out, ref.dl.abs() * (ep + 2 * U) + ref.p * (dG + ddot)
