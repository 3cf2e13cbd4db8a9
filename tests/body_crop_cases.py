"""Cases and inputs shared by test_body_crop_reference.py (host), test_ccl_core_host.py (the sanitised core program),
test_gpu_ccl.py / test_gpu_body_crop.py (csrc/ccl.hip, u3d.data) and tests/golden/gen_golden_body_crop.py (the
reference's own lines, g21_body_crop.npz). Inputs are rebuilt from seeds; the fixture holds outputs and a checksum of
the inputs.
"""
import functools
import hashlib

import numpy as np

# the labelling tile of csrc/ccl_core.h (z, y, x); the GPU tests assert it against u3d_ccl_tile
TILE = (8, 8, 64)


def checksum(*arrays):
    h = hashlib.sha256()
    for a in arrays:
        h.update(np.ascontiguousarray(a).tobytes())
    return h.hexdigest()


# ------------------------------------------------------------------------------------------------ labelling shapes
def label_shapes(T=TILE):
    tz, ty, tx = T
    shapes = [(1, 1, 257), (5, 7, 300), (17, 33, 70)]
    for t in (tz - 1, tz, tz + 1, 2 * tz + 1):
        shapes.append((t, 5, 9))
    for t in (ty - 1, ty, ty + 1, 2 * ty + 1):
        shapes.append((3, t, 9))
    for t in (tx - 1, tx, tx + 1, 2 * tx + 1):
        shapes.append((3, 5, t))
    shapes.append((2 * tz + 3, 2 * ty + 2, 2 * tx + 5))      # three tiles on every axis, 49 K voxels at (8, 8, 64)
    return shapes


BERNOULLI_P = (0.05, 0.2, 0.31, 0.5, 0.8)
PATTERNS = ("zeros", "ones") + tuple(f"bernoulli{p}" for p in BERNOULLI_P) + (
    "serpentine", "comb", "checkerboard", "edge", "corner")
# p = 0.31, near the cubic lattice's percolation threshold: about 11 000 components, the largest beyond 1 000 voxels
PERCOLATION_SHAPE = (40, 70, 70)


def serpentine(shape):
    """One path (n == 1): even planes hold full x rows at even y, joined at alternating ends by one voxel at odd y;
    consecutive even planes are joined by one voxel in the odd plane between, where the path ends. The path crosses
    every tile seam in both directions."""
    Z, Y, X = shape
    m = np.zeros(shape, dtype=np.uint8)
    side = 0                                             # the x end at which the path stands
    for k, z in enumerate(range(0, Z, 2)):
        ys = list(range(0, Y, 2))
        if k % 2:
            ys.reverse()
        for j, y in enumerate(ys):
            m[z, y, :] = 1
            side = X - 1 - side
            if j + 1 < len(ys):
                m[z, (y + ys[j + 1]) // 2, side] = 1
        if z + 2 < Z:
            m[z + 1, ys[-1], side] = 1
    return m


def comb(shape):
    """Teeth along x at (z of the last plane's parity, even y); they join only in the last x column (along z) and, in
    the last plane, along y in that column: every union that merges two teeth arrives at the end of the rows, and the
    root has to travel back to the first voxel. n == 1."""
    Z, Y, X = shape
    m = np.zeros(shape, dtype=np.uint8)
    m[(Z - 1) % 2::2, ::2, :] = 1
    m[:, ::2, X - 1] = 1
    m[Z - 1, :, X - 1] = 1
    return m


def checkerboard(shape):
    z, y, x = np.indices(shape)
    return ((z + y + x) % 2 == 0).astype(np.uint8)


def two_boxes(shape, kind, T=TILE):
    """Two 2 x 2 x 2 boxes (clipped to the volume) around the first interior tile corner (or the centre, where an axis
    has no seam), touching only along an edge ("edge") or only at a corner ("corner"): two components."""
    c = [t if s > t + 1 else max(1, s // 2) for s, t in zip(shape, T)]
    m = np.zeros(shape, dtype=np.uint8)
    m[max(0, c[0] - 2):c[0], max(0, c[1] - 2):c[1], max(0, c[2] - 2):c[2]] = 1
    if kind == "edge":
        m[max(0, c[0] - 2):c[0], c[1]:c[1] + 2, c[2]:c[2] + 2] = 1
    else:
        m[c[0]:c[0] + 2, c[1]:c[1] + 2, c[2]:c[2] + 2] = 1
    return m


def boxes_separable(shape, kind):
    """The two boxes exist and are apart only where the axes they are offset along are longer than 1."""
    return min(shape[1:]) >= 2 if kind == "edge" else min(shape) >= 2


@functools.lru_cache(maxsize=None)
def pattern(name, shape):
    if name == "zeros":
        m = np.zeros(shape, dtype=np.uint8)
    elif name == "ones":
        m = np.ones(shape, dtype=np.uint8)
    elif name.startswith("bernoulli"):
        p = float(name[len("bernoulli"):])
        g = np.random.default_rng([23, int(p * 100)] + list(shape))
        m = (g.random(shape) < p).astype(np.uint8)
    elif name == "serpentine":
        m = serpentine(shape)
    elif name == "comb":
        m = comb(shape)
    elif name == "checkerboard":
        m = checkerboard(shape)
    else:
        m = two_boxes(shape, name)
    m.setflags(write=False)
    return m


# ------------------------------------------------------------------------------------------------ largest component
def _blocks(shape, blocks):
    m = np.zeros(shape, dtype=np.uint8)
    for (z0, z1, y0, y1, x0, x1) in blocks:
        m[z0:z1, y0:y1, x0:x1] = 1
    return m


def largest_cases():
    """name -> (mask, num_limit, min_filter). Components in C order of their first voxel."""
    shape = (12, 20, 70)
    plain = _blocks(shape, [(0, 2, 0, 2, 0, 3), (1, 9, 4, 16, 5, 69), (10, 12, 0, 3, 0, 4)])    # 12, 6144, 24
    tie = _blocks(shape, [(0, 1, 0, 1, 0, 2), (1, 4, 2, 6, 3, 67), (6, 9, 2, 6, 3, 67), (10, 11, 0, 1, 0, 5)])
    hidden = np.zeros(shape, dtype=np.uint8)
    hidden[0, 0, 0:12:2] = 1                                                  # six specks: labels 1..6
    hidden[2:10, 2:18, 2:68] = 1                                              # label 7
    return {
        "plain": (plain, 10, 20.0),
        "tie": (tie, 10, 100.0),                    # labels 2 and 3 hold 768 voxels each: 2 wins
        "hidden": (hidden, 7, 1.0),                 # labels 1..6 are looked at: the big one is label 7, a speck wins
        "hidden_found": (hidden, 8, 1.0),           # one more label looked at: the big one
        "none": (plain, 10, 1e5),                   # nothing reaches min_filter
        "fractional": (plain, 10, 11.5),            # 12 >= 11.5 qualifies, and loses to 6144
        "fractional_cut": (_blocks(shape, [(0, 2, 0, 2, 0, 3), (4, 5, 0, 2, 0, 5)]), 10, 10.5),   # 12 passes, 10 < 10.5
        "exact": (_blocks(shape, [(0, 2, 0, 2, 0, 3)]), 10, 12.0),            # size == min_filter qualifies (not <)
    }


# ------------------------------------------------------------------------------------------------ body crop inputs
def synth(shape, seed, body, lo, hi, noise, arm=None, slab=None, specks=10, holes=40, label_x=None, big_codes=True):
    """image fp32 [Z, Y, X]: background N(lo, noise), a body box (and an arm box joined to it, a slab apart from it) at
    N(hi, noise), `specks` 3 x 3 x 3 bright blocks in the planes before the body (components that number before it),
    `holes` dark 2 x 2 x 2 blocks inside it, a NaN and an exact-threshold voxel left to the caller. label fp32: sparse
    codes 1..13 inside the body within x in label_x (both ends set), and, with big_codes, codes 14 and 15 outside that
    x range (they must be cleared before the range is taken)."""
    g = np.random.default_rng([24, seed])
    Z, Y, X = shape
    img = (lo + noise * g.standard_normal(shape)).astype(np.float32)

    def fill(b):
        sub = img[b[0]:b[1], b[2]:b[3], b[4]:b[5]]
        sub[...] = (hi + noise * g.standard_normal(sub.shape)).astype(np.float32)

    fill(body)
    if arm is not None:
        fill(arm)
    if slab is not None:
        fill(slab)
    for _ in range(specks):
        z = int(g.integers(0, max(1, body[0] - 4)))
        y, x = int(g.integers(0, Y - 3)), int(g.integers(0, X - 3))
        fill((z, z + 3, y, y + 3, x, x + 3))
    for _ in range(holes):
        z, y, x = (int(g.integers(body[2 * i] + 1, body[2 * i + 1] - 3)) for i in range(3))
        img[z:z + 2, y:y + 2, x:x + 2] = np.float32(lo)
    lab = np.zeros(shape, dtype=np.float32)
    lx0, lx1 = label_x if label_x is not None else (body[4], body[5] - 1)
    zc, yc = (body[0] + body[1]) // 2, (body[2] + body[3]) // 2
    n = max(8, (body[1] - body[0]) * (body[3] - body[2]) // 4)
    lab[g.integers(body[0], body[1], n), g.integers(body[2], body[3], n), g.integers(lx0, lx1 + 1, n)] = \
        g.integers(1, 14, n).astype(np.float32)
    lab[zc, yc, lx0], lab[zc, yc, lx1] = 1.0, 2.0
    if big_codes:
        lab[zc, yc, 0], lab[zc, yc, X - 1], lab[0, 0, X - 1] = 14.0, 15.0, 14.0
    return img, lab


# name -> (cid, kwargs of synth). The reference's filters (1e6, then 1e5 for the upper half) are no parameters of its
# crop section, so the fixture volumes hold millions of voxels.
FIXTURES = {
    # MRI, cid > 500: body 100 x 112 x 110 (> 1e6 after the x crop and the erosion), an arm at high x that lengthens
    # the z extent by 66: both get_body calls on the component route, the hand branch taken
    "mri_hand": (530, dict(shape=(200, 130, 120), seed=1, body=(22, 122, 10, 122, 6, 116), arm=(122, 188, 40, 70, 92, 112),
                           slab=(22, 150, 125, 129, 6, 80), lo=0.0, hi=200.0, noise=5.0, specks=14)),
    # CT, cid <= 410: body below 1e6 voxels: the first call falls back to the box opening, the upper half (>= 1e5) is
    # found as a component; no hand branch; label codes >= 14 outside the label's x range
    "ct_fallback": (100, dict(shape=(120, 100, 100), seed=2, body=(20, 100, 10, 90, 8, 92), arm=(100, 118, 40, 60, 70, 88),
                              lo=-900.0, hi=40.0, noise=30.0, specks=8)),
    # the special threshold 30000 (cid 518, > 500): both calls fall back; the arm is thick enough to survive the
    # opening, the hand branch is taken
    "special_both_fallback": (518, dict(shape=(90, 40, 60), seed=3, body=(4, 34, 4, 36, 4, 56), arm=(34, 86, 8, 30, 40, 54),
                                        lo=1000.0, hi=40000.0, noise=300.0, specks=4, holes=10)),
}

# small shapes for the GPU tests against the restatement: name -> (cid, min_filter, min_filter_up, kwargs)
SMALL = {
    # component route twice, hand taken
    "hand": (530, 2000.0, 500.0, dict(shape=(58, 20, 44), seed=11, body=(4, 16, 2, 18, 3, 41), arm=(16, 55, 6, 14, 30, 40),
                                      lo=0.0, hi=200.0, noise=5.0, specks=3, holes=6)),
    # the same geometry at CT intensities under a CT case id: the extents differ by more than 30, the case id alone
    # keeps the hand branch from firing
    "nohand_cid": (300, 2000.0, 500.0, dict(shape=(58, 20, 44), seed=11, body=(4, 16, 2, 18, 3, 41),
                                            arm=(16, 55, 6, 14, 30, 40), lo=-900.0, hi=40.0, noise=30.0, specks=3, holes=6)),
    # cid > 500 without an arm: extents agree, no hand
    "nohand_extent": (600, 2000.0, 500.0, dict(shape=(30, 20, 44), seed=12, body=(4, 26, 2, 18, 3, 41), lo=0.0, hi=200.0,
                                               noise=5.0, specks=3, holes=6)),
    # first call fallback (min_filter above the body), upper half found
    "fallback_first": (450, 1e5, 500.0, dict(shape=(30, 24, 44), seed=13, body=(4, 26, 2, 22, 3, 41), lo=0.0, hi=200.0,
                                             noise=5.0, specks=3, holes=6)),
    # both fallback, hand taken through the opening
    "fallback_both_hand": (518, 1e6, 1e5, dict(shape=(64, 24, 44), seed=14, body=(2, 16, 2, 22, 3, 41),
                                               arm=(16, 62, 4, 18, 28, 40), lo=1000.0, hi=40000.0, noise=300.0, specks=2,
                                               holes=4)),
}


@functools.lru_cache(maxsize=None)
def case_inputs(name):
    cid, kw = FIXTURES[name] if name in FIXTURES else (SMALL[name][0], SMALL[name][3])
    img, lab = synth(**kw)
    t = {540: 30000, 518: 30000}.get(cid, 25 if cid > 410 else -200)
    b = kw["body"]
    img[b[0] + 2, b[2] + 2, b[4] + 2] = np.float32("nan")     # NaN > t is false: a hole
    img[b[0] + 2, b[2] + 5, b[4] + 2] = np.float32(t)         # the comparison is strict: a hole
    img.setflags(write=False)
    lab.setflags(write=False)
    return cid, img, lab
