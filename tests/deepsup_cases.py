"""Inputs of the G16 deep-supervision cases, rebuilt from seeds (numpy Generator streams): the fixture
tests/golden/g16_deepsup.npz stores the reference's outputs and a checksum of these inputs, not the inputs.
Shared by the generator (tests/golden/gen_golden_deepsup.py) and the tests.

Cases (C = 14; geometry = target [S, D, H, W] and the level extents):
  A  (1, 16, 16, 8)   levels (2,2,1) (4,4,2) (8,8,4)                integer ratios 8, 4, 2
  B  (1, 20, 12, 10)  levels (3,2,2) (7,5,3) (10,6,5) (20,12,10)    L = 4, non-integer ratios, an identity level
  C  = A's tensors in get_loss's pre-train branch
  D  (2, 16, 16, 16)  levels (2,2,2) (4,4,4) (8,8,8)                S = 2; class 9 only at odd source indices
"""
import numpy as np

C = 14
LEVEL_WEIGHTS = (0.125, 0.25, 0.5, 1.0)
GEOM = {
    "A": ((1, 16, 16, 8), [(2, 2, 1), (4, 4, 2), (8, 8, 4)]),
    "B": ((1, 20, 12, 10), [(3, 2, 2), (7, 5, 3), (10, 6, 5), (20, 12, 10)]),
    "D": ((2, 16, 16, 16), [(2, 2, 2), (4, 4, 4), (8, 8, 8)]),
}
LABEL_T = [1, 0, 0, 1, 0, 1, 1, 0, 0, 0, 1, 0, 0]   # G9's "mix"
WEIGHT_FEATURE = 0.07
VANISHING = 9
N_SAMPLE = 4096
# The model fixture's input: oracle.weights_recipe.input_volume(shape, seed, kind="normal"). The seed is chosen for
# conditioning, from the reference alone: the gradient of a deep head's GroupNorm bias under the random projection
# is sum_v relu'(pre_v) * dA_v with |dA_v| = O(1), so ONE pre-activation that an fp32 forward puts on the other side
# of zero moves that gradient's norm by up to 0.6 % (seed 160: 1 of 262144 flipped, |pre| < 1e-4, norm off by
# 2.1e-3 while the head backward matched fp64 on its own feature to 1.3e-7). fp32 forwards of this net agree to
# about 3e-5 in the pre-activations; of the seeds 160..171, 166 has the fewest reference pre-activations within
# 3e-5 of zero (3 over the three heads) and the smallest norm change if every one of them flipped (1.9e-4).
MODEL_INPUT = ((2, 1, 32, 32, 32), 166)


def case_inputs(tag):
    """dict of float32 / int64 numpy arrays: logits [S, C, D, H, W], labels [S, 1, D, H, W], mask [15], deep (list),
    and for A / B the consistency branch's att (3 x [1, 13, D, H, W]), refine [13, 2, D, H, W], label_t [13]."""
    (S, *sp), levels = GEOM[tag]
    sp = tuple(sp)
    rng = np.random.default_rng([16, ord(tag)])
    out = {"logits": (rng.standard_normal((S, C) + sp) * 2).astype(np.float32)}
    lab = rng.integers(0, C, (S, 1) + sp)
    mask = np.concatenate([[1], rng.integers(0, 2, 14)]).astype(np.int64)
    mask[3], mask[5], mask[VANISHING] = 0, 1, 1
    if tag == "D":
        lab[lab == VANISHING] = 0
        lab[:, :, 1::4, 1::2, 1::6] = VANISHING   # odd (d, h, w) only: nearest at ratios 8 / 4 / 2 reads even indices
    out["labels"], out["mask"] = lab.astype(np.float32), mask
    out["deep"] = [(rng.standard_normal((S, C) + lv) * 2).astype(np.float32) for lv in levels]
    if tag != "D":
        out["att"] = [(rng.standard_normal((1, C - 1) + sp) * 3).astype(np.float32) for _ in range(3)]
        out["refine"] = (rng.standard_normal((C - 1, 2) + sp) * 3).astype(np.float32)
        out["label_t"] = np.array(LABEL_T, np.float32)
    return out


def checksum(inp):
    """fp64 sum of |x| over every array of a case: stored in the fixture, so a drifted random stream fails loudly."""
    arrs = [inp["logits"], inp["labels"], inp["mask"]] + inp["deep"] + inp.get("att", []) + \
        ([inp["refine"]] if "refine" in inp else [])
    return float(sum(np.abs(a.astype(np.float64)).sum() for a in arrs))


def sample_index(n, *key):
    return np.random.default_rng([163, *key]).integers(0, n, size=N_SAMPLE)


def model_projections(shapes):
    """The seeded projection of (logits, deep x8, deep x4, deep x2) whose backward the model fixture records."""
    rng = np.random.default_rng([161, 0])
    return [rng.standard_normal(s).astype(np.float32) for s in shapes]
