"""Inputs and weights of the G17 style-discriminator cases, rebuilt from seeds (numpy Generator streams): the fixtures
tests/golden/g17_disc*.npz store the reference's outputs and a checksum of these inputs, never the inputs. Shared by
the generator (tests/golden/gen_golden_disc.py), tests/test_disc_reference.py and the GPU model tests.

Cases (num_classes 2, ndf 32):
  M1  norm_style_discriminator_output  B = 2, 64 x 64 x 64
  M2  deep_style_discriminator_output  B = 2, 64 x 64 x 64, f_m at 8^3 / 16^3 / 32^3
  M3  deep_style_discriminator_output  B = 1, 64 x 66 x 70 -> 32 x 33 x 35 -> 16 x 16 x 17 -> 8^3: odd intermediate
      dims, where floor(n / 2) drops the last input plane from every tap but tap 3
  M4  the driver's step (train_amos_atlas_final.py:320-379) on M2's volume with 4 organs: generator pass on
      flist = [0, 2, 3] with frozen parameters, discriminator pass on all 4 with detached inputs
  M5  state_dict keys / shapes / default-initialised parameters after torch.manual_seed(0), the three modules
  M6  B = 0

Weights: He for LeakyReLU(0.2), normal with std sqrt(2 / (1.04 fan_in)), biases normal(0, 0.05). torch's default
initialisation shrinks the signal about 0.4x per layer, which would leave the logits dominated by the biases; with
this recipe the logits follow the inputs. Inputs: per sample and channel a coarse random field (one value per 16^3
cell) scaled by a per-sample gain, squashed to (0, 1) like the softmax maps and the atlas the driver feeds, so the
samples of a batch reach clearly different logits (the generator asserts it).
"""
import numpy as np

NUM_CLASSES, NDF = 2, 32
N_SAMPLE = 256
SLOPE = 0.2
FLIST = [0, 2, 3]
LABEL_T = [1, 0, 0, 1]

# tag -> (kind, B, (D, H, W))
GEOM = {
    "M1": ("norm", 2, (64, 64, 64)),
    "M2": ("deep", 2, (64, 64, 64)),
    "M3": ("deep", 1, (64, 66, 70)),
    "M4": ("deep", 4, (64, 64, 64)),
}
KINDS = {"norm": "norm_style_discriminator_output", "deep": "deep_style_discriminator_output",
         "seq": "get_style_discriminator_output"}


def halve(dims, times):
    for _ in range(times):
        dims = tuple(v // 2 for v in dims)
    return dims


def _map(rng, shape, gain, cell):
    """[*shape] float32 in (0, 1): a random value per cell^3 block, times gain, plus fine noise, through a sigmoid."""
    coarse = rng.standard_normal(tuple(-(-v // cell) for v in shape))
    for ax in range(3):
        coarse = np.repeat(coarse, cell, axis=ax)
    coarse = coarse[:shape[0], :shape[1], :shape[2]]
    v = gain * coarse + 0.3 * rng.standard_normal(shape)
    return (1.0 / (1.0 + np.exp(-v))).astype(np.float32)


def case_inputs(tag):
    """{"x": [B, 2, D, H, W], "f_m": [f at block3's, block2's, block1's output resolution] (deep only)}, float32."""
    kind, B, dims = GEOM[tag]
    rng = np.random.default_rng([17, int(tag[1])])
    gains = [0.6 + 1.1 * s for s in range(B)]
    x = np.stack([np.stack([_map(rng, dims, g * (1.0 if c == 0 else -0.7), 16) for c in range(NUM_CLASSES)])
                  for g in gains])
    out = {"x": x}
    if kind == "deep":
        out["f_m"] = [np.stack([_map(rng, halve(dims, 3 - i), g, 2 ** (i + 1))[None] for g in gains]) for i in range(3)]
    return out


def projection(tag, shape):
    """The seeded projection of the logits whose backward M1-M3 record: loss = sum(logits * projection)."""
    return np.random.default_rng([171, int(tag[1])]).standard_normal(shape).astype(np.float32)


def weights(named_shapes, seed=0):
    """[(name, shape)] in state_dict order -> {name: float32 array}, the He-for-LeakyReLU recipe above."""
    out = {}
    for i, (name, shape) in enumerate(named_shapes):
        rng = np.random.default_rng([172, seed, i])
        if len(shape) == 1:
            out[name] = (0.05 * rng.standard_normal(shape)).astype(np.float32)
        else:
            fan_in = int(np.prod(shape[1:]))
            out[name] = (np.sqrt(2.0 / ((1.0 + SLOPE ** 2) * fan_in)) * rng.standard_normal(shape)).astype(np.float32)
    return out


def fill(module, seed=0):
    """Load the recipe into a module (the reference's, the native one or tests/disc_reference.py's)."""
    import torch
    sd = module.state_dict()
    w = weights([(k, tuple(v.shape)) for k, v in sd.items()], seed)
    module.load_state_dict({k: torch.from_numpy(v) for k, v in w.items()})
    return w


def checksum(inp, w):
    """fp64 sum of |x| over the inputs and the weights: stored in the fixture, so a drifted stream fails loudly."""
    arrs = [inp["x"]] + list(inp.get("f_m", [])) + list(w.values())
    return float(sum(np.abs(a.astype(np.float64)).sum() for a in arrs))


def sample_index(n, *key):
    return np.random.default_rng([173, *key]).integers(0, n, size=min(N_SAMPLE, max(n, 1)))


def grad_summary(named_grads, n_sample=16):
    """[(name, grad tensor)] -> names, fp64 norms, sampled indices, sampled values: the gidx / gval form of G1-G3
    (tests/golden/gen_golden.py grad_summary), for any module."""
    import torch
    names, norms, idx_all, val_all = [], [], [], []
    for i, (k, g) in enumerate(named_grads):
        g = g.detach().reshape(-1).double().cpu()
        idx = np.random.default_rng([1234, i]).integers(0, g.numel(), size=n_sample)
        names.append(k)
        norms.append(g.norm().item())
        idx_all.append(idx)
        val_all.append(g[torch.from_numpy(idx)].numpy())
    return np.array(names), np.array(norms), np.stack(idx_all), np.stack(val_all)


def tensor_summary(t, *key):
    """(fp64 norm, sampled values) of an input / f_m gradient."""
    import torch
    flat = t.detach().reshape(-1).double().cpu()
    return flat.norm().item(), flat[torch.from_numpy(sample_index(flat.numel(), *key))].numpy()
