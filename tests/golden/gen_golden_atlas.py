"""Generate the G19 atlas fixture by running the REFERENCE on the CPU (test infrastructure, run where the reference is
present, as tests/golden/gen_golden.py whose shims it imports):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_atlas.py

  g19_atlas.npz
    crop_<tag>_*   AMOSDataSet_newatlas.__getitem__'s own lines on the cases of tests/atlas_cases.py: the resize of the
                   float64 atlas to the image's shape (MOTSDataset.py:357) and :370-397 (pad, truncate, crop, transpose)
                   exec'd as gen_golden.py::g15 does, np.random a seeded RandomState whose draws are recorded. Stored:
                   the atlas output (float64 in the reference; its values are multiples of 1/64, so the float32 copy
                   stored here is exact, which is asserted), the draws, the resized shape.
    dice_<case>_*  the reference's get_dice(preds, labels, 1, atlas, num_class) on the gated-Dice cases: the three
                   lists as float64 arrays and the argmax map.

Only outputs are stored: inputs are rebuilt from seeds by tests/atlas_cases.py (their checksum is stored).
"""
import math
import os
import sys
import types

import numpy as np
import torch

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_golden as G  # noqa: E402  (reference imports + shims)
import atlas_cases as AC  # noqa: E402


def crop_cases(out):
    src_methods = "\n".join(G._ref_lines("MOTSDataset.py", a, b) for a, b in ((171, 186), (269, 282), (284, 297)))
    src_resize = G._ref_lines("MOTSDataset.py", 357, 357)
    src_get = G._ref_lines("MOTSDataset.py", 370, 397).replace("return image.copy(), label.copy(), name, name, catlas",
                                                             "out = (image.copy(), label.copy(), catlas)")
    assert "catlas = nn.functional.interpolate(torch.tensor(self.atlas).unsqueeze(0), image.shape)" in src_resize
    assert "catlas = self.pad_image2(catlas" in src_get and "out = (" in src_get, "reference lines moved"
    ns = {"np": np, "math": math}
    exec(compile("class DS:\n" + "\n".join("    " + ln for ln in src_methods.splitlines()),
                 "MOTSDataset.py:171-297", "exec"), ns)
    for tag, (ashape, ishape, crop, usage, seed) in AC.CROP_CASES.items():
        atlas, image, label = AC.crop_inputs(tag)
        assert atlas.dtype == np.float64
        ds = ns["DS"]()
        ds.crop_d, ds.crop_h, ds.crop_w = crop
        ds.usage, ds.atlas = usage, atlas.copy()

        class _Rec:
            def __init__(self, seed):
                self.rs, self.draws = np.random.RandomState(seed), []

            def randint(self, *a):
                v = self.rs.randint(*a)
                self.draws.append(int(v))
                return v
        rec = _Rec(seed)
        npx = types.SimpleNamespace(**{k: getattr(np, k) for k in ("newaxis", "float32")})
        npx.random = rec
        env = {"self": ds, "image": image.copy(), "label": label.copy(), "name": AC.NAME, "np": npx, "nn": torch.nn,
               "torch": torch}
        exec(compile(src_resize, "MOTSDataset.py:357", "exec"), env)
        assert env["catlas"].dtype == np.float64 and env["catlas"].shape == (ashape[0],) + tuple(ishape)
        out[f"crop_{tag}_resized_shape"] = np.array(env["catlas"].shape)
        exec(compile(src_get, "MOTSDataset.py:370-397", "exec"), env)
        ca = env["out"][2]
        assert np.array_equal(ca.astype(np.float32).astype(np.float64), ca)
        out[f"crop_{tag}_catlas"] = ca.astype(np.float32)
        out[f"crop_{tag}_draws"] = np.array(rec.draws, dtype=np.int64)
        out[f"crop_{tag}_insum"] = np.array(AC.checksum(atlas, image, label))


def dice_cases(out):
    for case in AC.DICE_FIXTURE:
        preds, lab, atlas = AC.dice_inputs(case)
        ncls = case[2]
        dices, senc, spec, am = G.REV.get_dice(preds, lab, 1, atlas.double(), num_class=ncls)
        key = "dice_" + AC.case_id(case)
        out[f"{key}_dice"] = np.array([float(v) for v in dices])
        out[f"{key}_senc"] = np.array([float(v) for v in senc])
        out[f"{key}_spec"] = np.array([float(v) for v in spec])
        out[f"{key}_argmax"] = am.numpy().astype(np.int8)
        out[f"{key}_insum"] = np.array(AC.checksum(preds.numpy(), lab.numpy(), atlas.numpy()))


if __name__ == "__main__":
    out = {}
    crop_cases(out)
    dice_cases(out)
    G.save("g19_atlas.npz", **out)
