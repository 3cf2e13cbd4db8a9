"""Host-side contract of the atlas path (no device): the public entry points exist with the documented signatures, have
no CPU path, and the header, the signature table, the Makefile and INTEGRATION.md name the four native entry points."""
import inspect
import os
import re

import numpy as np
import pytest
import torch

from conftest import PKG, REPO

ENTRY_POINTS = ["u3d_atlas_crop", "u3d_select_probs_fwd", "u3d_select_probs_bwd", "u3d_dice_metric_atlas"]


def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def test_header_declares_the_entry_points():
    hdr = _read(REPO, "include", "u3d.h")
    for name in ENTRY_POINTS:
        assert re.search(r"^int " + name + r"\(", hdr, re.M), name


def test_signature_table_makefile_and_integration_rows():
    from u3d import _lib
    for name in ENTRY_POINTS:
        assert name in _lib._SIGS and name in _lib.exported_symbols()
    assert len(_lib._SIGS["u3d_atlas_crop"]) == 16 and len(_lib._SIGS["u3d_dice_metric_atlas"]) == 12
    assert len(_lib._SIGS["u3d_select_probs_fwd"]) == 12 and len(_lib._SIGS["u3d_select_probs_bwd"]) == 12
    srcs = re.search(r"^SRCS := (.*)$", _read(PKG, "csrc", "Makefile"), re.M).group(1).split()
    assert "atlas.hip" in srcs and os.path.exists(os.path.join(PKG, "csrc", "atlas.hip"))
    doc = _read(REPO, "INTEGRATION.md")
    for name in ENTRY_POINTS:
        assert f"`{name}`" in doc, name


def test_pair_helpers_exist_and_have_no_cpu_path():
    import utils
    from u3d import U3DError
    assert list(inspect.signature(utils.organ_atlas_pairs).parameters) == ["preds", "catlas", "index"]
    assert list(inspect.signature(utils.attention_pairs).parameters) == ["attn", "index"]
    preds, catlas = torch.zeros(1, 14, 2, 3, 4), torch.zeros(13, 2, 3, 4)
    with pytest.raises(U3DError, match="no CPU fallback"):
        utils.organ_atlas_pairs(preds, catlas, [0, 3])
    with pytest.raises(U3DError, match="no CPU fallback"):
        utils.attention_pairs(torch.zeros(1, 13, 2, 3, 4), [1])


def test_crop_patch_takes_the_raw_atlas():
    from u3d import U3DError, data
    sig = inspect.signature(data.crop_patch)
    assert list(sig.parameters)[:7] == ["image", "label", "catlas", "name", "crop_size", "usage", "rng"]   # as before
    assert sig.parameters["atlas"].default is None and sig.parameters["usage"].default == "train"
    assert list(inspect.signature(data.atlas_crop).parameters) == ["atlas", "image_shape", "offsets", "crop"]
    img = torch.zeros(20, 30, 12)
    with pytest.raises(ValueError, match="not both"):
        data.crop_patch(img, img, torch.zeros(13, 20, 30, 12), "0007", (8, 12, 16), atlas=torch.zeros(13, 6, 10, 7))
    with pytest.raises(U3DError, match="no CPU fallback"):
        data.atlas_crop(torch.zeros(13, 6, 10, 7), (20, 30, 12), (0, 0, 0), (12, 16, 8))
    with pytest.raises(U3DError, match="no CPU fallback"):
        data.crop_patch(img, img, None, "0007", (8, 12, 16), rng=np.random.RandomState(0),
                        atlas=torch.zeros(13, 6, 10, 7))


@pytest.mark.parametrize("fn", ["get_dice", "get_dice2"])
def test_gated_dice_has_no_cpu_path_and_is_no_stub(fn):
    import evaluate_amos
    from u3d import U3DError
    preds, labels, atlas = torch.zeros(1, 14, 2, 3, 4), torch.zeros(1, 2, 3, 4), torch.zeros(1, 13, 2, 3, 4)
    with pytest.raises(U3DError, match="no CPU fallback"):
        getattr(evaluate_amos, fn)(preds, labels, 1, atlas)
    src = _read(PKG, "evaluate_amos.py")
    assert "atlas branch" not in "".join(re.findall(r"NotImplementedError\([^)]*\)", src))
