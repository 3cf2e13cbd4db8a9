"""Host-side contract of the atlas construction (no device): zoom_index is scipy's zoom(order=0) index rule, average_shape
the reference's rounding; the public entry points exist, have no CPU path, and the header, the signature table, the
Makefile and INTEGRATION.md name the native entry points."""
import inspect
import os
import re

import numpy as np
import pytest
import torch
from scipy import ndimage

import atlas_build_cases as K
from conftest import PKG, REPO

ENTRY_POINTS = ["u3d_atlas_build_add", "u3d_atlas_build_normalize", "u3d_atlas_build_ws_bytes"]


def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def _scipy_index(n_in, n_out):
    """scipy's own answer: zoom of 1..n_in (0 = the constant outside the volume) -> source index, -1 for "nothing"."""
    z = ndimage.zoom(np.arange(1, n_in + 1, dtype=np.float64), n_out / n_in, order=0)
    assert z.shape == (n_out,)
    return z.astype(np.int64) - 1


def test_zoom_index_is_scipys_rule():
    from u3d.data import zoom_index
    pairs = [(i, o) for i in range(1, 70) for o in range(1, 70)] + K.QUIRK_PAIRS + [(512, 487), (100, 103), (768, 512)]
    lost = clamp_bad = rint_bad = 0
    for n_in, n_out in pairs:
        t = zoom_index(n_in, n_out)
        assert t.dtype == np.int32 and t.shape == (n_out,)
        want = _scipy_index(n_in, n_out)
        assert np.array_equal(t, want), (n_in, n_out)
        assert t.max() < n_in and t.min() >= -1
        lost += int((t < 0).any())
        z = (n_in - 1) / (n_out - 1) if n_out > 1 else 1.0
        cc = np.arange(n_out) * z
        clamp_bad += int(not np.array_equal(np.minimum(np.floor(cc + 0.5), n_in - 1), want))
        rint_bad += int(not np.array_equal(np.where(cc <= n_in - 1, np.rint(cc), -1), want))
    for p in K.QUIRK_PAIRS:
        assert zoom_index(*p)[-1] == -1, p
    assert lost > 0 and clamp_bad >= lost and rint_bad > 0     # the two plausible restatements are wrong somewhere
    print(f"zoom_index: {len(pairs)} pairs, {lost} lose the last plane, rint differs in {rint_bad}")
    with pytest.raises(ValueError):
        zoom_index(0, 3)


def test_average_shape_rounds_half_to_even():
    from u3d.data import average_shape
    assert average_shape([(4, 8, 5), (2, 10, 4)]) == (3, 9, 4)          # 4.5 -> 4
    assert average_shape([(5, 3, 1), (6, 4, 2)]) == (6, 4, 2)           # 5.5 -> 6, 3.5 -> 4, 1.5 -> 2
    assert average_shape([(1, 2, 2), (2, 3, 3)]) == (2, 2, 2)           # 1.5 -> 2, 2.5 -> 2
    assert average_shape([torch.Size([7, 8, 9])]) == (7, 8, 9)
    assert all(isinstance(v, int) for v in average_shape([(3, 3, 3), (4, 4, 4), (4, 4, 5)]))
    with pytest.raises(ValueError):
        average_shape([])


def test_header_signature_table_makefile_and_integration_rows():
    from u3d import _lib
    hdr = _read(REPO, "include", "u3d.h")
    for name in ENTRY_POINTS:
        assert re.search(r"^(int|long long) " + name + r"\(", hdr, re.M), name
        assert name in _lib._SIGS and name in _lib.exported_symbols()
    assert "floor(cc + 0.5)" in hdr                                      # the formula is spelled out
    assert len(_lib._SIGS["u3d_atlas_build_add"]) == 15 and len(_lib._SIGS["u3d_atlas_build_normalize"]) == 6
    assert _lib._SIGS["u3d_atlas_build_ws_bytes"] == [] and _lib._RESTYPE["u3d_atlas_build_ws_bytes"] is _lib.L
    srcs = re.search(r"^SRCS := (.*)$", _read(PKG, "csrc", "Makefile"), re.M).group(1).split()
    assert "atlas_build.hip" in srcs and os.path.exists(os.path.join(PKG, "csrc", "atlas_build.hip"))
    doc = _read(REPO, "INTEGRATION.md")
    assert "atlas_gen_mm.py:93-145" in doc
    for name in ENTRY_POINTS[:2] + ["u3d_aug_blur_axis"]:
        assert f"`{name}`" in doc, name


def test_public_entry_points_and_no_cpu_path():
    from u3d import U3DError, data
    assert list(inspect.signature(data.AtlasBuilder.__init__).parameters) == ["self", "shape", "num_labels", "device"]
    sig = inspect.signature(data.build_atlas)
    assert list(sig.parameters) == ["labels", "shape", "num_labels", "sigma"]
    assert sig.parameters["shape"].default is None and sig.parameters["num_labels"].default == 15
    assert sig.parameters["sigma"].default == 3.0
    assert inspect.signature(data.AtlasBuilder.finish).parameters["sigma"].default == 3.0
    with pytest.raises(ValueError):
        data.AtlasBuilder((3, 3, 3), num_labels=32)
    with pytest.raises(ValueError):
        data.AtlasBuilder((3, 3))
    with pytest.raises(U3DError, match="no CPU fallback"):
        data.AtlasBuilder((3, 3, 3), device="cpu")
    lab = torch.zeros(4, 5, 6, dtype=torch.uint8)
    b = data.AtlasBuilder((3, 3, 3))
    with pytest.raises(ValueError):
        b.add(torch.zeros(4, 5, dtype=torch.uint8))
    with pytest.raises(U3DError, match="no CPU fallback"):
        b.add(lab)
    if not torch.cuda.is_available():
        with pytest.raises(U3DError, match="no CPU fallback"):
            b.finish()
    with pytest.raises(U3DError, match="no CPU fallback"):
        data.build_atlas([lab, lab])
    with pytest.raises(U3DError, match="no CPU fallback"):
        data.build_atlas([lab], shape=(3, 3, 3))
    with pytest.raises(ValueError):
        data.build_atlas([], shape=(3, 3, 3))
