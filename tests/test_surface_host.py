"""Host-side contract of the surface metrics (no device): the entry points of csrc/edt.hip are declared in the header,
listed in the signature table with the declared arity and exported by the built library; the size queries answer
without a device; u3d.surface and evaluate_amos.get_surface_scores check their arguments and have no CPU path."""
import inspect
import os
import re

import pytest
import torch

import surface_cases as K
from conftest import PKG, REPO

ENTRY_POINTS = ["u3d_edt", "u3d_edt_ws_bytes", "u3d_edt_max_extent", "u3d_edt_tile", "u3d_surface_reduce_ws_bytes",
                "u3d_mask_surface", "u3d_class_boxes", "u3d_surface_dist_reduce"]


def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def _declared_arity(hdr, name):
    m = re.search(r"^(?:int|long long|void) " + name + r"\(([^;]*)\);", hdr, re.M)
    assert m, f"{name} is not declared in u3d.h"
    args = " ".join(m.group(1).split())
    return 0 if args == "void" else args.count(",") + 1


def test_entry_points_are_declared_listed_and_exported():
    from u3d import _lib
    hdr = _read(REPO, "include", "u3d.h")
    h = _lib.lib()
    for name in ENTRY_POINTS:
        assert name in _lib._SIGS and name in _lib.exported_symbols(), name
        assert len(_lib._SIGS[name]) == _declared_arity(hdr, name), name
        assert getattr(h, name) is not None, name
    for name in ("u3d_edt_ws_bytes", "u3d_surface_reduce_ws_bytes"):
        assert _lib._RESTYPE[name] is _lib.L
    assert "#define U3D_CLASS_RECORD 8" in hdr and "#define U3D_SURFACE_RECORD 5" in hdr
    srcs = re.search(r"^SRCS := (.*)$", _read(PKG, "csrc", "Makefile"), re.M).group(1).split()
    assert "edt.hip" in srcs and "edt_core.h" in _read(PKG, "csrc", "Makefile")
    for f in ("edt.hip", "edt_core.h"):
        assert os.path.exists(os.path.join(PKG, "csrc", f))


def test_size_queries_answer_without_a_device():
    from u3d import _lib, surface
    q = _lib.query
    assert q("u3d_edt_ws_bytes", 0) == -1 and q("u3d_edt_ws_bytes", 2 ** 31) == -1
    assert q("u3d_edt_ws_bytes", 1) == 8 and q("u3d_edt_ws_bytes", 2 ** 31 - 1) == 8 * (2 ** 31 - 1)
    assert surface.edt_max_extent() == K.MAX_EXTENT >= 1024
    assert surface.edt_tile() == (K.MAX_COLS, K.TILE_BYTES)
    assert K.tile_cols(K.MAX_EXTENT) >= 1 and K.tile_cols(K.MAX_EXTENT) * K.MAX_EXTENT * 8 <= K.TILE_BYTES
    assert K.TILE_BYTES <= 64 * 1024                                     # a workgroup's LDS without opting in to more
    assert 0 < q("u3d_surface_reduce_ws_bytes") <= 1 << 20


def test_constants_mirror_the_core_header():
    core = _read(PKG, "csrc", "edt_core.h")
    for name, value in (("MAX_EXTENT", K.MAX_EXTENT), ("MAX_COLS", K.MAX_COLS), ("TILE_BYTES", K.TILE_BYTES)):
        assert re.search(rf"constexpr int {name} = {value};", core), name
    assert K.line_thresholds() == [64, 128, 256, 512, 1024, 2048]
    assert [K.tile_cols(n) for n in (1, 64, 65, 128, 129, 1024, 1025, 2048)] == [64, 64, 32, 32, 16, 4, 2, 2]


def test_public_signatures():
    import evaluate_amos
    from u3d import surface
    assert list(inspect.signature(surface.distance_to).parameters) == ["mask", "spacing", "squared"]
    assert list(inspect.signature(surface.distance_transform_edt).parameters) == ["mask", "sampling", "squared"]
    assert list(inspect.signature(surface.mask_surface).parameters) == ["x", "value"]
    assert list(inspect.signature(surface.surface_distances).parameters) == ["a", "b", "spacing"]
    sig = inspect.signature(surface.surface_metrics)
    assert list(sig.parameters) == ["pred", "gt", "num_class", "spacing", "tolerance", "percentile"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[2:]] == [13, (1, 1, 1), 1.0, 95.0]
    sig = inspect.signature(evaluate_amos.get_surface_scores)
    assert list(sig.parameters) == ["preds", "labels", "t_id", "num_class", "spacing", "tolerance"]
    assert [sig.parameters[k].default for k in list(sig.parameters)[3:]] == [13, (1, 1, 1), 1.0]
    assert list(inspect.signature(evaluate_amos.get_dice).parameters) == ["preds", "labels", "t_id", "atlas", "num_class"]


def test_argument_errors():
    from u3d import surface
    m3 = torch.ones((3, 4, 5), dtype=torch.uint8)
    lab4 = torch.ones((2, 3, 4, 5), dtype=torch.int64)
    for f in (surface.distance_to, surface.distance_transform_edt, surface.mask_surface):
        for shape in ((4, 5), (1, 2, 3, 4), (0, 3, 4)):
            with pytest.raises(ValueError):
                f(torch.ones(shape, dtype=torch.uint8))
    with pytest.raises(ValueError):
        surface.surface_distances(torch.ones((3, 4), dtype=torch.uint8), m3)
    for bad in ((0, 1, 1), (1, -2, 1), (1, 1), (1, 1, float("inf")), (1, float("nan"), 1)):
        with pytest.raises(ValueError, match="spacing"):
            surface.distance_to(m3, spacing=bad)
        with pytest.raises(ValueError, match="spacing"):
            surface.distance_transform_edt(m3, sampling=bad)
        with pytest.raises(ValueError, match="spacing"):
            surface.surface_distances(m3, m3, spacing=bad)
        with pytest.raises(ValueError, match="spacing"):
            surface.surface_metrics(lab4, lab4, spacing=bad)
    with pytest.raises(ValueError, match="tolerance"):
        surface.surface_metrics(lab4, lab4, num_class=13, tolerance=[1.0] * 12)
    with pytest.raises(ValueError, match="tolerance"):
        surface.surface_metrics(lab4, lab4, num_class=3, tolerance=[1.0] * 4)
    with pytest.raises(ValueError):
        surface.surface_metrics(lab4[0, 0], lab4[0, 0])                 # rank 2
    with pytest.raises(ValueError):
        surface.surface_metrics(lab4, lab4[0])                          # ranks differ
    with pytest.raises(ValueError):
        surface.surface_metrics(lab4, lab4[:, :2])                      # shapes differ
    with pytest.raises(ValueError, match="integer"):
        surface.surface_metrics(lab4.float(), lab4)
    with pytest.raises(ValueError):
        surface.surface_metrics(lab4, lab4, num_class=65)
    with pytest.raises(ValueError):
        surface.surface_metrics(lab4, lab4, percentile=101)


def test_there_is_no_cpu_path():
    import evaluate_amos
    from u3d import U3DError, surface
    m3 = torch.ones((3, 4, 5), dtype=torch.uint8)
    lab4 = torch.ones((2, 3, 4, 5), dtype=torch.int64)
    for call in (lambda: surface.distance_to(m3), lambda: surface.distance_transform_edt(m3),
                 lambda: surface.mask_surface(m3), lambda: surface.mask_surface(lab4[0], value=1),
                 lambda: surface.surface_distances(m3, m3), lambda: surface.class_boxes(lab4[0], lab4[0], 3),
                 lambda: surface.surface_metrics(lab4, lab4.float()),
                 lambda: evaluate_amos.get_surface_scores(lab4, lab4[:, None].float(), 0),
                 lambda: evaluate_amos.get_surface_scores(torch.zeros((2, 14, 3, 4, 5)), lab4[:, None].float(), 0)):
        with pytest.raises(U3DError, match="no CPU fallback"):
            call()
