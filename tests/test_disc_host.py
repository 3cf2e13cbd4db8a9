"""Host-side contract of the style discriminators (no device): the three modules keep the reference's constructor,
submodule structure, state_dict keys / shapes and default initialisation (G17 case M5), have no CPU path, and name the
limit they enforce."""
import hashlib

import pytest
import torch

import disc_cases as DC
from conftest import golden

KINDS = ["norm", "deep", "seq"]


def _build(kind, num_classes=DC.NUM_CLASSES, **kw):
    import unet3D
    return getattr(unet3D, DC.KINDS[kind])(num_classes, **kw)


@pytest.mark.parametrize("kind", KINDS)
def test_m5_state_dict_and_default_init_match_reference(kind):
    g = golden("g17_disc.npz")
    torch.manual_seed(0)
    m = _build(kind)
    sd = m.state_dict()
    assert list(sd.keys()) == [str(k) for k in g[f"M5_{kind}_keys"]]
    assert [",".join(str(v) for v in t.shape) for t in sd.values()] == [str(s) for s in g[f"M5_{kind}_shapes"]]
    assert all(t.dtype == torch.float32 for t in sd.values())
    assert [t.double().abs().sum().item() for t in sd.values()] == list(g[f"M5_{kind}_abssum"])
    h = hashlib.sha256()
    for t in sd.values():
        h.update(t.contiguous().numpy().tobytes())
    assert h.hexdigest() == str(g[f"M5_{kind}_sha256"])  # bit for bit


def test_submodule_structure():
    deep = _build("deep")
    names = [n for n, _ in deep.named_modules()]
    for n in ["block1.0", "min_block1.0", "block2.0", "min_block2.0", "block3.0", "min_block3.0", "block4.0", "block4.2",
              "block4.4", "block4.8"]:
        assert n in names
    assert isinstance(deep.block4[8], torch.nn.Linear) and deep.block4[8].out_features == 2
    assert deep.ndf == 32 and _build("norm", ndf=64).ndf == 64
    norm = _build("norm")
    assert not any(n.startswith("min_block") for n, _ in norm.named_modules())
    seq = _build("seq")
    assert isinstance(seq, torch.nn.Sequential) and len(seq) == 15 and seq[14].out_features == 1
    assert all(p.requires_grad for p in deep.parameters())


@pytest.mark.parametrize("kind", KINDS)
def test_stub_is_gone(kind):
    try:
        _build(kind)
    except NotImplementedError:
        pytest.fail(f"{DC.KINDS[kind]} still raises NotImplementedError")


def test_other_discriminators_stay_stubs():
    import unet3D
    with pytest.raises(NotImplementedError):
        unet3D.get_style_discriminator(2)


def _args(kind, b=1, dims=(64, 64, 64), c=DC.NUM_CLASSES):
    x = torch.zeros((b, c) + dims)
    if kind != "deep":
        return (x,)
    return x, [torch.zeros((b, 1) + DC.halve(dims, 3 - i)) for i in range(3)]


@pytest.mark.parametrize("kind", KINDS)
def test_cpu_input_raises_not_falls_back(kind):
    from u3d import U3DError
    with pytest.raises(U3DError, match="no CPU fallback"):
        _build(kind)(*_args(kind))


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("ndf", [0, 16, 48])
def test_unsupported_ndf_raises(kind, ndf):
    from u3d import U3DError
    with pytest.raises(U3DError, match="multiple of 32"):
        _build(kind, ndf=ndf)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("nc", [0, 5])
def test_unsupported_num_classes_raises(kind, nc):
    from u3d import U3DError
    with pytest.raises(U3DError, match=r"1\.\.4"):
        _build(kind, num_classes=nc)


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("dims", [(63, 64, 64), (64, 64, 32), (1, 64, 64)])
def test_too_small_volume_raises_naming_the_limit(kind, dims):
    from u3d import U3DError
    with pytest.raises(U3DError, match=">= 64"):
        _build(kind)(*_args(kind, dims=dims))


def test_wrong_channel_count_and_f_m_shapes_raise():
    from u3d import U3DError
    with pytest.raises(U3DError, match="channels"):
        _build("norm")(torch.zeros(1, 3, 64, 64, 64))
    deep = _build("deep")
    x, f_m = _args("deep")
    with pytest.raises(U3DError, match=r"f_m\[2\]"):
        deep(x, [f_m[0], f_m[1], torch.zeros(1, 1, 32, 32, 31)])
    with pytest.raises(U3DError, match=r"f_m\[0\]"):
        deep(x, [f_m[2], f_m[1], f_m[2]])   # block1's resolution where block3's belongs
    with pytest.raises(U3DError, match="f_m"):
        deep(x, f_m[:2])


def test_reference_checkpoint_layout_loads():
    """A state_dict with the fixture's keys and shapes (what a reference checkpoint holds) loads strictly."""
    g = golden("g17_disc.npz")
    for kind in KINDS:
        sd = {str(k): torch.zeros([int(v) for v in str(s).split(",")])
              for k, s in zip(g[f"M5_{kind}_keys"], g[f"M5_{kind}_shapes"])}
        _build(kind).load_state_dict(sd, strict=True)


def test_abi_table_lists_the_disc_entry_points():
    from u3d import _lib
    names = [s for s in _lib.exported_symbols() if s.startswith("u3d_disc_")]
    assert len(names) == 17
    import os
    hdr = open(os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "include", "u3d.h")).read()
    for n in names:
        assert n + "(" in hdr
