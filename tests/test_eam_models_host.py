"""unet3D_with_eam, unet3D_with_eam_baseline and unet3D_with_feam without a GPU: the modules are the reference's (names,
shapes and order of named_parameters() as recorded in tests/golden/g18_eam.npz from the reference itself), a CPU
input fails with the no-fallback error and not with the stubs' NotImplementedError, and get_style_discriminator is
still a stub."""
import pytest
import torch

import eam_cases as EC
from conftest import golden


@pytest.mark.parametrize("tag", sorted(EC.MODELS))
def test_named_parameters_match_the_reference(tag):
    import unet3D
    g = golden("g18_eam.npz")
    m = EC.build(unet3D, tag)
    got = [(k, ",".join(str(s) for s in p.shape)) for k, p in m.named_parameters()]
    assert got == list(zip(g[f"{tag}_pnames"].tolist(), g[f"{tag}_pshapes"].tolist()))
    assert all(p.requires_grad for p in m.parameters())


@pytest.mark.parametrize("tag", sorted(EC.MODELS))
def test_ema_detaches_every_parameter(tag):
    import unet3D
    if tag == "base":
        with pytest.raises(TypeError):
            EC.build(unet3D, tag, ema=True)       # the reference's constructor has no ema argument
        return
    assert not any(p.requires_grad for p in EC.build(unet3D, tag, ema=True).parameters())


@pytest.mark.parametrize("train", [True, False])
@pytest.mark.parametrize("tag", sorted(EC.MODELS))
def test_cpu_input_is_the_no_fallback_error(tag, train):
    import unet3D
    from u3d._lib import U3DError
    m = EC.build(unet3D, tag).train(train)
    x = torch.zeros(1, 1, 16, 16, 16)
    with pytest.raises(U3DError):
        m(x, torch.zeros(1, 1, 16, 16, 16)) if tag == "feam" else m(x, None)


def test_style_discriminator_is_still_a_stub():
    import unet3D
    with pytest.raises(NotImplementedError):
        unet3D.get_style_discriminator(14)
