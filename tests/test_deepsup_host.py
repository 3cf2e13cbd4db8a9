"""Host-side contract of the deep-supervision feature (no device): unet3D_with_deepsup keeps the reference's
state_dict keys, has no CPU path, and get_loss's deep_out branch fails the way the reference does."""
import pytest
import torch

from conftest import golden

NC = 14


def _model(**kw):
    import unet3D
    return unet3D.unet3D_with_deepsup([1, 2, 2, 2, 2], num_classes=NC, weight_std=True, **kw)


def test_deepsup_state_dict_keys_match_reference():
    g = golden("g16_deepsup_model.npz")
    m = _model()
    keys = list(m.state_dict().keys())
    assert keys == [str(k) for k in g["keys"]]
    assert [k for k, _ in m.named_parameters()] == [str(k) for k in g["gnames"]]
    assert len(keys) == 119
    assert keys[-8:] == ["x1_resb.0.conv1.weight", "x1_resb.0.gn2.weight", "x1_resb.0.gn2.bias",
                         "x1_resb.0.conv2.weight", "precls_conv.0.weight", "precls_conv.0.bias",
                         "precls_conv.2.weight", "precls_conv.2.bias"]
    assert not any(k.startswith(("eam", "class_token")) for k in keys)


def test_deepsup_ema_detaches_every_parameter():
    assert not any(p.requires_grad for p in _model(ema=True).parameters())
    assert all(p.requires_grad for p in _model().parameters())


@pytest.mark.parametrize("train", [True, False])
def test_deepsup_cpu_forward_raises_not_falls_back(train):
    from u3d import U3DError
    m = _model().train(train)
    with pytest.raises(U3DError):
        m(torch.zeros(1, 1, 16, 16, 16), None)


def _loss_args(levels, c=NC):
    out = torch.zeros(1, NC, 8, 8, 8)
    deep = [torch.zeros(1, c, 2, 2, 2) for _ in range(levels)]
    return out, deep, torch.zeros(1, 1, 8, 8, 8)


def test_get_loss_five_levels_raise_index_error():
    from loss_functions.losses import get_loss
    out, deep, tgt = _loss_args(5)
    with pytest.raises(IndexError):
        get_loss(out, 0, deep, tgt)


def test_get_loss_level_with_wrong_class_count_raises_assertion():
    from loss_functions.losses import get_loss
    out, deep, tgt = _loss_args(2)
    deep[1] = torch.zeros(1, NC - 1, 4, 4, 4)
    with pytest.raises(AssertionError, match="shape do not match"):
        get_loss(out, 0, deep, tgt)
    deep[1] = torch.zeros(2, NC, 4, 4, 4)   # another batch
    with pytest.raises(AssertionError, match="shape do not match"):
        get_loss(out, 0, deep, tgt)


def test_get_loss_pretrain_branch_with_deep_out_has_no_cpu_path():
    """It is built now: CPU tensors fail with the no-fallback error, not NotImplementedError."""
    from loss_functions.losses import get_loss
    from u3d import U3DError
    out, deep, tgt = _loss_args(3)
    with pytest.raises(U3DError):
        get_loss(out, 0, deep, tgt)


def test_deep_supervision_loss_argument_errors():
    from u3d import U3DError
    from u3d.loss import deep_supervision_loss
    _, deep, tgt = _loss_args(3)
    with pytest.raises(U3DError):
        deep_supervision_loss(deep, tgt)
    with pytest.raises(IndexError):
        deep_supervision_loss(deep, tgt, level_weights=(0.5, 1.0))
    with pytest.raises(AssertionError):
        deep_supervision_loss(deep[:1] + [torch.zeros(1, 3, 2, 2, 2)], tgt)
