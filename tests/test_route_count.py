"""A conv's backward is routed once: during Tape.backward of a whole training step (driven on meta tensors by
tools/route_trace.py, nothing launched), ops.conv_route(dgrad=True) and ops.wgrad_route are each evaluated at most once
per conv backward closure that ran. Before ops.conv_bwd the same step evaluated the data-gradient route 51 times for
35 convs."""
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _tool():
    sys.path[:0] = [REPO, os.path.join(REPO, "multimodal-pl_amd"), os.path.join(REPO, "tools")]
    if not os.path.exists(os.path.join(REPO, "multimodal-pl_amd", "u3d", "libu3d.so")):
        pytest.skip("library not built")
    import route_trace
    return route_trace


@pytest.mark.parametrize("inp", ["bf16_2x96", "bf16_1x32"])
@pytest.mark.parametrize("model", ["unet3D", "baseline", "unet3D_g"])
def test_each_conv_backward_is_routed_once(monkeypatch, model, inp):
    rt = _tool()
    from u3d import ops, trunk
    n = {"dgrad": 0, "wgrad": 0, "convs": 0, "pend": 0, "stem": 0}
    inside = []

    def counted(mod, name, key, when=lambda a, kw: True):
        fn = getattr(mod, name)

        def wrapper(*a, **kw):
            if inside and when(a, kw):
                n[key] += 1
            return fn(*a, **kw)
        monkeypatch.setattr(mod, name, wrapper)

    counted(ops, "conv_route", "dgrad", lambda a, kw: bool(kw.get("dgrad", a[7] if len(a) > 7 else False)))
    counted(ops, "wgrad_route", "wgrad")
    counted(ops, "conv_bwd", "convs")             # one per conv backward closure that had a gradient
    counted(trunk.Tape, "pend_wgrad", "pend")     # (the same count, taken at the tape: every conv and the stem)
    counted(ops, "stem_wgrad", "stem")
    backward = trunk.Tape.backward

    def tape_backward(self, *a):
        inside.append(1)
        try:
            return backward(self, *a)
        finally:
            inside.pop()
    monkeypatch.setattr(trunk.Tape, "backward", tape_backward)

    shape, dtype = rt.TRUNK_INPUTS[inp]
    with rt.recording():
        rt.trunk_step(model, shape, dtype)
    print(n)
    assert n["convs"] >= 35 and n["convs"] == n["pend"] - n["stem"]
    assert 0 < n["dgrad"] <= n["convs"]
    assert 0 < n["wgrad"] <= n["convs"]
