"""Which kernels the dispatcher launches is pinned, exactly: tools/route_trace.py drives whole training steps and every
conv wrapper of u3d.ops on meta tensors (library calls recorded with their scalar arguments, workspace requests with
slot and size, nothing launched) and route_trace_expected.json holds a digest of each trace. The digests were written
by ``tools/route_trace.py --write`` from the tree before the routing was gathered into ops.conv_route, so a routing
change shows here as a changed digest (``--dump DIR`` on both trees, then diff, names the call). The configurations
that steer a conv's backward on the tape (backward flags, tape pieces, a formed loss gradient) were added with
ops.conv_bwd; their digests were written from the u3d package of the commit before it. The
whole-model configurations (model/...: model.forward and torch.autograd.backward of every model class, through the
autograd Function) were written from the tree before the model layer was gathered into trunk.TapeFn / trunk.run_model
(DESIGN.md section 22)."""
import json
import os
import sys

import pytest

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
EXPECTED = os.path.join(os.path.dirname(os.path.abspath(__file__)), "route_trace_expected.json")

with open(EXPECTED) as _f:
    WANT = json.load(_f)


def _tool():
    sys.path[:0] = [REPO, os.path.join(REPO, "multimodal-pl_amd"), os.path.join(REPO, "tools")]
    if not os.path.exists(os.path.join(REPO, "multimodal-pl_amd", "u3d", "libu3d.so")):
        pytest.skip("library not built")
    import route_trace
    return route_trace


def test_recorded_configurations_are_the_expected_ones():
    rt = _tool()
    assert sorted(rt.configs()) == sorted(WANT)
    names = set(WANT)
    for m in rt.MODELS:  # the step of every model at every input, and every flag flipped at bf16 2 x 96^3
        assert {f"trunk/{m}/{i}" for i in rt.TRUNK_INPUTS} <= names
        assert {f"trunk/{m}/bf16_2x96/{f}" for f in rt.FLAG_SETS} <= names
    assert WANT["trunk/unet3D/bf16_2x96"]["calls"]["u3d_conv32_ring_stats"] > 0  # the flagship step runs the ring
    assert len(rt.MODEL_TAGS) == 8
    for tag in rt.MODEL_TAGS:  # every model class through model.forward and autograd, and one inference each
        assert {f"model/{tag}/{i}" for i in rt.MODEL_INPUTS} | {f"model/{tag}/bf16_1x32/inference"} <= names
    for tag, entry in (("unet3D", "u3d_dynhead_bwd"), ("feam3_up", "u3d_upsample_trilinear_bwd"),
                       ("feam2_ema", "u3d_renew_token"), ("eam", "u3d_eam_pool_bwd"), ("feam", "u3d_eam_param_bwd")):
        assert WANT[f"model/{tag}/fp32_1x32"]["calls"][entry] > 0  # (the step ran whole: an error would end it early)


@pytest.mark.parametrize("name", sorted(WANT))
def test_route_trace(name):
    rt = _tool()
    from u3d import ops
    before = {n: getattr(ops, n) for n in ("call", "_stream", "require_device", *(k for kw in rt.FLAG_SETS.values()
                                                                                   for k in kw if hasattr(ops, k)))}
    got = rt.digest(rt.run_config(rt.configs()[name]))
    assert all(getattr(ops, n) is v for n, v in before.items()) and "get" not in vars(ops.WS)  # nothing left patched
    assert got["calls"] == WANT[name]["calls"]
    assert got == WANT[name]
