"""Generate the G21 body-crop fixture by running the REFERENCE's own lines on the CPU (test infrastructure, run where
the reference is present, as tests/golden/gen_golden.py whose shims it imports):

    PYTHONDONTWRITEBYTECODE=1 python tests/golden/gen_golden_body_crop.py

  g21_body_crop.npz, per case <name> of tests/body_crop_cases.py::FIXTURES
    <name>_bbox, _bbox_up     [2, 3]: min and (inclusive) max of the nonzero voxels of the two get_body masks
    <name>_size, _size_up     their voxel counts
    <name>_route, _route_up   0: a component was found, 1: the box-opening fallback ("Get max component failed")
    <name>_inter              [inter_all, inter_up, hand branch taken]
    <name>_shapes             [3, 3]: image_a, label_a and the final mask
    <name>_mask_bits          np.packbits of the final mask (maxcomponent as :199-203 leave it)
    <name>_sums               fp64 [nansum(image_a), sum(label_a), orilabelsum]
    <name>_sha                sha256 of image_a and label_a (bytes, C order)
    <name>_insum              a checksum of the inputs

preprocess/forward_crop.py:37-82 (getmaxcomponent, get_body), :148-149 and :157-207 are exec'd, dedented. The one
SimpleITK call, the connected-component filter (face connectivity: FullyConnectedOff is the last call), is stubbed with
scipy.ndimage.label and the face structure, which numbers components by their first voxel in C order as ITK's scan-line
filter does on the same memory layout (an assumption: SimpleITK is not installed where this runs). Only outputs are
stored: inputs are rebuilt from seeds by tests/body_crop_cases.py.
"""
import os
import sys
import types

import numpy as np
import scipy.ndimage as ndimage

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import gen_golden as G  # noqa: E402  (reference path + shims)
import body_crop_cases as BC  # noqa: E402

FNAME = "preprocess/forward_crop.py"
FACE = ndimage.generate_binary_structure(3, 1)

# what each case has to show, asserted on the reference's own variables: (route, route_up, hand)
EXPECT = {"mri_hand": (0, 0, True), "ct_fallback": (1, 0, False), "special_both_fallback": (1, 1, True)}


class _CCA:
    def SetFullyConnected(self, flag):
        self.full = bool(flag)

    def FullyConnectedOff(self):
        self.full = False

    def Execute(self, arr):
        assert self.full is False
        lab, self.n = ndimage.label(arr, structure=FACE)
        return lab

    def GetObjectCount(self):
        return self.n


def _bbox(m):
    idx = np.nonzero(m != 0)
    return np.array([[int(i.min()) for i in idx], [int(i.max()) for i in idx]], dtype=np.int64)


def run_case(name, out):
    cid, img, lab = BC.case_inputs(name)
    sitk = types.SimpleNamespace(ConnectedComponentImageFilter=_CCA, GetImageFromArray=lambda a: a,
                                 GetArrayFromImage=lambda a: a)
    src_fun = G._ref_lines(FNAME, 37, 82)
    src_lab = G._ref_lines(FNAME, 148, 149)
    src_crop = G._ref_lines(FNAME, 157, 207)
    for marker in ("cca.FullyConnectedOff()", "for i in range(1, num_limit):", "structure=np.ones((2,2,2))",
                   "getmaxcomponent(CT_array, 100, min_filter=min_filter)", "(CT_nii_array > thre)",
                   "structure=np.ones((10,10,10))"):
        assert marker in src_fun, f"reference lines moved: {marker}"
    assert "label[label >= 14] = 0" in src_lab and "orilabelsum = label.sum()" in src_lab, "reference lines moved"
    for marker in ("image = image[:, :, xmin:xmax]", "if cid == 540 or cid == 518:", "maxcomponent = get_body(image, thre)",
                   "np.min(arr) - 3", "image_a.shape[2] // 2 + 10", "get_body(image_up, thre, min_filter=1e5)",
                   "np.min(arr) - 5", "if inter_all - inter_up > 30 and cid > 500:",
                   "maxcomponent = maxcomponent[zmin_up:zmax_up, :, :]"):
        assert marker in src_crop, f"reference lines moved: {marker}"
    msgs = []
    env = {"np": np, "sitk": sitk, "ndimage": ndimage, "cid": cid, "image": img.copy(), "label": lab.copy(),
           "print": lambda *a, **k: msgs.append(" ".join(str(v) for v in a))}
    exec(compile(src_fun, FNAME + ":37-82", "exec"), env)
    inner, calls = env["get_body"], []

    def get_body(*a, **k):
        n0 = len(msgs)
        r = inner(*a, **k)
        calls.append((np.asarray(r) != 0, int(any(m.startswith("Get max component failed") for m in msgs[n0:]))))
        return r

    env["get_body"] = get_body
    exec(compile(src_lab, FNAME + ":148-149", "exec"), env)
    exec(compile(src_crop, FNAME + ":157-207", "exec"), env)
    assert len(calls) == 2
    (m0, r0), (m1, r1) = calls
    hand = "find hand" in msgs
    assert (r0, r1, hand) == EXPECT[name], (name, r0, r1, hand)
    if name == "ct_fallback":
        assert cid <= 410 and env["thre"] == -200 and (lab >= 14).any()
        assert env["inter_all"] - env["inter_up"] <= 30 or cid <= 500
    image_a, label_a, mask = env["image_a"], env["label_a"], np.asarray(env["maxcomponent"]) != 0
    out[f"{name}_bbox"], out[f"{name}_bbox_up"] = _bbox(m0), _bbox(m1)
    out[f"{name}_size"], out[f"{name}_size_up"] = np.int64(m0.sum()), np.int64(m1.sum())
    out[f"{name}_route"], out[f"{name}_route_up"] = np.int64(r0), np.int64(r1)
    out[f"{name}_inter"] = np.array([env["inter_all"], env["inter_up"], int(hand)], dtype=np.int64)
    out[f"{name}_shapes"] = np.array([image_a.shape, label_a.shape, mask.shape], dtype=np.int64)
    out[f"{name}_mask_bits"] = np.packbits(mask)
    out[f"{name}_sums"] = np.array([np.nansum(image_a.astype(np.float64)), label_a.astype(np.float64).sum(),
                                    float(env["orilabelsum"])], dtype=np.float64)
    out[f"{name}_sha"] = np.array([BC.checksum(image_a), BC.checksum(label_a)])
    out[f"{name}_insum"] = np.array(BC.checksum(img, lab))
    print(name, "routes", r0, r1, "hand", hand, "sizes", int(m0.sum()), int(m1.sum()), "inter", env["inter_all"],
          env["inter_up"], "image_a", image_a.shape)


if __name__ == "__main__":
    out = {}
    for name in BC.FIXTURES:
        run_case(name, out)
    G.save("g21_body_crop.npz", **out)
