"""The fp64 restatement of the deep-supervision loss (tests/deepsup_reference.py) against the reference's own outputs
(G16, cases A-D of tests/deepsup_cases.py). Value rtol 1e-5, gradients rtol 1e-4 with atol 1e-6 * max|ref|: the fp32
reference's own rounding (the figures test_gpu_parity.py uses for the G4 loss rows)."""
import numpy as np
import pytest
import torch

import deepsup_cases as DC
import deepsup_reference as DR
from conftest import golden


@pytest.fixture(scope="module")
def g16():
    return golden("g16_deepsup.npz")


def _run(inp, mask=None):
    w = (inp["mask"] if mask is None else mask)[:DC.C].astype(np.float64)
    return DR.deepsup_loss([torch.from_numpy(d) for d in inp["deep"]], torch.from_numpy(inp["labels"]), w)


def _close(got, ref, what):
    ref = np.asarray(ref, np.float64)
    np.testing.assert_allclose(got.numpy(), ref, rtol=1e-4, atol=1e-6 * np.abs(ref).max(), err_msg=what)


@pytest.mark.parametrize("tag", ["A", "B", "D"])
def test_inputs_rebuild_to_the_generators(g16, tag):
    np.testing.assert_allclose(DC.checksum(DC.case_inputs(tag)), float(g16[f"{tag}_insum"]), rtol=1e-12)


def test_nearest_index_is_torchs():
    assert DR.nearest_index(3, 20).tolist() == [0, 6, 13]
    assert DR.nearest_index(7, 20).tolist() == [0, 2, 5, 8, 11, 14, 17]
    for out, inn in ((3, 20), (7, 12), (5, 10), (10, 10), (2, 16), (6, 16), (11, 13)):
        ref = torch.nn.functional.interpolate(torch.arange(inn).float().reshape(1, 1, inn, 1, 1), (out, 1, 1),
                                              mode="nearest").reshape(-1)
        assert DR.nearest_index(out, inn).tolist() == ref.long().tolist(), (out, inn)


@pytest.mark.parametrize("tag", ["A", "B"])
def test_restatement_vs_reference_consistency_cases(g16, tag):
    """A / B: the deep term the reference's get_loss added (value: its own blocks per level; gradients: get_loss's)."""
    loss, levels, grads = _run(DC.case_inputs(tag))
    np.testing.assert_allclose(loss.item(), float(g16[f"{tag}_deep_value"]), rtol=1e-5)
    np.testing.assert_allclose([v.item() for v in levels], g16[f"{tag}_levels"], rtol=1e-5)
    # the deep term is what deep_out adds to get_loss (fp32 sums of O(3) values: 1e-6 of the total)
    added = float(g16[f"{tag}_value"]) - float(g16[f"{tag}_value_nodeep"])
    assert abs(loss.item() - added) < 2e-6 * float(g16[f"{tag}_value"])
    assert len(grads) == len(DC.GEOM[tag][1])
    for i, gr in enumerate(grads):
        _close(gr, g16[f"{tag}_ddeep{i}"], f"{tag} level {i}")


def test_pretrain_branch_discards_the_deep_term(g16):
    """C: the reference returns dice_loss alone with deep_out given, and the deep maps get no gradient."""
    assert float(g16["C_value"]) == float(g16["C_value_nodeep"])
    assert g16["C_deep_grad_none"].tolist() == [1, 1, 1]


def test_restatement_vs_reference_batch2(g16):
    inp = DC.case_inputs("D")
    loss, levels, grads = _run(inp)
    np.testing.assert_allclose(loss.item(), float(g16["D_value"]), rtol=1e-5)
    np.testing.assert_allclose([v.item() for v in levels], g16["D_levels"], rtol=1e-5)
    for i, gr in enumerate(grads):
        _close(gr, g16[f"D_ddeep{i}"], f"D level {i}")
    # the vanishing class: in the target, in no level's resized target
    lab = torch.from_numpy(inp["labels"])
    assert (lab == DC.VANISHING).any()
    for lv in DC.GEOM["D"][1]:
        assert not (DR.nearest_target(lab, lv) == DC.VANISHING).any()
    loss0, _, grads0 = _run(inp, mask=np.zeros(15, np.int64))
    assert loss0.item() == 0.0 == float(g16["Dzero_value"])
    for i, gr in enumerate(grads0):
        assert gr.abs().max().item() == 0.0 and np.abs(g16[f"Dzero_ddeep{i}"]).max() == 0.0
