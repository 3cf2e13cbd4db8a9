"""The multi-label volumes of postproc_cases.py hold the properties the tests of u3d_ccl_keep_largest rely on, judged from
the scipy oracle alone (no device)."""
import numpy as np

import body_crop_cases as BK
import postproc_cases as K


def test_the_cases_hold_what_they_claim():
    """Properties of the inputs the GPU tests rely on, from the oracle alone."""
    c = K.cases()
    for name, (codes, _) in c.items():
        if name.startswith("checker"):
            out, rec = K.oracle(name)
            n1, n2 = int((codes == 1).sum()), int((codes == 2).sum())
            assert rec[0].tolist() == [n1, n1, 1, 0] and rec[1].tolist()[:3] == [n2, n2, int(n2 > 0)]   # no two voxels join
            assert (rec[2:] == [0, 0, 0, -1]).all()
    out, rec = K.oracle("tie")
    assert rec[3].tolist() == [3, 2 + 768 + 768, 768, (1 * 20 + 2) * 70 + 3]       # label 4: the earlier box of two
    assert rec[8].tolist() == [1, 5, 5, 10 * 20 * 70] and rec[0].tolist() == [0, 0, 0, -1]
    codes, _ = c["crossing"]
    out, rec = K.oracle("crossing")
    tz, ty, tx = BK.TILE
    kept = np.argwhere((out == 3))
    assert rec[2][0] == 4 and all(kept[:, a].max() // t - kept[:, a].min() // t == 2 for a, t in enumerate((tz, ty, tx)))
    for v in (14, 200, 255):
        assert np.array_equal(out == v, codes == v) and (codes == v).any()         # codes above num_labels come through
    out1, rec1 = K.oracle("crossing-one-label")
    assert rec1.shape == (1, 4) and np.array_equal(out1 != codes, (codes == 1) & (out1 == 0))
    for name in ("serpentine", "comb"):
        out, rec = K.oracle(f"{name}-{K.BIG}")
        assert rec[4].tolist()[0] == 1 and (rec[:, 0] > 1).sum() >= 10             # one path in code 5, noise around it
    assert not K.oracle("background")[0].any() and (K.oracle("background")[1] == [0, 0, 0, -1]).all()
