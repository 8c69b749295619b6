"""The preprocessing kernels (csrc/image.hip: k_hist256, k_clahe_lut, k_clahe_apply, k_pyrdown_rows) against the oracle, byte for byte on every
pyramid level, at the cases of tests/preprocess_edge_data.py: planted clip excesses, rounding ties, every tile shape of the LUT kernel, every
form of the apply kernel, the padding rule, and the strip and band boundaries of the pyrDown row stream.  What each case reaches is asserted on
the CPU (tests/test_oracle_preprocess_edges.py), where the oracle is also pinned to a numpy restatement at the same inputs.  No tolerances."""
import numpy as np
import pytest

import preprocess_edge_data as pe

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def context_of():
    """one context per image size, shared by that size's contents (the cases come grouped by size)"""
    import icgvins
    held = {}

    def get(w, h):
        if (w, h) not in held:
            for c in held.values():
                c.close()
            held.clear()
            held[(w, h)] = icgvins.Context(w, h, n_slots=1, max_batch=1, max_points=64)
        return held[(w, h)]

    yield get
    for c in held.values():
        c.close()


@pytest.mark.parametrize("case", pe.CASES, ids=pe.case_id)
def test_preprocess_matches_the_oracle(oracle, context_of, case):
    w, h, _ = case
    img = pe.make(*case)
    c = context_of(w, h)
    mean = c.preprocess([0], [img], want_hist=True)
    sizes = pe.level_sizes(w, h)
    assert c.levels() == len(sizes), case
    exp = oracle.clahe(img)
    for level, (lw, lh) in enumerate(sizes):
        if level:
            exp = oracle.pyrdown(exp)
        got = c.download(0, level)
        assert got.shape == exp.shape == (lh, lw), (case, level)
        bad = np.argwhere(got != exp)
        assert bad.size == 0, (case, level, len(bad), bad[:8].tolist())
    assert mean[0] == oracle.histogram_mean(img), case
