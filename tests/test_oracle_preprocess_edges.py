"""The oracle's CLAHE and pyrDown against the numpy restatement of SURVEY.md B.2 / B.3 at the preprocessing edge cases
(tests/preprocess_edge_data.py), and the conditions those cases exist for: which clip outcomes, rounding ties, kernel paths and strip / band
shapes they reach.  The conditions are computed from the restatement and the Python mirror of the launch geometry, never from the kernels."""
import numpy as np
import pytest

import preprocess_edge_data as pe


@pytest.mark.parametrize("case", pe.CASES, ids=pe.case_id)
def test_oracle_matches_the_restatement(oracle, case):
    img, luts, levels = pe.restate(case)
    got, lut = oracle.clahe(img, want_lut=True)
    bad = np.argwhere(lut.reshape(pe.T, pe.T, 256) != luts)
    assert bad.size == 0, (case, "lut", len(bad), bad[:8])
    for level, exp in enumerate(levels):
        assert got.shape == exp.shape, (case, level)
        bad = np.argwhere(got != exp)
        assert bad.size == 0, (case, level, len(bad), bad[:8])
        if level + 1 < len(levels):
            got = oracle.pyrdown(got)


def test_cases_reach_the_edges():
    S = {case: pe.summary(case) for case in pe.CASES}

    # clip outcomes
    pairs = set().union(*(s["pairs"] for s in S.values()))
    assert any(s["unclipped"] for s in S.values())
    assert (1, 0) in pairs and any(b >= 2 and r == 0 for b, r in pairs), sorted(pairs)[:40]
    residuals = {r for _, r in pairs}
    assert {1, 2, 3, 85, 86, 127, 128, 129, 255} <= residuals, sorted(residuals)
    assert any(s["bin_at_clip"] for s in S.values()) and any(s["bin_over_by_one"] for s in S.values())
    # wave positions: every bin is, in some tile, the only one over the limit
    lone = set().union(*(s["lone_bins"] for s in S.values()))
    assert lone == set(range(256)), sorted(set(range(256)) - lone)

    # rounding ties, both parities
    lut_even, lut_odd = (sum(s["lut_ties"][i] for s in S.values()) for i in (0, 1))
    app_even, app_odd = (sum(s["apply_ties"][i] for s in S.values()) for i in (0, 1))
    assert lut_even >= 1000 and lut_odd >= 1000, (lut_even, lut_odd)
    assert app_even >= 1000 and app_odd >= 1000, (app_even, app_odd)
    # the two sizes chosen for their ties deliver them on their own
    assert min(S[(630, 357, "texture")]["lut_ties"]) >= 1000 and min(S[(672, 336, "texture")]["apply_ties"]) >= 1000
    # the range the float form's magic-constant rounding relies on
    assert max(s["res_max"] for s in S.values()) <= 255.0 and min(s["res_min"] for s in S.values()) >= 0.0

    # k_clahe_lut shapes
    tiles = [t for w, h in pe.SIZES for t in pe.tile_shapes(w, h)]
    assert any(t["fast"] for t in tiles)
    for why in ("nin>16", "bottom", "right", "nin<1"):
        assert any(t["why"] == {why} for t in tiles), why
    assert {1, 2} <= {t["ndw"] for t in tiles} and {1, 16, 17} <= {t["nin"] for t in tiles}
    assert any(t["nin"] == 16 and t["fast"] for t in tiles)
    assert {t["phase"] for t in tiles} == {0, 1, 2, 3}
    # all four phases with neighbours that differ, in one image (651 x 483: tw = 31)
    assert {t["phase"] for t in pe.tile_shapes(651, 483)} == {0, 1, 2, 3}
    ths = {pe.padded_geometry(w, h)[1] for w, h in pe.SIZES}
    assert any(th < 4 for th in ths) and any(4 <= th <= 16 for th in ths) and any(th > 16 for th in ths), ths
    assert any(pe.clip_limit(*pe.padded_geometry(w, h)[:2]) == 1 for w, h in pe.SIZES)
    # the padding rule with one divisible dimension: the divisible one gets a whole extra tile
    assert pe.padded_geometry(672, 100) == (33, 5, True) and pe.padded_geometry(100, 336) == (5, 17, True)
    assert pe.padded_geometry(672, 336) == (32, 16, False)

    # k_clahe_apply forms
    forms = {f for w, h in pe.SIZES for f in pe.apply_forms(w, h)}
    assert forms == {(True, True), (True, False), (False, True), (False, False)}, forms
    assert all(pe.strip_rows_fit(w, h) for w, h in pe.SIZES)

    # pyrDown
    steps = [s for w, h in pe.SIZES for s in pe.pyr_steps(w, h)]
    later = [e for s in steps for e in s["edge"][1:]]
    assert True in later and False in later
    for level in (0, 1):
        assert {s["sw"] % 4 for s in steps if s["level"] == level} == {0, 1, 2, 3}, level
    assert {(s["band_rows"], s["partial"]) for s in steps} == {(b, p) for b in (8, 16, 32) for p in (False, True)}
    assert {s["sh"] % 2 for s in steps} == {0, 1}
    # the predicate's flip and the band switches are straddled
    by_sw = {s["sw"]: s for s in steps if s["level"] == 0}
    assert by_sw[515]["edge"] == [True, True, True] and by_sw[516]["edge"] == [True, False, True]
    # the predicate is never false where a tap is reflected, and a full strip other than the first reflects (its last column's tap 2 x + 2
    # is the first column past the row: only there does the predicate's margin matter), at level 0 and at level 1
    assert all(e or not n for s in steps for e, n in zip(s["edge"], s["needs"]))
    for level in (0, 1):
        assert any(s["level"] == level and s["sw"] == 2 * k * pe.STRIP_OUT and s["needs"][k - 1] for s in steps for k in range(2, s["n_strips"] + 1)), level
    assert any(s["level"] == 1 and s["sw"] == 515 for s in steps) and any(s["level"] == 1 and s["sw"] == 516 for s in steps)
    assert {127, 128, 129, 255, 256, 257} <= {s["dh"] for s in steps}
    saturated = set().union(*(s["saturated"] for s in S.values()))
    assert saturated == {"interior", "left", "right", "top", "bottom"}, saturated
