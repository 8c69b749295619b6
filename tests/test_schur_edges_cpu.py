"""The Schur-path edge suite on the CPU: every case of schur_edge_data.py is where it claims to be (expected_plan restates what the host derives
for k_asm_runs / k_asm_camera / k_asm_landmarks / k_schur_reduce_w), and the check bodies of schur_edge_checks.py pass on the oracle shim — the
shim's double-precision elimination against the long-double reference formed from the shim's own r and J, per cell, within the derived bound
(n_t + 8) 2^-53 A.  test_gpu_schur_edges.py runs the same bodies on the HIP library."""
import numpy as np
import pytest

import schur_edge_checks as K
import schur_edge_data as D


@pytest.fixture(scope="module")
def shim():
    import icgvins
    from stream_utils import ensure_oracle_host
    lib = icgvins.load_library(ensure_oracle_host())
    return lambda: icgvins.Context(640, 480, n_slots=1, max_batch=1, max_points=64, lib=lib)


@pytest.fixture(scope="module")
def ctx(shim):
    c = shim()
    yield c
    c.close()


# ---- the plan assertions (shared with the GPU file) ----------------------------------------------------------------------------------------
def assert_width_plan(case, NT, wgs, LT):
    p = D.expected_plan(case)
    P = case["P"]
    assert p["TQ"] == (P + 3) // 4 and p["NT"] == p["TQ"] * (p["TQ"] + 1) // 2
    assert NT is None or p["NT"] == NT, (case["name"], p["NT"])
    assert wgs is None or p["reduce_workgroups"] == wgs, (case["name"], p["reduce_workgroups"])
    assert p["red_LT"] == LT, (case["name"], p["red_LT"])
    assert sum(n for _, n in p["gap_runs"]) <= 5 and p["K"] == case["n_poses"]  # full blocks, at most five spare columns
    if P > 256:
        assert p["owner"][256] is not None  # the second accs slot holds data
    return p


def assert_landmark_row_plan(case, LB, LB_min):
    p = D.expected_plan(case)
    launch = D.expected_launch([case])
    assert LB is None or launch["LB"] == LB, (case["name"], launch["LB"], p["NB"])
    assert LB_min is None or launch["LB"] >= LB_min, (case["name"], launch["LB"])
    assert launch["NBmax"] <= 256
    nm = case["name"]
    if nm == "LB1":
        assert p["NB"] >= 129 and case["n_poses"] == 65
    if nm == "LB2":
        assert case["n_poses"] == 33 and all(n == 9 for _, n in p["gap_runs"]) and case["P"] == 33 * 15 + 7
    if nm == "long_landmark":
        assert p["factors_per_landmark"].max() > D.ASML_FB and p["factors_per_landmark"].max() >= 65
    if nm == "gaps":
        assert sorted(n for _, n in p["gap_runs"]) == [1, 6, 7, 13] and p["gap_runs"][0][0] == 0
        assert case["col_pose"][2] == -1 and 2 in set(case["idx_i"]) | set(case["idx_j"])  # a constant pose in the middle, used by factors
        assert 0 <= case["col_td"] < case["P"] - 1  # a td column that is not the last column
    if nm == "td_first":
        assert case["col_td"] == 0
    if nm == "no_td":
        assert case["col_td"] == -1 and case["col_ext"] >= 0
    if nm == "no_ext":
        assert case["col_ext"] == -1 and case["col_td"] >= 0
    if nm == "no_ext_no_td":
        assert case["col_ext"] == -1 and case["col_td"] == -1
    return p


def assert_run_plans(cases):
    by = {c["name"]: (c, D.expected_plan(c)) for c in cases}
    c, p = by["run_lengths"]
    assert {1, 15, 16, 17, 32, 33} <= set(p["run_lengths"]) and p["n_runs"] % 4 != 0
    assert (0, 1) in p["runs"] and (1, 0) in p["runs"] and (1, 2) in p["runs"] and (2, 1) in p["runs"]
    act = c["active"].astype(bool)
    pair = np.stack([c["idx_i"], c["idx_j"]], axis=1)
    dead = (pair == (4, 0)).all(1)
    assert dead.sum() == p["runs"][(4, 0)] and not act[dead].any()  # a run with every factor inactive
    run = act[(pair == (3, 2)).all(1)]  # (list order inside a run is kept by the plan)
    assert len(run) == 33 and run[0] and not run[5:9].any() and run[9:20].all() and not run[20] and run[15]  # holes inside a pass of 16
    assert [by[f"K{K_}"][1]["K"] for K_ in (2, 3, 4, 5, 8, 9)] == [2, 3, 4, 5, 8, 9]
    for n in (7, 8, 9):
        c, p = by[f"nruns{n}"]
        assert p["n_runs"] == n and c["col_ext"] >= 0 and c["col_td"] >= 0


def assert_determinism_batch(cases):
    launch = D.expected_launch(cases)
    p0 = launch["plans"][0]
    assert p0["K"] < launch["Kmax"] and p0["NB"] < launch["NBmax"], (p0["K"], launch["Kmax"], p0["NB"], launch["NBmax"])
    assert p0["reduce_workgroups"] == 2 and p0["red_LT"] == 30 and cases[0]["L"] > 30
    return launch


# ---- the cases -----------------------------------------------------------------------------------------------------------------------------
WIDTH = D.width_cases()


@pytest.mark.parametrize("k", range(len(WIDTH)), ids=[w[0]["name"] for w in WIDTH])
def test_reduction_width(ctx, k):
    case, NT, wgs, LT = WIDTH[k]
    assert_width_plan(case, NT, wgs, LT)
    K.check_case(ctx, case, device=False)


def test_reduction_width_covers_every_branch():
    names = {w[0]["name"] for w in WIDTH}
    for P, LT in ((96, 32), (97, 30), (509, 6), (510, 6), (511, 6), (512, 6)):
        for L in (LT - 1, LT, LT + 1, 2 * LT + 1):
            assert f"width_P{P}_L{L}" in names
    assert {D.expected_plan(w[0])["red_LT"] for w in WIDTH if w[0]["P"] in (255, 256, 257)} == {12, 11}
    assert {w[0]["P"] % 4 for w in WIDTH if w[0]["P"] > 500} == {0, 1, 2, 3}


def test_wider_than_the_limit(ctx):
    """the shim has no width limit: the 513-column window is an ordinary case here (the HIP library refuses it, test_gpu_schur_edges.py)"""
    case = D.over_limit_case()
    assert case["P"] == 513 == D.P_LIMIT + 1
    K.check_case(ctx, case, device=False)
    K.check_case(ctx, WIDTH[0][0], device=False)


def test_landmark_counts(ctx, shim):
    one, holes = D.landmark_count_cases()
    assert one["L"] == 1
    p = D.expected_plan(holes)
    assert p["factors_per_landmark"][2] == 0 and p["factors_per_landmark"][5] > 0 and not holes["active"][holes["idx_lm"] == 5].any()
    K.check_case(ctx, one, device=False)
    st = {}
    K.check_case(ctx, holes, device=False, stats=st)
    dead = set(range(holes["L"])) - set(holes["idx_lm"][holes["active"] == 1].tolist())
    assert {2, 5} <= dead and st["inv_zero"] == len(dead)  # the landmark without factors, the one whose factors are all inactive
    batch = D.empty_window_batch()
    assert batch[1]["L"] == 0 and len(batch[1]["idx_i"]) == 0 and batch[0]["L"] > 0 and batch[2]["L"] > 0
    K.check_batch(shim, batch, device=False)


def test_runs(ctx):
    cases = D.run_cases()
    assert_run_plans(cases)
    for c in cases:
        K.check_case(ctx, c, device=False)


ROWS = D.landmark_row_cases()


@pytest.mark.parametrize("k", range(len(ROWS)), ids=[w[0]["name"] for w in ROWS])
def test_landmark_rows(ctx, k):
    case, LB, LB_min = ROWS[k]
    assert_landmark_row_plan(case, LB, LB_min)
    K.check_case(ctx, case, device=False)


def test_clamps(ctx, shim):
    """the reference takes each of the three clamp branches (h < min_diag, inside, h > max_diag) for at least one landmark with h > 0, through
    icg_reproj_schur and through icg_reproj_schur_windows, and a landmark without factors stays at inv = 0"""
    (case,) = D.clamp_cases()
    assert case["damps"] == (0.0, 1e-4, 3.0)
    st = {}
    K.check_case(ctx, case, device=False, stats=st)
    assert st["branches"] == {-1, 0, 1, 2}, st["branches"]
    st = {}
    K.check_batch(shim, D.clamp_batch(), device=False, damp1=[1e-4, 3.0], damp2=[3.0, 0.0], stats=st)
    assert {0, 1, 2} <= st["branches"], st["branches"]


def test_batches(shim):
    det = D.determinism_batch()
    assert_determinism_batch(det)
    K.check_batch(shim, det, device=False)
    wide = D.wide_batch()
    assert all(c["P"] == 257 for c in wide)
    K.check_batch(shim, wide, device=False)


COUNTS = D.count_cases()


@pytest.mark.parametrize("huber", [0.0, 1.5])
def test_cost_and_chi2_counts(ctx, huber):
    assert [len(c["idx_i"]) for c in COUNTS] == [1, 255, 256, 257, 513]
    outl = inl = 0
    for c in COUNTS:
        c = dict(c, huber=huber)
        st = {}
        K.check_case(ctx, c, device=False, stats=st)
        outl, inl = outl + st["huber_outliers"], inl + st["huber_inliers"]
        seen = K.check_chi2(ctx, c)
        assert (True, True) in seen and (False, False) in seen  # a threshold above the maximum, one below the minimum
        assert len(c["idx_i"]) == 1 or (False, True) in seen  # one in the middle
    assert (outl > 0 and inl > 0) if huber > 0 else outl == 0  # with Huber on both branches are taken
