"""GPU: icg_reproj_landmark_min_windows (csrc/reproj_schur.hip, k_lm_min_w: one wave per window) against the rule that defines it — the
host loop of MarginalizationBatch's first guard — applied to what icg_reproj_landmark_diag_windows reads back from the same resident
systems.  The partition covers the wave boundary (63, 64, 65 landmarks), a window of one landmark, one of 300 (five passes per lane) and
one without landmarks; at P = 7 and P = 67; all windows in one call and each window alone.  Equal as values (==): the diagonals here are
finite and positive, so no NaN is provoked on the device — the NaN, tie and signed-zero behaviour of the rule is pinned on its host twin in
test_landmark_min_cpu.py."""
import numpy as np
import pytest

import reproj_data as rd

pytestmark = pytest.mark.gpu

N_KF = 10
LANDMARKS = [1, 63, 64, 65, 300, 0]
FILL = -7.0


def host_rule(h):
    """mn = h[first]; mn = (x < mn) ? x : mn in landmark order; 0.0 without landmarks"""
    if len(h) == 0:
        return 0.0
    mn = h[0]
    for x in h:
        mn = x if x < mn else mn
    return mn


@pytest.fixture(scope="module")
def windows():
    wins = []
    for k, L in enumerate(LANDMARKS):
        if L == 0:
            ref = wins[0]
            wins.append(dict(obs_soa=np.zeros((15, 0)), idx_i=np.zeros(0, np.int32), idx_j=np.zeros(0, np.int32), idx_lm=np.zeros(0, np.int32),
                             poses=ref["poses"], ext=ref["ext"], invdepth=np.zeros(0), td=ref["td"]))
        else:
            wins.append(rd.make_window(L, N_KF, seed=40 + k, pixel_noise=1.0))
    # the smallest diagonal of the 64- and the 65-landmark window goes to the last landmark: lane 63, and lane 0's second pass
    # (h_ll of a landmark depends on its own factors only, so relabelling two landmarks swaps their diagonals; the test checks where it lies)
    for L, a in ((64, 20), (65, 50)):
        w = wins[LANDMARKS.index(L)]
        lab = w["idx_lm"].copy()
        w["idx_lm"][lab == a], w["idx_lm"][lab == L - 1] = L - 1, a
        w["invdepth"][[a, L - 1]] = w["invdepth"][[L - 1, a]]
    return wins


def columns(P, W):
    """P = 67: every pose, the extrinsic and td are free; P = 7: the last pose and td"""
    col_pose = np.full((W, N_KF), -1, np.int32)
    if P == 67:
        col_pose[:] = 6 * np.arange(N_KF)
        return col_pose.ravel(), np.full(W, 60, np.int32), np.full(W, 66, np.int32)
    col_pose[:, N_KF - 1] = 0
    return col_pose.ravel(), np.full(W, -1, np.int32), np.full(W, 6, np.int32)


def make_ctx():
    import icgvins
    return icgvins.Context(64, 64, n_slots=1, max_batch=1, max_points=64)


def resident_systems(ctx, wins, P):
    """the partition of `wins`, evaluated and reduced: -> the landmark offsets"""
    W = len(wins)
    lm_off = np.concatenate([[0], np.cumsum([len(w["invdepth"]) for w in wins])]).astype(np.int32)
    fac_off = np.concatenate([[0], np.cumsum([w["obs_soa"].shape[1] for w in wins])]).astype(np.int32)
    ctx.reproj_set_factors(np.concatenate([w["obs_soa"] for w in wins], axis=1), np.concatenate([w["idx_i"] + N_KF * k for k, w in enumerate(wins)]),
                           np.concatenate([w["idx_j"] + N_KF * k for k, w in enumerate(wins)]), np.concatenate([w["idx_lm"] + lm_off[k] for k, w in enumerate(wins)]))
    ctx.reproj_set_windows(fac_off, lm_off)
    return lm_off


def reduce_all(ctx, wins, P):
    ctx.reproj_eval_windows(np.concatenate([w["poses"] for w in wins]), np.stack([w["ext"] for w in wins]), np.concatenate([w["invdepth"] for w in wins]),
                            np.array([w["td"] for w in wins]), huber=1.0)
    ctx.reproj_schur_windows(P, *columns(P, len(wins)), damp=np.zeros(len(wins)), min_diag=0.0, max_diag=0.0)


def device_and_rule(wins, P):
    ctx = make_ctx()
    try:
        lm_off = resident_systems(ctx, wins, P)
        reduce_all(ctx, wins, P)
        h = ctx.reproj_landmark_diag_windows(max(int(lm_off[-1]), 1))
        got = ctx.reproj_landmark_min_windows()
    finally:
        ctx.close()
    return got, np.array([host_rule(h[lm_off[k]:lm_off[k + 1]]) for k in range(len(wins))]), h, lm_off


@pytest.mark.parametrize("P", [7, 67])
def test_minimum_per_window_equals_the_host_rule_in_one_call_and_alone(windows, P):
    got, exp, h, lm_off = device_and_rule(windows, P)
    assert np.isfinite(h[:lm_off[-1]]).all() and (h[:lm_off[-1]] > 0).all()  # (nothing degenerate is fed to the device here)
    assert got.shape == (len(windows),)
    for k, L in enumerate(LANDMARKS):
        assert got[k] == exp[k], (P, k, L, got[k], exp[k])
    assert got[LANDMARKS.index(0)] == 0.0
    assert len(set(exp)) == len(exp)  # (the windows are different problems: a result in the wrong slot would show)
    # the minimum is not at a fixed place: in the long window it lies beyond the first pass of the lanes or the test shows little
    where = {L: int(np.argmin(h[lm_off[k]:lm_off[k + 1]])) for k, L in enumerate(LANDMARKS) if L > 1}
    assert where[300] >= 64 and where[64] == 63 and where[65] == 64, where
    for k, L in enumerate(LANDMARKS):
        if L == 0:
            continue  # (a partition of one window without a factor has no resident factors at all)
        one, one_exp, _, _ = device_and_rule([windows[k]], P)
        assert one[0] == one_exp[0] == got[k], (P, k, L)


def test_refused_before_a_partition_and_before_a_schur_call(windows):
    ctx = make_ctx()
    try:
        out = np.full(len(windows), FILL)
        assert ctx.reproj_landmark_min_windows_raw(out) == -1 and (out == FILL).all()  # ICG_ERR_INVALID: no partition
        resident_systems(ctx, windows, 7)
        assert ctx.reproj_landmark_min_windows_raw(out) == -1 and (out == FILL).all()  # a partition, no resident window systems
        assert b"no resident window systems" in ctx.lib.icg_last_error(ctx.h)
        reduce_all(ctx, windows, 7)
        assert ctx.reproj_landmark_min_windows_raw(out) == 0 and (out != FILL).all()
    finally:
        ctx.close()
