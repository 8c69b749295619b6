"""GPU parity of the lane-per-item FP64 kernels with the CPU oracle on the edge inputs of point_edge_data.py: k_undistort / k_distort /
k_predict_mappoints / k_predict_rotation (csrc/points.hip, dev_camera.h) with a skewed camera and one whose undistortion takes the
`icdist < 0` break, index tables that reach every entry, non-finite predictions; cam_undistort in the LK epilogue; k_reproj_error with
values exactly on its gates; k_triangulate_seg on degenerate ray pairs; k_ins_camera_pose on every branch of quat2rotvec / rotvec2quat and
k_ins_mechanize on series that stay at the angle 0.  Launch boundaries: 255 / 256 / 257 items for the point kernels, 63 / 64 / 65 for
triangulation and INS, max_points and max_points + 1.  test_oracle_point_edges.py proves on the CPU that the inputs reach those edges.
Kernels and oracle are built without FMA contraction and use only + - * / sqrt on the camera, gate and triangulation paths: those are
compared bit for bit (D.same_floats: same NaN positions, same bits elsewhere); the INS kernels call sin / cos / atan2 and hold 1e-12."""
import numpy as np
import pytest

import ins_utils as iu
import point_edge_data as D
from ctypes_util import ptr

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import icgvins
    c = icgvins.Context(D.W, D.H, n_slots=1, max_batch=1, max_points=D.MAX_POINTS)
    yield c
    c.close()


def _assert_same(got, exp, *what):
    bad = D.float_diff(got, exp)
    assert bad.size == 0, (*what, len(bad), bad[:8], got[bad[:8]], exp[bad[:8]])


# ---- 1. camera maps -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", list(D.CAMERAS))
def test_undistort_distort_bit_exact(oracle, ctx, name):
    import icgvins
    cam = D.CAMERAS[name]
    ctx.set_camera(cam)
    for pts in [D.point_set(n) for n in D.POINT_SIZES] + [D.strong_points()[:D.MAX_POINTS]]:
        _assert_same(ctx.undistort(pts), oracle.undistort(cam, pts), name, "undistort", len(pts))
        _assert_same(ctx.distort(pts), oracle.distort(cam, pts), name, "distort", len(pts))
    empty = np.zeros((0, 2), np.float32)
    assert ctx.undistort(empty).shape == (0, 2) and ctx.distort(empty).shape == (0, 2)
    sentinel = np.float32([[12.5, -7.0]])  # n = 0 with a real buffer: left as it is
    buf = sentinel.copy()
    assert ctx.lib.icg_undistort_points(ctx.h, 0, ptr(buf)) == 0 and ctx.lib.icg_distort_points(ctx.h, 0, ptr(buf)) == 0
    assert np.array_equal(buf, sentinel)
    over = D.point_set(D.MAX_POINTS + 1)
    for f in (ctx.undistort, ctx.distort):
        with pytest.raises(icgvins.IcgError, match="max_points"):
            f(over)


@pytest.mark.parametrize("name", list(D.CAMERAS))
def test_predict_mappoints_pose_table_and_nonfinite(oracle, ctx, name):
    import icgvins
    cam = D.CAMERAS[name]
    ctx.set_camera(cam)
    poses, idx, pw, _ = D.mappoint_case()
    _assert_same(ctx.predict_mappoints(pw, idx, poses), D.expected_mappoints(oracle, cam, poses, idx, pw), name, idx)
    bad = idx.copy()
    bad[100] = 5
    with pytest.raises(icgvins.IcgError, match="pose_idx"):
        ctx.predict_mappoints(pw, bad, poses)


@pytest.mark.parametrize("name", list(D.CAMERAS))
def test_predict_rotation_table_bit_exact(oracle, ctx, name):
    cam = D.CAMERAS[name]
    ctx.set_camera(cam)
    rots, idx, pts = D.rotation_case()
    _assert_same(ctx.predict_rotation(pts, idx, rots), D.expected_rotation(oracle, cam, rots, idx, pts), name, idx)


def test_lk_epilogue_undistorts_through_the_break_branch(oracle):
    import icgvins
    a, b, pts, guess = D.lk_case()
    c = icgvins.Context(D.LK_W, D.LK_H, n_slots=2, max_batch=2, max_points=128)
    try:
        c.set_camera(D.LK_CAM)
        c.preprocess([0, 1], [a, b])
        ca, cb = oracle.clahe(a), oracle.clahe(b)
        assert np.array_equal(c.download(0, 0), ca) and np.array_equal(c.download(1, 0), cb)
        exp_pts, exp_st = oracle.lk_track_fb(ca, cb, pts, guess)
        got_pts, got_st, got_und, keep = c.lk_track_fb(0, 1, pts, guess, want_undist=True, want_keep=True)
        assert np.array_equal(got_st, exp_st) and np.array_equal(keep, np.nonzero(exp_st)[0])
        _assert_same(got_pts, exp_pts, "lk points")
        _assert_same(got_und, oracle.undistort(D.LK_CAM, exp_pts), "lk undistorted")
    finally:
        c.close()


# ---- 2. reprojection gate -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [255, 256, 257])
def test_reproj_error_on_its_gates(oracle, ctx, n):
    import icgvins
    d = D.reproj_case(n)
    ctx.set_camera(d["cam"])
    for max_error in D.MAX_ERRORS:
        exp_err, exp_good = D.oracle_reproj(oracle, d, max_error)
        err, good = ctx.reproj_error_batch(d["pose_idx"], d["lm_idx"], d["poses12"], d["pw"], d["pix"], max_error, D.MIN_DEPTH, D.MAX_DEPTH)
        assert np.array_equal(good, exp_good), (max_error, np.nonzero(good != exp_good)[0][:8], {k: (good[i], exp_good[i]) for k, i in d["where"].items()})
        fin = np.isfinite(exp_err)
        assert np.array_equal(np.isfinite(err), fin) and D.same_floats(err[~fin], exp_err[~fin])
        assert np.abs(err[fin] - exp_err[fin]).max() <= 1e-15 * np.abs(exp_err[fin]).max()
        w = d["where"]
        assert err[w["err_5"]] == 5.0 and err[w["z_min"]] == 0.0
    for which, at in (("pose_idx", 6), ("lm_idx", 40)):
        bad = {k: d[k].copy() for k in ("pose_idx", "lm_idx")}
        bad[which][n - 1] = at
        with pytest.raises(icgvins.IcgError, match="out of range"):
            ctx.reproj_error_batch(bad["pose_idx"], bad["lm_idx"], d["poses12"], d["pw"], d["pix"], 5.0)


# ---- 3. triangulation ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", D.TRI_SIZES)
def test_triangulate_degenerate_rays(oracle, ctx, n):
    P = D.tri_poses()
    i0, i1, pc0, pc1, cls, _ = D.tri_case(n)
    got = ctx.triangulate(i0, i1, P, pc0, pc1)
    exp = D.oracle_triangulate(oracle, P, i0, i1, pc0, pc1)
    bad = D.float_diff(got, exp)
    assert bad.size == 0, (len(bad), bad[:8], [D.TRI_CLASSES[k] for k in cls[bad[:8]]], got[bad[:8]], exp[bad[:8]])


def test_triangulate_invalid_arguments(ctx):
    import icgvins
    P = D.tri_poses()
    i0, i1, pc0, pc1, _, _ = D.tri_case(65)
    for which, at in ((0, 6), (1, -1)):
        idx = [i0.copy(), i1.copy()]
        idx[which][64] = at
        with pytest.raises(icgvins.IcgError, match="out of range"):
            ctx.triangulate(idx[0], idx[1], P, pc0, pc1)
    m = D.MAX_POINTS + 1
    with pytest.raises(icgvins.IcgError, match="max_points"):
        ctx.triangulate(np.resize(i0, m), np.resize(i1, m), P, np.resize(pc0, (m, 3)), np.resize(pc1, (m, 3)))


# ---- 4. INS -------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [63, 64, 65])
def test_ins_camera_pose_bracket_classes(oracle, ctx, n):
    orc = iu.OrcMisc(oracle.lib)
    pbc = iu.pose_b_c()
    br, interp, times, cls = D.bracket_case(n)
    out = ctx.ins_camera_pose_batch(br, interp, pbc, times)
    for i in range(n):
        e = D.oracle_bracket_pose(orc, br[i], interp[i], pbc, times[i])
        assert np.abs(out[i] - e).max() < 1e-12 * max(1.0, np.abs(e).max()), (i, D.BRACKET_CLASSES[cls[i]], interp[i], times[i] - br[i, 0], out[i], e)


def _colscale(e):
    return np.maximum(np.abs(e).reshape(-1, e.shape[-1]).max(axis=0), 1e-3)


@pytest.mark.parametrize("n_streams", [63, 64, 65])
def test_ins_mechanize_still_and_moving_series(oracle, ctx, n_streams):
    orc = iu.OrcMisc(oracle.lib)
    imus, states, still = D.mech_case(n_streams)
    lens = [len(i) for i in imus]
    off = np.concatenate([[0], np.cumsum(lens)]).astype(np.int32)
    for earth in (False, True):
        cfg = iu.make_cfg(earth, False)
        st, traj = ctx.ins_mechanize_batch(off, np.concatenate(imus), cfg, states)
        for s, n in enumerate(lens):
            if n == 0:
                assert np.array_equal(st[s], states[s]), s
                continue
            e_st, e_tr = orc.mechanize(cfg, imus[s], states[s])
            assert np.array_equal(traj[off[s]], states[s]), s
            got_tr = traj[off[s] + 1:off[s + 1]]
            if still[s] and not earth:  # sin(0), cos(0) and sqrt(1) only: the attitude comes back as it went in, the rest equals the oracle's bits
                assert np.array_equal(st[s, 4:8], states[s, 4:8]) and (got_tr[:, 4:8] == states[s, 4:8]).all(), s
                assert D.same_floats(st[s], e_st) and (n == 1 or D.same_floats(got_tr, e_tr)), (s, st[s], e_st)
            else:
                assert (np.abs(st[s] - e_st) / _colscale(e_st[None, :])).max() < 1e-12, (s, still[s], earth)
                if n > 1:
                    assert (np.abs(got_tr - e_tr) / _colscale(e_tr)).max() < 1e-12, (s, still[s], earth)
