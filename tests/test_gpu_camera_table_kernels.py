"""The context's camera table (icg_set_cameras) in the indexed C entries: icg_lk_track_fb_cams (k_lk_finish with a camera per point) and
icg_reproj_error_batch_cams (k_reproj_error with a camera per pose).  Every comparison is for equality of bits, against the single-camera
entries of the same library and against the oracle's undistortion."""
import numpy as np
import pytest

import camera_table_utils as ct
import icgvins
import synth

pytestmark = pytest.mark.gpu

W, H = 640, 480
CAMS = ct.cameras()
TABLE = np.array([CAMS["base"], CAMS["wide"], CAMS["tele"], CAMS["skew"]], np.float64)  # entry 3 is never used below
N_MAX = 257


def bits(a):
    return np.ascontiguousarray(a).view(np.uint32)


@pytest.fixture(scope="module")
def lk_ctx():
    ctx = icgvins.Context(W, H, n_slots=2, max_batch=2, max_points=1024)
    a = synth.texture(W, H, seed=1)
    b = synth.shift_image(a, 2.25, -1.5)
    ctx.preprocess([0, 1], [a, b])
    ctx.sync()
    pts = synth.random_points(N_MAX, W, H, 10, seed=2)
    # a few points at the border, so that lost points and status 0 take part too
    pts[5] = [3.0, 200.0]
    pts[17] = [W - 2.0, 100.0]
    yield ctx, pts
    ctx.close()


@pytest.mark.parametrize("n", [1, 255, 256, 257])
def test_indexed_lk_epilogue(lk_ctx, oracle, n):
    """either side of k_lk_finish's 256-thread block; cam_idx interleaved 0, 2, 1, 0, ..."""
    ctx, all_pts = lk_ctx
    pts = all_pts[:n].copy()
    guess = pts + np.float32(0.5)
    idx = np.array([0, 2, 1], np.int32)[np.arange(n) % 3]
    ctx.set_cameras(TABLE)
    ctx.set_camera(TABLE[3])  # (the by-value camera must play no part in the indexed call)
    out, st, und, keep = ctx.lk_track_fb_cams(0, 1, pts, guess, idx, want_keep=True)
    r_out, r_st, r_und, r_keep = ctx.lk_track_fb(0, 1, pts, guess, want_undist=True, want_keep=True)
    assert np.array_equal(bits(out), bits(r_out)) and np.array_equal(st, r_st) and np.array_equal(keep, r_keep)
    if n > 100:
        assert st.any() and not st.all()  # tracked and lost points both take part
    for k in (0, 1, 2):
        sel = idx == k
        if not sel.any():
            continue
        ctx.set_camera(TABLE[k])
        exp = ctx.undistort(out)
        assert np.array_equal(bits(und[sel]), bits(exp[sel])), k
        finite = np.isfinite(out).all(axis=1) & sel
        assert np.array_equal(bits(und[finite]), bits(oracle.undistort(TABLE[k], out[finite]))), k
        # every index equal to k: the unindexed call under camera k
        o2, s2, u2 = ctx.lk_track_fb_cams(0, 1, pts, guess, np.full(n, k, np.int32))
        r2 = ctx.lk_track_fb(0, 1, pts, guess, want_undist=True)
        assert np.array_equal(bits(o2), bits(r2[0])) and np.array_equal(s2, r2[1]) and np.array_equal(bits(u2), bits(r2[2])), k
    if n >= 3:  # three cameras really differ on these points
        ctx.set_camera(TABLE[0])
        assert not np.array_equal(bits(und), bits(ctx.undistort(out)))


def _untouched(res, fill):
    rc, out, st, und, keep, nkeep = res
    return bool((out == fill).all() and (st == fill).all() and (und == fill).all() and (keep == fill).all() and (nkeep == fill).all())


def test_indexed_lk_argument_errors_launch_nothing(lk_ctx):
    ctx, all_pts = lk_ctx
    n = 20
    pts = all_pts[:n].copy()
    ctx.set_cameras(TABLE)
    ctx.set_camera(TABLE[0])
    ctx.prof_enable(True)
    try:
        ctx.lk_track_fb_cams(0, 1, pts, pts, np.zeros(n, np.int32))
        ctx.sync()
        before = ctx.prof()
        assert before["lk_finish"][0] == 1
        bad = np.zeros(n, np.int32)
        for what, idx in (("-1", -1), ("n_cams", len(TABLE))):
            bad[:] = 0
            bad[n - 1] = idx
            res = ctx.lk_track_fb_cams(0, 1, pts, pts, bad, want_keep=True, check=False, fill=7)
            assert res[0] == -1 and _untouched(res, 7), what
            assert ctx.prof() == before, what
        res = ctx.lk_track_fb_cams(0, 1, pts, pts, None, want_keep=True, check=False, fill=7)
        assert res[0] == -1 and _untouched(res, 7)
        assert ctx.prof() == before
    finally:
        ctx.prof_enable(False)
    # no table set: a fresh context
    c2 = icgvins.Context(W, H, n_slots=2, max_batch=2, max_points=1024)
    try:
        c2.set_camera(TABLE[0])
        c2.prof_enable(True)
        res = c2.lk_track_fb_cams(0, 1, pts, pts, np.zeros(n, np.int32), want_keep=True, check=False, fill=7)
        assert res[0] == -1 and _untouched(res, 7)
        assert b"icg_set_cameras" in c2.lib.icg_last_error(c2.h)
        assert c2.prof() == {}
        # icg_set_cameras itself
        import ctypes as C
        assert c2.lib.icg_set_cameras(c2.h, 0, TABLE.ctypes.data_as(C.c_void_p)) == -1
        assert c2.lib.icg_set_cameras(c2.h, 2, None) == -1
    finally:
        c2.close()


# ---- reprojection error -------------------------------------------------------------------------------------------------------------------
POSE_CAM = np.array([2, 0, 1, 0, 2], np.int32)


def _observations(seed=5):
    """five poses, 14 landmarks in front of them, ~40 observations interleaved over the poses; key points = the projection under the
    pose's OWN camera + noise from 0.3 to 8 px, two landmarks outside the depth gate"""
    import harness as HH
    rng = np.random.RandomState(seed)
    poses = np.stack([np.concatenate([HH._rot_yp(rng.normal(0, 0.05), rng.normal(0, 0.03)).ravel(), rng.normal(0, 0.5, 3)]) for _ in range(5)])
    depth = np.concatenate([rng.uniform(3, 60, 12), [0.6, 400.0]])
    xy = rng.uniform([-0.3, -0.2], [0.3, 0.2], (14, 2))
    pw = np.stack([xy[:, 0] * depth, xy[:, 1] * depth, depth], axis=1)
    pose_idx, lm_idx, pix = [], [], []
    for l in range(14):
        for k in rng.choice(5, 3 if l % 7 else 2, replace=False):
            fx, fy, cx, cy, skew = TABLE[POSE_CAM[k]][:5]
            R, t = poses[k, :9].reshape(3, 3), poses[k, 9:]
            pc = R.T @ (pw[l] - t)
            noise = rng.normal(0, 1, 2) * rng.choice([0.3, 1.2, 4.0, 8.0])
            pose_idx.append(k), lm_idx.append(l)
            pix.append([fx * pc[0] / pc[2] + skew * pc[1] / pc[2] + cx + noise[0], fy * pc[1] / pc[2] + cy + noise[1]])
    return (np.array(pose_idx, np.int32), np.array(lm_idx, np.int32), np.ascontiguousarray(poses), np.ascontiguousarray(pw),
            np.ascontiguousarray(pix, np.float32))


def test_indexed_reprojection_error():
    pose_idx, lm_idx, poses, pw, pix = _observations()
    n = len(pose_idx)
    assert 36 <= n <= 44
    ctx = icgvins.Context(W, H, n_slots=2, max_batch=2, max_points=1024)
    try:
        ctx.set_cameras(TABLE)
        ctx.set_camera(TABLE[3])
        err, good = ctx.reproj_error_batch_cams(pose_idx, lm_idx, poses, POSE_CAM, pw, pix, 4.5)
        assert good.any() and not good.all()
        for c in (0, 1, 2):
            sel = POSE_CAM[pose_idx] == c
            assert sel.any()
            ctx.set_camera(TABLE[c])
            e1, g1 = ctx.reproj_error_batch(pose_idx[sel], lm_idx[sel], poses, pw, pix[sel], 4.5)
            assert np.array_equal(err[sel].view(np.uint64), e1.view(np.uint64)) and np.array_equal(good[sel], g1), c
        ctx.set_camera(TABLE[0])  # the cameras matter: one camera for all gives other errors
        e0, _ = ctx.reproj_error_batch(pose_idx, lm_idx, poses, pw, pix, 4.5)
        assert not np.array_equal(e0, err)
        # argument errors launch nothing and leave the outputs alone
        ctx.prof_enable(True)
        ctx.reproj_error_batch_cams(pose_idx, lm_idx, poses, POSE_CAM, pw, pix, 4.5)
        ctx.sync()
        before = ctx.prof()
        assert before["reproj_error"][0] == 1
        for what, idx in (("-1", -1), ("n_cams", len(TABLE))):
            bad = POSE_CAM.copy()
            bad[4] = idx
            rc, e, g = ctx.reproj_error_batch_cams(pose_idx, lm_idx, poses, bad, pw, pix, 4.5, check=False, fill=9)
            assert rc == -1 and (e == 9).all() and (g == 9).all() and ctx.prof() == before, what
        rc, e, g = ctx.reproj_error_batch_cams(pose_idx, lm_idx, poses, None, pw, pix, 4.5, check=False, fill=9)
        assert rc == -1 and (e == 9).all() and (g == 9).all() and ctx.prof() == before
    finally:
        ctx.close()
    c2 = icgvins.Context(W, H, n_slots=2, max_batch=2, max_points=1024)
    try:
        c2.set_camera(TABLE[0])
        c2.prof_enable(True)
        rc, e, g = c2.reproj_error_batch_cams(pose_idx, lm_idx, poses, POSE_CAM, pw, pix, 4.5, check=False, fill=9)
        assert rc == -1 and (e == 9).all() and (g == 9).all() and c2.prof() == {}
        assert b"icg_set_cameras" in c2.lib.icg_last_error(c2.h)
    finally:
        c2.close()
