"""CPU side of the point-kernel edge pass (point_edge_data.py): for each case family the oracle against an independent restatement, and
proof from the oracle alone that the cases reach the edges they are named for (the undistortion break branch at each iteration, NaN / inf /
negative-depth predictions, values exactly on the depth and error gates, every triangulation ray class, every bracket class of the INS
pose prior, the angle-0 branch of the mechanization), so that a later change of the data cannot empty test_gpu_point_edges.py silently."""
import numpy as np
import pytest

import ins_utils as iu
import point_edge_data as D


# ---- 1. camera maps -----------------------------------------------------------------------------------------------------------------
def undistort_numpy(cam, pts):
    """cv::undistortPoints(pts, K, D, noArray(), K) in numpy float64 -> (float32 points, iteration at which each point took the
    `icdist < 0` break, -1 if none): five fixed-point iterations from the skew-free normalised point; a negative inverse distortion factor
    puts the raw normalised point back and stops; skew applied on the output side only; one rounding to float"""
    fx, fy, cx, cy, skew, k1, k2, p1, p2, k3 = [np.float64(v) for v in cam]
    ifx, ify = 1.0 / fx, 1.0 / fy
    u, v = pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64)
    x0, y0 = (u - cx) * ifx, (v - cy) * ify
    x, y = x0.copy(), y0.copy()
    broke = np.full(len(pts), -1)
    for j in range(5):
        live = broke < 0
        r2 = x * x + y * y
        with np.errstate(all="ignore"):
            icd = 1.0 / (1 + ((k3 * r2 + k2) * r2 + k1) * r2)
        dx = 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
        dy = p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
        brk = live & (icd < 0)
        broke[brk] = j
        go = live & ~brk
        x = np.where(go, (x0 - dx) * icd, np.where(brk, x0, x))
        y = np.where(go, (y0 - dy) * icd, np.where(brk, y0, y))
    return np.stack([fx * x + skew * y + cx, fy * y + cy], 1).astype(np.float32), broke


def distort_numpy(cam, pts):
    """Camera::distortPoints in numpy float64: pixel2cam with the skew, the radtan forward model, cam2pixel at Z = 1, one rounding"""
    fx, fy, cx, cy, skew, k1, k2, p1, p2, k3 = [np.float64(v) for v in cam]
    px, py = pts[:, 0].astype(np.float64), pts[:, 1].astype(np.float64)
    y = (py - cy) / fy
    x = (px - cx - skew * y) / fx
    r2 = x * x + y * y
    rr = 1 + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2
    xd = x * rr + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)
    yd = y * rr + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y
    return np.stack([(fx * xd + skew * yd) / 1.0 + cx, fy * yd / 1.0 + cy], 1).astype(np.float32)


@pytest.mark.parametrize("name", list(D.CAMERAS))
def test_undistort_and_distort_vs_numpy(oracle, name):
    cam = D.CAMERAS[name]
    for pts in [D.point_set(n) for n in D.POINT_SIZES] + [D.strong_points()]:
        exp, _ = undistort_numpy(cam, pts)
        bad = D.float_diff(oracle.undistort(cam, pts), exp)
        assert bad.size == 0, (name, len(pts), bad[:8], pts[bad[:8]])
        bad = D.float_diff(oracle.distort(cam, pts), distort_numpy(cam, pts))
        assert bad.size == 0, (name, len(pts), bad[:8], pts[bad[:8]])


def test_strong_camera_breaks_at_every_iteration(oracle):
    pts = D.strong_points()
    got = oracle.undistort(D.STRONG, pts)
    exp, broke = undistort_numpy(D.STRONG, pts)
    assert D.same_floats(got, exp) and np.isfinite(got).all()
    assert [int((broke == j).sum()) for j in (-1, 0, 1, 2, 3, 4)] == [969, 48, 579, 240, 111, 53]
    # the point sets of the GPU test reach every class too, and the break decides the result there
    pts = D.point_set(D.MAX_POINTS)
    _, broke = undistort_numpy(D.STRONG, pts)
    assert all((broke == j).sum() >= 1 for j in (-1, 0, 1, 2, 3, 4))
    for n in (255, 256, 257):
        assert (undistort_numpy(D.STRONG, D.point_set(n))[1] >= 0).sum() > 50


def test_skew_is_asymmetric_in_the_cases(oracle):
    """undistort ignores the skew on the input side and applies it on the output side: with the skew also on the input side (what
    pixel2cam does) the results differ, so the cases can tell the two apart"""
    for name in ("SKEW", "STRONG"):
        cam = D.CAMERAS[name]
        pts = D.point_set(257)
        fx, fy, cx, cy, skew = cam[:5]
        shifted = pts.astype(np.float64)
        shifted[:, 0] -= skew * (shifted[:, 1] - cy) / fy  # = a skew-aware input side
        other, _ = undistort_numpy(cam, shifted.astype(np.float32))
        assert D.float_diff(oracle.undistort(cam, pts), other).size > 200


def _pc_numpy(poses, idx, pw):
    return np.stack([poses[k, :9].reshape(3, 3).T @ (p - poses[k, 9:]) for k, p in zip(idx, pw)])


@pytest.mark.parametrize("name", list(D.CAMERAS))
def test_mappoint_case_classes(oracle, name):
    cam = D.CAMERAS[name]
    poses, idx, pw, Z = D.mappoint_case()
    assert idx[0] == 0 and idx[-1] == 4 and set(idx) == set(range(5)) and len(pw) == 257
    assert len({tuple(p) for p in poses}) == 5 and len({tuple(p[:9]) for p in poses}) == 5 and len({tuple(p[9:]) for p in poses}) == 5
    pc = _pc_numpy(poses, idx, pw)
    assert pc[0, 2] == 0.0 and abs(pw[1, 0]) == 1e30
    assert ((pc[:, 2] > 0) & (pc[:, 2] < 1e-2)).sum() >= 10 and (pc[:, 2] < 0).sum() >= 10
    exp = D.expected_mappoints(oracle, cam, poses, idx, pw)
    nan, inf = np.isnan(exp).any(1), np.isinf(exp).any(1)
    assert nan[0] and inf[1] and not nan[1]
    assert np.isfinite(exp[pc[:, 2] < 0]).all(1).sum() >= 10  # negative depth: an ordinary finite prediction
    # the expectation against numpy: world2pixel restated, then the distortPoints restatement above
    fx, fy, cx, cy, skew = [np.float64(v) for v in cam[:5]]
    with np.errstate(all="ignore"):
        w2p = np.stack([(fx * pc[:, 0] + skew * pc[:, 1]) / pc[:, 2] + cx, fy * pc[:, 1] / pc[:, 2] + cy], 1).astype(np.float32)
        ref = distort_numpy(cam, w2p)
    # (numpy's matrix product may round pc in another order than the oracle's: compared where the prediction is an ordinary pixel)
    ok = np.isfinite(exp).all(1) & np.isfinite(ref).all(1) & (np.abs(exp).max(1) < 1e4) & (np.abs(pc[:, 2]) > 1e-2)
    assert ok.sum() >= 150 and np.abs(ref[ok] - exp[ok]).max() < 1e-2, (ok.sum(), np.abs(ref[ok] - exp[ok]).max())


@pytest.mark.parametrize("name", list(D.CAMERAS))
def test_rotation_case_classes(oracle, name):
    cam = D.CAMERAS[name]
    rots, idx, pts = D.rotation_case()
    assert set(idx) == set(range(4)) and len(pts) == 257
    assert not (np.signbit(rots) & (rots == 0)).any()  # the oracle forms I^T R: exact, but a -0 entry would come out as +0
    und = oracle.undistort(cam, pts)
    xyz = oracle.pixel2cam(cam, und)
    z90 = -xyz[idx == 3, 0]  # rotated Z under the 90 degree rotation about y
    assert (z90 > 0).sum() >= 10 and (z90 < 0).sum() >= 10
    exp = D.expected_rotation(oracle, cam, rots, idx, pts)
    if name != "CAM_1280":
        assert pts[0, 0] == cam[2] and pts[0, 1] == cam[3] and np.isnan(exp[0]).any()  # principal point: rotated Z exactly 0
    else:
        assert pts[1, 0] == cam[2] and pts[1, 1] == cam[3] and np.isnan(exp[1]).any()
    # identity rotation: predict_rotation is distortCameraPoint(pixel2cam(undistort(p))), restated here with numpy
    sel = idx == 0
    fx, fy, cx, cy, skew, k1, k2, p1, p2, k3 = [np.float64(v) for v in cam]
    u, _ = undistort_numpy(cam, pts[sel])
    y = (u[:, 1].astype(np.float64) - cy) / fy
    x = (u[:, 0].astype(np.float64) - cx - skew * y) / fx
    x, y = x / 1.0, y / 1.0
    r2 = x * x + y * y
    rr = 1 + k1 * r2 + k2 * r2 * r2 + k3 * r2 * r2 * r2
    xd = (x * rr + 2 * p1 * x * y + p2 * (r2 + 2 * x * x)).astype(np.float32).astype(np.float64)
    yd = (y * rr + p1 * (r2 + 2 * y * y) + 2 * p2 * x * y).astype(np.float32).astype(np.float64)
    ref = np.stack([(fx * xd + skew * yd) / 1.0 + cx, fy * yd / 1.0 + cy], 1).astype(np.float32)
    assert D.same_floats(exp[sel], ref)


def test_lk_case_reaches_the_break_branch(oracle):
    a, b, pts, guess = D.lk_case()
    assert a.shape == (D.LK_H, D.LK_W) and 90 <= len(pts) <= 110
    exp_pts, exp_st = oracle.lk_track_fb(oracle.clahe(a), oracle.clahe(b), pts, guess)
    und, broke = undistort_numpy(D.LK_CAM, exp_pts)
    assert D.same_floats(oracle.undistort(D.LK_CAM, exp_pts), und)
    tracked = exp_st != 0
    assert tracked.sum() >= 50 and (broke[tracked] >= 0).sum() >= 1 and (broke[tracked] < 0).sum() >= 20, (tracked.sum(), (broke[tracked] >= 0).sum())


# ---- 2. reprojection gate -----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("n", [255, 256, 257])
def test_reproj_gate_cases(oracle, n):
    d = D.reproj_case(n)
    assert {0, 5} <= set(d["pose_idx"]) and {0, 39} <= set(d["lm_idx"]) and len(d["poses12"]) == 6 and len(d["pw"]) == 40
    assert sorted(d["where"].values())[0] == 0 and sorted(d["where"].values())[-1] == n - 1
    for which, max_error in enumerate(D.MAX_ERRORS):
        err, good = D.oracle_reproj(oracle, d, max_error)
        for name, (l, _, _, g0, g1) in D.GATE_LANDMARKS.items():
            i = d["where"][name]
            assert d["lm_idx"][i] == l and d["pose_idx"][i] == 0 and good[i] == (g0, g1)[which], (name, max_error, err[i], good[i])
        w = d["where"]
        assert err[w["err_5"]] == 5.0 and err[w["z_min"]] == 0.0 and err[w["z_max_down"]] == 0.0
        assert np.isinf(err[w["z_0_inf"]]) and np.isnan(err[w["z_0_nan"]]) and np.isfinite(err[w["z_neg"]]) and err[w["z_neg"]] < 5.0
        # independent restatement of the error and the gate
        cam = d["cam"]
        pc = _pc_numpy(d["poses12"], d["pose_idx"], d["pw"][d["lm_idx"]])
        with np.errstate(all="ignore"):
            px = np.stack([(cam[0] * pc[:, 0] + cam[4] * pc[:, 1]) / pc[:, 2] + cam[2], cam[1] * pc[:, 1] / pc[:, 2] + cam[3]], 1).astype(np.float32)
            e = np.sqrt(((px - d["pix"]).astype(np.float64) ** 2).sum(1))
        fin = np.isfinite(err)
        assert np.array_equal(fin, np.isfinite(e)) and np.abs(err[fin] - e[fin]).max() < 1e-3  # (float pixels: pc rounds differently in numpy's product)
        sure = fin & (np.abs(e - max_error) > 1e-2) & (np.abs(pc[:, 2] - D.MIN_DEPTH) > 1e-6) & (np.abs(pc[:, 2] - D.MAX_DEPTH) > 1e-6)
        exp_good = (pc[:, 2] > D.MIN_DEPTH) & (pc[:, 2] < D.MAX_DEPTH) & ~(e > max_error)
        assert np.array_equal(good[sure] != 0, exp_good[sure]) and 0.2 < good.mean() < 0.95


# ---- 3. triangulation ---------------------------------------------------------------------------------------------------------------
def test_triangulation_classes(oracle):
    P = D.tri_poses()
    assert P.shape == (6, 12)
    i0, i1, pc0, pc1, cls, X = D.tri_case(300)
    assert set(i0) | set(i1) == set(range(6)) and (i0 == i1).sum() >= 10
    pw = D.oracle_triangulate(oracle, P, i0, i1, pc0, pc1)
    of = {name: pw[cls == k] for k, name in enumerate(D.TRI_CLASSES)}
    truth = {name: X[cls == k] for k, name in enumerate(D.TRI_CLASSES)}
    for name in ("noisy", "exact", "hard_pose", "parallel", "behind"):
        assert np.isfinite(of[name]).all(), name
    assert np.abs(of["exact"] - truth["exact"]).max() < 1e-8 * 40
    assert np.median(np.abs(of["noisy"] - truth["noisy"])) < 0.5
    assert (np.abs(of["parallel"]).max(1) > 1e14).all() and (np.abs(of["parallel"]).max(1) > 1e17).any()  # baseline / rounding of the rays
    # two singular values are zero: rounding picks the null vector, and the result is +-inf (w == 0), all zero, or finite garbage
    same = of["same_pose"]
    assert np.isinf(same).all(1).sum() >= 3 and (same == 0).all(1).sum() >= 3 and np.isfinite(same).all(1).sum() >= 10 and not np.isnan(same).any()
    assert (of["behind"][:, 2] < 0).all() and np.abs(of["behind"] - truth["behind"]).max() < 1e-6
    a = of["axis_rays"]
    assert np.isnan(a[:, 0]).all() and np.isnan(a[:, 1]).all() and np.isinf(a[:, 2]).all()
    # every size of the GPU test holds at least the first class, and 63 upward all of them
    for n in D.TRI_SIZES:
        assert len(set(D.tri_case(n)[4])) == min(n, len(D.TRI_CLASSES))
    # the well-conditioned classes against numpy's SVD of the DLT matrix
    worst = 0.0
    for k in np.nonzero(np.isin(cls, [0, 1]))[0]:
        T0, T1 = P[i0[k]].reshape(3, 4), P[i1[k]].reshape(3, 4)
        A = np.stack([pc0[k, 0] * T0[2] - T0[0], pc0[k, 1] * T0[2] - T0[1], pc1[k, 0] * T1[2] - T1[0], pc1[k, 1] * T1[2] - T1[1]])
        v = np.linalg.svd(A)[2][3]
        ref = v[:3] / v[3]
        worst = max(worst, np.abs(pw[k] - ref).max() / max(1.0, np.abs(ref).max()))
    assert worst < 1e-8, worst


# ---- 4. INS -------------------------------------------------------------------------------------------------------------------------
def test_bracket_classes_vs_scipy_slerp(oracle):
    from scipy.spatial.transform import Rotation, Slerp
    orc = iu.OrcMisc(oracle.lib)
    pbc = iu.pose_b_c()
    Rbc = pbc[:9].reshape(3, 3)
    br, interp, times, cls = D.bracket_case(65)
    assert all(((cls == k) & (interp == v)).sum() >= 1 for k in range(len(D.BRACKET_CLASSES)) for v in (0, 1))
    q0 = br[0, 4:8]
    # the classes are what they are named for: q1 on the far side of the double cover, a tiny angle, an angle near and at pi
    for k, name in enumerate(D.BRACKET_CLASSES):
        q1 = br[k, 12:16]
        dq = D.qmul(q1 * [-1, -1, -1, 1], q0)
        ang = 2 * np.arctan2(np.linalg.norm(dq[:3]), abs(dq[3]))
        assert name == "pi" or (dq[3] < 0) == (name in ("negated", "negated_small")), (name, dq)  # (at pi, w is a rounding residue)
        lo, hi = {"same": (0, 1e-15), "negated": (0, 1e-15), "negated_small": (2e-3, 3e-3), "tiny": (0.9e-9, 1.1e-9), "near_pi": (3.1, np.pi),
                  "pi": (np.pi - 1e-15, np.pi)}[name]
        assert lo <= ang <= hi, (name, ang)
    # the interpolation is a slerp, q0 exp(s log(q0^-1 q1)), composed with the body -> camera extrinsic: float64 evaluations of one closed form
    # in a few dozen unit-magnitude operations on both sides (1e-10); a wrong branch (double-cover sign, wrong angle) shows at 1e-3 or more
    for i in range(len(br)):
        e = D.oracle_bracket_pose(orc, br[i], interp[i], pbc, times[i])
        assert np.isfinite(e).all(), (i, D.BRACKET_CLASSES[cls[i]])
        if interp[i]:
            s = (times[i] - br[i, 0]) / (br[i, 8] - br[i, 0])
            R = Slerp([0.0, 1.0], Rotation.from_quat([br[i, 4:8], br[i, 12:16]]))([s]).as_matrix()[0]
            p = br[i, 1:4] + s * (br[i, 9:12] - br[i, 1:4])
        else:
            R, p = Rotation.from_quat(br[i, 4:8]).as_matrix(), br[i, 1:4]
        assert np.abs(e[:9].reshape(3, 3) - R @ Rbc).max() < 1e-10, (i, D.BRACKET_CLASSES[cls[i]], times[i] - br[i, 0])
        assert np.abs(e[9:] - (p + R @ pbc[9:])).max() < 1e-10 * 40, i


@pytest.mark.parametrize("n_streams", [63, 64, 65])
def test_still_series_take_the_zero_angle_branch(oracle, n_streams):
    orc = iu.OrcMisc(oracle.lib)
    imus, states, still = D.mech_case(n_streams)
    lens = [len(i) for i in imus]
    assert lens[:3] == [0, 1, 2] and lens[-3:] == [2, 1, 0] and still.sum() >= 30 and (~still).sum() >= 30
    for s in np.nonzero(still)[0]:
        assert not imus[s][:, 2:].any() and not states[s, 11:].any()
        st, traj = orc.mechanize(iu.make_cfg(False, False), imus[s], states[s])
        assert np.array_equal(st[4:8], states[s, 4:8]) and (len(traj) == 0 or (traj[:, 4:8] == states[s, 4:8]).all())  # bit-unchanged attitude
        if lens[s] > 1:
            assert st[0] == imus[s][-1, 0] and not np.array_equal(st[8:11], states[s, 8:11])  # gravity was integrated
            dt = imus[s][1:, 1].sum()
            assert np.abs(st[8:11] - (states[s, 8:11] + dt * np.array([0, 0, 9.7936]))).max() < 1e-12
        else:
            assert np.array_equal(st, states[s])
        st, _ = orc.mechanize(iu.make_cfg(True, False), imus[s], states[s])
        assert np.isfinite(st).all()
