"""Edge inputs for the lane-per-item FP64 kernels: the camera maps of csrc/points.hip and dev_camera.h (with their fused use in the LK
epilogue), k_reproj_error, k_triangulate_seg and the two INS kernels of csrc/ins.hip.  Shared by test_oracle_point_edges.py (CPU: the
oracle against independent restatements, and proof that each case reaches the edge it is named for) and test_gpu_point_edges.py (kernel
against oracle).  Numpy only; everything is deterministic."""
import numpy as np

import ins_utils as iu
import synth
from ctypes_util import ptr

W, H = 1280, 720
MAX_POINTS = 1024
SKEW = [700.0, 705.0, 631.0, 352.0, 0.8, -0.31, 0.12, 1e-3, -7e-4, -0.02]
STRONG = [700.0, 705.0, 631.0, 352.0, 0.8, -1.2, 0.1, 1e-3, -7e-4, 0.0]  # 1 + k1 r2 + k2 r2^2 < 0 for r2 in (0.90, 11.1): the break branch
CAMERAS = {"CAM_1280": list(synth.CAM_1280), "SKEW": SKEW, "STRONG": STRONG}
POINT_SIZES = (1, 255, 256, 257, MAX_POINTS)


# ---- comparison ---------------------------------------------------------------------------------------------------------------------
def float_diff(got, exp):
    """indices (first axis) at which two float arrays differ: NaN against non-NaN, or different bit patterns where neither is NaN (so
    +-inf and the sign of zero count; the sign and payload of a NaN, which differ between x86 and gfx950, do not)"""
    got, exp = np.ascontiguousarray(got), np.ascontiguousarray(exp)
    assert got.dtype == exp.dtype and got.shape == exp.shape and got.dtype in (np.float32, np.float64), (got.dtype, exp.dtype, got.shape, exp.shape)
    u = np.uint32 if got.dtype == np.float32 else np.uint64
    ng, ne = np.isnan(got), np.isnan(exp)
    bad = (ng != ne) | (~ng & ~ne & (got.view(u) != exp.view(u)))
    return np.nonzero(bad.reshape(len(bad), -1).any(1))[0]


def same_floats(got, exp):
    return float_diff(got, exp).size == 0


# ---- 1. camera maps -----------------------------------------------------------------------------------------------------------------
def point_set(n, seed=1):
    """n pixels: the principal points of the cameras, integer and half-integer pixels, points outside the image (negative, +-5000 px),
    then uniform points over the image"""
    special = [[631.0, 352.0], [640.0, 360.0], [0.0, 0.0], [1279.0, 719.0], [17.0, 702.0], [100.5, 200.5], [1279.5, 0.5], [630.5, 352.0],
               [-3.25, -11.0], [-40.0, 300.0], [1300.0, 760.5], [5000.0, 352.0], [-5000.0, 5000.0], [631.0, -5000.0], [5000.0, 5000.0]]
    rng = np.random.RandomState(seed)
    rnd = np.stack([rng.uniform(0, W, n), rng.uniform(0, H, n)], 1)
    return np.concatenate([np.array(special), rnd])[:n].astype(np.float32)


def strong_points():
    """the 2000 points on which the break statistics of STRONG are stated"""
    return np.random.RandomState(1).uniform([0, 0], [W, H], (2000, 2)).astype(np.float32)


def _rot(axis, ang):
    c, s = np.cos(ang), np.sin(ang)
    i, j = [(1, 2), (2, 0), (0, 1)][axis]
    R = np.eye(3)
    R[i, i], R[i, j], R[j, i], R[j, j] = c, -s, s, c
    return R


def mappoint_case(seed=11):
    """-> poses12 (5 x 12: R row-major camera -> world, t), pose_idx (257), pw (257 x 3), Z (camera-frame depth as built).  Pose 0 is the
    identity rotation.  Point 0: Z exactly 0 under pose 0; point 1: |X| = 1e30; points 2..21: Z slightly above 0; points 22..41: Z < 0"""
    rng = np.random.RandomState(seed)
    Rs = [np.eye(3), _rot(2, 0.05), _rot(0, -0.3) @ _rot(1, 0.2), _rot(1, -0.4) @ _rot(2, 1.1), _rot(0, 0.7) @ _rot(1, 0.5) @ _rot(2, -0.6)]
    ts = [[0.3, -0.2, 0.1], [1.5, 0.4, -0.7], [-2.0, 0.1, 0.6], [0.0, 3.0, 1.0], [-0.8, -1.1, 2.5]]
    poses = np.stack([np.concatenate([R.ravel(), t]) for R, t in zip(Rs, ts)])
    n = 257
    idx = rng.randint(0, 5, n).astype(np.int32)
    idx[0], idx[1], idx[n - 1] = 0, 0, 4
    Z = rng.uniform(2, 40, n)
    Z[2:22] = 10.0 ** rng.uniform(-9, -2, 20)
    Z[22:42] = -rng.uniform(0.5, 30, 20)
    pc = np.stack([rng.uniform(-0.6, 0.6, n) * Z, rng.uniform(-0.35, 0.35, n) * Z, Z], 1)
    pw = np.stack([Rs[k] @ p + ts[k] for k, p in zip(idx, pc)])
    pw[0] = [1.0, 0.5, ts[0][2]]
    pw[1] = [-1e30, 2.0, 10.0]
    Z[0], Z[1] = 0.0, 10.0 - ts[0][2]
    return poses, idx, pw, Z


def rotation_case(seed=12):
    """-> rots9 (4 x 9: identity, 0.05 rad yaw, 30 deg pitch, 90 deg about y with exact 0 / 1 entries), rot_idx (257), pts (257 x 2)"""
    rots = np.stack([np.eye(3), _rot(2, 0.05), _rot(0, np.deg2rad(30.0)), np.array([[0.0, 0, 1], [0, 1, 0], [-1, 0, 0]])]).reshape(4, 9)
    rng = np.random.RandomState(seed)
    idx = rng.randint(0, 4, 257).astype(np.int32)
    idx[0], idx[1], idx[256] = 3, 3, 0  # both principal points under the 90 degree rotation: rotated Z exactly 0 for the camera that owns it
    return rots, idx, point_set(257, seed=13)


def expected_mappoints(oracle, cam, poses, idx, pw):
    return np.concatenate([oracle.distort(cam, oracle.world2pixel(cam, poses[k], pw[i:i + 1])) for i, k in enumerate(idx)])


def expected_rotation(oracle, cam, rots, idx, pts):
    """the oracle per rotation with R_cur = I, R_pre = r: it then forms I^T r, which is r exactly"""
    exp = np.zeros_like(pts)
    for k in range(len(rots)):
        exp[idx == k] = oracle.predict_rotation(cam, np.eye(3), rots[k].reshape(3, 3), pts[idx == k])
    return exp


LK_W, LK_H = 160, 120
LK_CAM = [90.0, 90.0, 80.0, 60.0, 0.8, -1.2, 0.1, 1e-3, -7e-4, 0.0]


def lk_case():
    """160 x 120 frame pair and ~100 points over the whole frame; a band of them near the corners, where LK_CAM breaks"""
    a = synth.texture(LK_W, LK_H, seed=81)
    b = synth.shift_image(a, 1.25, -0.75)
    corners = [[x, y] for x in (6.0, 10.5, 149.0, 153.5) for y in (5.0, 9.5, 110.0, 114.5)]
    pts = np.concatenate([np.array(corners, np.float32), synth.random_points(84, LK_W, LK_H, 3, seed=82)])
    return a, b, pts, pts + np.float32([1.0, -0.5])


# ---- 2. reprojection gate -----------------------------------------------------------------------------------------------------------
MIN_DEPTH, MAX_DEPTH = 1.0, 200.0
GATE_LANDMARKS = {  # name: (landmark index, pw, offset of the key point from the projection, good at max_error 5.0, good just below 5.0)
    "z_min": (0, [0.0, 0.0, MIN_DEPTH], (0.0, 0.0), 0, 0),
    "z_min_up": (1, [0.0, 0.0, np.nextafter(MIN_DEPTH, np.inf)], (0.0, 0.0), 1, 1),
    "z_max": (2, [0.0, 0.0, MAX_DEPTH], (0.0, 0.0), 0, 0),
    "z_max_down": (3, [0.0, 0.0, np.nextafter(MAX_DEPTH, -np.inf)], (0.0, 0.0), 1, 1),
    "err_5": (4, [0.0, 0.0, 8.0], (3.0, 4.0), 1, 0),
    "z_0_inf": (5, [1.0, 1.0, 0.0], (0.0, 0.0), 0, 0),
    "z_0_nan": (6, [0.0, 0.0, 0.0], (0.0, 0.0), 0, 0),
    "z_neg": (7, [0.5, 0.2, -5.0], (0.0, 0.0), 0, 0),
}
MAX_ERRORS = (5.0, float(np.nextafter(5.0, 0.0)))


def reproj_case(n, seed=21):
    """n observations of 40 landmarks from 6 poses with CAM_1280.  Pose 0 is the identity at the origin and sees the eight gate landmarks
    (GATE_LANDMARKS; under it a point on the optical axis projects to (cx, cy) exactly), at the first, last and middle observations; the
    others are random, key point = projection + 0 .. 8 px.  -> dict with `where` = observation index of each gate case"""
    cam = np.array(synth.CAM_1280)
    rng = np.random.RandomState(seed)
    poses = [np.concatenate([np.eye(3).ravel(), [0.0, 0.0, 0.0]])]
    for k in range(5):
        R = _rot(1, rng.normal(0, 0.05)) @ _rot(0, rng.normal(0, 0.03))
        poses.append(np.concatenate([R.ravel(), rng.normal(0, 0.5, 3)]))
    poses = np.stack(poses)
    n_lm, n_gate = 40, len(GATE_LANDMARKS)
    depth = rng.uniform(3, 60, n_lm)
    pw = np.stack([rng.uniform(-0.4, 0.4, n_lm) * depth, rng.uniform(-0.25, 0.25, n_lm) * depth, depth], 1)
    for _, (l, p, _, _, _) in GATE_LANDMARKS.items():
        pw[l] = p
    pose_idx = rng.randint(0, 6, n).astype(np.int32)
    lm_idx = rng.randint(n_gate, n_lm, n).astype(np.int32)
    pose_idx[n // 3], lm_idx[n // 3] = 5, n_lm - 1
    slots = [0, n - 1, n // 2, n // 2 + 1, 2, n - 2, 3, n - 3]
    where = {}
    for s, (name, (l, _, _, _, _)) in zip(slots, GATE_LANDMARKS.items()):
        pose_idx[s], lm_idx[s], where[name] = 0, l, s
    pix = np.zeros((n, 2), np.float32)
    for i in range(n):
        R, t = poses[pose_idx[i], :9].reshape(3, 3), poses[pose_idx[i], 9:]
        pc = R.T @ (pw[lm_idx[i]] - t)
        with np.errstate(all="ignore"):
            pix[i] = [cam[0] * pc[0] / pc[2] + cam[2], cam[1] * pc[1] / pc[2] + cam[3]]
    pix += (rng.normal(0, 1, (n, 2)) * rng.choice([0.3, 1.2, 4.0, 8.0], (n, 1))).astype(np.float32)
    for name, (l, p, off, _, _) in GATE_LANDMARKS.items():  # pose 0: pc = pw; the key point at the stated offset from the float projection
        proj = np.float32([cam[0] * p[0] / p[2] + cam[2], cam[1] * p[1] / p[2] + cam[3]]) if p[2] != 0 else np.float32([cam[2], cam[3]])
        pix[where[name]] = proj - np.float32(off)
    return dict(cam=cam, poses12=poses, pw=pw, pose_idx=pose_idx, lm_idx=lm_idx, pix=pix, where=where)


def oracle_reproj(oracle, d, max_error):
    import ctypes as C
    n = len(d["pose_idx"])
    err, good = np.zeros(n), np.zeros(n, np.uint8)
    p = ptr
    oracle.lib.orc_reproj_error_batch(p(d["cam"]), n, p(d["pose_idx"]), p(d["lm_idx"]), p(d["poses12"]), p(d["pw"]), p(d["pix"]), C.c_double(max_error),
                                      C.c_double(MIN_DEPTH), C.c_double(MAX_DEPTH), p(err), p(good))
    return err, good


# ---- 3. triangulation ---------------------------------------------------------------------------------------------------------------
def oracle_triangulate(oracle, P, i0, i1, pc0, pc1):
    return np.stack([oracle.triangulate(P[a], P[b], x, y) for a, b, x, y in zip(i0, i1, pc0, pc1)])


TRI_SIZES = (1, 63, 64, 65, 300)
TRI_CLASSES = ("noisy", "exact", "hard_pose", "parallel", "same_pose", "behind", "axis_rays")


def tri_poses():
    """six 3 x 4 camera matrices [R | t]: identity, three generic, a 1e-9 pure-x baseline from the identity, a translation of 1e6"""
    def T(R, t):
        return np.hstack([R, np.array(t, np.float64)[:, None]]).ravel()
    return np.stack([T(np.eye(3), [0, 0, 0]), T(_rot(1, 0.05), [0.5, 0.05, 0.1]), T(_rot(0, -0.04) @ _rot(2, 0.1), [-0.6, 0.2, 0.05]),
                     T(_rot(1, -0.08) @ _rot(0, 0.03), [0.1, -0.7, -0.2]), T(np.eye(3), [1e-9, 0, 0]), T(_rot(1, 0.05), [1e6, -2e5, 3e5])])


def tri_case(n, seed=31):
    """n points, class i % 7 (TRI_CLASSES) -> T0_idx, T1_idx, pc0, pc1, cls, X (the world point the rays were built from, NaN where none)"""
    P = tri_poses().reshape(6, 3, 4)
    rng = np.random.RandomState(seed)
    i0, i1 = np.zeros(n, np.int32), np.zeros(n, np.int32)
    pc0, pc1, X = np.zeros((n, 3)), np.zeros((n, 3)), np.full((n, 3), np.nan)
    cls = np.arange(n) % len(TRI_CLASSES)

    def rays(a, b, Xw):
        out = []
        for k in (a, b):
            c = P[k, :, :3] @ Xw + P[k, :, 3]
            out.append(c / c[2])
        return out

    for i in range(n):
        name = TRI_CLASSES[cls[i]]
        Xw = np.array([rng.uniform(-8, 8), rng.uniform(-5, 5), rng.uniform(6, 40)])
        a, b = rng.choice(4, 2, replace=False)
        if name in ("noisy", "exact"):
            X[i] = Xw
            pc0[i], pc1[i] = rays(a, b, Xw)
            if name == "noisy":
                pc1[i, :2] += rng.normal(0, 1e-3, 2)
        elif name == "hard_pose":  # the tiny baseline, and the 1e6 translation seen against a generic pose
            a, b = [(0, 4), (4, 1), (5, 2), (3, 5)][(i // len(TRI_CLASSES)) % 4]
            X[i] = Xw if 5 not in (a, b) else P[5, :, :3].T @ (Xw - P[5, :, 3])
            pc0[i], pc1[i] = rays(a, b, X[i])
        elif name == "parallel":  # one world direction seen from two different centres
            d = Xw / Xw[2]
            pc0[i], pc1[i] = [(P[k, :, :3] @ d) / (P[k, :, :3] @ d)[2] for k in (a, b)]
        elif name == "same_pose":
            b = a
            pc0[i] = pc1[i] = rays(a, a, Xw)[0]
        elif name == "behind":
            X[i] = Xw * [1, 1, -1]
            a, b = 0, 1 + i % 3
            pc0[i], pc1[i] = rays(a, b, X[i])
        else:  # both rays along the optical axis, the baseline along x
            a, b = 0, 4
            pc0[i] = pc1[i] = [0.0, 0.0, 1.0]
        i0[i], i1[i] = a, b
    return i0, i1, pc0, pc1, cls, X


# ---- 4. INS -------------------------------------------------------------------------------------------------------------------------
def qmul(a, b):
    """Hamilton product, [x, y, z, w]"""
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx,
                     aw * bw - ax * bx - ay * by - az * bz])


def rotvec_quat(rv):
    rv = np.array(rv, np.float64)
    a = np.linalg.norm(rv)
    return np.array([*(np.sin(a / 2) * rv / a), np.cos(a / 2)]) if a > 0 else np.array([0.0, 0, 0, 1])


BRACKET_CLASSES = ("same", "negated", "negated_small", "tiny", "near_pi", "pi")


def bracket_q1(name, q0):
    return {"same": lambda: q0.copy(), "negated": lambda: -q0, "negated_small": lambda: -qmul(q0, rotvec_quat([1e-3, 2e-3, -1e-3])),
            "tiny": lambda: qmul(q0, rotvec_quat([1e-9, 0, 0])), "near_pi": lambda: qmul(q0, rotvec_quat([3.1, 0.2, 0.1])),
            "pi": lambda: qmul(q0, rotvec_quat([np.pi, 0, 0]))}[name]()


def bracket_case(n):
    """n queries cycling through BRACKET_CLASSES x (fraction 0, 0.25, just below 1, and interp = 0) -> brackets16, interp, times, cls"""
    q0 = rotvec_quat([0.3, -0.2, 0.5])
    rng = np.random.RandomState(41)
    br, interp, times = np.zeros((n, 16)), np.ones(n, np.int32), np.zeros(n)
    cls = np.arange(n) % len(BRACKET_CLASSES)
    for i in range(n):
        t0 = 2000.0 + 0.005 * i
        t1 = t0 + 0.005
        variant = (i // len(BRACKET_CLASSES)) % 4
        br[i] = [t0, *rng.normal(0, 20, 3), *q0, t1, 0, 0, 0, *bracket_q1(BRACKET_CLASSES[cls[i]], q0)]
        br[i, 9:12] = br[i, 1:4] + rng.normal(0, 0.05, 3)
        times[i] = [t0, t0 + 0.25 * (t1 - t0), np.nextafter(t1, -np.inf), t0 + 0.5 * (t1 - t0)][variant]
        interp[i] = 0 if variant == 3 else 1
    return br, interp, times, cls


def oracle_bracket_pose(orc, br, interp, pbc, time):
    """the oracle on one bracket: a two-state window for the interpolation, a one-state window queried outside for `the first state as is`"""
    imu, st = np.zeros((2, 8)), np.zeros((2, 23))
    imu[:, 0] = st[:, 0] = br[0], br[8]
    st[0, 1:8], st[1, 1:8] = br[1:8], br[9:16]
    if interp:
        e, f = orc.camera_pose(imu, st, pbc, time)
        assert f == 1
    else:
        e, f = orc.camera_pose(imu[:1], st[:1], pbc, br[0] - 1.0)
        assert f == 0
    return e


def _unit_norm_state(seed):
    """a state without biases or scale factors whose attitude has the floating-point norm 1.0 exactly, so that renormalising returns it"""
    for k in range(200):
        s = iu.make_state(2000.0, seed=1000 * seed + k)
        s[11:] = 0.0
        q = s[4:8] / np.sqrt(s[4] * s[4] + s[5] * s[5] + s[6] * s[6] + s[7] * s[7])
        if np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]) == 1.0:
            s[4:8] = q
            return s
    raise AssertionError("no attitude of norm exactly 1")


def still_imu(n, rate=200.0, t0=2000.0):
    """n samples with zero increments: rotvec2quat sees the angle 0 at every step"""
    imu = np.zeros((n, 8))
    imu[:, 0] = t0 + np.arange(1, n + 1) / rate
    imu[:, 1] = 1.0 / rate
    return imu


def mech_case(n_streams):
    """-> imus, states, still (bool per stream): still series of zero increments from unit-norm, bias-free states at the even streams,
    ordinary make_imu series at the odd ones; lengths 0, 1 and 2 at the first and the last streams"""
    rng = np.random.RandomState(50 + n_streams)
    lens = [int(x) for x in rng.randint(3, 40, n_streams)]
    lens[:3], lens[-3:] = [0, 1, 2], [2, 1, 0]
    imus, states, still = [], [], []
    for s, n in enumerate(lens):
        still.append(s % 2 == 0)
        if still[-1]:
            imus.append(still_imu(n))
            states.append(_unit_norm_state(s))
        else:
            imus.append(iu.make_imu(max(n, 1), seed=300 + s, jitter=(s % 4 == 1))[:n])
            states.append(iu.make_state(2000.0, seed=s, scale=False))
    return imus, np.stack(states), np.array(still)
