"""End-to-end checks of the replay harness + icg::GVINS on the synthetic GNSS / IMU / camera sequence of
gvins_data.py.  The same checks run on the oracle-backed host layer (CPU) and on the HIP-backed one (MI355X); the solver itself has no
reference to be pinned against (Ceres is absent), so the anchor is the known truth of the sequence and the formats of the result files."""
import ctypes as C
import os

import numpy as np

import harness as H

import gvins_data as gd
import reproj_data as rd
from ctypes_util import ErrBuf

STATE_TRACKING_NORMAL = 4
SUMMARY_KEYS = ["imu", "gnss", "gnss_dropped", "frames", "frames_tracked", "keyframes", "optimizations", "marginalizations", "ins_launches", "lost",
                "reprojection_factors", "chi2_removed", "final_state", "wall_seconds", "data_seconds", "unused"]


def run_replay(lib, files, start=0.0, end=0.0):
    summ = np.zeros(16)
    err = ErrBuf(1024)
    rc = lib.icgh_replay_run(files["config"].encode(), None, files["imu"].encode(), files["gnss"].encode(), files["images"].encode(), 0, C.c_double(start),
                             C.c_double(end), summ.ctypes.data_as(C.c_void_p), *err.args)
    assert rc == 0, (rc, err.text())
    return dict(zip(SUMMARY_KEYS, summ))


def trajectory_errors(seq, files):
    """per trajectory.csv row: (time since start, position error [m], attitude error [deg]) against the sequence's truth"""
    tr = np.loadtxt(os.path.join(files["out"], "trajectory.csv"))
    out = []
    for r in tr:
        Rnb, p = seq.truth_at(r[0], files["first_fix_local"])
        ang = np.linalg.norm(gd.rot_log(Rnb.T @ rd.quat_to_R(r[4:8]))) / gd.D2R
        out.append([r[0] - gd.T0, np.linalg.norm(r[1:4] - p), ang])
    return np.array(out), tr


def check_result_files(files, S):
    out = files["out"]
    cols = {"gvins.nav": 11, "trajectory.csv": 8, "statistics.txt": 15, "tracking.txt": 7, "mappoint.txt": 3}
    rows = {}
    for name, nc in cols.items():
        path = os.path.join(out, name)
        assert os.path.exists(path), name
        a = np.atleast_2d(np.loadtxt(path))
        assert a.shape[1] == nc, (name, a.shape)
        rows[name] = a
        for line in open(path):  # fileio/filesaver.cc:51-66: "%-15.9lf " per value
            assert line.endswith(" \n") and all(len(tok.split(".")[1]) == 9 for tok in line.split()), (name, line)
            break
    assert os.path.exists(os.path.join(out, "gvins.yaml"))
    # IMU_ERR.bin: raw doubles, 8 per navigation line (time, gyroscope bias [deg/h], accelerometer bias [mGal], odometer scale), misc.cc:452-470
    imu_err = np.fromfile(os.path.join(out, "IMU_ERR.bin"), np.float64).reshape(-1, 8)
    assert len(imu_err) == len(rows["gvins.nav"]) and np.array_equal(imu_err[:, 0], rows["gvins.nav"][:, 1]) and np.all(imu_err[:, 7] == 0)
    assert np.abs(imu_err[-1, 1:4]).max() < 500 and np.abs(imu_err[-1, 4:7]).max() < 5000  # estimates near the simulated 20-40 deg/h, 600-1000 mGal
    nav, traj, stat = rows["gvins.nav"], rows["trajectory.csv"], rows["statistics.txt"]
    # one navigation / trajectory line per 10 IMU epochs after the initialization (misc.cc:419-425)
    assert len(nav) == len(traj) and np.array_equal(nav[:, 1], traj[:, 0])
    assert np.allclose(np.diff(traj[:, 0]), 0.05, atol=1e-6)
    assert np.all(nav[:, 0] == 0) and np.all((nav[:, 10] >= 0) & (nav[:, 10] < 360))
    assert np.allclose(np.linalg.norm(traj[:, 4:8], axis=1), 1.0, atol=1e-9)
    # one statistics line per window optimization that saw at least two keyframes (ic_gvins.cc:938-940, 1029-1032)
    assert 0 < len(stat) <= S["optimizations"]
    assert np.all(np.diff(stat[:, 0]) > 0) and np.all(stat[:, 8] <= 5) and np.all(stat[:, 9] <= 15)  # optimize_num_iterations 20 -> 5 + 15
    return rows


def check_replay(lib_path, tmp_root, pos_tol=0.10, att_tol=0.30, bitwise=True):
    lib = C.CDLL(H.tools_lib(lib_path))
    seq = gd.Sequence(lib)
    files = seq.write(str(tmp_root))
    S = run_replay(lib, files)
    assert S["imu"] == files["n_imu"] - 1 and S["gnss"] == files["n_gnss"] and S["frames"] == files["n_images"]
    assert S["final_state"] == STATE_TRACKING_NORMAL and S["lost"] == 0
    # frames are only accepted once the GNSS/INS initialization is through (ic_gvins.cc:223): all but the first few are tracked
    assert files["n_images"] - 4 <= S["frames_tracked"] <= files["n_images"]
    assert S["keyframes"] >= 20 and S["marginalizations"] >= 10 and S["optimizations"] >= S["keyframes"] - 2
    assert S["reprojection_factors"] > 5000 and S["ins_launches"] < S["imu"] / 4  # INS epochs are mechanized as series, not one launch per epoch
    E, traj = trajectory_errors(seq, files)
    late = E[E[:, 0] > 4.0]
    assert len(late) > 60
    assert late[:, 1].max() < pos_tol, late[:, 1].max()
    assert late[:, 2].max() < att_tol, late[:, 2].max()
    # vision + IMU + GNSS beats the GNSS/INS-only phase in attitude (heading / levelling refined by the visual factors)
    early = E[(E[:, 0] > 2.6) & (E[:, 0] < 3.4)]
    assert late[:, 2].mean() < early[:, 2].mean()
    check_result_files(files, S)
    # the run is deterministic: the same files again give the same results — byte-identical files on the CPU backend; on the device the
    # normal equations are summed with FP64 atomics (order-free sums), so runs agree to rounding and every discrete
    # decision (keyframes, solver step counts, culled landmarks) is the same
    first = open(os.path.join(files["out"], "trajectory.csv"), "rb").read()
    first_stat = np.loadtxt(os.path.join(files["out"], "statistics.txt"))
    S2 = run_replay(lib, files)
    second_stat = np.loadtxt(os.path.join(files["out"], "statistics.txt"))
    if bitwise:
        assert open(os.path.join(files["out"], "trajectory.csv"), "rb").read() == first
        keep = [c for c in range(15) if c not in (10, 11, 12)]  # the three wall-clock columns differ
        assert np.array_equal(first_stat[:, keep], second_stat[:, keep])
    else:
        again = np.loadtxt(os.path.join(files["out"], "trajectory.csv"))
        assert again.shape == traj.shape and np.array_equal(again[:, 0], traj[:, 0])
        # rounding differences can end an LM solve one step earlier or later (function tolerance): 1 mm covers that, far below the accuracy
        assert np.abs(again[:, 1:] - traj[:, 1:]).max() < 1e-3, np.abs(again[:, 1:] - traj[:, 1:]).max()
        assert first_stat.shape == second_stat.shape and np.array_equal(first_stat[:, [0, 1, 2, 3, 13, 14]], second_stat[:, [0, 1, 2, 3, 13, 14]])
        assert np.abs(first_stat[:, 4:8] - second_stat[:, 4:8]).max() < 1e-2
    assert all(S[k] == S2[k] for k in SUMMARY_KEYS[:13] if bitwise or k not in ("reprojection_factors", "chi2_removed", "ins_launches"))
    return S, E


def check_replay_calibration(lib_path, tmp_root):
    """optimize_estimate_extrinsic / optimize_estimate_td and the Earth-rotation variants (INS mechanization + PreintegrationEarth) on.
    The sequence was made with the configured extrinsic and no delay: the time delay stays at zero; the lever arm of the camera is not
    observable on a straight drive, so its estimate wanders and the reference's guard (ic_gvins.cc:1320-1330: more than 1 m / 5 deg away
    from the current value is logged but not taken over) has to keep the states clean.  extrinsic.txt gets one row per window solve."""
    lib = C.CDLL(H.tools_lib(lib_path))
    seq = gd.Sequence(lib)
    files = seq.write(str(tmp_root), estimate_extrinsic=True, estimate_td=True, with_earth=True)
    S = run_replay(lib, files)
    assert S["final_state"] == STATE_TRACKING_NORMAL and S["lost"] == 0
    ext = np.atleast_2d(np.loadtxt(os.path.join(files["out"], "extrinsic.txt")))
    stat = np.atleast_2d(np.loadtxt(os.path.join(files["out"], "statistics.txt")))
    assert ext.shape[1] == 8 and len(ext) >= len(stat) >= 10
    assert np.all(np.isfinite(ext)) and np.abs(ext[:, 7]).max() < 0.005, np.abs(ext[:, 7]).max()  # time delay [s]
    # until the window is full the extrinsic block is constant (ic_gvins.cc:1750): rows repeat the configured value
    assert np.allclose(ext[0, 1:4], gd.T_BC, atol=1e-9) and np.allclose(ext[0, 4:7] % 360, [90.0, 0.0, 0.0], atol=1e-6)
    E, _ = trajectory_errors(seq, files)
    late = E[E[:, 0] > 4.0]
    assert late[:, 1].max() < 0.15 and late[:, 2].max() < 0.8, (late[:, 1].max(), late[:, 2].max())
    return S, E, ext


def check_replay_window(lib_path, tmp_root):
    """start/end bounds of the replay and a GNSS outage: fixes after `gnssoutagetime` are dropped (fusion_ros.cc:185-197) and the estimator
    keeps tracking on INS + vision"""
    lib = C.CDLL(H.tools_lib(lib_path))
    seq = gd.Sequence(lib)
    files = seq.write(str(tmp_root))
    cfg = open(files["config"]).read().replace("isusegnssoutage: false", "isusegnssoutage: true").replace("gnssoutagetime: 0", f"gnssoutagetime: {gd.T0 + 5.0}")
    open(files["config"], "w").write(cfg)
    S = run_replay(lib, files, end=gd.T0 + 7.0)
    assert S["gnss"] == 5 and S["gnss_dropped"] == 2 and S["final_state"] == STATE_TRACKING_NORMAL and S["lost"] == 0
    assert abs(S["data_seconds"] - 7.0) < 0.02
    E, _ = trajectory_errors(seq, files)
    late = E[E[:, 0] > 6.0]
    assert late[:, 1].max() < 0.5, late[:, 1].max()  # two seconds without GNSS: visual-inertial drift stays small
    return S, E


def run_replay_many(lib, files, outputs, wait_poll_us=0):
    n = len(outputs)
    for o in outputs:
        os.makedirs(o, exist_ok=True)
    arr = (C.c_char_p * n)(*[o.encode() for o in outputs])
    summ = np.zeros((n, 16))
    wall = C.c_double(0)
    err = ErrBuf(1024)
    rc = lib.icgh_replay_run_many(n, files["config"].encode(), arr, files["imu"].encode(), files["gnss"].encode(), files["images"].encode(), 0,
                                  int(wait_poll_us), summ.ctypes.data_as(C.c_void_p), C.byref(wall), *err.args)
    assert rc == 0, (rc, err.text())
    return [dict(zip(SUMMARY_KEYS, row)) for row in summ], wall.value


def check_replay_concurrent(lib_path, tmp_root, n=3, bitwise=True, wait_poll_us=0):
    """n estimators side by side in one process (one host thread, own device contexts and id space each): every stream's result files equal
    those of the same replay run alone — the streams of one GPU do not see each other"""
    lib = C.CDLL(H.tools_lib(lib_path))
    seq = gd.Sequence(lib)
    files = seq.write(str(tmp_root))
    S = run_replay(lib, files)
    alone = open(os.path.join(files["out"], "trajectory.csv"), "rb").read()
    alone_rows = np.loadtxt(os.path.join(files["out"], "trajectory.csv"))
    alone_track = open(os.path.join(files["out"], "tracking.txt")).read().split("\n")
    outs = [os.path.join(str(tmp_root), "stream%d" % k) for k in range(n)]
    SS, wall = run_replay_many(lib, files, outs, wait_poll_us)
    for k, o in enumerate(outs):
        assert all(SS[k][key] == S[key] for key in ("imu", "gnss", "frames", "frames_tracked", "keyframes", "optimizations", "marginalizations", "lost", "final_state"))
        if bitwise:
            assert open(os.path.join(o, "trajectory.csv"), "rb").read() == alone, k
        else:
            rows = np.loadtxt(os.path.join(o, "trajectory.csv"))
            assert rows.shape == alone_rows.shape and np.abs(rows - alone_rows).max() < 1e-3, k
        # tracking.txt: all columns but the last (wall-clock time per frame) are identical text on the CPU backend; on the device the
        # parallax / relative-motion columns inherit the rounding of the optimized poses, stamps and feature counts stay identical
        track = open(os.path.join(o, "tracking.txt")).read().split("\n")
        if bitwise:
            assert [" ".join(t.split()[:6]) for t in track] == [" ".join(t.split()[:6]) for t in alone_track], k
        else:
            a = np.array([[float(v) for v in t.split()[:6]] for t in alone_track if t.strip()])
            b = np.array([[float(v) for v in t.split()[:6]] for t in track if t.strip()])
            assert a.shape == b.shape and np.array_equal(a[:, [0, 1, 5]], b[:, [0, 1, 5]]) and np.abs(a - b).max() < 1e-2, k
    return SS, wall


def check_replay_tracking_loss(lib_path, tmp_root):
    """half a second of black images in the middle of the drive: the tracker reports TRACK_LOST, the lost frame and the empty first frames
    that follow become keyframes (ic_gvins.cc:540-549) and are dropped again as empty keyframes (:1397-1398), the tracker re-initializes
    on the first textured frames, and the estimator — carried by INS + GNSS meanwhile — stays at the truth"""
    lib = C.CDLL(H.tools_lib(lib_path))
    seq = gd.Sequence(lib)
    files = seq.write(str(tmp_root))
    names = [line.split()[1] for line in open(files["images"])]
    for name in names[40:50]:
        with open(os.path.join(str(tmp_root), "cam0", name), "wb") as f:
            f.write(b"P5\n%d %d\n255\n" % (seq.w, seq.h) + bytes(seq.w * seq.h))
    S = run_replay(lib, files)
    assert S["lost"] == 1 and S["final_state"] == STATE_TRACKING_NORMAL
    assert S["keyframes"] > 30 and S["marginalizations"] >= 10
    E, _ = trajectory_errors(seq, files)
    late = E[E[:, 0] > 4.0]
    assert late[:, 1].max() < 0.10 and late[:, 2].max() < 0.30, (late[:, 1].max(), late[:, 2].max())
    track = np.loadtxt(os.path.join(files["out"], "tracking.txt"))
    assert 10 <= len(track) < S["keyframes"]  # a row per keyframe decision of a frame in TRACK_TRACKING (tracking.cc:297-315), none while lost
    return S, E


def check_replay_input_formats(lib_path, tmp_root):
    """the other input flavours of the replay give the same run: IMU as angular rate / specific force (the fields of sensor_msgs/Imu, multiplied
    by dt as imuCallback does), Unix time stamps (converted with GpsTime::unix2gps), colour images (PPM -> BGR8 -> gray on the device)"""
    lib = C.CDLL(H.tools_lib(lib_path))
    seq = gd.Sequence(lib)
    files = seq.write(str(tmp_root))
    S = run_replay(lib, files)
    base = np.loadtxt(os.path.join(files["out"], "trajectory.csv"))
    root = str(tmp_root)
    week = 2200
    to_unix = lambda sow: sow + week * 604800 + 315964800 - 18
    imu = np.loadtxt(files["imu"])
    dt = np.diff(np.concatenate([[imu[0, 0] - 0.005], imu[:, 0]]))
    with open(os.path.join(root, "imu_rate_unix.txt"), "w") as f:
        for r, d in zip(imu, dt):
            f.write("%.9f %.15e %.15e %.15e %.15e %.15e %.15e\n" % ((to_unix(r[0]),) + tuple(r[1:] / d)))
    gn = np.loadtxt(files["gnss"])
    with open(os.path.join(root, "gnss_unix.txt"), "w") as f:
        for r in gn:
            f.write("%.9f %.12f %.12f %.6f %.3f %.3f %.3f\n" % ((to_unix(r[0]),) + tuple(r[1:])))
    os.makedirs(os.path.join(root, "cam1"), exist_ok=True)
    with open(os.path.join(root, "cam1", "images.txt"), "w") as f:
        for line in open(files["images"]):
            t, name = line.split()
            raw = open(os.path.join(root, "cam0", name), "rb").read()
            pix = np.frombuffer(raw[-seq.w * seq.h:], np.uint8)
            out = name.replace(".pgm", ".ppm")
            with open(os.path.join(root, "cam1", out), "wb") as g:
                g.write(b"P6\n%d %d\n255\n" % (seq.w, seq.h))
                g.write(np.repeat(pix, 3).tobytes())  # R = G = B: the BGR -> gray conversion returns the same image
            f.write("%.9f %s\n" % (to_unix(float(t)), out))
    files2 = dict(files, imu=os.path.join(root, "imu_rate_unix.txt"), gnss=os.path.join(root, "gnss_unix.txt"), images=os.path.join(root, "cam1", "images.txt"))
    summ = np.zeros(16)
    err = ErrBuf(1024)
    rc = lib.icgh_replay_run(files2["config"].encode(), None, files2["imu"].encode(), files2["gnss"].encode(), files2["images"].encode(), 1, C.c_double(0),
                             C.c_double(0), summ.ctypes.data_as(C.c_void_p), *err.args)
    assert rc == 0, err.value
    S2 = dict(zip(SUMMARY_KEYS, summ))
    # the first IMU line only initialises dt in both flavours; the rate file was derived with a 5 ms first interval
    for k in ("gnss", "frames", "frames_tracked", "keyframes", "marginalizations", "lost", "final_state"):
        assert S[k] == S2[k], (k, S[k], S2[k])
    other = np.loadtxt(os.path.join(files["out"], "trajectory.csv"))
    assert other.shape == base.shape
    assert np.abs(other[:, 0] - base[:, 0]).max() < 1e-5  # Unix stamps near 1.6e9 resolve 2.4e-7 s
    assert np.abs(other[:, 1:4] - base[:, 1:4]).max() < 2e-3 and np.abs(other[:, 4:8] - base[:, 4:8]).max() < 1e-4
    return S2


def check_against_reference_estimator(lib_path, tmp_root, golden_path, write_kwargs=None, blank=None, n_keyframe_features_exact=10, pos_tol=0.05):
    """icg::GVINS against the REFERENCE's own estimator on the same input files (tests/golden/gvins_ref_golden.npz: ic_gvins.cc compiled
    unmodified on interface shims, one run of its three threads).  The reference's output depends on thread timing and its solver there is a
    restated LM, so the comparison is: identical discrete structure (navigation-line stamps, keyframe stamps and spacing, tracked-frame
    stamps), the GNSS/INS phase before the first image to 0.1 mm, the first window's reprojection statistics to 1e-6 px, and the whole
    trajectory within 5 cm / 0.2 deg — the level at which two runs of the reference itself differ (3 cm between pacings)."""
    import zlib
    lib = C.CDLL(H.tools_lib(lib_path))
    seq = gd.Sequence(lib)
    files = seq.write(str(tmp_root), **(write_kwargs or {}))
    if blank:  # a stretch of black images: tracking loss and re-initialization
        for name in [line.split()[1] for line in open(files["images"])][blank[0]:blank[1]]:
            with open(os.path.join(str(tmp_root), "cam0", name), "wb") as f:
                f.write(b"P5\n%d %d\n255\n" % (seq.w, seq.h) + bytes(seq.w * seq.h))
    g = np.load(golden_path)
    root = os.path.dirname(files["images"])
    names = [line.split()[1] for line in open(files["images"])]
    crc = [zlib.crc32(open(files["imu"], "rb").read()), zlib.crc32(open(files["gnss"], "rb").read())]
    crc += [zlib.crc32(open(os.path.join(root, n), "rb").read()) for n in (names[0], names[len(names) // 2], names[-1])]
    assert list(g["checksums"]) == crc, "the synthetic sequence is not byte-identical to the one the golden was made from"
    S = run_replay(lib, files)
    assert S["final_state"] == int(g["final_state"]) == STATE_TRACKING_NORMAL
    return compare_result_files_with_reference_golden(files["out"], g, n_keyframe_features_exact, pos_tol)


def compare_result_files_with_reference_golden(out_dir, g, n_keyframe_features_exact=10, pos_tol=0.05):
    """the result files of one estimator run (trajectory.csv, gvins.nav, statistics.txt, tracking.txt, mappoint.txt, IMU_ERR.bin, extrinsic.txt
    under out_dir) against the arrays of a reference-estimator golden; tolerances: see check_against_reference_estimator"""
    files = {"out": out_dir}
    load = lambda name: np.loadtxt(os.path.join(files["out"], name))
    traj, nav, stat, track, mpts = load("trajectory.csv"), load("gvins.nav"), load("statistics.txt"), load("tracking.txt"), load("mappoint.txt")
    rt, rn, rs, rk, rm = g["trajectory"], g["nav"], g["statistics"], g["tracking"], g["mappoints"]
    # structure
    assert traj.shape == rt.shape and np.abs(traj[:, 0] - rt[:, 0]).max() < 1e-6
    # frame stamps carry the (possibly estimated, ~1e-5 s) camera time delay: 1 ms separates frames that are 50 ms apart.  The keyframe
    # decision is a parallax threshold, and in the reference the poses it is computed from depend on when its optimizer thread handed its
    # result over: one of its runs in a few picks a keyframe one frame later somewhere in the second half and stays shifted from there on.
    # Required: the same number of keyframes (+-1), identical keyframes over at least the first 20, and the per-keyframe columns on that part.
    assert abs(len(stat) - len(rs)) <= 1 and abs(len(track) - len(rk)) <= 1
    n = min(len(stat), len(rs))
    same = np.abs(stat[:n, 0] - rs[:n, 0]) < 1e-3
    m = n if same.all() else int(np.argmin(same))
    assert m >= 20, (m, stat[:n, 0] - rs[:n, 0])
    stat, rs = stat[:m], rs[:m]
    assert np.abs(stat[:, 1] - rs[:, 1]).max() < 1e-3 and np.array_equal(stat[:, 2], rs[:, 2])  # spacing and frame-id differences
    nt = min(len(track), len(rk))
    assert (np.abs(track[:nt, 0] - rk[:nt, 0]) < 1e-3).sum() >= min(nt, 20)
    k = n_keyframe_features_exact
    assert np.array_equal(stat[:k, 3], rs[:k, 3]) and np.abs(stat[:, 3] - rs[:, 3]).max() <= 10   # feature counts of the keyframes
    assert abs(len(mpts) - len(rm)) <= 15
    # numbers
    pre = traj[:, 0] < gd.T0 + 3.5  # GNSS/INS only: no image has been processed yet
    assert np.abs(traj[pre, 1:] - rt[pre, 1:]).max() < 1e-4, np.abs(traj[pre, 1:] - rt[pre, 1:]).max()
    assert np.abs(stat[0, 4:8] - rs[0, 4:8]).max() < 1e-6 and np.abs(stat[:, 4:8] - rs[:, 4:8]).max() < 0.25  # reprojection min / max / mean / rms [px]
    assert np.array_equal(stat[:, 8], rs[:, 8])  # successful steps of the first solve (the 5-iteration cap)
    dpos = np.linalg.norm(traj[:, 1:4] - rt[:, 1:4], axis=1)
    dq = np.abs(traj[:, 4:8] - rt[:, 4:8]).max(axis=1)
    assert dpos.max() < pos_tol and dq.max() < 2e-3, (dpos.max(), dq.max())
    assert np.abs(nav[:, 2:4] - rn[:, 2:4]).max() < 1e-6 and np.abs(nav[:, 8:11] - rn[:, 8:11]).max() < 0.25  # lat/lon [deg], attitude [deg] (single lines around a solve differ by a whole update)
    # IMU_ERR.bin (raw doubles as the reference writes them): the bias estimates follow the reference's
    ie, re_ = np.fromfile(os.path.join(files["out"], "IMU_ERR.bin"), np.float64).reshape(-1, 8), g["imu_err"]
    assert ie.shape == re_.shape and np.array_equal(ie[:, 0], re_[:, 0])
    assert np.abs(ie[pre][:, 1:7] - re_[pre][:, 1:7]).max() < 1e-3
    # a new estimate reaches the INS a few epochs later in the reference (its optimizer thread hands it over with try_lock), so single lines
    # around a window solve differ by a whole update: compare each line with the reference's lines at the same and the neighbouring stamps
    def line_difference(cols):
        best = np.full(len(ie), np.inf)
        for shift in (-1, 0, 1):
            idx = np.clip(np.arange(len(ie)) + shift, 0, len(re_) - 1)
            best = np.minimum(best, np.abs(ie[:, cols] - re_[idx][:, cols]).max(axis=1))
        return float(best.max())
    bias = dict(gyro_deg_per_h=line_difference(slice(1, 4)), acc_mgal=line_difference(slice(4, 7)))
    assert bias["gyro_deg_per_h"] < 20 and bias["acc_mgal"] < 800, bias  # of estimates that reach 70 deg/h and 1 700 mGal (weakly observable here)
    extra = {}
    if "extrinsic" in g.files and len(g["extrinsic"]):
        # extrinsic.txt: one row per window solve; while the block is constant (before the window is full) both repeat the configured value; the
        # lever arm is unobservable on this drive, so afterwards both estimates wander by metres in the same direction and both are kept out of the
        # states by the 1 m / 5 deg guard; the time delay stays within 1 ms in both
        ex, rx = np.atleast_2d(np.loadtxt(os.path.join(files["out"], "extrinsic.txt"))), g["extrinsic"]
        assert abs(len(ex) - len(rx)) <= 1
        const = np.all(np.abs(rx[:, 1:4] - rx[0, 1:4]) < 1e-9, axis=1)
        nconst = int(np.argmin(const)) if not const.all() else len(rx)
        assert np.allclose(ex[:nconst, 1:8], rx[:nconst, 1:8], atol=1e-6)
        assert np.abs(ex[:, 7]).max() < 1e-3 and np.abs(rx[:, 7]).max() < 1e-3
        if nconst < min(len(ex), len(rx)):
            a, b = ex[nconst:min(len(ex), len(rx)), 1:4] - rx[0, 1:4], rx[nconst:min(len(ex), len(rx)), 1:4] - rx[0, 1:4]
            cos = np.sum(a * b, axis=1) / (np.linalg.norm(a, axis=1) * np.linalg.norm(b, axis=1) + 1e-12)
            extra["extrinsic_direction_cosine_min"] = float(cos.min())
            assert np.median(cos) > 0.9, cos
    return dict(max_position_difference=float(dpos.max()), median_position_difference=float(np.median(dpos)), max_quaternion_difference=float(dq.max()), **bias, **extra)


def run_replay_lockstep(lib, files, outputs, groups=1):
    n = len(outputs)
    for o in outputs:
        os.makedirs(o, exist_ok=True)
    arr = (C.c_char_p * n)(*[o.encode() for o in outputs])
    summ = np.zeros((n, 16))
    wall = C.c_double(0)
    shared = np.zeros(3, np.int64)
    err = ErrBuf(1024)
    rc = lib.icgh_replay_run_lockstep(n, files["config"].encode(), arr, files["imu"].encode(), files["gnss"].encode(), files["images"].encode(), 0,
                                      int(groups), summ.ctypes.data_as(C.c_void_p), C.byref(wall), shared.ctypes.data_as(C.c_void_p), *err.args)
    assert rc == 0, (rc, err.text())
    return [dict(zip(SUMMARY_KEYS, row)) for row in summ], wall.value, [int(v) for v in shared]


def check_replay_lockstep(lib_path, tmp_root, n=3, bitwise=True, groups=1):
    """n estimators in lock-step on one thread, their window solves shared through one WindowSolverBatch: every stream's result files equal
    those of the stream replayed alone with its own WindowSolver"""
    lib = C.CDLL(H.tools_lib(lib_path))
    seq = gd.Sequence(lib)
    files = seq.write(str(tmp_root))
    S = run_replay(lib, files)
    alone = open(os.path.join(files["out"], "trajectory.csv"), "rb").read()
    alone_rows = np.loadtxt(os.path.join(files["out"], "trajectory.csv"))
    alone_stat = np.loadtxt(os.path.join(files["out"], "statistics.txt"))
    outs = [os.path.join(str(tmp_root), "lock%d" % k) for k in range(n)]
    SS, wall, shared = run_replay_lockstep(lib, files, outs, groups)
    assert shared[0] == n * (S["optimizations"] - 1)  # every solve but the GNSS/INS initialization one went through the driver
    assert shared[2] == -(-n // groups)  # identical streams become due in the same tick: all streams of a group share every batched solve
    for k, o in enumerate(outs):
        assert all(SS[k][key] == S[key] for key in ("imu", "gnss", "frames", "frames_tracked", "keyframes", "optimizations", "marginalizations", "lost", "final_state")), k
        rows = np.loadtxt(os.path.join(o, "trajectory.csv"))
        stat = np.loadtxt(os.path.join(o, "statistics.txt"))
        assert rows.shape == alone_rows.shape and stat.shape == alone_stat.shape
        if bitwise:
            assert open(os.path.join(o, "trajectory.csv"), "rb").read() == alone, (k, np.abs(rows - alone_rows).max())
            keep = [c for c in range(15) if c not in (10, 11, 12)]
            assert np.array_equal(stat[:, keep], alone_stat[:, keep])
        else:
            # (the step counts of columns 8 / 9 are compared on the CPU backend only: rounding can move a function-tolerance stop by one step)
            assert np.abs(rows - alone_rows).max() < 1e-3 and np.array_equal(stat[:, [0, 1, 2, 3, 13, 14]], alone_stat[:, [0, 1, 2, 3, 13, 14]])
    return SS, wall, shared


def check_replay_lockstep_different_streams(lib_path, tmp_root):
    """three DIFFERENT streams in one lock-step group — the plain sequence, the same drive with half a second of black images (loses track,
    re-initializes: its keyframes fall on other frames), and a drive with other sensor noise and a later first image — so the window solves of a
    tick form batches of one, two or three windows of different sizes: every stream still equals its own replay alone, bit for bit"""
    lib = C.CDLL(H.tools_lib(lib_path))
    root = str(tmp_root)
    sets = []
    seq = gd.Sequence(lib)
    sets.append(seq.write(os.path.join(root, "a")))
    b = seq.write(os.path.join(root, "b"))
    for name in [line.split()[1] for line in open(b["images"])][40:50]:
        with open(os.path.join(root, "b", "cam0", name), "wb") as f:
            f.write(b"P5\n%d %d\n255\n" % (seq.w, seq.h) + bytes(seq.w * seq.h))
    sets.append(b)
    sets.append(gd.Sequence(lib, seed=5, image_start=3.6, duration=7.0).write(os.path.join(root, "c"), track_max_features=120))
    alone = []
    for files in sets:
        S = run_replay(lib, files)
        alone.append((S, open(os.path.join(files["out"], "trajectory.csv"), "rb").read(), np.loadtxt(os.path.join(files["out"], "statistics.txt"))))
    n = len(sets)
    outs = [os.path.join(root, "lock%d" % k) for k in range(n)]
    for o in outs:
        os.makedirs(o, exist_ok=True)
    arr = lambda key: (C.c_char_p * n)(*[f[key].encode() for f in sets])
    summ, wall, shared, err = np.zeros((n, 16)), C.c_double(0), np.zeros(3, np.int64), ErrBuf(1024)
    rc = lib.icgh_replay_run_lockstep_files(n, arr("config"), (C.c_char_p * n)(*[o.encode() for o in outs]), arr("imu"), arr("gnss"), arr("images"), 1,
                                            summ.ctypes.data_as(C.c_void_p), C.byref(wall), shared.ctypes.data_as(C.c_void_p), *err.args)
    assert rc == 0, err.value
    solves = sum(int(a[0]["optimizations"]) - 1 for a in alone)
    assert shared[0] == solves and shared[1] < solves and 2 <= shared[2] <= n, shared  # some ticks batch several windows, not all of them all
    keep = [c for c in range(15) if c not in (10, 11, 12)]
    for k in range(n):
        S, traj, stat = alone[k]
        got = dict(zip(SUMMARY_KEYS, summ[k]))
        assert all(got[key] == S[key] for key in ("imu", "gnss", "frames", "frames_tracked", "keyframes", "optimizations", "marginalizations", "lost", "final_state")), k
        assert open(os.path.join(outs[k], "trajectory.csv"), "rb").read() == traj, k
        assert np.array_equal(np.loadtxt(os.path.join(outs[k], "statistics.txt"))[:, keep], stat[:, keep]), k
    assert alone[1][0]["lost"] == 1 and alone[0][0]["lost"] == 0
    return [int(v) for v in shared]


def lockstep_marg_counts(lib):
    """(batches, windows) that went through a MarginalizationBatch in the lock-step runs since the last call"""
    out = np.zeros(2, np.int64)
    lib.icgh_replay_lockstep_marg_counts(out.ctypes.data_as(C.c_void_p))
    return int(out[0]), int(out[1])


def check_replay_lockstep_shared_marginalizations(lib_path, tmp_root, bitwise=True):
    """ICG_LOCKSTEP_MARG_BATCH=1: the marginalizations of a tick go through ONE MarginalizationBatch (host/marg_batch.h) as the window solves
    go through one WindowSolverBatch — identical streams (every batch holds all windows) and three different streams (batches of one, two
    or three windows; a stream that loses track and re-initializes): every stream still equals its own replay alone."""
    lib = C.CDLL(H.tools_lib(lib_path))
    old = os.environ.get("ICG_LOCKSTEP_MARG_BATCH")
    os.environ["ICG_LOCKSTEP_MARG_BATCH"] = "1"
    try:
        lockstep_marg_counts(lib)
        SS, _, _ = check_replay_lockstep(lib_path, os.path.join(str(tmp_root), "same"), n=3, bitwise=bitwise, groups=1)
        batches, windows = lockstep_marg_counts(lib)
        n_marg = int(SS[0]["marginalizations"])
        # (a marginalization without reprojection factors — the oldest keyframe anchors no landmark — stays with its estimator)
        assert n_marg > 0 and windows == 3 * batches and n_marg - 4 <= batches <= n_marg, (batches, windows, n_marg)
        if bitwise:
            check_replay_lockstep_different_streams(lib_path, os.path.join(str(tmp_root), "diff"))
            batches, windows = lockstep_marg_counts(lib)
            assert windows > batches > 0, (batches, windows)  # some ticks marginalize several windows together, not all of them all
    finally:
        if old is None:
            os.environ.pop("ICG_LOCKSTEP_MARG_BATCH", None)
        else:
            os.environ["ICG_LOCKSTEP_MARG_BATCH"] = old
    return batches, windows


def check_replay_lockstep_wide_windows(lib_path, tmp_root, n=2, bitwise=True):
    """15-keyframe windows (BASELINE configs[3]; reference ic_gvins.cc:137,153 runs any optimize_windows_size): 97 free camera columns are a
    76 KB LDS tile of the batched assembly — within the 160 KiB of a gfx950 CU (WindowSolverBatch::kMaxCameraColumns = 138; rounds 2-4 capped
    the tile at 64 KB and solved such windows alone).  Every solve goes through the shared WindowSolverBatch and every stream still equals
    its own replay alone (bit for bit on the CPU backend)."""
    lib = C.CDLL(H.tools_lib(lib_path))
    seq = gd.Sequence(lib)
    files = seq.write(str(tmp_root), optimize_windows_size=15)
    S = run_replay(lib, files)
    alone = open(os.path.join(files["out"], "trajectory.csv"), "rb").read()
    alone_rows = np.loadtxt(os.path.join(files["out"], "trajectory.csv"))
    outs = [os.path.join(str(tmp_root), "lock%d" % k) for k in range(n)]
    SS, _, shared = run_replay_lockstep(lib, files, outs, 1)
    assert shared[0] == n * (S["optimizations"] - 1)
    batched_windows_upper = shared[1] * n
    assert 0 < shared[1] and batched_windows_upper == shared[0], shared  # narrow and wide windows alike are batched
    for k, o in enumerate(outs):
        assert all(SS[k][key] == S[key] for key in ("frames_tracked", "keyframes", "optimizations", "marginalizations", "lost", "final_state")), k
        if bitwise:
            assert open(os.path.join(o, "trajectory.csv"), "rb").read() == alone, k
        else:  # (on the device the FP64-atomic assembly reorders sums from launch to launch)
            rows = np.loadtxt(os.path.join(o, "trajectory.csv"))
            assert rows.shape == alone_rows.shape and np.abs(rows - alone_rows).max() < 1e-3, k
    return shared
