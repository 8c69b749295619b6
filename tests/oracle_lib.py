"""ctypes wrappers around oracle/liboracle.so (TEST INFRASTRUCTURE ONLY: tests/, smoke(), bench cpu_baseline)."""
import ctypes as C
import os
import subprocess

import numpy as np

from ctypes_util import f32, f64, i32, ptr, u8

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ORACLE_DIR = os.path.join(ROOT, "oracle")
ORACLE_SO = os.path.join(ORACLE_DIR, "liboracle.so")


class Oracle:
    def __init__(self, lib):
        self.lib = lib
        lib.orc_histogram_mean.restype = C.c_double

    # ---- factors
    def reproj_eval(self, obs_soa, idx_i, idx_j, idx_lm, poses, ext, invdepth, td, want_jac=True, huber=0.0):
        obs_soa = f64(obs_soa)
        n = obs_soa.shape[1]
        r = np.zeros((n, 2))
        J = np.zeros((n, 46))
        self.lib.orc_reproj_eval_batch(n, ptr(obs_soa), ptr(i32(idx_i)), ptr(i32(idx_j)), ptr(i32(idx_lm)), ptr(f64(poses)),
                                       ptr(f64(ext)), ptr(f64(invdepth)), C.c_double(td), 1 if want_jac else 0, ptr(r), ptr(J))
        if huber > 0:
            self.lib.orc_huber_correct_2x46(n, C.c_double(huber), ptr(r), ptr(J) if want_jac else None)
        return r, (J if want_jac else None)

    def reproj_eval_one(self, obs15, pose_i, pose_j, ext, invdepth, td, want_jac=True):
        r = np.zeros(2)
        J = np.zeros(46)
        self.lib.orc_reproj_eval_one(ptr(f64(obs15)), ptr(f64(pose_i)), ptr(f64(pose_j)), ptr(f64(ext)), C.c_double(invdepth),
                                     C.c_double(td), 1 if want_jac else 0, ptr(r), ptr(J))
        return r, J

    # ---- image
    def bgr2gray(self, bgr):
        bgr = u8(bgr)
        h, w, _ = bgr.shape
        out = np.zeros((h, w), np.uint8)
        self.lib.orc_bgr2gray(ptr(bgr), w, h, w * 3, ptr(out), w)
        return out

    def histogram_mean(self, img):
        img = u8(img)
        h, w = img.shape
        return self.lib.orc_histogram_mean(ptr(img), w, h, w)

    def clahe(self, img, clip=3.0, tiles=21, want_lut=False):
        img = u8(img)
        h, w = img.shape
        out = np.zeros_like(img)
        lut = np.zeros((tiles * tiles, 256), np.uint8)
        self.lib.orc_clahe(ptr(img), w, h, w, C.c_double(clip), tiles, ptr(out), w, ptr(lut))
        return (out, lut) if want_lut else out

    def pyrdown(self, img):
        img = u8(img)
        h, w = img.shape
        out = np.zeros(((h + 1) // 2, (w + 1) // 2), np.uint8)
        self.lib.orc_pyrdown(ptr(img), w, h, w, ptr(out), out.shape[1])
        return out

    def scharr(self, img):
        img = u8(img)
        h, w = img.shape
        out = np.zeros((h, w, 2), np.int16)
        self.lib.orc_scharr(ptr(img), w, h, w, ptr(out))
        return out

    # ---- LK
    def lk_track(self, prev, nxt, prev_pts, guess):
        prev, nxt = u8(prev), u8(nxt)
        h, w = prev.shape
        prev_pts = f32(prev_pts).reshape(-1, 2)
        n = prev_pts.shape[0]
        out = f32(guess).reshape(-1, 2).copy()
        st = np.zeros(n, np.uint8)
        err = np.zeros(n, np.float32)
        self.lib.orc_lk_track(ptr(prev), ptr(nxt), w, h, w, n, ptr(prev_pts), ptr(out), ptr(st), ptr(err))
        return out, st, err

    LK_EXITS = {"none": 0, "skipped": 1, "weak": 2, "out": 3, "converged": 4, "oscillation": 5, "cap": 6}  # oracle.h ORC_LK_EXIT_*

    def lk_track_trace(self, prev, nxt, prev_pts, guess):
        """lk_track plus, per point and pyramid level (axis 1, level 0 = full resolution): exit kind (LK_EXITS), iterations, in-level travel of
        the integer window position, the exact int64 window sums A (A11, A12, A22) and the largest |b1|, |b2|"""
        prev, nxt = u8(prev), u8(nxt)
        h, w = prev.shape
        prev_pts = f32(prev_pts).reshape(-1, 2)
        n = prev_pts.shape[0]
        out = f32(guess).reshape(-1, 2).copy()
        st = np.zeros(n, np.uint8)
        err = np.zeros(n, np.float32)
        tr = dict(exit=np.zeros((n, 4), np.int32), iters=np.zeros((n, 4), np.int32), travel=np.zeros((n, 4), np.int32),
                  A=np.zeros((n, 4, 3), np.int64), bmax=np.zeros((n, 4, 2), np.int64))
        tr["levels"] = self.lib.orc_lk_track_trace(ptr(prev), ptr(nxt), w, h, w, n, ptr(prev_pts), ptr(out), ptr(st), ptr(err), ptr(tr["exit"]),
                                                   ptr(tr["iters"]), ptr(tr["travel"]), ptr(tr["A"]), ptr(tr["bmax"]))
        return out, st, err, tr

    def lk_track_fb(self, prev, nxt, prev_pts, guess):
        prev, nxt = u8(prev), u8(nxt)
        h, w = prev.shape
        prev_pts = f32(prev_pts).reshape(-1, 2)
        guess = f32(guess).reshape(-1, 2)
        n = prev_pts.shape[0]
        out = np.zeros((n, 2), np.float32)
        st = np.zeros(n, np.uint8)
        self.lib.orc_lk_track_fb(ptr(prev), ptr(nxt), w, h, w, n, ptr(prev_pts), ptr(guess), ptr(out), ptr(st))
        return out, st

    # ---- camera
    def undistort(self, cam, pts):
        p = f32(pts).reshape(-1, 2).copy()
        self.lib.orc_undistort_points(ptr(f64(cam)), p.shape[0], ptr(p))
        return p

    def distort(self, cam, pts):
        p = f32(pts).reshape(-1, 2).copy()
        self.lib.orc_distort_points(ptr(f64(cam)), p.shape[0], ptr(p))
        return p

    def world2pixel(self, cam, pose12, pw):
        pw = f64(pw).reshape(-1, 3)
        out = np.zeros((pw.shape[0], 2), np.float32)
        self.lib.orc_world2pixel(ptr(f64(cam)), ptr(f64(pose12)), pw.shape[0], ptr(pw), ptr(out))
        return out

    def pixel2cam(self, cam, pts):
        pts = f32(pts).reshape(-1, 2)
        out = np.zeros((pts.shape[0], 3))
        self.lib.orc_pixel2cam(ptr(f64(cam)), pts.shape[0], ptr(pts), ptr(out))
        return out

    def predict_rotation(self, cam, R_cur, R_pre, pts):
        pts = f32(pts).reshape(-1, 2)
        out = np.zeros_like(pts)
        self.lib.orc_predict_rotation(ptr(f64(cam)), ptr(f64(R_cur)), ptr(f64(R_pre)), pts.shape[0], ptr(pts), ptr(out))
        return out


    # ---- detection
    def draw_circle(self, mask, cx, cy, r, value=0):
        h, w = mask.shape
        self.lib.orc_draw_filled_circle(ptr(mask), w, h, mask.strides[0], int(cx), int(cy), int(r), int(value))

    def circle_halfwidths(self, r):
        hw = np.zeros(r + 1, np.int32)
        self.lib.orc_circle_halfwidths(int(r), ptr(hw))
        return hw

    def min_eigen_map(self, img, roi):
        img = u8(img)
        h, w = img.shape
        rx, ry, rw, rh = roi
        eig = np.zeros((rh, rw), np.float32)
        self.lib.orc_min_eigen_map(ptr(img), w, h, w, rx, ry, rw, rh, ptr(eig))
        return eig

    def good_features(self, img, mask, roi, max_corners, quality, min_dist):
        img = u8(img)
        h, w = img.shape
        rx, ry, rw, rh = roi
        out = np.zeros((max_corners, 2), np.float32)
        m = None if mask is None else u8(mask)
        n = self.lib.orc_good_features(ptr(img), w, h, w, ptr(m), w, rx, ry, rw, rh, max_corners, C.c_double(quality),
                                       C.c_double(min_dist), ptr(out))
        return out[:n]

    def corner_subpix(self, img, roi, corners):
        img = u8(img)
        h, w = img.shape
        rx, ry, rw, rh = roi
        c = f32(corners).reshape(-1, 2).copy()
        self.lib.orc_corner_subpix(ptr(img), w, h, w, rx, ry, rw, rh, c.shape[0], ptr(c))
        return c

    SUBPIX_EXITS = {"converged": 1, "cap": 2, "out": 3, "singular": 4}  # oracle.h ORC_SUBPIX_EXIT_*

    def corner_subpix_trace(self, img, roi, corners):
        """corner_subpix plus, per corner: iterations entered, exit kind (SUBPIX_EXITS) and whether the 5-px reset fired"""
        img = u8(img)
        h, w = img.shape
        rx, ry, rw, rh = roi
        c = f32(corners).reshape(-1, 2).copy()
        n = c.shape[0]
        iters, kind, reset = np.zeros(n, np.int32), np.zeros(n, np.int32), np.zeros(n, np.int32)
        self.lib.orc_corner_subpix_trace(ptr(img), w, h, w, rx, ry, rw, rh, n, ptr(c), ptr(iters), ptr(kind), ptr(reset))
        return c, iters, kind, reset

    def subpix_mask(self):
        m = np.zeros(121, np.float32)
        self.lib.orc_subpix_mask(ptr(m))
        return m

    def detect(self, img, grid6, mask_pts, quota, max_out):
        img = u8(img)
        h, w = img.shape
        mask_pts = f32(mask_pts).reshape(-1, 2)
        out = np.zeros((max_out, 2), np.float32)
        blk = np.zeros(max_out, np.int32)
        n = self.lib.orc_detect(ptr(img), w, h, w, ptr(i32(grid6)), mask_pts.shape[0], ptr(mask_pts), ptr(i32(quota)), max_out,
                                ptr(out), ptr(blk))
        return out[:n], blk[:n]

    # ---- RANSAC / triangulation
    def seven_point(self, m1, m2):
        F = np.zeros((3, 9))
        n = self.lib.orc_seven_point(ptr(f64(m1)), ptr(f64(m2)), ptr(F))
        return F[:n].reshape(n, 3, 3)

    def fm_score(self, F, pts1, pts2, thresh):
        pts1, pts2 = f32(pts1).reshape(-1, 2), f32(pts2).reshape(-1, 2)
        mask = np.zeros(pts1.shape[0], np.uint8)
        n = self.lib.orc_fm_score(ptr(f64(F)), pts1.shape[0], ptr(pts1), ptr(pts2), C.c_double(thresh), ptr(mask))
        return n, mask

    def ransac_subsets(self, n_points, n_hyp, pts1=None, pts2=None):
        """hypothesis index stream of getSubset; with pts1/pts2 the FMEstimatorCallback::checkSubset rejection is applied"""
        idx = np.zeros((n_hyp, 7), np.int32)
        a = None if pts1 is None else f32(pts1)
        b = None if pts2 is None else f32(pts2)
        n = self.lib.orc_ransac_subsets(n_points, ptr(a), ptr(b), n_hyp, ptr(idx))
        return idx[:n]

    def solve_cubic(self, coeffs4):
        r = np.zeros(3)
        n = self.lib.orc_solve_cubic(ptr(f64(coeffs4)), ptr(r))
        return r[:n]

    def have_collinear_points(self, pts):
        pts = f32(pts)
        return bool(self.lib.orc_have_collinear_points(ptr(pts), pts.shape[0]))

    def fm_ransac(self, pts1, pts2, thresh=1.5, conf=0.99):
        pts1, pts2 = f32(pts1).reshape(-1, 2), f32(pts2).reshape(-1, 2)
        n = pts1.shape[0]
        mask = np.zeros(n, np.uint8)
        F = np.zeros(9)
        it = C.c_int(0)
        ok = self.lib.orc_find_fundamental_ransac(n, ptr(pts1), ptr(pts2), C.c_double(thresh), C.c_double(conf), ptr(mask), ptr(F),
                                                  C.byref(it))
        return ok, mask, F.reshape(3, 3), it.value

    def triangulate(self, T0, T1, pc0, pc1):
        pw = np.zeros(3)
        self.lib.orc_triangulate_point(ptr(f64(T0)), ptr(f64(T1)), ptr(f64(pc0)), ptr(f64(pc1)), ptr(pw))
        return pw


    # ---- preintegration
    def preint_integrate(self, variant, imu, state0, params):
        imu = f64(imu).reshape(-1, 8)
        n = imu.shape[0]
        cur, delta = np.zeros(16), np.zeros(16)
        jac, cov = np.zeros((15, 15)), np.zeros((15, 15))
        dt = C.c_double(0)
        pn = np.zeros((max(n - 1, 1), 4))
        self.lib.orc_preint_integrate(int(variant), n, ptr(imu), ptr(f64(state0)), ptr(f64(params)), ptr(cur), ptr(delta), ptr(jac),
                                      ptr(cov), C.byref(dt), ptr(pn))
        return dict(cur=cur, delta=delta, jac=jac, cov=cov, dt=dt.value, pn=pn[:n - 1])

    def preint_evaluate(self, variant, pre, gravity3, iewn3, pose0, mix0, pose1, mix1, want_jac=True):
        r = np.zeros(15)
        J = np.zeros(15 * 32) if want_jac else None
        pn = f64(pre["pn"])
        self.lib.orc_preint_evaluate(int(variant), ptr(f64(pre["delta"])), ptr(f64(pre["jac"])), ptr(f64(pre["cov"])),
                                     C.c_double(pre["dt"]), ptr(f64(gravity3)), ptr(f64(iewn3)), pn.shape[0], ptr(pn), None,
                                     ptr(f64(pose0)), ptr(f64(mix0)), ptr(f64(pose1)), ptr(f64(mix1)), ptr(r), ptr(J))
        if not want_jac:
            return r, None
        return r, (J[:105].reshape(15, 7), J[105:240].reshape(15, 9), J[240:345].reshape(15, 7), J[345:].reshape(15, 9))


    # ---- marginalization
    def sym_eigen(self, A):
        A = f64(A)
        n = A.shape[0]
        ev, V = np.zeros(n), np.zeros((n, n))
        self.lib.orc_sym_eigen(n, ptr(A), ptr(ev), ptr(V))
        return ev, V

    def reproj_accumulate_normal(self, r, J, idx_i, idx_j, idx_lm, col_pose, col_ext, col_lm, col_td, local_size):
        H, b = np.zeros((local_size, local_size)), np.zeros(local_size)
        r, J = f64(r), f64(J)
        self.lib.orc_reproj_accumulate_normal(r.shape[0], ptr(r), ptr(J), ptr(i32(idx_i)), ptr(i32(idx_j)), ptr(i32(idx_lm)),
                                              ptr(i32(col_pose)), int(col_ext), ptr(i32(col_lm)), int(col_td), local_size, ptr(H), ptr(b))
        return H, b

    def marginalize(self, H0, b0, m, eps=1e-8):
        H0, b0 = f64(H0), f64(b0)
        n = H0.shape[0]
        r = n - m
        J0, e0, Hp, bp = np.zeros((r, r)), np.zeros(r), np.zeros((r, r)), np.zeros(r)
        self.lib.orc_marginalize(n, m, ptr(H0), ptr(b0), C.c_double(eps), ptr(J0), ptr(e0), ptr(Hp), ptr(bp))
        return J0, e0, Hp, bp

    def marg_factor_eval(self, block_size, block_index, x0, x, J0, e0, want_jac=True):
        r = J0.shape[0]
        res = np.zeros(r)
        jac = np.zeros(r * int(np.sum(block_size))) if want_jac else None
        self.lib.orc_marg_factor_eval(r, len(block_size), ptr(i32(block_size)), ptr(i32(block_index)), ptr(f64(x0)), ptr(f64(x)),
                                      ptr(f64(J0)), ptr(f64(e0)), ptr(res), ptr(jac))
        return res, jac


def build():
    subprocess.run(["make", "-s", "-C", ORACLE_DIR], check=True)


def load():
    if not os.path.exists(ORACLE_SO):
        build()
    return Oracle(C.CDLL(ORACLE_SO))
