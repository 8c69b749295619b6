"""ctypes binding of libicgvins_hip.so (the C ABI in include/icgvins_hip.h).

This is plumbing for tests/bench: the product is the shared library.  There is NO CPU fallback here — if the
HIP library is missing or no GPU is visible, construction fails loudly.
"""
import ctypes as C
import os

import numpy as np

from ctypes_util import ErrBuf, f32, f64, i32, u8
from ctypes_util import ptr as _p  # (Context's methods have parameters named ptr)

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.path.join(_HERE, "libicgvins_hip.so")

EXPORTS = [
    "icg_ctx_create", "icg_ctx_destroy", "icg_last_error", "icg_ctx_sync", "icg_ctx_set_wait_mode", "icg_ctx_stream", "icg_set_camera",
    "icg_version", "icg_pyramid_levels", "icg_prof_enable", "icg_prof_get", "icg_prof_names", "icg_dev_alloc",
    "icg_dev_free", "icg_dev_upload", "icg_dev_download", "icg_frames_preprocess", "icg_frame_download",
    "icg_lk_track", "icg_lk_track_fb", "icg_undistort_points", "icg_distort_points", "icg_predict_mappoints",
    "icg_predict_rotation", "icg_fm_ransac", "icg_fm_ransac_device", "icg_detect", "icg_triangulate", "icg_reproj_eval_batch",
    "icg_reproj_set_factors", "icg_reproj_stage_factors", "icg_reproj_commit_factors", "icg_reproj_eval_resident", "icg_reproj_accumulate_normal", "icg_preint_batch", "icg_preint_evaluate_batch",
    "icg_ins_mechanize_batch", "icg_ins_camera_pose_batch", "icg_reproj_schur", "icg_reproj_backsub", "icg_reproj_cost", "icg_reproj_landmark_diag",
    "icg_reproj_error_batch", "icg_reproj_set_windows", "icg_reproj_eval_windows", "icg_reproj_schur_windows",
    "icg_reproj_schur_windows_view", "icg_reproj_reserve_windows", "icg_reproj_eval_resident_view", "icg_reproj_backsub_windows", "icg_reproj_cost_windows", "icg_reproj_fetch_residuals", "icg_reproj_chi2_cull",
    "icg_reproj_landmark_diag_windows",
    "icg_marg_prior_set", "icg_marg_prior_evaluate", "icg_marg_linearize_batch",
    "icg_chol_solve_batch", "icg_reproj_schur_windows_resident", "icg_reproj_solve_windows", "icg_reproj_host_parts_build",
    "icg_marg_prior_evaluate_resident", "icg_reproj_host_parts_build_prior",
    "icg_marg_linearize_batch_keep", "icg_marg_linearized_release", "icg_marg_prior_set_from_kept", "icg_marg_linearize_resident",
    "icg_reproj_landmark_min_windows",
    "icg_preint_set", "icg_preint_evaluate_resident", "icg_preint_fetch_resident", "icg_reproj_host_parts_build_preint",
    "icg_preint_odo_batch", "icg_preint_odo_evaluate_batch",
    "icg_preint_odo_set", "icg_preint_odo_evaluate_resident", "icg_preint_odo_fetch_resident", "icg_reproj_host_parts_build_preint_odo",
    "icg_set_cameras", "icg_lk_track_fb_cams", "icg_reproj_error_batch_cams", "icg_tracker_create_cams",
    "icg_nav_set", "icg_nav_evaluate_resident", "icg_nav_correct_resident", "icg_nav_fetch_resident", "icg_reproj_host_parts_build_nav",
    "icg_preint_batch_params", "icg_preint_odo_batch_params",
]


MARG_MAX_R = 1024  # ICG_MARG_MAX_R of include/icgvins_hip.h
MARG_LIN_MAX_P = 512  # ICG_MARG_LIN_MAX_P
CHOL_MAX_N = 512  # ICG_CHOL_MAX_N
HOST_PART_MAX_NR = 1024  # ICG_HOST_PART_MAX_NR
HP_JAC_FROM_PRIOR = -2  # ICG_HP_JAC_FROM_PRIOR
HP_JAC_FROM_PREINT = -3  # ICG_HP_JAC_FROM_PREINT
HP_JAC_FROM_PREINT_ODO = -4  # ICG_HP_JAC_FROM_PREINT_ODO
HP_JAC_FROM_NAV = -5  # ICG_HP_JAC_FROM_NAV
PREINT_SET_MAX = 65535 * 16  # ICG_PREINT_SET_MAX
NAV_SET_MAX = 65535  # ICG_NAV_SET_MAX
NAV_SHAPES = {0: (3, 7), 1: (6, 9), 2: (6, 7), 3: (9, 9), 4: (7, 10), 5: (10, 10)}  # residuals x block width by kind of navigation factor


class IcgError(RuntimeError):
    pass


class CtxConfig(C.Structure):
    _fields_ = [("device", C.c_int), ("width", C.c_int), ("height", C.c_int), ("n_slots", C.c_int),
                ("max_batch", C.c_int), ("max_points", C.c_int), ("max_factors", C.c_int)]


class Camera(C.Structure):
    _fields_ = [(k, C.c_double) for k in ("fx", "fy", "cx", "cy", "skew", "k1", "k2", "p1", "p2", "k3")]


class DetectGrid(C.Structure):
    _fields_ = [(k, C.c_int) for k in ("block_cols", "block_rows", "block_w", "block_h", "min_dist", "max_per_block")]


def load_library(path=LIB_PATH):
    if not os.path.exists(path):
        raise IcgError(f"{path} not found: build it with `python -c 'import __graft_entry__ as g; g.build()'`. "
                       "There is no CPU fallback.")
    lib = C.CDLL(path)
    lib.icg_last_error.restype = C.c_char_p
    lib.icg_last_error.argtypes = [C.c_void_p]
    lib.icg_version.restype = C.c_char_p
    lib.icg_ctx_stream.restype = C.c_void_p
    lib.icg_ctx_stream.argtypes = [C.c_void_p]
    lib.icg_ctx_destroy.argtypes = [C.c_void_p]
    lib.icg_ctx_destroy.restype = None
    return lib


class Context:
    """One icg_ctx: a HIP stream + resident frame slots on one MI355X."""

    def __init__(self, width, height, n_slots=4, max_batch=2, max_points=4096, max_factors=0, device=0, lib=None):
        self.lib = lib or load_library()
        cfg = CtxConfig(device, width, height, n_slots, max_batch, max_points, max_factors)
        h = C.c_void_p()
        rc = self.lib.icg_ctx_create(C.byref(cfg), C.byref(h))
        if rc != 0:
            raise IcgError(f"icg_ctx_create failed rc={rc}: {self.lib.icg_last_error(None).decode()}")
        self.h = h
        self.width, self.height = width, height
        self.n_slots, self.max_batch = n_slots, max_batch

    def close(self):
        if getattr(self, "h", None):
            self.lib.icg_ctx_destroy(self.h)
            self.h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def _ck(self, rc, what):
        if rc != 0:
            raise IcgError(f"{what} failed rc={rc}: {self.lib.icg_last_error(self.h).decode()}")

    # ---- misc
    def sync(self):
        self._ck(self.lib.icg_ctx_sync(self.h), "icg_ctx_sync")

    def levels(self):
        return self.lib.icg_pyramid_levels(self.h)

    def set_camera(self, cam10):
        cam = Camera(*[float(v) for v in cam10])
        self._ck(self.lib.icg_set_camera(self.h, C.byref(cam)), "icg_set_camera")

    def set_cameras(self, cams):
        """the context's camera table (n x 10): what the *_cams entries index"""
        cams = f64(cams).reshape(-1, 10)
        self._ck(self.lib.icg_set_cameras(self.h, cams.shape[0], _p(cams)), "icg_set_cameras")

    def prof_enable(self, on=True):
        self._ck(self.lib.icg_prof_enable(self.h, 1 if on else 0), "icg_prof_enable")

    def prof(self):
        buf = ErrBuf(4096)
        self._ck(self.lib.icg_prof_names(self.h, *buf.args), "icg_prof_names")
        out = {}
        for name in buf.text().split("\n"):
            if not name:
                continue
            n, ms = C.c_int(), C.c_double()
            self.lib.icg_prof_get(self.h, name.encode(), C.byref(n), C.byref(ms))
            out[name] = (n.value, ms.value)
        return out

    def dev_alloc(self, nbytes):
        p = C.c_void_p()
        self._ck(self.lib.icg_dev_alloc(self.h, C.c_size_t(nbytes), C.byref(p)), "icg_dev_alloc")
        return p.value

    def dev_free(self, ptr):
        self._ck(self.lib.icg_dev_free(self.h, C.c_void_p(ptr)), "icg_dev_free")

    def dev_upload(self, ptr, arr):
        arr = np.ascontiguousarray(arr)
        self._ck(self.lib.icg_dev_upload(self.h, C.c_void_p(ptr), _p(arr), C.c_size_t(arr.nbytes)), "icg_dev_upload")

    # ---- F1
    def preprocess(self, slots, images, want_hist=False):
        """images: list of HxW (or HxWx3) uint8 arrays (host)."""
        n = len(slots)
        imgs = [np.ascontiguousarray(im, dtype=np.uint8) for im in images]
        ch = 3 if imgs[0].ndim == 3 else 1
        stride = imgs[0].strides[0]
        ptrs = (C.c_void_p * n)(*[im.ctypes.data for im in imgs])
        hist = np.zeros(n, np.float64) if want_hist else None
        self._ck(self.lib.icg_frames_preprocess(self.h, n, _p(i32(slots)), ptrs, stride, ch, 0, _p(hist)),
                 "icg_frames_preprocess")
        # without want_hist the call returns with the upload still in flight: a frame that had to be copied to make it contiguous uint8 is a
        # temporary of this function and must outlive the upload (a column-major frame came out as garbage from some row on, a different row every run)
        if hist is None and any(a is not b for a, b in zip(imgs, images)):
            self.sync()
        return hist

    def preprocess_device(self, slots, dev_ptrs, stride, channels=1, want_hist=False):
        """dev_ptrs: frames that already live in device memory, rows `stride` bytes apart (stride >= width * channels).

        Allocation contract: gray frames whose stride and pointers are all multiples of 4 are read IN PLACE, as aligned dwords: the kernels
        then read up to 3 bytes past the last pixel of a row (never selected into a result), so every frame must lie in an allocation that
        extends at least stride * height + 16 bytes from the frame's pointer, and must stay unchanged until the call's kernels have run
        (the call is asynchronous unless want_hist).  What lies in the stride gap does not matter: the histogram, the LUTs and the output
        see the width * height pixels only.  Any other batch (an odd stride, one misaligned pointer, BGR) is first copied, visible pixels
        only, into the context's own staging planes.  Returns the brightness means (float64 per frame) if want_hist, else None."""
        n = len(slots)
        ptrs = (C.c_void_p * n)(*dev_ptrs)
        hist = np.zeros(n, np.float64) if want_hist else None
        self._ck(self.lib.icg_frames_preprocess(self.h, n, _p(i32(slots)), ptrs, stride, channels, 1, _p(hist)),
                 "icg_frames_preprocess")
        return hist

    def download(self, slot, level=0):
        w, h = self.width, self.height
        for _ in range(level):
            w, h = (w + 1) // 2, (h + 1) // 2
        out = np.zeros((h, w), np.uint8)
        self._ck(self.lib.icg_frame_download(self.h, slot, level, _p(out), w), "icg_frame_download")
        return out

    # ---- F2/F3
    def lk_track(self, prev_slot, next_slot, prev_pts, guess, want_err=True):
        prev_pts = f32(prev_pts).reshape(-1, 2)
        n = prev_pts.shape[0]
        nxt = f32(guess).reshape(-1, 2).copy()
        st = np.zeros(n, np.uint8)
        err = np.zeros(n, np.float32) if want_err else None
        ps = i32(np.broadcast_to(prev_slot, (n,)))
        ns = i32(np.broadcast_to(next_slot, (n,)))
        self._ck(self.lib.icg_lk_track(self.h, n, _p(ps), _p(ns), _p(prev_pts), _p(nxt), _p(st), _p(err)), "icg_lk_track")
        return nxt, st, err

    def lk_track_fb(self, prev_slot, next_slot, prev_pts, guess, want_undist=False, want_keep=False):
        prev_pts = f32(prev_pts).reshape(-1, 2)
        guess = f32(guess).reshape(-1, 2)
        n = prev_pts.shape[0]
        out = np.zeros((n, 2), np.float32)
        st = np.zeros(n, np.uint8)
        und = np.zeros((n, 2), np.float32) if want_undist else None
        keep = np.zeros(max(n, 1), np.int32) if want_keep else None
        nkeep = np.zeros(1, np.int32) if want_keep else None
        ps = i32(np.broadcast_to(prev_slot, (n,)))
        ns = i32(np.broadcast_to(next_slot, (n,)))
        self._ck(self.lib.icg_lk_track_fb(self.h, n, _p(ps), _p(ns), _p(prev_pts), _p(guess), _p(out), _p(st), _p(und),
                                           _p(keep), _p(nkeep)), "icg_lk_track_fb")
        res = [out, st]
        if want_undist:
            res.append(und)
        if want_keep:
            res.append(keep[:int(nkeep[0])])
        return tuple(res)

    def lk_track_fb_cams(self, prev_slot, next_slot, prev_pts, guess, cam_idx, want_keep=False, check=True, fill=0):
        """icg_lk_track_fb_cams: (out, status, undist[, keep]).  check=False: (rc, out, status, undist, keep, n_keep) with every output
        buffer pre-filled with `fill` (argument-error tests; cam_idx may be None)"""
        prev_pts = f32(prev_pts).reshape(-1, 2)
        guess = f32(guess).reshape(-1, 2)
        n = prev_pts.shape[0]
        out = np.full((n, 2), fill, np.float32)
        st = np.full(n, fill, np.uint8)
        und = np.full((n, 2), fill, np.float32)
        keep = np.full(max(n, 1), fill, np.int32) if want_keep else None
        nkeep = np.full(1, fill, np.int32) if want_keep else None
        ps = i32(np.broadcast_to(prev_slot, (n,)))
        ns = i32(np.broadcast_to(next_slot, (n,)))
        ci = None if cam_idx is None else i32(cam_idx)
        rc = self.lib.icg_lk_track_fb_cams(self.h, n, _p(ps), _p(ns), _p(prev_pts), _p(guess), _p(ci), _p(out), _p(st), _p(und), _p(keep), _p(nkeep))
        if not check:
            return rc, out, st, und, keep, nkeep
        self._ck(rc, "icg_lk_track_fb_cams")
        return (out, st, und, keep[:int(nkeep[0])]) if want_keep else (out, st, und)

    # ---- F4/F5
    def undistort(self, pts):
        p = f32(pts).reshape(-1, 2).copy()
        self._ck(self.lib.icg_undistort_points(self.h, p.shape[0], _p(p)), "icg_undistort_points")
        return p

    def distort(self, pts):
        p = f32(pts).reshape(-1, 2).copy()
        self._ck(self.lib.icg_distort_points(self.h, p.shape[0], _p(p)), "icg_distort_points")
        return p

    def predict_mappoints(self, pw, pose_idx, poses12):
        pw = f64(pw).reshape(-1, 3)
        poses12 = f64(poses12).reshape(-1, 12)
        n = pw.shape[0]
        out = np.zeros((n, 2), np.float32)
        self._ck(self.lib.icg_predict_mappoints(self.h, n, _p(pw), _p(i32(np.broadcast_to(pose_idx, (n,)))),
                                                 poses12.shape[0], _p(poses12), _p(out)), "icg_predict_mappoints")
        return out

    def predict_rotation(self, pts, rot_idx, rots9):
        pts = f32(pts).reshape(-1, 2)
        rots9 = f64(rots9).reshape(-1, 9)
        n = pts.shape[0]
        out = np.zeros((n, 2), np.float32)
        self._ck(self.lib.icg_predict_rotation(self.h, n, _p(pts), _p(i32(np.broadcast_to(rot_idx, (n,)))),
                                                rots9.shape[0], _p(rots9), _p(out)), "icg_predict_rotation")
        return out

    # ---- F6
    def fm_ransac(self, offsets, pts1, pts2, thresh=1.5, conf=0.99):
        offsets = i32(offsets)
        pts1 = f32(pts1).reshape(-1, 2)
        pts2 = f32(pts2).reshape(-1, 2)
        mask = np.ones(pts1.shape[0], np.uint8)
        self._ck(self.lib.icg_fm_ransac(self.h, len(offsets) - 1, _p(offsets), _p(pts1), _p(pts2), C.c_double(thresh),
                                         C.c_double(conf), _p(mask)), "icg_fm_ransac")
        return mask

    def fm_ransac_device(self, offsets, pts1, pts2, thresh=1.5, conf=0.99):
        """icg_fm_ransac_device: the whole RANSAC run of every set in one launch (the kernel the device-resident tracker uses)"""
        offsets = i32(offsets)
        pts1 = f32(pts1).reshape(-1, 2)
        pts2 = f32(pts2).reshape(-1, 2)
        mask = np.ones(pts1.shape[0], np.uint8)
        self._ck(self.lib.icg_fm_ransac_device(self.h, len(offsets) - 1, _p(offsets), _p(pts1), _p(pts2), C.c_double(thresh),
                                                C.c_double(conf), _p(mask)), "icg_fm_ransac_device")
        return mask

    # ---- F7
    def detect(self, slots, grid, mask_off, mask_pts, quota, max_per_job):
        slots = i32(slots)
        n = len(slots)
        g = DetectGrid(*[int(v) for v in grid])
        mask_off = i32(mask_off)
        mask_pts = f32(mask_pts).reshape(-1, 2)
        quota = i32(quota)
        out = np.zeros((n, max_per_job, 2), np.float32)
        cnt = np.zeros(n, np.int32)
        blk = np.zeros((n, max_per_job), np.int32)
        self._ck(self.lib.icg_detect(self.h, n, _p(slots), C.byref(g), _p(mask_off), _p(mask_pts), _p(quota), max_per_job,
                                      _p(out), _p(cnt), _p(blk)), "icg_detect")
        return out, cnt, blk

    # ---- F8
    def triangulate(self, T0_idx, T1_idx, Tcw12, pc0, pc1):
        Tcw12 = f64(Tcw12).reshape(-1, 12)
        pc0 = f64(pc0).reshape(-1, 3)
        pc1 = f64(pc1).reshape(-1, 3)
        n = pc0.shape[0]
        pw = np.zeros((n, 3), np.float64)
        self._ck(self.lib.icg_triangulate(self.h, n, _p(i32(np.broadcast_to(T0_idx, (n,)))),
                                           _p(i32(np.broadcast_to(T1_idx, (n,)))), Tcw12.shape[0], _p(Tcw12), _p(pc0),
                                           _p(pc1), _p(pw)), "icg_triangulate")
        return pw

    # ---- R1/R2
    def reproj_eval(self, obs_soa, idx_i, idx_j, idx_lm, poses, ext, invdepth, td, want_jac=True, huber=0.0):
        obs_soa = f64(obs_soa)
        n = obs_soa.shape[1]
        poses = f64(poses).reshape(-1, 7)
        invdepth = f64(invdepth).reshape(-1)
        r = np.zeros((n, 2))
        J = np.zeros((n, 46)) if want_jac else None
        self._ck(self.lib.icg_reproj_eval_batch(self.h, n, _p(obs_soa), _p(i32(idx_i)), _p(i32(idx_j)), _p(i32(idx_lm)),
                                                 poses.shape[0], _p(poses), _p(f64(ext)), invdepth.shape[0], _p(invdepth),
                                                 C.c_double(td), 1 if want_jac else 0, C.c_double(huber), _p(r), _p(J)),
                 "icg_reproj_eval_batch")
        return r, J

    def reproj_set_factors(self, obs_soa, idx_i, idx_j, idx_lm):
        obs_soa = f64(obs_soa)
        n = obs_soa.shape[1]
        self._ck(self.lib.icg_reproj_set_factors(self.h, n, _p(obs_soa), _p(i32(idx_i)), _p(i32(idx_j)), _p(i32(idx_lm))),
                 "icg_reproj_set_factors")
        self._nfac = n

    def reproj_set_factors_staged(self, obs_soa, idx_i, idx_j, idx_lm):
        """the same upload through icg_reproj_stage_factors / icg_reproj_commit_factors: the factor set is written into the context's pinned
        staging block in place (what the host layer does from its pool threads)"""
        obs_soa = f64(obs_soa)
        n = obs_soa.shape[1]
        po, pi = C.c_void_p(), C.c_void_p()
        self._ck(self.lib.icg_reproj_stage_factors(self.h, n, C.byref(po), C.byref(pi)), "icg_reproj_stage_factors")
        if n:
            np.ctypeslib.as_array(C.cast(po, C.POINTER(C.c_double)), shape=(15, n))[:] = obs_soa
            idx = np.ctypeslib.as_array(C.cast(pi, C.POINTER(C.c_int32)), shape=(3, n))
            idx[0], idx[1], idx[2] = i32(idx_i), i32(idx_j), i32(idx_lm)
        self._ck(self.lib.icg_reproj_commit_factors(self.h), "icg_reproj_commit_factors")
        self._nfac = n

    def reproj_eval_resident(self, poses, ext, invdepth, td, want_jac=True, huber=0.0, fetch=True):
        poses = f64(poses).reshape(-1, 7)
        invdepth = f64(invdepth).reshape(-1)
        n = self._nfac
        r = np.zeros((n, 2)) if fetch else None
        J = np.zeros((n, 46)) if (fetch and want_jac) else None
        self._ck(self.lib.icg_reproj_eval_resident(self.h, poses.shape[0], _p(poses), _p(f64(ext)), invdepth.shape[0],
                                                    _p(invdepth), C.c_double(td), 1 if want_jac else 0, C.c_double(huber),
                                                    _p(r), _p(J)), "icg_reproj_eval_resident")
        return r, J

    def reproj_accumulate_normal(self, local_size, col_pose, col_ext, col_lm, col_td):
        H = np.zeros((local_size, local_size))
        b = np.zeros(local_size)
        self._ck(self.lib.icg_reproj_accumulate_normal(self.h, local_size, _p(i32(col_pose)), int(col_ext), _p(i32(col_lm)),
                                                        int(col_td), _p(H), _p(b)), "icg_reproj_accumulate_normal")
        return H, b

    # ---- f3
    def reproj_error_batch(self, pose_idx, lm_idx, poses12, pw, pix, max_error, min_depth=1.0, max_depth=200.0):
        poses12 = f64(poses12).reshape(-1, 12)
        pw = f64(pw).reshape(-1, 3)
        pix = f32(pix).reshape(-1, 2)
        n = pix.shape[0]
        err, good = np.zeros(n), np.zeros(n, np.uint8)
        self._ck(self.lib.icg_reproj_error_batch(self.h, n, _p(i32(pose_idx)), _p(i32(lm_idx)), poses12.shape[0], _p(poses12), pw.shape[0],
                                                  _p(pw), _p(pix), C.c_double(max_error), C.c_double(min_depth), C.c_double(max_depth), _p(err),
                                                  _p(good)), "icg_reproj_error_batch")
        return err, good

    def reproj_error_batch_cams(self, pose_idx, lm_idx, poses12, pose_cam, pw, pix, max_error, min_depth=1.0, max_depth=200.0, check=True, fill=0):
        """icg_reproj_error_batch_cams: (err, good); check=False: (rc, err, good) with the outputs pre-filled with `fill`"""
        poses12 = f64(poses12).reshape(-1, 12)
        pw = f64(pw).reshape(-1, 3)
        pix = f32(pix).reshape(-1, 2)
        n = pix.shape[0]
        err, good = np.full(n, float(fill)), np.full(n, fill, np.uint8)
        pc = None if pose_cam is None else i32(pose_cam)
        rc = self.lib.icg_reproj_error_batch_cams(self.h, n, _p(i32(pose_idx)), _p(i32(lm_idx)), poses12.shape[0], _p(poses12), _p(pc), pw.shape[0],
                                                  _p(pw), _p(pix), C.c_double(max_error), C.c_double(min_depth), C.c_double(max_depth), _p(err), _p(good))
        if not check:
            return rc, err, good
        self._ck(rc, "icg_reproj_error_batch_cams")
        return err, good

    # ---- f1
    def reproj_schur(self, P, col_pose, col_ext, col_td, active=None, reassemble=True, damp=0.0, min_diag=1e-6, max_diag=1e32):
        S, s, dg, cost = np.zeros((P, P)), np.zeros(P), np.zeros(P), np.zeros(1)
        act = None if active is None else u8(active)
        self._ck(self.lib.icg_reproj_schur(self.h, int(P), _p(i32(col_pose)), int(col_ext), int(col_td), _p(act), 1 if reassemble else 0,
                                            C.c_double(damp), C.c_double(min_diag), C.c_double(max_diag), _p(S), _p(s), _p(dg), _p(cost)),
                 "icg_reproj_schur")
        return S, s, dg, float(cost[0])

    def reproj_backsub(self, P, delta_c, n_lm):
        out, terms = np.zeros(n_lm), np.zeros(2)
        self._ck(self.lib.icg_reproj_backsub(self.h, int(P), _p(f64(delta_c)), _p(out), _p(terms)), "icg_reproj_backsub")
        return out, terms

    def reproj_cost(self, active=None):
        cost = np.zeros(1)
        act = None if active is None else u8(active)
        self._ck(self.lib.icg_reproj_cost(self.h, _p(act), _p(cost)), "icg_reproj_cost")
        return float(cost[0])

    def reproj_landmark_diag(self, n_lm):
        """icg_reproj_landmark_diag: h_ll of every landmark from the system the last icg_reproj_schur left resident"""
        h = np.zeros(n_lm)
        self._ck(self.lib.icg_reproj_landmark_diag(self.h, _p(h)), "icg_reproj_landmark_diag")
        return h

    def reproj_chi2_cull(self, chi2, active):
        """icg_reproj_chi2_cull: a copy of `active` with every factor whose r0^2 + r1^2 exceeds chi2 cleared"""
        act = np.array(active, dtype=np.uint8, order="C").reshape(-1)
        if act.shape[0] != self._nfac:
            raise IcgError(f"reproj_chi2_cull: the mask has {act.shape[0]} entries, the resident set {self._nfac} factors")
        self._ck(self.lib.icg_reproj_chi2_cull(self.h, C.c_double(chi2), _p(act)), "icg_reproj_chi2_cull")
        return act

    def reproj_fetch_residuals(self):
        """icg_reproj_fetch_residuals: the resident residuals of the last evaluation (n x 2)"""
        r = np.zeros((self._nfac, 2))
        self._ck(self.lib.icg_reproj_fetch_residuals(self.h, _p(r)), "icg_reproj_fetch_residuals")
        return r

    # ---- f1, many windows per launch
    def reproj_set_windows(self, fac_off, lm_off):
        fac_off, lm_off = i32(fac_off), i32(lm_off)
        self._nwin = len(fac_off) - 1
        self._ck(self.lib.icg_reproj_set_windows(self.h, self._nwin, _p(fac_off), _p(lm_off)), "icg_reproj_set_windows")

    def reproj_eval_windows(self, poses, ext, invdepth, td, want_jac=True, huber=0.0):
        poses, ext, invdepth, td = f64(poses).reshape(-1, 7), f64(ext).reshape(-1, 7), f64(invdepth).reshape(-1), f64(td).reshape(-1)
        self._ck(self.lib.icg_reproj_eval_windows(self.h, poses.shape[0], _p(poses), _p(ext), invdepth.shape[0], _p(invdepth), _p(td),
                                                   1 if want_jac else 0, C.c_double(huber)), "icg_reproj_eval_windows")

    def _window_flags(self, active, reassemble, damp):
        """the per-factor mask (None = NULL: every factor) and the per-window reassemble flags (None: all) and dampings (None: 0) of the
        reproj_schur_windows* entries as the arrays they take"""
        W = self._nwin
        return (None if active is None else u8(active), np.ones(W, np.uint8) if reassemble is None else u8(reassemble),
                np.zeros(W) if damp is None else f64(damp))

    def reproj_schur_windows(self, P, col_pose, col_ext, col_td, active=None, reassemble=None, damp=None, min_diag=1e-6, max_diag=1e32):
        W = self._nwin
        S, s, dg, cost = np.zeros((W, P, P)), np.zeros((W, P)), np.zeros((W, P)), np.zeros(W)
        act, re, dm = self._window_flags(active, reassemble, damp)
        self._ck(self.lib.icg_reproj_schur_windows(self.h, int(P), _p(i32(col_pose)), _p(i32(col_ext)), _p(i32(col_td)), _p(act), _p(re), _p(dm),
                                                    C.c_double(min_diag), C.c_double(max_diag), _p(S), _p(s), _p(dg), _p(cost)),
                 "icg_reproj_schur_windows")
        return S, s, dg, cost

    def reproj_reserve_windows(self, P):
        self._ck(self.lib.icg_reproj_reserve_windows(self.h, int(P)), "icg_reproj_reserve_windows")

    def reproj_schur_windows_view(self, P, col_pose, col_ext, col_td, active=None, reassemble=None, damp=None, min_diag=1e-6, max_diag=1e32):
        """icg_reproj_schur_windows_view: the reduced systems are read where the reduction kernel left them (a copy is returned; only the
        16 x 16 tiles on and below the diagonal are defined)"""
        W = self._nwin
        s, dg, cost = np.zeros((W, P)), np.zeros((W, P)), np.zeros(W)
        act, re, dm = self._window_flags(active, reassemble, damp)
        view = C.POINTER(C.c_double)()
        self._ck(self.lib.icg_reproj_schur_windows_view(self.h, int(P), _p(i32(col_pose)), _p(i32(col_ext)), _p(i32(col_td)), _p(act), _p(re), _p(dm),
                                                         C.c_double(min_diag), C.c_double(max_diag), C.byref(view), _p(s), _p(dg), _p(cost)),
                 "icg_reproj_schur_windows_view")
        S = np.ctypeslib.as_array(view, shape=(W, P, P)).copy()
        return S, s, dg, cost

    def reproj_schur_windows_resident(self, P, col_pose, col_ext, col_td, active=None, reassemble=None, damp=None, min_diag=1e-6, max_diag=1e32):
        """icg_reproj_schur_windows_resident: the reduced systems stay on the device for reproj_solve_windows -> (s, diag_cc, cost)"""
        W = self._nwin
        s, dg, cost = np.zeros((W, P)), np.zeros((W, P)), np.zeros(W)
        act, re, dm = self._window_flags(active, reassemble, damp)
        self._ck(self.lib.icg_reproj_schur_windows_resident(self.h, int(P), _p(i32(col_pose)), _p(i32(col_ext)), _p(i32(col_td)), _p(act), _p(re),
                                                             _p(dm), C.c_double(min_diag), C.c_double(max_diag), _p(s), _p(dg), _p(cost)),
                 "icg_reproj_schur_windows_resident")
        return s, dg, cost

    def reproj_solve_windows(self, P, Pw, solve, dd, rhs, n_lm, host_part_new=None, host_S=None):
        """icg_reproj_solve_windows: host_S = the packed lower triangles of the flagged windows, flat -> (delta_c W x P, status, delta_l, lm_terms)"""
        W = self._nwin
        Pw, sv = i32(Pw).reshape(W), u8(solve).reshape(W)
        new = None if host_part_new is None else u8(host_part_new).reshape(W)
        hs = None if host_S is None else f64(host_S).reshape(-1)
        dd, rhs = f64(dd).reshape(W, P), f64(rhs).reshape(W, P)
        dc, st, dl, terms = np.zeros((W, P)), np.zeros(W, np.int32), np.zeros(n_lm), np.zeros((W, 2))
        self._ck(self.lib.icg_reproj_solve_windows(self.h, int(P), _p(Pw), _p(sv), _p(new), _p(hs), _p(dd), _p(rhs), _p(dc), _p(st), _p(dl), _p(terms)),
                 "icg_reproj_solve_windows")
        return dc, st, dl, terms

    def reproj_host_parts_build_raw(self, P, Pw, rebuild, blk_off, nr, nf, cols, jac_off, J, r, host_s, host_diag, part_out=None):
        """icg_reproj_host_parts_build on the caller's arrays (None = NULL; host_s, host_diag, part_out are written in place) -> the return code"""
        return self.lib.icg_reproj_host_parts_build(self.h, int(P), _p(Pw), _p(rebuild), _p(blk_off), _p(nr), _p(nf), _p(cols), _p(jac_off), _p(J), _p(r),
                                                    _p(host_s), _p(host_diag), _p(part_out))

    def _pack_host_blocks(self, windows):
        """the flat block arrays of the host-parts entries from per-window lists of blocks: (J nr x nf, r, cols, keep) or
        ("prior", p, prior_cols, cols, how) as reproj_host_parts_build_prior describes them
        -> (blk_off, nr, nf, cols, jac_off, J | None, r, prior_of, prior_cols | None)"""
        blocks = [b for win in windows for b in win]
        blk_off = i32(np.concatenate([[0], np.cumsum([len(win) for win in windows])]))
        is_prior = [isinstance(b[0], str) for b in blocks]
        nr = i32([self._marg_r[b[1]] if pr else np.shape(b[0])[0] for b, pr in zip(blocks, is_prior)])
        nf = i32([len(b[3]) if pr else np.shape(b[0])[1] for b, pr in zip(blocks, is_prior)])
        cols = i32(np.concatenate([i32(b[3] if pr else b[2]).reshape(-1) for b, pr in zip(blocks, is_prior)])) if blocks else i32([])
        r = f64(np.concatenate([np.full(n, np.nan) if pr else f64(b[1]).reshape(-1) for b, pr, n in zip(blocks, is_prior, nr)])) if blocks else f64([])
        prior_of = i32([b[1] if pr else -1 for b, pr in zip(blocks, is_prior)])
        pcs = [i32(b[2]).reshape(-1) for b, pr in zip(blocks, is_prior) if pr]
        prior_cols = i32(np.concatenate(pcs)) if pcs else None
        jac_off, Js, at = np.full(len(blocks), -1, np.int64), [], 0
        for k, (b, pr) in enumerate(zip(blocks, is_prior)):
            if pr and isinstance(b[4], str):
                jac_off[k] = HP_JAC_FROM_PRIOR if b[4] == "gather" else -1
            elif pr or not b[3]:
                jac_off[k] = at
                Js.append(f64(b[4] if pr else b[0]).reshape(-1))
                at += Js[-1].size
        J = f64(np.concatenate(Js)) if Js else None
        return blk_off, nr, nf, cols, jac_off, J, r, prior_of, prior_cols

    def _host_parts_build(self, entry, what, P, Pw, windows, rebuild, host_s, host_diag, with_priors):
        """the list forms of reproj_host_parts_build / _prior: pack the blocks, call entry, cut the packed parts of the rebuilt windows apart"""
        W = self._nwin
        Pw = i32(Pw).reshape(W)
        rb = np.ones(W, np.uint8) if rebuild is None else u8(rebuild).reshape(W)
        *flat, prior_of, prior_cols = self._pack_host_blocks(windows)
        s = np.zeros((W, P)) if host_s is None else host_s
        dg = np.zeros((W, P)) if host_diag is None else host_diag
        sizes = [int(Pw[w]) * (int(Pw[w]) + 1) // 2 if rb[w] else 0 for w in range(W)]
        part = np.zeros(max(1, sum(sizes)))
        self._ck(entry(P, Pw, rb, *flat, s, dg, part, *((prior_of, prior_cols) if with_priors else ())), what)
        ends = np.cumsum(sizes)
        return s, dg, [part[e - n:e].copy() if rb[w] else None for w, (n, e) in enumerate(zip(sizes, ends))]

    def reproj_host_parts_build(self, P, Pw, windows, rebuild=None, host_s=None, host_diag=None):
        """icg_reproj_host_parts_build.  windows: per window a list of blocks (J nr x nf, r, cols, keep); keep: the block goes up as -1 (J gives
        its shape only).  -> (host_s W x P, host_diag W x P, the packed parts of the rebuilt windows as a list, None for the others)"""
        return self._host_parts_build(self.reproj_host_parts_build_raw, "icg_reproj_host_parts_build", P, Pw, windows, rebuild, host_s, host_diag, False)

    def reproj_host_parts_build_prior_raw(self, P, Pw, rebuild, blk_off, nr, nf, cols, jac_off, J, r, host_s, host_diag, part_out, prior_of, prior_cols):
        """icg_reproj_host_parts_build_prior on the caller's arrays (None = NULL; the outputs are written in place) -> the return code"""
        return self.lib.icg_reproj_host_parts_build_prior(self.h, int(P), _p(Pw), _p(rebuild), _p(blk_off), _p(nr), _p(nf), _p(cols), _p(jac_off), _p(J), _p(r),
                                                          _p(host_s), _p(host_diag), _p(part_out), _p(prior_of), _p(prior_cols))

    def reproj_host_parts_build_preint_raw(self, P, Pw, rebuild, blk_off, nr, nf, cols, jac_off, J, r, host_s, host_diag, part_out, prior_of, prior_cols,
                                           preint_of, preint_cols):
        """icg_reproj_host_parts_build_preint on the caller's arrays (None = NULL; the outputs are written in place) -> the return code"""
        return self.lib.icg_reproj_host_parts_build_preint(self.h, int(P), _p(Pw), _p(rebuild), _p(blk_off), _p(nr), _p(nf), _p(cols), _p(jac_off), _p(J), _p(r),
                                                           _p(host_s), _p(host_diag), _p(part_out), _p(prior_of), _p(prior_cols), _p(preint_of), _p(preint_cols))

    def reproj_host_parts_build_preint_odo_raw(self, P, Pw, rebuild, blk_off, nr, nf, cols, jac_off, J, r, host_s, host_diag, part_out, prior_of, prior_cols,
                                               preint_of, preint_cols, preint_odo_of, preint_odo_cols):
        """icg_reproj_host_parts_build_preint_odo on the caller's arrays (None = NULL; the outputs are written in place) -> the return code"""
        return self.lib.icg_reproj_host_parts_build_preint_odo(self.h, int(P), _p(Pw), _p(rebuild), _p(blk_off), _p(nr), _p(nf), _p(cols), _p(jac_off), _p(J),
                                                               _p(r), _p(host_s), _p(host_diag), _p(part_out), _p(prior_of), _p(prior_cols), _p(preint_of),
                                                               _p(preint_cols), _p(preint_odo_of), _p(preint_odo_cols))

    def reproj_host_parts_build_nav_raw(self, P, Pw, rebuild, blk_off, nr, nf, cols, jac_off, J, r, host_s, host_diag, part_out, prior_of=None, prior_cols=None,
                                        preint_of=None, preint_cols=None, preint_odo_of=None, preint_odo_cols=None, nav_of=None, nav_cols=None):
        """icg_reproj_host_parts_build_nav on the caller's arrays (None = NULL; the outputs are written in place) -> the return code"""
        return self.lib.icg_reproj_host_parts_build_nav(self.h, int(P), _p(Pw), _p(rebuild), _p(blk_off), _p(nr), _p(nf), _p(cols), _p(jac_off), _p(J), _p(r),
                                                        _p(host_s), _p(host_diag), _p(part_out), _p(prior_of), _p(prior_cols), _p(preint_of), _p(preint_cols),
                                                        _p(preint_odo_of), _p(preint_odo_cols), _p(nav_of), _p(nav_cols))

    def reproj_host_parts_build_prior(self, P, Pw, windows, rebuild=None, host_s=None, host_diag=None):
        """icg_reproj_host_parts_build_prior.  windows: per window a list of blocks; an ordinary block is (J nr x nf, r, cols, keep) as in
        reproj_host_parts_build, a prior block is ("prior", p, prior_cols, cols, how): prior p of the resident set (marg_prior_set), how =
        "gather" (ICG_HP_JAC_FROM_PRIOR), "keep" (-1) or the Jacobian to upload.  The prior blocks' slots in r are filled with NaN: they
        are not read.  -> (host_s, host_diag, parts) as reproj_host_parts_build"""
        return self._host_parts_build(self.reproj_host_parts_build_prior_raw, "icg_reproj_host_parts_build_prior", P, Pw, windows, rebuild, host_s, host_diag,
                                      True)

    def reproj_backsub_windows(self, P, delta_c, n_lm):
        out, terms = np.zeros(n_lm), np.zeros((self._nwin, 2))
        self._ck(self.lib.icg_reproj_backsub_windows(self.h, int(P), _p(f64(delta_c)), _p(out), _p(terms)), "icg_reproj_backsub_windows")
        return out, terms

    def reproj_landmark_diag_windows(self, n_lm):
        """icg_reproj_landmark_diag_windows: h_ll of every landmark of the partition, in its global landmark order"""
        h = np.zeros(n_lm)
        self._ck(self.lib.icg_reproj_landmark_diag_windows(self.h, _p(h)), "icg_reproj_landmark_diag_windows")
        return h

    def reproj_landmark_min_windows_raw(self, out):
        """icg_reproj_landmark_min_windows into the caller's array (one double per window) -> the return code"""
        return self.lib.icg_reproj_landmark_min_windows(self.h, _p(out))

    def reproj_landmark_min_windows(self):
        """icg_reproj_landmark_min_windows: the smallest h_ll of every window of the partition (0.0 for a window without landmarks)"""
        mn = np.zeros(self._nwin)
        self._ck(self.reproj_landmark_min_windows_raw(mn), "icg_reproj_landmark_min_windows")
        return mn

    def reproj_cost_windows(self, active=None):
        cost = np.zeros(self._nwin)
        act = None if active is None else u8(active)
        self._ck(self.lib.icg_reproj_cost_windows(self.h, _p(act), _p(cost)), "icg_reproj_cost_windows")
        return cost

    # ---- P1 and P2 of both preintegration families: one body each over the family's widths, (imu, state0, params, delta, N, point); the entry is
    # icg_<stem>_<call> and the resident count self._<stem>_n
    _PREINT = ("preint", (8, 16, 9, 16, 15, 32))
    _PREINT_ODO = ("preint_odo", (9, 17, 25, 20, 19, 34))

    def _preint_batch_call(self, fam, variant, offsets, imu, state0, params, want_pn):
        stem, (w_imu, w_s0, _, w_del, N, _) = fam
        offsets = i32(offsets)
        n = len(offsets) - 1
        imu = f64(imu).reshape(-1, w_imu)
        state0 = f64(state0).reshape(n, w_s0)
        cur, delta, jac, cov, dt = np.zeros((n, 16)), np.zeros((n, w_del)), np.zeros((n, N, N)), np.zeros((n, N, N)), np.zeros(n)
        pn = np.zeros((imu.shape[0], 4)) if want_pn else None
        self._ck(getattr(self.lib, f"icg_{stem}_batch")(self.h, int(variant), n, _p(offsets), _p(imu), _p(state0), _p(params), _p(cur), _p(delta), _p(jac),
                                                        _p(cov), _p(dt), _p(pn)), f"icg_{stem}_batch")
        return cur, delta, jac, cov, dt, pn

    def preint_batch(self, variant, offsets, imu, state0, params, want_pn=True):
        """icg_preint_batch -> (cur n x 16, delta n x 16, jac n x 15 x 15, cov n x 15 x 15, dt n, pn total x 4 or None without want_pn)"""
        return self._preint_batch_call(self._PREINT, variant, offsets, imu, state0, f64(params), want_pn)

    def preint_odo_batch(self, variant, offsets, imu9, state0, params25, want_pn=True):
        """icg_preint_odo_batch (variant 2 = Odo, 3 = EarthOdo) -> as preint_batch with delta n x 20 and 19 x 19 matrices"""
        return self._preint_batch_call(self._PREINT_ODO, variant, offsets, imu9, state0, f64(params25).reshape(25), want_pn)

    def _preint_params_call(self, fn, name, widths, variant, offsets, imu, state0, params, want_pn, want_sqrt_info, want_status, fill):
        """the shared body of preint_batch_params / preint_odo_batch_params; widths = (imu, state0, params, delta, N)"""
        w_imu, w_s0, w_par, w_del, N = widths
        offsets = i32(offsets)
        n = len(offsets) - 1
        imu = f64(imu).reshape(-1, w_imu)
        state0 = f64(state0).reshape(n, w_s0)
        params = f64(params).reshape(n, w_par)
        mk = lambda *shape: np.full(shape, fill, np.float64)
        cur, delta, jac, cov, dt = mk(n, 16), mk(n, w_del), mk(n, N, N), mk(n, N, N), mk(n)
        pn = mk(imu.shape[0], 4) if want_pn else None
        S = mk(n, N, N) if want_sqrt_info else None
        status = np.full(n, -1, np.int32) if want_status else None
        self._ck(fn(self.h, int(variant), n, _p(offsets), _p(imu), _p(state0), _p(params), _p(cur), _p(delta), _p(jac), _p(cov), _p(dt), _p(pn),
                    _p(S), _p(status)), name)
        return cur, delta, jac, cov, dt, pn, S, status

    def preint_batch_params(self, variant, offsets, imu, state0, params, want_pn=True, want_sqrt_info=True, want_status=True, fill=0.0):
        """icg_preint_batch_params (params n x 9, one row per interval) -> (cur n x 16, delta n x 16, jac, cov n x 15 x 15, dt n, pn total x 4
        or None, sqrt_info n x 15 x 15 or None, status n or None); the output arrays start out filled with `fill`"""
        return self._preint_params_call(self.lib.icg_preint_batch_params, "icg_preint_batch_params", self._PREINT[1][:5], variant, offsets, imu, state0,
                                        params, want_pn, want_sqrt_info, want_status, fill)

    def preint_odo_batch_params(self, variant, offsets, imu9, state0, params25, want_pn=True, want_sqrt_info=True, want_status=True, fill=0.0):
        """icg_preint_odo_batch_params (params25 n x 25) -> as preint_batch_params with delta n x 20 and 19 x 19 matrices"""
        return self._preint_params_call(self.lib.icg_preint_odo_batch_params, "icg_preint_odo_batch_params", self._PREINT_ODO[1][:5], variant, offsets, imu9,
                                        state0, params25, want_pn, want_sqrt_info, want_status, fill)

    # ---- P2
    def _preint_evaluate_batch_call(self, fam, variant, delta, jac, cov, dt, env, points, pn_offsets, pn, want_jac):
        stem, (_, _, _, w_del, N, point) = fam
        points = f64(points).reshape(-1, point)
        n = points.shape[0]
        delta, jac, cov = f64(delta).reshape(n, w_del), f64(jac).reshape(n, N * N), f64(cov).reshape(n, N * N)
        dt, env = f64(dt).reshape(n), f64(env).reshape(n, 4)
        po = None if pn_offsets is None else i32(pn_offsets)
        pnr = None if pn is None else f64(pn).reshape(-1, 4)
        res = np.zeros((n, N))
        J = np.zeros((n, N * point)) if want_jac else None
        S = np.zeros((n, N, N))
        status = np.zeros(n, np.int32)
        self._ck(getattr(self.lib, f"icg_{stem}_evaluate_batch")(self.h, int(variant), n, _p(delta), _p(jac), _p(cov), _p(dt), _p(env), _p(po), _p(pnr),
                                                                 _p(points), _p(res), _p(J), _p(S), _p(status)), f"icg_{stem}_evaluate_batch")
        return res, J, S, status

    def _preint_set_call(self, fam, variant, delta, jac, sqrt_info, dt, env, q_nn, pn_offsets, pn):
        stem, (_, _, _, w_del, N, _) = fam
        variant = i32(variant).reshape(-1)
        n = len(variant)
        delta, jac, sqrt_info = f64(delta).reshape(n, w_del), f64(jac).reshape(n, N * N), f64(sqrt_info).reshape(n, N * N)
        dt, env, q_nn = f64(dt).reshape(n), f64(env).reshape(n, 4), f64(q_nn).reshape(n, 4)
        po = None if pn_offsets is None else i32(pn_offsets)
        pnr = None if pn is None else f64(pn).reshape(-1, 4)
        setattr(self, f"_{stem}_n", 0)
        self._ck(getattr(self.lib, f"icg_{stem}_set")(self.h, n, _p(variant), _p(delta), _p(jac), _p(sqrt_info), _p(dt), _p(env), _p(q_nn), _p(po), _p(pnr)),
                 f"icg_{stem}_set")
        setattr(self, f"_{stem}_n", n)

    def _preint_evaluate_resident_call(self, fam, points, q_corr, want_jac):
        stem, widths = fam
        n = getattr(self, f"_{stem}_n", 0)
        points, q_corr = f64(points).reshape(-1, widths[5]), f64(q_corr).reshape(-1, 4)
        if n and (points.shape[0] != n or q_corr.shape[0] != n):
            raise IcgError(f"{stem}_evaluate_resident: {points.shape[0]} points and {q_corr.shape[0]} quaternions, the resident set has {n} factors")
        sq = np.zeros(max(n, 1))
        self._ck(getattr(self.lib, f"icg_{stem}_evaluate_resident")(self.h, _p(points), _p(q_corr), 1 if want_jac else 0, _p(sq)), f"icg_{stem}_evaluate_resident")
        return sq[:n]

    def _preint_fetch_resident_call(self, fam, want_jac):
        stem, (_, _, _, _, N, point) = fam
        n = max(getattr(self, f"_{stem}_n", 0), 1)
        res = np.zeros((n, N))
        J = np.zeros((n, N * point)) if want_jac else None
        self._ck(getattr(self.lib, f"icg_{stem}_fetch_resident")(self.h, _p(res), _p(J)), f"icg_{stem}_fetch_resident")
        return res, J

    def preint_evaluate_batch(self, variant, delta, jac, cov, dt, env, points, pn_offsets=None, pn=None, want_jac=True):
        """icg_preint_evaluate_batch -> (residuals n x 15, jacobians n x 480 or None, sqrt_info n x 15 x 15, status n)"""
        return self._preint_evaluate_batch_call(self._PREINT, variant, delta, jac, cov, dt, env, points, pn_offsets, pn, want_jac)

    def preint_odo_evaluate_batch(self, variant, delta, jac, cov, dt, env, points, pn_offsets=None, pn=None, want_jac=True):
        """icg_preint_odo_evaluate_batch -> (residuals n x 19, jacobians n x 646 or None, sqrt_info n x 19 x 19, status n)"""
        return self._preint_evaluate_batch_call(self._PREINT_ODO, variant, delta, jac, cov, dt, env, points, pn_offsets, pn, want_jac)

    def preint_set(self, variant, delta, jac, sqrt_info, dt, env, q_nn, pn_offsets=None, pn=None):
        """icg_preint_set: len(variant) factors become resident (variant per factor; sqrt_info and q_nn are the host's)"""
        self._preint_set_call(self._PREINT, variant, delta, jac, sqrt_info, dt, env, q_nn, pn_offsets, pn)

    def preint_odo_set(self, variant, delta, jac, sqrt_info, dt, env, q_nn, pn_offsets=None, pn=None):
        """icg_preint_odo_set: len(variant) odometer factors become resident (variant 2 / 3 per factor; sqrt_info and q_nn are the host's)"""
        self._preint_set_call(self._PREINT_ODO, variant, delta, jac, sqrt_info, dt, env, q_nn, pn_offsets, pn)

    def preint_evaluate_resident(self, points, q_corr, want_jac=True):
        """icg_preint_evaluate_resident: residuals (and Jacobians) stay on the device -> sq_norm (r . r per factor)"""
        return self._preint_evaluate_resident_call(self._PREINT, points, q_corr, want_jac)

    def preint_odo_evaluate_resident(self, points, q_corr, want_jac=True):
        """icg_preint_odo_evaluate_resident: residuals (and Jacobians) stay on the device -> sq_norm (r . r per factor)"""
        return self._preint_evaluate_resident_call(self._PREINT_ODO, points, q_corr, want_jac)

    def preint_fetch_resident(self, want_jac=True):
        """icg_preint_fetch_resident -> (residuals n x 15, jacobians n x 480 or None) of the last resident evaluation"""
        return self._preint_fetch_resident_call(self._PREINT, want_jac)

    def preint_odo_fetch_resident(self, want_jac=True):
        """icg_preint_odo_fetch_resident -> (residuals n x 19, jacobians n x 646 or None) of the last resident evaluation"""
        return self._preint_fetch_resident_call(self._PREINT_ODO, want_jac)

    # ---- navigation factors (host/nav_factors.h), resident
    def nav_set(self, kind, aux_off, aux):
        """icg_nav_set: len(kind) navigation factors become resident (kind 0..5; constants aux[aux_off[f]:aux_off[f + 1]])"""
        kind, aux_off, aux = i32(kind).reshape(-1), i32(aux_off).reshape(-1), f64(aux).reshape(-1)
        n = len(kind)
        if len(aux_off) != n + 1:
            raise IcgError(f"nav_set: {len(aux_off)} offsets for {n} members (n + 1 are needed)")
        if len(aux) == 0:
            aux = np.zeros(1)  # (a set of error factors reads no constant; the entry still wants a pointer)
        self._nav_kind = None
        self._ck(self.lib.icg_nav_set(self.h, n, _p(kind), _p(aux_off), _p(aux)), "icg_nav_set")
        self._nav_kind = kind.copy()

    def _nav_totals(self):
        kind = getattr(self, "_nav_kind", None)
        if kind is None:
            return 0, 1, 1
        return len(kind), sum(NAV_SHAPES[int(k)][0] for k in kind), sum(NAV_SHAPES[int(k)][0] * NAV_SHAPES[int(k)][1] for k in kind)

    def nav_evaluate_resident(self, points, point_off, want_jac=True):
        """icg_nav_evaluate_resident: member f is evaluated at points[point_off[f]:][:width]; residuals (and Jacobians) stay on the device
        -> sq_norm (r . r per member)"""
        points, point_off = f64(points).reshape(-1), i32(point_off).reshape(-1)
        n = self._nav_totals()[0]
        if n:
            if len(point_off) != n:
                raise IcgError(f"nav_evaluate_resident: {len(point_off)} offsets, the resident set has {n} members")
            for f in range(n):
                if point_off[f] >= 0 and point_off[f] + NAV_SHAPES[int(self._nav_kind[f])][1] > len(points):
                    raise IcgError(f"nav_evaluate_resident: member {f} reads past the {len(points)} values of points")
        sq = np.zeros(max(n, 1))
        self._ck(self.lib.icg_nav_evaluate_resident(self.h, _p(points), _p(point_off), 1 if want_jac else 0, _p(sq)), "icg_nav_evaluate_resident")
        return sq[:n]

    def nav_correct_resident(self, robust, corr):
        """icg_nav_correct_resident: the corrector of the members with robust[f] != 0; corr n x 3 = sqrt_rho1, alpha_sq_norm, residual_scaling"""
        n = self._nav_totals()[0]
        robust, corr = np.ascontiguousarray(robust, np.uint8).reshape(-1), f64(corr).reshape(-1, 3)
        if n and (len(robust) != n or corr.shape[0] != n):
            raise IcgError(f"nav_correct_resident: {len(robust)} marks and {corr.shape[0]} scalar triples, the resident set has {n} members")
        self._ck(self.lib.icg_nav_correct_resident(self.h, _p(robust), _p(corr)), "icg_nav_correct_resident")

    def nav_fetch_resident(self, want_jac=True):
        """icg_nav_fetch_resident -> (residuals, jacobians or None) of the last resident evaluation, flat, member after member"""
        _, nr, nj = self._nav_totals()
        res = np.zeros(nr)
        J = np.zeros(nj) if want_jac else None
        self._ck(self.lib.icg_nav_fetch_resident(self.h, _p(res), _p(J)), "icg_nav_fetch_resident")
        return res, J

    # ---- M4
    def marg_prior_set(self, r, block_off, block_size, block_index, x0, J0, e0):
        """icg_marg_prior_set: the priors of len(r) windows become resident (x0 / J0 / e0: flat arrays, window after window)"""
        r, block_off, block_size, block_index = i32(r).reshape(-1), i32(block_off).reshape(-1), i32(block_size).reshape(-1), i32(block_index).reshape(-1)
        x0, J0, e0 = f64(x0).reshape(-1), f64(J0).reshape(-1), f64(e0).reshape(-1)
        self._marg = None
        self._ck(self.lib.icg_marg_prior_set(self.h, len(r), _p(r), _p(block_off), _p(block_size), _p(block_index), _p(x0), _p(J0), _p(e0)),
                 "icg_marg_prior_set")
        xs = np.array([int(block_size[block_off[w]:block_off[w + 1]].sum()) for w in range(len(r))], np.int64)
        self._marg = (len(r), int(r.sum()), int(xs.sum()), int((r.astype(np.int64) * xs).sum()))
        self._marg_r = r.copy()

    def marg_prior_evaluate(self, x, want_jac=False, want_grad=False, want_sq_norm=False):
        """icg_marg_prior_evaluate -> (residuals, jacobians | None, gradient | None, sq_norm | None), flat, window after window"""
        n, nr, nx, njac = getattr(self, "_marg", None) or (0, 0, 0, 0)
        x = f64(x).reshape(-1)
        if n and x.shape[0] != nx:
            raise IcgError(f"marg_prior_evaluate: x has {x.shape[0]} values, the resident set takes {nx}")
        res = np.zeros(nr)
        jac = np.zeros(njac) if want_jac else None
        grad = np.zeros(nr) if want_grad else None
        sq = np.zeros(n) if want_sq_norm else None
        self._ck(self.lib.icg_marg_prior_evaluate(self.h, _p(x), _p(res), _p(jac), _p(grad), _p(sq)), "icg_marg_prior_evaluate")
        return res, jac, grad, sq

    def marg_prior_evaluate_resident(self, x):
        """icg_marg_prior_evaluate_resident: the residuals stay on the device for reproj_host_parts_build_prior -> sq_norm (e . e per window)"""
        n, nr, nx, njac = getattr(self, "_marg", None) or (0, 0, 0, 0)
        x = f64(x).reshape(-1)
        if n and x.shape[0] != nx:
            raise IcgError(f"marg_prior_evaluate_resident: x has {x.shape[0]} values, the resident set takes {nx}")
        sq = np.zeros(max(n, 1))
        self._ck(self.lib.icg_marg_prior_evaluate_resident(self.h, _p(x), _p(sq)), "icg_marg_prior_evaluate_resident")
        return sq[:n]

    # ---- M3
    def marg_linearize_batch(self, P, m, H, b, eps=1e-8, want_Hp=True, want_bp=True, want_evals=True, want_min_ev=True, want_status=True):
        """icg_marg_linearize_batch: H / b flat, window after window -> dict(J0, e0, Hp, bp, evals, min_ev_m, status), flat (None where
        not asked for)"""
        P, m = i32(P).reshape(-1), i32(m).reshape(-1)
        H, b = f64(H).reshape(-1), f64(b).reshape(-1)
        n = len(P)
        if len(m) != n or H.shape[0] != int((P.astype(np.int64) ** 2).sum()) or b.shape[0] != int(P.sum()):
            raise IcgError("marg_linearize_batch: P, m, H, b do not describe the same windows")
        r = P.astype(np.int64) - m
        nr, nrr = int(r.clip(0).sum()), int((r.clip(0) ** 2).sum())
        out = dict(J0=np.zeros(nrr), e0=np.zeros(nr), Hp=np.zeros(nrr) if want_Hp else None, bp=np.zeros(nr) if want_bp else None,
                   evals=np.zeros(nr) if want_evals else None, min_ev_m=np.zeros(n) if want_min_ev else None,
                   status=np.zeros(n, np.int32) if want_status else None)
        self._ck(self.lib.icg_marg_linearize_batch(self.h, n, _p(P), _p(m), _p(H), _p(b), C.c_double(eps), _p(out["Hp"]), _p(out["bp"]),
                                                   _p(out["J0"]), _p(out["e0"]), _p(out["evals"]), _p(out["min_ev_m"]), _p(out["status"])),
                 "icg_marg_linearize_batch")
        return out

    def marg_linearize_batch_keep(self, P, m, H, b, eps=1e-8, want_J0=True, want_e0=True, want_Hp=True, want_bp=True, want_evals=True,
                                  want_min_ev=True, want_status=True):
        """icg_marg_linearize_batch_keep: marg_linearize_batch with J0 / e0 also left on the device -> (dict as there, keep id); J0 / e0
        are None when not asked for (not transferred)"""
        P, m = i32(P).reshape(-1), i32(m).reshape(-1)
        H, b = f64(H).reshape(-1), f64(b).reshape(-1)
        n = len(P)
        if len(m) != n or H.shape[0] != int((P.astype(np.int64) ** 2).sum()) or b.shape[0] != int(P.sum()):
            raise IcgError("marg_linearize_batch_keep: P, m, H, b do not describe the same windows")
        r = P.astype(np.int64) - m
        nr, nrr = int(r.clip(0).sum()), int((r.clip(0) ** 2).sum())
        out = dict(J0=np.zeros(nrr) if want_J0 else None, e0=np.zeros(nr) if want_e0 else None, Hp=np.zeros(nrr) if want_Hp else None,
                   bp=np.zeros(nr) if want_bp else None, evals=np.zeros(nr) if want_evals else None,
                   min_ev_m=np.zeros(n) if want_min_ev else None, status=np.zeros(n, np.int32) if want_status else None)
        keep = C.c_uint64(0)
        self._ck(self.lib.icg_marg_linearize_batch_keep(self.h, n, _p(P), _p(m), _p(H), _p(b), C.c_double(eps), _p(out["Hp"]), _p(out["bp"]),
                                                        _p(out["J0"]), _p(out["e0"]), _p(out["evals"]), _p(out["min_ev_m"]), _p(out["status"]),
                                                        C.byref(keep)), "icg_marg_linearize_batch_keep")
        return out, int(keep.value)

    def marg_linearize_resident(self, P, win, Pw, m, b, eps=1e-8, keep=False, want_J0=True, want_e0=True, want_Hp=True, want_bp=True, want_evals=True,
                                want_min_ev=True, want_status=True, want_H=True):
        """icg_marg_linearize_resident: system k is window win[k] of the resident reduced systems (reproj_schur_windows_resident, common width
        P) plus its resident host part; b flat -> dict(J0, e0, Hp, bp, evals, min_ev_m, status, H), flat in list order; keep: -> (dict, keep id)"""
        win, Pw, m = i32(win).reshape(-1), i32(Pw).reshape(-1), i32(m).reshape(-1)
        b = f64(b).reshape(-1)
        n = len(win)
        if len(Pw) != n or len(m) != n or b.shape[0] != int(Pw.sum()):
            raise IcgError("marg_linearize_resident: win, Pw, m, b do not describe the same systems")
        r = Pw.astype(np.int64) - m
        nr, nrr = int(r.clip(0).sum()), int((r.clip(0) ** 2).sum())
        out = dict(J0=np.zeros(nrr) if want_J0 or not keep else None, e0=np.zeros(nr) if want_e0 or not keep else None,
                   Hp=np.zeros(nrr) if want_Hp else None, bp=np.zeros(nr) if want_bp else None, evals=np.zeros(nr) if want_evals else None,
                   min_ev_m=np.zeros(n) if want_min_ev else None, status=np.zeros(n, np.int32) if want_status else None,
                   H=np.zeros(int((Pw.astype(np.int64) ** 2).sum())) if want_H else None)
        kid = C.c_uint64(0)
        self._ck(self.lib.icg_marg_linearize_resident(self.h, int(P), n, _p(win), _p(Pw), _p(m), _p(b), C.c_double(eps), _p(out["Hp"]), _p(out["bp"]),
                                                      _p(out["J0"]), _p(out["e0"]), _p(out["evals"]), _p(out["min_ev_m"]), _p(out["status"]),
                                                      _p(out["H"]), C.byref(kid) if keep else None), "icg_marg_linearize_resident")
        return (out, int(kid.value)) if keep else out

    def marg_linearized_release(self):
        """icg_marg_linearized_release: the linearization this context keeps is dropped"""
        self._ck(self.lib.icg_marg_linearized_release(self.h), "icg_marg_linearized_release")

    def marg_prior_set_from_kept(self, keep_id, src, r, block_off, block_size, block_index, x0, J0_host=None, e0_host=None):
        """icg_marg_prior_set_from_kept: marg_prior_set with window w's J0 / e0 taken from window src[w] of the kept linearization
        keep_id (any context of this device), or, for src[w] == -1, from J0_host / e0_host (those windows only, in set order)"""
        src, r = i32(src).reshape(-1), i32(r).reshape(-1)
        block_off, block_size, block_index = i32(block_off).reshape(-1), i32(block_size).reshape(-1), i32(block_index).reshape(-1)
        x0 = f64(x0).reshape(-1)
        J0_host = None if J0_host is None else f64(J0_host).reshape(-1)
        e0_host = None if e0_host is None else f64(e0_host).reshape(-1)
        self._marg = None
        self._ck(self.lib.icg_marg_prior_set_from_kept(self.h, C.c_uint64(keep_id), len(r), _p(src), _p(r), _p(block_off), _p(block_size),
                                                       _p(block_index), _p(x0), _p(J0_host), _p(e0_host)), "icg_marg_prior_set_from_kept")
        xs = np.array([int(block_size[block_off[w]:block_off[w + 1]].sum()) for w in range(len(r))], np.int64)
        self._marg = (len(r), int(r.sum()), int(xs.sum()), int((r.astype(np.int64) * xs).sum()))
        self._marg_r = r.copy()

    # ---- the reduced camera solve
    def chol_solve_batch(self, n, A, b, want_L=True, want_status=True):
        """icg_chol_solve_batch: A (n[k] x n[k] row-major, lower triangle read) and b flat, system after system -> (x, L | None, status | None),
        flat; L is zero above the diagonals"""
        n = i32(n).reshape(-1)
        A, b = f64(A).reshape(-1), f64(b).reshape(-1)
        if A.shape[0] != int((n.astype(np.int64).clip(0) ** 2).sum()) or b.shape[0] != int(n.clip(0).sum()):
            raise IcgError("chol_solve_batch: n, A, b do not describe the same systems")
        x = np.zeros(b.shape[0])
        L = np.zeros(A.shape[0]) if want_L else None
        status = np.zeros(len(n), np.int32) if want_status else None
        self._ck(self.lib.icg_chol_solve_batch(self.h, len(n), _p(n), _p(A), _p(b), _p(x), _p(L), _p(status)), "icg_chol_solve_batch")
        return x, L, status

    # ---- f4
    def ins_mechanize_batch(self, offsets, imu, cfg8, states23, want_traj=True):
        offsets = i32(offsets)
        n = len(offsets) - 1
        imu = f64(imu).reshape(-1, 8)
        st = f64(states23).reshape(n, 23).copy()
        traj = np.zeros((imu.shape[0], 23)) if want_traj else None
        self._ck(self.lib.icg_ins_mechanize_batch(self.h, n, _p(offsets), _p(imu), _p(f64(cfg8)), _p(st), _p(traj)),
                 "icg_ins_mechanize_batch")
        return st, traj

    def ins_camera_pose_batch(self, brackets16, interp, pose_b_c12, times):
        b = f64(brackets16).reshape(-1, 16)
        n = b.shape[0]
        out = np.zeros((n, 12))
        self._ck(self.lib.icg_ins_camera_pose_batch(self.h, n, _p(b), _p(i32(interp)), _p(f64(pose_b_c12)), _p(f64(times)), _p(out)),
                 "icg_ins_camera_pose_batch")
        return out
