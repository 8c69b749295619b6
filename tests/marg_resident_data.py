"""Inputs and ctypes drivers of the device-resident reduced system tests (host/capi_marg_resident.cc: icgh_backend_marg_resident,
icgh_backend_marg_plan_blocks): the visual problem, its second factor table (the factors anchored in keyframe 1, for the second
generation) and visual-inertial windows of 2 to 4 states."""
import ctypes as C

import numpy as np

import marg_data as md
import vio_data as vd
from backend_utils import marg_problem_args
from ctypes_util import bits, ErrBuf, ptr

VISUAL = dict(n_lm=40, n_kf=4, seed=7)


def visual_problem():
    return md.make_problem(**VISUAL)


def second_table(P):
    """the factors of problem P's window that are anchored in keyframe 1: (n2, obs2, ii2, jj2, ll2) and the arrays behind the pointers"""
    w = P["w"]
    keep = w["idx_i"] == 1
    obs = np.ascontiguousarray(w["obs_soa"][:, keep])
    ii, jj, ll = (np.ascontiguousarray(w[k][keep], np.int32) for k in ("idx_i", "idx_j", "idx_lm"))
    assert obs.shape[1] > 0
    return [obs.shape[1], ptr(obs), ptr(ii), ptr(jj), ptr(ll)], [obs, ii, jj, ll]


def _first_states(w, K):
    """the first K states of a visual-inertial window with the factors among them (make_vio_window keeps a landmark only when two other
    states see it, so a window of two states is cut from a longer one)"""
    keep = (w["ii"] < K) & (w["jj"] < K)
    lms, ll = np.unique(w["ll"][keep], return_inverse=True)
    offsets = np.ascontiguousarray(w["offsets"][:K])
    return dict(offsets=offsets, imu=np.ascontiguousarray(w["imu"][:offsets[K - 1]]), states=np.ascontiguousarray(w["states"][:K]), ext=w["ext"], td=w["td"],
                invdepth=np.ascontiguousarray(w["invdepth"][lms]), obs=np.ascontiguousarray(w["obs"][:, keep]), ii=np.ascontiguousarray(w["ii"][keep]),
                jj=np.ascontiguousarray(w["jj"][keep]), ll=ll.astype(np.int32))


def vio_windows(oracle):
    """visual-inertial windows of 2, 4, 3 and 2 states: different widths (37, 67, 52, 37 columns) in one batch"""
    wins = [vd.make_vio_window(oracle, n_intervals=k, per=20, n_lm=30, seed=30 + i) for i, k in enumerate((2, 3, 2, 3))]
    wins[0], wins[3] = _first_states(wins[0], 2), _first_states(wins[3], 2)
    assert [len(w["states"]) for w in wins] == [2, 4, 3, 2]
    for w in wins:
        assert (w["ii"] == 0).sum() >= 4  # enough factors anchored in state 0
    return wins


def _vio_group(wins):
    """the arguments n_intervals .. prior_mix0 (16 pointers) from vio_data.batch_leading_args, or 16 NULLs"""
    if wins is None:
        return [None] * 16, None
    args, st, inv, keep = vd.batch_leading_args(wins, [(w["states"], w["invdepth"]) for w in wins], 0, 100.0, 1.0)
    return args[1:17], (args, st, inv, keep)


def _visual_group(P, huber, prior_weight):
    if P is None:
        return [0, None, None, None, None, 0, None, None, 0, None, C.c_double(0.0), C.c_double(huber), C.c_double(prior_weight)], 0, 0
    return marg_problem_args(P, huber, prior_weight)


def backend_marg_resident(lib, mode, family, n_windows, P=None, vio=None, dense_window=-1, jitter=1e-3, huber=1.0, prior_weight=100.0, host_threads=4,
                          seed=5, perturb=1e-3, passes=1, profile=False):
    """icgh_backend_marg_resident -> (rc, message, dict).  family 0 / 2: n_windows jittered copies of problem P; family 1: the windows `vio`.
    passes: marginalizations on the same batch object (pass_ms: passes x 5); profile: kernel_ms of marg_form_h and host_part in the last pass."""
    vargs, K, L = _visual_group(P, huber, prior_weight)
    second, keep2 = second_table(P) if family == 2 else ([0, None, None, None, None], None)
    vio_args, keep_v = _vio_group(vio if family == 1 else None)
    if family == 1:
        cap = max(15 * len(w["states"]) + 7 for w in vio)
    else:
        cap = 6 * K + 7  # (every inverse depth is marginalized)
    ok, r_out, tag = np.zeros(n_windows, np.uint8), np.zeros(n_windows, np.int32), np.zeros(n_windows, np.int32)
    Hp, bp, J0, e0 = np.zeros(n_windows * cap * cap), np.zeros(n_windows * cap), np.zeros(n_windows * cap * cap), np.zeros(n_windows * cap)
    res, counts, phase = np.zeros(n_windows * cap), np.zeros(4, np.int32), np.zeros(4)
    pass_ms, kernel_ms = np.zeros((passes, 5)), np.zeros(2) if profile else None
    err = ErrBuf()
    rc = lib.icgh_backend_marg_resident(int(mode), int(family), int(n_windows), int(dense_window), C.c_double(jitter), *vargs, *second, *vio_args,
                                        int(host_threads), C.c_uint64(seed), C.c_double(perturb), ptr(ok), ptr(r_out), ptr(tag), ptr(Hp), ptr(bp), ptr(J0), ptr(e0),
                                        ptr(res), ptr(counts), ptr(phase), int(passes), ptr(pass_ms), ptr(kernel_ms), *err.args)
    del keep2, keep_v
    R, RR = int(r_out.sum()), int((r_out.astype(np.int64) ** 2).sum())
    out = dict(ok=ok, r=r_out, tag_slot=tag, Hp=Hp[:RR], bp=bp[:R], J0=J0[:RR], e0=e0[:R], residuals=res[:R], structured=int(counts[0]),
               dense=int(counts[1]), tagged=int(counts[2]), handed_off=int(counts[3]), phase_ms=phase, pass_ms=pass_ms, kernel_ms=kernel_ms)
    return rc, err.text(), out


def plan_blocks(lib, family, which, P=None, vio=None, huber=1.0, prior_weight=100.0):
    """icgh_backend_marg_plan_blocks -> (rc, message, dict(P, m, H, b, window)); window is dict(Pw, blocks) as host_part_data takes it"""
    vargs, K, L = _visual_group(P, huber, prior_weight)
    vio_args, keep_v = _vio_group(vio)
    caps = np.array([512 * 512, 64, 4096, 1 << 20, 1 << 14], np.int64)
    sizes = np.zeros(6, np.int64)
    H, b = np.zeros(caps[0]), np.zeros(512)
    nr, nf, jac_off = np.zeros(caps[1], np.int32), np.zeros(caps[1], np.int32), np.zeros(caps[1], np.int64)
    cols, J, r = np.zeros(caps[2], np.int32), np.zeros(caps[3]), np.zeros(caps[4])
    err = ErrBuf()
    rc = lib.icgh_backend_marg_plan_blocks(int(family), int(which), *vargs, *vio_args, ptr(caps), ptr(sizes), ptr(H), ptr(b), ptr(nr), ptr(nf), ptr(jac_off), ptr(cols),
                                           ptr(J), ptr(r), *err.args)
    del keep_v
    if rc != 0:
        return rc, err.text(), None
    Pw, m, nb = int(sizes[0]), int(sizes[1]), int(sizes[2])
    blocks, c_at, r_at = [], 0, 0
    for k in range(nb):
        a, f = int(nr[k]), int(nf[k])
        blocks.append((J[jac_off[k]:jac_off[k] + a * f].reshape(a, f).copy(), r[r_at:r_at + a].copy(), cols[c_at:c_at + f].copy()))
        c_at, r_at = c_at + f, r_at + a
    assert (c_at, r_at) == (int(sizes[3]), int(sizes[5]))
    return rc, "", dict(P=Pw, m=m, H=H[:Pw * Pw].reshape(Pw, Pw).copy(), b=b[:Pw].copy(), window=dict(Pw=Pw, blocks=blocks))


def split(out):
    """per good window: the bit patterns of Hp, bp, J0, e0 and the prior's residuals"""
    res, at, at2 = [], 0, 0
    for w, r in enumerate(out["r"]):
        r = int(r)
        if not out["ok"][w]:
            res.append(None)
            continue
        res.append(dict(Hp=bits(out["Hp"][at2:at2 + r * r]), J0=bits(out["J0"][at2:at2 + r * r]), bp=bits(out["bp"][at:at + r]), e0=bits(out["e0"][at:at + r]),
                        residuals=bits(out["residuals"][at:at + r])))
        at, at2 = at + r, at2 + r * r
    return res
