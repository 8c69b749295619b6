"""ctypes drivers of the device-prior marginalization tests (host/capi_marg_prior.cc: icgh_backend_marg_prior_resident,
icgh_backend_marg_prior_gather, icgh_backend_marg_prior_switch_alone) on the visual problem and second factor table of marg_resident_data."""
import ctypes as C

import numpy as np

import marg_resident_data as mr
from backend_utils import marg_problem_args
from ctypes_util import ErrBuf, ptr

CHAIN_A, CHAIN_B = 0, 1
# a mixed batch (capi_marg_prior.cc): the windows that are not ordinary second-generation windows
NO_PRIOR, DENSE, ROBUST, WEAK = 1, 2, 3, 4


def backend_marg_prior_resident(lib, mode, chain, n_windows, P, mixed=False, jitter=1e-3, huber=1.0, prior_weight=100.0, host_threads=4, seed=5, perturb=1e-3,
                                passes=1, profile=False):
    """icgh_backend_marg_prior_resident -> (rc, message, dict): the outputs of mr.backend_marg_resident and the counts device_priors,
    from_kept, deferred; kernel_ms (profile): marg_eval, host_part_prior, host_part, lm_min; wall_ms per pass"""
    vargs, K, L = marg_problem_args(P, huber, prior_weight)
    second, keep2 = mr.second_table(P)
    cap = 6 * K + 7
    ok, r_out, tag = np.zeros(n_windows, np.uint8), np.zeros(n_windows, np.int32), np.zeros(n_windows, np.int32)
    Hp, bp, J0, e0 = np.zeros(n_windows * cap * cap), np.zeros(n_windows * cap), np.zeros(n_windows * cap * cap), np.zeros(n_windows * cap)
    res, counts, phase = np.zeros(n_windows * cap), np.zeros(7, np.int32), np.zeros(4)
    kernel_ms, wall_ms = (np.zeros(4) if profile else None), np.zeros(passes)
    err = ErrBuf()
    rc = lib.icgh_backend_marg_prior_resident(int(mode), int(chain), int(n_windows), int(bool(mixed)), C.c_double(jitter), *vargs, *second, int(host_threads),
                                              C.c_uint64(seed), C.c_double(perturb), int(passes), ptr(ok), ptr(r_out), ptr(tag), ptr(Hp), ptr(bp), ptr(J0), ptr(e0),
                                              ptr(res), ptr(counts), ptr(phase), ptr(kernel_ms), ptr(wall_ms), *err.args)
    del keep2
    R, RR = int(r_out.sum()), int((r_out.astype(np.int64) ** 2).sum())
    out = dict(ok=ok, r=r_out, tag_slot=tag, Hp=Hp[:RR], bp=bp[:R], J0=J0[:RR], e0=e0[:R], residuals=res[:R], structured=int(counts[0]), dense=int(counts[1]),
               tagged=int(counts[2]), handed_off=int(counts[3]), device_priors=int(counts[4]), from_kept=int(counts[5]), deferred=int(counts[6]),
               phase_ms=phase, kernel_ms=kernel_ms, wall_ms=wall_ms)
    return rc, err.text(), out


def switch_alone(lib, P, huber=1.0, prior_weight=100.0):
    """icgh_backend_marg_prior_switch_alone -> (rc, message, kernel launches the batch's profiler counted)"""
    vargs, _, _ = marg_problem_args(P, huber, prior_weight)
    launches = np.full(1, -1, np.int32)
    err = ErrBuf()
    rc = lib.icgh_backend_marg_prior_switch_alone(*vargs, ptr(launches), *err.args)
    return rc, err.text(), int(launches[0])


def _blocks(nb, nr, nf, jac_off, cols, J, r):
    """per block: dict(nr, nf, jac_off, cols, r, c_at, r_at, J or None for a block without a Jacobian offset)"""
    out, c_at, r_at = [], 0, 0
    for k in range(nb):
        a, f, off = int(nr[k]), int(nf[k]), int(jac_off[k])
        out.append(dict(nr=a, nf=f, jac_off=off, cols=cols[c_at:c_at + f].copy(), r=r[r_at:r_at + a].copy(), c_at=c_at, r_at=r_at,
                        J=J[off:off + a * f].reshape(a, f).copy() if off >= 0 else None))
        c_at, r_at = c_at + f, r_at + a
    return out


def gather(lib, which, P, jitter=1e-3, huber=1.0, prior_weight=100.0):
    """icgh_backend_marg_prior_gather -> (rc, message, dict(deferred, eager: block lists; prior_block, prior_cols, J0 (r x r), prior_res,
    def_eval, eag_eval))"""
    vargs, K, L = marg_problem_args(P, huber, prior_weight)
    second, keep2 = mr.second_table(P)
    caps = np.array([64, 4096, 1 << 20, 1 << 14], np.int64)
    sizes = np.zeros(8, np.int64)

    def block_arrays():
        return (np.zeros(caps[0], np.int32), np.zeros(caps[0], np.int32), np.zeros(caps[0], np.int64), np.zeros(caps[1], np.int32), np.zeros(caps[2]),
                np.zeros(caps[3]))
    D, E = block_arrays(), block_arrays()
    prior_cols, J0, prior_res, def_eval, eag_eval = np.zeros(caps[1], np.int32), np.zeros(caps[2]), np.zeros(caps[3]), np.zeros(caps[2]), np.zeros(caps[2])
    err = ErrBuf()
    rc = lib.icgh_backend_marg_prior_gather(int(which), C.c_double(jitter), *vargs, *second, ptr(caps), ptr(sizes), *[ptr(a) for a in D], *[ptr(a) for a in E],
                                            ptr(prior_cols), ptr(J0), ptr(prior_res), ptr(def_eval), ptr(eag_eval), *err.args)
    del keep2
    if rc != 0:
        return rc, err.text(), None
    nb, pb, r, ne = int(sizes[0]), int(sizes[5]), int(sizes[6]), int(sizes[7])
    deferred, eager = _blocks(nb, *D), _blocks(nb, *E)
    n_pc = deferred[pb]["nf"] if pb >= 0 else 0
    return rc, "", dict(deferred=deferred, eager=eager, prior_block=pb, prior_cols=prior_cols[:n_pc].copy(), r=r, J0=J0[:r * r].reshape(r, r).copy(),
                        prior_res=prior_res[:r].copy(), def_eval=def_eval[:ne].copy(), eag_eval=eag_eval[:ne].copy(), sizes=sizes)
