"""Helpers of the reduced-camera-solve tests: the host reference of icg_chol_solve_batch (icgh_dense_cholesky_solve), seeded systems, and
icgh_backend_solve_batch_mode on a list of solve_utils problems."""
import ctypes as C

import numpy as np

from ctypes_util import bits, ErrBuf, ptr



def spd(n, seed):
    """A = M M^T + n I and a right-hand side, from a seeded generator"""
    rng = np.random.RandomState(seed)
    M = rng.normal(0, 1, (n, n))
    return M @ M.T + n * np.eye(n), rng.normal(0, 1, n)


def host_cholesky(lib, A, b):
    """solver_detail::choleskySolve through the host library -> (rc, x, L with zeros above the diagonal)"""
    n = len(b)
    Aw, x = np.ascontiguousarray(A, np.float64).copy(), np.ascontiguousarray(b, np.float64).copy()
    lib.icgh_dense_cholesky_solve.argtypes = [C.c_int, C.c_void_p, C.c_void_p]
    lib.icgh_dense_cholesky_solve.restype = C.c_int
    rc = lib.icgh_dense_cholesky_solve(n, Aw.ctypes.data, x.ctypes.data)
    return rc, x, np.tril(Aw.reshape(n, n))


def device_cholesky(ctx, systems):
    """systems: list of (A, b) -> list of (x, L, status) per system from ONE icg_chol_solve_batch call"""
    n = np.array([len(b) for _, b in systems], np.int32)
    A = np.concatenate([np.ascontiguousarray(a, np.float64).reshape(-1) for a, _ in systems])
    b = np.concatenate([np.ascontiguousarray(v, np.float64) for _, v in systems])
    x, L, st = ctx.chol_solve_batch(n, A, b)
    out, oa, ob = [], 0, 0
    for k, nk in enumerate(n):
        out.append((x[ob:ob + nk], L[oa:oa + nk * nk].reshape(nk, nk), int(st[k])))
        oa, ob = oa + nk * nk, ob + nk
    return out


def solve_batch_mode(lib, problems, mode, prior_weight=30.0, huber=1.0, iters1=6, iters2=18, chi2=5.991, solve_ms=None):
    """icgh_backend_solve_batch_mode (mode = None: icgh_backend_solve_batch) -> (rc, message, list of result dicts); a list given as
    solve_ms receives the entry's own time of solve + culling + solve"""
    W = len(problems)
    off = lambda sizes: np.concatenate([[0], np.cumsum(sizes)]).astype(np.int32)
    fac_off = off([P["obs"].shape[1] for P in problems])
    pose_off = off([P["start"]["poses"].shape[0] for P in problems])
    lm_off = off([len(P["start"]["invdepth"]) for P in problems])
    obs = np.ascontiguousarray(np.concatenate([P["obs"] for P in problems], axis=1))
    ii, jj, ll = (np.ascontiguousarray(np.concatenate([P[k] for P in problems]), np.int32) for k in ("ii", "jj", "ll"))
    poses = np.ascontiguousarray(np.concatenate([P["start"]["poses"] for P in problems]))
    ext = np.ascontiguousarray(np.stack([P["start"]["ext"] for P in problems]))
    inv = np.ascontiguousarray(np.concatenate([P["start"]["invdepth"] for P in problems]))
    td = np.array([P["start"]["td"] for P in problems], np.float64)
    prior = np.ascontiguousarray(np.concatenate([P["prior"] for P in problems]))
    summ, ms, err = np.zeros((W, 8)), C.c_double(0), ErrBuf()
    args = [W, ptr(fac_off), ptr(pose_off), ptr(lm_off), ptr(obs), ptr(ii), ptr(jj), ptr(ll), ptr(poses), ptr(ext), ptr(inv), ptr(td), ptr(prior),
            C.c_double(prior_weight), C.c_double(huber), 0, 0, int(iters1), int(iters2), C.c_double(chi2), ptr(summ), C.byref(ms), *err.args]
    rc = lib.icgh_backend_solve_batch(*args) if mode is None else lib.icgh_backend_solve_batch_mode(*args, int(mode))
    if solve_ms is not None:
        solve_ms.append(ms.value)
    out = [dict(poses=poses[pose_off[w]:pose_off[w + 1]], ext=ext[w], invdepth=inv[lm_off[w]:lm_off[w + 1]], td=td[w:w + 1], summary=summ[w])
           for w in range(W)]
    return rc, err.text(), out


def assert_same_results(a, b):
    """The batch entry returns no per-factor active flags: what it returns of the culling is summary[7], the number of factors the chi-square
    test between the two solves switched off, and every state the second solve reached on the factors left.  Both are compared here; a
    differing flag changes the second solve's system and with it these bits."""
    for w, (ra, rb) in enumerate(zip(a, b)):
        for key in ("summary", "poses", "ext", "invdepth", "td"):
            assert np.array_equal(bits(ra[key]), bits(rb[key])), (w, key, ra[key], rb[key])
