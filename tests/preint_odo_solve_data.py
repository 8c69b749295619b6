"""Shared by the odometer device-preintegration solver tests and profiles/preint_odo_solve_probe.py: the windows of prior_solve_data with
17-wide states (sodo behind the 16), 9-column IMU rows (the odometer increment behind the 8) and marginalization priors over pose (7) and mix
(10) blocks, and icgh_backend_solve_preint_odo_batch, which takes the integration results of the windows' intervals as arrays."""
import ctypes as C

import numpy as np

import preint_odo_data as od
from ctypes_util import ErrBuf, f64, i32, ptr, ptrs

PARAMS25 = od.params25()  # (the Earth rate of preint_data.PARAMS: non-zero, so that variant 3 is another problem than variant 2)


def odo_window(win, start):
    """a vio_data window and its (states K x 16, invdepth) start -> (imu9 rows, start states K x 17)"""
    imu = np.asarray(win["imu"], np.float64)
    k = np.arange(len(imu))
    odo = imu[:, 1] * (3.0 + 0.4 * np.sin(0.9 * k * imu[:, 1]))
    st = np.asarray(start[0], np.float64)
    return np.concatenate([imu, odo[:, None]], axis=1), np.concatenate([st, np.full((len(st), 1), od.SODO)], axis=1)


def intervals_of(wins, starts):
    """every interval of every window, window after window: (imu9 rows per interval, start state 17 per interval, intervals per window)"""
    imus, s0, counts = [], [], []
    for win, start in zip(wins, starts):
        imu9, st17 = odo_window(win, start)
        off = win["offsets"]
        counts.append(len(off) - 1)
        for k in range(len(off) - 1):
            imus.append(imu9[off[k]:off[k + 1]])
            s0.append(st17[k])
    return imus, s0, counts


def integrate_on_host(variant, wins, starts):
    """preint_odo_data.integrate_ld in float64 for every interval -> list of result dicts (delta, jac, cov, dt, pn), interval after interval"""
    imus, s0, _ = intervals_of(wins, starts)
    return [od.integrate_ld(variant, imu, s, PARAMS25, dtype=np.float64) for imu, s in zip(imus, s0)]


def integrate_on_device(ctx, variant, wins, starts):
    """one icg_preint_odo_batch call for every interval of every window -> the same list"""
    imus, s0, _ = intervals_of(wins, starts)
    off = np.cumsum([0] + [len(m) for m in imus]).astype(np.int32)
    cur, delta, jac, cov, dt, pn = ctx.preint_odo_batch(variant, off, np.concatenate(imus), np.stack(s0), PARAMS25)
    return [dict(delta=delta[k], jac=jac[k], cov=cov[k], dt=dt[k], pn=pn[off[k]:off[k + 1] - 1]) for k in range(len(imus))]


def make_prior(win, states, seed, weight=10.0, e0_scale=0.5):
    """prior_solve_data.make_prior over pose (7) and 10-wide mix blocks, linearized at the window's true states with sodo = SODO"""
    rng = np.random.RandomState(seed)
    blocks = [(2 * k, 7) for k in states] + [(2 * k + 1, 10) for k in states]
    blocks = [blocks[i] for i in rng.permutation(len(blocks))]
    index, col = [0] * len(blocks), 0
    for b in rng.permutation(len(blocks)):
        index[b] = col
        col += 6 if blocks[b][1] == 7 else 10
    r = col
    x0 = [np.concatenate([win["states"][c // 2, 7:], [od.SODO]]) if c % 2 else win["states"][c // 2, :7] for c, _ in blocks]
    return dict(r=r, size=np.array([s for _, s in blocks], np.int32), index=np.array(index, np.int32), param=np.array([c for c, _ in blocks], np.int32),
                x0=np.ascontiguousarray(np.concatenate(x0)), J0=np.ascontiguousarray(weight * (np.eye(r) + 0.25 * rng.uniform(-1, 1, (r, r)))),
                e0=rng.normal(0, e0_scale, r))


def five_windows(oracle):
    """prior_solve_data.five_windows with priors over 10-wide mix blocks -> (windows, starts, priors, state_const)"""
    import prior_solve_data as ps
    wins, starts, _, const = ps.five_windows(oracle)
    priors = [make_prior(wins[0], range(2), 31), None, make_prior(wins[2], range(4), 35), make_prior(wins[3], [0, 1, 2, 5], 34), make_prior(wins[4], range(8), 35)]
    return wins, starts, priors, const


def result_arrays(wins, results):
    """the integration results of every interval, window after window, as the per-window arrays the entries take
    -> (delta, jac, cov, dt, iewn, pn_off, pn)"""
    W = len(wins)
    counts = [len(w["offsets"]) - 1 for w in wins]
    at = np.cumsum([0] + counts)
    per = lambda key, shape: [f64(np.stack([np.asarray(r[key], np.float64).reshape(shape) for r in results[at[w]:at[w + 1]]])) for w in range(W)]
    iewn = [f64(np.tile(PARAMS25[6:9], (counts[w], 1))) for w in range(W)]
    rows = [[np.asarray(r["pn"], np.float64).reshape(-1, 4) for r in results[at[w]:at[w + 1]]] for w in range(W)]
    pn_off = [i32(np.cumsum([0] + [len(x) for x in rows[w]])) for w in range(W)]
    pn = [f64(np.concatenate(rows[w] + [np.zeros((1, 4))])) for w in range(W)]
    return [per("delta", 20), per("jac", 361), per("cov", 361), per("dt", ()), iewn, pn_off, pn]


def window_arrays(wins, starts, odo):
    """what the solve entries take of the windows themselves, in their order: states (K x 17 with odo, copies), n_fac .. invdepth (copies), td, the
    targets of the priors on state 0 -> (states, [n_fac, obs, ii, jj, ll, ext, n_lm, invdepth, td, pose0, mix0], n_intervals)"""
    st = [f64(odo_window(w, s)[1]).copy() for w, s in zip(wins, starts)] if odo else [f64(s).copy() for s, _ in starts]
    inv = [f64(v).copy() for _, v in starts]
    obs, ii, jj, ll = ([f64(w["obs"]) for w in wins], [i32(w["ii"]) for w in wins], [i32(w["jj"]) for w in wins], [i32(w["ll"]) for w in wins])
    ext, td = [f64(w["ext"]).copy() for w in wins], f64([w["td"] for w in wins])
    pose0 = [f64(w["states"][0, :7]) for w in wins]
    mix0 = [f64(np.concatenate([w["states"][0, 7:], [od.SODO]]) if odo else w["states"][0, 7:]) for w in wins]
    n_int, n_fac, n_lm = i32([len(w["offsets"]) - 1 for w in wins]), i32([o.shape[1] for o in obs]), i32([len(v) for v in inv])
    return st, [n_fac, obs, ii, jj, ll, ext, n_lm, inv, td, pose0, mix0], n_int


def prior_arrays(priors, W, state_const):
    """prior_r, prior_nb, the six tables per window (None without a prior) and the constant-state flags"""
    priors = [None] * W if priors is None else priors
    pr = lambda key, conv: [None if p is None else conv(p[key]) for p in priors]
    p_r, p_nb = i32([0 if p is None else p["r"] for p in priors]), i32([0 if p is None else len(p["size"]) for p in priors])
    tables = [pr("size", i32), pr("index", i32), pr("param", i32), pr("x0", f64), pr("J0", f64), pr("e0", f64)]
    return p_r, p_nb, tables, [None] * W if state_const is None else [None if c is None else i32(c) for c in state_const]


def as_args(arrays):
    """lists of per-window arrays as pointer tables, arrays as pointers"""
    return [ptrs(a) if isinstance(a, list) else ptr(a) for a in arrays]


def solve_preint_odo_batch(lib, wins, starts, results, priors, mode, variant=od.ODO, state_const=None, robust=None, preint_robust=None, iters=25,
                           prior_weight=100.0, huber=1.0, timer=None):
    """icgh_backend_solve_preint_odo_batch on vio_data windows from the given (states K x 16, invdepth) starts; results: the integration
    results of every interval, window after window (integrate_on_host / integrate_on_device); priors[w]: make_prior's dict or None
    -> (rc, message, states K x 17 per window, invdepth, summary W x 4, prior cost W x 2, odometer factors resident on the device)"""
    W = len(wins)
    given = result_arrays(wins, results)
    st, win, n_int = window_arrays(wins, starts, True)
    p_r, p_nb, tables, consts = prior_arrays(priors, W, state_const)
    rob = f64(np.zeros(W) if robust is None else robust)
    prob = f64(np.zeros(W) if preint_robust is None else preint_robust)
    summ, pcost, ms, err, n_dev = np.zeros((W, 4)), np.zeros((W, 2)), C.c_double(0), ErrBuf(), C.c_int32(-1)
    par19 = f64(od.params19(PARAMS25, od.ABV))
    rc = lib.icgh_backend_solve_preint_odo_batch(
        W, ptr(n_int), *as_args(given), ptr(par19), ptrs(st), *as_args(win), C.c_double(prior_weight), C.c_double(huber), int(iters), ptr(p_r), ptr(p_nb),
        *as_args(tables), ptr(rob), ptrs(consts), ptr(summ), ptr(pcost), C.byref(ms), int(variant), ptr(prob), C.byref(n_dev), int(mode), *err.args)
    if timer is not None:
        timer.append(ms.value)
    return rc, err.text(), st, win[7], summ, pcost, n_dev.value
