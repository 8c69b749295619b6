"""Inputs and ctypes wrappers for the many-stream preintegration tests and the probe (icg_preint_batch_params / icg_preint_odo_batch_params,
Preintegration::integrateStreams / PreintegrationOdo::integrateStreams through icgh_backend_preint_streams / icgh_backend_preint_odo_streams).

A family is the 15-state pair (variants 0 Normal, 1 Earth) or the odometer pair (2 Odo, 3 EarthOdo): FAMILIES["imu"] / FAMILIES["odo"] carry
the widths, the edge intervals the issue names (1, 2, 3, 41, 7 samples; odometer 41, 1, 2, 17, 41) and parameter rows that all differ
(Earth rate, gravity, noise figures; odometer also odo_std, odo_srw, cvb through abv, lodo)."""
import numpy as np

import preint_data as pd
import preint_odo_data as od
from ctypes_util import ErrBuf, f64, i32, ptr

SENTINEL = -1.2345e300
WIE = 7.292115e-5


def _rows9(n):
    k = np.arange(n, dtype=np.float64)
    rows = np.tile(pd.PARAMS, (n, 1))
    rows[:, 0] *= 1 + 0.11 * k
    rows[:, 1] *= 1 + 0.07 * k
    rows[:, 2] *= 1 + 0.05 * k
    rows[:, 3] *= 1 + 0.03 * k
    rows[:, 4] *= 1 + 0.02 * k
    rows[:, 5] = 9.8 - 1e-3 * k
    lat = 0.1 + 0.01 * k
    rows[:, 6], rows[:, 7], rows[:, 8] = WIE * np.cos(lat), 1e-7 * k, -WIE * np.sin(lat)
    return rows


class Family:
    def __init__(self, name):
        self.name, self.odo = name, name == "odo"
        self.variants = (2, 3) if self.odo else (0, 1)
        self.earth = self.variants[1]
        self.N = 19 if self.odo else 15
        self.w_imu, self.w_s0, self.w_par, self.w_delta, self.w_point = (9, 17, 25, 20, 34) if self.odo else (8, 16, 9, 16, 32)
        self.lens = [41, 1, 2, 17, 41] if self.odo else [1, 2, 3, 41, 7]
        self.p1, self.s = ("preint_odo", "preint_odo_eval") if self.odo else ("preint", "preint_eval")
        self.entry = "icg_preint_odo_batch_params" if self.odo else "icg_preint_batch_params"
        self.host_entry = "icgh_backend_preint_odo_streams" if self.odo else "icgh_backend_preint_streams"
        self.w_hostpar = 23 if self.odo else 13
        self.w_member = 17 + 20 + 2 + 3 + 3 * 361 if self.odo else 16 + 16 + 2 + 3 + 3 * 225

    # ---- inputs
    def interval(self, n, seed):
        return od._imu9(n, seed) if self.odo else pd.make_interval(n, seed=seed)

    def state(self, k=0):
        kw = dict(p=(1.0 + 40.0 * k, 2.0 - 25.0 * k, -0.5 + 0.3 * k), rv=(0.02, -0.03 + 0.01 * k, 0.4 - 0.05 * k), v=(3.0 + 0.1 * k, 0.2, -0.1))
        return od.state17(sodo=od.SODO * (1 + 0.1 * k), **kw) if self.odo else pd.state(**kw)

    def items(self, lens=None):
        return [(self.interval(n, 50 + i), self.state(i)) for i, n in enumerate(self.lens if lens is None else lens)]

    def abv(self, n):
        k = np.arange(n, dtype=np.float64)[:, None]
        return od.ABV[None, :] + k * np.array([0.0, 1e-3, -2e-3])[None, :]

    def rows(self, n):
        """n parameter rows, no two equal in any group of values"""
        r9 = _rows9(n)
        if not self.odo:
            return r9
        abv = self.abv(n)
        return np.stack([od.params25(abv=abv[k], lodo=od.LODO * (1 + 0.04 * k), odo_std=od.ODO_STD * (1 + 0.05 * k), odo_srw=od.ODO_SRW * (1 + 0.2 * k),
                                     base=r9[k]) for k in range(n)])

    def host_params(self, row, abv):
        """the single-parameter-set row of the host layer's existing entries (params9 / params19)"""
        return od.params19(row, abv) if self.odo else row

    def eval_points(self, items, cur):
        if self.odo:
            return np.stack([od.eval_point(s0, cur[i]) for i, (_, s0) in enumerate(items)])
        return np.stack([np.concatenate([s0, cur[i]]) for i, (_, s0) in enumerate(items)])

    # ---- the C ABI
    def single(self, ctx, variant, imu, s0, row):
        fn = ctx.preint_odo_batch if self.odo else ctx.preint_batch
        return fn(variant, np.array([0, len(imu)], np.int32), imu, s0[None, :], row)

    def batch(self, ctx, variant, items, row):
        fn = ctx.preint_odo_batch if self.odo else ctx.preint_batch
        return fn(variant, offsets_of(items), np.concatenate([i for i, _ in items]), np.stack([s for _, s in items]), row)

    def many(self, ctx, variant, items, rows, **kw):
        fn = ctx.preint_odo_batch_params if self.odo else ctx.preint_batch_params
        return fn(variant, offsets_of(items), np.concatenate([i for i, _ in items]), np.stack([s for _, s in items]), rows, **kw)

    def evaluate(self, ctx, variant, delta, jac, cov, dt, env, points, pn_offsets, pn):
        fn = ctx.preint_odo_evaluate_batch if self.odo else ctx.preint_evaluate_batch
        earth = variant == self.earth
        return fn(variant, delta, jac, cov, dt, env, points, pn_offsets if earth else None, pn if earth else None)


FAMILIES = {"imu": Family("imu"), "odo": Family("odo")}


def offsets_of(items):
    return np.cumsum([0] + [len(imu) for imu, _ in items]).astype(np.int32)


# ---- the host layer's streams entries -------------------------------------------------------------------------------------------------
def host_rows(fam, rows, abv=None, stations=None):
    """parameter rows of icgh_backend_preint[_odo]_streams: the single-set row, has_station, station[3]"""
    n = len(rows)
    abv = fam.abv(n) if abv is None else abv
    out = np.zeros((n, fam.w_hostpar))
    for k in range(n):
        out[k, :fam.w_hostpar - 4] = fam.host_params(rows[k], abv[k])
        if stations is not None:
            out[k, -4], out[k, -3:] = 1.0, stations[k]
    return out


def streams(lib, fam, variant, items, hostrows, mode, passes=1, redo=(), redo_state=None, profile=True):
    """-> dict(rc, msg, members 2 x n x W, ready 2 x n, pn 2 x total x 4, pn_doubles 2 x n, prof 3 x 4, seconds passes + 3); the arrays start
    out as SENTINEL / -1"""
    n = len(items)
    off = offsets_of(items)
    variant = i32(np.full(n, variant) if np.isscalar(variant) else variant)
    imu, s0 = f64(np.concatenate([i for i, _ in items])), f64(np.stack([s for _, s in items]))
    redo = i32(np.asarray(redo, np.int32).reshape(-1))
    rs = f64(np.zeros((1, fam.w_s0)) if redo_state is None else redo_state)
    o = dict(members=np.full((2, n, fam.w_member), SENTINEL), ready=np.full((2, n), -1, np.int32), pn=np.full((2, int(off[-1]), 4), SENTINEL),
             pn_doubles=np.full((2, n), -1, np.int32), prof=np.full((3, 4), -1.0), seconds=np.full(passes + 3, -1.0))
    err = ErrBuf()
    rc = getattr(lib, fam.host_entry)(n, ptr(variant), ptr(off), ptr(imu), ptr(s0), ptr(f64(hostrows)), int(mode), int(passes), 1 if profile else 0, len(redo),
                                      ptr(redo if len(redo) else i32([0])), ptr(rs), ptr(o["members"]), ptr(o["ready"]), ptr(o["pn"]),
                                      ptr(o["pn_doubles"]), ptr(o["prof"]), ptr(o["seconds"]), *err.args)
    o["rc"], o["msg"] = rc, err.text()
    return o


def member_fields(fam):
    """name -> slice of a member row"""
    NN = fam.N * fam.N
    if fam.odo:
        b = 42
        f = dict(cur=slice(0, 17), delta=slice(17, 37), dt=slice(37, 38), time=slice(38, 39), iewn=slice(39, 42))
    else:
        b = 37
        f = dict(cur=slice(0, 16), delta=slice(16, 32), dt=slice(32, 33), time=slice(33, 34), iewn=slice(34, 37))
    f.update(jac=slice(b, b + NN), cov=slice(b + NN, b + 2 * NN), sqrt_info=slice(b + 2 * NN, b + 3 * NN))
    return f
