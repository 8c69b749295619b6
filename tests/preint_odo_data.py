"""Cases, an extended-precision reference and per-block measures for the odometer preintegration (P1: k_preint_odo, variants 2 = Odo and
3 = EarthOdo; 19-wide error state dp, dv, dq, dbg, dba, ds, dsodo).

Cases       named (imu9 n x 9, state0 17, params25, abv 3) built on preint_data.make_interval / preint_data.state: `cases()`; the golden
            (tests/golden/preint_odo_ref_golden.npz, the reference's own classes) holds GOLDEN_NAMES for both variants.
Reference   integrate_ld: a NumPy restatement of preintegration_base.cc:39-70,86-92, preintegration_odo.cc:206-301 and
            preintegration_earth_odo.cc:230-383 with DENSE phi (19 x 19) and G (19 x 16), in np.longdouble (x87 extended) by default.  With
            dtype=np.float64 the same statements run in plain float64 (every matrix product a loop over k ascending from +0.0, no fused
            operations): the dense twin the kernel's sparse products must equal bit for bit where no sin / cos argument differs from zero.
            It calls neither the oracle nor the product.
Measures    block_rel (per block pair of a 19 x 19 array, blocks p, v, att, bg, ba, s, sodo), field_rel (per field of a state row)."""
import functools

import numpy as np

import preint_data as pd

LD = np.longdouble
assert np.finfo(LD).eps < 1e-18, "np.longdouble is not x87 extended precision on this platform"

TOL = 1e-12  # the project's per-block bound for P1 (tests/preint_edge_data.py:21)
BLOCKS = (("p", slice(0, 3)), ("v", slice(3, 6)), ("att", slice(6, 9)), ("bg", slice(9, 12)), ("ba", slice(12, 15)), ("s", slice(15, 18)),
          ("sodo", slice(18, 19)))
ODO, EARTH_ODO = 2, 3
VARIANTS = (ODO, EARTH_ODO)

# odometer noise: 0.05 m/s white noise per axis, 100 ppm / sqrt(Hz) random walk of the scale factor (realistic for a wheel encoder, > 0)
ODO_STD = np.array([0.05, 0.04, 0.06])
ODO_SRW = 1.0e-4
ABV = np.array([0.0, 0.012, -0.021])   # installation angles [rad] (roll is not observable and stays zero in the reference's configuration)
LODO = np.array([0.35, -0.12, 0.48])   # lever arm [m]
SODO = 0.013
GOLDEN_NAMES = ("plain", "two_samples", "three_samples", "standstill", "no_lever", "long")
TILTED = 7.292115e-5 * np.array([np.cos(0.53), 0.0, -np.sin(0.53)])


# ---------------------------------------------------------------- cases ----------------------------------------------------------------
def euler2matrix(e, T=np.float64):
    """Rotation::euler2matrix (rotation.h:84-88): Rz(e[2]) Ry(e[1]) Rx(e[0])"""
    e = np.asarray(e).astype(T)
    sx, cx, sy, cy, sz, cz = np.sin(e[0]), np.cos(e[0]), np.sin(e[1]), np.cos(e[1]), np.sin(e[2]), np.cos(e[2])
    return np.array([[cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx], [sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx],
                     [-sy, cy * sx, cy * cx]], T)


def params25(abv=ABV, lodo=LODO, iewn=None, odo_std=ODO_STD, odo_srw=ODO_SRW, base=None):
    """[0..8] as icg_preint_batch, [9..11] odo_std, [12] odo_srw, [13..21] cvb = euler2matrix(abv)^T row-major, [22..24] lodo"""
    p = np.zeros(25)
    p[:9] = pd.PARAMS if base is None else base
    if iewn is not None:
        p[6:9] = iewn
    p[9:12], p[12] = odo_std, odo_srw
    p[13:22] = euler2matrix(abv).T.reshape(9)
    p[22:25] = lodo
    return p


def params19(par25, abv):
    """what the host layer's C test entries take: [0..12] as params25, [13..15] abv, [16..18] lodo"""
    return np.concatenate([par25[:13], abv, par25[22:25]])


def _imu9(n, seed, odovel="varying"):
    imu = pd.make_interval(n, seed=seed)
    k = np.arange(n)
    odo = np.zeros(n) if odovel == "zero" else imu[:, 1] * (3.0 + 0.4 * np.sin(0.9 * k * imu[:, 1]) + 0.05 * np.cos(11.0 * k * imu[:, 1]))
    return np.concatenate([imu, odo[:, None]], axis=1)


def state17(sodo=SODO, **kw):
    return np.concatenate([pd.state(**kw), [sodo]])


@functools.lru_cache(maxsize=None)
def cases():
    """name -> (imu9 n x 9, state0 17, params25, abv 3), in a fixed order"""
    c = {}
    c["plain"] = (_imu9(41, 31), state17(), params25(), ABV)
    c["two_samples"] = (_imu9(2, 32), state17(), params25(), ABV)
    c["three_samples"] = (_imu9(3, 33), state17(), params25(), ABV)
    c["standstill"] = (_imu9(41, 34, odovel="zero"), state17(), params25(), ABV)  # s moves by the lever-arm term only
    z = np.zeros(3)
    c["no_lever"] = (_imu9(41, 35), state17(), params25(abv=z, lodo=z), z)
    c["long"] = (_imu9(201, 36), state17(), params25(), ABV)
    c["seven_samples"] = (_imu9(7, 37), state17(), params25(), ABV)
    c["one_sample"] = (_imu9(1, 38), state17(), params25(), ABV)
    # dtheta = 0, bg = 0, identity attitude, zero Earth rate: every sin / cos argument is exactly zero
    imu = _imu9(41, 39)
    imu[:, 2:5] = 0.0
    c["zero_rotation"] = (imu, state17(rv=(0.0, 0.0, 0.0), bg=(0.0, 0.0, 0.0)), params25(iewn=z), ABV)
    for imu, s0, par, abv in c.values():
        imu.setflags(write=False), s0.setflags(write=False), par.setflags(write=False)
    return c


def with_rate(par25, iewn):
    p = np.array(par25, np.float64)
    p[6:9] = iewn
    return p


def eval_point(s0, cur):
    """an evaluation point off the integrated state (pose0[7] mix0[10] pose1[7] mix1[10]): the start state with the biases and the scale
    factor moved (so that every first-order correction of evaluate() is exercised), the end state cur moved in every field"""
    s0, cur = np.asarray(s0, np.float64), np.asarray(cur, np.float64)
    mix0 = np.concatenate([s0[7:10], s0[10:13] + [2e-6, -3e-6, 1e-6], s0[13:16] + [1e-4, 2e-4, -1e-4], [s0[16] + 5e-4]])
    pose1 = cur[:7] + [0.01, -0.02, 0.005, 1e-3, -2e-3, 5e-4, 0.0]  # non-unit end quaternion (Ceres hands over whatever Plus() produced)
    mix1 = np.concatenate([cur[7:10] + 0.01, mix0[3:6] + 1e-5, mix0[6:9] + 1e-4, [mix0[9] + 1e-3]])
    return np.concatenate([s0[:7], mix0, pose1, mix1])


# -------------------------------------------------------------- reference --------------------------------------------------------------
# 3-vector / quaternion (x, y, z, w) / 3x3 helpers in the operation order of csrc/dev_math.h, for any NumPy float type
def _v(T, *x):
    return np.array(x, T)


def _crs(a, b):
    return np.array([a[1] * b[2] - a[2] * b[1], a[2] * b[0] - a[0] * b[2], a[0] * b[1] - a[1] * b[0]], a.dtype)


def _qinv(q):
    n2 = q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3]
    return np.array([-q[0] / n2, -q[1] / n2, -q[2] / n2, q[3] / n2], q.dtype)


def _qmul(a, b):
    ax, ay, az, aw = a
    bx, by, bz, bw = b
    return np.array([aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz, aw * bz + az * bw + ax * by - ay * bx,
                     aw * bw - ax * bx - ay * by - az * bz], a.dtype)


def _qmat(q):
    x, y, z, w = q
    two = q.dtype.type(2)
    tx, ty, tz = two * x, two * y, two * z
    twx, twy, twz = tx * w, ty * w, tz * w
    txx, txy, txz, tyy, tyz, tzz = tx * x, ty * x, tz * x, ty * y, tz * y, tz * z
    one = q.dtype.type(1)
    return np.array([[one - (tyy + tzz), txy - twz, txz + twy], [txy + twz, one - (txx + tzz), tyz - twx],
                     [txz - twy, tyz + twx, one - (txx + tyy)]], q.dtype)


def _mmul(p, q):
    return p[:, 0:1] * q[0:1, :] + p[:, 1:2] * q[1:2, :] + p[:, 2:3] * q[2:3, :]


def _mvec(m, v):
    return m[:, 0] * v[0] + m[:, 1] * v[1] + m[:, 2] * v[2]


def _skew(v):
    z = v.dtype.type(0)
    return np.array([[z, -v[2], v[1]], [v[2], z, -v[0]], [-v[1], v[0], z]], v.dtype)


def _normalized(q):
    n = np.sqrt(q[0] * q[0] + q[1] * q[1] + q[2] * q[2] + q[3] * q[3])
    return q / n


def _rotvec2quat(rv):
    T = rv.dtype.type
    angle = np.sqrt(rv[0] * rv[0] + rv[1] * rv[1] + rv[2] * rv[2])
    axis = rv / angle if angle > 0 else rv
    s, c = np.sin(T(0.5) * angle), np.cos(T(0.5) * angle)
    return np.array([s * axis[0], s * axis[1], s * axis[2], c], rv.dtype)


def _dense(a, b):
    """a @ b as the dense sum over k ascending from +0.0, one rounding per multiplication and per addition"""
    out = np.zeros((a.shape[0], b.shape[1]), a.dtype)
    for k in range(a.shape[1]):
        out = out + a[:, k:k + 1] * b[k:k + 1, :]
    return out


def integrate_ld(variant, imu9, state0, par25, dtype=LD):
    """-> dict(cur 16, delta 20 = p q v bg ba s sodo, jac 19x19, cov 19x19, dt, pn (n-1) x 4), all of `dtype`"""
    assert variant in VARIANTS
    T = np.dtype(dtype).type
    imu = np.asarray(imu9, np.float64).reshape(-1, 9).astype(T)
    s0 = np.asarray(state0, np.float64).reshape(17).astype(T)
    par = np.asarray(par25, np.float64).reshape(25).astype(T)
    gyr_arw, acc_vrw, gbstd, abstd, corr_time = par[:5]
    one, two, half, twelfth = T(1), T(2), T(0.5), T(1) / T(12)
    gravity = _v(T, 0, 0, par[5])
    iewn = par[6:9]
    cvb, lodo = par[13:22].reshape(3, 3), par[22:25]
    lodo_skew = _skew(lodo)
    I3 = np.eye(3, dtype=T)
    p, q, v, bg, ba, sodo = s0[0:3], s0[3:7], s0[7:10], s0[10:13], s0[13:16], s0[16]
    one_sodo = one + sodo
    dp, dv, ds, dq = np.zeros(3, T), np.zeros(3, T), np.zeros(3, T), _v(T, 0, 0, 0, 1)
    q0 = q.copy()
    time = T(0)
    J, P = np.eye(19, dtype=T), np.zeros((19, 19), T)
    noise = np.concatenate([np.repeat([gyr_arw * gyr_arw, acc_vrw * acc_vrw, two * gbstd * gbstd / corr_time, two * abstd * abstd / corr_time], 3),
                            par[9:12] * par[9:12], [par[12] * par[12]]]).astype(T)
    pn = np.zeros((max(len(imu) - 1, 0), 4), T)
    for k in range(1, len(imu)):
        pre_dt, dt, odovel = imu[k - 1, 1], imu[k, 1], imu[k, 8]
        pre_dth, pre_dvl = imu[k - 1, 2:5] - pre_dt * bg, imu[k - 1, 5:8] - pre_dt * ba  # compensationBias
        cur_dth, cur_dvl = imu[k, 2:5] - dt * bg, imu[k, 5:8] - dt * ba
        cd = _mvec(cvb, _v(T, odovel, 0, 0))
        sv = one_sodo * cd
        lev = (sv - _mvec(_qmat(_rotvec2quat(cur_dth)), lodo)) + lodo
        dvfb = (cur_dvl + half * _crs(cur_dth, cur_dvl)) + twelfth * (_crs(pre_dth, cur_dvl) + _crs(pre_dvl, cur_dth))
        dtheta = cur_dth + twelfth * _crs(pre_dth, cur_dth)
        if variant == ODO:
            ds = ds + _mvec(_qmat(dq), lev)  # before integration(), the old delta q
            time = time + dt
            dvel = _mvec(_qmat(q), dvfb) + dt * gravity
            p = (p + dt * v) + (half * dt) * dvel
            v = v + dvel
            q = _normalized(_qmul(q, _rotvec2quat(dtheta)))
            dvel = _mvec(_qmat(dq), dvfb)
            dp = (dp + dt * dv) + (half * dt) * dvel
            dv = dv + dvel
            dq = _normalized(_qmul(dq, _rotvec2quat(dtheta)))
            gv = _qmat(dq)
            C = -gv
            g60 = one
        else:
            time = time + dt
            dv_cor_g = dt * (gravity - two * _crs(iewn, v))
            qnn = _rotvec2quat(dt * (-iewn))
            halfm = (I3 + _qmat(qnn)) * half
            dvel = _mvec(_mmul(halfm, _qmat(q)), dvfb) + dv_cor_g
            p = (p + dt * v) + (half * dt) * dvel
            v = v + dvel
            pn[k - 1, 0], pn[k - 1, 1:4] = dt, p
            q = _normalized(_qmul(_qmul(qnn, q), _rotvec2quat(dtheta)))
            dnn = (-(time - half * dt)) * iewn
            cbbe = _qmat(_qmul(_qmul(_qmul(_qinv(q0), _rotvec2quat(dnn)), q0), dq))  # mid-interval, the old delta q
            ds = ds + _mvec(cbbe, lev)
            dvel = _mvec(cbbe, dvfb)
            dp = (dp + dt * dv) + (half * dt) * dvel
            dv = dv + dvel
            dq = _normalized(_qmul(dq, _rotvec2quat(dtheta)))
            C = -_qmat(_qmul(_qmul(_qmul(_qinv(q0), _rotvec2quat(time * (-iewn))), q0), dq))
            gv = C
            g60 = -one
        stheta = sv - _crs(cur_dth, lodo)
        phi = np.zeros((19, 19), T)
        phi[0:3, 0:3] = I3
        phi[0:3, 3:6] = I3 * dt
        phi[3:6, 3:6] = I3
        phi[3:6, 6:9] = _mmul(C, _skew(cur_dvl))
        phi[3:6, 12:15] = C * dt
        phi[6:9, 6:9] = I3 - _skew(cur_dth)
        phi[6:9, 9:12] = I3 * (-dt)
        phi[9:12, 9:12] = I3 * (one - dt / corr_time)
        phi[12:15, 12:15] = I3 * (one - dt / corr_time)
        phi[15:18, 6:9] = _mmul(C, _skew(stheta))
        phi[15:18, 9:12] = _mmul(C, lodo_skew) * dt
        phi[15:18, 15:18] = I3
        phi[15:18, 18] = _mvec(-C, cd)
        phi[18, 18] = one
        G = np.zeros((19, 16), T)
        G[3:6, 3:6] = gv
        G[6:9, 0:3] = I3 * g60
        G[9:12, 6:9] = I3
        G[12:15, 9:12] = I3
        G[15:18, 0:3] = _mmul(gv, lodo_skew)
        G[15:18, 12:15] = _mmul(gv, cvb) * one_sodo
        G[18, 15] = one
        M = _dense(G * noise[None, :], G.T.copy())
        T1, T2, T3 = _dense(phi, J), _dense(phi, P), _dense(phi, M)
        phiT = phi.T.copy()
        J = T1
        P = _dense(T2, phiT) + (half * dt) * (T3 + _dense(M, phiT))
    return dict(cur=np.concatenate([p, q, v, bg, ba]), delta=np.concatenate([dp, dq, dv, bg, ba, ds, [sodo]]), jac=J, cov=P, dt=time, pn=pn)


@functools.lru_cache(maxsize=None)
def reference(variant, name, rate=None):
    """integrate_ld of a named case (rate: an Earth rate as a tuple, replacing the case's), computed once per process (treat as read-only)"""
    imu, s0, par, _ = cases()[name]
    return integrate_ld(variant, imu, s0, par if rate is None else with_rate(par, np.array(rate)))


# --------------------------------------------------------------- measures --------------------------------------------------------------
def _rel_or_zero(got, exp):
    """max|got - exp| / max|exp|; where exp is all zero, got must be all == 0.0 (else inf)"""
    got, exp = np.asarray(got).astype(LD), np.asarray(exp).astype(LD)
    if not np.all(np.isfinite(got)):
        return float("inf")
    m = np.abs(exp).max() if exp.size else LD(0)
    if m == 0:
        return 0.0 if np.all(got == 0.0) else float("inf")
    return float(np.abs(got - exp).max() / m)


def block_rel(got, exp):
    """19x19 arrays -> (worst value, "row-col" name of the worst block), blocks p, v, att, bg, ba, s (3 wide) and sodo (1 wide)"""
    got, exp = np.asarray(got).reshape(19, 19), np.asarray(exp).reshape(19, 19)
    worst = (-1.0, None)
    for ni, si in BLOCKS:
        for nj, sj in BLOCKS:
            r = _rel_or_zero(got[si, sj], exp[si, sj])
            if r > worst[0]:
                worst = (r, f"{ni}-{nj}")
    return worst


def _bit_equal(a, b):
    return np.array_equal(np.ascontiguousarray(a, np.float64).view(np.uint64), np.ascontiguousarray(np.asarray(b, np.float64)).view(np.uint64))


def field_rel(got, exp):
    """state rows (cur 16 or delta 20) -> (worst value, field): p, q, v and s each relative to their own maximum; bg, ba and sodo (which P1
    never changes: exp carries the input) bit-equal, else inf"""
    got, exp = np.asarray(got, np.float64).ravel(), np.asarray(exp).ravel()
    assert got.shape == exp.shape and got.size in (16, 20)
    fields = [("p", slice(0, 3)), ("q", slice(3, 7)), ("v", slice(7, 10))] + ([("s", slice(16, 19))] if got.size == 20 else [])
    worst = (-1.0, None)
    for name, sl in fields:
        r = _rel_or_zero(got[sl], exp[sl])
        if r > worst[0]:
            worst = (r, name)
    for name, sl in [("bg", slice(10, 13)), ("ba", slice(13, 16))] + ([("sodo", slice(19, 20))] if got.size == 20 else []):
        if not _bit_equal(got[sl], exp[sl]):
            worst = (float("inf"), name)
    return worst


def whole_rel(got, exp):
    """max|got - exp| / max|exp| over the whole array: the measure of tests/test_gpu_preint.py"""
    got, exp = np.asarray(got).astype(LD), np.asarray(exp).astype(LD)
    return float(np.abs(got - exp).max() / max(LD(1e-300), np.abs(exp).max()))


def pn_rel(got, exp):
    """pn rows (dt, position): dt bit-equal (else inf); positions within their own magnitude"""
    got, exp = np.asarray(got, np.float64).reshape(-1, 4), np.asarray(exp).reshape(-1, 4)
    if got.shape != exp.shape:
        return float("inf")
    if len(exp) == 0:
        return 0.0
    if not np.array_equal(got[:, 0], np.asarray(exp[:, 0], np.float64)):
        return float("inf")
    return _rel_or_zero(got[:, 1:], exp[:, 1:])


def figures(got, exp):
    """{quantity: (value, where)} of the per-block / per-field measures"""
    return {"jac": block_rel(got["jac"], exp["jac"]), "cov": block_rel(got["cov"], exp["cov"]), "cur": field_rel(got["cur"], exp["cur"]),
            "delta": field_rel(got["delta"], exp["delta"])}


def check_result(got, exp, n, what, tol=TOL):
    """got: dict(cur, delta, jac, cov, dt[, pn]) in FP64; exp likewise (any precision).  Asserts the per-block / per-field measures at tol
    and returns the figures {quantity: value}."""
    fig = figures(got, exp)
    for k, (val, where) in fig.items():
        assert val <= tol, f"{what}: {k} block/field {where}: {val:.3g} > {tol:g}"
    ddt = abs(float(LD(float(got["dt"])) - LD(exp["dt"])))
    assert ddt <= 1e-15 * max(1, n), f"{what}: dt off by {ddt:.3g}"
    out = {k: v[0] for k, v in fig.items()}
    if got.get("pn") is not None and exp.get("pn") is not None:
        out["pn"] = pn_rel(got["pn"], exp["pn"])
        assert out["pn"] <= tol, f"{what}: pn: {out['pn']:.3g} > {tol:g}"
    return out


# ---------------------------------------------------------------- golden ---------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def golden():
    """tests/golden/preint_odo_ref_golden.npz -> list of result dicts (case, variant, station, iewn, cur, delta, jac, cov, dt, pn, point, r,
    J) with the inputs of their case attached (imu, s0, par25 carrying the reference's Earth rate, abv)"""
    import os
    g = np.load(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "preint_odo_ref_golden.npz"))
    out = []
    for k in range(int(g["n_results"])):
        r = {key: g[f"r{k}_{key}"] for key in ("station", "iewn", "cur", "delta", "jac", "cov", "pn", "point", "r", "J")}
        r["case"], r["variant"], r["dt"] = str(g[f"r{k}_case"]), int(g[f"r{k}_variant"]), float(g[f"r{k}_dt"])
        name = r["case"]
        r["imu"], r["s0"], r["abv"] = g[f"in_{name}_imu"], g[f"in_{name}_s0"], g[f"in_{name}_abv"]
        r["par25"] = with_rate(g[f"in_{name}_par25"], r["iewn"])
        out.append(r)
    return out
