"""Edge cases, an extended-precision reference and per-block measures for the preintegration inner loop (P1, k_preint).

Cases       named (imu, state0, params) built on preint_data.make_interval / preint_data.state; `cases(variant)` lists those of a variant
            (the Earth variant adds Earth-rate parameter sets on `plain` and `long`, and runs `zero_rotation` with a zero Earth rate).
Reference   integrate_ld: a NumPy np.longdouble (x87 extended, 64-bit significand) restatement of preintegration_base.cc:39-70,86-92,
            preintegration_normal.cc:183-253 and preintegration_earth.cc:205-335 with DENSE phi (15x15) and G (15x12).  It calls neither the
            oracle nor the product: the oracle (oracle/orc_preint.cc) is a line-by-line twin of the kernel, so their agreement alone says
            little about either.
Measures    block_rel (per 3x3 block of a 15x15 array), field_rel (per field of a 16-vector state), whole_rel (the whole-array measure the
            older tests use, kept to show what it misses: the covariance blocks span seven orders of magnitude)."""
import functools

import numpy as np

import preint_data as pd

LD = np.longdouble
# without an extended long double the reference is no arbiter for FP64 code: fail, do not skip
assert np.finfo(LD).eps < 1e-18, "np.longdouble is not x87 extended precision on this platform"

TOL = 1e-12  # the project's statement for this kernel (tests/test_gpu_preint.py: "values agree to ~1e-12 relative")
BLOCKS = ("p", "v", "att", "bg", "ba")

EARTH_RATES = {
    "zero": np.zeros(3),
    "tilted": 7.292115e-5 * np.array([np.cos(0.53), 0.0, -np.sin(0.53)]),
    "amplified": np.array([0.05, -0.03, 0.06]),  # every Earth-rate term is a first-order effect
}


# ---------------------------------------------------------------- cases ----------------------------------------------------------------
def _params(corr_time=None, noise=None, iewn=None):
    p = pd.PARAMS.copy()
    if corr_time is not None:
        p[4] = corr_time
    if noise is not None:
        p[0:4] = noise
    if iewn is not None:
        p[6:9] = iewn
    return p


def _zero_rotation(imu, rows):
    imu = imu.copy()
    imu[rows, 2:5] = 0.0
    return imu


@functools.lru_cache(maxsize=None)
def _base_cases():
    c = {}
    plain = pd.make_interval(41, seed=5)
    c["plain"] = (plain, pd.state(), _params())
    # bg = 0 and dtheta = 0: the bias-compensated increments, hence every rotvec2quat argument, are exactly zero
    s_nobg = pd.state(bg=(0.0, 0.0, 0.0))
    c["zero_rotation"] = (_zero_rotation(pd.make_interval(41, seed=6), slice(None)), s_nobg, _params())
    c["alternating_zero_rotation"] = (_zero_rotation(pd.make_interval(41, seed=7), slice(1, None, 2)), s_nobg, _params())
    imu = pd.make_interval(41, seed=8)
    imu[7, 1:8] = 0.0
    c["dt_zero_sample"] = (imu, pd.state(), _params())
    imu = pd.make_interval(41, seed=9)
    imu[:, 1:8] *= (1.0 + np.random.RandomState(90).uniform(-0.3, 0.3, len(imu)))[:, None]
    c["jitter_dt"] = (imu, pd.state(), _params())
    s = pd.state()
    s[3:7] *= 1.3
    c["non_unit_q0"] = (pd.make_interval(41, seed=10), s, _params())
    s = pd.state()
    s[3:7] *= -1.0
    c["negated_q0"] = (pd.make_interval(41, seed=11), s, _params())
    c["short_corr_time"] = (pd.make_interval(41, seed=12), pd.state(), _params(corr_time=0.5))       # decay 0.99
    c["corr_time_below_dt"] = (pd.make_interval(41, seed=13), pd.state(), _params(corr_time=0.004))  # decay -0.25
    c["zero_noise"] = (pd.make_interval(41, seed=14), pd.state(), _params(noise=0.0))
    c["large_bias"] = (pd.make_interval(41, seed=15), pd.state(bg=(0.05, -0.04, 0.03), ba=(0.5, -0.4, 0.3)), _params())
    c["long"] = (pd.make_interval(401, seed=16), pd.state(), _params())
    c["two_samples"] = (pd.make_interval(2, seed=17), pd.state(), _params())
    c["one_sample"] = (pd.make_interval(1, seed=18), pd.state(), _params())
    for imu, s0, par in c.values():
        imu.setflags(write=False), s0.setflags(write=False), par.setflags(write=False)
    return c


BASE_NAMES = tuple(_base_cases())


def cases(variant):
    """name -> (imu n x 8, state0 16, params 9) of a variant, in a fixed order"""
    out = {}
    for name, (imu, s0, par) in _base_cases().items():
        if variant == 1 and name == "zero_rotation":
            par = _params(iewn=EARTH_RATES["zero"])  # rotvec2quat(-iewn dt) must see an exact zero too
        out[name] = (imu, s0, par)
    if variant == 1:
        for base in ("plain", "long"):
            imu, s0, _ = _base_cases()[base]
            for rate, w in EARTH_RATES.items():
                out[f"{base}@{rate}"] = (imu, s0, _params(iewn=w))
    return out


def groups(variant):
    """the cases of a variant grouped by their parameter vector (a launch takes one): list of (params, [names])"""
    out = []
    for name, (_, _, par) in cases(variant).items():
        for p, names in out:
            if np.array_equal(p, par):
                names.append(name)
                break
        else:
            out.append((par, [name]))
    return out


# -------------------------------------------------------------- reference --------------------------------------------------------------
def _skew(v):
    return np.array([[0, -v[2], v[1]], [v[2], 0, -v[0]], [-v[1], v[0], 0]], LD)


def _qmul(a, b):  # Hamilton product, storage (x, y, z, w)
    av, bv = a[:3], b[:3]
    return np.concatenate([a[3] * bv + b[3] * av + np.cross(av, bv), [a[3] * b[3] - av @ bv]])


def _qinv(q):
    return np.concatenate([-q[:3], q[3:]]) / (q @ q)


def _qmat(q):  # Eigen's toRotationMatrix: from the raw coefficients, no normalisation
    x, y, z, w = q
    return np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - w * z), 2 * (x * z + w * y)],
                     [2 * (x * y + w * z), 1 - 2 * (x * x + z * z), 2 * (y * z - w * x)],
                     [2 * (x * z - w * y), 2 * (y * z + w * x), 1 - 2 * (x * x + y * y)]], LD)


def _rotvec2quat(rv):  # common/rotation.h:72-76
    angle = np.sqrt(rv @ rv)
    axis = rv / angle if angle > 0 else rv
    return np.concatenate([np.sin(angle / 2) * axis, [np.cos(angle / 2)]])


def _normalized(q):
    return q / np.sqrt(q @ q)


def integrate_ld(variant, imu, state0, params, mutate=None):
    """-> dict(cur 16, delta 16, jac 15x15, cov 15x15, dt, pn (n-1) x 4), all np.longdouble.
    mutate (deliberate errors, for showing that a measure sees them; they touch the covariance update only):
      "decay_cov"      the bias rows of phi are identity rows there (1 instead of 1 - dt / corr_time)
      "no_att_bg_cov"  the -I dt block (attitude rows, bg columns) is dropped there"""
    assert mutate in (None, "decay_cov", "no_att_bg_cov")
    imu = np.asarray(imu, np.float64).reshape(-1, 8).astype(LD)
    s0 = np.asarray(state0, np.float64).astype(LD)
    par = np.asarray(params, np.float64).astype(LD)
    gyr_arw, acc_vrw, gbstd, abstd, corr_time = par[:5]
    gravity = np.array([0, 0, par[5]], LD)
    iewn = par[6:9]
    one, half, I3 = LD(1), LD(1) / 2, np.eye(3, dtype=LD)
    p, q, v, bg, ba = s0[0:3], s0[3:7], s0[7:10], s0[10:13], s0[13:16]
    dp, dv, dq = np.zeros(3, LD), np.zeros(3, LD), np.array([0, 0, 0, 1], LD)
    q0 = q.copy()
    T = LD(0)
    J, P = np.eye(15, dtype=LD), np.zeros((15, 15), LD)
    noise = np.diag(np.repeat([gyr_arw * gyr_arw, acc_vrw * acc_vrw, 2 * gbstd * gbstd / corr_time, 2 * abstd * abstd / corr_time], 3))
    pn = np.zeros((max(len(imu) - 1, 0), 4), LD)
    for k in range(1, len(imu)):
        pre_dt, dt = imu[k - 1, 1], imu[k, 1]
        pre_dth, pre_dvl = imu[k - 1, 2:5] - pre_dt * bg, imu[k - 1, 5:8] - pre_dt * ba  # compensationBias
        cur_dth, cur_dvl = imu[k, 2:5] - dt * bg, imu[k, 5:8] - dt * ba
        T = T + dt
        dvfb = cur_dvl + half * np.cross(cur_dth, cur_dvl) + (one / 12) * (np.cross(pre_dth, cur_dvl) + np.cross(pre_dvl, cur_dth))
        dtheta = cur_dth + (one / 12) * np.cross(pre_dth, cur_dth)
        if variant == 0:
            dvel = _qmat(q) @ dvfb + gravity * dt
            p = p + dt * v + half * dt * dvel
            v = v + dvel
            q = _normalized(_qmul(q, _rotvec2quat(dtheta)))
            dvel = _qmat(dq) @ dvfb
            dp = dp + dt * dv + half * dt * dvel
            dv = dv + dvel
            dq = _normalized(_qmul(dq, _rotvec2quat(dtheta)))
            C = -_qmat(dq)  # phi(3,6) = C skew(dvel), phi(3,12) = C dt, G(3,3) = -C
            G_v, G_att = -C, I3
        else:
            dv_cor_g = (gravity - 2 * np.cross(iewn, v)) * dt
            qnn = _rotvec2quat(-iewn * dt)
            dvel = half * (I3 + _qmat(qnn)) @ _qmat(q) @ dvfb + dv_cor_g
            p = p + dt * v + half * dt * dvel
            v = v + dvel
            pn[k - 1, 0], pn[k - 1, 1:4] = dt, p
            q = _normalized(_qmul(_qmul(qnn, q), _rotvec2quat(dtheta)))
            qmid = _rotvec2quat(-(T - half * dt) * iewn)
            dvel = _qmat(_qmul(_qmul(_qmul(_qinv(q0), qmid), q0), dq)) @ dvfb
            dp = dp + dt * dv + half * dt * dvel
            dv = dv + dvel
            dq = _normalized(_qmul(dq, _rotvec2quat(dtheta)))
            qend = _rotvec2quat(-iewn * T)
            C = -_qmat(_qmul(_qmul(_qmul(_qinv(q0), qend), q0), dq))
            G_v, G_att = C, -I3
        phi = np.zeros((15, 15), LD)
        phi[0:3, 0:3] = I3
        phi[0:3, 3:6] = I3 * dt
        phi[3:6, 3:6] = I3
        phi[3:6, 6:9] = C @ _skew(cur_dvl)
        phi[3:6, 12:15] = C * dt
        phi[6:9, 6:9] = I3 - _skew(cur_dth)
        phi[6:9, 9:12] = -I3 * dt
        phi[9:12, 9:12] = I3 * (1 - dt / corr_time)
        phi[12:15, 12:15] = I3 * (1 - dt / corr_time)
        G = np.zeros((15, 12), LD)
        G[3:6, 3:6] = G_v
        G[6:9, 0:3] = G_att
        G[9:12, 6:9] = I3
        G[12:15, 9:12] = I3
        J = phi @ J
        phc = phi.copy()
        if mutate == "decay_cov":
            phc[9:15, 9:15] = np.eye(6, dtype=LD)
        elif mutate == "no_att_bg_cov":
            phc[6:9, 9:12] = 0
        M = G @ noise @ G.T
        P = phc @ P @ phc.T + half * dt * (phc @ M + M @ phc.T)
    return dict(cur=np.concatenate([p, q, v, bg, ba]), delta=np.concatenate([dp, dq, dv, bg, ba]), jac=J, cov=P, dt=T, pn=pn)


@functools.lru_cache(maxsize=None)
def reference(variant, name):
    """integrate_ld of a named case, computed once per process and shared (treat as read-only)"""
    return integrate_ld(variant, *cases(variant)[name])


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
    """15x15 arrays -> (worst value, "row-col" name of the worst 3x3 block), blocks in the order p, v, att, bg, ba"""
    got, exp = np.asarray(got).reshape(15, 15), np.asarray(exp).reshape(15, 15)
    worst = (-1.0, None)
    for i, ni in enumerate(BLOCKS):
        for j, nj in enumerate(BLOCKS):
            r = _rel_or_zero(got[3 * i:3 * i + 3, 3 * j:3 * j + 3], exp[3 * i:3 * i + 3, 3 * j:3 * j + 3])
            if r > worst[0]:
                worst = (r, f"{ni}-{nj}")
    return worst


def field_rel(got, exp):
    """16-vector states -> (worst value, field): p, q, v each relative to their own maximum; bg and ba (which P1 never changes: exp carries
    the input) bit-equal, else inf"""
    got, exp = np.asarray(got, np.float64).reshape(16), np.asarray(exp).reshape(16)
    worst = (-1.0, None)
    for name, sl in (("p", slice(0, 3)), ("q", slice(3, 7)), ("v", slice(7, 10))):
        r = _rel_or_zero(got[sl], exp[sl])
        if r > worst[0]:
            worst = (r, name)
    for name, sl in (("bg", slice(10, 13)), ("ba", slice(13, 16))):
        if not np.array_equal(got[sl].view(np.uint64), np.asarray(exp[sl], np.float64).view(np.uint64)):
            worst = (float("inf"), name)
    return worst


def whole_rel(got, exp):
    """max|got - exp| / max|exp| over the whole array: the measure of the older tests"""
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


def check_result(got, exp, n, what, tol=TOL):
    """got: dict(cur, delta, jac, cov, dt[, pn]) in FP64; exp likewise (any precision).  Asserts the per-block / per-field measures at tol and
    returns the figures {quantity: value}."""
    fig = {"jac": block_rel(got["jac"], exp["jac"]), "cov": block_rel(got["cov"], exp["cov"]),
           "cur": field_rel(got["cur"], exp["cur"]), "delta": field_rel(got["delta"], exp["delta"])}
    for k, (val, where) in fig.items():
        assert val <= tol, f"{what}: {k} block/field {where}: {val:.3g} > {tol:g}"
    ddt = abs(float(LD(float(got["dt"])) - LD(exp["dt"])))
    assert ddt <= 1e-15 * max(1, n), f"{what}: dt off by {ddt:.3g}"
    out = {k: v[0] for k, v in fig.items()}
    if got.get("pn") is not None and exp.get("pn") is not None:
        out["pn"] = pn_rel(got["pn"], exp["pn"])
        assert out["pn"] <= tol, f"{what}: pn: {out['pn']:.3g} > {tol:g}"
    return out
