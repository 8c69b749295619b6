"""GPU parity: batched IMU preintegration factor evaluation (P2, icg_preint_evaluate_batch) against the CPU oracle, the reference golden
and the host layer's own Preintegration::evaluate.  FP64 on both sides, no FMA contraction on either; the square-root information is
+ - * / sqrt only and is held to bit patterns against the host; residual and Jacobians contain sin/cos (device libm vs glibc) and the
oracle's own inversion, whose differences the whitening amplifies: they are held to the bound the project already uses for this quantity,
1e-6 x max(1, max|expected|) (backend_utils.check_preintegration), and the measured maximum is printed.

The 2-sample interval of the case list has a covariance whose inverse is not positive definite (one integration step leaves the position
block zero): the oracle and the host layer both return NaN in every entry for it (the Cholesky step takes the root of a negative number;
status 0: no pivot is zero).
A NaN cannot satisfy `|got - expected| < bound`, so the comparison is NaN-aware: got must be NaN exactly where expected is, and every other
entry is held to the bound; bit-for-bit comparisons hold the non-NaN entries to their bit patterns and the NaN entries to being NaN (the sign
and payload of a NaN are not part of IEEE arithmetic's results and differ between an x86 host and the device)."""
import ctypes as C

import numpy as np
import pytest

import preint_data as pd
import reproj_data as rd
from ctypes_util import ErrBuf, f64, ptr

pytestmark = pytest.mark.gpu

LENS = [41, 17, 2, 101, 60]
PERTURB = np.array([0.01, -0.02, 0.01, 0.001, 0.002, -0.001])


@pytest.fixture(scope="module")
def ctx():
    import icgvins
    c = icgvins.Context(640, 480, n_slots=1, max_batch=1, max_points=64)
    yield c
    c.close()


@pytest.fixture(scope="module")
def hostlib():
    import harness
    return C.CDLL(harness.HOST_LIB)


def _bound(exp):
    fin = np.abs(exp[np.isfinite(exp)])
    return 1e-6 * max(1.0, fin.max() if fin.size else 0.0)


def _err(got, exp):
    """max |got - exp| over the entries where exp is finite; got must be NaN exactly where exp is NaN"""
    got, exp = np.asarray(got), np.asarray(exp)
    assert np.array_equal(np.isnan(got), np.isnan(exp))
    m = np.isfinite(exp)
    return float(np.abs(got[m] - exp[m]).max()) if m.any() else 0.0


def _amax(a):
    a = np.abs(a[np.isfinite(a)])
    return float(a.max()) if a.size else 0.0


def _same_bits(a, b):
    """bit patterns equal on every non-NaN entry, NaN in the same places"""
    a, b = np.ascontiguousarray(a).ravel(), np.ascontiguousarray(b).ravel()
    na, nb = np.isnan(a), np.isnan(b)
    return np.array_equal(na, nb) and np.array_equal(a.view(np.uint64)[~na], b.view(np.uint64)[~nb])


def _eval_point(state0, cur, perturb=PERTURB, q1_scale=1.0):
    pose0, mix0 = pd.split(state0)
    pose1, mix1 = pd.split(cur)
    pose1 = rd.pose_plus(pose1, perturb)
    pose1[3:] *= q1_scale
    return np.concatenate([pose0, mix0, pose1, mix1])


def _pack(pres, params_list):
    """integration results (dicts with delta, jac, cov, dt, pn) -> the arrays of icg_preint_evaluate_batch"""
    delta = np.stack([p["delta"] for p in pres])
    jac = np.stack([np.asarray(p["jac"]).reshape(225) for p in pres])
    cov = np.stack([np.asarray(p["cov"]).reshape(225) for p in pres])
    dt = np.array([float(p["dt"]) for p in pres])
    env = np.stack([np.asarray(q)[5:9] for q in params_list])
    pn_off = np.cumsum([0] + [len(p["pn"]) for p in pres]).astype(np.int32)
    rows = [np.asarray(p["pn"]).reshape(-1, 4) for p in pres]
    pn = np.concatenate(rows) if pn_off[-1] > 0 else np.zeros((1, 4))
    return delta, jac, cov, dt, env, pn_off, pn


def _evaluate(ctx, variant, pres, params_list, points, want_jac=True):
    delta, jac, cov, dt, env, pn_off, pn = _pack(pres, params_list)
    return ctx.preint_evaluate_batch(variant, delta, jac, cov, dt, env, np.stack(points), pn_off if variant else None, pn if variant else None,
                                     want_jac=want_jac)


def _oracle_eval(oracle, variant, pre, params, ep):
    r, J = oracle.preint_evaluate(variant, pre, [0, 0, params[5]], params[6:9], ep[:7], ep[7:16], ep[16:23], ep[23:32])
    return r, np.concatenate([J[0].ravel(), J[1].ravel(), J[2].ravel(), J[3].ravel()])


def _intervals(oracle, variant, lens=LENS, seed0=20):
    imus = [pd.make_interval(n, seed=seed0 + i) for i, n in enumerate(lens)]
    states = [pd.state(p=(i, 1, 0), v=(2, 0.1 * i, 0)) for i in range(len(lens))]
    pres = [oracle.preint_integrate(variant, imus[i], states[i], pd.PARAMS) for i in range(len(lens))]
    return imus, states, pres


@pytest.mark.parametrize("variant", [0, 1])
def test_matches_oracle_on_identical_inputs(oracle, ctx, variant):
    _, states, pres = _intervals(oracle, variant)
    points = [_eval_point(states[i], pres[i]["cur"]) for i in range(len(LENS))]
    # one more factor on the first interval, with a non-unit end quaternion
    pres.append(pres[0])
    points.append(_eval_point(states[0], pres[0]["cur"], q1_scale=1.01))
    params = [pd.PARAMS] * len(pres)
    res, J, S, status = _evaluate(ctx, variant, pres, params, points)
    assert np.all(status == 0)
    worst = 0.0
    for i in range(len(pres)):
        r_exp, J_exp = _oracle_eval(oracle, variant, pres[i], pd.PARAMS, points[i])
        er, eJ = _err(res[i], r_exp), _err(J[i], J_exp)
        worst = max(worst, er / max(1.0, _amax(r_exp)), eJ / max(1.0, _amax(J_exp)))
        print(f"variant {variant} factor {i}: |dr| {er:.3e} (max|r| {_amax(r_exp):.3e})  |dJ| {eJ:.3e} (max|J| {_amax(J_exp):.3e})")
        if len(pres[i]["pn"]) != 1:  # (every interval but the 2-sample one has a finite, non-trivial expected residual)
            assert np.all(np.isfinite(r_exp)) and np.abs(r_exp).max() > 1e-3
        assert er < _bound(r_exp), i
        assert eJ < _bound(J_exp), i
    print(f"variant {variant}: measured maximum vs oracle, relative to max(1, max|expected|): {worst:.3e} (bound 1e-6)")


def test_matches_reference_golden(ctx):
    """every case of tests/golden/preint_ref_golden.npz (outputs of the reference's own PreintegrationFactor): the golden integration
    result in, r and J out, at the bound of backend_utils.check_preintegration_golden"""
    from test_oracle_vs_reference import preint_golden_cases
    n_cases, worst = 0, 0.0
    for k, c in preint_golden_cases():
        variant = int(c["variant"])
        offsets = np.array([0, len(c["imu"])], np.int32)
        pn = ctx.preint_batch(variant, offsets, c["imu"], c["s0"][None, :], c["params"])[5][:len(c["imu"]) - 1]
        pre = dict(delta=c["delta"], jac=c["jac"], cov=c["cov"], dt=float(c["dt"]), pn=pn if variant else np.zeros((0, 4)))
        pose0, mix0 = pd.split(c["s0"])
        pose1, mix1 = pd.split(c["s1"])
        ep = np.concatenate([pose0, mix0, pose1, mix1])
        res, J, _, status = _evaluate(ctx, variant, [pre], [c["params"]], [ep])
        assert status[0] == 0
        er, eJ = _err(res[0], c["r"]), _err(J[0], c["J"])
        worst = max(worst, er / max(1.0, _amax(c["r"])), eJ / max(1.0, _amax(c["J"])))
        print(f"golden case {k} (variant {variant}): |dr| {er:.3e}  |dJ| {eJ:.3e}")
        assert er < _bound(c["r"]), k
        assert eJ < _bound(c["J"]), k
        n_cases += 1
    assert n_cases == 8
    print(f"golden: measured maximum relative to max(1, max|expected|): {worst:.3e} (bound 1e-6)")


def _backend_preint_device(hostlib, variant, imus, states, points):
    n = len(imus)
    offsets = np.cumsum([0] + [len(m) for m in imus]).astype(np.int32)
    cur = np.zeros((n, 16))
    rh, rd_, Jh, Jd = np.zeros((n, 15)), np.zeros((n, 15)), np.zeros((n, 480)), np.zeros((n, 480))
    Sh, Sd = np.zeros((n, 225)), np.zeros((n, 225))
    okh, okd = np.full(n, -1, np.int32), np.full(n, -1, np.int32)
    err = ErrBuf()
    rc = hostlib.icgh_backend_preint_device(variant, n, ptr(offsets), ptr(f64(np.concatenate(imus))), ptr(f64(np.stack(states))), ptr(f64(pd.PARAMS)),
                                            ptr(f64(np.stack(points))), ptr(cur), ptr(rh), ptr(Jh), ptr(rd_), ptr(Jd), ptr(Sh), ptr(Sd), ptr(okh), ptr(okd),
                                            *err.args)
    assert rc == 0, (rc, err.value)
    return dict(cur=cur, rh=rh, rd=rd_, Jh=Jh, Jd=Jd, Sh=Sh, Sd=Sd, okh=okh, okd=okd)


@pytest.mark.parametrize("variant", [0, 1])
def test_sqrt_information_bit_for_bit_host_against_device(oracle, hostlib, variant):
    """the same Preintegration objects evaluated by PreintegrationFactor::Evaluate and by Preintegration::evaluateBatch"""
    imus, states, pres = _intervals(oracle, variant)
    points = [_eval_point(states[i], pres[i]["cur"]) for i in range(len(LENS))]
    o = _backend_preint_device(hostlib, variant, imus, states, points)
    assert np.all(o["okh"] == 1) and np.all(o["okd"] == 1)
    assert _amax(o["Sh"]) > 1.0
    for i in range(len(LENS)):
        assert np.all(np.isfinite(o["Sh"][i])) == (LENS[i] != 2), i
        assert _same_bits(o["Sd"][i], o["Sh"][i]), i
    worst = 0.0
    for i in range(len(LENS)):
        er, eJ = _err(o["rd"][i], o["rh"][i]), _err(o["Jd"][i], o["Jh"][i])
        worst = max(worst, er / max(1.0, _amax(o["rh"][i])), eJ / max(1.0, _amax(o["Jh"][i])))
        print(f"variant {variant} factor {i}: device vs host |dr| {er:.3e}  |dJ| {eJ:.3e}")
        assert er < _bound(o["rh"][i]), i
        assert eJ < _bound(o["Jh"][i]), i
    print(f"variant {variant}: measured maximum device vs host, relative to max(1, max|expected|): {worst:.3e} (bound 1e-6)")


@pytest.mark.parametrize("variant", [0, 1])
def test_batch_invariance(oracle, ctx, variant):
    """a factor's rows do not depend on the batch around it: alone (n_factors = 1) and inside a shuffled batch of 320"""
    lens = [41, 17, 2, 101, 60, 33, 8, 25]
    _, states, base = _intervals(oracle, variant, lens=lens, seed0=40)
    rng = np.random.RandomState(7)
    pres, points = [], []
    for k in range(320):
        b = k % len(lens)
        pres.append(base[b])
        points.append(_eval_point(states[b], base[b]["cur"], perturb=rng.normal(0, 1, 6) * np.array([0.02, 0.02, 0.02, 0.002, 0.002, 0.002])))
    order = rng.permutation(320)
    pres, points = [pres[k] for k in order], [points[k] for k in order]
    params = [pd.PARAMS] * 320
    res, J, S, status = _evaluate(ctx, variant, pres, params, points)
    assert np.all(status == 0)
    for k in range(320):
        r1, J1, S1, st1 = _evaluate(ctx, variant, [pres[k]], [pd.PARAMS], [points[k]])
        assert st1[0] == 0
        assert res[k].tobytes() == r1[0].tobytes() and J[k].tobytes() == J1[0].tobytes() and S[k].tobytes() == S1[0].tobytes(), k


@pytest.mark.parametrize("variant", [0, 1])
def test_status_singular_covariance(oracle, ctx, hostlib, variant):
    """an interval of one IMU sample has a zero covariance: status 1, zero rows, neighbours untouched; evaluateBatch's ok agrees with
    PreintegrationFactor::Evaluate"""
    lens = [41, 17, 1, 60, 25]
    imus, states, pres = _intervals(oracle, variant, lens=lens, seed0=60)
    assert not np.any(pres[2]["cov"])
    points = [_eval_point(states[i], pres[i]["cur"]) for i in range(len(lens))]
    params = [pd.PARAMS] * len(lens)
    res, J, S, status = _evaluate(ctx, variant, pres, params, points)
    assert list(status) == [0, 0, 1, 0, 0]
    assert not np.any(res[2]) and not np.any(J[2]) and not np.any(S[2])
    keep = [0, 1, 3, 4]
    res2, J2, S2, status2 = _evaluate(ctx, variant, [pres[k] for k in keep], [pd.PARAMS] * 4, [points[k] for k in keep])
    assert np.all(status2 == 0)
    for a, k in enumerate(keep):
        assert np.abs(res[k]).max() > 0
        assert res[k].tobytes() == res2[a].tobytes() and J[k].tobytes() == J2[a].tobytes() and S[k].tobytes() == S2[a].tobytes(), k
    o = _backend_preint_device(hostlib, variant, imus, states, points)
    assert list(o["okh"]) == [1, 1, 0, 1, 1]
    assert list(o["okd"]) == list(o["okh"])
    assert not np.any(o["rd"][2]) and not np.any(o["Jd"][2]) and not np.any(o["Sd"][2])


@pytest.mark.parametrize("variant", [0, 1])
def test_residual_only_returns_the_same_residual_bytes(oracle, ctx, variant):
    _, states, pres = _intervals(oracle, variant)
    points = [_eval_point(states[i], pres[i]["cur"]) for i in range(len(LENS))]
    params = [pd.PARAMS] * len(LENS)
    res, J, _, _ = _evaluate(ctx, variant, pres, params, points)
    res2, J2, _, st2 = _evaluate(ctx, variant, pres, params, points, want_jac=False)
    assert J2 is None and np.all(st2 == 0)
    assert _amax(res) > 0 and res.tobytes() == res2.tobytes()


def test_argument_errors_launch_nothing(oracle, ctx):
    _, states, pres = _intervals(oracle, 1)
    points = np.stack([_eval_point(states[i], pres[i]["cur"]) for i in range(len(LENS))])
    delta, jac, cov, dt, env, pn_off, pn = _pack(pres, [pd.PARAMS] * len(LENS))
    ctx.prof_enable(True)
    ctx.preint_evaluate_batch(1, delta, jac, cov, dt, env, points, pn_off, pn)
    count = ctx.prof()["preint_eval"][0]
    assert count >= 1
    n = len(LENS)
    res, J, S, status = np.zeros((n, 15)), np.zeros((n, 480)), np.zeros((n, 225)), np.zeros(n, np.int32)
    lib = ctx.lib

    def call(variant=1, n_factors=n, delta=delta, cov=cov, points=points, pn_off=pn_off, pn=pn, res=res, status=status):
        return lib.icg_preint_evaluate_batch(ctx.h, variant, n_factors, ptr(delta), ptr(jac), ptr(cov), ptr(dt), ptr(env), ptr(pn_off), ptr(pn), ptr(points),
                                             ptr(res), ptr(J), ptr(S), ptr(status))

    bad_off = pn_off.copy()
    bad_off[2] = bad_off[1] - 1
    cases = dict(zero_factors=dict(n_factors=0), negative_factors=dict(n_factors=-3), variant_2=dict(variant=2), variant_minus_1=dict(variant=-1),
                 null_delta=dict(delta=None), null_cov=dict(cov=None), null_points=dict(points=None), null_residuals=dict(res=None),
                 null_status=dict(status=None), earth_without_offsets=dict(pn_off=None), earth_without_pn=dict(pn=None),
                 offsets_not_monotone=dict(pn_off=bad_off))
    for name, kw in cases.items():
        rc = call(**kw)
        assert rc != 0, name
        assert len(lib.icg_last_error(ctx.h)) > 0, name
        assert ctx.prof()["preint_eval"][0] == count, name
    assert not np.any(res) and not np.any(J) and not np.any(S)
    assert call() == 0  # the context is still usable
    assert ctx.prof()["preint_eval"][0] == count + 1
    ctx.prof_enable(False)


def test_c4_shape_3840_earth_factors_in_one_call(oracle, ctx):
    """bench.py's C4 preintegration shape (256 streams x 15 intervals x 40 samples, Earth variant): integrated in one launch, evaluated in one
    call, checked against the oracle on a seeded sample of 64 factors — on the device's own integration results, i.e. identical inputs"""
    n_streams, n_int = 256, 15
    n = n_streams * n_int
    base = [pd.make_interval(41, seed=s) for s in range(n_int)]
    imu = np.concatenate(base * n_streams)
    off = (np.arange(n + 1) * 41).astype(np.int32)
    s0 = np.tile(pd.state(), (n, 1))
    cur, delta, jac, cov, dt, pn = ctx.preint_batch(1, off, imu, s0, pd.PARAMS)
    rng = np.random.RandomState(11)
    points = np.stack([_eval_point(s0[k], cur[k], perturb=rng.normal(0, 1, 6) * np.array([0.02, 0.02, 0.02, 0.002, 0.002, 0.002])) for k in range(n)])
    pn_rows = pn.reshape(n, 41, 4)[:, :40].reshape(-1, 4)  # row 40 of every interval is unused
    pn_off = (np.arange(n + 1) * 40).astype(np.int32)
    env = np.tile(pd.PARAMS[5:9], (n, 1))
    res, J, S, status = ctx.preint_evaluate_batch(1, delta, jac, cov, dt, env, points, pn_off, pn_rows)
    assert np.all(status == 0)
    worst = 0.0
    for k in np.random.RandomState(12).choice(n, 64, replace=False):
        pre = dict(delta=delta[k], jac=jac[k], cov=cov[k], dt=float(dt[k]), pn=pn_rows[40 * k:40 * k + 40])
        r_exp, J_exp = _oracle_eval(oracle, 1, pre, pd.PARAMS, points[k])
        er, eJ = np.abs(res[k] - r_exp).max(), np.abs(J[k] - J_exp).max()
        worst = max(worst, er / max(1.0, np.abs(r_exp).max()), eJ / max(1.0, np.abs(J_exp).max()))
        assert er < _bound(r_exp), k
        assert eJ < _bound(J_exp), k
    print(f"C4 shape: measured maximum vs oracle over 64 of {n} factors, relative to max(1, max|expected|): {worst:.3e} (bound 1e-6)")
