"""GPU parity, bit for bit: the resident odometer preintegration evaluation (icg_preint_odo_set + icg_preint_odo_evaluate_resident +
icg_preint_odo_fetch_resident) against the host layer's own PreintegrationOdo::evaluate on the same integration results (one
icg_preint_odo_batch call per variant).  The device is fed the host's values (icgh_backend_preint_odo_eval_split): square-root information,
the Earth-rate quaternion with the set, the correction quaternion with every point — what is left on the device is + - * / in the host's
order, so residuals, the four Jacobian blocks and the squared norm are held to their bit patterns.  No tolerance.  (An entry that is NaN on
the host — the 2-sample interval, whose information matrix is not positive definite — must be NaN on the device.)

The mixed set is O E E O E with 41, 1, 2, 17, 41 IMU samples: 0, 1 and 40 rows of pn among the EarthOdo factors.  The factor with no row is
an interval of one IMU sample: its covariance is zero, the host's evaluate() refuses it (zero rows here) and its square-root information is
all zeros, so the device's sums of +-0 from +0.0 are the same zeros."""
import ctypes as C

import numpy as np
import pytest

import preint_odo_data as od
import preint_odo_split_data as sd
import preint_split_data as sd15
from ctypes_util import bits, ptr, same_bits

pytestmark = pytest.mark.gpu

MIXED = [(od.ODO, 41), (od.EARTH_ODO, 1), (od.EARTH_ODO, 2), (od.ODO, 17), (od.EARTH_ODO, 41)]  # (variant, IMU samples)


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


@pytest.fixture(scope="module")
def host(ctx, hostlib):
    """the mixed set on the host at each kind of evaluation point: {kind: dict of arrays, one row per factor of MIXED}"""
    imus = [od._imu9(n, 50 + i) for i, (_, n) in enumerate(MIXED)]
    states = [od.state17(p=(i, 1, 0), v=(2, 0.1 * i, 0)) for i in range(len(MIXED))]
    par25 = od.params25(iewn=od.TILTED)
    results = [None] * len(MIXED)
    for v in od.VARIANTS:
        idx = [i for i, (vv, _) in enumerate(MIXED) if vv == v]
        off = np.cumsum([0] + [len(imus[i]) for i in idx]).astype(np.int32)
        cur, delta, jac, cov, dt, pn = ctx.preint_odo_batch(v, off, np.concatenate([imus[i] for i in idx]), np.stack([states[i] for i in idx]), par25)
        for a, i in enumerate(idx):
            results[i] = dict(variant=v, cur=cur[a], delta=delta[a], jac=jac[a], cov=cov[a], dt=dt[a], pn=pn[off[a]:off[a + 1] - 1], iewn=par25[6:9],
                              s0=states[i])
    out = {}
    for kind in sd.POINT_KINDS:
        pts = [sd.eval_point(kind, r["delta"], r["cur"], r["s0"]) for r in results]
        out[kind] = sd.eval_split(hostlib, results, pts, par25=par25)
    assert [len(r) for r in out["perturbed"]["pn_rows"]] == [0, 0, 1, 0, 40]
    assert list(out["perturbed"]["ok"]) == [1, 0, 1, 1, 1]
    assert not out["perturbed"]["sqrt_info"][1].any()
    return out


def _take(m, order):
    """the factors `order` of a host dict as the arguments of preint_odo_set and of an evaluation"""
    order = list(order)
    rows = [m["pn_rows"][i] for i in order]
    pn_off = np.cumsum([0] + [len(r) for r in rows]).astype(np.int32)
    pn = np.concatenate(rows) if pn_off[-1] > 0 else None
    g = lambda k: m[k][order]
    return (g("variant"), g("delta"), g("jac"), g("sqrt_info"), g("dt"), g("env"), g("q_nn"), pn_off, pn), g("points"), g("q_corr")


def _sq_norm(r):
    out = np.zeros(len(r))
    for f in range(len(r)):
        s = np.float64(0.0)
        for k in range(19):
            s = s + r[f, k] * r[f, k]
        out[f] = s
    return out


def _run(ctx, m, order, want_jac=True):
    set_args, pts, qc = _take(m, order)
    ctx.preint_odo_set(*set_args)
    sq = ctx.preint_odo_evaluate_resident(pts, qc, want_jac=want_jac)
    r, J = ctx.preint_odo_fetch_resident(want_jac=want_jac)
    return r, J, sq


SETS = {"one_odo": [0], "one_earth_odo": [4], "mixed": [0, 1, 2, 3, 4], "tiled_130": [0, 1, 2, 3, 4] * 26}


@pytest.mark.parametrize("kind", sd.POINT_KINDS)
@pytest.mark.parametrize("name", list(SETS))
def test_resident_evaluation_has_the_hosts_bits(ctx, host, name, kind):
    m, order = host[kind], SETS[name]
    with np.errstate(invalid="ignore"):
        r, J, sq = _run(ctx, m, order)
        assert same_bits(r, m["r_eval"][order])
        for got, exp in zip(sd.j_blocks(J), sd.j_blocks(m["J_eval"][order])):
            assert same_bits(got, exp)
        assert same_bits(sq, _sq_norm(m["r_eval"][order]))
        fin = np.isfinite(m["r_eval"][order]).all(axis=1) & (m["ok"][order] == 1)
        assert fin.any() and np.abs(J[fin]).max() > 1.0 and np.all(sq[fin] > 0)
        # residual only: the same residual and squared-norm bits, and the Jacobians of the evaluation before are no longer offered
        r0, J0, sq0 = _run(ctx, m, order, want_jac=False)
        assert J0 is None and same_bits(r0, r) and same_bits(sq0, sq)
        res = np.zeros((len(order), 19))
        Jb = np.zeros((len(order), 646))
        assert ctx.lib.icg_preint_odo_fetch_resident(ctx.h, ptr(res), ptr(Jb)) == -1
        assert b"want_jac = 0" in ctx.lib.icg_last_error(ctx.h) and not Jb.any()


def test_the_seventh_pose_columns_are_positive_zero(ctx, host):
    r, J, _ = _run(ctx, host["perturbed"], [0, 4])
    J0, _, J2, _ = sd.j_blocks(J)
    for f in range(2):
        for blk in (J0[f], J2[f]):
            assert np.array_equal(bits(blk[:, 6]), np.zeros(19, np.uint64)) and np.abs(blk[:, :6]).max() > 0


def test_a_factor_does_not_depend_on_the_set_around_it(ctx, host):
    m = host["perturbed"]
    with np.errstate(invalid="ignore"):
        r, J, sq = _run(ctx, m, SETS["tiled_130"])
        rr, Jr, sqr = _run(ctx, m, SETS["tiled_130"][::-1])
        assert same_bits(rr[::-1], r) and same_bits(Jr[::-1], J) and same_bits(sqr[::-1], sq)
        for i in range(5):
            r1, J1, sq1 = _run(ctx, m, [i])
            for k in (i, 125 + i):
                assert same_bits(r1[0], r[k]) and same_bits(J1[0], J[k]) and same_bits(sq1[0], sq[k]), (i, k)


def test_a_second_evaluation_replaces_the_first(ctx, host):
    a, b = host["perturbed"], host["large_bias_step"]
    order = SETS["mixed"]
    with np.errstate(invalid="ignore"):
        set_args, pts_a, qc_a = _take(a, order)
        _, pts_b, qc_b = _take(b, order)
        ctx.preint_odo_set(*set_args)
        ctx.preint_odo_evaluate_resident(pts_a, qc_a)
        ra, Ja = ctx.preint_odo_fetch_resident()
        sq_b = ctx.preint_odo_evaluate_resident(pts_b, qc_b)
        rb, Jb = ctx.preint_odo_fetch_resident()
        assert same_bits(ra, a["r_eval"][order]) and same_bits(rb, b["r_eval"][order]) and same_bits(Jb, b["J_eval"][order])
        assert not same_bits(ra, rb) and same_bits(sq_b, _sq_norm(b["r_eval"][order]))


def test_the_given_quaternions_are_used(ctx, host):
    """the identity in place of q_corr / q_nn changes the result of the factors that have a bias step / are EarthOdo factors"""
    m = host["large_bias_step"]
    set_args, pts, qc = _take(m, [0, 4])
    ident = np.tile([0.0, 0.0, 0.0, 1.0], (2, 1))
    ctx.preint_odo_set(*set_args)
    ctx.preint_odo_evaluate_resident(pts, ident)
    r, _ = ctx.preint_odo_fetch_resident()
    assert not same_bits(r[0], m["r_eval"][0]) and not same_bits(r[1], m["r_eval"][4])
    ctx.preint_odo_set(*(set_args[:6] + (ident,) + set_args[7:]))
    ctx.preint_odo_evaluate_resident(pts, qc)
    r, _ = ctx.preint_odo_fetch_resident()
    assert same_bits(r[0], m["r_eval"][0]) and not same_bits(r[1], m["r_eval"][4])  # (q_nn is not read for an Odo factor)


def test_a_15_state_set_in_the_same_context_is_unaffected(ctx, host, hostlib):
    """both sets resident at once: setting, evaluating and failing to set the odometer set leaves the 15-state set's results and its
    later evaluations at their own bits"""
    imus, states = sd15.intervals([41, 17])
    cur = sd15.current_states(hostlib, 1, imus, states)
    pts15 = [sd15.eval_point("perturbed", states[i], cur[i]) for i in range(2)]
    h = sd15.eval_split(hostlib, 1, imus, states, pts15)
    set15 = (h["variant"], h["delta"], h["jac"], h["sqrt_info"], h["dt"], h["env"], h["q_nn"], h["pn_off"], h["pn"])
    ctx.preint_set(*set15)
    ctx.preint_evaluate_resident(h["points"], h["q_corr"])
    m = host["perturbed"]
    r, J, sq = _run(ctx, m, SETS["mixed"])
    r15, J15 = ctx.preint_fetch_resident()  # kept over the odometer set's set / evaluate / fetch
    assert same_bits(r15, h["r_eval"]) and same_bits(J15, h["J_eval"])
    assert ctx.lib.icg_preint_odo_set(ctx.h, 0, None, None, None, None, None, None, None, None, None) == -1  # no odometer set any more
    sq15 = ctx.preint_evaluate_resident(h["points"], h["q_corr"])
    r15, J15 = ctx.preint_fetch_resident()
    assert same_bits(r15, h["r_eval"]) and same_bits(J15, h["J_eval"]) and np.all(sq15 > 0)
    # and the other way round: a new 15-state set does not disturb the odometer set's kept results
    with np.errstate(invalid="ignore"):
        r, J, sq = _run(ctx, m, SETS["mixed"])
        ctx.preint_set(*set15)
        ctx.preint_evaluate_resident(h["points"], h["q_corr"])
        r2, J2 = ctx.preint_odo_fetch_resident()
        assert same_bits(r2, r) and same_bits(J2, J) and same_bits(r, m["r_eval"])
    assert ctx.lib.icg_preint_set(ctx.h, 1, ptr(np.array([2], np.int32)), ptr(h["delta"]), ptr(h["jac"]), ptr(h["sqrt_info"]), ptr(h["dt"]), ptr(h["env"]),
                                  ptr(h["q_nn"]), None, None) == -1
    assert b"variant 2 is neither 0 (Normal) nor 1 (Earth)" in ctx.lib.icg_last_error(ctx.h)  # icg_preint_set goes on refusing variant 2


def test_argument_errors_launch_nothing(ctx, host):
    lib = ctx.lib
    m = host["perturbed"]
    order = SETS["mixed"]
    (variant, delta, jac, S, dt, env, qnn, pn_off, pn), pts, qc = _take(m, order)
    variant, pn_off = np.ascontiguousarray(variant, np.int32), np.ascontiguousarray(pn_off, np.int32)
    delta, jac, S, dt, env, qnn, pn, pts, qc = [np.ascontiguousarray(a, np.float64) for a in (delta, jac, S, dt, env, qnn, pn, pts, qc)]
    n = len(order)
    sq, res, J = np.zeros(n), np.zeros((n, 19)), np.zeros((n, 646))
    ctx.prof_enable(True)

    def set_(n_factors=n, variant=variant, delta=delta, jac=jac, S=S, dt=dt, env=env, qnn=qnn, pn_off=pn_off, pn=pn):
        return lib.icg_preint_odo_set(ctx.h, n_factors, ptr(variant), ptr(delta), ptr(jac), ptr(S), ptr(dt), ptr(env), ptr(qnn), ptr(pn_off), ptr(pn))

    def eval_(pts=pts, qc=qc, want_jac=1, sq=sq):
        return lib.icg_preint_odo_evaluate_resident(ctx.h, ptr(pts), ptr(qc), want_jac, ptr(sq))

    def fetch(res=res, J=J):
        return lib.icg_preint_odo_fetch_resident(ctx.h, ptr(res), ptr(J))

    def nothing_launched(before):
        ctx.sync()
        return ctx.prof() == before

    assert set_() == 0 and eval_() == 0
    ctx.sync()
    before = ctx.prof()
    assert before["preint_odo_set"][0] >= 1 and before["preint_odo_eval_given"][0] >= 1
    sq[:] = 0
    bad_variant, bad_mono, bad_first = variant.copy(), pn_off.copy(), pn_off.copy()
    bad_variant[3] = 1
    bad_mono[3] = bad_mono[2] - 1
    bad_first[0] = -1
    cases = [(dict(n_factors=0), -1, "n_factors = 0"), (dict(n_factors=-2), -1, "n_factors = -2"), (dict(n_factors=65535 * 16 + 1), -5, "at most 1048560"),
             (dict(variant=None), -1, "NULL"), (dict(delta=None), -1, "NULL"), (dict(jac=None), -1, "NULL"), (dict(S=None), -1, "NULL"), (dict(dt=None), -1, "NULL"),
             (dict(env=None), -1, "NULL"), (dict(qnn=None), -1, "NULL"), (dict(variant=bad_variant), -1, "factor 3: variant 1"),
             (dict(pn_off=bad_mono), -1, "factor 2: pn_offsets not monotone"), (dict(pn_off=bad_first), -1, "pn_offsets[0] = -1"),
             (dict(pn_off=None), -1, "an EarthOdo factor needs pn_offsets"), (dict(pn=None), -1, "NULL pn")]
    for over, code, text in cases:
        assert set_() == 0  # a set is resident ...
        ctx.sync()
        before = ctx.prof()
        rc = set_(**over)
        msg = lib.icg_last_error(ctx.h).decode()
        assert rc == code and text in msg and msg.startswith("icg_preint_odo_set:"), (over.keys(), rc, msg)
        # ... and after the failed call none is: the evaluation and the fetch refuse, and nothing ran
        assert eval_() == -1 and lib.icg_last_error(ctx.h).decode().startswith("icg_preint_odo_evaluate_resident: no odometer preintegration set is resident")
        assert fetch() == -1 and lib.icg_last_error(ctx.h).decode().startswith("icg_preint_odo_fetch_resident: no odometer preintegration set is resident")
        assert nothing_launched(before), (over.keys(), before, ctx.prof())
    assert not sq.any() and not res.any() and not J.any()
    # a set, nothing evaluated yet; NULL arguments of the evaluation and the fetch
    assert set_() == 0
    ctx.sync()
    before = ctx.prof()
    assert fetch() == -1 and "nothing was evaluated" in lib.icg_last_error(ctx.h).decode()
    for over in (dict(pts=None), dict(qc=None), dict(sq=None)):
        assert eval_(**over) == -1 and "icg_preint_odo_evaluate_resident: NULL argument" in lib.icg_last_error(ctx.h).decode(), over.keys()
    assert nothing_launched(before) and not sq.any()
    assert eval_(want_jac=0) == 0
    assert fetch(res=None) == -1 and "NULL residuals" in lib.icg_last_error(ctx.h).decode()
    assert fetch() == -1 and "want_jac = 0" in lib.icg_last_error(ctx.h).decode() and not J.any()
    assert fetch(J=None) == 0 and res.any()
    # a set without an EarthOdo factor takes NULL pn_offsets / pn; the context is still usable
    assert set_(n_factors=1, pn_off=None, pn=None) == 0
    assert eval_() == 0 and fetch() == 0
    with np.errstate(invalid="ignore"):
        assert same_bits(res[0], m["r_eval"][0]) and same_bits(J[0], m["J_eval"][0])
    ctx.prof_enable(False)
