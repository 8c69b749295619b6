"""GPU parity, bit for bit: the resident preintegration evaluation (icg_preint_set + icg_preint_evaluate_resident +
icg_preint_fetch_resident) against the host layer's own Preintegration::evaluate on the same integration results.  The device is fed the
host's values (icgh_backend_preint_eval_split): square-root information, the Earth-rate quaternion with the set, the correction quaternion
with every point — what is left on the device is + - * / in the host's order, so residuals, the four Jacobian blocks and the squared norm
are held to their bit patterns.  No tolerance.  (An entry that is NaN on the host — the 2-sample interval, whose information matrix is not
positive definite — must be NaN on the device: the sign and payload of a NaN are not part of IEEE arithmetic's results.)

The mixed set is N E E N E with 0, 1 and 40 rows of pn among the Earth factors.  The factor with no row is an interval of one IMU sample: its
covariance is zero, the host's evaluate() refuses it (zero rows here) and its square-root information is all zeros, so the device's sums of
+-0 from +0.0 are the same zeros."""
import ctypes as C

import numpy as np
import pytest

import preint_split_data as sd
from ctypes_util import bits, ptr, same_bits

pytestmark = pytest.mark.gpu

MIXED = [(0, 41), (1, 1), (1, 2), (0, 17), (1, 41)]  # (variant, IMU samples)


@pytest.fixture(scope="module")
def ctx():
    import icgvins
    c = icgvins.Context(640, 480, n_slots=1, max_batch=1, max_points=64)
    yield c
    c.close()


@pytest.fixture(scope="module")
def host():
    """the mixed set on the host at each kind of evaluation point: {kind: dict of arrays, one row per factor of MIXED}"""
    import harness
    lib = C.CDLL(harness.HOST_LIB)
    imus, states = sd.intervals([n for _, n in MIXED])
    idx = {v: [i for i, (vv, _) in enumerate(MIXED) if vv == v] for v in (0, 1)}
    cur = [None] * len(MIXED)
    for v in (0, 1):
        for i, c in zip(idx[v], sd.current_states(lib, v, [imus[i] for i in idx[v]], [states[i] for i in idx[v]])):
            cur[i] = c
    out = {}
    for kind in sd.POINT_KINDS:
        parts = {}
        for v in (0, 1):
            pts = [sd.eval_point(kind, states[i], cur[i]) for i in idx[v]]
            parts[v] = sd.eval_split(lib, v, [imus[i] for i in idx[v]], [states[i] for i in idx[v]], pts)
        m = {}
        for key in ("r_eval", "J_eval", "q_corr", "q_nn", "sqrt_info", "delta", "jac", "dt", "env", "points", "variant", "ok"):
            rows = [None] * len(MIXED)
            for v in (0, 1):
                for a, i in enumerate(idx[v]):
                    rows[i] = parts[v][key][a]
            m[key] = np.stack(rows)
        m["pn_rows"] = [None] * len(MIXED)
        for v in (0, 1):
            for a, i in enumerate(idx[v]):
                m["pn_rows"][i] = parts[v]["pn"][parts[v]["pn_off"][a]:parts[v]["pn_off"][a + 1]]
        out[kind] = m
    assert [len(r) for r in out["perturbed"]["pn_rows"]] == [40, 0, 1, 16, 40]
    assert list(out["perturbed"]["ok"]) == [1, 0, 1, 1, 1]
    return out


def _take(m, order):
    """the factors `order` of a host dict as the arguments of preint_set and of an evaluation"""
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
        for k in range(15):
            s = s + r[f, k] * r[f, k]
        out[f] = s
    return out


def _run(ctx, m, order, want_jac=True):
    set_args, pts, qc = _take(m, order)
    ctx.preint_set(*set_args)
    sq = ctx.preint_evaluate_resident(pts, qc, want_jac=want_jac)
    r, J = ctx.preint_fetch_resident(want_jac=want_jac)
    return r, J, sq


SETS = {"one_normal": [0], "one_earth": [4], "mixed": [0, 1, 2, 3, 4], "tiled_130": [0, 1, 2, 3, 4] * 26}


@pytest.mark.parametrize("kind", sd.POINT_KINDS)
@pytest.mark.parametrize("name", list(SETS))
def test_resident_evaluation_has_the_hosts_bits(ctx, host, name, kind):
    m, order = host[kind], SETS[name]
    with np.errstate(invalid="ignore"):
        r, J, sq = _run(ctx, m, order)
        assert same_bits(r, m["r_eval"][order])
        assert same_bits(J, m["J_eval"][order])
        assert same_bits(sq, _sq_norm(m["r_eval"][order]))
        fin = np.isfinite(m["r_eval"][order]).all(axis=1) & (m["ok"][order] == 1)
        assert fin.any() and np.abs(J[fin]).max() > 1.0 and np.all(sq[fin] > 0)
        # residual only: the same residual and squared-norm bits, and the Jacobians of the evaluation before are no longer offered
        r0, J0, sq0 = _run(ctx, m, order, want_jac=False)
        assert J0 is None and same_bits(r0, r) and same_bits(sq0, sq)
        res = np.zeros((len(order), 15))
        Jb = np.zeros((len(order), 480))
        assert ctx.lib.icg_preint_fetch_resident(ctx.h, res.ctypes.data_as(C.c_void_p), Jb.ctypes.data_as(C.c_void_p)) == -1
        assert b"want_jac = 0" in ctx.lib.icg_last_error(ctx.h) and not Jb.any()


def test_the_seventh_pose_columns_are_positive_zero(ctx, host):
    r, J, _ = _run(ctx, host["perturbed"], [0, 4])
    for f in range(2):
        for base in (0, 240):
            blk = J[f, base:base + 105].reshape(15, 7)
            assert np.array_equal(bits(blk[:, 6]), np.zeros(15, np.uint64)) and np.abs(blk[:, :6]).max() > 0


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
        ctx.preint_set(*set_args)
        ctx.preint_evaluate_resident(pts_a, qc_a)
        ra, Ja = ctx.preint_fetch_resident()
        sq_b = ctx.preint_evaluate_resident(pts_b, qc_b)
        rb, Jb = ctx.preint_fetch_resident()
        assert same_bits(ra, a["r_eval"][order]) and same_bits(rb, b["r_eval"][order]) and same_bits(Jb, b["J_eval"][order])
        assert not same_bits(ra, rb) and same_bits(sq_b, _sq_norm(b["r_eval"][order]))


def test_the_given_quaternions_are_used(ctx, host):
    """the identity in place of q_corr / q_nn changes the result of the factors that have a bias step / are Earth factors"""
    m = host["large_bias_step"]
    set_args, pts, qc = _take(m, [0, 4])
    ident = np.tile([0.0, 0.0, 0.0, 1.0], (2, 1))
    ctx.preint_set(*set_args)
    ctx.preint_evaluate_resident(pts, ident)
    r, _ = ctx.preint_fetch_resident()
    assert not same_bits(r[0], m["r_eval"][0]) and not same_bits(r[1], m["r_eval"][4])
    ctx.preint_set(*(set_args[:6] + (ident,) + set_args[7:]))
    ctx.preint_evaluate_resident(pts, qc)
    r, _ = ctx.preint_fetch_resident()
    assert same_bits(r[0], m["r_eval"][0]) and not same_bits(r[1], m["r_eval"][4])  # (q_nn is not read for a Normal factor)


def test_argument_errors_launch_nothing(ctx, host):
    import icgvins
    lib = ctx.lib
    m = host["perturbed"]
    order = SETS["mixed"]
    (variant, delta, jac, S, dt, env, qnn, pn_off, pn), pts, qc = _take(m, order)
    variant, pn_off = np.ascontiguousarray(variant, np.int32), np.ascontiguousarray(pn_off, np.int32)
    delta, jac, S, dt, env, qnn, pn, pts, qc = [np.ascontiguousarray(a, np.float64) for a in (delta, jac, S, dt, env, qnn, pn, pts, qc)]
    n = len(order)
    sq, res, J = np.zeros(n), np.zeros((n, 15)), np.zeros((n, 480))
    ctx.prof_enable(True)

    def set_(n_factors=n, variant=variant, delta=delta, jac=jac, S=S, dt=dt, env=env, qnn=qnn, pn_off=pn_off, pn=pn):
        return lib.icg_preint_set(ctx.h, n_factors, ptr(variant), ptr(delta), ptr(jac), ptr(S), ptr(dt), ptr(env), ptr(qnn), ptr(pn_off), ptr(pn))

    def eval_(pts=pts, qc=qc, want_jac=1, sq=sq):
        return lib.icg_preint_evaluate_resident(ctx.h, ptr(pts), ptr(qc), want_jac, ptr(sq))

    def fetch(res=res, J=J):
        return lib.icg_preint_fetch_resident(ctx.h, ptr(res), ptr(J))

    def nothing_launched(before):
        ctx.sync()
        return ctx.prof() == before

    assert set_() == 0 and eval_() == 0
    ctx.sync()
    before = ctx.prof()
    assert before["preint_set"][0] >= 1 and before["preint_eval_given"][0] >= 1
    sq[:] = 0
    bad_variant, bad_mono, bad_first = variant.copy(), pn_off.copy(), pn_off.copy()
    bad_variant[3] = 2
    bad_mono[3] = bad_mono[2] - 1
    bad_first[0] = -1
    cases = [(dict(n_factors=0), -1, "n_factors = 0"), (dict(n_factors=-2), -1, "n_factors = -2"), (dict(n_factors=65535 * 16 + 1), -5, "at most 1048560"),
             (dict(variant=None), -1, "NULL"), (dict(delta=None), -1, "NULL"), (dict(jac=None), -1, "NULL"), (dict(S=None), -1, "NULL"), (dict(dt=None), -1, "NULL"),
             (dict(env=None), -1, "NULL"), (dict(qnn=None), -1, "NULL"), (dict(variant=bad_variant), -1, "factor 3: variant 2"),
             (dict(pn_off=bad_mono), -1, "factor 2: pn_offsets not monotone"), (dict(pn_off=bad_first), -1, "pn_offsets[0] = -1"),
             (dict(pn_off=None), -1, "an Earth factor needs pn_offsets"), (dict(pn=None), -1, "NULL pn")]
    for over, code, text in cases:
        assert set_() == 0  # a set is resident ...
        ctx.sync()
        before = ctx.prof()
        rc = set_(**over)
        msg = lib.icg_last_error(ctx.h).decode()
        assert rc == code and text in msg and msg.startswith("icg_preint_set:"), (over.keys(), rc, msg)
        # ... and after the failed call none is: the evaluation and the fetch refuse, and nothing ran
        assert eval_() == -1 and "no preintegration set is resident" in lib.icg_last_error(ctx.h).decode()
        assert fetch() == -1 and "no preintegration set is resident" in lib.icg_last_error(ctx.h).decode()
        assert nothing_launched(before), (over.keys(), before, ctx.prof())
    assert not sq.any() and not res.any() and not J.any()
    # a set, nothing evaluated yet; NULL arguments of the evaluation and the fetch
    assert set_() == 0
    ctx.sync()
    before = ctx.prof()
    assert fetch() == -1 and "nothing was evaluated" in lib.icg_last_error(ctx.h).decode()
    for over in (dict(pts=None), dict(qc=None), dict(sq=None)):
        assert eval_(**over) == -1 and "NULL argument" in lib.icg_last_error(ctx.h).decode(), over.keys()
    assert nothing_launched(before) and not sq.any()
    assert eval_(want_jac=0) == 0
    assert fetch(res=None) == -1 and "NULL residuals" in lib.icg_last_error(ctx.h).decode()
    assert fetch() == -1 and "want_jac = 0" in lib.icg_last_error(ctx.h).decode() and not J.any()
    assert fetch(J=None) == 0 and res.any()
    # a set without an Earth factor takes NULL pn_offsets / pn; the context is still usable
    assert set_(n_factors=1, pn_off=None, pn=None) == 0
    assert eval_() == 0 and fetch() == 0
    with np.errstate(invalid="ignore"):
        assert same_bits(res[0], m["r_eval"][0]) and same_bits(J[0], m["J_eval"][0])
    ctx.prof_enable(False)
