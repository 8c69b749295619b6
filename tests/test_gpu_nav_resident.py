"""GPU parity, bit for bit: the resident navigation factors (icg_nav_set + icg_nav_evaluate_resident + icg_nav_correct_resident +
icg_nav_fetch_resident) against the product classes of the host layer (host/nav_factors.h through icgh_backend_nav_eval) on the same
members.  There is no trigonometry and no sqrt on the device (the corrector's three scalars arrive from the host), so residuals, Jacobians,
squared norms and corrected results are held to their bit patterns; kinds 0..3 also meet the reference golden within the 1e-12 the host is
held to.  The member sets: one of each kind alone, 0 3 1 2 5 4 0 (the non-unit GNSS quaternion first, a GNSS member with a zero lever arm
last: the rotation columns of its Jacobian are signed zeros), and that set tiled to 130 members (past 64 and past 128)."""
import ctypes as C

import numpy as np
import pytest

import nav_product_data as nd
import nav_utils as nu
from ctypes_util import bits, ptr, same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def ctx():
    import icgvins
    c = icgvins.Context(64, 64, n_slots=1, max_batch=1, max_points=64)
    yield c
    c.close()


@pytest.fixture(scope="module")
def hostlib():
    import harness
    return C.CDLL(harness.HOST_LIB)


def _sets():
    one = nd.one_of_each()
    s = {f"kind_{c[0]}": [c] for c in one}
    s["mixed"] = nd.mixed_set()
    s["tiled_130"] = nd.tiled(nd.mixed_set(), 130)
    return s


SETS = _sets()


def _run(ctx, cases, want_jac=True):
    kind, aux_off, aux, points, point_off = nd.pack(cases)
    ctx.nav_set(kind, aux_off, aux)
    sq = ctx.nav_evaluate_resident(points, point_off, want_jac=want_jac)
    r, J = ctx.nav_fetch_resident(want_jac=want_jac)
    return r, J, sq


@pytest.mark.parametrize("order", ["forward", "reversed"])
@pytest.mark.parametrize("name", list(SETS))
def test_resident_evaluation_has_the_hosts_bits(ctx, hostlib, name, order):
    cases = SETS[name] if order == "forward" else SETS[name][::-1]
    h = nd.host_eval(hostlib, cases)
    r, J, sq = _run(ctx, cases)
    assert np.array_equal(bits(r), bits(h["r"])) and np.array_equal(bits(J), bits(h["J"])) and np.array_equal(bits(sq), bits(h["sq"]))
    assert np.abs(r).max() > 0 and np.abs(J).max() > 0 and np.all(sq > 0)
    # residual only: the same bits, and the Jacobians of the evaluation before are no longer offered
    r0, J0, sq0 = _run(ctx, cases, want_jac=False)
    assert J0 is None and np.array_equal(bits(r0), bits(r)) and np.array_equal(bits(sq0), bits(sq))
    res, Jb = np.zeros_like(r), np.zeros_like(J)
    assert ctx.lib.icg_nav_fetch_resident(ctx.h, ptr(res), ptr(Jb)) == -1
    assert b"want_jac = 0" in ctx.lib.icg_last_error(ctx.h) and not Jb.any()


def test_a_member_does_not_depend_on_the_set_around_it(ctx, hostlib):
    cases = SETS["tiled_130"]
    r, J, sq = _run(ctx, cases)
    ro, jo = nd.offsets([c[0] for c in cases])
    for i, c in enumerate(cases[:7]):
        r1, J1, sq1 = _run(ctx, [c])
        for k in (i, 126 + i if 126 + i < 130 else 63 + i):
            assert cases[k] is c
            assert np.array_equal(bits(r1), bits(r[ro[k]:ro[k + 1]])) and np.array_equal(bits(J1), bits(J[jo[k]:jo[k + 1]])) and bits(sq1)[0] == bits(sq)[k]


def test_signed_zeros_and_the_seventh_pose_columns(ctx, hostlib):
    cases = SETS["mixed"]
    h = nd.host_eval(hostlib, cases)
    r, J, _ = _run(ctx, cases)
    for i, (kind, aux, _) in enumerate(cases):
        nr, nc = nd.SHAPES[kind]
        Jm = J[h["j_off"][i]:h["j_off"][i + 1]].reshape(nr, nc)
        if nc == 7:
            assert np.array_equal(bits(Jm[:, 6]), np.zeros(nr, np.uint64)), i  # +0.0
    # the zero-lever GNSS member: its rotation columns are zeros, some of them negative, exactly where the host's are
    Jz = J[h["j_off"][6]:h["j_off"][7]].reshape(3, 7)
    assert not Jz[:, 3:6].any() and np.signbit(Jz[:, 3:6]).any()
    assert np.array_equal(bits(Jz), bits(h["J"][h["j_off"][6]:h["j_off"][7]]))


def test_the_golden_is_met_on_the_device(ctx):
    cases = nu.factor_cases()
    exp = np.load(nu.GOLDEN)
    r, J, _ = _run(ctx, cases)
    ro, jo = nd.offsets([c[0] for c in cases])
    for i, (kind, _, _) in enumerate(cases):
        for g, e in ((r[ro[i]:ro[i + 1]], exp[f"factor_{i}_r"]), (J[jo[i]:jo[i + 1]], exp[f"factor_{i}_J"].ravel())):
            err = float(np.abs(g - e).max()) / max(1.0, float(np.abs(e).max()))
            assert err < 1e-12, (i, kind, err)


def _corrected(ctx, cases, robust, corr):
    kind, aux_off, aux, points, point_off = nd.pack(cases)
    ctx.nav_set(kind, aux_off, aux)
    ctx.nav_evaluate_resident(points, point_off)
    ctx.nav_correct_resident(robust, corr)
    return ctx.nav_fetch_resident()


@pytest.mark.parametrize("name", ["mixed", "tiled_130"])
def test_huber_correction_inside_and_outside(ctx, hostlib, name):
    cases = SETS[name]
    n = len(cases)
    huber = np.where(np.arange(n) % 3 == 0, 1.0, np.where(np.arange(n) % 3 == 1, 1e6, 0.0))
    huber[6] = 1.0  # the zero-lever GNSS member, outside: j - 0 * r * rtj decides the sign of its zeros
    h = nd.host_eval(hostlib, cases, huber=huber)
    marked = huber != 0
    assert (h["corr"][marked, 0] == 1.0).any() and (h["corr"][marked, 0] < 1.0).any() and h["corr"][6, 0] < 1.0
    r, J = _corrected(ctx, cases, marked, h["corr"])
    assert np.array_equal(bits(r), bits(h["r_corr"])) and np.array_equal(bits(J), bits(h["J_corr"]))
    assert not np.array_equal(bits(J), bits(h["J"]))
    for i in np.flatnonzero(~marked):  # unmarked members keep their bits
        rs, js = slice(h["r_off"][i], h["r_off"][i + 1]), slice(h["j_off"][i], h["j_off"][i + 1])
        assert np.array_equal(bits(r[rs]), bits(h["r"][rs])) and np.array_equal(bits(J[js]), bits(h["J"][js]))
    Jz = J[h["j_off"][6]:h["j_off"][7]].reshape(3, 7)
    assert not Jz[:, 3:].any() and np.array_equal(bits(Jz), bits(h["J_corr"][h["j_off"][6]:h["j_off"][7]]))


def test_correction_with_alpha_equals_the_host_twin(ctx, hostlib):
    cases = SETS["tiled_130"]
    n = len(cases)
    rng = np.random.RandomState(3)
    corr = np.stack([rng.uniform(0.3, 1.0, n), rng.uniform(-0.2, 0.2, n) / 50.0, rng.uniform(0.3, 1.2, n)], axis=1)
    mark = (np.arange(n) % 5 != 2)
    h = nd.host_eval(hostlib, cases, huber=mark.astype(np.float64), corr_in=corr)
    r, J = _corrected(ctx, cases, mark, corr)
    assert np.array_equal(bits(r), bits(h["r_corr"])) and np.array_equal(bits(J), bits(h["J_corr"]))
    assert not np.array_equal(bits(J), bits(h["J"]))


def test_a_second_correction_is_refused_and_an_evaluation_allows_one_again(ctx, hostlib):
    cases = SETS["mixed"]
    n = len(cases)
    huber = np.full(n, 1.0)
    h = nd.host_eval(hostlib, cases, huber=huber)
    kind, aux_off, aux, points, point_off = nd.pack(cases)
    rob, corr = np.ones(n, np.uint8), np.ascontiguousarray(h["corr"])
    lib = ctx.lib
    ctx.nav_set(kind, aux_off, aux)
    assert lib.icg_nav_correct_resident(ctx.h, ptr(rob), ptr(corr)) == -1 and b"nothing was evaluated" in lib.icg_last_error(ctx.h)
    ctx.nav_evaluate_resident(points, point_off, want_jac=False)
    assert lib.icg_nav_correct_resident(ctx.h, ptr(rob), ptr(corr)) == -1 and b"want_jac = 0" in lib.icg_last_error(ctx.h)
    ctx.nav_evaluate_resident(points, point_off)
    ctx.prof_enable(True)
    assert lib.icg_nav_correct_resident(ctx.h, ptr(rob), ptr(corr)) == 0
    ctx.sync()
    before = ctx.prof()
    assert before["nav_correct"][0] == 1
    assert lib.icg_nav_correct_resident(ctx.h, ptr(rob), ptr(corr)) == -1 and b"corrected already" in lib.icg_last_error(ctx.h)
    assert lib.icg_nav_correct_resident(ctx.h, None, ptr(corr)) == -1 and lib.icg_nav_correct_resident(ctx.h, ptr(rob), None) == -1
    ctx.sync()
    assert ctx.prof() == before
    ctx.prof_enable(False)
    r, J = ctx.nav_fetch_resident()  # corrected once, not twice
    assert np.array_equal(bits(r), bits(h["r_corr"])) and np.array_equal(bits(J), bits(h["J_corr"]))
    ctx.nav_evaluate_resident(points, point_off)
    r, J = ctx.nav_fetch_resident()
    assert np.array_equal(bits(r), bits(h["r"])) and np.array_equal(bits(J), bits(h["J"]))
    ctx.nav_correct_resident(rob, corr)


def test_a_second_evaluation_replaces_the_first(ctx, hostlib):
    a = SETS["mixed"]
    b = [(k, aux, x + 0.01 * (1 + np.arange(len(x)))) for k, aux, x in a]
    ha, hb = nd.host_eval(hostlib, a), nd.host_eval(hostlib, b)
    kind, aux_off, aux, pa, off_a = nd.pack(a)
    _, _, _, pb, off_b = nd.pack(b)
    ctx.nav_set(kind, aux_off, aux)
    ctx.nav_evaluate_resident(pa, off_a)
    ra, Ja = ctx.nav_fetch_resident()
    sqb = ctx.nav_evaluate_resident(pb, off_b)
    rb, Jb = ctx.nav_fetch_resident()
    assert np.array_equal(bits(ra), bits(ha["r"])) and np.array_equal(bits(rb), bits(hb["r"])) and np.array_equal(bits(Jb), bits(hb["J"]))
    assert np.array_equal(bits(sqb), bits(hb["sq"])) and not np.array_equal(bits(ra), bits(rb))


def test_the_other_resident_sets_keep_their_bits(ctx, hostlib):
    """a prior set, a 15-state set and an odometer set resident in the same context: setting, evaluating, correcting and failing to set the
    nav set leaves their kept results and their later evaluations at their own bits, and the nav set's survive theirs"""
    import marg_factor_data as mf
    import preint_odo_data as od
    import preint_odo_split_data as sdo
    import preint_split_data as sd15
    priors = [mf.make_prior([7], 42), mf.make_prior([7, 9] * 4 + [1], 43)]
    xp = np.concatenate([mf.make_x(p, 100 + k) for k, p in enumerate(priors)])
    ctx.marg_prior_set(*mf.set_args(priors))
    sq_prior = ctx.marg_prior_evaluate_resident(xp)
    imus, states = sd15.intervals([41, 17])
    cur = sd15.current_states(hostlib, 1, imus, states)
    h15 = sd15.eval_split(hostlib, 1, imus, states, [sd15.eval_point("perturbed", states[i], cur[i]) for i in range(2)])
    ctx.preint_set(h15["variant"], h15["delta"], h15["jac"], h15["sqrt_info"], h15["dt"], h15["env"], h15["q_nn"], h15["pn_off"], h15["pn"])
    ctx.preint_evaluate_resident(h15["points"], h15["q_corr"])
    par25 = od.params25(iewn=od.TILTED)
    imu9, s17 = od._imu9(17, 50), od.state17(p=(0, 1, 0), v=(2, 0, 0))
    c, d, jac, cov, dt, pn = ctx.preint_odo_batch(od.ODO, np.array([0, 17], np.int32), imu9, s17[None], par25)
    res = [dict(variant=od.ODO, cur=c[0], delta=d[0], jac=jac[0], cov=cov[0], dt=dt[0], pn=np.zeros((0, 4)), iewn=par25[6:9], s0=s17)]
    ho = sdo.eval_split(hostlib, res, [sdo.eval_point("perturbed", d[0], c[0], s17)], par25=par25)
    ctx.preint_odo_set(ho["variant"], ho["delta"], ho["jac"], ho["sqrt_info"], ho["dt"], ho["env"], ho["q_nn"], np.zeros(2, np.int32), None)
    ctx.preint_odo_evaluate_resident(ho["points"], ho["q_corr"])

    cases = SETS["tiled_130"]
    hn = nd.host_eval(hostlib, cases, huber=np.full(len(cases), 1.0))
    r, J = _corrected(ctx, cases, np.ones(len(cases), np.uint8), hn["corr"])
    assert np.array_equal(bits(r), bits(hn["r_corr"])) and np.array_equal(bits(J), bits(hn["J_corr"]))
    r15, J15 = ctx.preint_fetch_resident()
    ro, Jo = ctx.preint_odo_fetch_resident()
    assert same_bits(r15, h15["r_eval"]) and same_bits(J15, h15["J_eval"]) and same_bits(ro, ho["r_eval"]) and same_bits(Jo, ho["J_eval"])
    assert ctx.lib.icg_nav_set(ctx.h, 0, None, None, None) == -1  # no nav set any more; the others are as they were
    assert np.array_equal(bits(ctx.marg_prior_evaluate_resident(xp)), bits(sq_prior))
    ctx.preint_evaluate_resident(h15["points"], h15["q_corr"])
    ctx.preint_odo_evaluate_resident(ho["points"], ho["q_corr"])
    r15, J15 = ctx.preint_fetch_resident()
    ro, Jo = ctx.preint_odo_fetch_resident()
    assert same_bits(r15, h15["r_eval"]) and same_bits(J15, h15["J_eval"]) and same_bits(ro, ho["r_eval"]) and same_bits(Jo, ho["J_eval"])
    # the other way round: the nav set's kept results survive the other sets' set and evaluate
    r, J, _ = _run(ctx, cases)
    ctx.marg_prior_set(*mf.set_args(priors))
    ctx.marg_prior_evaluate_resident(xp)
    ctx.preint_set(h15["variant"], h15["delta"], h15["jac"], h15["sqrt_info"], h15["dt"], h15["env"], h15["q_nn"], h15["pn_off"], h15["pn"])
    ctx.preint_evaluate_resident(h15["points"], h15["q_corr"])
    ctx.preint_odo_set(ho["variant"], ho["delta"], ho["jac"], ho["sqrt_info"], ho["dt"], ho["env"], ho["q_nn"], np.zeros(2, np.int32), None)
    ctx.preint_odo_evaluate_resident(ho["points"], ho["q_corr"])
    r2, J2 = ctx.nav_fetch_resident()
    assert np.array_equal(bits(r2), bits(r)) and np.array_equal(bits(J2), bits(J)) and np.array_equal(bits(r), bits(hn["r"]))


def test_argument_errors_launch_nothing(ctx):
    lib = ctx.lib
    cases = SETS["mixed"]
    kind, aux_off, aux, points, point_off = nd.pack(cases)
    n = len(kind)
    ro, jo = nd.offsets(kind)
    sq, res, J = np.zeros(n), np.zeros(ro[-1]), np.zeros(jo[-1])
    ctx.prof_enable(True)

    def set_(n=n, kind=kind, aux_off=aux_off, aux=aux):
        return lib.icg_nav_set(ctx.h, n, ptr(kind), ptr(aux_off), ptr(aux))

    def eval_(points=points, point_off=point_off, want_jac=1, sq=sq):
        return lib.icg_nav_evaluate_resident(ctx.h, ptr(points), ptr(point_off), want_jac, ptr(sq))

    def fetch(res=res, J=J):
        return lib.icg_nav_fetch_resident(ctx.h, ptr(res), ptr(J))

    def nothing_launched(before):
        ctx.sync()
        return ctx.prof() == before

    assert set_() == 0 and eval_() == 0
    ctx.sync()
    before = ctx.prof()
    assert before["nav_set"][0] >= 1 and before["nav_eval"][0] >= 1
    sq[:] = 0
    bad_kind, neg_kind, bad_mono, bad_first, short = kind.copy(), kind.copy(), aux_off.copy(), aux_off.copy(), aux_off.copy()
    bad_kind[3], neg_kind[5] = 6, -1
    bad_mono[3] = bad_mono[2] - 1
    bad_first[0] = -1
    short[1:] -= 1  # the GNSS member 0 owns 8 constants
    table = [(dict(n=0), -1, "n = 0"), (dict(n=-2), -1, "n = -2"), (dict(n=65536), -5, "at most 65535"), (dict(kind=None), -1, "NULL"),
             (dict(aux_off=None), -1, "NULL"), (dict(aux=None), -1, "NULL"), (dict(kind=bad_kind), -1, "member 3: kind 6"),
             (dict(kind=neg_kind), -1, "member 5: kind -1"), (dict(aux_off=bad_mono), -1, "member 2: aux_off not monotone"),
             (dict(aux_off=bad_first), -1, "aux_off[0] = -1"), (dict(aux_off=short), -1, "member 0: kind 0 reads 9 constants, the member owns 8")]
    for over, code, text in table:
        assert set_() == 0  # a set is resident ...
        ctx.sync()
        before = ctx.prof()
        rc = set_(**over)
        msg = lib.icg_last_error(ctx.h).decode()
        assert rc == code and text in msg and msg.startswith("icg_nav_set:"), (over.keys(), rc, msg)
        # ... and after the failed call none is: evaluation, correction and fetch refuse, and nothing ran
        assert eval_() == -1 and lib.icg_last_error(ctx.h).decode().startswith("icg_nav_evaluate_resident: no nav set is resident")
        assert lib.icg_nav_correct_resident(ctx.h, ptr(np.ones(n, np.uint8)), ptr(np.ones((n, 3)))) == -1
        assert lib.icg_last_error(ctx.h).decode().startswith("icg_nav_correct_resident: no nav set is resident")
        assert fetch() == -1 and lib.icg_last_error(ctx.h).decode().startswith("icg_nav_fetch_resident: no nav set is resident")
        assert nothing_launched(before), (over.keys(), before, ctx.prof())
    assert not sq.any() and not res.any() and not J.any()
    assert set_() == 0
    ctx.sync()
    before = ctx.prof()
    assert fetch() == -1 and "nothing was evaluated" in lib.icg_last_error(ctx.h).decode()
    neg_off = point_off.copy()
    neg_off[4] = -3
    for over, text in ((dict(points=None), "NULL argument"), (dict(point_off=None), "NULL argument"), (dict(sq=None), "NULL argument"),
                       (dict(point_off=neg_off), "member 4: point_off = -3")):
        assert eval_(**over) == -1 and "icg_nav_evaluate_resident: " + text in lib.icg_last_error(ctx.h).decode(), over.keys()
    assert lib.icg_nav_evaluate_resident(None, ptr(points), ptr(point_off), 1, ptr(sq)) == -1
    assert nothing_launched(before) and not sq.any()
    assert eval_(want_jac=0) == 0
    assert fetch(res=None) == -1 and "NULL residuals" in lib.icg_last_error(ctx.h).decode()
    assert fetch() == -1 and "want_jac = 0" in lib.icg_last_error(ctx.h).decode() and not J.any()
    assert fetch(J=None) == 0 and res.any()
    assert eval_() == 0 and fetch() == 0 and J.any()  # the context is still usable
    ctx.prof_enable(False)
