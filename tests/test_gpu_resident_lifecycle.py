"""GPU: the lifecycle every resident factor set follows, one sequence over the preintegration, odometer preintegration and navigation
families, each step through the C entries: evaluate and fetch refuse before any set ("no ... set is resident"); a set alone leaves nothing
to fetch ("nothing was evaluated"); an evaluation without Jacobians offers residuals only ("kept no Jacobians (want_jac = 0)"); a larger
second set replaces every buffer and its results are invalid until it is evaluated; a failing set leaves no set; a smaller third set reuses
the buffers.  What a fetch returns is the host layer's evaluation of the same members, bit for bit.  The prior family has no fetch: its
resident evaluation is held to icg_marg_prior_evaluate's squared norms.

The sets: 2 members (preintegration: one plain factor and one Earth variant with a two-row pn; navigation: kinds 0 and 5, the narrowest
and the widest), then 3, then 1.  Every refusal is an argument check that returns before any launch."""
import ctypes as C

import numpy as np
import pytest

import marg_factor_data as mf
import nav_product_data as nd
import preint_odo_data as od
import preint_odo_split_data as sdo
import preint_split_data as sd15
from ctypes_util import bits, f64, i32, ptr, same_bits

pytestmark = pytest.mark.gpu


@pytest.fixture()
def ctx():
    import icgvins
    c = icgvins.Context(64, 64, n_slots=1, max_batch=1, max_points=64)
    yield c
    c.close()


@pytest.fixture(scope="module")
def hostlib():
    import harness
    return C.CDLL(harness.HOST_LIB)


class _Preint:
    """the 15- and the 19-state family over one dict of host arrays, a row per factor: plain, Earth variant (3 samples: two rows of pn), plain"""

    def __init__(self, ctx, stem, what, N, point, m):
        self.ctx, self.lib, self.stem, self.what, self.N, self.NJ, self.m = ctx, ctx.lib, stem, what, N, N * point, m
        assert len(m["pn_rows"][1]) == 2 and m["variant"][1] == m["variant"][0] + 1
        self.entry = {k: getattr(ctx.lib, f"{stem}_{k}") for k in ("set", "evaluate_resident", "fetch_resident")}

    def set(self, members):
        if not members:
            return self.entry["set"](self.ctx.h, 0, *[None] * 9)
        m, g = self.m, lambda k: f64(self.m[k][members])
        rows = [m["pn_rows"][i] for i in members]
        pn_off = i32(np.cumsum([0] + [len(r) for r in rows]))
        pn = f64(np.concatenate(rows + [np.zeros((1, 4))]))
        return self.entry["set"](self.ctx.h, len(members), ptr(i32(m["variant"][members])), ptr(g("delta")), ptr(g("jac")), ptr(g("sqrt_info")), ptr(g("dt")),
                                 ptr(g("env")), ptr(g("q_nn")), ptr(pn_off), ptr(pn))

    def evaluate(self, members, want_jac):
        sq = np.zeros(3)
        return self.entry["evaluate_resident"](self.ctx.h, ptr(f64(self.m["points"][members])), ptr(f64(self.m["q_corr"][members])), want_jac, ptr(sq))

    def fetch(self, members, want_jac):
        res, J = np.zeros((3, self.N)), np.zeros((3, self.NJ))
        rc = self.entry["fetch_resident"](self.ctx.h, ptr(res), ptr(J) if want_jac else None)
        return rc, res[:len(members)], J[:len(members)]

    def host(self, members):
        return self.m["r_eval"][members], self.m["J_eval"][members]


def _preint(ctx, hostlib):
    lens, variants = [17, 3, 9], [0, 1, 0]
    imus, states = sd15.intervals(lens)
    rows = [None] * 3
    for v in (0, 1):
        idx = [i for i in range(3) if variants[i] == v]
        im, st = [imus[i] for i in idx], [states[i] for i in idx]
        cur = sd15.current_states(hostlib, v, im, st)
        h = sd15.eval_split(hostlib, v, im, st, [sd15.eval_point("perturbed", s, c) for s, c in zip(st, cur)])
        for a, i in enumerate(idx):
            rows[i] = {k: h[k][a] for k in ("variant", "delta", "jac", "sqrt_info", "dt", "env", "q_nn", "points", "q_corr", "r_eval", "J_eval")}
            rows[i]["pn_rows"] = h["pn"][h["pn_off"][a]:h["pn_off"][a + 1]]
    m = {k: np.stack([r[k] for r in rows]) for k in rows[0] if k != "pn_rows"}
    m["pn_rows"] = [r["pn_rows"] for r in rows]
    return _Preint(ctx, "icg_preint", "preintegration", 15, 32, m)


def _preint_odo(ctx, hostlib):
    lens, variants = [17, 3, 9], [od.ODO, od.EARTH_ODO, od.ODO]
    imus = [od._imu9(n, 50 + i) for i, n in enumerate(lens)]
    states = [od.state17(p=(i, 1, 0), v=(2, 0.1 * i, 0)) for i in range(3)]
    par25 = od.params25(iewn=od.TILTED)
    results = [None] * 3
    for v in od.VARIANTS:
        idx = [i for i in range(3) if variants[i] == v]
        off = np.cumsum([0] + [len(imus[i]) for i in idx]).astype(np.int32)
        cur, delta, jac, cov, dt, pn = ctx.preint_odo_batch(v, off, np.concatenate([imus[i] for i in idx]), np.stack([states[i] for i in idx]), par25)
        for a, i in enumerate(idx):
            results[i] = dict(variant=v, cur=cur[a], delta=delta[a], jac=jac[a], cov=cov[a], dt=dt[a], pn=pn[off[a]:off[a + 1] - 1], iewn=par25[6:9], s0=states[i])
    m = sdo.eval_split(hostlib, results, [sdo.eval_point("perturbed", r["delta"], r["cur"], r["s0"]) for r in results], par25=par25)
    return _Preint(ctx, "icg_preint_odo", "odometer preintegration", 19, 34, m)


class _Nav:
    """kind 0, kind 5, kind 0 again (the zero-lever GNSS member)"""
    stem, what = "icg_nav", "nav"

    def __init__(self, ctx, hostlib):
        by = nd.one_of_each()
        self.ctx, self.lib, self.hostlib, self.cases = ctx, ctx.lib, hostlib, [by[0], by[5], nd.zero_lever_gnss()]
        assert [c[0] for c in self.cases] == [0, 5, 0]

    def set(self, members):
        if not members:
            return self.lib.icg_nav_set(self.ctx.h, 0, None, None, None)
        kind, aux_off, aux, _, _ = nd.pack([self.cases[i] for i in members])
        return self.lib.icg_nav_set(self.ctx.h, len(members), ptr(kind), ptr(aux_off), ptr(aux))

    def evaluate(self, members, want_jac):
        _, _, _, points, point_off = nd.pack([self.cases[i] for i in members])
        return self.lib.icg_nav_evaluate_resident(self.ctx.h, ptr(points), ptr(point_off), want_jac, ptr(np.zeros(3)))

    def fetch(self, members, want_jac):
        ro, jo = nd.offsets([self.cases[i][0] for i in members])
        res, J = np.zeros(16), np.zeros(142)  # (3 + 10 + 3 residuals, 21 + 100 + 21 Jacobian elements)
        rc = self.lib.icg_nav_fetch_resident(self.ctx.h, ptr(res), ptr(J) if want_jac else None)
        return rc, res[:ro[-1]], J[:jo[-1]]

    def host(self, members, huber=None):
        h = nd.host_eval(self.hostlib, [self.cases[i] for i in members], huber=huber)
        return (h["r"], h["J"]) if huber is None else h

    def correct(self, members, corr):
        return self.lib.icg_nav_correct_resident(self.ctx.h, ptr(np.ones(len(members), np.uint8)), ptr(f64(corr)))


FAMILIES = {"preint": _preint, "preint_odo": _preint_odo, "nav": _Nav}


@pytest.mark.parametrize("family", list(FAMILIES))
def test_set_evaluate_fetch_lifecycle(ctx, hostlib, family):
    F = FAMILIES[family](ctx, hostlib)
    err = lambda: ctx.lib.icg_last_error(ctx.h).decode()
    no_set = lambda entry: f"{F.stem}_{entry}: no {F.what} set is resident ({F.stem}_set first)"
    not_evaluated = lambda entry: f"{F.stem}_{entry}: nothing was evaluated since the set was made resident"
    no_jacobians = lambda entry: f"{F.stem}_{entry}: the last evaluation kept no Jacobians (want_jac = 0)"

    def fetched_equals_host(members, want_jac):
        rc, r, J = F.fetch(members, want_jac)
        assert rc == 0, err()
        hr, hJ = F.host(members)
        with np.errstate(invalid="ignore"):
            assert same_bits(r, hr) and np.abs(np.nan_to_num(r)).max() > 0
            if want_jac:
                assert same_bits(J, hJ) and np.abs(np.nan_to_num(J)).max() > 0
            else:
                assert not J.any()

    def refused(rc_and_more, text):
        rc = rc_and_more[0] if isinstance(rc_and_more, tuple) else rc_and_more
        assert rc == -1 and err() == text, (rc, err())

    two, three, one = [0, 1], [0, 1, 2], [0]
    # 1. before any set
    refused(F.evaluate(two, 1), no_set("evaluate_resident"))
    refused(F.fetch(two, True), no_set("fetch_resident"))
    # 2. a set, not evaluated
    assert F.set(two) == 0, err()
    refused(F.fetch(two, True), not_evaluated("fetch_resident"))
    refused(F.fetch(two, False), not_evaluated("fetch_resident"))
    # 3. evaluated without Jacobians
    assert F.evaluate(two, 0) == 0, err()
    fetched_equals_host(two, False)
    rc, _, J = F.fetch(two, True)
    refused(rc, no_jacobians("fetch_resident"))
    assert not J.any()
    if family == "nav":
        corr = F.host(two, huber=np.ones(2))["corr"]
        refused(F.correct(two, corr), no_jacobians("correct_resident"))
    # 4. evaluated with Jacobians
    assert F.evaluate(two, 1) == 0, err()
    fetched_equals_host(two, False)
    fetched_equals_host(two, True)
    if family == "nav":
        h = F.host(two, huber=np.ones(2))
        assert F.correct(two, h["corr"]) == 0, err()
        refused(F.correct(two, h["corr"]), "icg_nav_correct_resident: the last evaluation was corrected already")
        rc, r, J = F.fetch(two, True)  # corrected once
        assert rc == 0 and same_bits(r, h["r_corr"]) and same_bits(J, h["J_corr"])
    # 5. a larger set: every buffer is replaced
    assert F.set(three) == 0, err()
    refused(F.fetch(three, True), not_evaluated("fetch_resident"))
    refused(F.fetch(three, False), not_evaluated("fetch_resident"))
    assert F.evaluate(three, 1) == 0, err()
    fetched_equals_host(three, True)
    # 6. a failing set leaves none
    assert F.set([]) == -1 and err().startswith(f"{F.stem}_set: n")
    refused(F.evaluate(three, 1), no_set("evaluate_resident"))
    refused(F.fetch(three, True), no_set("fetch_resident"))
    # 7. a smaller set: nothing regrows
    assert F.set(one) == 0, err()
    refused(F.fetch(one, False), not_evaluated("fetch_resident"))
    assert F.evaluate(one, 1) == 0, err()
    fetched_equals_host(one, True)
    fetched_equals_host(one, False)


def _priors():
    """r = 6 and 7, then a third of r = 15"""
    priors = [mf.make_prior([7], 42), mf.make_prior([7, 1], 43), mf.make_prior([9, 7], 44)]
    assert [p["r"] for p in priors] == [6, 7, 15]
    return priors


@pytest.mark.parametrize("case", ["before_any_set", "after_a_failing_set", "two_windows_then_three"])
def test_prior_set_lifecycle(ctx, case):
    lib, priors = ctx.lib, _priors()
    x = np.concatenate([mf.make_x(p, 100 + k) for k, p in enumerate(priors)])
    sq = np.zeros(3)
    no_set = "icg_marg_prior_evaluate_resident: no prior set is resident (icg_marg_prior_set first)"
    if case == "before_any_set":
        assert lib.icg_marg_prior_evaluate_resident(ctx.h, ptr(x), ptr(sq)) == -1 and lib.icg_last_error(ctx.h).decode() == no_set
    elif case == "after_a_failing_set":
        ctx.marg_prior_set(*mf.set_args(priors[:2]))
        ctx.marg_prior_evaluate_resident(x[:sum(len(p["x0"]) for p in priors[:2])])
        assert lib.icg_marg_prior_set(ctx.h, 0, None, None, None, None, None, None, None) == -1
        assert lib.icg_marg_prior_evaluate_resident(ctx.h, ptr(x), ptr(sq)) == -1 and lib.icg_last_error(ctx.h).decode() == no_set
    else:
        for n in (2, 3):
            xn = x[:sum(len(p["x0"]) for p in priors[:n])]
            ctx.marg_prior_set(*mf.set_args(priors[:n]))
            got = ctx.marg_prior_evaluate_resident(xn)
            _, _, _, exp = ctx.marg_prior_evaluate(xn, want_sq_norm=True)
            assert len(got) == n and np.array_equal(bits(got), bits(exp)) and np.all(got > 0), (n, got, exp)
    assert case == "two_windows_then_three" or not sq.any()
