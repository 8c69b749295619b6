"""GPU: the resident marginalization priors as the host-part kernel reads them.  icg_marg_prior_evaluate_resident returns the squared norms
icg_marg_prior_evaluate returns, bit for bit; icg_reproj_host_parts_build_prior (residuals and Jacobians taken from the resident set on the
device) gives the part, s and diag icg_reproj_host_parts_build gives on the same context when it is fed the residuals and the gathered
local columns that icg_marg_prior_evaluate ships; the argument errors launch nothing."""
import numpy as np
import pytest

import marg_factor_data as mf
from ctypes_util import bits, ptr
from host_part_family_utils import _columns, _gathered, _partition

pytestmark = pytest.mark.gpu

FILL = 7.0
P = 260


def _priors():
    """r = 1 (a scalar block), 6 (one pose), 61, 142 and 257 (past one workgroup's rows); blocks listed out of column order, the last with two
    columns no block covers"""
    rng = np.random.RandomState(5)
    s61, s142, s255 = [7, 9] * 4 + [1], mf.C2_SIZES, [7, 9] * 17
    priors = [mf.make_prior([1], 41), mf.make_prior([7], 42), mf.make_prior(s61, 43, order=rng.permutation(len(s61))),
              mf.make_prior(s142, 44, order=rng.permutation(len(s142))), mf.make_prior(s255, 45, order=rng.permutation(len(s255)), gap_after=3, gap=2)]
    assert [p["r"] for p in priors] == [1, 6, 61, 142, 257]
    return priors


def _points(priors, seed):
    pts = [mf.make_x(p, seed + k, negate=(0, 2)) for k, p in enumerate(priors)]
    assert mf.dq_w(priors[1], pts[1])[0] < 0  # the single pose takes the dq.w < 0 branch
    return pts


@pytest.fixture()
def ctx():
    import icgvins
    c = icgvins.Context(64, 64, n_slots=1, max_batch=1, max_points=64)
    yield c
    c.close()


def test_resident_squared_norms_are_the_evaluate_entry_s_bits(ctx):
    priors = _priors()
    ctx.marg_prior_set(*mf.set_args(priors))
    for seed in (100, 200):
        x = np.concatenate(_points(priors, seed))
        res, _, _, sq = ctx.marg_prior_evaluate(x, want_sq_norm=True)
        got = ctx.marg_prior_evaluate_resident(x)
        assert np.array_equal(bits(got), bits(sq)), (seed, got, sq)
        for w, e in enumerate(mf.split(priors, res, "r")):
            assert bits(np.array([mf.sequential_sq_norm(e)]))[0] == bits(got)[w], w


def _same(got, ref, rebuilt):
    (gs, gd, gp), (rs, rdg, rp) = got, ref
    for w in rebuilt:
        assert np.array_equal(bits(gp[w]), bits(rp[w])), ("part", w)
        assert np.array_equal(bits(gs[w]), bits(rs[w])) and np.array_equal(bits(gd[w]), bits(rdg[w])), ("s / diag", w)


def test_build_from_resident_priors_equals_build_from_shipped_ones(ctx):
    priors = _priors()
    ctx.marg_prior_set(*mf.set_args(priors))
    rng = np.random.RandomState(9)
    mk = lambda nr, cols, scale=1.0: (rng.normal(0, scale, (nr, len(cols))), rng.normal(0, 1.0, nr), np.asarray(cols, np.int32))
    # where each prior sits: (partition window, prior of the set, dropped blocks, its columns in the window's system)
    pc = {p: _columns(priors[p], drop) for p, drop in ((3, ()), (2, (1,)), (1, ()), (4, ()), (0, ()))}
    assert len(pc[2][0]) == 61 - 9 and len(pc[4][0]) == 255  # a dropped (constant) block, and only the covered columns: nf < r
    cols = {3: 15 + rng.permutation(142), 2: rng.permutation(70)[:52], 1: np.arange(6), 4: rng.permutation(260)[:255], 0: np.array([4])}
    Pw = [160, 70, 31, 12, 260, 9]
    layout = [[mk(15, range(0, 30)), ("prior", 3), mk(6, range(0, 6), 30.0)],  # the prior between two ordinary blocks
              [("prior", 2), mk(9, range(6, 15), 10.0)],
              [mk(15, range(15, 30)), mk(6, range(0, 6), 30.0)],  # no prior
              [mk(3, [1, 5, 2]), ("prior", 1)],  # not rebuilt: its prior block only places the others' columns
              [("prior", 4)],
              [mk(2, [0, 3]), ("prior", 0)]]
    rebuild = [1, 1, 1, 0, 1, 1]
    rebuilt = [w for w in range(6) if rebuild[w]]
    _partition(ctx, 6)

    def resident(how, ordinary_r):
        wins = [[("prior", b[1], pc[b[1]][0], cols[b[1]], how) if isinstance(b[0], str) else (b[0], ordinary_r(b), b[2], False) for b in win] for win in layout]
        s, dg = np.full((6, P), FILL), np.full((6, P), FILL)
        return ctx.reproj_host_parts_build_prior(P, Pw, wins, rebuild=rebuild, host_s=s, host_diag=dg)

    def shipped(res, jac, ordinary_r):
        res_w, jac_w = mf.split(priors, res, "r"), mf.split(priors, jac, "jac")
        wins = [[(_gathered(priors[b[1]], jac_w[b[1]], pc[b[1]][1]), res_w[b[1]], cols[b[1]], False) if isinstance(b[0], str) else (b[0], ordinary_r(b), b[2], False)
                 for b in win] for win in layout]
        s, dg = np.full((6, P), FILL), np.full((6, P), FILL)
        return ctx.reproj_host_parts_build(P, Pw, wins, rebuild=rebuild, host_s=s, host_diag=dg)

    x1, x2 = (np.concatenate(_points(priors, seed)) for seed in (100, 200))
    ref_in = [ctx.marg_prior_evaluate(x, want_jac=True)[:2] for x in (x1, x2)]
    r1 = lambda b: b[1]
    r2 = lambda b: b[1] * 2.0 - 1.0  # (other residuals for the ordinary blocks at the second point)
    # first rebuild: the Jacobians are gathered on the device; second, at another point: they are kept
    ctx.marg_prior_evaluate_resident(x1)
    got1 = resident("gather", r1)
    ctx.marg_prior_evaluate_resident(x2)
    got2 = resident("keep", r2)
    ref1 = shipped(*ref_in[0], r1)
    ref2 = shipped(*ref_in[1], r2)
    _same(got1, ref1, rebuilt)
    _same(got2, ref2, rebuilt)
    assert any(not np.array_equal(bits(got1[2][w]), bits(got2[2][w])) or not np.array_equal(bits(got1[0][w]), bits(got2[0][w])) for w in (0, 1, 4))
    for got in (got1, got2):  # the window that is not rebuilt: nothing of it was written
        assert got[2][3] is None and (got[0][3] == FILL).all() and (got[1][3] == FILL).all()
    # run after run, and a gather over a kept layout: the same bits
    ctx.marg_prior_evaluate_resident(x1)
    _same(resident("gather", r1), ref1, rebuilt)


def test_argument_errors_launch_nothing(ctx):
    import icgvins
    priors = _priors()[:3]
    rng = np.random.RandomState(11)
    pc1, pc2 = _columns(priors[1])[0], _columns(priors[2])[0]
    good = dict(P=70, Pw=np.array([12, 70], np.int32), rebuild=np.ones(2, np.uint8), blk_off=np.array([0, 2, 3], np.int32), nr=np.array([3, 6, 61], np.int32),
                nf=np.array([3, 6, 61], np.int32), cols=np.concatenate([[1, 5, 2], np.arange(6, 12), np.arange(61)]).astype(np.int32),
                jac_off=np.array([0, -2, -2], np.int64), J=rng.normal(0, 1, 9), r=np.full(70, np.nan), prior_of=np.array([-1, 1, 2], np.int32),
                prior_cols=np.concatenate([pc1, pc2]).astype(np.int32))
    good["r"][:3] = rng.normal(0, 1, 3)
    s, dg, part = np.full((2, 70), FILL), np.full((2, 70), FILL), np.full(12 * 13 // 2 + 70 * 71 // 2, FILL)

    def call(**over):
        a = dict(good, s=s, dg=dg, part=part)
        a.update(over)
        rc = ctx.reproj_host_parts_build_prior_raw(a["P"], a["Pw"], a["rebuild"], a["blk_off"], a["nr"], a["nf"], a["cols"], a["jac_off"], a["J"], a["r"], a["s"], a["dg"],
                                                   a["part"], a["prior_of"], a["prior_cols"])
        return rc, ctx.lib.icg_last_error(ctx.h).decode()

    untouched = lambda: (s == FILL).all() and (dg == FILL).all() and (part == FILL).all()
    changed = lambda key, idx, val: {key: np.concatenate([good[key][:idx], [val], good[key][idx + 1:]]).astype(good[key].dtype)}
    _partition(ctx, 2)
    ctx.prof_enable(True)
    sq = np.zeros(3)
    x = np.concatenate(_points(priors, 100))

    def nothing_launched(before):
        """no scope of the context's profiler (marg_set, marg_eval, host_part_prior, host_part, ...) has moved since `before`"""
        ctx.sync()
        return ctx.prof() == before

    # no set is resident
    before = ctx.prof()
    assert ctx.lib.icg_marg_prior_evaluate_resident(ctx.h, ptr(x), ptr(sq)) == -1 and b"no prior set" in ctx.lib.icg_last_error(ctx.h)
    rc, msg = call()
    assert rc == -1 and "window 0, block 1: no prior set is resident and evaluated" in msg and untouched(), (rc, msg)
    assert nothing_launched(before) and not sq.any()
    ctx.marg_prior_set(*mf.set_args(priors))
    ctx.sync()
    before = ctx.prof()
    # a set, but not evaluated since it was set; NULL arguments of the resident evaluation
    rc, msg = call()
    assert rc == -1 and "window 0, block 1: no prior set is resident and evaluated" in msg and untouched(), (rc, msg)
    assert ctx.lib.icg_marg_prior_evaluate_resident(ctx.h, None, ptr(sq)) == -1 and b"NULL" in ctx.lib.icg_last_error(ctx.h)
    assert ctx.lib.icg_marg_prior_evaluate_resident(ctx.h, ptr(x), None) == -1 and b"NULL" in ctx.lib.icg_last_error(ctx.h)
    assert ctx.lib.icg_marg_prior_evaluate_resident(None, ptr(x), ptr(sq)) == -1
    assert nothing_launched(before) and not sq.any()
    ctx.marg_prior_evaluate_resident(x)
    ctx.sync()
    before = ctx.prof()
    assert before["marg_eval"][0] == 1
    cases = [(changed("prior_of", 1, 3), "window 0, block 1: prior 3 outside the resident set of 3"), (changed("prior_of", 2, 1), "window 1, block 0: 61 residuals, prior 1 has 6"),
             (changed("nr", 1, 5), "window 0, block 1: 5 residuals, prior 1 has 6"), (changed("prior_cols", 2, 6), "window 0, block 1: prior column 6 outside the prior (6)"),
             (changed("prior_cols", 6, -1), "window 1, block 0: prior column -1 outside the prior (61)"), (changed("jac_off", 0, -2), "window 0, block 0: jac_off = -2"),
             (dict(prior_of=None, prior_cols=None), "window 0, block 1: jac_off = -2"), (dict(prior_cols=None), "window 0, block 1: a prior block without prior_cols"),
             (changed("jac_off", 2, -1), "window 1, block 0: no kept Jacobian")]
    for over, text in cases:
        rc, msg = call(**over)
        assert rc == -1 and text in msg and untouched(), (over.keys(), rc, msg)
        assert nothing_launched(before), (over.keys(), before, ctx.prof())
    # a new set invalidates the kept residuals
    ctx.marg_prior_set(*mf.set_args(priors))
    ctx.sync()
    before = ctx.prof()
    rc, msg = call()
    assert rc == -1 and "no prior set is resident and evaluated" in msg and untouched(), (rc, msg)
    assert nothing_launched(before)
    # and the next valid sequence gives the bits of the shipped form
    ctx.marg_prior_evaluate_resident(x)
    rc, msg = call()
    assert rc == 0, msg
    res, jac, _, _ = ctx.marg_prior_evaluate(x, want_jac=True)
    res_w, jac_w = mf.split(priors, res, "r"), mf.split(priors, jac, "jac")
    wins = [[(good["J"].reshape(3, 3), good["r"][:3], [1, 5, 2], False), (_gathered(priors[1], jac_w[1], _columns(priors[1])[1]), res_w[1], np.arange(6, 12), False)],
            [(_gathered(priors[2], jac_w[2], _columns(priors[2])[1]), res_w[2], np.arange(61), False)]]
    rs, rdg, rp = ctx.reproj_host_parts_build(70, good["Pw"], wins)
    assert np.array_equal(bits(part), bits(np.concatenate(rp))) and np.array_equal(bits(s), bits(rs)) and np.array_equal(bits(dg), bits(rdg))
    after = ctx.prof()
    assert after["host_part_prior"][0] == 1 and after["host_part"][0] == 2 and after["marg_eval"][0] == before.get("marg_eval", (0, 0))[0] + 2
