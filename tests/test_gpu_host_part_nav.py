"""GPU: the resident navigation factors as the host-part kernel reads them.  icg_reproj_host_parts_build_nav (residuals and Jacobians taken
from the resident nav set on the device, row stride = the member's block width) gives the part, s and diag icg_reproj_host_parts_build gives
on the same context when it is fed the fetched residuals and the numpy-gathered columns of the fetched Jacobians: a pose prior and a GNSS
member on one pose block; a set member that is no block of any window (its parameter block is constant: a cost, no host block); a window with
members of all four families; a member between an ordinary block and a resident prior; an empty window; a window that is not rebuilt; member
order that is not block order; a later rebuild with -1; robustified members gathered after their correction, and refused before it.  The
four older entries are the new one with NULL for its arguments and give the bits they gave; the refusals name window and block, launch
nothing and touch no output.  Bit patterns throughout."""
import ctypes as C

import numpy as np
import pytest

import marg_factor_data as mf
import nav_product_data as nd
import host_part_family_utils as hp
from host_part_family_utils import ALL15, ALL34, CODE, FILL, _partition, _columns
from ctypes_util import bits

pytestmark = pytest.mark.gpu

P = 64
# the nav set: nd.mixed_set() = kinds 0 3 1 2 5 4 0, then a second pose prior whose block is constant in every window (member 7: in no layout)
KINDS = [0, 3, 1, 2, 5, 4, 0, 2]
POSE_COLS, MIX9, MIX10 = np.arange(6, dtype=np.int32), np.arange(9, dtype=np.int32), np.arange(10, dtype=np.int32)


@pytest.fixture()
def ctx():
    import icgvins
    c = icgvins.Context(64, 64, n_slots=1, max_batch=1, max_points=64)
    yield c
    c.close()


def _nav_cases(shift=0.0):
    cases = nd.mixed_set() + [nd.one_of_each()[2]]
    assert [c[0] for c in cases] == KINDS
    return [(k, aux, x + shift * (1 + np.arange(len(x)))) for k, aux, x in cases]


def _nav_set(ctx):
    kind, aux_off, aux, points, point_off = nd.pack(_nav_cases())
    ctx.nav_set(kind, aux_off, aux)
    return (points, point_off), nd.pack(_nav_cases(0.01))[3:]


def _member(flat_r, flat_J, m):
    ro, jo = nd.offsets(KINDS)
    nr, nc = nd.SHAPES[KINDS[m]]
    return flat_r[ro[m]:ro[m + 1]], flat_J[jo[m]:jo[m + 1]].reshape(nr, nc)


def _arrays(layout, Pw, rebuild):
    return hp.arrays(layout, Pw, rebuild, lambda b: nd.SHAPES[KINDS[b[1]]][0] if b[0] == "nav" else hp.nr_of(b))


def _call(ctx, a, W, **over):
    return hp.call(ctx, a, W, "nav", P=P, **over)


def _layout(rng, prior, how):
    mk = lambda nr, cols, scale=1.0: ("ord", rng.normal(0, scale, (nr, len(cols))), rng.normal(0, 1.0, nr), np.asarray(cols, np.int32))
    pc = _columns(prior)[0]
    layout = [[("nav", 3, POSE_COLS, np.arange(0, 6), how), ("nav", 0, POSE_COLS, np.arange(0, 6), how), ("nav", 1, MIX9, np.arange(6, 15), how)],  # one pose block twice
              [mk(9, range(6, 15), 10.0), ("nav", 6, POSE_COLS, 20 + rng.permutation(6), how), ("prior", 0, pc, np.arange(36, 42), how, prior["r"])],
              [("preint", 2, ALL15, rng.permutation(30), how), ("odo", 2, ALL34, 30 + rng.permutation(32), how), ("nav", 4, MIX10, 20 + rng.permutation(10), how),
               ("prior", 0, pc, np.arange(0, 6), how, prior["r"])],  # all four families
              [],  # rebuilt, no host block
              [("nav", 5, MIX10, np.arange(10), how), mk(3, [1, 5, 2])],  # not rebuilt: its member only places the others' columns
              [("nav", 2, MIX9[3:8], np.array([9, 2, 7, 4, 0], np.int32), how)]]  # some of the member's columns (the others constant or unused)
    return layout, [20, 42, 62, 10, 32, 12], [1, 1, 1, 1, 0, 1]


def _reference(ctx, layout, Pw, rebuild, nav, odo, fifteen, prior, prior_res, prior_jac):
    def member(b):
        r, J = _member(nav[0], nav[1], b[1])
        return J[:, b[2]], r
    return hp.reference(ctx, layout, Pw, rebuild, dict(hp.sources(prior, prior_res, prior_jac, fifteen, odo), nav=member), P=P)


def test_build_from_resident_members_equals_build_from_fetched_ones(ctx):
    pts_o, qcs_o, prior, x = hp.everything_resident(ctx)
    (p1, off1), (p2, off2) = _nav_set(ctx)
    ctx.nav_evaluate_resident(p1, off1)
    _partition(ctx, 6)
    layout, Pw, rebuild = _layout(np.random.RandomState(9), prior, "gather")
    rebuilt = [w for w in range(6) if rebuild[w]]
    keep_layout = [[b if b[0] == "ord" else b[:4] + ("keep",) + b[5:] for b in win] for win in layout]
    fifteen, odo = ctx.preint_fetch_resident(), ctx.preint_odo_fetch_resident()
    nav1 = ctx.nav_fetch_resident()
    a = _arrays(layout, Pw, rebuild)
    assert list(a["nav_of"][a["nav_of"] >= 0]) == [3, 0, 1, 6, 4, 5, 2]  # member order is not block order; member 7 is no block at all
    rc, msg, got1, _ = _call(ctx, a, 6)
    assert rc == 0, msg
    rc, msg, alone, _ = _call(ctx, _arrays(layout, Pw, [1, 0, 0, 0, 0, 0]), 6)  # a window alone: the same bits
    assert rc == 0, msg
    hp.same(alone, got1, [0])
    assert alone[2][1] is None and (alone[0][1:] == FILL).all()
    # second rebuild at point 2, residual only: -1 keeps the Jacobian gathered at point 1
    ctx.nav_evaluate_resident(p2, off2, want_jac=False)
    r2, _ = ctx.nav_fetch_resident(want_jac=False)
    rc, msg, got2, _ = _call(ctx, _arrays(keep_layout, Pw, rebuild), 6)
    assert rc == 0, msg
    res, jac = ctx.marg_prior_evaluate(x, want_jac=True)[:2]
    ref1 = _reference(ctx, layout, Pw, rebuild, nav1, odo, fifteen, prior, res, jac)
    ref2 = _reference(ctx, layout, Pw, rebuild, (r2, nav1[1]), odo, fifteen, prior, res, jac)
    hp.same(got1, ref1, rebuilt)
    hp.same(got2, ref2, rebuilt)
    assert not np.array_equal(bits(nav1[0]), bits(r2))
    for w in (0, 1, 2, 5):
        assert np.array_equal(bits(got1[2][w]), bits(got2[2][w])) and not np.array_equal(bits(got1[0][w]), bits(got2[0][w])), w
        assert got1[2][w].any()
    assert not got1[2][3].any() and not got1[0][3].any()  # the window without host blocks: a zero part
    for got in (got1, got2):  # the window that is not rebuilt: nothing of it was written
        assert got[2][4] is None and (got[0][4] == FILL).all() and (got[1][4] == FILL).all()
    ctx.prof_enable(True)
    ctx.nav_evaluate_resident(p1, off1)
    rc, msg, again, _ = _call(ctx, a, 6)
    assert rc == 0, msg
    hp.same(again, ref1, rebuilt)  # a gather over a kept layout
    ctx.sync()
    prof = ctx.prof()
    assert prof["host_part_prior"][0] == 1 and prof["host_part"][0] == 1  # no new kernel: the two launches of the older entries
    ctx.prof_enable(False)


def test_robustified_members_are_gathered_after_their_correction_only(ctx):
    import harness
    hostlib = C.CDLL(harness.HOST_LIB)
    prior = mf.make_prior([7], 42)
    (p1, off1), _ = _nav_set(ctx)
    _partition(ctx, 2)
    layout = [[("nav", 0, POSE_COLS, np.arange(0, 6), "gather"), ("nav", 3, POSE_COLS, np.arange(0, 6), "gather")], [("nav", 6, POSE_COLS, np.arange(2, 8), "gather")]]
    Pw, rebuild = [8, 8], [1, 1]
    a = _arrays(layout, Pw, rebuild)
    huber = np.array([1.0, 0, 0, 0, 0, 0, 1.0, 0])  # the GNSS members carry the loss; both are outside its kernel
    h = nd.host_eval(hostlib, _nav_cases(), huber=huber)
    assert (h["corr"][[0, 6], 0] < 1.0).all()
    ctx.nav_evaluate_resident(p1, off1)
    plain = ctx.nav_fetch_resident()
    ctx.nav_correct_resident(huber != 0, h["corr"])
    corrected = ctx.nav_fetch_resident()
    assert np.array_equal(bits(corrected[0]), bits(h["r_corr"])) and np.array_equal(bits(corrected[1]), bits(h["J_corr"]))
    rc, msg, got, _ = _call(ctx, a, 2)
    assert rc == 0, msg
    hp.same(got, _reference(ctx, layout, Pw, rebuild, corrected, None, None, prior, None, None), [0, 1])
    uncorrected = _reference(ctx, layout, Pw, rebuild, plain, None, None, prior, None, None)
    assert not np.array_equal(bits(got[2][0]), bits(uncorrected[2][0])) and not np.array_equal(bits(got[0][1]), bits(uncorrected[0][1]))
    # the set now has robustified members: the next evaluation is gathered after its correction only
    ctx.nav_evaluate_resident(p1, off1)
    ctx.prof_enable(True)
    ctx.sync()
    before = ctx.prof()
    rc, msg, (s, dg, _), part = _call(ctx, a, 2)
    assert rc == -1 and "window 0, block 0: the nav set has robustified members and its last evaluation is not corrected" in msg, (rc, msg)
    assert (s == FILL).all() and (dg == FILL).all() and (part == FILL).all()
    ctx.sync()
    assert ctx.prof() == before
    ctx.prof_enable(False)
    ctx.nav_correct_resident(huber != 0, h["corr"])
    rc, msg, again, _ = _call(ctx, a, 2)
    assert rc == 0, msg
    hp.same(again, got, [0, 1])


def test_the_older_entries_are_the_new_one_without_its_arguments(ctx):
    """the odometer test's own input (priors, 15-state and odometer factors, no nav block) through the new entry and through the old one"""
    pts, qcs, prior, x = hp.everything_resident(ctx)
    _partition(ctx, 6)
    layout, Pw, rebuild = hp.layout_odo(np.random.RandomState(9), prior, "gather")
    rebuilt = [w for w in range(6) if rebuild[w]]
    old_args = hp.arrays(layout, Pw, rebuild)
    a = _arrays(layout, Pw, rebuild)
    assert a["nav_cols"] is None and (a["nav_of"] < 0).all()
    for entry in ("odo", "preint", "prior", "plain"):
        keep = {"odo": ("ord", "prior", "preint", "odo"), "preint": ("ord", "prior", "preint"), "prior": ("ord", "prior"), "plain": ("ord",)}[entry]
        sub = [[b for b in win if b[0] in keep] for win in layout]
        rc, msg, old, _ = hp.call(ctx, hp.arrays(sub, Pw, rebuild), 6, entry)
        assert rc == 0, msg
        b = _arrays(sub, Pw, rebuild)
        drop = {f + "_of": None for f in CODE if f not in keep}
        for over in (dict(), dict(nav_of=None), dict(drop, nav_cols=None)):
            rc, msg, new, _ = _call(ctx, b, 6, **over)
            assert rc == 0, msg
            hp.same(new, old, rebuilt)
        assert any(p is not None and p.any() for p in old[2])
    assert old_args["odo_cols"] is not None


def test_argument_errors_name_window_and_block_and_launch_nothing(ctx):
    pts_o, qcs_o, prior, x = hp.everything_resident(ctx)
    (p1, off1), _ = _nav_set(ctx)
    _partition(ctx, 6)
    layout, Pw, rebuild = _layout(np.random.RandomState(9), prior, "gather")
    good = _arrays(layout, Pw, rebuild)
    ctx.prof_enable(True)

    def refused(text, **over):
        ctx.sync()
        before = ctx.prof()
        rc, msg, (s, dg, _), part = _call(ctx, good, 6, **over)
        assert rc == -1 and text in msg and msg.startswith("icg_reproj_host_parts_build"), (text, rc, msg)
        assert (s == FILL).all() and (dg == FILL).all() and (part == FILL).all(), text
        ctx.sync()
        assert ctx.prof() == before, (text, before, ctx.prof())
        return msg

    changed = lambda key, idx, val: {key: np.concatenate([good[key][:idx], [val], good[key][idx + 1:]]).astype(good[key].dtype)}
    # blocks of the call: 0, 1, 2 | 3, 4, 5 | 6, 7, 8, 9 | | 10, 11 | 12.  The nav set is there but nothing was evaluated
    refused("window 0, block 0: no nav set is resident and evaluated with Jacobians")
    ctx.nav_evaluate_resident(p1, off1, want_jac=False)
    refused("window 0, block 0: no nav set is resident and evaluated with Jacobians")
    ctx.nav_evaluate_resident(p1, off1)
    msg = refused("window 0, block 1: member 8 outside the resident nav set of 8", **changed("nav_of", 1, 8))
    assert msg.startswith("icg_reproj_host_parts_build_nav:")
    refused("window 0, block 1: 6 residuals, nav member 0 (kind 0) has 3", **changed("nr", 1, 6))
    refused("window 0, block 2: 3 residuals, nav member 1 (kind 3) has 9", **changed("nr", 2, 3))
    for bad in (6, 7, -1):  # a 7-wide member: the seventh pose column and anything outside the width
        refused(f"window 0, block 0: navigation column {bad} (0 .. 6 without 6)", **changed("nav_cols", 2, bad))
    refused("window 0, block 2: navigation column 9 (0 .. 8)", **changed("nav_cols", 12 + 4, 9))
    refused("window 2, block 2: navigation column 10 (0 .. 9)", **changed("nav_cols", 12 + 9 + 6 + 1, 10))
    refused("window 1, block 2: both a prior (0) and a navigation factor (1)", **changed("nav_of", 5, 1))
    refused("window 2, block 0: both a preintegration factor (2) and a navigation factor (0)", **changed("nav_of", 6, 0))
    refused("window 2, block 1: both an odometer preintegration factor (2) and a navigation factor (0)", **changed("nav_of", 7, 0))
    refused("window 1, block 0: ICG_HP_JAC_FROM_NAV for a block that is no navigation factor", **changed("jac_off", 3, -5))
    refused("window 2, block 1: ICG_HP_JAC_FROM_NAV for a block that is no navigation factor", **changed("jac_off", 7, -5))
    refused("window 0, block 0: ICG_HP_JAC_FROM_PREINT_ODO for a block that is no odometer preintegration factor", **changed("jac_off", 0, -4))
    refused("a navigation block without nav_cols", nav_cols=None)
    msg = refused("window 0, block 0: jac_off = -5", nav_of=None)  # -5 without nav_of: the older entry's own name and its own message
    assert msg.startswith("icg_reproj_host_parts_build_preint_odo:")
    # a new set invalidates what was evaluated; a failed set leaves none; then the good call goes through
    _nav_set(ctx)
    refused("no nav set is resident and evaluated")
    assert ctx.lib.icg_nav_set(ctx.h, 0, None, None, None) == -1
    refused("no nav set is resident and evaluated")
    _nav_set(ctx)
    ctx.nav_evaluate_resident(p1, off1)
    rc, msg, _, _ = _call(ctx, good, 6)
    assert rc == 0, msg
    ctx.prof_enable(False)
