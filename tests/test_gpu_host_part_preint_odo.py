"""GPU: the resident ODOMETER preintegration factors as the host-part kernel reads them.  icg_reproj_host_parts_build_preint_odo (residuals
and Jacobians taken from the resident odometer P2 set on the device, row stride 34) gives the part, s and diag icg_reproj_host_parts_build
gives on the same context when it is fed the fetched residuals and the numpy-gathered columns of the fetched Jacobians; a later rebuild with
-1 keeps the gathered Jacobian; a window may hold a 15-state resident factor, an odometer one and a resident prior at once; the three older
entries are the new one with NULL for its arguments and give the bits they gave; the argument errors name window and block, launch nothing
and touch no output.  Bit patterns throughout.

The sets are built from the device's own integration results and square-root information with arbitrary unit quaternions in place of the
host's: what is compared here is the gather, not the evaluation (tests/test_gpu_preint_odo_resident.py holds that to the host's bits)."""
import numpy as np
import pytest

import marg_factor_data as mf
import host_part_family_utils as hp
from host_part_family_utils import FILL, _partition
from host_part_family_utils import arrays as _arrays, everything_resident as _everything_resident, layout_odo as _layout, same as _same
from host_part_family_utils import resident_set15 as _resident_set15, resident_set_odo as _resident_set
from ctypes_util import bits

pytestmark = pytest.mark.gpu

P = 64


@pytest.fixture()
def ctx():
    import icgvins
    c = icgvins.Context(64, 64, n_slots=1, max_batch=1, max_points=64)
    yield c
    c.close()


def _call(ctx, a, W, entry="odo", **over):
    return hp.call(ctx, a, W, entry, P=P, **over)


def _reference(ctx, layout, Pw, rebuild, odo, fifteen, prior, prior_res, prior_jac):
    return hp.reference(ctx, layout, Pw, rebuild, hp.sources(prior, prior_res, prior_jac, fifteen, odo), P=P)


def test_build_from_resident_factors_equals_build_from_fetched_ones(ctx):
    pts, qcs, prior, x = _everything_resident(ctx)
    _partition(ctx, 6)
    layout, Pw, rebuild = _layout(np.random.RandomState(9), prior, "gather")
    rebuilt = [w for w in range(6) if rebuild[w]]
    keep_layout = [[b if b[0] == "ord" else b[:4] + ("keep",) + b[5:] for b in win] for win in layout]
    fifteen = ctx.preint_fetch_resident()
    r1, J1 = ctx.preint_odo_fetch_resident()
    # first rebuild at point 1: residuals and Jacobians are taken where they are
    rc, msg, got1, _ = _call(ctx, _arrays(layout, Pw, rebuild), 6)
    assert rc == 0, msg
    # a window alone (the others not rebuilt): the same bits
    rc, msg, alone, _ = _call(ctx, _arrays(layout, Pw, [1, 0, 0, 0, 0, 0]), 6)
    assert rc == 0, msg
    _same(alone, got1, [0])
    assert alone[2][1] is None and (alone[0][1:] == FILL).all()
    # second rebuild at point 2, residual only: -1 keeps the Jacobian gathered at point 1
    ctx.preint_odo_evaluate_resident(pts[1], qcs[1], want_jac=False)
    r2, _ = ctx.preint_odo_fetch_resident(want_jac=False)
    rc, msg, got2, _ = _call(ctx, _arrays(keep_layout, Pw, rebuild), 6)
    assert rc == 0, msg
    res, jac = ctx.marg_prior_evaluate(x, want_jac=True)[:2]
    ref1 = _reference(ctx, layout, Pw, rebuild, (r1, J1), fifteen, prior, res, jac)
    ref2 = _reference(ctx, layout, Pw, rebuild, (r2, J1), fifteen, prior, res, jac)
    _same(got1, ref1, rebuilt)
    _same(got2, ref2, rebuilt)
    assert not np.array_equal(bits(r1), bits(r2))
    for w in (0, 1, 2, 5):
        assert np.array_equal(bits(got1[2][w]), bits(got2[2][w])) and not np.array_equal(bits(got1[0][w]), bits(got2[0][w])), w
        assert got1[2][w].any()
    assert not got1[2][3].any() and not got1[0][3].any()  # the window without host blocks: a zero part
    for got in (got1, got2):  # the window that is not rebuilt: nothing of it was written
        assert got[2][4] is None and (got[0][4] == FILL).all() and (got[1][4] == FILL).all()
    ctx.prof_enable(True)
    ctx.preint_odo_evaluate_resident(pts[0], qcs[0])
    rc, msg, again, _ = _call(ctx, _arrays(layout, Pw, rebuild), 6)
    assert rc == 0, msg
    _same(again, ref1, rebuilt)  # a gather over a kept layout
    ctx.sync()
    prof = ctx.prof()
    assert prof["host_part_prior"][0] == 1 and prof["host_part"][0] == 1  # no new accumulation kernel: the two launches of the older entries
    ctx.prof_enable(False)


def test_the_older_entries_are_the_new_one_without_its_arguments(ctx):
    """the 15-state test's own input (priors and 15-state factors, no odometer block) through every entry that takes it"""
    pts15, qcs15 = _resident_set15(ctx)
    prior = mf.make_prior([7], 42)
    ctx.marg_prior_set(*mf.set_args([prior]))
    x = mf.make_x(prior, 100)
    ctx.marg_prior_evaluate_resident(x)
    ctx.preint_evaluate_resident(pts15[0], qcs15[0])
    r15, J15 = ctx.preint_fetch_resident()
    _partition(ctx, 6)
    layout, Pw, rebuild = hp.layout15(np.random.RandomState(9), prior, "gather")
    rebuilt = [w for w in range(6) if rebuild[w]]
    a = _arrays(layout, Pw, rebuild)
    assert a["odo_cols"] is None and (a["odo_of"] < 0).all()
    res, jac = ctx.marg_prior_evaluate(x, want_jac=True)[:2]
    ref = _reference(ctx, layout, Pw, rebuild, None, (r15, J15), prior, res, jac)  # icg_reproj_host_parts_build on fetched values
    assert ref[2][0].any() and ref[2][2].any()
    rc, msg, old, _ = _call(ctx, a, 6, entry="preint")
    assert rc == 0, msg
    _same(old, ref, rebuilt)
    for over in (dict(), dict(odo_of=None), dict(odo_of=None, odo_cols=None)):
        rc, msg, new, _ = _call(ctx, a, 6, **over)
        assert rc == 0, msg
        _same(new, ref, rebuilt)
    # the prior entry and the plain entry on the blocks they take
    no_factors = [[b for b in win if b[0] != "preint"] for win in layout]
    b = _arrays(no_factors, Pw, rebuild)
    rc, msg, by_prior, _ = _call(ctx, b, 6, entry="prior")
    assert rc == 0, msg
    rc, msg, by_new, _ = _call(ctx, b, 6, preint_of=None, preint_cols=None, odo_of=None)
    assert rc == 0, msg
    _same(by_new, by_prior, rebuilt)
    plain = [[blk for blk in win if blk[0] == "ord"] for win in layout]
    c = _arrays(plain, Pw, rebuild)
    rc, msg, by_plain, _ = _call(ctx, c, 6, entry="plain")
    assert rc == 0, msg
    rc, msg, by_new, _ = _call(ctx, c, 6, prior_of=None, preint_of=None, odo_of=None)
    assert rc == 0, msg
    _same(by_new, by_plain, rebuilt)
    assert by_plain[2][1].any()


def test_argument_errors_name_window_and_block_and_launch_nothing(ctx):
    pts, qcs = _resident_set(ctx)
    pts15, qcs15 = _resident_set15(ctx)
    prior = mf.make_prior([7], 42)
    ctx.marg_prior_set(*mf.set_args([prior]))
    ctx.marg_prior_evaluate_resident(mf.make_x(prior, 100))
    ctx.preint_evaluate_resident(pts15[0], qcs15[0])
    _partition(ctx, 6)
    layout, Pw, rebuild = _layout(np.random.RandomState(9), prior, "gather")
    good = _arrays(layout, Pw, rebuild)
    ctx.prof_enable(True)

    def refused(text, entry="odo", **over):
        ctx.sync()
        before = ctx.prof()
        rc, msg, (s, dg, _), part = _call(ctx, good, 6, entry=entry, **over)
        assert rc == -1 and text in msg and msg.startswith("icg_reproj_host_parts_build_pre"), (text, rc, msg)
        assert (s == FILL).all() and (dg == FILL).all() and (part == FILL).all(), text
        ctx.sync()
        assert ctx.prof() == before, (text, before, ctx.prof())
        return msg

    changed = lambda key, idx, val: {key: np.concatenate([good[key][:idx], [val], good[key][idx + 1:]]).astype(good[key].dtype)}
    # blocks of the call: 0, 1 | 2, 3 | 4, 5, 6 | | 7, 8 | 9, 10.  The odometer set is there but nothing was evaluated
    refused("window 0, block 0: no odometer preintegration set is resident and evaluated with Jacobians")
    ctx.preint_odo_evaluate_resident(pts[0], qcs[0], want_jac=False)
    refused("window 0, block 0: no odometer preintegration set is resident and evaluated with Jacobians")
    ctx.preint_odo_evaluate_resident(pts[0], qcs[0])
    msg = refused("window 0, block 1: factor 6 outside the resident odometer set of 6", **changed("odo_of", 1, 6))
    assert msg.startswith("icg_reproj_host_parts_build_preint_odo:")
    refused("window 1, block 0: 18 residuals, an odometer preintegration factor has 19", **changed("nr", 2, 18))
    for bad in (34, -1, 6, 23):
        refused(f"window 0, block 0: odometer preintegration column {bad} ", **changed("odo_cols", 3, bad))
    refused("window 2, block 2: both a prior (0) and an odometer preintegration factor (1)", **changed("odo_of", 6, 1))
    refused("window 5, block 0: both a preintegration factor (2) and an odometer preintegration factor (0)", **changed("odo_of", 9, 0))
    refused("window 2, block 2: both a prior (0) and a preintegration factor (1)", **changed("preint_of", 6, 1))
    refused("window 2, block 0: ICG_HP_JAC_FROM_PREINT_ODO for a block that is no odometer preintegration factor", **changed("jac_off", 4, -4))
    refused("window 2, block 2: ICG_HP_JAC_FROM_PREINT_ODO for a block that is no odometer preintegration factor", **changed("jac_off", 6, -4))
    refused("window 0, block 0: ICG_HP_JAC_FROM_PREINT for a block that is no preintegration factor", **changed("jac_off", 0, -3))
    refused("an odometer preintegration block without preint_odo_cols", odo_cols=None)
    # -4 without preint_odo_of: the older entry's own name
    msg = refused("ICG_HP_JAC_FROM_PREINT_ODO", entry="preint")
    assert msg.startswith("icg_reproj_host_parts_build_preint:")
    # a new set invalidates what was evaluated; a failed set leaves none; then the good call goes through
    _resident_set(ctx)
    refused("no odometer preintegration set is resident and evaluated")
    assert ctx.lib.icg_preint_odo_set(ctx.h, 0, None, None, None, None, None, None, None, None, None) == -1
    refused("no odometer preintegration set is resident and evaluated")
    _resident_set(ctx)
    ctx.preint_odo_evaluate_resident(pts[0], qcs[0])
    rc, msg, _, _ = _call(ctx, good, 6)
    assert rc == 0, msg
    ctx.prof_enable(False)
