"""GPU: which error icg_reproj_host_parts_build_preint reports.  Every refusal is compared by return code and by the WHOLE message, the
expected strings written out here from the entry's format strings; a call with two defects reports the first in the entry's order (the
call-level checks, then the blocks in ascending order with shape, capacity, nf > Pw, columns, prior rules, preintegration rules and jac_off
inside a block; a window that is not rebuilt is checked for shape and capacity only).  A refused call writes no output, launches nothing
and leaves the context as it was: the good call gives the same bits after all refusals as before them.

The smallest data that reaches every check: three windows (window 1 not rebuilt), P = 8, ordinary blocks of at most 3 x 3, one resident
prior of r = 7 (a 7-block and one uncovered column) and a resident P2 set of two factors."""
import numpy as np
import pytest

import marg_factor_data as mf
import preint_data as pd
import preint_split_data as sd
from host_part_family_utils import _partition, arrays as _arrays, unit as _unit
from ctypes_util import bits, i32

pytestmark = pytest.mark.gpu

FILL = 7.0
P = 8
W = 3
ME = "icg_reproj_host_parts_build_preint"
PW = [8, 5, 6]
REBUILD = [1, 0, 1]
INVALID, CAPACITY = -1, -5


def _resident_sets(ctx):
    """one prior of r = 7 and two preintegration factors (N E), both sets evaluated (the factors with Jacobians)"""
    prior = mf.make_prior([7], 42, gap_after=0, gap=1)
    assert prior["r"] == 7
    ctx.marg_prior_set(*mf.set_args([prior]))
    ctx.marg_prior_evaluate_resident(mf.make_x(prior, 100))
    n = 2
    imus, states = sd.intervals([21] * n, seed0=70)
    off = (np.arange(n + 1) * 21).astype(np.int32)
    cur, delta, jac, cov, dt, pn = ctx.preint_batch(1, off, np.concatenate(imus), np.stack(states), pd.PARAMS)
    pn_rows = pn.reshape(n, 21, 4)[:, :20].reshape(-1, 4)
    pn_off = (np.arange(n + 1) * 20).astype(np.int32)
    env = np.tile(pd.PARAMS[5:9], (n, 1))
    pts = np.stack([sd.eval_point("perturbed", states[i], cur[i]) for i in range(n)])
    _, _, S, status = ctx.preint_evaluate_batch(1, delta, jac, cov, dt, env, pts, pn_off, pn_rows)
    assert np.all(status == 0)
    rng = np.random.RandomState(3)
    ctx.preint_set([0, 1], delta, jac, S, dt, env, _unit(rng, n, 1e-5), pn_off, pn_rows)
    ctx.preint_evaluate_resident(pts, _unit(rng, n, 1e-3))


def _layout():
    """blocks 0 .. 8 of the call: (window 0) ordinary, prior, factor 1; (window 1, not rebuilt) ordinary, prior, factor 0; (window 2) factor 0,
    ordinary, prior.  The resident blocks of window 1 only advance the cursors of prior_cols and preint_cols."""
    rng = np.random.RandomState(11)
    mk = lambda nr, cols: ("ord", rng.normal(0, 1.0, (nr, len(cols))), rng.normal(0, 1.0, nr), np.asarray(cols, np.int32))
    return [[mk(3, [0, 1, 2]), ("prior", 0, i32(range(6)), i32(range(2, 8)), "gather", 7), ("preint", 1, i32([0, 7, 16, 23]), i32([0, 3, 5, 7]), "gather")],
            [mk(2, [4, 0, 2]), ("prior", 0, i32([5, 0, 3]), i32([1, 2, 3]), "gather", 7), ("preint", 0, i32([31, 8]), i32([0, 4]), "gather")],
            [("preint", 0, i32([1, 2, 24, 25, 30]), i32([5, 4, 3, 2, 1]), "gather"), mk(3, [0, 5]), ("prior", 0, i32([6, 2]), i32([0, 1]), "gather", 7)]]


def _call(ctx, a, P_arg=P, **over):
    a = dict(a)
    a.update(over)
    out = dict(host_s=np.full((W, P), FILL), host_diag=np.full((W, P), FILL), part_out=np.full(8 * 9 // 2 * W, FILL))
    given = {k: (over[k] if k in over else v) for k, v in out.items()}
    rc = ctx.reproj_host_parts_build_preint_raw(P_arg, a["Pw"], a["rebuild"], a["blk_off"], a["nr"], a["nf"], a["cols"], a["jac_off"], a["J"], a["r"],
                                                given["host_s"], given["host_diag"], given["part_out"], a["prior_of"], a["prior_cols"], a["preint_of"],
                                                a["preint_cols"])
    return rc, ctx.lib.icg_last_error(ctx.h).decode(), out


@pytest.fixture()
def ctx():
    import icgvins
    c = icgvins.Context(64, 64, n_slots=1, max_batch=1, max_points=64)
    yield c
    c.close()


def test_the_first_defect_in_the_entry_s_order_is_the_one_reported(ctx):
    _resident_sets(ctx)
    _partition(ctx, W)
    good = _arrays(_layout(), PW, REBUILD)
    assert list(good["blk_off"]) == [0, 3, 6, 9] and len(good["prior_cols"]) == 11 and len(good["preint_cols"]) == 11
    rc, msg, first = _call(ctx, good)
    assert rc == 0, msg
    assert all((first[k][0] != FILL).all() and (first[k][1] == FILL).all() for k in ("host_s", "host_diag"))
    ctx.prof_enable(True)

    def put(key, *idx_val):
        v = good[key].copy()
        v[list(idx_val[0::2])] = idx_val[1::2]
        return {key: v}

    def refused(code, text, P_arg=P, **over):
        ctx.sync()
        before = ctx.prof()
        rc, msg, out = _call(ctx, good, P_arg, **over)
        assert (rc, msg) == (code, f"{ME}: {text}"), (text, rc, msg)
        for k, v in out.items():
            assert (v == FILL).all(), (text, k)
        ctx.sync()
        assert ctx.prof() == before, (text, before, ctx.prof())

    # (a) one defect: the messages no other test names
    refused(INVALID, "P = 0", P_arg=0)
    refused(CAPACITY, "reduced systems of more than 512 camera columns are not supported (513)", P_arg=513)
    for key in ("Pw", "rebuild", "blk_off", "host_s", "host_diag"):
        refused(INVALID, "NULL argument", **{key: None})
    refused(INVALID, "window 0: blk_off[0] = 1", **put("blk_off", 0, 1))
    refused(INVALID, "window 1: blk_off decreases (2 after 3)", **put("blk_off", 2, 2))
    refused(INVALID, "window 0: Pw = 0 (1 .. 8)", **put("Pw", 0, 0))
    refused(INVALID, "window 0, block 0: 0 x 3", **put("nr", 0, 0))
    refused(CAPACITY, "window 0, block 0: 1025 residuals (at most 1024)", **put("nr", 0, 1025))
    refused(INVALID, "window 2, block 0: 5 columns in a system of 4", **put("Pw", 2, 4))
    refused(INVALID, "window 0, block 0: column 8 outside the system (8)", **put("cols", 1, 8))
    refused(INVALID, "window 0, block 0: column 0 twice", **put("cols", 1, 0))
    refused(INVALID, "window 0, block 0: jac_off = -5", **put("jac_off", 0, -5))
    refused(INVALID, "window 0, block 0: a Jacobian offset without J", J=None)
    refused(INVALID, "window 0, block 0: jac_off = -2", **put("jac_off", 0, -2))  # ICG_HP_JAC_FROM_PRIOR on an ordinary block
    refused(INVALID, "window 0, block 1: prior column 7 outside the prior (7)", **put("prior_cols", 1, 7))
    refused(INVALID, "window 0, block 1: 6 residuals, prior 0 has 7", **put("nr", 1, 6))
    refused(INVALID, "window 0, block 1: prior 1 outside the resident set of 1", **put("prior_of", 1, 1))
    refused(INVALID, "window 0, block 1: a prior block without prior_cols", prior_cols=None)
    # the cursors of prior_cols / preint_cols run over the resident blocks of the window that is not rebuilt too: entries 9 and 6 are the first of
    # window 2's prior (block 2) and factor (block 0), entries 6 and 4 belong to window 1 and are not looked at
    refused(INVALID, "window 2, block 2: prior column -1 outside the prior (7)", **put("prior_cols", 9, -1))
    refused(INVALID, "window 2, block 0: preintegration column 22 (0 .. 31 without 6 and 22)", **put("preint_cols", 6, 22))

    # (b) two defects: the entry's order decides
    # blocks in ascending order: a bad column in window 0 before a bad nr in window 1
    refused(INVALID, "window 0, block 0: column 8 outside the system (8)", rebuild=np.array([1, 1, 1], np.uint8), **put("cols", 1, 8), **put("nr", 3, 1025))
    # inside a block: nf > Pw before the columns
    refused(INVALID, "window 2, block 0: 5 columns in a system of 4", **put("Pw", 2, 4), **put("cols", 22, 5))
    # a window's blocks in their order, whichever family they are of: the prior of block 1 before the factor of block 2 ...
    refused(INVALID, "window 0, block 1: 6 residuals, prior 0 has 7", **put("nr", 1, 6), **put("preint_cols", 0, 6))
    # ... and the factor of block 0 before the prior of block 2
    refused(INVALID, "window 2, block 0: preintegration column 6 (0 .. 31 without 6 and 22)", **put("nr", 8, 6), **put("preint_cols", 6, 6))
    # the preintegration rules before the jac_off cases
    refused(INVALID, "window 0, block 1: both a prior (0) and a preintegration factor (1)", **put("preint_of", 1, 1), **put("jac_off", 1, -3))
    # a window that is not rebuilt: its capacity defect comes first in block order and is reported ...
    refused(CAPACITY, "window 1, block 0: 1025 residuals (at most 1024)", **put("nr", 3, 1025), **put("cols", 22, 5))
    # ... its column defect is not: the rebuilt window's is
    refused(INVALID, "window 2, block 0: column 5 twice", **put("cols", 13, 99, 22, 5))

    # (c) the good call after all refusals: the bits of the call before them (and so with the column defect of the window that is not rebuilt)
    for over in ({}, put("cols", 13, 99)):
        rc, msg, again = _call(ctx, good, **over)
        assert rc == 0, msg
        for k in first:
            assert np.array_equal(bits(again[k]), bits(first[k])), k
    ctx.prof_enable(False)
