"""GPU: the preintegration inner loop with one parameter row PER INTERVAL and the square-root information formed behind it on the device
(icg_preint_batch_params for the Normal / Earth variants, icg_preint_odo_batch_params for Odo / EarthOdo).

Every comparison of integration outputs is bit for bit (np.array_equal on the uint64 views): a call with a row per interval against
icg_preint_batch / icg_preint_odo_batch on each interval alone with its row, in every output and in the pn rows the kernel must leave
alone; a call whose rows are all equal against ONE call of the old entry on the batch.  sqrt_info / status against
icg_preint_evaluate_batch / icg_preint_odo_evaluate_batch on the call's own results (the same kernel: every pattern equal, NaNs too) and
against the host's sqrtInformation() (NaN in the same places: the 2- and 3-sample intervals have an indefinite inverse covariance on every
side).  The reference goldens go through one call per variant and meet the bounds tests/test_gpu_preint.py / test_gpu_preint_odo.py apply.
Argument errors return ICG_ERR_INVALID before any launch."""
import ctypes as C

import numpy as np
import pytest

import preint_edge_data as ed
import preint_odo_data as od
import preint_streams_data as sd
from ctypes_util import ErrBuf, bits, f64, i32, ptr, same_bits

pytestmark = pytest.mark.gpu

ICG_OK, ICG_ERR_INVALID = 0, -1
SENTINEL = sd.SENTINEL
CASES = [(name, v) for name, fam in sd.FAMILIES.items() for v in fam.variants]
OUT = ("cur", "delta", "jac", "cov", "dt")


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
def singles(ctx):
    """(family, variant, interval, row) -> the old entry's outputs for that interval alone with that row; computed once per pair"""
    cache = {}

    def get(fam, variant, i, k, items, rows):
        key = (fam.name, variant, i, k)
        if key not in cache:
            cache[key] = fam.single(ctx, variant, items[i][0], items[i][1], rows[k])
        return cache[key]
    return get


def _eq(a, b):
    return np.array_equal(bits(a), bits(b))


def _check_against_singles(fam, variant, got, order, rows_of, items, rows, singles):
    """got: the outputs of one params call on [items[i] for i in order] with rows [rows[k] for k in rows_of], its arrays SENTINEL-filled"""
    cur, delta, jac, cov, dt, pn = got[:6]
    off = np.cumsum([0] + [len(items[i][0]) for i in order])
    kept = bits(pn).reshape(-1, 4) == bits(SENTINEL)
    for slot, (i, k) in enumerate(zip(order, rows_of)):
        exp = singles(fam, variant, i, k, items, rows)
        for name, g, e in zip(OUT, (cur, delta, jac, cov, dt), exp[:5]):
            assert _eq(g[slot], e[0]), (slot, i, k, name)
        b, n = int(off[slot]), len(items[i][0])
        if variant == fam.earth:
            assert _eq(pn[b:b + n - 1], exp[5][:n - 1]), (slot, "pn")
            assert not np.any(kept[b:b + n - 1]), (slot, "a pn row of the interval's own was left out")
            assert np.all(kept[b + n - 1]), (slot, "the interval's last pn row was written")
        else:
            assert np.all(kept[b:b + n]), (slot, "a pn row was written by a variant that has none")


# ---- parity against single-interval calls ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("arrangement", ["as_is", "reversed", "alone", "tiled_130"])
@pytest.mark.parametrize("family,variant", CASES)
def test_row_per_interval_equals_the_old_entry_on_each_interval_alone(ctx, singles, family, variant, arrangement):
    fam = sd.FAMILIES[family]
    items, rows = fam.items(), fam.rows(130)
    assert len({r.tobytes() for r in rows}) == 130 and all(len({r[c] for r in rows[:5]}) == 5 for c in range(6))  # (the rows do differ)
    n5 = len(items)
    if arrangement == "as_is":
        order = rows_of = list(range(n5))
    elif arrangement == "reversed":
        order = rows_of = list(range(n5))[::-1]
    elif arrangement == "alone":
        order = rows_of = [fam.lens.index(41)]
    else:
        order, rows_of = [i % n5 for i in range(130)], list(range(130))
    got = fam.many(ctx, variant, [items[i] for i in order], rows[rows_of], fill=SENTINEL)
    _check_against_singles(fam, variant, got, order, rows_of, items, rows, singles)
    # without the S launch: the same integration outputs
    plain = fam.many(ctx, variant, [items[i] for i in order], rows[rows_of], want_sqrt_info=False, want_status=False, fill=SENTINEL)
    for a, b in zip(got[:6], plain[:6]):
        assert _eq(a, b)


# ---- shared row ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family,variant", CASES)
def test_equal_rows_equal_one_call_of_the_old_entry(ctx, family, variant):
    fam = sd.FAMILIES[family]
    items = fam.items() * 3  # 15 intervals
    row = fam.rows(3)[2]
    exp = fam.batch(ctx, variant, items, row)
    got = fam.many(ctx, variant, items, np.tile(row, (len(items), 1)))
    for name, g, e in zip(OUT + ("pn",), got[:6], exp):
        assert _eq(g, e), name


# ---- S and status -------------------------------------------------------------------------------------------------------------------
def _host_sqrt_info(hostlib, fam, variant, imu, s0, hostpar, point):
    """the host's sqrtInformation() of one interval through the existing entry (device P1 with the old entry, updateSqrtInformation on the host)"""
    N, NJ = fam.N, (646 if fam.odo else 480)
    off = np.array([0, len(imu)], np.int32)
    o = dict(cur=np.zeros((1, 16)), rh=np.zeros((1, N)), Jh=np.zeros((1, NJ)), rd=np.zeros((1, N)), Jd=np.zeros((1, NJ)), Sh=np.full((1, N * N), SENTINEL),
             Sd=np.zeros((1, N * N)), okh=np.full(1, -1, np.int32), okd=np.full(1, -1, np.int32))
    err = ErrBuf()
    fn = hostlib.icgh_backend_preint_odo_device if fam.odo else hostlib.icgh_backend_preint_device
    rc = fn(int(variant), 1, ptr(off), ptr(f64(imu)), ptr(f64(s0[None, :])), ptr(f64(hostpar)), ptr(f64(point[None, :])), ptr(o["cur"]), ptr(o["rh"]),
            ptr(o["Jh"]), ptr(o["rd"]), ptr(o["Jd"]), ptr(o["Sh"]), ptr(o["Sd"]), ptr(o["okh"]), ptr(o["okd"]), *err.args)
    assert rc == 0, err.text()
    return o["Sh"][0], int(o["okh"][0])


@pytest.mark.parametrize("family,variant", CASES)
def test_sqrt_info_and_status_are_the_evaluate_entrys_and_the_hosts(ctx, hostlib, family, variant):
    fam = sd.FAMILIES[family]
    items, rows, abv = fam.items(), fam.rows(5), fam.abv(5)
    N = fam.N
    cur, delta, jac, cov, dt, pn, S, status = fam.many(ctx, variant, items, rows, fill=SENTINEL)
    lens = [len(i) for i, _ in items]
    off = sd.offsets_of(items)
    pn_off = np.cumsum([0] + [n - 1 for n in lens]).astype(np.int32)
    pn_rows = np.concatenate([pn[off[i]:off[i] + n - 1] for i, n in enumerate(lens)] + [np.zeros((1, 4))])
    points = fam.eval_points(items, cur)
    _, _, S_ev, st_ev = fam.evaluate(ctx, variant, delta, jac.reshape(-1, N * N), cov.reshape(-1, N * N), dt, rows[:, 5:9], points, pn_off, pn_rows)
    assert np.array_equal(status, st_ev) and _eq(S, S_ev)
    one = lens.index(1)
    assert status[one] == 1 and np.all(bits(S[one]) == 0)  # a one-sample interval: singular covariance, a zero matrix
    for i in (lens.index(41), lens.index(17) if fam.odo else lens.index(7)):
        assert status[i] == 0 and np.all(np.isfinite(S[i])) and np.abs(S[i]).max() > 0
    for i, n in enumerate(lens):  # the 2- and 3-sample intervals are NaN on every side
        if n in (2, 3):
            assert status[i] == 0 and np.isnan(S[i]).any(), n
    for i, (imu, s0) in enumerate(items):
        Sh, okh = _host_sqrt_info(hostlib, fam, variant, imu, s0, fam.host_params(rows[i], abv[i]), points[i])
        assert same_bits(S[i], Sh), (i, lens[i])
        assert not np.any(bits(Sh) == bits(SENTINEL))
        assert (okh == 0) == (status[i] != 0) or np.isnan(Sh).any(), (i, okh, status[i])
    # each on its own
    only_S = fam.many(ctx, variant, items, rows, want_status=False)
    only_st = fam.many(ctx, variant, items, rows, want_sqrt_info=False)
    assert only_S[7] is None and _eq(only_S[6], S) and only_st[6] is None and np.array_equal(only_st[7], status)
    for a, b, c in zip(only_S[:5], only_st[:5], (cur, delta, jac, cov, dt)):
        assert _eq(a, c) and _eq(b, c)


@pytest.mark.parametrize("family,variant", CASES)
def test_without_sqrt_info_and_status_the_second_launch_is_not_made(ctx, family, variant):
    fam = sd.FAMILIES[family]
    items, rows = fam.items(), fam.rows(5)
    ctx.prof_enable(True)
    try:
        fam.many(ctx, variant, items, rows)
        p = ctx.prof()
        assert p[fam.p1][0] == 1 and p[fam.s][0] == 1, p
        fam.many(ctx, variant, items, rows, want_sqrt_info=False, want_status=False)
        p = ctx.prof()
        assert p[fam.p1][0] == 2 and p[fam.s][0] == 1, p
        fam.many(ctx, variant, items, rows, want_sqrt_info=False)
        p = ctx.prof()
        assert p[fam.p1][0] == 3 and p[fam.s][0] == 2, p
    finally:
        ctx.prof_enable(False)


# ---- reference golden ---------------------------------------------------------------------------------------------------------------
def _close(a, b, tol=1e-9):
    return np.abs(a - b).max() <= tol * max(1e-30, np.abs(b).max())


@pytest.mark.parametrize("variant", [0, 1])
def test_golden_cases_in_one_call_each_with_its_own_parameters(ctx, variant):
    """the bounds of tests/test_gpu_preint.py::test_preint_kernel_matches_reference_golden"""
    from test_oracle_vs_reference import preint_golden_cases
    cases = [c for _, c in preint_golden_cases() if int(c["variant"]) == variant]
    assert len(cases) >= 2
    items = [(c["imu"], c["s0"]) for c in cases]
    cur, delta, jac, cov, dt, _, S, status = sd.FAMILIES["imu"].many(ctx, variant, items, np.stack([c["params"] for c in cases]))
    for i, c in enumerate(cases):
        assert _close(cur[i], c["cur"]) and _close(delta[i], c["delta"])
        assert abs(dt[i] - float(c["dt"])) < 1e-12
        assert _close(jac[i], c["jac"]) and _close(cov[i], c["cov"], 1e-8)
        ed.check_result(dict(cur=cur[i], delta=delta[i], jac=jac[i], cov=cov[i], dt=dt[i]),
                        dict(cur=c["cur"], delta=c["delta"], jac=c["jac"], cov=c["cov"], dt=float(c["dt"])), len(c["imu"]), f"variant {variant} golden case {i}")


@pytest.mark.parametrize("variant", od.VARIANTS)
def test_odo_golden_cases_in_one_call_each_with_its_own_parameters(ctx, variant):
    """the bounds of tests/test_gpu_preint_odo.py::test_p1_matches_the_reference_and_integrate_ld against the reference"""
    gs = [g for g in od.golden() if g["variant"] == variant]
    assert len(gs) >= 2
    fam = sd.FAMILIES["odo"]
    cur, delta, jac, cov, dt, pn, S, status = fam.many(ctx, variant, [(g["imu"], g["s0"]) for g in gs], np.stack([g["par25"] for g in gs]))
    off = np.cumsum([0] + [len(g["imu"]) for g in gs])
    for i, g in enumerate(gs):
        n = len(g["imu"])
        got = dict(cur=cur[i], delta=delta[i], jac=jac[i], cov=cov[i], dt=dt[i], pn=pn[off[i]:off[i] + n - 1] if variant == od.EARTH_ODO else None)
        exp = dict(g, pn=g["pn"] if variant == od.EARTH_ODO else None)
        for k in ("cur", "delta", "jac", "cov"):
            assert od.whole_rel(got[k], exp[k]) <= (1e-8 if k == "cov" else 1e-9), (g["case"], k)
        od.check_result(got, exp, n, f"params call vs reference, variant {variant} {g['case']}")


# ---- argument errors ----------------------------------------------------------------------------------------------------------------
def _raw(ctx, fam, variant, n, offsets, imu, s0, rows, total, null=(), handle=True):
    """the entry on sentinel-filled outputs; `null` names the arguments passed as NULL -> (rc, message, outputs)"""
    m, NN = max(n, 1), fam.N * fam.N
    bufs = dict(cur=np.full((m, 16), SENTINEL), delta=np.full((m, fam.w_delta), SENTINEL), jac=np.full((m, NN), SENTINEL), cov=np.full((m, NN), SENTINEL),
                dt=np.full(m, SENTINEL), pn=np.full((max(total, 1), 4), SENTINEL), S=np.full((m, NN), SENTINEL), status=np.full(m, -7, np.int32))
    ins = dict(offsets=i32(offsets), imu=f64(imu), state0=f64(s0), params=f64(rows))
    p = lambda name, a: None if name in null else ptr(a)
    rc = getattr(ctx.lib, fam.entry)(ctx.h if handle else None, int(variant), int(n), p("offsets", ins["offsets"]), p("imu", ins["imu"]),
                                     p("state0", ins["state0"]), p("params", ins["params"]), p("cur", bufs["cur"]), p("delta", bufs["delta"]),
                                     p("jac", bufs["jac"]), p("cov", bufs["cov"]), p("dt", bufs["dt"]), p("pn", bufs["pn"]), p("S", bufs["S"]),
                                     p("status", bufs["status"]))
    return rc, ctx.lib.icg_last_error(ctx.h).decode(), bufs


def _untouched(bufs):
    return all(np.all(bits(b) == bits(SENTINEL)) for k, b in bufs.items() if k != "status") and np.all(bufs["status"] == -7)


@pytest.mark.parametrize("family,variant", CASES)
def test_argument_errors_launch_nothing_and_touch_nothing(ctx, family, variant):
    fam = sd.FAMILIES[family]
    imu41 = fam.interval(41, 3)
    imu, s0, rows = np.concatenate([imu41, imu41]), np.stack([fam.state(k) for k in range(3)]), fam.rows(3)
    good = [0, 41, 61, 82]
    ctx.prof_enable(True)
    try:
        rc, _, bufs = _raw(ctx, fam, variant, 3, good, imu, s0, rows, 82)
        assert rc == ICG_OK and not np.any(bits(bufs["cur"]) == bits(SENTINEL)) and np.all(bufs["status"] == 0)
        before = ctx.prof()
        assert before[fam.p1][0] == 1 and before[fam.s][0] == 1
        refused = []
        for bad in ({0: 2, 1: 3, 2: 0, 3: 1}[variant], -1, 4):
            refused.append(("variant %d" % bad, _raw(ctx, fam, bad, 3, good, imu, s0, rows, 82), None))
        refused.append(("n = -1", _raw(ctx, fam, variant, -1, good, imu, s0, rows, 82), None))
        for null in ("offsets", "imu", "state0", "params", "cur", "delta", "jac", "cov", "dt"):
            refused.append(("NULL " + null, _raw(ctx, fam, variant, 3, good, imu, s0, rows, 82, null=(null,)), None))
        refused.append(("offsets[0] < 0", _raw(ctx, fam, variant, 3, [-1, 41, 61, 82], imu, s0, rows, 82), "interval 0"))
        for k, offsets in enumerate(([0, 0, 41, 82], [0, 41, 41, 82], [0, 41, 82, 82])):
            refused.append((f"interval {k} empty", _raw(ctx, fam, variant, 3, offsets, imu, s0, rows, 82), f"interval {k} has no IMU sample"))
        for what, (rc, msg, bufs), names in refused:
            assert rc == ICG_ERR_INVALID and _untouched(bufs), what
            assert fam.entry in msg, (what, msg)
            if names:
                assert names in msg, (what, msg)
        rc, _, bufs = _raw(ctx, fam, variant, 3, good, imu, s0, rows, 82, handle=False)
        assert rc == ICG_ERR_INVALID and _untouched(bufs)
        rc, _, bufs = _raw(ctx, fam, variant, 0, [0], imu, s0, rows, 82)
        assert rc == ICG_OK and _untouched(bufs)
        assert ctx.prof() == before  # no profiler count moved
        # and the context still integrates
        rc, _, again = _raw(ctx, fam, variant, 3, good, imu, s0, rows, 82)
        assert rc == ICG_OK
    finally:
        ctx.prof_enable(False)
