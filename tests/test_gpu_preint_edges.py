"""GPU parity of the preintegration inner loop (P1, k_preint / icg_preint_batch) at the edges of tests/preint_edge_data.py:
per 3x3 block and per state field against the extended-precision restatement integrate_ld and against the CPU oracle (TOL = 1e-12:
kernel and oracle are built without contraction and differ in sin / cos alone), bit for bit where no sin / cos argument differs from
zero, independent of the neighbours in a launch, exact on degenerate intervals and pn rows, and refusing bad arguments untouched.

Measured on an MI355X, kernel against integrate_ld, worst block / field per case and variant: 41-sample cases jac <= 8.5e-16, cov <= 1.5e-15,
cur <= 1.2e-15, delta <= 5.9e-16, pn <= 8.6e-16; long (401 samples, all Earth rates) jac 1.0e-14, cov 8.5e-15, cur <= 2.2e-15, delta <= 1.1e-15,
pn <= 1.2e-15; two_samples <= 4.3e-16; one_sample exact.  These are the oracle's own figures (tests/test_oracle_preint_edges.py) digit for
digit; test_parity_per_block prints them per case."""
import ctypes as C

import numpy as np
import pytest

import preint_edge_data as ed

pytestmark = pytest.mark.gpu

ICG_OK, ICG_ERR_INVALID = 0, -1
SENTINEL = -1.2345e300
KEYS = ("cur", "delta", "jac", "cov", "dt")
GROUPS = [(v, gi) for v in (0, 1) for gi in range(len(ed.groups(v)))]


@pytest.fixture(scope="module")
def ctx():
    import icgvins
    c = icgvins.Context(640, 480, n_slots=1, max_batch=1, max_points=64)
    yield c
    c.close()


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


def _same_bits(a, b):
    return np.array_equal(_bits(a), _bits(b))


def _launch(ctx, variant, items, par, want_pn=True):
    """items: list of (imu, state0) -> per interval dict(cur, delta, jac, cov, dt, pn = the rows the interval owns (n - 1) or None)"""
    lens = [len(imu) for imu, _ in items]
    offsets = np.cumsum([0] + lens).astype(np.int32)
    cur, delta, jac, cov, dt, pn = ctx.preint_batch(variant, offsets, np.concatenate([imu for imu, _ in items]),
                                                    np.stack([s0 for _, s0 in items]), par, want_pn=want_pn)
    return [dict(cur=cur[i], delta=delta[i], jac=jac[i], cov=cov[i], dt=dt[i],
                 pn=pn[offsets[i]:offsets[i] + n - 1] if (want_pn and variant == 1) else None) for i, n in enumerate(lens)]


def _launch_named(ctx, variant, names, par, **kw):
    cs = ed.cases(variant)
    return _launch(ctx, variant, [cs[n][:2] for n in names], par, **kw)


# ---- 1. parity per block ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant,gi", GROUPS)
def test_parity_per_block(oracle, ctx, variant, gi):
    par, names = ed.groups(variant)[gi]
    cs = ed.cases(variant)
    out = _launch_named(ctx, variant, names, par)
    for name, got in zip(names, out):
        imu, s0, _ = cs[name]
        exp = ed.reference(variant, name)
        orc = oracle.preint_integrate(variant, imu, s0, par)
        if variant == 0:
            orc.pop("pn")
        for k in ("cur", "delta", "jac", "cov"):
            assert np.all(np.isfinite(got[k])), (name, k)
        # (figures first, then the assertions)
        fig = {k: (ed.block_rel if k in ("jac", "cov") else ed.field_rel)(got[k], exp[k])[0] for k in ("jac", "cov", "cur", "delta")}
        if variant == 1:
            fig["pn"] = ed.pn_rel(got["pn"], exp["pn"])
        print(f"GPUFIG variant {variant} {name}: " + "  ".join(f"{k} {v:.1e}" for k, v in fig.items()))
        ed.check_result(got, exp, len(imu), f"kernel vs integrate_ld, variant {variant} {name}")
        ed.check_result(got, orc, len(imu), f"kernel vs oracle, variant {variant} {name}")


# ---- 2. bits where no libm call can differ ------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1])
def test_zero_rotation_is_bit_identical_to_the_oracle(oracle, ctx, variant):
    """every sin / cos argument is exactly zero (Earth variant: with the zero Earth rate); the rest is + - * / sqrt without contraction on
    both sides, and the kernel's sparse products claim the bits of the oracle's dense ones"""
    imu, s0, par = ed.cases(variant)["zero_rotation"]
    if variant == 1:
        assert np.all(par[6:9] == 0.0)
    got = _launch(ctx, variant, [(imu, s0)], par)[0]
    orc = oracle.preint_integrate(variant, imu, s0, par)
    assert _same_bits(got["delta"][3:7], [0.0, 0.0, 0.0, 1.0])
    for k in KEYS:
        diff = np.flatnonzero(_bits(got[k]).ravel() != _bits(orc[k]).ravel())
        assert diff.size == 0, f"{k}: {diff.size} entries differ, first at flat index {diff[0]}"
    if variant == 1:
        assert _same_bits(got["pn"], orc["pn"])


# ---- 3. independence from the launch ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1])
@pytest.mark.parametrize("name", ["plain", "jitter_dt"])
def test_result_is_independent_of_the_launch(ctx, variant, name):
    par, names = ed.groups(variant)[0]
    assert name in names and "long" in names and "one_sample" in names
    cs = ed.cases(variant)
    fill = [n for n in names if n != name]
    spots = (0, 1, 63, 64, 65, 129)
    slots = [name if i in spots else fill[i % len(fill)] for i in range(130)]
    assert len({len(cs[n][0]) for n in slots}) >= 4  # neighbours of different lengths
    alone = _launch_named(ctx, variant, [name], par)[0]
    first = _launch_named(ctx, variant, slots, par)
    again = _launch_named(ctx, variant, slots, par)
    for i in spots:
        for k in KEYS + (("pn",) if variant == 1 else ()):
            assert _same_bits(first[i][k], alone[k]), (i, k)
    for i, (a, b) in enumerate(zip(first, again)):
        for k in KEYS + (("pn",) if variant == 1 else ()):
            assert _same_bits(a[k], b[k]), (i, slots[i], k)


# ---- 4. rows and degenerate intervals -----------------------------------------------------------------------------------------------
@pytest.mark.parametrize("variant", [0, 1])
def test_one_sample_intervals_are_exact(ctx, variant):
    par, names = ed.groups(variant)[0]
    batch = ["one_sample", "plain", "one_sample", "two_samples", "one_sample"]
    out = _launch_named(ctx, variant, batch, par)
    s0 = ed.cases(variant)["one_sample"][1]
    for i in (0, 2, 4):
        got = out[i]
        assert _same_bits(got["jac"], np.eye(15)) and _same_bits(got["cov"], np.zeros((15, 15)))
        assert _same_bits(got["cur"], s0)
        assert _same_bits(got["delta"], np.concatenate([[0, 0, 0], [0, 0, 0, 1], [0, 0, 0], s0[10:16]]))
        assert _same_bits(got["dt"], 0.0)
    assert np.abs(out[1]["cov"]).max() > 0 and np.abs(out[3]["cov"]).max() > 0


def _raw_call(ctx, variant, n, offsets, imu, s0, par, total, null=(), handle=True):
    """icg_preint_batch on sentinel-filled outputs; `null` names the arguments passed as NULL -> (rc, outputs)"""
    bufs = dict(cur=np.full((max(n, 1), 16), SENTINEL), delta=np.full((max(n, 1), 16), SENTINEL), jac=np.full((max(n, 1), 225), SENTINEL),
                cov=np.full((max(n, 1), 225), SENTINEL), dt=np.full(max(n, 1), SENTINEL), pn=np.full((max(total, 1), 4), SENTINEL))
    ins = dict(offsets=np.ascontiguousarray(offsets, np.int32), imu=np.ascontiguousarray(imu, np.float64),
               state0=np.ascontiguousarray(s0, np.float64), params=np.ascontiguousarray(par, np.float64))
    ptr = lambda name, a: None if name in null else a.ctypes.data_as(C.c_void_p)
    rc = ctx.lib.icg_preint_batch(ctx.h if handle else None, int(variant), int(n), ptr("offsets", ins["offsets"]), ptr("imu", ins["imu"]),
                                  ptr("state0", ins["state0"]), ptr("params", ins["params"]), ptr("cur", bufs["cur"]),
                                  ptr("delta", bufs["delta"]), ptr("jac", bufs["jac"]), ptr("cov", bufs["cov"]), ptr("dt", bufs["dt"]),
                                  ptr("pn", bufs["pn"]))
    return rc, bufs


def _untouched(bufs):
    return all(np.all(_bits(b) == _bits(SENTINEL)) for b in bufs.values())


@pytest.mark.parametrize("variant", [0, 1])
def test_pn_rows_written_are_exactly_the_intervals_own(ctx, variant):
    par, _ = ed.groups(variant)[0]
    cs = ed.cases(variant)
    batch = ["one_sample", "plain", "two_samples", "one_sample", "jitter_dt", "one_sample"]
    items = [cs[n][:2] for n in batch]
    lens = [len(imu) for imu, _ in items]
    offsets = np.cumsum([0] + lens).astype(np.int32)
    rc, bufs = _raw_call(ctx, variant, len(items), offsets, np.concatenate([i for i, _ in items]), np.stack([s for _, s in items]), par,
                         int(offsets[-1]))
    assert rc == ICG_OK
    ref = _launch(ctx, variant, items, par)
    kept = _bits(bufs["pn"]) == _bits(SENTINEL)
    for i, n in enumerate(lens):
        b = int(offsets[i])
        assert _same_bits(bufs["cur"][i], ref[i]["cur"]) and _same_bits(bufs["cov"][i].reshape(15, 15), ref[i]["cov"])
        if variant == 0:
            assert np.all(kept[b:b + n])
            continue
        assert np.all(kept[b + n - 1]), f"interval {i}: its last pn row was written"
        assert not np.any(np.all(kept[b:b + n - 1], axis=1)), f"interval {i}: a pn row of its own was left out"
        assert _same_bits(bufs["pn"][b:b + n - 1], ref[i]["pn"])
        assert np.array_equal(bufs["pn"][b:b + n - 1, 0], items[i][0][1:, 1])  # (dt, position) after sample index at row begin + index - 1


def test_earth_variant_without_pn_buffer(ctx):
    par, names = ed.groups(1)[0]
    batch = ["plain", "one_sample", "jitter_dt", "long", "two_samples"]
    with_pn = _launch_named(ctx, 1, batch, par)
    without = _launch_named(ctx, 1, batch, par, want_pn=False)
    for a, b in zip(with_pn, without):
        assert b["pn"] is None
        for k in KEYS:
            assert _same_bits(a[k], b[k]), k


# ---- 5. argument checks -------------------------------------------------------------------------------------------------------------
def _three_intervals():
    imu, s0, par = ed.cases(0)["plain"]
    return np.concatenate([imu, imu]), np.stack([s0, s0, s0]), par


@pytest.mark.parametrize("variant,n", [(2, 3), (-1, 3), (0, -1), (1, -1)])
def test_bad_variant_or_count_is_refused(ctx, variant, n):
    imu, s0, par = _three_intervals()
    rc, bufs = _raw_call(ctx, variant, n, [0, 41, 61, 82], imu, s0, par, 82)
    assert rc == ICG_ERR_INVALID and _untouched(bufs)


@pytest.mark.parametrize("null", ["offsets", "imu", "state0", "params", "cur", "delta", "jac", "cov", "dt"])
@pytest.mark.parametrize("variant", [0, 1])
def test_null_required_pointer_is_refused(ctx, variant, null):
    imu, s0, par = _three_intervals()
    rc, bufs = _raw_call(ctx, variant, 3, [0, 41, 61, 82], imu, s0, par, 82, null=(null,))
    assert rc == ICG_ERR_INVALID and _untouched(bufs)


def test_null_context_is_refused(ctx):
    imu, s0, par = _three_intervals()
    rc, bufs = _raw_call(ctx, 0, 3, [0, 41, 61, 82], imu, s0, par, 82, handle=False)
    assert rc == ICG_ERR_INVALID and _untouched(bufs)


@pytest.mark.parametrize("offsets", [[0, 0, 41, 82], [0, 41, 41, 82], [0, 41, 82, 82]], ids=["first", "middle", "last"])
@pytest.mark.parametrize("variant", [0, 1])
def test_interval_without_a_sample_is_refused(ctx, variant, offsets):
    imu, s0, par = _three_intervals()
    rc, bufs = _raw_call(ctx, variant, 3, offsets, imu, s0, par, 82)
    assert rc == ICG_ERR_INVALID and _untouched(bufs)
    assert b"no IMU sample" in ctx.lib.icg_last_error(ctx.h)


@pytest.mark.parametrize("variant", [0, 1])
def test_no_interval_is_ok_and_touches_nothing(ctx, variant):
    imu, s0, par = _three_intervals()
    rc, bufs = _raw_call(ctx, variant, 0, [0], imu, s0, par, 82)
    assert rc == ICG_OK and _untouched(bufs)


def test_context_still_integrates_after_refusals(oracle, ctx):
    imu, s0, par = ed.cases(0)["plain"]
    got = _launch(ctx, 0, [(imu, s0)], par)[0]
    ed.check_result(got, ed.reference(0, "plain"), len(imu), "after refused calls")
