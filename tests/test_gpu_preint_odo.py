"""GPU parity of the odometer preintegration (variants 2 = Odo, 3 = EarthOdo; 19-wide state): P1 (k_preint_odo / icg_preint_odo_batch) and
P2 (k_preint_odo_sqrt_info + k_preint_odo_evaluate / icg_preint_odo_evaluate_batch).

P1  against the reference golden (tests/golden/preint_odo_ref_golden.npz) and the extended-precision restatement
    preint_odo_data.integrate_ld: whole-array 1e-9 (covariance 1e-8) as tests/test_gpu_preint.py, per block and per field TOL = 1e-12;
    exact on a one-sample interval; bit-identical to the DENSE float64 restatement where every sin / cos argument is exactly zero (the pin
    that licenses the kernel's sparse products); independent of the neighbours in a launch; pn rows exactly the intervals' own.
P2  the device's square-root information equals the host's bit for bit; residuals and Jacobians against the host's PreintegrationOdo::evaluate
    and against the golden at the project's P2 rule 1e-6 x max(1, max|expected|), measured maximum printed (NaN-aware as
    tests/test_gpu_preint_eval.py: the 2- and 3-sample intervals have an indefinite inverse covariance and every side returns NaN for them);
    a residual-only call and a batch of 70 return the same bytes; a singular covariance (odo_srw = 0) gives zero rows and a refusal on both
    sides (status 1 at the C ABI, as icg_preint_evaluate_batch; ok = 0 through the host layer).
Refusals are argument checks that return before any launch: nothing is written, and the context integrates afterwards.

Measured on an MI355X (the tests print the figures): see DESIGN.md section 0."""
import ctypes as C

import numpy as np
import pytest

import preint_odo_data as od
from ctypes_util import ErrBuf, bits, f64, i32, ptr, same_bits

pytestmark = pytest.mark.gpu

ICG_OK, ICG_ERR_INVALID = 0, -1
SENTINEL = -1.2345e300
KEYS = ("cur", "delta", "jac", "cov", "dt")
GOLDEN = list(range(14))


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


def _launch(ctx, variant, items, par, want_pn=True):
    """items: list of (imu9, state17) -> per interval dict(cur, delta, jac, cov, dt, pn = the rows the interval owns (n - 1) or None)"""
    lens = [len(imu) for imu, _ in items]
    offsets = np.cumsum([0] + lens).astype(np.int32)
    cur, delta, jac, cov, dt, pn = ctx.preint_odo_batch(variant, offsets, np.concatenate([imu for imu, _ in items]),
                                                        np.stack([s0 for _, s0 in items]), par, want_pn=want_pn)
    return [dict(cur=cur[i], delta=delta[i], jac=jac[i], cov=cov[i], dt=dt[i],
                 pn=pn[offsets[i]:offsets[i] + n - 1] if (want_pn and variant == od.EARTH_ODO) else None) for i, n in enumerate(lens)]


def _named(names):
    cs = od.cases()
    return [cs[n][:2] for n in names]


def _whole(got, exp, what):
    """the whole-array bounds of tests/test_gpu_preint.py"""
    fig = {k: od.whole_rel(got[k], exp[k]) for k in ("cur", "delta", "jac", "cov")}
    for k, v in fig.items():
        assert v <= (1e-8 if k == "cov" else 1e-9), f"{what}: {k} {v:.3g}"
    return fig


# ---- P1: parity -----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("k", GOLDEN)
def test_p1_matches_the_reference_and_integrate_ld(ctx, k):
    g = od.golden()[k]
    v, n = g["variant"], len(g["imu"])
    got = _launch(ctx, v, [(g["imu"], g["s0"])], g["par25"])[0]
    for key in ("cur", "delta", "jac", "cov"):
        assert np.all(np.isfinite(got[key])), key
    ld = od.integrate_ld(v, g["imu"], g["s0"], g["par25"])
    exp_g = dict(g, pn=g["pn"] if v == od.EARTH_ODO else None)
    exp_ld = dict(ld, pn=ld["pn"] if v == od.EARTH_ODO else None)
    for name, exp in (("reference", exp_g), ("integrate_ld", exp_ld)):
        fig = {q: val for q, (val, _) in od.figures(got, exp).items()}
        if v == od.EARTH_ODO:
            fig["pn"] = od.pn_rel(got["pn"], exp["pn"])
        print(f"GPUFIG P1 vs {name}, variant {v} {g['case']} ({n} samples): " + "  ".join(f"{q} {val:.1e}" for q, val in fig.items()))
    for name, exp in (("reference", exp_g), ("integrate_ld", exp_ld)):
        _whole(got, exp, f"kernel vs {name}, variant {v} {g['case']}")
        od.check_result(got, exp, n, f"kernel vs {name}, variant {v} {g['case']}")


@pytest.mark.parametrize("variant", od.VARIANTS)
def test_p1_batch_of_lengths_1_2_3_41_7(ctx, variant):
    """offsets, and the partial last pass of 361 entries over 64 lanes, in one call"""
    names = ["one_sample", "two_samples", "three_samples", "plain", "seven_samples"]
    cs = od.cases()
    par = cs["plain"][2]
    assert [len(cs[n][0]) for n in names] == [1, 2, 3, 41, 7] and all(np.array_equal(cs[n][2], par) for n in names)
    out = _launch(ctx, variant, _named(names), par)
    for name, got in zip(names, out):
        exp = od.reference(variant, name)
        exp = dict(exp, pn=exp["pn"] if variant == od.EARTH_ODO else None)
        fig = od.check_result(got, exp, len(cs[name][0]), f"batch, variant {variant} {name}")
        _whole(got, exp, f"batch, variant {variant} {name}")
        print(f"GPUFIG P1 batch vs integrate_ld, variant {variant} {name}: " + "  ".join(f"{q} {val:.1e}" for q, val in fig.items()))


@pytest.mark.parametrize("variant", od.VARIANTS)
def test_one_sample_interval_is_exact(ctx, variant):
    cs = od.cases()
    par = cs["plain"][2]
    out = _launch(ctx, variant, _named(["one_sample", "plain", "one_sample"]), par)
    s0 = cs["one_sample"][1]
    for i in (0, 2):
        got = out[i]
        assert same_bits(got["jac"], np.eye(19)) and same_bits(got["cov"], np.zeros((19, 19)))
        assert same_bits(got["cur"], s0[:16])
        assert same_bits(got["delta"], np.concatenate([[0, 0, 0], [0, 0, 0, 1], [0, 0, 0], s0[10:16], [0, 0, 0], s0[16:17]]))
        assert same_bits(got["dt"], 0.0)
    assert np.abs(out[1]["cov"]).max() > 0


@pytest.mark.parametrize("variant", od.VARIANTS)
def test_zero_rotation_is_bit_identical_to_the_dense_float64_restatement(ctx, variant):
    """dtheta = 0, bg = 0, identity attitude, zero Earth rate: every sin / cos argument is exactly zero, the rest is + - * / sqrt without
    contraction on both sides, and the kernel's sparse products claim the bits of the dense sums over ascending k"""
    imu, s0, par, _ = od.cases()["zero_rotation"]
    assert np.all(imu[:, 2:5] == 0) and np.all(s0[10:13] == 0) and np.all(par[6:9] == 0) and np.array_equal(s0[3:7], [0, 0, 0, 1])
    got = _launch(ctx, variant, [(imu, s0)], par)[0]
    exp = od.integrate_ld(variant, imu, s0, par, dtype=np.float64)
    assert same_bits(got["delta"][3:7], [0.0, 0.0, 0.0, 1.0])
    assert np.abs(got["delta"][16:19]).max() > 0.3 and np.count_nonzero(got["cov"]) > 150  # (the case is not trivial)
    for k in KEYS:
        diff = np.flatnonzero(bits(got[k]) != bits(exp[k]))
        assert diff.size == 0, f"{k}: {diff.size} entries differ, first at flat index {diff[0]}"
    if variant == od.EARTH_ODO:
        assert same_bits(got["pn"], exp["pn"], nan_payload=True)


@pytest.mark.parametrize("variant", od.VARIANTS)
def test_result_is_independent_of_the_launch(ctx, variant):
    cs = od.cases()
    par = cs["plain"][2]
    fill = ["seven_samples", "long", "one_sample", "two_samples", "standstill"]
    spots = (0, 35, 69)
    slots = ["plain" if i in spots else fill[i % len(fill)] for i in range(70)]
    alone = _launch(ctx, variant, _named(["plain"]), par)[0]
    batch = _launch(ctx, variant, _named(slots), par)
    again = _launch(ctx, variant, _named(slots), par)
    keys = KEYS + (("pn",) if variant == od.EARTH_ODO else ())
    for i in spots:
        for k in keys:
            assert same_bits(batch[i][k], alone[k], nan_payload=True), (i, k)
    for i, (a, b) in enumerate(zip(batch, again)):
        for k in keys:
            assert same_bits(a[k], b[k], nan_payload=True), (i, slots[i], k)


# ---- P1: rows and argument checks -------------------------------------------------------------------------------------------------------
def _raw_call(ctx, variant, n, offsets, imu, s0, par, total, null=(), handle=True, with_pn=True):
    """icg_preint_odo_batch on sentinel-filled outputs; `null` names the arguments passed as NULL -> (rc, outputs)"""
    m = max(n, 1)
    bufs = dict(cur=np.full((m, 16), SENTINEL), delta=np.full((m, 20), SENTINEL), jac=np.full((m, 361), SENTINEL),
                cov=np.full((m, 361), SENTINEL), dt=np.full(m, SENTINEL), pn=np.full((max(total, 1), 4), SENTINEL))
    ins = dict(offsets=i32(offsets), imu=f64(imu), state0=f64(s0), params=f64(par))
    p = lambda name, a: None if name in null else ptr(a)
    rc = ctx.lib.icg_preint_odo_batch(ctx.h if handle else None, int(variant), int(n), p("offsets", ins["offsets"]), p("imu", ins["imu"]),
                                      p("state0", ins["state0"]), p("params", ins["params"]), p("cur", bufs["cur"]),
                                      p("delta", bufs["delta"]), p("jac", bufs["jac"]), p("cov", bufs["cov"]), p("dt", bufs["dt"]),
                                      ptr(bufs["pn"]) if with_pn else None)
    return rc, bufs


def _untouched(bufs):
    return all(np.all(bits(b) == bits(SENTINEL)) for b in bufs.values())


def test_pn_rows_written_are_exactly_the_intervals_own(ctx):
    cs = od.cases()
    par = cs["plain"][2]
    names = ["one_sample", "plain", "two_samples", "one_sample", "seven_samples", "one_sample"]
    items = _named(names)
    lens = [len(imu) for imu, _ in items]
    offsets = np.cumsum([0] + lens).astype(np.int32)
    rc, bufs = _raw_call(ctx, od.EARTH_ODO, len(items), offsets, np.concatenate([i for i, _ in items]), np.stack([s for _, s in items]), par,
                         int(offsets[-1]))
    assert rc == ICG_OK
    ref = _launch(ctx, od.EARTH_ODO, items, par)
    kept = bits(bufs["pn"]).reshape(-1, 4) == bits(SENTINEL)
    for i, n in enumerate(lens):
        b = int(offsets[i])
        assert same_bits(bufs["cur"][i], ref[i]["cur"]) and same_bits(bufs["cov"][i], ref[i]["cov"])
        assert np.all(kept[b + n - 1]), f"interval {i}: its last pn row was written"
        assert not np.any(np.all(kept[b:b + n - 1], axis=1)), f"interval {i}: a pn row of its own was left out"
        assert same_bits(bufs["pn"][b:b + n - 1], ref[i]["pn"])
        assert np.array_equal(bufs["pn"][b:b + n - 1, 0], items[i][0][1:, 1])  # (dt, position) after sample index at row begin + index - 1


def test_odo_variant_leaves_a_pn_buffer_alone_and_needs_none(ctx):
    cs = od.cases()
    par = cs["plain"][2]
    items = _named(["plain", "seven_samples"])
    offsets = np.array([0, 41, 48], np.int32)
    args = (od.ODO, 2, offsets, np.concatenate([i for i, _ in items]), np.stack([s for _, s in items]), par, 48)
    rc, with_buf = _raw_call(ctx, *args)
    assert rc == ICG_OK and np.all(bits(with_buf["pn"]) == bits(SENTINEL))
    rc, without = _raw_call(ctx, *args, with_pn=False)
    assert rc == ICG_OK
    for k in ("cur", "delta", "jac", "cov", "dt"):
        assert same_bits(with_buf[k], without[k]) and not np.any(bits(without[k]) == bits(SENTINEL)), k


def test_earth_odo_variant_without_pn_buffer(ctx):
    cs = od.cases()
    par = cs["plain"][2]
    names = ["plain", "one_sample", "seven_samples", "two_samples"]
    with_pn = _launch(ctx, od.EARTH_ODO, _named(names), par)
    without = _launch(ctx, od.EARTH_ODO, _named(names), par, want_pn=False)
    for a, b in zip(with_pn, without):
        assert b["pn"] is None
        for k in KEYS:
            assert same_bits(a[k], b[k]), k


def _three_intervals():
    imu, s0, par, _ = od.cases()["plain"]
    return np.concatenate([imu, imu]), np.stack([s0, s0, s0]), par


@pytest.mark.parametrize("variant,n", [(0, 3), (1, 3), (4, 3), (-1, 3), (2, -1), (3, -1)])
def test_bad_variant_or_count_is_refused(ctx, variant, n):
    imu, s0, par = _three_intervals()
    rc, bufs = _raw_call(ctx, variant, n, [0, 41, 61, 82], imu, s0, par, 82)
    assert rc == ICG_ERR_INVALID and _untouched(bufs)


@pytest.mark.parametrize("null", ["offsets", "imu", "state0", "params", "cur", "delta", "jac", "cov", "dt"])
@pytest.mark.parametrize("variant", od.VARIANTS)
def test_null_required_pointer_is_refused(ctx, variant, null):
    imu, s0, par = _three_intervals()
    rc, bufs = _raw_call(ctx, variant, 3, [0, 41, 61, 82], imu, s0, par, 82, null=(null,))
    assert rc == ICG_ERR_INVALID and _untouched(bufs)


def test_null_context_is_refused(ctx):
    imu, s0, par = _three_intervals()
    rc, bufs = _raw_call(ctx, od.ODO, 3, [0, 41, 61, 82], imu, s0, par, 82, handle=False)
    assert rc == ICG_ERR_INVALID and _untouched(bufs)


@pytest.mark.parametrize("offsets", [[0, 0, 41, 82], [0, 41, 41, 82], [0, 41, 82, 82]], ids=["first", "middle", "last"])
@pytest.mark.parametrize("variant", od.VARIANTS)
def test_interval_without_a_sample_is_refused(ctx, variant, offsets):
    imu, s0, par = _three_intervals()
    rc, bufs = _raw_call(ctx, variant, 3, offsets, imu, s0, par, 82)
    assert rc == ICG_ERR_INVALID and _untouched(bufs)
    assert b"no IMU sample" in ctx.lib.icg_last_error(ctx.h)


@pytest.mark.parametrize("variant", od.VARIANTS)
def test_no_interval_is_ok_and_touches_nothing(ctx, variant):
    imu, s0, par = _three_intervals()
    rc, bufs = _raw_call(ctx, variant, 0, [0], imu, s0, par, 82)
    assert rc == ICG_OK and _untouched(bufs)


# ---- P2 -----------------------------------------------------------------------------------------------------------------------------------
def _bound(exp):
    fin = np.abs(exp[np.isfinite(exp)])
    return 1e-6 * max(1.0, fin.max() if fin.size else 0.0)


def _err(got, exp):
    """max |got - exp| over the entries where exp is finite; got must be NaN exactly where exp is NaN"""
    got, exp = np.asarray(got), np.asarray(exp)
    assert np.array_equal(np.isnan(got), np.isnan(exp))
    m = np.isfinite(exp)
    return float(np.abs(got[m] - exp[m]).max()) if m.any() else 0.0


def _eval_golden(ctx, results, want_jac=True):
    """icg_preint_odo_evaluate_batch on the goldens' own integration results (one variant) at their evaluation points"""
    v = results[0]["variant"]
    pn_off = np.cumsum([0] + [len(g["pn"]) for g in results]).astype(np.int32)
    pn = np.concatenate([g["pn"].reshape(-1, 4) for g in results]) if pn_off[-1] > 0 else np.zeros((1, 4))
    env = np.stack([np.concatenate([g["par25"][5:6], g["iewn"]]) for g in results])
    earth = v == od.EARTH_ODO
    return ctx.preint_odo_evaluate_batch(v, np.stack([g["delta"] for g in results]), np.stack([g["jac"].reshape(361) for g in results]),
                                         np.stack([g["cov"].reshape(361) for g in results]), np.array([g["dt"] for g in results]), env,
                                         np.stack([g["point"] for g in results]), pn_off if earth else None, pn if earth else None,
                                         want_jac=want_jac)


@pytest.mark.parametrize("variant", od.VARIANTS)
def test_p2_matches_the_reference_on_the_golden_integration(ctx, variant):
    results = [g for g in od.golden() if g["variant"] == variant]
    res, J, S, status = _eval_golden(ctx, results)
    assert np.all(status == 0)
    worst = 0.0
    for i, g in enumerate(results):
        er, eJ = _err(res[i], g["r"]), _err(J[i], g["J"])
        print(f"GPUFIG P2 vs reference, variant {variant} {g['case']}: r {er:.3e} (bound {_bound(g['r']):.3e})  J {eJ:.3e} (bound {_bound(g['J']):.3e})")
        worst = max(worst, er / _bound(g["r"]), eJ / _bound(g["J"]))
    print(f"GPUFIG P2 vs reference, variant {variant}: worst error / bound {worst:.3e}")
    for i, g in enumerate(results):
        assert _err(res[i], g["r"]) < _bound(g["r"]) and _err(J[i], g["J"]) < _bound(g["J"]), g["case"]
    # residual-only call: the same residual bytes
    res_only, J_none, _, status2 = _eval_golden(ctx, results, want_jac=False)
    assert J_none is None and np.array_equal(status, status2)
    assert same_bits(res_only, res, nan_payload=True)


@pytest.mark.parametrize("variant", od.VARIANTS)
def test_p2_alone_and_in_a_batch_of_70(ctx, variant):
    results = [g for g in od.golden() if g["variant"] == variant]
    plain = next(g for g in results if g["case"] == "plain")
    alone = _eval_golden(ctx, [plain])
    spots = (0, 35, 69)
    batch = [plain if i in spots else results[i % len(results)] for i in range(70)]
    out = _eval_golden(ctx, batch)
    for i in spots:
        for a, b in zip(alone[:3], out[:3]):
            assert same_bits(a[0], b[i], nan_payload=True), i
        assert out[3][i] == 0


def _device_entry(hostlib, variant, items, par19, points):
    """icgh_backend_preint_odo_device: device P1, then host and device P2 on the same objects"""
    n = len(items)
    lens = [len(imu) for imu, _ in items]
    offsets = np.cumsum([0] + lens).astype(np.int32)
    imu, s0, pts = f64(np.concatenate([i for i, _ in items])), f64(np.stack([s for _, s in items])), f64(np.stack(points))
    o = dict(cur=np.zeros((n, 16)), rh=np.full((n, 19), SENTINEL), Jh=np.full((n, 646), SENTINEL), rd=np.full((n, 19), SENTINEL),
             Jd=np.full((n, 646), SENTINEL), Sh=np.full((n, 361), SENTINEL), Sd=np.full((n, 361), SENTINEL), okh=np.full(n, -1, np.int32),
             okd=np.full(n, -1, np.int32))
    err = ErrBuf()
    rc = hostlib.icgh_backend_preint_odo_device(int(variant), n, ptr(offsets), ptr(imu), ptr(s0), ptr(f64(par19)), ptr(pts), ptr(o["cur"]),
                                                ptr(o["rh"]), ptr(o["Jh"]), ptr(o["rd"]), ptr(o["Jd"]), ptr(o["Sh"]), ptr(o["Sd"]),
                                                ptr(o["okh"]), ptr(o["okd"]), *err.args)
    assert rc == 0, err.text()
    return o


@pytest.mark.parametrize("variant", od.VARIANTS)
def test_p2_device_against_host_on_the_same_objects(ctx, hostlib, variant):
    cs = od.cases()
    names = ["plain", "two_samples", "three_samples", "standstill", "long", "seven_samples"]
    par, abv = cs["plain"][2], cs["plain"][3]
    items = _named(names)
    p1 = _launch(ctx, variant, items, par)
    points = [od.eval_point(s0, p1[i]["cur"]) for i, (_, s0) in enumerate(items)]
    o = _device_entry(hostlib, variant, items, od.params19(par, abv), points)
    assert np.all(o["okh"] == 1) and np.all(o["okd"] == 1)
    for i, name in enumerate(names):
        assert same_bits(o["cur"][i], p1[i]["cur"])
        diff = np.flatnonzero(~((bits(o["Sd"][i]) == bits(o["Sh"][i])) | (np.isnan(o["Sd"][i]) & np.isnan(o["Sh"][i]))))
        assert diff.size == 0, f"{name}: S differs in {diff.size} entries, first at {diff[0]}"
        er, eJ = _err(o["rd"][i], o["rh"][i]), _err(o["Jd"][i], o["Jh"][i])
        print(f"GPUFIG P2 device vs host, variant {variant} {name}: r {er:.3e} (bound {_bound(o['rh'][i]):.3e})  J {eJ:.3e} (bound {_bound(o['Jh'][i]):.3e})")
        assert er < _bound(o["rh"][i]) and eJ < _bound(o["Jh"][i]), name
    assert np.all(np.isfinite(o["rh"][0])) and np.abs(o["rh"][0]).max() > 0


@pytest.mark.parametrize("variant", od.VARIANTS)
def test_p2_singular_covariance_gives_zero_rows_on_both_sides(ctx, hostlib, variant):
    cs = od.cases()
    par, abv = cs["plain"][2].copy(), cs["plain"][3]
    par[12] = 0.0  # odo_srw = 0: the scale factor's row and column of the covariance are zero
    items = _named(["plain", "seven_samples"])
    p1 = _launch(ctx, variant, items, par)
    assert all(np.all(p["cov"][18] == 0) and np.all(p["cov"][:, 18] == 0) for p in p1)
    points = [od.eval_point(s0, p1[i]["cur"]) for i, (_, s0) in enumerate(items)]
    o = _device_entry(hostlib, variant, items, od.params19(par, abv), points)
    assert np.all(o["okh"] == 0) and np.all(o["okd"] == 0)
    for k in ("rh", "Jh", "rd", "Jd", "Sh", "Sd"):
        assert np.all(bits(o[k]) == 0), k
    # the C entry itself: status 1, zero rows
    pn_off = np.cumsum([0] + [len(i) - 1 for i, _ in items]).astype(np.int32)
    earth = variant == od.EARTH_ODO
    res, J, S, status = ctx.preint_odo_evaluate_batch(variant, np.stack([p["delta"] for p in p1]), np.stack([p["jac"].reshape(361) for p in p1]),
                                                      np.stack([p["cov"].reshape(361) for p in p1]), np.array([p["dt"] for p in p1]),
                                                      np.tile(par[5:9], (2, 1)), np.stack(points), pn_off if earth else None,
                                                      np.concatenate([p["pn"] for p in p1]) if earth else None)
    assert np.all(status == 1) and np.all(bits(res) == 0) and np.all(bits(J) == 0) and np.all(bits(S) == 0)


def _raw_eval(ctx, variant, n, g, null=(), handle=True, pn_off=None):
    bufs = dict(r=np.full((max(n, 1), 19), SENTINEL), J=np.full((max(n, 1), 646), SENTINEL), S=np.full((max(n, 1), 361), SENTINEL),
                status=np.full(max(n, 1), -7, np.int32))
    m = max(n, 1)
    ins = dict(delta=f64(np.tile(g["delta"], (m, 1))), jac=f64(np.tile(g["jac"].reshape(361), (m, 1))), cov=f64(np.tile(g["cov"].reshape(361), (m, 1))),
               dt=f64(np.full(m, g["dt"])), env=f64(np.tile(np.concatenate([g["par25"][5:6], g["iewn"]]), (m, 1))), points=f64(np.tile(g["point"], (m, 1))),
               pn_off=i32(np.arange(m + 1) * len(g["pn"]) if pn_off is None else pn_off), pn=f64(np.tile(g["pn"].reshape(-1, 4), (m, 1))))
    p = lambda name, a: None if name in null else ptr(a)
    rc = ctx.lib.icg_preint_odo_evaluate_batch(ctx.h if handle else None, int(variant), int(n), p("delta", ins["delta"]), p("jac", ins["jac"]),
                                               p("cov", ins["cov"]), p("dt", ins["dt"]), p("env", ins["env"]), p("pn_off", ins["pn_off"]),
                                               p("pn", ins["pn"]), p("points", ins["points"]), p("r", bufs["r"]), p("J", bufs["J"]),
                                               p("S", bufs["S"]), p("status", bufs["status"]))
    return rc, bufs


def _eval_untouched(bufs):
    return all(np.all(bits(bufs[k]) == bits(SENTINEL)) for k in ("r", "J", "S")) and np.all(bufs["status"] == -7)


def test_p2_refusals_launch_nothing(ctx):
    g = next(g for g in od.golden() if g["variant"] == od.EARTH_ODO and g["case"] == "plain")
    rc, bufs = _raw_eval(ctx, od.EARTH_ODO, 2, g)
    assert rc == ICG_OK and np.all(bufs["status"] == 0) and same_bits(bufs["r"][0], bufs["r"][1])
    for variant in (0, 1, 4):
        rc, bufs = _raw_eval(ctx, variant, 2, g)
        assert rc == ICG_ERR_INVALID and _eval_untouched(bufs), variant
    for n in (0, -1):
        rc, bufs = _raw_eval(ctx, od.EARTH_ODO, n, g)
        assert rc == ICG_ERR_INVALID and _eval_untouched(bufs), n
    for null in ("delta", "jac", "cov", "dt", "env", "points", "r", "status", "pn_off", "pn"):
        rc, bufs = _raw_eval(ctx, od.EARTH_ODO, 2, g, null=(null,))
        assert rc == ICG_ERR_INVALID and _eval_untouched(bufs), null
    rc, bufs = _raw_eval(ctx, od.EARTH_ODO, 2, g, pn_off=[0, 40, 20])
    assert rc == ICG_ERR_INVALID and _eval_untouched(bufs)
    rc, bufs = _raw_eval(ctx, od.EARTH_ODO, 2, g, handle=False)
    assert rc == ICG_ERR_INVALID and _eval_untouched(bufs)
    # the Odo variant needs neither pn_offsets nor pn, and the Jacobians and S are optional
    g2 = next(g for g in od.golden() if g["variant"] == od.ODO and g["case"] == "plain")
    rc, bufs = _raw_eval(ctx, od.ODO, 2, g2, null=("pn_off", "pn", "J", "S"))
    assert rc == ICG_OK and np.all(bufs["status"] == 0) and _err(bufs["r"][1], g2["r"]) < _bound(g2["r"])
    assert np.all(bits(bufs["J"]) == bits(SENTINEL)) and np.all(bits(bufs["S"]) == bits(SENTINEL))


def test_context_still_integrates_after_refusals(ctx):
    imu, s0, par, _ = od.cases()["plain"]
    for variant in od.VARIANTS:
        got = _launch(ctx, variant, [(imu, s0)], par)[0]
        exp = od.reference(variant, "plain")
        od.check_result(got, dict(exp, pn=exp["pn"] if variant == od.EARTH_ODO else None), len(imu), f"after refused calls, variant {variant}")
