"""The CPU oracle's preintegration inner loop (orc_preint_integrate, the line-by-line twin of k_preint) at the edges of tests/preint_edge_data.py,
judged per 3x3 block / per state field (block_rel, field_rel) against the extended-precision restatement integrate_ld and against the
REFERENCE's own code (tests/golden/preint_edge_ref_golden.npz).  TOL = 1e-12 throughout.

Measured maxima, oracle against integrate_ld (worst of jac / cov per block, cur / delta per field, pn), both variants:
    41-sample cases    jac 8.5e-16   cov 1.5e-15   cur 1.2e-15   delta 5.9e-16   pn 8.6e-16
      (plain, zero_rotation, alternating_zero_rotation, dt_zero_sample, jitter_dt, non_unit_q0, negated_q0, short_corr_time,
       corr_time_below_dt, large_bias, and plain at the zero / tilted / amplified Earth rates; zero_noise: cov exactly 0)
    long (401 samples, also at the three Earth rates)
                       jac 1.0e-14   cov 8.5e-15   cur 2.2e-15   delta 1.1e-15   pn 1.2e-15
    two_samples        jac 9.6e-17   cov 4.3e-16   cur 1.4e-16   delta 1.9e-16   pn 5.4e-17
    one_sample         everything exact
The worst figure (1.0e-14) leaves a factor 100 to TOL."""
import os

import numpy as np
import pytest

import preint_edge_data as ed

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden", "preint_edge_ref_golden.npz")
REF_PREINT_SO = os.path.join(ROOT, "oracle", "_ref", "libref_preint.so")
CASES = [(v, name) for v in (0, 1) for name in ed.cases(v)]


def _bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


@pytest.mark.parametrize("variant,name", CASES)
def test_oracle_matches_long_double_reference(oracle, variant, name):
    imu, s0, par = ed.cases(variant)[name]
    got = oracle.preint_integrate(variant, imu, s0, par)
    exp = dict(ed.reference(variant, name))
    if variant == 0:
        got.pop("pn"), exp.pop("pn")  # the Normal variant keeps no pn list
    fig = ed.check_result(got, exp, len(imu), f"variant {variant} {name}")
    print(f"variant {variant} {name}: " + "  ".join(f"{k} {v:.1e}" for k, v in fig.items()))
    for k in ("cur", "delta", "jac", "cov"):
        assert np.all(np.isfinite(got[k]))


@pytest.mark.parametrize("variant", [0, 1])
def test_inputs_reach_their_edges(oracle, variant):
    cs = ed.cases(variant)
    # zero_rotation: every rotvec2quat argument is exactly zero, so the rotation is never touched
    imu, s0, par = cs["zero_rotation"]
    assert np.all(imu[:, 2:5] == 0.0) and np.all(s0[10:13] == 0.0) and np.any(s0[13:16] != 0.0) and np.any(imu[:, 5:8] != 0.0)
    if variant == 1:
        assert np.all(par[6:9] == 0.0)
    zr = oracle.preint_integrate(variant, imu, s0, par)
    assert np.array_equal(_bits(zr["delta"][3:7]), _bits([0.0, 0.0, 0.0, 1.0]))
    assert np.array_equal(_bits(zr["cur"][3:7]), _bits(s0[3:7]))
    imu = cs["alternating_zero_rotation"][0]
    assert np.all(imu[1::2, 2:5] == 0.0) and np.all(np.abs(imu[0::2, 2:5]).max(axis=1) > 0.0)
    imu = cs["dt_zero_sample"][0]
    assert np.all(imu[7, 1:8] == 0.0) and np.all(np.delete(imu[:, 1], 7) > 0.0)
    dts = cs["jitter_dt"][0][:, 1]
    assert dts.min() < 0.8 / 200.0 and dts.max() > 1.2 / 200.0 and len(np.unique(dts)) == len(dts)
    q0 = cs["non_unit_q0"][1][3:7]
    assert abs(np.linalg.norm(q0) - 1.3) < 1e-12
    assert np.array_equal(cs["negated_q0"][1][3:7], -cs["plain"][1][3:7])
    for name, decay in (("short_corr_time", 0.99), ("corr_time_below_dt", -0.25)):
        imu, _, par = cs[name]
        assert np.allclose(1 - imu[1:, 1] / par[4], decay, rtol=0, atol=1e-12)
    assert np.all(1 - cs["corr_time_below_dt"][0][1:, 1] / cs["corr_time_below_dt"][2][4] < 0)  # the decay is negative
    imu, s0, par = cs["zero_noise"]
    assert np.all(par[0:4] == 0.0)
    assert np.all(oracle.preint_integrate(variant, imu, s0, par)["cov"] == 0.0)
    assert np.all(np.asarray(ed.reference(variant, "zero_noise")["cov"]) == 0)
    assert [len(cs[n][0]) for n in ("long", "two_samples", "one_sample")] == [401, 2, 1]
    # plain: the covariance blocks span orders of magnitude, which is the reason for the block measure
    cov = np.asarray(ed.reference(variant, "plain")["cov"], np.float64)
    diag = [np.abs(cov[3 * i:3 * i + 3, 3 * i:3 * i + 3]).max() for i in range(5)]
    assert min(diag) < 1e-4 * np.abs(cov).max()
    if variant == 1:
        # amplified: the Earth rate is a first-order effect on the navigation state
        nominal, amplified = ed.reference(1, "plain"), ed.reference(1, "plain@amplified")
        assert float(np.abs(amplified["cur"] - nominal["cur"]).max()) > 1e-3
        assert np.count_nonzero(ed.EARTH_RATES["amplified"]) == 3 and np.count_nonzero(ed.EARTH_RATES["tilted"]) == 2


@pytest.mark.parametrize("variant", [0, 1])
def test_block_measure_sees_what_the_whole_array_measure_misses(variant):
    imu, s0, par = ed.cases(variant)["plain"]
    ref = ed.reference(variant, "plain")
    mut = ed.integrate_ld(variant, imu, s0, par, mutate="decay_cov")
    whole, (block, where) = ed.whole_rel(mut["cov"], ref["cov"]), ed.block_rel(mut["cov"], ref["cov"])
    print(f"decay_cov: whole {whole:.2e}, block {block:.2e} at {where}")  # 2.8e-9 and 5.6e-5 (ba-ba)
    assert whole < 1e-8   # under the bound the older tests put on the covariance
    assert block > 1e-6
    assert where in ("bg-bg", "ba-ba")
    assert ed.block_rel(mut["jac"], ref["jac"])[0] == 0.0  # the mutants touch the covariance update only
    mut = ed.integrate_ld(variant, imu, s0, par, mutate="no_att_bg_cov")
    block, where = ed.block_rel(mut["cov"], ref["cov"])
    print(f"no_att_bg_cov: whole {ed.whole_rel(mut['cov'], ref['cov']):.2e}, block {block:.2e} at {where}")  # 1.2e-6 and 1.0 (p-bg)
    assert block > 1e-2


def test_measures_on_known_arrays():
    a = np.zeros((15, 15))
    a[0:3, 0:3] = 1.0
    a[9:12, 9:12] = 1e-7
    b = a.copy()
    b[10, 10] *= 1 + 1e-3
    assert ed.whole_rel(b, a) == pytest.approx(1e-10, rel=1e-3)
    val, where = ed.block_rel(b, a)
    assert where == "bg-bg" and val == pytest.approx(1e-3, rel=1e-3)
    b = a.copy()
    b[14, 0] = 1e-300  # a block that is all zero in the reference must be all zero
    assert ed.block_rel(b, a) == (float("inf"), "ba-p")
    b[14, 0] = -0.0
    assert ed.block_rel(b, a)[0] == 0.0
    s = np.arange(1.0, 17.0)
    t = s.copy()
    t[8] += 1e-8
    assert ed.field_rel(t, s) == (pytest.approx(1e-9, rel=1e-3), "v")
    t = s.copy()
    t[15] = np.nextafter(t[15], 100.0)  # bg / ba: bits
    assert ed.field_rel(t, s) == (float("inf"), "ba")


# ---- the reference's own code -------------------------------------------------------------------------------------------------------
def edge_golden_results():
    g = np.load(GOLDEN)
    for k in range(int(g["n_results"])):
        name, variant = str(g[f"r{k}_case"]), int(g[f"r{k}_variant"])
        c = {key: g[f"r{k}_{key}"] for key in ("station", "iewn", "cur", "delta", "jac", "cov", "dt")}
        c.update(case=name, variant=variant, imu=g[f"in_{name}_imu"], s0=g[f"in_{name}_s0"], params=g[f"in_{name}_params"].copy())
        if variant == 1:
            c["params"][6:9] = c["iewn"]  # the Earth rate the reference derived from its station
        yield k, c


def test_edge_golden_inputs_are_the_cases():
    g = np.load(GOLDEN)
    assert list(g["case_names"]) == list(ed.BASE_NAMES)
    for name, (imu, s0, par) in ed.cases(0).items():
        assert np.array_equal(_bits(g[f"in_{name}_imu"]), _bits(imu)), name
        assert np.array_equal(_bits(g[f"in_{name}_s0"]), _bits(s0)) and np.array_equal(_bits(g[f"in_{name}_params"]), _bits(par)), name
    seen = {(c["variant"], c["case"], bool(np.any(c["station"] != 0))) for _, c in edge_golden_results()}
    want = {(v, n, False) for v in (0, 1) for n in ed.BASE_NAMES} | {(1, "plain", True), (1, "long", True)}
    assert seen == want
    # with station (0, 0, 0) the reference's rate is the nominal one of preint_data.PARAMS up to the latitude of p0 (metres from the
    # equator); STATION gives a tilted rate
    for _, c in edge_golden_results():
        if c["variant"] == 1:
            tilt = abs(c["iewn"][2]) / np.linalg.norm(c["iewn"])
            assert tilt > 0.3 if np.any(c["station"] != 0) else tilt < 1e-6


def test_oracle_and_long_double_reference_match_reference_golden(oracle):
    n = 0
    for k, c in edge_golden_results():
        v, what = c["variant"], f"golden result {k} (variant {c['variant']} {c['case']})"
        exp = {key: c[key] for key in ("cur", "delta", "jac", "cov")}
        exp["dt"] = float(c["dt"])
        got = oracle.preint_integrate(v, c["imu"], c["s0"], c["params"])
        got.pop("pn")
        ed.check_result(got, exp, len(c["imu"]), "oracle vs " + what)
        ld = ed.integrate_ld(v, c["imu"], c["s0"], c["params"])
        ld64 = {key: np.asarray(ld[key], np.float64) for key in ("cur", "delta", "jac", "cov")}
        ld64["dt"] = float(ld["dt"])
        ed.check_result(ld64, exp, len(c["imu"]), "integrate_ld vs " + what)
        n += 1
    assert n == 2 * len(ed.BASE_NAMES) + 2


@pytest.mark.skipif(not os.path.exists(REF_PREINT_SO), reason="oracle/_ref not built (needs the reference's sources)")
def test_edge_golden_is_current():
    """the generator, run on the reference library built here, reproduces the committed file: same keys, equal values"""
    import ctypes as C
    import sys
    sys.path.insert(0, os.path.join(ROOT, "tests", "golden"))
    import make_preint_edge_golden as gen
    fresh, g = gen.build(C.CDLL(REF_PREINT_SO)), np.load(GOLDEN)
    assert sorted(fresh) == sorted(g.files)
    for key in g.files:
        assert np.array_equal(np.asarray(fresh[key]), g[key]), key
