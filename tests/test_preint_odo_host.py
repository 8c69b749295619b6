"""CPU checks of the odometer preintegration (Odo, EarthOdo; 19-wide state) that need no device:
  * the extended-precision restatement preint_odo_data.integrate_ld against the reference golden (tests/golden/preint_odo_ref_golden.npz,
    PreintegrationOdo / PreintegrationEarthOdo themselves), per block and per field at TOL = 1e-12;
  * the host P2 (PreintegrationOdo::evaluate behind PreintegrationOdoFactor), fed the golden's own integration result through
    icgh_backend_preint_odo_eval_given, against the golden's residuals and Jacobians at the project's P2 rule 1e-6 x max(1, max|expected|)
    (tests/test_gpu_preint_eval.py), measured maximum printed, and at least 10x inside it;
  * a singular covariance (odo_srw = 0) makes evaluate() return false with the rows untouched; block sizes {7, 10, 7, 10}, 19 residuals.

The 2- and 3-sample intervals have a covariance whose inverse is not positive definite (one or two integration steps leave the position
block rank deficient): the reference itself returns NaN there (the Cholesky step takes the root of a negative number), and so does the
host.  As in tests/test_gpu_preint_eval.py the comparison is NaN-aware: got must be NaN exactly where expected is, every other entry is held
to the bound.

Measured here: integrate_ld against the golden, worst block / field over all 14 results: jac 1.6e-15, cov 8.2e-15, cur 1.3e-15,
delta 2.0e-14 (s of `standstill`, a distance of 1e-2 m), pn 6.5e-16.  Host P2 against the golden: 0 on every finite entry (the host's
inversion and Cholesky are the arithmetic of the reference build's linear algebra)."""
import ctypes as C

import numpy as np
import pytest

import preint_odo_data as od
from ctypes_util import ErrBuf, f64, ptr, ptr_or_null

SENTINEL = -1.2345e300
GOLDEN = list(range(14))


@pytest.fixture(scope="module")
def hostlib():
    import harness
    lib = C.CDLL(harness.HOST_LIB)
    lib.icgh_backend_preint_odo_eval_given.argtypes = ([C.c_int] + [C.c_void_p] * 4 + [C.c_double, C.c_void_p, C.c_int] + [C.c_void_p] * 6
                                                       + [C.c_char_p, C.c_int])
    return lib


def eval_given(lib, g, par25=None, delta=None):
    """icgh_backend_preint_odo_eval_given on a golden result's integration -> (rc, r 19, J 646, S 361, block sizes + residual count)"""
    r, J, S, bs = np.full(19, SENTINEL), np.full(646, SENTINEL), np.zeros(361), np.zeros(5, np.int32)
    err = ErrBuf()
    par19 = f64(od.params19(g["par25"] if par25 is None else par25, g["abv"]))
    rc = lib.icgh_backend_preint_odo_eval_given(g["variant"], ptr(par19), ptr(f64(g["delta"] if delta is None else delta)), ptr(f64(g["jac"])),
                                                ptr(f64(g["cov"])), g["dt"], ptr_or_null(f64(g["pn"])), len(g["pn"]), ptr(f64(g["iewn"])),
                                                ptr(f64(g["point"])), ptr(r), ptr(J), ptr(S), ptr(bs), *err.args)
    assert rc >= 0, err.text()
    return rc, r, J, S, bs


def test_golden_holds_the_issue_s_cases():
    res = od.golden()
    assert len(res) == len(GOLDEN)
    have = {(g["case"], g["variant"], bool(np.any(g["station"] != 0))) for g in res}
    for v in od.VARIANTS:
        for name in od.GOLDEN_NAMES:
            assert (name, v, False) in have
    assert ("plain", od.EARTH_ODO, True) in have and ("long", od.EARTH_ODO, True) in have
    cs = od.cases()
    for g in res:
        imu, s0, par25, abv = cs[g["case"]]
        # the stored inputs are the module's (the stored Earth rate is the reference's own)
        assert np.array_equal(g["imu"], imu) and np.array_equal(g["s0"], s0) and np.array_equal(g["abv"], abv)
        assert np.array_equal(np.delete(g["par25"], [6, 7, 8]), np.delete(par25, [6, 7, 8]))
        assert np.all(par25[9:13] > 0)
    assert len(cs["plain"][0]) == 41 and len(cs["long"][0]) == 201 and len(cs["two_samples"][0]) == 2
    assert np.all(cs["standstill"][0][:, 8] == 0) and np.ptp(cs["plain"][0][:, 8]) > 0
    assert np.all(cs["no_lever"][2][22:25] == 0) and np.all(cs["no_lever"][3] == 0) and np.all(cs["plain"][2][22:25] != 0)


@pytest.mark.parametrize("k", GOLDEN)
def test_integrate_ld_matches_the_reference(k):
    g = od.golden()[k]
    ld = od.integrate_ld(g["variant"], g["imu"], g["s0"], g["par25"])
    got = {key: np.asarray(ld[key], np.float64) for key in ("cur", "delta", "jac", "cov", "dt")}
    got["pn"] = np.asarray(ld["pn"], np.float64) if g["variant"] == od.EARTH_ODO else None
    exp = dict(g, pn=g["pn"] if g["variant"] == od.EARTH_ODO else None)
    fig = od.figures(got, exp)
    print(f"FIG integrate_ld vs reference, variant {g['variant']} {g['case']}: " + "  ".join(f"{q} {v:.1e} ({w})" for q, (v, w) in fig.items()))
    od.check_result(got, exp, len(g["imu"]), f"integrate_ld vs reference, variant {g['variant']} {g['case']}")
    # at a standstill s moves by the lever-arm term only: |lodo| x the rotation of the interval (0.6 m x 0.04 rad), not the 0.6 m driven in `plain`
    if g["case"] == "standstill":
        assert 0 < np.abs(g["delta"][16:19]).max() < 0.05
    if g["case"] == "plain":
        assert np.abs(g["delta"][16:19]).max() > 0.3
    assert g["delta"][19] == g["s0"][16]


def test_float64_restatement_agrees_with_the_extended_one():
    imu, s0, par25, _ = od.cases()["plain"]
    for v in od.VARIANTS:
        od.check_result({k: a for k, a in od.integrate_ld(v, imu, s0, par25, dtype=np.float64).items()}, od.reference(v, "plain"), len(imu),
                        f"float64 restatement, variant {v}")


def _bound(exp):
    fin = np.abs(exp[np.isfinite(exp)])
    return 1e-6 * max(1.0, fin.max() if fin.size else 0.0)


def _err(got, exp):
    """max |got - exp| over the entries where exp is finite; got must be NaN exactly where exp is NaN"""
    assert np.array_equal(np.isnan(got), np.isnan(exp))
    m = np.isfinite(exp)
    return float(np.abs(got[m] - exp[m]).max()) if m.any() else 0.0


@pytest.mark.parametrize("k", GOLDEN)
def test_host_p2_matches_the_reference_on_the_golden_integration(hostlib, k):
    g = od.golden()[k]
    rc, r, J, S, bs = eval_given(hostlib, g)
    assert rc == 1
    er, eJ = _err(r, g["r"]), _err(J, g["J"])
    print(f"FIG host P2 vs reference, variant {g['variant']} {g['case']}: r {er:.3e} (bound {_bound(g['r']):.3e})  J {eJ:.3e} (bound {_bound(g['J']):.3e})"
          f"  finite {int(np.isfinite(g['r']).sum())}/19")
    assert er < _bound(g["r"]) and eJ < _bound(g["J"])
    # (the generator's docstring: the noise parameters stay as they are while the host sits 10x inside the bound)
    assert 10 * er < _bound(g["r"]) and 10 * eJ < _bound(g["J"])
    if len(g["imu"]) >= 41:
        assert np.all(np.isfinite(g["r"])) and np.all(np.isfinite(g["J"])) and np.abs(g["r"]).max() > 0
        # S is upper triangular with a positive diagonal, and S^T S inverts the covariance
        S = S.reshape(19, 19)
        assert np.all(np.tril(S, -1) == 0) and np.all(np.diag(S) > 0)
        SL, PL = S.astype(np.longdouble), g["cov"].astype(np.longdouble)
        assert np.abs(SL @ PL @ SL.T - np.eye(19)).max() < 1e-4


@pytest.mark.parametrize("variant", od.VARIANTS)
def test_block_sizes_and_residual_count(hostlib, variant):
    g = next(g for g in od.golden() if g["variant"] == variant and g["case"] == "plain")
    _, r, J, _, bs = eval_given(hostlib, g)
    assert list(bs) == [7, 10, 7, 10, 19]
    assert not np.any(r == SENTINEL) and not np.any(J == SENTINEL)  # 19 residuals and 19 x (7 + 10 + 7 + 10) Jacobian entries were written


@pytest.mark.parametrize("variant", od.VARIANTS)
def test_sodo_of_the_evaluation_point_is_mix9(hostlib, variant):
    """the last residual is sodo1 - sodo0 whitened: with mix1[9] = mix0[9] it is exactly zero (S is upper triangular)"""
    g = dict(next(g for g in od.golden() if g["variant"] == variant and g["case"] == "plain"))
    g["point"] = g["point"].copy()
    g["point"][33] = g["point"][16]
    rc, r, _, _, _ = eval_given(hostlib, g)
    assert rc == 1 and r[18] == 0.0 and np.all(r[:18] != 0.0)


@pytest.mark.parametrize("variant", od.VARIANTS)
def test_singular_covariance_is_refused_with_rows_untouched(hostlib, variant):
    """odo_srw = 0: the scale factor's row and column of the covariance are zero, the inversion meets a zero pivot"""
    imu, s0, par25, abv = od.cases()["plain"]
    par = par25.copy()
    par[12] = 0.0
    ld = od.integrate_ld(variant, imu, s0, par, dtype=np.float64)
    assert np.all(ld["cov"][18] == 0) and np.all(ld["cov"][:, 18] == 0) and np.abs(ld["cov"][:18, :18]).max() > 0
    g = dict(variant=variant, par25=par, abv=abv, delta=ld["delta"], jac=ld["jac"], cov=ld["cov"], dt=float(ld["dt"]),
             pn=ld["pn"] if variant == od.EARTH_ODO else np.zeros((0, 4)), iewn=par[6:9], point=od.eval_point(s0, ld["cur"]))
    rc, r, J, S, _ = eval_given(hostlib, g)
    assert rc == 0
    assert np.all(r == SENTINEL) and np.all(J == SENTINEL) and np.all(S == 0)
