"""M4 on the device (icg_marg_prior_set / icg_marg_prior_evaluate): what can be checked without a GPU — the entry points are declared,
exported and bound, the host library exports the comparison entry, a build of the host layer WITHOUT the device entry points (the
oracle-backed checker library) still loads and refuses the device mode instead of computing on the CPU, and the host evaluation that
MarginalizationFactor::Evaluate was refactored into (evaluateMargPrior) equals the oracle bit for bit."""
import ctypes as C
import os
import re

import numpy as np

import marg_factor_data as mf
from ctypes_util import same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_points_are_declared_exported_and_bound():
    import harness
    import icgvins
    txt = open(os.path.join(ROOT, "include", "icgvins_hip.h")).read()
    assert txt.count("factors/marginalization_factor.h:47-101") >= 2  # each entry cites the reference interface it replaces
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = icgvins.load_library()
    for name in ("icg_marg_prior_set", "icg_marg_prior_evaluate"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", txt), name
        assert hasattr(lib, name), name
        assert name in icgvins.EXPORTS, name
    assert hasattr(icgvins.Context, "marg_prior_set") and hasattr(icgvins.Context, "marg_prior_evaluate")
    m = re.search(r"#define\s+ICG_MARG_MAX_R\s+(\d+)", txt)
    assert m and int(m.group(1)) == icgvins.MARG_MAX_R >= 512
    assert hasattr(C.CDLL(harness.HOST_LIB), "icgh_backend_marg_factor")


def _oracle_host():
    from stream_utils import ORACLE_HOST
    lib = C.CDLL(ORACLE_HOST)
    assert hasattr(lib, "icgh_backend_marg_factor")
    return lib


def test_host_layer_without_the_entry_points_loads_and_refuses():
    """oracle/libicgvins_host_oracle.so is the host layer on a C ABI implementation that defines neither entry: it must still load (ctypes
    binds every symbol at load time) and the device mode must fail by name, leaving every output untouched."""
    lib = _oracle_host()
    priors, points = mf.batch()
    mark = -7.25
    rc, msg, res, jac, grad, sq, sec = mf.backend_marg_factor(lib, 1, priors, [points], mark=mark)
    assert rc != 0
    assert "icg_marg_prior_set is not in this build" in msg
    for a in (res, jac, grad, sq, sec):
        assert np.all(a == mark)


def test_host_evaluation_equals_the_oracle_bit_for_bit():
    """mode 0 (evaluateMargPrior on the host pool) on the heterogeneous batch: residuals and Jacobian blocks are the oracle's bits;
    gradient and squared norm are the bits of the plain sequential sums"""
    import oracle_lib
    orc = oracle_lib.load()
    lib = _oracle_host()
    priors, points = mf.batch()
    rc, msg, res, jac, grad, sq, _ = mf.backend_marg_factor(lib, 0, priors, [points], host_threads=3)
    assert rc == 0, msg
    res_w, jac_w, grad_w = mf.split(priors, res[0], "r"), mf.split(priors, jac[0], "jac"), mf.split(priors, grad[0], "r")
    for w, (p, x) in enumerate(zip(priors, points)):
        e, J = orc.marg_factor_eval(p["size"], p["index"], p["x0"], x, p["J0"], p["e0"])
        assert same_bits(res_w[w], e), w
        assert same_bits(jac_w[w], J), w
        assert same_bits(grad_w[w], mf.sequential_gradient(p["J0"], e)), w
        assert same_bits(sq[0, w], mf.sequential_sq_norm(e)), w
    # without the optional outputs the residuals are the same
    rc, msg, res2, jac2, grad2, sq2, _ = mf.backend_marg_factor(lib, 0, priors, [points], want=(False, False, False))
    assert rc == 0 and jac2 is None and grad2 is None and sq2 is None
    assert same_bits(res2, res)


def test_host_entry_rejects_an_invalid_prior():
    lib = _oracle_host()
    p = mf.make_prior([7, 1], 5)
    bad = dict(p, index=np.array([0, 7], np.int32))  # index + local > r
    rc, msg, res, *_ = mf.backend_marg_factor(lib, 0, [bad], [[mf.make_x(p, 1)]], mark=3.5)
    assert rc != 0 and "window 0" in msg and np.all(res == 3.5)
