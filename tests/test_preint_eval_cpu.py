"""P2 on the device (icg_preint_evaluate_batch): what can be checked without a GPU — the entry point is declared, exported and bound, the
host library exports the comparison entry, and a build of the host layer WITHOUT the device entry point (the oracle-backed checker library)
still loads and refuses to evaluate instead of computing on the CPU."""
import ctypes as C
import os
import re

import numpy as np

import preint_data as pd
from ctypes_util import ErrBuf, ptr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_entry_point_is_declared_exported_and_bound():
    import harness
    import icgvins
    txt = open(os.path.join(ROOT, "include", "icgvins_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"\bint\s+icg_preint_evaluate_batch\s*\(", txt)
    assert hasattr(icgvins.load_library(), "icg_preint_evaluate_batch")
    assert "icg_preint_evaluate_batch" in icgvins.EXPORTS
    assert hasattr(icgvins.Context, "preint_evaluate_batch")
    assert hasattr(C.CDLL(harness.HOST_LIB), "icgh_backend_preint_device")


def test_host_layer_without_the_entry_point_loads_and_refuses():
    """oracle/libicgvins_host_oracle.so is the host layer on a C ABI implementation that does not define icg_preint_evaluate_batch: it must
    still load (ctypes binds every symbol at load time) and the device evaluation must fail by name, leaving every output untouched."""
    from stream_utils import ORACLE_HOST
    lib = C.CDLL(ORACLE_HOST)
    assert hasattr(lib, "icgh_backend_preint") and hasattr(lib, "icgh_backend_preint_device")
    p = ptr
    imu = np.ascontiguousarray(pd.make_interval(21, seed=3))
    s0 = np.ascontiguousarray(pd.state()[None, :])
    ep = np.ascontiguousarray(np.concatenate([s0[0], s0[0]])[None, :])
    offsets = np.array([0, 21], np.int32)
    mark = -7.25
    cur, rh, rd = np.full((1, 16), mark), np.full((1, 15), mark), np.full((1, 15), mark)
    Jh, Jd = np.full((1, 480), mark), np.full((1, 480), mark)
    Sh, Sd = np.full((1, 225), mark), np.full((1, 225), mark)
    okh, okd = np.full(1, 77, np.int32), np.full(1, 77, np.int32)
    err = ErrBuf()
    rc = lib.icgh_backend_preint_device(1, 1, p(offsets), p(imu), p(s0), p(np.ascontiguousarray(pd.PARAMS)), p(ep), p(cur), p(rh), p(Jh), p(rd),
                                        p(Jd), p(Sh), p(Sd), p(okh), p(okd), *err.args)
    assert rc != 0
    assert b"icg_preint_evaluate_batch is not in this build" in err.value
    for a in (cur, rh, rd, Jh, Jd, Sh, Sd):
        assert np.all(a == mark)
    assert okh[0] == 77 and okd[0] == 77
