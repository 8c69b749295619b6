"""Many-stream preintegration without a GPU: the two C entries are declared, exported and bound; and on the oracle-backed build of the host
layer, whose C ABI has neither icg_preint_batch_params nor icg_preint_odo_batch_params, the library still loads (the references are weak),
integrateStreamsAvailable() is false for both families, and integrateStreams fails by the entry's name and leaves every object as it was:
not integrated."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import preint_streams_data as sd
from ctypes_util import bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = {"imu": "icg_preint_batch_params", "odo": "icg_preint_odo_batch_params"}


@pytest.fixture(scope="module")
def lib():
    from stream_utils import ensure_oracle_host
    return C.CDLL(ensure_oracle_host())


def test_entries_are_declared_exported_and_bound():
    import icgvins
    txt = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "icgvins_hip.h")).read(), flags=re.S)
    for name, method in (("icg_preint_batch_params", "preint_batch_params"), ("icg_preint_odo_batch_params", "preint_odo_batch_params")):
        assert re.search(r"\bint\s+" + name + r"\s*\(", txt)
        assert name in icgvins.EXPORTS and hasattr(icgvins.Context, method)
    if os.path.exists(icgvins.LIB_PATH):
        hip = icgvins.load_library()
        assert hasattr(hip, "icg_preint_batch_params") and hasattr(hip, "icg_preint_odo_batch_params")


def test_streams_are_not_available_on_the_cpu_build(lib):
    assert lib.icgh_preint_streams_available() == 0 and lib.icgh_preint_odo_streams_available() == 0


@pytest.mark.parametrize("family", ["imu", "odo"])
def test_integrate_streams_fails_by_the_entrys_name_and_integrates_nothing(lib, family):
    fam = sd.FAMILIES[family]
    items = fam.items([41, 7, 1])
    hostrows = sd.host_rows(fam, fam.rows(3))
    r = sd.streams(lib, fam, fam.earth, items, hostrows, 1)
    assert r["rc"] == -4 and r["msg"] == ENTRIES[family] + " is not in this build", (r["rc"], r["msg"])
    f = sd.member_fields(fam)
    m = r["members"][0]
    assert np.all(r["ready"][0] == 0)  # still dirty: nothing was integrated
    assert np.all(bits(m[:, f["dt"]]) == 0) and np.all(bits(m[:, f["cov"]]) == 0) and np.all(bits(m[:, f["sqrt_info"]]) == 0)
    for k, (_, s0) in enumerate(items):
        assert np.array_equal(m[k, f["jac"]].reshape(fam.N, fam.N), np.eye(fam.N))
        assert np.array_equal(m[k, f["cur"]][:16], s0[:16])  # the current state is the start state
    assert np.all(r["pn_doubles"][0] == 0) and np.all(bits(r["pn"]) == bits(sd.SENTINEL))
    # the second stage was never reached
    assert np.all(bits(r["members"][1]) == bits(sd.SENTINEL)) and np.all(r["ready"][1] == -1) and np.all(r["prof"] == -1.0)


def test_integrate_batch_still_works_beside_it(lib):
    """mode 0 of the same entry on the CPU build: the 15-state family integrates through the shim's icg_preint_batch"""
    fam = sd.FAMILIES["imu"]
    items = fam.items([41, 7, 1])
    r = sd.streams(lib, fam, 1, items, sd.host_rows(fam, fam.rows(3)), 0)
    assert r["rc"] == 0, r["msg"]
    assert list(r["ready"][0]) == [1, 1, 0]
