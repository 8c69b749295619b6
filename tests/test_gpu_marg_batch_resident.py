"""GPU: MarginalizationBatch::setDeviceReducedSystem (host/marg_batch.h) — the reduced systems stay on the device between M2 and M3 —
gives every output bit, the structured / dense counts and ok of the device linearization alone, on three families of windows: jittered
visual windows with one dense window, visual-inertial windows of different widths (m = 15), and second-generation windows whose host
factors include the dense prior of the first marginalization.  With keeping on, the tags are the same and a prior set built from the
tagged views evaluates to the shipped set's bits.  No tolerance anywhere in this file."""
import ctypes as C

import numpy as np
import pytest

import marg_resident_data as mr
from ctypes_util import ErrBuf

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def lib():
    import harness
    return C.CDLL(harness.HOST_LIB)


@pytest.fixture(scope="module")
def vio(oracle):
    return mr.vio_windows(oracle)


def _run(lib, mode, family, vio):
    if family == 1:
        rc, msg, out = mr.backend_marg_resident(lib, mode, 1, len(vio), vio=vio)
    else:
        rc, msg, out = mr.backend_marg_resident(lib, mode, family, 6, P=mr.visual_problem(), dense_window=2 if family == 0 else -1)
    assert rc == 0, (mode, family, rc, msg)
    return out


def _same(a, b, what):
    assert np.array_equal(a["ok"], b["ok"]) and np.array_equal(a["r"], b["r"]), what
    assert (a["structured"], a["dense"]) == (b["structured"], b["dense"]), what
    for w, (x, y) in enumerate(zip(mr.split(a), mr.split(b))):
        assert (x is None) == (y is None), (what, w)
        if x is not None:
            for k in x:
                assert np.array_equal(x[k], y[k]), (what, w, k)


EXPECTED = {0: dict(ok=6, structured=5, dense=1), 1: dict(ok=4, structured=4, dense=0), 2: dict(ok=6, structured=6, dense=0)}


@pytest.mark.parametrize("family", [0, 1, 2])
def test_reduced_system_on_the_device_equals_the_device_linearization(lib, vio, family):
    assert lib.icgh_backend_marg_resident_available() == 1
    ref = _run(lib, 0, family, vio)
    e = EXPECTED[family]
    assert int(ref["ok"].sum()) == e["ok"] and (ref["structured"], ref["dense"]) == (e["structured"], e["dense"]), ref
    assert ref["tagged"] == 0 and ref["handed_off"] == 0 and (ref["tag_slot"] == -1).all()
    if family == 1:
        assert list(ref["r"]) == [22, 52, 37, 22]  # 15 K + 7 columns, 15 of them marginalized: different widths in one batch
    got = _run(lib, 1, family, vio)
    _same(got, ref, family)
    assert got["tagged"] == 0 and got["handed_off"] == 0
    parts = mr.split(ref)
    assert not np.array_equal(parts[0]["Hp"], parts[-1]["Hp"]) or family == 1  # (the windows are different problems)
    # keeping on: the same bits again, the same tags as the device linearization with keeping on, and the set built from the tagged views
    # on a second context evaluates to the shipped set's bits (`residuals` of the runs without keeping)
    kept_ref = _run(lib, 2, family, vio)
    kept = _run(lib, 3, family, vio)
    _same(kept_ref, ref, (family, "keep, mode 2"))
    _same(kept, ref, (family, "keep, mode 3"))
    assert np.array_equal(kept["tag_slot"], kept_ref["tag_slot"]) and kept["tagged"] == kept_ref["tagged"] == e["structured"]
    assert kept["handed_off"] == kept_ref["handed_off"] == e["structured"]
    assert sorted(kept["tag_slot"][kept["tag_slot"] >= 0]) == list(range(e["structured"]))


def test_switch_alone_is_refused_by_message(lib):
    err = ErrBuf()
    assert lib.icgh_backend_marg_resident_switch_alone(*err.args) == 1, err.value
    assert "setDeviceReducedSystem(true) needs setDeviceLinearization(true)" in err.text()
