"""The M3 -> M4 hand-off (icg_marg_linearize_batch_keep, icg_marg_linearized_release, icg_marg_prior_set_from_kept) as far as it can be
checked without a GPU: the entries are declared with the reference code they restate, exported and bound; a build of the host layer
WITHOUT them (the oracle-backed checker library) loads, says so and refuses setKeepLinearized by name; the tag of a kept linearization
travels from a MarginalizationInfo into the view of its MarginalizationFactor."""
import ctypes as C
import os
import re

import numpy as np

import marg_handoff_data as mh

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ENTRIES = ("icg_marg_linearize_batch_keep", "icg_marg_linearized_release", "icg_marg_prior_set_from_kept")


def _oracle_host():
    from stream_utils import ensure_oracle_host
    return C.CDLL(ensure_oracle_host())


def test_entries_are_declared_exported_and_bound():
    import harness
    import icgvins
    txt = open(os.path.join(ROOT, "include", "icgvins_hip.h")).read()
    # both new entries cite the reference code in the comment in front of their declaration
    for name in ("icg_marg_linearize_batch_keep", "icg_marg_prior_set_from_kept"):
        at = txt.index("int " + name + "(")
        comment = txt[txt.rindex("/*", 0, at):at]
        assert "factors/marginalization_info.h:153-192" in comment and "factors/marginalization_factor.h:47-101" in comment, name
    code = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    lib = icgvins.load_library()
    for name in ENTRIES:
        assert re.search(r"\bint\s+" + name + r"\s*\(", code), name
        assert hasattr(lib, name) and name in icgvins.EXPORTS, name
    for wrapper in ("marg_linearize_batch_keep", "marg_linearized_release", "marg_prior_set_from_kept"):
        assert hasattr(icgvins.Context, wrapper), wrapper
    host = C.CDLL(harness.HOST_LIB)
    assert hasattr(host, "icgh_backend_marg_handoff")
    assert host.icgh_backend_marg_handoff_available() == 3  # the product library links the C ABI that has them


def test_host_layer_without_the_entries_loads_and_refuses_by_name():
    import marg_data as md
    lib = _oracle_host()
    assert lib.icgh_backend_marg_handoff_available() == 0
    P = md.make_problem(n_lm=40, n_kf=4, seed=7)
    rc, msg, out = mh.backend_marg_handoff(lib, P, 3, 1)
    assert rc == -4 and msg.startswith("icg_marg_linearize_batch_keep is not in this build"), (rc, msg)
    assert out["priors"] == 0 and not out["timers_ms"].any()  # nothing was computed
    rc, msg, out = mh.backend_marg_handoff(lib, P, 3, 3)
    assert rc == -4 and msg.startswith("icg_marg_linearize_batch_keep is not in this build"), (rc, msg)
    # keeping off: what this build lacks is the device linearization itself
    rc, msg, out = mh.backend_marg_handoff(lib, P, 3, 0)
    assert rc == -4 and "icg_marg_linearize_batch is not in this build" in msg, (rc, msg)
    rc, msg, _ = mh.backend_marg_handoff(lib, P, 3, 2)
    assert rc == -1 and "mode" in msg, (rc, msg)


def test_tags_travel_from_the_info_into_the_factor_s_view():
    import harness
    for lib in (_oracle_host(), C.CDLL(harness.HOST_LIB)):
        out = np.full(4, 99, np.int64)
        lib.icgh_backend_marg_handoff_tags.argtypes = [C.c_uint64, C.c_int, C.c_void_p]
        assert lib.icgh_backend_marg_handoff_tags(0x1234567890, 17, out.ctypes.data_as(C.c_void_p)) == 0
        assert list(out) == [0, -1, 0x1234567890, 17], out
