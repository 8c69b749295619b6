"""The reduced camera solve's plumbing without a GPU: the new C entries are exported and listed, and the host layer's mode switch keeps mode 0
the existing solve and fails mode 1 by name where the device entries are not in the build (the oracle-backed host library)."""
import ctypes as C

import test_host_solver_cpu as ths
import reduced_solve_utils as ru

NEW = ("icg_chol_solve_batch", "icg_reproj_schur_windows_resident", "icg_reproj_solve_windows")


def test_new_entries_are_exported_and_listed():
    import icgvins
    lib = icgvins.load_library()
    for name in NEW:
        assert name in icgvins.EXPORTS, name
        assert hasattr(lib, name), name
    assert icgvins.CHOL_MAX_N == 512


def test_mode_switch_on_the_oracle_backed_host_library():
    from stream_utils import ensure_oracle_host
    lib = C.CDLL(ensure_oracle_host())
    assert hasattr(lib, "icgh_backend_solve_batch_mode")
    probs = ths._batch_problems()
    rc0, msg0, plain = ru.solve_batch_mode(lib, probs, None)
    assert rc0 == 0, msg0
    rc, msg, mode0 = ru.solve_batch_mode(lib, probs, 0)
    assert rc == 0, msg
    ru.assert_same_results(mode0, plain)
    rc, msg, _ = ru.solve_batch_mode(lib, probs, 1)
    assert rc == -4 and "icg_reproj_solve_windows is not in this build" in msg, (rc, msg)
