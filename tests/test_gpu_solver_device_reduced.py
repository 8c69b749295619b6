"""WindowSolverBatch with the reduced camera solves on the device (icgh_backend_solve_batch_mode, mode 1) against the host solves (mode 0)
and the existing entry: delta_c is the same bits, so the LM sequences and every result are identical as arrays.
The active flags: icgh_backend_solve_batch_mode has no output for them (they live in the WindowSolverBatch it builds and drops), so what is
compared of the culling is the entry's own record of it, summary[7] (the count of culled factors), together with every state the second
solve produced from the surviving factors (reduced_solve_utils.assert_same_results)."""
import ctypes as C

import pytest

import test_host_solver_cpu as ths
import reduced_solve_utils as ru

pytestmark = pytest.mark.gpu


def test_device_reduced_solve_equals_host_reduced_solve():
    import harness
    lib = C.CDLL(harness.HOST_LIB)
    probs = ths._batch_problems()
    rc, msg, plain = ru.solve_batch_mode(lib, probs, None)
    assert rc == 0, msg
    rc, msg, host = ru.solve_batch_mode(lib, probs, 0)
    assert rc == 0, msg
    rc, msg, dev = ru.solve_batch_mode(lib, probs, 1)
    assert rc == 0, msg
    ru.assert_same_results(host, plain)
    ru.assert_same_results(dev, host)
    assert any(r["summary"][4] + r["summary"][6] > 0 for r in host) and all(r["summary"][3] > 0 for r in host)  # rejected and accepted steps occur
