"""M3 for many windows (icg_marg_linearize_batch, MarginalizationLinearizer): what can be checked without a GPU — the entry is declared,
exported and bound; a build of the host layer WITHOUT the device entry (the oracle-backed checker library) loads and refuses the device
modes by name; the host mode (linearizeReduced on the pool) equals the oracle's orc_marginalize on the same (H, b, m) and satisfies the
linearization identities; and the free functions MarginalizationInfo now calls give the bits of the loops they were factored out of."""
import ctypes as C
import os
import re

import numpy as np

import marg_linearize_data as ml
from ctypes_util import ErrBuf, f64, i32, ptr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MARK = -7.25


def _oracle_host():
    from stream_utils import ORACLE_HOST
    lib = C.CDLL(ORACLE_HOST)
    assert hasattr(lib, "icgh_backend_marg_linearize")
    return lib


def _oracle():
    import oracle_lib
    return oracle_lib.load()


def test_entry_point_is_declared_exported_and_bound():
    import harness
    import icgvins
    txt = open(os.path.join(ROOT, "include", "icgvins_hip.h")).read()
    assert "factors/marginalization_info.h:153-192" in txt  # the entry cites the reference code it restates
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    assert re.search(r"\bint\s+icg_marg_linearize_batch\s*\(", txt)
    assert hasattr(icgvins.load_library(), "icg_marg_linearize_batch")
    assert "icg_marg_linearize_batch" in icgvins.EXPORTS and hasattr(icgvins.Context, "marg_linearize_batch")
    m = re.search(r"#define\s+ICG_MARG_LIN_MAX_P\s+(\d+)", txt)
    assert m and int(m.group(1)) == icgvins.MARG_LIN_MAX_P >= 256
    assert hasattr(C.CDLL(harness.HOST_LIB), "icgh_backend_marg_linearize")


def test_host_layer_without_the_entry_point_loads_and_refuses():
    lib = _oracle_host()
    systems = ml.batch()[3:6]
    rc, msg, out, sec = ml.backend_marg_linearize(lib, 1, systems, mark=MARK)
    assert rc != 0 and "icg_marg_linearize_batch is not in this build" in msg
    for a in list(out.values()) + [sec]:
        assert np.all(a == (int(MARK) if a.dtype == np.int32 else MARK))
    # the batched marginalization with the device linearization on fails by name as well, instead of computing on the host
    import backend_utils as bu
    import marg_data as md
    P = md.make_problem(n_lm=40, n_kf=4, seed=7)
    w = P["w"]
    obs = np.ascontiguousarray(P["obs"], np.float64)
    poses, inv = np.ascontiguousarray(w["poses"], np.float64), np.ascontiguousarray(w["invdepth"], np.float64)
    cap = 6 * poses.shape[0] + inv.shape[0] + 7
    sizes, counts, seconds = np.zeros(2, np.int32), np.zeros(2, np.int32), np.zeros(1)
    big = [np.zeros(2 * cap * cap) for _ in range(4)]
    err = ErrBuf()
    p_ = ptr
    rc = lib.icgh_backend_marginalize_batch(2, 2, -1, C.c_double(1e-3), 1, obs.shape[1], p_(obs), p_(i32(P["ii"])), p_(i32(P["jj"])),
                                            p_(i32(P["ll"])), poses.shape[0], p_(poses), p_(f64(w["ext"])), inv.shape[0], p_(inv),
                                            C.c_double(w["td"]), C.c_double(1.0), C.c_double(100.0), 2, p_(sizes), *[p_(a) for a in big],
                                            p_(counts), p_(seconds), *err.args)
    assert rc != 0 and b"icg_marg_linearize_batch is not in this build" in err.value, (rc, err.value)


def test_chosen_inputs_have_no_eigenvalue_near_the_floor_and_host_mode_equals_the_oracle():
    orc, lib = _oracle(), _oracle_host()
    systems = ml.batch()
    assert [(s["P"], s["m"]) for s in systems[:6]] == [(157, 15), (232, 15), (37 + ml.golden_m(), ml.golden_m()), (1, 0), (2, 1), (256, 0)]
    rc, msg, out, _ = ml.backend_marg_linearize(lib, 0, systems, host_threads=4)
    assert rc == 0, msg
    host = ml.split(systems, out)
    ml.assert_no_eigenvalue_near_the_floor(lib, systems, host)
    names = {s["name"]: h for s, h in zip(systems, host)}
    assert (names["rank_deficient"]["evals"] > ml.EPS).sum() == 100 and names["rank_deficient"]["status"] == 4
    assert names["zero_row"]["status"] == 4 and names["zero_row_m"]["status"] == 2 and names["c2"]["status"] == 0
    assert names["zero_row_m"]["min_ev_m"] <= ml.EPS and np.isinf(names["spd256_0"]["min_ev_m"])
    d = np.abs(np.diag(names["badly_scaled"]["Hp"]))
    assert d.max() / d.min() > 1e10
    for s, h in zip(systems, host):
        J0, e0, Hp, bp = orc.marginalize(s["H"], s["b"], s["m"])
        sc, sb = np.abs(Hp).max(), max(1.0, np.abs(bp).max())
        assert np.abs(h["Hp"] - Hp).max() <= 1e-8 * sc, s["name"]
        assert np.abs(h["bp"] - bp).max() <= 1e-8 * sb, s["name"]
        inv, ref = ml.invariants(s, h), ml.invariants(s, dict(J0=J0, e0=e0))
        # the linearization identities (b = -H x lies in the range of H, so also where Hp is rank-deficient)
        assert np.abs(inv["JtJ"] - h["Hp"]).max() <= 1e-8 * sc, (s["name"], np.abs(inv["JtJ"] - h["Hp"]).max() / sc)
        assert np.abs(inv["Jte"] + h["bp"]).max() <= 1e-8 * sb, (s["name"], np.abs(inv["Jte"] + h["bp"]).max() / sb)
        assert np.abs(inv["JtJ"] - ref["JtJ"]).max() <= 1e-8 * sc and np.abs(inv["Jte"] - ref["Jte"]).max() <= 1e-8 * sb, s["name"]
        assert abs(inv["cost"] - ref["cost"]) <= 1e-8 * max(1.0, ref["cost"]), s["name"]
        assert np.all(np.diff(h["evals"]) >= 0)
    # optional outputs left out: the required ones are the same bits
    rc, msg, out2, _ = ml.backend_marg_linearize(lib, 0, systems, want=(False,) * 5, host_threads=1)
    assert rc == 0 and ml.same_bits(out2["J0"], out["J0"]) and ml.same_bits(out2["e0"], out["e0"])


def _loops_before_the_refactoring(lib, H, b, m, eps=ml.EPS):
    """MarginalizationInfo::schurElimination and ::linearization as they stood before they were factored into schurReduce / linearizePrior
    (host/marg_m3.cc), restated loop for loop over numpy.float64 scalars; the eigen-solver through icgh_symmetric_eigen"""
    f, P = np.float64, H.shape[0]
    r = P - m

    def eigen(A):
        n = A.shape[0]
        ev, V = np.zeros(n), np.zeros((n, n))
        if n:
            assert lib.icgh_symmetric_eigen(n, ptr(np.ascontiguousarray(A)), ptr(ev), ptr(V)) == 0
        return ev, V

    Hmm = np.array([[f(0.5) * (H[i, j] + H[j, i]) for j in range(m)] for i in range(m)]).reshape(m, m)
    ev, V = eigen(Hmm)
    inv = [f(1.0) / ev[k] if ev[k] > eps else f(0.0) for k in range(m)]
    Wv = [[V[i, k] * inv[k] for k in range(m)] for i in range(m)]
    Hinv = np.zeros((m, m))
    for i in range(m):
        for j in range(i + 1):
            s = f(0)
            for k in range(m):
                s = s + Wv[i][k] * V[j, k]
            Hinv[i, j] = Hinv[j, i] = s
    T = np.zeros((r, m))
    for i in range(r):
        for j in range(m):
            s = f(0)
            for k in range(m):
                s = s + H[m + i, k] * Hinv[k, j]
            T[i, j] = s
    Hp, bp = np.zeros((r, r)), np.zeros(r)
    for i in range(r):
        for j in range(r):
            s = f(0)
            for k in range(m):
                s = s + T[i, k] * H[k, m + j]
            Hp[i, j] = H[m + i, m + j] - s
        s = f(0)
        for k in range(m):
            s = s + T[i, k] * b[k]
        bp[i] = b[m + i] - s
    ev, V = eigen(Hp)
    J0, e0 = np.zeros((r, r)), np.zeros(r)
    for k in range(r):
        S = ev[k] if ev[k] > eps else f(0.0)
        Sinv = f(1.0) / ev[k] if ev[k] > eps else f(0.0)
        ss, si = np.sqrt(S), np.sqrt(Sinv)
        vb = f(0)
        for i in range(r):
            J0[k, i] = ss * V[i, k]
            vb = vb + V[i, k] * -bp[i]
        e0[k] = si * vb
    return Hp, bp, J0, e0


def test_the_factored_host_functions_give_the_bits_of_the_loops_they_replace():
    lib = _oracle_host()
    systems = [ml.spd_system(24, 6, 21), ml.spd_system(9, 0, 22), ml.zero_row_system(23, P=20, m=5), ml.zero_row_system(24, P=20, m=5, where=2),
               ml.badly_scaled_system(25, P=18, m=4)]
    rc, msg, out, _ = ml.backend_marg_linearize(lib, 0, systems, host_threads=2)
    assert rc == 0, msg
    for s, h in zip(systems, ml.split(systems, out)):
        Hp, bp, J0, e0 = _loops_before_the_refactoring(lib, s["H"], s["b"], s["m"])
        assert ml.same_bits(h["Hp"], Hp) and ml.same_bits(h["bp"], bp), s["name"]
        assert ml.same_bits(h["J0"], J0) and ml.same_bits(h["e0"], e0), s["name"]
    # MarginalizationInfo itself (dense and landmark-eliminated path): its linearization is the old loop on its own Hp, bp
    import backend_utils as bu
    import marg_data as md
    P = md.make_problem(n_lm=40, n_kf=4, seed=7)
    for dense in (1, 0):
        lib.icgh_backend_marginalization_force_dense(dense)
        try:
            got = bu.backend_marginalize(lib, P)
        finally:
            lib.icgh_backend_marginalization_force_dense(0)
        r = got["r"]
        Hp, bp, J0, e0 = _loops_before_the_refactoring(lib, np.ascontiguousarray(got["Hp"]), np.ascontiguousarray(got["bp"]), 0)
        assert ml.same_bits(Hp, got["Hp"]) and ml.same_bits(bp, got["bp"])  # (m = 0: the Schur step is the identity)
        assert ml.same_bits(J0, got["J0"]) and ml.same_bits(e0, got["e0"]), (dense, r)


GUARD = 100.0 * ml.EPS  # MarginalizationInfo::STRUCTURED_GUARD


def _guarded_loops_before_the_refactoring(lib, H, b, m, guard=GUARD):
    """MarginalizationInfo::finishStructured's second guard and small M3 as they stood before they became schurReduceGuarded
    (host/marg_m3.cc): each eigenvector column DIVIDED by its eigenvalue, restated loop for loop over numpy.float64 scalars; the
    eigen-solver through icgh_symmetric_eigen.  None: the guard refuses."""
    f, P = np.float64, H.shape[0]
    r = P - m
    Hmm = np.array([[f(0.5) * (H[i, j] + H[j, i]) for j in range(m)] for i in range(m)]).reshape(m, m)
    ev, V = np.zeros(m), np.zeros((m, m))
    if m:
        assert lib.icgh_symmetric_eigen(m, ptr(np.ascontiguousarray(Hmm)), ptr(ev), ptr(V)) == 0
    for k in range(m):
        if not ev[k] > guard:
            return None
    Wv = [[V[i, k] / ev[k] for k in range(m)] for i in range(m)]
    Hinv = np.zeros((m, m))
    for i in range(m):
        for j in range(i + 1):
            s = f(0)
            for k in range(m):
                s = s + Wv[i][k] * V[j, k]
            Hinv[i, j] = Hinv[j, i] = s
    T = np.zeros((r, m))
    for i in range(r):
        for j in range(m):
            s = f(0)
            for k in range(m):
                s = s + H[m + i, k] * Hinv[k, j]
            T[i, j] = s
    Hp, bp = np.zeros((r, r)), np.zeros(r)
    for i in range(r):
        for j in range(r):
            s = f(0)
            for k in range(m):
                s = s + T[i, k] * H[k, m + j]
            Hp[i, j] = H[m + i, m + j] - s
        s = f(0)
        for k in range(m):
            s = s + T[i, k] * b[k]
        bp[i] = b[m + i] - s
    return Hp, bp


def _schur_reduce_guarded(lib, s, guard=GUARD):
    r = s["P"] - s["m"]
    Hp, bp = np.full((r, r), MARK), np.full(r, MARK)
    rc = lib.icgh_schur_reduce_guarded(s["P"], s["m"], ptr(s["H"]), ptr(np.ascontiguousarray(s["b"])), C.c_double(guard), ptr(Hp), ptr(bp))
    return rc, Hp, bp


def test_the_guarded_schur_step_gives_the_bits_of_the_loops_it_replaces_and_refuses_untouched():
    lib = _oracle_host()
    systems = [ml.spd_system(24, 6, 21), ml.badly_scaled_system(25, P=18, m=4), ml.spd_system(9, 0, 22), ml.spd_system(7, 1, 23),
               ml.spd_system(6, 5, 24), ml.zero_row_system(23, P=20, m=5)]  # m = 0, m = 1 and r = 1 (P = m + 1) among them; the last one's
    # zero row lies in the retained block (index 19), so its m-block passes the guard and Hp has a zero row and column
    assert [(s["m"], s["P"] - s["m"]) for s in systems[2:]] == [(0, 9), (1, 6), (5, 1), (5, 15)]
    rc, msg, out, _ = ml.backend_marg_linearize(lib, 0, systems, host_threads=2)
    assert rc == 0, msg
    differs = []
    for s, floored in zip(systems, ml.split(systems, out)):
        want = _guarded_loops_before_the_refactoring(lib, s["H"], s["b"], s["m"])
        rc, Hp, bp = _schur_reduce_guarded(lib, s)
        assert rc == 1 and want is not None, s["name"]
        assert ml.same_bits(Hp, want[0]) and ml.same_bits(bp, want[1]), s["name"]
        differs.append(not ml.same_bits(Hp, floored["Hp"]))
        if s["m"] == 0:
            assert ml.same_bits(Hp, s["H"]) and ml.same_bits(bp, s["b"])
    # V / ev against V * (1 / ev): the two forms of the step are not the same bits, and neither one-liner may replace the other
    assert differs[0] or differs[1], differs
    assert not differs[2]  # (m = 0: nothing is scaled)
    # refusals: an m-block eigenvalue at or below the guard (exactly 0 here; then exactly at the guard) leaves the outputs as they were
    z = ml.zero_row_system(24, P=20, m=5, where=2)  # (the zero row inside the m-block)
    assert _guarded_loops_before_the_refactoring(lib, z["H"], z["b"], z["m"]) is None
    rc, Hp, bp = _schur_reduce_guarded(lib, z)
    assert rc == 0 and np.all(Hp == MARK) and np.all(bp == MARK)
    s = systems[0]
    smallest = float(ml.host_eigenvalues(lib, 0.5 * (s["H"][:6, :6] + s["H"][:6, :6].T))[0])
    rc, Hp, bp = _schur_reduce_guarded(lib, s, guard=smallest)
    assert rc == 0 and np.all(Hp == MARK) and np.all(bp == MARK)
    assert _schur_reduce_guarded(lib, s, guard=np.nextafter(smallest, 0.0))[0] == 1
    assert _schur_reduce_guarded(lib, s, guard=float("nan"))[0] == 0
    assert lib.icgh_schur_reduce_guarded(5, 5, ptr(s["H"]), ptr(s["b"]), C.c_double(GUARD), ptr(Hp), ptr(bp)) == -1


def test_the_first_guard_refuses_a_landmark_minimum_at_the_guard_or_nan_and_leaves_the_outputs():
    """MarginalizationInfo::finishStructured's first guard on a real window (icgh_backend_marginalize_min_hll: the device factor set reports
    the smallest landmark diagonal the test chooses): above the guard the landmark-eliminated path gives its bits, at the guard and for a
    NaN it refuses with Hp_ / bp_ still empty when the dense assembly starts, and the window gets the dense path's bits."""
    import backend_utils as bu
    import marg_data as md
    lib = _oracle_host()
    P = md.make_problem(n_lm=40, n_kf=4, seed=7)
    ref = {}
    for dense in (1, 0):
        lib.icgh_backend_marginalization_force_dense(dense)
        try:
            ref[dense] = bu.backend_marginalize(lib, P)
        finally:
            lib.icgh_backend_marginalization_force_dense(0)
    assert not ml.same_bits(ref[0]["Hp"], ref[1]["Hp"])  # (the two paths are told apart by their bits)

    def run(min_hll):
        args, K, L = bu.marg_problem_args(P, 1.0, 100.0)
        cap = 6 * K + L + 7
        flags, sizes, Hp, bp = np.zeros(2, np.int32), np.zeros(2, np.int32), np.zeros(cap * cap), np.zeros(cap)
        err = ErrBuf()
        rc = lib.icgh_backend_marginalize_min_hll(*args, C.c_double(min_hll), ptr(flags), ptr(sizes), ptr(Hp), ptr(bp), *err.args)
        assert rc == 0, (rc, err.value)
        r = int(sizes[1])
        return int(flags[0]), int(flags[1]), Hp[:r * r], bp[:r]

    structured, at_dense, Hp, bp = run(float(np.nextafter(GUARD, np.inf)))
    assert (structured, at_dense) == (1, -1) and ml.same_bits(Hp, ref[0]["Hp"]) and ml.same_bits(bp, ref[0]["bp"])
    for refused in (GUARD, float("nan"), 0.0):
        structured, at_dense, Hp, bp = run(refused)
        assert (structured, at_dense) == (0, 0), refused
        assert ml.same_bits(Hp, ref[1]["Hp"]) and ml.same_bits(bp, ref[1]["bp"]), refused


def test_host_entry_rejects_an_invalid_system():
    lib = _oracle_host()
    good = ml.spd_system(5, 2, 31)
    for bad in (dict(good, m=5), dict(good, m=-1)):
        rc, msg, out, _ = ml.backend_marg_linearize(lib, 0, [good, bad], mark=MARK)
        assert rc != 0 and "window 1" in msg and np.all(out["J0"] == MARK)
