"""The Schur-path edge suite on the HIP library: csrc/reproj_asm.hip and csrc/reproj_schur.hip (k_asm_runs, k_asm_camera, k_asm_landmarks, k_schur_inv_w,
k_schur_reduce_w, k_schur_backsub_w, k_terms_reduce_w, k_reproj_cost_w, k_lm_diag_w, k_reproj_chi2) on the cases of schur_edge_data.py, every
output cell against the long-double reference of schur_edge_checks.py within (n_t + 8) 2^-53 A.  test_schur_edges_cpu.py proves that the cases
reach their edges and that the reference is right.  Device only, bit for bit: S from the copying call is symmetric, a call repeated gives the
same bits, a window alone equals the same window in a batch where its K < Kmax and its NB < NBmax, and reassemble = 0 at a new damping equals a
fresh assembly at that damping — what the kernels' comments promise ("the value of a window does not depend on the batch it is reduced in")."""
import pytest

import schur_edge_checks as K
import schur_edge_data as D
import test_schur_edges_cpu as T

pytestmark = pytest.mark.gpu


def _make_ctx():
    import icgvins
    return icgvins.Context(640, 480, n_slots=1, max_batch=1, max_points=64)


@pytest.fixture(scope="module")
def ctx():
    c = _make_ctx()
    yield c
    c.close()


@pytest.mark.parametrize("P", sorted({w[0]["P"] for w in T.WIDTH}))
def test_reduction_width_on_gpu(ctx, P):
    for case, NT, wgs, LT in T.WIDTH:
        if case["P"] == P:
            T.assert_width_plan(case, NT, wgs, LT)
            K.check_case(ctx, case, device=True)


def test_wider_than_the_limit_is_refused_and_the_context_lives_on(ctx):
    K.check_refusal(ctx, D.over_limit_case())
    K.check_case(ctx, T.WIDTH[0][0], device=True)


def test_landmark_counts_on_gpu(ctx):
    one, holes = D.landmark_count_cases()
    K.check_case(ctx, one, device=True)
    K.check_case(ctx, holes, device=True)
    K.check_batch(_make_ctx, D.empty_window_batch(), device=True)


def test_runs_on_gpu(ctx):
    cases = D.run_cases()
    T.assert_run_plans(cases)
    for c in cases:
        K.check_case(ctx, c, device=True)


@pytest.mark.parametrize("k", range(len(T.ROWS)), ids=[w[0]["name"] for w in T.ROWS])
def test_landmark_rows_on_gpu(ctx, k):
    case, LB, LB_min = T.ROWS[k]
    T.assert_landmark_row_plan(case, LB, LB_min)
    K.check_case(ctx, case, device=True)


def test_clamps_on_gpu(ctx):
    (case,) = D.clamp_cases()
    st = {}
    K.check_case(ctx, case, device=True, stats=st)
    assert st["branches"] == {-1, 0, 1, 2}, st["branches"]
    st = {}
    K.check_batch(_make_ctx, D.clamp_batch(), device=True, damp1=[1e-4, 3.0], damp2=[3.0, 0.0], stats=st)
    assert {0, 1, 2} <= st["branches"], st["branches"]


def test_window_alone_equals_window_in_batch_on_gpu():
    det = D.determinism_batch()
    T.assert_determinism_batch(det)
    K.check_batch(_make_ctx, det, device=True)
    K.check_batch(_make_ctx, D.wide_batch(), device=True)


@pytest.mark.parametrize("huber", [0.0, 1.5])
def test_cost_and_chi2_counts_on_gpu(ctx, huber):
    outl = inl = 0
    for c in T.COUNTS:
        c = dict(c, huber=huber)
        st = {}
        K.check_case(ctx, c, device=True, stats=st)
        outl, inl = outl + st["huber_outliers"], inl + st["huber_inliers"]
        seen = K.check_chi2(ctx, c)
        assert (True, True) in seen and (False, False) in seen
        assert len(c["idx_i"]) == 1 or (False, True) in seen
    assert (outl > 0 and inl > 0) if huber > 0 else outl == 0
