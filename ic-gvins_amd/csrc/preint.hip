// P1: IMU preintegration inner loop, batched over independent intervals (one 64-lane wavefront per interval).
//
// Reference: preintegration/preintegration_base.cc:39-70,86-92 (two-sample coning/sculling integration, bias
// compensation), preintegration_normal.cc:183-253 and preintegration_earth.cc:205-335 (per-sample error-state transition
// phi = I + F dt, jacobian_ = phi jacobian_, covariance_ = phi P phi^T + 0.5 dt (phi G Q G^T + G Q G^T phi^T)).
// The reference does this with heap-allocated dynamic Eigen matrices, one IMU sample at a time.  Here the 15x15 Jacobian
// and covariance stay in LDS for the whole interval; every lane carries the (uniform) navigation state redundantly and
// owns <=4 of the 225 matrix entries in each of the six 15x15 products per sample.  Strictly sequential over the
// samples of an interval (quaternion renormalisation), embarrassingly parallel across intervals/streams.
//
// The products are evaluated SPARSELY and stay bit-identical to the dense ones: phi = I + F dt has at most 7 structural non-zeros per
// row (rows of p: 2, v: 7, attitude: 4, bg / ba: 1) and G Q G^T is block diagonal; a dense sum  a = 0; a += phi[i][k] * x[k]  visits
// the same non-zero terms in the same ascending-k order, and the skipped terms are exact zeros (x finite), which leave every partial sum
// unchanged (pinned bit for bit against the oracle's dense products by tests/test_gpu_preint_edges.py).  Entries are dealt to the lanes sorted by the cost of their row (first pass) / column (second pass), so a wave's lanes
// run the same straight-line code: ~21 term-iterations per product pass instead of 60.  Measured: -15 % per launch (3 840 intervals x 40
// samples 1.56 -> 1.30 ms; one 200-sample interval 2.07 -> 1.80 ms) — the rest of a sample is the strictly sequential FP64 navigation update
// (~1 300 dependent operations incl. six sin/cos and a dozen divisions in the Earth variant), which every lane carries redundantly.
// Compute/latency bound (72 B in per sample, state on chip): reported as IMU samples/s, not against the HBM roofline.
//
// P2: the factor evaluation on an integration result (bodies in preint_shared.h, shared with the odometer family of preint_odo.hip and
// instantiated here at N = 15), batched over independent factors, one 64-lane wavefront
// per factor, two launches per call:
//   k_preint_sqrt_info   S = LLT(cov^-1).matrixL()^T (preintegration_normal.cc:39-40, preintegration_earth.cc:39-40) with the arithmetic and the
//                        order of the host layer's Preintegration::updateSqrtInformation: Gauss-Jordan with partial pivoting on the 15 x 30
//                        augmented matrix in LDS (the entries of one elimination step are independent: lanes own entries; the pivot search is
//                        a 16-lane reduction), mirrored lower triangle, column Cholesky (lane i owns row i).  Only + - * / sqrt, all correctly
//                        rounded on both sides: S is bit-identical to the host's.
//   k_preint_evaluate    residual 15 + Jacobians 15x7 | 15x9 | 15x7 | 15x9 (preintegration_normal.cc:38-142, preintegration_earth.cc:37-164,
//                        preintegration_factor.h:45-69; quaternion helpers rotation.h:103-119).  Every lane carries the (uniform) geometry
//                        redundantly, lane 0 lays the unwhitened 15 x 32 Jacobian and the residual out in LDS, then each lane owns 8 of the
//                        15 + 480 outputs and forms each as the dense 15-term sum over k ascending from zero, as the host's Preintegration::evaluate
//                        does.  The only primitives that may round differently from the host are sin / cos in rotvec2quat.
//   k_preint_evaluate_given  the same body for a set of factors RESIDENT on the device (icg_preint_set): the two
//                        rotvec2quat results and S come from the host, so nothing is left that may round differently; one launch per call.
// Latency bound like P1 (~8 KB in, ~4 KB out, a few thousand dependent FP64 operations per factor, no reuse across factors): reported as
// factors/s, not against the HBM roofline.
#include "preint_shared.h"

using namespace icgd;
using namespace icg_preint;

namespace {
struct nav_state {
    d3 p;
    dq q;
    d3 v, bg, ba;
};
__device__ __forceinline__ nav_state load_state(const double *s) {
    nav_state st;
    st.p  = mk3(s[0], s[1], s[2]);
    st.q  = dq{s[3], s[4], s[5], s[6]};
    st.v  = mk3(s[7], s[8], s[9]);
    st.bg = mk3(s[10], s[11], s[12]);
    st.ba = mk3(s[13], s[14], s[15]);
    return st;
}
__device__ __forceinline__ void store_state(const nav_state &st, double *s) {
    s[0] = st.p.x, s[1] = st.p.y, s[2] = st.p.z;
    s[3] = st.q.x, s[4] = st.q.y, s[5] = st.q.z, s[6] = st.q.w;
    s[7] = st.v.x, s[8] = st.v.y, s[9] = st.v.z;
    s[10] = st.bg.x, s[11] = st.bg.y, s[12] = st.bg.z;
    s[13] = st.ba.x, s[14] = st.ba.y, s[15] = st.ba.z;
}
} // namespace

#define PI_IDX(i, j) ((i) * 15 + (j))
// rows of phi in descending order of their number of structural non-zeros: v (7), attitude (4), p (2), bg, ba (1)
#define ROWMAP(r) ((r) < 6 ? (r) + 3 : ((r) < 9 ? (r) - 6 : (r)))

// params_stride: doubles between the parameter rows of two intervals (icg_preint_batch_params: 9), 0 = one row for the whole launch
// (icg_preint_batch).  The row address depends on the workgroup index alone: wave-uniform, so the nine values stay scalar loads.
__global__ __launch_bounds__(64) void k_preint(int variant, const int32_t *offsets, const double *imu, const double *state0,
                                               const double *params_rows, int params_stride, double *cur_state, double *delta_state,
                                               double *jac_out, double *cov_out, double *delta_time_out, double *pn_out) {
    __shared__ double J[225], P[225], M[225], T1[225], T2[225], T3[225], PV[15 * 7];
    const int s = blockIdx.x, lane = threadIdx.x;
    const int begin = offsets[s], n = offsets[s + 1] - offsets[s];
    const double *params = params_rows + (size_t) s * (size_t) params_stride;
    const double gyr_arw = params[0], acc_vrw = params[1], gbstd = params[2], abstd = params[3], corr_time = params[4];
    const d3 gravity = mk3(0, 0, params[5]);
    const d3 iewn    = mk3(params[6], params[7], params[8]);
    nav_state cur = load_state(state0 + 16 * (size_t) s);
    nav_state del;
    del.p = del.v = mk3(0, 0, 0);
    del.q         = dq{0, 0, 0, 1};
    del.bg        = cur.bg;
    del.ba        = cur.ba;
    const dq q0   = cur.q;
    double delta_time = 0;
    double noise[12];
#pragma unroll
    for (int i = 0; i < 3; i++) {
        noise[i]     = gyr_arw * gyr_arw;
        noise[3 + i] = acc_vrw * acc_vrw;
        noise[6 + i] = 2 * gbstd * gbstd / corr_time;
        noise[9 + i] = 2 * abstd * abstd / corr_time;
    }
    for (int e = lane; e < 225; e += 64) {
        J[e] = (e / 15 == e % 15) ? 1.0 : 0.0;
        P[e] = 0.0;
    }
    __syncthreads();

    for (int index = 1; index < n; index++) {
        const double *pp = imu + 8 * (size_t) (begin + index - 1), *pc = imu + 8 * (size_t) (begin + index);
        d3 pre_dtheta = mk3(pp[2], pp[3], pp[4]), pre_dvel = mk3(pp[5], pp[6], pp[7]);
        d3 cur_dtheta = mk3(pc[2], pc[3], pc[4]), cur_dvel = mk3(pc[5], pc[6], pc[7]);
        const double pre_dt = pp[1], dt = pc[1];
        pre_dtheta = sub(pre_dtheta, scl(pre_dt, del.bg));
        pre_dvel   = sub(pre_dvel, scl(pre_dt, del.ba));
        cur_dtheta = sub(cur_dtheta, scl(dt, del.bg));
        cur_dvel   = sub(cur_dvel, scl(dt, del.ba));
        delta_time += dt;
        d3 dvfb   = add(add(cur_dvel, scl(0.5, crs(cur_dtheta, cur_dvel))),
                        scl(1.0 / 12.0, add(crs(pre_dtheta, cur_dvel), crs(pre_dvel, cur_dtheta))));
        d3 dtheta = add(cur_dtheta, scl(1.0 / 12.0, crs(pre_dtheta, cur_dtheta)));
        m33 blk36, blk312; // phi(3,6) and phi(3,12) blocks
        m33 gblk;          // gt(3,3) block
        double g60;        // gt(6,0) diagonal sign
        if (variant == 0) {
            d3 dvel = add(m_vec(q_mat(cur.q), dvfb), scl(dt, gravity));
            cur.p   = add(add(cur.p, scl(dt, cur.v)), scl(0.5 * dt, dvel));
            cur.v   = add(cur.v, dvel);
            cur.q   = q_normalized(q_mul(cur.q, rotvec2quat(dtheta)));
            dvel    = m_vec(q_mat(del.q), dvfb);
            del.p   = add(add(del.p, scl(dt, del.v)), scl(0.5 * dt, dvel));
            del.v   = add(del.v, dvel);
            del.q   = q_normalized(q_mul(del.q, rotvec2quat(dtheta)));
            m33 Rq  = q_mat(del.q);
            blk36   = m_mul(m_neg(Rq), m_skew(cur_dvel));
            blk312  = m_scale(m_neg(Rq), dt);
            gblk    = Rq;
            g60     = 1.0;
        } else {
            d3 dv_cor_g = scl(dt, sub(gravity, scl(2.0, crs(iewn, cur.v))));
            d3 dnn      = scl(dt, neg3(iewn));
            dq qnn      = rotvec2quat(dnn);
            m33 half    = m_scale(m_add(m_eye(), q_mat(qnn)), 0.5);
            d3 dvel     = add(m_vec(m_mul(half, q_mat(cur.q)), dvfb), dv_cor_g);
            cur.p       = add(add(cur.p, scl(dt, cur.v)), scl(0.5 * dt, dvel));
            cur.v       = add(cur.v, dvel);
            if (pn_out && lane == 0) { // pn_ (earth :235): (dt, position) per sample, row begin+index-1
                double *pn = pn_out + 4 * (size_t) (begin + index - 1);
                pn[0] = dt, pn[1] = cur.p.x, pn[2] = cur.p.y, pn[3] = cur.p.z;
            }
            cur.q       = q_normalized(q_mul(q_mul(qnn, cur.q), rotvec2quat(dtheta)));
            dnn         = scl(-(delta_time - 0.5 * dt), iewn);
            dvel        = m_vec(q_mat(q_mul(q_mul(q_mul(q_inv(q0), rotvec2quat(dnn)), q0), del.q)), dvfb);
            del.p       = add(add(del.p, scl(dt, del.v)), scl(0.5 * dt, dvel));
            del.v       = add(del.v, dvel);
            del.q       = q_normalized(q_mul(del.q, rotvec2quat(dtheta)));
            d3 dnn2     = scl(delta_time, neg3(iewn));
            m33 cbb0    = m_neg(q_mat(q_mul(q_mul(q_mul(q_inv(q0), rotvec2quat(dnn2)), q0), del.q)));
            blk36       = m_mul(cbb0, m_skew(cur_dvel));
            blk312      = m_scale(cbb0, dt);
            gblk        = cbb0;
            g60         = -1.0;
        }
        // ---- sparse rows of phi (<= 7 structural non-zeros, ascending k) by lanes 0..14; G Q G^T (block diagonal) by everyone ----
        const m33 sk  = m_skew(cur_dtheta);
        const double decay = 1 - dt / corr_time;
        if (lane < 15) {
            const int i = lane, bi = i / 3, ii = i - bi * 3;
            // values only; the column of term t follows from the row's class (see PHI_ROW_TERMS below):
            //   p rows:   k = i, 3+ii            v rows:  k = 3+ii, 6, 7, 8, 12, 13, 14
            //   att rows: k = 6, 7, 8, 9+ii      bg / ba: k = i
            double *pv = &PV[i * 7];
            if (bi == 0) {
                pv[0] = 1.0, pv[1] = dt;
            } else if (bi == 1) {
                pv[0] = 1.0;
                for (int kk = 0; kk < 3; kk++) pv[1 + kk] = blk36.a[ii * 3 + kk], pv[4 + kk] = blk312.a[ii * 3 + kk];
            } else if (bi == 2) {
                for (int kk = 0; kk < 3; kk++) pv[kk] = ((ii == kk) ? 1.0 : 0.0) - sk.a[ii * 3 + kk];
                pv[3] = -dt;
            } else {
                pv[0] = decay;
            }
        }
        for (int e = lane; e < 225; e += 64) {
            const int i = e / 15, j = e - i * 15;
            const int bi = i / 3, bj = j / 3, ii = i - bi * 3, jj = j - bj * 3;
            double m = 0;
            // m = sum_k gt[i][k] * noise[k] * gt[j][k] over the structural non-zeros of both rows (gt: v rows = gblk on the accelerometer
            // noise, attitude rows = +-1 on the gyroscope noise, bg / ba rows = 1 on their random-walk noise)
            if (bi == bj) {
                if (bi == 1) {
#pragma unroll
                    for (int k = 0; k < 3; k++) m += gblk.a[ii * 3 + k] * noise[3 + k] * gblk.a[jj * 3 + k];
                } else if (bi == 2) {
                    if (ii == jj) m += g60 * noise[ii] * g60;
                } else if (bi == 3) {
                    if (ii == jj) m += 1.0 * noise[6 + ii] * 1.0;
                } else if (bi == 4) {
                    if (ii == jj) m += 1.0 * noise[9 + ii] * 1.0;
                }
            }
            M[e] = m;
        }
        __syncthreads();
        // ---- pass 1, entries sorted by the class of their ROW: T1 = phi*J, T2 = phi*P, T3 = phi*M ----
        // every class is straight-line code with constant column offsets: all LDS loads of an entry are independent and in flight together
        for (int e = lane; e < 225; e += 64) {
            const int i = ROWMAP(e / 15), j = e % 15;
            const int bi = i / 3, ii = i - bi * 3;
            const double *pv = &PV[i * 7];
            double a = 0, b = 0, t1 = 0;
#define PHI_TERM(k, val)                                                                                                               \
    {                                                                                                                                  \
        const double phv = (val);                                                                                                      \
        a += phv * J[PI_IDX(k, j)];                                                                                                    \
        b += phv * P[PI_IDX(k, j)];                                                                                                    \
        t1 += phv * M[PI_IDX(k, j)];                                                                                                   \
    }
            if (bi == 1) {
                PHI_TERM(3 + ii, pv[0]) PHI_TERM(6, pv[1]) PHI_TERM(7, pv[2]) PHI_TERM(8, pv[3]) PHI_TERM(12, pv[4]) PHI_TERM(13, pv[5])
                PHI_TERM(14, pv[6])
            } else if (bi == 2) {
                PHI_TERM(6, pv[0]) PHI_TERM(7, pv[1]) PHI_TERM(8, pv[2]) PHI_TERM(9 + ii, pv[3])
            } else if (bi == 0) {
                PHI_TERM(i, pv[0]) PHI_TERM(3 + ii, pv[1])
            } else {
                PHI_TERM(i, pv[0])
            }
#undef PHI_TERM
            T1[PI_IDX(i, j)] = a;
            T2[PI_IDX(i, j)] = b;
            T3[PI_IDX(i, j)] = t1;
        }
        __syncthreads();
        // ---- pass 2, entries sorted by the class of their COLUMN: J = T1 ; P = T2*phi^T + 0.5 dt (phi*M + M*phi^T) ----
        for (int e = lane; e < 225; e += 64) {
            const int j = ROWMAP(e / 15), i = e % 15;
            const int bj = j / 3, jj = j - bj * 3;
            const double *pv = &PV[j * 7];
            double pc2 = 0, t2 = 0;
#define PHIT_TERM(k, val)                                                                                                              \
    {                                                                                                                                  \
        const double phv = (val);                                                                                                      \
        pc2 += T2[PI_IDX(i, k)] * phv;                                                                                                 \
        t2 += M[PI_IDX(i, k)] * phv;                                                                                                   \
    }
            if (bj == 1) {
                PHIT_TERM(3 + jj, pv[0]) PHIT_TERM(6, pv[1]) PHIT_TERM(7, pv[2]) PHIT_TERM(8, pv[3]) PHIT_TERM(12, pv[4]) PHIT_TERM(13, pv[5])
                PHIT_TERM(14, pv[6])
            } else if (bj == 2) {
                PHIT_TERM(6, pv[0]) PHIT_TERM(7, pv[1]) PHIT_TERM(8, pv[2]) PHIT_TERM(9 + jj, pv[3])
            } else if (bj == 0) {
                PHIT_TERM(j, pv[0]) PHIT_TERM(3 + jj, pv[1])
            } else {
                PHIT_TERM(j, pv[0])
            }
#undef PHIT_TERM
            J[PI_IDX(i, j)] = T1[PI_IDX(i, j)];
            P[PI_IDX(i, j)] = pc2 + 0.5 * dt * (T3[PI_IDX(i, j)] + t2);
        }
        __syncthreads();
    }
    for (int e = lane; e < 225; e += 64) {
        jac_out[225 * (size_t) s + e] = J[e];
        cov_out[225 * (size_t) s + e] = P[e];
    }
    if (lane == 0) {
        store_state(cur, cur_state + 16 * (size_t) s);
        store_state(del, delta_state + 16 * (size_t) s);
        delta_time_out[s] = delta_time;
    }
}

// ================================================================ P2 ================================================================
// The bodies are preint_shared.h's, instantiated for the 15-wide state.
__global__ __launch_bounds__(64) void k_preint_sqrt_info(int n, const double *cov, double *sqrt_info, int32_t *status) {
    sqrt_info_body<15>(n, cov, sqrt_info, status);
}

__global__ __launch_bounds__(64) void k_preint_evaluate(int variant, int n, const double *delta_state, const double *jac, const double *delta_time,
                                                        const double *env, const int32_t *pn_offsets, const double *pn, const double *points,
                                                        const double *sqrt_info, const int32_t *status, double *residuals, double *jacobians) {
    evaluate_body<15, false>(variant, n, delta_state, jac, delta_time, env, pn_offsets, pn, points, sqrt_info, status, nullptr, nullptr, residuals,
                             jacobians, nullptr);
}

// the resident set's instantiation: the variant is the factor's own
__global__ __launch_bounds__(64) void k_preint_evaluate_given(int n, const int32_t *variant, const double *delta_state, const double *jac,
                                                              const double *delta_time, const double *env, const int32_t *pn_offsets, const double *pn,
                                                              const double *points, const double *sqrt_info, const double *q_corr, const double *q_nn,
                                                              double *residuals, double *jacobians, double *sq_norm) {
    evaluate_body<15, true>(blockIdx.x < (unsigned) n ? variant[blockIdx.x] : 0, n, delta_state, jac, delta_time, env, pn_offsets, pn, points, sqrt_info,
                            nullptr, q_corr, q_nn, residuals, jacobians, sq_norm);
}

// ================================================================ the C entries ================================================================
static const kernels<15> K15 = {k_preint, k_preint_sqrt_info, k_preint_evaluate, k_preint_evaluate_given};

extern "C" int icg_preint_batch(icg_ctx *ctx, int variant, int n_intervals, const int32_t *offsets, const double *imu,
                                const double *state0, const double *params, double *cur_state, double *delta_state, double *jac,
                                double *cov, double *delta_time, double *pn) {
    return batch_entry(K15, "batch", false, ctx, variant, n_intervals, offsets, imu, state0, params, cur_state, delta_state, jac, cov, delta_time, pn,
                       nullptr, nullptr);
}

extern "C" int icg_preint_batch_params(icg_ctx *ctx, int variant, int n_intervals, const int32_t *offsets, const double *imu,
                                       const double *state0, const double *params, double *cur_state, double *delta_state, double *jac,
                                       double *cov, double *delta_time, double *pn, double *sqrt_info, int32_t *status) {
    return batch_entry(K15, "batch_params", true, ctx, variant, n_intervals, offsets, imu, state0, params, cur_state, delta_state, jac, cov, delta_time,
                       pn, sqrt_info, status);
}

extern "C" int icg_preint_evaluate_batch(icg_ctx *ctx, int variant, int n_factors, const double *delta_state, const double *jac,
                                         const double *cov, const double *delta_time, const double *env, const int32_t *pn_offsets,
                                         const double *pn, const double *points, double *residuals, double *jacobians, double *sqrt_info,
                                         int32_t *status) {
    return evaluate_batch_entry(K15, ctx, variant, n_factors, delta_state, jac, cov, delta_time, env, pn_offsets, pn, points, residuals, jacobians,
                                sqrt_info, status);
}

extern "C" int icg_preint_set(icg_ctx *ctx, int n_factors, const int32_t *variant, const double *delta_state, const double *jac, const double *sqrt_info,
                              const double *delta_time, const double *env, const double *q_nn, const int32_t *pn_offsets, const double *pn) {
    return set_entry<15>(ctx, n_factors, variant, delta_state, jac, sqrt_info, delta_time, env, q_nn, pn_offsets, pn);
}

extern "C" int icg_preint_evaluate_resident(icg_ctx *ctx, const double *points, const double *q_corr, int want_jac, double *sq_norm) {
    return evaluate_resident_entry(K15, ctx, points, q_corr, want_jac, sq_norm);
}

extern "C" int icg_preint_fetch_resident(icg_ctx *ctx, double *residuals, double *jacobians) {
    return fetch_resident_entry<15>(ctx, residuals, jacobians);
}
