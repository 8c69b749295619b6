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
// P2: the factor evaluation on an integration result (second half of this file), batched over independent factors, one 64-lane wavefront
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
//   k_preint_evaluate_given  the same body for a set of factors RESIDENT on the device (icg_preint_set, last part of this file): the two
//                        rotvec2quat results and S come from the host, so nothing is left that may round differently; one launch per call.
// Latency bound like P1 (~8 KB in, ~4 KB out, a few thousand dependent FP64 operations per factor, no reuse across factors): reported as
// factors/s, not against the HBM roofline.
#include <algorithm>

#include "dev_math.h"
#include "icg_internal.h"

using namespace icgd;

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
__device__ __forceinline__ d3 neg3(d3 a) { return mk3(-a.x, -a.y, -a.z); }
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

extern "C" int icg_preint_batch(icg_ctx *ctx, int variant, int n_intervals, const int32_t *offsets, const double *imu,
                                const double *state0, const double *params, double *cur_state, double *delta_state, double *jac,
                                double *cov, double *delta_time, double *pn) {
    if (!ctx || n_intervals < 0 || (variant != 0 && variant != 1)) return ICG_ERR_INVALID;
    if (n_intervals == 0) return ICG_OK;
    if (!offsets || !imu || !state0 || !params || !cur_state || !delta_state || !jac || !cov || !delta_time) return ICG_ERR_INVALID;
    const int total = offsets[n_intervals];
    if (offsets[0] < 0) return icg_fail(ctx, ICG_ERR_INVALID, "offsets[0] = %d", offsets[0]);
    for (int s = 0; s < n_intervals; s++)
        if (offsets[s + 1] - offsets[s] < 1) return icg_fail(ctx, ICG_ERR_INVALID, "interval %d has no IMU sample", s);
    ICG_HIP(ctx, hipSetDevice(ctx->cfg.device));
    icg_call c(ctx);
    int rc = c.reserve((size_t) total * 96 + (size_t) n_intervals * (16 * 8 * 3 + 225 * 8 * 2 + 16) + 1024);
    if (rc) return rc;
    const int32_t *d_off = c.in(offsets, (size_t) n_intervals + 1);
    const double *d_imu  = c.in(imu, 8 * (size_t) total);
    const double *d_s0   = c.in(state0, 16 * (size_t) n_intervals);
    const double *d_par  = c.in(params, 9);
    if ((rc = c.seal())) return rc;
    double *d_cur = c.out_zc(cur_state, 16 * (size_t) n_intervals);
    double *d_del = c.out_zc(delta_state, 16 * (size_t) n_intervals);
    double *d_jac = c.out_zc(jac, 225 * (size_t) n_intervals);
    double *d_cov = c.out_zc(cov, 225 * (size_t) n_intervals);
    double *d_dt  = c.out_zc(delta_time, (size_t) n_intervals);
    // pn is written by the Earth variant only, rows begin .. begin + n - 2 of every interval: the Normal variant gets no buffer, and the one
    // row per interval that the kernel leaves alone is staged from the caller's, so that the copy back returns it unchanged
    double *d_pn  = (pn && variant == 1) ? c.out_zc(pn, 4 * (size_t) total) : nullptr;
    ICG_LAUNCH_GUARD(c);
    if (d_pn)
        for (int s = 0; s < n_intervals; s++) {
            const size_t last = 4 * ((size_t) offsets[s + 1] - 1);
            memcpy(d_pn + last, pn + last, 4 * sizeof(double));
        }
    {
        icg_prof_scope ps(ctx, "preint");
        hipLaunchKernelGGL(k_preint, dim3(n_intervals), dim3(64), 0, ctx->stream, variant, d_off, d_imu, d_s0, d_par, 0, d_cur, d_del,
                           d_jac, d_cov, d_dt, d_pn);
    }
    ICG_HIP(ctx, hipGetLastError());
    return c.finish();
}

__global__ __launch_bounds__(64) void k_preint_sqrt_info(int n, const double *cov, double *sqrt_info, int32_t *status);

// icg_preint_batch with one parameter row per interval, and (optionally) the square-root information of every result formed behind the
// integration.  cov is then a mirrored output: k_preint leaves it in the device arena, k_preint_sqrt_info reads it there, and one copy
// brings it down; S and status are written once per lane and go through the host mapping like the other outputs.
extern "C" int icg_preint_batch_params(icg_ctx *ctx, int variant, int n_intervals, const int32_t *offsets, const double *imu,
                                       const double *state0, const double *params, double *cur_state, double *delta_state, double *jac,
                                       double *cov, double *delta_time, double *pn, double *sqrt_info, int32_t *status) {
    if (!ctx) return ICG_ERR_INVALID;
    if (variant != 0 && variant != 1) return icg_fail(ctx, ICG_ERR_INVALID, "icg_preint_batch_params: variant %d is neither 0 (Normal) nor 1 (Earth)", variant);
    if (n_intervals < 0) return icg_fail(ctx, ICG_ERR_INVALID, "icg_preint_batch_params: n_intervals = %d", n_intervals);
    if (n_intervals == 0) return ICG_OK;
    if (!offsets || !imu || !state0 || !params || !cur_state || !delta_state || !jac || !cov || !delta_time)
        return icg_fail(ctx, ICG_ERR_INVALID, "icg_preint_batch_params: NULL argument");
    if (offsets[0] < 0) return icg_fail(ctx, ICG_ERR_INVALID, "icg_preint_batch_params: interval 0: offsets[0] = %d", offsets[0]);
    for (int s = 0; s < n_intervals; s++)
        if (offsets[s + 1] - offsets[s] < 1) return icg_fail(ctx, ICG_ERR_INVALID, "icg_preint_batch_params: interval %d has no IMU sample", s);
    const int total    = offsets[n_intervals];
    const size_t n     = (size_t) n_intervals;
    const bool want_S  = sqrt_info || status;
    ICG_HIP(ctx, hipSetDevice(ctx->cfg.device));
    icg_call c(ctx);
    int rc = c.reserve((size_t) total * 96 + n * (16 * 8 * 3 + 225 * 8 * 3 + 9 * 8 + 16 + 4) + 16 * 256);
    if (rc) return rc;
    const int32_t *d_off = c.in(offsets, n + 1);
    const double *d_imu  = c.in(imu, 8 * (size_t) total);
    const double *d_s0   = c.in(state0, 16 * n);
    const double *d_par  = c.in(params, 9 * n);
    if ((rc = c.seal())) return rc;
    double *d_cur = c.out_zc(cur_state, 16 * n);
    double *d_del = c.out_zc(delta_state, 16 * n);
    double *d_jac = c.out_zc(jac, 225 * n);
    double *d_dt  = c.out_zc(delta_time, n);
    double *d_pn  = (pn && variant == 1) ? c.out_zc(pn, 4 * (size_t) total) : nullptr; // (icg_preint_batch's rule)
    double *d_S   = want_S ? c.out_zc(sqrt_info, 225 * n) : nullptr;
    int32_t *d_st = want_S ? c.out_zc(status, n) : nullptr;
    double *d_cov = want_S ? c.out(cov, 225 * n) : c.out_zc(cov, 225 * n); // (last: no zero-copy region inside the span copied back)
    ICG_LAUNCH_GUARD(c);
    if (d_pn)
        for (int s = 0; s < n_intervals; s++) {
            const size_t last = 4 * ((size_t) offsets[s + 1] - 1);
            memcpy(d_pn + last, pn + last, 4 * sizeof(double));
        }
    {
        icg_prof_scope ps(ctx, "preint");
        hipLaunchKernelGGL(k_preint, dim3(n_intervals), dim3(64), 0, ctx->stream, variant, d_off, d_imu, d_s0, d_par, 9, d_cur, d_del,
                           d_jac, d_cov, d_dt, d_pn);
    }
    if (want_S) {
        icg_prof_scope ps(ctx, "preint_eval");
        hipLaunchKernelGGL(k_preint_sqrt_info, dim3(n_intervals), dim3(64), 0, ctx->stream, n_intervals, d_cov, d_S, d_st);
    }
    ICG_HIP(ctx, hipGetLastError());
    return c.finish();
}

// ================================================================ P2 ================================================================
namespace {
// the host layer's P2 scales the axis by the reciprocal of the angle (dev_math.h's rotvec2quat, used by P1, divides): same order here
__device__ __forceinline__ dq rotvec2quat_rcp(d3 rv) {
    double angle = sqrt(rv.x * rv.x + rv.y * rv.y + rv.z * rv.z);
    d3 axis      = rv;
    if (angle > 0) axis = scl(1.0 / angle, rv);
    double s = sin(0.5 * angle), c = cos(0.5 * angle);
    return dq{s * axis.x, s * axis.y, s * axis.z, c};
}
__device__ __forceinline__ d3 q_vec(dq q) { return mk3(q.x, q.y, q.z); }
// bottom-right 3x3 of quaternionleft(q) / quaternionright(q) (rotation.h:103-119)
__device__ __forceinline__ m33 qleft_br(dq q) { return m_add(m_scale(m_eye(), q.w), m_skew(q_vec(q))); }
__device__ __forceinline__ m33 qright_br(dq q) { return m_add(m_scale(m_eye(), q.w), m_scale(m_skew(q_vec(q)), -1.0)); }
// bottom-right 3x3 of quaternionleft(a) * quaternionright(b): the 4-term sums over k ascending
__device__ __forceinline__ m33 qleft_qright_br(dq a, dq b) {
    double L[4][4], R[4][4];
    L[0][0] = a.w, L[0][1] = -a.x, L[0][2] = -a.y, L[0][3] = -a.z, L[1][0] = a.x, L[2][0] = a.y, L[3][0] = a.z;
    R[0][0] = b.w, R[0][1] = -b.x, R[0][2] = -b.y, R[0][3] = -b.z, R[1][0] = b.x, R[2][0] = b.y, R[3][0] = b.z;
    const m33 sa = m_skew(q_vec(a)), sb = m_skew(q_vec(b));
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            L[1 + i][1 + j] = (i == j ? a.w : 0.0) + 1.0 * sa.a[i * 3 + j];
            R[1 + i][1 + j] = (i == j ? b.w : 0.0) + -1.0 * sb.a[i * 3 + j];
        }
    m33 out;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            double s = 0;
#pragma unroll
            for (int k = 0; k < 4; k++) s += L[1 + i][k] * R[k][1 + j];
            out.a[i * 3 + j] = s;
        }
    return out;
}
} // namespace

#define PE_W 30         // row length of the augmented matrix
#define PE_U 33         // row length of the unwhitened block: 32 Jacobian columns (7 | 9 | 7 | 9) + the residual
#define PE_NOUT (15 + 480)

__global__ __launch_bounds__(64) void k_preint_sqrt_info(int n, const double *cov, double *sqrt_info, int32_t *status) {
    __shared__ double w[15 * PE_W], L[225], fcol[15];
    const int f = blockIdx.x, lane = threadIdx.x;
    if (f >= n) return;
    const double *C = cov + 225 * (size_t) f;
    double *S       = sqrt_info + 225 * (size_t) f;
    for (int e = lane; e < 15 * PE_W; e += 64) {
        const int i = e / PE_W, j = e - i * PE_W;
        w[e]        = j < 15 ? C[i * 15 + j] : (i == j - 15 ? 1.0 : 0.0);
    }
    for (int e = lane; e < 225; e += 64) L[e] = 0.0;
    __syncthreads();
    for (int c = 0; c < 15; c++) {
        // first row r >= c of maximal |w[r][c]| (ties to the lower index): lanes c..14 hold a candidate, the others one that never wins
        const bool cand = lane >= c && lane < 15;
        double best     = cand ? fabs(w[lane * PE_W + c]) : -1.0;
        int piv         = cand ? lane : 15;
#pragma unroll
        for (int m = 8; m >= 1; m >>= 1) {
            const double ob = __shfl_xor(best, m);
            const int op    = __shfl_xor(piv, m);
            if (ob > best || (ob == best && op < piv)) best = ob, piv = op;
        }
        piv = __shfl(piv, 0);
        if (piv < c || piv > 14) piv = c; // (a NaN column compares false everywhere: the host keeps row c)
        if (w[piv * PE_W + c] == 0.0) {   // uniform: singular covariance
            for (int e = lane; e < 225; e += 64) S[e] = 0.0;
            if (lane == 0) status[f] = 1;
            return;
        }
        if (piv != c && lane < PE_W) {
            const double a = w[c * PE_W + lane], b = w[piv * PE_W + lane];
            w[c * PE_W + lane] = b, w[piv * PE_W + lane] = a;
        }
        __syncthreads();
        const double d = w[c * PE_W + c];
        __syncthreads();
        if (lane < PE_W) w[c * PE_W + lane] /= d;
        if (lane < 15) fcol[lane] = w[lane * PE_W + c]; // (row c's own entry is not used)
        __syncthreads();
        for (int e = lane; e < 15 * PE_W; e += 64) {
            const int r = e / PE_W, j = e - r * PE_W;
            const double fr = fcol[r];
            if (r != c && fr != 0.0) w[e] -= fr * w[c * PE_W + j];
        }
        __syncthreads();
    }
    // inverse = right half, lower triangle mirrored; column Cholesky, lane i owns row i: t = inv[i][j] - sum_k L[i][k] L[j][k], k ascending
    const int i = lane < 15 ? lane : 14;
    for (int j = 0; j < 15; j++) {
        double t = w[(i >= j ? i : j) * PE_W + 15 + (i >= j ? j : i)];
        for (int k = 0; k < j; k++) t -= L[i * 15 + k] * L[j * 15 + k];
        const double ljj = sqrt(__shfl(t, j));
        if (lane < 15 && lane >= j) L[lane * 15 + j] = lane == j ? ljj : t / ljj;
        __syncthreads();
    }
    for (int e = lane; e < 225; e += 64) S[e] = L[(e % 15) * 15 + e / 15];
    if (lane == 0) status[f] = 0;
}

// The one evaluation body.  GIVEN = false: icg_preint_evaluate_batch (status from k_preint_sqrt_info, rotvec2quat on the device, Jacobians
// in the four blocks).  GIVEN = true: icg_preint_evaluate_resident — the two quaternions that need sin / cos / sqrt arrive from the host
// (q_corr per evaluation point, q_nn with the set), so what is left is + - * / in the host's order; the Jacobian is one row-major 15 x 32
// matrix per factor (the columns of U; 6 and 22 are sums of +-0 from +0.0, i.e. +0.0, like the host's seventh pose columns) and lane 0 adds
// sq_norm = sum_k r[k]^2, k ascending from +0.0.  status / sq_norm / q_corr / q_nn are not read by the instantiation that does not use them.
template <bool GIVEN>
__device__ __forceinline__ void preint_evaluate_body(int variant, int n, const double *delta_state, const double *jac, const double *delta_time,
                                                     const double *env, const int32_t *pn_offsets, const double *pn, const double *points,
                                                     const double *sqrt_info, const int32_t *status, const double *q_corr, const double *q_nn,
                                                     double *residuals, double *jacobians, double *sq_norm) {
    __shared__ double S[225], U[15 * PE_U];
    const int f = blockIdx.x, lane = threadIdx.x;
    if (f >= n) return;
    double *r_out = residuals + 15 * (size_t) f;
    double *J_out = jacobians ? jacobians + 480 * (size_t) f : nullptr;
    if (!GIVEN && status[f] != 0) { // singular covariance: zero rows
        for (int o = lane; o < PE_NOUT; o += 64) {
            if (o < 15)
                r_out[o] = 0.0;
            else if (J_out)
                J_out[o - 15] = 0.0;
        }
        return;
    }
    for (int e = lane; e < 225; e += 64) S[e] = sqrt_info[225 * (size_t) f + e];
    for (int e = lane; e < 15 * PE_U; e += 64) U[e] = 0.0;
    __syncthreads();

    const double *J15 = jac + 225 * (size_t) f, *pt = points + 32 * (size_t) f;
    const nav_state d = load_state(delta_state + 16 * (size_t) f);
    const d3 p0 = mk3(pt[0], pt[1], pt[2]), p1 = mk3(pt[16], pt[17], pt[18]);
    const dq q0 = q_from_xyzw(pt + 3), q1 = q_from_xyzw(pt + 19);
    const d3 v0 = mk3(pt[7], pt[8], pt[9]), bg0 = mk3(pt[10], pt[11], pt[12]), ba0 = mk3(pt[13], pt[14], pt[15]);
    const d3 v1 = mk3(pt[23], pt[24], pt[25]), bg1 = mk3(pt[26], pt[27], pt[28]), ba1 = mk3(pt[29], pt[30], pt[31]);
    const d3 gravity = mk3(0, 0, env[4 * (size_t) f]);
    const d3 iewn    = mk3(env[4 * (size_t) f + 1], env[4 * (size_t) f + 2], env[4 * (size_t) f + 3]);
    m33 dp_dbg, dp_dba, dv_dbg, dv_dba, dq_dbg;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            dp_dbg.a[i * 3 + j] = J15[PI_IDX(i, 9 + j)];
            dp_dba.a[i * 3 + j] = J15[PI_IDX(i, 12 + j)];
            dv_dbg.a[i * 3 + j] = J15[PI_IDX(3 + i, 9 + j)];
            dv_dba.a[i * 3 + j] = J15[PI_IDX(3 + i, 12 + j)];
            dq_dbg.a[i * 3 + j] = J15[PI_IDX(6 + i, 9 + j)];
        }
    const d3 dbg = sub(bg0, d.bg), dba = sub(ba0, d.ba);
    const d3 corrected_p = add(add(d.p, m_vec(dp_dba, dba)), m_vec(dp_dbg, dbg));
    const d3 corrected_v = add(add(d.v, m_vec(dv_dba, dba)), m_vec(dv_dbg, dbg));
    dq q_c;
    if (GIVEN)
        q_c = q_from_xyzw(q_corr + 4 * (size_t) f);
    else
        q_c = rotvec2quat_rcp(m_vec(dq_dbg, dbg));
    const dq corrected_q = q_mul(d.q, q_c);
    const double T       = delta_time[f];
    const m33 cnb0       = q_mat(q_inv(q0));
    const d3 half_g_TT   = scl(T, scl(T, scl(0.5, gravity))); // ((0.5 g) T) T
    d3 rp, rv;
    dq qe;
    // the blocks that differ between the variants: J0(0,0) J0(0,3) J0(3,0) J0(3,3) J0(6,3) | J2(3,0) J2(6,3) | J1(6,3)
    m33 j0_00, j0_03, j0_30, j0_33, j0_63, j2_30, j2_63, j1_63;
    if (variant == 0) {
        const d3 dpn = sub(sub(sub(p1, p0), scl(T, v0)), half_g_TT);
        const d3 dvn = sub(sub(v1, v0), scl(T, gravity));
        const d3 rdp = q_rot(q_inv(q0), dpn), rdv = q_rot(q_inv(q0), dvn);
        rp = sub(rdp, corrected_p), rv = sub(rdv, corrected_v);
        qe    = q_mul(q_mul(q_inv(corrected_q), q_inv(q0)), q1);
        j0_00 = m_scale(cnb0, -1.0);
        j0_03 = m_skew(rdp);
        j0_33 = m_skew(rdv);
        j0_63 = m_scale(qleft_qright_br(q_mul(q_inv(q1), q0), corrected_q), -1.0);
        j2_63 = qleft_br(qe);
        j1_63 = m_mul(m_scale(qleft_br(q_mul(q_mul(q_inv(q1), q0), d.q)), -1.0), dq_dbg);
    } else {
        const m33 iewn_skew = m_skew(iewn);
        d3 p_cor            = mk3(0, 0, 0);
        for (int k = pn_offsets[f]; k < pn_offsets[f + 1]; k++) {
            const double *row = pn + 4 * (size_t) k;
            p_cor             = add(p_cor, scl(row[0], sub(mk3(row[1], row[2], row[3]), p0)));
        }
        p_cor          = m_vec(m_scale(iewn_skew, 2.0), p_cor);
        const d3 v_cor = m_vec(m_scale(iewn_skew, 2.0), sub(p1, p0));
        dq qnn;
        if (GIVEN)
            qnn = q_from_xyzw(q_nn + 4 * (size_t) f);
        else
            qnn = rotvec2quat_rcp(scl(T, neg3(iewn)));
        const d3 dpn   = add(sub(sub(sub(p1, p0), scl(T, v0)), half_g_TT), p_cor);
        const d3 dvn   = add(sub(sub(v1, v0), scl(T, gravity)), v_cor);
        const dq qb0b1 = q_mul(q_mul(q_inv(q1), qnn), q0);
        const d3 rdp = m_vec(cnb0, dpn), rdv = m_vec(cnb0, dvn);
        rp = sub(rdp, corrected_p), rv = sub(rdv, corrected_v);
        qe    = q_mul(qb0b1, corrected_q);
        j0_00 = m_add(m_scale(cnb0, -1.0), m_scale(m_mul(m_scale(cnb0, 2.0), iewn_skew), -T));
        j0_03 = m_skew(rdp);
        j0_30 = m_mul(m_scale(cnb0, -2.0), iewn_skew);
        j0_33 = m_skew(rdv);
        j0_63 = qleft_qright_br(qb0b1, corrected_q);
        j2_30 = m_mul(m_scale(cnb0, 2.0), iewn_skew);
        j2_63 = m_scale(qright_br(qe), -1.0);
        j1_63 = m_mul(qleft_br(q_mul(qb0b1, d.q)), dq_dbg);
    }
    const d3 rbg = sub(bg1, bg0), rba = sub(ba1, ba0);
    if (lane == 0) {
        // block (r0, c0) of the 15 x 32 Jacobian [J0 (cols 0..6) | J1 (7..15) | J2 (16..22) | J3 (23..31)]; column 32 = residual
#define PE_PUT(r0, c0, blk)                                                                                                            \
    {                                                                                                                                  \
        const m33 b_ = (blk);                                                                                                          \
        _Pragma("unroll") for (int i_ = 0; i_ < 3; i_++) _Pragma("unroll") for (int j_ = 0; j_ < 3; j_++)                               \
            U[((r0) + i_) * PE_U + (c0) + j_] = b_.a[i_ * 3 + j_];                                                                     \
    }
        const double rr[15] = {rp.x, rp.y, rp.z, rv.x, rv.y, rv.z, 2 * qe.x, 2 * qe.y, 2 * qe.z, rbg.x, rbg.y, rbg.z, rba.x, rba.y, rba.z};
#pragma unroll
        for (int k = 0; k < 15; k++) U[k * PE_U + 32] = rr[k];
        if (jacobians) {
            PE_PUT(0, 0, j0_00)
            PE_PUT(0, 3, j0_03)
            PE_PUT(3, 3, j0_33)
            PE_PUT(6, 3, j0_63)
            PE_PUT(0, 16, cnb0)
            PE_PUT(6, 16 + 3, j2_63)
            if (variant != 0) {
                PE_PUT(3, 0, j0_30)
                PE_PUT(3, 16, j2_30)
            }
            PE_PUT(0, 7, m_scale(cnb0, -T))
            PE_PUT(0, 7 + 3, m_scale(dp_dbg, -1.0))
            PE_PUT(0, 7 + 6, m_scale(dp_dba, -1.0))
            PE_PUT(3, 7, m_scale(cnb0, -1.0))
            PE_PUT(3, 7 + 3, m_scale(dv_dbg, -1.0))
            PE_PUT(3, 7 + 6, m_scale(dv_dba, -1.0))
            PE_PUT(6, 7 + 3, j1_63)
            PE_PUT(9, 7 + 3, m_scale(m_eye(), -1.0))
            PE_PUT(12, 7 + 6, m_scale(m_eye(), -1.0))
            PE_PUT(3, 23, cnb0)
            PE_PUT(9, 23 + 3, m_eye())
            PE_PUT(12, 23 + 6, m_eye())
        }
#undef PE_PUT
    }
    __syncthreads();
    // whitening: out[i][col] = sum_k S[i][k] U[k][col], dense, k ascending from zero
    const int n_out = jacobians ? PE_NOUT : 15;
    double r_mine   = 0;
    for (int o = lane; o < n_out; o += 64) {
        int i, col;
        double *dst;
        if (o < 15) {
            i = o, col = 32, dst = r_out + o;
        } else {
            const int q = o - 15;
            dst         = J_out + q;
            if (GIVEN)
                i = q >> 5, col = q & 31;
            else if (q < 105)
                i = q / 7, col = q - i * 7;
            else if (q < 240)
                i = (q - 105) / 9, col = 7 + (q - 105) - i * 9;
            else if (q < 345)
                i = (q - 240) / 7, col = 16 + (q - 240) - i * 7;
            else
                i = (q - 345) / 9, col = 23 + (q - 345) - i * 9;
        }
        double s = 0;
#pragma unroll
        for (int k = 0; k < 15; k++) s += S[i * 15 + k] * U[k * PE_U + col];
        *dst = s;
        if (GIVEN && o < 15) r_mine = s; // (o == lane: the first pass of lanes 0 .. 14)
    }
    if (GIVEN) {
        __shared__ double R[15];
        if (lane < 15) R[lane] = r_mine;
        __syncthreads();
        if (lane == 0) {
            double s = 0;
            for (int k = 0; k < 15; k++) s += R[k] * R[k];
            sq_norm[f] = s;
        }
    }
}

__global__ __launch_bounds__(64) void k_preint_evaluate(int variant, int n, const double *delta_state, const double *jac, const double *delta_time,
                                                        const double *env, const int32_t *pn_offsets, const double *pn, const double *points,
                                                        const double *sqrt_info, const int32_t *status, double *residuals, double *jacobians) {
    preint_evaluate_body<false>(variant, n, delta_state, jac, delta_time, env, pn_offsets, pn, points, sqrt_info, status, nullptr, nullptr, residuals,
                                jacobians, nullptr);
}

// the resident set's instantiation: the variant is the factor's own
__global__ __launch_bounds__(64) void k_preint_evaluate_given(int n, const int32_t *variant, const double *delta_state, const double *jac,
                                                              const double *delta_time, const double *env, const int32_t *pn_offsets, const double *pn,
                                                              const double *points, const double *sqrt_info, const double *q_corr, const double *q_nn,
                                                              double *residuals, double *jacobians, double *sq_norm) {
    preint_evaluate_body<true>(blockIdx.x < (unsigned) n ? variant[blockIdx.x] : 0, n, delta_state, jac, delta_time, env, pn_offsets, pn, points, sqrt_info,
                               nullptr, q_corr, q_nn, residuals, jacobians, sq_norm);
}

extern "C" int icg_preint_evaluate_batch(icg_ctx *ctx, int variant, int n_factors, const double *delta_state, const double *jac,
                                         const double *cov, const double *delta_time, const double *env, const int32_t *pn_offsets,
                                         const double *pn, const double *points, double *residuals, double *jacobians, double *sqrt_info,
                                         int32_t *status) {
    if (!ctx) return ICG_ERR_INVALID;
    if (variant != 0 && variant != 1) return icg_fail(ctx, ICG_ERR_INVALID, "icg_preint_evaluate_batch: variant %d is neither 0 (Normal) nor 1 (Earth)", variant);
    if (n_factors <= 0) return icg_fail(ctx, ICG_ERR_INVALID, "icg_preint_evaluate_batch: n_factors = %d", n_factors);
    if (!delta_state || !jac || !cov || !delta_time || !env || !points || !residuals || !status)
        return icg_fail(ctx, ICG_ERR_INVALID, "icg_preint_evaluate_batch: NULL argument");
    int total_pn = 0;
    if (variant == 1) {
        if (!pn_offsets) return icg_fail(ctx, ICG_ERR_INVALID, "icg_preint_evaluate_batch: the Earth variant needs pn_offsets");
        if (pn_offsets[0] < 0) return icg_fail(ctx, ICG_ERR_INVALID, "icg_preint_evaluate_batch: pn_offsets[0] = %d", pn_offsets[0]);
        for (int k = 0; k < n_factors; k++)
            if (pn_offsets[k + 1] < pn_offsets[k]) return icg_fail(ctx, ICG_ERR_INVALID, "icg_preint_evaluate_batch: pn_offsets not monotone at factor %d", k);
        total_pn = pn_offsets[n_factors];
        if (total_pn > 0 && !pn) return icg_fail(ctx, ICG_ERR_INVALID, "icg_preint_evaluate_batch: NULL pn");
    }
    const size_t n = (size_t) n_factors;
    ICG_HIP(ctx, hipSetDevice(ctx->cfg.device));
    icg_call c(ctx);
    int rc = c.reserve(n * 8 * (16 + 225 + 225 + 1 + 4 + 32 + 15 + 480 + 225 + 1) + (n + 1) * 4 + (size_t) total_pn * 32 + 16 * 256);
    if (rc) return rc;
    const double *d_del = c.in(delta_state, 16 * n);
    const double *d_jac = c.in(jac, 225 * n);
    const double *d_cov = c.in(cov, 225 * n);
    const double *d_dt  = c.in(delta_time, n);
    const double *d_env = c.in(env, 4 * n);
    const double *d_pts = c.in(points, 32 * n);
    const int32_t *d_po = variant == 1 ? c.in(pn_offsets, n + 1) : nullptr;
    const double *d_pn  = variant == 1 ? c.in(pn, 4 * (size_t) total_pn) : nullptr;
    if ((rc = c.seal())) return rc;
    double *d_r   = c.out(residuals, 15 * n);
    double *d_J   = jacobians ? c.out(jacobians, 480 * n) : nullptr;
    double *d_S   = c.out(sqrt_info, 225 * n); // (kept on the device only when the caller does not ask for it)
    int32_t *d_st = c.out(status, n);
    ICG_LAUNCH_GUARD(c);
    {
        icg_prof_scope ps(ctx, "preint_eval");
        hipLaunchKernelGGL(k_preint_sqrt_info, dim3(n_factors), dim3(64), 0, ctx->stream, n_factors, d_cov, d_S, d_st);
        hipLaunchKernelGGL(k_preint_evaluate, dim3(n_factors), dim3(64), 0, ctx->stream, variant, n_factors, d_del, d_jac, d_dt, d_env, d_po,
                           d_pn, d_pts, d_S, d_st, d_r, d_J);
    }
    ICG_HIP(ctx, hipGetLastError());
    return c.finish();
}

// ================================================ P2 on a resident set of factors ================================================
// What an integration result contributes to its factor is constant over a solve; only the evaluation point changes.  icg_preint_set keeps
// it on the device (one buffer, laid out as icg_preint_set in icg_internal.h says); an evaluation ships 32 + 4 doubles per factor up and one
// squared norm back, and leaves the whitened residuals and Jacobians where the set owns them.
namespace {
struct preint_view {
    const double *delta, *jac, *S, *dt, *env, *qnn, *pn;
    const int32_t *pn_off, *variant;
};
preint_view preint_set_view(const icg_preint_resident &s) {
    const size_t n = (size_t) s.n;
    preint_view v;
    const double *p = reinterpret_cast<const double *>(s.d_set);
    v.delta = p, p += 16 * n;
    v.jac = p, p += 225 * n;
    v.S = p, p += 225 * n;
    v.dt = p, p += n;
    v.env = p, p += 4 * n;
    v.qnn = p, p += 4 * n;
    v.pn = p, p += 4 * (size_t) s.total_pn;
    v.pn_off  = reinterpret_cast<const int32_t *>(p);
    v.variant = v.pn_off + (n + 1);
    return v;
}
} // namespace

extern "C" int icg_preint_set(icg_ctx *ctx, int n_factors, const int32_t *variant, const double *delta_state, const double *jac, const double *sqrt_info,
                              const double *delta_time, const double *env, const double *q_nn, const int32_t *pn_offsets, const double *pn) {
    if (!ctx) return ICG_ERR_INVALID;
    icg_preint_resident &s = ctx->preint;
    s.n               = 0; // whatever set the context held is gone, also when this call fails
    s.res_valid = s.jac_valid = false;
    if (n_factors <= 0) return icg_fail(ctx, ICG_ERR_INVALID, "icg_preint_set: n_factors = %d", n_factors);
    if (n_factors > ICG_PREINT_SET_MAX) // (before any array is read: the arrays of such a set are not looked at)
        return icg_fail(ctx, ICG_ERR_CAPACITY, "icg_preint_set: %d factors in one set (at most %d)", n_factors, ICG_PREINT_SET_MAX);
    if (!variant || !delta_state || !jac || !sqrt_info || !delta_time || !env || !q_nn) return icg_fail(ctx, ICG_ERR_INVALID, "icg_preint_set: NULL argument");
    const size_t n = (size_t) n_factors;
    bool any_earth = false;
    for (size_t f = 0; f < n; f++) {
        if (variant[f] != 0 && variant[f] != 1)
            return icg_fail(ctx, ICG_ERR_INVALID, "icg_preint_set: factor %zu: variant %d is neither 0 (Normal) nor 1 (Earth)", f, variant[f]);
        any_earth |= variant[f] == 1;
    }
    int64_t total_pn = 0;
    if (pn_offsets) {
        if (pn_offsets[0] < 0) return icg_fail(ctx, ICG_ERR_INVALID, "icg_preint_set: factor 0: pn_offsets[0] = %d", pn_offsets[0]);
        for (size_t f = 0; f < n; f++)
            if (pn_offsets[f + 1] < pn_offsets[f]) return icg_fail(ctx, ICG_ERR_INVALID, "icg_preint_set: factor %zu: pn_offsets not monotone", f);
        total_pn = pn_offsets[n];
        if (total_pn > 0 && !pn) return icg_fail(ctx, ICG_ERR_INVALID, "icg_preint_set: NULL pn for %lld rows", (long long) total_pn);
    } else if (any_earth) {
        return icg_fail(ctx, ICG_ERR_INVALID, "icg_preint_set: an Earth factor needs pn_offsets");
    }
    if (n_factors > ICG_PREINT_SET_MAX) // (again where the buffers are sized: the bound is what keeps `bytes` and the grids in range)
        return icg_fail(ctx, ICG_ERR_CAPACITY, "icg_preint_set: %d factors in one set (at most %d)", n_factors, ICG_PREINT_SET_MAX);
    const size_t n_dbl = (16 + 225 + 225 + 1 + 4 + 4) * n + 4 * (size_t) total_pn, bytes = 8 * n_dbl + 4 * (2 * n + 1);
    ICG_HIP(ctx, hipSetDevice(ctx->cfg.device));
    int rc;
    if ((rc = icg_grow(ctx, (void **) &s.d_set, &s.set_cap, bytes, bytes + bytes / 4))) return rc;
    icg_call c(ctx);
    if ((rc = c.reserve(bytes + 4 * 256))) return rc;
    const size_t off = icg_arena_alloc(ctx, bytes);
    if ((rc = c.overflowed())) return rc; // (nothing may be written through an allocation that did not fit)
    {
        double *p = icg_h<double>(ctx, off);
        memcpy(p, delta_state, 8 * 16 * n), p += 16 * n;
        memcpy(p, jac, 8 * 225 * n), p += 225 * n;
        memcpy(p, sqrt_info, 8 * 225 * n), p += 225 * n;
        memcpy(p, delta_time, 8 * n), p += n;
        memcpy(p, env, 8 * 4 * n), p += 4 * n;
        memcpy(p, q_nn, 8 * 4 * n), p += 4 * n;
        if (total_pn > 0) memcpy(p, pn, 8 * 4 * (size_t) total_pn), p += 4 * (size_t) total_pn;
        int32_t *q = reinterpret_cast<int32_t *>(p);
        if (pn_offsets)
            memcpy(q, pn_offsets, 4 * (n + 1));
        else
            memset(q, 0, 4 * (n + 1));
        memcpy(q + (n + 1), variant, 4 * n);
    }
    c.mirror_lo = std::min(c.mirror_lo, off), c.mirror_hi = std::max(c.mirror_hi, off + bytes);
    if ((rc = c.seal())) return rc;
    ICG_LAUNCH_GUARD(c);
    {
        icg_prof_scope ps(ctx, "preint_set");
        ICG_HIP(ctx, hipMemcpyAsync(s.d_set, icg_d<char>(ctx, off), bytes, hipMemcpyDeviceToDevice, ctx->stream));
    }
    if ((rc = c.finish())) return rc;
    s.total_pn = total_pn;
    s.n        = n_factors;
    return ICG_OK;
}

extern "C" int icg_preint_evaluate_resident(icg_ctx *ctx, const double *points, const double *q_corr, int want_jac, double *sq_norm) {
    if (!ctx) return ICG_ERR_INVALID;
    icg_preint_resident &s = ctx->preint;
    if (s.n <= 0) return icg_fail(ctx, ICG_ERR_INVALID, "icg_preint_evaluate_resident: no preintegration set is resident (icg_preint_set first)");
    if (!points || !q_corr || !sq_norm) return icg_fail(ctx, ICG_ERR_INVALID, "icg_preint_evaluate_resident: NULL argument");
    ICG_HIP(ctx, hipSetDevice(ctx->cfg.device));
    const size_t n = (size_t) s.n;
    bool replaced  = false;
    int rc         = icg_grow(ctx, (void **) &s.d_res, &s.res_cap, 8 * 15 * n, 8 * 15 * n, &replaced);
    if (replaced) s.res_valid = false;
    if (rc) return rc;
    if (want_jac) {
        replaced = false;
        rc       = icg_grow(ctx, (void **) &s.d_jac, &s.jac_cap, 8 * 480 * n, 8 * 480 * n, &replaced);
        if (replaced) s.jac_valid = false;
        if (rc) return rc;
    }
    icg_call c(ctx);
    if ((rc = c.reserve(8 * (32 + 4 + 1) * n + 4 * 256))) return rc;
    const double *d_pts = c.in(points, 32 * n);
    const double *d_qc  = c.in(q_corr, 4 * n);
    if ((rc = c.seal())) return rc;
    double *d_sq = c.out(sq_norm, n);
    ICG_LAUNCH_GUARD(c);
    s.res_valid = s.jac_valid = false; // (until the kernel below is through)
    const preint_view v = preint_set_view(s);
    {
        icg_prof_scope ps(ctx, "preint_eval_given");
        hipLaunchKernelGGL(k_preint_evaluate_given, dim3(s.n), dim3(64), 0, ctx->stream, s.n, v.variant, v.delta, v.jac, v.dt, v.env, v.pn_off, v.pn, d_pts, v.S,
                           d_qc, v.qnn, s.d_res, want_jac ? s.d_jac : (double *) nullptr, d_sq);
    }
    ICG_HIP(ctx, hipGetLastError());
    if ((rc = c.finish())) return rc;
    s.res_valid = true;
    s.jac_valid = want_jac != 0;
    return ICG_OK;
}

extern "C" int icg_preint_fetch_resident(icg_ctx *ctx, double *residuals, double *jacobians) {
    if (!ctx) return ICG_ERR_INVALID;
    const icg_preint_resident &s = ctx->preint;
    if (s.n <= 0) return icg_fail(ctx, ICG_ERR_INVALID, "icg_preint_fetch_resident: no preintegration set is resident (icg_preint_set first)");
    if (!residuals) return icg_fail(ctx, ICG_ERR_INVALID, "icg_preint_fetch_resident: NULL residuals");
    if (!s.res_valid) return icg_fail(ctx, ICG_ERR_INVALID, "icg_preint_fetch_resident: nothing was evaluated since the set was made resident");
    if (jacobians && !s.jac_valid)
        return icg_fail(ctx, ICG_ERR_INVALID, "icg_preint_fetch_resident: the last evaluation kept no Jacobians (want_jac = 0)");
    ICG_HIP(ctx, hipSetDevice(ctx->cfg.device));
    const size_t n = (size_t) s.n;
    std::vector<double> J32(jacobians ? 480 * n : 0);
    ICG_HIP(ctx, hipMemcpyAsync(residuals, s.d_res, 8 * 15 * n, hipMemcpyDeviceToHost, ctx->stream));
    if (jacobians) ICG_HIP(ctx, hipMemcpyAsync(J32.data(), s.d_jac, 8 * 480 * n, hipMemcpyDeviceToHost, ctx->stream));
    if (int rc = icg_stream_wait(ctx)) return rc;
    if (jacobians) { // 15 x 32 row-major -> 15x7 | 15x9 | 15x7 | 15x9
        static const int c0[5] = {0, 7, 16, 23, 32}, o0[4] = {0, 105, 240, 345};
        for (size_t f = 0; f < n; f++)
            for (int b = 0; b < 4; b++) {
                const int w = c0[b + 1] - c0[b];
                for (int i = 0; i < 15; i++) memcpy(jacobians + 480 * f + o0[b] + i * w, &J32[480 * f + 32 * i + c0[b]], 8 * (size_t) w);
            }
    }
    return ICG_OK;
}
