// Odometer preintegration (the reference's Odo and EarthOdo variants): P1 and P2 with the 19-wide error state dp, dv, dq, dbg, dba, ds, dsodo
// and the 16 noise channels gyro 3, accel 3, bg 3, ba 3, odo 3, sodo 1.  This file holds the P1 kernel of the family; its P2 kernels and
// its C entries are instantiations at N = 19 of the bodies it shares with the 15-state family (preint_shared.h).
//
// P1, k_preint_odo: one 64-lane wavefront per interval, strictly sequential over its samples; J and P (19 x 19) and the temporaries of the
// products stay in LDS for the whole interval (six 361-double matrices, 17.3 KB, + 19 x 8 values of phi, the three 3 x 3 blocks of G and the
// 16 noise variances: 18 944 B); every lane carries the (uniform) navigation state redundantly and owns <= 6 of the 361 entries of every
// product.  The per-sample blocks reach the lanes that index them by row THROUGH LDS (lane 0 lays them out with constant indices): indexed
// as register arrays they went to scratch memory (584 B per lane) and the kernel took 3.19 ms instead of 1.65 ms for 3 840 intervals x 41
// samples.  255 VGPRs, no scratch, two waves per SIMD.
// Reference: preintegration_base.cc:39-70,86-92 (two-sample integration, bias compensation); preintegration_odo.cc:206-272 (the distance
// increment s BEFORE integration(), with the old delta q; phi, G); preintegration_earth_odo.cc:230-346 (s with the mid-interval rotation cbbe
// and the old delta q; phi / G with cbb0 of the new one); noise :289-301.  cvb = euler2matrix(abv)^T arrives from the host: no sin / cos of
// the installation angles here.
// phi = I + F dt has at most 8 structural non-zeros per row (p: k = i, 3+ii; v: 3+ii, 6, 7, 8, 12, 13, 14; attitude: 6, 7, 8, 9+ii; bg, ba, sodo:
// k = i; s: 6, 7, 8, 9, 10, 11, 15+ii, 18) and G Q G^T has the blocks (v,v), (att,att), (att,s), (s,att), (s,s), (bg,bg), (ba,ba), (sodo,sodo):
// the s rows share the gyroscope channels with the attitude rows.  The products visit exactly the non-zero terms in ascending k, so every
// sum has the bits of the dense one (k_preint's rule; pinned by tests/test_gpu_preint_odo.py against a dense float64 restatement).
//   J = phi J ;  P = (phi P) phi^T + 0.5 dt (phi M + M phi^T),  M = G Q G^T
// Latency bound like k_preint (80 B in per sample): reported as intervals/s, not against the HBM roofline.
//
// P2 (bodies in preint_shared.h): k_preint_odo_sqrt_info (S = LLT(cov^-1).matrixL()^T, Gauss-Jordan with partial pivoting on the 19 x 38
// augmented matrix, mirrored lower triangle, column Cholesky: the arithmetic and order of the host's preintSqrtInformation<19>, S bit-identical) and
// k_preint_odo_evaluate (residual 19 + Jacobians 19x7 | 19x10 | 19x7 | 19x10, each output the dense 19-term sum over ascending k;
// preintegration_odo.cc:40-159, preintegration_earth_odo.cc:41-183, preintegration_factor.h:45-69).  One wavefront per factor.
//   k_preint_odo_evaluate_given  the same body for a set of factors RESIDENT on the device (icg_preint_odo_set):
//                                the two quaternions that need sin / cos / sqrt and the square-root information come from the host, the
//                                variant is the factor's own, the Jacobian is one 19 x 34 matrix and one lane adds r . r: the host's bits.
//                                221 VGPRs, no scratch, 8 376 B of LDS, two waves per SIMD.
#include "preint_shared.h"

using namespace icgd;
using namespace icg_preint;

#define PO_N 19
#define PO_NN 361
#define PO_IDX(i, j) ((i) * PO_N + (j))
#define PO_PV 8 // values of phi kept per row
// rows of phi in descending order of their number of structural non-zeros: s (8), v (7), attitude (4), p (2), bg, ba, sodo (1)
#define PO_ROWMAP(r) ((r) < 3 ? (r) + 15 : ((r) < 9 ? (r) : ((r) < 12 ? (r) - 9 : ((r) < 18 ? (r) - 3 : 18))))

// params_stride: doubles between the parameter rows of two intervals (icg_preint_odo_batch_params: 25), 0 = one row for the whole launch
// (icg_preint_odo_batch); wave-uniform like k_preint's, the row stays on the scalar path.
__global__ __launch_bounds__(64) void k_preint_odo(int variant, const int32_t *offsets, const double *imu, const double *state0,
                                                   const double *params_rows, int params_stride, double *cur_state, double *delta_state,
                                                   double *jac_out, double *cov_out, double *delta_time_out, double *pn_out) {
    __shared__ double J[PO_NN], P[PO_NN], M[PO_NN], T1[PO_NN], T2[PO_NN], T3[PO_NN], PV[PO_N * PO_PV];
    __shared__ double GM[27], NZ[16]; // the blocks gv, gs0, gs12 of G of the current sample; the diagonal of the noise matrix
    const int s = blockIdx.x, lane = threadIdx.x;
    const int begin = offsets[s], n = offsets[s + 1] - offsets[s];
    const double *params = params_rows + (size_t) s * (size_t) params_stride;
    const double gyr_arw = params[0], acc_vrw = params[1], gbstd = params[2], abstd = params[3], corr_time = params[4];
    const d3 gravity = mk3(0, 0, params[5]);
    const d3 iewn    = mk3(params[6], params[7], params[8]);
    m33 cvb;
#pragma unroll
    for (int i = 0; i < 9; i++) cvb.a[i] = params[13 + i];
    const d3 lodo        = mk3(params[22], params[23], params[24]);
    const m33 lodo_skew  = m_skew(lodo);
    const double *st0    = state0 + 17 * (size_t) s;
    d3 cur_p = mk3(st0[0], st0[1], st0[2]), cur_v = mk3(st0[7], st0[8], st0[9]);
    dq cur_q = dq{st0[3], st0[4], st0[5], st0[6]};
    const d3 bg = mk3(st0[10], st0[11], st0[12]), ba = mk3(st0[13], st0[14], st0[15]);
    const double sodo = st0[16], one_sodo = 1 + sodo;
    d3 del_p = mk3(0, 0, 0), del_v = mk3(0, 0, 0), del_s = mk3(0, 0, 0);
    dq del_q      = dq{0, 0, 0, 1};
    const dq q0   = cur_q;
    double delta_time = 0;
    if (lane == 0) { // the diagonal of Q (setNoiseMatrix)
#pragma unroll
        for (int i = 0; i < 3; i++) {
            NZ[i]      = gyr_arw * gyr_arw;
            NZ[3 + i]  = acc_vrw * acc_vrw;
            NZ[6 + i]  = 2 * gbstd * gbstd / corr_time;
            NZ[9 + i]  = 2 * abstd * abstd / corr_time;
            NZ[12 + i] = params[9 + i] * params[9 + i];
        }
        NZ[15] = params[12] * params[12];
    }
    for (int e = lane; e < PO_NN; e += 64) {
        J[e] = (e / PO_N == e % PO_N) ? 1.0 : 0.0;
        P[e] = 0.0;
    }
    __syncthreads();

    for (int index = 1; index < n; index++) {
        const double *pp = imu + 9 * (size_t) (begin + index - 1), *pc = imu + 9 * (size_t) (begin + index);
        d3 pre_dtheta = mk3(pp[2], pp[3], pp[4]), pre_dvel = mk3(pp[5], pp[6], pp[7]);
        d3 cur_dtheta = mk3(pc[2], pc[3], pc[4]), cur_dvel = mk3(pc[5], pc[6], pc[7]);
        const double pre_dt = pp[1], dt = pc[1], odovel = pc[8];
        pre_dtheta = sub(pre_dtheta, scl(pre_dt, bg));
        pre_dvel   = sub(pre_dvel, scl(pre_dt, ba));
        cur_dtheta = sub(cur_dtheta, scl(dt, bg));
        cur_dvel   = sub(cur_dvel, scl(dt, ba));
        // the distance increment in the body frame: cvb dsodo (1 + sodo) - R(dtheta) lodo + lodo, dtheta the bias-compensated increment
        // (not the coning-corrected one)
        const d3 cd  = m_vec(cvb, mk3(odovel, 0, 0));
        const d3 sv  = scl(one_sodo, cd);
        const d3 lev = add(sub(sv, m_vec(q_mat(rotvec2quat(cur_dtheta)), lodo)), lodo);
        d3 dvfb   = add(add(cur_dvel, scl(0.5, crs(cur_dtheta, cur_dvel))),
                        scl(1.0 / 12.0, add(crs(pre_dtheta, cur_dvel), crs(pre_dvel, cur_dtheta))));
        d3 dtheta = add(cur_dtheta, scl(1.0 / 12.0, crs(pre_dtheta, cur_dtheta)));
        m33 C;      // phi(3,6) = C skew(dvel), phi(3,12) = C dt, phi(15,6) = C skew(stheta), phi(15,9) = C skew(lodo) dt, phi(15,18) = -C cvb dsodo
        m33 gv;     // gt(3,3); gt(15,0) = gv skew(lodo), gt(15,12) = gv cvb (1 + sodo)
        double g60; // gt(6,0) diagonal sign
        if (variant == 2) {
            del_s = add(del_s, m_vec(q_mat(del_q), lev)); // (odo :213: before integration(), the old delta q)
            delta_time += dt;
            d3 dvel = add(m_vec(q_mat(cur_q), dvfb), scl(dt, gravity));
            cur_p   = add(add(cur_p, scl(dt, cur_v)), scl(0.5 * dt, dvel));
            cur_v   = add(cur_v, dvel);
            cur_q   = q_normalized(q_mul(cur_q, rotvec2quat(dtheta)));
            dvel    = m_vec(q_mat(del_q), dvfb);
            del_p   = add(add(del_p, scl(dt, del_v)), scl(0.5 * dt, dvel));
            del_v   = add(del_v, dvel);
            del_q   = q_normalized(q_mul(del_q, rotvec2quat(dtheta)));
            gv      = q_mat(del_q);
            C       = m_neg(gv);
            g60     = 1.0;
        } else {
            delta_time += dt;
            d3 dv_cor_g = scl(dt, sub(gravity, scl(2.0, crs(iewn, cur_v))));
            d3 dnn      = scl(dt, neg3(iewn));
            dq qnn      = rotvec2quat(dnn);
            m33 half    = m_scale(m_add(m_eye(), q_mat(qnn)), 0.5);
            d3 dvel     = add(m_vec(m_mul(half, q_mat(cur_q)), dvfb), dv_cor_g);
            cur_p       = add(add(cur_p, scl(dt, cur_v)), scl(0.5 * dt, dvel));
            cur_v       = add(cur_v, dvel);
            if (pn_out && lane == 0) { // pn_ (earth_odo :261): (dt, position) per sample, row begin+index-1
                double *pn = pn_out + 4 * (size_t) (begin + index - 1);
                pn[0] = dt, pn[1] = cur_p.x, pn[2] = cur_p.y, pn[3] = cur_p.z;
            }
            cur_q       = q_normalized(q_mul(q_mul(qnn, cur_q), rotvec2quat(dtheta)));
            dnn         = scl(-(delta_time - 0.5 * dt), iewn);
            const m33 cbbe = q_mat(q_mul(q_mul(q_mul(q_inv(q0), rotvec2quat(dnn)), q0), del_q)); // (:273: mid-interval, the old delta q)
            del_s       = add(del_s, m_vec(cbbe, lev));
            dvel        = m_vec(cbbe, dvfb);
            del_p       = add(add(del_p, scl(dt, del_v)), scl(0.5 * dt, dvel));
            del_v       = add(del_v, dvel);
            del_q       = q_normalized(q_mul(del_q, rotvec2quat(dtheta)));
            d3 dnn2     = scl(delta_time, neg3(iewn));
            C           = m_neg(q_mat(q_mul(q_mul(q_mul(q_inv(q0), rotvec2quat(dnn2)), q0), del_q)));
            gv          = C;
            g60         = -1.0;
        }
        const d3 stheta   = sub(sv, crs(cur_dtheta, lodo));
        const m33 blk36   = m_mul(C, m_skew(cur_dvel)), blk312 = m_scale(C, dt);
        const m33 blk156  = m_mul(C, m_skew(stheta)), blk159 = m_scale(m_mul(C, lodo_skew), dt);
        const d3 col1518  = m_vec(m_neg(C), cd);
        const m33 gs0     = m_mul(gv, lodo_skew), gs12 = m_scale(m_mul(gv, cvb), one_sodo);
        // ---- sparse rows of phi (<= 8 structural non-zeros, ascending k) and the three blocks of G, laid out in LDS by lane 0 with constant
        // indices (a lane-dependent index into a register array would put the array into scratch memory); G Q G^T then by everyone ----
        const m33 sk       = m_skew(cur_dtheta);
        const double decay = 1 - dt / corr_time;
        if (lane == 0) {
            // values only; the column of term t follows from the row's class (see PHI_TERM below)
            const double c1518[3] = {col1518.x, col1518.y, col1518.z};
#pragma unroll
            for (int ii = 0; ii < 3; ii++) {
                double *pp0 = &PV[ii * PO_PV], *pv1 = &PV[(3 + ii) * PO_PV], *pa = &PV[(6 + ii) * PO_PV], *ps = &PV[(15 + ii) * PO_PV];
                pp0[0] = 1.0, pp0[1] = dt;
                pv1[0] = 1.0;
#pragma unroll
                for (int kk = 0; kk < 3; kk++) {
                    pv1[1 + kk] = blk36.a[ii * 3 + kk], pv1[4 + kk] = blk312.a[ii * 3 + kk];
                    pa[kk]      = ((ii == kk) ? 1.0 : 0.0) - sk.a[ii * 3 + kk];
                    ps[kk] = blk156.a[ii * 3 + kk], ps[3 + kk] = blk159.a[ii * 3 + kk];
                }
                pa[3] = -dt;
                ps[6] = 1.0, ps[7] = c1518[ii];
                PV[(9 + ii) * PO_PV] = decay, PV[(12 + ii) * PO_PV] = decay;
            }
            PV[18 * PO_PV] = 1.0;
#pragma unroll
            for (int t = 0; t < 9; t++) GM[t] = gv.a[t], GM[9 + t] = gs0.a[t], GM[18 + t] = gs12.a[t];
        }
        __syncthreads();
        for (int e = lane; e < PO_NN; e += 64) {
            const int i = e / PO_N, j = e - i * PO_N;
            const int bi = i / 3, bj = j / 3, ii = i - bi * 3, jj = j - bj * 3;
            const double *gvm = GM, *gs0m = GM + 9, *gs12m = GM + 18;
            double m = 0;
            // m = sum_k gt[i][k] * noise[k] * gt[j][k] over the structural non-zeros of both rows, k ascending (gt: v rows = gv on the
            // accelerometer channels 3..5, attitude rows = +-1 on the gyroscope channels 0..2, bg / ba rows = 1 on 6..8 / 9..11, s rows = gs0 on
            // the gyroscope channels and gs12 on the odometer channels 12..14, the sodo row = 1 on channel 15)
            if (bi == 1 && bj == 1) {
#pragma unroll
                for (int k = 0; k < 3; k++) m += gvm[ii * 3 + k] * NZ[3 + k] * gvm[jj * 3 + k];
            } else if (bi == 2 && bj == 2) {
                if (ii == jj) m += g60 * NZ[ii] * g60;
            } else if (bi == 2 && bj == 5) {
                m += g60 * NZ[ii] * gs0m[jj * 3 + ii];
            } else if (bi == 5 && bj == 2) {
                m += gs0m[ii * 3 + jj] * NZ[jj] * g60;
            } else if (bi == 5 && bj == 5) {
#pragma unroll
                for (int k = 0; k < 3; k++) m += gs0m[ii * 3 + k] * NZ[k] * gs0m[jj * 3 + k];
#pragma unroll
                for (int k = 0; k < 3; k++) m += gs12m[ii * 3 + k] * NZ[12 + k] * gs12m[jj * 3 + k];
            } else if (bi == 3 && bj == 3) {
                if (ii == jj) m += 1.0 * NZ[6 + ii] * 1.0;
            } else if (bi == 4 && bj == 4) {
                if (ii == jj) m += 1.0 * NZ[9 + ii] * 1.0;
            } else if (bi == 6 && bj == 6) {
                m += 1.0 * NZ[15] * 1.0;
            }
            M[e] = m;
        }
        __syncthreads();
        // ---- pass 1, entries sorted by the class of their ROW: T1 = phi*J, T2 = phi*P, T3 = phi*M ----
        for (int e = lane; e < PO_NN; e += 64) {
            const int i = PO_ROWMAP(e / PO_N), j = e % PO_N;
            const int bi = i / 3, ii = i - bi * 3;
            const double *pv = &PV[i * PO_PV];
            double a = 0, b = 0, t1 = 0;
#define PHI_TERM(k, val)                                                                                                               \
    {                                                                                                                                  \
        const double phv = (val);                                                                                                      \
        a += phv * J[PO_IDX(k, j)];                                                                                                    \
        b += phv * P[PO_IDX(k, j)];                                                                                                    \
        t1 += phv * M[PO_IDX(k, j)];                                                                                                   \
    }
            if (bi == 5) {
                PHI_TERM(6, pv[0]) PHI_TERM(7, pv[1]) PHI_TERM(8, pv[2]) PHI_TERM(9, pv[3]) PHI_TERM(10, pv[4]) PHI_TERM(11, pv[5])
                PHI_TERM(15 + ii, pv[6]) PHI_TERM(18, pv[7])
            } else if (bi == 1) {
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
            T1[PO_IDX(i, j)] = a;
            T2[PO_IDX(i, j)] = b;
            T3[PO_IDX(i, j)] = t1;
        }
        __syncthreads();
        // ---- pass 2, entries sorted by the class of their COLUMN: J = T1 ; P = T2*phi^T + 0.5 dt (phi*M + M*phi^T) ----
        for (int e = lane; e < PO_NN; e += 64) {
            const int j = PO_ROWMAP(e / PO_N), i = e % PO_N;
            const int bj = j / 3, jj = j - bj * 3;
            const double *pv = &PV[j * PO_PV];
            double pc2 = 0, t2 = 0;
#define PHIT_TERM(k, val)                                                                                                              \
    {                                                                                                                                  \
        const double phv = (val);                                                                                                      \
        pc2 += T2[PO_IDX(i, k)] * phv;                                                                                                 \
        t2 += M[PO_IDX(i, k)] * phv;                                                                                                   \
    }
            if (bj == 5) {
                PHIT_TERM(6, pv[0]) PHIT_TERM(7, pv[1]) PHIT_TERM(8, pv[2]) PHIT_TERM(9, pv[3]) PHIT_TERM(10, pv[4]) PHIT_TERM(11, pv[5])
                PHIT_TERM(15 + jj, pv[6]) PHIT_TERM(18, pv[7])
            } else if (bj == 1) {
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
            J[PO_IDX(i, j)] = T1[PO_IDX(i, j)];
            P[PO_IDX(i, j)] = pc2 + 0.5 * dt * (T3[PO_IDX(i, j)] + t2);
        }
        __syncthreads();
    }
    for (int e = lane; e < PO_NN; e += 64) {
        jac_out[PO_NN * (size_t) s + e] = J[e];
        cov_out[PO_NN * (size_t) s + e] = P[e];
    }
    if (lane == 0) {
        double *c = cur_state + 16 * (size_t) s, *d = delta_state + 20 * (size_t) s;
        c[0] = cur_p.x, c[1] = cur_p.y, c[2] = cur_p.z, c[3] = cur_q.x, c[4] = cur_q.y, c[5] = cur_q.z, c[6] = cur_q.w;
        c[7] = cur_v.x, c[8] = cur_v.y, c[9] = cur_v.z;
        d[0] = del_p.x, d[1] = del_p.y, d[2] = del_p.z, d[3] = del_q.x, d[4] = del_q.y, d[5] = del_q.z, d[6] = del_q.w;
        d[7] = del_v.x, d[8] = del_v.y, d[9] = del_v.z;
        c[10] = d[10] = bg.x, c[11] = d[11] = bg.y, c[12] = d[12] = bg.z;
        c[13] = d[13] = ba.x, c[14] = d[14] = ba.y, c[15] = d[15] = ba.z;
        d[16] = del_s.x, d[17] = del_s.y, d[18] = del_s.z, d[19] = sodo;
        delta_time_out[s] = delta_time;
    }
}

// ================================================================ P2 ================================================================
// The bodies are preint_shared.h's, instantiated for the 19-wide state.
__global__ __launch_bounds__(64) void k_preint_odo_sqrt_info(int n, const double *cov, double *sqrt_info, int32_t *status) {
    sqrt_info_body<19>(n, cov, sqrt_info, status);
}

__global__ __launch_bounds__(64) void k_preint_odo_evaluate(int variant, int n, const double *delta_state, const double *jac,
                                                            const double *delta_time, const double *env, const int32_t *pn_offsets,
                                                            const double *pn, const double *points, const double *sqrt_info,
                                                            const int32_t *status, double *residuals, double *jacobians) {
    evaluate_body<19, false>(variant, n, delta_state, jac, delta_time, env, pn_offsets, pn, points, sqrt_info, status, nullptr, nullptr, residuals,
                             jacobians, nullptr);
}

// the resident set's instantiation: the variant is the factor's own
__global__ __launch_bounds__(64) void k_preint_odo_evaluate_given(int n, const int32_t *variant, const double *delta_state, const double *jac,
                                                                  const double *delta_time, const double *env, const int32_t *pn_offsets,
                                                                  const double *pn, const double *points, const double *sqrt_info,
                                                                  const double *q_corr, const double *q_nn, double *residuals,
                                                                  double *jacobians, double *sq_norm) {
    evaluate_body<19, true>(blockIdx.x < (unsigned) n ? variant[blockIdx.x] : 2, n, delta_state, jac, delta_time, env, pn_offsets, pn, points,
                            sqrt_info, nullptr, q_corr, q_nn, residuals, jacobians, sq_norm);
}

// ================================================================ the C entries ================================================================
static const kernels<19> K19 = {k_preint_odo, k_preint_odo_sqrt_info, k_preint_odo_evaluate, k_preint_odo_evaluate_given};

extern "C" int icg_preint_odo_batch(icg_ctx *ctx, int variant, int n_intervals, const int32_t *offsets, const double *imu9,
                                    const double *state0, const double *params25, double *cur_state, double *delta_state, double *jac,
                                    double *cov, double *delta_time, double *pn) {
    return batch_entry(K19, "batch", false, ctx, variant, n_intervals, offsets, imu9, state0, params25, cur_state, delta_state, jac, cov, delta_time,
                       pn, nullptr, nullptr);
}

extern "C" int icg_preint_odo_batch_params(icg_ctx *ctx, int variant, int n_intervals, const int32_t *offsets, const double *imu9,
                                           const double *state0, const double *params25, double *cur_state, double *delta_state,
                                           double *jac, double *cov, double *delta_time, double *pn, double *sqrt_info, int32_t *status) {
    return batch_entry(K19, "batch_params", true, ctx, variant, n_intervals, offsets, imu9, state0, params25, cur_state, delta_state, jac, cov,
                       delta_time, pn, sqrt_info, status);
}

extern "C" int icg_preint_odo_evaluate_batch(icg_ctx *ctx, int variant, int n_factors, const double *delta_state, const double *jac,
                                             const double *cov, const double *delta_time, const double *env, const int32_t *pn_offsets,
                                             const double *pn, const double *points, double *residuals, double *jacobians, double *sqrt_info,
                                             int32_t *status) {
    return evaluate_batch_entry(K19, ctx, variant, n_factors, delta_state, jac, cov, delta_time, env, pn_offsets, pn, points, residuals, jacobians,
                                sqrt_info, status);
}

extern "C" int icg_preint_odo_set(icg_ctx *ctx, int n_factors, const int32_t *variant, const double *delta_state, const double *jac,
                                  const double *sqrt_info, const double *delta_time, const double *env, const double *q_nn,
                                  const int32_t *pn_offsets, const double *pn) {
    return set_entry<19>(ctx, n_factors, variant, delta_state, jac, sqrt_info, delta_time, env, q_nn, pn_offsets, pn);
}

extern "C" int icg_preint_odo_evaluate_resident(icg_ctx *ctx, const double *points, const double *q_corr, int want_jac, double *sq_norm) {
    return evaluate_resident_entry(K19, ctx, points, q_corr, want_jac, sq_norm);
}

extern "C" int icg_preint_odo_fetch_resident(icg_ctx *ctx, double *residuals, double *jacobians) {
    return fetch_resident_entry<19>(ctx, residuals, jacobians);
}
