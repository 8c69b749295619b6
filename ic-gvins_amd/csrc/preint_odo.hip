// Odometer preintegration (the reference's Odo and EarthOdo variants): P1 and P2 with the 19-wide error state dp, dv, dq, dbg, dba, ds, dsodo
// and the 16 noise channels gyro 3, accel 3, bg 3, ba 3, odo 3, sodo 1.  The 19-state twins of k_preint / k_preint_sqrt_info /
// k_preint_evaluate (preint.hip), beside them: nothing there changes.
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
// P2: k_preint_odo_sqrt_info (S = LLT(cov^-1).matrixL()^T, Gauss-Jordan with partial pivoting on the 19 x 38 augmented matrix, mirrored
// lower triangle, column Cholesky: the arithmetic and order of the host's PreintegrationOdo::updateSqrtInformation, S bit-identical) and
// k_preint_odo_evaluate (residual 19 + Jacobians 19x7 | 19x10 | 19x7 | 19x10, each output the dense 19-term sum over ascending k;
// preintegration_odo.cc:40-159, preintegration_earth_odo.cc:41-183, preintegration_factor.h:45-69).  One wavefront per factor.
//   k_preint_odo_evaluate_given  the same body for a set of factors RESIDENT on the device (icg_preint_odo_set, last part of this file):
//                                the two quaternions that need sin / cos / sqrt and the square-root information come from the host, the
//                                variant is the factor's own, the Jacobian is one 19 x 34 matrix and one lane adds r . r: the host's bits.
//                                215 VGPRs, no scratch, 8 376 B of LDS, two waves per SIMD.
#include "dev_math.h"
#include "icg_internal.h"

using namespace icgd;

namespace {
__device__ __forceinline__ d3 neg3(d3 a) { return mk3(-a.x, -a.y, -a.z); }
// the host layer's P2 scales the axis by the reciprocal of the angle (dev_math.h's rotvec2quat, used by P1, divides)
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

extern "C" int icg_preint_odo_batch(icg_ctx *ctx, int variant, int n_intervals, const int32_t *offsets, const double *imu9,
                                    const double *state0, const double *params25, double *cur_state, double *delta_state, double *jac,
                                    double *cov, double *delta_time, double *pn) {
    if (!ctx || n_intervals < 0 || (variant != 2 && variant != 3)) return ICG_ERR_INVALID;
    if (n_intervals == 0) return ICG_OK;
    if (!offsets || !imu9 || !state0 || !params25 || !cur_state || !delta_state || !jac || !cov || !delta_time) return ICG_ERR_INVALID;
    const int total = offsets[n_intervals];
    if (offsets[0] < 0) return icg_fail(ctx, ICG_ERR_INVALID, "offsets[0] = %d", offsets[0]);
    for (int s = 0; s < n_intervals; s++)
        if (offsets[s + 1] - offsets[s] < 1) return icg_fail(ctx, ICG_ERR_INVALID, "interval %d has no IMU sample", s);
    ICG_HIP(ctx, hipSetDevice(ctx->cfg.device));
    icg_call c(ctx);
    int rc = c.reserve((size_t) total * (72 + 32) + (size_t) n_intervals * (8 * (17 + 16 + 20 + 1) + PO_NN * 8 * 2 + 4) + 16 * 256);
    if (rc) return rc;
    const int32_t *d_off = c.in(offsets, (size_t) n_intervals + 1);
    const double *d_imu  = c.in(imu9, 9 * (size_t) total);
    const double *d_s0   = c.in(state0, 17 * (size_t) n_intervals);
    const double *d_par  = c.in(params25, 25);
    if ((rc = c.seal())) return rc;
    double *d_cur = c.out_zc(cur_state, 16 * (size_t) n_intervals);
    double *d_del = c.out_zc(delta_state, 20 * (size_t) n_intervals);
    double *d_jac = c.out_zc(jac, PO_NN * (size_t) n_intervals);
    double *d_cov = c.out_zc(cov, PO_NN * (size_t) n_intervals);
    double *d_dt  = c.out_zc(delta_time, (size_t) n_intervals);
    // pn is written by the EarthOdo variant only, rows begin .. begin + n - 2 of every interval: the Odo variant gets no buffer, and the one
    // row per interval that the kernel leaves alone is staged from the caller's, so that the copy back returns it unchanged
    double *d_pn  = (pn && variant == 3) ? c.out_zc(pn, 4 * (size_t) total) : nullptr;
    ICG_LAUNCH_GUARD(c);
    if (d_pn)
        for (int s = 0; s < n_intervals; s++) {
            const size_t last = 4 * ((size_t) offsets[s + 1] - 1);
            memcpy(d_pn + last, pn + last, 4 * sizeof(double));
        }
    {
        icg_prof_scope ps(ctx, "preint_odo");
        hipLaunchKernelGGL(k_preint_odo, dim3(n_intervals), dim3(64), 0, ctx->stream, variant, d_off, d_imu, d_s0, d_par, 0, d_cur, d_del,
                           d_jac, d_cov, d_dt, d_pn);
    }
    ICG_HIP(ctx, hipGetLastError());
    return c.finish();
}

__global__ __launch_bounds__(64) void k_preint_odo_sqrt_info(int n, const double *cov, double *sqrt_info, int32_t *status);

// icg_preint_odo_batch with one parameter row per interval and (optionally) the square-root information of every result formed behind the
// integration: the 19-state twin of icg_preint_batch_params (preint.hip), the same staging.
extern "C" int icg_preint_odo_batch_params(icg_ctx *ctx, int variant, int n_intervals, const int32_t *offsets, const double *imu9,
                                           const double *state0, const double *params25, double *cur_state, double *delta_state,
                                           double *jac, double *cov, double *delta_time, double *pn, double *sqrt_info, int32_t *status) {
    if (!ctx) return ICG_ERR_INVALID;
    if (variant != 2 && variant != 3)
        return icg_fail(ctx, ICG_ERR_INVALID, "icg_preint_odo_batch_params: variant %d is neither 2 (Odo) nor 3 (EarthOdo)", variant);
    if (n_intervals < 0) return icg_fail(ctx, ICG_ERR_INVALID, "icg_preint_odo_batch_params: n_intervals = %d", n_intervals);
    if (n_intervals == 0) return ICG_OK;
    if (!offsets || !imu9 || !state0 || !params25 || !cur_state || !delta_state || !jac || !cov || !delta_time)
        return icg_fail(ctx, ICG_ERR_INVALID, "icg_preint_odo_batch_params: NULL argument");
    if (offsets[0] < 0) return icg_fail(ctx, ICG_ERR_INVALID, "icg_preint_odo_batch_params: interval 0: offsets[0] = %d", offsets[0]);
    for (int s = 0; s < n_intervals; s++)
        if (offsets[s + 1] - offsets[s] < 1) return icg_fail(ctx, ICG_ERR_INVALID, "icg_preint_odo_batch_params: interval %d has no IMU sample", s);
    const int total   = offsets[n_intervals];
    const size_t n    = (size_t) n_intervals;
    const bool want_S = sqrt_info || status;
    ICG_HIP(ctx, hipSetDevice(ctx->cfg.device));
    icg_call c(ctx);
    int rc = c.reserve((size_t) total * (72 + 32) + n * (8 * (17 + 25 + 16 + 20 + 1) + PO_NN * 8 * 3 + 8) + 16 * 256);
    if (rc) return rc;
    const int32_t *d_off = c.in(offsets, n + 1);
    const double *d_imu  = c.in(imu9, 9 * (size_t) total);
    const double *d_s0   = c.in(state0, 17 * n);
    const double *d_par  = c.in(params25, 25 * n);
    if ((rc = c.seal())) return rc;
    double *d_cur = c.out_zc(cur_state, 16 * n);
    double *d_del = c.out_zc(delta_state, 20 * n);
    double *d_jac = c.out_zc(jac, PO_NN * n);
    double *d_dt  = c.out_zc(delta_time, n);
    double *d_pn  = (pn && variant == 3) ? c.out_zc(pn, 4 * (size_t) total) : nullptr; // (icg_preint_odo_batch's rule)
    double *d_S   = want_S ? c.out_zc(sqrt_info, PO_NN * n) : nullptr;
    int32_t *d_st = want_S ? c.out_zc(status, n) : nullptr;
    double *d_cov = want_S ? c.out(cov, PO_NN * n) : c.out_zc(cov, PO_NN * n); // (last: no zero-copy region inside the span copied back)
    ICG_LAUNCH_GUARD(c);
    if (d_pn)
        for (int s = 0; s < n_intervals; s++) {
            const size_t last = 4 * ((size_t) offsets[s + 1] - 1);
            memcpy(d_pn + last, pn + last, 4 * sizeof(double));
        }
    {
        icg_prof_scope ps(ctx, "preint_odo");
        hipLaunchKernelGGL(k_preint_odo, dim3(n_intervals), dim3(64), 0, ctx->stream, variant, d_off, d_imu, d_s0, d_par, 25, d_cur, d_del,
                           d_jac, d_cov, d_dt, d_pn);
    }
    if (want_S) {
        icg_prof_scope ps(ctx, "preint_odo_eval");
        hipLaunchKernelGGL(k_preint_odo_sqrt_info, dim3(n_intervals), dim3(64), 0, ctx->stream, n_intervals, d_cov, d_S, d_st);
    }
    ICG_HIP(ctx, hipGetLastError());
    return c.finish();
}

// ================================================================ P2 ================================================================
#define POE_W 38        // row length of the augmented matrix
#define POE_U 35         // row length of the unwhitened block: 34 Jacobian columns (7 | 10 | 7 | 10) + the residual
#define POE_NOUT (19 + 646)

__global__ __launch_bounds__(64) void k_preint_odo_sqrt_info(int n, const double *cov, double *sqrt_info, int32_t *status) {
    __shared__ double w[PO_N * POE_W], L[PO_NN], fcol[PO_N];
    const int f = blockIdx.x, lane = threadIdx.x;
    if (f >= n) return;
    const double *C = cov + PO_NN * (size_t) f;
    double *S       = sqrt_info + PO_NN * (size_t) f;
    for (int e = lane; e < PO_N * POE_W; e += 64) {
        const int i = e / POE_W, j = e - i * POE_W;
        w[e]        = j < PO_N ? C[i * PO_N + j] : (i == j - PO_N ? 1.0 : 0.0);
    }
    for (int e = lane; e < PO_NN; e += 64) L[e] = 0.0;
    __syncthreads();
    for (int c = 0; c < PO_N; c++) {
        // first row r >= c of maximal |w[r][c]| (ties to the lower index): lanes c..18 hold a candidate, the others one that never wins
        const bool cand = lane >= c && lane < PO_N;
        double best     = cand ? fabs(w[lane * POE_W + c]) : -1.0;
        int piv         = cand ? lane : PO_N;
#pragma unroll
        for (int m = 16; m >= 1; m >>= 1) {
            const double ob = __shfl_xor(best, m);
            const int op    = __shfl_xor(piv, m);
            if (ob > best || (ob == best && op < piv)) best = ob, piv = op;
        }
        piv = __shfl(piv, 0);
        if (piv < c || piv > PO_N - 1) piv = c; // (a NaN column compares false everywhere: the host keeps row c)
        if (w[piv * POE_W + c] == 0.0) {        // uniform: singular covariance
            for (int e = lane; e < PO_NN; e += 64) S[e] = 0.0;
            if (lane == 0) status[f] = 1;
            return;
        }
        if (piv != c && lane < POE_W) {
            const double a = w[c * POE_W + lane], b = w[piv * POE_W + lane];
            w[c * POE_W + lane] = b, w[piv * POE_W + lane] = a;
        }
        __syncthreads();
        const double d = w[c * POE_W + c];
        __syncthreads();
        if (lane < POE_W) w[c * POE_W + lane] /= d;
        __syncthreads();
        if (lane < PO_N) fcol[lane] = w[lane * POE_W + c]; // (row c's own entry is not used)
        __syncthreads();
        for (int e = lane; e < PO_N * POE_W; e += 64) {
            const int r = e / POE_W, j = e - r * POE_W;
            const double fr = fcol[r];
            if (r != c && fr != 0.0) w[e] -= fr * w[c * POE_W + j];
        }
        __syncthreads();
    }
    // inverse = right half, lower triangle mirrored; column Cholesky, lane i owns row i: t = inv[i][j] - sum_k L[i][k] L[j][k], k ascending
    const int i = lane < PO_N ? lane : PO_N - 1;
    for (int j = 0; j < PO_N; j++) {
        double t = w[(i >= j ? i : j) * POE_W + PO_N + (i >= j ? j : i)];
        for (int k = 0; k < j; k++) t -= L[i * PO_N + k] * L[j * PO_N + k];
        const double ljj = sqrt(__shfl(t, j));
        if (lane < PO_N && lane >= j) L[lane * PO_N + j] = lane == j ? ljj : t / ljj;
        __syncthreads();
    }
    for (int e = lane; e < PO_NN; e += 64) S[e] = L[(e % PO_N) * PO_N + e / PO_N];
    if (lane == 0) status[f] = 0;
}

// The one evaluation body (preint.hip's precedent).  GIVEN = false: icg_preint_odo_evaluate_batch (status from k_preint_odo_sqrt_info,
// rotvec2quat on the device, Jacobians in the four blocks).  GIVEN = true: icg_preint_odo_evaluate_resident — the two quaternions that need
// sin / cos / sqrt arrive from the host (q_corr per evaluation point, q_nn with the set), so what is left is + - * / in the host's order;
// the Jacobian is one row-major 19 x 34 matrix per factor (the columns of U; 6 and 23 are sums of +-0 from +0.0, i.e. +0.0, like the host's
// seventh pose columns) and lane 0 adds sq_norm = sum_k r[k]^2, k ascending from +0.0.  status / sq_norm / q_corr / q_nn are not read by
// the instantiation that does not use them.
template <bool GIVEN>
__device__ __forceinline__ void preint_odo_evaluate_body(int variant, int n, const double *delta_state, const double *jac,
                                                         const double *delta_time, const double *env, const int32_t *pn_offsets,
                                                         const double *pn, const double *points, const double *sqrt_info,
                                                         const int32_t *status, const double *q_corr, const double *q_nn, double *residuals,
                                                         double *jacobians, double *sq_norm) {
    __shared__ double S[PO_NN], U[PO_N * POE_U];
    const int f = blockIdx.x, lane = threadIdx.x;
    if (f >= n) return;
    double *r_out = residuals + PO_N * (size_t) f;
    double *J_out = jacobians ? jacobians + 646 * (size_t) f : nullptr;
    if (!GIVEN && status[f] != 0) { // singular covariance: zero rows
        for (int o = lane; o < POE_NOUT; o += 64) {
            if (o < PO_N)
                r_out[o] = 0.0;
            else if (J_out)
                J_out[o - PO_N] = 0.0;
        }
        return;
    }
    for (int e = lane; e < PO_NN; e += 64) S[e] = sqrt_info[PO_NN * (size_t) f + e];
    for (int e = lane; e < PO_N * POE_U; e += 64) U[e] = 0.0;
    __syncthreads();

    const double *J19 = jac + PO_NN * (size_t) f, *pt = points + 34 * (size_t) f, *ds = delta_state + 20 * (size_t) f;
    const d3 d_p = mk3(ds[0], ds[1], ds[2]), d_v = mk3(ds[7], ds[8], ds[9]), d_bg = mk3(ds[10], ds[11], ds[12]), d_ba = mk3(ds[13], ds[14], ds[15]);
    const dq d_q = q_from_xyzw(ds + 3);
    const d3 d_s = mk3(ds[16], ds[17], ds[18]);
    const double d_sodo = ds[19];
    const d3 p0 = mk3(pt[0], pt[1], pt[2]), p1 = mk3(pt[17], pt[18], pt[19]);
    const dq q0 = q_from_xyzw(pt + 3), q1 = q_from_xyzw(pt + 20);
    const d3 v0 = mk3(pt[7], pt[8], pt[9]), bg0 = mk3(pt[10], pt[11], pt[12]), ba0 = mk3(pt[13], pt[14], pt[15]);
    const d3 v1 = mk3(pt[24], pt[25], pt[26]), bg1 = mk3(pt[27], pt[28], pt[29]), ba1 = mk3(pt[30], pt[31], pt[32]);
    const double sodo0 = pt[16], sodo1 = pt[33];
    const d3 gravity = mk3(0, 0, env[4 * (size_t) f]);
    const d3 iewn    = mk3(env[4 * (size_t) f + 1], env[4 * (size_t) f + 2], env[4 * (size_t) f + 3]);
    m33 dp_dbg, dp_dba, dv_dbg, dv_dba, dq_dbg, ds_dbg;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            dp_dbg.a[i * 3 + j] = J19[PO_IDX(i, 9 + j)];
            dp_dba.a[i * 3 + j] = J19[PO_IDX(i, 12 + j)];
            dv_dbg.a[i * 3 + j] = J19[PO_IDX(3 + i, 9 + j)];
            dv_dba.a[i * 3 + j] = J19[PO_IDX(3 + i, 12 + j)];
            dq_dbg.a[i * 3 + j] = J19[PO_IDX(6 + i, 9 + j)];
            ds_dbg.a[i * 3 + j] = J19[PO_IDX(15 + i, 9 + j)];
        }
    const d3 ds_dsodo = mk3(J19[PO_IDX(15, 18)], J19[PO_IDX(16, 18)], J19[PO_IDX(17, 18)]);
    const d3 dbg = sub(bg0, d_bg), dba = sub(ba0, d_ba);
    const double dsodo   = sodo0 - d_sodo;
    const d3 corrected_p = add(add(d_p, m_vec(dp_dba, dba)), m_vec(dp_dbg, dbg));
    const d3 corrected_v = add(add(d_v, m_vec(dv_dba, dba)), m_vec(dv_dbg, dbg));
    dq q_c;
    if (GIVEN)
        q_c = q_from_xyzw(q_corr + 4 * (size_t) f);
    else
        q_c = rotvec2quat_rcp(m_vec(dq_dbg, dbg));
    const dq corrected_q = q_mul(d_q, q_c);
    const d3 corrected_s = add(add(d_s, m_vec(ds_dbg, dbg)), scl(dsodo, ds_dsodo));
    const double T       = delta_time[f];
    const m33 cnb0       = q_mat(q_inv(q0));
    const d3 half_g_TT   = scl(T, scl(T, scl(0.5, gravity))); // ((0.5 g) T) T
    const d3 dp01        = sub(p1, p0);
    d3 rp, rv, rds;
    dq qe;
    // the blocks that differ between the variants: J0(0,0) J0(0,3) J0(3,0) J0(3,3) J0(6,3) | J2(3,0) J2(6,3) | J1(6,3)
    m33 j0_00, j0_03, j0_30, j0_33, j0_63, j2_30, j2_63, j1_63;
    if (variant == 2) {
        const d3 dpn = sub(sub(sub(p1, p0), scl(T, v0)), half_g_TT);
        const d3 dvn = sub(sub(v1, v0), scl(T, gravity));
        const d3 rdp = q_rot(q_inv(q0), dpn), rdv = q_rot(q_inv(q0), dvn);
        rds   = q_rot(q_inv(q0), dp01);
        rp = sub(rdp, corrected_p), rv = sub(rdv, corrected_v);
        qe    = q_mul(q_mul(q_inv(corrected_q), q_inv(q0)), q1);
        j0_00 = m_scale(cnb0, -1.0);
        j0_03 = m_skew(rdp);
        j0_33 = m_skew(rdv);
        j0_63 = m_scale(qleft_qright_br(q_mul(q_inv(q1), q0), corrected_q), -1.0);
        j2_63 = qleft_br(qe);
        j1_63 = m_mul(m_scale(qleft_br(q_mul(q_mul(q_inv(q1), q0), d_q)), -1.0), dq_dbg);
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
        rds   = m_vec(cnb0, dp01);
        rp = sub(rdp, corrected_p), rv = sub(rdv, corrected_v);
        qe    = q_mul(qb0b1, corrected_q);
        j0_00 = m_add(m_scale(cnb0, -1.0), m_scale(m_mul(m_scale(cnb0, 2.0), iewn_skew), -T));
        j0_03 = m_skew(rdp);
        j0_30 = m_mul(m_scale(cnb0, -2.0), iewn_skew);
        j0_33 = m_skew(rdv);
        j0_63 = qleft_qright_br(qb0b1, corrected_q);
        j2_30 = m_mul(m_scale(cnb0, 2.0), iewn_skew);
        j2_63 = m_scale(qright_br(qe), -1.0);
        j1_63 = m_mul(qleft_br(q_mul(qb0b1, d_q)), dq_dbg);
    }
    const d3 rbg = sub(bg1, bg0), rba = sub(ba1, ba0), rs = sub(rds, corrected_s);
    if (lane == 0) {
        // block (r0, c0) of the 19 x 34 Jacobian [J0 (cols 0..6) | J1 (7..16) | J2 (17..23) | J3 (24..33)]; column 34 = residual
#define POE_PUT(r0, c0, blk)                                                                                                           \
    {                                                                                                                                  \
        const m33 b_ = (blk);                                                                                                          \
        _Pragma("unroll") for (int i_ = 0; i_ < 3; i_++) _Pragma("unroll") for (int j_ = 0; j_ < 3; j_++)                               \
            U[((r0) + i_) * POE_U + (c0) + j_] = b_.a[i_ * 3 + j_];                                                                    \
    }
        const double rr[PO_N] = {rp.x, rp.y, rp.z, rv.x, rv.y, rv.z, 2 * qe.x, 2 * qe.y, 2 * qe.z, rbg.x, rbg.y, rbg.z, rba.x, rba.y, rba.z,
                                 rs.x, rs.y, rs.z, sodo1 - sodo0};
#pragma unroll
        for (int k = 0; k < PO_N; k++) U[k * POE_U + 34] = rr[k];
        if (jacobians) {
            POE_PUT(0, 0, j0_00)
            POE_PUT(0, 3, j0_03)
            POE_PUT(3, 3, j0_33)
            POE_PUT(6, 3, j0_63)
            POE_PUT(15, 0, m_scale(cnb0, -1.0))
            POE_PUT(15, 3, m_skew(rds))
            POE_PUT(0, 17, cnb0)
            POE_PUT(6, 17 + 3, j2_63)
            POE_PUT(15, 17, cnb0)
            if (variant != 2) {
                POE_PUT(3, 0, j0_30)
                POE_PUT(3, 17, j2_30)
            }
            POE_PUT(0, 7, m_scale(cnb0, -T))
            POE_PUT(0, 7 + 3, m_scale(dp_dbg, -1.0))
            POE_PUT(0, 7 + 6, m_scale(dp_dba, -1.0))
            POE_PUT(3, 7, m_scale(cnb0, -1.0))
            POE_PUT(3, 7 + 3, m_scale(dv_dbg, -1.0))
            POE_PUT(3, 7 + 6, m_scale(dv_dba, -1.0))
            POE_PUT(6, 7 + 3, j1_63)
            POE_PUT(9, 7 + 3, m_scale(m_eye(), -1.0))
            POE_PUT(12, 7 + 6, m_scale(m_eye(), -1.0))
            POE_PUT(15, 7 + 3, m_scale(ds_dbg, -1.0))
            U[15 * POE_U + 7 + 9] = ds_dsodo.x * -1.0, U[16 * POE_U + 7 + 9] = ds_dsodo.y * -1.0, U[17 * POE_U + 7 + 9] = ds_dsodo.z * -1.0;
            U[18 * POE_U + 7 + 9] = -1.0;
            POE_PUT(3, 24, cnb0)
            POE_PUT(9, 24 + 3, m_eye())
            POE_PUT(12, 24 + 6, m_eye())
            U[18 * POE_U + 24 + 9] = 1.0;
        }
#undef POE_PUT
    }
    __syncthreads();
    // whitening: out[i][col] = sum_k S[i][k] U[k][col], dense, k ascending from zero
    const int n_out = jacobians ? POE_NOUT : PO_N;
    double r_mine   = 0;
    for (int o = lane; o < n_out; o += 64) {
        int i, col;
        double *dst;
        if (o < PO_N) {
            i = o, col = 34, dst = r_out + o;
        } else {
            const int q = o - PO_N;
            dst         = J_out + q;
            if (GIVEN)
                i = q / 34, col = q - i * 34;
            else if (q < 133)
                i = q / 7, col = q - i * 7;
            else if (q < 323)
                i = (q - 133) / 10, col = 7 + (q - 133) - i * 10;
            else if (q < 456)
                i = (q - 323) / 7, col = 17 + (q - 323) - i * 7;
            else
                i = (q - 456) / 10, col = 24 + (q - 456) - i * 10;
        }
        double s = 0;
#pragma unroll
        for (int k = 0; k < PO_N; k++) s += S[i * PO_N + k] * U[k * POE_U + col];
        *dst = s;
        if (GIVEN && o < PO_N) r_mine = s; // (o == lane: the first pass of lanes 0 .. 18)
    }
    if (GIVEN) {
        __shared__ double R[PO_N];
        if (lane < PO_N) R[lane] = r_mine;
        __syncthreads();
        if (lane == 0) {
            double s = 0;
            for (int k = 0; k < PO_N; k++) s += R[k] * R[k];
            sq_norm[f] = s;
        }
    }
}

__global__ __launch_bounds__(64) void k_preint_odo_evaluate(int variant, int n, const double *delta_state, const double *jac,
                                                            const double *delta_time, const double *env, const int32_t *pn_offsets,
                                                            const double *pn, const double *points, const double *sqrt_info,
                                                            const int32_t *status, double *residuals, double *jacobians) {
    preint_odo_evaluate_body<false>(variant, n, delta_state, jac, delta_time, env, pn_offsets, pn, points, sqrt_info, status, nullptr, nullptr,
                                    residuals, jacobians, nullptr);
}

// the resident set's instantiation: the variant is the factor's own
__global__ __launch_bounds__(64) void k_preint_odo_evaluate_given(int n, const int32_t *variant, const double *delta_state, const double *jac,
                                                                  const double *delta_time, const double *env, const int32_t *pn_offsets,
                                                                  const double *pn, const double *points, const double *sqrt_info,
                                                                  const double *q_corr, const double *q_nn, double *residuals,
                                                                  double *jacobians, double *sq_norm) {
    preint_odo_evaluate_body<true>(blockIdx.x < (unsigned) n ? variant[blockIdx.x] : 2, n, delta_state, jac, delta_time, env, pn_offsets, pn,
                                   points, sqrt_info, nullptr, q_corr, q_nn, residuals, jacobians, sq_norm);
}

extern "C" int icg_preint_odo_evaluate_batch(icg_ctx *ctx, int variant, int n_factors, const double *delta_state, const double *jac,
                                             const double *cov, const double *delta_time, const double *env, const int32_t *pn_offsets,
                                             const double *pn, const double *points, double *residuals, double *jacobians, double *sqrt_info,
                                             int32_t *status) {
    if (!ctx) return ICG_ERR_INVALID;
    if (variant != 2 && variant != 3)
        return icg_fail(ctx, ICG_ERR_INVALID, "icg_preint_odo_evaluate_batch: variant %d is neither 2 (Odo) nor 3 (EarthOdo)", variant);
    if (n_factors <= 0) return icg_fail(ctx, ICG_ERR_INVALID, "icg_preint_odo_evaluate_batch: n_factors = %d", n_factors);
    if (!delta_state || !jac || !cov || !delta_time || !env || !points || !residuals || !status)
        return icg_fail(ctx, ICG_ERR_INVALID, "icg_preint_odo_evaluate_batch: NULL argument");
    int total_pn = 0;
    if (variant == 3) {
        if (!pn_offsets) return icg_fail(ctx, ICG_ERR_INVALID, "icg_preint_odo_evaluate_batch: the EarthOdo variant needs pn_offsets");
        if (pn_offsets[0] < 0) return icg_fail(ctx, ICG_ERR_INVALID, "icg_preint_odo_evaluate_batch: pn_offsets[0] = %d", pn_offsets[0]);
        for (int k = 0; k < n_factors; k++)
            if (pn_offsets[k + 1] < pn_offsets[k])
                return icg_fail(ctx, ICG_ERR_INVALID, "icg_preint_odo_evaluate_batch: pn_offsets not monotone at factor %d", k);
        total_pn = pn_offsets[n_factors];
        if (total_pn > 0 && !pn) return icg_fail(ctx, ICG_ERR_INVALID, "icg_preint_odo_evaluate_batch: NULL pn");
    }
    const size_t n = (size_t) n_factors;
    ICG_HIP(ctx, hipSetDevice(ctx->cfg.device));
    icg_call c(ctx);
    int rc = c.reserve(n * 8 * (20 + PO_NN + PO_NN + 1 + 4 + 34 + PO_N + 646 + PO_NN + 1) + (n + 1) * 4 + (size_t) total_pn * 32 + 16 * 256);
    if (rc) return rc;
    const double *d_del = c.in(delta_state, 20 * n);
    const double *d_jac = c.in(jac, PO_NN * n);
    const double *d_cov = c.in(cov, PO_NN * n);
    const double *d_dt  = c.in(delta_time, n);
    const double *d_env = c.in(env, 4 * n);
    const double *d_pts = c.in(points, 34 * n);
    const int32_t *d_po = variant == 3 ? c.in(pn_offsets, n + 1) : nullptr;
    const double *d_pn  = variant == 3 ? c.in(pn, 4 * (size_t) total_pn) : nullptr;
    if ((rc = c.seal())) return rc;
    double *d_r   = c.out(residuals, PO_N * n);
    double *d_J   = jacobians ? c.out(jacobians, 646 * n) : nullptr;
    double *d_S   = c.out(sqrt_info, PO_NN * n); // (kept on the device only when the caller does not ask for it)
    int32_t *d_st = c.out(status, n);
    ICG_LAUNCH_GUARD(c);
    {
        icg_prof_scope ps(ctx, "preint_odo_eval");
        hipLaunchKernelGGL(k_preint_odo_sqrt_info, dim3(n_factors), dim3(64), 0, ctx->stream, n_factors, d_cov, d_S, d_st);
        hipLaunchKernelGGL(k_preint_odo_evaluate, dim3(n_factors), dim3(64), 0, ctx->stream, variant, n_factors, d_del, d_jac, d_dt, d_env, d_po,
                           d_pn, d_pts, d_S, d_st, d_r, d_J);
    }
    ICG_HIP(ctx, hipGetLastError());
    return c.finish();
}

// ============================================ P2 on a resident set of odometer factors ============================================
// The 19-state twin of icg_preint_set / icg_preint_evaluate_resident / icg_preint_fetch_resident (preint.hip), with a resident struct of
// its own (ctx->preint_odo): both sets may be resident in one context at once.  An evaluation ships 34 + 4 doubles per factor up and one
// squared norm back, and leaves the whitened residuals (19) and the whitened 19 x 34 Jacobian where the set owns them.
namespace {
struct preint_odo_view {
    const double *delta, *jac, *S, *dt, *env, *qnn, *pn;
    const int32_t *pn_off, *variant;
};
preint_odo_view preint_odo_set_view(const icg_preint_odo_resident &s) {
    const size_t n = (size_t) s.n;
    preint_odo_view v;
    const double *p = reinterpret_cast<const double *>(s.d_set);
    v.delta = p, p += 20 * n;
    v.jac = p, p += PO_NN * n;
    v.S = p, p += PO_NN * n;
    v.dt = p, p += n;
    v.env = p, p += 4 * n;
    v.qnn = p, p += 4 * n;
    v.pn = p, p += 4 * (size_t) s.total_pn;
    v.pn_off  = reinterpret_cast<const int32_t *>(p);
    v.variant = v.pn_off + (n + 1);
    return v;
}
} // namespace

extern "C" int icg_preint_odo_set(icg_ctx *ctx, int n_factors, const int32_t *variant, const double *delta_state, const double *jac,
                                  const double *sqrt_info, const double *delta_time, const double *env, const double *q_nn,
                                  const int32_t *pn_offsets, const double *pn) {
    if (!ctx) return ICG_ERR_INVALID;
    icg_preint_odo_resident &s = ctx->preint_odo;
    s.n                        = 0; // whatever odometer set the context held is gone, also when this call fails
    s.res_valid = s.jac_valid = false;
    if (n_factors <= 0) return icg_fail(ctx, ICG_ERR_INVALID, "icg_preint_odo_set: n_factors = %d", n_factors);
    if (n_factors > ICG_PREINT_SET_MAX) // (before any array is read: the arrays of such a set are not looked at)
        return icg_fail(ctx, ICG_ERR_CAPACITY, "icg_preint_odo_set: %d factors in one set (at most %d)", n_factors, ICG_PREINT_SET_MAX);
    if (!variant || !delta_state || !jac || !sqrt_info || !delta_time || !env || !q_nn)
        return icg_fail(ctx, ICG_ERR_INVALID, "icg_preint_odo_set: NULL argument");
    const size_t n = (size_t) n_factors;
    bool any_earth = false;
    for (size_t f = 0; f < n; f++) {
        if (variant[f] != 2 && variant[f] != 3)
            return icg_fail(ctx, ICG_ERR_INVALID, "icg_preint_odo_set: factor %zu: variant %d is neither 2 (Odo) nor 3 (EarthOdo)", f, variant[f]);
        any_earth |= variant[f] == 3;
    }
    int64_t total_pn = 0;
    if (pn_offsets) {
        if (pn_offsets[0] < 0) return icg_fail(ctx, ICG_ERR_INVALID, "icg_preint_odo_set: factor 0: pn_offsets[0] = %d", pn_offsets[0]);
        for (size_t f = 0; f < n; f++)
            if (pn_offsets[f + 1] < pn_offsets[f]) return icg_fail(ctx, ICG_ERR_INVALID, "icg_preint_odo_set: factor %zu: pn_offsets not monotone", f);
        total_pn = pn_offsets[n];
        if (total_pn > 0 && !pn) return icg_fail(ctx, ICG_ERR_INVALID, "icg_preint_odo_set: NULL pn for %lld rows", (long long) total_pn);
    } else if (any_earth) {
        return icg_fail(ctx, ICG_ERR_INVALID, "icg_preint_odo_set: an EarthOdo factor needs pn_offsets");
    }
    const size_t n_dbl = (20 + PO_NN + PO_NN + 1 + 4 + 4) * n + 4 * (size_t) total_pn, bytes = 8 * n_dbl + 4 * (2 * n + 1);
    ICG_HIP(ctx, hipSetDevice(ctx->cfg.device));
    int rc;
    if ((rc = icg_grow(ctx, (void **) &s.d_set, &s.set_cap, bytes, bytes + bytes / 4))) return rc;
    icg_call c(ctx);
    if ((rc = c.reserve(bytes + 4 * 256))) return rc;
    const size_t off = icg_arena_alloc(ctx, bytes);
    if ((rc = c.overflowed())) return rc; // (nothing may be written through an allocation that did not fit)
    {
        double *p = icg_h<double>(ctx, off);
        memcpy(p, delta_state, 8 * 20 * n), p += 20 * n;
        memcpy(p, jac, 8 * PO_NN * n), p += PO_NN * n;
        memcpy(p, sqrt_info, 8 * PO_NN * n), p += PO_NN * n;
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
        icg_prof_scope ps(ctx, "preint_odo_set");
        ICG_HIP(ctx, hipMemcpyAsync(s.d_set, icg_d<char>(ctx, off), bytes, hipMemcpyDeviceToDevice, ctx->stream));
    }
    if ((rc = c.finish())) return rc;
    s.total_pn = total_pn;
    s.n        = n_factors;
    return ICG_OK;
}

extern "C" int icg_preint_odo_evaluate_resident(icg_ctx *ctx, const double *points, const double *q_corr, int want_jac, double *sq_norm) {
    if (!ctx) return ICG_ERR_INVALID;
    icg_preint_odo_resident &s = ctx->preint_odo;
    if (s.n <= 0)
        return icg_fail(ctx, ICG_ERR_INVALID, "icg_preint_odo_evaluate_resident: no odometer preintegration set is resident (icg_preint_odo_set first)");
    if (!points || !q_corr || !sq_norm) return icg_fail(ctx, ICG_ERR_INVALID, "icg_preint_odo_evaluate_resident: NULL argument");
    ICG_HIP(ctx, hipSetDevice(ctx->cfg.device));
    const size_t n = (size_t) s.n;
    bool replaced  = false;
    int rc         = icg_grow(ctx, (void **) &s.d_res, &s.res_cap, 8 * PO_N * n, 8 * PO_N * n, &replaced);
    if (replaced) s.res_valid = false;
    if (rc) return rc;
    if (want_jac) {
        replaced = false;
        rc       = icg_grow(ctx, (void **) &s.d_jac, &s.jac_cap, 8 * 646 * n, 8 * 646 * n, &replaced);
        if (replaced) s.jac_valid = false;
        if (rc) return rc;
    }
    icg_call c(ctx);
    if ((rc = c.reserve(8 * (34 + 4 + 1) * n + 4 * 256))) return rc;
    const double *d_pts = c.in(points, 34 * n);
    const double *d_qc  = c.in(q_corr, 4 * n);
    if ((rc = c.seal())) return rc;
    double *d_sq = c.out(sq_norm, n);
    ICG_LAUNCH_GUARD(c);
    s.res_valid = s.jac_valid = false; // (until the kernel below is through)
    const preint_odo_view v = preint_odo_set_view(s);
    {
        icg_prof_scope ps(ctx, "preint_odo_eval_given");
        hipLaunchKernelGGL(k_preint_odo_evaluate_given, dim3(s.n), dim3(64), 0, ctx->stream, s.n, v.variant, v.delta, v.jac, v.dt, v.env, v.pn_off, v.pn,
                           d_pts, v.S, d_qc, v.qnn, s.d_res, want_jac ? s.d_jac : (double *) nullptr, d_sq);
    }
    ICG_HIP(ctx, hipGetLastError());
    if ((rc = c.finish())) return rc;
    s.res_valid = true;
    s.jac_valid = want_jac != 0;
    return ICG_OK;
}

extern "C" int icg_preint_odo_fetch_resident(icg_ctx *ctx, double *residuals, double *jacobians) {
    if (!ctx) return ICG_ERR_INVALID;
    const icg_preint_odo_resident &s = ctx->preint_odo;
    if (s.n <= 0)
        return icg_fail(ctx, ICG_ERR_INVALID, "icg_preint_odo_fetch_resident: no odometer preintegration set is resident (icg_preint_odo_set first)");
    if (!residuals) return icg_fail(ctx, ICG_ERR_INVALID, "icg_preint_odo_fetch_resident: NULL residuals");
    if (!s.res_valid) return icg_fail(ctx, ICG_ERR_INVALID, "icg_preint_odo_fetch_resident: nothing was evaluated since the set was made resident");
    if (jacobians && !s.jac_valid)
        return icg_fail(ctx, ICG_ERR_INVALID, "icg_preint_odo_fetch_resident: the last evaluation kept no Jacobians (want_jac = 0)");
    ICG_HIP(ctx, hipSetDevice(ctx->cfg.device));
    const size_t n = (size_t) s.n;
    std::vector<double> J34(jacobians ? 646 * n : 0);
    ICG_HIP(ctx, hipMemcpyAsync(residuals, s.d_res, 8 * PO_N * n, hipMemcpyDeviceToHost, ctx->stream));
    if (jacobians) ICG_HIP(ctx, hipMemcpyAsync(J34.data(), s.d_jac, 8 * 646 * n, hipMemcpyDeviceToHost, ctx->stream));
    if (int rc = icg_stream_wait(ctx)) return rc;
    if (jacobians) { // 19 x 34 row-major -> 19x7 | 19x10 | 19x7 | 19x10
        static const int c0[5] = {0, 7, 17, 24, 34}, o0[4] = {0, 133, 323, 456};
        for (size_t f = 0; f < n; f++)
            for (int b = 0; b < 4; b++) {
                const int w = c0[b + 1] - c0[b];
                for (int i = 0; i < PO_N; i++) memcpy(jacobians + 646 * f + o0[b] + i * w, &J34[646 * f + 34 * i + c0[b]], 8 * (size_t) w);
            }
    }
    return ICG_OK;
}
