// What the two preintegration families share: the IMU-only one (Normal / Earth, 15-wide error state, preint.hip) and the odometer one
// (Odo / EarthOdo, 19-wide, preint_odo.hip).  One record per family states its widths, variant numbers and the words of its entries;
// everything below is written once against that record:
//   device   the quaternion helpers of P2, the square-root information body (template <int N>) and the evaluation body
//            (template <int N, bool GIVEN>, the 19-state extras under `if constexpr (N == 19)`)
//   host     the bodies of the C entries: P1 staging (*_batch, *_batch_params), *_evaluate_batch, and the resident set
//            (*_set, *_evaluate_resident, *_fetch_resident and the view of the set's buffer)
// The .hip files keep the P1 kernels (k_preint, k_preint_odo: structured differently on purpose), the thin __global__ instantiations of the
// bodies and the extern "C" entries, each an argument hand-over.  Every floating-point expression below has the operands and the order the
// host layer's evaluate() has: both files are built with -ffp-contract=off and the tests compare bits.
#pragma once
#include <algorithm>
#include <vector>

#include "dev_math.h"
#include "icg_internal.h"

namespace icg_preint {
using namespace icgd;

// ---------------------------------------------------------------- the family record ----------------------------------------------------------------
template <int N_> struct family;
template <> struct family<15> {
    static constexpr int N = 15, STATE0 = 16, CUR = 16, DELTA = 16, IMU = 8, PARAMS = 9, POINT = 32, MIX = 9, VARIANT0 = 0;
    static constexpr const char *plain = "Normal", *earth = "Earth";
    static constexpr const char *stem = "icg_preint", *what = "preintegration";
    static constexpr const char *scope_p1 = "preint", *scope_eval = "preint_eval", *scope_set = "preint_set", *scope_given = "preint_eval_given";
    static icg_preint_resident &set_of(icg_ctx *ctx) { return ctx->preint; }
};
template <> struct family<19> {
    static constexpr int N = 19, STATE0 = 17, CUR = 16, DELTA = 20, IMU = 9, PARAMS = 25, POINT = 34, MIX = 10, VARIANT0 = 2;
    static constexpr const char *plain = "Odo", *earth = "EarthOdo";
    static constexpr const char *stem = "icg_preint_odo", *what = "odometer preintegration";
    static constexpr const char *scope_p1 = "preint_odo", *scope_eval = "preint_odo_eval", *scope_set = "preint_odo_set",
                                *scope_given = "preint_odo_eval_given";
    static icg_preint_resident &set_of(icg_ctx *ctx) { return ctx->preint_odo; }
};
// derived: N x N matrices, the whitened Jacobian N x POINT (row-major in a resident set; as the four blocks N x 7 | MIX | 7 | MIX for a
// caller), first column / first element of every block
template <int N> struct widths {
    typedef family<N> F;
    static constexpr int NN = N * N, NJ = N * F::POINT;
    static constexpr int col0[5] = {0, 7, 7 + F::MIX, 14 + F::MIX, F::POINT};
    static constexpr int off0[5] = {0, N * 7, N * (7 + F::MIX), N * (14 + F::MIX), NJ};
};

// ---------------------------------------------------------------- device helpers ----------------------------------------------------------------
__device__ __forceinline__ d3 neg3(d3 a) { return mk3(-a.x, -a.y, -a.z); }
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

// ---------------------------------------------------------------- square-root information ----------------------------------------------------------------
// S = LLT(cov^-1).matrixL()^T with the arithmetic and the order of the host layer's updateSqrtInformation: Gauss-Jordan with partial pivoting
// on the N x 2N augmented matrix in LDS (the entries of one elimination step are independent: lanes own entries; the pivot search is a
// butterfly over the power of two that covers N), mirrored lower triangle, column Cholesky (lane i owns row i).  Only + - * / sqrt, all
// correctly rounded on both sides: S is bit-identical to the host's.  One 64-lane workgroup per matrix.
template <int N> __device__ __forceinline__ void sqrt_info_body(int n, const double *cov, double *sqrt_info, int32_t *status) {
    constexpr int NN = N * N, W = 2 * N; // W: row length of the augmented matrix
    constexpr int COVER = N <= 16 ? 16 : 32;
    static_assert(N <= COVER && W <= 64, "one wavefront: a lane per row of the pivot search and per entry of a row");
    __shared__ double w[N * W], L[NN], fcol[N];
    const int f = blockIdx.x, lane = threadIdx.x;
    if (f >= n) return;
    const double *C = cov + NN * (size_t) f;
    double *S       = sqrt_info + NN * (size_t) f;
    for (int e = lane; e < N * W; e += 64) {
        const int i = e / W, j = e - i * W;
        w[e]        = j < N ? C[i * N + j] : (i == j - N ? 1.0 : 0.0);
    }
    for (int e = lane; e < NN; e += 64) L[e] = 0.0;
    __syncthreads();
    for (int c = 0; c < N; c++) {
        // first row r >= c of maximal |w[r][c]| (ties to the lower index): lanes c..N-1 hold a candidate, the others one that never wins
        const bool cand = lane >= c && lane < N;
        double best     = cand ? fabs(w[lane * W + c]) : -1.0;
        int piv         = cand ? lane : N;
#pragma unroll
        for (int m = COVER / 2; m >= 1; m >>= 1) {
            const double ob = __shfl_xor(best, m);
            const int op    = __shfl_xor(piv, m);
            if (ob > best || (ob == best && op < piv)) best = ob, piv = op;
        }
        piv = __shfl(piv, 0);
        if (piv < c || piv > N - 1) piv = c; // (a NaN column compares false everywhere: the host keeps row c)
        if (w[piv * W + c] == 0.0) {         // uniform: singular covariance
            for (int e = lane; e < NN; e += 64) S[e] = 0.0;
            if (lane == 0) status[f] = 1;
            return;
        }
        if (piv != c && lane < W) {
            const double a = w[c * W + lane], b = w[piv * W + lane];
            w[c * W + lane] = b, w[piv * W + lane] = a;
        }
        __syncthreads();
        const double d = w[c * W + c];
        __syncthreads();
        if (lane < W) w[c * W + lane] /= d;
        // no barrier between the division and reading the column: the workgroup is one wavefront, the only entry of column c the division
        // touches is row c's, written by lane c and read back by lane c alone, and a lane reads what it wrote before in program order
        if (lane < N) fcol[lane] = w[lane * W + c]; // (row c's own entry is not used)
        __syncthreads();
        for (int e = lane; e < N * W; e += 64) {
            const int r = e / W, j = e - r * W;
            const double fr = fcol[r];
            if (r != c && fr != 0.0) w[e] -= fr * w[c * W + j];
        }
        __syncthreads();
    }
    // inverse = right half, lower triangle mirrored; column Cholesky, lane i owns row i: t = inv[i][j] - sum_k L[i][k] L[j][k], k ascending
    const int i = lane < N ? lane : N - 1;
    for (int j = 0; j < N; j++) {
        double t = w[(i >= j ? i : j) * W + N + (i >= j ? j : i)];
        for (int k = 0; k < j; k++) t -= L[i * N + k] * L[j * N + k];
        const double ljj = sqrt(__shfl(t, j));
        if (lane < N && lane >= j) L[lane * N + j] = lane == j ? ljj : t / ljj;
        __syncthreads();
    }
    for (int e = lane; e < NN; e += 64) S[e] = L[(e % N) * N + e / N];
    if (lane == 0) status[f] = 0;
}

// ---------------------------------------------------------------- evaluation ----------------------------------------------------------------
// The one evaluation body: residual N + Jacobians N x 7 | MIX | 7 | MIX (preintegration_normal.cc:38-142, preintegration_earth.cc:37-164,
// preintegration_odo.cc:40-159, preintegration_earth_odo.cc:41-183, preintegration_factor.h:45-69).  Every lane carries the (uniform) geometry
// redundantly, lane 0 lays the unwhitened N x POINT Jacobian and the residual out in LDS, then the lanes share the N + N * POINT outputs and
// form each as the dense N-term sum over k ascending from zero, as the host's evaluate() does.
// GIVEN = false: *_evaluate_batch (status from the square-root kernel, rotvec2quat on the device — sin / cos are the only primitives that may
// round differently from the host —, Jacobians in the four blocks).  GIVEN = true: *_evaluate_resident — the two quaternions that need
// sin / cos / sqrt arrive from the host (q_corr per evaluation point, q_nn with the set), so what is left is + - * / in the host's order; the
// Jacobian is one row-major N x POINT matrix per factor (the columns of U; the seventh column of either pose is a sum of +-0 from +0.0, i.e.
// +0.0, like the host's) and lane 0 adds sq_norm = sum_k r[k]^2, k ascending from +0.0.  status / sq_norm / q_corr / q_nn are not read by the
// instantiation that does not use them.
template <int N, bool GIVEN>
__device__ __forceinline__ void evaluate_body(int variant, int n, const double *delta_state, const double *jac, const double *delta_time,
                                              const double *env, const int32_t *pn_offsets, const double *pn, const double *points,
                                              const double *sqrt_info, const int32_t *status, const double *q_corr, const double *q_nn,
                                              double *residuals, double *jacobians, double *sq_norm) {
    typedef family<N> F;
    constexpr int NN = N * N, P = F::POINT, NJ = N * P, UW = P + 1; // UW: row length of the unwhitened block, column P = the residual
    constexpr int C1 = 7, C2 = 7 + F::MIX, C3 = 14 + F::MIX;          // first columns of J1, J2, J3
    constexpr int P1 = F::POINT / 2;                                  // the second state of an evaluation point
    __shared__ double S[NN], U[N * UW];
    const int f = blockIdx.x, lane = threadIdx.x;
    if (f >= n) return;
    double *r_out = residuals + N * (size_t) f;
    double *J_out = jacobians ? jacobians + NJ * (size_t) f : nullptr;
    if (!GIVEN && status[f] != 0) { // singular covariance: zero rows
        for (int o = lane; o < N + NJ; o += 64) {
            if (o < N)
                r_out[o] = 0.0;
            else if (J_out)
                J_out[o - N] = 0.0;
        }
        return;
    }
    for (int e = lane; e < NN; e += 64) S[e] = sqrt_info[NN * (size_t) f + e];
    for (int e = lane; e < N * UW; e += 64) U[e] = 0.0;
    __syncthreads();

    const double *JN = jac + NN * (size_t) f, *pt = points + P * (size_t) f, *ds = delta_state + F::DELTA * (size_t) f;
    const d3 d_p = mk3(ds[0], ds[1], ds[2]), d_v = mk3(ds[7], ds[8], ds[9]), d_bg = mk3(ds[10], ds[11], ds[12]), d_ba = mk3(ds[13], ds[14], ds[15]);
    const dq d_q = q_from_xyzw(ds + 3);
    const d3 p0 = mk3(pt[0], pt[1], pt[2]), p1 = mk3(pt[P1], pt[P1 + 1], pt[P1 + 2]);
    const dq q0 = q_from_xyzw(pt + 3), q1 = q_from_xyzw(pt + P1 + 3);
    const d3 v0 = mk3(pt[7], pt[8], pt[9]), bg0 = mk3(pt[10], pt[11], pt[12]), ba0 = mk3(pt[13], pt[14], pt[15]);
    const d3 v1 = mk3(pt[P1 + 7], pt[P1 + 8], pt[P1 + 9]), bg1 = mk3(pt[P1 + 10], pt[P1 + 11], pt[P1 + 12]),
             ba1 = mk3(pt[P1 + 13], pt[P1 + 14], pt[P1 + 15]);
    const d3 gravity = mk3(0, 0, env[4 * (size_t) f]);
    const d3 iewn    = mk3(env[4 * (size_t) f + 1], env[4 * (size_t) f + 2], env[4 * (size_t) f + 3]);
    m33 dp_dbg, dp_dba, dv_dbg, dv_dba, dq_dbg;
#pragma unroll
    for (int i = 0; i < 3; i++)
#pragma unroll
        for (int j = 0; j < 3; j++) {
            dp_dbg.a[i * 3 + j] = JN[i * N + 9 + j];
            dp_dba.a[i * 3 + j] = JN[i * N + 12 + j];
            dv_dbg.a[i * 3 + j] = JN[(3 + i) * N + 9 + j];
            dv_dba.a[i * 3 + j] = JN[(3 + i) * N + 12 + j];
            dq_dbg.a[i * 3 + j] = JN[(6 + i) * N + 9 + j];
        }
    const d3 dbg = sub(bg0, d_bg), dba = sub(ba0, d_ba);
    const d3 corrected_p = add(add(d_p, m_vec(dp_dba, dba)), m_vec(dp_dbg, dbg));
    const d3 corrected_v = add(add(d_v, m_vec(dv_dba, dba)), m_vec(dv_dbg, dbg));
    dq q_c;
    if (GIVEN)
        q_c = q_from_xyzw(q_corr + 4 * (size_t) f);
    else
        q_c = rotvec2quat_rcp(m_vec(dq_dbg, dbg));
    const dq corrected_q = q_mul(d_q, q_c);
    // the odometer family's extras: the distance increment s (rows 15..17) and the scale factor sodo (row 18)
    m33 ds_dbg;
    d3 ds_dsodo, corrected_s, rds;
    double sodo0 = 0, sodo1 = 0;
    if constexpr (N == 19) {
        const d3 d_s        = mk3(ds[16], ds[17], ds[18]);
        const double d_sodo = ds[19];
        sodo0 = pt[16], sodo1 = pt[P1 + 16];
#pragma unroll
        for (int i = 0; i < 3; i++)
#pragma unroll
            for (int j = 0; j < 3; j++) ds_dbg.a[i * 3 + j] = JN[(15 + i) * N + 9 + j];
        ds_dsodo           = mk3(JN[15 * N + 18], JN[16 * N + 18], JN[17 * N + 18]);
        const double dsodo = sodo0 - d_sodo;
        corrected_s        = add(add(d_s, m_vec(ds_dbg, dbg)), scl(dsodo, ds_dsodo));
    }
    const double T     = delta_time[f];
    const m33 cnb0     = q_mat(q_inv(q0));
    const d3 half_g_TT = scl(T, scl(T, scl(0.5, gravity))); // ((0.5 g) T) T
    const d3 dp01      = sub(p1, p0);
    d3 rp, rv;
    dq qe;
    // the blocks that differ between the variants: J0(0,0) J0(0,3) J0(3,0) J0(3,3) J0(6,3) | J2(3,0) J2(6,3) | J1(6,3)
    m33 j0_00, j0_03, j0_30, j0_33, j0_63, j2_30, j2_63, j1_63;
    if (variant == F::VARIANT0) {
        const d3 dpn = sub(sub(sub(p1, p0), scl(T, v0)), half_g_TT);
        const d3 dvn = sub(sub(v1, v0), scl(T, gravity));
        const d3 rdp = q_rot(q_inv(q0), dpn), rdv = q_rot(q_inv(q0), dvn);
        if constexpr (N == 19) rds = q_rot(q_inv(q0), dp01);
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
        if constexpr (N == 19) rds = m_vec(cnb0, dp01);
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
    const d3 rbg = sub(bg1, bg0), rba = sub(ba1, ba0);
    if (lane == 0) {
        // block (r0, c0) of the N x POINT Jacobian [J0 (cols 0..6) | J1 (7..) | J2 (C2..) | J3 (C3..)]; column POINT = residual
#define PE_PUT(r0, c0, blk)                                                                                                            \
    {                                                                                                                                  \
        const m33 b_ = (blk);                                                                                                          \
        _Pragma("unroll") for (int i_ = 0; i_ < 3; i_++) _Pragma("unroll") for (int j_ = 0; j_ < 3; j_++)                               \
            U[((r0) + i_) * UW + (c0) + j_] = b_.a[i_ * 3 + j_];                                                                       \
    }
        double rr[N] = {rp.x, rp.y, rp.z, rv.x, rv.y, rv.z, 2 * qe.x, 2 * qe.y, 2 * qe.z, rbg.x, rbg.y, rbg.z, rba.x, rba.y, rba.z};
        if constexpr (N == 19) {
            const d3 rs = sub(rds, corrected_s);
            rr[15] = rs.x, rr[16] = rs.y, rr[17] = rs.z, rr[18] = sodo1 - sodo0;
        }
#pragma unroll
        for (int k = 0; k < N; k++) U[k * UW + P] = rr[k];
        if (jacobians) {
            PE_PUT(0, 0, j0_00)
            PE_PUT(0, 3, j0_03)
            PE_PUT(3, 3, j0_33)
            PE_PUT(6, 3, j0_63)
            if constexpr (N == 19) {
                PE_PUT(15, 0, m_scale(cnb0, -1.0))
                PE_PUT(15, 3, m_skew(rds))
            }
            PE_PUT(0, C2, cnb0)
            PE_PUT(6, C2 + 3, j2_63)
            if constexpr (N == 19) PE_PUT(15, C2, cnb0)
            if (variant != F::VARIANT0) {
                PE_PUT(3, 0, j0_30)
                PE_PUT(3, C2, j2_30)
            }
            PE_PUT(0, C1, m_scale(cnb0, -T))
            PE_PUT(0, C1 + 3, m_scale(dp_dbg, -1.0))
            PE_PUT(0, C1 + 6, m_scale(dp_dba, -1.0))
            PE_PUT(3, C1, m_scale(cnb0, -1.0))
            PE_PUT(3, C1 + 3, m_scale(dv_dbg, -1.0))
            PE_PUT(3, C1 + 6, m_scale(dv_dba, -1.0))
            PE_PUT(6, C1 + 3, j1_63)
            PE_PUT(9, C1 + 3, m_scale(m_eye(), -1.0))
            PE_PUT(12, C1 + 6, m_scale(m_eye(), -1.0))
            if constexpr (N == 19) { // the s rows against bg and sodo, the sodo row against sodo: the two scalar columns C1 + 9 and C3 + 9
                PE_PUT(15, C1 + 3, m_scale(ds_dbg, -1.0))
                U[15 * UW + C1 + 9] = ds_dsodo.x * -1.0, U[16 * UW + C1 + 9] = ds_dsodo.y * -1.0, U[17 * UW + C1 + 9] = ds_dsodo.z * -1.0;
                U[18 * UW + C1 + 9] = -1.0;
            }
            PE_PUT(3, C3, cnb0)
            PE_PUT(9, C3 + 3, m_eye())
            PE_PUT(12, C3 + 6, m_eye())
            if constexpr (N == 19) U[18 * UW + C3 + 9] = 1.0;
        }
#undef PE_PUT
    }
    __syncthreads();
    // whitening: out[i][col] = sum_k S[i][k] U[k][col], dense, k ascending from zero
    const int n_out = jacobians ? N + NJ : N;
    double r_mine   = 0;
    for (int o = lane; o < n_out; o += 64) {
        int i, col;
        double *dst;
        if (o < N) {
            i = o, col = P, dst = r_out + o;
        } else {
            const int q = o - N;
            dst         = J_out + q;
            if (GIVEN) {
                i = q / P, col = q - i * P;
            } else { // the four blocks N x 7 | MIX | 7 | MIX, one after the other
                constexpr int O1 = N * C1, O2 = N * C2, O3 = N * C3;
                if (q < O1)
                    i = q / 7, col = q - i * 7;
                else if (q < O2)
                    i = (q - O1) / F::MIX, col = C1 + (q - O1) - i * F::MIX;
                else if (q < O3)
                    i = (q - O2) / 7, col = C2 + (q - O2) - i * 7;
                else
                    i = (q - O3) / F::MIX, col = C3 + (q - O3) - i * F::MIX;
            }
        }
        double s = 0;
#pragma unroll
        for (int k = 0; k < N; k++) s += S[i * N + k] * U[k * UW + col];
        *dst = s;
        if (GIVEN && o < N) r_mine = s; // (o == lane: the first pass of lanes 0 .. N-1)
    }
    if (GIVEN) {
        __shared__ double R[N];
        if (lane < N) R[lane] = r_mine;
        __syncthreads();
        if (lane == 0) {
            double s = 0;
            for (int k = 0; k < N; k++) s += R[k] * R[k];
            sq_norm[f] = s;
        }
    }
}

// ================================================================ host side ================================================================
// The kernels of a family, handed to the entry bodies by the file that defines them.
template <int N> struct kernels {
    void (*p1)(int, const int32_t *, const double *, const double *, const double *, int, double *, double *, double *, double *, double *, double *);
    void (*sqrt_info)(int, const double *, double *, int32_t *);
    void (*evaluate)(int, int, const double *, const double *, const double *, const double *, const int32_t *, const double *, const double *,
                     const double *, const int32_t *, double *, double *);
    void (*given)(int, const int32_t *, const double *, const double *, const double *, const double *, const int32_t *, const double *,
                  const double *, const double *, const double *, const double *, double *, double *, double *);
};

// P1 staging, *_batch (`entry` = "batch", per_interval = false: ONE parameter row for the launch, kernel row stride 0, no S) and *_batch_params
// (one row per interval, and — when the caller passes sqrt_info or status — the square-root information of every result formed behind the
// integration.  cov is then a mirrored output: the P1 kernel leaves it in the device arena, the square-root kernel reads it there, and one
// copy brings it down; S and status are written once per lane and go through the host mapping like the other outputs).
template <int N>
int batch_entry(const kernels<N> &K, const char *entry, bool per_interval, icg_ctx *ctx, int variant, int n_intervals, const int32_t *offsets,
                const double *imu, const double *state0, const double *params, double *cur_state, double *delta_state, double *jac, double *cov,
                double *delta_time, double *pn, double *sqrt_info, int32_t *status) {
    typedef family<N> F;
    constexpr int NN = N * N, EARTH = F::VARIANT0 + 1;
    if (!ctx) return ICG_ERR_INVALID;
    if (variant != F::VARIANT0 && variant != EARTH)
        return icg_fail(ctx, ICG_ERR_INVALID, "%s_%s: variant %d is neither %d (%s) nor %d (%s)", F::stem, entry, variant, F::VARIANT0, F::plain, EARTH,
                        F::earth);
    if (n_intervals < 0) return icg_fail(ctx, ICG_ERR_INVALID, "%s_%s: n_intervals = %d", F::stem, entry, n_intervals);
    if (n_intervals == 0) return ICG_OK;
    if (!offsets || !imu || !state0 || !params || !cur_state || !delta_state || !jac || !cov || !delta_time)
        return icg_fail(ctx, ICG_ERR_INVALID, "%s_%s: NULL argument", F::stem, entry);
    if (offsets[0] < 0) return icg_fail(ctx, ICG_ERR_INVALID, "%s_%s: interval 0: offsets[0] = %d", F::stem, entry, offsets[0]);
    for (int s = 0; s < n_intervals; s++)
        if (offsets[s + 1] - offsets[s] < 1) return icg_fail(ctx, ICG_ERR_INVALID, "%s_%s: interval %d has no IMU sample", F::stem, entry, s);
    const int total   = offsets[n_intervals];
    const size_t n    = (size_t) n_intervals;
    const bool want_S = sqrt_info || status;
    ICG_HIP(ctx, hipSetDevice(ctx->cfg.device));
    icg_call c(ctx);
    int rc = c.reserve((size_t) total * (8 * F::IMU + 32) + n * (8 * (F::STATE0 + F::PARAMS + F::CUR + F::DELTA + 1) + NN * 8 * 3 + 16) + 16 * 256);
    if (rc) return rc;
    const int32_t *d_off = c.in(offsets, n + 1);
    const double *d_imu  = c.in(imu, F::IMU * (size_t) total);
    const double *d_s0   = c.in(state0, F::STATE0 * n);
    const double *d_par  = c.in(params, F::PARAMS * (per_interval ? n : 1));
    if ((rc = c.seal())) return rc;
    double *d_cur = c.out_zc(cur_state, F::CUR * n);
    double *d_del = c.out_zc(delta_state, F::DELTA * n);
    double *d_jac = c.out_zc(jac, NN * n);
    double *d_dt  = c.out_zc(delta_time, n);
    // pn is written by the Earth variant only, rows begin .. begin + n - 2 of every interval: the other variant gets no buffer, and the one
    // row per interval that the kernel leaves alone is staged from the caller's, so that the copy back returns it unchanged
    double *d_pn  = (pn && variant == EARTH) ? c.out_zc(pn, 4 * (size_t) total) : nullptr;
    double *d_S   = want_S ? c.out_zc(sqrt_info, NN * n) : nullptr;
    int32_t *d_st = want_S ? c.out_zc(status, n) : nullptr;
    double *d_cov = want_S ? c.out(cov, NN * n) : c.out_zc(cov, NN * n); // (last: no zero-copy region inside the span copied back)
    ICG_LAUNCH_GUARD(c);
    if (d_pn)
        for (int s = 0; s < n_intervals; s++) {
            const size_t last = 4 * ((size_t) offsets[s + 1] - 1);
            memcpy(d_pn + last, pn + last, 4 * sizeof(double));
        }
    {
        icg_prof_scope ps(ctx, F::scope_p1);
        hipLaunchKernelGGL(K.p1, dim3(n_intervals), dim3(64), 0, ctx->stream, variant, d_off, d_imu, d_s0, d_par, per_interval ? F::PARAMS : 0, d_cur,
                           d_del, d_jac, d_cov, d_dt, d_pn);
    }
    if (want_S) {
        icg_prof_scope ps(ctx, F::scope_eval);
        hipLaunchKernelGGL(K.sqrt_info, dim3(n_intervals), dim3(64), 0, ctx->stream, n_intervals, (const double *) d_cov, d_S, d_st);
    }
    ICG_HIP(ctx, hipGetLastError());
    return c.finish();
}

// P2 for many factors at once: square-root information, then the evaluation.  Latency bound like P1 (a few KB in and out and a few thousand
// dependent FP64 operations per factor, no reuse across factors): reported as factors/s, not against the HBM roofline.
template <int N>
int evaluate_batch_entry(const kernels<N> &K, icg_ctx *ctx, int variant, int n_factors, const double *delta_state, const double *jac,
                         const double *cov, const double *delta_time, const double *env, const int32_t *pn_offsets, const double *pn,
                         const double *points, double *residuals, double *jacobians, double *sqrt_info, int32_t *status) {
    typedef family<N> F;
    constexpr int NN = N * N, NJ = widths<N>::NJ, EARTH = F::VARIANT0 + 1;
    if (!ctx) return ICG_ERR_INVALID;
    if (variant != F::VARIANT0 && variant != EARTH)
        return icg_fail(ctx, ICG_ERR_INVALID, "%s_evaluate_batch: variant %d is neither %d (%s) nor %d (%s)", F::stem, variant, F::VARIANT0, F::plain,
                        EARTH, F::earth);
    if (n_factors <= 0) return icg_fail(ctx, ICG_ERR_INVALID, "%s_evaluate_batch: n_factors = %d", F::stem, n_factors);
    if (!delta_state || !jac || !cov || !delta_time || !env || !points || !residuals || !status)
        return icg_fail(ctx, ICG_ERR_INVALID, "%s_evaluate_batch: NULL argument", F::stem);
    int total_pn = 0;
    if (variant == EARTH) {
        if (!pn_offsets) return icg_fail(ctx, ICG_ERR_INVALID, "%s_evaluate_batch: the %s variant needs pn_offsets", F::stem, F::earth);
        if (pn_offsets[0] < 0) return icg_fail(ctx, ICG_ERR_INVALID, "%s_evaluate_batch: pn_offsets[0] = %d", F::stem, pn_offsets[0]);
        for (int k = 0; k < n_factors; k++)
            if (pn_offsets[k + 1] < pn_offsets[k])
                return icg_fail(ctx, ICG_ERR_INVALID, "%s_evaluate_batch: pn_offsets not monotone at factor %d", F::stem, k);
        total_pn = pn_offsets[n_factors];
        if (total_pn > 0 && !pn) return icg_fail(ctx, ICG_ERR_INVALID, "%s_evaluate_batch: NULL pn", F::stem);
    }
    const size_t n = (size_t) n_factors;
    ICG_HIP(ctx, hipSetDevice(ctx->cfg.device));
    icg_call c(ctx);
    int rc = c.reserve(n * 8 * (F::DELTA + NN + NN + 1 + 4 + F::POINT + N + NJ + NN + 1) + (n + 1) * 4 + (size_t) total_pn * 32 + 16 * 256);
    if (rc) return rc;
    const double *d_del = c.in(delta_state, F::DELTA * n);
    const double *d_jac = c.in(jac, NN * n);
    const double *d_cov = c.in(cov, NN * n);
    const double *d_dt  = c.in(delta_time, n);
    const double *d_env = c.in(env, 4 * n);
    const double *d_pts = c.in(points, F::POINT * n);
    const int32_t *d_po = variant == EARTH ? c.in(pn_offsets, n + 1) : nullptr;
    const double *d_pn  = variant == EARTH ? c.in(pn, 4 * (size_t) total_pn) : nullptr;
    if ((rc = c.seal())) return rc;
    double *d_r   = c.out(residuals, N * n);
    double *d_J   = jacobians ? c.out(jacobians, NJ * n) : nullptr;
    double *d_S   = c.out(sqrt_info, NN * n); // (kept on the device only when the caller does not ask for it)
    int32_t *d_st = c.out(status, n);
    ICG_LAUNCH_GUARD(c);
    {
        icg_prof_scope ps(ctx, F::scope_eval);
        hipLaunchKernelGGL(K.sqrt_info, dim3(n_factors), dim3(64), 0, ctx->stream, n_factors, d_cov, d_S, d_st);
        hipLaunchKernelGGL(K.evaluate, dim3(n_factors), dim3(64), 0, ctx->stream, variant, n_factors, d_del, d_jac, d_dt, d_env, d_po, d_pn, d_pts,
                           (const double *) d_S, (const int32_t *) d_st, d_r, d_J);
    }
    ICG_HIP(ctx, hipGetLastError());
    return c.finish();
}

// ------------------------------------------------ P2 on a resident set of factors ------------------------------------------------
// What an integration result contributes to its factor is constant over a solve; only the evaluation point changes.  *_set keeps it on the
// device (one buffer, laid out as icg_preint_resident in icg_internal.h says); an evaluation ships POINT + 4 doubles per factor up and one
// squared norm back, and leaves the whitened residuals and Jacobians where the set owns them.  Each family has a resident struct of its own in
// the context: both sets may be resident at once.
struct set_view {
    const double *delta, *jac, *S, *dt, *env, *qnn, *pn;
    const int32_t *pn_off, *variant;
};
template <int N> set_view view_of(const icg_preint_resident &s) {
    constexpr int NN = N * N;
    const size_t n   = (size_t) s.n;
    set_view v;
    const double *p = reinterpret_cast<const double *>(s.d_set);
    v.delta = p, p += family<N>::DELTA * n;
    v.jac = p, p += NN * n;
    v.S = p, p += NN * n;
    v.dt = p, p += n;
    v.env = p, p += 4 * n;
    v.qnn = p, p += 4 * n;
    v.pn = p, p += 4 * (size_t) s.total_pn;
    v.pn_off  = reinterpret_cast<const int32_t *>(p);
    v.variant = v.pn_off + (n + 1);
    return v;
}

template <int N>
int set_entry(icg_ctx *ctx, int n_factors, const int32_t *variant, const double *delta_state, const double *jac, const double *sqrt_info,
              const double *delta_time, const double *env, const double *q_nn, const int32_t *pn_offsets, const double *pn) {
    typedef family<N> F;
    constexpr int NN = N * N, EARTH = F::VARIANT0 + 1;
    if (!ctx) return ICG_ERR_INVALID;
    icg_preint_resident &s = F::set_of(ctx);
    s.n                    = 0; // whatever set of this family the context held is gone, also when this call fails
    icg_resident_invalidate(s.out);
    if (n_factors <= 0) return icg_fail(ctx, ICG_ERR_INVALID, "%s_set: n_factors = %d", F::stem, n_factors);
    // before any array is read (the arrays of such a set are not looked at); the bound is also what keeps `bytes` and the grids in range
    if (n_factors > ICG_PREINT_SET_MAX)
        return icg_fail(ctx, ICG_ERR_CAPACITY, "%s_set: %d factors in one set (at most %d)", F::stem, n_factors, ICG_PREINT_SET_MAX);
    if (!variant || !delta_state || !jac || !sqrt_info || !delta_time || !env || !q_nn)
        return icg_fail(ctx, ICG_ERR_INVALID, "%s_set: NULL argument", F::stem);
    const size_t n = (size_t) n_factors;
    bool any_earth = false;
    for (size_t f = 0; f < n; f++) {
        if (variant[f] != F::VARIANT0 && variant[f] != EARTH)
            return icg_fail(ctx, ICG_ERR_INVALID, "%s_set: factor %zu: variant %d is neither %d (%s) nor %d (%s)", F::stem, f, variant[f], F::VARIANT0,
                            F::plain, EARTH, F::earth);
        any_earth |= variant[f] == EARTH;
    }
    int64_t total_pn = 0;
    if (pn_offsets) {
        if (pn_offsets[0] < 0) return icg_fail(ctx, ICG_ERR_INVALID, "%s_set: factor 0: pn_offsets[0] = %d", F::stem, pn_offsets[0]);
        for (size_t f = 0; f < n; f++)
            if (pn_offsets[f + 1] < pn_offsets[f]) return icg_fail(ctx, ICG_ERR_INVALID, "%s_set: factor %zu: pn_offsets not monotone", F::stem, f);
        total_pn = pn_offsets[n];
        if (total_pn > 0 && !pn) return icg_fail(ctx, ICG_ERR_INVALID, "%s_set: NULL pn for %lld rows", F::stem, (long long) total_pn);
    } else if (any_earth) {
        return icg_fail(ctx, ICG_ERR_INVALID, "%s_set: an %s factor needs pn_offsets", F::stem, F::earth);
    }
    const size_t n_dbl = (F::DELTA + NN + NN + 1 + 4 + 4) * n + 4 * (size_t) total_pn, bytes = 8 * n_dbl + 4 * (2 * n + 1);
    ICG_HIP(ctx, hipSetDevice(ctx->cfg.device));
    const int rc = icg_resident_upload(ctx, &s.d_set, &s.set_cap, bytes, F::scope_set, [&](char *host) {
        double *p = reinterpret_cast<double *>(host);
        memcpy(p, delta_state, 8 * F::DELTA * n), p += F::DELTA * n;
        memcpy(p, jac, 8 * NN * n), p += NN * n;
        memcpy(p, sqrt_info, 8 * NN * n), p += NN * n;
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
    });
    if (rc) return rc;
    s.total_pn = total_pn;
    s.n        = n_factors;
    return ICG_OK;
}

template <int N>
int evaluate_resident_entry(const kernels<N> &K, icg_ctx *ctx, const double *points, const double *q_corr, int want_jac, double *sq_norm) {
    typedef family<N> F;
    constexpr int NJ = widths<N>::NJ;
    if (!ctx) return ICG_ERR_INVALID;
    icg_preint_resident &s = F::set_of(ctx);
    if (int rc = icg_resident_require(ctx, s.out, s.n, ICG_NEED_SET, F::stem, "_evaluate_resident", F::what)) return rc;
    if (!points || !q_corr || !sq_norm) return icg_fail(ctx, ICG_ERR_INVALID, "%s_evaluate_resident: NULL argument", F::stem);
    ICG_HIP(ctx, hipSetDevice(ctx->cfg.device));
    const size_t n = (size_t) s.n;
    int rc         = icg_resident_reserve(ctx, s.out, 8 * N * n, want_jac ? 8 * NJ * n : 0);
    if (rc) return rc;
    icg_call c(ctx);
    if ((rc = c.reserve(8 * (F::POINT + 4 + 1) * n + 4 * 256))) return rc;
    const double *d_pts = c.in(points, F::POINT * n);
    const double *d_qc  = c.in(q_corr, 4 * n);
    if ((rc = c.seal())) return rc;
    double *d_sq = c.out(sq_norm, n);
    ICG_LAUNCH_GUARD(c);
    icg_resident_invalidate(s.out); // (until the kernel below is through)
    const set_view v = view_of<N>(s);
    {
        icg_prof_scope ps(ctx, F::scope_given);
        hipLaunchKernelGGL(K.given, dim3(s.n), dim3(64), 0, ctx->stream, s.n, v.variant, v.delta, v.jac, v.dt, v.env, v.pn_off, v.pn, d_pts, v.S, d_qc,
                           v.qnn, s.out.d_res, want_jac ? s.out.d_jac : (double *) nullptr, d_sq);
    }
    ICG_HIP(ctx, hipGetLastError());
    if ((rc = c.finish())) return rc;
    icg_resident_end(s.out, want_jac != 0);
    return ICG_OK;
}

template <int N> int fetch_resident_entry(icg_ctx *ctx, double *residuals, double *jacobians) {
    typedef family<N> F;
    typedef widths<N> W;
    if (!ctx) return ICG_ERR_INVALID;
    const icg_preint_resident &s = F::set_of(ctx);
    int rc;
    if ((rc = icg_resident_require(ctx, s.out, s.n, ICG_NEED_SET, F::stem, "_fetch_resident", F::what))) return rc;
    if (!residuals) return icg_fail(ctx, ICG_ERR_INVALID, "%s_fetch_resident: NULL residuals", F::stem);
    if ((rc = icg_resident_require(ctx, s.out, s.n, jacobians ? ICG_NEED_JACOBIANS : ICG_NEED_RESULTS, F::stem, "_fetch_resident", F::what))) return rc;
    ICG_HIP(ctx, hipSetDevice(ctx->cfg.device));
    const size_t n = (size_t) s.n;
    std::vector<double> JP(jacobians ? W::NJ * n : 0);
    ICG_HIP(ctx, hipMemcpyAsync(residuals, s.out.d_res, 8 * N * n, hipMemcpyDeviceToHost, ctx->stream));
    if (jacobians) ICG_HIP(ctx, hipMemcpyAsync(JP.data(), s.out.d_jac, 8 * W::NJ * n, hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = icg_stream_wait(ctx))) return rc;
    if (jacobians) // N x POINT row-major -> N x 7 | N x MIX | N x 7 | N x MIX
        for (size_t f = 0; f < n; f++)
            for (int b = 0; b < 4; b++) {
                const int c0 = W::col0[b], w = W::col0[b + 1] - c0;
                for (int i = 0; i < N; i++) memcpy(jacobians + W::NJ * f + W::off0[b] + i * w, &JP[W::NJ * f + F::POINT * i + c0], 8 * (size_t) w);
            }
    return ICG_OK;
}

} // namespace icg_preint
