// The small navigation factors of the window (host/nav_factors.h: GnssFactor, ImuErrorFactor, ImuPosePriorFactor, ImuMixPriorFactor and the
// odometer widths of the second and the fourth) as a resident set: icg_nav_set / _evaluate_resident / _correct_resident / _fetch_resident.
// Every Evaluate is restated operation for operation (no contraction, no trigonometry, no sqrt), so what stays on the device has the host's
// bit patterns.  Both kernels give a member 16 lanes, four members to a workgroup: a member is a few dozen operations, which one lane does
// into the member's LDS slot; the 16 lanes then store the slot as the contiguous run of doubles the concatenated layout makes of it.
#include <algorithm>

#include "icg_internal.h"
#include "dev_math.h"

using namespace icgd;

#define NAV_LANES 16      // per member
#define NAV_PER_BLOCK 4   // members per workgroup of 64
#define NAV_MAX_R 10      // residuals of the largest member
#define NAV_SLOT 112      // NAV_MAX_R residuals + 10 x 10 Jacobian entries, padded

static inline int nav_aux_len(int kind) { return kind == 0 ? 9 : kind == 2 ? 13 : kind == 3 ? 18 : kind == 5 ? 20 : 0; }

// ImuErrorFactor's constants (reference imu_error_factor.h:89-91)
#define NAV_GRY_BIAS_STD (7200 / 3600.0 * M_PI / 180.0)
#define NAV_ACC_BIAS_STD (2.0e4 * 1.0e-5)
#define NAV_ODO_SCALE_STD (2.0e4 * 1.0e-6)

// r (nr) and, with want_jac, the non-zero entries of J (nr x width row-major, zeroed by the caller) of one member
__device__ __forceinline__ void nav_member(int kind, const double *a, const double *x, double *r, double *J, bool want_jac) {
    switch (kind) {
    case 0: { // GnssFactor: a = blh3, std3, lever3
        const m33 R    = q_mat(q_from_xyzw(x + 3));
        const d3 lever = mk3(a[6], a[7], a[8]);
        const d3 rl    = m_vec(R, lever);
        const double w0 = 1.0 / a[3], w1 = 1.0 / a[4], w2 = 1.0 / a[5];
        r[0] = w0 * (x[0] + rl.x - a[0]);
        r[1] = w1 * (x[1] + rl.y - a[1]);
        r[2] = w2 * (x[2] + rl.z - a[2]);
        if (want_jac) {
            const double S[9] = {0, -lever.z, lever.y, lever.z, 0, -lever.x, -lever.y, lever.x, 0};
            const double w[3] = {w0, w1, w2};
#pragma unroll
            for (int i = 0; i < 3; i++) {
                J[i * 7 + i] = w[i];
#pragma unroll
                for (int j = 0; j < 3; j++)
                    J[i * 7 + 3 + j] = w[i] * -(R.a[i * 3 + 0] * S[0 * 3 + j] + R.a[i * 3 + 1] * S[1 * 3 + j] + R.a[i * 3 + 2] * S[2 * 3 + j]);
            }
        }
        break;
    }
    case 1:
    case 4: { // ImuErrorFactor, 6 x 9 or 7 x 10
        const int nc = kind == 4 ? 10 : 9;
#pragma unroll
        for (int k = 0; k < 3; k++) {
            r[k + 0] = x[k + 3] / NAV_GRY_BIAS_STD;
            r[k + 3] = x[k + 6] / NAV_ACC_BIAS_STD;
        }
        if (kind == 4) r[6] = x[9] / NAV_ODO_SCALE_STD;
        if (want_jac) {
#pragma unroll
            for (int k = 0; k < 3; k++) {
                J[(k + 0) * nc + k + 3] = 1.0 / NAV_GRY_BIAS_STD;
                J[(k + 3) * nc + k + 6] = 1.0 / NAV_ACC_BIAS_STD;
            }
            if (kind == 4) J[6 * nc + 9] = 1.0 / NAV_ODO_SCALE_STD;
        }
        break;
    }
    case 2: { // ImuPosePriorFactor: a = pose7, std6; d = q^-1 * q_p in the host's order
        const double n2 = x[3] * x[3] + x[4] * x[4] + x[5] * x[5] + x[6] * x[6];
        const double ax = -x[3] / n2, ay = -x[4] / n2, az = -x[5] / n2, aw = x[6] / n2;
        const double bx = a[3], by = a[4], bz = a[5], bw = a[6];
        const double dx = aw * bx + ax * bw + ay * bz - az * by;
        const double dy = aw * by + ay * bw + az * bx - ax * bz;
        const double dz = aw * bz + az * bw + ax * by - ay * bx;
        const double dw = aw * bw - ax * bx - ay * by - az * bz;
        const double w[6] = {1.0 / a[7], 1.0 / a[8], 1.0 / a[9], 1.0 / a[10], 1.0 / a[11], 1.0 / a[12]};
        r[0] = w[0] * (x[0] - a[0]);
        r[1] = w[1] * (x[1] - a[1]);
        r[2] = w[2] * (x[2] - a[2]);
        r[3] = w[3] * (2 * dx);
        r[4] = w[4] * (2 * dy);
        r[5] = w[5] * (2 * dz);
        if (want_jac) {
            const double B[9] = {dw, dz, -dy, -dz, dw, dx, dy, -dx, dw};
#pragma unroll
            for (int k = 0; k < 3; k++) J[k * 7 + k] = w[k];
#pragma unroll
            for (int i = 0; i < 3; i++)
#pragma unroll
                for (int j = 0; j < 3; j++) J[(3 + i) * 7 + 3 + j] = w[3 + i] * -B[i * 3 + j];
        }
        break;
    }
    default: { // 3, 5: ImuMixPriorFactor, 9 x 9 or 10 x 10: a = mix, std
        const int nc = kind == 5 ? 10 : 9;
        for (int k = 0; k < nc; k++) {
            r[k] = (x[k] - a[k]) / a[nc + k];
            if (want_jac) J[k * nc + k] = 1.0 / a[nc + k];
        }
        break;
    }
    }
}

__global__ __launch_bounds__(64) void k_nav_evaluate(int n, const int32_t *kind, const int32_t *aux_off, const int32_t *r_off, const int32_t *j_off,
                                                     const int32_t *p_off, const double *aux, const double *points, double *res, double *jac,
                                                     double *sq_norm) {
    __shared__ double slot[NAV_PER_BLOCK][NAV_SLOT];
    const int g = threadIdx.x / NAV_LANES, sub = threadIdx.x % NAV_LANES;
    const int f     = blockIdx.x * NAV_PER_BLOCK + g;
    const bool live = f < n;
    const int kd    = live ? kind[f] : 0;
    const int nr = icg_nav_nr(kd), nj = nr * icg_nav_width(kd);
    double *S = slot[g];
    if (jac)
        for (int e = sub; e < nj; e += NAV_LANES) S[NAV_MAX_R + e] = 0.0;
    __syncthreads();
    if (live && sub == 0) {
        nav_member(kd, aux + aux_off[f], points + p_off[f], S, S + NAV_MAX_R, jac != nullptr);
        double s = 0;
        for (int k = 0; k < nr; k++) s += S[k] * S[k];
        sq_norm[f] = s;
    }
    __syncthreads();
    if (live) {
        if (sub < nr) res[r_off[f] + sub] = S[sub];
        if (jac) {
            double *J = jac + j_off[f];
            for (int e = sub; e < nj; e += NAV_LANES) J[e] = S[NAV_MAX_R + e];
        }
    }
}

// the corrector of ResidualBlockInfo::Evaluate on the kept results of the marked members: a lane per column, then a lane per residual
__global__ __launch_bounds__(64) void k_nav_correct(int n, const int32_t *kind, const int32_t *r_off, const int32_t *j_off, const uint8_t *robust,
                                                    const double *corr, double *res, double *jac) {
    const int g = threadIdx.x / NAV_LANES, sub = threadIdx.x % NAV_LANES;
    const int f     = blockIdx.x * NAV_PER_BLOCK + g;
    const bool live = f < n && robust[f] != 0;
    const int kd    = live ? kind[f] : 0;
    const int nr = icg_nav_nr(kd), nc = icg_nav_width(kd);
    double *r = live ? res + r_off[f] : res, *J = live ? jac + j_off[f] : jac;
    if (live && sub < nc) {
        const double sqrt_rho1 = corr[3 * (size_t) f], alpha_sq_norm = corr[3 * (size_t) f + 1];
        double rtj = 0;
        for (int k = 0; k < nr; k++) rtj += r[k] * J[k * nc + sub];
        for (int k = 0; k < nr; k++) {
            const double j  = J[k * nc + sub];
            J[k * nc + sub] = sqrt_rho1 * (j - alpha_sq_norm * r[k] * rtj);
        }
    }
    __syncthreads(); // the residuals are scaled after every column of the member has read them
    if (live && sub < nr) r[sub] = r[sub] * corr[3 * (size_t) f + 2];
}

namespace {
struct nav_view {
    const double *aux;
    const int32_t *kind, *aux_off, *r_off, *j_off, *p_off;
};
nav_view nav_set_view(const icg_nav_resident &s) {
    const size_t n = (size_t) s.n;
    nav_view v;
    v.aux     = reinterpret_cast<const double *>(s.d_set);
    v.kind    = reinterpret_cast<const int32_t *>(v.aux + s.total_aux);
    v.aux_off = v.kind + n;
    v.r_off   = v.aux_off + n;
    v.j_off   = v.r_off + (n + 1);
    v.p_off   = v.j_off + (n + 1);
    return v;
}
inline int nav_grid(int n) { return (n + NAV_PER_BLOCK - 1) / NAV_PER_BLOCK; }
} // namespace

extern "C" int icg_nav_set(icg_ctx *ctx, int n_members, const int32_t *kind, const int32_t *aux_off, const double *aux) {
    if (!ctx) return ICG_ERR_INVALID;
    icg_nav_resident &s = ctx->nav;
    s.n                 = 0; // whatever nav set the context held is gone, also when this call fails
    icg_resident_invalidate(s.out), s.corrected = s.any_robust = false;
    if (n_members <= 0) return icg_fail(ctx, ICG_ERR_INVALID, "icg_nav_set: n = %d", n_members);
    if (n_members > ICG_NAV_SET_MAX) // (before any array is read)
        return icg_fail(ctx, ICG_ERR_CAPACITY, "icg_nav_set: %d members in one set (at most %d)", n_members, ICG_NAV_SET_MAX);
    if (!kind || !aux_off || !aux) return icg_fail(ctx, ICG_ERR_INVALID, "icg_nav_set: NULL argument");
    const size_t n = (size_t) n_members;
    if (aux_off[0] < 0) return icg_fail(ctx, ICG_ERR_INVALID, "icg_nav_set: member 0: aux_off[0] = %d", aux_off[0]);
    for (size_t f = 0; f < n; f++) {
        if (kind[f] < 0 || kind[f] > 5) return icg_fail(ctx, ICG_ERR_INVALID, "icg_nav_set: member %zu: kind %d is outside 0..5", f, kind[f]);
        if (aux_off[f + 1] < aux_off[f]) return icg_fail(ctx, ICG_ERR_INVALID, "icg_nav_set: member %zu: aux_off not monotone", f);
        if (aux_off[f + 1] - aux_off[f] < nav_aux_len(kind[f]))
            return icg_fail(ctx, ICG_ERR_INVALID, "icg_nav_set: member %zu: kind %d reads %d constants, the member owns %d", f, kind[f],
                            nav_aux_len(kind[f]), aux_off[f + 1] - aux_off[f]);
    }
    const size_t total_aux = (size_t) aux_off[n], bytes = 8 * total_aux + 4 * (5 * n + 3);
    s.h_kind.assign(kind, kind + n);
    s.h_r_off.assign(n + 1, 0), s.h_j_off.assign(n + 1, 0), s.h_p_off.assign(n + 1, 0);
    for (size_t f = 0; f < n; f++) {
        s.h_r_off[f + 1] = s.h_r_off[f] + icg_nav_nr(kind[f]);
        s.h_j_off[f + 1] = s.h_j_off[f] + icg_nav_nr(kind[f]) * icg_nav_width(kind[f]);
        s.h_p_off[f + 1] = s.h_p_off[f] + icg_nav_width(kind[f]);
    }
    ICG_HIP(ctx, hipSetDevice(ctx->cfg.device));
    const int rc = icg_resident_upload(ctx, &s.d_set, &s.set_cap, bytes, "nav_set", [&](char *host) {
        double *p = reinterpret_cast<double *>(host);
        if (total_aux) memcpy(p, aux, 8 * total_aux);
        int32_t *q = reinterpret_cast<int32_t *>(p + total_aux);
        memcpy(q, kind, 4 * n), q += n;
        memcpy(q, aux_off, 4 * n), q += n;
        memcpy(q, s.h_r_off.data(), 4 * (n + 1)), q += n + 1;
        memcpy(q, s.h_j_off.data(), 4 * (n + 1)), q += n + 1;
        memcpy(q, s.h_p_off.data(), 4 * (n + 1));
    });
    if (rc) return rc;
    s.total_aux = (int64_t) total_aux;
    s.n         = n_members;
    return ICG_OK;
}

extern "C" int icg_nav_evaluate_resident(icg_ctx *ctx, const double *points, const int32_t *point_off, int want_jac, double *sq_norm) {
    if (!ctx) return ICG_ERR_INVALID;
    icg_nav_resident &s = ctx->nav;
    if (int rc = icg_resident_require(ctx, s.out, s.n, ICG_NEED_SET, "icg_nav", "_evaluate_resident", "nav")) return rc;
    if (!points || !point_off || !sq_norm) return icg_fail(ctx, ICG_ERR_INVALID, "icg_nav_evaluate_resident: NULL argument");
    const size_t n = (size_t) s.n;
    for (size_t f = 0; f < n; f++)
        if (point_off[f] < 0) return icg_fail(ctx, ICG_ERR_INVALID, "icg_nav_evaluate_resident: member %zu: point_off = %d", f, point_off[f]);
    ICG_HIP(ctx, hipSetDevice(ctx->cfg.device));
    const size_t total_r = (size_t) s.h_r_off[n], total_j = (size_t) s.h_j_off[n], total_p = (size_t) s.h_p_off[n];
    int rc = icg_resident_reserve(ctx, s.out, 8 * total_r, want_jac ? 8 * total_j : 0);
    if (rc) return rc;
    icg_call c(ctx);
    if ((rc = c.reserve(8 * (total_p + n) + 4 * 256))) return rc;
    // the members' blocks, packed in member order: the kernel reads no address the caller's offsets name
    double *d_pts, *p = c.stage<double>(total_p, &d_pts);
    if (!p) return c.overflowed();
    for (size_t f = 0; f < n; f++) memcpy(p + s.h_p_off[f], points + point_off[f], 8 * (size_t) (s.h_p_off[f + 1] - s.h_p_off[f]));
    if ((rc = c.seal())) return rc;
    double *d_sq = c.out(sq_norm, n);
    ICG_LAUNCH_GUARD(c);
    icg_resident_invalidate(s.out), s.corrected = false; // (until the kernel below is through)
    const nav_view v = nav_set_view(s);
    {
        icg_prof_scope ps(ctx, "nav_eval");
        hipLaunchKernelGGL(k_nav_evaluate, dim3(nav_grid(s.n)), dim3(64), 0, ctx->stream, s.n, v.kind, v.aux_off, v.r_off, v.j_off, v.p_off, v.aux,
                           (const double *) d_pts, s.out.d_res, want_jac ? s.out.d_jac : (double *) nullptr, d_sq);
    }
    ICG_HIP(ctx, hipGetLastError());
    if ((rc = c.finish())) return rc;
    icg_resident_end(s.out, want_jac != 0);
    return ICG_OK;
}

extern "C" int icg_nav_correct_resident(icg_ctx *ctx, const uint8_t *robust, const double *corr) {
    if (!ctx) return ICG_ERR_INVALID;
    icg_nav_resident &s = ctx->nav;
    int rc;
    if ((rc = icg_resident_require(ctx, s.out, s.n, ICG_NEED_SET, "icg_nav", "_correct_resident", "nav"))) return rc;
    if (!robust || !corr) return icg_fail(ctx, ICG_ERR_INVALID, "icg_nav_correct_resident: NULL argument");
    if ((rc = icg_resident_require(ctx, s.out, s.n, ICG_NEED_JACOBIANS, "icg_nav", "_correct_resident", "nav"))) return rc;
    if (s.corrected) return icg_fail(ctx, ICG_ERR_INVALID, "icg_nav_correct_resident: the last evaluation was corrected already");
    ICG_HIP(ctx, hipSetDevice(ctx->cfg.device));
    const size_t n = (size_t) s.n;
    icg_call c(ctx);
    if ((rc = c.reserve(n * (1 + 24) + 4 * 256))) return rc;
    const uint8_t *d_rob = c.in(robust, n);
    const double *d_corr = c.in(corr, 3 * n);
    if ((rc = c.seal())) return rc;
    ICG_LAUNCH_GUARD(c);
    icg_resident_invalidate(s.out); // (until the kernel below is through)
    const nav_view v = nav_set_view(s);
    {
        icg_prof_scope ps(ctx, "nav_correct");
        hipLaunchKernelGGL(k_nav_correct, dim3(nav_grid(s.n)), dim3(64), 0, ctx->stream, s.n, v.kind, v.r_off, v.j_off, d_rob, d_corr, s.out.d_res, s.out.d_jac);
    }
    ICG_HIP(ctx, hipGetLastError());
    if ((rc = c.finish())) return rc;
    icg_resident_end(s.out, true), s.corrected = true;
    for (size_t f = 0; f < n; f++) s.any_robust |= robust[f] != 0;
    return ICG_OK;
}

extern "C" int icg_nav_fetch_resident(icg_ctx *ctx, double *residuals, double *jacobians) {
    if (!ctx) return ICG_ERR_INVALID;
    const icg_nav_resident &s = ctx->nav;
    int rc;
    if ((rc = icg_resident_require(ctx, s.out, s.n, ICG_NEED_SET, "icg_nav", "_fetch_resident", "nav"))) return rc;
    if (!residuals) return icg_fail(ctx, ICG_ERR_INVALID, "icg_nav_fetch_resident: NULL residuals");
    if ((rc = icg_resident_require(ctx, s.out, s.n, jacobians ? ICG_NEED_JACOBIANS : ICG_NEED_RESULTS, "icg_nav", "_fetch_resident", "nav"))) return rc;
    ICG_HIP(ctx, hipSetDevice(ctx->cfg.device));
    const size_t n = (size_t) s.n;
    ICG_HIP(ctx, hipMemcpyAsync(residuals, s.out.d_res, 8 * (size_t) s.h_r_off[n], hipMemcpyDeviceToHost, ctx->stream));
    if (jacobians) ICG_HIP(ctx, hipMemcpyAsync(jacobians, s.out.d_jac, 8 * (size_t) s.h_j_off[n], hipMemcpyDeviceToHost, ctx->stream));
    return icg_stream_wait(ctx);
}
