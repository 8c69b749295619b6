// The reduced camera solve on the device: solver_detail::choleskySolve (host/dense_kernels.cc) for many systems at once, one WAVE per
// system — icg_chol_solve_batch, and the solve step of icg_reproj_solve_windows (reproj_schur.hip).
//
// The host solve is fixed-order arithmetic: column tiles of two, every element one subtraction of a dot8-ordered inner product of two row
// prefixes (eight interleaved partial sums combined as ((p0+p4)+(p2+p6))+((p1+p5)+(p3+p7)), then the tail in order), the second column of a
// tile the "- l00 * C1[j]" term behind it, then the division; the diagonal tests in the order d0, d1; the forward solve with dot8; the
// backward column sweep.  Here lane (i mod 64) of the wave owns row i and forms the sums of its own elements serially, in the host's order,
// one multiply and one add per term (the file is built with -ffp-contract=off, like marg.hip / marg_linearize.hip); FP64 division and square
// root are correctly rounded on the device.  The result is the host's, bit for bit.
//
// A wave needs no barrier: the lanes run in lock-step, so a tile is (A) every lane subtracts the two inner products of its rows >= j,
// (B) the owners of rows j and j + 1 finish the diagonal tile and the wave learns c00, c10, c11 by lane broadcast, (C) every lane divides its
// rows > j + 1; one memory fence per tile orders (C)'s stores before the next tile's reads of the two new pivot rows.
//
// The right-hand side rides along as row n of the matrix: the forward solve's y[j] = (b[j] - dot8(A_j, y, j)) / A_jj is exactly the first
// column's arithmetic on that row, and for the second column (j + 1 is odd, so dot8 over j + 1 terms has the same eight-blocks as dot8 over j
// terms and one more term at the end of its tail) y[j + 1] = (b[j + 1] - (E + (t + y[j] * c10))) / c11 with E and t the two halves of the
// row's inner product with C1: the forward solve costs no pass of its own.
//
// Storage: the lower triangle packed, row i at i (i + 1) / 2, and the right-hand side behind it: n (n + 1) / 2 + n doubles — 18.8 KB at C2's
// visual P = 67, 100.5 KB at the estimator's P = 157.  It lives in LDS when it fits (k_chol_solve<true>; up to four waves = systems share a
// workgroup's LDS, fewer when the launch has not enough systems to fill the CUs that way), in a global scratch block otherwise
// (k_chol_solve<false>, the same code, up to n = 512).  Which of the two a system takes depends on its own n only.
#include "icg_internal.h"

#include <atomic>
#include <cmath>

#define CHOL_MAX_WAVES 4

namespace {

__host__ __device__ static inline size_t chol_row(int i) { return ((size_t) i * ((size_t) i + 1)) >> 1; }
__host__ __device__ static inline size_t chol_doubles(int n) { return chol_row(n) + (size_t) n; }

// orders the wave's stores before its later loads (other lanes' rows); the lanes of a wave run in lock-step, no s_barrier is involved
__device__ __forceinline__ void chol_wave_sync() {
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// the inner products of the row prefix R with the prefixes C0 and C1 (length j) as dot8 forms them: E = the combined eight partial sums,
// t = the tail; dot8 = E + t
__device__ __forceinline__ void chol_dots(const double *R, const double *C0, const double *C1, int j, double &E0, double &t0, double &E1, double &t1) {
    double p[8] = {0, 0, 0, 0, 0, 0, 0, 0}, q[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int k = 0;
    for (; k + 8 <= j; k += 8) {
#pragma unroll
        for (int u = 0; u < 8; u++) {
            const double r = R[k + u];
            p[u] += r * C0[k + u];
            q[u] += r * C1[k + u];
        }
    }
    t0 = 0.0, t1 = 0.0;
    for (; k < j; k++) {
        const double r = R[k];
        t0 += r * C0[k];
        t1 += r * C1[k];
    }
    E0 = ((p[0] + p[4]) + (p[2] + p[6])) + ((p[1] + p[5]) + (p[3] + p[7]));
    E1 = ((q[0] + q[4]) + (q[2] + q[6])) + ((q[1] + q[5]) + (q[3] + q[7]));
}

__device__ __forceinline__ bool chol_bad_pivot(double d) { return !(d > 0.0) || !isfinite(d); }

// grid: ceil(n_items / wpg) workgroups of wpg waves; dynamic LDS: wpg * lds_stride doubles (IN_LDS)
template <bool IN_LDS>
__global__ __launch_bounds__(64 * CHOL_MAX_WAVES) void k_chol_solve(int n_items, int wpg, int lds_stride, const int32_t *__restrict__ items,
                                                                    const icg_chol_desc *__restrict__ desc, icg_chol_ptrs p) {
    extern __shared__ double chol_lds[];
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int it = (int) blockIdx.x * wpg + wave;
    if (it >= n_items) return; // (whole waves leave: the kernel has no barrier)
    const int w = items[it];
    const icg_chol_desc D = desc[w];
    const int n = D.n;
    double *T = IN_LDS ? chol_lds + (size_t) wave * lds_stride : p.scratch + D.s_off;
    double *x = p.x + D.x_off;
    // ---- the host factors' part: kept on the device until it is replaced
    const double *Hsrc = nullptr;
    if (D.flags & ICG_CHOL_PART_NEW) {
        Hsrc        = p.Hnew + D.Hnew_off;
        double *dst = p.H + D.H_off;
        for (size_t e = lane; e < chol_row(n); e += 64) dst[e] = Hsrc[e];
    } else if (D.flags & ICG_CHOL_PART) {
        Hsrc = p.H + D.H_off;
    }
    if (!(D.flags & ICG_CHOL_SOLVE)) {
        for (int k = lane; k < D.x_len; k += 64) x[k] = 0.0;
        if (p.status && lane == 0) p.status[w] = 0;
        return;
    }
    // ---- A = (lower(A) + lower(host part)) + dd on the diagonal, the right-hand side behind it
    {
        const double *A = p.A + D.A_off, *dd = D.dd_off >= 0 ? p.dd + D.dd_off : nullptr;
        for (int i = 0; i < n; i++) {
            const double *Ai = A + (size_t) i * D.ldA;
            double *Ti       = T + chol_row(i);
            for (int k = lane; k <= i; k += 64) {
                double v = Ai[k];
                if (Hsrc) v = v + Hsrc[chol_row(i) + k];
                if (dd && k == i) v = v + dd[i];
                Ti[k] = v;
            }
        }
        const double *b = p.b + D.b_off;
        for (int k = lane; k < n; k += 64) T[chol_row(n) + k] = b[k];
    }
    chol_wave_sync();
    // ---- factorization and forward solve: rows j .. n of column tile (j, j + 1); row n is the right-hand side
    bool failed = false;
    double bE = 0.0, bt = 0.0; // the right-hand side's inner product with C1, kept by the lane that owns row n
    for (int j = 0; j < n; j += 2) {
        const bool pair = j + 1 < n;
        double *C0 = T + chol_row(j), *C1 = pair ? T + chol_row(j + 1) : C0;
        const int i0 = lane >= j ? lane : lane + (((j - lane + 63) >> 6) << 6); // the lane's first row >= j
        for (int i = i0; i <= n; i += 64) {                                     // (A)
            double *R = T + chol_row(i);
            double E0, t0, E1, t1;
            chol_dots(R, C0, C1, j, E0, t0, E1, t1);
            R[j] = R[j] - (E0 + t0);
            if (pair && i > j) {
                if (i < n)
                    R[j + 1] = R[j + 1] - (E1 + t1);
                else
                    bE = E1, bt = t1;
            }
        }
        double c00 = 0.0, c10 = 0.0, c11 = 0.0; // (B)
        int bad = 0;
        if (lane == (j & 63)) {
            const double d0 = C0[j];
            bad             = chol_bad_pivot(d0);
            c00             = sqrt(d0);
            C0[j]           = c00;
        }
        c00 = __shfl(c00, j & 63);
        if (__shfl(bad, j & 63)) {
            failed = true;
            break;
        }
        if (pair) {
            if (lane == ((j + 1) & 63)) {
                c10             = C1[j] / c00;
                C1[j]           = c10;
                const double d1 = C1[j + 1] - c10 * c10;
                bad             = chol_bad_pivot(d1);
                c11             = sqrt(d1);
                C1[j + 1]       = c11;
            }
            c10 = __shfl(c10, (j + 1) & 63);
            c11 = __shfl(c11, (j + 1) & 63);
            if (__shfl(bad, (j + 1) & 63)) {
                failed = true;
                break;
            }
        }
        const int jl = pair ? j + 2 : j + 1; // (C)
        const int i1 = lane >= jl ? lane : lane + (((jl - lane + 63) >> 6) << 6);
        for (int i = i1; i <= n; i += 64) {
            double *R        = T + chol_row(i);
            const double l00 = R[j] / c00;
            R[j]             = l00;
            if (pair) {
                if (i < n)
                    R[j + 1] = (R[j + 1] - l00 * c10) / c11;
                else
                    R[j + 1] = (R[j + 1] - (bE + (bt + l00 * c10))) / c11;
            }
        }
        chol_wave_sync();
    }
    if (failed) {
        for (int k = lane; k < D.x_len; k += 64) x[k] = 0.0;
        if (p.status && lane == 0) p.status[w] = 1;
        return;
    }
    // ---- L^T x = y as the host's column sweep: y[k] is only ever touched by lane k mod 64
    double *Y = T + chol_row(n);
    for (int r = n - 1; r >= 0; r--) {
        const double *Ar = T + chol_row(r);
        double xr        = 0.0;
        if (lane == (r & 63)) {
            xr   = Y[r] / Ar[r];
            Y[r] = xr;
        }
        xr = __shfl(xr, r & 63);
        for (int k = lane; k < r; k += 64) Y[k] = Y[k] - Ar[k] * xr;
    }
    for (int k = lane; k < D.x_len; k += 64) x[k] = k < n ? Y[k] : 0.0;
    if (p.L && D.L_off >= 0) {
        double *L = p.L + D.L_off;
        for (int i = 0; i < n; i++)
            for (int k = lane; k <= i; k += 64) L[(size_t) i * n + k] = T[chol_row(i) + k];
    }
    if (p.status && lane == 0) p.status[w] = 0;
}

int chol_cu_count(icg_ctx *ctx) {
    static std::atomic<int> per_dev[16];
    const int dev = ctx->cfg.device & 15;
    int v         = per_dev[dev].load(std::memory_order_relaxed);
    if (v == 0) {
        if (hipDeviceGetAttribute(&v, hipDeviceAttributeMultiprocessorCount, ctx->cfg.device) != hipSuccess || v <= 0) v = 256;
        per_dev[dev].store(v, std::memory_order_relaxed);
    }
    return v;
}

} // namespace

int icg_chol_plan_build(icg_ctx *ctx, std::vector<icg_chol_desc> &desc, icg_chol_plan &plan) {
    const size_t n = desc.size(), limit = icg_lds_limit(ctx); // (k_chol_solve has no static LDS)
    plan.items.resize(n);
    plan.n_lds = plan.n_glob = 0;
    size_t stride = 0, scratch = 0;
    std::vector<char> fast(n);
    for (size_t w = 0; w < n; w++) {
        const size_t need = chol_doubles(desc[w].n);
        fast[w]           = need * sizeof(double) <= limit;
        desc[w].s_off     = (int64_t) scratch;
        if (fast[w]) {
            plan.n_lds++;
            if (need > stride) stride = need;
        } else {
            scratch += need;
        }
    }
    {
        int a = 0, z = plan.n_lds;
        for (size_t w = 0; w < n; w++) plan.items[(size_t) (fast[w] ? a++ : z++)] = (int32_t) w;
    }
    plan.n_glob     = (int) n - plan.n_lds;
    plan.lds_stride = (int) stride;
    // waves per workgroup: as many as the LDS holds, at most four, and not more than it takes to give every CU a workgroup
    const int fit  = stride ? (int) std::min<size_t>(CHOL_MAX_WAVES, limit / (stride * sizeof(double))) : 1;
    const int want = (plan.n_lds + chol_cu_count(ctx) - 1) / chol_cu_count(ctx);
    plan.wpg       = std::max(1, std::min(fit, want));
    return icg_grow(ctx, (void **) &ctx->d_chol_scratch, &ctx->chol_scratch_cap, scratch * sizeof(double), scratch * sizeof(double));
}

int icg_chol_enqueue(icg_ctx *ctx, const icg_chol_plan &plan, const icg_chol_desc *d_desc, const int32_t *d_items, icg_chol_ptrs p) {
    p.scratch = ctx->d_chol_scratch;
    if (plan.n_lds > 0) {
        const size_t lds = (size_t) plan.wpg * plan.lds_stride * sizeof(double);
        static icg_lds_grant granted;
        if (int rc = icg_allow_lds(ctx, reinterpret_cast<const void *>(k_chol_solve<true>), lds, icg_lds_limit(ctx), granted)) return rc;
        icg_prof_scope ps(ctx, "chol_solve_lds");
        hipLaunchKernelGGL(k_chol_solve<true>, dim3((unsigned) ((plan.n_lds + plan.wpg - 1) / plan.wpg)), dim3(64 * plan.wpg), lds, ctx->stream, plan.n_lds,
                           plan.wpg, plan.lds_stride, d_items, d_desc, p);
    }
    if (plan.n_glob > 0) {
        icg_prof_scope ps(ctx, "chol_solve_global");
        hipLaunchKernelGGL(k_chol_solve<false>, dim3((unsigned) plan.n_glob), dim3(64), 0, ctx->stream, plan.n_glob, 1, 0, d_items + plan.n_lds, d_desc, p);
    }
    ICG_HIP(ctx, hipGetLastError());
    return ICG_OK;
}

extern "C" int icg_chol_solve_batch(icg_ctx *ctx, int n_systems, const int32_t *n, const double *A, const double *b, double *x, double *L, int32_t *status) {
    if (!ctx) return ICG_ERR_INVALID;
    if (n_systems <= 0) return icg_fail(ctx, ICG_ERR_INVALID, "icg_chol_solve_batch: n_systems = %d", n_systems);
    if (n_systems > 65535) return icg_fail(ctx, ICG_ERR_CAPACITY, "icg_chol_solve_batch: %d systems in one call (at most 65535)", n_systems);
    if (!n || !A || !b || !x) return icg_fail(ctx, ICG_ERR_INVALID, "icg_chol_solve_batch: NULL argument");
    const size_t ns = (size_t) n_systems;
    for (size_t w = 0; w < ns; w++)
        if (n[w] <= 0) return icg_fail(ctx, ICG_ERR_INVALID, "icg_chol_solve_batch: system %zu: n = %d", w, n[w]);
    for (size_t w = 0; w < ns; w++) // (after the argument checks: an invalid batch is invalid whatever its size)
        if (n[w] > ICG_CHOL_MAX_N)
            return icg_fail(ctx, ICG_ERR_CAPACITY, "icg_chol_solve_batch: system %zu: n = %d is above the limit %d", w, n[w], ICG_CHOL_MAX_N);
    ICG_HIP(ctx, hipSetDevice(ctx->cfg.device));
    std::vector<icg_chol_desc> desc(ns);
    size_t ta = 0, tb = 0;
    for (size_t w = 0; w < ns; w++) {
        desc[w] = {n[w], n[w], n[w], ICG_CHOL_SOLVE, (int64_t) ta, -1, -1, -1, (int64_t) tb, (int64_t) tb, L ? (int64_t) ta : -1, 0};
        ta += (size_t) n[w] * n[w], tb += (size_t) n[w];
    }
    icg_chol_plan plan;
    int rc = icg_chol_plan_build(ctx, desc, plan);
    if (rc) return rc;
    icg_call c(ctx);
    if ((rc = c.reserve(sizeof(double) * (2 * ta + 2 * tb) + ns * (sizeof(icg_chol_desc) + 8) + 16 * 256))) return rc;
    icg_chol_ptrs p{};
    p.A                         = c.in(A, ta);
    p.b                         = c.in(b, tb);
    const icg_chol_desc *d_desc = c.in(desc.data(), ns);
    const int32_t *d_items      = c.in(plan.items.data(), ns);
    if ((rc = c.seal())) return rc;
    // the factor comes back through a private block: only its lower triangles are handed on, what lies above the caller's diagonals stays
    std::vector<double> Lfull(L ? ta : 0);
    std::vector<int32_t> st_own(status ? 0 : ns);
    if (!status) status = st_own.data();
    p.x      = c.out(x, tb);
    p.status = c.out(status, ns);
    p.L      = L ? c.out(Lfull.data(), ta) : nullptr;
    ICG_LAUNCH_GUARD(c);
    if ((rc = icg_chol_enqueue(ctx, plan, d_desc, d_items, p))) return rc;
    if ((rc = c.finish())) return rc;
    if (L) {
        for (size_t w = 0; w < ns; w++) {
            if (status[w]) continue; // (no factor exists)
            const size_t off = (size_t) desc[w].A_off, nn = (size_t) n[w];
            for (size_t i = 0; i < nn; i++) memcpy(L + off + i * nn, Lfull.data() + off + i * nn, sizeof(double) * (i + 1));
        }
    }
    return ICG_OK;
}
