// M4: MarginalizationFactor::Evaluate (factors/marginalization_factor.h:47-101) for many priors at once, with the priors RESIDENT on the
// device.  A prior (x0, J0, e0 and its block layout) is constant between two marginalizations while every LM iteration evaluates it at a
// new x: icg_marg_prior_set uploads the priors of many windows once (icg_marg_prior_set_from_kept takes them where a kept linearization
// left them; both through one store kernel that reads each window at a pointer of its own), icg_marg_prior_evaluate ships only x in and e (optionally the
// Jacobian blocks, J0^T e and |e|^2) out; icg_marg_prior_evaluate_resident keeps e on the device for the host-part kernel (host_part.hip) and
// ships |e|^2 only.  FP64, no contraction; every sum is formed in the host's order (host/factors.cc
// evaluateMargPrior, oracle/orc_marg.cc), so the residuals and Jacobian blocks are the same IEEE values bit for bit, alone or in a batch.
#include "icg_internal.h"

#define MARG_THREADS 256
#define MARG_TILE 32

namespace {

// what the kernels read of the resident set (device pointers)
struct marg_dev {
    const int32_t *r;        // n: retained size of window w
    const int32_t *blk_off;  // n+1: window w owns blocks [blk_off[w], blk_off[w+1])
    const int32_t *e_off;    // n+1: first residual of window w (prefix sum of r)
    const int32_t *x_off;    // n+1: first parameter of window w in x / x0
    const int32_t *blk_size; // per block: global size (7 = pose, local 6)
    const int32_t *blk_index;// per block: first local column
    const int32_t *blk_xoff; // per block: first parameter in x / x0
    const int32_t *x_blk;    // per parameter of x: the block it belongs to
    const int64_t *j_off;    // n+1: first element of window w's J0 (prefix sum of r^2)
    const int64_t *jac_off;  // n+1: first element of window w's Jacobian blocks (prefix sum of r * sum(size))
    const double *J;         // J0 of every window, row-major
    const double *JT;        // the same matrices transposed: what a thread per row reads coalesced
    const double *e0, *x0;
};

// Set time: the row-major J0 of every window into its two resident forms, and its e0.  The windows of a set may come from different places:
// window w's J0 is read at src_J[w] and its e0 at src_e[w] — a window of a kept linearization (icg_lin_kept, this context's or another's on
// the device; icg_marg_prior_set_from_kept) or of the part the host shipped (every window of icg_marg_prior_set).  32 x 32 tiles: the source
// is read and J written along rows, JT written along rows from the padded tile; the workgroups of tile 0 also gather the window's e0.
__global__ __launch_bounds__(MARG_THREADS) void k_marg_store_from(int n_windows, const int32_t *__restrict__ r_of, const int64_t *__restrict__ j_off,
                                                                  const int32_t *__restrict__ e_off, const double *const *__restrict__ src_J,
                                                                  const double *const *__restrict__ src_e, double *__restrict__ J, double *__restrict__ JT,
                                                                  double *__restrict__ e0) {
    __shared__ double tile[MARG_TILE][MARG_TILE + 1];
    const int w = blockIdx.y;
    if (w >= n_windows) return;
    const int r = r_of[w], nt = (r + MARG_TILE - 1) / MARG_TILE;
    const double *s = src_J[w];
    double *d = J + j_off[w], *dt = JT + j_off[w];
    if (blockIdx.x == 0) {
        const double *se = src_e[w];
        double *de       = e0 + e_off[w];
        for (int i = threadIdx.x; i < r; i += MARG_THREADS) de[i] = se[i];
    }
    const int tx = threadIdx.x & (MARG_TILE - 1), ty = threadIdx.x / MARG_TILE; // 32 x 8
    for (int t = blockIdx.x; t < nt * nt; t += gridDim.x) {                      // (uniform per workgroup)
        const int ti = t / nt, tj = t - ti * nt;
        for (int y = ty; y < MARG_TILE; y += MARG_THREADS / MARG_TILE) {
            const int i = ti * MARG_TILE + y, k = tj * MARG_TILE + tx;
            if (i < r && k < r) {
                const double v = s[(size_t) i * r + k];
                d[(size_t) i * r + k] = v;
                tile[y][tx]           = v;
            }
        }
        __syncthreads();
        for (int y = ty; y < MARG_TILE; y += MARG_THREADS / MARG_TILE) {
            const int k = tj * MARG_TILE + y, i = ti * MARG_TILE + tx;
            if (i < r && k < r) dt[(size_t) k * r + i] = tile[tx][y];
        }
        __syncthreads();
    }
}

// One workgroup per window.  dx (a thread per block) and e (a thread per row) live in LDS; a row's sum is one thread's chain of r
// dependent multiply-add pairs in k order — latency-bound by construction, the window count is what fills the chip.
__global__ __launch_bounds__(MARG_THREADS) void k_marg_evaluate(int n_windows, marg_dev m, const double *__restrict__ x, double *__restrict__ residuals,
                                                                double *__restrict__ gradient, double *__restrict__ sq_norm) {
    __shared__ double dx[ICG_MARG_MAX_R], e[ICG_MARG_MAX_R];
    const int w = blockIdx.x, tid = threadIdx.x;
    if (w >= n_windows) return;
    const int r = m.r[w], b0 = m.blk_off[w], b1 = m.blk_off[w + 1], eo = m.e_off[w];
    for (int i = tid; i < r; i += MARG_THREADS) dx[i] = 0.0; // columns no block covers stay 0
    __syncthreads();
    for (int b = b0 + tid; b < b1; b += MARG_THREADS) { // :61-77
        const int size = m.blk_size[b], index = m.blk_index[b], xo = m.blk_xoff[b];
        const double *xb = x + xo, *x0 = m.x0 + xo;
        if (size == 7) {
            const double n2 = x0[3] * x0[3] + x0[4] * x0[4] + x0[5] * x0[5] + x0[6] * x0[6];
            const double ax = -x0[3] / n2, ay = -x0[4] / n2, az = -x0[5] / n2, aw = x0[6] / n2;
            const double bx = xb[3], by = xb[4], bz = xb[5], bw = xb[6];
            const double dqx = aw * bx + ax * bw + ay * bz - az * by;
            const double dqy = aw * by + ay * bw + az * bx - ax * bz;
            const double dqz = aw * bz + az * bw + ax * by - ay * bx;
            const double dqw = aw * bw - ax * bx - ay * by - az * bz;
            for (int k = 0; k < 3; k++) dx[index + k] = xb[k] - x0[k];
            const double sgn = dqw < 0 ? -2.0 : 2.0;
            dx[index + 3]    = sgn * dqx;
            dx[index + 4]    = sgn * dqy;
            dx[index + 5]    = sgn * dqz;
        } else {
            for (int k = 0; k < size; k++) dx[index + k] = xb[k] - x0[k];
        }
    }
    __syncthreads();
    const double *JT = m.JT + m.j_off[w];
    for (int i = tid; i < r; i += MARG_THREADS) { // e = e0 + J0 dx (:79-80)
        double s = 0;
#pragma unroll 8
        for (int k = 0; k < r; k++) s += JT[(size_t) k * r + i] * dx[k];
        const double v = m.e0[eo + i] + s;
        e[i]             = v;
        residuals[eo + i] = v;
    }
    if (!gradient && !sq_norm) return;
    __syncthreads();
    if (gradient) {
        const double *J = m.J + m.j_off[w];
        for (int k = tid; k < r; k += MARG_THREADS) {
            double s = 0;
#pragma unroll 8
            for (int i = 0; i < r; i++) s += J[(size_t) i * r + k] * e[i];
            gradient[eo + k] = s;
        }
    }
    if (sq_norm && tid == MARG_THREADS - 1) { // (the last thread: idle in the passes above unless r is a multiple of the workgroup)
        double s = 0;
        for (int i = 0; i < r; i++) s += e[i] * e[i];
        sq_norm[w] = s;
    }
}

// The Jacobian blocks Ceres receives (:83-98): a pure copy, a thread per output element.  Window w's output is its blocks concatenated,
// block b an r x size[b] row-major matrix starting at r * (parameters in front of b): element o lies in the block of parameter o / r.
__global__ __launch_bounds__(MARG_THREADS) void k_marg_jacobians(int n_windows, marg_dev m, double *__restrict__ jacobians) {
    const int w = blockIdx.y;
    if (w >= n_windows) return;
    const int r = m.r[w], xo = m.x_off[w];
    const int total = (int) (m.jac_off[w + 1] - m.jac_off[w]); // (icg_marg_prior_set keeps a window's count below 2^31 - grid size)
    const double *J = m.J + m.j_off[w];
    double *out     = jacobians + m.jac_off[w];
    for (int o = blockIdx.x * MARG_THREADS + threadIdx.x; o < total; o += gridDim.x * MARG_THREADS) {
        const int c = o / r, b = m.x_blk[xo + c];
        const int size = m.blk_size[b], index = m.blk_index[b], local = size == 7 ? 6 : size;
        const int rem = o - r * (m.blk_xoff[b] - xo);
        const int i = rem / size, j = rem - i * size;
        out[o] = j < local ? J[(size_t) i * r + index + j] : 0.0;
    }
}

marg_dev marg_view(const icg_marg_set &s) {
    const size_t n = (size_t) s.n, B = (size_t) s.n_blocks;
    marg_dev m;
    m.j_off   = reinterpret_cast<const int64_t *>(s.d_meta);
    m.jac_off = m.j_off + (n + 1);
    const int32_t *p = reinterpret_cast<const int32_t *>(m.jac_off + (n + 1));
    m.r = p, p += n;
    m.blk_off = p, p += n + 1;
    m.e_off = p, p += n + 1;
    m.x_off = p, p += n + 1;
    m.blk_size = p, p += B;
    m.blk_index = p, p += B;
    m.blk_xoff = p, p += B;
    m.x_blk = p;
    m.J = s.d_J, m.JT = s.d_J + s.total_j;
    m.e0 = s.d_e0, m.x0 = s.d_x0;
    return m;
}

// Both set entries.  Window w takes J0 / e0 from window src[w] of the kept linearization keep_id (src[w] >= 0) or from the next window of
// J0 / e0 (src[w] == -1), which hold only those windows.  src == NULL (icg_marg_prior_set): every window is a -1; from_kept only picks the entry's argument check and profiler scope.
int marg_set(const char *fn, bool from_kept, icg_ctx *ctx, uint64_t keep_id, int n_windows, const int32_t *src, const int32_t *r, const int32_t *block_off,
             const int32_t *block_size, const int32_t *block_index, const double *x0, const double *J0, const double *e0) {
    if (!ctx) return ICG_ERR_INVALID;
    icg_marg_set &s = ctx->marg;
    s.n             = 0; // whatever set the context held is gone, also when this call fails
    icg_resident_invalidate(s.out); // and so are the residuals it kept
    if (n_windows <= 0) return icg_fail(ctx, ICG_ERR_INVALID, "%s: n_windows = %d", fn, n_windows);
    if (n_windows > 65535) return icg_fail(ctx, ICG_ERR_CAPACITY, "%s: %d windows in one set (at most 65535)", fn, n_windows);
    if (!r || !block_off || !block_size || !block_index || !x0 || (from_kept ? !src : (!J0 || !e0))) return icg_fail(ctx, ICG_ERR_INVALID, "%s: NULL argument", fn);
    if (block_off[0] != 0) return icg_fail(ctx, ICG_ERR_INVALID, "%s: window 0: block_off[0] = %d", fn, block_off[0]);
    const size_t n = (size_t) n_windows;
    for (size_t w = 0; w < n; w++) {
        if (r[w] <= 0) return icg_fail(ctx, ICG_ERR_INVALID, "%s: window %zu: r = %d", fn, w, r[w]);
        if (block_off[w + 1] < block_off[w]) return icg_fail(ctx, ICG_ERR_INVALID, "%s: window %zu: block_off not monotone", fn, w);
        for (int b = block_off[w]; b < block_off[w + 1]; b++) {
            const int size = block_size[b], index = block_index[b], local = size == 7 ? 6 : size;
            if (size <= 0 || index < 0 || (int64_t) index + local > r[w])
                return icg_fail(ctx, ICG_ERR_INVALID, "%s: window %zu: block %d (size %d, index %d) does not fit r = %d", fn, w,
                                b - block_off[w], size, index, r[w]);
        }
    }
    const icg_lin_kept *K = nullptr;
    const auto src_of = [&](size_t w) { return src ? src[w] : -1; };
    size_t host_j = 0, host_e = 0; // elements of J0 / e0: the windows the host ships
    {
        bool any_kept = false;
        for (size_t w = 0; w < n; w++) {
            if (src_of(w) < -1) return icg_fail(ctx, ICG_ERR_INVALID, "%s: window %zu: src = %d", fn, w, src[w]);
            any_kept |= src_of(w) >= 0;
        }
        // (the id is looked at whenever a window names it; a set of shipped windows alone needs none)
        const icg_ctx *owner = any_kept ? icg_kept_lookup(keep_id) : nullptr;
        if (any_kept && !owner)
            return icg_fail(ctx, ICG_ERR_INVALID, "%s: the kept linearization %llu is gone (released, replaced by a later linearize call, or its context destroyed)", fn,
                            (unsigned long long) keep_id);
        if (owner && owner->cfg.device != ctx->cfg.device)
            return icg_fail(ctx, ICG_ERR_INVALID, "%s: the kept linearization %llu lives on device %d, this context on device %d", fn, (unsigned long long) keep_id,
                            owner->cfg.device, ctx->cfg.device);
        K = owner ? &owner->lin_kept : nullptr;
        for (size_t w = 0; w < n; w++) {
            if (src_of(w) < 0) {
                if (!J0 || !e0) return icg_fail(ctx, ICG_ERR_INVALID, "%s: window %zu: src = -1 and no host J0 / e0", fn, w);
                host_j += (size_t) r[w] * r[w], host_e += (size_t) r[w];
                continue;
            }
            if ((size_t) src[w] >= K->r.size())
                return icg_fail(ctx, ICG_ERR_INVALID, "%s: window %zu: src = %d, the kept linearization has %zu windows", fn, w, src[w], K->r.size());
            if (K->r[(size_t) src[w]] != r[w])
                return icg_fail(ctx, ICG_ERR_INVALID, "%s: window %zu: r = %d, kept window %d has r = %d", fn, w, r[w], src[w], K->r[(size_t) src[w]]);
        }
    }
    for (size_t w = 0; w < n; w++) // (after the argument checks: an invalid set is invalid whatever its size)
        if (r[w] > ICG_MARG_MAX_R)
            return icg_fail(ctx, ICG_ERR_CAPACITY, "%s: window %zu: r = %d is above the limit %d", fn, w, r[w], ICG_MARG_MAX_R);
    // layout: int64 j_off, jac_off (n+1 each) | int32 r, blk_off, e_off, x_off, blk_size, blk_index, blk_xoff, x_blk
    const size_t B = (size_t) block_off[n];
    size_t X       = 0;
    for (size_t b = 0; b < B; b++) X += (size_t) block_size[b];
    if (X > (size_t) 1 << 30) return icg_fail(ctx, ICG_ERR_CAPACITY, "%s: %zu parameters in one set", fn, X);
    const size_t meta_bytes = 2 * (n + 1) * 8 + (n + 3 * (n + 1) + 3 * B + X) * 4;
    s.h_meta.assign((meta_bytes + 7) / 8, 0);
    int64_t *j_off = s.h_meta.data(), *jac_off = j_off + (n + 1);
    int32_t *p = reinterpret_cast<int32_t *>(jac_off + (n + 1));
    int32_t *m_r = p, *m_boff = p + n, *m_eoff = m_boff + (n + 1), *m_xoff = m_eoff + (n + 1), *m_size = m_xoff + (n + 1), *m_index = m_size + B,
            *m_bxoff = m_index + B, *m_xblk = m_bxoff + B;
    int64_t tj = 0, tjac = 0, te = 0, tx = 0, max_jac = 0;
    int max_r = 0;
    for (size_t w = 0; w < n; w++) {
        m_r[w] = r[w], m_boff[w] = block_off[w], m_eoff[w] = (int32_t) te, m_xoff[w] = (int32_t) tx;
        j_off[w] = tj, jac_off[w] = tjac;
        int64_t xs = 0;
        for (int b = block_off[w]; b < block_off[w + 1]; b++) {
            m_size[b] = block_size[b], m_index[b] = block_index[b], m_bxoff[b] = (int32_t) (tx + xs);
            for (int k = 0; k < block_size[b]; k++) m_xblk[tx + xs + k] = b;
            xs += block_size[b];
        }
        tx += xs, te += r[w], tj += (int64_t) r[w] * r[w], tjac += (int64_t) r[w] * xs;
        if ((int64_t) r[w] * xs > max_jac) max_jac = (int64_t) r[w] * xs;
        if (r[w] > max_r) max_r = r[w];
    }
    if (max_jac > (int64_t) 1 << 30) return icg_fail(ctx, ICG_ERR_CAPACITY, "%s: %lld Jacobian elements in one window", fn, (long long) max_jac);
    if (te > (int64_t) 1 << 30) return icg_fail(ctx, ICG_ERR_CAPACITY, "%s: %lld residuals in one set", fn, (long long) te);
    s.h_r.assign(m_r, m_r + n), s.h_e_off.assign(m_eoff, m_eoff + n), s.h_j_off.assign(j_off, j_off + n); // (for host_part.hip)
    m_boff[n] = block_off[n], m_eoff[n] = (int32_t) te, m_xoff[n] = (int32_t) tx, j_off[n] = tj, jac_off[n] = tjac;

    ICG_HIP(ctx, hipSetDevice(ctx->cfg.device));
    int rc;
    const size_t b_J = sizeof(double) * 2 * (size_t) tj, b_e0 = sizeof(double) * (size_t) te, b_x0 = sizeof(double) * (size_t) (tx > 0 ? tx : 1);
    if ((rc = icg_grow(ctx, (void **) &s.d_J, &s.J_cap, b_J, b_J))) return rc;
    if ((rc = icg_grow(ctx, (void **) &s.d_e0, &s.e0_cap, b_e0, b_e0))) return rc;
    if ((rc = icg_grow(ctx, (void **) &s.d_x0, &s.x0_cap, b_x0, b_x0))) return rc;
    if ((rc = icg_grow(ctx, (void **) &s.d_meta, &s.meta_cap, s.h_meta.size() * 8, s.h_meta.size() * 8))) return rc;
    icg_call c(ctx);
    if ((rc = c.reserve(sizeof(double) * (host_j + host_e + (size_t) tx) + s.h_meta.size() * 8 + 2 * n * sizeof(double *) + 8 * 256))) return rc;
    const double *a_J    = c.in(J0, host_j);
    const double *a_e0   = c.in(e0, host_e);
    const double *a_x0   = c.in(x0, (size_t) tx);
    const int64_t *a_met = c.in(s.h_meta.data(), s.h_meta.size());
    const double *const *a_src;
    { // where window w's J0 (n entries) and e0 (n more) lie on the device
        std::vector<const double *> from(2 * n);
        size_t hj = 0, he = 0;
        for (size_t w = 0; w < n; w++) {
            if (src_of(w) < 0) {
                from[w] = a_J + hj, from[n + w] = a_e0 + he;
                hj += (size_t) r[w] * r[w], he += (size_t) r[w];
            } else {
                from[w] = K->d_buf + K->rr_off[(size_t) src[w]], from[n + w] = K->d_buf + K->total_rr + K->r_off[(size_t) src[w]];
            }
        }
        a_src = c.in(from.data(), 2 * n);
    }
    if ((rc = c.seal())) return rc;
    ICG_LAUNCH_GUARD(c);
    ICG_HIP(ctx, hipMemcpyAsync(s.d_meta, a_met, s.h_meta.size() * 8, hipMemcpyDeviceToDevice, ctx->stream));
    if (tx > 0) ICG_HIP(ctx, hipMemcpyAsync(s.d_x0, a_x0, sizeof(double) * (size_t) tx, hipMemcpyDeviceToDevice, ctx->stream));
    {
        const int nt         = (max_r + MARG_TILE - 1) / MARG_TILE;
        const int32_t *a_r32 = reinterpret_cast<const int32_t *>(a_met + 2 * (n + 1));
        icg_prof_scope ps(ctx, from_kept ? "marg_set_from" : "marg_set");
        hipLaunchKernelGGL(k_marg_store_from, dim3(nt * nt, n_windows), dim3(MARG_THREADS), 0, ctx->stream, n_windows, a_r32, a_met, a_r32 + n + (n + 1), a_src,
                           a_src + n, s.d_J, s.d_J + tj, s.d_e0);
    }
    ICG_HIP(ctx, hipGetLastError());
    if ((rc = c.finish())) return rc;
    s.n_blocks = (int) B, s.total_r = te, s.total_x = tx, s.total_j = tj, s.total_jac = tjac, s.max_jac = max_jac;
    s.n = n_windows;
    return ICG_OK;
}

} // namespace

extern "C" int icg_marg_prior_set(icg_ctx *ctx, int n_windows, const int32_t *r, const int32_t *block_off, const int32_t *block_size,
                                  const int32_t *block_index, const double *x0, const double *J0, const double *e0) {
    return marg_set("icg_marg_prior_set", false, ctx, 0, n_windows, nullptr, r, block_off, block_size, block_index, x0, J0, e0);
}

// The same set with J0 / e0 taken where icg_marg_linearize_batch_keep left them (factors/marginalization_info.h:153-192 →
// factors/marginalization_factor.h:47-101 without the detour through the host).
extern "C" int icg_marg_prior_set_from_kept(icg_ctx *ctx, uint64_t keep_id, int n_windows, const int32_t *src, const int32_t *r, const int32_t *block_off,
                                            const int32_t *block_size, const int32_t *block_index, const double *x0, const double *J0_host,
                                            const double *e0_host) {
    return marg_set("icg_marg_prior_set_from_kept", true, ctx, keep_id, n_windows, src, r, block_off, block_size, block_index, x0, J0_host, e0_host);
}

extern "C" int icg_marg_prior_evaluate(icg_ctx *ctx, const double *x, double *residuals, double *jacobians, double *gradient, double *sq_norm) {
    if (!ctx) return ICG_ERR_INVALID;
    const icg_marg_set &s = ctx->marg;
    if (int rc = icg_resident_require(ctx, s.out, s.n, ICG_NEED_SET, "icg_marg_prior", "_evaluate", "prior")) return rc;
    if (!residuals || (!x && s.total_x > 0)) return icg_fail(ctx, ICG_ERR_INVALID, "icg_marg_prior_evaluate: NULL argument");
    ICG_HIP(ctx, hipSetDevice(ctx->cfg.device));
    const size_t n = (size_t) s.n;
    icg_call c(ctx);
    int rc = c.reserve(sizeof(double) * (size_t) (s.total_x + 2 * s.total_r + (jacobians ? s.total_jac : 0) + (int64_t) n) + 8 * 256);
    if (rc) return rc;
    const double *d_x = c.in(x, (size_t) s.total_x);
    if ((rc = c.seal())) return rc;
    double *d_r   = c.out(residuals, (size_t) s.total_r);
    double *d_g   = gradient ? c.out(gradient, (size_t) s.total_r) : nullptr;
    double *d_sq  = sq_norm ? c.out(sq_norm, n) : nullptr;
    double *d_jac = jacobians ? c.out(jacobians, (size_t) s.total_jac) : nullptr;
    ICG_LAUNCH_GUARD(c);
    const marg_dev m = marg_view(s);
    {
        icg_prof_scope ps(ctx, "marg_eval");
        hipLaunchKernelGGL(k_marg_evaluate, dim3(s.n), dim3(MARG_THREADS), 0, ctx->stream, s.n, m, d_x, d_r, d_g, d_sq);
    }
    if (d_jac && s.max_jac > 0) {
        icg_prof_scope ps(ctx, "marg_jac");
        int64_t gx = (s.max_jac + MARG_THREADS - 1) / MARG_THREADS;
        if (gx > 1024) gx = 1024;
        hipLaunchKernelGGL(k_marg_jacobians, dim3((unsigned) gx, s.n), dim3(MARG_THREADS), 0, ctx->stream, s.n, m, d_jac);
    }
    ICG_HIP(ctx, hipGetLastError());
    return c.finish();
}

// The same evaluation with the residuals left where icg_reproj_host_parts_build_prior reads them (the set's own buffer): x up, one squared
// norm per window back.  k_marg_evaluate as above, so sq_norm[w] is the value icg_marg_prior_evaluate returns, bit for bit.
extern "C" int icg_marg_prior_evaluate_resident(icg_ctx *ctx, const double *x, double *sq_norm) {
    if (!ctx) return ICG_ERR_INVALID;
    icg_marg_set &s = ctx->marg;
    if (int rc = icg_resident_require(ctx, s.out, s.n, ICG_NEED_SET, "icg_marg_prior", "_evaluate_resident", "prior")) return rc;
    if (!sq_norm || (!x && s.total_x > 0)) return icg_fail(ctx, ICG_ERR_INVALID, "icg_marg_prior_evaluate_resident: NULL argument");
    ICG_HIP(ctx, hipSetDevice(ctx->cfg.device));
    const size_t n = (size_t) s.n, b_res = sizeof(double) * (size_t) s.total_r;
    int rc = icg_resident_reserve(ctx, s.out, b_res, 0);
    if (rc) return rc;
    icg_call c(ctx);
    if ((rc = c.reserve(sizeof(double) * (size_t) (s.total_x + (int64_t) n) + 4 * 256))) return rc;
    const double *d_x = c.in(x, (size_t) s.total_x);
    if ((rc = c.seal())) return rc;
    double *d_sq = c.out(sq_norm, n);
    ICG_LAUNCH_GUARD(c);
    icg_resident_invalidate(s.out); // (until the kernel below is through)
    {
        icg_prof_scope ps(ctx, "marg_eval");
        hipLaunchKernelGGL(k_marg_evaluate, dim3(s.n), dim3(MARG_THREADS), 0, ctx->stream, s.n, marg_view(s), d_x, s.out.d_res, (double *) nullptr, d_sq);
    }
    ICG_HIP(ctx, hipGetLastError());
    if ((rc = c.finish())) return rc;
    icg_resident_end(s.out, false);
    return ICG_OK;
}
