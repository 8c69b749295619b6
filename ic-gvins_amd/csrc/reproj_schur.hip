// f1: landmark elimination, back-substitution and cost of the resident reprojection factors, one window or many windows per launch.
//
// Reference: the DENSE_SCHUR step of GVINS::gvinsOptimization (ic_gvins.cc:1130-1239, 1763-1837): the inverse-depth blocks (1 x 1) go first.
// The systems are assembled by reproj_asm.hip (layout of a window's block: there); this file reduces them, solves for the landmarks and
// holds every entry point that does so: icg_reproj_schur*, _backsub*, _cost*, _landmark_diag*, _accumulate_normal, _solve_windows.
#include <chrono>
#include <cstdio>
#include <cstdlib>

#include "reproj_internal.h"
#include "../host/lm_min_rule.h"

__global__ void k_schur_inv_w(const win_desc *wd, int P, double *sys, double min_diag, double max_diag) {
    const win_desc W = wd[blockIdx.y];
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= W.L) return;
    const int N = P + W.L;
    const double *H = sys + W.sys_off;
    double *inv = sys + W.sys_off + (size_t) N * N + N;
    const double h = H[(size_t) (P + l) * N + P + l];
    // a landmark without any active factor has an empty row: it is left where it is (delta_l = 0)
    inv[l] = h > 0.0 ? 1.0 / (h + fmin(fmax(h, min_diag), max_diag) * W.damp) : 0.0;
}

// S = Hcc - G^T diag(inv) G,  s = bc - G^T (inv b_l),  diag = diag(Hcc).
// Rounds 1-5 ran 16 x 16 output tiles of one thread per element, every tile re-reading its two G panels from memory with two barriers per 16
// landmarks: 157-199 us for 256 windows of a 0.35 GFLOP contraction.  Now a workgroup owns (up to 256 of) the 4 x 4 register tiles of the
// LOWER triangle of one window's S: the G rows of 32 landmarks are staged in LDS once per pass and every thread reads its row and column
// quadruples from there (4 ds_read_b128 per landmark for 16 FMAs).  The upper triangle is the mirror image of the lower one (S is
// symmetric; the factorizations read rows >= columns): written as such when the caller wants the full matrix, not at all otherwise.
// Landmarks are added in index order: the value of a window does not depend on the batch it is reduced in.
#define SCH_LT 32 // landmark rows per pass (fewer for wide systems: LT * 4 TQ <= 3 072 elements, twelve per thread)
#define SCH_PRE 12
// grid (ceil(NT / 256), W), NT = TQ (TQ + 1) / 2 lower tiles, TQ = ceil(P / 4); dynamic LDS: LT * 4 TQ doubles (G) + 2 LT (inv, b_l)
__global__ __launch_bounds__(256) void k_schur_reduce_w(const win_desc *wd, int P, int LT, const double *sys, double *S, double *s, double *diag,
                                                       int lower_only) {
    extern __shared__ double sm[];
    const win_desc W = wd[blockIdx.y];
    const int L = W.L, N = P + L, TQ = (P + 3) >> 2, PP = 4 * TQ, NT = (TQ * (TQ + 1)) >> 1;
    const double *H = sys + W.sys_off, *b = H + (size_t) N * N, *inv = b + N;
    double *g = sm, *sw = sm + LT * PP, *swb = sw + LT;
    const int t = threadIdx.x, tid = blockIdx.x * 256 + t;
    // tile (ti, tj), tj <= ti, from the triangular index
    int ti = (int) ((sqrtf(8.0f * (float) tid + 1.0f) - 1.0f) * 0.5f);
    while ((ti + 1) * (ti + 2) / 2 <= tid) ti++;
    while (ti * (ti + 1) / 2 > tid) ti--;
    const int tj     = tid - ti * (ti + 1) / 2;
    const bool owner = tid < NT;
    double acc[4][4];
#pragma unroll
    for (int rr = 0; rr < 4; rr++)
#pragma unroll
        for (int cc = 0; cc < 4; cc++) acc[rr][cc] = 0.0;
    double accs[2] = {0.0, 0.0}; // s entries t and t + 256 (the window's first workgroup; P <= 512)
    // staging: element e = t + 256 k of a pass is row e / PP, column e % PP of the slice; the next pass is fetched into registers while
    // this one is multiplied (one workgroup per CU at 256 windows: nobody else would hide the round trip)
    int pl[SCH_PRE], pc[SCH_PRE];
    double pre[SCH_PRE];
#pragma unroll
    for (int k = 0; k < SCH_PRE; k++) {
        const int e = t + 256 * k;
        pl[k] = e / PP, pc[k] = e - pl[k] * PP;
        if (e >= LT * PP) pl[k] = -1;
    }
    auto fetch = [&](int l0) {
#pragma unroll
        for (int k = 0; k < SCH_PRE; k++) {
            pre[k] = 0.0;
            if (pl[k] >= 0 && l0 + pl[k] < L && pc[k] < P) pre[k] = H[(size_t) (P + l0 + pl[k]) * N + pc[k]];
        }
    };
    fetch(0);
    for (int l0 = 0; l0 < L; l0 += LT) {
        const int nl = min(LT, L - l0);
        __syncthreads();
#pragma unroll
        for (int k = 0; k < SCH_PRE; k++)
            if (pl[k] >= 0) g[t + 256 * k] = pre[k];
        if (t < LT) sw[t] = t < nl ? inv[l0 + t] : 0.0, swb[t] = t < nl ? b[P + l0 + t] : 0.0;
        __syncthreads();
        if (l0 + LT < L) fetch(l0 + LT);
        if (owner) {
            for (int l = 0; l < nl; l++) {
                const double wl  = sw[l];
                const double2 a0 = *reinterpret_cast<const double2 *>(&g[l * PP + 4 * ti]), a1 = *reinterpret_cast<const double2 *>(&g[l * PP + 4 * ti + 2]);
                const double2 b0 = *reinterpret_cast<const double2 *>(&g[l * PP + 4 * tj]), b1 = *reinterpret_cast<const double2 *>(&g[l * PP + 4 * tj + 2]);
                const double av[4] = {a0.x * wl, a0.y * wl, a1.x * wl, a1.y * wl}, bv[4] = {b0.x, b0.y, b1.x, b1.y};
#pragma unroll
                for (int rr = 0; rr < 4; rr++)
#pragma unroll
                    for (int cc = 0; cc < 4; cc++) acc[rr][cc] = fma(av[rr], bv[cc], acc[rr][cc]);
            }
        }
        if (blockIdx.x == 0) {
#pragma unroll
            for (int k = 0; k < 2; k++) {
                const int i = t + 256 * k;
                if (i < P)
                    for (int l = 0; l < nl; l++) accs[k] = fma(g[l * PP + i] * sw[l], swb[l], accs[k]);
            }
        }
    }
    if (owner) {
        double *Sw = S + (size_t) blockIdx.y * P * P;
#pragma unroll
        for (int rr = 0; rr < 4; rr++)
#pragma unroll
            for (int cc = 0; cc < 4; cc++) {
                const int i = 4 * ti + rr, j = 4 * tj + cc;
                if (i >= P || j > i) continue; // (cells above the diagonal inside a diagonal tile are mirrors too)
                const double v       = H[(size_t) i * N + j] - acc[rr][cc];
                Sw[(size_t) i * P + j] = v;
                if (!lower_only && j < i) Sw[(size_t) j * P + i] = v;
            }
    }
    if (blockIdx.x == 0) {
#pragma unroll
        for (int k = 0; k < 2; k++) {
            const int i = t + 256 * k;
            if (i < P) s[(size_t) blockIdx.y * P + i] = b[i] - accs[k], diag[(size_t) blockIdx.y * P + i] = H[(size_t) i * N + i];
        }
    }
}

// one wave per landmark (global index): delta_l = (b_l - G_l . delta_c) * inv_l; lterms[l][2] = b_l^2 / (h_ll + d_l), d_l delta_l^2 — the
// landmark's part of the LM model decrease 0.5 (delta^T b + delta^T D delta): with the reduced right-hand side s, delta^T b =
// delta_c^T s + sum lterms[.][0], so the step-quality ratio is formed without moving G or b_l to the host
__global__ __launch_bounds__(64) void k_schur_backsub_w(const win_desc *wd, const int32_t *lm_win, int lm_base, int P, const double *sys,
                                                        const double *delta_c, double *delta_l, double *lterms, double min_diag, double max_diag) {
    const int lg = lm_base + blockIdx.x, wi = lm_win ? lm_win[lg] : 0;
    const win_desc W = wd[wi];
    const int l = lg - W.lm_begin, N = P + W.L;
    const double *H = sys + W.sys_off, *b = H + (size_t) N * N, *inv = b + N;
    const double *dc = delta_c + (size_t) wi * P;
    double acc = 0.0;
    for (int i = threadIdx.x; i < P; i += 64) acc += H[(size_t) (P + l) * N + i] * dc[i];
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (threadIdx.x == 0) {
        const double bl = b[P + l], wv = inv[l];
        const double d  = (bl - acc) * wv;
        delta_l[lg]     = d;
        double t0 = 0.0, t1 = 0.0;
        if (wv > 0.0) {
            const double dl = fmin(fmax(H[(size_t) (P + l) * N + P + l], min_diag), max_diag) * W.damp; // the damping that went into inv
            t0 = bl * bl * wv, t1 = dl * d * d;
        }
        lterms[2 * (size_t) lg] = t0, lterms[2 * (size_t) lg + 1] = t1;
    }
}

// sum of 256 per-thread partial sums in a fixed tree: butterfly inside each wave, the four wave sums in order
__device__ __forceinline__ double block_sum_256(double v, double *sh4) {
#pragma unroll
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    if ((threadIdx.x & 63) == 0) sh4[threadIdx.x >> 6] = v;
    __syncthreads();
    return ((sh4[0] + sh4[1]) + sh4[2]) + sh4[3];
}

// one workgroup per window: terms[w] = the window's landmark terms, thread t adds landmarks t, t + 256, ... in that order
__global__ __launch_bounds__(256) void k_terms_reduce_w(const win_desc *wd, const double *lterms, double *terms) {
    __shared__ double sh[2][4];
    const win_desc W = wd[blockIdx.x];
    double t0 = 0.0, t1 = 0.0;
    for (int l = threadIdx.x; l < W.L; l += 256) t0 += lterms[2 * (size_t) (W.lm_begin + l)], t1 += lterms[2 * (size_t) (W.lm_begin + l) + 1];
    t0 = block_sum_256(t0, sh[0]);
    t1 = block_sum_256(t1, sh[1]);
    if (threadIdx.x == 0) terms[2 * blockIdx.x] = t0, terms[2 * blockIdx.x + 1] = t1;
}

// 0.5 * sum rho(|r|^2) of the window's active factors from the resident (possibly Huber-corrected) residuals: the corrector leaves
// |r_c|^2 = rho'(s) s, i.e. s for inliers and a sqrt(s) > a^2 for outliers, so rho(s) = 2 a sqrt(s) - a^2 = 2 |r_c|^2 - a^2.
// One workgroup per window, thread t adds factors fac_begin + t, + 256, ... in that order, then the fixed tree: the value of a window does
// not depend on the batch it is evaluated in.
__global__ __launch_bounds__(256) void k_reproj_cost_w(const win_desc *wd, const double *r, const uint8_t *active, double huber, double *out) {
    __shared__ double sh[4];
    const win_desc W = wd[blockIdx.x];
    double acc = 0.0;
    for (int f = W.fac_begin + threadIdx.x; f < W.fac_end; f += 256) {
        if (active && !active[f]) continue;
        const double r0 = r[2 * (size_t) f], r1 = r[2 * (size_t) f + 1];
        double q = r0 * r0 + r1 * r1;
        if (huber > 0.0 && q > huber * huber) q = 2.0 * q - huber * huber;
        acc += 0.5 * q;
    }
    acc = block_sum_256(acc, sh);
    if (threadIdx.x == 0) out[blockIdx.x] = acc;
}

// h_ll of every landmark (global landmark order of the partition) from the systems left resident by the last assembly: the diagonal
// element (P + l, P + l) of each window's block
__global__ void k_lm_diag_w(const win_desc *wd, int P, const double *sys, double *h_ll) {
    const win_desc W = wd[blockIdx.y];
    const int l = blockIdx.x * blockDim.x + threadIdx.x;
    if (l >= W.L) return;
    const size_t N = (size_t) P + W.L;
    h_ll[W.lm_begin + l] = sys[W.sys_off + (size_t) (P + l) * N + P + l];
}

// The smallest of those diagonals per window, the value of the batched M3's first guard (host/lm_min_rule.h: the host loop's result as a
// value), so that one double per window comes back instead of one per landmark.  One wave per window: lane t takes landmarks t, t + 64, ...
// (a window of 300 makes five passes), the lanes are joined by the xor butterfly; a window without landmarks gives 0.0.
// grid (W), block 64
__global__ __launch_bounds__(64) void k_lm_min_w(const win_desc *wd, int P, const double *sys, double *min_hll) {
    const win_desc W = wd[blockIdx.x];
    const int t      = threadIdx.x;
    const size_t N   = (size_t) P + W.L;
    const double *d  = sys + W.sys_off + (size_t) P * N + P; // (P + l, P + l) is d[l (N + 1)]
    double m = icg_lm_min::start();
    for (int l = t; l < W.L; l += icg_lm_min::kLanes) m = icg_lm_min::take(m, d[(size_t) l * (N + 1)]);
#pragma unroll
    for (int k = icg_lm_min::kLanes / 2; k >= 1; k >>= 1) m = icg_lm_min::take(m, __shfl_xor(m, k, icg_lm_min::kLanes));
    if (t == 0) min_hll[blockIdx.x] = W.L > 0 ? icg_lm_min::finish(d[0], m) : 0.0;
}

// Window w's block of d_sys at width P: H (N x N, N = P + L_w) | b (N) | inv (L_w).  Returns the doubles the partition's systems take; off
// (if given) receives the W + 1 block offsets.
static size_t sys_layout(const icg_partition &pt, int P, std::vector<int64_t> *off) {
    if (off) off->assign((size_t) pt.W + 1, 0);
    int64_t total = 0;
    for (int w = 0; w < pt.W; w++) {
        const int64_t N = P + (pt.lm_off[(size_t) w + 1] - pt.lm_off[(size_t) w]);
        total += N * N + N + (N - P);
        if (off) (*off)[(size_t) w + 1] = total;
    }
    return (size_t) total;
}

// staging arena of one Schur call: descriptors, column owners and blocks, the active flags, and per window s, diag, cost and (unless the
// reduced systems stay on the device) S
static size_t schur_arena_bytes(int W, int P, int n, size_t n_owner, size_t n_blocks, bool S_staged) {
    return sizeof(win_desc) * (size_t) W + sizeof(int16_t) * n_owner + sizeof(int32_t) * n_blocks + (size_t) n +
           sizeof(double) * ((size_t) W * ((S_staged ? (size_t) P * P : 0) + 2 * (size_t) P + 1)) + 8192;
}

// d_sys for `doubles` of systems (+ 25 % when it grows); a replaced buffer holds nobody's system
static int ensure_sys_capacity(icg_ctx *ctx, size_t doubles) {
    bool replaced = false;
    const int rc  = icg_grow(ctx, (void **) &ctx->d_sys, &ctx->sys_cap, sizeof(double) * doubles, sizeof(double) * (doubles + doubles / 4), &replaced);
    if (replaced) ctx->part_1.sys_valid = ctx->part_w.sys_valid = 0;
    return rc;
}

// a device buffer of the reduced camera solve (d_red_S, d_red_H): grown without keeping its contents
// (growing d_red_S alone would leave the host parts in d_red_H intact; they are dropped all the same, one rule for both buffers — the host
// layer ships a window's part again with its next re-linearization, and a caller that solves before that gets A = S + dd, as documented)
int icg_red_ensure_capacity(icg_ctx *ctx, double **buf, size_t *cap, size_t bytes) {
    bool replaced = false;
    const int rc  = icg_grow(ctx, (void **) buf, cap, bytes, bytes, &replaced);
    if (replaced) {
        ctx->red_W = 0;
        icg_red_drop_host_parts(ctx, ctx->red_H_cols.size());
    }
    return rc;
}

static std::vector<win_desc> build_win_desc(const icg_partition &pt, const uint8_t *reassemble, const double *damp) {
    const int W = pt.W;
    std::vector<win_desc> out((size_t) W);
    for (int w = 0; w < W; w++) {
        win_desc &d = out[(size_t) w];
        d.fac_begin = pt.fac_off[(size_t) w], d.fac_end = pt.fac_off[(size_t) w + 1];
        d.lm_begin = pt.lm_off[(size_t) w], d.L = pt.lm_off[(size_t) w + 1] - pt.lm_off[(size_t) w];
        d.sys_off    = pt.sys_off.size() == (size_t) W + 1 ? pt.sys_off[(size_t) w] : 0;
        d.K          = pt.plan_valid ? pt.plan.pose_off[(size_t) w + 1] - pt.plan.pose_off[(size_t) w] : 0;
        d.reassemble = reassemble ? reassemble[w] : 1;
        d.damp       = damp ? damp[w] : (pt.damp.size() == (size_t) W ? pt.damp[(size_t) w] : 0.0);
        d.NB = d.pad = 0;
    }
    return out;
}

// Assembly (for the windows with reassemble[w] != 0) + landmark elimination of every window of the partition.
// S_view != nullptr: the reduced systems are written by the reduction kernel straight into the context's pinned staging memory (zero-copy)
// and *S_view points there — no device-to-host copy and no 9 MB copy-out per LM step at 256 windows; valid until the next call on ctx.
static int schur_impl(icg_ctx *ctx, icg_partition &pt, int P, const int32_t *col_pose, const int32_t *col_ext, const int32_t *col_td, const uint8_t *active,
                      const uint8_t *reassemble, const double *damp, double min_diag, double max_diag, double *S, const double **S_view,
                      double *s, double *diag_cc, double *cost, bool S_resident = false) {
    const bool tdbg = getenv("ICG_ABI_DEBUG") != nullptr;
    auto tnow       = [] { return std::chrono::steady_clock::now(); };
    auto t_begin    = tnow();
    const int W = pt.W, n = ctx->n_factors_resident;
    bool any_new = false;
    for (int w = 0; w < W; w++) any_new |= reassemble[w] != 0;
    if (any_new && (!ctx->rJ_valid || !ctx->rJ_has_jac)) return icg_fail(ctx, ICG_ERR_INVALID, "no resident Jacobians: evaluate with want_jac first");
    ICG_HIP(ctx, hipSetDevice(ctx->cfg.device));
    if (P > 512) return icg_fail(ctx, ICG_ERR_CAPACITY, "reduced systems of more than 512 camera columns are not supported (%d)", P);
    const int TQ = (P + 3) / 4, NT = TQ * (TQ + 1) / 2;
    const int red_LT     = std::max(1, std::min(SCH_LT, (256 * SCH_PRE) / (4 * TQ)));
    const size_t red_lds = sizeof(double) * ((size_t) red_LT * 4 * TQ + 2 * (size_t) red_LT); // <= 24.5 KB
    static icg_lds_grant red_granted;
    if (int rca = icg_allow_lds(ctx, reinterpret_cast<const void *>(k_schur_reduce_w), red_lds, icg_lds_limit(ctx) - 256, red_granted)) return rca; // (- the kernels' few static words)
    // system layout
    if (!pt.sys_valid || pt.sys_P != P) {
        for (int w = 0; w < W; w++)
            if (!reassemble[w]) return icg_fail(ctx, ICG_ERR_INVALID, "window %d: nothing resident of size %d to re-damp", w, P);
        sys_layout(pt, P, &pt.sys_off);
        pt.damp.assign((size_t) W, 0.0);
    }
    int rc = ensure_sys_capacity(ctx, (size_t) pt.sys_off[(size_t) W] + 8);
    if (rc) return rc;
    if (S_resident) {
        // the third destination: the lower tiles stay in a buffer of the context for icg_reproj_solve_windows
        if (ctx->red_W != W || ctx->red_P != P) {
            ctx->red_W = 0;
            icg_red_drop_host_parts(ctx, (size_t) W); // (host parts of another shape are not this partition's)
        }
        if ((rc = icg_red_ensure_capacity(ctx, &ctx->d_red_S, &ctx->red_S_cap, sizeof(double) * (size_t) W * P * P))) return rc;
        if ((rc = icg_red_ensure_capacity(ctx, &ctx->d_red_H, &ctx->red_H_cap, sizeof(double) * (size_t) W * ((size_t) P * (P + 1) / 2)))) return rc;
    }
    icg_partition &other = &pt == &ctx->part_1 ? ctx->part_w : ctx->part_1;
    other.sys_valid      = 0; // (d_sys is shared: whatever the other partition left there is overwritten)
    pt.sys_valid         = 0;
    ctx->red_S_valid     = false; // (d_red_S was reduced from the d_sys that is rewritten now; the host parts stay)
    std::vector<win_desc> wd = build_win_desc(pt, reassemble, damp);
    icg_asm_columns cols;
    if ((rc = icg_asm_columns_build(ctx, pt, P, col_pose, col_ext, col_td, wd, cols))) return rc;
    pt.damp.assign(damp, damp + W);
    icg_call c(ctx);
    if ((rc = c.reserve(schur_arena_bytes(W, P, n, cols.owner.size(), cols.blocks.size(), !S_resident)))) return rc;
    const win_desc *d_wd = c.in(wd.data(), (size_t) W);
    const int16_t *d_own = c.in(cols.owner.data(), cols.owner.size());
    const int32_t *d_blk = c.in(cols.blocks.data(), cols.blocks.size());
    const uint8_t *d_act = active ? c.in(active, (size_t) n) : nullptr;
    auto t_prep = tnow();
    if ((rc = c.seal())) return rc;
    // (the zero-copy region is allocated LAST: finish() copies ONE device range back that spans all mirrored outputs, and must not run
    // over memory the kernel wrote through the host mapping)
    double *d_cost = c.out(any_new ? cost : (double *) nullptr, (size_t) W);
    double *d_S    = S_resident ? ctx->d_red_S : S_view ? nullptr : c.out(S, (size_t) W * P * P);
    double *d_s    = c.out(s, (size_t) W * P);
    double *d_dg   = c.out(diag_cc, (size_t) W * P); // user pointer may be null: still a valid device scratch
    if (S_view) {
        d_S     = c.out_zc((double *) nullptr, (size_t) W * P * P);
        *S_view = d_S;
    }
    ICG_LAUNCH_GUARD(c);
    if (any_new) icg_asm_enqueue(ctx, pt, P, cols.NBmax, d_wd, d_own, d_blk, d_act);
    {
        icg_prof_scope ps(ctx, "schur_reduce");
        const int Lmax = icg_partition_Lmax(pt);
        hipLaunchKernelGGL(k_schur_inv_w, dim3((Lmax + 255) / 256, W), dim3(256), 0, ctx->stream, d_wd, P, ctx->d_sys, min_diag, max_diag);
        hipLaunchKernelGGL(k_schur_reduce_w, dim3((unsigned) ((NT + 255) / 256), W), dim3(256), red_lds, ctx->stream, d_wd, P, red_LT, (const double *) ctx->d_sys, d_S, d_s,
                           d_dg, S_view || S_resident ? 1 : 0);
        // the cost belongs to the linearization point: only meaningful while the resident residuals are the ones assembled
        if (any_new) hipLaunchKernelGGL(k_reproj_cost_w, dim3(W), dim3(256), 0, ctx->stream, d_wd, (const double *) ctx->d_rJ, d_act, ctx->last_huber, d_cost);
    }
    ICG_HIP(ctx, hipGetLastError());
    auto t_launch = tnow();
    if (tdbg) (void) hipStreamSynchronize(ctx->stream);
    auto t_kernels = tnow();
    if ((rc = c.finish())) return rc;
    if (tdbg) {
        auto ms = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
        fprintf(stderr, "[icg_reproj_schur] W=%d: host prep %.3f, h2d+launch %.3f, kernels %.3f, d2h+copy-out %.3f ms\n", W, ms(t_begin, t_prep),
                ms(t_prep, t_launch), ms(t_launch, t_kernels), ms(t_kernels, tnow()));
    }
    pt.sys_P = P, pt.sys_valid = 1;
    ctx->sys_min_diag = min_diag, ctx->sys_max_diag = max_diag;
    if (S_resident) ctx->red_W = W, ctx->red_P = P, ctx->red_S_valid = true, ctx->hp.H_P = P;
    return ICG_OK;
}

// landmark steps and their terms of the LM model decrease from the delta_c on the device (d_lt: 2 x n_lm doubles of working memory)
static void backsub_enqueue(icg_ctx *ctx, const icg_partition &pt, int P, const win_desc *d_wd, const double *d_dc, double *d_dl, double *d_lt, double *d_tm) {
    const int W = pt.W, n_lm = pt.lm_off[(size_t) W];
    icg_prof_scope ps(ctx, "schur_backsub");
    hipLaunchKernelGGL(k_schur_backsub_w, dim3(n_lm), dim3(64), 0, ctx->stream, d_wd, W > 1 ? (const int32_t *) ctx->d_lmwin : (const int32_t *) nullptr, 0, P,
                       (const double *) ctx->d_sys, d_dc, d_dl, d_lt, ctx->sys_min_diag, ctx->sys_max_diag);
    hipLaunchKernelGGL(k_terms_reduce_w, dim3(W), dim3(256), 0, ctx->stream, d_wd, (const double *) d_lt, d_tm);
}

static int backsub_impl(icg_ctx *ctx, icg_partition &pt, int P, const double *delta_c, double *delta_l, double *lm_terms) {
    const int W = pt.W, n_lm = pt.lm_off[(size_t) W];
    if (n_lm == 0) return ICG_OK;
    ICG_HIP(ctx, hipSetDevice(ctx->cfg.device));
    const std::vector<win_desc> wd = build_win_desc(pt, nullptr, nullptr);
    icg_call c(ctx);
    int rc = c.reserve(sizeof(win_desc) * (size_t) W + sizeof(double) * ((size_t) W * P + 3 * (size_t) n_lm + 2 * (size_t) W) + 4096);
    if (rc) return rc;
    const win_desc *d_wd = c.in(wd.data(), (size_t) W);
    const double *d_dc   = c.in(delta_c, (size_t) W * P);
    if ((rc = c.seal())) return rc;
    double *d_dl = c.out(delta_l, (size_t) n_lm);
    double *d_tm = c.out(lm_terms, 2 * (size_t) W);
    double *d_lt = c.out((double *) nullptr, 2 * (size_t) n_lm);
    ICG_LAUNCH_GUARD(c);
    backsub_enqueue(ctx, pt, P, d_wd, d_dc, d_dl, d_lt, d_tm);
    ICG_HIP(ctx, hipGetLastError());
    return c.finish();
}

static int cost_impl(icg_ctx *ctx, icg_partition &pt, const uint8_t *active, double *cost) {
    const int W = pt.W, n = ctx->n_factors_resident;
    ICG_HIP(ctx, hipSetDevice(ctx->cfg.device));
    const std::vector<win_desc> wd = build_win_desc(pt, nullptr, nullptr);
    icg_call c(ctx);
    int rc = c.reserve(sizeof(win_desc) * (size_t) W + (size_t) n + sizeof(double) * (size_t) W + 4096);
    if (rc) return rc;
    const win_desc *d_wd = c.in(wd.data(), (size_t) W);
    const uint8_t *d_act = active ? c.in(active, (size_t) n) : nullptr;
    if ((rc = c.seal())) return rc;
    double *d_cost = c.out(cost, (size_t) W);
    ICG_LAUNCH_GUARD(c);
    {
        icg_prof_scope ps(ctx, "reproj_cost");
        hipLaunchKernelGGL(k_reproj_cost_w, dim3(W), dim3(256), 0, ctx->stream, d_wd, (const double *) ctx->d_rJ, d_act, ctx->last_huber, d_cost);
    }
    ICG_HIP(ctx, hipGetLastError());
    return c.finish();
}

static int landmark_diag_impl(icg_ctx *ctx, icg_partition &pt, double *h_ll) {
    const int W = pt.W, P = pt.sys_P, n_lm = pt.lm_off[(size_t) W];
    if (n_lm == 0) return ICG_OK;
    ICG_HIP(ctx, hipSetDevice(ctx->cfg.device));
    const std::vector<win_desc> wd = build_win_desc(pt, nullptr, nullptr);
    const int Lmax = icg_partition_Lmax(pt);
    icg_call c(ctx);
    int rc = c.reserve(sizeof(win_desc) * (size_t) W + sizeof(double) * (size_t) n_lm + 4096);
    if (rc) return rc;
    const win_desc *d_wd = c.in(wd.data(), (size_t) W);
    if ((rc = c.seal())) return rc;
    double *d_out = c.out(h_ll, (size_t) n_lm);
    ICG_LAUNCH_GUARD(c);
    {
        icg_prof_scope ps(ctx, "schur_reduce");
        hipLaunchKernelGGL(k_lm_diag_w, dim3((Lmax + 255) / 256, W), dim3(256), 0, ctx->stream, d_wd, P, (const double *) ctx->d_sys, d_out);
    }
    ICG_HIP(ctx, hipGetLastError());
    return c.finish();
}

static int landmark_min_impl(icg_ctx *ctx, icg_partition &pt, double *min_hll) {
    const int W = pt.W, P = pt.sys_P;
    if (pt.lm_off[(size_t) W] == 0) { // (no landmark anywhere: nothing to read on the device)
        std::fill(min_hll, min_hll + W, 0.0);
        return ICG_OK;
    }
    ICG_HIP(ctx, hipSetDevice(ctx->cfg.device));
    const std::vector<win_desc> wd = build_win_desc(pt, nullptr, nullptr);
    icg_call c(ctx);
    int rc = c.reserve((sizeof(win_desc) + sizeof(double)) * (size_t) W + 4096);
    if (rc) return rc;
    const win_desc *d_wd = c.in(wd.data(), (size_t) W);
    if ((rc = c.seal())) return rc;
    double *d_out = c.out(min_hll, (size_t) W);
    ICG_LAUNCH_GUARD(c);
    {
        icg_prof_scope ps(ctx, "lm_min");
        hipLaunchKernelGGL(k_lm_min_w, dim3(W), dim3(icg_lm_min::kLanes), 0, ctx->stream, d_wd, P, (const double *) ctx->d_sys, d_out);
    }
    ICG_HIP(ctx, hipGetLastError());
    return c.finish();
}

// ---- single window: every resident factor ----------------------------------------------------------------------------------------------
extern "C" int icg_reproj_schur(icg_ctx *ctx, int P, const int32_t *col_pose, int32_t col_ext, int32_t col_td, const uint8_t *active,
                                int reassemble, double damp, double min_diag, double max_diag, double *S, double *s, double *diag_cc,
                                double *cost) {
    if (!ctx || P <= 0 || !col_pose || !S || !s) return ICG_ERR_INVALID;
    if (ctx->n_factors_resident == 0) return icg_fail(ctx, ICG_ERR_INVALID, "no resident factors");
    if (reassemble && (!ctx->rJ_valid || !ctx->rJ_has_jac))
        return icg_fail(ctx, ICG_ERR_INVALID, "no resident Jacobians: call icg_reproj_eval_resident with want_jac first");
    if (!reassemble && (!ctx->part_1.sys_valid || ctx->part_1.sys_P != P))
        return icg_fail(ctx, ICG_ERR_INVALID, "no resident normal equations of size %d to re-damp", P);
    int rc = icg_asm_single_partition(ctx, ctx->last_n_lm);
    if (rc) return rc;
    const uint8_t re = reassemble ? 1 : 0;
    return schur_impl(ctx, ctx->part_1, P, col_pose, &col_ext, &col_td, active, &re, &damp, min_diag, max_diag, S, nullptr, s, diag_cc,
                      reassemble ? cost : nullptr);
}

extern "C" int icg_reproj_landmark_diag(icg_ctx *ctx, double *h_ll) {
    if (!ctx || !h_ll) return ICG_ERR_INVALID;
    if (!ctx->part_1.sys_valid) return icg_fail(ctx, ICG_ERR_INVALID, "no resident Schur system: call icg_reproj_schur first");
    return landmark_diag_impl(ctx, ctx->part_1, h_ll);
}

extern "C" int icg_reproj_backsub(icg_ctx *ctx, int P, const double *delta_c, double *delta_l, double *lm_terms) {
    if (!ctx || !delta_c || !delta_l) return ICG_ERR_INVALID;
    if (!ctx->part_1.sys_valid || ctx->part_1.sys_P != P) return icg_fail(ctx, ICG_ERR_INVALID, "no resident Schur system of size %d: call icg_reproj_schur first", P);
    return backsub_impl(ctx, ctx->part_1, P, delta_c, delta_l, lm_terms);
}

extern "C" int icg_reproj_cost(icg_ctx *ctx, const uint8_t *active, double *cost) {
    if (!ctx || !cost) return ICG_ERR_INVALID;
    if (!ctx->rJ_valid) return icg_fail(ctx, ICG_ERR_INVALID, "no resident residuals: call icg_reproj_eval_resident first");
    *cost = 0.0;
    if (ctx->n_factors_resident == 0) return ICG_OK;
    // (the cost needs the factor range only: a one-window descriptor without a plan)
    icg_partition &pt = ctx->part_1;
    if (pt.W != 1 || pt.fac_off.size() != 2 || pt.fac_off[1] != ctx->n_factors_resident) {
        pt.W = 1, pt.fac_off = {0, ctx->n_factors_resident}, pt.lm_off = {0, ctx->last_n_lm};
        pt.plan_valid = false, pt.sys_valid = 0;
    }
    return cost_impl(ctx, pt, active, cost);
}

// M2 for a caller-defined dense layout (MarginalizationInfo::constructEquation, factors/marginalization_info.h:195-230): the system is
// assembled in the compact layout above (free poses in pose order, then extrinsic, then td; landmark l in row V + l) by the same kernels
// and spread into the caller's local_size x local_size matrix on the host — every cell has one source, no sum is formed there.
extern "C" int icg_reproj_accumulate_normal(icg_ctx *ctx, int local_size, const int32_t *col_pose, int32_t col_ext,
                                            const int32_t *col_lm, int32_t col_td, double *H0, double *b0) {
    if (!ctx || local_size <= 0 || !col_pose || !col_lm || !H0 || !b0) return ICG_ERR_INVALID;
    if (!ctx->rJ_valid || !ctx->rJ_has_jac) return icg_fail(ctx, ICG_ERR_INVALID, "no resident Jacobians: call icg_reproj_eval_* with want_jac first");
    const int n = ctx->n_factors_resident, L = ctx->last_n_lm;
    if (n == 0) return ICG_OK;
    auto inside = [&](int col, int width) { return col < 0 || col + width <= local_size; };
    std::vector<int32_t> vcol((size_t) ctx->last_n_poses, -1), vmap;
    for (int k = 0; k < ctx->last_n_poses; k++)
        if (col_pose[k] >= 0) {
            if (!inside(col_pose[k], 6)) return icg_fail(ctx, ICG_ERR_INVALID, "pose %d: column %d outside the system (%d)", k, col_pose[k], local_size);
            vcol[(size_t) k] = (int32_t) vmap.size();
            for (int x = 0; x < 6; x++) vmap.push_back(col_pose[k] + x);
        }
    if (!inside(col_ext, 6) || !inside(col_td, 1)) return icg_fail(ctx, ICG_ERR_INVALID, "ext/td column outside the system (%d)", local_size);
    int vext = -1, vtd = -1;
    if (col_ext >= 0) {
        vext = (int) vmap.size();
        for (int x = 0; x < 6; x++) vmap.push_back(col_ext + x);
    }
    if (col_td >= 0) vtd = (int) vmap.size(), vmap.push_back(col_td);
    for (int l = 0; l < L; l++)
        if (!inside(col_lm[l], 1)) return icg_fail(ctx, ICG_ERR_INVALID, "landmark %d: column %d outside the system (%d)", l, col_lm[l], local_size);
    const int V = std::max(1, (int) vmap.size());
    int rc = icg_asm_single_partition(ctx, L);
    if (rc) return rc;
    const size_t N = (size_t) V + L;
    std::vector<double> S((size_t) V * V), s((size_t) V), sys(N * N + N);
    const uint8_t re  = 1;
    const double zero = 0.0;
    if ((rc = schur_impl(ctx, ctx->part_1, V, vcol.data(), &vext, &vtd, nullptr, &re, &zero, 0.0, 0.0, S.data(), nullptr, s.data(), nullptr, nullptr))) return rc;
    ICG_HIP(ctx, hipMemcpyAsync(sys.data(), ctx->d_sys, sizeof(double) * (N * N + N), hipMemcpyDeviceToHost, ctx->stream));
    if ((rc = icg_stream_wait(ctx))) return rc;
    ctx->part_1.sys_valid = 0; // (a by-product: not a system the Schur entry points may re-damp)
    const size_t LS = (size_t) local_size;
    const double *H = sys.data(), *b = H + N * N;
    for (size_t a = 0; a < vmap.size(); a++) {
        for (size_t c = 0; c < vmap.size(); c++) H0[(size_t) vmap[a] * LS + (size_t) vmap[c]] += H[a * N + c];
        b0[(size_t) vmap[a]] += b[a];
    }
    for (int l = 0; l < L; l++) {
        if (col_lm[l] < 0) continue;
        const size_t cl = (size_t) col_lm[l], row = ((size_t) V + (size_t) l) * N;
        for (size_t a = 0; a < vmap.size(); a++) {
            H0[cl * LS + (size_t) vmap[a]] += H[row + a];
            H0[(size_t) vmap[a] * LS + cl] += H[row + a];
        }
        H0[cl * LS + cl] += H[row + (size_t) V + (size_t) l];
        b0[cl] += b[(size_t) V + (size_t) l];
    }
    return ICG_OK;
}

static int windows_args_ok(icg_ctx *ctx, int P, const int32_t *col_pose, const int32_t *col_ext, const int32_t *col_td, const uint8_t *reassemble,
                           const double *damp, double *s) {
    if (!ctx || P <= 0 || !col_pose || !col_ext || !col_td || !reassemble || !damp || !s) return ICG_ERR_INVALID;
    if (ctx->part_w.W <= 0 || !ctx->part_w.plan_valid) return icg_fail(ctx, ICG_ERR_INVALID, "no window partition: call icg_reproj_set_windows first");
    return ICG_OK;
}

// Problem-setup companion of the batched calls: sizes the resident window systems (W x ((P + L_w)^2 + ...) doubles of device memory) and the
// staging arena of the largest per-step call for reduced systems of size P, so that the first LM step of a solve does not pay a device
// allocation and a pinned re-allocation (4 ms at 256 C2 windows).  A hint: the calls themselves still grow what they need.
extern "C" int icg_reproj_reserve_windows(icg_ctx *ctx, int P) {
    if (!ctx || P <= 0) return ICG_ERR_INVALID;
    const icg_partition &pt = ctx->part_w;
    const int W = pt.W, n = ctx->n_factors_resident;
    if (W <= 0) return icg_fail(ctx, ICG_ERR_INVALID, "no window partition: call icg_reproj_set_windows first");
    ICG_HIP(ctx, hipSetDevice(ctx->cfg.device));
    int rc = ensure_sys_capacity(ctx, sys_layout(pt, P, nullptr) + 8);
    if (rc) return rc;
    icg_call c(ctx);
    return c.reserve(schur_arena_bytes(W, P, n, (size_t) W * P, (size_t) W * P, true)); // (a hint: about one column block per column at the most)
}

extern "C" int icg_reproj_schur_windows(icg_ctx *ctx, int P, const int32_t *col_pose, const int32_t *col_ext, const int32_t *col_td,
                                        const uint8_t *active, const uint8_t *reassemble, const double *damp, double min_diag, double max_diag,
                                        double *S, double *s, double *diag_cc, double *cost) {
    if (!S) return ICG_ERR_INVALID;
    if (int rc = windows_args_ok(ctx, P, col_pose, col_ext, col_td, reassemble, damp, s)) return rc;
    return schur_impl(ctx, ctx->part_w, P, col_pose, col_ext, col_td, active, reassemble, damp, min_diag, max_diag, S, nullptr, s, diag_cc, cost);
}

extern "C" int icg_reproj_schur_windows_view(icg_ctx *ctx, int P, const int32_t *col_pose, const int32_t *col_ext, const int32_t *col_td,
                                             const uint8_t *active, const uint8_t *reassemble, const double *damp, double min_diag,
                                             double max_diag, const double **S_view, double *s, double *diag_cc, double *cost) {
    if (!S_view) return ICG_ERR_INVALID;
    if (int rc = windows_args_ok(ctx, P, col_pose, col_ext, col_td, reassemble, damp, s)) return rc;
    return schur_impl(ctx, ctx->part_w, P, col_pose, col_ext, col_td, active, reassemble, damp, min_diag, max_diag, nullptr, S_view, s, diag_cc, cost);
}

extern "C" int icg_reproj_schur_windows_resident(icg_ctx *ctx, int P, const int32_t *col_pose, const int32_t *col_ext, const int32_t *col_td,
                                                 const uint8_t *active, const uint8_t *reassemble, const double *damp, double min_diag,
                                                 double max_diag, double *s, double *diag_cc, double *cost) {
    if (int rc = windows_args_ok(ctx, P, col_pose, col_ext, col_td, reassemble, damp, s)) return rc;
    return schur_impl(ctx, ctx->part_w, P, col_pose, col_ext, col_td, active, reassemble, damp, min_diag, max_diag, nullptr, nullptr, s, diag_cc, cost, true);
}

// The reduced camera solve of every window (k_chol_solve, chol.hip: one wave per window, the host's arithmetic bit for bit) and the landmark
// back-substitution on the delta_c it leaves on the device: the two host phases "reduced solve" and "back-substitution" of an LM step as one
// call.  Up: dd and rhs (2 W P doubles) and the host parts that changed; down: delta_c, status, delta_l, lm_terms.
extern "C" int icg_reproj_solve_windows(icg_ctx *ctx, int P, const int32_t *Pw, const uint8_t *solve, const uint8_t *host_part_new, const double *host_S,
                                        const double *dd, const double *rhs, double *delta_c, int32_t *status, double *delta_l, double *lm_terms) {
    if (!ctx) return ICG_ERR_INVALID;
    if (P <= 0 || !Pw || !solve || !dd || !rhs || !delta_c) return icg_fail(ctx, ICG_ERR_INVALID, "icg_reproj_solve_windows: invalid argument");
    icg_partition &pt = ctx->part_w;
    const int W       = pt.W;
    if (W <= 0 || !ctx->red_S_valid || ctx->red_W != W || ctx->red_P != P || !pt.sys_valid || pt.sys_P != P)
        return icg_fail(ctx, ICG_ERR_INVALID, "no resident reduced systems of size %d: call icg_reproj_schur_windows_resident first", P);
    const size_t slot = (size_t) P * (P + 1) / 2;
    std::vector<icg_chol_desc> desc((size_t) W);
    std::vector<int32_t> new_cols(ctx->red_H_cols);
    size_t t_new = 0;
    for (int w = 0; w < W; w++) {
        const bool is_new = host_part_new && host_part_new[w];
        if ((solve[w] || is_new) && (Pw[w] <= 0 || Pw[w] > P))
            return icg_fail(ctx, ICG_ERR_INVALID, "icg_reproj_solve_windows: window %d: Pw = %d (1 .. %d)", w, Pw[w], P);
        if (is_new && !host_S) return icg_fail(ctx, ICG_ERR_INVALID, "icg_reproj_solve_windows: window %d: host_part_new without host_S", w);
        int flags = solve[w] ? ICG_CHOL_SOLVE : 0;
        if (is_new) {
            flags |= ICG_CHOL_PART_NEW;
            new_cols[(size_t) w] = Pw[w];
        } else if (solve[w] && new_cols[(size_t) w] != 0) {
            if (new_cols[(size_t) w] != Pw[w])
                return icg_fail(ctx, ICG_ERR_INVALID, "icg_reproj_solve_windows: window %d: the resident host part has %d columns, not %d", w,
                                new_cols[(size_t) w], Pw[w]);
            flags |= ICG_CHOL_PART;
        }
        const int nw    = solve[w] || is_new ? Pw[w] : 1;
        desc[(size_t) w] = {nw, P, P, flags, (int64_t) w * P * P, (int64_t) (w * slot), (int64_t) t_new, (int64_t) w * P, (int64_t) w * P, (int64_t) w * P, -1, 0};
        if (is_new) t_new += (size_t) Pw[w] * (Pw[w] + 1) / 2;
    }
    ICG_HIP(ctx, hipSetDevice(ctx->cfg.device));
    icg_chol_plan plan;
    int rc = icg_chol_plan_build(ctx, desc, plan);
    if (rc) return rc;
    const int n_lm = pt.lm_off[(size_t) W];
    const std::vector<win_desc> wd = build_win_desc(pt, nullptr, nullptr);
    icg_call c(ctx);
    if ((rc = c.reserve((sizeof(win_desc) + sizeof(icg_chol_desc) + 8) * (size_t) W + sizeof(double) * (t_new + 3 * (size_t) W * P + 3 * (size_t) n_lm + 2 * (size_t) W) +
                        16 * 256)))
        return rc;
    icg_chol_ptrs p{};
    const win_desc *d_wd        = c.in(wd.data(), (size_t) W);
    const icg_chol_desc *d_desc = c.in(desc.data(), (size_t) W);
    const int32_t *d_items      = c.in(plan.items.data(), (size_t) W);
    p.dd                        = c.in(dd, (size_t) W * P);
    p.b                         = c.in(rhs, (size_t) W * P);
    p.Hnew                      = t_new ? c.in(host_S, t_new) : nullptr;
    if ((rc = c.seal())) return rc;
    p.A      = ctx->d_red_S;
    p.H      = ctx->d_red_H;
    p.x      = c.out(delta_c, (size_t) W * P);
    p.status = c.out(status, (size_t) W); // (user pointer may be null: still a valid device scratch)
    double *d_dl = c.out(n_lm > 0 ? delta_l : (double *) nullptr, (size_t) std::max(n_lm, 1));
    double *d_tm = c.out(lm_terms, 2 * (size_t) W); // (zeros without landmarks: set below)
    double *d_lt = c.out((double *) nullptr, 2 * (size_t) std::max(n_lm, 1));
    ICG_LAUNCH_GUARD(c);
    // from here on the device copy of the flagged host parts is being replaced: a failure below leaves those windows without one
    for (int w = 0; w < W; w++)
        if (host_part_new && host_part_new[w]) ctx->red_H_cols[(size_t) w] = 0;
    if ((rc = icg_chol_enqueue(ctx, plan, d_desc, d_items, p))) return rc;
    if (n_lm > 0) {
        backsub_enqueue(ctx, pt, P, d_wd, p.x, d_dl, d_lt, d_tm);
    } else {
        ICG_HIP(ctx, hipMemsetAsync(d_tm, 0, sizeof(double) * 2 * (size_t) W, ctx->stream));
    }
    ICG_HIP(ctx, hipGetLastError());
    if ((rc = c.finish())) return rc;
    ctx->red_H_cols.swap(new_cols);
    return ICG_OK;
}

extern "C" int icg_reproj_landmark_diag_windows(icg_ctx *ctx, double *h_ll) {
    if (!ctx || !h_ll) return ICG_ERR_INVALID;
    if (!ctx->part_w.sys_valid) return icg_fail(ctx, ICG_ERR_INVALID, "no resident window systems: call icg_reproj_schur_windows first");
    return landmark_diag_impl(ctx, ctx->part_w, h_ll);
}

extern "C" int icg_reproj_landmark_min_windows(icg_ctx *ctx, double *min_hll) {
    if (!ctx || !min_hll) return ICG_ERR_INVALID;
    if (!ctx->part_w.sys_valid) return icg_fail(ctx, ICG_ERR_INVALID, "no resident window systems: call icg_reproj_schur_windows first");
    return landmark_min_impl(ctx, ctx->part_w, min_hll);
}

extern "C" int icg_reproj_backsub_windows(icg_ctx *ctx, int P, const double *delta_c, double *delta_l, double *lm_terms) {
    if (!ctx || !delta_c || !delta_l) return ICG_ERR_INVALID;
    if (!ctx->part_w.sys_valid || ctx->part_w.sys_P != P)
        return icg_fail(ctx, ICG_ERR_INVALID, "no resident window systems of size %d: call icg_reproj_schur_windows first", P);
    return backsub_impl(ctx, ctx->part_w, P, delta_c, delta_l, lm_terms);
}

extern "C" int icg_reproj_cost_windows(icg_ctx *ctx, const uint8_t *active, double *cost) {
    if (!ctx || !cost) return ICG_ERR_INVALID;
    if (!ctx->rJ_valid) return icg_fail(ctx, ICG_ERR_INVALID, "no resident residuals: call icg_reproj_eval_windows first");
    if (ctx->part_w.W <= 0) return icg_fail(ctx, ICG_ERR_INVALID, "no window partition");
    return cost_impl(ctx, ctx->part_w, active, cost);
}
