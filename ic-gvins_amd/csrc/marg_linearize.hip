// M3: the Schur step on the marginalized pose / mix block and the linearization of the reduced system (factors/marginalization_info.h:153-192)
// for many windows at once — one workgroup per window, icg_marg_linearize_batch.
//
// The eigen-solver is host/factors.cc symmetricEigen restated for a workgroup: Householder tridiagonalisation, accumulation of the
// transformations and implicit QL, in place in ONE n x n working matrix (stored transposed, W[j * n + i] = v(i, j), as the host stores it)
// with d and e beside it.  Every accumulated sum of the host code is a fixed-order chain per output element; here one thread owns a chain and
// adds its terms in the host's order, one multiply and one add per term (the file is built with -ffp-contract=off), and everything that is
// element-wise on the host (the rank-2 update, the Givens rotations) is spread over the threads.  The scalar recurrences (scale, h, the c / s
// sequence of a QL sweep) are computed by every thread redundantly from the same LDS values: uniform by construction, no broadcast needed.
// The one operation that may round differently from the host is hypot (libm there, the device library here).
//
// Working memory: a C2 window (r = 142) is 142^2 + 2 * 142 doubles = 163 584 B, which one workgroup may own on gfx950 (160 KiB of LDS per CU):
// k_marg_linearize<true>.  A window that does not fit (C4: r = 217) runs the same code on a global scratch block (L2 / Infinity Cache
// resident), d and e still in LDS: k_marg_linearize<false>.  Which of the two a window takes depends on its own (P, m) only, so its bits
// are the same alone and in any batch.
//
// icg_marg_linearize_resident is the same M3 on systems that never left the device: M2 (factors/marginalization_info.h:195-230) is the sum of
// the host-evaluated factors' J^T J and the landmark-eliminated visual part, and both halves are resident after
// icg_reproj_host_parts_build (packed lower triangle `part`, ctx->d_red_H) and icg_reproj_schur_windows_resident (lower triangle of S, row
// stride P, ctx->d_red_S).  k_marg_form_h writes, for every cell i >= j of a selected window,
//     H[i][j] = H[j][i] = part[i (i + 1) / 2 + j] + S_w[i * P + j]        (part first, then S: the host's plan.H += S; no part: +0.0 + S)
// into a buffer of the context, and k_marg_linearize (M3, :153-192) runs unchanged on that buffer.
#include "icg_internal.h"

#include <cmath>

#define LIN_THREADS 256
#define LIN_WAVES (LIN_THREADS / 64)
#define LIN_SLOTS ((ICG_MARG_LIN_MAX_P + LIN_THREADS - 1) / LIN_THREADS) // elements of a length-n vector one thread owns

namespace {

struct lin_desc {
    int32_t P, m;
    int64_t h_off, b_off; // window's H (P x P) and b (P) in the inputs
    int64_t r_off, rr_off; // window's r-vectors (bp, e0, evals) and r x r matrices (Hp, J0) in the outputs
    int64_t s_off;         // window's block in the global scratch: bp (r) | working memory (only for a window that does not fit in LDS)
};

// doubles of working memory a window needs beside d and e: phase (a) holds W (m x m), Hinv (m x m), T (r x m), phase (b) W (r x r)
__host__ __device__ static inline size_t lin_work(int m, int r) {
    const size_t a = 2 * (size_t) m * m + (size_t) r * m, b = (size_t) r * r;
    return a > b ? a : b;
}

// symmetricEigen (host/factors.cc) on W (n x n, transposed: W[j * n + i] = v(i, j); the lower triangle of the input is what is read).
// On return d holds the eigenvalues in QL order, the rows of W the eigenvectors (W[x * n + i] = component i of the vector of d[x]) and the
// memory of e the ascending order as int32: ord[k] = x of the k-th smallest eigenvalue.  Returns true when a QL sweep hit the 60-iteration
// cap.  Called by all threads of the workgroup (barriers inside); W, d, e must be visible (a barrier after they were written).
__device__ __forceinline__ bool lin_eigen(const int n, double *W, double *d, double *e, int *s_m) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    bool capped = false;
    // ---- tridiagonalise
    for (int j = tid; j < n; j += LIN_THREADS) d[j] = W[(size_t) j * n + n - 1];
    __syncthreads();
    for (int i = n - 1; i > 0; i--) {
        double scale = 0.0, h = 0.0;
        for (int k = 0; k < i; k++) scale += fabs(d[k]);
        const double dl = d[i - 1];
        __syncthreads();
        if (scale == 0.0) {
            if (tid == 0) e[i] = dl;
            for (int j = tid; j < i; j += LIN_THREADS) {
                d[j]                  = W[(size_t) j * n + i - 1];
                W[(size_t) j * n + i] = 0.0;
                W[(size_t) i * n + j] = 0.0;
            }
        } else {
            for (int k = tid; k < i; k += LIN_THREADS) d[k] = d[k] / scale;
            __syncthreads();
            for (int k = 0; k < i; k++) h += d[k] * d[k];
            const double f = d[i - 1];
            double g       = sqrt(h);
            if (f > 0) g = -g;
            h = h - f * g;
            __syncthreads();
            if (tid == 0) {
                e[i]     = scale * g;
                d[i - 1] = f - g;
            }
            __syncthreads();
            // e[j] = sum_{j' < j} v(j, j') d[j'] + v(j, j) d[j] + sum_{k > j} v(k, j) d[k]: the order in which the host's column loop adds them
            double *ci = W + (size_t) i * n;
            for (int j = tid; j < i; j += LIN_THREADS) {
                ci[j]     = d[j]; // v(j, i) = d[j]
                double s  = 0.0;
                for (int jp = 0; jp < j; jp++) s += W[(size_t) jp * n + j] * d[jp];
                const double *cj = W + (size_t) j * n;
                s += cj[j] * d[j];
                for (int k = j + 1; k < i; k++) s += cj[k] * d[k];
                e[j] = s;
            }
            __syncthreads();
            for (int j = tid; j < i; j += LIN_THREADS) e[j] = e[j] / h;
            __syncthreads();
            double f2 = 0.0;
            for (int j = 0; j < i; j++) f2 += e[j] * d[j];
            const double hh = f2 / (h + h);
            __syncthreads();
            for (int j = tid; j < i; j += LIN_THREADS) e[j] = e[j] - hh * d[j];
            __syncthreads();
            for (int jj = wave; jj < i; jj += LIN_WAVES) { // rank-2 update of the lower triangle: element-wise, a wave per column
                const double fj = d[jj], gj = e[jj];
                double *cj = W + (size_t) jj * n;
                for (int k = jj + lane; k < i; k += 64) cj[k] = cj[k] - (fj * e[k] + gj * d[k]);
            }
            __syncthreads();
            for (int jj = tid; jj < i; jj += LIN_THREADS) {
                d[jj]                  = W[(size_t) jj * n + i - 1];
                W[(size_t) jj * n + i] = 0.0;
            }
        }
        if (tid == 0) d[i] = h;
        __syncthreads();
    }
    // ---- accumulate the transformations
    for (int i = 0; i < n - 1; i++) {
        const double h = d[i + 1];
        if (tid == 0) {
            W[(size_t) i * n + n - 1] = W[(size_t) i * n + i];
            W[(size_t) i * n + i]     = 1.0;
        }
        __syncthreads();
        double *u = W + (size_t) (i + 1) * n;
        if (h != 0.0) {
            for (int k = tid; k <= i; k += LIN_THREADS) d[k] = u[k] / h;
            __syncthreads();
            for (int j = tid; j <= i; j += LIN_THREADS) {
                double *cj = W + (size_t) j * n;
                double g   = 0.0;
                for (int k = 0; k <= i; k++) g += u[k] * cj[k];
                for (int k = 0; k <= i; k++) cj[k] = cj[k] - g * d[k];
            }
            __syncthreads();
        }
        for (int k = tid; k <= i; k += LIN_THREADS) u[k] = 0.0;
        __syncthreads();
    }
    for (int j = tid; j < n; j += LIN_THREADS) {
        d[j]                      = W[(size_t) j * n + n - 1];
        W[(size_t) j * n + n - 1] = 0.0;
    }
    double shifted[LIN_SLOTS];
#pragma unroll
    for (int q = 0; q < LIN_SLOTS; q++) {
        const int k = tid + q * LIN_THREADS;
        shifted[q]  = k + 1 < n ? e[k + 1] : 0.0;
    }
    __syncthreads();
    if (tid == 0) W[(size_t) (n - 1) * n + n - 1] = 1.0;
#pragma unroll
    for (int q = 0; q < LIN_SLOTS; q++) {
        const int k = tid + q * LIN_THREADS;
        if (k < n) e[k] = shifted[q];
    }
    __syncthreads();
    // ---- implicit QL.  A sweep's c / s recurrence is computed by every thread that owns an eigenvector component; the thread applies each
    // rotation to its component as it goes (the rotations of a sweep chain along the columns, not across components).  d and e are only read
    // during a sweep: the new values are kept in the registers of one owner thread each and written behind a barrier.
    double f = 0.0, tst1 = 0.0;
    const double eps = 2.220446049250313e-16;
    for (int l = 0; l < n; l++) {
        {
            const double t = fabs(d[l]) + fabs(e[l]);
            if (tst1 < t) tst1 = t;
        }
        if (tid == 0) *s_m = n - 1; // (e[n - 1] = 0 ends the host's search there at the latest)
        __syncthreads();
        for (int mm = l + tid; mm < n - 1; mm += LIN_THREADS)
            if (fabs(e[mm]) <= eps * tst1) {
                atomicMin(s_m, mm);
                break;
            }
        __syncthreads();
        const int m = *s_m;
        if (m > l) {
            int iter = 0;
            bool more;
            do {
                iter++;
                double g        = d[l];
                const double el = e[l], el1 = e[l + 1];
                double p        = (d[l + 1] - g) / (2.0 * el);
                double r        = hypot(p, 1.0);
                if (p < 0) r = -r;
                const double dl0 = el / (p + r), dl1 = el * (p + r);
                double h         = g - dl0;
                __syncthreads();
                if (tid == 0) d[l] = dl0, d[l + 1] = dl1;
                for (int i = l + 2 + tid; i < n; i += LIN_THREADS) d[i] = d[i] - h;
                __syncthreads();
                f += h;
                double keep_d[LIN_SLOTS], keep_e[LIN_SLOTS], new_dl = 0.0, new_el = 0.0;
                if (tid < n) {
                    p        = d[m];
                    double c = 1.0, c2 = c, c3 = c, s = 0.0, s2 = 0.0;
                    double cur[LIN_SLOTS];
#pragma unroll
                    for (int q = 0; q < LIN_SLOTS; q++) {
                        const int k = tid + q * LIN_THREADS;
                        cur[q]      = k < n ? W[(size_t) m * n + k] : 0.0;
                        keep_d[q] = keep_e[q] = 0.0;
                    }
                    for (int i = m - 1; i >= l; i--) {
                        c3 = c2;
                        c2 = c;
                        s2 = s;
                        const double ei = e[i], di = d[i];
                        g               = c * ei;
                        h               = c * p;
                        r               = hypot(p, ei);
                        const double en = s * r; // e[i + 1]
                        s               = ei / r;
                        c               = p / r;
                        p               = c * di - s * g;
                        const double dn = h + s * (c * g + s * di); // d[i + 1]
#pragma unroll
                        for (int q = 0; q < LIN_SLOTS; q++) {
                            const int k = tid + q * LIN_THREADS;
                            if (k == i + 1) keep_d[q] = dn, keep_e[q] = en;
                            if (k < n) {
                                const double a = W[(size_t) i * n + k], b = cur[q];
                                W[(size_t) (i + 1) * n + k] = s * a + c * b;
                                cur[q]                      = c * a - s * b;
                            }
                        }
                    }
#pragma unroll
                    for (int q = 0; q < LIN_SLOTS; q++) {
                        const int k = tid + q * LIN_THREADS;
                        if (k < n) W[(size_t) l * n + k] = cur[q];
                    }
                    p      = -s * s2 * c3 * el1 * el / dl1;
                    new_el = s * p;
                    new_dl = c * p;
                }
                __syncthreads();
                if (tid < n) {
#pragma unroll
                    for (int q = 0; q < LIN_SLOTS; q++) {
                        const int k = tid + q * LIN_THREADS;
                        if (k > l && k <= m) d[k] = keep_d[q], e[k] = keep_e[q];
                    }
                    if (tid == 0) e[l] = new_el, d[l] = new_dl;
                }
                __syncthreads();
                more = fabs(e[l]) > eps * tst1 && iter < 60;
            } while (more);
            if (fabs(e[l]) > eps * tst1) capped = true; // (left the loop on the iteration cap)
        }
        __syncthreads();
        if (tid == 0) {
            d[l] = d[l] + f;
            e[l] = 0.0;
        }
        __syncthreads();
    }
    // ---- ascending order (ties by index), kept where e was
    int rank[LIN_SLOTS];
#pragma unroll
    for (int q = 0; q < LIN_SLOTS; q++) {
        const int x = tid + q * LIN_THREADS;
        rank[q]     = 0;
        if (x < n) {
            const double dx = d[x];
            for (int y = 0; y < n; y++) {
                const double dy = d[y];
                rank[q] += (dy < dx || (dy == dx && y < x)) ? 1 : 0;
            }
        }
    }
    __syncthreads();
    int *ord = reinterpret_cast<int *>(e);
#pragma unroll
    for (int q = 0; q < LIN_SLOTS; q++) {
        const int x = tid + q * LIN_THREADS;
        if (x < n) ord[rank[q]] = x;
    }
    __syncthreads();
    return capped;
}

template <bool IN_LDS>
__global__ __launch_bounds__(LIN_THREADS) void k_marg_linearize(int n_items, const int32_t *__restrict__ items, const lin_desc *__restrict__ desc,
                                                                const double *__restrict__ H, const double *__restrict__ b, double eps, double *Hp,
                                                                double *bp, double *J0, double *e0, double *evals, double *min_ev_m, int32_t *status,
                                                                double *scratch) {
    extern __shared__ double lin_lds[];
    __shared__ int s_m;
    if ((int) blockIdx.x >= n_items) return;
    const int w = items[blockIdx.x], tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const lin_desc D = desc[w];
    const int P = D.P, m = D.m, r = P - m, nmax = m > r ? m : r;
    double *d = lin_lds, *e = lin_lds + nmax;
    double *S       = IN_LDS ? lin_lds + 2 * (size_t) nmax : scratch + D.s_off + r;
    double *bpw     = scratch + D.s_off;
    const double *Hw = H + D.h_off, *bw = b + D.b_off;
    double *J0w = J0 + D.rr_off;
    int st       = 0;
    double minev = INFINITY;
    double *T    = S + 2 * (size_t) m * m; // r x m
    if (m > 0) { // ---- (a) :170-192 on the m leading columns
        double *Wm = S, *Hinv = S + (size_t) m * m;
        for (int idx = tid; idx < m * m; idx += LIN_THREADS) {
            const int i = idx / m, j = idx - i * m;
            Wm[(size_t) j * m + i] = 0.5 * (Hw[(size_t) i * P + j] + Hw[(size_t) j * P + i]);
        }
        __syncthreads();
        if (lin_eigen(m, Wm, d, e, &s_m)) st |= 1;
        const int *ord = reinterpret_cast<const int *>(e);
        minev          = d[ord[0]];
        if (minev <= eps) st |= 2;
        double *inv = T; // (T is formed after Hinv is complete)
        for (int k = tid; k < m; k += LIN_THREADS) {
            const double ev = d[ord[k]];
            inv[k]          = ev > eps ? 1.0 / ev : 0.0;
        }
        __syncthreads();
        for (int idx = tid; idx < m * m; idx += LIN_THREADS) {
            const int i = idx / m, j = idx - i * m;
            if (j > i) continue;
            double s = 0;
            for (int k = 0; k < m; k++) {
                const double *vk = Wm + (size_t) ord[k] * m;
                const double wv  = vk[i] * inv[k];
                s += wv * vk[j];
            }
            Hinv[(size_t) i * m + j] = Hinv[(size_t) j * m + i] = s;
        }
        __syncthreads();
        for (int idx = tid; idx < r * m; idx += LIN_THREADS) {
            const int i = idx / m, j = idx - i * m;
            double s = 0;
            for (int k = 0; k < m; k++) s += Hw[(size_t) (m + i) * P + k] * Hinv[(size_t) k * m + j];
            T[idx] = s;
        }
        __syncthreads();
    }
    // Hp goes to the window's J0 block first (the working matrix may overlap T) and is loaded transposed from there
    double *Hpw = Hp ? Hp + D.rr_off : nullptr;
    for (int idx = tid; idx < r * r; idx += LIN_THREADS) {
        const int i = idx / r, j = idx - i * r;
        double v = Hw[(size_t) (m + i) * P + m + j];
        if (m > 0) {
            double s = 0;
            for (int k = 0; k < m; k++) s += T[(size_t) i * m + k] * Hw[(size_t) k * P + m + j];
            v = v - s;
        }
        J0w[idx] = v;
        if (Hpw) Hpw[idx] = v;
    }
    for (int i = tid; i < r; i += LIN_THREADS) {
        double v = bw[m + i];
        if (m > 0) {
            double s = 0;
            for (int k = 0; k < m; k++) s += T[(size_t) i * m + k] * bw[k];
            v = v - s;
        }
        bpw[i] = v;
        if (bp) bp[D.r_off + i] = v;
    }
    __syncthreads();
    double *Wr = S;
    for (int idx = tid; idx < r * r; idx += LIN_THREADS) {
        const int i = idx / r, j = idx - i * r;
        Wr[(size_t) j * r + i] = J0w[idx];
    }
    __syncthreads();
    // ---- (b) :153-167
    if (lin_eigen(r, Wr, d, e, &s_m)) st |= 1;
    const int *ord = reinterpret_cast<const int *>(e);
    if (d[ord[0]] <= eps) st |= 4;
    for (int k = tid; k < r; k += LIN_THREADS) {
        const double ev = d[ord[k]];
        if (evals) evals[D.r_off + k] = ev;
        const double Sinv = ev > eps ? 1.0 / ev : 0.0, si = sqrt(Sinv);
        const double *src = Wr + (size_t) ord[k] * r;
        double vb         = 0;
        for (int i = 0; i < r; i++) vb += src[i] * -bpw[i];
        e0[D.r_off + k] = si * vb;
    }
    for (int k = wave; k < r; k += LIN_WAVES) {
        const double ev = d[ord[k]];
        const double ss = sqrt(ev > eps ? ev : 0.0);
        const double *src = Wr + (size_t) ord[k] * r;
        for (int i = lane; i < r; i += 64) J0w[(size_t) k * r + i] = ss * src[i];
    }
    if (tid == 0) {
        if (min_ev_m) min_ev_m[w] = minev;
        if (status) status[w] = st;
    }
}

// ---- the reduced systems formed where their halves lie (icg_marg_linearize_resident)
#define FORM_TILE 32
#define FORM_THREADS 256
struct form_desc {
    int32_t Pw, has_part;
    int64_t S_off, part_off, h_off; // the window's S (row stride P) in d_red_S, its packed part in d_red_H, its H (Pw x Pw) in the formed buffer
};

// grid (tiles of the widest window's lower triangle, selected windows); a workgroup owns the 32 x 32 tile (ti, tj), tj <= ti, of one window.
// The cells i >= j of the tile are summed and stored along their rows (part, S and H contiguous in j), kept in a padded LDS tile and stored
// once more transposed, again along rows of H: both stores are contiguous.  The diagonal is written by the first store only.
__global__ __launch_bounds__(FORM_THREADS) void k_marg_form_h(const form_desc *__restrict__ desc, int P, const double *__restrict__ S,
                                                             const double *__restrict__ part, double *__restrict__ H) {
    __shared__ double tile[FORM_TILE][FORM_TILE + 1];
    const form_desc D = desc[blockIdx.y];
    const int Pw = D.Pw, nt = (Pw + FORM_TILE - 1) / FORM_TILE, t = blockIdx.x;
    if (t >= nt * (nt + 1) / 2) return; // (a narrower window than the widest of the call: uniform over the workgroup)
    int ti = (int) ((sqrtf(8.0f * (float) t + 1.0f) - 1.0f) * 0.5f);
    while ((ti + 1) * (ti + 2) / 2 <= t) ti++;
    while (ti * (ti + 1) / 2 > t) ti--;
    const int tj = t - ti * (ti + 1) / 2;
    const double *Sw = S + D.S_off, *pw = part + D.part_off;
    double *Hw = H + D.h_off;
    const int tx = threadIdx.x & (FORM_TILE - 1), ty = threadIdx.x / FORM_TILE; // 32 x 8
    for (int y = ty; y < FORM_TILE; y += FORM_THREADS / FORM_TILE) {
        const int i = ti * FORM_TILE + y, j = tj * FORM_TILE + tx;
        if (i < Pw && j <= i) {
            const double a = D.has_part ? pw[(size_t) i * (i + 1) / 2 + j] : 0.0;
            const double v = a + Sw[(size_t) i * P + j];
            Hw[(size_t) i * Pw + j] = v;
            tile[y][tx]             = v;
        }
    }
    __syncthreads();
    for (int y = ty; y < FORM_TILE; y += FORM_THREADS / FORM_TILE) {
        const int j = tj * FORM_TILE + y, i = ti * FORM_TILE + tx; // the cell (i, j), i > j, goes to H[j][i]
        if (i < Pw && j < i) Hw[(size_t) j * Pw + i] = tile[tx][y];
    }
}

// where icg_marg_linearize_resident takes its systems from: system k is window win[k] of the resident partition (common stride P)
struct lin_resident {
    int P;
    const int32_t *win;
    double *H_out; // optional: the formed systems, for tests and diagnostics
};

// All entries.  H comes from the caller (R == nullptr: uploaded with b) or is formed on the device from the resident halves (R); the
// descriptors, the LDS / global-scratch split, the outputs and the keep logic are one path.
// keep: J0 / e0 are written into the context's kept buffer (icg_lin_kept) instead of the arena's outgoing slots, which a
// device-to-device copy then feeds where the host asked for them — the kernels and their launches are the same either way.
int lin_batch(const char *fn, bool keep, icg_ctx *ctx, int n_windows, const int32_t *P, const int32_t *m, const double *H, const double *b, double eps,
              double *Hp, double *bp, double *J0, double *e0, double *evals, double *min_ev_m, int32_t *status, uint64_t *keep_id,
              const lin_resident *R = nullptr) {
    if (!ctx) return ICG_ERR_INVALID;
    icg_kept_drop(ctx); // whatever linearization the context kept is gone, also when this call fails
    if (keep && !keep_id) return icg_fail(ctx, ICG_ERR_INVALID, "%s: NULL argument", fn);
    if (keep) *keep_id = 0;
    if (n_windows <= 0) return icg_fail(ctx, ICG_ERR_INVALID, "%s: %s = %d", fn, R ? "n_sel" : "n_windows", n_windows);
    if (n_windows > 65535) return icg_fail(ctx, ICG_ERR_CAPACITY, "%s: %d windows in one call (at most 65535)", fn, n_windows);
    if (!P || !m || (R ? !R->win : !H) || !b || (!keep && (!J0 || !e0))) return icg_fail(ctx, ICG_ERR_INVALID, "%s: NULL argument", fn);
    if (!(eps >= 0.0)) return icg_fail(ctx, ICG_ERR_INVALID, "%s: eps = %g", fn, eps);
    const size_t n = (size_t) n_windows;
    if (R) {
        const int W = ctx->part_w.W;
        if (W <= 0 || !ctx->red_S_valid || ctx->red_W != W || ctx->red_P != R->P || R->P <= 0)
            return icg_fail(ctx, ICG_ERR_INVALID, "%s: no resident reduced systems of %d columns: call icg_reproj_schur_windows_resident first", fn, R->P);
        std::vector<char> listed((size_t) W, 0);
        for (size_t k = 0; k < n; k++) {
            const int w = R->win[k];
            if (w < 0 || w >= W) return icg_fail(ctx, ICG_ERR_INVALID, "%s: position %zu: window %d outside the partition of %d", fn, k, w, W);
            if (listed[(size_t) w]) return icg_fail(ctx, ICG_ERR_INVALID, "%s: position %zu: window %d is listed twice", fn, k, w);
            listed[(size_t) w] = 1;
            if (P[k] <= 0 || P[k] > R->P) return icg_fail(ctx, ICG_ERR_INVALID, "%s: position %zu, window %d: Pw = %d (1 .. %d)", fn, k, w, P[k], R->P);
            const int have = (size_t) w < ctx->red_H_cols.size() ? ctx->red_H_cols[(size_t) w] : 0;
            if (have != 0 && have != P[k])
                return icg_fail(ctx, ICG_ERR_INVALID, "%s: position %zu, window %d: the resident host part has %d columns, not %d", fn, k, w, have, P[k]);
            if (m[k] < 0 || m[k] >= P[k])
                return icg_fail(ctx, ICG_ERR_INVALID, "%s: position %zu, window %d: m = %d (0 <= m < Pw = %d)", fn, k, w, m[k], P[k]);
        }
    }
    for (size_t w = 0; w < n; w++)
        if (P[w] <= 0 || m[w] < 0 || m[w] >= P[w])
            return icg_fail(ctx, ICG_ERR_INVALID, "%s: window %zu: P = %d, m = %d (0 <= m < P)", fn, w, P[w], m[w]);
    for (size_t w = 0; w < n; w++) // (after the argument checks: an invalid batch is invalid whatever its size)
        if (P[w] > ICG_MARG_LIN_MAX_P)
            return icg_fail(ctx, ICG_ERR_CAPACITY, "%s: window %zu: P = %d is above the limit %d", fn, w, P[w], ICG_MARG_LIN_MAX_P);
    ICG_HIP(ctx, hipSetDevice(ctx->cfg.device));
    const size_t lds_limit = icg_lds_limit(ctx) - 256; // (- the kernel's static words)
    std::vector<lin_desc> desc(n);
    std::vector<int32_t> items(n); // the windows that run in LDS first, then the others
    size_t th = 0, tb = 0, tr = 0, trr = 0, ts = 0, lds_fast = 0, lds_slow = 0;
    int n_fast = 0;
    std::vector<char> fast(n);
    for (size_t w = 0; w < n; w++) {
        const int r = P[w] - m[w], nmax = m[w] > r ? m[w] : r;
        const size_t need = (lin_work(m[w], r) + 2 * (size_t) nmax) * sizeof(double);
        fast[w]           = need <= lds_limit;
        desc[w]           = {P[w], m[w], (int64_t) th, (int64_t) tb, (int64_t) tr, (int64_t) trr, (int64_t) ts};
        th += (size_t) P[w] * P[w], tb += (size_t) P[w], tr += (size_t) r, trr += (size_t) r * r;
        ts += (size_t) r + (fast[w] ? 0 : lin_work(m[w], r));
        if (fast[w]) {
            n_fast++;
            if (need > lds_fast) lds_fast = need;
        } else if (2 * (size_t) nmax * sizeof(double) > lds_slow) {
            lds_slow = 2 * (size_t) nmax * sizeof(double);
        }
    }
    {
        int a = 0, z = n_fast;
        for (size_t w = 0; w < n; w++) items[(size_t) (fast[w] ? a++ : z++)] = (int32_t) w;
    }
    int rc = icg_grow(ctx, (void **) &ctx->d_lin_scratch, &ctx->lin_scratch_cap, ts * sizeof(double), ts * sizeof(double));
    if (rc) return rc;
    if (R && (rc = icg_grow(ctx, (void **) &ctx->d_lin_H, &ctx->lin_H_cap, th * sizeof(double), th * sizeof(double)))) return rc;
    std::vector<form_desc> form(R ? n : 0);
    int form_tiles = 0;
    for (size_t k = 0; k < form.size(); k++) {
        const size_t w = (size_t) R->win[k], slot = (size_t) R->P * (R->P + 1) / 2;
        const int nt = (P[k] + FORM_TILE - 1) / FORM_TILE;
        form[k]      = {P[k], w < ctx->red_H_cols.size() && ctx->red_H_cols[w] != 0 ? 1 : 0, (int64_t) (w * (size_t) R->P * R->P), (int64_t) (w * slot), desc[k].h_off};
        form_tiles   = std::max(form_tiles, nt * (nt + 1) / 2);
    }
    icg_lin_kept &K = ctx->lin_kept;
    if (keep && (rc = icg_grow(ctx, (void **) &K.d_buf, &K.cap, (trr + tr) * sizeof(double), (trr + tr) * sizeof(double)))) return rc;
    static icg_lds_grant granted;
    if ((rc = icg_allow_lds(ctx, reinterpret_cast<const void *>(k_marg_linearize<true>), lds_fast, lds_limit, granted))) return rc;
    icg_call c(ctx);
    const size_t out_doubles = 2 * trr + 3 * tr + n;
    rc = c.reserve(sizeof(double) * ((R && !R->H_out ? 0 : th) + tb + out_doubles) + n * (sizeof(lin_desc) + sizeof(form_desc) + 8) + 20 * 256);
    if (rc) return rc;
    const double *d_H       = R ? ctx->d_lin_H : c.in(H, th);
    const double *d_b       = c.in(b, tb);
    const lin_desc *d_desc  = c.in(desc.data(), n);
    const int32_t *d_items  = c.in(items.data(), n);
    const form_desc *d_form = R ? c.in(form.data(), n) : nullptr;
    if ((rc = c.seal())) return rc;
    // (keep: the outgoing slots are still laid out — the arena offsets of the other outputs do not depend on the entry)
    double *a_J0 = c.out(J0, trr), *a_e0 = c.out(e0, tr);
    double *d_J0 = keep ? K.d_buf : a_J0, *d_e0 = keep ? K.d_buf + trr : a_e0;
    double *d_Hp  = Hp ? c.out(Hp, trr) : nullptr;
    double *d_bp  = bp ? c.out(bp, tr) : nullptr;
    double *d_ev  = evals ? c.out(evals, tr) : nullptr;
    double *d_min = min_ev_m ? c.out(min_ev_m, n) : nullptr;
    int32_t *d_st = status ? c.out(status, n) : nullptr;
    double *a_H   = R && R->H_out ? c.out(R->H_out, th) : nullptr;
    ICG_LAUNCH_GUARD(c);
    if (R) {
        icg_prof_scope ps(ctx, "marg_form_h");
        hipLaunchKernelGGL(k_marg_form_h, dim3((unsigned) form_tiles, (unsigned) n), dim3(FORM_THREADS), 0, ctx->stream, d_form, R->P, (const double *) ctx->d_red_S,
                           (const double *) ctx->d_red_H, ctx->d_lin_H);
    }
    if (a_H) ICG_HIP(ctx, hipMemcpyAsync(a_H, ctx->d_lin_H, th * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    if (n_fast > 0) {
        icg_prof_scope ps(ctx, "marg_lin_lds");
        hipLaunchKernelGGL(k_marg_linearize<true>, dim3(n_fast), dim3(LIN_THREADS), lds_fast, ctx->stream, n_fast, d_items, d_desc, d_H, d_b, eps, d_Hp, d_bp,
                           d_J0, d_e0, d_ev, d_min, d_st, ctx->d_lin_scratch);
    }
    if (n_windows - n_fast > 0) {
        icg_prof_scope ps(ctx, "marg_lin_global");
        hipLaunchKernelGGL(k_marg_linearize<false>, dim3(n_windows - n_fast), dim3(LIN_THREADS), lds_slow, ctx->stream, n_windows - n_fast, d_items + n_fast,
                           d_desc, d_H, d_b, eps, d_Hp, d_bp, d_J0, d_e0, d_ev, d_min, d_st, ctx->d_lin_scratch);
    }
    ICG_HIP(ctx, hipGetLastError());
    if (keep && J0) ICG_HIP(ctx, hipMemcpyAsync(a_J0, d_J0, trr * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    if (keep && e0) ICG_HIP(ctx, hipMemcpyAsync(a_e0, d_e0, tr * sizeof(double), hipMemcpyDeviceToDevice, ctx->stream));
    if ((rc = c.finish())) return rc;
    if (keep) {
        K.total_rr = (int64_t) trr, K.total_r = (int64_t) tr;
        K.r.resize(n), K.rr_off.resize(n), K.r_off.resize(n);
        for (size_t w = 0; w < n; w++) K.r[w] = P[w] - m[w], K.rr_off[w] = desc[w].rr_off, K.r_off[w] = desc[w].r_off;
        *keep_id = icg_kept_register(ctx);
    }
    return ICG_OK;
}

} // namespace

extern "C" int icg_marg_linearize_batch(icg_ctx *ctx, int n_windows, const int32_t *P, const int32_t *m, const double *H, const double *b, double eps,
                                        double *Hp, double *bp, double *J0, double *e0, double *evals, double *min_ev_m, int32_t *status) {
    return lin_batch("icg_marg_linearize_batch", false, ctx, n_windows, P, m, H, b, eps, Hp, bp, J0, e0, evals, min_ev_m, status, nullptr);
}

// The same call with J0 / e0 of every window also left on the device for icg_marg_prior_set_from_kept (factors/marginalization_info.h:153-192
// feeding factors/marginalization_factor.h:47-101 without the detour through the host).
extern "C" int icg_marg_linearize_batch_keep(icg_ctx *ctx, int n_windows, const int32_t *P, const int32_t *m, const double *H, const double *b, double eps,
                                             double *Hp, double *bp, double *J0, double *e0, double *evals, double *min_ev_m, int32_t *status,
                                             uint64_t *keep_id) {
    return lin_batch("icg_marg_linearize_batch_keep", true, ctx, n_windows, P, m, H, b, eps, Hp, bp, J0, e0, evals, min_ev_m, status, keep_id);
}

// M3 on the reduced systems the context holds (see the head of this file): system k is window win[k] of the resident partition, formed on the
// device from its host-factor part and its S (M2, factors/marginalization_info.h:195-230), then linearized (:153-192) by the same kernels.
extern "C" int icg_marg_linearize_resident(icg_ctx *ctx, int P, int n_sel, const int32_t *win, const int32_t *Pw, const int32_t *m, const double *b,
                                           double eps, double *Hp, double *bp, double *J0, double *e0, double *evals, double *min_ev_m, int32_t *status,
                                           double *H_out, uint64_t *keep_id) {
    const lin_resident R{P, win, H_out};
    return lin_batch("icg_marg_linearize_resident", keep_id != nullptr, ctx, n_sel, Pw, m, nullptr, b, eps, Hp, bp, J0, e0, evals, min_ev_m, status, keep_id, &R);
}
