// F6: cv::findFundamentalMat(FM_RANSAC, 1.5 px, 0.99) outlier cull (tracking/tracking.cc:547-555) and
// F8: Tracking::triangulatePoint (tracking/tracking.cc:800-811), batched.
//
// Algorithm definition: SURVEY.md Appendix B.9/B.10 with the formulation pinned in oracle/orc_ransac.cc
// (one-sided Jacobi null space, transcendental-free cubic, double scoring with float compare, sequential
// best/niters replay).  F6 runs one point set's whole RANSAC run inside one workgroup (k_fm_ransac_sets); the device-resident tracker
// launches it on its segments and the C entry points stage their sets as segments and make the same launch.  F8 is a lane per point
// (k_triangulate_seg), likewise shared by the tracker and icg_triangulate.
#include <algorithm>
#include <cfloat>
#include <cmath>
#include <map>
#include <mutex>

#include "icg_internal.h"

__device__ int dev_solve_cubic_real(const double c[4], double roots[3]) {
    double a = c[0], b = c[1], cc = c[2], d = c[3];
    double scale = fmax(fmax(fabs(a), fabs(b)), fmax(fabs(cc), fabs(d)));
    if (scale == 0) return 0;
    int n = 0;
    if (fabs(a) <= 1e-14 * scale) {
        if (fabs(b) <= 1e-14 * scale) {
            if (fabs(cc) <= 1e-14 * scale) return 0;
            roots[0] = -d / cc;
            return 1;
        }
        double disc = cc * cc - 4 * b * d;
        if (disc < 0) return 0;
        double sq = sqrt(disc);
        double q  = -0.5 * (cc + (cc >= 0 ? sq : -sq));
        roots[0]  = q / b; // cv::solveCubic's quadratic branch: x0 = q/a1, x1 = a3/q (q the larger-magnitude root of the resolvent)
        roots[1]  = (q != 0) ? d / q : roots[0];
        return disc > 0 ? 2 : 1;
    }
    const double p = b / a, q = cc / a, r = d / a;
    const double B = 1.0 + fmax(fabs(p), fmax(fabs(q), fabs(r)));
    double lo = -B, hi = B;
    for (int it = 0; it < 200; it++) {
        double mid = 0.5 * (lo + hi);
        if (mid == lo || mid == hi) break;
        double fm = ((mid + p) * mid + q) * mid + r;
        if (fm < 0)
            lo = mid;
        else
            hi = mid;
    }
    double x1 = 0.5 * (lo + hi);
    for (int it = 0; it < 2; it++) {
        double dfx = (3 * x1 + 2 * p) * x1 + q;
        if (dfx != 0) {
            double fx = ((x1 + p) * x1 + q) * x1 + r;
            double xn = x1 - fx / dfx;
            if (xn >= -B && xn <= B) x1 = xn;
        }
    }
    roots[n++] = x1;
    double b2 = p + x1, c2 = q + b2 * x1;
    double disc = b2 * b2 - 4 * c2;
    if (disc >= 0) {
        double sq = sqrt(disc);
        double qq = -0.5 * (b2 + (b2 >= 0 ? sq : -sq));
        double r1 = qq, r2 = (qq != 0) ? c2 / qq : qq;
        roots[n++] = r1;
        roots[n++] = r2;
    }
    // ascending insertion sort (n <= 3)
    for (int i = 1; i < n; i++) {
        double v = roots[i];
        int j    = i - 1;
        while (j >= 0 && roots[j] > v) {
            roots[j + 1] = roots[j];
            j--;
        }
        roots[j + 1] = v;
    }
    if (n == 3) { // cv::solveCubic's order of three real roots: (smallest, largest, middle)
        const double mid = roots[1];
        roots[1]         = roots[2];
        roots[2]         = mid;
    }
    return n;
}

// The seven-point solve of ONE hypothesis by the calling lane: up to three fundamental matrices into out27, their number into *n_out.
__device__ __forceinline__ void seven_point_solve(const int *idx /*7*/, const float2 *pts1, const float2 *pts2, double *out27, int *n_out) {
    // M = A^T (9 x 7) register resident; see oracle/orc_ransac.cc null_space_9x7 for the definition this mirrors.
    double M[9][7];
#pragma unroll
    for (int i = 0; i < 7; i++) {
        const float2 a = pts1[idx[i]], b = pts2[idx[i]];
        const double x1 = a.x, y1 = a.y, x2 = b.x, y2 = b.y;
        M[0][i] = x2 * x1;
        M[1][i] = x2 * y1;
        M[2][i] = x2;
        M[3][i] = y2 * x1;
        M[4][i] = y2 * y1;
        M[5][i] = y2;
        M[6][i] = x1;
        M[7][i] = y1;
        M[8][i] = 1;
    }
    for (int sweep = 0; sweep < 30; sweep++) {
        bool changed = false;
#pragma unroll
        for (int p = 0; p < 6; p++)
#pragma unroll
            for (int q = p + 1; q < 7; q++) {
                double alpha = 0, beta = 0, gamma = 0;
#pragma unroll
                for (int k = 0; k < 9; k++) {
                    double gp = M[k][p], gq = M[k][q];
                    alpha += gp * gp;
                    beta += gq * gq;
                    gamma += gp * gq;
                }
                if (gamma != 0.0 && !(fabs(gamma) <= 1e-15 * sqrt(alpha * beta))) {
                    changed     = true;
                    double zeta = (beta - alpha) / (2.0 * gamma);
                    double t    = 1.0 / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                    if (zeta < 0) t = -t;
                    double c = 1.0 / sqrt(1.0 + t * t);
                    double s = c * t;
#pragma unroll
                    for (int k = 0; k < 9; k++) {
                        double gp = M[k][p], gq = M[k][q];
                        M[k][p] = c * gp - s * gq;
                        M[k][q] = s * gp + c * gq;
                    }
                }
            }
        if (!changed) break;
    }
    double B[9][9]; // B[c][k]: basis vector c, coordinate k
#pragma unroll
    for (int c = 0; c < 7; c++) {
        double s = 0;
#pragma unroll
        for (int k = 0; k < 9; k++) s += M[k][c] * M[k][c];
        double w = sqrt(s);
#pragma unroll
        for (int k = 0; k < 9; k++) B[c][k] = (w > 0) ? M[k][c] / w : 0.0;
    }
#pragma unroll
    for (int t = 0; t < 2; t++) {
        const int nb = 7 + t;
        int js = 0;
        double best = 0;
#pragma unroll
        for (int j = 0; j < 9; j++) {
            double d = 0;
#pragma unroll
            for (int c = 0; c < nb; c++) d += B[c][j] * B[c][j];
            if (j == 0 || d < best) {
                best = d;
                js   = j;
            }
        }
        double v[9];
#pragma unroll
        for (int k = 0; k < 9; k++) v[k] = (k == js) ? 1.0 : 0.0;
#pragma unroll
        for (int pass = 0; pass < 2; pass++)
#pragma unroll
            for (int c = 0; c < nb; c++) {
                double d = 0;
#pragma unroll
                for (int k = 0; k < 9; k++) d += B[c][k] * v[k];
#pragma unroll
                for (int k = 0; k < 9; k++) v[k] -= d * B[c][k];
            }
        double s = 0;
#pragma unroll
        for (int k = 0; k < 9; k++) s += v[k] * v[k];
        double w = sqrt(s);
#pragma unroll
        for (int k = 0; k < 9; k++) B[nb][k] = (w > 0) ? v[k] / w : 0.0;
    }
    double f1[9], f2[9];
#pragma unroll
    for (int k = 0; k < 9; k++) {
        f1[k] = B[7][k];
        f2[k] = B[8][k];
    }
    for (int i = 0; i < 9; i++) f1[i] -= f2[i];
    double c[4], t0, t1, t2;
    t0   = f2[4] * f2[8] - f2[5] * f2[7];
    t1   = f2[3] * f2[8] - f2[5] * f2[6];
    t2   = f2[3] * f2[7] - f2[4] * f2[6];
    c[3] = f2[0] * t0 - f2[1] * t1 + f2[2] * t2;
    c[2] = f1[0] * t0 - f1[1] * t1 + f1[2] * t2 - f1[3] * (f2[1] * f2[8] - f2[2] * f2[7]) +
           f1[4] * (f2[0] * f2[8] - f2[2] * f2[6]) - f1[5] * (f2[0] * f2[7] - f2[1] * f2[6]) +
           f1[6] * (f2[1] * f2[5] - f2[2] * f2[4]) - f1[7] * (f2[0] * f2[5] - f2[2] * f2[3]) +
           f1[8] * (f2[0] * f2[4] - f2[1] * f2[3]);
    t0   = f1[4] * f1[8] - f1[5] * f1[7];
    t1   = f1[3] * f1[8] - f1[5] * f1[6];
    t2   = f1[3] * f1[7] - f1[4] * f1[6];
    c[0] = f1[0] * t0 - f1[1] * t1 + f1[2] * t2;
    c[1] = f2[0] * t0 - f2[1] * t1 + f2[2] * t2 - f2[3] * (f1[1] * f1[8] - f1[2] * f1[7]) +
           f2[4] * (f1[0] * f1[8] - f1[2] * f1[6]) - f2[5] * (f1[0] * f1[7] - f1[1] * f1[6]) +
           f2[6] * (f1[1] * f1[5] - f1[2] * f1[4]) - f2[7] * (f1[0] * f1[5] - f1[2] * f1[3]) +
           f2[8] * (f1[0] * f1[4] - f1[1] * f1[3]);
    double roots[3];
    const int n = dev_solve_cubic_real(c, roots);
    double *out = out27;
    for (int k = 0; k < n; k++) {
        double lambda = roots[k], mu = 1.;
        double s   = f1[8] * roots[k] + f2[8];
        double *Fk = out + 9 * k;
        if (fabs(s) > DBL_EPSILON) {
            mu = 1. / s;
            lambda *= mu;
            Fk[8] = 1.;
        } else
            Fk[8] = 0.;
        for (int i = 0; i < 8; i++) Fk[i] = f1[i] * lambda + f2[i] * mu;
    }
    *n_out = n;
}

// ---------------------------------------------------------------------------------------------------------
// F8: 4x4 DLT, smallest right singular vector by one-sided Jacobi (registers), one lane per point.
// one point: T0 / T1 its two 3x4 camera matrices, pc0 / pc1 / pw entry i of the arrays
__device__ __forceinline__ void triangulate_point(int i, const double *T0, const double *T1, const double *pc0, const double *pc1, double *pw) {
    double D[4][4], V[4][4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        D[0][j] = pc0[3 * i] * T0[2 * 4 + j] - T0[0 * 4 + j];
        D[1][j] = pc0[3 * i + 1] * T0[2 * 4 + j] - T0[1 * 4 + j];
        D[2][j] = pc1[3 * i] * T1[2 * 4 + j] - T1[0 * 4 + j];
        D[3][j] = pc1[3 * i + 1] * T1[2 * 4 + j] - T1[1 * 4 + j];
    }
#pragma unroll
    for (int a = 0; a < 4; a++)
#pragma unroll
        for (int b = 0; b < 4; b++) V[a][b] = (a == b) ? 1.0 : 0.0;
    for (int sweep = 0; sweep < 30; sweep++) {
        bool changed = false;
#pragma unroll
        for (int p = 0; p < 3; p++)
#pragma unroll
            for (int q = p + 1; q < 4; q++) {
                double alpha = 0, beta = 0, gamma = 0;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    alpha += D[k][p] * D[k][p];
                    beta += D[k][q] * D[k][q];
                    gamma += D[k][p] * D[k][q];
                }
                if (gamma == 0.0) continue;
                if (fabs(gamma) <= 1e-15 * sqrt(alpha * beta)) continue;
                changed     = true;
                double zeta = (beta - alpha) / (2.0 * gamma);
                double t    = 1.0 / (fabs(zeta) + sqrt(1.0 + zeta * zeta));
                if (zeta < 0) t = -t;
                double c = 1.0 / sqrt(1.0 + t * t);
                double s = c * t;
#pragma unroll
                for (int k = 0; k < 4; k++) {
                    double gp = D[k][p], gq = D[k][q];
                    D[k][p] = c * gp - s * gq;
                    D[k][q] = s * gp + c * gq;
                    double vp = V[k][p], vq = V[k][q];
                    V[k][p] = c * vp - s * vq;
                    V[k][q] = s * vp + c * vq;
                }
            }
        if (!changed) break;
    }
    int best  = 0;
    double bn = 0;
#pragma unroll
    for (int j = 0; j < 4; j++) {
        double s = 0;
#pragma unroll
        for (int k = 0; k < 4; k++) s += D[k][j] * D[k][j];
        if (j == 0 || s < bn) {
            bn   = s;
            best = j;
        }
    }
    double v0 = V[0][0], v1 = V[1][0], v2 = V[2][0], v3 = V[3][0];
#pragma unroll
    for (int j = 1; j < 4; j++)
        if (best == j) {
            v0 = V[0][j];
            v1 = V[1][j];
            v2 = V[2][j];
            v3 = V[3][j];
        }
    pw[3 * i]     = v0 / v3;
    pw[3 * i + 1] = v1 / v3;
    pw[3 * i + 2] = v2 / v3;
}

// segmented form (device-resident tracker): stream s owns entries [s * seg_cap, s * seg_cap + count[s]) of the point arrays and the
// camera matrices [s * tcw_cap, ...) — its T0 / T1 indices are local to that table
__global__ void k_triangulate_seg(int n_seg, int seg_cap, const int32_t *count, const int32_t *T0_idx, const int32_t *T1_idx, int tcw_cap,
                                  const double *Tcw12, const double *pc0, const double *pc1, double *pw) {
    const int s = blockIdx.y;
    const int k = blockIdx.x * blockDim.x + threadIdx.x;
    if (s >= n_seg || k >= count[s]) return;
    const int i      = s * seg_cap + k;
    const double *T  = Tcw12 + 12 * (size_t) s * tcw_cap;
    triangulate_point(i, T + 12 * (size_t) T0_idx[i], T + 12 * (size_t) T1_idx[i], pc0, pc1, pw);
}

extern "C" int icg_triangulate(icg_ctx *ctx, int n, const int32_t *T0_idx, const int32_t *T1_idx, int n_T,
                               const double *Tcw12, const double *pc0, const double *pc1, double *pw) {
    if (!ctx || n < 0) return ICG_ERR_INVALID;
    if (n == 0) return ICG_OK;
    if (!T0_idx || !T1_idx || !Tcw12 || !pc0 || !pc1 || !pw || n_T <= 0) return ICG_ERR_INVALID;
    if (n > ctx->cfg.max_points) return icg_fail(ctx, ICG_ERR_CAPACITY, "%d points > max_points %d", n, ctx->cfg.max_points);
    for (int i = 0; i < n; i++)
        if (T0_idx[i] < 0 || T0_idx[i] >= n_T || T1_idx[i] < 0 || T1_idx[i] >= n_T)
            return icg_fail(ctx, ICG_ERR_INVALID, "pose index out of range at point %d", i);
    ICG_HIP(ctx, hipSetDevice(ctx->cfg.device));
    icg_call c(ctx);
    int rc = c.reserve((size_t) n * (8 + 48 + 24) + (size_t) n_T * 96 + 64);
    if (rc) return rc;
    // one segment of n points with the whole camera-matrix table: the tracker's launch
    const int32_t *d_n  = c.in_zc(&n, 1);
    const int32_t *d_i0 = c.in_zc(T0_idx, (size_t) n);
    const int32_t *d_i1 = c.in_zc(T1_idx, (size_t) n);
    const double *d_T   = c.in_zc(Tcw12, 12 * (size_t) n_T);
    const double *d_p0  = c.in_zc(pc0, 3 * (size_t) n);
    const double *d_p1  = c.in_zc(pc1, 3 * (size_t) n);
    double *d_pw = c.out_zc(pw, 3 * (size_t) n);
    ICG_LAUNCH_GUARD(c);
    if ((rc = icg_triangulate_launch_segments(ctx, 1, n, d_n, d_i0, d_i1, n_T, d_T, d_p0, d_p1, d_pw))) return rc;
    return c.finish();
}

// ---------------------------------------------------------------------------------------------------------
// F6: cv::findFundamentalMat(FM_RANSAC) of one point set per workgroup, the WHOLE run in one launch:
//   round:  wave 0 draws up to fm_round_size(round) <= FM_HPW subsets from the set's cv::RNG (getSubset + checkSubset with a collinearity test per lane,
//           RNG-consuming redraws) -> LDS
//           wave 0, a lane per hypothesis: seven-point solve (a strictly serial FP64 chain per hypothesis whose rotations cannot be spread over
//           lanes without changing its rounding; different hypotheses advance in different lanes) -> models in LDS
//           four waves, a wave per (hypothesis, model): inlier bits by ballot + count -> LDS
//           thread 0 replays the hypotheses in order: best mask, max_good, niters = RANSACUpdateNumIters(...)
// Any chunking of the hypothesis stream gives the sequential algorithm's result: scores do not depend on one another, and hypotheses past
// the updated niters are discarded.  RANSACUpdateNumIters needs log and pow: their values for every (set size, inlier count) come from a
// table the HOST computed with OpenCV's libm calls (fm_denom_row), so the iteration counts are the sequential algorithm's bit for bit; the
// comparisons, the division and lrint run on the device in IEEE double.
__device__ __forceinline__ unsigned dev_rng_next(unsigned long long &state) {
    state = (unsigned long long) (unsigned) state * 4164903690U + (unsigned) (state >> 32);
    return (unsigned) state;
}
// getSubset + checkSubset of ONE hypothesis by a whole wave (round 5).  The draws (cv::RNG, duplicate rejection) are uniform integer work that
// every lane repeats; checkSubset's collinearity test — the last point against the 15 pairs of the other six, in both point sets: 30
// independent FP64 tests of calib3d's haveCollinearPoints(m, 7), an OR — runs a test per lane (lanes 30..63 repeat tests of lanes 0..29: every lane stays active, because FP64
// and the other half-rate VALU instructions take ~5x as long on gfx950 when 16 or fewer lanes are active — under `if (t == 0)` the
// up-to-32 subsets of a round cost more than the seven-point solves and the scoring together; profiles/ubench/valu_cost_r05.txt).
// idx_lds: the hypothesis' seven indices in LDS (written here, read by the solve).  Same subsets, same RNG consumption as OpenCV's getSubset
// (the sequential form of oracle/orc_ransac.cc).
__device__ bool dev_get_subset_wave(unsigned long long &rng, int n, const float2 *p1, const float2 *p2, int *idx_lds, int lane) {
    const int pr = lane % 15;
    const int j  = pr < 1 ? 1 : pr < 3 ? 2 : pr < 6 ? 3 : pr < 10 ? 4 : 5; // pairs (j, k), k < j < 6, in the order of haveCollinearPoints
    const int k  = pr - j * (j - 1) / 2;
    const float2 *pts = ((lane / 15) & 1) ? p2 : p1;
    for (int attempt = 0; attempt < 10000; attempt++) {
        int idx[7];
        for (int i = 0; i < 7; i++) {
            int v;
            for (;;) {
                v = (int) (dev_rng_next(rng) % (unsigned) n); // RNG::uniform(0, n), n > 0
                bool dup = false;
                for (int q = 0; q < i; q++) dup |= idx[q] == v;
                if (!dup) break;
            }
            idx[i] = v;
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup"); // (the previous attempt's readers are done: one wave, LDS queue in order)
        __builtin_amdgcn_wave_barrier();
        if (lane == 0) {
#pragma unroll
            for (int q = 0; q < 7; q++) idx_lds[q] = idx[q];
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        __builtin_amdgcn_wave_barrier();
        const float2 a = pts[idx_lds[6]], b = pts[idx_lds[j]], c = pts[idx_lds[k]];
        const double dx1 = b.x - a.x, dy1 = b.y - a.y; // (float differences widened, as the CPU form: pts[..].x - pts[..].x in float, then double)
        const double dx2 = c.x - a.x, dy2 = c.y - a.y;
        const bool bad   = fabs(dx2 * dy1 - dy2 * dx1) <= (double) FLT_EPSILON * (fabs(dx1) + fabs(dy1) + fabs(dx2) + fabs(dy2));
        if (__ballot(bad) == 0ull) return true;
    }
    return false;
}

#define FM_HPW 32 // hypotheses per round at most (the LDS tables)
// Hypotheses of round r: 8, 8, 16, then FM_HPW.  Every round is also capped by niters - iter.  After the forward-backward LK cull most sets
// consume fewer than ten hypotheses (FM_HIST below; profiles/r08_ransac_rounds_subpix_groups.txt), so a first round of FM_HPW drew, solved
// and scored mostly discarded ones; the solve is one serial FP64 chain per round whatever the round's size, so the rounds grow quickly.
__device__ __forceinline__ int fm_round_size(int r) { return r < 2 ? 8 : r == 2 ? 16 : FM_HPW; }
#define FMS_MAX_WORDS 16 // 64-bit inlier words per model in LDS: the tracker's form takes sets of up to 1024 points

// symmetric epipolar distance of one correspondence under F (double, compared in float): the inlier test of the scoring and of the mask
__device__ __forceinline__ bool fm_inlier(double F0, double F1, double F2, double F3, double F4, double F5, double F6, double F7, double F8, float2 a0,
                                          float2 b0, float thresh2) {
    const double x1 = a0.x, y1 = a0.y, x2 = b0.x, y2 = b0.y;
    double a = F0 * x1 + F1 * y1 + F2;
    double b = F3 * x1 + F4 * y1 + F5;
    double c = F6 * x1 + F7 * y1 + F8;
    double s2 = 1. / (a * a + b * b);
    double d2 = x2 * a + y2 * b + c;
    a         = F0 * x2 + F3 * y2 + F6;
    b         = F1 * x2 + F4 * y2 + F7;
    c         = F2 * x2 + F5 * y2 + F8;
    double s1 = 1. / (a * a + b * b);
    double d1 = x1 * a + y1 * b + c;
    float e   = (float) fmax(d1 * d1 * s1, d2 * d2 * s2);
    return e <= thresh2;
}

#if defined(FM_HIST)
// profiling build (EXTRA_HIPFLAGS=-DFM_HIST, off in the product): consumed hypotheses (iter at exit) of every set since the library was
// loaded, printed when the process ends
__device__ unsigned long long g_fm_hist[1024];
static void fm_hist_dump() {
    static unsigned long long h[1024];
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_fm_hist), sizeof h) != hipSuccess) return;
    for (int k = 0; k < 1024; k++)
        if (h[k]) fprintf(stderr, "[fm hist] consumed %4d sets %10llu\n", k, h[k]);
}
#endif

// LARGE = false (the tracker's form): the inlier words of every model of a round and the best mask live in LDS (sets up to 64 * FMS_MAX_WORDS
// points), denom_tab is the shared table of fm_denom_table (row n = the set size).  LARGE = true (stand-alone calls with a set above that):
// no inlier words are kept — the replay keeps the best model's nine coefficients and the mask is that model's inlier test re-evaluated per
// point at the end (the same IEEE operations as the scoring: the same bits); denom_tab is the call's own table, row s = set s.
template <bool LARGE>
__global__ __launch_bounds__(256, 1) void k_fm_ransac_sets(int n_sets, int seg_cap, const int32_t *count, const float2 *pts1, const float2 *pts2,
                                                           float thresh2, double log_num, const double *denom_tab, int tab_n, uint8_t *mask) {
    __shared__ double Fm[FM_HPW][27];
    __shared__ int n_sh[FM_HPW];
    __shared__ int idx_sh[FM_HPW][7];
    __shared__ int good_sh[FM_HPW * 3];
    __shared__ unsigned long long bits_sh[FM_HPW * 3][FMS_MAX_WORDS];
    __shared__ unsigned long long best_sh[FMS_MAX_WORDS];
    __shared__ double best_F[9];
    __shared__ int nh_sh, iter_sh, niters_sh, max_good_sh;
    const int s = blockIdx.x, t = threadIdx.x, wave = t >> 6, lane = t & 63;
    if (s >= n_sets) return;
    const int n = count[s];
    if (n <= 0) return; // no set for this stream in this step
    const float2 *p1 = pts1 + (size_t) s * seg_cap, *p2 = pts2 + (size_t) s * seg_cap;
    uint8_t *m       = mask + (size_t) s * seg_cap;
    if (n < 15 || n > tab_n || (!LARGE && n > 64 * FMS_MAX_WORDS)) { // the reference only calls findFundamentalMat with >= 15 points: leave untouched
        for (int i = t; i < n; i += 256) m[i] = 1;
        return;
    }
    const int words = (n + 63) >> 6;
    unsigned long long rng = 0xffffffffffffffffull; // cv::RNG((uint64) -1): the fixed seed of every findFundamentalMat call
    if (t == 0) iter_sh = 0, niters_sh = 1000, max_good_sh = 0;
    if (!LARGE && t < FMS_MAX_WORDS) best_sh[t] = 0;
    __syncthreads();
    for (int round = 0;; round++) {
        if (wave == 0) { // all 64 lanes: see dev_get_subset_wave
            const int it0 = iter_sh;
            int nh        = min(fm_round_size(round), niters_sh - it0);
            for (int h = 0; h < nh; h++) {
                if (!dev_get_subset_wave(rng, n, p1, p2, idx_sh[h], lane)) {
                    // ptsetreg.cpp run(): no valid subset -> the iterations end here (nothing found if this was the first one)
                    if (lane == 0) niters_sh = it0 + h;
                    nh = h;
                    break;
                }
            }
            if (lane == 0) nh_sh = nh;
        }
        __syncthreads();
        const int nh = nh_sh;
        if (nh <= 0) break;
        // FM_HPW lanes solve whatever nh is: lanes nh..FM_HPW-1 repeat hypothesis lane % nh into their own, unread slots of Fm / n_sh (the
        // FP64 chain issued with 16 or fewer active lanes takes ~5x as long; copies take their original's branches, so nothing diverges more)
        if (wave == 0 && lane < FM_HPW) {
            int nm = 0;
            seven_point_solve(idx_sh[lane % nh], p1, p2, Fm[lane], &nm);
            n_sh[lane] = nm;
        }
        __syncthreads();
        for (int pair = wave; pair < 3 * nh; pair += 4) {
            const int hl = pair / 3, model = pair - 3 * hl;
            if (model >= n_sh[hl]) {
                if (lane == 0) good_sh[pair] = -1;
                continue;
            }
            const double *F = Fm[hl] + 9 * model;
            const double F0 = F[0], F1 = F[1], F2 = F[2], F3 = F[3], F4 = F[4], F5 = F[5], F6 = F[6], F7 = F[7], F8 = F[8];
            int cnt = 0;
            for (int base = 0; base < n; base += 64) {
                const int i = base + lane;
                bool in     = false;
                if (i < n) in = fm_inlier(F0, F1, F2, F3, F4, F5, F6, F7, F8, p1[i], p2[i], thresh2);
                const unsigned long long mm = __ballot(in);
                if (!LARGE && lane == 0) bits_sh[pair][base >> 6] = mm;
                cnt += __popcll(mm);
            }
            if (lane == 0) good_sh[pair] = cnt;
        }
        __syncthreads();
        if (t == 0) { // sequential replay of RANSACPointSetRegistrator::run over the scores (ptsetreg.cpp)
            int iter = iter_sh, niters = niters_sh, max_good = max_good_sh;
            for (int h = 0; h < nh && iter < niters; h++, iter++) {
                for (int mdl = 0; mdl < 3; mdl++) {
                    const int good = good_sh[h * 3 + mdl];
                    if (good < 0) break;
                    if (good > max(max_good, 7 - 1)) {
                        if constexpr (LARGE)
                            for (int k = 0; k < 9; k++) best_F[k] = Fm[h][9 * mdl + k];
                        else
                            for (int w = 0; w < words; w++) best_sh[w] = bits_sh[h * 3 + mdl][w];
                        max_good = good;
                        // RANSACUpdateNumIters(conf, (n - good) / n, 7, niters) with log(1 - (1 - ep)^7) from the host's table
                        const double denom = denom_tab[(size_t) (LARGE ? s : n) * (tab_n + 1) + good];
                        if (denom != denom) { // (NaN marks 1 - (1 - ep)^7 < DBL_MIN: "return 0")
                            niters = 0;
                        } else {
                            niters = (denom >= 0 || -log_num >= niters * (-denom)) ? niters : (int) lrint(log_num / denom);
                        }
                    }
                }
            }
            iter_sh = iter, niters_sh = niters, max_good_sh = max_good;
        }
        __syncthreads();
        // (the stop test is read into a register by every thread BEFORE thread 0 may write niters_sh at the top of the next round)
        const bool stop = iter_sh >= niters_sh;
        __syncthreads();
        if (stop) break;
    }
#if defined(FM_HIST)
    if (t == 0) atomicAdd(&g_fm_hist[min(iter_sh, 1023)], 1ull);
#endif
    const bool found = max_good_sh > 0;
    if constexpr (LARGE) {
        const double *F = best_F;
        for (int i = t; i < n; i += 256)
            m[i] = found ? (uint8_t) fm_inlier(F[0], F[1], F[2], F[3], F[4], F[5], F[6], F[7], F[8], p1[i], p2[i], thresh2) : (uint8_t) 0;
    } else {
        for (int i = t; i < n; i += 256) m[i] = found ? (uint8_t) ((best_sh[i >> 6] >> (i & 63)) & 1ull) : (uint8_t) 0;
    }
}

// log(1 - (1 - ep)^7) for ep = (n - good) / n, good = 0..n: the libm calls of OpenCV's RANSACUpdateNumIters (NaN where it returns 0 before
// taking the logarithm)
static void fm_denom_row(int n, double *row) {
    for (int good = 0; good <= n; good++) {
        double ep    = (double) (n - good) / n;
        ep           = std::min(std::max(ep, 0.), 1.);
        double denom = 1. - std::pow(1. - ep, 7);
        row[good]    = denom < DBL_MIN ? std::nan("") : std::log(denom);
    }
}

// the rows n = 0..tab_n of the tracker's form: one table per process and device, shared by every tracker
static int fm_denom_table(icg_ctx *ctx, int tab_n, const double **d_tab) {
    static std::mutex mu;
    static std::map<std::pair<int, int>, double *> tabs;
    std::lock_guard<std::mutex> lock(mu);
    auto key = std::make_pair(ctx->cfg.device, tab_n);
    auto it  = tabs.find(key);
    if (it == tabs.end()) {
        std::vector<double> h((size_t) (tab_n + 1) * (tab_n + 1), 0.0);
        for (int n = 1; n <= tab_n; n++) fm_denom_row(n, &h[(size_t) n * (tab_n + 1)]);
        double *d = nullptr;
        ICG_HIP(ctx, hipMalloc((void **) &d, h.size() * sizeof(double)));
        ICG_HIP(ctx, hipMemcpy(d, h.data(), h.size() * sizeof(double), hipMemcpyHostToDevice));
        it = tabs.emplace(key, d).first;
    }
    *d_tab = it->second;
    return 0;
}

template <bool LARGE>
static int fm_ransac_launch(icg_ctx *ctx, int n_sets, int seg_cap, const int32_t *d_count, const float2 *d_p1, const float2 *d_p2, double thresh,
                            double conf, const double *d_tab, int tab_n, uint8_t *d_mask) {
    if (thresh <= 0) thresh = 3;
    if (conf < DBL_EPSILON || conf > 1 - DBL_EPSILON) conf = 0.99;
    double p         = std::min(std::max(conf, 0.), 1.);
    const double num = std::log(std::max(1. - p, DBL_MIN)); // the numerator of RANSACUpdateNumIters
#if defined(FM_HIST)
    static std::once_flag hist_once;
    std::call_once(hist_once, [] { atexit(fm_hist_dump); });
#endif
    icg_prof_scope ps(ctx, "fm_ransac_sets");
    hipLaunchKernelGGL(k_fm_ransac_sets<LARGE>, dim3(n_sets), dim3(256), 0, ctx->stream, n_sets, seg_cap, d_count, d_p1, d_p2, (float) (thresh * thresh), num,
                       d_tab, tab_n, d_mask);
    ICG_HIP(ctx, hipGetLastError());
    return ICG_OK;
}

int icg_fm_ransac_launch_sets(icg_ctx *ctx, int n_sets, int seg_cap, const int32_t *d_count, const float2 *d_p1, const float2 *d_p2, double thresh,
                              double conf, uint8_t *d_mask) {
    const int tab_n     = std::min(seg_cap, 64 * FMS_MAX_WORDS);
    const double *d_tab = nullptr;
    int rc = fm_denom_table(ctx, tab_n, &d_tab);
    if (rc) return rc;
    return fm_ransac_launch<false>(ctx, n_sets, seg_cap, d_count, d_p1, d_p2, thresh, conf, d_tab, tab_n, d_mask);
}

int icg_triangulate_launch_segments(icg_ctx *ctx, int n_seg, int seg_cap, const int32_t *d_count, const int32_t *d_T0, const int32_t *d_T1, int tcw_cap,
                                    const double *d_Tcw, const double *d_pc0, const double *d_pc1, double *d_pw) {
    icg_prof_scope ps(ctx, "triangulate");
    hipLaunchKernelGGL(k_triangulate_seg, dim3((seg_cap + 63) / 64, n_seg), dim3(64), 0, ctx->stream, n_seg, seg_cap, d_count, d_T0, d_T1, tcw_cap, d_Tcw,
                       d_pc0, d_pc1, d_pw);
    ICG_HIP(ctx, hipGetLastError());
    return ICG_OK;
}

// The stand-alone form: the sets are staged as segments of the padded largest set size and run by the tracker's launch, ONE launch and ONE
// wait for the whole batch.  A batch with a set above 64 * FMS_MAX_WORDS points runs the LARGE form of the kernel instead, with the rows of
// its own set sizes tabulated here.
extern "C" int icg_fm_ransac(icg_ctx *ctx, int n_sets, const int32_t *offsets, const float *pts1, const float *pts2, double thresh, double conf,
                             uint8_t *mask) {
    if (!ctx || n_sets < 0) return ICG_ERR_INVALID;
    if (n_sets == 0) return ICG_OK;
    if (!offsets || !pts1 || !pts2 || !mask) return ICG_ERR_INVALID;
    int seg_cap = 1;
    for (int s = 0; s < n_sets; s++) {
        const int n = offsets[s + 1] - offsets[s];
        if (n < 0) return ICG_ERR_INVALID;
        seg_cap = std::max(seg_cap, n);
    }
    const int total = offsets[n_sets];
    if (total > ctx->cfg.max_points) return icg_fail(ctx, ICG_ERR_CAPACITY, "%d points > max_points %d", total, ctx->cfg.max_points);
    const bool large = seg_cap > 64 * FMS_MAX_WORDS;
    seg_cap          = (seg_cap + 63) & ~63;
    ICG_HIP(ctx, hipSetDevice(ctx->cfg.device));
    const size_t cells = (size_t) n_sets * seg_cap;
    std::vector<float> a(2 * cells, 0.f), b(2 * cells, 0.f);
    std::vector<int32_t> cnt((size_t) n_sets);
    std::vector<double> tab(large ? (size_t) n_sets * (seg_cap + 1) : 0, 0.0);
    for (int s = 0; s < n_sets; s++) {
        const int n = offsets[s + 1] - offsets[s];
        cnt[(size_t) s] = n;
        memcpy(a.data() + 2 * (size_t) s * seg_cap, pts1 + 2 * (size_t) offsets[s], sizeof(float) * 2 * (size_t) n);
        memcpy(b.data() + 2 * (size_t) s * seg_cap, pts2 + 2 * (size_t) offsets[s], sizeof(float) * 2 * (size_t) n);
        if (large && n >= 15) fm_denom_row(n, &tab[(size_t) s * (seg_cap + 1)]);
    }
    std::vector<uint8_t> m(cells, 0);
    icg_call c(ctx);
    int rc = c.reserve(cells * (16 + 1) + sizeof(int32_t) * (size_t) n_sets + sizeof(double) * tab.size() + 4096);
    if (rc) return rc;
    const float2 *d_p1  = (const float2 *) c.in(a.data(), 2 * cells);
    const float2 *d_p2  = (const float2 *) c.in(b.data(), 2 * cells);
    const int32_t *d_n  = c.in(cnt.data(), (size_t) n_sets);
    const double *d_tab = large ? c.in(tab.data(), tab.size()) : nullptr;
    if ((rc = c.seal())) return rc;
    uint8_t *d_m = c.out(m.data(), cells);
    ICG_LAUNCH_GUARD(c);
    rc = large ? fm_ransac_launch<true>(ctx, n_sets, seg_cap, d_n, d_p1, d_p2, thresh, conf, d_tab, seg_cap, d_m)
               : icg_fm_ransac_launch_sets(ctx, n_sets, seg_cap, d_n, d_p1, d_p2, thresh, conf, d_m);
    if (rc || (rc = c.finish())) return rc;
    for (int s = 0; s < n_sets; s++) memcpy(mask + offsets[s], m.data() + (size_t) s * seg_cap, (size_t) cnt[(size_t) s]);
    return ICG_OK;
}

// kept for callers of the earlier one-launch entry point: icg_fm_ransac is that form now
extern "C" int icg_fm_ransac_device(icg_ctx *ctx, int n_sets, const int32_t *offsets, const float *pts1, const float *pts2, double thresh, double conf,
                                    uint8_t *mask) {
    return icg_fm_ransac(ctx, n_sets, offsets, pts1, pts2, thresh, conf, mask);
}
