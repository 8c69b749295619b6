// ---- M2 / f1: the normal equations of the resident reprojection factors, assembled in a fixed order ------------------------------------
// Reference: factors/marginalization_info.h:195-230 (constructEquation: H0 += Ji^T Jj over the block pairs of a factor, b0 -= Ji^T e) and
// the DENSE_SCHUR step of GVINS::gvinsOptimization (ic_gvins.cc:1130-1239, 1763-1837): the inverse-depth blocks (1 x 1) go first.
//
// System of one window, N = P + L:   H = [Hcc G^T; G diag(h_ll)]  (row-major N x N: Hcc in rows/columns < P, landmark l in row P + l —
// only its P camera columns and its diagonal element are ever written or read),  b (N),  inv (L) = 1 / (h_ll + d_l).
//
// No atomics anywhere: rounds 1-5 scattered every J^T J product with FP64 atomicAdd (LDS + global), which made every sum depend on the
// arrival order — results equal to rounding only, the lock-step tests could not ask for identical bits, and same-address LDS atomics were
// the cost of the launch (0.8-1.1 ms for 256 windows of 2 700 factors).  Now every output cell is owned by one thread that adds its
// contributions in an order fixed by the window's own factor list (icg_asm_plan):
//   k_asm_runs       one wave per run = the factors of one ordered (reference pose i, observer pose j) pair.  All of them send their
//                    19 camera columns [Ji | Jj | Je | Jtd] (+ the residual as a 20th column: b = -J^T r) to the SAME cells, so the wave
//                    keeps the 20 x 20 product A^T A (A = the run's 2 rows per factor) in registers — lane t owns one 2 x 2 tile of the 55 in
//                    the upper triangle — and walks the run in list order, 16 factors staged in LDS at a time (operands are LDS broadcasts:
//                    4 ds_read_b128 + 8 v_fma_f64 per factor and lane).  Output: 220 doubles per run, one coalesced 32-B store per lane.
//   k_asm_camera     one thread per cell of Hcc (and of bc): gathers the cell from the runs that touch it — (i,j) and (j,i) for a cell
//                    between two poses, row and column p of the pair table for a cell of pose p's diagonal block or against the shared
//                    extrinsic / td block, every run for the (ext|td)^2 block — and stores it.  Cells nobody touches are stored as zero:
//                    no memset of the system (the old path cleared 1 MB per window per launch).
//   k_asm_landmarks  one thread per (landmark, camera column | h_ll | b_l): walks the landmark's factors in list order.
// Algorithmic traffic per launch: J and r once per kernel that needs them (2 x 384 B per factor), 1.76 KB per run out and in, the system
// rows once.  Bound: HBM/L2 streaming of J; the FP64 FMAs (420 per factor) are 2 % of the vector peak.
#include <chrono>
#include <cstdio>
#include <cstdlib>

#include "reproj_internal.h"

#define ASM_SUB 16   // factors staged per pass
#define ASM_ROW 40   // doubles per staged factor: two rows of 20 columns [Ji 0..5 | Jj 6..11 | Je 12..17 | Jtd 18 | -r 19]
#define ASM_PART 220 // doubles per run: 55 upper-triangular 2 x 2 tiles of the 20 x 20 product
#define ASM_EXT 0xFFF // owner code of the shared (extrinsic | td) pseudo-block: columns 12..18 of a factor's row

// index of (la, lb) inside a run's block: tile (la/2, lb/2) of the upper triangle, element (la&1, lb&1); the diagonal tiles hold both halves
__device__ __forceinline__ int asm_part_index(int la, int lb) {
    int ba = la >> 1, bb = lb >> 1;
    if (ba > bb) {
        const int t = la;
        la = lb, lb = t;
        ba = la >> 1, bb = lb >> 1;
    }
    return (ba * 10 - ((ba * (ba - 1)) >> 1) + (bb - ba)) * 4 + ((la & 1) << 1) + (lb & 1);
}

__global__ __launch_bounds__(256) void k_asm_runs(int n_runs, const int4 *runs, const win_desc *wd, const int32_t *perm, const double *r,
                                                 const double *J, const uint8_t *active, double *part) {
    __shared__ double tiles[4][ASM_SUB * ASM_ROW];
    const int wave = threadIdx.x >> 6, t = threadIdx.x & 63;
    const int ri   = blockIdx.x * 4 + wave;
    if (ri >= n_runs) return;
    const int4 R = runs[ri]; // first, count, li | lj << 16, window
    if (!wd[R.w].reassemble) return;
    double *tile = tiles[wave];
    // this lane's tile of the upper triangle (lanes 55..63 idle along on tile 0 and store nothing)
    int bx = 0, rem = t < 55 ? t : 0, len = 10;
    while (rem >= len) rem -= len, bx++, len--;
    const int by = bx + rem;
    // staging role: lane -> factor t / 4 of the pass, elements (t & 3) + 4 k of its 48 values (J 0..45, r 46..47)
    const int fi = t >> 2, sub = t & 3;
    double v[12];
    auto fetch = [&](int pass) {
        const int k = pass * ASM_SUB + fi;
        bool on     = k < R.y;
        int f       = 0;
        if (on) {
            f = perm[R.x + k];
            if (active && !active[f]) on = false;
        }
        const double *Jf = J + 46 * (size_t) f;
#pragma unroll
        for (int kk = 0; kk < 11; kk++) v[kk] = on ? Jf[sub + 4 * kk] : 0.0;
        v[11] = on ? (sub < 2 ? Jf[44 + sub] : -r[2 * (size_t) f + (sub - 2)]) : 0.0;
    };
    const int npass = (R.y + ASM_SUB - 1) / ASM_SUB;
    double a00 = 0.0, a01 = 0.0, a10 = 0.0, a11 = 0.0;
    fetch(0);
    for (int pass = 0; pass < npass; pass++) {
        // registers -> LDS in the padded two-row layout (the 7th, always-zero column of every 2 x 7 block and the landmark column are dropped)
#pragma unroll
        for (int kk = 0; kk < 12; kk++) {
            const int c = sub + 4 * kk;
            if (c < 42) {
                const int q = c / 7, x = c - 7 * q;
                if (x < 6) tile[fi * ASM_ROW + (q & 1) * 20 + (q >> 1) * 6 + x] = v[kk];
            } else if (c >= 44) {
                tile[fi * ASM_ROW + (c & 1) * 20 + 18 + ((c - 44) >> 1)] = v[kk];
            }
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        __builtin_amdgcn_wave_barrier();
        if (pass + 1 < npass) fetch(pass + 1); // in flight while this pass is multiplied
#pragma unroll
        for (int g = 0; g < ASM_SUB; g++) {
            const double2 x0 = *reinterpret_cast<const double2 *>(&tile[g * ASM_ROW + 2 * bx]);
            const double2 x1 = *reinterpret_cast<const double2 *>(&tile[g * ASM_ROW + 20 + 2 * bx]);
            const double2 y0 = *reinterpret_cast<const double2 *>(&tile[g * ASM_ROW + 2 * by]);
            const double2 y1 = *reinterpret_cast<const double2 *>(&tile[g * ASM_ROW + 20 + 2 * by]);
            a00 = fma(x1.x, y1.x, fma(x0.x, y0.x, a00));
            a01 = fma(x1.x, y1.y, fma(x0.x, y0.y, a01));
            a10 = fma(x1.y, y1.x, fma(x0.y, y0.x, a10));
            a11 = fma(x1.y, y1.y, fma(x0.y, y0.y, a11));
        }
        __builtin_amdgcn_fence(__ATOMIC_SEQ_CST, "workgroup");
        __builtin_amdgcn_wave_barrier();
    }
    if (t < 55) {
        double *dst = part + (size_t) ri * ASM_PART + 4 * t;
        *reinterpret_cast<double2 *>(dst)     = make_double2(a00, a01);
        *reinterpret_cast<double2 *>(dst + 2) = make_double2(a10, a11);
    }
}

// owner[w * P + a] of a camera column: (local pose << 3) | x for column x of a pose block, (ASM_EXT << 3) | x for the extrinsic (x < 6) and td
// (x == 6), -1 for a column no visual factor of the window touches (host-only blocks, empty tail columns).
// The gathers are chains of additions in a fixed order, but their loads are independent: they are issued eight at a time (a missing run
// contributes +0.0, which leaves every partial sum as it is) — one thread walks up to K^2 runs, and a dependent L2 round trip per run made
// the (ext|td)^2 cells the critical path of the launch.
__device__ __forceinline__ double asm_gather_all(const double *part, int r0, int r1, int idx, double acc) {
    for (int rr = r0; rr < r1; rr += 8) {
        double v[8];
#pragma unroll
        for (int u = 0; u < 8; u++) v[u] = rr + u < r1 ? part[(size_t) (rr + u) * ASM_PART + idx] : 0.0;
#pragma unroll
        for (int u = 0; u < 8; u++) acc += v[u];
    }
    return acc;
}
// every run with local pose p as reference (row p of the pair table, element i_r of the run's block) or as observer (column p, element i_o)
__device__ __forceinline__ double asm_gather_pose(const double *part, const int32_t *pr, int Kmax, int K, int p, int i_r, int i_o, double acc) {
    for (int q = 0; q < K; q += 4) {
        int rr[4], ro[4];
#pragma unroll
        for (int u = 0; u < 4; u++) rr[u] = q + u < K ? pr[p * Kmax + q + u] : -1, ro[u] = q + u < K ? pr[(q + u) * Kmax + p] : -1;
        double vr[4], vo[4];
#pragma unroll
        for (int u = 0; u < 4; u++) vr[u] = rr[u] >= 0 ? part[(size_t) rr[u] * ASM_PART + i_r] : 0.0, vo[u] = ro[u] >= 0 ? part[(size_t) ro[u] * ASM_PART + i_o] : 0.0;
#pragma unroll
        for (int u = 0; u < 4; u++) acc += vr[u], acc += vo[u];
    }
    return acc;
}
// grid (ceil((P * P + P) / 256), W)
__global__ __launch_bounds__(256) void k_asm_camera(const win_desc *wd, const int32_t *run_off, const int32_t *pair_run, int Kmax, const int16_t *owner,
                                                   int P, const double *part, double *sys) {
    const int w       = blockIdx.y;
    const win_desc W = wd[w];
    if (!W.reassemble) return;
    const int e = blockIdx.x * 256 + threadIdx.x;
    if (e >= P * P + P) return;
    const int N          = P + W.L, K = W.K;
    double *H            = sys + W.sys_off, *b = H + (size_t) N * N;
    const int16_t *own   = owner + (size_t) w * P;
    const int32_t *pr    = pair_run + (size_t) w * Kmax * Kmax;
    const int r0 = run_off[w], r1 = run_off[w + 1];
    double acc = 0.0;
    if (e < P * P) {
        const int a = e / P, c = e - a * P;
        const int oa = own[a], oc = own[c];
        if (oa >= 0 && oc >= 0) {
            const int pa = oa >> 3, xa = oa & 7, pc = oc >> 3, xc = oc & 7;
            if (pa == ASM_EXT && pc == ASM_EXT) {
                acc = asm_gather_all(part, r0, r1, asm_part_index(12 + xa, 12 + xc), acc);
            } else if (pa != ASM_EXT && pc != ASM_EXT && pa != pc) {
                const int r_ac = pr[pa * Kmax + pc], r_ca = pr[pc * Kmax + pa];
                const double v_ac = r_ac >= 0 ? part[(size_t) r_ac * ASM_PART + asm_part_index(xa, 6 + xc)] : 0.0;
                const double v_ca = r_ca >= 0 ? part[(size_t) r_ca * ASM_PART + asm_part_index(6 + xa, xc)] : 0.0;
                acc = v_ac + v_ca;
            } else {
                // pose p's diagonal block, or pose p against the shared block
                const int p   = pa != ASM_EXT ? pa : pc;
                const int i_r = asm_part_index(pa == ASM_EXT ? 12 + xa : xa, pc == ASM_EXT ? 12 + xc : xc);         // p is the run's reference
                const int i_o = asm_part_index(pa == ASM_EXT ? 12 + xa : 6 + xa, pc == ASM_EXT ? 12 + xc : 6 + xc); // p is the run's observer
                acc = asm_gather_pose(part, pr, Kmax, K, p, i_r, i_o, acc);
            }
        }
        H[(size_t) a * N + c] = acc;
    } else {
        const int a  = e - P * P;
        const int oa = own[a];
        if (oa >= 0) {
            const int pa = oa >> 3, xa = oa & 7;
            if (pa == ASM_EXT)
                acc = asm_gather_all(part, r0, r1, asm_part_index(12 + xa, 19), acc);
            else
                acc = asm_gather_pose(part, pr, Kmax, K, pa, asm_part_index(xa, 19), asm_part_index(6 + xa, 19), acc);
        }
        b[a] = acc;
    }
}

// Landmark rows.  The P camera columns of a window are cut into blocks (host, per call): the six columns of a free pose, the six of the
// extrinsic, runs of up to six columns that no visual factor touches (stored as zeros), and one block for (td column, h_ll, b_l).  A thread
// owns one (landmark, block) pair and walks the landmark's factors ONCE for the whole block — the first version owned single cells and walked
// them once per column (70 % of its iterations found a pose that is neither the factor's reference nor its observer).  A workgroup owns LB
// consecutive landmarks (LB * blocks <= 256); their factors are one contiguous range of the landmark-major list, staged in LDS 64 at a
// time (J and r of a factor = 48 doubles: ONE round trip of independent coalesced loads per pass instead of the dependent lrec -> J -> J
// chain per cell), then added in list order.  An inactive factor is staged as zeros.
#define ASML_FB 64
#define ASM_BLK_TD 0xFFE  // (td column or 0xFFF = none, h_ll, b_l)
#define ASM_BLK_GAP 0xFFD // columns of host-only blocks: zeros
// blocks[w * NBmax + k] = col0 | width << 12 | code << 16 (code: local pose, ASM_EXT, ASM_BLK_TD, ASM_BLK_GAP); grid (ceil(Lmax / LB), W)
__global__ __launch_bounds__(256) void k_asm_landmarks(const win_desc *wd, const int32_t *blocks, int NBmax, int P, int LB, const int32_t *lm_foff,
                                                      const int4 *lrec, const double *r, const double *J, const uint8_t *active, double *sys) {
    __shared__ double st[ASML_FB * 48];
    __shared__ int st_i[ASML_FB], st_j[ASML_FB];
    const int w       = blockIdx.y;
    const win_desc W = wd[w];
    if (!W.reassemble) return;
    const int l0 = blockIdx.x * LB;
    if (l0 >= W.L) return;
    const int t = threadIdx.x, nl = min(LB, W.L - l0), NB = W.NB;
    const int N = P + W.L;
    double *H   = sys + W.sys_off, *b = H + (size_t) N * N;
    const int il = t / NB, ib = t - il * NB;
    const bool has = il < nl;
    int col0 = 0, width = 0, code = ASM_BLK_GAP, fb = 0, fe = 0;
    if (has) {
        const int blk = blocks[(size_t) w * NBmax + ib];
        col0 = blk & 0xFFF, width = (blk >> 12) & 0xF, code = blk >> 16;
        fb = lm_foff[W.lm_begin + l0 + il], fe = lm_foff[W.lm_begin + l0 + il + 1];
    }
    double acc[6] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    const int f_begin = lm_foff[W.lm_begin + l0], f_end = lm_foff[W.lm_begin + l0 + nl];
    const int fi = t >> 2, sub = t & 3;
    for (int c0 = f_begin; c0 < f_end; c0 += ASML_FB) {
        const int nc = min(ASML_FB, f_end - c0);
        __syncthreads(); // (the previous pass has been consumed)
        if (fi < nc) {
            const int4 rec = lrec[c0 + fi]; // factor, local_i, local_j
            const bool on  = !active || active[rec.x];
            const double *Jf = J + 46 * (size_t) rec.x;
#pragma unroll
            for (int kk = 0; kk < 12; kk++) {
                const int c = sub + 4 * kk;
                st[fi * 48 + c] = on ? (c < 46 ? Jf[c] : r[2 * (size_t) rec.x + (c - 46)]) : 0.0;
            }
            if (sub == 0) st_i[fi] = rec.y, st_j[fi] = rec.z;
        }
        __syncthreads();
        if (code == ASM_BLK_GAP) continue;
        const int g1 = min(fe, c0 + nc) - c0;
        for (int g = max(fb, c0) - c0; g < g1; g++) {
            const double *Jf = &st[g * 48];
            const double jl0 = Jf[42], jl1 = Jf[43];
            if (code == ASM_BLK_TD) {
                acc[0] = fma(jl1, Jf[45], fma(jl0, Jf[44], acc[0]));
                acc[1] = fma(jl1, jl1, fma(jl0, jl0, acc[1]));
                acc[2] = fma(jl1, -Jf[47], fma(jl0, -Jf[46], acc[2]));
                continue;
            }
            int o;
            if (code == ASM_EXT)
                o = 28;
            else if (code == st_i[g])
                o = 0;
            else if (code == st_j[g])
                o = 14;
            else
                continue;
#pragma unroll
            for (int x = 0; x < 6; x++) acc[x] = fma(jl1, Jf[o + 7 + x], fma(jl0, Jf[o + x], acc[x]));
        }
    }
    if (!has) return;
    const int l = l0 + il;
    double *row = H + (size_t) (P + l) * N;
    if (code == ASM_BLK_TD) {
        if (col0 != 0xFFF) row[col0] = acc[0];
        row[P + l] = acc[1];
        b[P + l]   = acc[2];
    } else {
#pragma unroll
        for (int x = 0; x < 6; x++)
            if (x < width) row[col0 + x] = acc[x];
    }
}

// ---- the assembly plan of a partition (host, once per factor set / partition) ---------------------------------------------------------------
static int asm_plan_build(icg_ctx *ctx, icg_partition &pt) {
    const int W = pt.W, n = ctx->n_factors_resident, n_lm = pt.lm_off[(size_t) W];
    icg_asm_plan &pl = pt.plan;
    pt.plan_valid    = false;
    if ((int) ctx->h_fidx.size() != 3 * n) return icg_fail(ctx, ICG_ERR_INVALID, "no resident factors");
    const int32_t *ii = ctx->h_fidx.data(), *jj = ii + n, *ll = jj + n;
    int max_pose = -1;
    for (int f = 0; f < n; f++) {
        if (ii[f] < 0 || jj[f] < 0) return icg_fail(ctx, ICG_ERR_INVALID, "factor %d: negative pose index", f);
        if (ii[f] == jj[f]) return icg_fail(ctx, ICG_ERR_INVALID, "factor %d: reference and observer pose are the same block (%d)", f, ii[f]);
        max_pose = std::max(max_pose, std::max((int) ii[f], (int) jj[f]));
    }
    std::vector<int32_t> pose_win((size_t) (max_pose + 1), -1), g2l((size_t) (max_pose + 1), -1), used;
    std::vector<int32_t> perm((size_t) std::max(n, 1)), runs, lrec(4 * (size_t) std::max(n, 1)), lm_foff((size_t) n_lm + 1, 0), cnt;
    pl.run_off.assign((size_t) W + 1, 0);
    pl.pose_off.assign((size_t) W + 1, 0);
    pl.pose_glob.clear();
    pl.Kmax = 1;
    for (int w = 0; w < W; w++) {
        const int f0 = pt.fac_off[(size_t) w], f1 = pt.fac_off[(size_t) w + 1], l0 = pt.lm_off[(size_t) w], l1 = pt.lm_off[(size_t) w + 1];
        used.clear();
        for (int f = f0; f < f1; f++)
            for (int32_t p : {ii[f], jj[f]}) {
                int32_t &pw = pose_win[(size_t) p];
                if (pw >= 0 && pw != w) return icg_fail(ctx, ICG_ERR_INVALID, "pose %d is used by windows %d and %d", (int) p, (int) pw, w);
                if (pw < 0) pw = w, used.push_back(p);
            }
        std::sort(used.begin(), used.end());
        const int K = (int) used.size();
        if (K >= ASM_EXT) return icg_fail(ctx, ICG_ERR_CAPACITY, "window %d uses %d poses (limit %d)", w, K, ASM_EXT - 1);
        for (int k = 0; k < K; k++) g2l[(size_t) used[(size_t) k]] = k;
        pl.pose_glob.insert(pl.pose_glob.end(), used.begin(), used.end());
        pl.pose_off[(size_t) w + 1] = (int32_t) pl.pose_glob.size();
        pl.Kmax                      = std::max(pl.Kmax, K);
        // runs: stable counting sort of the window's factors by the ordered local pose pair
        cnt.assign((size_t) K * K + 1, 0);
        for (int f = f0; f < f1; f++) cnt[(size_t) g2l[(size_t) ii[f]] * K + g2l[(size_t) jj[f]] + 1]++;
        for (size_t k = 0; k < (size_t) K * K; k++) {
            if (cnt[k + 1] > 0) {
                runs.push_back(f0 + cnt[k]), runs.push_back(cnt[k + 1]);
                runs.push_back((int32_t) (k / (size_t) K) | ((int32_t) (k % (size_t) K) << 16)), runs.push_back(w);
            }
            cnt[k + 1] += cnt[k];
        }
        for (int f = f0; f < f1; f++) perm[(size_t) f0 + (size_t) cnt[(size_t) g2l[(size_t) ii[f]] * K + g2l[(size_t) jj[f]]]++] = f;
        pl.run_off[(size_t) w + 1] = (int32_t) (runs.size() / 4);
        // landmark-major records: stable counting sort by landmark
        for (int f = f0; f < f1; f++) {
            if (ll[f] < l0 || ll[f] >= l1) return icg_fail(ctx, ICG_ERR_INVALID, "factor %d: landmark %d outside its window's range [%d, %d)", f, (int) ll[f], l0, l1);
            lm_foff[(size_t) ll[f] + 1]++;
        }
    }
    for (int l = 0; l < n_lm; l++) lm_foff[(size_t) l + 1] += lm_foff[(size_t) l];
    {
        std::vector<int32_t> pos(lm_foff.begin(), lm_foff.end() - 1);
        for (int w = 0; w < W; w++) {
            // (g2l of a pose is its number inside its own window: poses are not shared between windows)
            for (int f = pt.fac_off[(size_t) w]; f < pt.fac_off[(size_t) w + 1]; f++) {
                int32_t *rec = &lrec[4 * (size_t) pos[(size_t) ll[f]]++];
                rec[0] = f, rec[1] = g2l[(size_t) ii[f]], rec[2] = g2l[(size_t) jj[f]], rec[3] = 0;
            }
        }
    }
    pl.n_runs = (int) (runs.size() / 4);
    std::vector<int32_t> pair_run((size_t) W * pl.Kmax * pl.Kmax, -1);
    for (int k = 0; k < pl.n_runs; k++) {
        const int32_t lilj = runs[4 * (size_t) k + 2], w = runs[4 * (size_t) k + 3];
        pair_run[((size_t) w * pl.Kmax + (size_t) (lilj & 0xFFFF)) * pl.Kmax + (size_t) (lilj >> 16)] = k;
    }
    // one device allocation, 256-byte aligned sections
    ICG_HIP(ctx, hipSetDevice(ctx->cfg.device));
    const size_t b_perm = icg_align_up(sizeof(int32_t) * (size_t) std::max(n, 1), 256), b_runs = icg_align_up(sizeof(int32_t) * std::max<size_t>(runs.size(), 4), 256),
                 b_roff = icg_align_up(sizeof(int32_t) * ((size_t) W + 1), 256), b_pair = icg_align_up(sizeof(int32_t) * pair_run.size(), 256),
                 b_lrec = icg_align_up(sizeof(int32_t) * lrec.size(), 256), b_lmf = icg_align_up(sizeof(int32_t) * lm_foff.size(), 256);
    const size_t total = b_perm + b_runs + b_roff + b_pair + b_lrec + b_lmf;
    if (int rc = icg_grow(ctx, (void **) &pl.d_buf, &pl.buf_cap, total, total + total / 4)) return rc;
    char *p       = pl.d_buf;
    pl.d_perm     = reinterpret_cast<int32_t *>(p), p += b_perm;
    pl.d_runs     = reinterpret_cast<int32_t *>(p), p += b_runs;
    pl.d_run_off  = reinterpret_cast<int32_t *>(p), p += b_roff;
    pl.d_pair_run = reinterpret_cast<int32_t *>(p), p += b_pair;
    pl.d_lrec     = reinterpret_cast<int32_t *>(p), p += b_lrec;
    pl.d_lm_foff  = reinterpret_cast<int32_t *>(p);
    ICG_HIP(ctx, hipStreamSynchronize(ctx->stream)); // (a launch of the previous plan may still read the buffer)
    if (n) ICG_HIP(ctx, hipMemcpyAsync(pl.d_perm, perm.data(), sizeof(int32_t) * (size_t) n, hipMemcpyHostToDevice, ctx->stream));
    if (!runs.empty()) ICG_HIP(ctx, hipMemcpyAsync(pl.d_runs, runs.data(), sizeof(int32_t) * runs.size(), hipMemcpyHostToDevice, ctx->stream));
    ICG_HIP(ctx, hipMemcpyAsync(pl.d_run_off, pl.run_off.data(), sizeof(int32_t) * ((size_t) W + 1), hipMemcpyHostToDevice, ctx->stream));
    if (!pair_run.empty()) ICG_HIP(ctx, hipMemcpyAsync(pl.d_pair_run, pair_run.data(), sizeof(int32_t) * pair_run.size(), hipMemcpyHostToDevice, ctx->stream));
    if (n) ICG_HIP(ctx, hipMemcpyAsync(pl.d_lrec, lrec.data(), sizeof(int32_t) * 4 * (size_t) n, hipMemcpyHostToDevice, ctx->stream));
    ICG_HIP(ctx, hipMemcpyAsync(pl.d_lm_foff, lm_foff.data(), sizeof(int32_t) * lm_foff.size(), hipMemcpyHostToDevice, ctx->stream));
    const size_t part = (size_t) pl.n_runs * ASM_PART;
    if (int rc = icg_grow(ctx, (void **) &pl.d_part, &pl.part_cap, sizeof(double) * part, sizeof(double) * (part + part / 4))) return rc;
    ICG_HIP(ctx, hipStreamSynchronize(ctx->stream)); // (the host vectors go out of scope)
    pt.plan_valid = true;
    return ICG_OK;
}

int icg_asm_single_partition(icg_ctx *ctx, int n_lm) {
    icg_partition &pt = ctx->part_1;
    const int n       = ctx->n_factors_resident;
    if (pt.plan_valid && pt.W == 1 && pt.fac_off[1] == n && pt.lm_off[1] == n_lm) return ICG_OK;
    pt.W = 1;
    pt.fac_off = {0, n}, pt.lm_off = {0, n_lm};
    pt.sys_valid = 0;
    return asm_plan_build(ctx, pt);
}

// owner of every camera column of every window (k_asm_camera), and the column blocks of the landmark rows (k_asm_landmarks): owned blocks
// start where their owner's column 0 sits, unowned columns in runs of up to six
int icg_asm_columns_build(icg_ctx *ctx, const icg_partition &pt, int P, const int32_t *col_pose, const int32_t *col_ext, const int32_t *col_td,
                          std::vector<win_desc> &wd, icg_asm_columns &cols) {
    const int W            = pt.W;
    const icg_asm_plan &pl = pt.plan;
    int rc;
    std::vector<int16_t> &owner = cols.owner;
    owner.assign((size_t) W * P, (int16_t) -1);
    for (int w = 0; w < W; w++) {
        int16_t *ow = &owner[(size_t) w * P];
        auto claim  = [&](int col, int width, int code, const char *what) -> int {
            if (col < 0) return 0;
            if (col + width > P) return icg_fail(ctx, ICG_ERR_INVALID, "window %d: %s column %d outside the reduced system (%d)", w, what, col, P);
            for (int x = 0; x < width; x++) {
                if (ow[col + x] != -1) return icg_fail(ctx, ICG_ERR_INVALID, "window %d: camera column %d is claimed by two blocks", w, col + x);
                ow[col + x] = (int16_t) ((code << 3) | (code == ASM_EXT && width == 1 ? 6 : x));
            }
            return 0;
        };
        for (int k = pl.pose_off[(size_t) w]; k < pl.pose_off[(size_t) w + 1]; k++) {
            const int g = pl.pose_glob[(size_t) k];
            if (g >= ctx->last_n_poses) return icg_fail(ctx, ICG_ERR_INVALID, "pose %d of the factors is beyond the %d evaluated poses", g, ctx->last_n_poses);
            if ((rc = claim(col_pose[g], 6, k - pl.pose_off[(size_t) w], "pose"))) return rc;
        }
        if ((rc = claim(col_ext[w], 6, ASM_EXT, "extrinsic"))) return rc;
        if ((rc = claim(col_td[w], 1, ASM_EXT, "td"))) return rc;
    }
    std::vector<std::vector<int32_t>> blk((size_t) W);
    int NBmax = 1;
    for (int w = 0; w < W; w++) {
        const int16_t *ow = &owner[(size_t) w * P];
        std::vector<int32_t> &B = blk[(size_t) w];
        for (int a = 0; a < P;) {
            const int o = ow[a];
            if (o < 0) {
                int wdt = 1;
                while (a + wdt < P && wdt < 6 && ow[a + wdt] < 0) wdt++;
                B.push_back(a | (wdt << 12) | (ASM_BLK_GAP << 16));
                a += wdt;
            } else if ((o >> 3) == ASM_EXT && (o & 7) == 6) {
                a += 1; // td: part of the (td, h_ll, b_l) block below
            } else {
                B.push_back(a | (6 << 12) | ((o >> 3) << 16)); // (claim() laid the six columns of a pose / the extrinsic down contiguously)
                a += 6;
            }
        }
        B.push_back((col_td[w] >= 0 ? col_td[w] : 0xFFF) | (1 << 12) | (ASM_BLK_TD << 16));
        wd[(size_t) w].NB = (int32_t) B.size();
        NBmax             = std::max(NBmax, (int) B.size());
    }
    if (NBmax > 256) return icg_fail(ctx, ICG_ERR_CAPACITY, "a window's camera columns fall into %d blocks (limit 256)", NBmax);
    cols.NBmax = NBmax;
    cols.blocks.assign((size_t) W * NBmax, 0);
    for (int w = 0; w < W; w++) std::copy(blk[(size_t) w].begin(), blk[(size_t) w].end(), cols.blocks.begin() + (size_t) w * NBmax);
    return ICG_OK;
}

void icg_asm_enqueue(icg_ctx *ctx, const icg_partition &pt, int P, int NBmax, const win_desc *d_wd, const int16_t *d_owner, const int32_t *d_blocks,
                     const uint8_t *d_active) {
    const icg_asm_plan &pl = pt.plan;
    const double *d_r = ctx->d_rJ, *d_J = icg_resident_J(ctx);
    const int W = pt.W, Lmax = icg_partition_Lmax(pt);
    icg_prof_scope ps(ctx, "reproj_normal");
    if (pl.n_runs > 0)
        hipLaunchKernelGGL(k_asm_runs, dim3((unsigned) ((pl.n_runs + 3) / 4)), dim3(256), 0, ctx->stream, pl.n_runs, reinterpret_cast<const int4 *>(pl.d_runs),
                           d_wd, (const int32_t *) pl.d_perm, d_r, d_J, d_active, pl.d_part);
    hipLaunchKernelGGL(k_asm_camera, dim3((unsigned) ((P * P + P + 255) / 256), W), dim3(256), 0, ctx->stream, d_wd, (const int32_t *) pl.d_run_off,
                       (const int32_t *) pl.d_pair_run, pl.Kmax, d_owner, P, (const double *) pl.d_part, ctx->d_sys);
    const int LB = std::max(1, 256 / NBmax); // landmarks per workgroup: one (landmark, block) pair per thread
    hipLaunchKernelGGL(k_asm_landmarks, dim3((unsigned) ((Lmax + LB - 1) / LB), W), dim3(256), 0, ctx->stream, d_wd, d_blocks, NBmax, P, LB,
                       (const int32_t *) pl.d_lm_foff, reinterpret_cast<const int4 *>(pl.d_lrec), d_r, d_J, d_active, ctx->d_sys);
}

// ---- f1, many windows per launch ------------------------------------------------------------------------------------------------
// One solver in flight per stream is bounded by the runtime's rate of small launches and copies (~100 per window and solve, DESIGN.md
// §6).  Here the windows of many streams advance in lock-step: ONE evaluation, ONE assembly, ONE reduction, ONE back-substitution
// call per LM step for all of them.  The resident factor set is partitioned into W windows (factors sorted by window, landmarks
// contiguous per window, poses indexed globally); every window has its own extrinsic / td, its own reduced system of the common
// size P and its own damping.  Window w's system lives at d_sys + sys_off[w]: H (N_w x N_w, N_w = P + L_w) | b (N_w) | inv (L_w).
extern "C" int icg_reproj_set_windows(icg_ctx *ctx, int n_windows, const int32_t *fac_off, const int32_t *lm_off) {
    if (!ctx || n_windows <= 0 || !fac_off || !lm_off) return ICG_ERR_INVALID;
    const int n = ctx->n_factors_resident;
    if (fac_off[0] != 0 || fac_off[n_windows] != n) return icg_fail(ctx, ICG_ERR_INVALID, "fac_off must cover the %d resident factors", n);
    if (lm_off[0] != 0) return icg_fail(ctx, ICG_ERR_INVALID, "lm_off must start at 0");
    for (int w = 0; w < n_windows; w++)
        if (fac_off[w + 1] < fac_off[w] || lm_off[w + 1] < lm_off[w]) return icg_fail(ctx, ICG_ERR_INVALID, "window %d: offsets not monotone", w);
    ICG_HIP(ctx, hipSetDevice(ctx->cfg.device));
    const int n_lm = lm_off[n_windows];
    if (int rc = icg_grow(ctx, (void **) &ctx->d_lmwin, &ctx->lmwin_cap, sizeof(int32_t) * (size_t) n_lm, sizeof(int32_t) * (size_t) (n_lm + n_lm / 4 + 64))) return rc;
    std::vector<int32_t> fwin((size_t) n), lwin((size_t) std::max(n_lm, 1));
    for (int w = 0; w < n_windows; w++) {
        for (int f = fac_off[w]; f < fac_off[w + 1]; f++) fwin[(size_t) f] = w;
        for (int l = lm_off[w]; l < lm_off[w + 1]; l++) lwin[(size_t) l] = w;
    }
    if (n) ICG_HIP(ctx, hipMemcpyAsync(ctx->d_fwin, fwin.data(), sizeof(int32_t) * (size_t) n, hipMemcpyHostToDevice, ctx->stream));
    if (n_lm) ICG_HIP(ctx, hipMemcpyAsync(ctx->d_lmwin, lwin.data(), sizeof(int32_t) * (size_t) n_lm, hipMemcpyHostToDevice, ctx->stream));
    ICG_HIP(ctx, hipStreamSynchronize(ctx->stream));
    icg_partition &pt = ctx->part_w;
    pt.W              = n_windows;
    pt.fac_off.assign(fac_off, fac_off + n_windows + 1);
    pt.lm_off.assign(lm_off, lm_off + n_windows + 1);
    pt.sys_valid = 0;
    ctx->red_W   = 0; // (the resident reduced systems and host parts belonged to the partition that is replaced)
    icg_red_drop_host_parts(ctx, 0);
    const auto t0 = std::chrono::steady_clock::now();
    int rc       = asm_plan_build(ctx, pt);
    if (rc) pt.W = 0;
    if (getenv("ICG_ABI_DEBUG"))
        fprintf(stderr, "[icg_reproj_set_windows] W=%d n=%d: assembly plan %.3f ms\n", n_windows, n,
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
    return rc;
}
