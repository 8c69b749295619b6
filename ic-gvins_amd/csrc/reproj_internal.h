// What the three translation units of the reprojection back-end share (host side only: a kernel is launched from the file that defines it):
//   reproj.hip        R1/R2  k_reproj_eval, the resident factor set and its evaluation (one window / many windows), chi-square culling
//   reproj_asm.hip    M2/f1  the partition of the factors into windows, its assembly plan and the fixed-order assembly k_asm_*
//   reproj_schur.hip  f1     landmark elimination, back-substitution, cost and the reduced camera solve: the Schur entry points
#pragma once
#include <algorithm>

#include "icg_internal.h"

// one window of a partition as the kernels see it
struct win_desc {
    int32_t fac_begin, fac_end, lm_begin, L;
    int64_t sys_off;
    int32_t K, reassemble; // K: poses used by the window's factors (local numbering of the plan)
    double damp;
    int32_t NB, pad; // column blocks of the landmark rows (k_asm_landmarks)
};

// the resident results of the last evaluation: r (n x 2) at d_rJ, J (n x 46) behind the residuals of a full buffer
static inline double *icg_resident_J(const icg_ctx *ctx) { return ctx->d_rJ + 2 * (size_t) ctx->factors_cap; }

// the most landmarks a window of the partition has (at least 1): what the per-landmark grids are sized by
static inline int icg_partition_Lmax(const icg_partition &pt) {
    int Lmax = 1;
    for (int w = 0; w < pt.W; w++) Lmax = std::max(Lmax, (int) (pt.lm_off[(size_t) w + 1] - pt.lm_off[(size_t) w]));
    return Lmax;
}

// ---- reproj_asm.hip -------------------------------------------------------------------------------------------------------------------------
// the implicit partition behind the single-window entry points: every resident factor, landmarks 0 .. n_lm - 1
int icg_asm_single_partition(icg_ctx *ctx, int n_lm);
// Where the camera columns of every window's reduced system (width P) come from.  owner (W x P) is what k_asm_camera reads, blocks
// (W x NBmax, wd[w].NB of them used) what k_asm_landmarks reads; fails for columns outside the system or claimed twice.
struct icg_asm_columns {
    std::vector<int16_t> owner;
    std::vector<int32_t> blocks;
    int NBmax = 1;
};
int icg_asm_columns_build(icg_ctx *ctx, const icg_partition &pt, int P, const int32_t *col_pose, const int32_t *col_ext, const int32_t *col_td,
                          std::vector<win_desc> &wd, icg_asm_columns &cols);
// enqueues k_asm_runs, k_asm_camera, k_asm_landmarks for the windows of wd with reassemble != 0: their (H | b) in ctx->d_sys from the resident r, J
void icg_asm_enqueue(icg_ctx *ctx, const icg_partition &pt, int P, int NBmax, const win_desc *d_wd, const int16_t *d_owner, const int32_t *d_blocks,
                     const uint8_t *d_active);

// ---- reproj_schur.hip -----------------------------------------------------------------------------------------------------------------------
// a device buffer of the reduced camera solve (d_red_S, d_red_H) for `bytes`, grown without keeping its contents: a replaced buffer drops the
// resident reduced systems and every window's host part
int icg_red_ensure_capacity(icg_ctx *ctx, double **buf, size_t *cap, size_t bytes);
