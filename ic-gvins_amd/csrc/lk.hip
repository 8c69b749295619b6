// F2/F3: pyramidal Lucas-Kanade exactly as cv::calcOpticalFlowPyrLK is parameterised by the reference
// (tracking/tracking.cc:385-393, 487-496: win 21x21, maxLevel 3, (COUNT+EPS,30,0.01), USE_INITIAL_FLOW,
// minEigThreshold 1e-4), plus the forward/backward/border cull of tracking.cc:396-403 / 499-506.
// Arithmetic definition: SURVEY.md Appendix B.4/B.5 (OpenCV LKTrackerInvoker): Q14 bilinear weights, patch samples
// with 5 fractional bits, Scharr derivatives, window sums accumulated as EXACT integers (wave-reduced in int64), one
// conversion to float, 2x2 solve in float without FMA contraction -> bit-identical to the CPU restatement.
//
// MI355X mapping: ONE 64-lane wavefront per feature (one workgroup = one wave, so LDS staging needs no cross-wave
// barrier and thousands of features from many camera streams fill the 256 CUs).
//   * per level the 24x24 u8 neighbourhood of the previous image is staged in LDS (reflect-101 applied at load),
//     Scharr derivatives of the 22x22 support are computed ON THE FLY into LDS (the derivative planes are never
//     materialised in HBM: -5.3 B/px of traffic per frame vs OpenCV's layout),
//   * each lane owns a 7-pixel horizontal run of the 21x21 window (63 lanes x 7 = 441): it reads its 4x10-byte patch of
//     the staged tile as aligned dwords (+ v_alignbyte), computes its Scharr derivatives and I/Ix/Iy samples in
//     registers and keeps them there for all <=30 Gauss-Newton iterations,
//   * the next image is read through a 32x32 u8 LDS tile (re-staged only when the window leaves it); the lane's 2x8
//     bytes of it are CACHED IN REGISTERS and re-fetched only when the integer window position changes, so a typical
//     iteration touches no LDS at all (v1 spent 39% of its wave cycles in LDS issue stalls: rocprofv3 SQ_WAIT_INST_LDS),
//   * A11/A12/A22 and b1/b2 are per-lane int32 partials (bounded: 7*4080^2 < 2^27, 7*8160*4080 < 2^28) reduced exactly:
//     DPP butterflies in 32 bits up to 16 / 8 lanes, then 16-bit halves through row_mirror/row_bcast DPP stages;
//   * the kernel is VALU-issue bound (rocprofv3: ~11k VALU instructions per point in v2), so the integer math is packed:
//     pixels, Scharr terms and Q14 weights all fit 16 bits -> v_pk_{add,sub,mul_lo}_u16 for the derivative stencil and
//     v_dot2_i32_i16 for every bilinear blend (2 taps per instruction) and for the window products; the patch sample is
//     folded into the blend's rounding constant (c0 = 256 - 512*I) so a residual costs 2 dot2 + 1 shift.
//   * (round 6) the Scharr terms carry a factor 4 so that a blended derivative is the HIGH half of its dot2 result (packed by one v_perm, no
//     shift); the three window sums of a level come out of one reduction tree (v_permlane32_swap + v_permlane16_swap); the eigenvalue test
//     needs no division (threshold on the numerator) and the square root no range scaling; the verdict on a point (border, forward-backward
//     distance, undistortion: FP64 that every lane of the wave computed alike) is k_lk_finish's, a thread per point.
//     6.3 k vector instructions per tracked point (7.1 k in rounds 4-5), 93 VGPRs, no scratch, 5 waves per SIMD.
//   * (round 7) the level set-up of a window whose 22x22 support lies inside the level differentiates the BLENDED patch: the Q14 blend and the
//     Scharr stencil are integer linear maps and the descale is the only rounding, so the wave blends the 23x23 grid once (B, 32 bits, through
//     LDS: two v_perm + two v_dot2 per position) and every lane runs a separable 32-bit Scharr (v_mad_i32_i24) over its 3x9 piece of B — the
//     same bits as blending Ix, Iy and I separately (tests/test_lk_blend_first_identity.py pins the algebra).  Windows over a border keep the
//     packed 16-bit form above, where the derivative plane is masked to zero outside the image.
//   * (round 9) the uniform and address work around that arithmetic: the level scale 2^-level from its bit pattern (was an FP64 division per
//     level and pass), tile loads inside a level by the level's scalar base + ONE 32-bit lane offset (lk_offset: a 24-bit multiply; bound checked by
//     icg_ctx_create) instead of a 64-bit address per lane, the segment decode by icg_div_magic.  5.73 k vector instructions per tracked point,
//     93 VGPRs, no scratch, 5 waves per SIMD (profiles/r09_uniform_prologues.txt).
//   * (round 10) tile loads over a border of a level: 3.05 of the 16 tile loads of a point cross one on the bench's frames (a third of them a column
//     border).  They were a reflect-101 loop, a 64-bit address, a byte load and a shift-or per pixel outside — unrolled at three call sites, 60 % of
//     the kernel's text.  On levels of at least LK_JT x LK_JT a single reflection is a closed form, and a dword with mirrored pixels is ONE unaligned
//     dword load inside the row and one v_perm (lk_load4_mirror, as k_pyrdown_rows' edge waves do), and a tile over a row border only is plain
//     dwords from mirrored rows; smaller levels, which only tests build, go through two loops that are not unrolled (lk_stage_small).
//     5.60 k vector instructions per tracked point, scalar instructions -7 %, 15 856 -> 10 928 bytes of text, no global_load_ubyte and no 64-bit
//     lane address outside lk_stage_small, 93 VGPRs, no scratch, 5 waves per SIMD (profiles/r10_lk_border_tiles.txt).
//   * (round 13) the pixel pairs of the two Q14 blends that read two adjacent rows are taken VERTICALLY: with VP[c] = (row r, row r + 1) at
//     column c and the weights packed by columns, Wl = (w00, w10), Wr = (w01, w11), a blend is dot2(VP[k+1], Wr, dot2(VP[k], Wl, c)) — the same
//     four products and the same 32-bit sum as with the horizontal pairs (tests/test_lk_vertical_pairs_identity.py), and neighbouring positions
//     share a pair: the lane's 7 pixels of an iteration need 8 pairs instead of 14 (lk_fetch_J: 8 v_perm per fetch and 8 registers held through
//     the iterations), the 12 positions of an interior set-up lane 13 instead of 24.  The border set-up keeps its horizontal pairs (converted, it
//     pays in v_perm what it saves in v_alignbit).  The iteration's tail: the level's result is formed once behind the loops, not in every
//     iteration; one compare decides "not converged" on the common path; the previous step is one packed register.  85 vector instructions per
//     iteration in the text (92 before), 87 VGPRs in both kernels (k_lk_track: 100 before, now 5 waves per SIMD too), no scratch
//     (profiles/r13_lk_vertical_pairs.txt: fetches, set-ups and iterations per point, counters and times against round 12).
// Algorithmic HBM bytes per point and direction: 4 levels x (24^2 + 22^2) B; everything else is
// LDS/VGPR traffic.
#include <cfloat>
#if defined(LK_TILE_HIST)
#include <cstdio>
#include <cstdlib>
#include <mutex>
#endif

#include "dev_camera.h"
#include "icg_internal.h"

using namespace icgd;

#define LK_IT 24   // I tile side (22 support + 1 halo each side)
#define LK_IS 28   // I tile row stride in bytes (7 dwords: every lane reads 4 aligned dwords per row)
#define LK_JT 32   // J tile side
#define LK_JS 36   // J tile row stride in bytes (9 dwords: 3 aligned dwords cover any 8-byte run)
#define LK_JM 5    // J tile margin around the 22x22 support
#define LK_BW 28   // B plane row stride in dwords (23 columns; 16-byte rows for the four-dword stores of the blend)
#define LK_BH 26   // B plane rows: 23 blended rows + 3 rows of zeros that lane 63 differentiates (it owns no pixels)
#define LK_MAX_ITERS 30
#ifndef LK_WAVES_PER_EU
#define LK_WAVES_PER_EU 5 // second __launch_bounds__ argument of k_lk_track_fb (the resource remarks of the build are quoted in DESIGN.md section 4)
#endif

struct lk_smem {
    unsigned int I[LK_IT * LK_IS / 4];
    unsigned int J[LK_JT * LK_JS / 4 + 1];
    int B[LK_BH * LK_BW] __attribute__((aligned(16))); // the unrounded Q14 blend of the I tile (+ 256), interior windows only
};

// Exact wave-wide integer sums.  The per-lane partials are bounded (see the kernel comment), so the first butterfly
// stages run in 32 bits as fused DPP adds (quad_perm xor1, xor2, row_half_mirror[, row_mirror]).
__device__ __forceinline__ int dpp_add_xor1(int v) { return v + __builtin_amdgcn_update_dpp(0, v, 0xB1, 0xF, 0xF, false); }
__device__ __forceinline__ int dpp_add_xor2(int v) { return v + __builtin_amdgcn_update_dpp(0, v, 0x4E, 0xF, 0xF, false); }
__device__ __forceinline__ int dpp_add_half_mirror(int v) { return v + __builtin_amdgcn_update_dpp(0, v, 0x141, 0xF, 0xF, false); }
__device__ __forceinline__ int dpp_add_mirror(int v) { return v + __builtin_amdgcn_update_dpp(0, v, 0x140, 0xF, 0xF, false); }

// Exact wave-wide sum of bounded int32 partials, returned as (float) of the exact integer (what the CPU restatement's
// (float)(int64 sum) produces).  Stages: 32-bit DPP butterflies while the group sums still fit int32 (8 lanes for
// |partial| <= 2^28, 16 lanes for <= 2^27); the group sums are then split into a signed high and an unsigned low 16-bit
// half, which both survive the remaining cross-row stages (row_mirror / row_bcast15 / row_bcast31, one fused
// v_add_u32_dpp each) without overflow; lane 63 holds both totals, hi*65536 + lo is formed exactly in double and one
// v_cvt_f32_f64 rounds once (RNE) like i64->f32.  No scalar carry chains, no 64-bit DPP moves.
// (round 5) the totals are combined in f32, not f64: |hi| < 2^24 and lo < 2^24 convert exactly, hi * 65536 is exact, and the one rounding of
// the fused multiply-add is RNE of the exact integer hi * 65536 + lo — what i64 -> f32 gives.  Two conversions + one v_fma on the lane that
// holds the totals, ONE v_readlane of the result (was: two readlanes, two v_cvt_f64_i32, v_ldexp_f64, v_add_f64, v_cvt_f32_f64).
__device__ __forceinline__ float lk_combine_f32(int hi, int lo) { return __builtin_fmaf((float) hi, 65536.f, (float) lo); }
__device__ __forceinline__ float lk_readlane_f32(float v, int lane) {
    return __int_as_float(__builtin_amdgcn_readlane(__float_as_int(v), lane));
}
__device__ __forceinline__ float wave_sum_tail_f32(int hi, int lo) {
    hi += __builtin_amdgcn_update_dpp(0, hi, 0x142, 0xA, 0xF, false); // row_bcast15: rows 1,3 += lane 15 of rows 0,2
    lo += __builtin_amdgcn_update_dpp(0, lo, 0x142, 0xA, 0xF, false);
    hi += __builtin_amdgcn_update_dpp(0, hi, 0x143, 0xC, 0xF, false); // row_bcast31: rows 2,3 += lane 31
    lo += __builtin_amdgcn_update_dpp(0, lo, 0x143, 0xC, 0xF, false);
    return lk_readlane_f32(lk_combine_f32(hi, lo), 63);
}
// |per-lane partial| <= 2^28: sums of 8 lanes fit in int32
__device__ __forceinline__ float wave_sum_i32x8_f32(int v) {
    v = dpp_add_xor1(v);
    v = dpp_add_xor2(v);
    v = dpp_add_half_mirror(v);
    int hi = v >> 16, lo = v & 0xffff;
    hi     = dpp_add_mirror(hi);
    lo     = dpp_add_mirror(lo);
    return wave_sum_tail_f32(hi, lo);
}
// |per-lane partial| <= 2^27: sums of 16 lanes fit in int32
__device__ __forceinline__ float wave_sum_i32x16_f32(int v) {
    v = dpp_add_xor1(v);
    v = dpp_add_xor2(v);
    v = dpp_add_half_mirror(v);
    v = dpp_add_mirror(v);
    return wave_sum_tail_f32(v >> 16, v & 0xffff);
}

// TWO exact wave-wide sums from ONE reduction tree (round 5).  v_permlane32_swap (gfx950) exchanges the upper half of the first register with
// the lower half of the second: one add later lanes 0..31 hold the 2-lane sums of v1 and lanes 32..63 those of v2, and every further DPP
// stage works on both values at once; lane 31 ends with the total of v1, lane 63 with the total of v2.
typedef unsigned int lk_u2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ int lk_fold32(int v1, int v2) {
    const lk_u2 r = __builtin_amdgcn_permlane32_swap((unsigned int) v1, (unsigned int) v2, false, false);
    return (int) (r.x + r.y);
}
__device__ __forceinline__ void wave_sum2_finish_f32(int hi, int lo, float &f1, float &f2) {
    hi += __builtin_amdgcn_update_dpp(0, hi, 0x142, 0xA, 0xF, false); // row_bcast15: lanes 31 / 63 = totals of lanes 0..31 / 32..63
    lo += __builtin_amdgcn_update_dpp(0, lo, 0x142, 0xA, 0xF, false);
    const float t = lk_combine_f32(hi, lo);
    f1 = lk_readlane_f32(t, 31);
    f2 = lk_readlane_f32(t, 63);
}
// |per-lane partial| <= 2^28: sums of 8 lanes fit in int32
__device__ __forceinline__ void wave_sum2_i32x8_f32(int v1, int v2, float &f1, float &f2) {
    int v = lk_fold32(v1, v2);
    v     = dpp_add_xor1(v);
    v     = dpp_add_xor2(v);
    int hi = v >> 16, lo = v & 0xffff;
    hi     = dpp_add_half_mirror(hi);
    lo     = dpp_add_half_mirror(lo);
    hi     = dpp_add_mirror(hi);
    lo     = dpp_add_mirror(lo);
    wave_sum2_finish_f32(hi, lo, f1, f2);
}
// |per-lane partial| <= 2^27: sums of 16 lanes fit in int32
__device__ __forceinline__ void wave_sum2_i32x16_f32(int v1, int v2, float &f1, float &f2) {
    int v = lk_fold32(v1, v2);
    v     = dpp_add_xor1(v);
    v     = dpp_add_xor2(v);
    v     = dpp_add_half_mirror(v);
    int hi = v >> 16, lo = v & 0xffff;
    hi     = dpp_add_mirror(hi);
    lo     = dpp_add_mirror(lo);
    wave_sum2_finish_f32(hi, lo, f1, f2);
}

// THREE exact wave-wide sums from ONE reduction tree (round 6): after v_permlane32_swap has put v1 | v2 and v3 | 0 side by side,
// v_permlane16_swap (gfx950) interleaves the two registers by rows of 16 lanes — row 0 carries v1, row 1 v3, row 2 v2 — and the four DPP
// stages that are left work on all of them at once; every lane of a row ends with the total of its row.  20 instructions for the three
// window sums of the level set-up (were 31).  |per-lane partial| <= 2^27: sums of 16 lanes fit in int32.
__device__ __forceinline__ void wave_sum3_i32x16_f32(int v1, int v2, int v3, float &f1, float &f2, float &f3) {
    const int x       = lk_fold32(v1, v2); // lanes 0..31: 2-lane sums of v1, lanes 32..63: of v2
    const int y       = lk_fold32(v3, 0);  // lanes 0..31: 2-lane sums of v3, lanes 32..63: 0
    const lk_u2 r     = __builtin_amdgcn_permlane16_swap((unsigned int) x, (unsigned int) y, false, false); // odd rows of x <-> even rows of y
    int v             = (int) (r.x + r.y); // rows: v1, v3, v2, 0 (4-lane sums)
    v                 = dpp_add_xor1(v);
    v                 = dpp_add_xor2(v);   // 16-lane sums
    int hi = v >> 16, lo = v & 0xffff;
    hi                = dpp_add_half_mirror(hi);
    lo                = dpp_add_half_mirror(lo);
    hi                = dpp_add_mirror(hi);
    lo                = dpp_add_mirror(lo);
    const float t     = lk_combine_f32(hi, lo);
    f1                = lk_readlane_f32(t, 0);
    f3                = lk_readlane_f32(t, 16);
    f2                = lk_readlane_f32(t, 32);
}

__device__ __forceinline__ int lk_descale(int v, int n) { return (v + (1 << (n - 1))) >> n; }

// The Q14 weights as the packed pairs the blends consume, W0 = (w00, w01), W1 = (w10, w11) (round 5).  rint() by the magic constant: for
// 0 <= x < 2^22 the low 16 bits of bits(x + 1.5 * 2^23) are rint(x) (the addition rounds to nearest even on an integer grid and the
// constant is even) — one full-rate v_add_f32 instead of v_rndne_f32 + v_cvt_i32_f32; w11 = 2^14 - w00 - w01 - w10 is formed on the biased
// bit patterns modulo 2^16 (the three biases 0x4B400000 have zero low halves) and v_perm picks the low halves.  Same weights, bit for bit.
// (round 13) VERTICAL = true packs the same four weights by columns, Wl = (w00, w10), Wr = (w01, w11), for the blends that consume vertical
// pixel pairs (lk_fetch_J, the interior set-up): the same two v_perm with other operands.
template <bool VERTICAL = false>
__device__ __forceinline__ void lk_weights_pk(float a, float b, unsigned int &W0, unsigned int &W1) {
    const float A = a * (float) (1 << 14), A1 = (float) (1 << 14) - A, b1 = 1.f - b;
    const unsigned int r00 = __float_as_uint(A1 * b1 + 12582912.f), r01 = __float_as_uint(A * b1 + 12582912.f);
    const unsigned int r10 = __float_as_uint(A1 * b + 12582912.f);
    const unsigned int r11 = 0x4000u - (r00 + r01 + r10);
    W0 = __builtin_amdgcn_perm(VERTICAL ? r10 : r01, r00, 0x05040100u);
    W1 = __builtin_amdgcn_perm(r11, VERTICAL ? r01 : r10, 0x05040100u);
}

__device__ __forceinline__ void lk_weights(float a, float b, int &w00, int &w01, int &w10, int &w11) {
    // rint((1-a)(1-b) 2^14) etc.; the power-of-two scale commutes with every rounding, so it is applied to a once:
    // fl(fl(1-a) fl(1-b)) 2^14 == fl((2^14 - a 2^14) fl(1-b))   (bit-identical, 8 fewer VALU ops per iteration)
    const float A = a * (float) (1 << 14), A1 = (float) (1 << 14) - A, b1 = 1.f - b;
    w00 = (int) rintf(A1 * b1);
    w01 = (int) rintf(A * b1);
    w10 = (int) rintf(A1 * b);
    w11 = (1 << 14) - w00 - w01 - w10;
}

__device__ __forceinline__ int lk_byte(unsigned int w, int k) { return (int) ((w >> (8 * k)) & 0xffu); }

typedef unsigned int __attribute__((aligned(1))) lk_u32u;

// Byte offset of (row, col) inside a level for the tile loads (round 9; round 10: the mirrored loads over a border too): the level's base pointer is wave-uniform
// and stays in scalar registers, the lane adds ONE 32-bit offset — global_load with a scalar base and a vector offset — instead of a 64-bit
// address of its own (two v_mad_u64_u32, two v_lshl_add_u64 and the moves between them per load).  0 <= row < h and 0 <= col < pitch on
// these paths, and icg_ctx_create admits only layouts with h, pitch < 2^24 and pitch * h < 2^31: the 24-bit multiply-add is exact.
__device__ __forceinline__ unsigned int lk_offset(int row, int pitch, int col) {
    return __umul24((unsigned int) row, (unsigned int) pitch) + (unsigned int) col;
}

// ---- tile loads over a level's border (round 10) ----
// A window the kernel accepts has -ICG_LK_WIN <= ipx, inx <= W - 1 (and the same on rows: the range tests of lk_track_wave).  The I tile starts
// one pixel before ipx and is LK_IT wide: it reaches at most ICG_LK_WIN + 1 = 22 positions outside the level on either side.  The J tile
// starts LK_JM before inx and is LK_JT wide: columns inx - 5 .. inx + 26, at most ICG_LK_WIN + LK_JM = 26 positions outside.  On a level with
// W - 1 >= 26 ONE reflection therefore lands inside — |c| <= 26 <= W - 1 on the left, 2 (W - 1) - c >= W - 27 >= 0 on the right — and
// reflect-101 is the closed form r(c) = (W - 1) - |(W - 1) - |c|| (lk_mirror).  Levels of at least LK_JT on both sides take this form;
// smaller ones, which only tests build, keep the general loops (lk_stage_small).
static_assert(LK_JT >= ICG_LK_WIN + LK_JM + 1, "one reflection must land inside every level that takes the closed-form border path");
static_assert(LK_IT - 1 - 1 <= LK_JT - 1 - LK_JM, "the I tile reaches no further outside a level than the J tile");
__device__ __forceinline__ int lk_mirror(int c, int n) { return (n - 1) - abs((n - 1) - abs(c)); }

// The dword of image columns x .. x + 3 of one row under reflect-101, from ONE unaligned dword load that lies inside the row and one v_perm.
// The load starts at s = clamp(x, 0, W - 4) when at most two of the columns are outside (x in [-2, W - 2]) and at the mirror image of the
// dword's last column, r(x + 3) = -3 - x or 2 W - 5 - x, when three or four are (the bytes then come out reversed).  One expression gives all
// three without a compare: s = min(max(min(x, 2 W - 5 - x), 0, -3 - x), W - 4) — 2 W - 5 - x is below x only right of column W - 2, -3 - x is
// positive only left of column -2 — and its outer clamp holds for EVERY x, so no load starts before column 0 or ends after column W - 1.
// The selector is the 4-byte window at offset o = x - s + 2, at most 5, of the byte sequence 2 1 0 1 2 3 2 1 (0) — a dword mirrored at both
// of its ends; the ninth byte is the zero a right shift fills in: o = 0 and 1 are the straddles of column 0 (x = -2: bytes 2 1 0 1, x = -1:
// 1 0 1 2), o = 2 the identity, o = 3 and 4 the straddles of column W - 1 (x = W - 3: 1 2 3 2, x = W - 2: 2 3 2 1), o = 5 the reversed dword
// 3 2 1 0 (x - s is 2 x + 3 <= -3 on the left, a huge unsigned number, and 2 (x - W) + 5 >= 3 on the right).  Straight-line code, the same
// for every lane, no loop and no byte load; tests/test_lk_mirror_dword.py restates it against a per-byte reflect-101.  The load and the
// v_perm are two calls: the loads of a tile are issued together and permuted together (lk_mirror_apply) before the load function returns — the
// one place where the wave waits for a tile before the level's barrier: an I tile over a column border (0.42 per point on the bench's frames) has
// arrived before the J tile's loads are issued.  (Carried to the stores behind the barrier, the selectors were seven more registers
// to define on the inside path of every level.)
__device__ __forceinline__ unsigned int lk_load4_mirror(const unsigned char *img, unsigned int row_off, int x, int W, unsigned int &sel) {
    const int s           = min(max(max(min(x, 2 * W - 5 - x), 0), -3 - x), W - 4);
    const unsigned int sh = min((unsigned int) (8 * (x - s) + 16), 40u); // 8 o
    sel                   = (unsigned int) (0x0102030201000102ull >> sh);
    return *reinterpret_cast<const lk_u32u *>(img + (row_off + (unsigned int) s));
}
__device__ __forceinline__ unsigned int lk_mirror_apply(unsigned int d, unsigned int sel) { return __builtin_amdgcn_perm(0u, d, sel); }

#if defined(LK_TILE_HIST)
// profiling build (EXTRA_HIPFLAGS=-DLK_TILE_HIST, off in the product): tile loads since the library was loaded by level, tile (0: I at the level
// start, 1: J at the level start, 2: J re-staged) and path (0: inside, 1: over a row border only, 2: over a column border), the points that
// k_lk_track_fb tracked and the passes it ran; printed when the process ends (profiles/r10_lk_border_tiles.txt)
__device__ unsigned long long g_lk_tile_hist[4][3][3];
// (round 13) and, of both kernels: fetches of the lane's pixel pairs (epochs of constant integer window position), interior and border level
// set-ups, Gauss-Newton iterations (profiles/r13_lk_vertical_pairs.txt)
__device__ unsigned long long g_lk_tile_points[6];
static void lk_tile_hist_dump() {
    static unsigned long long h[4][3][3], p[6];
    if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_lk_tile_hist), sizeof h) != hipSuccess) return;
    if (hipMemcpyFromSymbol(p, HIP_SYMBOL(g_lk_tile_points), sizeof p) != hipSuccess) return;
    fprintf(stderr, "LK_TILE_HIST points %llu passes %llu\n", p[0], p[1]);
    fprintf(stderr, "LK_TILE_HIST fetches %llu interior_setups %llu border_setups %llu iterations %llu\n", p[2], p[3], p[4], p[5]);
    for (int l = 0; l < 4; l++)
        for (int k = 0; k < 3; k++)
            fprintf(stderr, "LK_TILE_HIST level %d tile %d inside %llu rows %llu columns %llu\n", l, k, h[l][k][0], h[l][k][1], h[l][k][2]);
}
__device__ __forceinline__ void lk_tile_hist(int level, int kind, int x0, int y0, int T, int W, int H, int lane) {
    const int path = (x0 < 0 || x0 + T > W) ? 2 : (y0 < 0 || y0 + T > H) ? 1 : 0;
    if (lane == 0) atomicAdd(&g_lk_tile_hist[min(level, 3)][kind][path], 1ull);
}
#define LK_HIST(level, kind, x0, y0, T) lk_tile_hist(level, kind, x0, y0, T, W, H, lane)
#define LK_COUNT(what) do { if (lane == 0) atomicAdd(&g_lk_tile_points[what], 1ull); } while (0)
#else
#define LK_HIST(level, kind, x0, y0, T)
#define LK_COUNT(what)
#endif

// Tile loads are split into "issue all global loads into registers" and "write them to LDS", so that the loads of the
// previous-image tile and of the next-image tile of a level fly together (one HBM/L2 round trip per level instead of
// two or more back-to-back ones: the wave has few siblings to hide latency behind at 84 VGPRs).
// Four ways, chosen wave-uniformly: a tile inside the level loads plain dwords (round 9); on a level of at least LK_JT x LK_JT a tile over the
// top or bottom border only loads plain dwords from mirrored rows (lk_mirror), and a tile over the left or right border mirrored dwords
// (lk_load4_mirror) — offsets by lk_offset on the same scalar base: no 64-bit address per lane, no byte load, no loop; levels smaller than
// that are staged by lk_stage_small (the callers test for them).
// 24x24 I tile: dword i = lane + 64*q -> (row i/6, dword column i%6), tile (r,c) <-> image (ipx-1+c, ipy-1+r)
__device__ __forceinline__ void lk_load_I(unsigned int (&v)[3], const unsigned char *I, int W, int H, int pitch, int ipx, int ipy, int lane) {
    const bool cols_in = ipx - 1 >= 0 && ipx - 1 + LK_IT <= W, rows_in = ipy - 1 >= 0 && ipy - 1 + LK_IT <= H; // wave-uniform
    if (cols_in && rows_in) {
#pragma unroll
        for (int q = 0; q < 3; q++) {
            const int i = lane + 64 * q;
            const int r = i / 6, cd = i - r * 6;
            v[q] = 0;
            if (i < LK_IT * 6) v[q] = *reinterpret_cast<const lk_u32u *>(I + lk_offset(ipy - 1 + r, pitch, ipx - 1 + 4 * cd));
        }
    } else if (cols_in) {
        asm volatile(""); // (real branches: left alone, the compiler joins the loads of the forms behind 64-bit addresses for all of them)
#pragma unroll
        for (int q = 0; q < 3; q++) {
            const int i = lane + 64 * q;
            const int r = i / 6, cd = i - r * 6;
            v[q] = 0;
            if (i < LK_IT * 6) v[q] = *reinterpret_cast<const lk_u32u *>(I + lk_offset(lk_mirror(ipy - 1 + r, H), pitch, ipx - 1 + 4 * cd));
        }
        asm volatile("");
    } else {
        asm volatile("");
        unsigned int sel[3] = {0, 0, 0}; // (lanes past the tile: perm of 0 by 0 is 0, and nothing stores it)
#pragma unroll
        for (int q = 0; q < 3; q++) {
            const int i = lane + 64 * q;
            const int r = i / 6, cd = i - r * 6;
            v[q] = 0;
            if (i < LK_IT * 6) v[q] = lk_load4_mirror(I, lk_offset(lk_mirror(ipy - 1 + r, H), pitch, 0), ipx - 1 + 4 * cd, W, sel[q]);
        }
#pragma unroll
        for (int q = 0; q < 3; q++) v[q] = lk_mirror_apply(v[q], sel[q]);
        asm volatile("");
    }
}
__device__ __forceinline__ void lk_store_I(lk_smem &S, const unsigned int (&v)[3], int lane) {
#pragma unroll
    for (int q = 0; q < 3; q++) {
        const int i = lane + 64 * q;
        const int r = i / 6, cd = i - r * 6;
        if (i < LK_IT * 6) S.I[(r * LK_IS >> 2) + cd] = v[q];
    }
}
// 32x32 J tile: lane -> (row lane>>1, 16 pixels at column (lane&1)*16) = 4 packed dwords, tile (r,c) <-> image (jx0+c, jy0+r)
__device__ __forceinline__ void lk_load_J(unsigned int (&v)[4], const unsigned char *J, int W, int H, int pitch, int jx0, int jy0, int lane) {
    const int r = lane >> 1, c0 = (lane & 1) * 16;
    const bool cols_in = jx0 >= 0 && jx0 + LK_JT <= W, rows_in = jy0 >= 0 && jy0 + LK_JT <= H; // wave-uniform
    if (cols_in && rows_in) {
        const unsigned char *row = J + lk_offset(jy0 + r, pitch, jx0 + c0);
#pragma unroll
        for (int q = 0; q < 4; q++) v[q] = *reinterpret_cast<const lk_u32u *>(row + 4 * q);
    } else if (cols_in) {
        asm volatile(""); // (as in lk_load_I)
        const unsigned char *row = J + lk_offset(lk_mirror(jy0 + r, H), pitch, jx0 + c0);
#pragma unroll
        for (int q = 0; q < 4; q++) v[q] = *reinterpret_cast<const lk_u32u *>(row + 4 * q);
        asm volatile("");
    } else {
        asm volatile("");
        const unsigned int row_off = lk_offset(lk_mirror(jy0 + r, H), pitch, 0);
        unsigned int sel[4];
#pragma unroll
        for (int q = 0; q < 4; q++) v[q] = lk_load4_mirror(J, row_off, jx0 + c0 + 4 * q, W, sel[q]);
#pragma unroll
        for (int q = 0; q < 4; q++) v[q] = lk_mirror_apply(v[q], sel[q]);
        asm volatile("");
    }
}
__device__ __forceinline__ void lk_store_J(lk_smem &S, const unsigned int (&v)[4], int lane) {
    const int r = lane >> 1, c0 = (lane & 1) * 16;
    unsigned int *dst = &S.J[(r * LK_JS + c0) >> 2];
#pragma unroll
    for (int q = 0; q < 4; q++) dst[q] = v[q];
}
// The general form of a tile load, for levels smaller than LK_JT on a side (a window may then reach further outside than the level is wide,
// and reflect-101 is a loop): every byte through icg_reflect101, in loops over the tile's dwords and their bytes that are not unrolled — only
// tests build such levels, and unrolled at its three call sites this form was most of the kernel's text.  It writes straight into LDS: the
// caller has passed the barrier that the register forms put between their loads and their stores.  ROWS x DPR dwords, SD dwords of LDS row
// stride; the same bytes at the same places as lk_load_I + lk_store_I (LK_IT, 6) and lk_load_J + lk_store_J (LK_JT, 8).  The trip count is
// wave-uniform: lanes past the last dword repeat it (the same value to the same address).
template <int ROWS, int DPR, int SD>
__device__ __forceinline__ void lk_stage_small(unsigned int *dst, const unsigned char *img, int W, int H, int pitch, int x0, int y0, int lane) {
#pragma unroll 1
    for (int base = 0; base < ROWS * DPR; base += 64) {
        const int i = min(base + lane, ROWS * DPR - 1);
        const int r = i / DPR, cd = i - r * DPR;
        const unsigned char *row = img + (size_t) icg_reflect101(y0 + r, H) * pitch;
        unsigned int v = 0;
#pragma unroll 1
        for (int k = 0; k < 4; k++) v |= (unsigned int) row[icg_reflect101(x0 + 4 * cd + k, W)] << (8 * k);
        dst[r * SD + cd] = v;
    }
}
__device__ __forceinline__ bool lk_small_level(int W, int H) { return min(W, H) < LK_JT; } // wave-uniform
// (re-)stage the J tile between two barriers of the caller's
__device__ __forceinline__ void lk_stage_J(lk_smem &S, const unsigned char *J, int W, int H, int pitch, int jx0, int jy0,
                                           int lane) {
    if (lk_small_level(W, H)) {
        lk_stage_small<LK_JT, LK_JT / 4, LK_JS / 4>(S.J, J, W, H, pitch, jx0, jy0, lane);
    } else {
        unsigned int v[4];
        lk_load_J(v, J, W, H, pitch, jx0, jy0, lane);
        lk_store_J(S, v, lane);
    }
}

typedef short s16x2 __attribute__((ext_vector_type(2)));
typedef unsigned short u16x2 __attribute__((ext_vector_type(2)));

// packed 16-bit helpers (all operands stay inside 16 bits: pixels <= 255, Scharr terms <= 4080, Q14 weights <= 16384)
__device__ __forceinline__ unsigned int pk_add(unsigned int a, unsigned int b) {
    return __builtin_bit_cast(unsigned int, (u16x2) (__builtin_bit_cast(u16x2, a) + __builtin_bit_cast(u16x2, b)));
}
__device__ __forceinline__ unsigned int pk_sub(unsigned int a, unsigned int b) {
    return __builtin_bit_cast(unsigned int, (u16x2) (__builtin_bit_cast(u16x2, a) - __builtin_bit_cast(u16x2, b)));
}
__device__ __forceinline__ unsigned int pk_mul(unsigned int a, unsigned short k) {
    return __builtin_bit_cast(unsigned int, (u16x2) (__builtin_bit_cast(u16x2, a) * k));
}
// exact a.lo*b.lo + a.hi*b.hi + c on signed 16-bit halves (v_dot2_i32_i16)
__device__ __forceinline__ int dot2(unsigned int a, unsigned int b, int c) {
    return __builtin_amdgcn_sdot2(__builtin_bit_cast(s16x2, a), __builtin_bit_cast(s16x2, b), c, false);
}
// the same with a SEPARATE accumulator register (VOP3P v_dot2_i32_i16).  The builtin is selected as v_dot2c, whose accumulator is tied to the
// destination: an accumulator that must survive (c0[k] in every iteration, the rounding constants of the set-up) costs a v_mov per use.
__device__ __forceinline__ int dot2_keep(unsigned int a, unsigned int b, int c) {
    int d;
    asm("v_dot2_i32_i16 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "v"(c));
    return d;
}
// the same with a wave-uniform accumulator from a scalar register (one SGPR operand is allowed on the constant bus): the rounding constants
// of the set-up's blends cost no VGPR this way (round 6: pinned in VGPRs they were the two registers k_lk_track_fb spilled at 5 waves)
__device__ __forceinline__ int dot2_keep_s(unsigned int a, unsigned int b, int c_uniform) {
    int d;
    asm("v_dot2_i32_i16 %0, %1, %2, %3" : "=v"(d) : "v"(a), "v"(b), "s"(c_uniform));
    return d;
}
// a.lo*b.lo + a.hi*b.hi with the accumulator 0 as an inline constant
__device__ __forceinline__ int dot2_zero(unsigned int a, unsigned int b) {
    int d;
    asm("v_dot2_i32_i16 %0, %1, %2, 0" : "=v"(d) : "v"(a), "v"(b));
    return d;
}
// a * 12 + c and a * 40 + c on a signed 24-bit a (v_mad_i32_i24), the accumulator a register or wave-uniform: the Scharr weights x 4 of the
// 32-bit stencil.  (Left to the compiler, two chained multiply-adds become two multiplications and a v_add3: three half-rate issues for two.)
__device__ __forceinline__ int mad24_12(int a, int c) {
    int d;
    asm("v_mad_i32_i24 %0, %1, 12, %2" : "=v"(d) : "v"(a), "v"(c));
    return d;
}
__device__ __forceinline__ int mad24_40_s(int a, int c_uniform) {
    int d;
    asm("v_mad_i32_i24 %0, %1, 40, %2" : "=v"(d) : "v"(a), "s"(c_uniform));
    return d;
}
// (lo16(a), lo16(b)) as one packed register
__device__ __forceinline__ unsigned int pk_lo16(int a, int b) {
    return __builtin_amdgcn_perm((unsigned int) b, (unsigned int) a, 0x05040100u);
}
// (hi16(a), hi16(b)) as one packed register
__device__ __forceinline__ unsigned int pk_hi16(int a, int b) {
    return __builtin_amdgcn_perm((unsigned int) b, (unsigned int) a, 0x07060302u);
}
// the pair one 16-bit element further: (a.hi, b.lo)
__device__ __forceinline__ unsigned int pk_shift(unsigned int a, unsigned int b) { return __builtin_amdgcn_alignbit(b, a, 16); }

// (upper, 0, lower, 0): byte c & 3 of the upper row's dword and of the lower row's dword as one u16 pair (v_perm_b32 of lower : upper)
__device__ __forceinline__ constexpr unsigned int lk_vpair_sel(int c) { return 0x0c000c00u | (unsigned int) (c & 3) | ((unsigned int) (4 + (c & 3)) << 16); }

// the lane's two 8-pixel rows of the window at integer position (inx, iny), from the staged tile (3 aligned dwords + a
// byte funnel shift per row), expanded to the 8 VERTICALLY adjacent u16 pixel pairs the bilinear blend consumes (round 13):
// VP[k] = (J[row0][o + k], J[row0 + 1][o + k]).  blend_k = dot2(VP[k + 1], Wr, dot2(VP[k], Wl, c)) is the four products and the 32-bit sum
// of the horizontal pairs' dot2(JB[k], W1, dot2(JA[k], W0, c)) — 8 v_perm and 8 registers per fetch instead of 14 and 14
// (tests/test_lk_vertical_pairs_identity.py restates both chains and the byte selection).
__device__ __forceinline__ void lk_fetch_J(const lk_smem &S, int row0, int o, unsigned int (&VP)[8]) {
    const int idx = o >> 2, sh = o & 3;
    const unsigned int *r0 = &S.J[__umul24((unsigned int) row0, LK_JS >> 2) + (unsigned int) idx]; // (row0 < 32: a 24-bit multiply-add, no 64-bit one)
    const unsigned int *r1 = r0 + (LK_JS >> 2);
    const unsigned int d0 = r0[0], d1 = r0[1], d2 = r0[2];
    const unsigned int e0 = r1[0], e1 = r1[1], e2 = r1[2];
    const unsigned int a0 = __builtin_amdgcn_alignbyte(d1, d0, sh), a1 = __builtin_amdgcn_alignbyte(d2, d1, sh);
    const unsigned int b0 = __builtin_amdgcn_alignbyte(e1, e0, sh), b1 = __builtin_amdgcn_alignbyte(e2, e1, sh);
#pragma unroll
    for (int k = 0; k < 8; k++) VP[k] = __builtin_amdgcn_perm(k < 4 ? b0 : b1, k < 4 ? a0 : a1, lk_vpair_sel(k));
}

// The three rows of zeros under the B plane (what lane 63, which owns no pixels, differentiates): written once per kernel, before the first
// level's barriers; no level writes them again.
__device__ __forceinline__ void lk_zero_rows(lk_smem &S, int lane) {
    static_assert(3 * LK_BW <= 128, "two stores per lane cover the rows of zeros");
    S.B[(LK_BH - 3) * LK_BW + lane] = 0;
    if (lane < 3 * LK_BW - 64) S.B[(LK_BH - 3) * LK_BW + 64 + lane] = 0;
}

// One calcOpticalFlowPyrLK point, executed cooperatively by a full wave (lk_zero_rows has run). Returns status.
__device__ bool lk_track_wave(const icg_pyr_desc &P, const unsigned char *slotI, const unsigned char *slotJ,
                              float2 prevPt, float2 &nextIO, lk_smem &S, int lane, float *err_out) {
    const float FLT_SCALE = 1.f / (1 << 20);
    const double eps2     = 0.01 * 0.01;
    bool status           = true;
    float errv            = 0.f;
    float2 nextStore      = nextIO;
    const int maxLevel    = P.n_levels - 1;
    const bool active     = lane < 63;
    const int ly          = active ? lane / 3 : 0;
    const int lx0         = active ? (lane - ly * 3) * 7 : 0;
    const unsigned int am = active ? ~0u : 0u; // lane 63 owns no pixels: its derivative weights are zeroed (Ix = Iy = 0 -> no contribution to any sum)
    // rounding constants of the set-up's blends, kept in scalar registers for dot2_keep_s (opaque to the optimizer: not re-materialised per use)
    int rnd15 = 1 << 15, rnd8 = 1 << 8;
    asm volatile("" : "+s"(rnd15), "+s"(rnd8));

    for (int level = maxLevel; level >= 0; --level) {
        const int W = P.w[level], H = P.h[level], pitch = P.pitch[level];
        const unsigned char *I = slotI + P.off[level];
        const unsigned char *J = slotJ + P.off[level];
        // 2^-level from its bit pattern (round 9; (float) (1. / (1 << level)) was an FP64 division at the head of every level: level is a loop variable)
        const float scale      = __uint_as_float((unsigned int) (127 - level) << 23);
        float prevx = prevPt.x * scale, prevy = prevPt.y * scale;
        float nptx, npty;
        if (level == maxLevel) {
            nptx = nextStore.x * scale;
            npty = nextStore.y * scale;
        } else {
            nptx = nextStore.x * 2.f;
            npty = nextStore.y * 2.f;
        }
        nextStore = make_float2(nptx, npty);

        prevx -= (float) ICG_LK_HALF;
        prevy -= (float) ICG_LK_HALF;
        const int ipx = (int) floorf(prevx), ipy = (int) floorf(prevy);
        if (ipx < -ICG_LK_WIN || ipx >= W || ipy < -ICG_LK_WIN || ipy >= H) {
            if (level == 0) {
                status = false;
                errv   = 0.f;
            }
            continue;
        }
        unsigned int W0, W1; // the interior set-up and the iterations: Wl = (w00, w10), Wr = (w01, w11); the border set-up: (w00, w01), (w10, w11)
        const float pax = prevx - ipx, pay = prevy - ipy;

        // ---- stage the 24x24 neighbourhood of the previous image AND the 32x32 tile of the next image around the
        //      level's starting estimate in one go (both address sets are known here) ----
        int jx0 = -1000000, jy0 = -1000000;
        {
            const int inx0 = (int) floorf(nptx - (float) ICG_LK_HALF), iny0 = (int) floorf(npty - (float) ICG_LK_HALF);
            const bool jok = !(inx0 < -ICG_LK_WIN || inx0 >= W || iny0 < -ICG_LK_WIN || iny0 >= H); // else iteration 0 bails out
            const bool small = lk_small_level(W, H);
            unsigned int vi[3] = {0, 0, 0}, vj[4] = {0, 0, 0, 0};
            LK_HIST(level, 0, ipx - 1, ipy - 1, LK_IT);
            if (!small) lk_load_I(vi, I, W, H, pitch, ipx, ipy, lane);
            if (jok) {
                jx0 = inx0 - LK_JM;
                jy0 = iny0 - LK_JM;
                LK_HIST(level, 1, jx0, jy0, LK_JT);
                if (!small) lk_load_J(vj, J, W, H, pitch, jx0, jy0, lane);
            }
            __syncthreads(); // previous level's LDS readers are done
            if (!small) {
                lk_store_I(S, vi, lane);
                if (jok) lk_store_J(S, vj, lane);
            } else {
                lk_stage_small<LK_IT, LK_IT / 4, LK_IS / 4>(S.I, I, W, H, pitch, ipx - 1, ipy - 1, lane);
                if (jok) lk_stage_small<LK_JT, LK_JT / 4, LK_JS / 4>(S.J, J, W, H, pitch, jx0, jy0, lane);
            }
            __syncthreads();
        }

        // ---- per lane: 4 rows x 10 bytes -> I samples and on-the-fly Scharr derivatives of its 7-pixel run ----
        // c0[k] = 256 - 512*Ival[k]: the patch sample folded into the rounding constant of the J blend, so that
        //         diff = ((Jblend + 256) >> 9) - Ival == (Jblend + c0) >> 9 exactly (Ival is an integer)
        // IXP/IYP: the derivative samples as packed i16 pairs (k, k+1), k = 0,2,4,6 (upper half of the last pair is 0)
        int c0[7];
        unsigned int IXP[4], IYP[4];
        int sA11 = 0, sA12 = 0, sA22 = 0;
        float A11, A12, A22;
        // derivative at support position (c = lx0+j, r = ly+rr): 3x3 neighbourhood = tile rows rr..rr+2, cols j..j+2.
        // The derivative plane is ZERO outside the image: X = ipx+lx0+j in [0,W), Y = ipy+ly+rr in [0,H).
        const bool all_in = ipx >= 0 && ipx + 22 <= W && ipy >= 0 && ipy + 22 <= H; // wave-uniform
        if (all_in) {
            // Interior windows (round 7): the blend and the Scharr stencil are integer linear maps and the only rounding is the final descale, so
            //   sum_ab w_ab Scharr(I)(x+a, y+b) = Scharr(B)(x, y),  B(x, y) = sum_ab w_ab I(x+a, y+b)  (|B| <= 255 * 2^14; 4 * 16 * |B| < 2^29).
            // ONE blend of the 23x23 grid shared through LDS and a 32-bit separable Scharr replace three blends of derivative planes that
            // vertically adjacent lanes computed twice.  (A real branch: the empty asm keeps the compiler from merging the two forms.)
            asm volatile("" ::: "memory");
            LK_COUNT(3);
            lk_weights_pk<true>(pax, pay, W0, W1);
            {
                // lane -> (row lane/2, 12 columns at (lane&1)*12) of B; lanes 46..63 repeat row 22 (same values to the same addresses: the
                // wave stays full).  B carries the +256 of the patch sample's rounding; every difference below cancels it.  Column 23
                // (from the tile row's padding bytes) is written and never read.
                const int br = min(lane >> 1, 22), bs = lane & 1;
                const unsigned int *p = &S.I[(br * LK_IS >> 2) + 3 * bs];
                unsigned int d[2][4];
#pragma unroll
                for (int q = 0; q < 4; q++) d[0][q] = p[q], d[1][q] = p[(LK_IS >> 2) + q];
                int *dst = &S.B[br * LK_BW + 12 * bs];
                // (round 13) the 13 vertical pairs (I[br][c], I[br + 1][c]) of the lane's 12 positions, one v_perm each (were 24 horizontal pairs)
                unsigned int VP[13];
#pragma unroll
                for (int c = 0; c < 13; c++) VP[c] = __builtin_amdgcn_perm(d[1][c >> 2], d[0][c >> 2], lk_vpair_sel(c));
#pragma unroll
                for (int q = 0; q < 3; q++) {
                    int bv[4];
#pragma unroll
                    for (int e = 0; e < 4; e++) bv[e] = dot2(VP[4 * q + e + 1], W1, dot2_keep_s(VP[4 * q + e], W0, rnd8));
                    *reinterpret_cast<int4 *>(dst + 4 * q) = make_int4(bv[0], bv[1], bv[2], bv[3]);
                }
            }
            __syncthreads();
            // per lane: rows ly..ly+2, columns lx0..lx0+8 of B -> vertical smooth (x 4, as in the border form: the descaled derivative is the
            // HIGH half of 4 v + 2^15) and vertical difference once each, then the horizontal difference / smooth.  All products are 24-bit:
            // B + 256 < 2^22, sums of two < 2^23.  The rounding constant of Ix rides in the smooth terms ((j/2) 2^15: S[k+2] - S[k] keeps
            // one 2^15), that of Iy is the accumulator of its first product.  Lane 63 reads the rows of zeros: (0 + 2^15) >> 16 = 0.
            int bo = ly * LK_BW + lx0 + ((lane + 1) >> 6) * ((LK_BH - 3) * LK_BW); // lane 63 (ly = lx0 = 0): the rows of zeros
            asm volatile("" : "+v"(bo)); // (one address register + immediate offsets; folded into the struct offset, every read got its own)
            const int *bp = &S.B[bo];
            int Sm[9], Vd[9];
#pragma unroll
            for (int jj = 0; jj < 9; jj++) {
                const int b0 = bp[jj], b1 = bp[LK_BW + jj], b2 = bp[2 * LK_BW + jj];
                Sm[jj] = mad24_12(b0 + b2, mad24_40_s(b1, (jj >> 1) << 15));
                Vd[jj] = b2 - b0;
                if (jj >= 1 && jj <= 7) c0[jj - 1] = 256 - (b1 & ~511); // c0 = 256 - 512 * ((blend + 256) >> 9)
            }
            int bx[7], by[7];
#pragma unroll
            for (int k = 0; k < 7; k++) {
                bx[k] = Sm[k + 2] - Sm[k];
                by[k] = mad24_12(Vd[k] + Vd[k + 2], mad24_40_s(Vd[k + 1], rnd15));
            }
#pragma unroll
            for (int m = 0; m < 4; m++) {
                IXP[m] = m < 3 ? pk_hi16(bx[2 * m], bx[2 * m + 1]) : (unsigned int) bx[6] >> 16;
                IYP[m] = m < 3 ? pk_hi16(by[2 * m], by[2 * m + 1]) : (unsigned int) by[6] >> 16;
            }
        } else {
            // windows that reach over the image border: the derivative plane is zero outside the image, so the identity above does not hold
            LK_COUNT(4);
            lk_weights_pk(pax, pay, W0, W1);
            const int idx = lx0 >> 2, sh = lx0 & 3;
            unsigned int Pp[4][5]; // pixel pairs (col 2m, 2m+1) of tile rows ly..ly+3, cols lx0..lx0+9
            // pair m = bytes sh + 2m, sh + 2m + 1 of the row's four dwords: for every sh in 0..3 it lies inside ONE pair of adjacent dwords that
            // does not depend on sh — (d1:d0) for m = 0, 1, (d2:d1) for m = 2, 3, (d3:d2) for m = 4 — so v_perm takes it straight from the
            // loaded dwords with two per-lane selectors (round 6: the three v_alignbyte per row that normalised the row first are gone)
            const unsigned int sel0 = 0x0c000c00u | (unsigned int) sh | ((unsigned int) (sh + 1) << 16), sel1 = sel0 + 0x00020002u;
#pragma unroll
            for (int r = 0; r < 4; r++) {
                const unsigned int *p = &S.I[((ly + r) * LK_IS >> 2) + idx];
                const unsigned int d0 = p[0], d1 = p[1], d2 = p[2], d3 = p[3];
                Pp[r][0] = __builtin_amdgcn_perm(d1, d0, sel0);
                Pp[r][1] = __builtin_amdgcn_perm(d1, d0, sel1);
                Pp[r][2] = __builtin_amdgcn_perm(d2, d1, sel0);
                Pp[r][3] = __builtin_amdgcn_perm(d2, d1, sel1);
                Pp[r][4] = __builtin_amdgcn_perm(d3, d2, sel0);
            }
            unsigned int DX[2][4], DY[2][4];
#pragma unroll
            for (int rr = 0; rr < 2; rr++) {
                unsigned int T0[5], T1[5];
#pragma unroll
                for (int m = 0; m < 5; m++) {
                    T0[m] = pk_add(pk_mul(pk_add(Pp[rr][m], Pp[rr + 2][m]), 12), pk_mul(Pp[rr + 1][m], 40)); // 4 * (3*(p0+p2) + 10*p1)
                    T1[m] = pk_sub(Pp[rr + 2][m], Pp[rr][m]);                                                // p2 - p0
                }
#pragma unroll
                for (int m = 0; m < 4; m++) {
                    DX[rr][m] = pk_sub(T0[m + 1], T0[m]);                                                       // 4 * (t0[j+2] - t0[j])
                    DY[rr][m] = pk_add(pk_mul(pk_add(T1[m], T1[m + 1]), 12), pk_mul(pk_shift(T1[m], T1[m + 1]), 40)); // 4 * (3*(t1[j]+t1[j+2]) + 10*t1[j+1])
                }
            }
            { // the derivatives outside the image are zero
#pragma unroll
                for (int rr = 0; rr < 2; rr++) {
                    const int Y           = ipy + ly + rr;
                    const unsigned int RM = (Y >= 0 && Y < H) ? ~0u : 0u;
#pragma unroll
                    for (int m = 0; m < 4; m++) {
                        const int X0 = ipx + lx0 + 2 * m, X1 = X0 + 1;
                        const unsigned int CM = ((X0 >= 0 && X0 < W) ? 0x0000ffffu : 0u) | ((X1 >= 0 && X1 < W) ? 0xffff0000u : 0u);
                        DX[rr][m] &= CM & RM;
                        DY[rr][m] &= CM & RM;
                    }
                }
            }
            // The Scharr terms above carry a factor 4 (12, 40 for 3, 10: |4 d| <= 16 320 still fits 16 bits), so the blended derivative
            // (sum w d + 2^13) >> 14 is the HIGH half of sum w (4 d) + 2^15: one v_perm packs two of them, no shift (round 6: 14 shifts per level).
            int bx[7], by[7];
            const unsigned int W0d = W0 & am, W1d = W1 & am; // (lane 63: (0 + 2^15) >> 16 = 0)
#pragma unroll
            for (int k = 0; k < 7; k++) {
                const int m = k >> 1;
                // (v[k], v[k+1]) pairs of the two derivative rows and of tile rows 1, 2 at columns k+1, k+2
                const unsigned int dx0 = (k & 1) ? pk_shift(DX[0][m], DX[0][m + 1]) : DX[0][m];
                const unsigned int dx1 = (k & 1) ? pk_shift(DX[1][m], DX[1][m + 1]) : DX[1][m];
                const unsigned int dy0 = (k & 1) ? pk_shift(DY[0][m], DY[0][m + 1]) : DY[0][m];
                const unsigned int dy1 = (k & 1) ? pk_shift(DY[1][m], DY[1][m + 1]) : DY[1][m];
                const int m1 = (k + 1) >> 1;
                const unsigned int i1 = ((k + 1) & 1) ? pk_shift(Pp[1][m1], Pp[1][m1 + 1]) : Pp[1][m1];
                const unsigned int i2 = ((k + 1) & 1) ? pk_shift(Pp[2][m1], Pp[2][m1 + 1]) : Pp[2][m1];
                bx[k]        = dot2(dx1, W1d, dot2_keep_s(dx0, W0d, rnd15));
                by[k]        = dot2(dy1, W1d, dot2_keep_s(dy0, W0d, rnd15));
                // c0 = 256 - 512 * ((blend + 256) >> 9) = 256 - ((blend + 256) & ~511)
                c0[k]        = 256 - (dot2(i2, W1, dot2_keep_s(i1, W0, rnd8)) & ~511);
            }
#pragma unroll
            for (int m = 0; m < 4; m++) {
                IXP[m] = m < 3 ? pk_hi16(bx[2 * m], bx[2 * m + 1]) : (unsigned int) bx[6] >> 16;
                IYP[m] = m < 3 ? pk_hi16(by[2 * m], by[2 * m + 1]) : (unsigned int) by[6] >> 16;
            }
        }
        {
            sA11 = dot2(IXP[3], IXP[3], dot2(IXP[2], IXP[2], dot2(IXP[1], IXP[1], dot2(IXP[0], IXP[0], 0))));
            sA12 = dot2(IXP[3], IYP[3], dot2(IXP[2], IYP[2], dot2(IXP[1], IYP[1], dot2(IXP[0], IYP[0], 0))));
            sA22 = dot2(IYP[3], IYP[3], dot2(IYP[2], IYP[2], dot2(IYP[1], IYP[1], dot2(IYP[0], IYP[0], 0))));
            wave_sum3_i32x16_f32(sA11, sA12, sA22, A11, A12, A22);
            A11 *= FLT_SCALE, A12 *= FLT_SCALE, A22 *= FLT_SCALE;
        }
        float D            = A11 * A22 - A12 * A12;
        // (the argument of the root: A = n 2^-20 rounded to 24 bits, so a difference is zero or at least 2^-20 — zero or >= 2^-40, icg_sqrt_unscaled's domain)
        const float eig2 = A22 + A11 - icg_sqrt_unscaled((A11 - A22) * (A11 - A22) + 4.f * A12 * A12);
        // minEig = eig2 / (2 * 21 * 21) < 1e-4f, without the division (round 6: ten instructions per level): a correctly rounded quotient is
        // non-decreasing in its numerator, so the test is eig2 < T with T the smallest float whose quotient by 882 reaches 1e-4f —
        // T = 0x3DB4A233 (0.088199995; fl(T / 882) = 1e-4f, fl(pred(T) / 882) = 9.999998e-5: searched over the floats around 0.0882)
        static_assert(ICG_LK_WIN == 21, "the threshold constant below is for a 21 x 21 window");
        const bool weak = eig2 < __uint_as_float(0x3DB4A233u) || D < FLT_EPSILON;
        if (weak) {
            if (level == 0) status = false;
            continue;
        }
        D = 1.f / D;
        // the 2^-20 of the window sums folded into the inverse determinant (round 5): b1, b2 stay unscaled integers-as-floats, and scaling by a
        // power of two commutes with every rounding of (A12 b2 - A22 b1) D (no intermediate leaves the normal range: |b| >= 1 or 0,
        // A = n 2^-20, 2^-28 <= D <= 2^23) — the step is the same float, bit for bit, two multiplications per iteration cheaper
        const float Ds = D * FLT_SCALE;
        nptx -= (float) ICG_LK_HALF;
        npty -= (float) ICG_LK_HALF;
        float pdx = 0.f, pdy = 0.f;
        int cinx = -1000000, ciny = -1000000; // integer window position whose pixel pairs are cached in VP
        unsigned int VP[8];
#pragma unroll
        for (int k = 0; k < 8; k++) VP[k] = 0;

        // The Gauss-Newton iterations, as EPOCHS of constant integer window position: the lane's pixel pairs VP are fetched once per epoch
        // and are loop-invariant inside it (written as one loop with a conditional re-fetch, they were loop-carried through the condition
        // and the compiler copied all of them twice per iteration: 28 of ~130 VALU instructions with the 14 horizontal pairs of rounds 4-12).  Same checks in the same order.
        // Round 5 (instruction diet by the measured issue costs, profiles/ubench: conversions, roundings, compares, DPP, dot2, FP64 and
        // everything VOP3 cost twice a plain add / mul): the fractional position a = npt - floor(npt) is carried from
        // the epoch test of the previous iteration (the window stays in the epoch iff 0 <= a < 1 on both axes: one subtraction and one
        // unsigned compare per axis instead of floor, convert, compare and convert back), the weights come packed from lk_weights_pk,
        // c0[k] is read in place (dot2_keep), b1 and b2 come out of ONE reduction tree, the oscillation test compares in f32
        // (|s| < 0.01 in double  <=>  |s| <= 0.01f for a float s: 0.01f < 0.01 < nextafter(0.01f)).
        int j = 0;
        bool more = true, osc = false;
        while (more) {
            const float fx = floorf(nptx), fy = floorf(npty);
            const int inx = (int) fx, iny = (int) fy;
            if (inx < -ICG_LK_WIN || inx >= W || iny < -ICG_LK_WIN || iny >= H) {
                if (level == 0) status = false;
                break;
            }
            if (!(inx >= jx0 && inx <= jx0 + (LK_JT - 22) && iny >= jy0 && iny <= jy0 + (LK_JT - 22))) {
                jx0 = inx - LK_JM;
                jy0 = iny - LK_JM;
                LK_HIST(level, 2, jx0, jy0, LK_JT);
                __syncthreads();
                lk_stage_J(S, J, W, H, pitch, jx0, jy0, lane);
                __syncthreads();
            }
            LK_COUNT(2);
            lk_fetch_J(S, iny - jy0 + ly, (inx - jx0) + lx0, VP);
            cinx = inx;
            ciny = iny;
            float ax = nptx - fx, ay = npty - fy; // == nptx - (float) inx
            for (;;) {
                LK_COUNT(5);
                lk_weights_pk<true>(ax, ay, W0, W1);
                int diff[7];
#pragma unroll
                for (int k = 0; k < 7; k++) diff[k] = dot2(VP[k + 1], W1, dot2_keep(VP[k], W0, c0[k])) >> 9;
                int sb1 = 0, sb2 = 0;
#pragma unroll
                for (int m = 0; m < 4; m++) {
                    const unsigned int dp = m < 3 ? pk_lo16(diff[2 * m], diff[2 * m + 1]) : (unsigned int) diff[6]; // IXP[3].hi == 0
                    // (the first product takes its zero accumulator as an inline constant: v_dot2c's tied accumulator cost a v_mov 0 per sum)
                    sb1 = m ? dot2(dp, IXP[m], sb1) : dot2_zero(dp, IXP[m]);
                    sb2 = m ? dot2(dp, IYP[m], sb2) : dot2_zero(dp, IYP[m]);
                }
                float b1, b2;
                wave_sum2_i32x8_f32(sb1, sb2, b1, b2);
                const float dx = (float) ((A12 * b2 - A22 * b1) * Ds);
                const float dy = (float) ((A12 * b1 - A11 * b2) * Ds);
                nptx += dx;
                npty += dy;
                // ddx^2 + ddy^2 <= eps^2 in double (dx^2 is exact in double, so the fused form rounds the same sum once, as the two-step form
                // does).  Round 6: the float sum of the float squares is within 2^-22 of it, relatively — outside a band of 1e-5 around eps^2
                // it decides the test, and only inside the band the FP64 form runs (four half-rate instructions of every iteration before).
                // Round 13: n2 above the band is every iteration but a level's last, so that ONE compare is the common path; the other compare
                // and the FP64 form sit behind it.  nextStore = npt + half window is formed once behind the loops, not in every iteration.
                const float n2 = dx * dx + dy * dy;
                if (!(n2 > 1.00001e-4f)) { // wave-uniform; a real branch (the empty asm keeps the compiler from computing both forms always)
                    asm volatile("");
                    bool converged = n2 < 9.9999e-5f;
                    if (!converged) converged = __builtin_fma((double) dx, (double) dx, (double) dy * (double) dy) <= eps2;
                    if (converged) {
                        more = false;
                        break;
                    }
                }
                const float sx = dx + pdx, sy = dy + pdy;
                pdx = dx;
                pdy = dy;
                if (j > 0 && fabsf(sx) <= 0.01f && fabsf(sy) <= 0.01f) {
                    osc  = true; // (pdx, pdy hold this iteration's step: half of it is taken back behind the loops)
                    more = false;
                    break;
                }
                if (++j >= LK_MAX_ITERS) {
                    more = false;
                    break;
                }
                ax = nptx - fx;
                ay = npty - fy;
                // floor(npt) unchanged on both axes <=> 0 <= a < 1 <=> bits(a) < bits(1.0f) as unsigned (a negative a has the sign bit set);
                // when a rounding makes a == 1.0f for a position still inside the pixel, the next epoch finds the same pixels again
                if (!(__float_as_uint(ax) < 0x3f800000u && __float_as_uint(ay) < 0x3f800000u)) break; // next epoch: bounds test, tile, fetch
            }
        }
        // (round 13) the level's result, once: the position after the last step — when the bounds test ended the level before any step, the
        // level's start as it came — and on the oscillation exit half of the last step back
        if (j > 0 || !more) nextStore = make_float2(nptx + (float) ICG_LK_HALF, npty + (float) ICG_LK_HALF);
        if (osc) {
            nextStore.x -= pdx * 0.5f;
            nextStore.y -= pdy * 0.5f;
        }

        if (status && level == 0) {
            // OpenCV >= 3.4 epilogue (taken because the reference passes an err vector, tracking.cc:381,386,391)
            const float ex = nextStore.x - (float) ICG_LK_HALF, ey = nextStore.y - (float) ICG_LK_HALF;
            const int inx = (int) floorf(ex), iny = (int) floorf(ey);
            if (inx < -ICG_LK_WIN || inx >= W || iny < -ICG_LK_WIN || iny >= H) {
                status = false;
                continue;
            }
            if (err_out) {
                if (inx != cinx || iny != ciny) {
                    if (!(inx >= jx0 && inx <= jx0 + (LK_JT - 22) && iny >= jy0 && iny <= jy0 + (LK_JT - 22))) {
                        jx0 = inx - LK_JM;
                        jy0 = iny - LK_JM;
                        __syncthreads();
                        lk_stage_J(S, J, W, H, pitch, jx0, jy0, lane);
                        __syncthreads();
                    }
                    lk_fetch_J(S, iny - jy0 + ly, (inx - jx0) + lx0, VP);
                }
                lk_weights_pk<true>(ex - inx, ey - iny, W0, W1);
                int se = 0;
#pragma unroll
                for (int k = 0; k < 7; k++) {
                    const int diff = dot2(VP[k + 1], W1, dot2_keep(VP[k], W0, c0[k])) >> 9;
                    se += diff < 0 ? -diff : diff;
                }
                se &= (int) am; // lane 63 owns no pixels
                errv = wave_sum_i32x16_f32(se) * 1.f / (float) (32 * ICG_LK_WIN * ICG_LK_WIN);
            }
        }
    }
    nextIO = nextStore;
    if (err_out && lane == 0) *err_out = errv;
    return status;
}

__global__ __launch_bounds__(64) void k_lk_track(icg_pyr_desc P, int n, const int32_t *prev_slot, const int32_t *next_slot,
                                                 const float2 *prev_pts, float2 *next_pts, unsigned char *status, float *err) {
    __shared__ lk_smem S;
    const int i = icg_xcd_chunked(blockIdx.x, n);
    if (i >= n) return;
    const int lane = threadIdx.x;
    lk_zero_rows(S, lane);
    const unsigned char *sI = P.base + (size_t) prev_slot[i] * P.slot_bytes;
    const unsigned char *sJ = P.base + (size_t) next_slot[i] * P.slot_bytes;
    float2 nx = next_pts[i];
    bool st   = lk_track_wave(P, sI, sJ, prev_pts[i], nx, S, lane, err ? err + i : nullptr);
    if (lane == 0) {
        next_pts[i] = nx;
        status[i]   = st ? 1 : 0;
    }
}

// (Parameter order: inputs first, outputs last, and seg_count ahead of the four integers — the early exit then fetches seg_count, the sizes and
// the magic without the output pointers, which the compiler otherwise loads with them and parks in VGPR lanes for the whole kernel: 10 SGPRs
// parked with seg_count behind seg_magic, 2 in this order; profiles/r09_uniform_prologues.txt met the same with another order.)
__global__ __launch_bounds__(64, LK_WAVES_PER_EU) void k_lk_track_fb(icg_pyr_desc P, int n, const int32_t *prev_slot,
                                                    const int32_t *next_slot, const float2 *prev_pts,
                                                    const float2 *guess_pts, const int32_t *seg_count, int img_w, int img_h,
                                                    int seg_cap, unsigned int seg_magic,
                                                    float2 *out_pts, unsigned char *status, float2 *out_bwd) {
    __shared__ lk_smem S;
    const int i = icg_xcd_chunked(blockIdx.x, n);
    if (i >= n) return;
    // segmented call (device-resident tracker, tracker.hip): the points of stream s are entries [s * seg_cap, s * seg_cap + seg_count[s])
    // of every array; the stage kernel that ran before this launch left the count in device memory — no host round trip sizes the grid
    // (seg_magic = icg_div_magic(seg_cap): i and the quotient are wave-uniform, the decode is scalar — the division by a run-time value was a
    // v_rcp_iflag_f32 and its fix-up sequence in every wave of the grid, the half that leaves here included)
    if (seg_count) {
        const int s = icg_div_by_magic(i, seg_magic);
        if (i - s * seg_cap >= seg_count[s]) return; // wave-uniform
    }
    const int lane = threadIdx.x;
#if defined(LK_TILE_HIST)
    if (lane == 0) atomicAdd(&g_lk_tile_points[0], 1ull);
#endif
    lk_zero_rows(S, lane);
    const unsigned char *sP = P.base + (size_t) prev_slot[i] * P.slot_bytes;
    const unsigned char *sN = P.base + (size_t) next_slot[i] * P.slot_bytes;
    const float2 p0 = prev_pts[i];
    float2 fwd      = guess_pts[i];
    float2 bwd      = p0;
    bool st_f = false, st_b = false;
    // forward then backward through ONE copy of the tracker body (16 KB of code instead of 32 KB in the shared I-cache)
    for (int dir = 0; dir < 2; dir++) {
        if (dir) {
            // the cull of tracking.cc:396-403 needs the backward track only for points that are still alive
            // (isOnBorder compares in double: (double) f < 5.0 <=> f < 5.0f and (double) f > w - 5.0 <=> f > (float) (w - 5) for a float f and
            // an image narrower than 2^24 — the float form keeps two FP64 constants out of the registers for the whole forward pass)
            const bool border = fwd.x < 5.f || fwd.y < 5.f || fwd.x > (float) (img_w - 5) || fwd.y > (float) (img_h - 5);
            if (!st_f || border) break; // wave-uniform
        }
        const unsigned char *a = dir ? sN : sP, *b = dir ? sP : sN;
        const float2 from      = dir ? fwd : p0;
        float2 io              = dir ? bwd : fwd;
#if defined(LK_TILE_HIST)
        if (lane == 0) atomicAdd(&g_lk_tile_points[1], 1ull);
#endif
        const bool st          = lk_track_wave(P, a, b, from, io, S, lane, nullptr);
        if (dir) {
            bwd  = io;
            st_b = st;
        } else {
            fwd  = io;
            st_f = st;
        }
    }
    // The verdict on the point — isOnBorder, ptsDistance, undistortPoints — is k_lk_finish's, a THREAD per point: as the tail of this kernel it
    // was ~390 wave-instructions per point that every lane computed alike, most of them FP64 (five divisions of the undistortion's fixed-point
    // iteration, a square root): 5.5 % of the kernel's vector instructions and more of its time (round 6).
    if (lane == 0) {
        out_pts[i] = fwd;
        out_bwd[i] = bwd;
        status[i]  = (unsigned char) ((st_f && st_b) ? 1u : 0u); // (the backward pass is skipped for a lost or border point: st_b stays false)
    }
}

// isOnBorder (tracking.cc:847-849) and ptsDistance (tracking.cc:841-845) on the forward / backward results of k_lk_track_fb, then
// undistortPoints of the forward result (Camera::undistortPoints, camera.cc:72-74, of the point's own camera where a table is given); one
// thread per point.  bwd_undist holds the backward result on entry and, when the caller asked for
// undistorted points, the undistorted point on exit (the segmented tracker passes its undistorted-point array; the C entry point a scratch
// array or the caller's).
__global__ __launch_bounds__(256) void k_lk_finish(int n, const float2 *prev_pts, const float2 *out_pts, float2 *bwd_undist, unsigned char *status,
                                                   int want_undist, int has_cam, icg_camera cam, int img_w, int img_h, int seg_cap,
                                                   unsigned int seg_magic, const int32_t *seg_count, const icg_camera *cams, const int32_t *cam_idx) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    int s = 0;
    if (seg_count) {
        s = icg_div_by_magic(i, seg_magic);
        if (i - s * seg_cap >= seg_count[s]) return;
    }
    const float2 p0 = prev_pts[i], fwd = out_pts[i], bwd = bwd_undist[i];
    const bool border = (double) fwd.x < 5.0 || (double) fwd.y < 5.0 || ((double) fwd.x > (img_w - 5.0)) || ((double) fwd.y > (img_h - 5.0));
    const double ddx = (double) (bwd.x - p0.x), ddy = (double) (bwd.y - p0.y);
    const double dist = sqrt(ddx * ddx + ddy * ddy);
    status[i] = (unsigned char) ((status[i] && !border && dist < 0.5) ? 1u : 0u);
    if (!want_undist) return;
    // camera table (icg_set_cameras): the camera of the point's segment — its stream — in the tracker's launch, of cam_idx[i] in the
    // unsegmented one; without a table the by-value camera, the code of the single-camera entries as it was
    if (cams) {
        const icg_camera c = cams[seg_count ? s : cam_idx[i]];
        bwd_undist[i]      = cam_undistort(c, fwd);
    } else
        bwd_undist[i] = has_cam ? cam_undistort(cam, fwd) : fwd;
}

// order-preserving compaction indices (what reduceVector keeps, tracking.cc:831-839); single workgroup scan.
__global__ __launch_bounds__(1024) void k_keep_indices(int n, const unsigned char *status, int32_t *keep_idx, int32_t *n_keep) {
    __shared__ int wave_tot[16];
    __shared__ int base;
    const int t = threadIdx.x, lane = t & 63, wv = t >> 6;
    if (t == 0) base = 0;
    __syncthreads();
    for (int start = 0; start < n; start += 1024) {
        const int i   = start + t;
        const bool k  = i < n && status[i];
        const unsigned long long m = __ballot(k);
        const int pre = __popcll(m & ((1ull << lane) - 1ull));
        if (lane == 0) wave_tot[wv] = __popcll(m);
        __syncthreads();
        int off = base;
        for (int w = 0; w < wv; w++) off += wave_tot[w];
        if (k) keep_idx[off + pre] = i;
        __syncthreads();
        if (t == 0) {
            int s = 0;
            for (int w = 0; w < 16; w++) s += wave_tot[w];
            base += s;
        }
        __syncthreads();
    }
    if (t == 0) *n_keep = base;
}

// ---- host side ---------------------------------------------------------------------------------------------
static int check_slots(icg_ctx *ctx, int n, const int32_t *a, const int32_t *b) {
    for (int i = 0; i < n; i++)
        if (a[i] < 0 || a[i] >= ctx->cfg.n_slots || b[i] < 0 || b[i] >= ctx->cfg.n_slots)
            return icg_fail(ctx, ICG_ERR_INVALID, "slot index out of range at point %d", i);
    return 0;
}

extern "C" int icg_lk_track(icg_ctx *ctx, int n, const int32_t *prev_slot, const int32_t *next_slot, const float *prev_pts,
                            float *next_pts, uint8_t *status, float *err) {
    if (!ctx || n < 0) return ICG_ERR_INVALID;
    if (n == 0) return ICG_OK;
    if (!prev_slot || !next_slot || !prev_pts || !next_pts || !status) return ICG_ERR_INVALID;
    if (n > ctx->cfg.max_points) return icg_fail(ctx, ICG_ERR_CAPACITY, "%d points > max_points %d", n, ctx->cfg.max_points);
    int rc = check_slots(ctx, n, prev_slot, next_slot);
    if (rc) return rc;
    ICG_HIP(ctx, hipSetDevice(ctx->cfg.device));
    icg_call c(ctx);
    if ((rc = c.reserve((size_t) n * 64))) return rc;
    const int32_t *d_ps = c.in_zc(prev_slot, (size_t) n);
    const int32_t *d_ns = c.in_zc(next_slot, (size_t) n);
    const float2 *d_pp  = (const float2 *) c.in_zc(prev_pts, 2 * (size_t) n);
    float2 *d_np        = (float2 *) c.out_zc(next_pts, 2 * (size_t) n); // in/out: initial flow in, result out
    memcpy(d_np, next_pts, sizeof(float) * 2 * (size_t) n);
    unsigned char *d_st = c.out_zc(status, (size_t) n);
    float *d_err        = err ? c.out_zc(err, (size_t) n) : nullptr;
    ICG_LAUNCH_GUARD(c);
    {
        icg_prof_scope ps(ctx, "lk_track");
        hipLaunchKernelGGL(k_lk_track, dim3(icg_xcd_grid(n)), dim3(64), 0, ctx->stream, icg_make_pyr_desc(ctx), n, d_ps, d_ns, d_pp, d_np,
                           d_st, d_err);
    }
    ICG_HIP(ctx, hipGetLastError());
    return c.finish();
}

// the forward / backward track and its verdict of n points: k_lk_track_fb + k_lk_finish, asynchronous on the context's stream.  seg_count
// null: one list of n points; otherwise n = n_seg * seg_cap entries in segments (icg_lk_launch_segments).  bwd_undist: see k_lk_finish.
// cams / cam_idx: k_lk_finish's camera table and per-point index (null: the context's camera by value).
static void lk_fb_launch(icg_ctx *ctx, int n, int seg_cap, const int32_t *seg_count, bool want_undist, const int32_t *prev_slot, const int32_t *next_slot,
                         const float2 *prev, const float2 *guess, float2 *out, uint8_t *status, float2 *bwd_undist, const icg_camera *cams = nullptr,
                         const int32_t *cam_idx = nullptr) {
    const unsigned int seg_magic = seg_count ? icg_div_magic(seg_cap) : 0u; // (0: divisor 1, and what an unsegmented call passes)
#if defined(LK_TILE_HIST)
    static std::once_flag hist_once;
    std::call_once(hist_once, [] { atexit(lk_tile_hist_dump); });
#endif
    {
        icg_prof_scope ps(ctx, "lk_track_fb");
        hipLaunchKernelGGL(k_lk_track_fb, dim3(icg_xcd_grid(n)), dim3(64), 0, ctx->stream, icg_make_pyr_desc(ctx), n, prev_slot, next_slot, prev, guess,
                           seg_count, ctx->cfg.width, ctx->cfg.height, seg_cap, seg_magic, out, status, bwd_undist);
    }
    {
        icg_prof_scope ps(ctx, "lk_finish");
        hipLaunchKernelGGL(k_lk_finish, dim3((n + 255) / 256), dim3(256), 0, ctx->stream, n, prev, (const float2 *) out, bwd_undist, status,
                           want_undist ? 1 : 0, ctx->has_cam ? 1 : 0, ctx->cam, ctx->cfg.width, ctx->cfg.height, seg_cap, seg_magic, seg_count, cams,
                           cam_idx);
    }
}

// icg_lk_track_fb and icg_lk_track_fb_cams: one body; cam_idx null is the single-camera entry
static int lk_track_fb_entry(icg_ctx *ctx, int n, const int32_t *prev_slot, const int32_t *next_slot, const float *prev_pts, const float *guess_pts,
                             const int32_t *cam_idx, float *out_pts, uint8_t *status, float *out_undist, int32_t *keep_idx, int32_t *n_keep) {
    if (n == 0) {
        if (n_keep) *n_keep = 0;
        return ICG_OK;
    }
    if (!prev_slot || !next_slot || !prev_pts || !guess_pts || !out_pts || !status) return ICG_ERR_INVALID;
    if ((keep_idx == nullptr) != (n_keep == nullptr)) return ICG_ERR_INVALID;
    if (!cam_idx && out_undist && !ctx->has_cam) return icg_fail(ctx, ICG_ERR_INVALID, "out_undist requested but camera not set");
    if (cam_idx) {
        const int n_cams = (int) ctx->cams.size();
        for (int i = 0; i < n; i++)
            if (cam_idx[i] < 0 || cam_idx[i] >= n_cams) return icg_fail(ctx, ICG_ERR_INVALID, "cam_idx[%d] = %d outside the table of %d cameras", i, cam_idx[i], n_cams);
    }
    if (n > ctx->cfg.max_points) return icg_fail(ctx, ICG_ERR_CAPACITY, "%d points > max_points %d", n, ctx->cfg.max_points);
    int rc = check_slots(ctx, n, prev_slot, next_slot);
    if (rc) return rc;
    ICG_HIP(ctx, hipSetDevice(ctx->cfg.device));
    icg_call c(ctx);
    if ((rc = c.reserve((size_t) n * (cam_idx ? 112 : 104)))) return rc;
    const int32_t *d_ps = c.in_zc(prev_slot, (size_t) n);
    const int32_t *d_ns = c.in_zc(next_slot, (size_t) n);
    const float2 *d_pp  = (const float2 *) c.in_zc(prev_pts, 2 * (size_t) n);
    const float2 *d_gs  = (const float2 *) c.in_zc(guess_pts, 2 * (size_t) n);
    const int32_t *d_ci = cam_idx ? c.in_zc(cam_idx, (size_t) n) : nullptr;
    float2 *d_out       = (float2 *) c.out_zc(out_pts, 2 * (size_t) n);
    unsigned char *d_st = c.out_zc(status, (size_t) n);
    // (the backward results travel from k_lk_track_fb to k_lk_finish in the undistorted-point array, or in device scratch when none was asked for)
    float2 *d_und       = out_undist ? (float2 *) c.out_zc(out_undist, 2 * (size_t) n) : (float2 *) c.out<float>(nullptr, 2 * (size_t) n);
    int32_t *d_keep     = keep_idx ? c.out_zc(keep_idx, (size_t) n) : nullptr;
    int32_t *d_nkeep    = keep_idx ? c.out_zc(n_keep, 1) : nullptr;
    ICG_LAUNCH_GUARD(c);
    lk_fb_launch(ctx, n, 0, nullptr, out_undist != nullptr, d_ps, d_ns, d_pp, d_gs, d_out, d_st, d_und, cam_idx ? ctx->d_cams : nullptr, d_ci);
    if (keep_idx) {
        icg_prof_scope ps(ctx, "keep_indices");
        hipLaunchKernelGGL(k_keep_indices, dim3(1), dim3(1024), 0, ctx->stream, n, d_st, d_keep, d_nkeep);
    }
    ICG_HIP(ctx, hipGetLastError());
    return c.finish();
}

extern "C" int icg_lk_track_fb(icg_ctx *ctx, int n, const int32_t *prev_slot, const int32_t *next_slot,
                               const float *prev_pts, const float *guess_pts, float *out_pts, uint8_t *status,
                               float *out_undist, int32_t *keep_idx, int32_t *n_keep) {
    if (!ctx || n < 0) return ICG_ERR_INVALID;
    return lk_track_fb_entry(ctx, n, prev_slot, next_slot, prev_pts, guess_pts, nullptr, out_pts, status, out_undist, keep_idx, n_keep);
}

// out_undist[i] under camera cam_idx[i] of the context's table (icg_set_cameras): the reference constructs a Tracking per camera
// (tracking/tracking.h:51) and undistorts with that camera (tracking.cc:423, 520-524; Camera::undistortPoints, camera.cc:72-74)
extern "C" int icg_lk_track_fb_cams(icg_ctx *ctx, int n, const int32_t *prev_slot, const int32_t *next_slot, const float *prev_pts,
                                    const float *guess_pts, const int32_t *cam_idx, float *out_pts, uint8_t *status, float *out_undist,
                                    int32_t *keep_idx, int32_t *n_keep) {
    if (!ctx || n < 0) return ICG_ERR_INVALID;
    if (ctx->cams.empty()) return icg_fail(ctx, ICG_ERR_INVALID, "icg_lk_track_fb_cams: no camera table (icg_set_cameras)");
    if (!cam_idx) return icg_fail(ctx, ICG_ERR_INVALID, "icg_lk_track_fb_cams: NULL cam_idx");
    return lk_track_fb_entry(ctx, n, prev_slot, next_slot, prev_pts, guess_pts, cam_idx, out_pts, status, out_undist, keep_idx, n_keep);
}

// Segmented launch for the device-resident tracker (tracker.hip): every array is device memory laid out as n_seg segments of seg_cap
// entries, d_count[s] of them valid; asynchronous on the context's stream (the tracker's next stage kernel is stream-ordered behind it).
int icg_lk_launch_segments(icg_ctx *ctx, int n_seg, int seg_cap, const int32_t *d_count, const int32_t *d_prev_slot, const int32_t *d_next_slot,
                           const float2 *d_prev, const float2 *d_guess, float2 *d_out, uint8_t *d_status, float2 *d_undist, const icg_camera *d_seg_cams) {
    if (!d_seg_cams && !ctx->has_cam) return icg_fail(ctx, ICG_ERR_INVALID, "camera not set");
    if (n_seg < 1 || seg_cap < 1 || (unsigned long long) n_seg * seg_cap * seg_cap >= (1ull << 32)) // (icg_div_magic is exact for entry * seg_cap < 2^32)
        return icg_fail(ctx, ICG_ERR_INVALID, "%d segments of %d entries: the segment decode needs n_seg * seg_cap^2 < 2^32", n_seg, seg_cap);
    lk_fb_launch(ctx, n_seg * seg_cap, seg_cap, d_count, true, d_prev_slot, d_next_slot, d_prev, d_guess, d_out, d_status, d_undist, d_seg_cams);
    ICG_HIP(ctx, hipGetLastError());
    return ICG_OK;
}
