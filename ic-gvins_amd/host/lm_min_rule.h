// The smallest landmark diagonal of one window, the value of the first conditioning guard of the structured marginalization
// (MarginalizationBatch::marginalize step 4, factors/marginalization_info.h:170-192), as a rule 64 lanes can follow.  The host loop defines it:
//     mn = h[0];  for every h[l] in landmark order: mn = (h[l] < mn) ? h[l] : mn;        (0.0 for a window without landmarks)
// A NaN in h[0] stays (nothing compares below it); a NaN anywhere else never compares below mn and is ignored.  So the result is h[0] when
// that is NaN and the smallest non-NaN value otherwise, and that can be taken in any grouping: every lane starts from +inf (the value no
// element compares above), takes its elements with the loop's own step, lanes are joined with the same step — no operand of a join is a NaN —
// and h[0] is looked at once more at the end.  Equal to the loop as a VALUE; which of two zeros of different sign comes out depends on the
// grouping (the guard tests > 1e-6).
// Shared by k_lm_min_w (csrc/reproj_schur.hip) and its host twin lmMinOfWindow (one function walks the lanes of the kernel in order).
#pragma once
#include <limits>

#if defined(__HIPCC__)
#define ICG_LM_MIN_FN __host__ __device__ __forceinline__
#else
#define ICG_LM_MIN_FN inline
#endif

namespace icg_lm_min {

constexpr int kLanes = 64;

ICG_LM_MIN_FN double start() { return std::numeric_limits<double>::infinity(); }
// the loop's step: x joins mn (a NaN x does not)
ICG_LM_MIN_FN double take(double mn, double x) { return x < mn ? x : mn; }
// first = h[0], m = the joined lanes (never a NaN)
ICG_LM_MIN_FN double finish(double first, double m) { return first != first ? first : m; }

// the kernel's schedule on the host: lane t takes landmarks t, t + 64, ... in order, the lanes are joined by the xor butterfly 32, 16, ... 1
// (lane 0's value), then finish.  h[l * stride] is landmark l's diagonal.
inline double lmMinOfWindow(const double *h, int L, long stride = 1) {
    if (L <= 0) return 0.0;
    double m[kLanes];
    for (int t = 0; t < kLanes; t++) {
        m[t] = start();
        for (int l = t; l < L; l += kLanes) m[t] = take(m[t], h[(long) l * stride]);
    }
    for (int k = kLanes / 2; k >= 1; k >>= 1) {
        double o[kLanes];
        for (int t = 0; t < kLanes; t++) o[t] = m[t ^ k];
        for (int t = 0; t < kLanes; t++) m[t] = take(m[t], o[t]);
    }
    return finish(h[0], m[0]);
}

} // namespace icg_lm_min
