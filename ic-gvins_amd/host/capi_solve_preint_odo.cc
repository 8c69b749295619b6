// C entry points of libicgvins_host.so: the odometer preintegration factor with its trigonometric part split out
// (PreintegrationOdo::evaluateGiven), for tests that feed the device's resident evaluation (icg_preint_odo_set /
// icg_preint_odo_evaluate_resident) from the host's own values, and WindowSolverBatch::setDevicePreintegration on visual-inertial windows
// whose motion factors are PreintegrationOdoFactors.  The 19-state twin of capi_solve_preint.cc; the per-factor body of the split entry is shared
// (preint_eval_split_factor, capi_preint_streams.h).
#include <chrono>
#include <memory>
#include <string>

#include "capi_preint_streams.h"
#include "capi_solve_windows.h"

using namespace icg;

extern "C" {

// n factors built from GIVEN integration results (setIntegrationResult; no device is touched): per factor variant (2 Odo, 3 EarthOdo),
// delta_state 20, jac 361, cov 361, delta_time 1 in icg_preint_odo_batch's layout, iewn 3 (the interval's Earth rate), and for an EarthOdo
// factor the rows [pn_offsets[f], pn_offsets[f+1]) of pn (rows of 4: dt, position; not read for an Odo factor).  params19 as
// icgh_backend_preint_odo.  Every factor is evaluated at its point (points: 34 per factor = pose0[7] mix0[10] pose1[7] mix1[10]) twice on the
// host:
//   r_eval 19, J_eval 646 (19x7 | 19x10 | 19x7 | 19x10)   PreintegrationOdo::evaluate
//   r_given, J_given                                      correctionQuaternion / earthRateQuaternion + evaluateGiven; with q_corr_in
//                                                         (optional, 4 per factor) that quaternion takes the place of
//                                                         correctionQuaternion's, with q_nn_in (optional) of earthRateQuaternion's
//   q_corr 4, q_nn 4                                      the accessors' quaternions (x, y, z, w)
// and what icg_preint_odo_set takes besides the inputs above is returned per factor: sqrt_info 361 (zeros for a singular covariance), env 4
// (gravity, iewn).  ok[k] = 1: both evaluations succeeded (0: singular covariance, zero rows).  -1: a variant that is neither 2 nor 3.
int icgh_backend_preint_odo_eval_split(int n, const int32_t *variant, const double *params19, const double *delta_state, const double *jac,
                                       const double *cov, const double *delta_time, const int32_t *pn_offsets, const double *pn, const double *iewn,
                                       const double *points, const double *q_corr_in, const double *q_nn_in, double *r_eval, double *J_eval,
                                       double *r_given, double *J_given, double *q_corr, double *q_nn, double *sqrt_info, double *env, int32_t *ok,
                                       char *err, int errlen) {
    return guarded(err, errlen, [&] {
        auto P         = odo_params19(params19);
        const size_t N = (size_t) n;
        memset(r_eval, 0, sizeof(double) * 19 * N), memset(J_eval, 0, sizeof(double) * 646 * N);
        memset(r_given, 0, sizeof(double) * 19 * N), memset(J_given, 0, sizeof(double) * 646 * N);
        for (size_t k = 0; k < N; k++) {
            if (variant[k] != 2 && variant[k] != 3) {
                set_err(err, errlen, ("factor " + std::to_string(k) + ": variant " + std::to_string(variant[k]) + " is neither 2 (Odo) nor 3 (EarthOdo)").c_str());
                return -1;
            }
            const int rows = variant[k] == 3 && pn_offsets ? pn_offsets[k + 1] - pn_offsets[k] : 0;
            const auto obj = odo_from_result(P, variant[k], delta_state + 20 * k, jac + 361 * k, cov + 361 * k, delta_time[k],
                                             rows > 0 ? pn + 4 * (size_t) pn_offsets[k] : nullptr, rows, iewn + 3 * k);
            ok[k] = preint_eval_split_factor(*obj, points + 34 * k, q_corr_in ? q_corr_in + 4 * k : nullptr, q_nn_in ? q_nn_in + 4 * k : nullptr, r_eval + 19 * k,
                                             J_eval + 646 * k, r_given + 19 * k, J_given + 646 * k, q_corr + 4 * k, q_nn + 4 * k, sqrt_info + 361 * k, env + 4 * k)
                        ? 1
                        : 0;
        }
        return 0;
    });
}

// The visual-inertial windows of icgh_backend_solve_preint_batch (solve_vio_windows, capi_solve_windows.h: the same blocks and the same
// order of the residual blocks) with 17-wide states (p3, q4 xyzw, v3, bg3, ba3, sodo), 10-wide mix blocks and PreintegrationOdoFactors.
// The integration results are GIVEN, per window w and interval k of it (n_intervals[w] intervals between its n_intervals[w] + 1 states):
// delta[w] 20 per interval, jac[w] and cov[w] 361, dt[w] 1, iewn[w] 3, in icg_preint_odo_batch's layout; pn[w] rows of 4 with pn_off[w]
// (n_intervals[w] + 1 offsets: interval k owns rows [pn_off[w][k], pn_off[w][k+1]); read for variant 3 only, both may be NULL otherwise) —
// so the same entry runs on a C ABI without icg_preint_odo_batch and on the device.  variant: 2 Odo / 3 EarthOdo for every interval of
// the call.  prior_mix0[w]: 10 values.  The optional marginalization priors name pose (7) and mix (10) blocks: prior_param = 2 * state (+ 1
// for the mix block).  preint_robust, state_const, summary4, prior_cost, solve_ms as there; odo_on_device (optional out): the odometer
// factors that were resident on the device in the solve.
// mode: 0 host; 1 device reduced solve; 2 and device host part; 3 and device prior; 4 = mode 2 plus the device preintegration
// (setDevicePreintegration), 5 = mode 3 plus it; 4 + 16: the switch WITHOUT setDeviceHostPart, which solve() refuses by name (-3); other
// values, or another variant: -1.  A mode whose C entries are not in the build computes nothing: -4 and the entry's name first.
// -3: solve() failed (err: its message); -5: prepare() or a prior's evaluation failed.
int icgh_backend_solve_preint_odo_batch(int W, const int32_t *n_intervals, const double *const *delta, const double *const *jac, const double *const *cov,
                                        const double *const *dt, const double *const *iewn, const int32_t *const *pn_off, const double *const *pn,
                                        const double *params19, double *const *states17, const int32_t *n_fac, const double *const *obs_soa,
                                        const int32_t *const *idx_i, const int32_t *const *idx_j, const int32_t *const *idx_lm, double *const *ext,
                                        const int32_t *n_lm, double *const *invdepth, double *td, const double *const *prior_pose0,
                                        const double *const *prior_mix0, double prior_weight, double huber, int iters, const int32_t *prior_r,
                                        const int32_t *prior_nb, const int32_t *const *prior_size, const int32_t *const *prior_index,
                                        const int32_t *const *prior_param, const double *const *prior_x0, const double *const *prior_J0,
                                        const double *const *prior_e0, const double *prior_robust, const int32_t *const *state_const, double *summary4,
                                        double *prior_cost, double *solve_ms, int variant, const double *preint_robust, int32_t *odo_on_device, int mode,
                                        char *err, int errlen) {
    return guarded(err, errlen, [&] {
        const bool without_parts = mode == 4 + 16;
        if (without_parts) mode = 4;
        if (mode < 0 || mode > 5 || (variant != 2 && variant != 3)) {
            set_err(err, errlen, "mode must be 0 (host), 1 (device reduced solve), 2 (and device host part), 3 (and device prior), 4 (mode 2 and device "
                                 "preintegration) or 5 (mode 3 and device preintegration); variant 2 (Odo) or 3 (EarthOdo)");
            return -1;
        }
        if (odo_on_device) *odo_on_device = 0;
        const VioBatchArgs a{W,       variant,  n_intervals, nullptr,  nullptr,  nullptr,  delta,       jac,      cov,      dt,           iewn,
                             pn_off,  pn,       params19,    states17, n_fac,    obs_soa,  idx_i,       idx_j,    idx_lm,   ext,          n_lm,
                             invdepth, td,      prior_pose0, prior_mix0, prior_weight, huber, iters,    prior_r,  prior_nb, prior_size,   prior_index,
                             prior_param, prior_x0, prior_J0, prior_e0, prior_robust, preint_robust, state_const, 0, nullptr, nullptr,    nullptr,
                             nullptr, summary4, prior_cost,  solve_ms, nullptr,  odo_on_device, nullptr};
        return solve_vio_windows(a, mode, without_parts, false, err, errlen);
    });
}

} // extern "C"
