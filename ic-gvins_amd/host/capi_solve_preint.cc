// C entry points of libicgvins_host.so: the preintegration factor with its trigonometric part split out (Preintegration::evaluateGiven), for
// tests that feed the device's resident evaluation (icg_preint_set / icg_preint_evaluate_resident) from the host's own values (the per-factor
// body: preint_eval_split_factor, capi_preint_streams.h), and WindowSolverBatch::setDevicePreintegration on the windows of
// icgh_backend_solve_prior_batch (solve_vio_windows, capi_solve_windows.h).
#include <memory>
#include <string>

#include "capi_preint_streams.h"
#include "capi_solve_windows.h"

using namespace icg;

extern "C" {

// The n intervals (variant, offsets, imu, state0, params9 as icgh_backend_preint) are integrated (one icg_preint_batch launch) and every
// factor is evaluated at its point (points: 32 per factor = pose0[7] mix0[9] pose1[7] mix1[9]) twice on the host:
//   r_eval 15, J_eval 480 (15x7 | 15x9 | 15x7 | 15x9)   Preintegration::evaluate
//   r_given, J_given                                    correctionQuaternion / earthRateQuaternion + evaluateGiven; with q_corr_in (optional,
//                                                       4 per factor) that quaternion takes the place of correctionQuaternion's
//   q_corr 4, q_nn 4                                    the accessors' quaternions (x, y, z, w)
//   cur_state 16                                        the integration's end state
// and what icg_preint_set takes is returned per factor: sqrt_info 225, delta_state 16, jac 225, delta_time 1, env 4 (gravity, iewn),
// pn_offsets n+1 and pn (rows of 4: dt, position; pn_cap rows of room, the complete rows evaluate() sums).  ok[k] = 1: both evaluations
// succeeded (0: not integrated or singular covariance, zero rows).  Returns -2 when the integration fails, -3 when pn does not fit.
int icgh_backend_preint_eval_split(int variant, int n, const int32_t *offsets, const double *imu, const double *state0, const double *params9,
                                   const double *points, const double *q_corr_in, double *cur_state, double *r_eval, double *J_eval, double *r_given, double *J_given,
                                   double *q_corr, double *q_nn, double *sqrt_info, double *delta_state, double *jac, double *delta_time, double *env,
                                   int32_t *pn_offsets, double *pn, int pn_cap, int32_t *ok, char *err, int errlen) {
    return guarded(err, errlen, [&] {
        TempCtx T(0);
        auto P = preint_params(params9);
        vector<std::shared_ptr<Preintegration>> pre;
        vector<Preintegration *> raw;
        for (int k = 0; k < n; k++) {
            pre.push_back(preint_interval(variant, P, offsets, imu, k, state0 + 16 * (size_t) k));
            raw.push_back(pre.back().get());
        }
        std::string e;
        if (!Preintegration::integrateBatch(T.ctx, raw, &e)) {
            set_err(err, errlen, e.c_str());
            return -2;
        }
        const size_t N = (size_t) n;
        memset(r_eval, 0, sizeof(double) * 15 * N), memset(J_eval, 0, sizeof(double) * 480 * N);
        memset(r_given, 0, sizeof(double) * 15 * N), memset(J_given, 0, sizeof(double) * 480 * N);
        pn_offsets[0] = 0;
        for (size_t k = 0; k < N; k++) {
            const Preintegration &p = *pre[k];
            ok[k] = preint_eval_split_factor(p, points + 32 * k, q_corr_in ? q_corr_in + 4 * k : nullptr, nullptr, r_eval + 15 * k, J_eval + 480 * k, r_given + 15 * k,
                                             J_given + 480 * k, q_corr + 4 * k, q_nn + 4 * k, sqrt_info + 225 * k, env + 4 * k)
                        ? 1
                        : 0;
            preint_put_state(p.currentState(), cur_state + 16 * k);
            preint_put_state(p.deltaState(), delta_state + 16 * k);
            memcpy(jac + 225 * k, p.jacobian().data(), sizeof(double) * 225);
            delta_time[k] = p.deltaTime();
            const size_t rows = p.pnRows().size() / 4;
            if ((size_t) pn_offsets[k] + rows > (size_t) pn_cap) {
                set_err(err, errlen, "pn does not fit");
                return -3;
            }
            memcpy(pn + 4 * (size_t) pn_offsets[k], p.pnRows().data(), sizeof(double) * 4 * rows);
            pn_offsets[k + 1] = pn_offsets[k] + (int32_t) rows;
        }
        return 0;
    });
}

// icgh_backend_solve_prior_batch (capi_solve_prior.cc: the same windows, built by the same code, the same arguments up to solve_ms) with
//   variant           0 Normal / 1 Earth for every interval of the call
//   preint_robust     optional, per window: != 0 gives the window's preintegration factors a Huber loss of that delta (such a factor stays on
//                     the pool in every mode)
//   preint_on_device  optional out: the preintegration factors that were resident on the device in the solve
// mode: 0 - 3 as there; 4 = mode 2 plus the device preintegration (setDevicePreintegration), 5 = mode 3 plus it; 4 + 16: the preintegration
// switch with the reduced solve but WITHOUT setDeviceHostPart, which solve() refuses by name (-3); other values: -1.  A mode whose C entries
// are not in the build computes nothing: -4 and the entry's name first.
int icgh_backend_solve_preint_batch(int W, const int32_t *n_intervals, const int32_t *const *offsets, const double *const *imu, const double *params9,
                                    double *const *states16, const int32_t *n_fac, const double *const *obs_soa, const int32_t *const *idx_i,
                                    const int32_t *const *idx_j, const int32_t *const *idx_lm, double *const *ext, const int32_t *n_lm, double *const *invdepth,
                                    double *td, const double *const *prior_pose0, const double *const *prior_mix0, double prior_weight, double huber, int iters,
                                    const int32_t *prior_r, const int32_t *prior_nb, const int32_t *const *prior_size, const int32_t *const *prior_index,
                                    const int32_t *const *prior_param, const double *const *prior_x0, const double *const *prior_J0,
                                    const double *const *prior_e0, const double *prior_robust, const int32_t *const *state_const, double *summary4,
                                    double *prior_cost, double *solve_ms, int variant, const double *preint_robust, int32_t *preint_on_device, int mode, char *err,
                                    int errlen) {
    return guarded(err, errlen, [&] {
        const bool without_parts = mode == 4 + 16;
        if (without_parts) mode = 4;
        if (mode < 0 || mode > 5 || (variant != 0 && variant != 1)) {
            set_err(err, errlen, "mode must be 0 (host), 1 (device reduced solve), 2 (and device host part), 3 (and device prior), 4 (mode 2 and device "
                                 "preintegration) or 5 (mode 3 and device preintegration); variant 0 (Normal) or 1 (Earth)");
            return -1;
        }
        const VioBatchArgs a{W,       variant,  n_intervals, offsets,  imu,      params9,  nullptr,     nullptr,  nullptr,  nullptr,      nullptr,
                             nullptr, nullptr,  nullptr,     states16, n_fac,    obs_soa,  idx_i,       idx_j,    idx_lm,   ext,          n_lm,
                             invdepth, td,      prior_pose0, prior_mix0, prior_weight, huber, iters,    prior_r,  prior_nb, prior_size,   prior_index,
                             prior_param, prior_x0, prior_J0, prior_e0, prior_robust, preint_robust, state_const, 0, nullptr, nullptr,    nullptr,
                             nullptr, summary4, prior_cost,  solve_ms, preint_on_device, nullptr, nullptr};
        return solve_vio_windows(a, mode, without_parts, false, err, errlen);
    });
}

} // extern "C"
