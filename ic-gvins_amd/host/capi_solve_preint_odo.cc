// C entry points of libicgvins_host.so: the odometer preintegration factor with its trigonometric part split out
// (PreintegrationOdo::evaluateGiven), for tests that feed the device's resident evaluation (icg_preint_odo_set /
// icg_preint_odo_evaluate_resident) from the host's own values, and WindowSolverBatch::setDevicePreintegration on visual-inertial windows
// whose motion factors are PreintegrationOdoFactors.  The 19-state twin of capi_solve_preint.cc.
#include <chrono>
#include <memory>
#include <string>

#include "preintegration_odo.h"
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
            const PreintegrationOdo &p = *obj;
            const double *ep    = points + 34 * k;
            const double *pp[4] = {ep, ep + 7, ep + 17, ep + 24};
            double *je[4] = {J_eval + 646 * k, J_eval + 646 * k + 133, J_eval + 646 * k + 323, J_eval + 646 * k + 456};
            double *jg[4] = {J_given + 646 * k, J_given + 646 * k + 133, J_given + 646 * k + 323, J_given + 646 * k + 456};
            p.correctionQuaternion(pp[1], q_corr + 4 * k);
            p.earthRateQuaternion(q_nn + 4 * k);
            const bool a = p.evaluate(pp, r_eval + 19 * k, je);
            const bool b = p.evaluateGiven(pp, q_corr_in ? q_corr_in + 4 * k : q_corr + 4 * k, q_nn_in ? q_nn_in + 4 * k : q_nn + 4 * k, r_given + 19 * k, jg);
            ok[k]        = a && b ? 1 : 0;
            memcpy(sqrt_info + 361 * k, p.sqrtInformation().data(), sizeof(double) * 361);
            env[4 * k] = p.gravity();
            for (int i = 0; i < 3; i++) env[4 * k + 1 + i] = p.earthRate()[i];
        }
        return 0;
    });
}

// The visual-inertial windows of icgh_backend_solve_preint_batch (solve_prior_windows, capi_solve_windows.h: the same blocks and the same
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
        const bool prior = mode == 3 || mode == 5, preint = mode >= 4;
        if (odo_on_device) *odo_on_device = 0;
        // (the entry a mode adds is named first: a build without any of them says what that mode itself is missing)
        if (preint && WindowSolverBatch::devicePreintegrationOdoMissing()) {
            set_err(err, errlen, (std::string(WindowSolverBatch::devicePreintegrationOdoMissing()) + " is not in this build").c_str());
            return -4;
        }
        if (preint && !WindowSolverBatch::devicePreintegrationAvailable()) {
            set_err(err, errlen, (std::string(WindowSolverBatch::devicePreintegrationMissing()) + " is not in this build").c_str());
            return -4;
        }
        if (prior && !WindowSolverBatch::devicePriorAvailable()) {
            set_err(err, errlen, MarginalizationPriorSet::residentAvailable() ? "icg_reproj_host_parts_build_prior is not in this build"
                                                                              : "icg_marg_prior_evaluate_resident is not in this build");
            return -4;
        }
        if (mode >= 2 && !WindowSolverBatch::deviceHostPartAvailable()) {
            set_err(err, errlen, "icg_reproj_host_parts_build is not in this build");
            return -4;
        }
        if (mode >= 1 && !WindowSolverBatch::deviceReducedSolveAvailable()) {
            set_err(err, errlen, "icg_reproj_solve_windows is not in this build");
            return -4;
        }
        auto params = odo_params19(params19);
        TempCtx T(0);
        struct Win {
            int K;
            vector<double> pose, mix;
            vector<std::shared_ptr<PreintegrationOdo>> pre;
        };
        vector<Win> wins((size_t) W);
        for (int w = 0; w < W; w++) {
            Win &V = wins[(size_t) w];
            V.K    = n_intervals[w] + 1;
            V.pose.resize((size_t) V.K * 7), V.mix.resize((size_t) V.K * 10);
            for (int k = 0; k < V.K; k++)
                memcpy(&V.pose[7 * (size_t) k], states17[w] + 17 * (size_t) k, sizeof(double) * 7), memcpy(&V.mix[10 * (size_t) k], states17[w] + 17 * (size_t) k + 7, sizeof(double) * 10);
            for (int k = 0; k < n_intervals[w]; k++) {
                const size_t j = (size_t) k;
                const int rows = variant == 3 && pn_off && pn_off[w] ? pn_off[w][k + 1] - pn_off[w][k] : 0;
                V.pre.push_back(odo_from_result(params, variant, delta[w] + 20 * j, jac[w] + 361 * j, cov[w] + 361 * j, dt[w][j],
                                                rows > 0 ? pn[w] + 4 * (size_t) pn_off[w][k] : nullptr, rows, iewn[w] + 3 * j));
            }
        }
        vector<std::unique_ptr<ReprojectionFactor>> factors;
        WindowSolverBatch solver(0, huber);
        solver.setDeviceReducedSolve(mode >= 1);
        solver.setDeviceHostPart(mode >= 2 && !without_parts);
        solver.setDevicePrior(prior);
        solver.setDevicePreintegration(preint);
        vector<int> prior_id((size_t) W, -1);
        for (int w = 0; w < W; w++) {
            const OnBatchWindow win{solver, solver.addWindow()};
            Win &V    = wins[(size_t) w];
            const int K = V.K;
            double *P = V.pose.data(), *M = V.mix.data();
            for (int k = 0; k < K; k++) win.addParameterBlock(P + 7 * (size_t) k, 7, true), win.addParameterBlock(M + 10 * (size_t) k, 10);
            win.addParameterBlock(ext[w], 7, true);
            for (int l = 0; l < n_lm[w]; l++) win.addParameterBlock(invdepth[w] + l, 1);
            win.addParameterBlock(td + w, 1);
            win.setParameterBlockConstant(ext[w]);
            win.setParameterBlockConstant(td + w);
            for (int k = 0; state_const && state_const[w] && k < K; k++)
                if (state_const[w][k]) win.setParameterBlockConstant(P + 7 * (size_t) k), win.setParameterBlockConstant(M + 10 * (size_t) k);
            reprojections_from_soa(obs_soa[w], n_fac[w], 0, n_fac[w], idx_i[w], idx_j[w], idx_lm[w], P, ext[w], invdepth[w], td + w, factors, window_add(solver, win.w));
            std::shared_ptr<ceres::LossFunction> preint_loss;
            if (preint_robust && preint_robust[w] != 0) preint_loss = std::make_shared<HuberLossHip>(preint_robust[w]);
            for (int k = 0; k + 1 < K; k++)
                win.addResidualBlock(std::make_shared<PreintegrationOdoFactor>(V.pre[(size_t) k]), preint_loss,
                                     {P + 7 * (size_t) k, M + 10 * (size_t) k, P + 7 * (size_t) (k + 1), M + 10 * (size_t) (k + 1)});
            pose_prior(win, P, prior_pose0[w], prior_weight);
            if (prior_r && prior_r[w] > 0) {
                // (between the two ordinary priors: a resident prior is not the window's last host block)
                vector<double *> blocks;
                for (int b = 0; b < prior_nb[w]; b++) {
                    const int code = prior_param[w][b], k = code / 2;
                    if (code < 0 || k >= K || prior_size[w][b] != (code % 2 ? 10 : 7)) {
                        set_err(err, errlen, ("window " + std::to_string(w) + ": prior block " + std::to_string(b) + " does not name a pose (7) or mix (10) block").c_str());
                        return -1;
                    }
                    blocks.push_back(code % 2 ? M + 10 * (size_t) k : P + 7 * (size_t) k);
                }
                std::shared_ptr<ceres::LossFunction> loss;
                if (prior_robust && prior_robust[w] != 0) loss = std::make_shared<HuberLossHip>(prior_robust[w]);
                prior_id[(size_t) w] = win.addResidualBlock(
                    std::make_shared<ArrayPriorFactor>(prior_r[w], prior_nb[w], prior_size[w], prior_index[w], prior_x0[w], prior_J0[w], prior_e0[w]), loss, blocks);
            }
            win.addResidualBlock(std::make_shared<OdoMixPriorFactor>(prior_mix0[w], prior_weight), nullptr, {M});
        }
        auto prior_costs = [&](int at) {
            for (int w = 0; w < W && prior_cost; w++) {
                prior_cost[2 * (size_t) w + at] = 0.0;
                if (prior_id[(size_t) w] >= 0 && !solver.evaluateResidualBlock(w, prior_id[(size_t) w], false, prior_cost + 2 * (size_t) w + at)) return false;
            }
            return true;
        };
        if (!solver.prepare() || !prior_costs(0)) {
            set_err(err, errlen, solver.error().empty() ? "a prior failed to evaluate" : solver.error().c_str());
            return -5;
        }
        const auto t0 = std::chrono::steady_clock::now();
        WindowSolverBatch::Options opt;
        vector<WindowSolverBatch::Summary> sum;
        opt.max_num_iterations = iters;
        if (!solver.solve(opt, &sum)) {
            set_err(err, errlen, solver.error().c_str());
            return -3;
        }
        if (solve_ms) *solve_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        if (odo_on_device) *odo_on_device = solver.odometerPreintegrationsOnDevice();
        if (!prior_costs(1)) {
            set_err(err, errlen, "a prior failed to evaluate");
            return -5;
        }
        for (int w = 0; w < W; w++) {
            put_summary4(sum[(size_t) w], summary4 + 4 * (size_t) w);
            const Win &V = wins[(size_t) w];
            for (int k = 0; k < V.K; k++)
                memcpy(states17[w] + 17 * (size_t) k, &V.pose[7 * (size_t) k], sizeof(double) * 7), memcpy(states17[w] + 17 * (size_t) k + 7, &V.mix[10 * (size_t) k], sizeof(double) * 10);
        }
        return 0;
    });
}

} // extern "C"
