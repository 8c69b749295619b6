// C entry points of libicgvins_host.so: the navigation factors of the product (nav_factors.h) for tests and probes, alone
// (icgh_backend_nav_eval) and in the batched window solve (icgh_backend_solve_nav_batch: WindowSolverBatch::setDeviceNavFactors).  Flat layouts as
// icg_nav_set / icg_nav_evaluate_resident take them: kind 0..5 per member, its constants at aux + aux_off[f] (aux_off has n + 1 entries),
// its parameter block at points + point_off[f]; results concatenated in member order (nr residuals, nr x width Jacobian entries).
#include <memory>
#include <string>

#include "nav_factors.h"
#include "capi_solve_windows.h"

using namespace icg;

namespace {
std::shared_ptr<ceres::CostFunction> make_nav_factor(int kind, const double *a) {
    switch (kind) {
    case 0: {
        GNSS g;
        g.blh = Vector3d(a[0], a[1], a[2]), g.std = Vector3d(a[3], a[4], a[5]);
        return std::make_shared<GnssFactor>(g, Vector3d(a[6], a[7], a[8]));
    }
    case 1: return std::make_shared<ImuErrorFactor>();
    case 2: return std::make_shared<ImuPosePriorFactor>(a, a + 7);
    case 3: return std::make_shared<ImuMixPriorFactor>(a, a + 9);
    case 4: return std::make_shared<ImuErrorFactor>(2);
    case 5: return std::make_shared<ImuMixPriorFactor>(a, a + 10, 2);
    }
    throw std::runtime_error("kind " + std::to_string(kind) + " is outside 0..5");
}
} // namespace

extern "C" {

// Every member through the product class's Evaluate and, where it is marked, through the Ceres corrector.  Outputs, concatenated: r / J (the
// class's own), r_corr / J_corr (what ResidualBlockInfo::Evaluate holds; equal to r / J for an unmarked member), corr 3 per member
// (sqrt_rho1, alpha_sq_norm, residual_scaling; 1, 0, 1 for an unmarked member), sq_norm per member (sum_k r[k]^2, k ascending), shape 3 per
// member (kind as NavFactor reports it, nr, width).  huber (NULL: no member is marked): huber[f] != 0 marks member f.
//   corr_in == NULL  the marked member carries HuberLoss(huber[f]); r_corr / J_corr are ResidualBlockInfo::Evaluate's, corr is
//                    correctorScalars of that loss at the member's sq_norm
//   corr_in != NULL  the twin of icg_nav_correct_resident: the marked member is corrected with the three scalars at corr_in + 3 f, whatever
//                    they are, in ResidualBlockInfo::Evaluate's operation order; corr returns them
// Any output may be NULL.  -2: a member that is no NavFactor with one block of its width.
int icgh_backend_nav_eval(int n, const int32_t *kind, const int32_t *aux_off, const double *aux, const double *points, const int32_t *point_off,
                          const double *huber, const double *corr_in, double *r, double *J, double *r_corr, double *J_corr, double *corr,
                          double *sq_norm, int32_t *shape, char *err, int errlen) {
    return guarded(err, errlen, [&] {
        size_t ro = 0, jo = 0;
        for (int f = 0; f < n; f++) {
            auto cost       = make_nav_factor(kind[f], aux + aux_off[f]);
            const auto *nav = dynamic_cast<const NavFactor *>(cost.get());
            if (!nav || cost->parameter_block_sizes().size() != 1 || cost->parameter_block_sizes()[0] != nav->navWidth() ||
                cost->num_residuals() != nav->navResiduals()) {
                set_err(err, errlen, ("member " + std::to_string(f) + " is no navigation factor on one block of its width").c_str());
                return -2;
            }
            const int nr = nav->navResiduals(), nc = nav->navWidth();
            if (shape) shape[3 * f] = nav->navKind(), shape[3 * f + 1] = nr, shape[3 * f + 2] = nc;
            vector<double> x(points + point_off[f], points + point_off[f] + nc);
            const double *pp[1] = {x.data()};
            vector<double> rr((size_t) nr), JJ((size_t) nr * nc);
            double *jj[1] = {JJ.data()};
            if (!cost->Evaluate(pp, rr.data(), jj)) return -3;
            {
                vector<double> r2((size_t) nr);
                if (!cost->Evaluate(pp, r2.data(), nullptr) || memcmp(r2.data(), rr.data(), sizeof(double) * (size_t) nr)) return -3;
            }
            double sq = 0;
            for (double v : rr) sq += v * v;
            vector<double> rc = rr, Jc = JJ;
            CorrectorScalars cs{1.0, 0.0, 1.0};
            const bool marked = huber && huber[f] != 0.0;
            if (marked && !corr_in) {
                auto loss = std::make_shared<ceres::HuberLoss>(huber[f]);
                double rho[3];
                loss->Evaluate(sq, rho);
                cs = correctorScalars(sq, rho);
                ResidualBlockInfo info(cost, loss, vector<double *>{x.data()}, vector<int>{});
                if (!info.Evaluate()) return -3;
                rc = info.residuals(), Jc = info.jacobians()[0];
            } else if (marked) {
                cs = CorrectorScalars{corr_in[3 * f], corr_in[3 * f + 1], corr_in[3 * f + 2]};
                for (int c = 0; c < nc; c++) {
                    double rtj = 0;
                    for (int k = 0; k < nr; k++) rtj += rc[(size_t) k] * Jc[(size_t) k * nc + c];
                    for (int k = 0; k < nr; k++) {
                        double &j = Jc[(size_t) k * nc + c];
                        j         = cs.sqrt_rho1 * (j - cs.alpha_sq_norm * rc[(size_t) k] * rtj);
                    }
                }
                for (double &v : rc) v *= cs.residual_scaling;
            }
            if (r) memcpy(r + ro, rr.data(), sizeof(double) * (size_t) nr);
            if (J) memcpy(J + jo, JJ.data(), sizeof(double) * (size_t) nr * nc);
            if (r_corr) memcpy(r_corr + ro, rc.data(), sizeof(double) * (size_t) nr);
            if (J_corr) memcpy(J_corr + jo, Jc.data(), sizeof(double) * (size_t) nr * nc);
            if (corr) corr[3 * f] = cs.sqrt_rho1, corr[3 * f + 1] = cs.alpha_sq_norm, corr[3 * f + 2] = cs.residual_scaling;
            if (sq_norm) sq_norm[f] = sq;
            ro += (size_t) nr, jo += (size_t) nr * nc;
        }
        return 0;
    });
}

// The visual-inertial windows of icgh_backend_solve_preint_batch (variant 0 Normal / 1 Earth: states of 16, mix blocks of 9, the intervals
// integrated here from offsets / imu / params9) and of icgh_backend_solve_preint_odo_batch (variant 2 Odo / 3 EarthOdo: states of 17, mix blocks
// of 10, the integration results GIVEN as delta / jac / cov / dt / iewn / pn_off / pn with params19); the arguments of the variant that is not
// asked for may be NULL.  The same blocks and the same order of the residual blocks as there: the motion factors, the pose prior on state 0,
// the optional marginalization prior, the mix prior on state 0.  With nav_factors != 0 the stand-in priors are the product's navigation
// factors, and two more groups follow:
//   ImuPosePriorFactor(prior_pose0, std 1 / prior_weight) and ImuMixPriorFactor(prior_mix0, std 1 / prior_weight) on state 0
//   an ImuErrorFactor on the last state's mix block
//   a GnssFactor on every state: blh gnss_blh[w] + 3 k, std gnss_std3, lever gnss_lever3, behind HuberLoss(gnss_huber[w]) where that is not 0
// With nav_factors == 0 the windows are exactly those entries' (their stand-in priors, nothing added): the same bits as theirs.
// mode: 0 host; 1 device reduced solve; 2 and device host part; 3 and device prior; 4 = mode 2 plus the device preintegration, 5 = mode 3
// plus it.  device_nav: 1 = setDeviceNavFactors(true); 1 + 16: that switch WITHOUT setDeviceHostPart, which solve() refuses by name (-3).
// nav_on_device (optional out): the navigation factors that were resident on the device in the solve.  states, invdepth, summary4,
// prior_cost, solve_ms as there.  Other modes or variants: -1.  A mode whose C entries are not in the build computes nothing: -4 and the
// entry's name, icg_nav_set's first of all.  -2: the integration failed; -3: solve() failed (err: its message); -5: prepare() or a prior's
// evaluation failed.
int icgh_backend_solve_nav_batch(int W, int variant, const int32_t *n_intervals, const int32_t *const *offsets, const double *const *imu, const double *params9,
                                 const double *const *delta, const double *const *jac, const double *const *cov, const double *const *dt,
                                 const double *const *iewn, const int32_t *const *pn_off, const double *const *pn, const double *params19, double *const *states,
                                 const int32_t *n_fac, const double *const *obs_soa, const int32_t *const *idx_i, const int32_t *const *idx_j,
                                 const int32_t *const *idx_lm, double *const *ext, const int32_t *n_lm, double *const *invdepth, double *td,
                                 const double *const *prior_pose0, const double *const *prior_mix0, double prior_weight, double huber, int iters,
                                 const int32_t *prior_r, const int32_t *prior_nb, const int32_t *const *prior_size, const int32_t *const *prior_index,
                                 const int32_t *const *prior_param, const double *const *prior_x0, const double *const *prior_J0, const double *const *prior_e0,
                                 const int32_t *const *state_const, int nav_factors, const double *const *gnss_blh, const double *gnss_std3,
                                 const double *gnss_lever3, const double *gnss_huber, double *summary4, double *prior_cost, double *solve_ms,
                                 int32_t *nav_on_device, int mode, int device_nav, char *err, int errlen) {
    return guarded(err, errlen, [&] {
        const bool without_parts = device_nav == 1 + 16;
        if (without_parts) device_nav = 1;
        if (mode < 0 || mode > 5 || variant < 0 || variant > 3 || (device_nav != 0 && device_nav != 1)) {
            set_err(err, errlen, "mode must be 0 (host), 1 (device reduced solve), 2 (and device host part), 3 (and device prior), 4 (mode 2 and device "
                                 "preintegration) or 5 (mode 3 and device preintegration); variant 0 .. 3; device_nav 0 or 1 (+ 16)");
            return -1;
        }
        const bool odo = variant >= 2, prior = mode == 3 || mode == 5, preint = mode >= 4;
        const int mw = odo ? 10 : 9, sw = 7 + mw; // mix and state widths
        if (nav_on_device) *nav_on_device = 0;
        // (the entry a mode adds is named first: a build without any of them says what that mode itself is missing)
        const char *missing = device_nav && mode >= 1 ? WindowSolverBatch::deviceNavFactorsMissing() : nullptr;
        if (!missing && preint && odo) missing = WindowSolverBatch::devicePreintegrationOdoMissing();
        if (!missing && preint) missing = WindowSolverBatch::devicePreintegrationMissing();
        if (!missing && prior && !WindowSolverBatch::devicePriorAvailable())
            missing = MarginalizationPriorSet::residentAvailable() ? "icg_reproj_host_parts_build_prior" : "icg_marg_prior_evaluate_resident";
        if (!missing && mode >= 2 && !WindowSolverBatch::deviceHostPartAvailable()) missing = "icg_reproj_host_parts_build";
        if (!missing && mode >= 1 && !WindowSolverBatch::deviceReducedSolveAvailable()) missing = "icg_reproj_solve_windows";
        if (missing) {
            set_err(err, errlen, (std::string(missing) + " is not in this build").c_str());
            return -4;
        }
        TempCtx T(0);
        struct Win {
            int K;
            vector<double> pose, mix;
            vector<std::shared_ptr<Preintegration>> pre;
            vector<std::shared_ptr<PreintegrationOdo>> pre_odo;
        };
        vector<Win> wins((size_t) W);
        vector<Preintegration *> raw;
        auto p9 = odo ? nullptr : preint_params(params9);
        auto p19 = odo ? odo_params19(params19) : nullptr;
        for (int w = 0; w < W; w++) {
            Win &V = wins[(size_t) w];
            V.K    = n_intervals[w] + 1;
            V.pose.resize((size_t) V.K * 7), V.mix.resize((size_t) V.K * mw);
            for (int k = 0; k < V.K; k++)
                memcpy(&V.pose[7 * (size_t) k], states[w] + sw * (size_t) k, sizeof(double) * 7),
                    memcpy(&V.mix[(size_t) mw * k], states[w] + sw * (size_t) k + 7, sizeof(double) * (size_t) mw);
            for (int k = 0; k < n_intervals[w]; k++) {
                const size_t j = (size_t) k;
                if (odo) {
                    const int rows = variant == 3 && pn_off && pn_off[w] ? pn_off[w][k + 1] - pn_off[w][k] : 0;
                    V.pre_odo.push_back(odo_from_result(p19, variant, delta[w] + 20 * j, jac[w] + 361 * j, cov[w] + 361 * j, dt[w][j],
                                                        rows > 0 ? pn[w] + 4 * (size_t) pn_off[w][k] : nullptr, rows, iewn[w] + 3 * j));
                } else {
                    V.pre.push_back(preint_interval(variant, p9, offsets[w], imu[w], k, states[w] + 16 * j));
                    raw.push_back(V.pre.back().get());
                }
            }
        }
        std::string e;
        if (!odo && !Preintegration::integrateBatch(T.ctx, raw, &e)) {
            set_err(err, errlen, e.c_str());
            return -2;
        }
        vector<std::unique_ptr<ReprojectionFactor>> factors;
        WindowSolverBatch solver(0, huber);
        solver.setDeviceReducedSolve(mode >= 1);
        solver.setDeviceHostPart(mode >= 2 && !without_parts);
        solver.setDevicePrior(prior);
        solver.setDevicePreintegration(preint);
        solver.setDeviceNavFactors(device_nav != 0);
        vector<int> prior_id((size_t) W, -1);
        vector<double> std_w(10, 1.0 / prior_weight);
        int n_nav = 0;
        for (int w = 0; w < W; w++) {
            const OnBatchWindow win{solver, solver.addWindow()};
            Win &V      = wins[(size_t) w];
            const int K = V.K;
            double *P = V.pose.data(), *M = V.mix.data();
            for (int k = 0; k < K; k++) win.addParameterBlock(P + 7 * (size_t) k, 7, true), win.addParameterBlock(M + (size_t) mw * k, mw);
            win.addParameterBlock(ext[w], 7, true);
            for (int l = 0; l < n_lm[w]; l++) win.addParameterBlock(invdepth[w] + l, 1);
            win.addParameterBlock(td + w, 1);
            win.setParameterBlockConstant(ext[w]);
            win.setParameterBlockConstant(td + w);
            for (int k = 0; state_const && state_const[w] && k < K; k++)
                if (state_const[w][k]) win.setParameterBlockConstant(P + 7 * (size_t) k), win.setParameterBlockConstant(M + (size_t) mw * k);
            reprojections_from_soa(obs_soa[w], n_fac[w], 0, n_fac[w], idx_i[w], idx_j[w], idx_lm[w], P, ext[w], invdepth[w], td + w, factors, window_add(solver, win.w));
            for (int k = 0; k + 1 < K; k++) {
                const vector<double *> blocks{P + 7 * (size_t) k, M + (size_t) mw * k, P + 7 * (size_t) (k + 1), M + (size_t) mw * (k + 1)};
                if (odo)
                    win.addResidualBlock(std::make_shared<PreintegrationOdoFactor>(V.pre_odo[(size_t) k]), nullptr, blocks);
                else
                    win.addResidualBlock(std::make_shared<PreintegrationFactor>(V.pre[(size_t) k]), nullptr, blocks);
            }
            if (nav_factors) {
                double pose_std[6];
                for (double &v : pose_std) v = 1.0 / prior_weight;
                win.addResidualBlock(std::make_shared<ImuPosePriorFactor>(prior_pose0[w], pose_std), nullptr, {P}), n_nav++;
            } else
                pose_prior(win, P, prior_pose0[w], prior_weight);
            if (prior_r && prior_r[w] > 0) {
                // (between the two ordinary priors: a resident prior is not the window's last host block)
                vector<double *> blocks;
                for (int b = 0; b < prior_nb[w]; b++) {
                    const int code = prior_param[w][b], k = code / 2;
                    if (code < 0 || k >= K || prior_size[w][b] != (code % 2 ? mw : 7)) {
                        set_err(err, errlen, ("window " + std::to_string(w) + ": prior block " + std::to_string(b) + " does not name a pose or mix block").c_str());
                        return -1;
                    }
                    blocks.push_back(code % 2 ? M + (size_t) mw * k : P + 7 * (size_t) k);
                }
                prior_id[(size_t) w] = win.addResidualBlock(
                    std::make_shared<ArrayPriorFactor>(prior_r[w], prior_nb[w], prior_size[w], prior_index[w], prior_x0[w], prior_J0[w], prior_e0[w]), nullptr, blocks);
            }
            if (!nav_factors) {
                if (odo)
                    win.addResidualBlock(std::make_shared<OdoMixPriorFactor>(prior_mix0[w], prior_weight), nullptr, {M});
                else
                    win.addResidualBlock(std::make_shared<MixPriorFactor>(prior_mix0[w], prior_weight), nullptr, {M});
                continue;
            }
            win.addResidualBlock(std::make_shared<ImuMixPriorFactor>(prior_mix0[w], std_w.data(), variant), nullptr, {M}), n_nav++;
            win.addResidualBlock(std::make_shared<ImuErrorFactor>(variant), nullptr, {M + (size_t) mw * (K - 1)}), n_nav++;
            std::shared_ptr<ceres::LossFunction> loss;
            if (gnss_huber && gnss_huber[w] != 0) loss = std::make_shared<ceres::HuberLoss>(gnss_huber[w]);
            for (int k = 0; k < K; k++) {
                GNSS g;
                const double *b = gnss_blh[w] + 3 * (size_t) k;
                g.blh = Vector3d(b[0], b[1], b[2]), g.std = Vector3d(gnss_std3[0], gnss_std3[1], gnss_std3[2]);
                win.addResidualBlock(std::make_shared<GnssFactor>(g, Vector3d(gnss_lever3[0], gnss_lever3[1], gnss_lever3[2])), loss, {P + 7 * (size_t) k}), n_nav++;
            }
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
        if (nav_on_device) *nav_on_device = solver.navFactorsOnDevice();
        if (!prior_costs(1)) {
            set_err(err, errlen, "a prior failed to evaluate");
            return -5;
        }
        for (int w = 0; w < W; w++) {
            put_summary4(sum[(size_t) w], summary4 + 4 * (size_t) w);
            const Win &V = wins[(size_t) w];
            for (int k = 0; k < V.K; k++)
                memcpy(states[w] + sw * (size_t) k, &V.pose[7 * (size_t) k], sizeof(double) * 7),
                    memcpy(states[w] + sw * (size_t) k + 7, &V.mix[(size_t) mw * k], sizeof(double) * (size_t) mw);
        }
        return 0;
    });
}

} // extern "C"
