// Shared by capi_solve_prior.cc, capi_solve_preint.cc, capi_solve_preint_odo.cc and capi_solve_nav.cc (internal linkage, like
// capi_windows.h): the batch of visual-inertial windows with optional marginalization priors on plain arrays and optional navigation
// factors, built, solved and copied back by ONE function (solve_vio_windows) for the four entries icgh_backend_solve_{prior, preint,
// preint_odo, nav}_batch, which differ in the arguments they have, in the modes and variants they admit and in the counter they return; and the
// order in which a C entry that is missing from the build is named (vio_missing_entry).
#pragma once
#include <chrono>
#include <cstdlib>
#include <memory>

#include "factors.h"
#include "nav_factors.h"
#include "solver_batch_hip.h"
#include "capi_windows.h"

namespace {
// A linearized prior on plain arrays (what MarginalizationFactor is over a MarginalizationInfo): the arrays are copied, Evaluate is
// evaluateMargPrior over them, and the solver recognises the prior through MargPriorSource.
class ArrayPriorFactor : public ceres::CostFunction, public icg::MargPriorSource {
public:
    ArrayPriorFactor(int r, int n_blocks, const int32_t *size, const int32_t *index, const double *x0, const double *J0, const double *e0)
        : size_(size, size + n_blocks), index_(index, index + n_blocks), J0_(J0, J0 + (size_t) r * r), e0_(e0, e0 + r) {
        size_t n = 0;
        for (int s : size_) n += (size_t) s;
        x0_.assign(x0, x0 + n);
        n = 0;
        for (int s : size_) x0_ptr_.push_back(x0_.data() + n), n += (size_t) s, mutable_parameter_block_sizes()->push_back(s);
        set_num_residuals(r);
        view_.r = r, view_.n_blocks = n_blocks, view_.size = size_.data(), view_.index = index_.data(), view_.x0 = x0_ptr_.data(), view_.J0 = J0_.data(),
        view_.e0 = e0_.data();
    }
    ArrayPriorFactor(const ArrayPriorFactor &) = delete;
    bool Evaluate(const double *const *parameters, double *residuals, double **jacobians) const override {
        icg::evaluateMargPrior(view_, parameters, residuals, jacobians);
        return true;
    }
    const icg::MargPriorView &margPriorView() const override { return view_; }

private:
    std::vector<int> size_, index_;
    std::vector<double> x0_, J0_, e0_;
    std::vector<const double *> x0_ptr_;
    icg::MargPriorView view_;
};

// ---- the batch of visual-inertial windows ---------------------------------------------------------------------------------------------
// What the four entries take, each documented where it is exported; a group an entry does not have is NULL / 0.
struct VioBatchArgs {
    int W, variant; // 0 Normal, 1 Earth: mix blocks of 9, states of 16, the intervals integrated here; 2 Odo, 3 EarthOdo: 10 and 17, the results given
    const int32_t *n_intervals;
    const int32_t *const *offsets; // variants 0, 1
    const double *const *imu;
    const double *params9;
    const double *const *delta, *const *jac, *const *cov, *const *dt, *const *iewn; // variants 2, 3
    const int32_t *const *pn_off;
    const double *const *pn;
    const double *params19;
    double *const *states;
    const int32_t *n_fac;
    const double *const *obs_soa;
    const int32_t *const *idx_i, *const *idx_j, *const *idx_lm;
    double *const *ext;
    const int32_t *n_lm;
    double *const *invdepth;
    double *td;
    const double *const *prior_pose0, *const *prior_mix0;
    double prior_weight, huber;
    int iters;
    const int32_t *prior_r, *prior_nb;
    const int32_t *const *prior_size, *const *prior_index, *const *prior_param;
    const double *const *prior_x0, *const *prior_J0, *const *prior_e0;
    const double *prior_robust, *preint_robust; // optional Huber deltas per window: such a prior, such preintegration factors stay on the pool
    const int32_t *const *state_const;
    int nav_factors; // != 0: the product's navigation factors in place of the stand-in priors, an ImuErrorFactor, a GNSS fix per state
    const double *const *gnss_blh;
    const double *gnss_std3, *gnss_lever3, *gnss_huber;
    double *summary4, *prior_cost, *solve_ms;
    int32_t *preint_on_device, *odo_on_device, *nav_on_device; // optional: the members of the resident sets in the solve
};

// The first C entry a solve in `mode` (0 .. 5 as the entries document it) lacks in this build, nullptr when none: the entry a switch adds is
// named first, so that a build without any of them says what the mode itself is missing.
const char *vio_missing_entry(int mode, bool odo, bool device_nav) {
    using icg::WindowSolverBatch;
    const bool prior = mode == 3 || mode == 5, preint = mode >= 4;
    const char *missing = device_nav && mode >= 1 ? WindowSolverBatch::deviceNavFactorsMissing() : nullptr;
    if (!missing && preint && odo) missing = WindowSolverBatch::devicePreintegrationOdoMissing();
    if (!missing && preint) missing = WindowSolverBatch::devicePreintegrationMissing();
    if (!missing && prior && !WindowSolverBatch::devicePriorAvailable())
        missing = icg::MarginalizationPriorSet::residentAvailable() ? "icg_reproj_host_parts_build_prior" : "icg_marg_prior_evaluate_resident";
    if (!missing && mode >= 2 && !WindowSolverBatch::deviceHostPartAvailable()) missing = "icg_reproj_host_parts_build";
    if (!missing && mode >= 1 && !WindowSolverBatch::deviceReducedSolveAvailable()) missing = "icg_reproj_solve_windows";
    return missing;
}

// Builds the windows, solves and copies back.  mode: 0 host; 1 device reduced solve; 2 and device host part; 3 and device prior; 4 = mode 2
// plus the device preintegration, 5 = mode 3 plus it (the entry has checked it and the variant); without_parts: the switches of the mode
// WITHOUT setDeviceHostPart, which solve() refuses by name.  The residual blocks of a window, in the order of the host sums: the motion
// factors, the pose prior on state 0, the optional marginalization prior (between the two ordinary priors: a resident prior is not the
// window's last host block), the mix prior on state 0; with nav_factors the error factor on the last state and the GNSS fixes behind them.
// Returns 0, -1: a prior block that names no block of the window, -2: the integration failed, -3: solve() failed (err: its message),
// -4: a C entry of the mode is not in this build (nothing is computed), -5: prepare() or a prior's evaluation failed.
int solve_vio_windows(const VioBatchArgs &a, int mode, bool without_parts, bool device_nav, char *err, int errlen) {
    using namespace icg;
    const int W    = a.W;
    const bool odo = a.variant >= 2;
    if (const char *missing = vio_missing_entry(mode, odo, device_nav)) {
        set_err(err, errlen, (std::string(missing) + " is not in this build").c_str());
        return -4;
    }
    for (int32_t *n : {a.preint_on_device, a.odo_on_device, a.nav_on_device})
        if (n) *n = 0;
    auto params = odo ? odo_params19(a.params19) : preint_params(a.params9);
    TempCtx T(0);
    vector<std::unique_ptr<ReprojectionFactor>> factors;
    vector<VioWindow> wins((size_t) W);
    vector<Preintegration *> raw;
    for (int w = 0; w < W; w++) {
        if (!odo) {
            wins[(size_t) w] = vio_window(a.n_intervals[w], a.offsets[w], a.imu[w], params, a.states[w], raw, a.variant);
            continue;
        }
        VioWindow &V = wins[(size_t) w];
        V.K = a.n_intervals[w] + 1, V.mw = 10;
        V.take(a.states[w]);
        for (int k = 0; k < a.n_intervals[w]; k++) {
            const size_t j = (size_t) k;
            const int rows = a.variant == 3 && a.pn_off && a.pn_off[w] ? a.pn_off[w][k + 1] - a.pn_off[w][k] : 0;
            V.pre_odo.push_back(odo_from_result(params, a.variant, a.delta[w] + 20 * j, a.jac[w] + 361 * j, a.cov[w] + 361 * j, a.dt[w][j],
                                                rows > 0 ? a.pn[w] + 4 * (size_t) a.pn_off[w][k] : nullptr, rows, a.iewn[w] + 3 * j));
        }
    }
    std::string e;
    if (!odo && !Preintegration::integrateBatch(T.ctx, raw, &e)) {
        set_err(err, errlen, e.c_str());
        return -2;
    }
    WindowSolverBatch solver(0, a.huber);
    solver.setDeviceReducedSolve(mode >= 1);
    solver.setDeviceHostPart(mode >= 2 && !without_parts);
    solver.setDevicePrior(mode == 3 || mode == 5);
    solver.setDevicePreintegration(mode >= 4);
    solver.setDeviceNavFactors(device_nav);
    vector<int> prior_id((size_t) W, -1);
    const vector<double> nav_std(10, 1.0 / a.prior_weight);
    auto huber_hip = [](const double *delta, int w) { return delta && delta[w] != 0 ? std::make_shared<HuberLossHip>(delta[w]) : nullptr; };
    for (int w = 0; w < W; w++) {
        const OnBatchWindow win{solver, solver.addWindow()};
        VioWindow &V = wins[(size_t) w];
        const int K  = V.K;
        vio_blocks(win, V, a.ext[w], a.n_lm[w], a.invdepth[w], a.td + w);
        for (int k = 0; a.state_const && a.state_const[w] && k < K; k++)
            if (a.state_const[w][k]) win.setParameterBlockConstant(V.P(k)), win.setParameterBlockConstant(V.M(k));
        reprojections_from_soa(a.obs_soa[w], a.n_fac[w], 0, a.n_fac[w], a.idx_i[w], a.idx_j[w], a.idx_lm[w], V.P(0), a.ext[w], a.invdepth[w], a.td + w, factors,
                               window_add(solver, win.w));
        vio_preint_factors(win, V, huber_hip(a.preint_robust, w));
        if (a.nav_factors)
            win.addResidualBlock(std::make_shared<ImuPosePriorFactor>(a.prior_pose0[w], nav_std.data()), nullptr, {V.P(0)});
        else
            pose_prior(win, V.P(0), a.prior_pose0[w], a.prior_weight);
        if (a.prior_r && a.prior_r[w] > 0) {
            vector<double *> blocks;
            for (int b = 0; b < a.prior_nb[w]; b++) {
                const int code = a.prior_param[w][b], k = code / 2;
                if (code < 0 || k >= K || a.prior_size[w][b] != (code % 2 ? V.mw : 7)) {
                    set_err(err, errlen, ("window " + std::to_string(w) + ": prior block " + std::to_string(b) + " does not name a pose (7) or mix (" +
                                          std::to_string(V.mw) + ") block").c_str());
                    return -1;
                }
                blocks.push_back(code % 2 ? V.M(k) : V.P(k));
            }
            prior_id[(size_t) w] = win.addResidualBlock(
                std::make_shared<ArrayPriorFactor>(a.prior_r[w], a.prior_nb[w], a.prior_size[w], a.prior_index[w], a.prior_x0[w], a.prior_J0[w], a.prior_e0[w]),
                huber_hip(a.prior_robust, w), blocks);
        }
        if (!a.nav_factors) {
            vio_mix_prior(win, V, a.prior_mix0[w], a.prior_weight);
            continue;
        }
        win.addResidualBlock(std::make_shared<ImuMixPriorFactor>(a.prior_mix0[w], nav_std.data(), a.variant), nullptr, {V.M(0)});
        win.addResidualBlock(std::make_shared<ImuErrorFactor>(a.variant), nullptr, {V.M(K - 1)});
        std::shared_ptr<ceres::LossFunction> loss;
        if (a.gnss_huber && a.gnss_huber[w] != 0) loss = std::make_shared<ceres::HuberLoss>(a.gnss_huber[w]);
        for (int k = 0; k < K; k++) {
            GNSS g;
            const double *b = a.gnss_blh[w] + 3 * (size_t) k;
            g.blh = Vector3d(b[0], b[1], b[2]), g.std = Vector3d(a.gnss_std3[0], a.gnss_std3[1], a.gnss_std3[2]);
            win.addResidualBlock(std::make_shared<GnssFactor>(g, Vector3d(a.gnss_lever3[0], a.gnss_lever3[1], a.gnss_lever3[2])), loss, {V.P(k)});
        }
    }
    auto prior_costs = [&](int at) {
        for (int w = 0; w < W && a.prior_cost; w++) {
            a.prior_cost[2 * (size_t) w + at] = 0.0;
            if (prior_id[(size_t) w] >= 0 && !solver.evaluateResidualBlock(w, prior_id[(size_t) w], false, a.prior_cost + 2 * (size_t) w + at)) return false;
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
    opt.max_num_iterations = a.iters;
    if (!solver.solve(opt, &sum)) {
        set_err(err, errlen, solver.error().c_str());
        return -3;
    }
    if (a.solve_ms) *a.solve_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    if (a.preint_on_device) *a.preint_on_device = solver.preintegrationsOnDevice();
    if (a.odo_on_device) *a.odo_on_device = solver.odometerPreintegrationsOnDevice();
    if (a.nav_on_device) *a.nav_on_device = solver.navFactorsOnDevice();
    if (!prior_costs(1)) {
        set_err(err, errlen, "a prior failed to evaluate");
        return -5;
    }
    for (int w = 0; w < W; w++) {
        put_summary4(sum[(size_t) w], a.summary4 + 4 * (size_t) w);
        wins[(size_t) w].put(a.states[w]);
    }
    return 0;
}
} // namespace

