// Shared by capi_solve_prior.cc, capi_solve_preint.cc, capi_solve_preint_odo.cc and capi_solve_nav.cc (internal linkage, like
// capi_windows.h): the batch of visual-inertial windows with optional marginalization priors on plain arrays, built and solved once for the
// first two entries, which differ in the modes they admit and in the switches they set; and what the odometer windows of the last two share.
#pragma once
#include <chrono>
#include <cstdlib>
#include <memory>

#include "factors.h"
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

// ---- the odometer windows (capi_solve_preint_odo.cc, capi_solve_nav.cc): parameters of 19 and objects from GIVEN integration results
std::shared_ptr<icg::IntegrationParameters> odo_params19(const double *params19) {
    using icg::Vector3d;
    auto P     = preint_params(params19);
    P->odo_std = Vector3d(params19[9], params19[10], params19[11]);
    P->odo_srw = params19[12];
    P->abv     = Vector3d(params19[13], params19[14], params19[15]);
    P->lodo    = Vector3d(params19[16], params19[17], params19[18]);
    return P;
}

// a PreintegrationOdo as if integrateBatch had returned the given result (no device, no IMU samples)
std::shared_ptr<icg::PreintegrationOdo> odo_from_result(const std::shared_ptr<icg::IntegrationParameters> &P, int variant, const double *delta20,
                                                        const double *jac361, const double *cov361, double delta_time, const double *pn, int pn_rows,
                                                        const double *iewn3) {
    using namespace icg;
    IntegrationState st;
    st.bg   = Vector3d(delta20[10], delta20[11], delta20[12]);
    st.ba   = Vector3d(delta20[13], delta20[14], delta20[15]);
    st.sodo = delta20[19];
    auto p  = std::make_shared<PreintegrationOdo>(P, IMU(), st, variant == 2 ? PreintegrationOdo::ODO : PreintegrationOdo::EARTH_ODO);
    double cur16[16];
    preint_put_state(st, cur16);
    p->setIntegrationResult(cur16, delta20, jac361, cov361, delta_time, pn_rows > 0 ? pn : nullptr, pn_rows > 0 ? pn_rows : 0,
                            Vector3d(iewn3[0], iewn3[1], iewn3[2]));
    return p;
}

// the arguments icgh_backend_solve_prior_batch and icgh_backend_solve_preint_batch share (documented at the first)
struct PriorWindowArgs {
    int W;
    const int32_t *n_intervals;
    const int32_t *const *offsets;
    const double *const *imu;
    const double *params9;
    double *const *states16;
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
    const double *prior_robust;
    const int32_t *const *state_const;
    double *summary4, *prior_cost, *solve_ms;
};
// which switches of WindowSolverBatch a solve sets, the variant of its intervals, an optional Huber delta per window for its preintegration
// factors (such a factor stays on the pool) and, on return, how many preintegration factors were resident
struct PriorWindowSwitches {
    bool reduced = false, host_part = false, prior = false, preint = false;
    int variant                 = 0;
    const double *preint_robust = nullptr;
    int32_t *preint_on_device   = nullptr;
};

// builds the windows, integrates, solves; the return codes of icgh_backend_solve_prior_batch from -2 on
int solve_prior_windows(const PriorWindowArgs &a, const PriorWindowSwitches &sw, char *err, int errlen) {
    using namespace icg;
    const int W = a.W;
    auto params = preint_params(a.params9);
    TempCtx T(0);
    vector<std::unique_ptr<ReprojectionFactor>> factors;
    vector<VioWindow> wins;
    vector<Preintegration *> raw;
    for (int w = 0; w < W; w++) wins.push_back(vio_window(a.n_intervals[w], a.offsets[w], a.imu[w], params, a.states16[w], raw, sw.variant));
    std::string e;
    if (!Preintegration::integrateBatch(T.ctx, raw, &e)) {
        set_err(err, errlen, e.c_str());
        return -2;
    }
    WindowSolverBatch solver(0, a.huber);
    solver.setDeviceReducedSolve(sw.reduced);
    solver.setDeviceHostPart(sw.host_part);
    solver.setDevicePrior(sw.prior);
    solver.setDevicePreintegration(sw.preint);
    vector<int> prior_id((size_t) W, -1);
    for (int w = 0; w < W; w++) {
        const OnBatchWindow win{solver, solver.addWindow()};
        VioWindow &V = wins[(size_t) w];
        const int K  = V.K;
        double *P = V.pose.data(), *M = V.mix.data();
        vio_blocks(win, V, a.ext[w], a.n_lm[w], a.invdepth[w], a.td + w);
        for (int k = 0; a.state_const && a.state_const[w] && k < K; k++)
            if (a.state_const[w][k]) win.setParameterBlockConstant(P + 7 * (size_t) k), win.setParameterBlockConstant(M + 9 * (size_t) k);
        reprojections_from_soa(a.obs_soa[w], a.n_fac[w], 0, a.n_fac[w], a.idx_i[w], a.idx_j[w], a.idx_lm[w], P, a.ext[w], a.invdepth[w], a.td + w, factors,
                               window_add(solver, win.w));
        std::shared_ptr<ceres::LossFunction> preint_loss;
        if (sw.preint_robust && sw.preint_robust[w] != 0) preint_loss = std::make_shared<HuberLossHip>(sw.preint_robust[w]);
        vio_motion_factors(win, V, a.prior_pose0[w], a.prior_weight, preint_loss);
        if (a.prior_r && a.prior_r[w] > 0) {
            // (between the two ordinary priors: a resident prior is not the window's last host block)
            vector<double *> blocks;
            for (int b = 0; b < a.prior_nb[w]; b++) {
                const int code = a.prior_param[w][b], k = code / 2;
                if (code < 0 || k >= K || a.prior_size[w][b] != (code % 2 ? 9 : 7)) {
                    set_err(err, errlen, ("window " + std::to_string(w) + ": prior block " + std::to_string(b) + " does not name a pose (7) or mix (9) block").c_str());
                    return -1;
                }
                blocks.push_back(code % 2 ? M + 9 * (size_t) k : P + 7 * (size_t) k);
            }
            std::shared_ptr<ceres::LossFunction> loss;
            if (a.prior_robust && a.prior_robust[w] != 0) loss = std::make_shared<HuberLossHip>(a.prior_robust[w]);
            prior_id[(size_t) w] = win.addResidualBlock(
                std::make_shared<ArrayPriorFactor>(a.prior_r[w], a.prior_nb[w], a.prior_size[w], a.prior_index[w], a.prior_x0[w], a.prior_J0[w], a.prior_e0[w]), loss,
                blocks);
        }
        vio_mix_prior(win, V, a.prior_mix0[w], a.prior_weight);
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
    if (sw.preint_on_device) *sw.preint_on_device = solver.preintegrationsOnDevice();
    if (!prior_costs(1)) {
        set_err(err, errlen, "a prior failed to evaluate");
        return -5;
    }
    for (int w = 0; w < W; w++) {
        put_summary4(sum[(size_t) w], a.summary4 + 4 * (size_t) w);
        wins[(size_t) w].put(a.states16[w]);
    }
    return 0;
}
} // namespace
