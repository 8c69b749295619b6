// C entry point of libicgvins_host.so for WindowSolverBatch::setDevicePrior: a batch of visual-inertial windows, each optionally with a
// marginalization prior given as plain arrays, solved with the prior on the host pool or resident on the device.  For tests and probes.
#include <chrono>
#include <cstdlib>
#include <memory>

#include "factors.h"
#include "solver_batch_hip.h"
#include "capi_windows.h"

using namespace icg;

namespace {
// A linearized prior on plain arrays (what MarginalizationFactor is over a MarginalizationInfo): the arrays are copied, Evaluate is
// evaluateMargPrior over them, and the solver recognises the prior through MargPriorSource.
class ArrayPriorFactor : public ceres::CostFunction, public MargPriorSource {
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
        evaluateMargPrior(view_, parameters, residuals, jacobians);
        return true;
    }
    const MargPriorView &margPriorView() const override { return view_; }

private:
    std::vector<int> size_, index_;
    std::vector<double> x0_, J0_, e0_;
    std::vector<const double *> x0_ptr_;
    MargPriorView view_;
};
} // namespace

extern "C" {

// icgh_backend_solve_vio_batch (capi_solve_parts.cc: the same windows, the same leading arguments) with, per window and optionally, a
// marginalization prior and constant states.
//   prior_r[w]       the prior's retained size, 0 = window w has no prior.  The prior has prior_nb[w] blocks; block b has global size
//                    prior_size[w][b] (7 or 9), first local column prior_index[w][b], and is the parameter block prior_param[w][b] of the
//                    window: 2 k = the pose of state k, 2 k + 1 = its mix block.  prior_x0[w] (the blocks' linearization points,
//                    concatenated), prior_J0[w] (r x r row-major), prior_e0[w] (r): the layout of icg_marg_prior_set for one window.
//   prior_robust[w]  != 0: the prior's residual block gets a Huber loss of that delta (such a prior stays on the pool in every mode)
//   state_const[w]   n_intervals[w] + 1 flags (NULL: none): the pose and mix blocks of a flagged state are constant
//   prior_cost       W x 2: the prior's own cost 0.5 |e|^2 (no loss) from its Evaluate at the start and at the end; 0 without a prior
// mode: 0 = host, 1 = device reduced solve, 2 = that and the device host part, 3 = those and the device prior (setDevicePrior); 3 + 16: the
// prior switch with the reduced solve but WITHOUT setDeviceHostPart, which solve() refuses by name (-3).  A mode whose C entries are not in
// the build computes nothing: -4 and the entry's name.  summary4 is W x 4 as there; *solve_ms: the wall time of the solve alone.
int icgh_backend_solve_prior_batch(int W, const int32_t *n_intervals, const int32_t *const *offsets, const double *const *imu, const double *params9,
                                   double *const *states16, const int32_t *n_fac, const double *const *obs_soa, const int32_t *const *idx_i,
                                   const int32_t *const *idx_j, const int32_t *const *idx_lm, double *const *ext, const int32_t *n_lm, double *const *invdepth,
                                   double *td, const double *const *prior_pose0, const double *const *prior_mix0, double prior_weight, double huber, int iters,
                                   const int32_t *prior_r, const int32_t *prior_nb, const int32_t *const *prior_size, const int32_t *const *prior_index,
                                   const int32_t *const *prior_param, const double *const *prior_x0, const double *const *prior_J0,
                                   const double *const *prior_e0, const double *prior_robust, const int32_t *const *state_const, double *summary4,
                                   double *prior_cost, double *solve_ms, int mode, char *err, int errlen) {
    return guarded(err, errlen, [&] {
        const bool without_parts = mode == 3 + 16;
        if (without_parts) mode = 3;
        if (mode < 0 || mode > 3) {
            set_err(err, errlen, "mode must be 0 (host), 1 (device reduced solve), 2 (and device host part) or 3 (and device prior)");
            return -1;
        }
        // (the entry a mode adds is named first: a build without any of them says what that mode itself is missing)
        if (mode == 3 && !WindowSolverBatch::devicePriorAvailable()) {
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
        auto params = preint_params(params9);
        TempCtx T(0);
        vector<std::unique_ptr<ReprojectionFactor>> factors;
        vector<VioWindow> wins;
        vector<Preintegration *> raw;
        for (int w = 0; w < W; w++) wins.push_back(vio_window(n_intervals[w], offsets[w], imu[w], params, states16[w], raw));
        std::string e;
        if (!Preintegration::integrateBatch(T.ctx, raw, &e)) {
            set_err(err, errlen, e.c_str());
            return -2;
        }
        WindowSolverBatch solver(0, huber);
        solver.setDeviceReducedSolve(mode >= 1);
        solver.setDeviceHostPart(mode >= 2 && !without_parts);
        solver.setDevicePrior(mode == 3);
        vector<int> prior_id((size_t) W, -1);
        for (int w = 0; w < W; w++) {
            const OnBatchWindow win{solver, solver.addWindow()};
            VioWindow &V = wins[(size_t) w];
            const int K  = V.K;
            double *P = V.pose.data(), *M = V.mix.data();
            vio_blocks(win, V, ext[w], n_lm[w], invdepth[w], td + w);
            for (int k = 0; state_const && state_const[w] && k < K; k++)
                if (state_const[w][k]) win.setParameterBlockConstant(P + 7 * (size_t) k), win.setParameterBlockConstant(M + 9 * (size_t) k);
            reprojections_from_soa(obs_soa[w], n_fac[w], 0, n_fac[w], idx_i[w], idx_j[w], idx_lm[w], P, ext[w], invdepth[w], td + w, factors,
                                   window_add(solver, win.w));
            vio_motion_factors(win, V, prior_pose0[w], prior_weight);
            if (prior_r && prior_r[w] > 0) {
                // (between the two ordinary priors: a resident prior is not the window's last host block)
                vector<double *> blocks;
                for (int b = 0; b < prior_nb[w]; b++) {
                    const int code = prior_param[w][b], k = code / 2;
                    if (code < 0 || k >= K || prior_size[w][b] != (code % 2 ? 9 : 7)) {
                        set_err(err, errlen, ("window " + std::to_string(w) + ": prior block " + std::to_string(b) + " does not name a pose (7) or mix (9) block").c_str());
                        return -1;
                    }
                    blocks.push_back(code % 2 ? M + 9 * (size_t) k : P + 7 * (size_t) k);
                }
                std::shared_ptr<ceres::LossFunction> loss;
                if (prior_robust && prior_robust[w] != 0) loss = std::make_shared<HuberLossHip>(prior_robust[w]);
                prior_id[(size_t) w] = win.addResidualBlock(
                    std::make_shared<ArrayPriorFactor>(prior_r[w], prior_nb[w], prior_size[w], prior_index[w], prior_x0[w], prior_J0[w], prior_e0[w]), loss, blocks);
            }
            vio_mix_prior(win, V, prior_mix0[w], prior_weight);
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
        if (!prior_costs(1)) {
            set_err(err, errlen, "a prior failed to evaluate");
            return -5;
        }
        for (int w = 0; w < W; w++) {
            put_summary4(sum[(size_t) w], summary4 + 4 * (size_t) w);
            wins[(size_t) w].put(states16[w]);
        }
        return 0;
    });
}

} // extern "C"
