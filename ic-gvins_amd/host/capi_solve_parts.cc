// C entry points of libicgvins_host.so around the host-factor part of a window's reduced system (WindowSolverBatch::setDeviceHostPart): the
// host twin of icg_reproj_host_parts_build, the batch solve with both device switches, and a batch of visual-inertial windows.  For tests and
// probes.  Where icg_reproj_host_parts_build is not in the build (this layer on another implementation of the C ABI) all three compute
// nothing: -4 and "icg_reproj_host_parts_build is not in this build".
#include <chrono>
#include <cstdlib>
#include <memory>
#include <random>

#include "factors.h"
#include "solver_batch_hip.h"
#include "capi_windows.h"

using namespace icg;

namespace {
const char *kNoHostParts = "icg_reproj_host_parts_build is not in this build";

// r = A (x - x0) over n blocks of 9 (the mix blocks of a window): 9 n residuals, a constant dense Jacobian.  It stands in for the width of
// the marginalization prior: A = weight (I + 0.25 U), U uniform in (-1, 1) from a seeded generator.
class DenseLinearFactor : public ceres::CostFunction {
public:
    DenseLinearFactor(int n_blocks, const double *const *x0, double weight, uint32_t seed) : n_(9 * n_blocks), A_((size_t) n_ * n_), x0_((size_t) n_) {
        set_num_residuals(n_);
        mutable_parameter_block_sizes()->assign((size_t) n_blocks, 9);
        std::mt19937 gen(seed);
        for (int i = 0; i < n_; i++)
            for (int j = 0; j < n_; j++) {
                const double u      = ((double) (gen() >> 8) + 0.5) / 8388608.0 - 1.0; // 24 bits -> (-1, 1)
                A_[(size_t) i * n_ + j] = weight * ((i == j ? 1.0 : 0.0) + 0.25 * u);
            }
        for (int b = 0; b < n_blocks; b++) memcpy(&x0_[9 * (size_t) b], x0[b], sizeof(double) * 9);
    }
    bool Evaluate(const double *const *parameters, double *residuals, double **jacobians) const override {
        for (int i = 0; i < n_; i++) {
            double acc = 0;
            for (int j = 0; j < n_; j++) acc += A_[(size_t) i * n_ + j] * (parameters[j / 9][j % 9] - x0_[(size_t) j]);
            residuals[i] = acc;
        }
        if (jacobians)
            for (int b = 0; b < n_ / 9; b++)
                if (jacobians[b])
                    for (int i = 0; i < n_; i++) memcpy(jacobians[b] + 9 * (size_t) i, &A_[(size_t) i * n_ + 9 * (size_t) b], sizeof(double) * 9);
        return true;
    }

private:
    int n_;
    std::vector<double> A_, x0_;
};
} // namespace

extern "C" {

// The host twin of icg_reproj_host_parts_build on its flat arrays (every block with its Jacobian at J + jac_off[b]): the accumulation step of
// solver_detail::hostFactors, per window.  part: the packed lower triangles of the leading Pw[w] columns, window after window; host_s and
// host_diag: W x P.
int icgh_host_part_from_blocks(int W, int P, const int32_t *Pw, const int32_t *blk_off, const int32_t *nr, const int32_t *nf, const int32_t *cols,
                               const int64_t *jac_off, const double *J, const double *r, double *part, double *host_s, double *host_diag, char *err,
                               int errlen) {
    return guarded(err, errlen, [&] {
        if (!WindowSolverBatch::deviceHostPartAvailable()) {
            set_err(err, errlen, kNoHostParts);
            return -4;
        }
        size_t r_at = 0, c_at = 0;
        vector<double> S;
        vector<int> bc;
        for (int w = 0; w < W; w++) {
            S.assign((size_t) P * P, 0.0);
            double *s = host_s + (size_t) w * P, *dg = host_diag + (size_t) w * P;
            std::fill(s, s + P, 0.0), std::fill(dg, dg + P, 0.0);
            for (int b = blk_off[w]; b < blk_off[w + 1]; b++) {
                bc.assign(cols + c_at, cols + c_at + nf[b]);
                for (int c : bc)
                    if (c < 0 || c >= Pw[w]) throw std::runtime_error("icgh_host_part_from_blocks: a column outside the window's system");
                solver_detail::accumulateHostBlock(P, bc, nr[b], J + jac_off[b], r + r_at, S.data(), s, dg);
                r_at += (size_t) nr[b], c_at += (size_t) nf[b];
            }
            for (int i = 0; i < Pw[w]; i++, part += i) memcpy(part, &S[(size_t) i * P], sizeof(double) * ((size_t) i + 1));
        }
        return 0;
    });
}

// icgh_backend_solve_batch_mode (capi_solve.cc) with the second switch.  host_part_mode: 0 = the host-factor parts are formed on the host
// pool, 1 = on the device (WindowSolverBatch::setDeviceHostPart; the same bits; needs reduced_solve_mode 1).
int icgh_backend_solve_batch_parts(int W, const int32_t *fac_off, const int32_t *pose_off, const int32_t *lm_off, const double *obs_soa,
                                   const int32_t *idx_i, const int32_t *idx_j, const int32_t *idx_lm, double *poses, double *ext, double *invdepth,
                                   double *td, const double *prior_poses, double prior_weight, double huber, int ext_constant, int td_constant,
                                   int iters1, int iters2, double chi2, double *summary8, double *solve_ms, char *err, int errlen,
                                   int reduced_solve_mode, int host_part_mode) {
    return guarded(err, errlen, [&] {
        if ((reduced_solve_mode != 0 && reduced_solve_mode != 1) || (host_part_mode != 0 && host_part_mode != 1)) {
            set_err(err, errlen, "reduced_solve_mode and host_part_mode must be 0 (host) or 1 (device)");
            return -1;
        }
        if (reduced_solve_mode == 1 && !WindowSolverBatch::deviceReducedSolveAvailable()) {
            set_err(err, errlen, "icg_reproj_solve_windows is not in this build");
            return -4;
        }
        if (host_part_mode == 1 && !WindowSolverBatch::deviceHostPartAvailable()) {
            set_err(err, errlen, kNoHostParts);
            return -4;
        }
        const int n = fac_off[W];
        vector<std::unique_ptr<ReprojectionFactor>> factors;
        WindowSolverBatch solver(0, huber);
        solver.setDeviceReducedSolve(reduced_solve_mode == 1);
        solver.setDeviceHostPart(host_part_mode == 1);
        for (int w = 0; w < W; w++) {
            const OnBatchWindow win{solver, solver.addWindow()};
            double *P = poses + 7 * (size_t) pose_off[w], *E = ext + 7 * (size_t) w, *D = invdepth + lm_off[w], *TD = td + w;
            const int K = pose_off[w + 1] - pose_off[w], L = lm_off[w + 1] - lm_off[w];
            visual_blocks(win, K, P, E, L, D, TD, ext_constant != 0, td_constant != 0);
            reprojections_from_soa(obs_soa, n, fac_off[w], fac_off[w + 1], idx_i, idx_j, idx_lm, P, E, D, TD, factors, window_add(solver, win.w));
            pose_priors(win, K, P, prior_poses + 7 * (size_t) pose_off[w], prior_weight);
        }
        if (!solver.prepare()) {
            set_err(err, errlen, solver.error().c_str());
            return -5;
        }
        auto t0 = std::chrono::steady_clock::now();
        WindowSolverBatch::Options opt;
        vector<WindowSolverBatch::Summary> s1, s2;
        opt.max_num_iterations = iters1;
        if (!solver.solve(opt, &s1)) {
            set_err(err, errlen, solver.error().c_str());
            return -2;
        }
        vector<int> removed((size_t) W, 0);
        if (chi2 > 0) {
            removed                = solver.removeReprojectionFactorsByChi2(chi2);
            opt.max_num_iterations = iters2;
            if (!solver.solve(opt, &s2)) {
                set_err(err, errlen, solver.error().c_str());
                return -4;
            }
        }
        if (solve_ms) *solve_ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
        for (int w = 0; w < W; w++)
            put_summary8(s1[(size_t) w], chi2 > 0 ? &s2[(size_t) w] : nullptr, removed[(size_t) w], summary8 + 8 * (size_t) w);
        return 0;
    });
}

// W windows with the factor mix of icgh_backend_solve_vio (capi_solve.cc) in ONE WindowSolverBatch: window w has n_intervals[w]
// preintegration factors between n_intervals[w] + 1 pose + mix states, its reprojection factors, a pose prior and a mix prior on state 0
// and, where dense[w] != 0, one dense linear factor r = A (x - x0) over all its mix blocks (9 (K + 1) rows and columns, x0 the mix blocks
// at the start, A from dense_seed + w: a constant Jacobian of the width a marginalization prior has).  Every per-window array is reached
// through an array of W pointers and laid out as icgh_backend_solve_vio takes it (ext and the poses constant-extrinsic, constant-td as
// there); params9 is shared; td has W entries; summary4 is W x 4.  mode: 0 = host, 1 = device reduced solve, 2 = device reduced solve and
// device host part.  *solve_ms: the wall time of the solve alone.
int icgh_backend_solve_vio_batch(int W, const int32_t *n_intervals, const int32_t *const *offsets, const double *const *imu, const double *params9,
                                 double *const *states16, const int32_t *n_fac, const double *const *obs_soa, const int32_t *const *idx_i,
                                 const int32_t *const *idx_j, const int32_t *const *idx_lm, double *const *ext, const int32_t *n_lm, double *const *invdepth,
                                 double *td, const double *const *prior_pose0, const double *const *prior_mix0, double prior_weight, double huber, int iters,
                                 const int32_t *dense, double dense_weight, uint32_t dense_seed, double *summary4, double *solve_ms, int mode, char *err,
                                 int errlen) {
    return guarded(err, errlen, [&] {
        if (mode < 0 || mode > 2) {
            set_err(err, errlen, "mode must be 0 (host), 1 (device reduced solve) or 2 (device reduced solve and device host part)");
            return -1;
        }
        if (!WindowSolverBatch::deviceHostPartAvailable()) {
            set_err(err, errlen, kNoHostParts);
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
        // preintegration of every interval from its start state: one icg_preint_batch launch for all windows
        for (int w = 0; w < W; w++) wins.push_back(vio_window(n_intervals[w], offsets[w], imu[w], params, states16[w], raw));
        std::string e;
        if (!Preintegration::integrateBatch(T.ctx, raw, &e)) {
            set_err(err, errlen, e.c_str());
            return -2;
        }
        WindowSolverBatch solver(0, huber);
        solver.setDeviceReducedSolve(mode >= 1);
        solver.setDeviceHostPart(mode == 2);
        for (int w = 0; w < W; w++) {
            const OnBatchWindow win{solver, solver.addWindow()};
            VioWindow &V = wins[(size_t) w];
            vio_blocks(win, V, ext[w], n_lm[w], invdepth[w], td + w);
            reprojections_from_soa(obs_soa[w], n_fac[w], 0, n_fac[w], idx_i[w], idx_j[w], idx_lm[w], V.pose.data(), ext[w], invdepth[w], td + w, factors,
                                   window_add(solver, win.w));
            vio_motion_factors(win, V, prior_pose0[w], prior_weight);
            vio_mix_prior(win, V, prior_mix0[w], prior_weight);
            if (dense && dense[w]) {
                vector<double *> blocks;
                for (int k = 0; k < V.K; k++) blocks.push_back(&V.mix[9 * (size_t) k]);
                win.addResidualBlock(std::make_shared<DenseLinearFactor>(V.K, blocks.data(), dense_weight, dense_seed + (uint32_t) w), nullptr, blocks);
            }
        }
        if (!solver.prepare()) {
            set_err(err, errlen, solver.error().c_str());
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
        for (int w = 0; w < W; w++) {
            put_summary4(sum[(size_t) w], summary4 + 4 * (size_t) w);
            wins[(size_t) w].put(states16[w]);
        }
        return 0;
    });
}

} // extern "C"
