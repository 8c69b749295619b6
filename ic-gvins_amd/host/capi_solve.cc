// C entry points of libicgvins_host.so: the window optimization (WindowSolver / WindowSolverBatch) for tests and bench.py.
#include <atomic>
#include <chrono>
#include <cstdlib>
#include <memory>
#include <thread>

#include "factors.h"
#include "solver_hip.h"
#include "solver_batch_hip.h"
#include "capi_windows.h"

using namespace icg;

extern "C" {

int icgh_backend_solve_batch_parts(int W, const int32_t *fac_off, const int32_t *pose_off, const int32_t *lm_off, const double *obs_soa,
                                   const int32_t *idx_i, const int32_t *idx_j, const int32_t *idx_lm, double *poses, double *ext, double *invdepth,
                                   double *td, const double *prior_poses, double prior_weight, double huber, int ext_constant, int td_constant,
                                   int iters1, int iters2, double chi2, double *summary8, double *solve_ms, char *err, int errlen,
                                   int reduced_solve_mode, int host_part_mode); // capi_solve_parts.cc

// ---- f1: the window optimization flow of GVINS::gvinsOptimization (ic_gvins.cc:1130-1239) on WindowSolver -----------------
// Reprojection factors from flat arrays (as icgh_backend_reproj) + one PosePriorFactor per pose (weight prior_weight, target
// prior_poses: fixes the gauge like the reference's marginalization prior / GNSS factors do).  Two solves with the chi-square
// culling pass in between (chi2 <= 0: one solve of iters1 iterations).  All parameter arrays are updated in place.
// summary10: initial cost, cost after solve 1, final cost, successful steps 1, unsuccessful 1, successful 2, unsuccessful 2, removed,
// ms spent in solve + culling, ms spent building the problem (context, factor upload)
int icgh_backend_solve(int n, const double *obs_soa, const int32_t *idx_i, const int32_t *idx_j, const int32_t *idx_lm, int n_poses,
                       double *poses, double *ext, int n_lm, double *invdepth, double *td, const double *prior_poses, double prior_weight,
                       double huber, int ext_constant, int td_constant, int iters1, int iters2, double chi2, double *summary8,
                       uint8_t *active_out, char *err, int errlen) {
    return guarded(err, errlen, [&] {
        auto t_begin = std::chrono::steady_clock::now();
        vector<std::unique_ptr<ReprojectionFactor>> factors;
        ReprojectionBatch batch(0);
        reprojections_from_soa(obs_soa, n, 0, n, idx_i, idx_j, idx_lm, poses, ext, invdepth, td, factors, batch_add(batch));
        batch.finalize();
        auto t_built = std::chrono::steady_clock::now();
        WindowSolver solver(&batch, huber);
        visual_blocks(solver, n_poses, poses, ext, n_lm, invdepth, td, ext_constant != 0, td_constant != 0);
        pose_priors(solver, n_poses, poses, prior_poses, prior_weight);
        WindowSolver::Options opt;
        WindowSolver::Summary s1, s2;
        opt.max_num_iterations = iters1;
        if (!solver.solve(opt, &s1)) {
            set_err(err, errlen, solver.error().c_str());
            return -2;
        }
        put_summary8(s1, nullptr, 0, summary8);
        if (chi2 > 0) {
            int removed = solver.removeReprojectionFactorsByChi2(chi2);
            if (removed < 0) {
                set_err(err, errlen, solver.error().c_str());
                return -3;
            }
            opt.max_num_iterations = iters2;
            if (!solver.solve(opt, &s2)) {
                set_err(err, errlen, solver.error().c_str());
                return -4;
            }
            put_summary8(s1, &s2, removed, summary8);
        }
        summary8[8] = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_built).count();
        summary8[9] = std::chrono::duration<double, std::milli>(t_built - t_begin).count();
        if (active_out) memcpy(active_out, solver.activeReprojectionFactors().data(), (size_t) n);
        if (getenv("ICG_SOLVER_DEBUG")) fprintf(stderr, "%s\n%s\n", s1.BriefReport().c_str(), s2.BriefReport().c_str());
        return 0;
    });
}

// icgh_backend_solve for W windows at once on WindowSolverBatch (lock-step LM, one launch per phase for all windows).  Arrays are
// concatenated window-major: window w owns factors [fac_off[w], fac_off[w+1]) (obs_soa is 15 x n_total, idx_* LOCAL to the window),
// poses [pose_off[w], ..), inverse depths [lm_off[w], ..); ext is W x 7, td has W entries.  summary8 is W x 8 as in icgh_backend_solve.
// Returns the wall time of the two solves + culling in ms through *solve_ms.
// (the body is that of icgh_backend_solve_batch_parts, capi_solve_parts.cc, with the host parts formed on the host)
// reduced_solve_mode: 0 = the reduced camera solves on the host pool, 1 = on the device (WindowSolverBatch::setDeviceReducedSolve; the same
// bits).  Without the device entry points in the build mode 1 computes nothing: -4 and "icg_reproj_solve_windows is not in this build".
int icgh_backend_solve_batch_mode(int W, const int32_t *fac_off, const int32_t *pose_off, const int32_t *lm_off, const double *obs_soa,
                                  const int32_t *idx_i, const int32_t *idx_j, const int32_t *idx_lm, double *poses, double *ext, double *invdepth,
                                  double *td, const double *prior_poses, double prior_weight, double huber, int ext_constant, int td_constant,
                                  int iters1, int iters2, double chi2, double *summary8, double *solve_ms, char *err, int errlen,
                                  int reduced_solve_mode) {
    if (reduced_solve_mode != 0 && reduced_solve_mode != 1) {
        set_err(err, errlen, "reduced_solve_mode must be 0 (host) or 1 (device)");
        return -1;
    }
    return icgh_backend_solve_batch_parts(W, fac_off, pose_off, lm_off, obs_soa, idx_i, idx_j, idx_lm, poses, ext, invdepth, td, prior_poses, prior_weight,
                                          huber, ext_constant, td_constant, iters1, iters2, chi2, summary8, solve_ms, err, errlen, reduced_solve_mode, 0);
}

int icgh_backend_solve_batch(int W, const int32_t *fac_off, const int32_t *pose_off, const int32_t *lm_off, const double *obs_soa, const int32_t *idx_i,
                             const int32_t *idx_j, const int32_t *idx_lm, double *poses, double *ext, double *invdepth, double *td,
                             const double *prior_poses, double prior_weight, double huber, int ext_constant, int td_constant, int iters1, int iters2,
                             double chi2, double *summary8, double *solve_ms, char *err, int errlen) {
    return icgh_backend_solve_batch_mode(W, fac_off, pose_off, lm_off, obs_soa, idx_i, idx_j, idx_lm, poses, ext, invdepth, td, prior_poses, prior_weight,
                                         huber, ext_constant, td_constant, iters1, iters2, chi2, summary8, solve_ms, err, errlen, 0);
}

// Aggregate solve throughput with many windows in flight: `threads` host threads, each with its own ReprojectionBatch (own icg_ctx
// and HIP stream, like the stream groups of the front-end) and its own copy of the problem, each solving it `repeat` times from
// the same start (problem construction outside the timed region).  Returns the wall time in seconds for threads x repeat solves,
// < 0 on error.  Same flow as icgh_backend_solve (two solves with the chi-square pass).
double icgh_backend_solve_throughput(int n, const double *obs_soa, const int32_t *idx_i, const int32_t *idx_j, const int32_t *idx_lm, int n_poses,
                                     const double *poses, const double *ext, int n_lm, const double *invdepth, double td,
                                     const double *prior_poses, double prior_weight, double huber, int iters1, int iters2, double chi2, int threads,
                                     int repeat, char *err, int errlen) {
    return guarded(err, errlen, -1.0, [&] {
        struct Job {
            vector<double> P, E, D;
            double TD;
            vector<std::unique_ptr<ReprojectionFactor>> factors;
            std::unique_ptr<ReprojectionBatch> batch;
        };
        vector<std::unique_ptr<Job>> jobs;
        for (int t = 0; t < threads; t++) {
            std::unique_ptr<Job> J(new Job);
            J->P.assign(poses, poses + 7 * (size_t) n_poses), J->E.assign(ext, ext + 7), J->D.assign(invdepth, invdepth + n_lm), J->TD = td;
            J->batch.reset(new ReprojectionBatch(0));
            if (threads > 4) J->batch->setWaitMode(ICG_WAIT_POLL, 5); // more solvers than spare host cores: do not spin on completion
            reprojections_from_soa(obs_soa, n, 0, n, idx_i, idx_j, idx_lm, J->P.data(), J->E.data(), J->D.data(), &J->TD, J->factors, batch_add(*J->batch));
            J->batch->finalize();
            jobs.push_back(std::move(J));
        }
        std::atomic<int> failed{0};
        auto work = [&](int t) {
            Job &J = *jobs[(size_t) t];
            for (int r = 0; r < repeat; r++) {
                J.P.assign(poses, poses + 7 * (size_t) n_poses), J.E.assign(ext, ext + 7), J.D.assign(invdepth, invdepth + n_lm), J.TD = td;
                WindowSolver solver(J.batch.get(), huber);
                visual_blocks(solver, n_poses, J.P.data(), J.E.data(), n_lm, J.D.data(), &J.TD, false, false);
                pose_priors(solver, n_poses, J.P.data(), prior_poses, prior_weight);
                WindowSolver::Options opt;
                WindowSolver::Summary s1;
                opt.max_num_iterations = iters1;
                if (!solver.solve(opt, &s1)) failed++;
                if (chi2 > 0) {
                    solver.removeReprojectionFactorsByChi2(chi2);
                    opt.max_num_iterations = iters2;
                    if (!solver.solve(opt, &s1)) failed++;
                }
            }
        };
        auto t0 = std::chrono::steady_clock::now();
        vector<std::thread> th;
        for (int t = 1; t < threads; t++) th.emplace_back(work, t);
        work(0);
        for (auto &x : th) x.join();
        double sec = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
        if (failed.load()) {
            set_err(err, errlen, "a solve failed");
            return -2.0;
        }
        return sec;
    });
}

// f1 with the factor mix of the real window: K preintegration factors (device P1 + host P2) between K+1 states, reprojection
// factors on the same pose blocks (device), a pose prior and a velocity/bias prior on state 0 (what the marginalization prior
// provides in the real window).  states: (K+1) x 16 (p3, q4 xyzw, v3, bg3, ba3) in/out;
// imu rows of 8, interval k owns rows [offsets[k], offsets[k+1]).  summary4: initial cost, final cost, successful, unsuccessful steps.
int icgh_backend_solve_vio(int n_intervals, const int32_t *offsets, const double *imu, const double *params9, double *states16, int n,
                           const double *obs_soa, const int32_t *idx_i, const int32_t *idx_j, const int32_t *idx_lm, double *ext, int n_lm,
                           double *invdepth, double *td, const double *prior_pose0, const double *prior_mix0, double prior_weight, double huber,
                           int iters, double *summary4, char *err, int errlen) {
    return guarded(err, errlen, [&] {
        vector<std::unique_ptr<ReprojectionFactor>> factors;
        ReprojectionBatch batch(0);
        // preintegration of every interval from its start state: one icg_preint_batch launch on a context of its own
        TempCtx T(0);
        vector<Preintegration *> raw;
        VioWindow W = vio_window(n_intervals, offsets, imu, preint_params(params9), states16, raw);
        reprojections_from_soa(obs_soa, n, 0, n, idx_i, idx_j, idx_lm, W.pose.data(), ext, invdepth, td, factors, batch_add(batch));
        batch.finalize();
        std::string e;
        if (!Preintegration::integrateBatch(T.ctx, raw, &e)) {
            set_err(err, errlen, e.c_str());
            return -2;
        }
        WindowSolver solver(&batch, huber);
        vio_blocks(solver, W, ext, n_lm, invdepth, td);
        vio_motion_factors(solver, W, prior_pose0, prior_weight);
        vio_mix_prior(solver, W, prior_mix0, prior_weight);
        WindowSolver::Options opt;
        WindowSolver::Summary sum;
        opt.max_num_iterations = iters;
        if (!solver.solve(opt, &sum)) {
            set_err(err, errlen, solver.error().c_str());
            return -3;
        }
        put_summary4(sum, summary4);
        W.put(states16);
        if (getenv("ICG_SOLVER_DEBUG")) fprintf(stderr, "%s\n", sum.BriefReport().c_str());
        return 0;
    });
}

} // extern "C"
