// WindowSolverBatch: W Levenberg-Marquardt problems in lock-step on one device context.  See solver_batch_hip.h.
#include "solver_batch_hip.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <stdexcept>
#include <thread>

#include "../../include/icgvins_hip.h"

// A build of this layer on another implementation of the C ABI may not have the entry points: the references stay weak (null when absent)
// and solve() reports it; the product library links libicgvins_hip.so, which defines them.
#pragma weak icg_chol_solve_batch
#pragma weak icg_reproj_schur_windows_resident
#pragma weak icg_reproj_solve_windows
#pragma weak icg_reproj_host_parts_build

namespace icg {

using solver_detail::choleskySolve;

bool WindowSolverBatch::deviceReducedSolveAvailable() {
    return &icg_chol_solve_batch != nullptr && &icg_reproj_schur_windows_resident != nullptr && &icg_reproj_solve_windows != nullptr;
}

bool WindowSolverBatch::deviceHostPartAvailable() { return &icg_reproj_host_parts_build != nullptr; }

// The per-window host phases of an LM step (host factors, reduced solves, trial bookkeeping) take tens of microseconds per window: they
// run on a persistent pool — spawning threads per phase (four phases per step) cost more than the phases themselves.
template <typename F> void WindowSolverBatch::forEachWindow(size_t n, F &&fn) {
    if (host_threads_ <= 1 || n < 4) {
        for (size_t w = 0; w < n; w++) fn(w);
        return;
    }
    if (!pool_) pool_.reset(new HostPool(host_threads_));
    const std::function<void(int)> f = [&](int w) { fn((size_t) w); };
    pool_->parallelFor((int) n, f);
}

WindowSolverBatch::WindowSolverBatch(int device, double huber_delta, int host_threads) : huber_(huber_delta) {
    host_threads_ = host_threads > 0 ? host_threads : (int) std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
    if (const char *e = getenv("ICG_SOLVER_THREADS")) host_threads_ = std::max(1, atoi(e)); // diagnostics
    icg_ctx_config cfg{};
    cfg.device = device, cfg.width = 64, cfg.height = 64, cfg.n_slots = 1, cfg.max_batch = 1, cfg.max_points = 64;
    if (icg_ctx_create(&cfg, &ctx_) != ICG_OK) throw std::runtime_error(std::string("WindowSolverBatch: ") + icg_last_error(nullptr));
}

WindowSolverBatch::~WindowSolverBatch() { icg_ctx_destroy(ctx_); }

int WindowSolverBatch::addWindow() {
    windows_.emplace_back();
    finalized_ = false;
    return (int) windows_.size() - 1;
}

void WindowSolverBatch::clear() {
    windows_.clear();
    active_.clear();
    col_pose_.clear(), col_ext_.clear(), col_td_.clear();
    P_ = n_factors_ = n_poses_ = n_lm_ = 0;
    finalized_ = false;
    error_.clear();
}

void WindowSolverBatch::removeResidualBlock(int w, int id) { windows_.at((size_t) w).problem.removeResidualBlock(id); }

bool WindowSolverBatch::evaluateResidualBlock(int w, int id, bool apply_loss_function, double *cost) const {
    return windows_.at((size_t) w).problem.evaluateResidualBlock(id, apply_loss_function, cost);
}

void WindowSolverBatch::addParameterBlock(int w, double *values, int size, bool pose_manifold) {
    windows_.at((size_t) w).problem.addParameterBlock(values, size, pose_manifold);
}

void WindowSolverBatch::setParameterBlockConstant(int w, double *values) { windows_.at((size_t) w).problem.setParameterBlockConstant(values); }

int WindowSolverBatch::addResidualBlock(int w, std::shared_ptr<ceres::CostFunction> cost, std::shared_ptr<ceres::LossFunction> loss,
                                        const std::vector<double *> &blocks) {
    return windows_.at((size_t) w).problem.addResidualBlock(std::move(cost), std::move(loss), blocks);
}

void WindowSolverBatch::addReprojectionFactor(int w, const ReprojectionFactor *factor, double *pose_i, double *pose_j, double *extrinsic, double *invdepth,
                                              double *td) {
    Window &W = windows_.at((size_t) w);
    if ((W.ext && W.ext != extrinsic) || (W.td && W.td != td)) throw std::runtime_error("WindowSolverBatch: one extrinsic / td block per window");
    W.ext = extrinsic, W.td = td;
    VisualFactor f;
    memcpy(f.obs, factor->observation(), sizeof f.obs);
    f.pose_i = pose_i, f.pose_j = pose_j, f.invdepth = invdepth;
    for (double *p : {pose_i, pose_j})
        if (!W.pose_index.count(p)) {
            W.pose_index[p] = (int) W.poses.size();
            W.poses.push_back(p);
        }
    if (!W.lm_index.count(invdepth)) {
        W.lm_index[invdepth] = (int) W.landmarks.size();
        W.landmarks.push_back(invdepth);
    }
    W.visual.push_back(f);
    finalized_ = false;
}

// uploads the factors of all windows (window-major) and the partition
bool WindowSolverBatch::finalize() {
    n_factors_ = n_poses_ = n_lm_ = 0;
    std::vector<int32_t> fac_off{0}, lm_off{0};
    for (Window &W : windows_) {
        W.fac_begin = n_factors_, W.pose_begin = n_poses_, W.lm_begin = n_lm_;
        n_factors_ += (int) W.visual.size(), n_poses_ += (int) W.poses.size(), n_lm_ += (int) W.landmarks.size();
        fac_off.push_back(n_factors_), lm_off.push_back(n_lm_);
    }
    if (n_factors_ == 0) {
        error_ = "no reprojection factors";
        return false;
    }
    // (written by the pool's threads straight into the context's pinned staging block: icg_reproj_stage_factors)
    double *obs   = nullptr;
    int32_t *idx3 = nullptr;
    if (icg_reproj_stage_factors(ctx_, n_factors_, &obs, &idx3) != ICG_OK) {
        error_ = icg_last_error(ctx_);
        return false;
    }
    int32_t *ii = idx3, *jj = idx3 + n_factors_, *ll = idx3 + 2 * (size_t) n_factors_;
    forEachWindow(windows_.size(), [&](size_t w) {
        const Window &W = windows_[w];
        for (size_t k = 0; k < W.visual.size(); k++) {
            const size_t f = (size_t) W.fac_begin + k;
            for (int c = 0; c < 15; c++) obs[(size_t) c * n_factors_ + f] = W.visual[k].obs[c];
            ii[f] = W.pose_begin + W.pose_index.at(W.visual[k].pose_i);
            jj[f] = W.pose_begin + W.pose_index.at(W.visual[k].pose_j);
            ll[f] = W.lm_begin + W.lm_index.at(W.visual[k].invdepth);
        }
    });
    if (icg_reproj_commit_factors(ctx_) != ICG_OK ||
        icg_reproj_set_windows(ctx_, (int) windows_.size(), fac_off.data(), lm_off.data()) != ICG_OK) {
        error_ = icg_last_error(ctx_);
        return false;
    }
    active_.assign((size_t) n_factors_, 1);
    finalized_ = true;
    return true;
}

bool WindowSolverBatch::prepare() {
    if (!finalized_ && !finalize()) return false;
    // device memory of the window systems and the staging memory of a step, for the layout as it stands now (solve() re-derives the layout)
    if (layout()) (void) icg_reproj_reserve_windows(ctx_, P_);
    error_.clear();
    return true;
}

bool WindowSolverBatch::layout() {
    P_ = 0;
    col_pose_.assign((size_t) n_poses_, -1);
    col_ext_.assign(windows_.size(), -1);
    col_td_.assign(windows_.size(), -1);
    // (a thousand hash look-ups per window: 1.3 ms for 256 windows on one thread, at the head of every solve — spread over the pool)
    std::vector<std::string> errs(windows_.size());
    forEachWindow(windows_.size(), [&](size_t w) {
        Window &W = windows_[w];
        W.P       = W.problem.assignColumns(W.landmarks, &errs[w]);
        if (W.P < 0) return;
        for (size_t k = 0; k < W.poses.size(); k++) col_pose_[(size_t) W.pose_begin + k] = W.problem.column(W.poses[k]);
        if (W.ext) col_ext_[w] = W.problem.column(W.ext);
        if (W.td) col_td_[w] = W.problem.column(W.td);
        if (!device_host_part_) return;
        // the blocks of the window's host part: their shapes and columns follow from the problem, not from an evaluation
        W.host_blocks.clear(), W.host_cols.clear();
        std::vector<int> cols;
        for (size_t id = 0; id < W.problem.residuals.size(); id++) {
            const solver_detail::Residual &R = W.problem.residuals[id];
            if (R.removed) continue;
            solver_detail::hostBlockColumns(W.problem, R, cols);
            if (cols.empty()) continue;
            W.host_blocks.push_back({(int) id, R.cost->num_residuals(), (int) cols.size(), 0, 0, 0});
            W.host_cols.insert(W.host_cols.end(), cols.begin(), cols.end());
        }
    });
    for (size_t w = 0; w < windows_.size(); w++) {
        if (!errs[w].empty()) {
            error_ = errs[w];
            return false;
        }
        P_ = std::max(P_, windows_[w].P);
    }
    if (device_host_part_) {
        hp_blk_off_.assign(1, 0), hp_nr_.clear(), hp_nf_.clear(), hp_cols_.clear();
        hp_J_total_ = hp_r_total_ = 0;
        for (Window &W : windows_) {
            W.blk_begin = (int) hp_nr_.size();
            for (Window::HostBlock &B : W.host_blocks) {
                B.J_off = hp_J_total_, B.r_off = hp_r_total_, B.c_off = hp_cols_.size();
                hp_J_total_ += (size_t) B.nr * B.nf, hp_r_total_ += (size_t) B.nr;
                hp_nr_.push_back(B.nr), hp_nf_.push_back(B.nf);
            }
            hp_cols_.insert(hp_cols_.end(), W.host_cols.begin(), W.host_cols.end());
            hp_blk_off_.push_back((int32_t) hp_nr_.size());
        }
    }
    return P_ > 0;
}

void WindowSolverBatch::gather(std::vector<double> &poses, std::vector<double> &ext, std::vector<double> &inv, std::vector<double> &td) {
    poses.resize(7 * (size_t) n_poses_), ext.assign(7 * windows_.size(), 0.0), inv.resize((size_t) n_lm_), td.assign(windows_.size(), 0.0);
    // (scattered reads through the callers' parameter pointers: spread over the pool like the other per-window phases)
    forEachWindow(windows_.size(), [&](size_t w) {
        const Window &W = windows_[w];
        for (size_t k = 0; k < W.poses.size(); k++) memcpy(&poses[7 * ((size_t) W.pose_begin + k)], W.poses[k], sizeof(double) * 7);
        for (size_t k = 0; k < W.landmarks.size(); k++) inv[(size_t) W.lm_begin + k] = *W.landmarks[k];
        if (W.ext) memcpy(&ext[7 * w], W.ext, sizeof(double) * 7);
        if (W.td) td[w] = *W.td;
    });
}

namespace {
struct BatchClock { // ICG_SOLVER_DEBUG=1: wall time per phase of the lock-step loop
    bool on = getenv("ICG_SOLVER_DEBUG") != nullptr;
    double ms[10] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0};
    std::chrono::steady_clock::time_point t;
    void start() {
        if (on) t = std::chrono::steady_clock::now();
    }
    void stop(int k) {
        if (on) ms[k] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
    }
};
} // namespace

bool WindowSolverBatch::solve(const Options &o, std::vector<Summary> *summaries) {
    BatchClock clk;
    const auto t_solve = std::chrono::steady_clock::now();
    if (!finalized_ && !finalize()) return false;
    if (!layout()) {
        if (error_.empty()) error_ = "nothing to optimize";
        return false;
    }
    const size_t NW = windows_.size();
    const int P     = P_;
    const bool dev_solve = device_reduced_, dev_part = device_host_part_;
    if (dev_solve && !deviceReducedSolveAvailable()) {
        error_ = "icg_reproj_solve_windows is not in this build";
        return false;
    }
    if (dev_part && !deviceHostPartAvailable()) {
        error_ = "icg_reproj_host_parts_build is not in this build";
        return false;
    }
    if (dev_part && !dev_solve) {
        error_ = "setDeviceHostPart(true) needs setDeviceReducedSolve(true): the host parts are built where the device solve reads them";
        return false;
    }
    // The reduced systems: their lower tiles are read where the reduction kernel writes them (pinned memory) and every window is factored by a
    // host thread (dense_kernels.cc).  An earlier device form, since deleted (a workgroup per window, three barriers per column, every host
    // part shipped per re-linearization), lost to this on MI355X, 256 C2 windows (P = 67), two solves: 26.5 ms against 21.1 ms.  With
    // setDeviceReducedSolve(true) the systems stay on the device instead and one wave per window solves them there without a barrier
    // (icg_reproj_solve_windows, k_chol_solve), this thread pool only damping and deciding; DESIGN.md section 8 item 3 has the times of both.
    struct State {
        solver_detail::TrustRegion tr;
        double model;
        bool done, relinearize, redamp, stepped;
        int iters;
        std::vector<double> s, diag, delta_c, dd;
    };
    std::vector<State> st(NW, State{solver_detail::TrustRegion(o), 0, false, true, false, false, 0, {}, {}, {}, {}});
    std::vector<double> poses, ext, inv, td, s((size_t) NW * P), diag((size_t) NW * P), cost(NW), delta_c((size_t) NW * P), delta_l((size_t) n_lm_),
        terms(2 * NW), damp(NW);
    const double *S = nullptr; // W x P x P reduced systems, left in the context's pinned staging memory by the reduction kernel (valid until
                               // the next call on ctx_: consumed by the reduced solves below, before the back-substitution call)
    std::vector<uint8_t> reassemble(NW);
    std::vector<double> host_cost(NW, 0.0);
    // device reduced solve: what one icg_reproj_solve_windows call takes and returns
    std::vector<int32_t> dev_Pw, dev_status;
    std::vector<uint8_t> dev_solve_flag, dev_part_new;
    std::vector<double> dev_dd, dev_rhs, dev_parts;
    std::vector<size_t> dev_part_off;
    if (dev_solve) {
        dev_Pw.resize(NW), dev_status.resize(NW), dev_solve_flag.resize(NW), dev_part_new.resize(NW), dev_part_off.resize(NW + 1);
        dev_dd.resize((size_t) NW * P), dev_rhs.resize((size_t) NW * P);
        for (size_t w = 0; w < NW; w++) dev_Pw[w] = windows_[w].P, windows_[w].host_part_dirty = false;
    }
    // device host part: the buffers of one icg_reproj_host_parts_build call (J and r of every block at the offsets of layout()), the
    // Jacobians as each block last shipped them in this solve, and what comes back
    std::vector<double> hp_J, hp_r, hp_shipped, hp_s, hp_diag;
    std::vector<int64_t> hp_jac_off;
    std::vector<uint8_t> hp_has_shipped;
    if (dev_part) {
        hp_J.resize(hp_J_total_), hp_shipped.resize(hp_J_total_), hp_r.assign(hp_r_total_, 0.0);
        hp_jac_off.assign(hp_nr_.size(), 0), hp_has_shipped.assign(hp_nr_.size(), 0);
        hp_s.assign((size_t) NW * P, 0.0), hp_diag.assign((size_t) NW * P, 0.0);
    }
    auto fail = [&](const char *what) {
        error_ = std::string(what) + ": " + icg_last_error(ctx_);
        return false;
    };
    bool first = true;
    for (;;) {
        // ---- (re)linearize / re-damp --------------------------------------------------------------------------------------------
        bool any_lin = false, any_sys = false;
        for (size_t w = 0; w < NW; w++) {
            reassemble[w] = (!st[w].done && st[w].relinearize) ? 1 : 0;
            damp[w]       = 1.0 / st[w].tr.radius;
            any_lin |= reassemble[w] != 0;
            any_sys |= !st[w].done && (st[w].relinearize || st[w].redamp);
        }
        if (any_lin) {
            clk.start();
            gather(poses, ext, inv, td);
            if (icg_reproj_eval_windows(ctx_, n_poses_, poses.data(), ext.data(), n_lm_, inv.data(), td.data(), 1, huber_) != ICG_OK)
                return fail("icg_reproj_eval_windows");
            clk.stop(0);
        }
        if (any_sys) {
            // The device half (assembly + landmark elimination of every window: one call) and the host half (the host-evaluated factors of
            // every window that is re-linearized: priors, preintegration, marginalization prior — on the pool) do not depend on each other:
            // the call runs on a helper thread while this one drives the pool (what WindowSolver::linearize does per window with
            // runHalves); the sums that need both are formed after the join.
            clk.start();
            int dev_rc = ICG_OK;
            if (!side_) side_.reset(new SideThread());
            SideCall dev(*side_, [&] {
                if (dev_solve)
                    dev_rc = icg_reproj_schur_windows_resident(ctx_, P, col_pose_.data(), col_ext_.data(), col_td_.data(), active_.data(), reassemble.data(),
                                                               damp.data(), o.min_lm_diagonal, o.max_lm_diagonal, s.data(), diag.data(), cost.data());
                else
                    dev_rc = icg_reproj_schur_windows_view(ctx_, P, col_pose_.data(), col_ext_.data(), col_td_.data(), active_.data(), reassemble.data(),
                                                           damp.data(), o.min_lm_diagonal, o.max_lm_diagonal, &S, s.data(), diag.data(), cost.data());
            });
            std::atomic<int> host_failed{0};
            host_cost.assign(NW, 0.0);
            forEachWindow(NW, [&](size_t w) {
                if (st[w].done || !st[w].relinearize) return;
                Window &W = windows_[w];
                if (dev_part) {
                    // evaluate and gather only: every block's Jd and res at its place in the call buffers, the cost in residual order
                    thread_local std::vector<int> cols;
                    thread_local std::vector<double> none;
                    size_t next = 0;
                    for (size_t id = 0; id < W.problem.residuals.size(); id++) {
                        const solver_detail::Residual &R = W.problem.residuals[id];
                        if (R.removed) continue;
                        const bool has = next < W.host_blocks.size() && W.host_blocks[next].residual == (int) id;
                        double *Jd     = has ? &hp_J[W.host_blocks[next].J_off] : nullptr;
                        if (solver_detail::gatherHostBlock(W.problem, R, &host_cost[w], cols, none, none, Jd, has ? &hp_r[W.host_blocks[next].r_off] : nullptr) < 0) {
                            host_failed++;
                            return;
                        }
                        if (!has) continue;
                        // the same Jacobian as at the window's previous rebuild stays where it is on the device
                        const Window::HostBlock &B = W.host_blocks[next];
                        const size_t b = (size_t) W.blk_begin + next, bytes = sizeof(double) * (size_t) B.nr * B.nf;
                        if (hp_has_shipped[b] && memcmp(Jd, &hp_shipped[B.J_off], bytes) == 0) {
                            hp_jac_off[b] = -1;
                        } else {
                            hp_jac_off[b] = (int64_t) B.J_off;
                            memcpy(&hp_shipped[B.J_off], Jd, bytes);
                            hp_has_shipped[b] = 1;
                        }
                        next++;
                    }
                    return;
                }
                W.host_S.assign((size_t) P * P, 0.0), W.host_s.assign((size_t) P, 0.0), W.host_diag.assign((size_t) P, 0.0);
                if (!solver_detail::hostFactors(W.problem, P, W.host_S.data(), W.host_s.data(), W.host_diag.data(), &host_cost[w])) host_failed++;
                W.host_part_dirty = true;
            });
            clk.stop(2);
            clk.start();
            dev.join();
            clk.stop(1); // (what is left of the device call once the host half is through)
            if (dev_rc != ICG_OK) return fail(dev_solve ? "icg_reproj_schur_windows_resident" : "icg_reproj_schur_windows_view");
            if (host_failed.load()) {
                error_ = "a host cost function failed to evaluate";
                return false;
            }
            if (dev_part && any_lin) {
                // the parts of the re-linearized windows, built in their slots on the device; s and diag of those windows come back
                clk.start();
                if (icg_reproj_host_parts_build(ctx_, P, dev_Pw.data(), reassemble.data(), hp_blk_off_.data(), hp_nr_.data(), hp_nf_.data(), hp_cols_.data(),
                                                hp_jac_off.data(), hp_J.data(), hp_r.data(), hp_s.data(), hp_diag.data(), nullptr) != ICG_OK)
                    return fail("icg_reproj_host_parts_build");
                clk.stop(8);
            }
            clk.start();
            forEachWindow(NW, [&](size_t w) {
                State &T = st[w];
                if (T.done || !(T.relinearize || T.redamp)) return;
                Window &W = windows_[w];
                // the cost at the linearization point initialises the window on the first pass; afterwards it equals the accepted
                // trial cost and is kept (the same bookkeeping as WindowSolver)
                if (T.relinearize && first) T.tr.cost = cost[w] + host_cost[w], T.tr.summary.initial_cost = T.tr.cost;
                // the window's reduced system is used where it arrived (S, s, diag of the batched call) plus the host factors' part: no
                // per-window copy of the P x P block (9 MB per step at 256 windows)
                T.s.resize((size_t) P), T.diag.resize((size_t) P);
                const double *hs = dev_part ? &hp_s[w * P] : W.host_s.data(), *hd = dev_part ? &hp_diag[w * P] : W.host_diag.data();
                for (int k = 0; k < P; k++) {
                    T.s[(size_t) k]    = s[w * P + (size_t) k] + hs[(size_t) k];
                    T.diag[(size_t) k] = diag[w * P + (size_t) k] + hd[(size_t) k];
                }
                T.relinearize = T.redamp = false;
            });
            clk.stop(2);
        }
        first = false;
        // ---- every open window: iteration budget, gradient test, reduced solve ----------------------------------------------------
        clk.start();
        std::fill(delta_c.begin(), delta_c.end(), 0.0);
        forEachWindow(NW, [&](size_t w) {
            State &T  = st[w];
            T.stepped = false;
            if (T.done) return;
            if (T.iters >= o.max_num_iterations) {
                T.done = true;
                return;
            }
            T.iters++;
            if (T.tr.gradientConverged(o, T.s)) {
                T.done = true;
                return;
            }
            const int Pw = windows_[w].P; // columns beyond Pw are empty (zero rows): solve the leading block only
            T.tr.damp(o, T.diag, Pw, T.dd);
            if (dev_solve) { // the solve itself follows for all windows at once
                std::copy(T.dd.begin(), T.dd.end(), dev_dd.begin() + (long) (w * P));
                std::copy(T.s.begin(), T.s.end(), dev_rhs.begin() + (long) (w * P));
                T.stepped = true;
                return;
            }
            std::vector<double> Ab((size_t) Pw * Pw), bb(T.s.begin(), T.s.begin() + Pw);
            const double *Sw = &S[w * (size_t) P * P], *Hw = windows_[w].host_S.data();
            for (int i = 0; i < Pw; i++) // lower triangle: what the view holds and what choleskySolve reads
                for (int j = 0; j <= i; j++) Ab[(size_t) i * Pw + j] = Sw[(size_t) i * P + j] + Hw[(size_t) i * P + j];
            for (int k = 0; k < Pw; k++) Ab[(size_t) k * Pw + k] += T.dd[(size_t) k];
            if (!choleskySolve(Pw, Ab, bb)) {
                T.redamp = true;
                T.done   = T.tr.reject(o);
                return;
            }
            T.delta_c.assign((size_t) P, 0.0);
            std::copy(bb.begin(), bb.end(), T.delta_c.begin());
            std::copy(T.delta_c.begin(), T.delta_c.end(), delta_c.begin() + (long) (w * P));
            T.stepped = true;
        });
        bool dev_any = false;
        if (dev_solve) {
            // the windows that solve in this step, and of those the host parts a re-linearization rebuilt since they were last shipped
            size_t total = 0;
            for (size_t w = 0; w < NW; w++) {
                dev_solve_flag[w] = st[w].stepped ? 1 : 0;
                dev_part_new[w]   = st[w].stepped && windows_[w].host_part_dirty ? 1 : 0;
                dev_part_off[w]   = total;
                if (dev_part_new[w]) total += (size_t) dev_Pw[w] * ((size_t) dev_Pw[w] + 1) / 2;
                dev_any |= st[w].stepped;
            }
            dev_part_off[NW] = total;
            dev_parts.resize(total);
            forEachWindow(NW, [&](size_t w) {
                if (!dev_part_new[w]) return;
                const double *Hw = windows_[w].host_S.data();
                double *dst      = dev_parts.data() + dev_part_off[w];
                for (int i = 0; i < dev_Pw[w]; i++, dst += i) memcpy(dst, Hw + (size_t) i * P, sizeof(double) * ((size_t) i + 1));
            });
        }
        if (dev_any) {
            if (icg_reproj_solve_windows(ctx_, P, dev_Pw.data(), dev_solve_flag.data(), dev_part ? nullptr : dev_part_new.data(),
                                         dev_parts.empty() ? nullptr : dev_parts.data(),
                                         dev_dd.data(), dev_rhs.data(), delta_c.data(), dev_status.data(), delta_l.data(), terms.data()) != ICG_OK)
                return fail("icg_reproj_solve_windows");
            for (size_t w = 0; w < NW; w++) {
                State &T = st[w];
                if (!T.stepped) continue;
                windows_[w].host_part_dirty = false;
                if (dev_status[w] != 0) {
                    T.stepped = false, T.redamp = true;
                    T.done = T.tr.reject(o);
                    continue;
                }
                T.delta_c.assign(delta_c.begin() + (long) (w * P), delta_c.begin() + (long) ((w + 1) * P));
            }
        }
        bool any_step = false, all_done = true;
        for (size_t w = 0; w < NW; w++) any_step |= st[w].stepped, all_done &= st[w].done;
        clk.stop(3);
        if (all_done) break;
        if (!any_step) continue; // only re-damping this round
        // ---- landmark back-substitution for all windows, model decrease, trial points ---------------------------------------------
        clk.start();
        if (!dev_solve && n_lm_ > 0 && icg_reproj_backsub_windows(ctx_, P, delta_c.data(), delta_l.data(), terms.data()) != ICG_OK)
            return fail("icg_reproj_backsub_windows");
        clk.stop(4);
        clk.start();
        forEachWindow(NW, [&](size_t w) {
            State &T = st[w];
            if (!T.stepped) return;
            Window &W = windows_[w];
            T.model   = solver_detail::TrustRegion::modelDecrease(&terms[2 * w], T.delta_c, T.s, T.dd);
            if (!(T.model > 0.0)) {
                T.redamp = true, T.stepped = false;
                T.done   = T.tr.reject(o);
                return;
            }
            if (T.tr.parameterConverged(o, W.problem, T.delta_c, delta_l.data() + W.lm_begin, W.landmarks.size())) {
                T.done = true, T.stepped = false;
                return;
            }
            W.problem.backup();
            W.problem.applyCameraStep(T.delta_c.data());
            for (size_t k = 0; k < W.landmarks.size(); k++) *W.landmarks[k] += delta_l[(size_t) W.lm_begin + k];
        });
        bool any_trial = false;
        for (size_t w = 0; w < NW; w++) any_trial |= st[w].stepped;
        clk.stop(5);
        if (!any_trial) continue;
        // the trial costs: the visual factors' on the device (evaluation + cost reduction, one call each) beside the host factors' on the pool
        clk.start();
        gather(poses, ext, inv, td);
        const char *dev_fail = nullptr;
        if (!side_) side_.reset(new SideThread());
        SideCall trial(*side_, [&] {
            if (icg_reproj_eval_windows(ctx_, n_poses_, poses.data(), ext.data(), n_lm_, inv.data(), td.data(), 0, huber_) != ICG_OK)
                dev_fail = "icg_reproj_eval_windows";
            else if (icg_reproj_cost_windows(ctx_, active_.data(), cost.data()) != ICG_OK)
                dev_fail = "icg_reproj_cost_windows";
        });
        std::atomic<int> trial_failed{0};
        host_cost.assign(NW, 0.0);
        forEachWindow(NW, [&](size_t w) {
            if (!st[w].stepped) return;
            if (!solver_detail::hostFactors(windows_[w].problem, P, nullptr, nullptr, nullptr, &host_cost[w])) trial_failed++;
        });
        trial.join();
        if (dev_fail) return fail(dev_fail);
        clk.stop(6);
        clk.start();
        forEachWindow(NW, [&](size_t w) {
            State &T = st[w];
            if (!T.stepped || trial_failed.load()) return;
            bool accepted;
            T.done = T.tr.trial(o, cost[w] + host_cost[w], T.model, windows_[w].problem, &accepted);
            if (accepted)
                T.relinearize = !T.done;
            else
                T.redamp = true;
        });
        if (trial_failed.load()) {
            error_ = "a host cost function failed to evaluate";
            return false;
        }
        clk.stop(7);
    }
    if (clk.on)
        fprintf(stderr, "[WindowSolverBatch] %zu windows: eval+jac %.2f, schur beyond the host half %.2f, host linearize (beside the device call) %.2f, reduced solves %.2f, backsub %.2f, model+apply %.2f, "
                        "trial eval+cost %.2f, trial host %.2f, host parts on the device %.2f ms; whole solve %.2f ms\n",
                NW, clk.ms[0], clk.ms[1], clk.ms[2], clk.ms[3], clk.ms[4], clk.ms[5], clk.ms[6], clk.ms[7], clk.ms[8],
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_solve).count());
    if (summaries) {
        summaries->resize(NW);
        for (size_t w = 0; w < NW; w++) (*summaries)[w] = st[w].tr.summary, (*summaries)[w].final_cost = st[w].tr.cost;
    }
    return true;
}

std::vector<int> WindowSolverBatch::removeReprojectionFactorsByChi2(double chi2) {
    std::vector<int> removed(windows_.size(), 0);
    if (!finalized_ && !finalize()) return removed;
    std::vector<double> poses, ext, inv, td;
    gather(poses, ext, inv, td);
    // raw residuals, no loss: problem.EvaluateResidualBlock(id, false, &cost, ...) with cost = 0.5 |r|^2 (ic_gvins.cc:1278-1284); the
    // test runs where the residuals are, only the flags come back
    std::vector<uint8_t> before(active_);
    if (icg_reproj_eval_windows(ctx_, n_poses_, poses.data(), ext.data(), n_lm_, inv.data(), td.data(), 0, 0.0) != ICG_OK ||
        icg_reproj_chi2_cull(ctx_, chi2, active_.data()) != ICG_OK) {
        error_ = icg_last_error(ctx_);
        active_.swap(before);
        return removed;
    }
    forEachWindow(windows_.size(), [&](size_t w) {
        int r = 0;
        for (size_t k = 0; k < windows_[w].visual.size(); k++) {
            const size_t f = (size_t) windows_[w].fac_begin + k;
            r += before[f] && !active_[f];
        }
        removed[w] = r;
    });
    return removed;
}

} // namespace icg
