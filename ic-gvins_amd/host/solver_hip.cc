// WindowSolver: Levenberg-Marquardt on the reduced camera system, visual factors eliminated on the device.  See solver_hip.h.
#include "solver_hip.h"

#include <chrono>
#include <cmath>
#include <cstdlib>
#include <cstdio>
#include <atomic>
#include <functional>
#include <mutex>

#include "../../include/icgvins_hip.h"

namespace icg {

namespace {
// ICG_SOLVER_DEBUG=1: wall time per phase of the LM loop, printed by solve()
struct PhaseClock {
    double ms[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    int calls[8] = {0, 0, 0, 0, 0, 0, 0, 0};
    bool on = getenv("ICG_SOLVER_DEBUG") != nullptr;
};
thread_local PhaseClock g_clock; // per thread: concurrent estimators (Replay::runMany, lock-step groups) each print their own
struct PhaseScope {
    int k;
    std::chrono::steady_clock::time_point t0;
    explicit PhaseScope(int k_) : k(k_), t0(std::chrono::steady_clock::now()) {}
    ~PhaseScope() {
        if (g_clock.on) {
            g_clock.ms[k] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            g_clock.calls[k]++;
        }
    }
};
enum { PH_EVAL_JAC = 0, PH_SCHUR, PH_HOST_FACTORS, PH_CHOLESKY, PH_BACKSUB, PH_EVAL_TRIAL, PH_COST, PH_CHI2 };

// One helper thread per process for WindowSolver::setHostFactorOverlap: whoever holds `owner` hands it the HOST half (the host factors of a
// linearization) and drives the device half itself — the calling thread is the one that talks to the device, always — anybody else runs the
// halves in turn.  The helper's phase clock (thread_local) is merged into the caller's after the join, so ICG_SOLVER_DEBUG books every phase.
std::atomic<bool> g_overlap{false};
struct OverlapHelper {
    std::mutex owner; // try_lock'ed by the solver that wants the helper
    SideThread thread;
};
OverlapHelper &overlapHelper() {
    static OverlapHelper h;
    return h;
}
// device() and host() both run, side by side when the overlap is on and the helper is free; -> both succeeded
bool runHalves(bool want_overlap, const std::function<bool()> &device, const std::function<bool()> &host) {
    if (want_overlap && g_overlap.load(std::memory_order_relaxed)) {
        OverlapHelper &h = overlapHelper();
        std::unique_lock<std::mutex> lock(h.owner, std::try_to_lock);
        if (lock.owns_lock()) {
            bool b = false;
            PhaseClock helper_clock;
            SideCall call(h.thread, [&] {
                g_clock = PhaseClock();
                try {
                    b = host();
                } catch (...) {
                    b = false;
                }
                helper_clock = g_clock;
            });
            const bool a = device(); // on the calling thread (an exception joins the helper first: `host` lives in the caller's frame)
            call.join();
            for (int k = 0; k < 8; k++) g_clock.ms[k] += helper_clock.ms[k], g_clock.calls[k] += helper_clock.calls[k];
            return a && b;
        }
    }
    const bool a = device();
    return host() && a;
}

using solver_detail::choleskySolve;
} // namespace

std::string solver_detail::Summary::BriefReport() const {
    char buf[256];
    snprintf(buf, sizeof buf, "WindowSolver: initial cost %.6e, final cost %.6e, %d successful / %d unsuccessful steps, %s", initial_cost,
             final_cost, num_successful_steps, num_unsuccessful_steps, termination.c_str());
    return buf;
}

void WindowSolver::setHostFactorOverlap(bool on) { g_overlap.store(on); }

WindowSolver::WindowSolver(ReprojectionBatch *visual, double huber_delta) : visual_(visual), huber_(huber_delta) {
    if (visual_) active_.assign((size_t) visual_->size(), 1);
}

void WindowSolver::addParameterBlock(double *values, int size, bool pose_manifold) { problem_.addParameterBlock(values, size, pose_manifold); }

void WindowSolver::setParameterBlockConstant(double *values) { problem_.setParameterBlockConstant(values); }

WindowSolver::ResidualBlockId WindowSolver::addResidualBlock(std::shared_ptr<ceres::CostFunction> cost, std::shared_ptr<ceres::LossFunction> loss,
                                                             const std::vector<double *> &blocks) {
    return problem_.addResidualBlock(std::move(cost), std::move(loss), blocks);
}

void WindowSolver::removeResidualBlock(ResidualBlockId id) { problem_.removeResidualBlock(id); }

bool WindowSolver::evaluateResidualBlock(ResidualBlockId id, bool apply_loss_function, double *cost) const {
    return problem_.evaluateResidualBlock(id, apply_loss_function, cost);
}

int WindowSolver::numActiveReprojectionFactors() const {
    int n = 0;
    for (uint8_t a : active_) n += a;
    return n;
}

// column layout of the reduced system (Problem::assignColumns); the inverse depths of the visual batch are eliminated on the device
// (column P + batch landmark index there)
bool WindowSolver::layout() {
    static const std::vector<double *> no_landmarks;
    const int P = problem_.assignColumns(visual_ ? visual_->lm_ptrs_ : no_landmarks, &error_);
    if (P < 0) return false;
    P_ = P;
    if (visual_) {
        col_pose_.resize(visual_->pose_ptrs_.size());
        for (size_t k = 0; k < col_pose_.size(); k++) col_pose_[k] = problem_.column(visual_->pose_ptrs_[k]);
        col_ext_ = visual_->ext_ ? problem_.column(visual_->ext_) : -1;
        col_td_  = visual_->td_ ? problem_.column(visual_->td_) : -1;
        if (active_.size() != (size_t) visual_->size()) active_.assign((size_t) visual_->size(), 1);
    }
    return P_ > 0;
}

bool WindowSolver::linearize(double damp, bool reassemble, const Options &o, std::vector<double> &S, std::vector<double> &s,
                             std::vector<double> &diag, double *cost) {
    S.assign((size_t) P_ * P_, 0.0);
    s.assign((size_t) P_, 0.0);
    diag.assign((size_t) P_, 0.0);
    double vc = 0, hc = 0;
    const bool has_visual = visual_ && visual_->size() > 0;
    std::string device_error;
    auto device = [&]() -> bool {
        if (!has_visual) return true;
        if (reassemble) {
            PhaseScope ps(PH_EVAL_JAC);
            if (!visual_->run(true, huber_, false)) {
                device_error = visual_->error();
                return false;
            }
        }
        PhaseScope ps(PH_SCHUR);
        if (icg_reproj_schur(visual_->ctx_, P_, col_pose_.data(), col_ext_, col_td_, active_.data(), reassemble ? 1 : 0, damp, o.min_lm_diagonal,
                             o.max_lm_diagonal, S.data(), s.data(), diag.data(), &vc) != ICG_OK) {
            device_error = icg_last_error(visual_->ctx_);
            return false;
        }
        return true;
    };
    auto host = [&]() -> bool {
        if (!reassemble) return true;
        host_S_.assign((size_t) P_ * P_, 0.0);
        host_s_.assign((size_t) P_, 0.0);
        host_diag_.assign((size_t) P_, 0.0);
        PhaseScope ps(PH_HOST_FACTORS);
        return solver_detail::hostFactors(problem_, P_, host_S_.data(), host_s_.data(), host_diag_.data(), &hc);
    };
    if (!runHalves(has_visual && reassemble && !problem_.residuals.empty(), device, host)) {
        error_ = device_error.empty() ? "a host cost function failed to evaluate" : device_error;
        return false;
    }
    if (reassemble && cost) *cost = vc + hc;
    for (size_t k = 0; k < S.size(); k++) S[k] += host_S_[k];
    for (size_t k = 0; k < s.size(); k++) s[k] += host_s_[k], diag[k] += host_diag_[k];
    return true;
}

bool WindowSolver::evaluateCost(double *cost) {
    double vc = 0, hc = 0;
    const bool has_visual = visual_ && visual_->size() > 0;
    std::string device_error;
    auto device = [&]() -> bool {
        if (!has_visual) return true;
        {
            PhaseScope ps(PH_EVAL_TRIAL);
            if (!visual_->run(false, huber_, false)) {
                device_error = visual_->error();
                return false;
            }
        }
        PhaseScope ps(PH_COST);
        if (icg_reproj_cost(visual_->ctx_, active_.data(), &vc) != ICG_OK) {
            device_error = icg_last_error(visual_->ctx_);
            return false;
        }
        return true;
    };
    auto host = [&]() -> bool { return solver_detail::hostFactors(problem_, P_, nullptr, nullptr, nullptr, &hc); };
    if (!runHalves(has_visual && !problem_.residuals.empty(), device, host)) {
        error_ = device_error.empty() ? "a host cost function failed to evaluate" : device_error;
        return false;
    }
    const double c = vc + hc;
    *cost = c;
    return true;
}

bool WindowSolver::solve(const Options &o, Summary *summary) {
    if (!layout()) {
        if (error_.empty()) error_ = "nothing to optimize";
        return false;
    }
    const size_t L = visual_ ? visual_->lm_ptrs_.size() : 0;
    solver_detail::TrustRegion tr(o);
    std::vector<double> S, s, diag, dd, delta_l(L, 0.0);
    if (!linearize(1.0 / tr.radius, true, o, S, s, diag, &tr.cost)) return false;
    tr.summary.initial_cost = tr.cost;
    bool need_redamp = false;
    for (int iter = 0; iter < o.max_num_iterations; iter++) {
        if (need_redamp && !linearize(1.0 / tr.radius, false, o, S, s, diag, nullptr)) return false;
        need_redamp = false;
        if (tr.gradientConverged(o, s)) break;
        // (S + D) delta_c = s with the LM diagonal of the camera block
        tr.damp(o, diag, P_, dd);
        std::vector<double> A(S), delta_c(s);
        for (int k = 0; k < P_; k++) A[(size_t) k * P_ + k] += dd[(size_t) k];
        bool ok;
        {
            PhaseScope ps(PH_CHOLESKY);
            ok = choleskySolve(P_, A, delta_c);
        }
        double lm_terms[2] = {0, 0};
        if (ok && L > 0) {
            PhaseScope psb(PH_BACKSUB);
            if (icg_reproj_backsub(visual_->ctx_, P_, delta_c.data(), delta_l.data(), lm_terms) != ICG_OK) {
                error_ = icg_last_error(visual_->ctx_);
                return false;
            }
        }
        const double model = ok ? solver_detail::TrustRegion::modelDecrease(lm_terms, delta_c, s, dd) : 0.0;
        if (!ok || !(model > 0.0)) {
            need_redamp = true;
            if (tr.reject(o)) break;
            continue;
        }
        if (tr.parameterConverged(o, problem_, delta_c, delta_l.data(), L)) break;
        problem_.backup();
        problem_.applyCameraStep(delta_c.data());
        for (size_t l = 0; l < L; l++) *visual_->lm_ptrs_[l] += delta_l[l];
        double new_cost = 0;
        if (!evaluateCost(&new_cost)) return false;
        bool accepted;
        if (tr.trial(o, new_cost, model, problem_, &accepted)) break;
        if (!accepted)
            need_redamp = true;
        else if (iter + 1 < o.max_num_iterations && !linearize(1.0 / tr.radius, true, o, S, s, diag, nullptr))
            return false;
    }
    tr.summary.final_cost = tr.cost;
    if (summary) *summary = tr.summary;
    if (g_clock.on) {
        static const char *names[8] = {"eval+jac", "schur", "host_factors", "cholesky", "backsub", "eval_trial", "cost", "chi2"};
        for (int k = 0; k < 8; k++)
            if (g_clock.calls[k]) fprintf(stderr, "[WindowSolver] %-28s %3d calls %8.3f ms\n", names[k], g_clock.calls[k], g_clock.ms[k]);
        g_clock = PhaseClock();
    }
    return true;
}

int WindowSolver::removeReprojectionFactorsByChi2(double chi2) {
    if (!visual_ || visual_->size() == 0) return 0;
    if (active_.size() != (size_t) visual_->size()) active_.assign((size_t) visual_->size(), 1);
    if (!visual_->run(false, 0.0)) { // EvaluateResidualBlock(id, false, &cost, ...): raw residuals, no loss
        error_ = visual_->error();
        return -1;
    }
    int removed = 0;
    for (int f = 0; f < visual_->size(); f++) {
        if (!active_[(size_t) f]) continue;
        const double *r = visual_->residual(f);
        const double cost = 0.5 * (r[0] * r[0] + r[1] * r[1]);
        if (cost * 2.0 > chi2) {
            active_[(size_t) f] = 0;
            removed++;
        }
    }
    return removed;
}

} // namespace icg
