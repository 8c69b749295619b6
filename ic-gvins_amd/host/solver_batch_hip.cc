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
#pragma weak icg_reproj_host_parts_build_prior
#pragma weak icg_reproj_host_parts_build_preint
#pragma weak icg_reproj_host_parts_build_preint_odo
#pragma weak icg_reproj_host_parts_build_nav

namespace icg {

// the first entry a family lacks in this build: one of its set's, or its host-part entry
template <class Set> static const char *missingFor(bool has_entry, const char *entry) { return !Set::available() ? Set::missingEntry() : has_entry ? nullptr : entry; }
const char *WindowSolverBatch::devicePreintegrationMissing() {
    return missingFor<PreintegrationSet>(&icg_reproj_host_parts_build_preint != nullptr, "icg_reproj_host_parts_build_preint");
}
const char *WindowSolverBatch::devicePreintegrationOdoMissing() {
    return missingFor<PreintegrationOdoSet>(&icg_reproj_host_parts_build_preint_odo != nullptr, "icg_reproj_host_parts_build_preint_odo");
}
const char *WindowSolverBatch::deviceNavFactorsMissing() { return missingFor<NavFactorSet>(&icg_reproj_host_parts_build_nav != nullptr, "icg_reproj_host_parts_build_nav"); }

bool WindowSolverBatch::devicePreintegrationAvailable() { return devicePreintegrationMissing() == nullptr; }

using solver_detail::choleskySolve;

bool WindowSolverBatch::deviceReducedSolveAvailable() {
    return &icg_chol_solve_batch != nullptr && &icg_reproj_schur_windows_resident != nullptr && &icg_reproj_solve_windows != nullptr;
}

bool WindowSolverBatch::deviceHostPartAvailable() { return &icg_reproj_host_parts_build != nullptr; }

bool WindowSolverBatch::devicePriorAvailable() { return &icg_reproj_host_parts_build_prior != nullptr && MarginalizationPriorSet::residentAvailable(); }

// What differs between the families of resident residuals; the table is rules(), behind Run.  A new family is an entry there, a value of Family, its set among
// the members and the case for its C entry in buildHostParts().
struct WindowSolverBatch::FamilyRules {
    bool WindowSolverBatch::*enabled; // its switch
    bool (*joins)(const solver_detail::Residual &R, int taken, std::string *err); // layout(): may R join, `taken` members being in its window already?  (*err set: no layout)
    const int *(*firstColumns)(const solver_detail::Residual &R); // per parameter block of a member, where its columns begin in the member's source matrix
    int64_t jac_from; // hostHalfOfWindow(): the jac_off of a resident block, ...
    bool once;        // ... at the window's first rebuild of a solve only (its Jacobian is kept afterwards) or at every one
    const char *entry;        // the narrowest host-part entry that serves it
    const char *(*missing)(); // optional: what a solve with members of the family lacks in this build, asked at its head
    bool (*set)(WindowSolverBatch &S, Run &R);                           // head of solve(): the members become resident
    void (*pack)(WindowSolverBatch &S, size_t k, double *const *blocks); // member k's evaluation point from its parameter blocks
    bool (*evaluate)(WindowSolverBatch &S, Run &R, bool want_jac);       // R.sq of the family, and whatever else the family does once it is evaluated
};

WindowSolverBatch::WindowSolverBatch(int device, double huber_delta, int host_threads)
    : factors_(device, host_threads, "WindowSolverBatch"), huber_(huber_delta) {}

WindowSolverBatch::~WindowSolverBatch() = default;

int WindowSolverBatch::addWindow() {
    windows_.emplace_back();
    finalized_ = false;
    return factors_.addWindow();
}

void WindowSolverBatch::clear() {
    windows_.clear();
    factors_.clear();
    active_.clear();
    col_pose_.clear(), col_ext_.clear(), col_td_.clear();
    P_         = 0;
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
    if (!factors_.add(w, factor->observation(), pose_i, pose_j, extrinsic, invdepth, td))
        throw std::runtime_error("WindowSolverBatch: one extrinsic / td block per window");
    finalized_ = false;
}

// uploads the factors of all windows (window-major) and the partition
bool WindowSolverBatch::finalize() {
    if (!factors_.upload(&error_)) return false;
    if (factors_.numFactors() == 0) return refuse("no reprojection factors");
    active_.assign((size_t) factors_.numFactors(), 1);
    finalized_ = true;
    return true;
}

bool WindowSolverBatch::prepare() {
    if (!finalized_ && !finalize()) return false;
    // device memory of the window systems and the staging memory of a step, for the layout as it stands now (solve() re-derives the layout)
    if (layout()) (void) icg_reproj_reserve_windows(factors_.ctx(), P_);
    error_.clear();
    return true;
}

bool WindowSolverBatch::layout() {
    P_ = 0;
    col_pose_.assign((size_t) factors_.numPoses(), -1);
    col_ext_.assign(windows_.size(), -1);
    col_td_.assign(windows_.size(), -1);
    // (a thousand hash look-ups per window: 1.3 ms for 256 windows on one thread, at the head of every solve — spread over the pool)
    std::vector<std::string> errs(windows_.size());
    factors_.forEachWindow(windows_.size(), [&](size_t w) {
        Window &W                        = windows_[w];
        const WindowFactorSet::Window &F = factors_.window(w);
        W.P                              = W.problem.assignColumns(F.landmarks, &errs[w]);
        if (W.P < 0) return;
        for (size_t k = 0; k < F.poses.size(); k++) col_pose_[(size_t) F.pose_begin + k] = W.problem.column(F.poses[k]);
        if (F.ext) col_ext_[w] = W.problem.column(F.ext);
        if (F.td) col_td_[w] = W.problem.column(F.td);
        if (!device_host_part_) return;
        // the blocks of the window's host part: their shapes and columns follow from the problem, not from an evaluation
        W.host_blocks.clear(), W.host_cols.clear();
        W.resident_of_residual.assign(W.problem.residuals.size(), {}), W.resident_of_block.clear();
        for (std::vector<int32_t> &c : W.resident_cols) c.clear();
        int count[kFamilies] = {}; // (the window's own: the set indices follow once all windows are laid out)
        std::vector<int> cols;
        for (size_t id = 0; id < W.problem.residuals.size(); id++) {
            const solver_detail::Residual &R = W.problem.residuals[id];
            if (R.removed) continue;
            Window::Resident &res = W.resident_of_residual[id];
            for (int f = 0; f < kFamilies && res.family == kNone && errs[w].empty(); f++) // the first family, of those switched on, whose rule takes the residual
                if (this->*rules(f).enabled && rules(f).joins(R, count[f], &errs[w])) res = {f, count[f]++};
            if (!errs[w].empty()) return;
            solver_detail::hostBlockColumns(W.problem, R, cols);
            if (cols.empty()) continue;
            W.resident_of_block.push_back(res);
            // a resident block's columns of its source matrix: the free local columns of its non-constant parameter blocks in block order, the
            // columns gatherHostBlock selects, counted from where the family's source matrix holds the block
            for (size_t a = 0; res.family != kNone && a < R.blocks.size(); a++) {
                const solver_detail::Block &A = W.problem.blocks[(size_t) W.problem.block_of.at(R.blocks[a])];
                if (A.column < 0) continue;
                const int first = rules(res.family).firstColumns(R)[a];
                for (int x = 0; x < A.local; x++) W.resident_cols[res.family].push_back(first + x);
            }
            W.host_blocks.push_back({(int) id, R.cost->num_residuals(), (int) cols.size(), 0, 0, 0});
            W.host_cols.insert(W.host_cols.end(), cols.begin(), cols.end());
        }
    });
    for (size_t w = 0; w < windows_.size(); w++) {
        if (!errs[w].empty()) return refuse(errs[w]);
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
        // the resident sets: the windows' priors in window order, the preintegration factors in window and residual order
        for (ResidentFamily &F : resident_) F.where.clear(), F.cols.clear(), F.of.assign(hp_nr_.size(), -1);
        for (size_t w = 0; w < windows_.size(); w++) {
            Window &W = windows_[w];
            int base[kFamilies];
            for (int f = 0; f < kFamilies; f++) base[f] = members(f);
            for (size_t id = 0; id < W.resident_of_residual.size(); id++) {
                Window::Resident &res = W.resident_of_residual[id];
                if (res.family == kNone) continue;
                res.index += base[res.family];
                resident_[res.family].where.push_back({(int) w, (int) id});
            }
            for (size_t k = 0; k < W.resident_of_block.size(); k++) {
                Window::Resident &res = W.resident_of_block[k];
                if (res.family != kNone) resident_[res.family].of[(size_t) W.blk_begin + k] = (res.index += base[res.family]);
            }
            for (int f = 0; f < kFamilies; f++) resident_[f].cols.insert(resident_[f].cols.end(), W.resident_cols[f].begin(), W.resident_cols[f].end());
        }
    }
    return P_ > 0;
}

namespace {
// ICG_SOLVER_DEBUG=1: wall time per phase of the lock-step loop
enum { PH_EVAL_JAC = 0, PH_SCHUR_TAIL, PH_HOST_LINEARIZE, PH_REDUCED_SOLVES, PH_BACKSUB, PH_MODEL_APPLY, PH_TRIAL_EVAL, PH_TRIAL_HOST, PH_HOST_PARTS, PH_COUNT };
struct BatchClock {
    bool on = getenv("ICG_SOLVER_DEBUG") != nullptr;
    double ms[PH_COUNT] = {};
    std::chrono::steady_clock::time_point t;
    void start() {
        if (on) t = std::chrono::steady_clock::now();
    }
    void stop(int k) {
        if (on) ms[k] += std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t).count();
    }
};
} // namespace

// What one solve() works on.  The reduced systems: their lower tiles are read where the reduction kernel writes them (pinned memory) and every
// window is factored by a host thread (dense_kernels.cc).  An earlier device form, since deleted (a workgroup per window, three barriers per
// column, every host part shipped per re-linearization), lost to this on MI355X, 256 C2 windows (P = 67), two solves: 26.5 ms against 21.1 ms.
// With setDeviceReducedSolve(true) the systems stay on the device instead and one wave per window solves them there without a barrier
// (icg_reproj_solve_windows, k_chol_solve), the thread pool only damping and deciding; DESIGN.md section 8 item 3 has the times of both.
struct WindowSolverBatch::Run {
    struct State {
        solver_detail::TrustRegion tr;
        double model;
        bool done, relinearize, redamp, stepped;
        int iters;
        std::vector<double> s, diag, delta_c, dd;
    };
    // device reduced solve: what one icg_reproj_solve_windows call takes and returns
    struct DeviceSolve {
        std::vector<int32_t> Pw, status;
        std::vector<uint8_t> solve_flag, part_new;
        std::vector<double> dd, rhs, parts;
        std::vector<size_t> part_off;
    };
    // device host part: the buffers of one icg_reproj_host_parts_build call (J and r of every block at the offsets of layout()), the
    // Jacobians as each block last shipped them in this solve, and what comes back
    struct DeviceParts {
        std::vector<double> J, r, shipped, s, diag;
        std::vector<int64_t> jac_off;
        std::vector<uint8_t> has_shipped;
    };

    const Options &o;
    const ReducedPath path;
    const size_t NW;
    const int P;
    std::vector<State> st;
    std::vector<double> poses, ext, inv, td, s, diag, cost, delta_c, delta_l, terms, damp;
    const double *S = nullptr; // W x P x P reduced systems, left in the context's pinned staging memory by the reduction kernel (valid until
                               // the next call on the context: consumed by the reduced solves, before the back-substitution call)
    std::vector<uint8_t> reassemble;
    std::vector<double> host_cost;
    DeviceSolve dev;
    DeviceParts hp;
    // per family of resident residuals: on for this solve (its switch is set and its set has members); r . r of every member at the last evaluated point
    bool on[kFamilies] = {}, any_on = false;
    std::vector<double> sq[kFamilies]; // (a navigation factor with a loss: rho[0] of its r . r, what its place in the host cost takes)
    // navigation factors: the members that carry a loss and, at a linearization, their three corrector scalars
    std::vector<uint8_t> nav_robust;
    std::vector<const ceres::LossFunction *> nav_loss;
    std::vector<double> nav_corr;
    bool any_nav_robust = false;
    std::vector<std::vector<double>> res_cost; // deferred(): the cost of every residual of every window as the pool recorded it (a resident one's comes from sq)
    std::vector<uint8_t> gathered;             // the windows whose prior Jacobian was gathered on the device in this solve
    std::string resident_err;                  // what the evaluation of a family failed with (side thread: error_ takes it after the join)
    bool deferred() const { return any_on; } // a device value takes a residual's place in the host cost: the pool records per residual
    bool first = true;                                        // no window has its initial cost yet
    bool all_done = false, any_step = false, any_trial = false; // what solve() decides on after a phase
    BatchClock clk;

    Run(const Options &options, ReducedPath reduced_path, size_t n_windows, int columns, int n_lm)
        : o(options), path(reduced_path), NW(n_windows), P(columns),
          st(NW, State{solver_detail::TrustRegion(o), 0, false, true, false, false, 0, {}, {}, {}, {}}), s(NW * P), diag(NW * P), cost(NW),
          delta_c(NW * P), delta_l((size_t) n_lm), terms(2 * NW), damp(NW), reassemble(NW), host_cost(NW, 0.0) {}
    bool deviceSolve() const { return path != ReducedPath::HostSolve; }
    bool deviceParts() const { return path == ReducedPath::DeviceSolveDeviceParts; }
};

// ---- the families, each described once ----------------------------------------------------------------------------------------------------
using solver_detail::Residual;
static const MargPriorView &viewOf(const Residual &R) { return dynamic_cast<const MargPriorSource *>(R.cost.get())->margPriorView(); }
template <class Factor> static bool readyFactor(const Residual &R, int, std::string *) { // a preintegration factor of either kind: no loss, integrated and whitened
    const auto *f = R.loss ? nullptr : dynamic_cast<const Factor *>(R.cost.get());
    return f && f->preintegration().ready() && R.blocks.size() == 4;
}
template <class Factor> static auto integrationOf(const Residual &M) { return &static_cast<const Factor *>(M.cost.get())->preintegration(); }
template <int... first> constexpr int kFirstColumns[] = {first...}; // (of a family whose members' blocks begin at the same columns of their source matrices)

const WindowSolverBatch::FamilyRules &WindowSolverBatch::rules(int family) {
    typedef WindowSolverBatch S;
    static const auto listOf = [](const S &s, int f, auto get) { // the member list a set takes
        std::vector<decltype(get(s.member(f, 0)))> list;
        for (size_t k = 0; k < (size_t) s.members(f); k++) list.push_back(get(s.member(f, k)));
        return list;
    };
    static const FamilyRules table[kFamilies] = {
        // Marginalization priors: the window's first prior without a loss (a robustified or a second prior stays on the pool).  Source matrix: J0, shipped by set().
        {&S::device_prior_,
         [](const Residual &R, int taken, std::string *err) {
             if (taken || R.loss || !dynamic_cast<const MargPriorSource *>(R.cost.get())) return false;
             const MargPriorView &v = viewOf(R);
             const auto &sizes      = R.cost->parameter_block_sizes();
             if (v.r == R.cost->num_residuals() && v.n_blocks == (int) sizes.size() && std::equal(sizes.begin(), sizes.end(), v.size)) return true;
             *err = "a marginalization prior's view does not describe its residual block";
             return false;
         },
         [](const Residual &R) -> const int * { return viewOf(R).index; }, ICG_HP_JAC_FROM_PRIOR, true, "icg_reproj_host_parts_build_prior", nullptr,
         [](S &s, Run &R) { return R.gathered.assign(R.NW, 0), s.prior_set_.set(s.factors_.ctx(), listOf(s, kPrior, [](const Residual &M) { return viewOf(M); }), &s.error_); },
         [](S &s, size_t k, double *const *blocks) { s.prior_set_.pack(k, blocks); },
         [](S &s, Run &R, bool) { return s.prior_set_.evaluateResident(R.sq[kPrior].data(), &R.resident_err); }},
        // Preintegration factors.  Source matrix: the whitened 15 x 32 Jacobian (7 | 9 | 7 | 9).
        {&S::device_preint_, readyFactor<PreintegrationFactor>, [](const Residual &) -> const int * { return kFirstColumns<0, 7, 16, 23>; }, ICG_HP_JAC_FROM_PREINT, false, "icg_reproj_host_parts_build_preint", nullptr,
         [](S &s, Run &) { return s.preint_set_.set(s.factors_.ctx(), listOf(s, kPreint, integrationOf<PreintegrationFactor>), &s.error_); },
         [](S &s, size_t k, double *const *blocks) { s.preint_set_.pack(k, blocks); },
         [](S &s, Run &R, bool want_jac) { return s.preint_set_.evaluateResident(want_jac, R.sq[kPreint].data(), &R.resident_err); }},
        // The odometer variants behind the same switch, in a set of their own: 19 x 34 (7 | 10 | 7 | 10).  A solve that holds such a factor needs their entries.
        {&S::device_preint_, readyFactor<PreintegrationOdoFactor>, [](const Residual &) -> const int * { return kFirstColumns<0, 7, 17, 24>; },
         ICG_HP_JAC_FROM_PREINT_ODO, false, "icg_reproj_host_parts_build_preint_odo", &S::devicePreintegrationOdoMissing,
         [](S &s, Run &) { return s.preint_odo_set_.set(s.factors_.ctx(), listOf(s, kPreintOdo, integrationOf<PreintegrationOdoFactor>), &s.error_); },
         [](S &s, size_t k, double *const *blocks) { s.preint_odo_set_.pack(k, blocks); },
         [](S &s, Run &R, bool want_jac) { return s.preint_odo_set_.evaluateResident(want_jac, R.sq[kPreintOdo].data(), &R.resident_err); }},
        // Navigation factors: one parameter block of the factor's own width, which is its source matrix's; a loss is allowed.
        {&S::device_nav_,
         [](const Residual &R, int, std::string *) {
             const auto *nf = dynamic_cast<const NavFactor *>(R.cost.get());
             return nf && R.blocks.size() == 1 && R.cost->parameter_block_sizes().size() == 1 && R.cost->parameter_block_sizes()[0] == nf->navWidth() &&
                    R.cost->num_residuals() == nf->navResiduals();
         },
         [](const Residual &) -> const int * { return kFirstColumns<0>; }, ICG_HP_JAC_FROM_NAV, false, "icg_reproj_host_parts_build_nav", nullptr,
         [](S &s, Run &R) { // the members with a loss are marked for the corrector
             const size_t n = (size_t) s.members(kNav);
             R.nav_robust.assign(n, 0), R.nav_loss.assign(n, nullptr), R.nav_corr.assign(3 * n, 0.0);
             for (size_t k = 0; k < n; k++) R.nav_loss[k] = s.member(kNav, k).loss.get(), R.nav_robust[k] = R.nav_loss[k] ? 1 : 0, R.any_nav_robust |= R.nav_loss[k] != nullptr;
             return s.nav_set_.set(s.factors_.ctx(), listOf(s, kNav, [](const Residual &M) { return dynamic_cast<const NavFactor *>(M.cost.get()); }), &s.error_);
         },
         [](S &s, size_t k, double *const *blocks) { s.nav_set_.pack(k, blocks[0]); },
         [](S &s, Run &R, bool want_jac) {
             // A member with a loss: rho on the host from its squared norm; rho[0] takes its place in the cost, and at a linearization the corrector's
             // scalars go up for one correction of what the evaluation kept
             std::vector<double> &sq = R.sq[kNav];
             if (!s.nav_set_.evaluateResident(want_jac, sq.data(), &R.resident_err)) return false;
             for (size_t k = 0; R.any_nav_robust && k < sq.size(); k++) {
                 if (!R.nav_loss[k]) continue;
                 double rho[3];
                 R.nav_loss[k]->Evaluate(sq[k], rho);
                 if (want_jac) {
                     const CorrectorScalars cs = correctorScalars(sq[k], rho);
                     R.nav_corr[3 * k] = cs.sqrt_rho1, R.nav_corr[3 * k + 1] = cs.alpha_sq_norm, R.nav_corr[3 * k + 2] = cs.residual_scaling;
                 }
                 sq[k] = rho[0];
             }
             return !(want_jac && R.any_nav_robust) || s.nav_set_.correct(R.nav_robust.data(), R.nav_corr.data(), &R.resident_err);
         }}};
    return table[family];
}

bool WindowSolverBatch::fail(const char *what) {
    error_ = std::string(what) + ": " + icg_last_error(factors_.ctx());
    return false;
}

bool WindowSolverBatch::resolvePath(ReducedPath *path) {
    if (device_reduced_ && !deviceReducedSolveAvailable()) return refuse("icg_reproj_solve_windows is not in this build");
    if (device_host_part_ && !deviceHostPartAvailable()) return refuse("icg_reproj_host_parts_build is not in this build");
    if (device_host_part_ && !device_reduced_)
        return refuse("setDeviceHostPart(true) needs setDeviceReducedSolve(true): the host parts are built where the device solve reads them");
    if (device_prior_ && !devicePriorAvailable())
        return refuse(std::string(MarginalizationPriorSet::residentAvailable() ? "icg_reproj_host_parts_build_prior" : "icg_marg_prior_evaluate_resident") + " is not in this build");
    if (device_prior_ && !device_host_part_)
        return refuse("setDevicePrior(true) needs setDeviceHostPart(true): the resident prior is read where the host parts are built");
    if (device_preint_ && !devicePreintegrationAvailable()) return refuse(std::string(devicePreintegrationMissing()) + " is not in this build");
    if (device_preint_ && !device_host_part_)
        return refuse("setDevicePreintegration(true) needs setDeviceHostPart(true): the resident factors are read where the host parts are built");
    if (device_nav_ && !device_host_part_)
        return refuse("setDeviceNavFactors(true) needs setDeviceHostPart(true): the resident factors are read where the host parts are built");
    if (device_nav_ && deviceNavFactorsMissing()) return refuse(std::string(deviceNavFactorsMissing()) + " is not in this build");
    *path = device_host_part_ ? ReducedPath::DeviceSolveDeviceParts : device_reduced_ ? ReducedPath::DeviceSolve : ReducedPath::HostSolve;
    return true;
}

bool WindowSolverBatch::solve(const Options &o, std::vector<Summary> *summaries) {
    const auto t_solve = std::chrono::steady_clock::now();
    if (!finalized_ && !finalize()) return false;
    if (!layout()) {
        if (error_.empty()) error_ = "nothing to optimize";
        return false;
    }
    ReducedPath path;
    if (!resolvePath(&path)) return false;
    const size_t NW = windows_.size();
    Run R(o, path, NW, P_, factors_.numLandmarks());
    if (R.deviceSolve()) {
        Run::DeviceSolve &D = R.dev;
        D.Pw.resize(NW), D.status.resize(NW), D.solve_flag.resize(NW), D.part_new.resize(NW), D.part_off.resize(NW + 1);
        D.dd.resize(NW * R.P), D.rhs.resize(NW * R.P);
        for (size_t w = 0; w < NW; w++) D.Pw[w] = windows_[w].P, windows_[w].host_part_dirty = false;
    }
    if (R.deviceParts()) {
        Run::DeviceParts &H = R.hp;
        H.J.resize(hp_J_total_), H.shipped.resize(hp_J_total_), H.r.assign(hp_r_total_, 0.0);
        H.jac_off.assign(hp_nr_.size(), 0), H.has_shipped.assign(hp_nr_.size(), 0);
        H.s.assign(NW * R.P, 0.0), H.diag.assign(NW * R.P, 0.0);
    }
    for (int f = 0; f < kFamilies; f++) { // a family that is switched on and has members becomes resident once per solve; a build without its entries refuses by name
        const FamilyRules &F = rules(f);
        if (!(this->*F.enabled) || members(f) == 0) continue;
        if (F.missing && F.missing()) return refuse(std::string(F.missing()) + " is not in this build");
        if (!F.set(*this, R)) return false;
        R.on[f] = R.any_on = true, R.sq[f].assign((size_t) members(f), 0.0);
    }
    if (R.deferred()) {
        R.res_cost.resize(NW);
        for (size_t w = 0; w < NW; w++) R.res_cost[w].assign(windows_[w].problem.residuals.size(), 0.0);
    }
    for (;;) {
        if (!linearize(R) || !reducedSolves(R)) return false;
        if (R.all_done) break;
        if (!R.any_step) continue; // only re-damping this round
        if (!trialPoints(R)) return false;
        if (!R.any_trial) continue;
        if (!trialCosts(R)) return false;
    }
    const BatchClock &clk = R.clk;
    if (clk.on)
        fprintf(stderr, "[WindowSolverBatch] %zu windows: eval+jac %.2f, schur beyond the host half %.2f, host linearize (beside the device call) %.2f, reduced solves %.2f, backsub %.2f, model+apply %.2f, "
                        "trial eval+cost %.2f, trial host %.2f, host parts on the device %.2f ms; whole solve %.2f ms\n",
                NW, clk.ms[PH_EVAL_JAC], clk.ms[PH_SCHUR_TAIL], clk.ms[PH_HOST_LINEARIZE], clk.ms[PH_REDUCED_SOLVES], clk.ms[PH_BACKSUB], clk.ms[PH_MODEL_APPLY],
                clk.ms[PH_TRIAL_EVAL], clk.ms[PH_TRIAL_HOST], clk.ms[PH_HOST_PARTS],
                std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t_solve).count());
    if (summaries) {
        summaries->resize(NW);
        for (size_t w = 0; w < NW; w++) (*summaries)[w] = R.st[w].tr.summary, (*summaries)[w].final_cost = R.st[w].tr.cost;
    }
    return true;
}

// ---- (re)linearize / re-damp ------------------------------------------------------------------------------------------------------------
bool WindowSolverBatch::linearize(Run &R) {
    const size_t NW  = R.NW;
    const int P      = R.P;
    const Options &o = R.o;
    icg_ctx *ctx     = factors_.ctx();
    bool any_lin = false, any_sys = false;
    for (size_t w = 0; w < NW; w++) {
        R.reassemble[w] = (!R.st[w].done && R.st[w].relinearize) ? 1 : 0;
        R.damp[w]       = 1.0 / R.st[w].tr.radius;
        any_lin |= R.reassemble[w] != 0;
        any_sys |= !R.st[w].done && (R.st[w].relinearize || R.st[w].redamp);
    }
    if (any_lin) {
        R.clk.start();
        factors_.gather(R.poses, R.ext, R.inv, R.td);
        if (icg_reproj_eval_windows(ctx, factors_.numPoses(), R.poses.data(), R.ext.data(), factors_.numLandmarks(), R.inv.data(), R.td.data(), 1, huber_) !=
            ICG_OK)
            return fail("icg_reproj_eval_windows");
        R.clk.stop(PH_EVAL_JAC);
    }
    if (any_sys) {
        // The device half (assembly + landmark elimination of every window: one call) and the host half (the host-evaluated factors of
        // every window that is re-linearized: priors, preintegration, marginalization prior — on the pool) do not depend on each other:
        // the call runs on a helper thread while this one drives the pool (what WindowSolver::linearize does per window with
        // runHalves); the sums that need both are formed after the join.
        R.clk.start();
        int dev_rc = ICG_OK;
        bool resident_ok = true;
        if (any_lin) packResident(R);
        if (!side_) side_.reset(new SideThread());
        SideCall dev(*side_, [&] {
            if (R.deviceSolve()) {
                dev_rc = icg_reproj_schur_windows_resident(ctx, P, col_pose_.data(), col_ext_.data(), col_td_.data(), active_.data(), R.reassemble.data(),
                                                           R.damp.data(), o.min_lm_diagonal, o.max_lm_diagonal, R.s.data(), R.diag.data(), R.cost.data());
                if (dev_rc == ICG_OK && any_lin) resident_ok = evaluateResident(R, true);
            } else
                dev_rc = icg_reproj_schur_windows_view(ctx, P, col_pose_.data(), col_ext_.data(), col_td_.data(), active_.data(), R.reassemble.data(),
                                                       R.damp.data(), o.min_lm_diagonal, o.max_lm_diagonal, &R.S, R.s.data(), R.diag.data(), R.cost.data());
        });
        std::atomic<int> host_failed{0};
        R.host_cost.assign(NW, 0.0);
        factors_.forEachWindow(NW, [&](size_t w) {
            if (R.st[w].done || !R.st[w].relinearize) return;
            if (!hostHalfOfWindow(R, w)) host_failed++;
        });
        R.clk.stop(PH_HOST_LINEARIZE);
        R.clk.start();
        dev.join();
        R.clk.stop(PH_SCHUR_TAIL); // (what is left of the device call once the host half is through)
        if (dev_rc != ICG_OK) return fail(R.deviceSolve() ? "icg_reproj_schur_windows_resident" : "icg_reproj_schur_windows_view");
        if (!resident_ok) return refuse(R.resident_err);
        if (host_failed.load()) return refuse("a host cost function failed to evaluate");
        if (R.deviceParts() && any_lin) {
            // the parts of the re-linearized windows, built in their slots on the device; s and diag of those windows come back
            R.clk.start();
            if (!buildHostParts(R)) return false;
            R.clk.stop(PH_HOST_PARTS);
        }
        R.clk.start();
        factors_.forEachWindow(NW, [&](size_t w) {
            Run::State &T = R.st[w];
            if (T.done || !(T.relinearize || T.redamp)) return;
            Window &W = windows_[w];
            if (R.deferred() && T.relinearize) sumHostCosts(R, w); // (the device values have arrived)
            // the cost at the linearization point initialises the window on the first pass; afterwards it equals the accepted
            // trial cost and is kept (the same bookkeeping as WindowSolver)
            if (T.relinearize && R.first) T.tr.cost = R.cost[w] + R.host_cost[w], T.tr.summary.initial_cost = T.tr.cost;
            // the window's reduced system is used where it arrived (S, s, diag of the batched call) plus the host factors' part: no
            // per-window copy of the P x P block (9 MB per step at 256 windows)
            T.s.resize((size_t) P), T.diag.resize((size_t) P);
            const double *hs = R.deviceParts() ? &R.hp.s[w * P] : W.host_s.data(), *hd = R.deviceParts() ? &R.hp.diag[w * P] : W.host_diag.data();
            for (int k = 0; k < P; k++) {
                T.s[(size_t) k]    = R.s[w * P + (size_t) k] + hs[(size_t) k];
                T.diag[(size_t) k] = R.diag[w * P + (size_t) k] + hd[(size_t) k];
            }
            T.relinearize = T.redamp = false;
        });
        R.clk.stop(PH_HOST_LINEARIZE);
    }
    R.first = false;
    return true;
}

// the host-evaluated factors of a re-linearized window (on a pool thread, beside the device call); false: one failed to evaluate
bool WindowSolverBatch::hostHalfOfWindow(Run &R, size_t w) {
    Window &W = windows_[w];
    switch (R.path) {
    case ReducedPath::HostSolve:
    case ReducedPath::DeviceSolve: {
        const int P = R.P;
        W.host_S.assign((size_t) P * P, 0.0), W.host_s.assign((size_t) P, 0.0), W.host_diag.assign((size_t) P, 0.0);
        const bool ok     = solver_detail::hostFactors(W.problem, P, W.host_S.data(), W.host_s.data(), W.host_diag.data(), &R.host_cost[w]);
        W.host_part_dirty = true;
        return ok;
    }
    case ReducedPath::DeviceSolveDeviceParts: {
        // evaluate and gather only: every block's Jd and res at its place in the call buffers, the cost in residual order
        Run::DeviceParts &H = R.hp;
        thread_local std::vector<int> cols;
        thread_local std::vector<double> none;
        size_t next = 0;
        for (size_t id = 0; id < W.problem.residuals.size(); id++) {
            const solver_detail::Residual &Res = W.problem.residuals[id];
            if (Res.removed) continue;
            const bool has = next < W.host_blocks.size() && W.host_blocks[next].residual == (int) id;
            double *cost   = &R.host_cost[w];
            if (R.deferred()) cost = &R.res_cost[w][id], *cost = 0.0; // per residual: the window's sum waits for the device values
            if (const int family = W.resident_of_residual[id].family; family != kNone) {
                // evaluated where it is resident: placed only.  A prior's Jacobian is gathered from J0 at the window's first rebuild of the solve and kept, a factor's at every rebuild
                if (has) H.jac_off[(size_t) W.blk_begin + next++] = rules(family).once && R.gathered[w] ? -1 : rules(family).jac_from;
                continue;
            }
            double *Jd = has ? &H.J[W.host_blocks[next].J_off] : nullptr;
            if (solver_detail::gatherHostBlock(W.problem, Res, cost, cols, none, none, Jd, has ? &H.r[W.host_blocks[next].r_off] : nullptr) < 0)
                return false;
            if (!has) continue;
            // the same Jacobian as at the window's previous rebuild stays where it is on the device
            const Window::HostBlock &B = W.host_blocks[next];
            const size_t b = (size_t) W.blk_begin + next, bytes = sizeof(double) * (size_t) B.nr * B.nf;
            if (H.has_shipped[b] && memcmp(Jd, &H.shipped[B.J_off], bytes) == 0) {
                H.jac_off[b] = -1;
            } else {
                H.jac_off[b] = (int64_t) B.J_off;
                memcpy(&H.shipped[B.J_off], Jd, bytes);
                H.has_shipped[b] = 1;
            }
            next++;
        }
        return true;
    }
    }
    return false;
}

// resident residuals: every member's parameter blocks at their places in its set's evaluation point (a preintegration factor's with its correction
// quaternion), on the driving thread before the phase's device call
void WindowSolverBatch::packResident(const Run &R) {
    for (int f = 0; f < kFamilies; f++)
        for (size_t k = 0; R.on[f] && k < (size_t) members(f); k++) rules(f).pack(*this, k, member(f, k).blocks.data());
}

// the resident evaluation of a phase (side thread), one squared norm per member: family after family until one fails, with Jacobians at a
// linearization and the residual only at a trial point (the cost is all it needs)
bool WindowSolverBatch::evaluateResident(Run &R, bool want_jac) {
    for (int f = 0; f < kFamilies; f++)
        if (R.on[f] && !rules(f).evaluate(*this, R, want_jac)) return false;
    return true;
}

// The host-part call of a linearization, by the narrowest entry that serves the families that are on (a C ABI without the wider ones keeps working with the
// narrower switches).  The resident blocks take their residuals where they are, and their Jacobians at every rebuild (factors) or a window's first (priors).
bool WindowSolverBatch::buildHostParts(Run &R) {
    Run::DeviceParts &H     = R.hp;
    int widest = kNone; // the last family that is on
    const int32_t *of[kFamilies] = {}, *cols[kFamilies] = {};
    for (int f = 0; f < kFamilies; f++)
        if (R.on[f]) of[f] = resident_[f].of.data(), cols[f] = resident_[f].cols.data(), widest = f;
    auto call = [&](auto entry, auto... resident) { // (every entry takes the narrowest one's arguments first)
        return entry(factors_.ctx(), R.P, R.dev.Pw.data(), R.reassemble.data(), hp_blk_off_.data(), hp_nr_.data(), hp_nf_.data(), hp_cols_.data(), H.jac_off.data(),
                     H.J.data(), H.r.data(), H.s.data(), H.diag.data(), nullptr, resident...);
    };
    int rc;
    switch (widest) { // (the one place outside rules() that names the families: the entries' signatures differ)
    case kNav: rc = call(icg_reproj_host_parts_build_nav, of[kPrior], cols[kPrior], of[kPreint], cols[kPreint], of[kPreintOdo], cols[kPreintOdo], of[kNav], cols[kNav]); break;
    case kPreintOdo: rc = call(icg_reproj_host_parts_build_preint_odo, of[kPrior], cols[kPrior], of[kPreint], cols[kPreint], of[kPreintOdo], cols[kPreintOdo]); break;
    case kPreint: rc = call(icg_reproj_host_parts_build_preint, of[kPrior], cols[kPrior], of[kPreint], cols[kPreint]); break;
    case kPrior: rc = call(icg_reproj_host_parts_build_prior, of[kPrior], cols[kPrior]); break;
    default: rc = call(icg_reproj_host_parts_build);
    }
    if (rc != ICG_OK) return fail(widest == kNone ? "icg_reproj_host_parts_build" : rules(widest).entry);
    for (size_t w = 0; w < R.gathered.size(); w++) R.gathered[w] |= R.reassemble[w]; // (sized by a family whose Jacobians are kept from a window's first rebuild)
    return true;
}

// the window's host cost from the costs the pool recorded per residual and half the device's squared norm in a resident residual's place,
// added up from zero in residual order: hostFactors' sum
void WindowSolverBatch::sumHostCosts(Run &R, size_t w) {
    const Window &W = windows_[w];
    double cost     = 0.0;
    for (size_t id = 0; id < W.problem.residuals.size(); id++) {
        if (W.problem.residuals[id].removed) continue;
        const Window::Resident &res = W.resident_of_residual[id];
        cost += res.family != kNone ? 0.5 * R.sq[res.family][(size_t) res.index] : R.res_cost[w][id];
    }
    R.host_cost[w] = cost;
}

// ---- every open window: iteration budget, gradient test, reduced solve --------------------------------------------------------------------
bool WindowSolverBatch::reducedSolves(Run &R) {
    const size_t NW  = R.NW;
    const int P      = R.P;
    const Options &o = R.o;
    R.clk.start();
    std::fill(R.delta_c.begin(), R.delta_c.end(), 0.0);
    factors_.forEachWindow(NW, [&](size_t w) {
        Run::State &T = R.st[w];
        T.stepped     = false;
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
        T.tr.damp(o, T.diag, windows_[w].P, T.dd); // columns beyond the window's P are empty (zero rows): the leading block only
        switch (R.path) {
        case ReducedPath::HostSolve: solveWindowOnHost(R, w); break;
        case ReducedPath::DeviceSolve:
        case ReducedPath::DeviceSolveDeviceParts: // the solve itself follows for all windows at once
            std::copy(T.dd.begin(), T.dd.end(), R.dev.dd.begin() + (long) (w * P));
            std::copy(T.s.begin(), T.s.end(), R.dev.rhs.begin() + (long) (w * P));
            T.stepped = true;
            break;
        }
    });
    if (R.deviceSolve() && !solveWindowsOnDevice(R)) return false;
    R.any_step = false, R.all_done = true;
    for (size_t w = 0; w < NW; w++) R.any_step |= R.st[w].stepped, R.all_done &= R.st[w].done;
    R.clk.stop(PH_REDUCED_SOLVES);
    return true;
}

// the damped system of window w from the view plus its host part, factored on this (pool) thread
void WindowSolverBatch::solveWindowOnHost(Run &R, size_t w) {
    Run::State &T = R.st[w];
    const int P = R.P, Pw = windows_[w].P;
    std::vector<double> Ab((size_t) Pw * Pw), bb(T.s.begin(), T.s.begin() + Pw);
    const double *Sw = &R.S[w * (size_t) P * P], *Hw = windows_[w].host_S.data();
    for (int i = 0; i < Pw; i++) // lower triangle: what the view holds and what choleskySolve reads
        for (int j = 0; j <= i; j++) Ab[(size_t) i * Pw + j] = Sw[(size_t) i * P + j] + Hw[(size_t) i * P + j];
    for (int k = 0; k < Pw; k++) Ab[(size_t) k * Pw + k] += T.dd[(size_t) k];
    if (!choleskySolve(Pw, Ab, bb)) {
        T.redamp = true;
        T.done   = T.tr.reject(R.o);
        return;
    }
    T.delta_c.assign((size_t) P, 0.0);
    std::copy(bb.begin(), bb.end(), T.delta_c.begin());
    std::copy(T.delta_c.begin(), T.delta_c.end(), R.delta_c.begin() + (long) (w * P));
    T.stepped = true;
}

// every window that was staged: one call solves them where their systems are and back-substitutes (delta_l, terms)
bool WindowSolverBatch::solveWindowsOnDevice(Run &R) {
    const size_t NW     = R.NW;
    const int P         = R.P;
    Run::DeviceSolve &D = R.dev;
    // the windows that solve in this step, and of those the host parts a re-linearization rebuilt since they were last shipped
    bool any     = false;
    size_t total = 0;
    for (size_t w = 0; w < NW; w++) {
        D.solve_flag[w] = R.st[w].stepped ? 1 : 0;
        D.part_new[w]   = R.st[w].stepped && windows_[w].host_part_dirty ? 1 : 0;
        D.part_off[w]   = total;
        if (D.part_new[w]) total += (size_t) D.Pw[w] * ((size_t) D.Pw[w] + 1) / 2;
        any |= R.st[w].stepped;
    }
    D.part_off[NW] = total;
    D.parts.resize(total);
    factors_.forEachWindow(NW, [&](size_t w) {
        if (!D.part_new[w]) return;
        const double *Hw = windows_[w].host_S.data();
        double *dst      = D.parts.data() + D.part_off[w];
        for (int i = 0; i < D.Pw[w]; i++, dst += i) memcpy(dst, Hw + (size_t) i * P, sizeof(double) * ((size_t) i + 1));
    });
    if (!any) return true;
    if (icg_reproj_solve_windows(factors_.ctx(), P, D.Pw.data(), D.solve_flag.data(), R.deviceParts() ? nullptr : D.part_new.data(),
                                 D.parts.empty() ? nullptr : D.parts.data(), D.dd.data(), D.rhs.data(), R.delta_c.data(), D.status.data(),
                                 R.delta_l.data(), R.terms.data()) != ICG_OK)
        return fail("icg_reproj_solve_windows");
    for (size_t w = 0; w < NW; w++) {
        Run::State &T = R.st[w];
        if (!T.stepped) continue;
        windows_[w].host_part_dirty = false;
        if (D.status[w] != 0) {
            T.stepped = false, T.redamp = true;
            T.done = T.tr.reject(R.o);
            continue;
        }
        T.delta_c.assign(R.delta_c.begin() + (long) (w * P), R.delta_c.begin() + (long) ((w + 1) * P));
    }
    return true;
}

// ---- landmark back-substitution for all windows, model decrease, trial points -------------------------------------------------------------
bool WindowSolverBatch::trialPoints(Run &R) {
    const size_t NW = R.NW;
    R.clk.start();
    if (!R.deviceSolve() && factors_.numLandmarks() > 0 &&
        icg_reproj_backsub_windows(factors_.ctx(), R.P, R.delta_c.data(), R.delta_l.data(), R.terms.data()) != ICG_OK)
        return fail("icg_reproj_backsub_windows");
    R.clk.stop(PH_BACKSUB);
    R.clk.start();
    factors_.forEachWindow(NW, [&](size_t w) {
        Run::State &T = R.st[w];
        if (!T.stepped) return;
        Window &W                        = windows_[w];
        const WindowFactorSet::Window &F = factors_.window(w);
        T.model                          = solver_detail::TrustRegion::modelDecrease(&R.terms[2 * w], T.delta_c, T.s, T.dd);
        if (!(T.model > 0.0)) {
            T.redamp = true, T.stepped = false;
            T.done   = T.tr.reject(R.o);
            return;
        }
        if (T.tr.parameterConverged(R.o, W.problem, T.delta_c, R.delta_l.data() + F.lm_begin, F.landmarks.size())) {
            T.done = true, T.stepped = false;
            return;
        }
        W.problem.backup();
        W.problem.applyCameraStep(T.delta_c.data());
        for (size_t k = 0; k < F.landmarks.size(); k++) *F.landmarks[k] += R.delta_l[(size_t) F.lm_begin + k];
    });
    R.any_trial = false;
    for (size_t w = 0; w < NW; w++) R.any_trial |= R.st[w].stepped;
    R.clk.stop(PH_MODEL_APPLY);
    return true;
}

// ---- the trial costs: the visual factors' on the device (evaluation + cost reduction, one call each) beside the host factors' on the pool;
// accept / reject per window ---------------------------------------------------------------------------------------------------------------
bool WindowSolverBatch::trialCosts(Run &R) {
    const size_t NW = R.NW;
    icg_ctx *ctx    = factors_.ctx();
    R.clk.start();
    factors_.gather(R.poses, R.ext, R.inv, R.td);
    const char *dev_fail = nullptr;
    bool resident_ok = true;
    packResident(R);
    if (!side_) side_.reset(new SideThread());
    SideCall trial(*side_, [&] {
        if (icg_reproj_eval_windows(ctx, factors_.numPoses(), R.poses.data(), R.ext.data(), factors_.numLandmarks(), R.inv.data(), R.td.data(), 0, huber_) !=
            ICG_OK)
            dev_fail = "icg_reproj_eval_windows";
        else if (icg_reproj_cost_windows(ctx, active_.data(), R.cost.data()) != ICG_OK)
            dev_fail = "icg_reproj_cost_windows";
        else
            resident_ok = evaluateResident(R, false);
    });
    std::atomic<int> trial_failed{0};
    R.host_cost.assign(NW, 0.0);
    factors_.forEachWindow(NW, [&](size_t w) {
        if (!R.st[w].stepped) return;
        if (!R.deferred()) {
            if (!solver_detail::hostFactors(windows_[w].problem, R.P, nullptr, nullptr, nullptr, &R.host_cost[w])) trial_failed++;
            return;
        }
        // the cost-only pass of hostFactors per residual, the resident ones left to the device
        const Window &W = windows_[w];
        for (size_t id = 0; id < W.problem.residuals.size(); id++) {
            const solver_detail::Residual &Res = W.problem.residuals[id];
            if (Res.removed || W.resident_of_residual[id].family != kNone) continue;
            if (!solver_detail::residualCost(Res, true, &R.res_cost[w][id])) {
                trial_failed++;
                return;
            }
        }
    });
    trial.join();
    if (dev_fail) return fail(dev_fail);
    if (!resident_ok) return refuse(R.resident_err);
    R.clk.stop(PH_TRIAL_EVAL);
    R.clk.start();
    factors_.forEachWindow(NW, [&](size_t w) {
        Run::State &T = R.st[w];
        if (!T.stepped || trial_failed.load()) return;
        if (R.deferred()) sumHostCosts(R, w);
        bool accepted;
        T.done = T.tr.trial(R.o, R.cost[w] + R.host_cost[w], T.model, windows_[w].problem, &accepted);
        if (accepted)
            T.relinearize = !T.done;
        else
            T.redamp = true;
    });
    if (trial_failed.load()) return refuse("a host cost function failed to evaluate");
    R.clk.stop(PH_TRIAL_HOST);
    return true;
}

std::vector<int> WindowSolverBatch::removeReprojectionFactorsByChi2(double chi2) {
    std::vector<int> removed(windows_.size(), 0);
    if (!finalized_ && !finalize()) return removed;
    std::vector<double> poses, ext, inv, td;
    factors_.gather(poses, ext, inv, td);
    icg_ctx *ctx = factors_.ctx();
    // raw residuals, no loss: problem.EvaluateResidualBlock(id, false, &cost, ...) with cost = 0.5 |r|^2 (ic_gvins.cc:1278-1284); the
    // test runs where the residuals are, only the flags come back
    std::vector<uint8_t> before(active_);
    if (icg_reproj_eval_windows(ctx, factors_.numPoses(), poses.data(), ext.data(), factors_.numLandmarks(), inv.data(), td.data(), 0, 0.0) != ICG_OK ||
        icg_reproj_chi2_cull(ctx, chi2, active_.data()) != ICG_OK) {
        error_ = icg_last_error(ctx);
        active_.swap(before);
        return removed;
    }
    factors_.forEachWindow(windows_.size(), [&](size_t w) {
        const WindowFactorSet::Window &F = factors_.window(w);
        int r                            = 0;
        for (int k = 0; k < F.size(); k++) {
            const size_t f = (size_t) F.fac_begin + (size_t) k;
            r += before[f] && !active_[f];
        }
        removed[w] = r;
    });
    return removed;
}

} // namespace icg
