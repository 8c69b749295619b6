// Many sliding windows optimized together — the multi-stream form of WindowSolver (solver_hip.h), SURVEY.md §8 row f1.
//
// One WindowSolver per camera stream is bounded by the runtime's rate of small launches and copies (~100 per window and solve).
// WindowSolverBatch advances the LM iterations of W independent windows in lock-step on ONE device context: per iteration one
// evaluation launch for the reprojection factors of all windows, one assembly + elimination launch sequence, one back-substitution
// launch; each window keeps its own trust-region radius, accepts or rejects its own step and stops by its own tolerances, exactly as
// a WindowSolver of its own would (tests: identical step sequences and optima): the problem model, the column layout and the step rule of
// a window are solver_detail.h's, shared with WindowSolver; the lock-step schedule is this class's own.  Host-evaluated factors
// (preintegration, marginalization prior, priors) stay per window on the host, and so do the P x P reduced solves unless
// setDeviceReducedSolve(true) moves them to the device (icg_reproj_solve_windows: the same bits, off by default).
#pragma once
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "host_pool.h"
#include "nav_factor_set.h"
#include "preintegration_odo.h"
#include "solver_hip.h"
#include "window_factors.h"

namespace icg {

class WindowSolverBatch {
public:
    typedef WindowSolver::Options Options;
    typedef WindowSolver::Summary Summary;
    static constexpr int kMaxCameraColumns = icg::kMaxCameraColumns; // (window_factors.h)

    // host_threads: the per-window host phases (host factors, reduced solves, cost bookkeeping) are spread over this many threads
    explicit WindowSolverBatch(int device = 0, double huber_delta = 1.0, int host_threads = 0 /* 0 = hardware concurrency, at most 16 */);
    ~WindowSolverBatch();
    WindowSolverBatch(const WindowSolverBatch &) = delete;
    WindowSolverBatch &operator=(const WindowSolverBatch &) = delete;

    int addWindow();
    int numWindows() const { return (int) windows_.size(); }
    // drops every window but keeps the device context (a batch object that is re-used for one set of windows after another)
    void clear();
    void addParameterBlock(int w, double *values, int size, bool pose_manifold = false);
    void setParameterBlockConstant(int w, double *values);
    int addResidualBlock(int w, std::shared_ptr<ceres::CostFunction> cost, std::shared_ptr<ceres::LossFunction> loss, const std::vector<double *> &blocks);
    void removeResidualBlock(int w, int id);
    // problem.EvaluateResidualBlock(id, apply_loss_function, &cost, nullptr, nullptr) for a host factor of window w
    bool evaluateResidualBlock(int w, int id, bool apply_loss_function, double *cost) const;
    int numReprojectionFactors(int w) const { return factors_.window((size_t) w).size(); }
    // a reprojection factor of window w with the five blocks it would get in AddResidualBlock (only its observation constants are
    // read from `factor`); all factors of a window share its extrinsic and td blocks
    void addReprojectionFactor(int w, const ReprojectionFactor *factor, double *pose_i, double *pose_j, double *extrinsic, double *invdepth, double *td);

    // uploads the factor set and the window partition (done by the first solve() otherwise): problem setup, not part of a solve
    bool prepare();
    // The reduced camera solves of an LM step on the device: the reduced systems stay resident (icg_reproj_schur_windows_resident) and the
    // phases "reduced solve" and "back-substitution" become one icg_reproj_solve_windows call; a window's host-factor part is shipped only in
    // a step that re-linearized it.  The iteration budget, the gradient test, the damping, the reject / re-damp decisions (taken from the
    // call's status) and the trial handling stay on the host, and delta_c is the host solve's bit for bit: the LM sequence does not change.
    // Off by default.  The three C entries are referenced weakly: in a build of this layer on a C ABI without them
    // deviceReducedSolveAvailable() is false and solve() fails by name when the option is on.
    void setDeviceReducedSolve(bool on) { device_reduced_ = on; }
    bool deviceReducedSolve() const { return device_reduced_; }
    static bool deviceReducedSolveAvailable();
    // With the device reduced solve: the host-factor part of every re-linearized window (J^T J of the factors the device does not evaluate) is
    // built on the device too (icg_reproj_host_parts_build: hostFactors' bits).  The pool threads only evaluate and gather the factors'
    // residuals and Jacobians into one call buffer; no P x P host part is formed and none is shipped.  A block whose gathered Jacobian equals
    // (memcmp) what the window shipped at its previous rebuild of this solve goes up as its residuals only: the constant J0 of a linearized
    // prior crosses the link once per solve.  The trial costs stay on the pool.  Off by default; needs setDeviceReducedSolve(true) (solve()
    // fails otherwise) and the C entry, which is referenced weakly like the three above.
    void setDeviceHostPart(bool on) { device_host_part_ = on; }
    bool deviceHostPart() const { return device_host_part_; }
    static bool deviceHostPartAvailable();
    // With the device host part: every window's marginalization prior is RESIDENT on the device for the solve (MarginalizationPriorSet: J0 goes
    // up once per solve()) and evaluated there at every linearization and every trial point (icg_marg_prior_evaluate_resident, on the side
    // thread that makes the phase's device call: after the Schur call, beside the trial evaluation).  Its residual and its Jacobian reach the
    // host-part kernel without crossing the link (icg_reproj_host_parts_build_prior: the first rebuild of a window in a solve gathers the
    // Jacobian from J0 on the device, the later ones keep it); per evaluation only x goes up and one squared norm per window comes back, and
    // 0.5 * that norm takes the prior's place in the window's host cost, summed in residual order as hostFactors sums it: states, inverse
    // depths and summaries are the host's bit for bit.  The prior of a window is its first residual block whose cost function implements
    // MargPriorSource (factors.h) and has no loss function; a robustified prior and a second prior in a window stay on the pool.  Off by
    // default; needs setDeviceHostPart(true) (solve() fails otherwise) and the two C entries, referenced weakly like the ones above.
    void setDevicePrior(bool on) { device_prior_ = on; }
    bool devicePrior() const { return device_prior_; }
    static bool devicePriorAvailable();
    // windows of the last solve() whose resident prior took J0 / e0 from a kept device linearization instead of the host arrays
    // (MarginalizationPriorSet::handedOff: priors tagged by MarginalizationBatch::setKeepLinearized); needs no switch of its own
    int priorsHandedOff() const { return prior_set_.handedOff(); }
    // With the device host part: the preintegration factors of every window are RESIDENT on the device for the solve (PreintegrationSet: the
    // integration results go up once per solve()) and evaluated there at every linearization (with Jacobians) and every trial point (residual
    // only), on the side thread like the resident priors.  The driving thread packs the evaluation points and the correction quaternions
    // (Preintegration::correctionQuaternion: the device calls no sin / cos); residual and Jacobian reach the host-part kernel without crossing
    // the link (icg_reproj_host_parts_build_preint gathers the free columns at every rebuild: the Jacobian changes with the point), one
    // squared norm per factor comes back and 0.5 * that norm takes the factor's place in the window's host cost, summed in residual order:
    // states, inverse depths and summaries are the host's bit for bit.  A residual block joins the set when it has no loss function, its cost
    // is a PreintegrationFactor and its Preintegration is ready() at the head of the solve; a robustified, unintegrated or singular factor
    // stays on the pool and behaves as without the switch.  Independent of setDevicePrior.  Off by default; needs setDeviceHostPart(true)
    // (solve() fails otherwise) and the C entries, referenced weakly like the ones above.
    void setDevicePreintegration(bool on) { device_preint_ = on; }
    bool devicePreintegration() const { return device_preint_; }
    static bool devicePreintegrationAvailable();
    static const char *devicePreintegrationMissing(); // the first entry the build lacks for it, nullptr when available
    int preintegrationsOnDevice() const { return members(kPreint); } // factors of the last layout that joined the resident set
    // The same switch serves the odometer variants: a residual block without a loss, with four parameter blocks, whose cost is a
    // PreintegrationOdoFactor with preintegration().ready() joins the resident ODOMETER set (PreintegrationOdoSet; 19 residuals, a 19 x 34
    // Jacobian, icg_reproj_host_parts_build_preint_odo) under the same rules and with the same place in the host cost.  A solve without such a
    // factor issues exactly the calls it issued before; one that holds such a factor needs the odometer entries (solve() names the first that
    // is missing).  The number of odometer factors of the last layout that joined their resident set:
    int odometerPreintegrationsOnDevice() const { return members(kPreintOdo); }
    static const char *devicePreintegrationOdoMissing(); // the first entry the build lacks for the odometer factors, nullptr when none
    // With the device host part: the navigation factors of every window (nav_factors.h: GnssFactor, ImuErrorFactor, ImuPosePriorFactor,
    // ImuMixPriorFactor, in both widths) are RESIDENT on the device for the solve (NavFactorSet: kinds and constants go up once per solve())
    // and evaluated there at every linearization (with Jacobians) and every trial point (residual only), last of the resident families.  A
    // residual block joins the set when its cost is a NavFactor with exactly one parameter block of the factor's width; a loss function is
    // allowed: at a linearization rho is evaluated on the host from the returned squared norm (no sqrt on the device), the three corrector
    // scalars of the members with a loss go up in one NavFactorSet::correct call, and the host-part kernel reads what
    // ResidualBlockInfo::Evaluate would hold.  0.5 rho[0] (0.5 times the squared norm without a loss) takes the factor's place in the window's
    // host cost, summed in residual order: states, inverse depths and summaries are the host's bit for bit.  Independent of setDevicePrior
    // and setDevicePreintegration.  Off by default; needs setDeviceHostPart(true) (solve() fails otherwise) and the C entries, referenced
    // weakly like the ones above (solve() names the first that is missing).
    void setDeviceNavFactors(bool on) { device_nav_ = on; }
    bool deviceNavFactors() const { return device_nav_; }
    static const char *deviceNavFactorsMissing();                       // the first entry the build lacks for it, nullptr when available
    int navFactorsOnDevice() const { return members(kNav); }         // factors of the last layout that joined the resident set
    bool solve(const Options &options, std::vector<Summary> *summaries);
    // removeReprojectionFactorsByChi2 (ic_gvins.cc:1269-1297) for every window; returns the number removed per window
    std::vector<int> removeReprojectionFactorsByChi2(double chi2);
    const std::string &error() const { return error_; }

private:
    // The families of residuals that may be resident on the device for a solve, in the order of their precedence in layout() and of their evaluation.  What differs
    // between them is written once per family in the table behind rules() (solver_batch_hip.cc); the rest loops over it and over what layout() derives, a ResidentFamily.
    enum Family { kNone = -1, kPrior = 0, kPreint = 1, kPreintOdo = 2, kNav = 3, kFamilies = 4 };
    struct FamilyRules;
    static const FamilyRules &rules(int family);
    struct ResidentFamily {
        std::vector<std::pair<int, int>> where; // the members, in window and residual order: (window, residual)
        std::vector<int32_t> of, cols; // per block of the host-part list its member (-1: none); the resident blocks' columns of their members' source matrices
    };
    int members(int family) const { return (int) resident_[family].where.size(); }
    const solver_detail::Residual &member(int f, size_t k) const { return windows_[(size_t) resident_[f].where[k].first].problem.residuals[(size_t) resident_[f].where[k].second]; }
    // a window beside its record in factors_: the host-evaluated part of its problem and its state across the steps of a solve
    struct Window {
        solver_detail::Problem problem{"WindowSolverBatch"};
        int P{0};
        std::vector<double> host_S, host_s, host_diag;
        bool host_part_dirty{false}; // host_S was rebuilt since it was last shipped to the device (device reduced solve)
        // device host part: the factors with a free column, in residual order, and where their pieces lie in the buffers of a call
        struct HostBlock {
            int residual, nr, nf;
            size_t J_off, r_off, c_off;
        };
        std::vector<HostBlock> host_blocks;
        std::vector<int32_t> host_cols; // their columns, block after block
        int blk_begin{0};
        // resident residuals (layout()): per residual and per block of host_blocks the family it is resident in on the device (kNone: evaluated on
        // the pool; a resident residual whose blocks are all constant has a cost but no host block) and its index in that family's set; per family
        // the columns of the members' source matrices (a prior's J0, a factor's 15 x 32 or 19 x 34 Jacobian, a navigation factor's nr x width one) its blocks take, block after block
        struct Resident { int family{kNone}, index{-1}; };
        std::vector<Resident> resident_of_residual, resident_of_block;
        std::vector<int32_t> resident_cols[kFamilies];
    };
    // how solve() forms and solves the reduced systems: resolved from the two setters at its top
    enum class ReducedPath { HostSolve, DeviceSolve, DeviceSolveDeviceParts };
    struct Run; // what one solve() works on (solver_batch_hip.cc)
    bool finalize();
    bool layout();
    bool resolvePath(ReducedPath *path);
    // the phases of a lock-step LM round, in their order; false: error_ is set
    bool linearize(Run &R);
    bool reducedSolves(Run &R);
    bool trialPoints(Run &R);
    bool trialCosts(Run &R);
    // where the paths differ: the host half of a window's linearization, and the reduced solves
    bool hostHalfOfWindow(Run &R, size_t w);
    // resident residuals: the evaluation point of every member of the families that are on (driving thread), their evaluation in a phase (side
    // thread, family after family; Jacobians at a linearization only), the host-part call of the narrowest entry that serves them, and a
    // window's host cost once the device values are there
    void packResident(const Run &R);
    bool evaluateResident(Run &R, bool want_jac);
    bool buildHostParts(Run &R);
    void sumHostCosts(Run &R, size_t w);
    void solveWindowOnHost(Run &R, size_t w);
    bool solveWindowsOnDevice(Run &R);
    bool fail(const char *what); // (error_ = what: the context's last error)
    bool refuse(const std::string &what) { return error_ = what, false; }

    WindowFactorSet factors_; // the context, every window's reprojection factors, the host threads
    double huber_;
    std::unique_ptr<SideThread> side_; // runs the device call of a phase beside the pool's host half
    std::vector<Window> windows_;
    std::vector<uint8_t> active_;
    std::vector<int32_t> col_pose_, col_ext_, col_td_;
    int P_{0};
    bool finalized_{false};
    bool device_reduced_{false}, device_host_part_{false}, device_prior_{false}, device_preint_{false}, device_nav_{false};
    // device host part (layout()): the block list of all windows as icg_reproj_host_parts_build takes it, and the sizes of a call's J and r
    std::vector<int32_t> hp_blk_off_, hp_nr_, hp_nf_, hp_cols_;
    size_t hp_J_total_{0}, hp_r_total_{0};
    ResidentFamily resident_[kFamilies]; // (layout())
    MarginalizationPriorSet prior_set_;
    PreintegrationSet preint_set_;
    PreintegrationOdoSet preint_odo_set_;
    NavFactorSet nav_set_;
    std::string error_;
};

} // namespace icg
