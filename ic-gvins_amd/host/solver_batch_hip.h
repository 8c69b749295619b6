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
#include "solver_hip.h"

namespace icg {

class WindowSolverBatch {
public:
    typedef WindowSolver::Options Options;
    typedef WindowSolver::Summary Summary;
    // Widest reduced system of the device path: the assembly (csrc/reproj_asm.hip k_asm_*) keeps no per-window tile in LDS any more — rounds 2-5
    // held the camera block there (82, then 138 columns).  The reduction kernel k_schur_reduce_w stages its landmark rows of 4 ceil(P/4)
    // doubles in SCH_PRE * 256 = 3 072 elements per pass (at least one row up to P = 3 072) and keeps two entries of s per thread (t and
    // t + 256): P <= 512.  A window that can exceed it is the caller's to solve on the host.
    static constexpr int kMaxCameraColumns = 512;

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
    int numReprojectionFactors(int w) const { return (int) windows_.at((size_t) w).visual.size(); }
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
    bool solve(const Options &options, std::vector<Summary> *summaries);
    // removeReprojectionFactorsByChi2 (ic_gvins.cc:1269-1297) for every window; returns the number removed per window
    std::vector<int> removeReprojectionFactorsByChi2(double chi2);
    const std::string &error() const { return error_; }

private:
    struct VisualFactor {
        double obs[15];
        double *pose_i, *pose_j, *invdepth;
    };
    struct Window {
        solver_detail::Problem problem{"WindowSolverBatch"};
        std::vector<VisualFactor> visual;
        double *ext{nullptr}, *td{nullptr};
        std::vector<double *> poses, landmarks; // first-seen order of the visual factors
        std::unordered_map<const double *, int> pose_index, lm_index;
        int P{0};
        int fac_begin{0}, lm_begin{0}, pose_begin{0};
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
    };
    bool finalize();
    bool layout();
    void gather(std::vector<double> &poses, std::vector<double> &ext, std::vector<double> &inv, std::vector<double> &td);

    // fn(w) for every window on the persistent helper threads (created on first use: a batch of one or two windows never needs them)
    template <typename F> void forEachWindow(size_t n, F &&fn);

    icg_ctx *ctx_{nullptr};
    double huber_;
    int host_threads_;
    std::unique_ptr<HostPool> pool_;
    std::unique_ptr<SideThread> side_; // runs the device call of a phase beside the pool's host half
    std::vector<Window> windows_;
    std::vector<uint8_t> active_;
    std::vector<int32_t> col_pose_, col_ext_, col_td_;
    int P_{0}, n_factors_{0}, n_poses_{0}, n_lm_{0};
    bool finalized_{false};
    bool device_reduced_{false}, device_host_part_{false};
    // device host part (layout()): the block list of all windows as icg_reproj_host_parts_build takes it, and the sizes of a call's J and r
    std::vector<int32_t> hp_blk_off_, hp_nr_, hp_nf_, hp_cols_;
    size_t hp_J_total_{0}, hp_r_total_{0};
    std::string error_;
};

} // namespace icg
