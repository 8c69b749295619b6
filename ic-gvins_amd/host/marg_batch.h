// The marginalizations of many camera streams in one pass — the multi-stream form of MarginalizationInfo::marginalization()
// (reference factors/marginalization_info.h:73-101, one call per stream and keyframe from GVINS::gvinsMarginalization,
// ic_gvins.cc:1412-1693), SURVEY.md §8 rows M2 / M3.
//
// One MarginalizationInfo per stream costs three device round trips per marginalization (evaluation with the robust correction,
// assembly + landmark elimination, the h_ll read-back) for ~1 k factors: launch- and wait-bound, the device idles.
// MarginalizationBatch keeps every stream's MarginalizationInfo exactly as the caller built it and runs the windows in lock-step:
//
//   1  ONE evaluation launch for the reprojection factors of all windows (icg_reproj_eval_windows, Huber correction on the device)
//   2  per window, on the host threads: M1 bookkeeping (updateParameterBlocksIndex, marginalization_info.h:232-253), the host-evaluated
//      factors (prior, preintegration, GNSS: ResidualBlockInfo::Evaluate) and the layout of the compact camera system
//   3  ONE assembly + landmark-elimination launch sequence (icg_reproj_schur_windows, no damping) and ONE read-back of the landmark
//      diagonals (icg_reproj_landmark_diag_windows) for all windows
//   4  per window, on the host threads: conditioning guard, the reference's eigen / 1e-8-floor procedure on the few pose / mix columns
//      (M3, :170-192) and the linearization (:153-167)
//
// A window whose marginalized set does not have the structure of gvinsMarginalization, or that fails the conditioning guard, takes the
// reference's dense M2 + M3 on its own (a one-window context created on first use) — the same rule MarginalizationInfo applies alone.
// Results per window are those of MarginalizationInfo::marginalization() on a ReprojectionBatch of its own (tests: Hp, bp, J0, e0).
//
// Options, all off by default, each pinned bit for bit against the one before it: setDeviceLinearization (step 4 in one device call),
// setKeepLinearized (J0 / e0 stay on the device), setDeviceReducedSystem (S and the host factors' J^T J stay on the device), setDevicePrior
// (the previous marginalization's prior is evaluated and gathered on the device; the first guard's minimum is reduced there).
#pragma once
#include <memory>
#include <mutex>
#include <string>
#include <unordered_map>
#include <unordered_set>
#include <vector>

#include "factors.h"
#include "window_factors.h"

namespace icg {

class MarginalizationBatch {
public:
    explicit MarginalizationBatch(int device = 0, double huber_delta = 1.0, int host_threads = 0 /* 0 = hardware concurrency, at most 16 */);
    ~MarginalizationBatch();
    MarginalizationBatch(const MarginalizationBatch &)            = delete;
    MarginalizationBatch &operator=(const MarginalizationBatch &) = delete;

    // a stream's marginalization: `info` is filled by the caller as for marginalization() (updateParamtersIds, addResidualBlockInfo for
    // every factor incl. the reprojection ones); the batch becomes the info's device factor set
    int addWindow(const std::shared_ptr<MarginalizationInfo> &info);
    // the reprojection factors of window w with the five blocks of their ResidualBlockInfo (instead of ReprojectionBatch::add);
    // all factors of a window share its extrinsic and td blocks, a pose block belongs to one window
    void addReprojectionFactor(int w, const ReprojectionFactor *factor, double *pose_i, double *pose_j, double *extrinsic, double *invdepth, double *td);
    int numWindows() const { return (int) windows_.size(); }
    int numReprojectionFactors(int w) const { return factors_.window((size_t) w).size(); }
    // drops every window, keeps the device context (a batch object lives as long as the group of streams it serves)
    void clear();

    // marginalization() of every window.  ok[w] = what the window's own call would have returned (false: info->isValid() is false, as
    // there); the return value is false only when a device call all windows share failed (error()).  A window that failed by itself
    // (its dense fallback could not run) has ok[w] == 0 and its message in windowError(); the other windows are unaffected.
    bool marginalize(std::vector<char> *ok);

    // Step 4 on the device (default off): the guard on the landmark diagonals stays on the host, then ALL planned windows go through one
    // icg_marg_linearize_batch call (M3 on the camera block + linearization, marg_linearize_hip.h); the conditioning guard of the small
    // block (every eigenvalue > 100 x the floor) is applied to the call's min_ev_m.  A window that fails either guard, or whose QL
    // iteration hit its cap, takes the host path of the default mode.  The device's hypot may round differently from the host's: results
    // agree with the default mode to rounding, not bit for bit.  marginalize() fails (error()) when the entry point is not in the build.
    void setDeviceLinearization(bool on) { device_linearization_ = on; }
    bool deviceLinearization() const { return device_linearization_; }
    // With the device linearization (default off; marginalize() fails with a message without setDeviceLinearization(true), or when
    // icg_marg_linearize_batch_keep is not in the build): the device call also KEEPS J0 / e0 of its windows on the device
    // (MarginalizationLinearizer::linearizeKeep), and every window whose prior is taken from the device arrays — it passed both guards —
    // is tagged with the kept linearization's id and its index in that call (MarginalizationInfo::keptId / keptSlot).  A
    // MarginalizationFactor built from a tagged info carries the tag in its view, and MarginalizationPriorSet::set /
    // WindowSolverBatch::setDevicePrior then take J0 / e0 where they lie instead of packing and uploading them.  Windows on the host or
    // dense path stay untagged and are shipped.  The results are those of the device linearization, bit for bit.
    // Resident cost: sum r^2 + sum r doubles in the batch's context (41 MB for 256 C2-estimator windows, r = 142) from marginalize() until
    // the next marginalize() or the destructor releases it.  clear() does NOT release it — the caller clears before it solves.
    void setKeepLinearized(bool on) { keep_linearized_ = on; }
    bool keepLinearized() const { return keep_linearized_; }
    static bool keepLinearizedAvailable();
    uint64_t keptId() const { return kept_id_; } // of the last marginalize(); 0: nothing is kept
    void releaseKept();                          // drops the kept linearization now (tags that name it fall back to shipping)

    // With the device linearization (default off; marginalize() fails with a message without setDeviceLinearization(true), or — naming the
    // entry — when icg_marg_linearize_resident, icg_reproj_schur_windows_resident or icg_reproj_host_parts_build is not in the build): the
    // reduced system H of a window never crosses the link.  Step 2 lays the compact system out and gathers the host factors as blocks (no
    // J^T J on the pool); step 3 leaves S on the device (icg_reproj_schur_windows_resident), builds the host-factor parts there
    // (icg_reproj_host_parts_build: planStructured's arithmetic, bit for bit) and reads the landmark diagonals; step 4 applies the first
    // guard on the host and hands the windows that pass it to ONE icg_marg_linearize_resident call, which forms H = part + S on the
    // device and runs the kernels of icg_marg_linearize_batch on it, with b = host_s + s.  Up: the factor blocks and b; down: s, host_s, the
    // landmark diagonals and the prior.  Every output bit is the one setDeviceLinearization(true) alone gives, and it composes with
    // setKeepLinearized.  The one difference: a window whose QL sweep hit its iteration cap takes the DENSE path here — the device
    // linearization alone finishes it on the host from the H it holds there, which this mode never has.
    void setDeviceReducedSystem(bool on) { device_reduced_system_ = on; }
    bool deviceReducedSystem() const { return device_reduced_system_; }
    static bool deviceReducedSystemAvailable();

    // With the device-resident reduced system (default off; marginalize() fails with a message without setDeviceReducedSystem(true), or —
    // naming the entry — when icg_marg_prior_set, icg_marg_prior_evaluate_resident, icg_reproj_host_parts_build_prior or
    // icg_reproj_landmark_min_windows is not in the build): the prior the previous marginalization left is read from the device.  Each
    // window hands over its first host factor whose cost function is a MargPriorSource, that has no loss function and whose view describes
    // the residual block (WindowSolverBatch::layout's test); a robustified prior and a second prior stay on the pool.  The views of the
    // taken priors form ONE resident MarginalizationPriorSet on the batch's context — tagged views take J0 / e0 from the linearization
    // setKeepLinearized kept (it is released only after the set is built), untagged ones are shipped once.  Step 2 snapshots the prior's
    // blocks but does not evaluate it and emits its block without Jacobian or residual; step 3 evaluates the set at the blocks' current
    // values (icg_marg_prior_evaluate_resident, between the Schur call and the host parts), builds the host parts with the prior's block
    // gathered from J0 on the device (icg_reproj_host_parts_build_prior, ICG_HP_JAC_FROM_PRIOR) and takes the first guard's minimum per window
    // from the device (icg_reproj_landmark_min_windows) instead of reading every landmark diagonal back.  A window that leaves the
    // structured device path (not planned, a failed guard, the QL cap, forced dense) runs the deferred Evaluate() on the pool before its
    // dense path; no other window does.  Up: x and the other host factors' blocks; the prior's residual and r x r Jacobian cross nothing.
    // Every output bit, ok, the tags and the structured / dense counts are those of setDeviceReducedSystem(true) alone, and it composes
    // with setKeepLinearized.  Resident cost: the set's copy (2 r^2 + r doubles per prior) in the batch's context until the next set
    // replaces it or the batch is destroyed.
    void setDevicePrior(bool on) { device_prior_ = on; }
    bool devicePrior() const { return device_prior_; }
    static bool devicePriorAvailable();

    // diagnostics of the last marginalize(): windows that took the landmark-eliminated device path / the dense path; wall time of the
    // four phases above [ms]; setDevicePrior: priors handed to the device, those of them the set took from the kept linearization, and
    // deferred host evaluations that ran
    int structuredWindows() const { return n_structured_; }
    int denseWindows() const { return n_dense_; }
    int devicePriors() const { return n_device_priors_; }
    int devicePriorsFromKept() const { return n_priors_from_kept_; }
    int deferredPriorEvaluations() const { return n_deferred_evaluations_; }
    const double *lastPhaseMs() const { return phase_ms_; }
    icg_ctx *context() const { return factors_.ctx(); } // the batch's partitioned context (its profiler: icg_prof_enable / icg_prof_get)
    const std::string &error() const { return error_; }
    const std::string &windowError() const { return window_error_; } // first per-window failure of the last marginalize()

private:
    // one window's view of the batch: what MarginalizationInfo asks of its device factors
    struct Slice : public DeviceFactorSet {
        MarginalizationBatch *owner{nullptr};
        size_t w{0}; // its record in owner->factors_
        std::shared_ptr<MarginalizationInfo> info;
        std::unordered_set<const ReprojectionFactor *> members;
        bool evaluated{false};
        std::string err;
        const WindowFactorSet::Window &record() const { return owner->factors_.window(w); }
        bool owns(const ReprojectionFactor *factor) const override { return members.count(factor) != 0; }
        int size() const override { return record().size(); }
        const std::vector<double *> &landmarkBlocks() const override { return record().landmarks; }
        bool evaluateCorrected(double huber_delta) override;
        bool accumulateNormal(const std::unordered_map<const double *, int> &column_of, int local_size, double *H0, double *b0) override;
        bool accumulateLandmarkEliminated(const std::unordered_map<const double *, int> &, int, double *, double *, double *) override;
        const std::string &error() const override { return err; }
    };
    bool layout();
    bool denseNormalOfWindow(Slice &W, const std::unordered_map<const double *, int> &column_of, int local_size, double *H0, double *b0);
    // marginalize(): a window's progress through the phases; what the device M3 returns; what one call works on (marg_batch.cc)
    struct State;
    struct DeviceM3;
    struct Run;
    // the four phases above, in their order; false: a device call all windows share failed (fail(): error_ is set, no window stays evaluated)
    bool evaluateWindows(Run &R), assembleAndEliminate(Run &R), guardAndLinearize(Run &R), fail(const std::string &what);
    void bookkeeping(Run &R), addEliminated(Run &R, size_t w);
    static void invalidate(MarginalizationInfo &I);
    bool linearizeOnDevice(Run &R, std::string *what);

    WindowFactorSet factors_; // the partitioned context, every window's reprojection factors, the host threads
    icg_ctx *dense_ctx_{nullptr}; // one-window context of the dense path (created on first use)
    std::mutex dense_mutex_;
    int device_{0};
    double huber_{1.0};
    std::vector<std::unique_ptr<Slice>> windows_;
    bool laid_out_{false};
    bool device_linearization_{false}, keep_linearized_{false}, device_reduced_system_{false}, device_prior_{false};
    uint64_t kept_id_{0};
    MarginalizationPriorSet prior_set_; // setDevicePrior: the taken priors of the last marginalize(), resident in factors_'s context
    int n_device_priors_{0}, n_priors_from_kept_{0}, n_deferred_evaluations_{0};
    std::vector<std::shared_ptr<ResidualBlockInfo>> retired_; // factor records of marginalized windows, freed by clear() / the destructor
    int n_structured_{0}, n_dense_{0};
    double phase_ms_[4]{0, 0, 0, 0};
    std::string error_, window_error_;
};

} // namespace icg
