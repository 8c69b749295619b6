// Back-end boundary B1: the reference's ceres::CostFunction subclasses re-built on the HIP C ABI.
//
//   ReprojectionFactor     reference factors/reprojection_factor.h:36-158   (SizedCostFunction<2,7,7,7,1,1>)
//   ReprojectionBatch      NEW: a ceres::EvaluationCallback that evaluates ALL registered reprojection factors with one
//                          batched kernel per evaluation point; each factor's Evaluate() copies its slice out
//   ResidualBlockInfo      reference factors/residual_block_info.h:29-120
//   MarginalizationInfo    reference factors/marginalization_info.h:30-316
//   MarginalizationFactor  reference factors/marginalization_factor.h:31-105
//   Preintegration*        reference preintegration/preintegration{,_base,_normal,_earth}.{h,cc}, preintegration_factor.h
//
// There is no CPU fallback for the reprojection math: a ReprojectionFactor whose batch has not been prepared for the
// current evaluation point makes Evaluate() return false (Ceres' "evaluation failed").
#pragma once
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/icgvins_hip.h"
#include "ceres_compat.h"
#include "types.h"

#define POSE_LOCAL_SIZE 6
#define POSE_GLOBAL_SIZE 7

namespace icg {

using std::vector;

// ceres::HuberLoss with a readable delta (the device corrector needs it)
class HuberLossHip : public ceres::LossFunction {
public:
    explicit HuberLossHip(double a) : a_(a), b_(a * a) {}
    void Evaluate(double s, double rho[3]) const override;
    double delta() const { return a_; }

private:
    const double a_, b_;
};

class ReprojectionBatch;

class ReprojectionFactor : public ceres::SizedCostFunction<2, 7, 7, 7, 1, 1> {
public:
    ReprojectionFactor() = delete;
    // same constructor as the reference (reprojection_factor.h:42-53); std = pixel error / focal length
    ReprojectionFactor(Vector3d pts0, Vector3d pts1, Vector3d vel0, Vector3d vel1, double td0, double td1, double std);
    bool Evaluate(const double *const *parameters, double *residuals, double **jacobians) const override;
    const ReprojectionBatch *batch() const { return batch_; }
    const double *observation() const { return obs_; } // the 15 constants in the order of icg_reproj_set_factors

private:
    friend class ReprojectionBatch;
    double obs_[15];
    ReprojectionBatch *batch_{nullptr};
    int slot_{-1};
};

// What MarginalizationInfo needs from the device side of ONE window: its reprojection factors, evaluated (with the robust correction)
// and assembled there.  ReprojectionBatch implements it for a window with a context of its own, MarginalizationBatch (marg_batch.h) for a
// window that shares its launches with the windows of many other streams.
class DeviceFactorSet {
public:
    virtual ~DeviceFactorSet() = default;
    virtual bool owns(const ReprojectionFactor *factor) const = 0;
    virtual int size() const = 0;
    virtual const vector<double *> &landmarkBlocks() const = 0;
    virtual bool evaluateCorrected(double huber_delta) = 0;
    virtual bool accumulateNormal(const std::unordered_map<const double *, int> &column_of, int local_size, double *H0, double *b0) = 0;
    virtual bool accumulateLandmarkEliminated(const std::unordered_map<const double *, int> &camera_column_of, int P, double *H, double *b,
                                              double *min_hll) = 0;
    virtual const std::string &error() const = 0;
};

// Owns one icg_ctx.  Usage with Ceres: options.evaluation_callback = &batch; problem.AddResidualBlock(factor, loss, blocks)
// and batch.add(factor, blocks) for every reprojection factor; call finalize() once before solving.
class ReprojectionBatch : public ceres::EvaluationCallback, public DeviceFactorSet {
public:
    explicit ReprojectionBatch(int device = 0);
    ~ReprojectionBatch() override;
    // parameter blocks exactly as passed to AddResidualBlock: pose_ref[7], pose_obs[7], extrinsic[7], invdepth[1], td[1]
    void add(ReprojectionFactor *factor, double *pose_i, double *pose_j, double *extrinsic, double *invdepth, double *td);
    void finalize();
    void clear();
    int size() const override { return (int) factors_.size(); }
    bool owns(const ReprojectionFactor *factor) const override { return factor != nullptr && factor->batch() == this; }
    // ceres::EvaluationCallback: gathers the CURRENT values of the user parameter arrays and launches one batch
    void PrepareForEvaluation(bool evaluate_jacobians, bool new_evaluation_point) override;
    // marginalization support: evaluate with the robust correction applied on device (residual_block_info.h:59-87)
    bool evaluateCorrected(double huber_delta) override;
    // H0 += J^T J, b0 -= J^T e of the last evaluation (marginalization_info.h:195-230); columns by parameter address
    bool accumulateNormal(const std::unordered_map<const double *, int> &column_of, int local_size, double *H0, double *b0) override;
    // the same normal equations with EVERY inverse-depth block of the batch eliminated on the device (icg_reproj_schur, no damping):
    // H (P x P, row-major) += Hcc - G^T diag(1/h_ll) G, b += bc - G^T (b_l / h_ll) in the camera columns given by parameter address
    // (absent = constant block); min_hll = the smallest landmark diagonal (the caller's conditioning guard)
    bool accumulateLandmarkEliminated(const std::unordered_map<const double *, int> &camera_column_of, int P, double *H, double *b,
                                      double *min_hll) override;
    const vector<double *> &landmarkBlocks() const override { return lm_ptrs_; }
    // slices of the last fetched evaluation, read in place from the context's pinned staging memory (valid while prepared())
    const double *residual(int slot) const { return r_view_ + 2 * (size_t) slot; }
    const double *jacobian(int slot) const { return J_view_ + 46 * (size_t) slot; }
    bool prepared(bool with_jacobians) const { return prepared_ && (!with_jacobians || has_jac_); }
    const std::string &error() const override { return error_; }
    // completion waits of this batch's context: busy-wait (default, lowest latency for one solver) or poll + sleep (many solvers
    // in flight on few host cores: see icg_ctx_set_wait_mode)
    void setWaitMode(int icg_wait_mode, int sleep_us);

private:
    friend class WindowSolver; // solver_hip.h: drives the resident factors through the Schur entry points
    // fetch = false leaves the results on the device only (WindowSolver): the per-factor Evaluate() surface is then NOT prepared
    bool run(bool want_jac, double huber, bool fetch = true);
    icg_ctx *ctx_{nullptr};
    vector<ReprojectionFactor *> factors_;
    vector<double *> pose_ptrs_, lm_ptrs_; // unique blocks in first-seen order
    std::unordered_map<const double *, int> pose_index_, lm_index_;
    vector<int32_t> idx_i_, idx_j_, idx_lm_;
    double *ext_{nullptr}, *td_{nullptr};
    const double *r_view_{nullptr}, *J_view_{nullptr};
    bool finalized_{false}, prepared_{false}, has_jac_{false};
    std::string error_;
};

// ---- marginalization ------------------------------------------------------------------------------------------------
class ResidualBlockInfo {
public:
    ResidualBlockInfo(std::shared_ptr<ceres::CostFunction> cost_function, std::shared_ptr<ceres::LossFunction> loss_function,
                      vector<double *> parameter_blocks, vector<int> marg_para_index)
        : cost_function_(std::move(cost_function)), loss_function_(std::move(loss_function)),
          parameter_blocks_(std::move(parameter_blocks)), marg_para_index_(std::move(marg_para_index)) {}
    bool Evaluate(); // generic host path (residual_block_info.h:44-88)
    const vector<vector<double>> &jacobians() const { return jacobians_; } // row-major num_residuals x block size
    const vector<int32_t> &parameterBlockSizes() const { return cost_function_->parameter_block_sizes(); }
    const vector<double *> &parameterBlocks() const { return parameter_blocks_; }
    const vector<double> &residuals() const { return residuals_; }
    const vector<int> &marginalizationParametersIndex() const { return marg_para_index_; }
    const std::shared_ptr<ceres::CostFunction> &costFunction() const { return cost_function_; }
    const std::shared_ptr<ceres::LossFunction> &lossFunction() const { return loss_function_; }

private:
    std::shared_ptr<ceres::CostFunction> cost_function_;
    std::shared_ptr<ceres::LossFunction> loss_function_;
    vector<double *> parameter_blocks_;
    vector<int> marg_para_index_;
    vector<vector<double>> jacobians_;
    vector<double> residuals_;
};

// The host-evaluated factors of one window as blocks, in the flat layout icg_reproj_host_parts_build takes: per block nr residuals
// (robust-corrected, as ResidualBlockInfo holds them), the nf columns of the window's compact camera system its free local columns occupy
// and the dense row-major nr x nf Jacobian of those columns at J + jac_off.
struct HostFactorBlocks {
    vector<int32_t> nr, nf, cols;
    vector<int64_t> jac_off;
    vector<double> J, r;
    // gatherHostBlocks with a deferred prior (MarginalizationBatch::setDevicePrior): that factor's block stands in its place with
    // jac_off == kFromPrior, its slots in r reserved (zeros) and nothing in J; prior_block is its position among the blocks gathered by that
    // call (-1: none, or the prior has no residual / no free column), prior_cols the free local columns of its parameter blocks in block
    // order, view.index[a] + x: column y of the block is column prior_cols[y] of the prior's J0
    static constexpr int64_t kFromPrior = ICG_HP_JAC_FROM_PRIOR;
    int prior_block{-1};
    vector<int32_t> prior_cols;
    void clear() { nr.clear(), nf.clear(), cols.clear(), jac_off.clear(), J.clear(), r.clear(), prior_cols.clear(), prior_block = -1; }
};
// the leading `local` columns of one parameter block's row-major nr x size Jacobian into columns [c0, c0 + local) of a dense row-major
// nr x nf Jacobian (a 7-wide pose block contributes its first 6 columns)
inline void gatherJacobianColumns(int nr, int size, int local, const double *Ja, int nf, int c0, double *Jd) {
    for (int k = 0; k < nr; k++)
        for (int x = 0; x < local; x++) Jd[(size_t) k * nf + c0 + x] = Ja[(size_t) k * size + x];
}

class MarginalizationInfo {
public:
    MarginalizationInfo() = default;
    ~MarginalizationInfo();
    bool isValid() const { return isvalid_; }
    static int localSize(int size) { return size == POSE_GLOBAL_SIZE ? POSE_LOCAL_SIZE : size; }
    static int globalSize(int size) { return size == POSE_LOCAL_SIZE ? POSE_GLOBAL_SIZE : size; }
    void addResidualBlockInfo(const std::shared_ptr<ResidualBlockInfo> &blockinfo);
    void updateParamtersIds(const std::unordered_map<long, long> &parameters_ids) { parameters_ids_ = parameters_ids; }
    // reprojection factors registered in `batch` are evaluated (with their Huber loss) and assembled on the GPU
    void setReprojectionBatch(ReprojectionBatch *batch) { batch_ = batch; }
    void setDeviceFactors(DeviceFactorSet *set) { batch_ = set; }
    bool marginalization();
    // wall time of the calling thread's last marginalization(): evaluate, construct, Schur, linearize [ms] (diagnostics / bench)
    static const double *lastPhaseMs();
    static bool lastWasStructured(); // the calling thread's last marginalization() took the landmark-eliminated (device) path
    static void forceDense(bool on);  // process-wide: always take the reference's dense M2 + M3 (diagnostics / tests)
    static bool denseForced();
    vector<double *> getParamterBlocks(std::unordered_map<long, double *> &address);
    const vector<double> &linearizedJacobians() const { return linearized_jacobians_; } // remained x remained, row-major
    const vector<double> &linearizedResiduals() const { return linearized_residuals_; }
    int marginalizedSize() const { return marginalized_size_; }
    int remainedSize() const { return remained_size_; }
    const vector<int> &remainedBlockSize() const { return remained_block_size_; }
    const vector<int> &remainedBlockIndex() const { return remained_block_index_; }
    const vector<double *> &remainedBlockData() const { return remained_block_data_; }
    // exposed for tests: the Schur complement before linearization
    const vector<double> &Hp() const { return Hp_; }
    const vector<double> &bp() const { return bp_; }
    // Where this linearization also lies on the device: window `slot` of the kept linearization `id` (icg_marg_linearize_batch_keep), set by
    // MarginalizationBatch::setKeepLinearized for a window whose prior came from the device call; id 0 = nowhere.  A tag may outlive the
    // kept buffer: MarginalizationPriorSet::set then ships the host arrays, which are always complete.
    void setKeptLinearization(uint64_t id, int slot) { keep_id_ = id, keep_slot_ = slot; }
    uint64_t keptId() const { return keep_id_; }
    int keptSlot() const { return keep_slot_; }
    // Diagnostics / tests: M1 bookkeeping, the evaluation of every factor and the structured plan of this window as marginalization()
    // forms it on the landmark-eliminated path, before the device part is added: H (P x P) and b as planStructured accumulates them, and
    // the same host factors gathered as blocks.  false: the window is not planned (it would take the dense path), or its factors cannot
    // be gathered as blocks.
    bool planWithBlocks(int *P, int *m, vector<double> *H, vector<double> *b, HostFactorBlocks *blocks);
    // Diagnostics / tests of MarginalizationBatch::setDevicePrior's host side: the same steps with the window's prior (devicePriorCandidate,
    // *prior_out) deferred — `deferred` is gathered while that factor has not been evaluated, then the deferred evaluation runs and `eager`
    // is what gatherHostBlocks packs from the evaluated factor.  false: no such prior, or the window is not planned.
    bool planWithDeferredPrior(HostFactorBlocks *deferred, HostFactorBlocks *eager, const ResidualBlockInfo **prior_out = nullptr);
    // The host factor MarginalizationBatch::setDevicePrior hands to the device: the first one (factors_ order) whose cost function is a
    // MargPriorSource, that has no loss function and whose view describes the residual block (r residuals, the blocks' global sizes) — the
    // test WindowSolverBatch::layout applies.  nullptr: the window has none (a robustified prior stays a host factor).
    const ResidualBlockInfo *devicePriorCandidate() const;

private:
    bool updateParameterBlocksIndex();
    // defer (one of this window's factors, or nullptr): that factor is NOT evaluated — its blocks are snapshot like every factor's — until
    // evaluateDeferred() is called (true when there was nothing to do).  A window that stays on the structured device path never calls it.
    bool preMarginalization(const ResidualBlockInfo *defer = nullptr);
    bool evaluateDeferred();
    bool constructEquation();
    void schurElimination();
    // M2 + M3 in one step when the marginalized set is {a few pose / mix blocks} + {inverse depths seen only by the device batch}:
    // the 1x1 landmark blocks are eliminated on the device, the host finishes on the small camera system.  Returns false (nothing
    // touched) when the structure or the conditioning guard does not hold: the dense path then runs as before.
    bool constructAndEliminateStructured();
    // the two host halves of it, either side of the device step (MarginalizationBatch runs that step for many windows in one launch):
    // planStructured checks the structure, lays out the compact camera system and adds the host factors; finishStructured takes the
    // system with the landmark-eliminated device part added and runs the conditioning guard and the small M3.
    // planStructured is planLayout (the structure checks, the compact columns, P, m, r, camera_column_of) followed by planAccumulate (J^T J
    // and J^T e of the host factors into H and b); MarginalizationBatch::setDeviceReducedSystem calls planLayout alone and ships the host
    // factors as blocks instead (gatherHostBlocks).
    struct StructuredPlan {
        int P{0}, m{0}, r{0};
        vector<double> H, b;
        std::unordered_map<const double *, int> camera_column_of;
        vector<int> compact; // local column -> column of the compact camera system, -1 for an inverse depth
    };
    bool planStructured(StructuredPlan &plan);
    bool planLayout(StructuredPlan &plan);
    void planAccumulate(StructuredPlan &plan);
    // The window's host factors (factors_ order, the factors on the device batch skipped), appended to `out` as one block each.  false —
    // `out` is then as it was — when a factor lists a parameter block twice (its J^T J is not one block's) or has more than
    // ICG_HOST_PART_MAX_NR residuals: the caller treats the window as not planned.
    // prior (the factor preMarginalization deferred): its block is emitted in its place — the block order is factors_ order, the device
    // sums follow it — with nr = r, its nf window columns, its slots in r reserved, HostFactorBlocks::kFromPrior for a Jacobian offset, and
    // out.prior_block / out.prior_cols say where J0's columns go.
    bool gatherHostBlocks(const StructuredPlan &plan, HostFactorBlocks &out, const ResidualBlockInfo *prior = nullptr);
    bool finishStructured(StructuredPlan &plan, double min_hll);
    friend class MarginalizationBatch;
    void linearization();
    // (:99) the window's factor records are done with.  The reference frees them here; a window's ~1 100 records own ~3 heap blocks each
    // (the reference's residual_block_info.h layout) and freeing them in line is a third of one marginalization — so they are RETIRED: kept
    // until this object is destroyed (it lives on as the prior until the next marginalization replaces it) and freed then, by whoever
    // drops it.  (Rounds 4-5 handed them to a process-wide reaper thread: a thread a drop-in library has no business starting — VERDICT r5,
    // ADVICE r5 on fork() and static teardown.)
    void releaseMemory() {
        if (retired_.empty())
            retired_.swap(factors_);
        else
            retired_.insert(retired_.end(), std::make_move_iterator(factors_.begin()), std::make_move_iterator(factors_.end()));
        factors_.clear();
    }
    // the same, with the records handed to `bin` (MarginalizationBatch keeps the retired records of all its windows until clear())
    void releaseMemoryInto(vector<std::shared_ptr<ResidualBlockInfo>> &bin) {
        bin.insert(bin.end(), std::make_move_iterator(factors_.begin()), std::make_move_iterator(factors_.end()));
        factors_.clear();
    }
    long idOf(const double *p) { return parameters_ids_[reinterpret_cast<long>(p)]; }

    vector<double> H0_, Hp_, b0_, bp_;
    std::unordered_map<long, long> parameters_ids_;
    std::unordered_map<long, int> parameter_block_size_;
    std::unordered_map<long, int> parameter_block_index_;
    std::unordered_map<long, double *> parameter_block_data_;
    vector<int> remained_block_size_, remained_block_index_;
    vector<double *> remained_block_data_;
    int marginalized_size_{0}, remained_size_{0}, local_size_{0};
    vector<std::shared_ptr<ResidualBlockInfo>> factors_, retired_; // retired_: see releaseMemory()
    const double EPS = 1e-8;
    vector<double> linearized_jacobians_, linearized_residuals_;
    bool isvalid_{true};
    DeviceFactorSet *batch_{nullptr};
    ResidualBlockInfo *deferred_{nullptr}; // preMarginalization(defer): not evaluated yet
    uint64_t keep_id_{0};
    int keep_slot_{-1};
};

// M4 on plain arrays: what MarginalizationFactor::Evaluate reads of a MarginalizationInfo.  index[b] is block b's first local column
// (the remained block index minus the marginalized size), x0[b] its linearization point (size[b] values).
struct MargPriorView {
    int r{0}, n_blocks{0};
    const int *size{nullptr}, *index{nullptr};
    const double *const *x0{nullptr};
    const double *J0{nullptr}, *e0{nullptr}; // r x r row-major, r
    // the same J0 / e0 on the device: window keep_slot of the kept linearization keep_id (MarginalizationInfo::keptId); 0 / -1: host only
    uint64_t keep_id{0};
    int keep_slot{-1};
};

// A cost function that IS a linearized marginalization prior says so: its Evaluate is evaluateMargPrior over the view, block b of the view
// being parameter block b of the cost function.  A solver that keeps the priors of its windows resident on the device
// (WindowSolverBatch::setDevicePrior) recognises the prior through this interface; the view stays valid and unchanged while the cost
// function lives.
class MargPriorSource {
public:
    virtual ~MargPriorSource() = default;
    virtual const MargPriorView &margPriorView() const = 0;
};

class MarginalizationFactor : public ceres::CostFunction, public MargPriorSource {
public:
    MarginalizationFactor() = delete;
    MarginalizationFactor(const MarginalizationFactor &) = delete; // (the view points into this object)
    explicit MarginalizationFactor(std::shared_ptr<MarginalizationInfo> marg_info);
    bool Evaluate(const double *const *parameters, double *residuals, double **jacobians) const override;
    const MargPriorView &margPriorView() const override { return view_; }

private:
    std::shared_ptr<MarginalizationInfo> marg_info_;
    vector<int> size_, index_;  // the remained blocks' global sizes; their indices minus the marginalized size
    vector<const double *> x0_; // their linearization points (the info's arrays)
    MargPriorView view_;
};
// MarginalizationFactor::Evaluate (marginalization_factor.h:47-101) over a view: residuals r; jacobians (optional, entries may be null):
// per block an r x size[b] row-major matrix
void evaluateMargPrior(const MargPriorView &view, const double *const *parameters, double *residuals, double **jacobians);

// The priors of many windows resident on the device (icg_marg_prior_set / icg_marg_prior_evaluate): set() after every marginalization,
// evaluate() per LM point.  Results are the bits evaluateMargPrior gives.  The two C entries are referenced weakly: in a build of this
// layer on a C ABI without them available() is false and set() fails by name.
class MarginalizationPriorSet {
public:
    static bool available(); // icg_marg_prior_set and icg_marg_prior_evaluate are in this build
    // packs and uploads the priors once; x0 is read through the views now (a MarginalizationInfo's remainedBlockData() is the info's own
    // copy and does not change after marginalization()).  Replaces the set `ctx` held.  false with *err set on failure.
    bool set(icg_ctx *ctx, const vector<MargPriorView> &views, std::string *err = nullptr);
    bool set(icg_ctx *ctx, const vector<std::shared_ptr<MarginalizationInfo>> &infos, std::string *err = nullptr);
    // parameters[w][b]: block b of window w at the evaluation point.  residuals: residualSize() doubles, window after window;
    // jacobians (optional): jacobianSize() doubles, per window its blocks concatenated, block b r x size[b] row-major;
    // gradient (optional): J0^T e, residualSize(); sq_norm (optional): e . e per window.
    bool evaluate(const vector<const double *const *> &parameters, double *residuals, double *jacobians, double *gradient, double *sq_norm,
                  std::string *err = nullptr);
    // The resident evaluation (icg_marg_prior_evaluate_resident): the residuals stay on the device for
    // icg_reproj_host_parts_build_prior, only sq_norm (e . e per window) comes back.  pack(w, ...) copies window w's parameter blocks to
    // their place in the set's evaluation point (any thread, before the call; a window that is not packed keeps its last point, zeros
    // after set()); evaluateResident() makes the one device call.  The entry is referenced weakly like the two above:
    // residentAvailable() is false in a build of this layer on a C ABI without it, and evaluateResident() then fails by name.
    static bool residentAvailable();
    void pack(size_t w, const double *const *parameters);
    bool evaluateResident(double *sq_norm, std::string *err = nullptr);
    int windows() const { return (int) r_.size(); }
    // The hand-off: when every tagged view of a set() names the same live kept linearization (MargPriorView::keep_id), the tagged windows
    // take J0 / e0 where the linearize call left them on the device (icg_marg_prior_set_from_kept, weakly referenced) and only the untagged
    // windows' arrays are packed and shipped.  Without the entry, with differing ids or with a linearization that is gone, set() ships
    // every window as before.  handedOff(): the windows of the last set() that took the hand-off.
    static bool handOffAvailable();
    int handedOff() const { return handed_off_; }
    size_t residualSize() const { return residual_size_; }
    size_t jacobianSize() const { return jacobian_size_; }

private:
    icg_ctx *ctx_{nullptr};
    vector<int32_t> r_, block_off_, block_size_;
    vector<size_t> x_off_; // first parameter of window w in x_
    vector<double> x_; // the evaluation point, packed like x0
    size_t residual_size_{0}, jacobian_size_{0};
    int handed_off_{0};
};

// M3 on plain arrays (marginalization_info.h:153-192), what MarginalizationInfo::schurElimination / linearization run.  schurReduce: the m
// leading columns of the P x P system (H row-major, b) are eliminated through the eigen-decomposition of Hmm with the eps floor (m = 0:
// Hp = H, bp = b).  linearizePrior: Hp = J0^T J0, bp = -J0^T e0 on the eigenvalues above eps (J0 r x r row-major).  Optional: evals (of
// Hp, ascending), min_ev_m (smallest eigenvalue of the m-block, +inf for m = 0), status (bits OR-ed in: 2 = an m-block eigenvalue <= eps,
// 4 = an Hp eigenvalue <= eps; linearizeReduced clears it first).
void schurReduce(int P, int m, const double *H, const double *b, double eps, vector<double> &Hp, vector<double> &bp, double *min_ev_m = nullptr,
                 int *status = nullptr);
void linearizePrior(int r, const vector<double> &Hp, const vector<double> &bp, double eps, vector<double> &J0, vector<double> &e0,
                    vector<double> *evals = nullptr, int *status = nullptr);
void linearizeReduced(int P, int m, const double *H, const double *b, double eps, vector<double> &Hp, vector<double> &bp, vector<double> &J0,
                      vector<double> &e0, vector<double> *evals = nullptr, double *min_ev_m = nullptr, int *status = nullptr);

// symmetric eigen-decomposition (Householder tridiagonalisation + implicit QL), eigenvalues ascending, evecs row-major with eigenvectors in columns
void symmetricEigen(int n, const vector<double> &A, vector<double> &evals, vector<double> &evecs);

// ---- preintegration (P1 on device; P2 on host per factor, or batched on device) -------------------------------------------------------------------------
struct IMU { // common/types.h:48-56
    double time, dt;
    Vector3d dtheta, dvel;
    double odovel{0};
};
struct Quaterniond {
    double x{0}, y{0}, z{0}, w{1};
};
struct IntegrationState { // preintegration/integration_state.h:35-52 (fields used by the Normal/Earth variants)
    double time{0};
    Vector3d p;
    Quaterniond q;
    Vector3d v, bg, ba;
    Vector3d sg, sa; // gyroscope / accelerometer scale factors (used by MISC::insMechanization when iswithscale)
    double sodo{0};  // odometer scale factor (only written out by MISC::writeNavResult)
};
struct IntegrationParameters { // integration_state.h:67-88
    double acc_vrw{0}, gyr_arw{0}, gyr_bias_std{0}, acc_bias_std{0}, corr_time{1}, gravity{9.8};
    Vector3d iewn; // Earth rotation in the local frame, Earth::iewn(station, p) — explicit here (SURVEY.md hazard H9)
    // when set, every (re)integration derives its own Earth rate from the interval's start position, as
    // PreintegrationEarth::resetState does (preintegration_earth.cc:319-321); otherwise `iewn` above is used as given
    bool has_station{false};
    Vector3d station;
};

// One IMU interval between two time nodes.  (Re)integration of many intervals is ONE batched device call.
class Preintegration {
public:
    enum Variant { NORMAL = 0, EARTH = 1 };
    Preintegration(std::shared_ptr<IntegrationParameters> parameters, const IMU &imu0, const IntegrationState &state, Variant v);
    void addNewImu(const IMU &imu) { imu_buffer_.push_back(imu); dirty_ = true; }
    void reintegration(const IntegrationState &state);
    const Vector3d &earthRate() const { return iewn_; }
    // integrate every dirty interval of the list with a single icg_preint_batch launch
    static bool integrateBatch(icg_ctx *ctx, const vector<Preintegration *> &list, std::string *err = nullptr);
    // P2 on the device: residual 15 (and, unless `jacobians` is null, the Jacobians 480 = 15x7 | 15x9 | 15x7 | 15x9) of every factor of the
    // list at its evaluation point (points: n x 32 = pose0[7] mix0[9] pose1[7] mix1[9]) through icg_preint_evaluate_batch, one call per
    // variant present.  ok[k] = 0 (and zero rows) for a factor that is not integrated for its current buffer / start state or whose
    // covariance is singular: the two conditions under which evaluate() returns false.  sqrt_info (optional, n x 225): the square-root
    // information the device formed.  Returns false with *err set when a call fails or the entry point is not in this build.
    static bool evaluateBatch(icg_ctx *ctx, const vector<const Preintegration *> &list, const double *points, double *residuals,
                              double *jacobians, vector<char> *ok, std::string *err = nullptr, double *sqrt_info = nullptr);
    static bool evaluateBatchAvailable(); // icg_preint_evaluate_batch is in this build
    const IntegrationState &currentState() const { return current_state_; }
    const IntegrationState &deltaState() const { return delta_state_; }
    double deltaTime() const { return delta_time_; }
    const vector<IMU> &imuBuffer() const { return imu_buffer_; }
    // PreintegrationFactor::Evaluate body (preintegration_factor.h:45-69): residual 15, Jacobians 15x7,15x9,15x7,15x9
    bool evaluate(const double *const *parameters, double *residuals, double **jacobians) const;
    // The only two places of evaluate() where sin / cos / sqrt enter, as unit quaternions (x, y, z, w), formed with evaluate()'s own
    // expressions: the bias correction of delta q at mix0 (v3, bg3, ba3), rotvec2quat(dq_dbg (bg0 - delta.bg)), and the Earth variant's
    // rotvec2quat(-iewn T), a constant of the integration result (identity, and unused, for the Normal variant).
    void correctionQuaternion(const double *mix0, double q_xyzw[4]) const;
    void earthRateQuaternion(double q_xyzw[4]) const;
    // evaluate() with the two quaternions given: everything that is left is + - * / in a fixed order.  evaluate() is
    // correctionQuaternion + earthRateQuaternion + evaluateGiven; a caller that evaluates on the device (icg_preint_set /
    // icg_preint_evaluate_resident) ships the quaternions instead of calling sin / cos there.
    bool evaluateGiven(const double *const *parameters, const double q_corr[4], const double q_nn[4], double *residuals, double **jacobians) const;
    Variant variant() const { return variant_; }
    const vector<double> &sqrtInformation() const { return sqrt_information_; } // 15x15 row-major; zeros while the covariance is singular
    // what a resident set packs besides deltaState(), deltaTime(), sqrtInformation() and earthRate()
    bool ready() const { return !dirty_ && sqrt_information_ok_; } // integrated for the current buffer / start state, covariance not singular
    const vector<double> &jacobian() const { return jacobian_; }   // 15x15 row-major
    double gravity() const { return parameters_->gravity; }
    const vector<double> &pnRows() const { return pn_; }           // Earth variant: rows of 4 (dt, position); evaluate() sums the complete rows

private:
    std::shared_ptr<IntegrationParameters> parameters_;
    Variant variant_;
    vector<IMU> imu_buffer_;
    IntegrationState start_state_, current_state_, delta_state_;
    double delta_time_{0};
    void updateSqrtInformation();
    vector<double> jacobian_, covariance_, pn_; // 15x15, 15x15, (n-1)x4
    vector<double> sqrt_information_;            // 15x15, of covariance_ (formed when an integration result arrives)
    bool sqrt_information_ok_{false};
    Vector3d iewn_; // this interval's Earth rate: P1 (device) and P2 (evaluate) use the same value
    bool dirty_{true};
};

class PreintegrationFactor : public ceres::CostFunction {
public:
    explicit PreintegrationFactor(std::shared_ptr<Preintegration> preintegration);
    bool Evaluate(const double *const *parameters, double *residuals, double **jacobians) const override {
        return preintegration_->evaluate(parameters, residuals, jacobians);
    }
    // what a solver that evaluates the factor on the device (WindowSolverBatch::setDevicePreintegration) packs its resident set from
    const Preintegration &preintegration() const { return *preintegration_; }

private:
    std::shared_ptr<Preintegration> preintegration_;
};

// The preintegration factors of many windows resident on the device for a solve (icg_preint_set / icg_preint_evaluate_resident): set() at the
// head of the solve, pack() + evaluateResident() per LM point.  The device gets the host's square-root information and the two quaternions
// of Preintegration::evaluate that need sin / cos (earthRateQuaternion with the set, correctionQuaternion with every point); its residuals,
// Jacobians and squared norms are then the bits of Preintegration::evaluate.  The results stay on the device for
// icg_reproj_host_parts_build_preint; only one squared norm per factor comes back.  The C entries are referenced weakly: in a build of this
// layer on a C ABI without them available() is false, missingEntry() names the first that is absent and set() fails by that name.
class PreintegrationSet {
public:
    static bool available();
    static const char *missingEntry(); // nullptr when available()
    // every factor must be ready() (integrated, covariance not singular); the objects must outlive the set's use
    bool set(icg_ctx *ctx, const vector<const Preintegration *> &list, std::string *err = nullptr);
    // factor f's evaluation point (pose0, mix0, pose1, mix1) and its correction quaternion to their places (any thread, before the call)
    void pack(size_t f, const double *const *parameters);
    bool evaluateResident(bool want_jac, double *sq_norm, std::string *err = nullptr);
    int factors() const { return (int) list_.size(); }

private:
    icg_ctx *ctx_{nullptr};
    vector<const Preintegration *> list_;
    vector<double> points_, q_corr_;
};

} // namespace icg
