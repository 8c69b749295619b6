// The reprojection factor of boundary B1 and its batch (see factors.h for the reference lines each class mirrors).
#pragma once
#include <memory>
#include <string>
#include <unordered_map>
#include <vector>

#include "../../include/icgvins_hip.h"
#include "ceres_compat.h"
#include "types.h"

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

} // namespace icg
