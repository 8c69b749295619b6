// Host side of the back-end boundary: the reprojection factor and its batch (see factors.h for the reference lines each class mirrors).
#include "reproj_factors.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <limits>
#include <stdexcept>

namespace icg {

void HuberLossHip::Evaluate(double s, double rho[3]) const {
    if (s > b_) {
        const double r = std::sqrt(s);
        rho[0]         = 2.0 * a_ * r - b_;
        rho[1]         = std::max(std::numeric_limits<double>::min(), a_ / r);
        rho[2]         = -rho[1] / (2.0 * s);
    } else {
        rho[0] = s;
        rho[1] = 1.0;
        rho[2] = 0.0;
    }
}

// ---- ReprojectionFactor / ReprojectionBatch ---------------------------------------------------------------------------
ReprojectionFactor::ReprojectionFactor(Vector3d pts0, Vector3d pts1, Vector3d vel0, Vector3d vel1, double td0, double td1,
                                       double std) {
    for (int i = 0; i < 3; i++) {
        obs_[i]     = pts0[i];
        obs_[3 + i] = pts1[i];
        obs_[6 + i] = vel0[i];
        obs_[9 + i] = vel1[i];
    }
    obs_[12] = td0;
    obs_[13] = td1;
    obs_[14] = std; // sqrt_info = 1/std on the diagonal (reprojection_factor.h:50-52)
}

bool ReprojectionFactor::Evaluate(const double *const *, double *residuals, double **jacobians) const {
    // The values were computed by ReprojectionBatch::PrepareForEvaluation for the state currently stored in the user
    // parameter arrays (which is what Ceres passes here).  No batch / not prepared -> evaluation failed, loudly.
    if (!batch_ || slot_ < 0 || !batch_->prepared(jacobians != nullptr)) return false;
    const double *r = batch_->residual(slot_);
    residuals[0]    = r[0];
    residuals[1]    = r[1];
    if (jacobians) {
        const double *J = batch_->jacobian(slot_);
        if (jacobians[0]) memcpy(jacobians[0], J, sizeof(double) * 14);
        if (jacobians[1]) memcpy(jacobians[1], J + 14, sizeof(double) * 14);
        if (jacobians[2]) memcpy(jacobians[2], J + 28, sizeof(double) * 14);
        if (jacobians[3]) memcpy(jacobians[3], J + 42, sizeof(double) * 2);
        if (jacobians[4]) memcpy(jacobians[4], J + 44, sizeof(double) * 2);
    }
    return true;
}

ReprojectionBatch::ReprojectionBatch(int device) {
    icg_ctx_config cfg{};
    cfg.device      = device;
    cfg.width       = 64; // the back-end context holds no images
    cfg.height      = 64;
    cfg.n_slots     = 1;
    cfg.max_batch   = 1;
    cfg.max_points  = 64;
    cfg.max_factors = 4096;
    if (icg_ctx_create(&cfg, &ctx_) != ICG_OK) throw std::runtime_error(std::string("ReprojectionBatch: ") + icg_last_error(nullptr));
}

ReprojectionBatch::~ReprojectionBatch() {
    for (auto *f : factors_) {
        f->batch_ = nullptr;
        f->slot_  = -1;
    }
    icg_ctx_destroy(ctx_);
}

void ReprojectionBatch::setWaitMode(int icg_wait_mode, int sleep_us) { (void) icg_ctx_set_wait_mode(ctx_, icg_wait_mode, sleep_us); }

void ReprojectionBatch::clear() {
    for (auto *f : factors_) {
        f->batch_ = nullptr;
        f->slot_  = -1;
    }
    factors_.clear();
    pose_ptrs_.clear();
    lm_ptrs_.clear();
    pose_index_.clear();
    lm_index_.clear();
    idx_i_.clear();
    idx_j_.clear();
    idx_lm_.clear();
    ext_ = td_ = nullptr;
    finalized_ = prepared_ = has_jac_ = false;
}

void ReprojectionBatch::add(ReprojectionFactor *factor, double *pose_i, double *pose_j, double *extrinsic, double *invdepth,
                            double *td) {
    auto index_of = [](std::unordered_map<const double *, int> &m, vector<double *> &v, double *p) {
        auto it = m.find(p);
        if (it != m.end()) return it->second;
        int k = (int) v.size();
        v.push_back(p);
        m[p] = k;
        return k;
    };
    if (ext_ && (ext_ != extrinsic || td_ != td)) throw std::runtime_error("ReprojectionBatch: one extrinsic/td block per batch");
    ext_ = extrinsic;
    td_  = td;
    factor->batch_ = this;
    factor->slot_  = (int) factors_.size();
    factors_.push_back(factor);
    idx_i_.push_back(index_of(pose_index_, pose_ptrs_, pose_i));
    idx_j_.push_back(index_of(pose_index_, pose_ptrs_, pose_j));
    idx_lm_.push_back(index_of(lm_index_, lm_ptrs_, invdepth));
    finalized_ = prepared_ = false;
}

void ReprojectionBatch::finalize() {
    const int n = (int) factors_.size();
    if (n == 0) { // a window without visual factors (the reference solves those too: GNSS / IMU only)
        finalized_ = true;
        prepared_  = false;
        return;
    }
    vector<double> obs((size_t) 15 * n);
    for (int k = 0; k < n; k++)
        for (int c = 0; c < 15; c++) obs[(size_t) c * n + k] = factors_[(size_t) k]->obs_[c];
    if (icg_reproj_set_factors(ctx_, n, obs.data(), idx_i_.data(), idx_j_.data(), idx_lm_.data()) != ICG_OK)
        throw std::runtime_error(std::string("icg_reproj_set_factors: ") + icg_last_error(ctx_));
    finalized_ = true;
    prepared_  = false;
}

bool ReprojectionBatch::run(bool want_jac, double huber, bool fetch) {
    prepared_ = false;
    if (factors_.empty()) {
        prepared_ = has_jac_ = true;
        return true;
    }
    if (!finalized_) finalize();
    vector<double> poses(7 * pose_ptrs_.size()), inv(lm_ptrs_.size());
    for (size_t k = 0; k < pose_ptrs_.size(); k++) memcpy(&poses[7 * k], pose_ptrs_[k], sizeof(double) * 7);
    for (size_t k = 0; k < lm_ptrs_.size(); k++) inv[k] = *lm_ptrs_[k];
    r_view_ = J_view_ = nullptr;
    int rc = fetch ? icg_reproj_eval_resident_view(ctx_, (int) pose_ptrs_.size(), poses.data(), ext_, (int) lm_ptrs_.size(), inv.data(), *td_,
                                                   want_jac ? 1 : 0, huber, &r_view_, &J_view_)
                   : icg_reproj_eval_resident(ctx_, (int) pose_ptrs_.size(), poses.data(), ext_, (int) lm_ptrs_.size(), inv.data(), *td_,
                                              want_jac ? 1 : 0, huber, nullptr, nullptr);
    if (rc != ICG_OK) {
        error_ = icg_last_error(ctx_);
        return false;
    }
    prepared_ = fetch;
    has_jac_  = fetch && want_jac;
    return true;
}

void ReprojectionBatch::PrepareForEvaluation(bool evaluate_jacobians, bool /*new_evaluation_point*/) { run(evaluate_jacobians, 0.0); }

// (the marginalization never reads a factor's slice: the batch is assembled on the device, nothing is fetched)
bool ReprojectionBatch::evaluateCorrected(double huber_delta) { return run(true, huber_delta, false); }

bool ReprojectionBatch::accumulateNormal(const std::unordered_map<const double *, int> &column_of, int local_size, double *H0,
                                         double *b0) {
    if (factors_.empty()) return true;
    auto col = [&](const double *p) {
        auto it = column_of.find(p);
        return it == column_of.end() ? -1 : it->second;
    };
    vector<int32_t> cp(pose_ptrs_.size()), cl(lm_ptrs_.size());
    for (size_t k = 0; k < pose_ptrs_.size(); k++) cp[k] = col(pose_ptrs_[k]);
    for (size_t k = 0; k < lm_ptrs_.size(); k++) cl[k] = col(lm_ptrs_[k]);
    prepared_ = false; // (any further call on the context invalidates the fetched views)
    int rc = icg_reproj_accumulate_normal(ctx_, local_size, cp.data(), col(ext_), cl.data(), col(td_), H0, b0);
    if (rc != ICG_OK) {
        error_ = icg_last_error(ctx_);
        return false;
    }
    return true;
}

bool ReprojectionBatch::accumulateLandmarkEliminated(const std::unordered_map<const double *, int> &camera_column_of, int P, double *H,
                                                     double *b, double *min_hll) {
    if (factors_.empty()) return true;
    auto col = [&](const double *p) {
        auto it = camera_column_of.find(p);
        return it == camera_column_of.end() ? -1 : it->second;
    };
    vector<int32_t> cp(pose_ptrs_.size());
    for (size_t k = 0; k < pose_ptrs_.size(); k++) cp[k] = col(pose_ptrs_[k]);
    vector<double> S((size_t) P * P), s((size_t) P), hll(lm_ptrs_.size());
    prepared_ = false;
    int rc = icg_reproj_schur(ctx_, P, cp.data(), col(ext_), col(td_), nullptr, 1, 0.0, 0.0, 0.0, S.data(), s.data(), nullptr, nullptr);
    if (rc == ICG_OK) rc = icg_reproj_landmark_diag(ctx_, hll.data());
    if (rc != ICG_OK) {
        error_ = icg_last_error(ctx_);
        return false;
    }
    for (size_t k = 0; k < S.size(); k++) H[k] += S[k];
    for (int k = 0; k < P; k++) b[(size_t) k] += s[(size_t) k];
    double mn = hll.empty() ? 0.0 : hll[0];
    for (double v : hll) mn = std::min(mn, v);
    if (min_hll) *min_hll = mn;
    return true;
}

} // namespace icg
