// M4 on the HIP C ABI: the marginalization priors of many windows resident on the device.  MarginalizationFactor::Evaluate
// (marginalization_factor.h:47-101) stays what the per-factor Ceres callback runs (marginalization.cc evaluateMargPrior); MarginalizationPriorSet
// is the same evaluation for MANY priors per call, for a driver that holds the priors of many windows and evaluates them at every LM point:
// J0 / e0 / x0 cross the link once per marginalization, an evaluation ships the parameters in and the results out.
#include <cstring>

#include "factors.h"
#include "resident_call.h"

// A build of this layer on another implementation of the C ABI may not have the entry points: the references stay weak (null when absent)
// and set() reports it; the product library links libicgvins_hip.so, which defines them.
#pragma weak icg_marg_prior_set
#pragma weak icg_marg_prior_evaluate
#pragma weak icg_marg_prior_evaluate_resident
#pragma weak icg_marg_prior_set_from_kept

namespace icg {

bool MarginalizationPriorSet::available() { return &icg_marg_prior_set != nullptr && &icg_marg_prior_evaluate != nullptr; }

bool MarginalizationPriorSet::residentAvailable() { return available() && &icg_marg_prior_evaluate_resident != nullptr; }

bool MarginalizationPriorSet::handOffAvailable() { return available() && &icg_marg_prior_set_from_kept != nullptr; }

bool MarginalizationPriorSet::set(icg_ctx *ctx, const vector<MargPriorView> &views, std::string *err) {
    if (!available()) {
        if (err) *err = "icg_marg_prior_set is not in this build";
        return false;
    }
    ctx_        = nullptr;
    handed_off_ = 0;
    // the hand-off is taken when every tagged view names the same kept linearization (whether it is still alive the entry says)
    auto tagged = [](const MargPriorView &v) { return v.keep_id != 0 && v.keep_slot >= 0 && v.r > 0; };
    uint64_t keep_id = 0;
    int n_tagged     = 0;
    bool one_id      = true;
    for (const MargPriorView &v : views) {
        if (!tagged(v)) continue;
        if (n_tagged++ == 0) keep_id = v.keep_id;
        one_id = one_id && v.keep_id == keep_id;
    }
    vector<int32_t> index, src;
    vector<double> x0, e0, J0;
    // hand: the tagged windows' J0 / e0 stay behind (src = their kept window), the others' are packed in set order
    auto pack = [&](bool hand) {
        r_.clear(), block_off_.assign(1, 0), block_size_.clear(), x_off_.clear();
        index.clear(), src.clear(), x0.clear(), e0.clear(), J0.clear();
        residual_size_ = jacobian_size_ = 0;
        size_t nj = 0;
        for (const MargPriorView &v : views)
            if (v.r > 0 && !(hand && tagged(v))) nj += (size_t) v.r * (size_t) v.r;
        J0.reserve(nj);
        for (const MargPriorView &v : views) {
            r_.push_back(v.r);
            x_off_.push_back(x0.size());
            size_t xs = 0;
            for (int b = 0; b < v.n_blocks; b++) {
                block_size_.push_back(v.size[b]);
                index.push_back(v.index[b]);
                if (v.size[b] > 0) x0.insert(x0.end(), v.x0[b], v.x0[b] + v.size[b]), xs += (size_t) v.size[b];
            }
            block_off_.push_back((int32_t) block_size_.size());
            src.push_back(hand && tagged(v) ? v.keep_slot : -1);
            if (v.r > 0) {
                if (src.back() < 0) {
                    J0.insert(J0.end(), v.J0, v.J0 + (size_t) v.r * v.r);
                    e0.insert(e0.end(), v.e0, v.e0 + v.r);
                }
                residual_size_ += (size_t) v.r;
                jacobian_size_ += (size_t) v.r * xs;
            }
        }
        // (valid pointers for empty arrays: the entry checks its arguments and names what is wrong)
        block_size_.reserve(1), index.reserve(1), x0.reserve(1), J0.reserve(1), e0.reserve(1), r_.reserve(1), src.reserve(1);
    };
    int rc = ICG_ERR_INVALID;
    if (handOffAvailable() && n_tagged > 0 && one_id && ctx) {
        pack(true);
        rc = icg_marg_prior_set_from_kept(ctx, keep_id, (int) views.size(), src.data(), r_.data(), block_off_.data(), block_size_.data(), index.data(), x0.data(),
                                          J0.data(), e0.data());
        if (rc == ICG_OK) handed_off_ = n_tagged;
        // (refused — the kept linearization is gone, or anything else: the host arrays are complete, the set is shipped as ever and the
        // plain entry reports whatever is wrong with it)
    }
    if (rc != ICG_OK) {
        pack(false);
        rc = icg_marg_prior_set(ctx, (int) views.size(), r_.data(), block_off_.data(), block_size_.data(), index.data(), x0.data(), J0.data(), e0.data());
    }
    if (rc != ICG_OK) {
        if (err) *err = ctx ? icg_last_error(ctx) : "icg_marg_prior_set: no context";
        r_.clear();
        return false;
    }
    x_.assign(x0.size(), 0.0);
    ctx_ = ctx;
    return true;
}

bool MarginalizationPriorSet::set(icg_ctx *ctx, const vector<std::shared_ptr<MarginalizationInfo>> &infos, std::string *err) {
    vector<vector<int>> index(infos.size());
    vector<MargPriorView> views(infos.size());
    for (size_t w = 0; w < infos.size(); w++) {
        const MarginalizationInfo &info = *infos[w];
        for (int i : info.remainedBlockIndex()) index[w].push_back(i - info.marginalizedSize());
        MargPriorView &v = views[w];
        v.r        = info.remainedSize();
        v.n_blocks = (int) info.remainedBlockSize().size();
        v.size     = info.remainedBlockSize().data();
        v.index    = index[w].data();
        v.x0       = info.remainedBlockData().data();
        v.J0       = info.linearizedJacobians().data();
        v.e0       = info.linearizedResiduals().data();
        v.keep_id = info.keptId(), v.keep_slot = info.keptSlot();
    }
    return set(ctx, views, err);
}

bool MarginalizationPriorSet::evaluate(const vector<const double *const *> &parameters, double *residuals, double *jacobians, double *gradient,
                                       double *sq_norm, std::string *err) {
    if (available() && ctx_ && parameters.size() != r_.size()) {
        if (err) *err = "MarginalizationPriorSet::evaluate: one parameter list per window";
        return false;
    }
    return residentCall(available() ? nullptr : "icg_marg_prior_evaluate", ctx_, "MarginalizationPriorSet::evaluate: no set", err, [&] {
        for (size_t w = 0; w < r_.size(); w++) pack(w, parameters[w]);
        return icg_marg_prior_evaluate(ctx_, x_.data(), residuals, jacobians, gradient, sq_norm);
    });
}

void MarginalizationPriorSet::pack(size_t w, const double *const *parameters) {
    double *x = x_.data() + x_off_[w];
    for (int32_t b = block_off_[w]; b < block_off_[w + 1]; b++) {
        memcpy(x, parameters[b - block_off_[w]], sizeof(double) * (size_t) block_size_[(size_t) b]);
        x += block_size_[(size_t) b];
    }
}

bool MarginalizationPriorSet::evaluateResident(double *sq_norm, std::string *err) {
    return residentCall(residentAvailable() ? nullptr : "icg_marg_prior_evaluate_resident", ctx_, "MarginalizationPriorSet::evaluateResident: no set", err,
                        [&] { return icg_marg_prior_evaluate_resident(ctx_, x_.data(), sq_norm); });
}

} // namespace icg
