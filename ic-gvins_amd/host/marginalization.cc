// Host side of the back-end boundary: the factor records, MarginalizationInfo's bookkeeping and dense path, and the linearized prior
// (see factors.h for the reference lines each class mirrors).  The landmark-eliminated path is marginalization_structured.cc.
#include "factors.h"

#include <atomic>
#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>

namespace icg {

// ---- ResidualBlockInfo (generic host path) ------------------------------------------------------------------------------
bool ResidualBlockInfo::Evaluate() {
    const int nr = cost_function_->num_residuals();
    residuals_.assign((size_t) nr, 0.0);
    const vector<int32_t> &block_sizes = cost_function_->parameter_block_sizes();
    vector<double *> raw(block_sizes.size());
    jacobians_.resize(block_sizes.size());
    for (size_t i = 0; i < block_sizes.size(); i++) {
        jacobians_[i].assign((size_t) nr * block_sizes[i], 0.0);
        raw[i] = jacobians_[i].data();
    }
    if (!cost_function_->Evaluate(parameter_blocks_.data(), residuals_.data(), raw.data())) return false;
    if (loss_function_) { // Ceres corrector (residual_block_info.h:59-87)
        double sq_norm = 0, rho[3];
        for (double v : residuals_) sq_norm += v * v;
        loss_function_->Evaluate(sq_norm, rho);
        const CorrectorScalars cs = correctorScalars(sq_norm, rho);
        const double sqrt_rho1 = cs.sqrt_rho1, alpha_sq_norm = cs.alpha_sq_norm, residual_scaling = cs.residual_scaling;
        for (size_t i = 0; i < jacobians_.size(); i++) {
            const int nc = block_sizes[i];
            for (int c = 0; c < nc; c++) {
                double rtj = 0;
                for (int k = 0; k < nr; k++) rtj += residuals_[(size_t) k] * jacobians_[i][(size_t) k * nc + c];
                for (int k = 0; k < nr; k++) {
                    double &j = jacobians_[i][(size_t) k * nc + c];
                    j         = sqrt_rho1 * (j - alpha_sq_norm * residuals_[(size_t) k] * rtj);
                }
            }
        }
        for (double &v : residuals_) v *= residual_scaling;
    }
    return true;
}

// ---- MarginalizationInfo ------------------------------------------------------------------------------------------------
MarginalizationInfo::~MarginalizationInfo() {
    for (auto &block : parameter_block_data_) delete[] block.second;
}

void MarginalizationInfo::addResidualBlockInfo(const std::shared_ptr<ResidualBlockInfo> &blockinfo) { // :53-67
    factors_.push_back(blockinfo);
    const auto &parameter_blocks = blockinfo->parameterBlocks();
    const auto &block_sizes      = blockinfo->parameterBlockSizes();
    for (size_t k = 0; k < parameter_blocks.size(); k++) parameter_block_size_[idOf(parameter_blocks[k])] = block_sizes[k];
    for (int index : blockinfo->marginalizationParametersIndex()) parameter_block_index_[idOf(parameter_blocks[(size_t) index])] = 0;
}

namespace {
thread_local double g_marg_phase_ms[4] = {0, 0, 0, 0};
thread_local bool g_marg_structured   = false;
// process-wide switch (diagnostics / tests): force the reference's dense M2 + M3 even where the structured path applies
std::atomic<int> g_marg_force_dense{0};
}
const double *MarginalizationInfo::lastPhaseMs() { return g_marg_phase_ms; }
bool MarginalizationInfo::lastWasStructured() { return g_marg_structured; }
void MarginalizationInfo::forceDense(bool on) { g_marg_force_dense.store(on ? 1 : 0); }
bool MarginalizationInfo::denseForced() { return g_marg_force_dense.load() != 0; }

bool MarginalizationInfo::marginalization() { // :73-101
    if (!updateParameterBlocksIndex()) {
        isvalid_ = false;
        releaseMemory();
        return false;
    }
    const bool dbg = getenv("ICG_MARG_DEBUG") != nullptr;
    auto now       = [] { return std::chrono::steady_clock::now(); };
    auto ms        = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
        return std::chrono::duration<double, std::milli>(b - a).count();
    };
    auto t0 = now();
    if (!preMarginalization()) {
        isvalid_ = false;
        releaseMemory();
        return false;
    }
    auto t1 = now();
    auto t2 = t1;
    g_marg_structured = g_marg_force_dense.load() == 0 && constructAndEliminateStructured();
    if (!g_marg_structured) {
        if (!constructEquation()) {
            isvalid_ = false;
            releaseMemory();
            return false;
        }
        t2 = now();
        schurElimination();
    } else {
        t2 = now(); // (structured path: assembly and elimination are one step, booked under "construct")
    }
    auto t3 = now();
    linearization();
    auto t4 = now();
    g_marg_phase_ms[0] = ms(t0, t1), g_marg_phase_ms[1] = ms(t1, t2), g_marg_phase_ms[2] = ms(t2, t3), g_marg_phase_ms[3] = ms(t3, t4);
    if (dbg)
        fprintf(stderr, "[marginalization] m=%d r=%d: evaluate %.3f ms, construct %.3f ms, schur %.3f ms, linearize %.3f ms\n", marginalized_size_,
                remained_size_, ms(t0, t1), ms(t1, t2), ms(t2, t3), ms(t3, t4));
    releaseMemory();
    return true;
}

vector<double *> MarginalizationInfo::getParamterBlocks(std::unordered_map<long, double *> &address) { // :103-122
    vector<double *> remained_block_addr;
    remained_block_data_.clear();
    remained_block_index_.clear();
    remained_block_size_.clear();
    for (const auto &block : parameter_block_index_) {
        if (block.second >= marginalized_size_) {
            remained_block_data_.push_back(parameter_block_data_[block.first]);
            remained_block_size_.push_back(parameter_block_size_[block.first]);
            remained_block_index_.push_back(parameter_block_index_[block.first]);
            remained_block_addr.push_back(address[block.first]);
        }
    }
    return remained_block_addr;
}

bool MarginalizationInfo::updateParameterBlocksIndex() { // :232-253
    int index = 0;
    for (auto &block : parameter_block_index_) {
        block.second = index;
        index += localSize(parameter_block_size_[block.first]);
    }
    marginalized_size_ = index;
    for (const auto &block : parameter_block_size_) {
        if (parameter_block_index_.find(block.first) == parameter_block_index_.end()) {
            parameter_block_index_[block.first] = index;
            index += localSize(block.second);
        }
    }
    remained_size_ = index - marginalized_size_;
    local_size_    = index;
    return marginalized_size_ > 0;
}

bool MarginalizationInfo::onBatch(const std::shared_ptr<ResidualBlockInfo> &f) const {
    if (!batch_) return false;
    auto *rf = dynamic_cast<ReprojectionFactor *>(f->costFunction().get());
    if (rf == nullptr || !batch_->owns(rf)) return false;
    return f->lossFunction() == nullptr || dynamic_cast<HuberLossHip *>(f->lossFunction().get()) != nullptr;
}

bool MarginalizationInfo::preMarginalization(const ResidualBlockInfo *defer) { // :256-273
    // every reprojection factor of the batch: ONE device launch incl. the robust correction
    double delta = 0;
    for (const auto &factor : factors_)
        if (onBatch(factor)) {
            auto *hl = dynamic_cast<HuberLossHip *>(factor->lossFunction().get());
            delta    = hl ? hl->delta() : 0.0;
            break;
        }
    if (batch_ && batch_->size() > 0 && !batch_->evaluateCorrected(delta)) return false;
    deferred_ = nullptr;
    for (const auto &factor : factors_) {
        if (factor.get() == defer) // (its blocks are snapshot below like every factor's; evaluateDeferred() runs the evaluation if it is needed)
            deferred_ = factor.get();
        else if (!onBatch(factor) && !factor->Evaluate())
            return false;
        const vector<int32_t> &block_sizes = factor->parameterBlockSizes();
        for (size_t k = 0; k < block_sizes.size(); k++) {
            long id  = idOf(factor->parameterBlocks()[k]);
            int size = block_sizes[k];
            if (parameter_block_data_.find(id) == parameter_block_data_.end()) {
                auto *data = new double[(size_t) size];
                memcpy(data, factor->parameterBlocks()[k], sizeof(double) * (size_t) size);
                parameter_block_data_[id] = data;
            }
        }
    }
    return true;
}

// Each cell of a block pair (i, j >= i) is summed over k ascending from zero and added to H; for i != j the mirror cell is STORED from it
// (a factor that lists a parameter block twice is handled by this order of stores, which is why this is not the block form J^T J of
// gatherHostBlocks); then b -= J_i^T e.
void MarginalizationInfo::accumulateHostFactors(const int *column_of_local, int stride, double *H, double *b) {
    const size_t L = (size_t) stride;
    auto first     = [&](double *block) {
        const int local = parameter_block_index_[idOf(block)];
        return column_of_local ? column_of_local[local] : local;
    };
    for (const auto &factor : factors_) {
        if (onBatch(factor)) continue;
        const auto &blocks = factor->parameterBlocks();
        const int nr       = (int) factor->residuals().size();
        for (size_t i = 0; i < blocks.size(); i++) {
            const int row0 = first(blocks[i]);
            const int gi   = parameter_block_size_[idOf(blocks[i])];
            const int rows = localSize(gi);
            const vector<double> &Ji = factor->jacobians()[i];
            for (size_t j = i; j < blocks.size(); ++j) {
                const int col0 = first(blocks[j]);
                const int gj   = parameter_block_size_[idOf(blocks[j])];
                const int cols = localSize(gj);
                const vector<double> &Jj = factor->jacobians()[j];
                for (int x = 0; x < rows; x++)
                    for (int y = 0; y < cols; y++) {
                        double s = 0;
                        for (int k = 0; k < nr; k++) s += Ji[(size_t) k * gi + x] * Jj[(size_t) k * gj + y];
                        H[(size_t) (row0 + x) * L + col0 + y] += s;
                        if (i != j) H[(size_t) (col0 + y) * L + row0 + x] = H[(size_t) (row0 + x) * L + col0 + y];
                    }
            }
            for (int x = 0; x < rows; x++) {
                double s = 0;
                for (int k = 0; k < nr; k++) s += Ji[(size_t) k * gi + x] * factor->residuals()[(size_t) k];
                b[(size_t) row0 + x] -= s;
            }
        }
    }
}

bool MarginalizationInfo::constructEquation() { // :195-230
    const size_t L = (size_t) local_size_;
    H0_.assign(L * L, 0.0);
    b0_.assign(L, 0.0);
    accumulateHostFactors(nullptr, local_size_, H0_.data(), b0_.data());
    std::unordered_map<const double *, int> column_of;
    bool any_device = false;
    for (const auto &factor : factors_) {
        if (!onBatch(factor)) continue;
        any_device = true;
        for (double *p : factor->parameterBlocks()) column_of[p] = parameter_block_index_[idOf(p)];
    }
    if (any_device && !batch_->accumulateNormal(column_of, local_size_, H0_.data(), b0_.data())) return false;
    return true;
}

void MarginalizationInfo::schurElimination() { // :170-192
    schurReduce(local_size_, marginalized_size_, H0_.data(), b0_.data(), EPS, Hp_, bp_, nullptr, nullptr);
}

void MarginalizationInfo::linearization() { // :153-167
    linearizePrior(remained_size_, Hp_, bp_, EPS, linearized_jacobians_, linearized_residuals_, nullptr, nullptr);
    keep_id_ = 0, keep_slot_ = -1; // (a linearization made here lies on the host only)
}

// ---- MarginalizationFactor (marginalization_factor.h:31-105) ----------------------------------------------------------
MarginalizationFactor::MarginalizationFactor(std::shared_ptr<MarginalizationInfo> marg_info) : marg_info_(std::move(marg_info)) {
    for (auto size : marg_info_->remainedBlockSize()) mutable_parameter_block_sizes()->push_back(size);
    set_num_residuals(marg_info_->remainedSize());
    // The view Evaluate reads, fixed here like the block sizes above.  The remained-block lists are COPIED: getParamterBlocks() clears and
    // refills them in the info, and the factor keeps describing the blocks it was built for.  The linearization points they name, J0 and e0
    // stay the info's own arrays, which change only in marginalization(): a factor is built from an info after its marginalization() and
    // getParamterBlocks(), as the estimator does, and the info is not marginalized again while a factor reads it.
    const int marginalizaed_size = marg_info_->marginalizedSize();
    size_                        = marg_info_->remainedBlockSize();
    for (int i : marg_info_->remainedBlockIndex()) index_.push_back(i - marginalizaed_size);
    x0_.assign(marg_info_->remainedBlockData().begin(), marg_info_->remainedBlockData().end());
    view_.r        = marg_info_->remainedSize();
    view_.n_blocks = (int) size_.size();
    view_.size     = size_.data();
    view_.index    = index_.data();
    view_.x0       = x0_.data();
    view_.J0       = marg_info_->linearizedJacobians().data();
    view_.e0       = marg_info_->linearizedResiduals().data();
    view_.keep_id = marg_info_->keptId(), view_.keep_slot = marg_info_->keptSlot();
}

bool MarginalizationFactor::Evaluate(const double *const *parameters, double *residuals, double **jacobians) const {
    evaluateMargPrior(view_, parameters, residuals, jacobians);
    return true;
}

void evaluateMargPrior(const MargPriorView &view, const double *const *parameters, double *residuals, double **jacobians) {
    const int remained_size = view.r;
    const double *J0 = view.J0, *e0 = view.e0;
    vector<double> dx((size_t) remained_size, 0.0);
    for (int i = 0; i < view.n_blocks; i++) {
        const int size = view.size[i], index = view.index[i];
        const double *x = parameters[i], *x0 = view.x0[i];
        if (size == POSE_GLOBAL_SIZE) { // :64-72
            const double n2 = x0[3] * x0[3] + x0[4] * x0[4] + x0[5] * x0[5] + x0[6] * x0[6];
            const double ax = -x0[3] / n2, ay = -x0[4] / n2, az = -x0[5] / n2, aw = x0[6] / n2;
            const double bx = x[3], by = x[4], bz = x[5], bw = x[6];
            const double dqx = aw * bx + ax * bw + ay * bz - az * by;
            const double dqy = aw * by + ay * bw + az * bx - ax * bz;
            const double dqz = aw * bz + az * bw + ax * by - ay * bx;
            const double dqw = aw * bw - ax * bx - ay * by - az * bz;
            for (int k = 0; k < 3; k++) dx[(size_t) index + k] = x[k] - x0[k];
            const double sgn      = dqw < 0 ? -2.0 : 2.0;
            dx[(size_t) index + 3] = sgn * dqx;
            dx[(size_t) index + 4] = sgn * dqy;
            dx[(size_t) index + 5] = sgn * dqz;
        } else {
            for (int k = 0; k < size; k++) dx[(size_t) index + k] = x[k] - x0[k];
        }
    }
    for (int i = 0; i < remained_size; i++) { // e = e0 + J0 * dx  (:79-80)
        double s = 0;
        for (int k = 0; k < remained_size; k++) s += J0[(size_t) i * remained_size + k] * dx[(size_t) k];
        residuals[i] = e0[(size_t) i] + s;
    }
    if (jacobians) {
        for (int b = 0; b < view.n_blocks; b++) {
            if (!jacobians[b]) continue;
            const int size = view.size[b], index = view.index[b];
            const int local_size = MarginalizationInfo::localSize(size);
            for (int i = 0; i < remained_size; i++)
                for (int j = 0; j < size; j++)
                    jacobians[b][(size_t) i * size + j] = j < local_size ? J0[(size_t) i * remained_size + index + j] : 0.0;
        }
    }
}

} // namespace icg
