// MarginalizationInfo on the landmark-eliminated path: the structured plan of a window, its host factors as H / b or as blocks, the deferred
// prior, and the small M3 behind the conditioning guard.  (marginalization.cc holds the bookkeeping and the dense path.)
#include "factors.h"

namespace icg {

const ResidualBlockInfo *MarginalizationInfo::devicePriorCandidate() const {
    for (const auto &factor : factors_) {
        if (onBatch(factor) || factor->lossFunction()) continue;
        const auto *src = dynamic_cast<const MargPriorSource *>(factor->costFunction().get());
        if (!src) continue;
        const MargPriorView &v = src->margPriorView();
        const auto &sizes      = factor->parameterBlockSizes();
        bool fits              = v.r > 0 && v.r == factor->costFunction()->num_residuals() && v.n_blocks == (int) sizes.size();
        for (int b = 0; fits && b < v.n_blocks; b++) fits = v.size[b] == sizes[(size_t) b];
        if (fits) return factor.get(); // (the window's FIRST such prior; a second one stays a host factor)
    }
    return nullptr;
}

bool MarginalizationInfo::evaluateDeferred() {
    ResidualBlockInfo *f = deferred_;
    deferred_            = nullptr;
    return f == nullptr || f->Evaluate();
}

// The marginalized set of GVINS::gvinsMarginalization (ic_gvins.cc:1425-1610) is {pose, mix of the oldest state} + {the inverse depths
// anchored in the oldest keyframe}, and an inverse depth is touched by reprojection factors only.  Hmm is then
//     [ A   B ]   A: the few pose / mix columns (15),  D: DIAGONAL (one 1x1 block per landmark),
//     [ B^T D ]
// and the reference's dense pseudo-inverse of Hmm (eigen-decomposition with a 1e-8 floor, :170-181) equals the plain inverse
// whenever Hmm is safely positive definite.  Then  Hrr - Hrm Hmm^-1 Hmr  can be taken in two exact steps: the landmark block first
// (reciprocals of h_ll: done on the DEVICE together with the assembly, the resident f1 kernels), the small A-block second (the
// reference's own eigen / floor procedure on 15 columns instead of 15 + L).  Guard: every h_ll and every eigenvalue of the reduced
// A-block at least 100 x the reference's floor — otherwise this returns false and the dense path runs.
bool MarginalizationInfo::constructAndEliminateStructured() {
    StructuredPlan plan;
    if (!planStructured(plan)) return false;
    double min_hll = 0;
    if (!batch_->accumulateLandmarkEliminated(plan.camera_column_of, plan.P, plan.H.data(), plan.b.data(), &min_hll)) return false;
    return finishStructured(plan, min_hll);
}

bool MarginalizationInfo::planStructured(StructuredPlan &plan) {
    if (!planLayout(plan)) return false;
    planAccumulate(plan);
    return true;
}

bool MarginalizationInfo::planLayout(StructuredPlan &plan) {
    if (!batch_ || batch_->size() == 0) return false;
    // landmark blocks of the batch: all marginalized, size 1, and touched by batch factors only
    std::unordered_map<long, char> is_lm;
    for (double *p : batch_->landmarkBlocks()) {
        const long id = idOf(p);
        auto it = parameter_block_index_.find(id);
        if (it == parameter_block_index_.end() || it->second >= marginalized_size_ || parameter_block_size_[id] != 1) return false;
        is_lm[id] = 1;
    }
    for (const auto &factor : factors_) {
        const bool on_batch = onBatch(factor);
        for (double *p : factor->parameterBlocks()) {
            const bool lm = is_lm.count(idOf(p)) != 0;
            if (lm && !on_batch) return false; // a host factor on an inverse depth: Hmm's landmark block is not diagonal
        }
        if (!on_batch && dynamic_cast<ReprojectionFactor *>(factor->costFunction().get()) != nullptr) return false;
    }
    // compact camera columns: every non-landmark column of the local ordering, order kept (marginalized ones first)
    const int L = local_size_;
    vector<int> &compact = plan.compact;
    compact.assign((size_t) L, -1);
    {
        vector<char> lm_col((size_t) L, 0);
        for (const auto &kv : is_lm) lm_col[(size_t) parameter_block_index_[kv.first]] = 1;
        int c = 0;
        for (int k = 0; k < L; k++)
            if (!lm_col[(size_t) k]) compact[(size_t) k] = c++;
    }
    const int n_lm = (int) is_lm.size();
    const int P = L - n_lm, m = marginalized_size_ - n_lm, r = remained_size_;
    if (m < 0 || P != m + r) return false;
    plan.P = P, plan.m = m, plan.r = r;
    plan.camera_column_of.clear();
    for (const auto &factor : factors_) {
        if (!onBatch(factor)) continue;
        for (double *p : factor->parameterBlocks())
            if (!is_lm.count(idOf(p))) plan.camera_column_of[p] = compact[(size_t) parameter_block_index_[idOf(p)]];
    }
    return true;
}

void MarginalizationInfo::planAccumulate(StructuredPlan &plan) { // host factors: J^T J / J^T e straight into the compact system
    plan.H.assign((size_t) plan.P * plan.P, 0.0), plan.b.assign((size_t) plan.P, 0.0);
    accumulateHostFactors(plan.compact.data(), plan.P, plan.H.data(), plan.b.data());
}

bool MarginalizationInfo::gatherHostBlocks(const StructuredPlan &plan, HostFactorBlocks &out, const ResidualBlockInfo *prior) {
    // one pass over the factors decides what becomes a block and how large; nothing of `out` is touched before every factor has passed
    struct Block {
        const ResidualBlockInfo *factor;
        int nr, nf;
        bool from_prior; // (the deferred prior has not been evaluated: its residual count is the cost function's, its Jacobian takes no room in J)
    };
    vector<Block> list;
    size_t n_J = 0, n_r = 0, n_c = 0;
    for (const auto &factor : factors_) {
        if (onBatch(factor)) continue;
        const auto &blocks    = factor->parameterBlocks();
        const bool from_prior = factor.get() == prior;
        const size_t nr       = from_prior ? (size_t) factor->costFunction()->num_residuals() : factor->residuals().size();
        if (nr > (size_t) ICG_HOST_PART_MAX_NR) return false;
        size_t nf = 0;
        for (size_t i = 0; i < blocks.size(); i++) {
            for (size_t j = 0; j < i; j++)
                if (blocks[j] == blocks[i]) return false; // (accumulateHostFactors' mirror store is not a block's J^T J for such a factor)
            nf += (size_t) localSize(parameter_block_size_[idOf(blocks[i])]);
        }
        if (nr == 0 || nf == 0) continue;
        list.push_back({factor.get(), (int) nr, (int) nf, from_prior});
        n_J += from_prior ? 0 : nr * nf, n_r += nr, n_c += nf;
    }
    const size_t first_block = out.nr.size(), n_blocks = list.size();
    out.nr.reserve(out.nr.size() + n_blocks), out.nf.reserve(out.nf.size() + n_blocks), out.jac_off.reserve(out.jac_off.size() + n_blocks);
    out.cols.reserve(out.cols.size() + n_c), out.r.reserve(out.r.size() + n_r);
    size_t at = out.J.size();
    out.J.resize(at + n_J);
    for (const Block &B : list) {
        const auto &blocks = B.factor->parameterBlocks();
        const int nr = B.nr, nf = B.nf;
        if (B.from_prior) { // its place in the block list, its columns and its slots in r; J0's columns instead of a Jacobian
            const MargPriorView &v = dynamic_cast<const MargPriorSource *>(B.factor->costFunction().get())->margPriorView();
            for (size_t i = 0; i < blocks.size(); i++) {
                const long id   = idOf(blocks[i]);
                const int local = localSize(parameter_block_size_[id]), first = plan.compact[(size_t) parameter_block_index_[id]];
                for (int x = 0; x < local; x++) out.cols.push_back(first + x), out.prior_cols.push_back(v.index[i] + x);
            }
            out.prior_block = (int) (out.nr.size() - first_block);
            out.nr.push_back(nr), out.nf.push_back(nf), out.jac_off.push_back(HostFactorBlocks::kFromPrior);
            out.r.insert(out.r.end(), (size_t) nr, 0.0);
            continue;
        }
        int c0 = 0;
        for (size_t i = 0; i < blocks.size(); i++) {
            const long id   = idOf(blocks[i]);
            const int size  = parameter_block_size_[id], local = localSize(size);
            const int first = plan.compact[(size_t) parameter_block_index_[id]];
            for (int x = 0; x < local; x++) out.cols.push_back(first + x);
            gatherJacobianColumns(nr, size, local, B.factor->jacobians()[i].data(), nf, c0, &out.J[at]);
            c0 += local;
        }
        out.nr.push_back(nr), out.nf.push_back(nf), out.jac_off.push_back((int64_t) at);
        out.r.insert(out.r.end(), B.factor->residuals().begin(), B.factor->residuals().end());
        at += (size_t) nr * nf;
    }
    return true;
}

bool MarginalizationInfo::planWithBlocks(int *P, int *m, vector<double> *H, vector<double> *b, HostFactorBlocks *blocks) {
    if (!updateParameterBlocksIndex() || !preMarginalization()) return false;
    StructuredPlan plan;
    if (!planStructured(plan)) return false;
    blocks->clear();
    if (!gatherHostBlocks(plan, *blocks)) return false;
    *P = plan.P, *m = plan.m;
    H->swap(plan.H), b->swap(plan.b);
    return true;
}

bool MarginalizationInfo::planWithDeferredPrior(HostFactorBlocks *deferred, HostFactorBlocks *eager, const ResidualBlockInfo **prior_out) {
    if (!updateParameterBlocksIndex()) return false;
    const ResidualBlockInfo *prior = devicePriorCandidate();
    if (prior_out) *prior_out = prior;
    if (!prior || !preMarginalization(prior)) return false;
    StructuredPlan plan;
    if (!planLayout(plan)) return false;
    deferred->clear(), eager->clear();
    if (!prior->residuals().empty() || !gatherHostBlocks(plan, *deferred, prior)) return false; // (deferred: nothing was evaluated)
    return evaluateDeferred() && gatherHostBlocks(plan, *eager);
}

// the first guard (which refuses a NaN as well), then the second step on the m leading columns: the reference's procedure (:170-192) on
// the reduced system behind the second guard.  Hp_ / bp_ are as they were when either guard refuses.
bool MarginalizationInfo::finishStructured(StructuredPlan &plan, double min_hll) {
    if (!(min_hll > STRUCTURED_GUARD)) return false;
    return schurReduceGuarded(plan.P, plan.m, plan.H.data(), plan.b.data(), STRUCTURED_GUARD, Hp_, bp_);
}

} // namespace icg
