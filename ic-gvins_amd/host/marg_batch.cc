// MarginalizationBatch: see marg_batch.h.  Reference: factors/marginalization_info.h:73-101 (marginalization), :153-273 (the steps).
#include "marg_batch.h"
#include "marg_linearize_hip.h"

#include <algorithm>
#include <atomic>
#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <stdexcept>

// A build of this layer on another implementation of the C ABI may not have the entries of the device-resident reduced system: the
// references stay weak (null when absent) and marginalize() refuses by name; the product library links libicgvins_hip.so, which defines them.
#pragma weak icg_marg_linearize_resident
#pragma weak icg_reproj_schur_windows_resident
#pragma weak icg_reproj_host_parts_build
#pragma weak icg_reproj_host_parts_build_prior
#pragma weak icg_reproj_landmark_min_windows

namespace icg {

// the first of the three entries setDeviceReducedSystem needs that this build lacks, nullptr when all are there
static const char *missingReducedSystemEntry() {
    if (&icg_marg_linearize_resident == nullptr) return "icg_marg_linearize_resident";
    if (&icg_reproj_schur_windows_resident == nullptr) return "icg_reproj_schur_windows_resident";
    if (&icg_reproj_host_parts_build == nullptr) return "icg_reproj_host_parts_build";
    return nullptr;
}

bool MarginalizationBatch::deviceReducedSystemAvailable() { return missingReducedSystemEntry() == nullptr; }

// the same for setDevicePrior (icg_marg_prior_set_from_kept is not among them: without it the set ships every prior)
static const char *missingDevicePriorEntry() {
    if (!MarginalizationPriorSet::available()) return "icg_marg_prior_set";
    if (!MarginalizationPriorSet::residentAvailable()) return "icg_marg_prior_evaluate_resident";
    if (&icg_reproj_host_parts_build_prior == nullptr) return "icg_reproj_host_parts_build_prior";
    if (&icg_reproj_landmark_min_windows == nullptr) return "icg_reproj_landmark_min_windows";
    return nullptr;
}

bool MarginalizationBatch::devicePriorAvailable() { return missingDevicePriorEntry() == nullptr; }

MarginalizationBatch::MarginalizationBatch(int device, double huber_delta, int host_threads)
    : factors_(device, host_threads, "MarginalizationBatch"), device_(device), huber_(huber_delta) {}

bool MarginalizationBatch::keepLinearizedAvailable() { return MarginalizationLinearizer::keepAvailable(); }

void MarginalizationBatch::releaseKept() {
    if (kept_id_ != 0) MarginalizationLinearizer::releaseKept(factors_.ctx());
    kept_id_ = 0;
}

MarginalizationBatch::~MarginalizationBatch() {
    releaseKept();
    clear();
    if (dense_ctx_) icg_ctx_destroy(dense_ctx_);
}

void MarginalizationBatch::clear() {
    for (auto &W : windows_)
        if (W->info && W->info->batch_ == W.get()) W->info->batch_ = nullptr; // (an info may outlive the batch: it keeps only its results)
    windows_.clear();
    factors_.clear();
    retired_.clear(); // (the factor records of the windows marginalized since the last clear())
    laid_out_ = false;
}

int MarginalizationBatch::addWindow(const std::shared_ptr<MarginalizationInfo> &info) {
    if (!info) throw std::runtime_error("MarginalizationBatch: null MarginalizationInfo");
    std::unique_ptr<Slice> W(new Slice);
    W->owner = this;
    W->w     = (size_t) factors_.addWindow();
    W->info  = info;
    info->setDeviceFactors(W.get());
    windows_.push_back(std::move(W));
    laid_out_ = false;
    return (int) windows_.size() - 1;
}

void MarginalizationBatch::addReprojectionFactor(int w, const ReprojectionFactor *factor, double *pose_i, double *pose_j, double *extrinsic,
                                                 double *invdepth, double *td) {
    Slice &W = *windows_.at((size_t) w);
    if (!factor || !pose_i || !pose_j || !extrinsic || !invdepth || !td) throw std::runtime_error("MarginalizationBatch: null block");
    if (!factors_.add(w, factor->observation(), pose_i, pose_j, extrinsic, invdepth, td))
        throw std::runtime_error("MarginalizationBatch: one extrinsic / td block per window");
    W.members.insert(factor);
    laid_out_ = false;
}

// a pose block belongs to one window; then the factor set of all windows goes up
bool MarginalizationBatch::layout() {
    std::unordered_map<const double *, size_t> pose_owner;
    for (size_t w = 0; w < windows_.size(); w++)
        for (double *p : factors_.window(w).poses) {
            auto it = pose_owner.find(p);
            if (it != pose_owner.end() && it->second != w) {
                error_ = "a pose block is used by the reprojection factors of two windows";
                return false;
            }
            pose_owner[p] = w;
        }
    laid_out_ = factors_.upload(&error_); // (no factor anywhere — only host factors: nothing for the device, and that is fine)
    return laid_out_;
}

bool MarginalizationBatch::Slice::evaluateCorrected(double huber_delta) {
    if (!evaluated) {
        err = "a window of a MarginalizationBatch is marginalized by MarginalizationBatch::marginalize(), not on its own";
        return false;
    }
    if (huber_delta != owner->huber_) {
        err = "the Huber delta of a window's reprojection factors differs from the batch's";
        return false;
    }
    return true; // (evaluated with every other window's factors, one launch: marginalize() phase 1)
}

bool MarginalizationBatch::Slice::accumulateLandmarkEliminated(const std::unordered_map<const double *, int> &, int, double *, double *, double *) {
    err = "a window of a MarginalizationBatch is marginalized by MarginalizationBatch::marginalize(), not on its own";
    return false;
}

bool MarginalizationBatch::Slice::accumulateNormal(const std::unordered_map<const double *, int> &column_of, int local_size, double *H0, double *b0) {
    return owner->denseNormalOfWindow(*this, column_of, local_size, H0, b0);
}

// The dense M2 of one window (marginalization_info.h:195-230): its factors alone on a one-window context, evaluated there once more (the
// batched evaluation lives in the partitioned context, whose dense assembly would mix the windows' shared columns).
bool MarginalizationBatch::denseNormalOfWindow(Slice &slice, const std::unordered_map<const double *, int> &column_of, int local_size, double *H0,
                                               double *b0) {
    const WindowFactorSet::Window &W = slice.record();
    const int n                      = W.size();
    if (n == 0) return true;
    std::lock_guard<std::mutex> lock(dense_mutex_);
    try {
        if (!dense_ctx_) dense_ctx_ = backendContext(device_, "MarginalizationBatch (dense path)");
    } catch (const std::exception &e) {
        slice.err = e.what();
        return false;
    }
    std::vector<double> obs((size_t) 15 * n);
    for (int k = 0; k < n; k++)
        for (int c = 0; c < 15; c++) obs[(size_t) c * n + k] = W.obs[(size_t) 15 * k + c];
    std::vector<double> poses(7 * W.poses.size()), inv(W.landmarks.size());
    for (size_t k = 0; k < W.poses.size(); k++) memcpy(&poses[7 * k], W.poses[k], sizeof(double) * 7);
    for (size_t k = 0; k < W.landmarks.size(); k++) inv[k] = *W.landmarks[k];
    auto col = [&](const double *p) {
        auto it = column_of.find(p);
        return it == column_of.end() ? -1 : it->second;
    };
    std::vector<int32_t> cp(W.poses.size()), cl(W.landmarks.size());
    for (size_t k = 0; k < W.poses.size(); k++) cp[k] = col(W.poses[k]);
    for (size_t k = 0; k < W.landmarks.size(); k++) cl[k] = col(W.landmarks[k]);
    int rc = icg_reproj_set_factors(dense_ctx_, n, obs.data(), W.idx_i.data(), W.idx_j.data(), W.idx_lm.data());
    if (rc == ICG_OK)
        rc = icg_reproj_eval_resident(dense_ctx_, (int) W.poses.size(), poses.data(), W.ext, (int) W.landmarks.size(), inv.data(), *W.td, 1, huber_,
                                      nullptr, nullptr);
    if (rc == ICG_OK) rc = icg_reproj_accumulate_normal(dense_ctx_, local_size, cp.data(), col(W.ext), cl.data(), col(W.td), H0, b0);
    if (rc != ICG_OK) {
        slice.err = icg_last_error(dense_ctx_);
        return false;
    }
    return true;
}

struct MarginalizationBatch::State {
    bool alive{false}, planned{false};
    MarginalizationInfo::StructuredPlan plan;
    HostFactorBlocks blocks; // setDeviceReducedSystem: the window's host factors, instead of their J^T J in plan.H
};

struct MarginalizationBatch::DeviceM3 {
    std::vector<char> on_device; // per window: its prior is in the arrays below
    std::vector<double> Hp, bp, J0, e0;
    std::vector<size_t> r_off, rr_off;
    std::vector<int> slot; // per window: its index in the device call
    uint64_t keep_id{0};   // setKeepLinearized: the call's kept linearization
};

// what one marginalize() works on, handed from phase to phase
struct MarginalizationBatch::Run {
    const size_t NW;
    std::vector<State> st;
    std::vector<const ResidualBlockInfo *> taken; // setDevicePrior: the prior each window hands over ...
    std::vector<int32_t> prior_in_set;            // ... and its index in the resident set (window order)
    int P = 0;                                        // columns of the widest planned window's reduced system
    std::vector<double> S, s, hll, host_s, min_dev;   // what phase 3 reads back (S and hll, or host_s and min_dev, by the switches)
    std::vector<char> added, structured, good;        // per window: its eliminated part was added; it took the structured path; it has a prior
    std::vector<double> min_hll;                      // the smallest landmark diagonal of a window, for the first guard
    DeviceM3 dev;
    std::chrono::steady_clock::time_point t0, t1, t2, t3, t4;
    // setDeviceReducedSystem: the block lists of the planned windows, concatenated as one icg_reproj_host_parts_build(_prior) call takes them
    struct HostPartCall {
        std::vector<int32_t> Pw, blk_off, nr, nf, cols, prior_of, prior_cols;
        std::vector<uint8_t> rebuild;
        std::vector<int64_t> jac_off;
        std::vector<double> J, r;
    };
    explicit Run(size_t n) : NW(n), st(n), taken(n, nullptr), prior_in_set(n, -1), added(n, 0), structured(n, 0), good(n, 0), min_hll(n, 0.0),
          dev{std::vector<char>(n, 0), {}, {}, {}, {}, std::vector<size_t>(n, 0), std::vector<size_t>(n, 0), std::vector<int>(n, -1), 0} {}
    HostPartCall hostPartCall(bool dev_prior) const {
        HostPartCall C{std::vector<int32_t>(NW, 1), std::vector<int32_t>(NW + 1, 0), {}, {}, {}, {}, {}, std::vector<uint8_t>(NW, 0), {}, {}, {}};
        for (size_t w = 0; w < NW; w++) {
            if (st[w].planned) {
                const HostFactorBlocks &B = st[w].blocks;
                C.Pw[w] = st[w].plan.P, C.rebuild[w] = 1;
                for (int64_t off : B.jac_off) C.jac_off.push_back(off < 0 ? off : (int64_t) C.J.size() + off); // (< 0: ICG_HP_JAC_FROM_PRIOR)
                if (dev_prior) {
                    C.prior_of.insert(C.prior_of.end(), B.nr.size(), -1);
                    if (B.prior_block >= 0) C.prior_of[C.nr.size() + (size_t) B.prior_block] = prior_in_set[w];
                    C.prior_cols.insert(C.prior_cols.end(), B.prior_cols.begin(), B.prior_cols.end());
                }
                C.nr.insert(C.nr.end(), B.nr.begin(), B.nr.end()), C.nf.insert(C.nf.end(), B.nf.begin(), B.nf.end());
                C.cols.insert(C.cols.end(), B.cols.begin(), B.cols.end());
                C.J.insert(C.J.end(), B.J.begin(), B.J.end()), C.r.insert(C.r.end(), B.r.begin(), B.r.end());
            }
            C.blk_off[w + 1] = (int32_t) C.nr.size();
        }
        return C;
    }
};

// device M3 (setDeviceLinearization): every window whose eliminated part was added and that passes the first guard, one call.  resident
// (setDeviceReducedSystem): the windows' systems are formed on the device from what steps 3 left there; only b = host_s + s goes up.
bool MarginalizationBatch::linearizeOnDevice(Run &R, std::string *what) {
    const std::vector<State> &st = R.st;
    DeviceM3 &dev                = R.dev;
    const bool resident          = device_reduced_system_;
    const size_t NW    = st.size();
    const double GUARD = MarginalizationInfo::STRUCTURED_GUARD, EPS = MarginalizationInfo::EPS; // (finishStructured's guard; the floor)
    std::vector<int32_t> dP, dm;
    std::vector<size_t> h_off, who;
    size_t th = 0, tb = 0, tr = 0, trr = 0;
    for (size_t w = 0; w < NW; w++) {
        if (!R.added[w] || !(R.min_hll[w] > GUARD)) continue;
        const MarginalizationInfo::StructuredPlan &plan = st[w].plan;
        dev.on_device[w] = 1, dev.r_off[w] = tr, dev.rr_off[w] = trr;
        dev.slot[w] = (int) who.size();
        who.push_back(w), h_off.push_back(th);
        dP.push_back(plan.P), dm.push_back(plan.m);
        th += (size_t) plan.P * plan.P, tb += (size_t) plan.P, tr += (size_t) plan.r, trr += (size_t) plan.r * plan.r;
    }
    if (who.empty()) return true;
    std::vector<double> dH(resident ? 0 : th), db(tb), dev_min(who.size());
    std::vector<int32_t> dev_status(who.size());
    std::vector<size_t> b_off(who.size(), 0);
    for (size_t k = 1; k < who.size(); k++) b_off[k] = b_off[k - 1] + (size_t) dP[k - 1];
    dev.Hp.resize(trr), dev.bp.resize(tr), dev.J0.resize(trr), dev.e0.resize(tr);
    if (resident) {
        std::vector<int32_t> win(who.size());
        for (size_t k = 0; k < who.size(); k++) {
            const size_t w = who[k], at = w * (size_t) R.P;
            win[k]         = (int32_t) w;
            for (int i = 0; i < dP[k]; i++) db[b_off[k] + (size_t) i] = R.host_s[at + (size_t) i] + R.s[at + (size_t) i]; // (plan.b += s)
        }
        uint64_t id = 0;
        if (icg_marg_linearize_resident(factors_.ctx(), R.P, (int) who.size(), win.data(), dP.data(), dm.data(), db.data(), EPS, dev.Hp.data(),
                                        dev.bp.data(), dev.J0.data(), dev.e0.data(), nullptr, dev_min.data(), dev_status.data(), nullptr,
                                        keep_linearized_ ? &id : nullptr) != ICG_OK) {
            *what = icg_last_error(factors_.ctx());
            return false;
        }
        dev.keep_id = id;
    } else {
        factors_.forEachWindow(who.size(), [&](size_t k) {
            const MarginalizationInfo::StructuredPlan &plan = st[who[k]].plan;
            memcpy(&dH[h_off[k]], plan.H.data(), sizeof(double) * plan.H.size());
            memcpy(&db[b_off[k]], plan.b.data(), sizeof(double) * plan.b.size());
        });
        MarginalizationLinearizer lin(true, factors_.ctx());
        if (keep_linearized_) {
            dev.keep_id = lin.linearizeKeep((int) who.size(), dP.data(), dm.data(), dH.data(), db.data(), EPS, dev.Hp.data(), dev.bp.data(), dev.J0.data(),
                                            dev.e0.data(), nullptr, dev_min.data(), dev_status.data(), what);
            if (dev.keep_id == 0) return false;
        } else if (!lin.linearize((int) who.size(), dP.data(), dm.data(), dH.data(), db.data(), EPS, dev.Hp.data(), dev.bp.data(), dev.J0.data(),
                                  dev.e0.data(), nullptr, dev_min.data(), dev_status.data(), what)) {
            return false;
        }
    }
    for (size_t k = 0; k < who.size(); k++) // second guard of finishStructured, and a solver that did not converge
        if (!(dev_min[k] > GUARD) || (dev_status[k] & 1)) dev.on_device[who[k]] = 0;
    return true;
}

// a window that has no valid prior after this call
void MarginalizationBatch::invalidate(MarginalizationInfo &I) {
    I.isvalid_ = false;
    I.releaseMemory();
}

// a device call all windows share failed: no window stays evaluated
bool MarginalizationBatch::fail(const std::string &what) {
    error_ = what;
    for (auto &W : windows_) W->evaluated = false;
    return false;
}

// ---- 1: every window's reprojection factors, one launch (residual_block_info.h:44-88 with the corrector :59-87 on the device) -------------
bool MarginalizationBatch::evaluateWindows(Run &R) {
    icg_ctx *ctx = factors_.ctx();
    // setDevicePrior: the resident set of the priors the windows hand over.  The set copies J0 / e0 — from the kept linearization where the
    // views are tagged with it — so it is built before anything drops that linearization: the release here, and
    // icg_marg_linearize_resident in step 4.
    if (device_prior_) {
        std::vector<MargPriorView> views;
        for (size_t w = 0; w < R.NW; w++) {
            const ResidualBlockInfo *f = windows_[w]->info->devicePriorCandidate();
            if (!f) continue;
            const MargPriorView &v = dynamic_cast<const MargPriorSource *>(f->costFunction().get())->margPriorView();
            if (v.r > ICG_MARG_MAX_R) continue; // (wider than a resident prior may be: it stays a host factor)
            R.taken[w] = f, R.prior_in_set[w] = (int32_t) views.size();
            views.push_back(v);
        }
        std::string what;
        if (!views.empty() && !prior_set_.set(ctx, views, &what)) return fail(what);
        n_device_priors_    = (int) views.size();
        n_priors_from_kept_ = views.empty() ? 0 : prior_set_.handedOff();
        releaseKept();
    }
    if (factors_.numFactors() > 0) {
        std::vector<double> poses, ext, inv, td;
        factors_.gather(poses, ext, inv, td);
        if (icg_reproj_eval_windows(ctx, factors_.numPoses(), poses.data(), ext.data(), factors_.numLandmarks(), inv.data(), td.data(), 1, huber_) != ICG_OK)
            return fail(icg_last_error(ctx));
    }
    for (auto &W : windows_) W->evaluated = true;
    return true;
}

// ---- 2: M1 bookkeeping, host factors, compact camera layout per window -------------------------------------------------------------------
void MarginalizationBatch::bookkeeping(Run &R) {
    const bool force_dense = MarginalizationInfo::denseForced();
    factors_.forEachWindow(R.NW, [&](size_t w) {
        MarginalizationInfo &I = *windows_[w]->info;
        State &T               = R.st[w];
        // (setDevicePrior: the point the taken prior is evaluated at on the device — the values its Evaluate() would read here; the factor
        // itself is deferred, its blocks are still snapshot)
        if (R.taken[w]) prior_set_.pack((size_t) R.prior_in_set[w], R.taken[w]->parameterBlocks().data());
        if (!I.updateParameterBlocksIndex() || !I.preMarginalization(R.taken[w])) return invalidate(I); // (:75-86: nothing to marginalize / an evaluation failed)
        T.alive = true;
        if (device_reduced_system_) // (layout and gather only: the blocks' J^T J is formed on the device in step 3)
            T.planned = !force_dense && I.planLayout(T.plan) && I.gatherHostBlocks(T.plan, T.blocks, R.taken[w]);
        else
            T.planned = !force_dense && I.planStructured(T.plan);
    });
}

// ---- 3: assembly + landmark elimination of every planned window, one launch sequence; the landmark diagonals ------------------------------
// (csrc/reproj_schur.hip, schur_impl: reduced systems of up to kMaxCameraColumns columns; a wider window takes the dense path on its own)
bool MarginalizationBatch::assembleAndEliminate(Run &R) {
    const size_t NW   = R.NW;
    std::vector<State> &st = R.st;
    icg_ctx *ctx      = factors_.ctx();
    for (size_t w = 0; w < NW; w++) {
        if (!st[w].planned) continue;
        const WindowFactorSet::Window &W = factors_.window(w);
        int V                            = 0;
        for (double *p : W.poses) V += st[w].plan.camera_column_of.count(p) ? 6 : 0;
        V += (W.ext && st[w].plan.camera_column_of.count(W.ext) ? 6 : 0) + (W.td && st[w].plan.camera_column_of.count(W.td) ? 1 : 0);
        if (V > kMaxCameraColumns) st[w].planned = false;
    }
    for (size_t w = 0; w < NW; w++)
        if (st[w].planned) R.P = std::max(R.P, st[w].plan.P);
    const int P = R.P;
    if (P == 0) return true;
    std::vector<int32_t> col_pose((size_t) factors_.numPoses(), -1), col_ext(NW, -1), col_td(NW, -1);
    for (size_t w = 0; w < NW; w++) {
        if (!st[w].planned) continue; // (its columns stay constant: the window adds nothing to any reduced system that is read)
        const WindowFactorSet::Window &W = factors_.window(w);
        auto col                         = [&](const double *p) {
            auto it = st[w].plan.camera_column_of.find(p);
            return it == st[w].plan.camera_column_of.end() ? -1 : it->second;
        };
        for (size_t k = 0; k < W.poses.size(); k++) col_pose[(size_t) W.pose_begin + k] = col(W.poses[k]);
        col_ext[w] = col(W.ext), col_td[w] = col(W.td);
    }
    std::vector<uint8_t> reassemble(NW, 1);
    std::vector<double> damp(NW, 0.0), diag_cc(NW * (size_t) P), cost(NW, 0.0);
    R.s.assign(NW * (size_t) P, 0.0), R.hll.assign((size_t) std::max(factors_.numLandmarks(), 1), 0.0);
    if (!device_reduced_system_) {
        R.S.assign(NW * (size_t) P * P, 0.0);
        if (icg_reproj_schur_windows(ctx, P, col_pose.data(), col_ext.data(), col_td.data(), nullptr, reassemble.data(), damp.data(), 0.0, 0.0, R.S.data(),
                                     R.s.data(), diag_cc.data(), cost.data()) != ICG_OK ||
            icg_reproj_landmark_diag_windows(ctx, R.hll.data()) != ICG_OK)
            return fail(icg_last_error(ctx));
        return true;
    }
    // S stays on the device; the host-factor part of every planned window is built beside it from the window's blocks
    Run::HostPartCall C = R.hostPartCall(device_prior_);
    std::vector<double> host_diag(NW * (size_t) P, 0.0);
    R.host_s.assign(NW * (size_t) P, 0.0);
    if (icg_reproj_schur_windows_resident(ctx, P, col_pose.data(), col_ext.data(), col_td.data(), nullptr, reassemble.data(), damp.data(), 0.0, 0.0,
                                          R.s.data(), diag_cc.data(), cost.data()) != ICG_OK)
        return fail(icg_last_error(ctx));
    if (device_prior_) {
        // the taken priors are evaluated where they lie (e = e0 + J0 dx at the packed point, between the Schur call and the host parts), their
        // blocks take residual and Jacobian columns from there, and the first guard's minimum comes back as one double per window
        std::vector<double> sq((size_t) std::max(n_device_priors_, 1));
        std::string what;
        if (n_device_priors_ > 0 && !prior_set_.evaluateResident(sq.data(), &what)) return fail(what);
        R.min_dev.assign(NW, 0.0);
        if (icg_reproj_host_parts_build_prior(ctx, P, C.Pw.data(), C.rebuild.data(), C.blk_off.data(), C.nr.data(), C.nf.data(), C.cols.data(), C.jac_off.data(),
                                              C.J.data(), C.r.data(), R.host_s.data(), host_diag.data(), nullptr,
                                              n_device_priors_ > 0 ? C.prior_of.data() : nullptr, C.prior_cols.data()) != ICG_OK ||
            icg_reproj_landmark_min_windows(ctx, R.min_dev.data()) != ICG_OK)
            return fail(icg_last_error(ctx));
    } else if (icg_reproj_host_parts_build(ctx, P, C.Pw.data(), C.rebuild.data(), C.blk_off.data(), C.nr.data(), C.nf.data(), C.cols.data(), C.jac_off.data(),
                                           C.J.data(), C.r.data(), R.host_s.data(), host_diag.data(), nullptr) != ICG_OK ||
               icg_reproj_landmark_diag_windows(ctx, R.hll.data()) != ICG_OK)
        return fail(icg_last_error(ctx));
    return true;
}

// the landmark-eliminated device part joins the window's compact system; the smallest landmark diagonal for the first guard
void MarginalizationBatch::addEliminated(Run &R, size_t w) {
    const WindowFactorSet::Window &W          = factors_.window(w);
    MarginalizationInfo::StructuredPlan &plan = R.st[w].plan;
    const int Pw = plan.P, P = R.P;
    if (!device_reduced_system_) { // (resident: the sum is formed on the device, icg_marg_linearize_resident)
        const double *Sw = &R.S[w * (size_t) P * P], *sw = &R.s[w * (size_t) P];
        for (int i = 0; i < Pw; i++) {
            for (int j = 0; j < Pw; j++) plan.H[(size_t) i * Pw + j] += Sw[(size_t) i * P + j];
            plan.b[(size_t) i] += sw[i];
        }
    }
    if (device_prior_) { // (reduced on the device, icg_reproj_landmark_min_windows: the value of the loop below)
        R.min_hll[w] = R.min_dev[w];
    } else {
        double mn = W.landmarks.empty() ? 0.0 : R.hll[(size_t) W.lm_begin];
        for (size_t l = 0; l < W.landmarks.size(); l++) mn = std::min(mn, R.hll[(size_t) W.lm_begin + l]);
        R.min_hll[w] = mn;
    }
    R.added[w] = 1;
}

// ---- 4: guard + M3 on the camera block (or the dense M2 + M3), linearization --------------------------------------------------------------
bool MarginalizationBatch::guardAndLinearize(Run &R) {
    const size_t NW        = R.NW;
    std::vector<State> &st = R.st;
    const DeviceM3 &dev    = R.dev;
    if (device_linearization_) {
        factors_.forEachWindow(NW, [&](size_t w) {
            if (st[w].alive && st[w].planned) addEliminated(R, w);
        });
        std::string what;
        if (!linearizeOnDevice(R, &what)) return fail(what);
        kept_id_ = dev.keep_id;
    }
    std::atomic<int> n_deferred{0};
    factors_.forEachWindow(NW, [&](size_t w) {
        if (!st[w].alive) return;
        MarginalizationInfo &I = *windows_[w]->info;
        if (dev.on_device[w]) {
            const size_t r = (size_t) st[w].plan.r, at = dev.r_off[w], at2 = dev.rr_off[w];
            I.Hp_.assign(dev.Hp.begin() + (long) at2, dev.Hp.begin() + (long) (at2 + r * r));
            I.bp_.assign(dev.bp.begin() + (long) at, dev.bp.begin() + (long) (at + r));
            I.linearized_jacobians_.assign(dev.J0.begin() + (long) at2, dev.J0.begin() + (long) (at2 + r * r));
            I.linearized_residuals_.assign(dev.e0.begin() + (long) at, dev.e0.begin() + (long) (at + r));
            I.setKeptLinearization(dev.keep_id, dev.keep_id ? dev.slot[w] : -1); // (what the device call kept is this window's prior)
            R.structured[w] = R.good[w] = 1;
            return;
        }
        bool done = false;
        if (st[w].planned && !device_reduced_system_) { // (resident: there is no H on the host to finish from — the window takes the dense path)
            if (!R.added[w]) addEliminated(R, w);
            done            = I.finishStructured(st[w].plan, R.min_hll[w]);
            R.structured[w] = done ? 1 : 0;
        }
        if (!done) {
            // (setDevicePrior: the window left the structured device path, so its prior is evaluated on the pool after all — only here)
            if (R.taken[w] && (n_deferred++, !I.evaluateDeferred())) return invalidate(I);
            if (!I.constructEquation()) return invalidate(I); // (:88-92 with the window's own dense assembly on the device)
            I.schurElimination();
        }
        I.linearization();
        R.good[w] = 1;
    });
    // (:99) the factor records of the windows that went through are retired: kept by this batch until clear() / destruction (factors.h
    // MarginalizationInfo::releaseMemory: freeing ~3 300 heap blocks per window in line is 45 of the 90 ms of 256 C2 windows)
    for (size_t w = 0; w < NW; w++)
        if (R.good[w]) windows_[w]->info->releaseMemoryInto(retired_);
    n_deferred_evaluations_ = n_deferred.load();
    return true;
}

bool MarginalizationBatch::marginalize(std::vector<char> *ok) {
    const size_t NW = windows_.size();
    if (ok) ok->assign(NW, 0);
    n_structured_ = n_dense_ = 0;
    phase_ms_[0] = phase_ms_[1] = phase_ms_[2] = phase_ms_[3] = 0;
    n_device_priors_ = n_priors_from_kept_ = n_deferred_evaluations_ = 0;
    error_.clear();
    window_error_.clear();
    // what the switches need of each other and of the build, in this order (no window is evaluated yet: fail() only sets the message)
    if (device_prior_ && !device_reduced_system_)
        return fail("setDevicePrior(true) needs setDeviceReducedSystem(true): the resident prior is read by the device call that builds the host-factor parts");
    if (device_prior_ && !devicePriorAvailable()) return fail(std::string(missingDevicePriorEntry()) + " is not in this build");
    if (device_reduced_system_ && !device_linearization_)
        return fail("setDeviceReducedSystem(true) needs setDeviceLinearization(true): the resident reduced systems are read by the device call's linearization");
    if (device_reduced_system_ && !deviceReducedSystemAvailable()) return fail(std::string(missingReducedSystemEntry()) + " is not in this build");
    if (keep_linearized_ && !device_linearization_)
        return fail("setKeepLinearized(true) needs setDeviceLinearization(true): what is kept is the device call's linearization");
    if (keep_linearized_ && !keepLinearizedAvailable()) return fail("icg_marg_linearize_batch_keep is not in this build");
    if (NW == 0) return true;
    // (the last marginalize()'s; this one keeps its own below.  setDevicePrior: the resident set is built from it first, in phase 1)
    if (!device_prior_) releaseKept();
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto ms  = [](auto a, auto b) { return std::chrono::duration<double, std::milli>(b - a).count(); };
    const auto t_layout = now();
    if (!laid_out_ && !layout()) return false;
    const double layout_ms = ms(t_layout, now());
    Run R(NW);
    R.t0 = now();
    if (!evaluateWindows(R)) return false;
    R.t1 = now(), bookkeeping(R), R.t2 = now();
    if (!assembleAndEliminate(R)) return false;
    R.t3 = now();
    if (!guardAndLinearize(R)) return false;
    R.t4 = now();
    for (size_t w = 0; w < NW; w++) {
        windows_[w]->evaluated = false;
        if (R.good[w]) (R.structured[w] ? n_structured_ : n_dense_)++;
        if (ok) (*ok)[w] = R.good[w];
        // (a window that failed on its own — its dense path left a message — is reported through ok[w] and windowError() only: the other
        // windows' priors are good, as they are when every stream marginalizes alone and one of them logs "no valid prior")
        if (!R.good[w] && R.st[w].alive && window_error_.empty() && !windows_[w]->err.empty())
            window_error_ = "window " + std::to_string(w) + ": " + windows_[w]->err;
    }
    phase_ms_[0] = ms(R.t0, R.t1), phase_ms_[1] = ms(R.t1, R.t2), phase_ms_[2] = ms(R.t2, R.t3), phase_ms_[3] = ms(R.t3, R.t4);
    if (getenv("ICG_MARG_DEBUG"))
        fprintf(stderr, "[marginalization batch] %zu windows (%d structured, %d dense): evaluate %.3f ms, bookkeeping + host factors %.3f ms, assemble + eliminate %.3f ms, M3 + linearize %.3f ms; layout (factor upload + partition) %.3f ms\n",
                NW, n_structured_, n_dense_, phase_ms_[0], phase_ms_[1], phase_ms_[2], phase_ms_[3], layout_ms);
    return true; // (false above: a launch all windows share failed)
}

} // namespace icg
