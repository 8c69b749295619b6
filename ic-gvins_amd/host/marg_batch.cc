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

struct MarginalizationBatch::ReducedRhs {
    int P;
    const std::vector<double> &s, &host_s;
};

struct MarginalizationBatch::DeviceM3 {
    std::vector<char> on_device; // per window: its prior is in the arrays below
    std::vector<double> Hp, bp, J0, e0;
    std::vector<size_t> r_off, rr_off;
    std::vector<int> slot; // per window: its index in the device call
    uint64_t keep_id{0};   // setKeepLinearized: the call's kept linearization
};

// device M3 (setDeviceLinearization): every window whose eliminated part was added and that passes the first guard, one call.  resident
// (setDeviceReducedSystem): the windows' systems are formed on the device from what steps 3 left there; only b = host_s + s goes up.
bool MarginalizationBatch::linearizeOnDevice(const std::vector<State> &st, const std::vector<char> &added, const std::vector<double> &min_hll,
                                             DeviceM3 &dev, std::string *what, const ReducedRhs *resident) {
    const size_t NW    = st.size();
    const double GUARD = 100.0 * 1e-8; // (finishStructured: 100 x the reference's floor)
    std::vector<int32_t> dP, dm;
    std::vector<size_t> h_off, who;
    size_t th = 0, tb = 0, tr = 0, trr = 0;
    for (size_t w = 0; w < NW; w++) {
        if (!added[w] || !(min_hll[w] > GUARD)) continue;
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
            const size_t w = who[k], at = w * (size_t) resident->P;
            win[k]         = (int32_t) w;
            for (int i = 0; i < dP[k]; i++) db[b_off[k] + (size_t) i] = resident->host_s[at + (size_t) i] + resident->s[at + (size_t) i]; // (plan.b += s)
        }
        uint64_t id = 0;
        if (icg_marg_linearize_resident(factors_.ctx(), resident->P, (int) who.size(), win.data(), dP.data(), dm.data(), db.data(), 1e-8, dev.Hp.data(),
                                        dev.bp.data(), dev.J0.data(), dev.e0.data(), nullptr, dev_min.data(), dev_status.data(), nullptr,
                                        keep_linearized_ ? &id : nullptr) != ICG_OK) {
            *what = icg_last_error(factors_.ctx());
            return false;
        }
        dev.keep_id = id;
        for (size_t k = 0; k < who.size(); k++) // second guard of finishStructured, and a solver that did not converge
            if (!(dev_min[k] > GUARD) || (dev_status[k] & 1)) dev.on_device[who[k]] = 0;
        return true;
    }
    factors_.forEachWindow(who.size(), [&](size_t k) {
        const MarginalizationInfo::StructuredPlan &plan = st[who[k]].plan;
        memcpy(&dH[h_off[k]], plan.H.data(), sizeof(double) * plan.H.size());
        memcpy(&db[b_off[k]], plan.b.data(), sizeof(double) * plan.b.size());
    });
    MarginalizationLinearizer lin(true, factors_.ctx());
    if (keep_linearized_) {
        dev.keep_id = lin.linearizeKeep((int) who.size(), dP.data(), dm.data(), dH.data(), db.data(), 1e-8, dev.Hp.data(), dev.bp.data(), dev.J0.data(),
                                        dev.e0.data(), nullptr, dev_min.data(), dev_status.data(), what);
        if (dev.keep_id == 0) return false;
    } else if (!lin.linearize((int) who.size(), dP.data(), dm.data(), dH.data(), db.data(), 1e-8, dev.Hp.data(), dev.bp.data(), dev.J0.data(),
                              dev.e0.data(), nullptr, dev_min.data(), dev_status.data(), what)) {
        return false;
    }
    for (size_t k = 0; k < who.size(); k++) // second guard of finishStructured, and a solver that did not converge
        if (!(dev_min[k] > GUARD) || (dev_status[k] & 1)) dev.on_device[who[k]] = 0;
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
    if (device_prior_ && !device_reduced_system_) {
        error_ = "setDevicePrior(true) needs setDeviceReducedSystem(true): the resident prior is read by the device call that builds the host-factor parts";
        return false;
    }
    if (device_prior_ && !devicePriorAvailable()) {
        error_ = std::string(missingDevicePriorEntry()) + " is not in this build";
        return false;
    }
    if (device_reduced_system_ && !device_linearization_) {
        error_ = "setDeviceReducedSystem(true) needs setDeviceLinearization(true): the resident reduced systems are read by the device call's linearization";
        return false;
    }
    if (device_reduced_system_ && !deviceReducedSystemAvailable()) {
        error_ = std::string(missingReducedSystemEntry()) + " is not in this build";
        return false;
    }
    const bool resident = device_reduced_system_;
    if (keep_linearized_ && !device_linearization_) {
        error_ = "setKeepLinearized(true) needs setDeviceLinearization(true): what is kept is the device call's linearization";
        return false;
    }
    if (keep_linearized_ && !keepLinearizedAvailable()) {
        error_ = "icg_marg_linearize_batch_keep is not in this build";
        return false;
    }
    if (NW == 0) return true;
    const bool dev_prior = device_prior_;
    // (the last marginalize()'s; this one keeps its own below.  setDevicePrior: the resident set is built from it first, in phase 1)
    if (!dev_prior) releaseKept();
    auto now = [] { return std::chrono::steady_clock::now(); };
    auto ms  = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
        return std::chrono::duration<double, std::milli>(b - a).count();
    };
    const auto t_layout = now();
    if (!laid_out_ && !layout()) return false;
    const double layout_ms = ms(t_layout, now());
    auto fail = [&](const std::string &what) {
        error_ = what;
        for (auto &W : windows_) W->evaluated = false;
        return false;
    };

    // ---- 1: every window's reprojection factors, one launch (residual_block_info.h:44-88 with the corrector :59-87 on the device) -------
    auto t0 = now();
    icg_ctx *ctx      = factors_.ctx();
    const int n_poses = factors_.numPoses(), n_lm = factors_.numLandmarks();
    // setDevicePrior: the prior each window hands over and its index in the resident set (window order).  The set copies J0 / e0 — from the
    // kept linearization where the views are tagged with it — so it is built before anything drops that linearization: the release here,
    // and icg_marg_linearize_resident in step 4.
    std::vector<const ResidualBlockInfo *> taken(NW, nullptr);
    std::vector<int32_t> prior_in_set(NW, -1);
    if (dev_prior) {
        std::vector<MargPriorView> views;
        for (size_t w = 0; w < NW; w++) {
            const ResidualBlockInfo *f = windows_[w]->info->devicePriorCandidate();
            if (!f) continue;
            const MargPriorView &v = dynamic_cast<const MargPriorSource *>(f->costFunction().get())->margPriorView();
            if (v.r > ICG_MARG_MAX_R) continue; // (wider than a resident prior may be: it stays a host factor)
            taken[w] = f, prior_in_set[w] = (int32_t) views.size();
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
        if (icg_reproj_eval_windows(ctx, n_poses, poses.data(), ext.data(), n_lm, inv.data(), td.data(), 1, huber_) != ICG_OK)
            return fail(icg_last_error(ctx));
    }
    for (auto &W : windows_) W->evaluated = true;
    auto t1 = now();

    // ---- 2: M1 bookkeeping, host factors, compact camera layout per window -------------------------------------------------------------
    std::vector<State> st(NW);
    const bool force_dense = MarginalizationInfo::denseForced();
    factors_.forEachWindow(NW, [&](size_t w) {
        MarginalizationInfo &I = *windows_[w]->info;
        // (setDevicePrior: the point the taken prior is evaluated at on the device — the values its Evaluate() would read here; the factor
        // itself is deferred, its blocks are still snapshot)
        if (taken[w]) prior_set_.pack((size_t) prior_in_set[w], taken[w]->parameterBlocks().data());
        if (!I.updateParameterBlocksIndex() || !I.preMarginalization(taken[w])) { // (:75-86: nothing to marginalize / an evaluation failed)
            I.isvalid_ = false;
            I.releaseMemory();
            return;
        }
        st[w].alive = true;
        if (resident) // (layout and gather only: the blocks' J^T J is formed on the device in step 3)
            st[w].planned = !force_dense && I.planLayout(st[w].plan) && I.gatherHostBlocks(st[w].plan, st[w].blocks, taken[w]);
        else
            st[w].planned = !force_dense && I.planStructured(st[w].plan);
    });
    auto t2 = now();

    // ---- 3: assembly + landmark elimination of every planned window, one launch sequence; the landmark diagonals --------------------------
    // (csrc/reproj_schur.hip, schur_impl: reduced systems of up to kMaxCameraColumns columns; a wider window takes the dense path on its own)
    for (size_t w = 0; w < NW; w++) {
        if (!st[w].planned) continue;
        const WindowFactorSet::Window &W = factors_.window(w);
        int V                            = 0;
        for (double *p : W.poses) V += st[w].plan.camera_column_of.count(p) ? 6 : 0;
        V += (W.ext && st[w].plan.camera_column_of.count(W.ext) ? 6 : 0) + (W.td && st[w].plan.camera_column_of.count(W.td) ? 1 : 0);
        if (V > kMaxCameraColumns) st[w].planned = false;
    }
    int P = 0;
    for (size_t w = 0; w < NW; w++)
        if (st[w].planned) P = std::max(P, st[w].plan.P);
    std::vector<double> S, s, hll, host_s, min_dev;
    if (P > 0) {
        std::vector<int32_t> col_pose((size_t) n_poses, -1), col_ext(NW, -1), col_td(NW, -1);
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
        s.assign(NW * (size_t) P, 0.0), hll.assign((size_t) std::max(n_lm, 1), 0.0);
        if (resident) {
            // S stays on the device; the host-factor part of every planned window is built beside it from the window's blocks
            std::vector<int32_t> Pw(NW, 1), blk_off(NW + 1, 0), nr, nf, cols, prior_of, prior_cols;
            std::vector<uint8_t> rebuild(NW, 0);
            std::vector<int64_t> jac_off;
            std::vector<double> J, r, host_diag(NW * (size_t) P, 0.0);
            host_s.assign(NW * (size_t) P, 0.0);
            for (size_t w = 0; w < NW; w++) {
                if (st[w].planned) {
                    const HostFactorBlocks &B = st[w].blocks;
                    Pw[w] = st[w].plan.P, rebuild[w] = 1;
                    for (int64_t off : B.jac_off) jac_off.push_back(off < 0 ? off : (int64_t) J.size() + off); // (< 0: ICG_HP_JAC_FROM_PRIOR)
                    if (dev_prior) {
                        prior_of.insert(prior_of.end(), B.nr.size(), -1);
                        if (B.prior_block >= 0) prior_of[nr.size() + (size_t) B.prior_block] = prior_in_set[w];
                        prior_cols.insert(prior_cols.end(), B.prior_cols.begin(), B.prior_cols.end());
                    }
                    nr.insert(nr.end(), B.nr.begin(), B.nr.end()), nf.insert(nf.end(), B.nf.begin(), B.nf.end());
                    cols.insert(cols.end(), B.cols.begin(), B.cols.end());
                    J.insert(J.end(), B.J.begin(), B.J.end()), r.insert(r.end(), B.r.begin(), B.r.end());
                }
                blk_off[w + 1] = (int32_t) nr.size();
            }
            if (icg_reproj_schur_windows_resident(ctx, P, col_pose.data(), col_ext.data(), col_td.data(), nullptr, reassemble.data(), damp.data(), 0.0, 0.0,
                                                  s.data(), diag_cc.data(), cost.data()) != ICG_OK)
                return fail(icg_last_error(ctx));
            if (dev_prior) {
                // the taken priors are evaluated where they lie (e = e0 + J0 dx at the packed point), their blocks take residual and Jacobian
                // columns from there, and the first guard's minimum comes back as one double per window
                std::vector<double> sq((size_t) std::max(n_device_priors_, 1));
                std::string what;
                if (n_device_priors_ > 0 && !prior_set_.evaluateResident(sq.data(), &what)) return fail(what);
                min_dev.assign(NW, 0.0);
                if (icg_reproj_host_parts_build_prior(ctx, P, Pw.data(), rebuild.data(), blk_off.data(), nr.data(), nf.data(), cols.data(), jac_off.data(),
                                                      J.data(), r.data(), host_s.data(), host_diag.data(), nullptr,
                                                      n_device_priors_ > 0 ? prior_of.data() : nullptr, prior_cols.data()) != ICG_OK ||
                    icg_reproj_landmark_min_windows(ctx, min_dev.data()) != ICG_OK)
                    return fail(icg_last_error(ctx));
            } else if (icg_reproj_host_parts_build(ctx, P, Pw.data(), rebuild.data(), blk_off.data(), nr.data(), nf.data(), cols.data(), jac_off.data(),
                                                   J.data(), r.data(), host_s.data(), host_diag.data(), nullptr) != ICG_OK ||
                       icg_reproj_landmark_diag_windows(ctx, hll.data()) != ICG_OK)
                return fail(icg_last_error(ctx));
        } else {
            S.assign(NW * (size_t) P * P, 0.0);
            if (icg_reproj_schur_windows(ctx, P, col_pose.data(), col_ext.data(), col_td.data(), nullptr, reassemble.data(), damp.data(), 0.0, 0.0, S.data(),
                                         s.data(), diag_cc.data(), cost.data()) != ICG_OK ||
                icg_reproj_landmark_diag_windows(ctx, hll.data()) != ICG_OK)
                return fail(icg_last_error(ctx));
        }
    }
    auto t3 = now();

    // ---- 4: guard + M3 on the camera block (or the dense M2 + M3), linearization -------------------------------------------------------------
    std::vector<char> structured(NW, 0), good(NW, 0), added(NW, 0);
    std::vector<double> min_hll(NW, 0.0);
    // the landmark-eliminated device part joins the window's compact system; the smallest landmark diagonal for the first guard
    auto addEliminated = [&](size_t w) {
        const WindowFactorSet::Window &W          = factors_.window(w);
        MarginalizationInfo::StructuredPlan &plan = st[w].plan;
        const int Pw                              = plan.P;
        if (!resident) { // (resident: the sum is formed on the device, icg_marg_linearize_resident)
            const double *Sw = &S[w * (size_t) P * P], *sw = &s[w * (size_t) P];
            for (int i = 0; i < Pw; i++) {
                for (int j = 0; j < Pw; j++) plan.H[(size_t) i * Pw + j] += Sw[(size_t) i * P + j];
                plan.b[(size_t) i] += sw[i];
            }
        }
        if (dev_prior) { // (reduced on the device, icg_reproj_landmark_min_windows: the value of the loop below)
            min_hll[w] = min_dev[w];
        } else {
            double mn = W.landmarks.empty() ? 0.0 : hll[(size_t) W.lm_begin];
            for (size_t l = 0; l < W.landmarks.size(); l++) mn = std::min(mn, hll[(size_t) W.lm_begin + l]);
            min_hll[w] = mn;
        }
        added[w]   = 1;
    };
    DeviceM3 dev{std::vector<char>(NW, 0), {}, {}, {}, {}, std::vector<size_t>(NW, 0), std::vector<size_t>(NW, 0), std::vector<int>(NW, -1), 0};
    if (device_linearization_) {
        factors_.forEachWindow(NW, [&](size_t w) {
            if (st[w].alive && st[w].planned) addEliminated(w);
        });
        std::string what;
        const ReducedRhs rhs{P, s, host_s};
        if (!linearizeOnDevice(st, added, min_hll, dev, &what, resident ? &rhs : nullptr)) return fail(what);
        kept_id_ = dev.keep_id;
    }
    std::atomic<int> n_deferred{0};
    factors_.forEachWindow(NW, [&](size_t w) {
        if (!st[w].alive) return;
        Slice &W               = *windows_[w];
        MarginalizationInfo &I = *W.info;
        if (dev.on_device[w]) {
            const size_t r = (size_t) st[w].plan.r, at = dev.r_off[w], at2 = dev.rr_off[w];
            I.Hp_.assign(dev.Hp.begin() + (long) at2, dev.Hp.begin() + (long) (at2 + r * r));
            I.bp_.assign(dev.bp.begin() + (long) at, dev.bp.begin() + (long) (at + r));
            I.linearized_jacobians_.assign(dev.J0.begin() + (long) at2, dev.J0.begin() + (long) (at2 + r * r));
            I.linearized_residuals_.assign(dev.e0.begin() + (long) at, dev.e0.begin() + (long) (at + r));
            I.setKeptLinearization(dev.keep_id, dev.keep_id ? dev.slot[w] : -1); // (what the device call kept is this window's prior)
            structured[w] = good[w] = 1;
            return;
        }
        bool done = false;
        if (st[w].planned && !resident) { // (resident: there is no H on the host to finish from — the window takes the dense path)
            if (!added[w]) addEliminated(w);
            done          = I.finishStructured(st[w].plan, min_hll[w]);
            structured[w] = done ? 1 : 0;
        }
        if (!done) {
            // (setDevicePrior: the window left the structured device path, so its prior is evaluated on the pool after all — only here)
            if (taken[w]) {
                n_deferred++;
                if (!I.evaluateDeferred()) {
                    I.isvalid_ = false;
                    I.releaseMemory();
                    return;
                }
            }
            if (!I.constructEquation()) { // (:88-92 with the window's own dense assembly on the device)
                I.isvalid_ = false;
                I.releaseMemory();
                return;
            }
            I.schurElimination();
        }
        I.linearization();
        good[w] = 1;
    });
    // (:99) the factor records of the windows that went through are retired: kept by this batch until clear() / destruction (factors.h
    // MarginalizationInfo::releaseMemory: freeing ~3 300 heap blocks per window in line is 45 of the 90 ms of 256 C2 windows)
    for (size_t w = 0; w < NW; w++)
        if (good[w]) windows_[w]->info->releaseMemoryInto(retired_);
    auto t4 = now();
    n_deferred_evaluations_ = n_deferred.load();
    for (size_t w = 0; w < NW; w++) {
        windows_[w]->evaluated = false;
        if (good[w]) (structured[w] ? n_structured_ : n_dense_)++;
        if (ok) (*ok)[w] = good[w];
        // (a window that failed on its own — its dense path left a message — is reported through ok[w] and windowError() only: the other
        // windows' priors are good, as they are when every stream marginalizes alone and one of them logs "no valid prior")
        if (!good[w] && st[w].alive && window_error_.empty() && !windows_[w]->err.empty())
            window_error_ = "window " + std::to_string(w) + ": " + windows_[w]->err;
    }
    phase_ms_[0] = ms(t0, t1), phase_ms_[1] = ms(t1, t2), phase_ms_[2] = ms(t2, t3), phase_ms_[3] = ms(t3, t4);
    if (getenv("ICG_MARG_DEBUG"))
        fprintf(stderr, "[marginalization batch] %zu windows (%d structured, %d dense): evaluate %.3f ms, bookkeeping + host factors %.3f ms, assemble + eliminate %.3f ms, M3 + linearize %.3f ms; layout (factor upload + partition) %.3f ms\n",
                NW, n_structured_, n_dense_, phase_ms_[0], phase_ms_[1], phase_ms_[2], phase_ms_[3], layout_ms);
    return true; // (false above: a launch all windows share failed)
}

} // namespace icg
