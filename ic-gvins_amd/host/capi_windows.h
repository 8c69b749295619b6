// The test problems the capi_*.cc files build, shared like capi_util.h (internal linkage, included by capi_*.cc and nothing else): the
// jittered marginalization windows, the visual window and the visual-inertial window on a solver, MargPriorViews over the flat layout of
// icg_marg_prior_set, and the summary packers.  The order in which a builder adds residual blocks is the order of the host sums: it is part
// of what the entries compute.
#pragma once
#include <string>
#include <unordered_map>
#include <vector>

#include "marg_batch.h"
#include "solver_batch_hip.h"
#include "solver_hip.h"
#include "capi_util.h"

namespace {

// uniform doubles in [-1, 1) from a 64-bit LCG (tests/backend_utils.py restates it)
struct Uniform {
    uint64_t s;
    double operator()() {
        s = s * 6364136223846793005ull + 1442695040888963407ull;
        return (double) ((s >> 11) & ((1ull << 53) - 1)) / (double) (1ull << 52) - 1.0;
    }
};
const uint64_t kJitterSeed = 0x9E3779B97F4A7C15ull;
// the stream of an evaluation point, from a caller's seed
Uniform point_stream(uint64_t seed) { return Uniform{seed * 2862933555777941757ull + 3037000493ull}; }

// where a reprojection factor and its five blocks go: a ReprojectionBatch, or window w of a MarginalizationBatch / WindowSolverBatch
auto batch_add(icg::ReprojectionBatch &batch) {
    return [&batch](icg::ReprojectionFactor *f, double *pi, double *pj, double *ext, double *lm, double *td) { batch.add(f, pi, pj, ext, lm, td); };
}
template <class B>
auto window_add(B &b, int w) {
    return [&b, w](icg::ReprojectionFactor *f, double *pi, double *pj, double *ext, double *lm, double *td) { b.addReprojectionFactor(w, f, pi, pj, ext, lm, td); };
}

// ---- the marginalization problem: pose 0 and the landmarks it references leave the window -----------------------------------------------
// the SoA arguments the marginalization entries share, as icgh_backend_marginalize takes them
struct MargArgs {
    int n;
    const double *obs_soa;
    const int32_t *idx_i, *idx_j, *idx_lm;
    int n_poses;
    const double *poses, *ext;
    int n_lm;
    const double *invdepth;
    double td, huber_delta, prior_weight;
};
// One window: its own copy of the parameters, their ids (pose k -> k, landmark l -> 100000 + l, extrinsic -> 900000, td -> 900001) and the
// info with every reprojection factor marginalizing {pose_ref, invdepth} as ic_gvins.cc:1600-1606 does, then a host-evaluated prior on
// pose 0 (it stands in for the prior / IMU factors of the real window; x += 0.01: a non-zero residual).
struct MargWindow {
    std::vector<double> P, E, D, pose0_prior;
    double TD;
    std::unordered_map<long, long> ids;
    std::unordered_map<long, double *> address;
    std::shared_ptr<icg::MarginalizationInfo> info;
    std::vector<std::shared_ptr<icg::ReprojectionFactor>> factors;
};
// n_windows of them: window 0 as given, window w > 0 with the positions of its poses and then its inverse depths moved by `jitter` (one
// generator runs on across the windows); window dense_window gets a host factor on one of its inverse depths, which takes it off the
// landmark-eliminated path.
std::vector<std::unique_ptr<MargWindow>> marg_windows(const MargArgs &a, int n_windows, int dense_window, double jitter) {
    using namespace icg;
    auto loss = a.huber_delta > 0 ? std::make_shared<HuberLossHip>(a.huber_delta) : nullptr;
    std::vector<std::unique_ptr<MargWindow>> wins;
    Uniform rnd{kJitterSeed};
    for (int w = 0; w < n_windows; w++) {
        std::unique_ptr<MargWindow> W(new MargWindow);
        W->P.assign(a.poses, a.poses + 7 * (size_t) a.n_poses), W->E.assign(a.ext, a.ext + 7), W->D.assign(a.invdepth, a.invdepth + a.n_lm), W->TD = a.td;
        if (w > 0) {
            for (int k = 0; k < a.n_poses; k++)
                for (int c = 0; c < 3; c++) W->P[7 * (size_t) k + c] += jitter * rnd();
            for (int l = 0; l < a.n_lm; l++) W->D[(size_t) l] *= 1.0 + jitter * rnd();
        }
        auto reg = [&](double *p, long id) { W->ids[reinterpret_cast<long>(p)] = id, W->address[id] = p; };
        for (int k = 0; k < a.n_poses; k++) reg(&W->P[7 * (size_t) k], k);
        for (int l = 0; l < a.n_lm; l++) reg(&W->D[(size_t) l], 100000 + l);
        reg(W->E.data(), 900000);
        reg(&W->TD, 900001);
        W->info = std::make_shared<MarginalizationInfo>();
        W->info->updateParamtersIds(W->ids);
        for (int k = 0; k < a.n; k++) {
            W->factors.push_back(reproj_factor_from_soa(a.obs_soa, a.n, k));
            double *pi = &W->P[7 * (size_t) a.idx_i[k]], *pj = &W->P[7 * (size_t) a.idx_j[k]], *lm = &W->D[(size_t) a.idx_lm[k]];
            W->info->addResidualBlockInfo(
                std::make_shared<ResidualBlockInfo>(W->factors.back(), loss, std::vector<double *>{pi, pj, W->E.data(), lm, &W->TD}, std::vector<int>{0, 3}));
        }
        W->pose0_prior.assign(W->P.begin(), W->P.begin() + 7);
        W->pose0_prior[0] += 0.01;
        W->info->addResidualBlockInfo(std::make_shared<ResidualBlockInfo>(std::make_shared<PosePriorFactor>(W->pose0_prior.data(), a.prior_weight), nullptr,
                                                                          std::vector<double *>{&W->P[0]}, std::vector<int>{0}));
        if (w == dense_window && a.n > 0) {
            double *lm = &W->D[(size_t) a.idx_lm[0]];
            W->info->addResidualBlockInfo(std::make_shared<ResidualBlockInfo>(std::make_shared<ScalarPriorFactor>(*lm * 1.01, 0.5 * a.prior_weight), nullptr,
                                                                              std::vector<double *>{lm}, std::vector<int>{0}));
        }
        wins.push_back(std::move(W));
    }
    return wins;
}
// a window's reprojection factors with their five blocks, into batch_add(...) or window_add(...)
template <class Add>
void marg_reprojections(const MargArgs &a, MargWindow &W, Add &&add) {
    for (int k = 0; k < a.n; k++)
        add(W.factors[(size_t) k].get(), &W.P[7 * (size_t) a.idx_i[k]], &W.P[7 * (size_t) a.idx_j[k]], W.E.data(), &W.D[(size_t) a.idx_lm[k]], &W.TD);
}

// ---- one window on a solver: the builders below take a WindowSolver, or window w of a WindowSolverBatch behind this adapter, which hides
// the leading window index; both then present the same calls
struct OnBatchWindow {
    icg::WindowSolverBatch &s;
    int w;
    void addParameterBlock(double *values, int size, bool pose_manifold = false) const { s.addParameterBlock(w, values, size, pose_manifold); }
    void setParameterBlockConstant(double *values) const { s.setParameterBlockConstant(w, values); }
    int addResidualBlock(std::shared_ptr<ceres::CostFunction> cost, std::shared_ptr<ceres::LossFunction> loss, const std::vector<double *> &blocks) const {
        return s.addResidualBlock(w, std::move(cost), std::move(loss), blocks);
    }
};

// ---- the visual window: K poses, the extrinsic, L inverse depths, td; a pose prior on every pose ---------------------------------------
// The parameter blocks in that order and the optional constants.  The reprojection factors go to whatever holds them (the ReprojectionBatch
// a WindowSolver stands on, a window of a WindowSolverBatch): a list of their own, whose order against the host blocks is free.
template <class S>
void visual_blocks(S &&s, int K, double *P, double *E, int L, double *D, double *TD, bool ext_constant, bool td_constant) {
    for (int k = 0; k < K; k++) s.addParameterBlock(P + 7 * (size_t) k, 7, true);
    s.addParameterBlock(E, 7, true);
    for (int l = 0; l < L; l++) s.addParameterBlock(D + l, 1);
    s.addParameterBlock(TD, 1);
    if (ext_constant) s.setParameterBlockConstant(E);
    if (td_constant) s.setParameterBlockConstant(TD);
}
// a pose prior on one pose block; one per pose (targets prior_poses, K x 7) fixes the gauge like the reference's marginalization prior / GNSS
// factors do
template <class S>
void pose_prior(S &&s, double *pose, const double *target, double prior_weight) {
    s.addResidualBlock(std::make_shared<PosePriorFactor>(target, prior_weight), nullptr, {pose});
}
template <class S>
void pose_priors(S &&s, int K, double *P, const double *prior_poses, double prior_weight) {
    for (int k = 0; k < K; k++) pose_prior(s, P + 7 * (size_t) k, prior_poses + 7 * (size_t) k, prior_weight);
}
// factors [f0, f1) of the 15 x n observation table with indices local to the window: created into `factors` and handed to
// add(factor, pose_i, pose_j, extrinsic, invdepth, td)
template <class Add>
void reprojections_from_soa(const double *obs_soa, int n, int f0, int f1, const int32_t *idx_i, const int32_t *idx_j, const int32_t *idx_lm, double *P, double *E,
                            double *D, double *TD, std::vector<std::unique_ptr<icg::ReprojectionFactor>> &factors, Add &&add) {
    for (int f = f0; f < f1; f++) {
        factors.push_back(reproj_factor_from_soa(obs_soa, n, f));
        add(factors.back().get(), P + 7 * (size_t) idx_i[f], P + 7 * (size_t) idx_j[f], E, D + idx_lm[f], TD);
    }
}

// ---- the visual-inertial window: K = n_intervals + 1 states of a pose (7) and a mix block (mw = 9: velocity, biases; 10 with the odometer scale
// behind them, the windows of the odometer factors) -----------------------------------------------------------------------------------------
struct VioWindow {
    int K = 0, mw = 9;
    std::vector<double> pose, mix;
    std::vector<std::shared_ptr<icg::Preintegration>> pre;        // interval k from its start state (mw = 9) ...
    std::vector<std::shared_ptr<icg::PreintegrationOdo>> pre_odo; // ... or its given odometer integration result (mw = 10)
    double *P(int k) { return &pose[7 * (size_t) k]; }
    double *M(int k) { return &mix[(size_t) mw * k]; }
    // states: K rows of p3, q4 xyzw and the mix block (v3, bg3, ba3[, sodo])
    void take(const double *states) {
        pose.resize((size_t) K * 7), mix.resize((size_t) K * mw);
        for (int k = 0; k < K; k++) memcpy(P(k), states + (size_t) (7 + mw) * k, sizeof(double) * 7), memcpy(M(k), states + (size_t) (7 + mw) * k + 7, sizeof(double) * mw);
    }
    void put(double *states) {
        for (int k = 0; k < K; k++) memcpy(states + (size_t) (7 + mw) * k, P(k), sizeof(double) * 7), memcpy(states + (size_t) (7 + mw) * k + 7, M(k), sizeof(double) * mw);
    }
};
// the window's states and its preintegration objects (imu rows of 8, interval k owns rows [offsets[k], offsets[k+1])), each also appended to
// `raw` for the one Preintegration::integrateBatch of the entry; variant: 0 Normal, 1 Earth, for every interval
VioWindow vio_window(int n_intervals, const int32_t *offsets, const double *imu, const std::shared_ptr<icg::IntegrationParameters> &params,
                     const double *states16, std::vector<icg::Preintegration *> &raw, int variant = 0) {
    VioWindow W;
    W.K = n_intervals + 1;
    W.take(states16);
    for (int k = 0; k < n_intervals; k++) {
        W.pre.push_back(preint_interval(variant, params, offsets, imu, k, states16 + 16 * (size_t) k));
        raw.push_back(W.pre.back().get());
    }
    return W;
}
// pose and mix interleaved per state, the extrinsic, the inverse depths, td; extrinsic and td constant (estimated off-line in the default
// configuration: optimize_estimate_extrinsic: false)
template <class S>
void vio_blocks(S &&s, VioWindow &W, double *ext, int n_lm, double *invdepth, double *td) {
    for (int k = 0; k < W.K; k++) {
        s.addParameterBlock(W.P(k), 7, true);
        s.addParameterBlock(W.M(k), W.mw);
    }
    s.addParameterBlock(ext, 7, true);
    for (int l = 0; l < n_lm; l++) s.addParameterBlock(invdepth + l, 1);
    s.addParameterBlock(td, 1);
    s.setParameterBlockConstant(ext);
    s.setParameterBlockConstant(td);
}
// The window's host factors come in parts, so that an entry can put a block of its own between them or behind them: the preintegration
// factors of the window's kind (optionally behind a loss function), ...
template <class S>
void vio_preint_factors(S &&s, VioWindow &W, std::shared_ptr<ceres::LossFunction> preint_loss = nullptr) {
    for (int k = 0; k + 1 < W.K; k++) {
        const std::vector<double *> blocks{W.P(k), W.M(k), W.P(k + 1), W.M(k + 1)};
        if (W.mw == 10)
            s.addResidualBlock(std::make_shared<icg::PreintegrationOdoFactor>(W.pre_odo[(size_t) k]), preint_loss, blocks);
        else
            s.addResidualBlock(std::make_shared<icg::PreintegrationFactor>(W.pre[(size_t) k]), preint_loss, blocks);
    }
}
// ... with the pose prior on state 0 behind them, ...
template <class S>
void vio_motion_factors(S &&s, VioWindow &W, const double *prior_pose0, double prior_weight, std::shared_ptr<ceres::LossFunction> preint_loss = nullptr) {
    vio_preint_factors(s, W, preint_loss);
    pose_prior(s, W.P(0), prior_pose0, prior_weight);
}
// ... and the velocity / bias (/ odometer scale) prior on state 0
template <class S>
void vio_mix_prior(S &&s, VioWindow &W, const double *prior_mix0, double prior_weight) {
    if (W.mw == 10)
        s.addResidualBlock(std::make_shared<OdoMixPriorFactor>(prior_mix0, prior_weight), nullptr, {W.M(0)});
    else
        s.addResidualBlock(std::make_shared<MixPriorFactor>(prior_mix0, prior_weight), nullptr, {W.M(0)});
}

// ---- views and summaries --------------------------------------------------------------------------------------------------------------
// The flat layout of icg_marg_prior_set (r, block_off, block_size, block_index, x0 per window, window after window) as MargPriorViews.  The
// constructor only lays out: each entry validates its windows (sizes, indices, its own message) before it takes a view.  The arrays the
// views point into live here.
struct FlatPriors {
    const int32_t *r, *block_off;
    std::vector<int> size, index;
    std::vector<const double *> x0_ptr;   // per block
    std::vector<size_t> x_off, e_off, j_off; // per window: first parameter, first residual (sum r), first element of J0 (sum r^2)
    FlatPriors(size_t W, const int32_t *r_, const int32_t *block_off_, const int32_t *block_size, const int32_t *block_index, const double *x0)
        : r(r_), block_off(block_off_), size(block_size, block_size + block_off_[W]), index(block_index, block_index + block_off_[W]),
          x0_ptr((size_t) block_off_[W]), x_off(W + 1, 0), e_off(W + 1, 0), j_off(W + 1, 0) {
        for (size_t w = 0; w < W; w++) {
            size_t xs = 0;
            for (int b = block_off[w]; b < block_off[w + 1]; b++) x0_ptr[(size_t) b] = x0 + x_off[w] + xs, xs += (size_t) size[(size_t) b];
            x_off[w + 1] = x_off[w] + xs, e_off[w + 1] = e_off[w] + (size_t) r[w], j_off[w + 1] = j_off[w] + (size_t) r[w] * r[w];
        }
    }
    // window w over J0 / e0 of all windows, optionally tagged with (keep id, slot)
    icg::MargPriorView view(size_t w, const double *J0, const double *e0, uint64_t keep_id = 0, int keep_slot = -1) const {
        icg::MargPriorView v;
        v.r = r[w], v.n_blocks = block_off[w + 1] - block_off[w];
        v.size = size.data() + block_off[w], v.index = index.data() + block_off[w], v.x0 = x0_ptr.data() + block_off[w];
        v.J0 = J0 + j_off[w], v.e0 = e0 + e_off[w];
        v.keep_id = keep_id, v.keep_slot = keep_slot;
        return v;
    }
};

// initial cost, final cost, successful and unsuccessful steps
void put_summary4(const icg::solver_detail::Summary &s, double *o) {
    o[0] = s.initial_cost, o[1] = s.final_cost, o[2] = s.num_successful_steps, o[3] = s.num_unsuccessful_steps;
}
// initial cost, cost after solve 1, final cost, successful and unsuccessful steps of solve 1, of solve 2, removed; s2 = NULL: one solve
void put_summary8(const icg::solver_detail::Summary &s1, const icg::solver_detail::Summary *s2, int removed, double *o) {
    o[0] = s1.initial_cost, o[1] = s1.final_cost, o[2] = s1.final_cost, o[3] = s1.num_successful_steps, o[4] = s1.num_unsuccessful_steps, o[5] = o[6] = o[7] = 0;
    if (s2) o[2] = s2->final_cost, o[5] = s2->num_successful_steps, o[6] = s2->num_unsuccessful_steps, o[7] = removed;
}

} // namespace
