// C entry points of libicgvins_host.so: the marginalization back end (R1, M1-M4) for tests and probes.
#include <algorithm>
#include <chrono>
#include <cmath>
#include <memory>

#include "factors.h"
#include "host_pool.h"
#include "marg_batch.h"
#include "marg_linearize_hip.h"
#include "capi_windows.h"

using namespace icg;

extern "C" {

// R1 through the ceres::CostFunction surface: factors + EvaluationCallback, one Evaluate() per factor.
// rc: 0 ok, 1 = an unprepared factor did NOT fail (contract violation), <0 = error.
int icgh_backend_reproj(int n, const double *obs_soa, const int32_t *idx_i, const int32_t *idx_j, const int32_t *idx_lm,
                        int n_poses, const double *poses, const double *ext, int n_lm, const double *invdepth, double td,
                        double *out_r, double *out_J, char *err, int errlen) {
    return guarded(err, errlen, [&] {
        vector<double> P(poses, poses + 7 * (size_t) n_poses), E(ext, ext + 7), D(invdepth, invdepth + n_lm);
        double TD = td;
        vector<std::unique_ptr<ReprojectionFactor>> factors;
        ReprojectionBatch batch(0);
        for (int k = 0; k < n; k++) factors.push_back(reproj_factor_from_soa(obs_soa, n, k));
        // before registration / preparation Evaluate must fail
        {
            double r[2];
            const double *params[5] = {&P[0], &P[0], E.data(), &D[0], &TD};
            if (n > 0 && factors[0]->Evaluate(params, r, nullptr)) return 1;
        }
        for (int k = 0; k < n; k++)
            batch.add(factors[(size_t) k].get(), &P[7 * (size_t) idx_i[k]], &P[7 * (size_t) idx_j[k]], E.data(), &D[(size_t) idx_lm[k]], &TD);
        batch.finalize();
        {
            double r[2];
            const double *params[5] = {&P[0], &P[0], E.data(), &D[0], &TD};
            if (n > 0 && factors[0]->Evaluate(params, r, nullptr)) return 1; // registered but not prepared
        }
        batch.PrepareForEvaluation(true, true);
        for (int k = 0; k < n; k++) {
            const double *params[5] = {&P[7 * (size_t) idx_i[k]], &P[7 * (size_t) idx_j[k]], E.data(), &D[(size_t) idx_lm[k]], &TD};
            double *J              = out_J + 46 * (size_t) k;
            double *jac[5]         = {J, J + 14, J + 28, J + 42, J + 44};
            if (!factors[(size_t) k]->Evaluate(params, out_r + 2 * (size_t) k, jac)) {
                set_err(err, errlen, batch.error().c_str());
                return -2;
            }
        }
        return 0;
    });
}

// M1-M4 through the reference's API: marginalize pose 0 and the landmarks it references.  Parameter ids: pose k -> k,
// landmark l -> 100000 + l, extrinsic -> 900000, td -> 900001.  estimate_ext/td = 0 keeps those blocks out (constant).
// Outputs: sizes[0..1] = marginalized, remained local sizes; rem_ids/rem_index/rem_size per retained block (caller
// allocates n_poses + n_lm + 2 entries); Hp, bp, J0, e0 sized by the caller to (6*n_poses + n_lm + 7)^2 etc.
// Then evaluates MarginalizationFactor at x = current parameters perturbed by `perturb` (applied as p += d, per block by
// id order of rem_ids) and writes residuals to marg_res.
int icgh_backend_marginalize(int n, const double *obs_soa, const int32_t *idx_i, const int32_t *idx_j, const int32_t *idx_lm,
                             int n_poses, const double *poses, const double *ext, int n_lm, const double *invdepth, double td,
                             double huber_delta, double prior_weight, int estimate_ext, int estimate_td, int32_t *sizes,
                             int64_t *rem_ids, int32_t *rem_index, int32_t *rem_size, int32_t *n_rem, double *Hp, double *bp,
                             double *J0, double *e0, const double *x_eval /* concatenated by rem order, may be NULL */,
                             double *marg_res, char *err, int errlen) {
    return guarded(err, errlen, [&] {
        (void) estimate_ext;
        (void) estimate_td;
        const MargArgs args{n, obs_soa, idx_i, idx_j, idx_lm, n_poses, poses, ext, n_lm, invdepth, td, huber_delta, prior_weight};
        auto wins = marg_windows(args, 1, -1, 0.0);
        MargWindow &W = *wins[0];
        auto &info    = W.info;
        ReprojectionBatch batch(0);
        info->setReprojectionBatch(&batch);
        marg_reprojections(args, W, batch_add(batch));
        batch.finalize();
        if (!info->marginalization()) {
            set_err(err, errlen, ("marginalization failed: " + batch.error()).c_str());
            return -2;
        }
        auto blocks = info->getParamterBlocks(W.address);
        sizes[0]    = info->marginalizedSize();
        sizes[1]    = info->remainedSize();
        *n_rem      = (int32_t) blocks.size();
        for (size_t b = 0; b < blocks.size(); b++) {
            rem_ids[b]   = W.ids[reinterpret_cast<long>(blocks[b])];
            rem_index[b] = info->remainedBlockIndex()[b];
            rem_size[b]  = info->remainedBlockSize()[b];
        }
        const size_t r = (size_t) info->remainedSize();
        memcpy(Hp, info->Hp().data(), sizeof(double) * r * r);
        memcpy(bp, info->bp().data(), sizeof(double) * r);
        memcpy(J0, info->linearizedJacobians().data(), sizeof(double) * r * r);
        memcpy(e0, info->linearizedResiduals().data(), sizeof(double) * r);
        if (x_eval && marg_res) {
            MarginalizationFactor factor(info);
            vector<const double *> params;
            size_t off = 0;
            for (size_t b = 0; b < blocks.size(); b++) {
                params.push_back(x_eval + off);
                off += (size_t) rem_size[b];
            }
            if (!factor.Evaluate(params.data(), marg_res, nullptr)) return -3;
        }
        return 0;
    });
}

// The first guard of MarginalizationInfo::finishStructured on a real window: the window of icgh_backend_marginalize marginalized on a device
// factor set that is a ReprojectionBatch in everything but the smallest landmark diagonal it reports, which is the caller's `min_hll`.
// flags[0] = lastWasStructured(); flags[1] = the sizes of Hp() + bp() when the dense assembly started (-1: the dense path did not run) —
// they are empty before marginalization(), so 0 says that the refusal left them as they were.  Hp (r x r), bp (r), sizes[0..1] = m, r.
int icgh_backend_marginalize_min_hll(int n, const double *obs_soa, const int32_t *idx_i, const int32_t *idx_j, const int32_t *idx_lm, int n_poses,
                                     const double *poses, const double *ext, int n_lm, const double *invdepth, double td, double huber_delta,
                                     double prior_weight, double min_hll, int32_t *flags, int32_t *sizes, double *Hp, double *bp, char *err, int errlen) {
    struct ReportedMinimum : DeviceFactorSet {
        ReprojectionBatch batch{0};
        const MarginalizationInfo *info{nullptr};
        double min_hll{0};
        int at_dense{-1};
        bool owns(const ReprojectionFactor *f) const override { return batch.owns(f); }
        int size() const override { return batch.size(); }
        const vector<double *> &landmarkBlocks() const override { return batch.landmarkBlocks(); }
        bool evaluateCorrected(double delta) override { return batch.evaluateCorrected(delta); }
        bool accumulateNormal(const std::unordered_map<const double *, int> &column_of, int local_size, double *H0, double *b0) override {
            at_dense = (int) (info->Hp().size() + info->bp().size());
            return batch.accumulateNormal(column_of, local_size, H0, b0);
        }
        bool accumulateLandmarkEliminated(const std::unordered_map<const double *, int> &columns, int P, double *H, double *b, double *mn) override {
            const bool ok = batch.accumulateLandmarkEliminated(columns, P, H, b, nullptr);
            *mn           = min_hll;
            return ok;
        }
        const std::string &error() const override { return batch.error(); }
    };
    return guarded(err, errlen, [&] {
        const MargArgs args{n, obs_soa, idx_i, idx_j, idx_lm, n_poses, poses, ext, n_lm, invdepth, td, huber_delta, prior_weight};
        auto wins = marg_windows(args, 1, -1, 0.0);
        MargWindow &W = *wins[0];
        ReportedMinimum set;
        set.info = W.info.get(), set.min_hll = min_hll;
        W.info->setDeviceFactors(&set);
        // (a factor's batch() is the ReprojectionBatch inside the set, so owns() holds for exactly the factors added here)
        marg_reprojections(args, W, batch_add(set.batch));
        set.batch.finalize();
        if (!W.info->marginalization()) {
            set_err(err, errlen, ("marginalization failed: " + set.batch.error()).c_str());
            return -2;
        }
        flags[0] = MarginalizationInfo::lastWasStructured() ? 1 : 0, flags[1] = set.at_dense;
        sizes[0] = W.info->marginalizedSize(), sizes[1] = W.info->remainedSize();
        const size_t r = (size_t) W.info->remainedSize();
        memcpy(Hp, W.info->Hp().data(), sizeof(double) * r * r), memcpy(bp, W.info->bp().data(), sizeof(double) * r);
        return 0;
    });
}

// The marginalizations of n_windows streams (M1-M4 of each: the window of icgh_backend_marginalize, window w > 0 with its poses and inverse
// depths moved by a deterministic jitter of relative size `jitter`), mode 0: one MarginalizationBatch (marg_batch.h: the windows share
// their device launches), mode 1: one MarginalizationInfo::marginalization() after the other on a ReprojectionBatch (what a stream on its
// own does), mode 2: mode 0 with MarginalizationBatch::setDeviceLinearization (M3 + linearization of all windows in one device call).  dense_window >= 0: that window gets a host factor on one of its inverse depths, which takes it off the landmark-eliminated
// path in both modes.  The whole set is marginalized `reps` times on the SAME batch object (as a group of streams does keyframe after
// keyframe: the problems are rebuilt each time, outside the clock).  Outputs per window of the last repetition (r = sizes[1], equal for
// all windows): Hp (r x r), bp, J0 (r x r), e0; counts = windows on the structured / dense path, seconds = wall time of the
// marginalizations alone in the fastest repetition (problem construction excluded).
int icgh_backend_marginalize_batch(int mode, int n_windows, int dense_window, double jitter, int reps, int n, const double *obs_soa,
                                   const int32_t *idx_i, const int32_t *idx_j, const int32_t *idx_lm, int n_poses, const double *poses,
                                   const double *ext, int n_lm, const double *invdepth, double td, double huber_delta, double prior_weight,
                                   int host_threads, int32_t *sizes, double *Hp, double *bp, double *J0, double *e0, int32_t *counts,
                                   double *seconds, char *err, int errlen) {
    return guarded(err, errlen, [&] {
        const MargArgs args{n, obs_soa, idx_i, idx_j, idx_lm, n_poses, poses, ext, n_lm, invdepth, td, huber_delta, prior_weight};
        vector<std::unique_ptr<MargWindow>> wins;
        vector<char> ok((size_t) n_windows, 0);
        std::string what;
        double best = -1.0;
        std::unique_ptr<MarginalizationBatch> mb;
        std::unique_ptr<ReprojectionBatch> batch;
        if (mode == 0 || mode == 2) {
            mb.reset(new MarginalizationBatch(0, huber_delta, host_threads));
            mb->setDeviceLinearization(mode == 2);
        } else {
            batch.reset(new ReprojectionBatch(0));
        }
        for (int rep = 0; rep < std::max(1, reps); rep++) {
            if (mb) mb->clear(); // (before the infos of the last repetition go)
            if (batch) batch->clear();
            wins.clear();
            wins = marg_windows(args, n_windows, dense_window, jitter);
            counts[0] = counts[1] = 0;
            double took = 0;
            if (mb) {
                for (auto &W : wins) marg_reprojections(args, *W, window_add(*mb, mb->addWindow(W->info)));
                auto t0         = std::chrono::steady_clock::now();
                const bool good = mb->marginalize(&ok);
                took            = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
                if (!good) {
                    set_err(err, errlen, ("batched marginalization failed: " + mb->error()).c_str());
                    return -2;
                }
                what = mb->windowError();
                counts[0] = mb->structuredWindows(), counts[1] = mb->denseWindows();
            } else {
                for (size_t w = 0; w < wins.size(); w++) {
                    MargWindow &W = *wins[w];
                    batch->clear();
                    marg_reprojections(args, W, batch_add(*batch));
                    W.info->setReprojectionBatch(batch.get());
                    auto a = std::chrono::steady_clock::now();
                    batch->finalize();
                    ok[w] = W.info->marginalization() ? 1 : 0;
                    took += std::chrono::duration<double>(std::chrono::steady_clock::now() - a).count();
                    if (!ok[w]) what = batch->error();
                    counts[MarginalizationInfo::lastWasStructured() ? 0 : 1] += ok[w] ? 1 : 0;
                }
            }
            for (int w = 0; w < n_windows; w++)
                if (!ok[(size_t) w]) {
                    set_err(err, errlen, ("marginalization of window " + std::to_string(w) + " failed: " + what).c_str());
                    return -2;
                }
            if (best < 0 || took < best) best = took;
        }
        *seconds = best;
        const size_t r = (size_t) wins[0]->info->remainedSize();
        sizes[0] = wins[0]->info->marginalizedSize(), sizes[1] = (int32_t) r;
        for (int w = 0; w < n_windows; w++) {
            const MarginalizationInfo &I = *wins[(size_t) w]->info;
            if ((size_t) I.remainedSize() != r) {
                set_err(err, errlen, "windows of different remained size");
                return -3;
            }
            memcpy(Hp + (size_t) w * r * r, I.Hp().data(), sizeof(double) * r * r);
            memcpy(bp + (size_t) w * r, I.bp().data(), sizeof(double) * r);
            memcpy(J0 + (size_t) w * r * r, I.linearizedJacobians().data(), sizeof(double) * r * r);
            memcpy(e0 + (size_t) w * r, I.linearizedResiduals().data(), sizeof(double) * r);
        }
        if (mb) mb->clear(); // (the infos die with `wins` before the batch does)
        if (batch) batch->clear();
        return 0;
    });
}

// phases of the last MarginalizationInfo::marginalization() of this process: evaluate, construct, Schur, linearize [ms]
void icgh_backend_marginalization_phases(double *out4) { memcpy(out4, MarginalizationInfo::lastPhaseMs(), sizeof(double) * 4); }
int icgh_backend_marginalization_structured(void) { return MarginalizationInfo::lastWasStructured() ? 1 : 0; }
void icgh_backend_marginalization_force_dense(int on) { MarginalizationInfo::forceDense(on != 0); }

// M3 on raw arrays, for comparison and timing (profiles/marg_linearize_probe.py): the reduced systems of n_windows windows in the layout of
// icg_marg_linearize_batch.  mode 0: linearizeReduced per window on a HostPool of host_threads threads, mode 1: one
// icg_marg_linearize_batch call (MarginalizationLinearizer).  J0 and e0 are required, Hp / bp / evals / min_ev_m / status may be NULL.
// The batch is run reps + 1 times, the first pass untimed: seconds[0] = the fastest call (transfers included), seconds[1] = the device
// time of the kernels of one call (mode 1; 0 in mode 0).  Without the device entry point in the build mode 1 computes nothing: -4 and
// "icg_marg_linearize_batch is not in this build".
int icgh_backend_marg_linearize(int mode, int n_windows, const int32_t *P, const int32_t *m, const double *H, const double *b, double eps,
                                int host_threads, int reps, double *Hp, double *bp, double *J0, double *e0, double *evals, double *min_ev_m,
                                int32_t *status, double *seconds, char *err, int errlen) {
    return guarded(err, errlen, [&] {
        if (mode != 0 && mode != 1) {
            set_err(err, errlen, "icgh_backend_marg_linearize: mode is neither 0 (host) nor 1 (device)");
            return -1;
        }
        if (mode == 1 && !MarginalizationLinearizer::available()) {
            set_err(err, errlen, "icg_marg_linearize_batch is not in this build");
            return -4;
        }
        if (n_windows <= 0 || !P || !m || !H || !b || !J0 || !e0 || !seconds) {
            set_err(err, errlen, "icgh_backend_marg_linearize: invalid argument");
            return -1;
        }
        for (int w = 0; w < n_windows; w++)
            if (P[w] <= 0 || m[w] < 0 || m[w] >= P[w]) {
                set_err(err, errlen, ("icgh_backend_marg_linearize: window " + std::to_string(w) + " is not a valid system").c_str());
                return -1;
            }
        std::unique_ptr<TempCtx> T(mode == 1 ? new TempCtx(0) : nullptr);
        icg_ctx *ctx   = T ? T->ctx : nullptr;
        const int last = reps > 0 ? reps : 0;
        double best, best_kernel = 0;
        std::string what;
        {
            MarginalizationLinearizer lin(mode == 1, ctx, host_threads < 1 ? 1 : host_threads);
            best = best_of(reps, [&](int pass) {
                if (ctx && pass == last) icg_prof_enable(ctx, 1); // (the last pass carries the event records: its wall time still counts)
                return lin.linearize(n_windows, P, m, H, b, eps, Hp, bp, J0, e0, evals, min_ev_m, status, &what);
            });
        }
        if (best < 0) {
            set_err(err, errlen, what.c_str());
            return -2;
        }
        for (const char *name : {"marg_lin_lds", "marg_lin_global"}) {
            int launches = 0;
            double ms    = 0;
            if (ctx && icg_prof_get(ctx, name, &launches, &ms) == ICG_OK && launches > 0) best_kernel += 1e-3 * ms / launches;
        }
        seconds[0] = best, seconds[1] = best_kernel;
        return 0;
    });
}

// M4 on raw arrays, for comparison and timing (profiles/marg_factor_probe.py): the priors of n_windows windows in the layout of
// icg_marg_prior_set, evaluated at n_points points (x: n_points sets laid out like x0).  mode 0: every window by evaluateMargPrior on a
// HostPool of host_threads threads, gradient J0^T e and e . e by the same sequential sums as the kernel; mode 1: one
// MarginalizationPriorSet::set, then one evaluate per point.  Outputs per point, point after point: residuals (sum r), jacobians (sum of
// r * sum(size), may be NULL), gradient (sum r, may be NULL), sq_norm (n_windows, may be NULL).  The points are evaluated reps + 1 times,
// the first pass untimed; seconds[0] = the set (mode 1; 0 in mode 0), seconds[1] = the fastest evaluation of one point.
// Without the device entry points in the build mode 1 computes nothing: -4 and "icg_marg_prior_set is not in this build".
int icgh_backend_marg_factor(int mode, int n_windows, const int32_t *r, const int32_t *block_off, const int32_t *block_size,
                             const int32_t *block_index, const double *x0, const double *J0, const double *e0, int n_points, const double *x,
                             int host_threads, int reps, double *residuals, double *jacobians, double *gradient, double *sq_norm,
                             double *seconds, char *err, int errlen) {
    return guarded(err, errlen, [&] {
        if (mode != 0 && mode != 1) {
            set_err(err, errlen, "icgh_backend_marg_factor: mode is neither 0 (host) nor 1 (device)");
            return -1;
        }
        if (mode == 1 && !MarginalizationPriorSet::available()) {
            set_err(err, errlen, "icg_marg_prior_set is not in this build");
            return -4;
        }
        if (n_windows <= 0 || n_points <= 0 || !r || !block_off || !block_size || !block_index || !x0 || !J0 || !e0 || !x || !residuals || !seconds) {
            set_err(err, errlen, "icgh_backend_marg_factor: invalid argument");
            return -1;
        }
        const size_t W = (size_t) n_windows;
        const FlatPriors flat(W, r, block_off, block_size, block_index, x0);
        const vector<size_t> &e_off = flat.e_off, &x_off = flat.x_off;
        vector<size_t> jac_off(W + 1, 0);
        vector<MargPriorView> views(W);
        for (size_t w = 0; w < W; w++) {
            bool ok = r[w] > 0 && block_off[w + 1] >= block_off[w] && (w > 0 || block_off[0] == 0);
            for (int b = block_off[w]; ok && b < block_off[w + 1]; b++)
                ok = flat.size[(size_t) b] > 0 && flat.index[(size_t) b] >= 0 &&
                     flat.index[(size_t) b] + MarginalizationInfo::localSize(flat.size[(size_t) b]) <= r[w];
            if (!ok) {
                set_err(err, errlen, ("icgh_backend_marg_factor: window " + std::to_string(w) + " is not a valid prior").c_str());
                return -1;
            }
            views[w]       = flat.view(w, J0, e0);
            jac_off[w + 1] = jac_off[w] + (size_t) r[w] * (x_off[w + 1] - x_off[w]);
        }
        const size_t R = e_off[W], X = x_off[W], NJ = jac_off[W];
        double best = -1; // (over the points: each one evaluated reps + 1 times)
        seconds[0] = seconds[1] = 0;
        if (mode == 0) {
            HostPool pool(host_threads < 1 ? 1 : host_threads);
            for (int p = 0; p < n_points; p++) {
                const double t = best_of(reps, [&](int) {
                    pool.parallelFor(n_windows, [&](int wi) {
                        const size_t w         = (size_t) wi;
                        const MargPriorView &v = views[w];
                        vector<const double *> params((size_t) v.n_blocks);
                        vector<double *> jac((size_t) v.n_blocks, nullptr);
                        size_t xs = 0;
                        for (int b = 0; b < v.n_blocks; b++) {
                            params[(size_t) b] = x + (size_t) p * X + x_off[w] + xs;
                            if (jacobians) jac[(size_t) b] = jacobians + (size_t) p * NJ + jac_off[w] + (size_t) v.r * xs;
                            xs += (size_t) v.size[b];
                        }
                        double *e = residuals + (size_t) p * R + e_off[w];
                        evaluateMargPrior(v, params.data(), e, jacobians ? jac.data() : nullptr);
                        if (gradient)
                            for (int k = 0; k < v.r; k++) {
                                double s = 0;
                                for (int i = 0; i < v.r; i++) s += v.J0[(size_t) i * v.r + k] * e[i];
                                gradient[(size_t) p * R + e_off[w] + (size_t) k] = s;
                            }
                        if (sq_norm) {
                            double s = 0;
                            for (int i = 0; i < v.r; i++) s += e[i] * e[i];
                            sq_norm[(size_t) p * W + w] = s;
                        }
                    });
                    return true;
                });
                if (best < 0 || t < best) best = t;
            }
            seconds[1] = best;
            return 0;
        }
        TempCtx T(0);
        std::string e;
        MarginalizationPriorSet set;
        const double t_set = best_of(0, [&](int) { return set.set(T.ctx, views, &e); });
        if (t_set < 0) {
            set_err(err, errlen, e.c_str());
            return -2;
        }
        seconds[0] = t_set;
        vector<vector<const double *>> params(W);
        vector<const double *const *> plist(W);
        for (int p = 0; p < n_points; p++) {
            const double t = best_of(reps, [&](int) {
                for (size_t w = 0; w < W; w++) {
                    params[w].resize((size_t) views[w].n_blocks);
                    size_t xs = 0;
                    for (int b = 0; b < views[w].n_blocks; b++) params[w][(size_t) b] = x + (size_t) p * X + x_off[w] + xs, xs += (size_t) views[w].size[b];
                    plist[w] = params[w].data();
                }
                return set.evaluate(plist, residuals + (size_t) p * R, jacobians ? jacobians + (size_t) p * NJ : nullptr,
                                    gradient ? gradient + (size_t) p * R : nullptr, sq_norm ? sq_norm + (size_t) p * W : nullptr, &e);
            });
            if (t < 0) {
                set_err(err, errlen, e.c_str());
                return -3;
            }
            if (best < 0 || t < best) best = t;
        }
        seconds[1] = best;
        return 0;
    });
}

} // extern "C"
