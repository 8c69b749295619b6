// C entry point of libicgvins_host.so for the M3 -> M4 hand-off on the device (MarginalizationBatch::setKeepLinearized ->
// MarginalizationPriorSet::set / WindowSolverBatch::setDevicePrior): the host chain marginalize -> clear -> set -> evaluate -> solve on the
// windows of icgh_backend_marginalize_batch.  For tests and probes.
#include <algorithm>
#include <chrono>
#include <memory>

#include "factors.h"
#include "marg_batch.h"
#include "marg_linearize_hip.h"
#include "solver_batch_hip.h"
#include "capi_windows.h"

using namespace icg;

extern "C" {

// The windows of icgh_backend_marginalize_batch (the same leading arguments: window w > 0 jittered, dense_window >= 0 takes that window off
// the landmark-eliminated path) marginalized by ONE MarginalizationBatch with the device linearization; mode bit 0: setKeepLinearized,
// bit 1: the kept linearization is released before the priors are set (they are then shipped).  Then, in the order a driver keeps:
//   a MarginalizationFactor per good window, the batch cleared;
//   a MarginalizationPriorSet set from the factors' views on a SECOND context and evaluated at x = x0 + perturb * u (u uniform in
//     [-1, 1) from `seed`, every parameter of every block): residuals, gradient (sum r each, prior after prior), sq_norm and — through
//     pack / evaluateResident — sq_norm_resident (one per prior);
//   solve_iters > 0: a WindowSolverBatch (device reduced solve, host part and prior: mode 3 of icgh_backend_solve_prior_batch) over the
//     same windows — every pose, the constant extrinsic and td, the inverse depths, the reprojection factors, a pose prior of
//     prior_weight on every pose and the window's marginalization prior; states (n_windows x n_poses x 7), invdepth_out (n_windows x n_lm)
//     and summary4 (n_windows x 4: initial cost, final cost, successful and unsuccessful steps) are what the solve leaves.
// counts[0] = priors (good windows), [1] = their residuals together, [2] = windows the set took from the kept linearization
// (MarginalizationPriorSet::handedOff), [3] = windows tagged by the batch (device-linearized and kept), [4] = structured and [5] = dense
// windows of the batch, [6] = WindowSolverBatch::priorsHandedOff.  timers_ms: marginalize, set, evaluate, resident evaluation, solve.
// The caller sizes residuals / gradient for n_windows * (6 n_poses + n_lm + 7).  Without the entries a mode needs nothing is computed: -4
// and the entry's name (bit 0 set: MarginalizationBatch::marginalize refuses by name).
int icgh_backend_marg_handoff(int mode, int n_windows, int dense_window, double jitter, int n, const double *obs_soa, const int32_t *idx_i,
                              const int32_t *idx_j, const int32_t *idx_lm, int n_poses, const double *poses, const double *ext, int n_lm,
                              const double *invdepth, double td, double huber_delta, double prior_weight, int host_threads, uint64_t seed, double perturb,
                              int solve_iters, int32_t *counts, double *residuals, double *gradient, double *sq_norm, double *sq_norm_resident,
                              double *states, double *invdepth_out, double *summary4, double *timers_ms, char *err, int errlen) {
    return guarded(err, errlen, [&] {
        if (mode < 0 || mode > 3 || mode == 2 || n_windows <= 0 || !counts || !residuals || !gradient || !sq_norm || !sq_norm_resident || !timers_ms ||
            (solve_iters > 0 && (!states || !invdepth_out || !summary4))) {
            set_err(err, errlen, "icgh_backend_marg_handoff: invalid argument (mode: 0 = shipped, 1 = kept, 3 = kept and released before the set)");
            return -1;
        }
        const bool keep = (mode & 1) != 0, release_first = (mode & 2) != 0;
        const MargArgs args{n, obs_soa, idx_i, idx_j, idx_lm, n_poses, poses, ext, n_lm, invdepth, td, huber_delta, prior_weight};
        auto wins = marg_windows(args, n_windows, dense_window, jitter);
        vector<vector<double>> pose_prior; // the poses each window starts from: the targets of its solve's pose priors
        for (auto &W : wins) pose_prior.push_back(W->P);
        auto now = [] { return std::chrono::steady_clock::now(); };
        auto ms  = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point b) {
            return std::chrono::duration<double, std::milli>(b - a).count();
        };
        for (int k = 0; k < 7; k++) counts[k] = 0;
        for (int k = 0; k < 5; k++) timers_ms[k] = 0;

        // ---- marginalize (the batch's context owns what is kept)
        MarginalizationBatch mb(0, huber_delta, host_threads);
        mb.setDeviceLinearization(true);
        mb.setKeepLinearized(keep);
        for (auto &W : wins) marg_reprojections(args, *W, window_add(mb, mb.addWindow(W->info)));
        vector<char> ok;
        auto t0 = now();
        if (!mb.marginalize(&ok)) {
            set_err(err, errlen, mb.error().c_str());
            mb.clear();
            return mb.error().find("is not in this build") != std::string::npos ? -4 : -2;
        }
        timers_ms[0] = ms(t0, now());
        counts[4] = mb.structuredWindows(), counts[5] = mb.denseWindows();

        // ---- the priors: a factor per good window, then the batch is cleared (a driver clears before it solves)
        vector<int> good;
        vector<std::shared_ptr<MarginalizationFactor>> priors;
        vector<vector<double *>> blocks;
        for (int w = 0; w < n_windows; w++) {
            if (!ok[(size_t) w]) continue;
            MargWindow &W = *wins[(size_t) w];
            good.push_back(w);
            blocks.push_back(W.info->getParamterBlocks(W.address));
            priors.push_back(std::make_shared<MarginalizationFactor>(W.info));
            counts[3] += W.info->keptId() != 0 ? 1 : 0;
        }
        mb.clear();
        if (release_first) mb.releaseKept();
        if (good.empty()) {
            set_err(err, errlen, ("no window was marginalized: " + mb.windowError()).c_str());
            return -2;
        }
        counts[0] = (int32_t) good.size();

        // ---- set on a second context, evaluate at the perturbed point
        {
            TempCtx T(0);
            MarginalizationPriorSet set;
            vector<MargPriorView> views;
            for (auto &f : priors) views.push_back(f->margPriorView());
            std::string e;
            t0 = now();
            if (!set.set(T.ctx, views, &e)) {
                set_err(err, errlen, e.c_str());
                return -3;
            }
            timers_ms[1] = ms(t0, now());
            counts[1] = (int32_t) set.residualSize(), counts[2] = set.handedOff();
            Uniform rnd = point_stream(seed);
            vector<vector<double>> xs(views.size());
            vector<vector<const double *>> params(views.size());
            vector<const double *const *> plist(views.size());
            for (size_t p = 0; p < views.size(); p++) {
                const MargPriorView &v = views[p];
                size_t total           = 0;
                for (int b = 0; b < v.n_blocks; b++) total += (size_t) v.size[b];
                xs[p].reserve(total);
                for (int b = 0; b < v.n_blocks; b++)
                    for (int k = 0; k < v.size[b]; k++) xs[p].push_back(v.x0[b][k] + perturb * rnd());
                size_t at = 0;
                for (int b = 0; b < v.n_blocks; b++) params[p].push_back(xs[p].data() + at), at += (size_t) v.size[b];
                plist[p] = params[p].data();
            }
            t0 = now();
            if (!set.evaluate(plist, residuals, nullptr, gradient, sq_norm, &e)) {
                set_err(err, errlen, e.c_str());
                return -3;
            }
            timers_ms[2] = ms(t0, now());
            if (MarginalizationPriorSet::residentAvailable()) {
                for (size_t p = 0; p < views.size(); p++) set.pack(p, plist[p]);
                t0 = now();
                if (!set.evaluateResident(sq_norm_resident, &e)) {
                    set_err(err, errlen, e.c_str());
                    return -3;
                }
                timers_ms[3] = ms(t0, now());
            }
        }
        if (solve_iters <= 0) return 0;

        // ---- the windows solved with their priors resident (the solver's own context: the third)
        if (!WindowSolverBatch::devicePriorAvailable() || !WindowSolverBatch::deviceHostPartAvailable() || !WindowSolverBatch::deviceReducedSolveAvailable()) {
            set_err(err, errlen, "icg_reproj_host_parts_build_prior is not in this build");
            return -4;
        }
        WindowSolverBatch solver(0, huber_delta);
        solver.setDeviceReducedSolve(true);
        solver.setDeviceHostPart(true);
        solver.setDevicePrior(true);
        for (size_t g = 0; g < good.size(); g++) {
            MargWindow &W = *wins[(size_t) good[g]];
            const OnBatchWindow win{solver, solver.addWindow()};
            visual_blocks(win, n_poses, W.P.data(), W.E.data(), n_lm, W.D.data(), &W.TD, true, true);
            marg_reprojections(args, W, window_add(solver, win.w));
            pose_priors(win, n_poses, W.P.data(), pose_prior[(size_t) good[g]].data(), prior_weight);
            solver.addResidualBlock(win.w, priors[g], nullptr, blocks[g]);
        }
        if (!solver.prepare()) {
            set_err(err, errlen, solver.error().c_str());
            return -5;
        }
        WindowSolverBatch::Options opt;
        vector<WindowSolverBatch::Summary> sum;
        opt.max_num_iterations = solve_iters;
        t0                     = now();
        if (!solver.solve(opt, &sum)) {
            set_err(err, errlen, solver.error().c_str());
            return -3;
        }
        timers_ms[4] = ms(t0, now());
        counts[6]    = solver.priorsHandedOff();
        for (size_t g = 0; g < good.size(); g++) {
            const MargWindow &W = *wins[(size_t) good[g]];
            memcpy(states + g * 7 * (size_t) n_poses, W.P.data(), sizeof(double) * 7 * (size_t) n_poses);
            memcpy(invdepth_out + g * (size_t) n_lm, W.D.data(), sizeof(double) * (size_t) n_lm);
            put_summary4(sum[g], summary4 + 4 * g);
        }
        return 0;
    });
}

// The hand-off on raw arrays, for timing (profiles/marg_handoff_probe.py): the reduced systems of n_windows windows in the layout of
// icg_marg_linearize_batch and a block layout per window in the layout of icg_marg_prior_set (r[w] = P[w] - m[w]).  One pass is the chain
//   M3 of all windows in one device call (MarginalizationLinearizer: linearize, mode 0 / linearizeKeep, mode 1) on one context
//   -> MarginalizationPriorSet::set from views on the downloaded J0 / e0 (mode 1: tagged with the kept linearization) on a SECOND context
//   -> one evaluateResident at x.
// reps + 1 passes, the first untimed (it grows the arenas and the resident buffers); ms is reps x 3: linearize, set, resident evaluation
// of every timed pass [ms].  A last, untimed pass runs the set under the context's profiler: *store_kernel_ms = the device time of its
// store kernel (marg_set, mode 0 / marg_set_from, mode 1).  sq_norm (n_windows) and *handed_off are the last pass's.
int icgh_backend_marg_handoff_chain(int mode, int n_windows, const int32_t *P, const int32_t *m, const double *H, const double *b, double eps,
                                    const int32_t *block_off, const int32_t *block_size, const int32_t *block_index, const double *x0, const double *x,
                                    int reps, double *sq_norm, int32_t *handed_off, double *ms, double *store_kernel_ms, char *err, int errlen) {
    return guarded(err, errlen, [&] {
        if ((mode != 0 && mode != 1) || n_windows <= 0 || reps < 1 || !P || !m || !H || !b || !block_off || !block_size || !block_index || !x0 || !x ||
            !sq_norm || !handed_off || !ms || !store_kernel_ms) {
            set_err(err, errlen, "icgh_backend_marg_handoff_chain: invalid argument (mode: 0 = shipped, 1 = kept and handed off)");
            return -1;
        }
        if (!MarginalizationLinearizer::available() || !MarginalizationPriorSet::residentAvailable()) {
            set_err(err, errlen, "icg_marg_linearize_batch is not in this build");
            return -4;
        }
        if (mode == 1 && !(MarginalizationLinearizer::keepAvailable() && MarginalizationPriorSet::handOffAvailable())) {
            set_err(err, errlen, "icg_marg_linearize_batch_keep is not in this build");
            return -4;
        }
        const size_t W = (size_t) n_windows;
        for (size_t w = 0; w < W; w++)
            if (P[w] <= 0 || m[w] < 0 || m[w] >= P[w] || block_off[w + 1] < block_off[w]) {
                set_err(err, errlen, ("icgh_backend_marg_handoff_chain: window " + std::to_string(w) + " is not a valid system").c_str());
                return -1;
            }
        vector<int32_t> r(W);
        for (size_t w = 0; w < W; w++) r[w] = P[w] - m[w];
        const FlatPriors flat(W, r.data(), block_off, block_size, block_index, x0);
        vector<const double *> x_ptr(flat.x0_ptr.size()); // x laid out like x0
        for (size_t bk = 0; bk < x_ptr.size(); bk++) x_ptr[bk] = x + (flat.x0_ptr[bk] - x0);
        TempCtx Tlin(0), Tset(0);
        MarginalizationLinearizer lin(true, Tlin.ctx);
        MarginalizationPriorSet set;
        vector<double> J0(flat.j_off[W]), e0(flat.e_off[W]);
        vector<MargPriorView> views(W);
        auto now = [] { return std::chrono::steady_clock::now(); };
        auto took = [](std::chrono::steady_clock::time_point a, std::chrono::steady_clock::time_point z) {
            return std::chrono::duration<double, std::milli>(z - a).count();
        };
        std::string e;
        for (int pass = 0; pass < reps + 2; pass++) {
            const bool profiled = pass == reps + 1;
            double *t           = pass >= 1 && !profiled ? ms + 3 * (size_t) (pass - 1) : nullptr;
            auto a              = now();
            uint64_t id         = 0;
            if (mode == 1) {
                id = lin.linearizeKeep(n_windows, P, m, H, b, eps, nullptr, nullptr, J0.data(), e0.data(), nullptr, nullptr, nullptr, &e);
                if (id == 0) {
                    set_err(err, errlen, e.c_str());
                    return -2;
                }
            } else if (!lin.linearize(n_windows, P, m, H, b, eps, nullptr, nullptr, J0.data(), e0.data(), nullptr, nullptr, nullptr, &e)) {
                set_err(err, errlen, e.c_str());
                return -2;
            }
            auto z = now();
            if (t) t[0] = took(a, z);
            for (size_t w = 0; w < W; w++) views[w] = flat.view(w, J0.data(), e0.data(), id, id ? (int) w : -1);
            if (profiled) icg_prof_enable(Tset.ctx, 1);
            a = now();
            if (!set.set(Tset.ctx, views, &e)) {
                set_err(err, errlen, e.c_str());
                return -3;
            }
            z = now();
            if (t) t[1] = took(a, z);
            *handed_off = set.handedOff();
            if (profiled) {
                int launches = 0;
                double kms   = 0;
                (void) icg_ctx_sync(Tset.ctx);
                *store_kernel_ms = icg_prof_get(Tset.ctx, mode == 1 ? "marg_set_from" : "marg_set", &launches, &kms) == ICG_OK && launches > 0 ? kms / launches : 0.0;
                icg_prof_enable(Tset.ctx, 0);
            }
            a = now();
            for (size_t w = 0; w < W; w++) set.pack(w, x_ptr.data() + block_off[w]);
            if (!set.evaluateResident(sq_norm, &e)) {
                set_err(err, errlen, e.c_str());
                return -3;
            }
            z = now();
            if (t) t[2] = took(a, z);
        }
        return 0;
    });
}

// Tags without a device: a MargPriorView built from an untagged MarginalizationInfo has id 0 and slot -1, and MarginalizationFactor copies
// a tag into its view.  out4: view id and slot of the untagged info; view id and slot after setKeptLinearization(id, slot).
int icgh_backend_marg_handoff_tags(uint64_t id, int slot, int64_t *out4) {
    auto info = std::make_shared<MarginalizationInfo>();
    {
        MarginalizationFactor f(info);
        out4[0] = (int64_t) f.margPriorView().keep_id, out4[1] = f.margPriorView().keep_slot;
    }
    info->setKeptLinearization(id, slot);
    MarginalizationFactor f(info);
    out4[2] = (int64_t) f.margPriorView().keep_id, out4[3] = f.margPriorView().keep_slot;
    return 0;
}

// what of the hand-off this build of the host layer has: bit 0 = icg_marg_linearize_batch_keep / icg_marg_linearized_release, bit 1 =
// icg_marg_prior_set_from_kept
int icgh_backend_marg_handoff_available(void) {
    return (MarginalizationLinearizer::keepAvailable() ? 1 : 0) | (MarginalizationPriorSet::handOffAvailable() ? 2 : 0);
}

} // extern "C"
