// C entry points of libicgvins_host.so for the batched marginalization that reads the previous prior from the device
// (MarginalizationBatch::setDevicePrior): second-generation windows marginalized with and without the switch, on the batch object that
// produced their priors or after a default-path first generation; the host side of the mode on one window without a device (the deferred
// prior's block against the block gatherHostBlocks packs); and the host twin of the first guard's device reduction.  For tests and probes.
#include <chrono>
#include <memory>

#include "factors.h"
#include "lm_min_rule.h"
#include "marg_batch.h"
#include "marg_linearize_hip.h"
#include "capi_marg_cases.h"

using namespace icg;

namespace {

// the windows of a mixed batch that are not ordinary second-generation windows (n_windows >= 6; window 0 and 5 .. are ordinary)
enum { kNoPriorWindow = 1, kDenseWindow = 2, kRobustWindow = 3, kWeakWindow = 4 };

SecondExtras extras_of(int mixed, int w) {
    SecondExtras e;
    if (mixed) e.lm_host_factor = w == kDenseWindow, e.robust_prior = w == kRobustWindow, e.weak_landmark = w == kWeakWindow;
    return e;
}

// generation 1 of `wins` on `batch` (window `skip` stays out: it enters generation 2 as a first-generation window); the batch is cleared
bool first_generation(MarginalizationBatch &batch, const MargArgs &args, vector<std::unique_ptr<MargWindow>> &wins, int skip, std::string *what) {
    vector<char> ok;
    for (size_t w = 0; w < wins.size(); w++)
        if ((int) w != skip) marg_reprojections(args, *wins[w], window_add(batch, batch.addWindow(wins[w]->info)));
    if (!batch.marginalize(&ok)) {
        *what = "generation 1: " + batch.error();
        batch.clear();
        return false;
    }
    batch.clear();
    for (size_t k = 0; k < ok.size(); k++)
        if (!ok[k]) {
            *what = "generation 1: a window was not marginalized";
            return false;
        }
    return true;
}

} // namespace

extern "C" {

// Second-generation windows (family 2 of icgh_backend_marg_resident: the jittered visual windows n .. prior_weight one keyframe later, the
// reprojection factors of the second table n2 .. idx2_lm, generation 1's MarginalizationFactor among the host factors) marginalized by ONE
// MarginalizationBatch with setDeviceLinearization and setDeviceReducedSystem; mode bit 0: setDevicePrior, bit 1: setKeepLinearized.
// chain 0 (A): generation 1 is marginalized on the SAME batch object with the same switches, clear(), then generation 2 — with bit 1 the
// generation-1 priors carry live tags and the resident set comes from the kept linearization.  chain 1 (B): generation 1 on a separate
// default-path batch; every prior is untagged and shipped.
// mixed != 0 (n_windows >= 6): window 1 is a first-generation window without a prior, window 2 has a host factor on an inverse depth that
// leaves (not planned: dense path), window 3's prior has a Huber loss, window 4 has one more inverse depth seen by a single factor with a
// standard deviation of 1e6 (its h_ll fails the first guard); the others are ordinary.
// Outputs of generation 2 as marg_case_outputs writes them (capi_marg_cases.h).  counts (7): structured, dense, tagged windows, windows
// the second context's set took from the kept linearization, priors taken to the device, priors the batch's set took from the kept
// linearization, deferred host evaluations that ran.  phase_ms: the four phases of marginalize().  passes > 1: the whole chain that many
// times on the same batch object; the outputs are the last pass's.  kernel_ms (optional, 4): the last generation-2 marginalize() runs
// under the context's profiler and leaves the device time of marg_eval, host_part_prior, host_part, lm_min (0 where none ran).
// wall_ms (optional, passes): the wall time of generation 2's marginalize().  Without an entry the mode needs: -4 and the entry's name.
int icgh_backend_marg_prior_resident(int mode, int chain, int n_windows, int mixed, double jitter, int n, const double *obs_soa, const int32_t *idx_i,
                                     const int32_t *idx_j, const int32_t *idx_lm, int n_poses, const double *poses, const double *ext, int n_lm,
                                     const double *invdepth, double td, double huber_delta, double prior_weight, int n2, const double *obs2_soa,
                                     const int32_t *idx2_i, const int32_t *idx2_j, const int32_t *idx2_lm, int host_threads, uint64_t seed, double perturb,
                                     int passes, uint8_t *ok_out, int32_t *r_out, int32_t *tag_slot, double *Hp, double *bp, double *J0, double *e0,
                                     double *residuals, int32_t *counts, double *phase_ms, double *kernel_ms, double *wall_ms, char *err, int errlen) {
    return guarded(err, errlen, [&] {
        if (mode < 0 || mode > 3 || chain < 0 || chain > 1 || n_windows <= 0 || (mixed && n_windows < 6) || passes < 1 || !ok_out || !r_out || !tag_slot || !Hp ||
            !bp || !J0 || !e0 || !residuals || !counts || !phase_ms) {
            set_err(err, errlen, "icgh_backend_marg_prior_resident: invalid argument (mode: bit 0 = device prior, bit 1 = keep; chain 0 or 1; a mixed batch has 6 windows or more)");
            return -1;
        }
        for (int k = 0; k < 7; k++) counts[k] = 0;
        for (int k = 0; k < 4; k++) phase_ms[k] = 0;
        for (int w = 0; w < n_windows; w++) ok_out[w] = 0, r_out[w] = 0, tag_slot[w] = -1;
        if (!MarginalizationLinearizer::available()) {
            set_err(err, errlen, "icg_marg_linearize_batch is not in this build");
            return -4;
        }
        if (!MarginalizationBatch::deviceReducedSystemAvailable()) {
            set_err(err, errlen, "icg_marg_linearize_resident is not in this build");
            return -4;
        }
        if ((mode & 2) && !MarginalizationBatch::keepLinearizedAvailable()) {
            set_err(err, errlen, "icg_marg_linearize_batch_keep is not in this build");
            return -4;
        }
        const MargArgs args{n, obs_soa, idx_i, idx_j, idx_lm, n_poses, poses, ext, n_lm, invdepth, td, huber_delta, prior_weight};
        const SecondTable table{n2, obs2_soa, idx2_i, idx2_j, idx2_lm};
        const int no_prior = mixed ? kNoPriorWindow : -1;
        vector<std::unique_ptr<MargWindow>> wins;
        vector<std::unique_ptr<Case>> cases;
        vector<char> ok;
        MarginalizationBatch mb(0, huber_delta, host_threads);
        mb.setDeviceLinearization(true);
        mb.setDeviceReducedSystem(true);
        mb.setDevicePrior((mode & 1) != 0);
        mb.setKeepLinearized((mode & 2) != 0);
        for (int pass = 0; pass < passes; pass++) {
            mb.clear(); // (before the infos of the last pass go)
            cases.clear(), wins.clear();
            wins = marg_windows(args, n_windows, -1, jitter);
            std::string what;
            if (chain == 0) {
                if (!first_generation(mb, args, wins, no_prior, &what)) {
                    set_err(err, errlen, what.c_str());
                    return what.find("is not in this build") != std::string::npos ? -4 : -2;
                }
            } else {
                MarginalizationBatch first(0, huber_delta, host_threads);
                if (!first_generation(first, args, wins, no_prior, &what)) {
                    set_err(err, errlen, what.c_str());
                    return -2;
                }
            }
            Uniform rnd{kJitterSeed ^ 0x5DEECE66Dull};
            for (int w = 0; w < n_windows; w++)
                cases.push_back(w == no_prior ? visual_case(args, *wins[(size_t) w]) : second_generation_case(args, *wins[(size_t) w], table, jitter, rnd, extras_of(mixed, w)));
            for (auto &c : cases) c->addReprojections(window_add(mb, mb.addWindow(c->info)));
            const bool profiled = kernel_ms && pass == passes - 1;
            if (profiled) icg_prof_enable(mb.context(), 1);
            const auto t0   = std::chrono::steady_clock::now();
            const bool good = mb.marginalize(&ok);
            const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
            if (!good) {
                set_err(err, errlen, mb.error().c_str());
                mb.clear();
                return mb.error().find("is not in this build") != std::string::npos ? -4 : -2;
            }
            if (wall_ms) wall_ms[pass] = ms;
            if (profiled) {
                const char *names[4] = {"marg_eval", "host_part_prior", "host_part", "lm_min"};
                (void) icg_ctx_sync(mb.context());
                for (int k = 0; k < 4; k++) {
                    int launches = 0;
                    double total = 0;
                    kernel_ms[k] = icg_prof_get(mb.context(), names[k], &launches, &total) == ICG_OK && launches > 0 ? total : 0.0;
                }
                icg_prof_enable(mb.context(), 0);
            }
        }
        counts[0] = mb.structuredWindows(), counts[1] = mb.denseWindows();
        counts[4] = mb.devicePriors(), counts[5] = mb.devicePriorsFromKept(), counts[6] = mb.deferredPriorEvaluations();
        for (int k = 0; k < 4; k++) phase_ms[k] = mb.lastPhaseMs()[k];
        return marg_case_outputs(cases, ok, mb, seed, perturb, ok_out, r_out, tag_slot, Hp, bp, J0, e0, residuals, &counts[2], &counts[3], err, errlen);
    });
}

// every entry setDevicePrior needs is in this build
int icgh_backend_marg_prior_available(void) { return MarginalizationBatch::devicePriorAvailable() ? 1 : 0; }

// setDevicePrior(true) on a batch with the device linearization but without setDeviceReducedSystem(true), one first-generation window in
// it: 1 and marginalize()'s message in err when it refuses, 0 when it does not.  launches: the kernel launches the batch's profiler counted
// over the call (every name it knows).
int icgh_backend_marg_prior_switch_alone(int n, const double *obs_soa, const int32_t *idx_i, const int32_t *idx_j, const int32_t *idx_lm, int n_poses,
                                         const double *poses, const double *ext, int n_lm, const double *invdepth, double td, double huber_delta,
                                         double prior_weight, int32_t *launches, char *err, int errlen) {
    return guarded(err, errlen, [&] {
        const MargArgs args{n, obs_soa, idx_i, idx_j, idx_lm, n_poses, poses, ext, n_lm, invdepth, td, huber_delta, prior_weight};
        vector<std::unique_ptr<MargWindow>> wins = marg_windows(args, 1, -1, 0.0);
        MarginalizationBatch mb(0, huber_delta, 1);
        mb.setDeviceLinearization(true);
        mb.setDevicePrior(true);
        marg_reprojections(args, *wins[0], window_add(mb, mb.addWindow(wins[0]->info)));
        icg_prof_enable(mb.context(), 1);
        vector<char> ok;
        const bool ran = mb.marginalize(&ok);
        (void) icg_ctx_sync(mb.context());
        int total = 0;
        char names[4096] = {0};
        if (icg_prof_names(mb.context(), names, (int) sizeof names) == ICG_OK)
            for (char *save = nullptr, *name = strtok_r(names, "\n", &save); name; name = strtok_r(nullptr, "\n", &save)) {
                int count = 0;
                double ms = 0;
                if (icg_prof_get(mb.context(), name, &count, &ms) == ICG_OK) total += count;
            }
        if (launches) *launches = total;
        icg_prof_enable(mb.context(), 0);
        set_err(err, errlen, mb.error().c_str());
        mb.clear();
        return ran ? 0 : 1;
    });
}

// The host side of setDevicePrior on window `which` of the second generation (generation 1 on a default-path batch, as chain 1 above),
// nothing marginalized: the blocks gathered with the prior deferred (nr, nf, jac_off per block, cols, r, and J without the prior's
// Jacobian), the same blocks after the deferred evaluation as gatherHostBlocks packs them (e_*), prior_block, prior_cols, the prior's view
// J0 (r x r) with evaluateMargPrior's residual at the window's current blocks (prior_res), and the factor's residuals and Jacobian blocks
// (concatenated, block b r x size[b]) after the deferred evaluation (def_eval) and from an eager Evaluate() of a ResidualBlockInfo of its
// own (eag_eval).  sizes (8): blocks, columns, doubles of J, of e_J, of r, prior_block, r of the prior, doubles of an evaluation.
// caps (4): the capacities of the per-block arrays, of cols / prior_cols, of J / e_J / J0 / the evaluations, of r / e_r / prior_res; -6 when
// one is too small (sizes is filled in).  -2: the window has no such prior or is not planned.
int icgh_backend_marg_prior_gather(int which, double jitter, int n, const double *obs_soa, const int32_t *idx_i, const int32_t *idx_j, const int32_t *idx_lm,
                                   int n_poses, const double *poses, const double *ext, int n_lm, const double *invdepth, double td, double huber_delta,
                                   double prior_weight, int n2, const double *obs2_soa, const int32_t *idx2_i, const int32_t *idx2_j, const int32_t *idx2_lm,
                                   const int64_t *caps, int64_t *sizes, int32_t *nr, int32_t *nf, int64_t *jac_off, int32_t *cols, double *J, double *r,
                                   int32_t *e_nr, int32_t *e_nf, int64_t *e_jac_off, int32_t *e_cols, double *e_J, double *e_r, int32_t *prior_cols, double *J0,
                                   double *prior_res, double *def_eval, double *eag_eval, char *err, int errlen) {
    return guarded(err, errlen, [&] {
        if (which < 0 || !caps || !sizes || !nr || !nf || !jac_off || !cols || !J || !r || !e_nr || !e_nf || !e_jac_off || !e_cols || !e_J || !e_r || !prior_cols ||
            !J0 || !prior_res || !def_eval || !eag_eval) {
            set_err(err, errlen, "icgh_backend_marg_prior_gather: invalid argument");
            return -1;
        }
        const MargArgs args{n, obs_soa, idx_i, idx_j, idx_lm, n_poses, poses, ext, n_lm, invdepth, td, huber_delta, prior_weight};
        vector<std::unique_ptr<MargWindow>> wins = marg_windows(args, which + 1, -1, jitter);
        std::string what;
        {
            MarginalizationBatch first(0, huber_delta, 1);
            if (!first_generation(first, args, wins, -1, &what)) {
                set_err(err, errlen, what.c_str());
                return -2;
            }
        }
        vector<std::unique_ptr<Case>> cases = second_generation(args, wins, n2, obs2_soa, idx2_i, idx2_j, idx2_lm, jitter);
        Case &c = *cases[(size_t) which];
        ReprojectionBatch batch(0);
        c.info->setReprojectionBatch(&batch);
        c.addReprojections(batch_add(batch));
        batch.finalize();
        HostFactorBlocks D, E;
        const ResidualBlockInfo *prior = nullptr;
        if (!c.info->planWithDeferredPrior(&D, &E, &prior)) {
            set_err(err, errlen, ("no deferred prior, or the window is not planned: " + batch.error()).c_str());
            return -2;
        }
        const MargPriorView &v = dynamic_cast<const MargPriorSource *>(prior->costFunction().get())->margPriorView();
        // the deferred evaluation's results, and an eager evaluation of the same factor
        ResidualBlockInfo eager(prior->costFunction(), prior->lossFunction(), prior->parameterBlocks(), prior->marginalizationParametersIndex());
        if (!eager.Evaluate()) {
            set_err(err, errlen, "the prior's evaluation failed");
            return -2;
        }
        auto flat = [](const ResidualBlockInfo &f) {
            vector<double> out(f.residuals());
            for (const auto &Jb : f.jacobians()) out.insert(out.end(), Jb.begin(), Jb.end());
            return out;
        };
        const vector<double> def = flat(*prior), eag = flat(eager);
        vector<double> res((size_t) v.r);
        evaluateMargPrior(v, prior->parameterBlocks().data(), res.data(), nullptr);
        sizes[0] = (int64_t) D.nr.size(), sizes[1] = (int64_t) D.cols.size(), sizes[2] = (int64_t) D.J.size(), sizes[3] = (int64_t) E.J.size();
        sizes[4] = (int64_t) D.r.size(), sizes[5] = D.prior_block, sizes[6] = v.r, sizes[7] = (int64_t) def.size();
        if (E.nr.size() != D.nr.size() || E.cols.size() != D.cols.size() || E.r.size() != D.r.size() || eag.size() != def.size()) {
            set_err(err, errlen, "the deferred and the eager gather differ in shape");
            return -2;
        }
        if (sizes[0] > caps[0] || sizes[1] > caps[1] || (int64_t) D.prior_cols.size() > caps[1] || sizes[3] > caps[2] || (int64_t) v.r * v.r > caps[2] ||
            sizes[7] > caps[2] || sizes[4] > caps[3] || v.r > caps[3]) {
            set_err(err, errlen, "icgh_backend_marg_prior_gather: an output array is too small");
            return -6;
        }
        auto put = [](auto *dst, const auto &src) {
            if (!src.empty()) memcpy(dst, src.data(), sizeof(src[0]) * src.size());
        };
        put(nr, D.nr), put(nf, D.nf), put(jac_off, D.jac_off), put(cols, D.cols), put(J, D.J), put(r, D.r), put(prior_cols, D.prior_cols);
        put(e_nr, E.nr), put(e_nf, E.nf), put(e_jac_off, E.jac_off), put(e_cols, E.cols), put(e_J, E.J), put(e_r, E.r);
        memcpy(J0, v.J0, sizeof(double) * (size_t) v.r * v.r);
        put(prior_res, res), put(def_eval, def), put(eag_eval, eag);
        return 0;
    });
}

// icg_lm_min::lmMinOfWindow (host/lm_min_rule.h), the walk of k_lm_min_w's lanes on the host, beside the sequential loop it stands for:
// out[0] = the twin, out[1] = the loop  (mn = h[0]; mn = (h[l] < mn) ? h[l] : mn in order; 0.0 for n == 0)
void icgh_lm_min_twin(const double *h, int n, double *out) {
    out[0]    = icg_lm_min::lmMinOfWindow(h, n);
    double mn = n > 0 ? h[0] : 0.0;
    for (int l = 0; l < n; l++) mn = (h[l] < mn) ? h[l] : mn;
    out[1] = mn;
}

} // extern "C"
