// C entry points of libicgvins_host.so for the device-resident reduced system of the batched marginalization
// (MarginalizationBatch::setDeviceReducedSystem): the marginalizations of three window families with and without the switch, and the
// claim the mode rests on — the host-factor blocks a window ships form planStructured's H and b bit for bit — on one window without a
// device.  For tests and probes.
#include <algorithm>
#include <chrono>
#include <memory>

#include "factors.h"
#include "marg_batch.h"
#include "marg_linearize_hip.h"
#include "capi_marg_cases.h"

using namespace icg;

namespace {

// family 1, the arguments n_intervals .. prior_mix0 of icgh_backend_solve_vio_batch: every per-window array behind an array of pointers
struct VioArgs {
    const int32_t *n_intervals;
    const int32_t *const *offsets;
    const double *const *imu;
    const double *params9;
    double *const *states16;
    const int32_t *n_fac;
    const double *const *obs_soa;
    const int32_t *const *idx_i, *const *idx_j, *const *idx_lm;
    double *const *ext;
    const int32_t *n_lm;
    double *const *invdepth;
    double *td;
    const double *const *prior_pose0, *const *prior_mix0;
};

// a MarginalizationInfo behind the calls the window builders of capi_windows.h make on a solver: a parameter block gets the next id, a
// residual block becomes a ResidualBlockInfo that marginalizes those of its blocks listed in `leaving`; constants stay ordinary blocks (the
// reference's marginalization has no constant blocks)
struct OnInfo {
    Case &c;
    const vector<const double *> &leaving;
    void addParameterBlock(double *values, int, bool = false) const {
        const long key = reinterpret_cast<long>(values);
        if (c.ids.count(key)) return;
        const long id = (long) c.ids.size();
        c.ids[key] = id, c.address[id] = values;
    }
    void setParameterBlockConstant(double *) const {}
    int addResidualBlock(std::shared_ptr<ceres::CostFunction> cost, std::shared_ptr<ceres::LossFunction> loss, const vector<double *> &blocks) const {
        vector<int> drop;
        for (size_t k = 0; k < blocks.size(); k++)
            if (std::find(leaving.begin(), leaving.end(), blocks[k]) != leaving.end()) drop.push_back((int) k);
        c.info->addResidualBlockInfo(std::make_shared<ResidualBlockInfo>(std::move(cost), std::move(loss), blocks, drop));
        return 0;
    }
};

// family 1: visual-inertial windows (vio_window / vio_blocks / vio_motion_factors / vio_mix_prior) that marginalize the pose and the mix
// block of state 0 (m = 15) and the inverse depths anchored there; only the reprojection factors anchored in state 0 take part
// (ic_gvins.cc:1554-1610).  `raw` collects the preintegration objects for the caller's one integrateBatch.
struct VioCase {
    VioWindow V;
    vector<const double *> leaving;
};
std::unique_ptr<Case> vio_case(const VioArgs &v, int w, const std::shared_ptr<IntegrationParameters> &params, double huber, double prior_weight,
                               vector<Preintegration *> &raw) {
    std::unique_ptr<Case> c(new Case);
    auto vc = std::make_shared<VioCase>();
    vc->V   = vio_window(v.n_intervals[w], v.offsets[w], v.imu[w], params, v.states16[w], raw);
    VioWindow &V = vc->V;
    vc->leaving  = {&V.pose[0], &V.mix[0]};
    c->keep.push_back(vc);
    c->info = std::make_shared<MarginalizationInfo>();
    const OnInfo on{*c, vc->leaving};
    vio_blocks(on, V, v.ext[w], v.n_lm[w], v.invdepth[w], v.td + w);
    c->info->updateParamtersIds(c->ids);
    auto loss = huber > 0 ? std::make_shared<HuberLossHip>(huber) : nullptr;
    for (int k = 0; k < v.n_fac[w]; k++) {
        if (v.idx_i[w][k] != 0) continue;
        c->owned.push_back(reproj_factor_from_soa(v.obs_soa[w], v.n_fac[w], k));
        double *pi = &V.pose[0], *pj = &V.pose[7 * (size_t) v.idx_j[w][k]], *lm = v.invdepth[w] + v.idx_lm[w][k];
        c->info->addResidualBlockInfo(
            std::make_shared<ResidualBlockInfo>(c->owned.back(), loss, vector<double *>{pi, pj, v.ext[w], lm, v.td + w}, vector<int>{0, 3}));
        c->reproj.push_back({c->owned.back().get(), {pi, pj, v.ext[w], lm, v.td + w}});
    }
    return c;
}
// (the host factors read the preintegration results: added after the caller's integrateBatch)
void vio_host_factors(Case &c, const VioArgs &v, int w, double prior_weight) {
    VioCase &vc = *std::static_pointer_cast<VioCase>(c.keep[0]);
    const OnInfo on{c, vc.leaving};
    vio_motion_factors(on, vc.V, v.prior_pose0[w], prior_weight);
    vio_mix_prior(on, vc.V, v.prior_mix0[w], prior_weight);
}

vector<std::unique_ptr<Case>> vio_cases(const VioArgs &v, int n_windows, double huber, double prior_weight) {
    auto params = preint_params(v.params9);
    vector<std::unique_ptr<Case>> out;
    vector<Preintegration *> raw;
    for (int w = 0; w < n_windows; w++) out.push_back(vio_case(v, w, params, huber, prior_weight, raw));
    TempCtx T(0);
    std::string e;
    if (!Preintegration::integrateBatch(T.ctx, raw, &e)) throw std::runtime_error(e);
    for (int w = 0; w < n_windows; w++) vio_host_factors(*out[(size_t) w], v, w, prior_weight);
    return out;
}

} // namespace

extern "C" {

// The marginalizations of n_windows windows by ONE MarginalizationBatch with the device linearization; mode bit 0: setDeviceReducedSystem,
// bit 1: setKeepLinearized.  family 0: the jittered windows of icgh_backend_marginalize_batch (the arguments n .. prior_weight; dense_window
// >= 0 takes that window off the landmark-eliminated path).  family 2: those windows marginalized once on the default path and then once
// more, one keyframe later, with generation 1's MarginalizationFactor among the host factors and the reprojection factors of the second
// table (n2 .. idx2_lm, anchored in keyframe 1); the outputs are generation 2's.  family 1: visual-inertial windows of 2 to 4 states
// (the arguments n_intervals .. prior_mix0 of icgh_backend_solve_vio_batch, huber_delta and prior_weight as above) that marginalize state
// 0's pose and mix blocks.  Arguments of the other families are not read.
// Per window w: ok[w], r_out[w] (0 when not ok), tag_slot[w] (its index in the kept linearization, -1: untagged); Hp, J0 (r x r) and bp,
// e0 (r) of the good windows, concatenated in window order.  Then a MarginalizationFactor per good window, a MarginalizationPriorSet set
// from their views on a SECOND context and evaluated at x = x0 + perturb * u (u from `seed`): residuals (sum r).
// counts: structured, dense, tagged windows, windows the set took from the kept linearization.  phase_ms: the four phases of marginalize().
// passes > 1: the windows are rebuilt (outside the clock) and marginalized that many times on the SAME batch object, as a group of streams
// does keyframe after keyframe; the outputs are the last pass's, pass_ms (optional, passes x 5) holds the four phases and the wall time of
// marginalize() of every pass.  kernel_ms (optional, 2): the last pass runs under the context's profiler and leaves the device time of
// marg_form_h and host_part there (0 where the kernel did not run).
// Without an entry the mode needs nothing is computed: -4 and the entry's name.
int icgh_backend_marg_resident(int mode, int family, int n_windows, int dense_window, double jitter, int n, const double *obs_soa, const int32_t *idx_i,
                               const int32_t *idx_j, const int32_t *idx_lm, int n_poses, const double *poses, const double *ext, int n_lm,
                               const double *invdepth, double td, double huber_delta, double prior_weight, int n2, const double *obs2_soa,
                               const int32_t *idx2_i, const int32_t *idx2_j, const int32_t *idx2_lm, const int32_t *n_intervals,
                               const int32_t *const *offsets, const double *const *imu, const double *params9, double *const *states16, const int32_t *n_fac,
                               const double *const *vobs_soa, const int32_t *const *vidx_i, const int32_t *const *vidx_j, const int32_t *const *vidx_lm,
                               double *const *vext, const int32_t *vn_lm, double *const *vinvdepth, double *vtd, const double *const *prior_pose0,
                               const double *const *prior_mix0, int host_threads, uint64_t seed, double perturb, uint8_t *ok_out, int32_t *r_out,
                               int32_t *tag_slot, double *Hp, double *bp, double *J0, double *e0, double *residuals, int32_t *counts, double *phase_ms,
                               int passes, double *pass_ms, double *kernel_ms, char *err, int errlen) {
    return guarded(err, errlen, [&] {
        if (mode < 0 || mode > 3 || family < 0 || family > 2 || n_windows <= 0 || passes < 1 || !ok_out || !r_out || !tag_slot || !Hp || !bp || !J0 || !e0 || !residuals ||
            !counts || !phase_ms) {
            set_err(err, errlen, "icgh_backend_marg_resident: invalid argument (mode: bit 0 = device reduced system, bit 1 = keep; family 0, 1 or 2)");
            return -1;
        }
        for (int k = 0; k < 4; k++) counts[k] = 0, phase_ms[k] = 0;
        for (int w = 0; w < n_windows; w++) ok_out[w] = 0, r_out[w] = 0, tag_slot[w] = -1;
        // what the mode needs, before anything is built (MarginalizationBatch::marginalize would refuse by the same names)
        if ((mode & 1) && !MarginalizationBatch::deviceReducedSystemAvailable()) {
            set_err(err, errlen, "icg_marg_linearize_resident is not in this build");
            return -4;
        }
        if (!MarginalizationLinearizer::available()) {
            set_err(err, errlen, "icg_marg_linearize_batch is not in this build");
            return -4;
        }
        if ((mode & 2) && !MarginalizationBatch::keepLinearizedAvailable()) {
            set_err(err, errlen, "icg_marg_linearize_batch_keep is not in this build");
            return -4;
        }
        const MargArgs args{n, obs_soa, idx_i, idx_j, idx_lm, n_poses, poses, ext, n_lm, invdepth, td, huber_delta, prior_weight};
        const VioArgs vio{n_intervals, offsets, imu, params9, states16, n_fac, vobs_soa, vidx_i, vidx_j, vidx_lm, vext, vn_lm, vinvdepth, vtd, prior_pose0, prior_mix0};
        vector<std::unique_ptr<MargWindow>> wins;
        vector<std::unique_ptr<Case>> cases;
        vector<char> ok;
        MarginalizationBatch mb(0, huber_delta, host_threads);
        mb.setDeviceLinearization(true);
        mb.setDeviceReducedSystem((mode & 1) != 0);
        mb.setKeepLinearized((mode & 2) != 0);
        for (int pass = 0; pass < passes; pass++) {
            mb.clear(); // (before the infos of the last pass go)
            cases.clear(), wins.clear();
            if (family == 1) {
                cases = vio_cases(vio, n_windows, huber_delta, prior_weight);
            } else {
                wins = marg_windows(args, n_windows, dense_window, jitter);
                if (family == 0) {
                    cases = visual_cases(args, wins);
                } else {
                    // generation 1 on the default path (host linearization): the same priors whatever `mode` is
                    MarginalizationBatch first(0, huber_delta, host_threads);
                    for (auto &W : wins) marg_reprojections(args, *W, window_add(first, first.addWindow(W->info)));
                    if (!first.marginalize(&ok)) {
                        set_err(err, errlen, ("generation 1: " + first.error()).c_str());
                        return -2;
                    }
                    first.clear();
                    for (int w = 0; w < n_windows; w++)
                        if (!ok[(size_t) w]) {
                            set_err(err, errlen, ("generation 1: window " + std::to_string(w) + " was not marginalized").c_str());
                            return -2;
                        }
                    cases = second_generation(args, wins, n2, obs2_soa, idx2_i, idx2_j, idx2_lm, jitter);
                }
            }
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
            if (pass_ms) {
                for (int k = 0; k < 4; k++) pass_ms[5 * (size_t) pass + k] = mb.lastPhaseMs()[k];
                pass_ms[5 * (size_t) pass + 4] = ms;
            }
            if (profiled) {
                const char *names[2] = {"marg_form_h", "host_part"};
                (void) icg_ctx_sync(mb.context());
                for (int k = 0; k < 2; k++) {
                    int launches = 0;
                    double total = 0;
                    kernel_ms[k] = icg_prof_get(mb.context(), names[k], &launches, &total) == ICG_OK && launches > 0 ? total : 0.0;
                }
                icg_prof_enable(mb.context(), 0);
            }
        }
        counts[0] = mb.structuredWindows(), counts[1] = mb.denseWindows();
        for (int k = 0; k < 4; k++) phase_ms[k] = mb.lastPhaseMs()[k];
        return marg_case_outputs(cases, ok, mb, seed, perturb, ok_out, r_out, tag_slot, Hp, bp, J0, e0, residuals, &counts[2], &counts[3], err, errlen);
    });
}

// icg_marg_linearize_resident, icg_reproj_schur_windows_resident and icg_reproj_host_parts_build are all in this build
int icgh_backend_marg_resident_available(void) { return MarginalizationBatch::deviceReducedSystemAvailable() ? 1 : 0; }

// setDeviceReducedSystem(true) on a batch without setDeviceLinearization(true): 1 and marginalize()'s message in err when it refuses (it
// does so before it looks at its windows), 0 when it does not.
int icgh_backend_marg_resident_switch_alone(char *err, int errlen) {
    return guarded(err, errlen, [&] {
        MarginalizationBatch mb(0, 1.0, 1);
        mb.setDeviceReducedSystem(true);
        vector<char> ok;
        if (mb.marginalize(&ok)) return 0;
        set_err(err, errlen, mb.error().c_str());
        return 1;
    });
}

// Window `which` of family 0 (the unjittered window of icgh_backend_marginalize) or family 1 (as above), planned on a ReprojectionBatch of
// its own without anything being marginalized: H (P x P) and b (P) as planStructured accumulates the host factors, sizes = P, m, blocks,
// columns, Jacobian doubles, residuals, and the same host factors as gathered blocks in the flat layout of icgh_host_part_from_blocks (nr,
// nf, jac_off per block; cols; J; r).  caps: the capacities of H (doubles), the per-block arrays, cols, J and r; -6 when one is too small
// (sizes is filled in).  -2: the window is not planned.
int icgh_backend_marg_plan_blocks(int family, int which, int n, const double *obs_soa, const int32_t *idx_i, const int32_t *idx_j, const int32_t *idx_lm,
                                  int n_poses, const double *poses, const double *ext, int n_lm, const double *invdepth, double td, double huber_delta,
                                  double prior_weight, const int32_t *n_intervals, const int32_t *const *offsets, const double *const *imu,
                                  const double *params9, double *const *states16, const int32_t *n_fac, const double *const *vobs_soa,
                                  const int32_t *const *vidx_i, const int32_t *const *vidx_j, const int32_t *const *vidx_lm, double *const *vext,
                                  const int32_t *vn_lm, double *const *vinvdepth, double *vtd, const double *const *prior_pose0,
                                  const double *const *prior_mix0, const int64_t *caps, int64_t *sizes, double *H, double *b, int32_t *nr, int32_t *nf,
                                  int64_t *jac_off, int32_t *cols, double *J, double *r, char *err, int errlen) {
    return guarded(err, errlen, [&] {
        if ((family != 0 && family != 1) || which < 0 || !caps || !sizes || !H || !b || !nr || !nf || !jac_off || !cols || !J || !r) {
            set_err(err, errlen, "icgh_backend_marg_plan_blocks: invalid argument (family 0 or 1)");
            return -1;
        }
        const MargArgs args{n, obs_soa, idx_i, idx_j, idx_lm, n_poses, poses, ext, n_lm, invdepth, td, huber_delta, prior_weight};
        const VioArgs vio{n_intervals, offsets, imu, params9, states16, n_fac, vobs_soa, vidx_i, vidx_j, vidx_lm, vext, vn_lm, vinvdepth, vtd, prior_pose0, prior_mix0};
        vector<std::unique_ptr<MargWindow>> wins;
        vector<std::unique_ptr<Case>> cases;
        if (family == 0) {
            wins  = marg_windows(args, which + 1, -1, 0.0);
            cases = visual_cases(args, wins);
        } else {
            cases = vio_cases(vio, which + 1, huber_delta, prior_weight);
        }
        Case &c = *cases[(size_t) which];
        ReprojectionBatch batch(0);
        c.info->setReprojectionBatch(&batch);
        c.addReprojections(batch_add(batch));
        batch.finalize();
        int P = 0, m = 0;
        vector<double> Hv, bv;
        HostFactorBlocks B;
        if (!c.info->planWithBlocks(&P, &m, &Hv, &bv, &B)) {
            set_err(err, errlen, ("the window is not planned: " + batch.error()).c_str());
            return -2;
        }
        sizes[0] = P, sizes[1] = m, sizes[2] = (int64_t) B.nr.size(), sizes[3] = (int64_t) B.cols.size(), sizes[4] = (int64_t) B.J.size(), sizes[5] = (int64_t) B.r.size();
        if ((int64_t) Hv.size() > caps[0] || sizes[2] > caps[1] || sizes[3] > caps[2] || sizes[4] > caps[3] || sizes[5] > caps[4]) {
            set_err(err, errlen, "icgh_backend_marg_plan_blocks: an output array is too small");
            return -6;
        }
        auto put = [](auto *dst, const auto &src) {
            if (!src.empty()) memcpy(dst, src.data(), sizeof(src[0]) * src.size());
        };
        put(H, Hv), put(b, bv), put(nr, B.nr), put(nf, B.nf), put(jac_off, B.jac_off), put(cols, B.cols), put(J, B.J), put(r, B.r);
        return 0;
    });
}

} // extern "C"
