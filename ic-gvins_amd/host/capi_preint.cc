// C entry points of libicgvins_host.so: IMU preintegration (P1 on the device, P2 on the host or the device) for tests and probes.
#include <algorithm>
#include <cmath>
#include <memory>

#include "factors.h"
#include "host_pool.h"
#include "capi_util.h"
#include "capi_preint_streams.h"

using namespace icg;

namespace {
// The n intervals of the flat arrays as Preintegration objects.  imu: total x 8; offsets: n+1 (interval k owns the rows
// [offsets[k], offsets[k+1])); state0: n x 16; params9 as icg_preint_batch.  integrate(): one icg_preint_batch launch for all of them.
struct Intervals {
    vector<std::shared_ptr<Preintegration>> pre;
    vector<Preintegration *> raw;
    vector<const Preintegration *> craw;

    Intervals(int variant, int n, const int32_t *offsets, const double *imu, const double *state0, const double *params9) {
        auto P = preint_params(params9);
        for (int k = 0; k < n; k++) {
            auto p = preint_interval(variant, P, offsets, imu, k, state0 + 16 * (size_t) k);
            pre.push_back(p);
            raw.push_back(p.get());
            craw.push_back(p.get());
        }
    }
    bool integrate(icg_ctx *ctx, char *err, int errlen) {
        std::string e;
        if (Preintegration::integrateBatch(ctx, raw, &e)) return true;
        set_err(err, errlen, e.c_str());
        return false;
    }
};

// icgh_backend_preint_streams' family (capi_preint_streams.h).  Parameter row of 13: the 9 of icg_preint_batch, has_station, station[3]; with
// has_station the interval's Earth rate comes from its own start position and [6..8] are not used.  Member row of 712: cur_state 16,
// delta_state 16, delta_time, the time of the current state, the Earth rate 3, jac 225, cov 225, sqrt_info 225.
struct StreamsFamily {
    typedef Preintegration Obj;
    static constexpr int IMU_W = 8, STATE_W = 16, PARAM_W = 13, MEMBER_W = 16 + 16 + 2 + 3 + 3 * 225;
    static constexpr const char *P1 = "preint", *S = "preint_eval";
    static std::shared_ptr<Obj> make(int variant, const double *row, const int32_t *offsets, const double *imu, int k, const double *state16) {
        if (variant != 0 && variant != 1) throw std::runtime_error("variant " + std::to_string(variant) + " is neither 0 (Normal) nor 1 (Earth)");
        auto P         = preint_params(row);
        P->has_station = row[9] != 0;
        P->station     = Vector3d(row[10], row[11], row[12]);
        return preint_interval(variant, P, offsets, imu, k, state16);
    }
    static IntegrationState state(const double *row) { return preint_state(row); }
    static void put(const Obj &p, double *o) {
        preint_put_state(p.currentState(), o);
        preint_put_state(p.deltaState(), o + 16);
        o[32] = p.deltaTime(), o[33] = p.currentState().time;
        for (int i = 0; i < 3; i++) o[34 + i] = p.earthRate()[i];
        const vector<double> *m[3] = {&p.jacobian(), &p.covariance(), &p.sqrtInformation()};
        for (int b = 0; b < 3; b++)
            for (size_t i = 0; i < 225; i++) o[37 + 225 * b + i] = i < m[b]->size() ? (*m[b])[i] : 0.0;
    }
    static bool available(int mode) { return mode == 0 || Preintegration::integrateStreamsAvailable(); }
    static bool integrate(int mode, icg_ctx *ctx, const vector<Obj *> &list, std::string *e) {
        return mode == 0 ? Preintegration::integrateBatch(ctx, list, e) : Preintegration::integrateStreams(ctx, list, e);
    }
};

// one factor on the host at its evaluation point ep (pose0[7], mix0[9], pose1[7], mix1[9]): r 15, J 480 (15x7 | 15x9 | 15x7 | 15x9)
bool evaluate_on_host(const PreintegrationFactor &f, const double *ep, double *r, double *J) {
    const double *pp[4] = {ep, ep + 7, ep + 16, ep + 23};
    double *jj[4]       = {J, J + 105, J + 240, J + 345};
    return f.Evaluate(pp, r, jj);
}
} // namespace

extern "C" {

// P1 (device batch) + P2 (host evaluate) through the Preintegration / PreintegrationFactor classes.
// imu: total x 8; offsets: n+1; state0: n x 16; params9 as icg_preint_batch; pose/mix: the evaluation point per interval
// (pose0[7], mix0[9], pose1[7], mix1[9] concatenated = 32 doubles per interval).  Outputs: cur_state n x 16, residuals
// n x 15, jacobians n x 480 (15x7 | 15x9 | 15x7 | 15x9).
int icgh_backend_preint(int variant, int n, const int32_t *offsets, const double *imu, const double *state0, const double *params9,
                        const double *eval_point, double *cur_state, double *residuals, double *jacobians, char *err, int errlen) {
    return guarded(err, errlen, [&] {
        TempCtx T(0);
        Intervals I(variant, n, offsets, imu, state0, params9);
        // unintegrated factors must fail
        {
            double r[15];
            const double *pp[4] = {eval_point, eval_point + 7, eval_point + 16, eval_point + 23};
            if (PreintegrationFactor(I.pre[0]).Evaluate(pp, r, nullptr)) return 1;
        }
        if (!I.integrate(T.ctx, err, errlen)) return -2;
        for (int k = 0; k < n; k++) {
            preint_put_state(I.pre[(size_t) k]->currentState(), cur_state + 16 * (size_t) k);
            const PreintegrationFactor f(I.pre[(size_t) k]);
            if (!evaluate_on_host(f, eval_point + 32 * (size_t) k, residuals + 15 * (size_t) k, jacobians + 480 * (size_t) k)) return -3;
        }
        return 0;
    });
}

// The same integration, evaluated twice on the SAME objects: once per factor on the host (PreintegrationFactor::Evaluate) and once through
// Preintegration::evaluateBatch (icg_preint_evaluate_batch), so both paths can be compared on identical inputs.  Arguments as
// icgh_backend_preint; outputs per interval for the host / the device path: residuals 15, jacobians 480, sqrt_info 225 (the host's
// sqrt_information_ / the kernel's), ok (1 = evaluated; 0 = the factor cannot be evaluated, e.g. singular covariance: zero rows).
// Without the device entry point in the build nothing is computed: -4 and "icg_preint_evaluate_batch is not in this build".
int icgh_backend_preint_device(int variant, int n, const int32_t *offsets, const double *imu, const double *state0, const double *params9,
                               const double *eval_point, double *cur_state, double *residuals_host, double *jacobians_host,
                               double *residuals_dev, double *jacobians_dev, double *sqrt_info_host, double *sqrt_info_dev, int32_t *ok_host,
                               int32_t *ok_dev, char *err, int errlen) {
    return guarded(err, errlen, [&] {
        if (!Preintegration::evaluateBatchAvailable()) {
            set_err(err, errlen, "icg_preint_evaluate_batch is not in this build");
            return -4;
        }
        TempCtx T(0);
        Intervals I(variant, n, offsets, imu, state0, params9);
        if (!I.integrate(T.ctx, err, errlen)) return -2;
        memset(residuals_host, 0, sizeof(double) * 15 * (size_t) n);
        memset(jacobians_host, 0, sizeof(double) * 480 * (size_t) n);
        for (int k = 0; k < n; k++) {
            preint_put_state(I.pre[(size_t) k]->currentState(), cur_state + 16 * (size_t) k);
            const PreintegrationFactor f(I.pre[(size_t) k]);
            ok_host[k] = evaluate_on_host(f, eval_point + 32 * (size_t) k, residuals_host + 15 * (size_t) k, jacobians_host + 480 * (size_t) k) ? 1 : 0;
            memcpy(sqrt_info_host + 225 * (size_t) k, I.pre[(size_t) k]->sqrtInformation().data(), sizeof(double) * 225);
        }
        vector<char> ok;
        std::string e;
        if (!Preintegration::evaluateBatch(T.ctx, I.craw, eval_point, residuals_dev, jacobians_dev, &ok, &e, sqrt_info_dev)) {
            set_err(err, errlen, e.c_str());
            return -3;
        }
        for (int k = 0; k < n; k++) ok_dev[k] = ok[(size_t) k];
        return 0;
    });
}

// The intervals of many streams, each with its own parameter set, through Preintegration::integrateBatch (mode 0) or ::integrateStreams
// (mode 1): flow, outputs and return codes in capi_preint_streams.h, the rows in StreamsFamily above.  variant: per interval, 0 or 1.
int icgh_backend_preint_streams(int n, const int32_t *variant, const int32_t *offsets, const double *imu, const double *state0, const double *params13,
                                int mode, int passes, int profile, int n_redo, const int32_t *redo, const double *redo_state, double *members, int32_t *ready,
                                double *pn, int32_t *pn_doubles, double *prof, double *seconds, char *err, int errlen) {
    return guarded(err, errlen, [&] {
        return preint_streams_entry<StreamsFamily>(n, variant, offsets, imu, state0, params13, mode, passes, profile, n_redo, redo, redo_state, members, ready, pn,
                                                   pn_doubles, prof, seconds, err, errlen);
    });
}
// 1 when Preintegration::integrateStreams has its C entry in this build
int icgh_preint_streams_available(void) { return Preintegration::integrateStreamsAvailable() ? 1 : 0; }

// Timing of P2 on one set of intervals (profiles/preint_eval_probe.py): integrated once (one icg_preint_batch launch), then evaluated `reps`
// times (a) by PreintegrationFactor::Evaluate, one call per factor, on a HostPool of `threads` threads and (b) by one
// Preintegration::evaluateBatch call.  out6: host seconds (best of reps), evaluateBatch wall seconds incl. packing and transfers (best),
// device time of the two kernels per call [ms] (mean over reps, event-timed), max |r_dev - r_host|, max |J_dev - J_host|, factors evaluated.
int icgh_backend_preint_eval_time(int variant, int n, const int32_t *offsets, const double *imu, const double *state0, const double *params9,
                                  const double *eval_point, int threads, int reps, double *out6, char *err, int errlen) {
    return guarded(err, errlen, [&] {
        if (!Preintegration::evaluateBatchAvailable()) {
            set_err(err, errlen, "icg_preint_evaluate_batch is not in this build");
            return -4;
        }
        TempCtx T(0);
        Intervals I(variant, n, offsets, imu, state0, params9);
        vector<std::unique_ptr<PreintegrationFactor>> factors;
        for (const auto &p : I.pre) factors.emplace_back(new PreintegrationFactor(p));
        if (!I.integrate(T.ctx, err, errlen)) return -2;
        const size_t N = (size_t) n;
        vector<double> rh(15 * N), Jh(480 * N), rd(15 * N), Jd(480 * N);
        vector<char> okh(N, 0), okd;
        HostPool pool(threads < 1 ? 1 : threads);
        const double best_host = best_of(reps, [&](int) {
            pool.parallelFor(n, [&](int k) {
                const size_t j = (size_t) k;
                okh[j]         = evaluate_on_host(*factors[j], eval_point + 32 * j, rh.data() + 15 * j, Jh.data() + 480 * j) ? 1 : 0;
            });
            return true;
        });
        std::string e;
        const double best_dev = best_of(reps, [&](int pass) {
            if (pass == 1) icg_prof_enable(T.ctx, 1); // (the timed passes carry the event records)
            return Preintegration::evaluateBatch(T.ctx, I.craw, eval_point, rd.data(), Jd.data(), &okd, &e);
        });
        if (best_dev < 0) {
            set_err(err, errlen, e.c_str());
            return -3;
        }
        int launches = 0;
        double ms    = 0;
        icg_prof_get(T.ctx, "preint_eval", &launches, &ms);
        double dr = 0, dJ = 0, evaluated = 0;
        for (size_t k = 0; k < N; k++) {
            if (okh[k] != okd[k]) {
                set_err(err, errlen, ("host and device disagree on whether factor " + std::to_string(k) + " can be evaluated").c_str());
                return -5;
            }
            evaluated += okh[k] ? 1 : 0;
            for (int i = 0; i < 15; i++) dr = std::max(dr, std::fabs(rd[15 * k + i] - rh[15 * k + i]));
            for (int i = 0; i < 480; i++) dJ = std::max(dJ, std::fabs(Jd[480 * k + i] - Jh[480 * k + i]));
        }
        out6[0] = best_host, out6[1] = best_dev, out6[2] = launches > 0 ? ms / launches : 0.0, out6[3] = dr, out6[4] = dJ, out6[5] = evaluated;
        return 0;
    });
}

} // extern "C"
