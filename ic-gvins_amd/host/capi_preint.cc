// C entry points of libicgvins_host.so: IMU preintegration (P1 on the device, P2 on the host or the device) for tests and probes.
#include <memory>

#include "capi_util.h"
#include "capi_preint_streams.h"

using namespace icg;

namespace {
// The 15-state family of the shared bodies (capi_preint_streams.h): imu rows of 8, start states of 16, params9 as icg_preint_batch; a stream's
// parameter row has 13 and its member row 712.  variant: 0 = NORMAL, otherwise EARTH; only the streams entry refuses other numbers.
struct PreintFamily {
    typedef Preintegration Obj;
    typedef PreintegrationFactor Factor;
    static constexpr int PARAMS_W = 9;
    static constexpr const char *P1 = "preint", *S = "preint_eval";
    static std::shared_ptr<IntegrationParameters> params(const double *params9) { return preint_params(params9); }
    static IntegrationState state(const double *row) { return preint_state(row); }
    static std::shared_ptr<Obj> interval(int variant, const std::shared_ptr<IntegrationParameters> &P, const int32_t *offsets, const double *imu, int k,
                                         const double *state16) {
        return preint_interval(variant, P, offsets, imu, k, state16);
    }
    static void checkStreamVariant(int variant) {
        if (variant != 0 && variant != 1) throw std::runtime_error("variant " + std::to_string(variant) + " is neither 0 (Normal) nor 1 (Earth)");
    }
};
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
        PreintIntervals<PreintFamily> I(variant, n, offsets, imu, state0, params9);
        // unintegrated factors must fail
        {
            double r[15], J[480];
            if (evaluate_on_host(PreintegrationFactor(I.pre[0]), eval_point, r, J)) return 1;
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
// Preintegration::evaluateBatch (icg_preint_evaluate_batch): preint_device_entry (capi_preint_streams.h).  Arguments as icgh_backend_preint;
// outputs per interval for the host / the device path: residuals 15, jacobians 480, sqrt_info 225, ok.
int icgh_backend_preint_device(int variant, int n, const int32_t *offsets, const double *imu, const double *state0, const double *params9,
                               const double *eval_point, double *cur_state, double *residuals_host, double *jacobians_host,
                               double *residuals_dev, double *jacobians_dev, double *sqrt_info_host, double *sqrt_info_dev, int32_t *ok_host,
                               int32_t *ok_dev, char *err, int errlen) {
    return guarded(err, errlen, [&] {
        return preint_device_entry<PreintFamily>(variant, n, offsets, imu, state0, params9, eval_point, cur_state, residuals_host, jacobians_host, residuals_dev,
                                                 jacobians_dev, sqrt_info_host, sqrt_info_dev, ok_host, ok_dev, err, errlen);
    });
}

// The intervals of many streams, each with its own parameter set, through Preintegration::integrateBatch (mode 0) or ::integrateStreams
// (mode 1): flow, outputs and return codes in capi_preint_streams.h, the rows there.  variant: per interval, 0 or 1.
int icgh_backend_preint_streams(int n, const int32_t *variant, const int32_t *offsets, const double *imu, const double *state0, const double *params13,
                                int mode, int passes, int profile, int n_redo, const int32_t *redo, const double *redo_state, double *members, int32_t *ready,
                                double *pn, int32_t *pn_doubles, double *prof, double *seconds, char *err, int errlen) {
    return guarded(err, errlen, [&] {
        return preint_streams_entry<PreintFamily>(n, variant, offsets, imu, state0, params13, mode, passes, profile, n_redo, redo, redo_state, members, ready, pn,
                                                   pn_doubles, prof, seconds, err, errlen);
    });
}
// 1 when Preintegration::integrateStreams has its C entry in this build
int icgh_preint_streams_available(void) { return Preintegration::integrateStreamsAvailable() ? 1 : 0; }

// Timing of P2 on one set of intervals (profiles/preint_eval_probe.py): preint_time_entry (capi_preint_streams.h) without the P1 passes.
// out6: host seconds (best of reps), evaluateBatch wall seconds incl. packing and transfers (best), device time of the two kernels per call
// [ms] (mean over reps, event-timed), max |r_dev - r_host|, max |J_dev - J_host|, factors evaluated.
int icgh_backend_preint_eval_time(int variant, int n, const int32_t *offsets, const double *imu, const double *state0, const double *params9,
                                  const double *eval_point, int threads, int reps, double *out6, char *err, int errlen) {
    return guarded(err, errlen, [&] {
        double out8[8];
        const int rc = preint_time_entry<PreintFamily>(false, variant, n, offsets, imu, state0, params9, eval_point, threads, reps, out8, err, errlen);
        if (rc == 0) memcpy(out6, out8 + 2, sizeof(double) * 6);
        return rc;
    });
}

} // extern "C"
