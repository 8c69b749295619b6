// C entry points of libicgvins_host.so: odometer preintegration (PreintegrationOdo: P1 on the device, P2 on the host or the device) for
// tests and probes.  Flat layouts: imu9 rows (time, dt, dtheta[3], dvel[3], odovel), state0 rows of 17 (p3, q4 xyzw, v3, bg3, ba3, sodo),
// params19 (odo_params19, capi_util.h), evaluation points of 34 (pose0[7], mix0[10], pose1[7], mix1[10]).
#include <memory>

#include "capi_util.h"
#include "capi_preint_streams.h"

using namespace icg;

namespace {
IMU odo_imu(const double *row9) {
    IMU s    = ins_imu(row9);
    s.odovel = row9[8];
    return s;
}
PreintegrationOdo::Variant odo_variant(int variant) {
    if (variant != 2 && variant != 3) throw std::runtime_error("variant " + std::to_string(variant) + " is neither 2 (Odo) nor 3 (EarthOdo)");
    return variant == 2 ? PreintegrationOdo::ODO : PreintegrationOdo::EARTH_ODO;
}

// The 19-state family of the shared bodies (capi_preint_streams.h); a stream's parameter row has 23 and its member row 1125.  variant: 2 or 3,
// every entry refuses other numbers.
struct OdoFamily {
    typedef PreintegrationOdo Obj;
    typedef PreintegrationOdoFactor Factor;
    static constexpr int PARAMS_W = 19;
    static constexpr const char *P1 = "preint_odo", *S = "preint_odo_eval";
    static std::shared_ptr<IntegrationParameters> params(const double *params19) { return odo_params19(params19); }
    static IntegrationState state(const double *s17) {
        IntegrationState st = preint_state(s17);
        st.sodo             = s17[16];
        return st;
    }
    static std::shared_ptr<Obj> interval(int variant, const std::shared_ptr<IntegrationParameters> &P, const int32_t *offsets, const double *imu9, int k,
                                         const double *state17) {
        auto p = std::make_shared<Obj>(P, odo_imu(imu9 + 9 * (size_t) offsets[k]), state(state17), odo_variant(variant));
        for (int row = offsets[k] + 1; row < offsets[k + 1]; row++) p->addNewImu(odo_imu(imu9 + 9 * (size_t) row));
        return p;
    }
    static void checkStreamVariant(int variant) { odo_variant(variant); }
};
} // namespace

extern "C" {

// P1 (device batch) + P2 (host evaluate) through the PreintegrationOdo / PreintegrationOdoFactor classes.  Outputs per interval: cur_state 16,
// delta_state 20, jac 361, cov 361, delta_time 1, residuals 19, jacobians 646.  1: a factor that is not integrated evaluated; -2: the
// integration failed (err); -3: an integrated factor did not evaluate.
int icgh_backend_preint_odo(int variant, int n, const int32_t *offsets, const double *imu9, const double *state0, const double *params19,
                            const double *eval_point, double *cur_state, double *delta_state, double *jac, double *cov, double *delta_time,
                            double *residuals, double *jacobians, char *err, int errlen) {
    return guarded(err, errlen, [&] {
        TempCtx T(0);
        PreintIntervals<OdoFamily> I(variant, n, offsets, imu9, state0, params19);
        {
            double r[19], J[646];
            if (evaluate_on_host(PreintegrationOdoFactor(I.pre[0]), eval_point, r, J)) return 1;
        }
        if (!I.integrate(T.ctx, err, errlen)) return -2;
        for (int k = 0; k < n; k++) {
            const size_t j             = (size_t) k;
            const PreintegrationOdo &p = *I.pre[j];
            preint_put_state(p.currentState(), cur_state + 16 * j);
            PreintegrationOdo::deltaRow(p.deltaState(), delta_state + 20 * j);
            memcpy(jac + 361 * j, p.jacobian().data(), sizeof(double) * 361);
            memcpy(cov + 361 * j, p.covariance().data(), sizeof(double) * 361);
            delta_time[j] = p.deltaTime();
            const PreintegrationOdoFactor f(I.pre[j]);
            if (!evaluate_on_host(f, eval_point + 34 * j, residuals + 19 * j, jacobians + 646 * j)) return -3;
        }
        return 0;
    });
}

// The same integration, evaluated twice on the SAME objects: once per factor on the host (PreintegrationOdoFactor::Evaluate) and once through
// PreintegrationOdo::evaluateBatch (icg_preint_odo_evaluate_batch): preint_device_entry (capi_preint_streams.h).  Outputs per interval for the
// host / the device path: residuals 19, jacobians 646, sqrt_info 361, ok.
int icgh_backend_preint_odo_device(int variant, int n, const int32_t *offsets, const double *imu9, const double *state0, const double *params19,
                                   const double *eval_point, double *cur_state, double *residuals_host, double *jacobians_host,
                                   double *residuals_dev, double *jacobians_dev, double *sqrt_info_host, double *sqrt_info_dev,
                                   int32_t *ok_host, int32_t *ok_dev, char *err, int errlen) {
    return guarded(err, errlen, [&] {
        return preint_device_entry<OdoFamily>(variant, n, offsets, imu9, state0, params19, eval_point, cur_state, residuals_host, jacobians_host, residuals_dev,
                                              jacobians_dev, sqrt_info_host, sqrt_info_dev, ok_host, ok_dev, err, errlen);
    });
}

// The intervals of many streams, each with its own parameter set, through PreintegrationOdo::integrateBatch (mode 0) or ::integrateStreams
// (mode 1): flow, outputs and return codes in capi_preint_streams.h, the rows there.  variant: per interval, 2 or 3.
int icgh_backend_preint_odo_streams(int n, const int32_t *variant, const int32_t *offsets, const double *imu9, const double *state0,
                                    const double *params23, int mode, int passes, int profile, int n_redo, const int32_t *redo, const double *redo_state,
                                    double *members, int32_t *ready, double *pn, int32_t *pn_doubles, double *prof, double *seconds, char *err,
                                    int errlen) {
    return guarded(err, errlen, [&] {
        return preint_streams_entry<OdoFamily>(n, variant, offsets, imu9, state0, params23, mode, passes, profile, n_redo, redo, redo_state, members, ready, pn,
                                               pn_doubles, prof, seconds, err, errlen);
    });
}
// 1 when PreintegrationOdo::integrateStreams has its C entry in this build
int icgh_preint_odo_streams_available(void) { return PreintegrationOdo::integrateStreamsAvailable() ? 1 : 0; }

// Host P2 on a GIVEN integration result: the object is built from delta_state 20, jac 361, cov 361, delta_time, the pn rows (pn_rows x 4;
// EarthOdo), the interval's Earth rate iewn3 and the parameters (odo_from_result, capi_util.h), then evaluated on the host at eval_point.  No
// device is touched.  Outputs: residuals 19, jacobians 646, sqrt_info 361; residuals and jacobians are written only when the factor
// evaluates.  Returns 1 evaluated, 0 the factor refused (singular covariance), negative on an error.  block_sizes5 (optional): the factor's
// four parameter block sizes and its number of residuals.
int icgh_backend_preint_odo_eval_given(int variant, const double *params19, const double *delta_state, const double *jac, const double *cov,
                                       double delta_time, const double *pn, int pn_rows, const double *iewn3, const double *eval_point,
                                       double *residuals, double *jacobians, double *sqrt_info, int32_t *block_sizes5, char *err, int errlen) {
    return guarded(err, errlen, [&] {
        odo_variant(variant);
        const PreintegrationOdoFactor f(odo_from_result(odo_params19(params19), variant, delta_state, jac, cov, delta_time, pn, variant == 3 ? pn_rows : 0, iewn3));
        if (block_sizes5) {
            const auto &b = f.parameter_block_sizes();
            if (b.size() != 4) return -2;
            for (int k = 0; k < 4; k++) block_sizes5[k] = b[(size_t) k];
            block_sizes5[4] = f.num_residuals();
        }
        if (sqrt_info) memcpy(sqrt_info, f.preintegration().sqrtInformation().data(), sizeof(double) * 361);
        return evaluate_on_host(f, eval_point, residuals, jacobians) ? 1 : 0;
    });
}

// Timing for profiles/preint_odo_probe.py: preint_time_entry (capi_preint_streams.h) with the P1 passes, all of its out8.
int icgh_backend_preint_odo_time(int variant, int n, const int32_t *offsets, const double *imu9, const double *state0, const double *params19,
                                 const double *eval_point, int threads, int reps, double *out8, char *err, int errlen) {
    return guarded(err, errlen, [&] {
        return preint_time_entry<OdoFamily>(true, variant, n, offsets, imu9, state0, params19, eval_point, threads, reps, out8, err, errlen);
    });
}

} // extern "C"
