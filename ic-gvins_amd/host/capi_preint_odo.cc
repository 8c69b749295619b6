// C entry points of libicgvins_host.so: odometer preintegration (PreintegrationOdo: P1 on the device, P2 on the host or the device) for
// tests and probes.  Flat layouts: imu9 rows (time, dt, dtheta[3], dvel[3], odovel), state0 rows of 17 (p3, q4 xyzw, v3, bg3, ba3, sodo),
// params19 = [0..8] as icg_preint_batch, [9..11] odo_std, [12] odo_srw, [13..15] abv, [16..18] lodo (the host forms cvb from abv), evaluation
// points of 34 (pose0[7], mix0[10], pose1[7], mix1[10]).
#include <algorithm>
#include <cmath>
#include <memory>

#include "preintegration_odo.h"
#include "host_pool.h"
#include "capi_util.h"
#include "capi_preint_streams.h"

using namespace icg;

namespace {
std::shared_ptr<IntegrationParameters> odo_params(const double *params19) {
    auto P     = preint_params(params19);
    P->odo_std = Vector3d(params19[9], params19[10], params19[11]);
    P->odo_srw = params19[12];
    P->abv     = Vector3d(params19[13], params19[14], params19[15]);
    P->lodo    = Vector3d(params19[16], params19[17], params19[18]);
    return P;
}
IMU odo_imu(const double *row9) {
    IMU s    = ins_imu(row9);
    s.odovel = row9[8];
    return s;
}
IntegrationState odo_state(const double *s17) {
    IntegrationState st = preint_state(s17);
    st.sodo             = s17[16];
    return st;
}
PreintegrationOdo::Variant odo_variant(int variant) {
    if (variant != 2 && variant != 3) throw std::runtime_error("variant " + std::to_string(variant) + " is neither 2 (Odo) nor 3 (EarthOdo)");
    return variant == 2 ? PreintegrationOdo::ODO : PreintegrationOdo::EARTH_ODO;
}
void put_delta20(const IntegrationState &d, double *o) {
    preint_put_state(d, o);
    o[16] = d.s[0], o[17] = d.s[1], o[18] = d.s[2], o[19] = d.sodo;
}

// The n intervals of the flat arrays as PreintegrationOdo objects; integrate(): icg_preint_odo_batch for all of them.
struct OdoIntervals {
    vector<std::shared_ptr<PreintegrationOdo>> pre;
    vector<PreintegrationOdo *> raw;
    vector<const PreintegrationOdo *> craw;

    OdoIntervals(int variant, int n, const int32_t *offsets, const double *imu9, const double *state0, const double *params19) {
        auto P       = odo_params(params19);
        const auto v = odo_variant(variant);
        for (int k = 0; k < n; k++) {
            auto p = std::make_shared<PreintegrationOdo>(P, odo_imu(imu9 + 9 * (size_t) offsets[k]), odo_state(state0 + 17 * (size_t) k), v);
            for (int row = offsets[k] + 1; row < offsets[k + 1]; row++) p->addNewImu(odo_imu(imu9 + 9 * (size_t) row));
            pre.push_back(p);
            raw.push_back(p.get());
            craw.push_back(p.get());
        }
    }
    bool integrate(icg_ctx *ctx, char *err, int errlen) {
        std::string e;
        if (PreintegrationOdo::integrateBatch(ctx, raw, &e)) return true;
        set_err(err, errlen, e.c_str());
        return false;
    }
};

// icgh_backend_preint_odo_streams' family (capi_preint_streams.h).  Parameter row of 23: params19, has_station, station[3].  Member row of
// 1125: cur_state 16, its sodo, delta_state 20, delta_time, the time of the current state, the Earth rate 3, jac 361, cov 361, sqrt_info 361.
struct OdoStreamsFamily {
    typedef PreintegrationOdo Obj;
    static constexpr int IMU_W = 9, STATE_W = 17, PARAM_W = 23, MEMBER_W = 17 + 20 + 2 + 3 + 3 * 361;
    static constexpr const char *P1 = "preint_odo", *S = "preint_odo_eval";
    static std::shared_ptr<Obj> make(int variant, const double *row, const int32_t *offsets, const double *imu9, int k, const double *state17) {
        auto P         = odo_params(row);
        P->has_station = row[19] != 0;
        P->station     = Vector3d(row[20], row[21], row[22]);
        auto p = std::make_shared<PreintegrationOdo>(P, odo_imu(imu9 + 9 * (size_t) offsets[k]), odo_state(state17), odo_variant(variant));
        for (int r = offsets[k] + 1; r < offsets[k + 1]; r++) p->addNewImu(odo_imu(imu9 + 9 * (size_t) r));
        return p;
    }
    static IntegrationState state(const double *row) { return odo_state(row); }
    static void put(const Obj &p, double *o) {
        preint_put_state(p.currentState(), o);
        o[16] = p.currentState().sodo;
        put_delta20(p.deltaState(), o + 17);
        o[37] = p.deltaTime(), o[38] = p.currentState().time;
        for (int i = 0; i < 3; i++) o[39 + i] = p.earthRate()[i];
        const vector<double> *m[3] = {&p.jacobian(), &p.covariance(), &p.sqrtInformation()};
        for (int b = 0; b < 3; b++)
            for (size_t i = 0; i < 361; i++) o[42 + 361 * b + i] = i < m[b]->size() ? (*m[b])[i] : 0.0;
    }
    static bool available(int mode) { return mode == 0 ? PreintegrationOdo::integrateBatchAvailable() : PreintegrationOdo::integrateStreamsAvailable(); }
    static bool integrate(int mode, icg_ctx *ctx, const vector<Obj *> &list, std::string *e) {
        return mode == 0 ? PreintegrationOdo::integrateBatch(ctx, list, e) : PreintegrationOdo::integrateStreams(ctx, list, e);
    }
};

// one factor on the host at its evaluation point ep: r 19, J 646 (19x7 | 19x10 | 19x7 | 19x10)
bool evaluate_on_host(const PreintegrationOdoFactor &f, const double *ep, double *r, double *J) {
    const double *pp[4] = {ep, ep + 7, ep + 17, ep + 24};
    double *jj[4]       = {J, J + 133, J + 323, J + 456};
    return f.Evaluate(pp, r, jj);
}
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
        OdoIntervals I(variant, n, offsets, imu9, state0, params19);
        {
            double r[19];
            const double *pp[4] = {eval_point, eval_point + 7, eval_point + 17, eval_point + 24};
            if (PreintegrationOdoFactor(I.pre[0]).Evaluate(pp, r, nullptr)) return 1;
        }
        if (!I.integrate(T.ctx, err, errlen)) return -2;
        for (int k = 0; k < n; k++) {
            const size_t j             = (size_t) k;
            const PreintegrationOdo &p = *I.pre[j];
            preint_put_state(p.currentState(), cur_state + 16 * j);
            put_delta20(p.deltaState(), delta_state + 20 * j);
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
// PreintegrationOdo::evaluateBatch (icg_preint_odo_evaluate_batch).  Outputs per interval for the host / the device path: residuals 19,
// jacobians 646, sqrt_info 361, ok (1 = evaluated; 0 = the factor cannot be evaluated, e.g. singular covariance: zero rows).  Without the
// device entry point in the build nothing is computed: -4.
int icgh_backend_preint_odo_device(int variant, int n, const int32_t *offsets, const double *imu9, const double *state0, const double *params19,
                                   const double *eval_point, double *cur_state, double *residuals_host, double *jacobians_host,
                                   double *residuals_dev, double *jacobians_dev, double *sqrt_info_host, double *sqrt_info_dev,
                                   int32_t *ok_host, int32_t *ok_dev, char *err, int errlen) {
    return guarded(err, errlen, [&] {
        if (!PreintegrationOdo::evaluateBatchAvailable()) {
            set_err(err, errlen, "icg_preint_odo_evaluate_batch is not in this build");
            return -4;
        }
        TempCtx T(0);
        OdoIntervals I(variant, n, offsets, imu9, state0, params19);
        if (!I.integrate(T.ctx, err, errlen)) return -2;
        memset(residuals_host, 0, sizeof(double) * 19 * (size_t) n);
        memset(jacobians_host, 0, sizeof(double) * 646 * (size_t) n);
        for (int k = 0; k < n; k++) {
            const size_t j = (size_t) k;
            preint_put_state(I.pre[j]->currentState(), cur_state + 16 * j);
            const PreintegrationOdoFactor f(I.pre[j]);
            ok_host[k] = evaluate_on_host(f, eval_point + 34 * j, residuals_host + 19 * j, jacobians_host + 646 * j) ? 1 : 0;
            memcpy(sqrt_info_host + 361 * j, I.pre[j]->sqrtInformation().data(), sizeof(double) * 361);
        }
        vector<char> ok;
        std::string e;
        if (!PreintegrationOdo::evaluateBatch(T.ctx, I.craw, eval_point, residuals_dev, jacobians_dev, &ok, &e, sqrt_info_dev)) {
            set_err(err, errlen, e.c_str());
            return -3;
        }
        for (int k = 0; k < n; k++) ok_dev[k] = ok[(size_t) k];
        return 0;
    });
}

// The intervals of many streams, each with its own parameter set, through PreintegrationOdo::integrateBatch (mode 0) or ::integrateStreams
// (mode 1): flow, outputs and return codes in capi_preint_streams.h, the rows in OdoStreamsFamily above.  variant: per interval, 2 or 3.
int icgh_backend_preint_odo_streams(int n, const int32_t *variant, const int32_t *offsets, const double *imu9, const double *state0,
                                    const double *params23, int mode, int passes, int profile, int n_redo, const int32_t *redo, const double *redo_state,
                                    double *members, int32_t *ready, double *pn, int32_t *pn_doubles, double *prof, double *seconds, char *err,
                                    int errlen) {
    return guarded(err, errlen, [&] {
        return preint_streams_entry<OdoStreamsFamily>(n, variant, offsets, imu9, state0, params23, mode, passes, profile, n_redo, redo, redo_state, members, ready,
                                                      pn, pn_doubles, prof, seconds, err, errlen);
    });
}
// 1 when PreintegrationOdo::integrateStreams has its C entry in this build
int icgh_preint_odo_streams_available(void) { return PreintegrationOdo::integrateStreamsAvailable() ? 1 : 0; }

// Host P2 on a GIVEN integration result: the object is built from delta_state 20, jac 361, cov 361, delta_time, the pn rows (pn_rows x 4;
// EarthOdo), the interval's Earth rate iewn3 and the parameters, then evaluated on the host at eval_point.  No device is touched.  Outputs:
// residuals 19, jacobians 646, sqrt_info 361; residuals and jacobians are written only when the factor evaluates.  Returns 1 evaluated, 0 the
// factor refused (singular covariance), negative on an error.  block_sizes5 (optional): the factor's four parameter block sizes and its
// number of residuals.
int icgh_backend_preint_odo_eval_given(int variant, const double *params19, const double *delta_state, const double *jac, const double *cov,
                                       double delta_time, const double *pn, int pn_rows, const double *iewn3, const double *eval_point,
                                       double *residuals, double *jacobians, double *sqrt_info, int32_t *block_sizes5, char *err, int errlen) {
    return guarded(err, errlen, [&] {
        auto P = odo_params(params19);
        IntegrationState st;
        st.bg   = Vector3d(delta_state[10], delta_state[11], delta_state[12]);
        st.ba   = Vector3d(delta_state[13], delta_state[14], delta_state[15]);
        st.sodo = delta_state[19];
        auto p  = std::make_shared<PreintegrationOdo>(P, IMU(), st, odo_variant(variant));
        double cur16[16];
        preint_put_state(st, cur16);
        p->setIntegrationResult(cur16, delta_state, jac, cov, delta_time, pn, variant == 3 ? pn_rows : 0, Vector3d(iewn3[0], iewn3[1], iewn3[2]));
        const PreintegrationOdoFactor f(p);
        if (block_sizes5) {
            const auto &b = f.parameter_block_sizes();
            if (b.size() != 4) return -2;
            for (int k = 0; k < 4; k++) block_sizes5[k] = b[(size_t) k];
            block_sizes5[4] = f.num_residuals();
        }
        if (sqrt_info) memcpy(sqrt_info, p->sqrtInformation().data(), sizeof(double) * 361);
        return evaluate_on_host(f, eval_point, residuals, jacobians) ? 1 : 0;
    });
}

// Timing for profiles/preint_odo_probe.py: the intervals are integrated `reps` times by icg_preint_odo_batch (every pass marks them dirty
// again) and evaluated `reps` times on a HostPool of `threads` threads and by one evaluateBatch call.  out8: device time of the P1 kernel per
// call [ms] (event-timed mean), P1 wall seconds (best), host P2 seconds (best), device P2 wall seconds incl. packing and transfers (best),
// device time of the two P2 kernels per call [ms], max |r_dev - r_host|, max |J_dev - J_host|, factors evaluated.
int icgh_backend_preint_odo_time(int variant, int n, const int32_t *offsets, const double *imu9, const double *state0, const double *params19,
                                 const double *eval_point, int threads, int reps, double *out8, char *err, int errlen) {
    return guarded(err, errlen, [&] {
        if (!PreintegrationOdo::evaluateBatchAvailable()) {
            set_err(err, errlen, "icg_preint_odo_evaluate_batch is not in this build");
            return -4;
        }
        TempCtx T(0);
        OdoIntervals I(variant, n, offsets, imu9, state0, params19);
        vector<std::unique_ptr<PreintegrationOdoFactor>> factors;
        for (const auto &p : I.pre) factors.emplace_back(new PreintegrationOdoFactor(p));
        std::string e;
        const double best_p1 = best_of(reps, [&](int pass) {
            if (pass == 1) icg_prof_enable(T.ctx, 1);
            for (auto *p : I.raw) p->reintegration(IntegrationState(p->startState()));
            return PreintegrationOdo::integrateBatch(T.ctx, I.raw, &e);
        });
        if (best_p1 < 0) {
            set_err(err, errlen, e.c_str());
            return -2;
        }
        const size_t N = (size_t) n;
        vector<double> rh(19 * N), Jh(646 * N), rd(19 * N), Jd(646 * N);
        vector<char> okh(N, 0), okd;
        HostPool pool(threads < 1 ? 1 : threads);
        const double best_host = best_of(reps, [&](int) {
            pool.parallelFor(n, [&](int k) {
                const size_t j = (size_t) k;
                okh[j]         = evaluate_on_host(*factors[j], eval_point + 34 * j, rh.data() + 19 * j, Jh.data() + 646 * j) ? 1 : 0;
            });
            return true;
        });
        const double best_dev = best_of(reps, [&](int) { return PreintegrationOdo::evaluateBatch(T.ctx, I.craw, eval_point, rd.data(), Jd.data(), &okd, &e); });
        if (best_dev < 0) {
            set_err(err, errlen, e.c_str());
            return -3;
        }
        int l1 = 0, l2 = 0;
        double ms1 = 0, ms2 = 0;
        icg_prof_get(T.ctx, "preint_odo", &l1, &ms1);
        icg_prof_get(T.ctx, "preint_odo_eval", &l2, &ms2);
        double dr = 0, dJ = 0, evaluated = 0;
        for (size_t k = 0; k < N; k++) {
            if (okh[k] != okd[k]) {
                set_err(err, errlen, ("host and device disagree on whether factor " + std::to_string(k) + " can be evaluated").c_str());
                return -5;
            }
            evaluated += okh[k] ? 1 : 0;
            for (int i = 0; i < 19; i++) dr = std::max(dr, std::fabs(rd[19 * k + i] - rh[19 * k + i]));
            for (int i = 0; i < 646; i++) dJ = std::max(dJ, std::fabs(Jd[646 * k + i] - Jh[646 * k + i]));
        }
        out8[0] = l1 > 0 ? ms1 / l1 : 0.0, out8[1] = best_p1, out8[2] = best_host, out8[3] = best_dev, out8[4] = l2 > 0 ? ms2 / l2 : 0.0;
        out8[5] = dr, out8[6] = dJ, out8[7] = evaluated;
        return 0;
    });
}

} // extern "C"
