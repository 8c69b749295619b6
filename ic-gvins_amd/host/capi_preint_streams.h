// The bodies that the test entries of the two preintegration families share (capi_preint.cc: Preintegration; capi_preint_odo.cc:
// PreintegrationOdo; the *_eval_split entries of capi_solve_preint.cc / capi_solve_preint_odo.cc), each written once over a family record F:
//   Obj, Factor                          Preintegration / PreintegrationOdo and its cost function; the widths are Obj's
//   PARAMS_W                             doubles of the entries' parameter vector (9 / 19); a stream's row has has_station, station[3] behind them:
//                                        with has_station the interval's Earth rate comes from its own start position and [6..8] are not used
//   P1, S                                the profiler's names of the integration and of the square-root-information / evaluation launches
//   params(row), state(state_row)        the flat rows as objects
//   interval(variant, params, offsets, imu, k, state_row)   interval k (it owns the imu rows [offsets[k], offsets[k+1])) from its start state
//   checkStreamVariant(variant)          throws for a variant number that is not the family's
//
// preint_streams_entry, the body of icgh_backend_preint_streams and icgh_backend_preint_odo_streams: the intervals of many streams, every one
// with a parameter set of its own, integrated by integrateBatch (mode 0) or integrateStreams (mode 1), with every member the two must agree
// on, the launches the context's profiler recorded and the wall time around the integrate call.  Member row: cur_state 16 (and its sodo for
// the odometer family), delta_state, delta_time, the time of the current state, the Earth rate 3, jac, cov, sqrt_info.
// The flow: `passes` times (every pass but the first marks all intervals dirty again from their own start states) integrate the list; store
// the members (stage 0); integrate the clean list once more; reintegration(redo_state) of the n_redo intervals `redo` and one more
// integrate; store the members (stage 1).
//   members   2 x n x MEMBER_W          ready  2 x n         pn  2 x total x 4 (interval k from row offsets[k]; pn_doubles 2 x n: how many)
//   profile   1: the context's profiler is on for the whole entry (every launch carries two event records); 0: off, prof comes back as zeros
//   prof      3 x 4 = launches and milliseconds of P1, launches and milliseconds of S, cumulative, after the passes / the clean call / the redo
//   seconds   passes + 3: the wall time around every pass's integrate call, around the clean call, around the redo call, and (mode 0) of one
//             host loop over all intervals that forms the square-root information again, which is what integrateBatch spends on it
// Returns 0; -2 an integrate call failed (err); -4 the mode's entry point is not in this build: err is what the integrate call said (it
// names the entry), and stage 0 of members / ready / pn shows the objects as that call left them (not integrated).
#pragma once
#include <algorithm>
#include <chrono>
#include <cmath>
#include <string>
#include <vector>

#include "capi_util.h"
#include "host_pool.h"

namespace {

// The n intervals of the flat arrays as objects (imu: total x IMU_ROW; offsets: n+1; state0: n x STATE0_ROW; params: PARAMS_W); integrate(): one
// *_batch launch for all of them.
template <class F> struct PreintIntervals {
    typedef typename F::Obj Obj;
    std::vector<std::shared_ptr<Obj>> pre;
    std::vector<Obj *> raw;
    std::vector<const Obj *> craw;

    PreintIntervals(int variant, int n, const int32_t *offsets, const double *imu, const double *state0, const double *params) {
        auto P = F::params(params);
        for (int k = 0; k < n; k++) {
            pre.push_back(F::interval(variant, P, offsets, imu, k, state0 + (size_t) Obj::STATE0_ROW * (size_t) k));
            raw.push_back(pre.back().get());
            craw.push_back(pre.back().get());
        }
    }
    bool integrate(icg_ctx *ctx, char *err, int errlen) {
        std::string e;
        if (Obj::integrateBatch(ctx, raw, &e)) return true;
        set_err(err, errlen, e.c_str());
        return false;
    }
};

// one evaluation at the point ep (pose0[7], mix0[M], pose1[7], mix1[M]) into r (N) and J (NUM_JAC = N x 7 | N x M | N x 7 | N x M); eval(pp, r, jj)
// is the factor's Evaluate or one of the object's evaluate members
template <class P, class E> bool preint_evaluate_at(E &&eval, const double *ep, double *r, double *J) {
    constexpr int N = P::NUM_STATE, M = P::NUM_MIX;
    const double *pp[4] = {ep, ep + 7, ep + 7 + M, ep + 14 + M};
    double *jj[4]       = {J, J + N * 7, J + N * (7 + M), J + N * (14 + M)};
    return eval(pp, r, jj);
}
template <class Factor> bool evaluate_on_host(const Factor &f, const double *ep, double *r, double *J) {
    typedef typename std::decay<decltype(f.preintegration())>::type P;
    return preint_evaluate_at<P>([&](const double *const *pp, double *rr, double **jj) { return f.Evaluate(pp, rr, jj); }, ep, r, J);
}

// The per-factor body of the two *_eval_split entries: the factor at its point twice on the host, by evaluate (r_eval, J_eval) and by
// correctionQuaternion / earthRateQuaternion + evaluateGiven (r_given, J_given; q_corr_in / q_nn_in, when not null, in the accessors' place),
// with the accessors' quaternions, the square-root information and env 4 (gravity, iewn).  All pointers are the factor's own rows.
template <class P>
bool preint_eval_split_factor(const P &p, const double *ep, const double *q_corr_in, const double *q_nn_in, double *r_eval, double *J_eval,
                              double *r_given, double *J_given, double *q_corr, double *q_nn, double *sqrt_info, double *env) {
    p.correctionQuaternion(ep + 7, q_corr);
    p.earthRateQuaternion(q_nn);
    const bool a = preint_evaluate_at<P>([&](const double *const *pp, double *r, double **jj) { return p.evaluate(pp, r, jj); }, ep, r_eval, J_eval);
    const bool b = preint_evaluate_at<P>(
        [&](const double *const *pp, double *r, double **jj) { return p.evaluateGiven(pp, q_corr_in ? q_corr_in : q_corr, q_nn_in ? q_nn_in : q_nn, r, jj); },
        ep, r_given, J_given);
    memcpy(sqrt_info, p.sqrtInformation().data(), sizeof(double) * P::NUM_COV);
    env[0] = p.gravity();
    for (int i = 0; i < 3; i++) env[1 + i] = p.earthRate()[i];
    return a && b;
}

// The body of icgh_backend_preint_device / icgh_backend_preint_odo_device: the same integration, evaluated twice on the SAME objects, once per
// factor on the host (Factor::Evaluate) and once through Obj::evaluateBatch, so both paths can be compared on identical inputs.  Outputs per
// interval for the host / the device path: residuals N, jacobians NUM_JAC, sqrt_info N x N (the host's sqrt_information_ / the kernel's), ok
// (1 = evaluated; 0 = the factor cannot be evaluated, e.g. singular covariance: zero rows).  Without the device entry point in the build
// nothing is computed: -4 and its name.  -2: the integration failed; -3: evaluateBatch failed.
template <class F>
int preint_device_entry(int variant, int n, const int32_t *offsets, const double *imu, const double *state0, const double *params,
                        const double *eval_point, double *cur_state, double *residuals_host, double *jacobians_host, double *residuals_dev,
                        double *jacobians_dev, double *sqrt_info_host, double *sqrt_info_dev, int32_t *ok_host, int32_t *ok_dev, char *err, int errlen) {
    typedef typename F::Obj Obj;
    constexpr size_t N = Obj::NUM_STATE, NN = Obj::NUM_COV, JAC = Obj::NUM_JAC, POINT = Obj::NUM_POINT;
    if (!Obj::evaluateBatchAvailable()) {
        set_err(err, errlen, (std::string(Obj::EVAL_NAME) + " is not in this build").c_str());
        return -4;
    }
    TempCtx T(0);
    PreintIntervals<F> I(variant, n, offsets, imu, state0, params);
    if (!I.integrate(T.ctx, err, errlen)) return -2;
    memset(residuals_host, 0, sizeof(double) * N * (size_t) n);
    memset(jacobians_host, 0, sizeof(double) * JAC * (size_t) n);
    for (size_t k = 0; k < (size_t) n; k++) {
        preint_put_state(I.pre[k]->currentState(), cur_state + 16 * k);
        const typename F::Factor f(I.pre[k]);
        ok_host[k] = evaluate_on_host(f, eval_point + POINT * k, residuals_host + N * k, jacobians_host + JAC * k) ? 1 : 0;
        memcpy(sqrt_info_host + NN * k, I.pre[k]->sqrtInformation().data(), sizeof(double) * NN);
    }
    std::vector<char> ok;
    std::string e;
    if (!Obj::evaluateBatch(T.ctx, I.craw, eval_point, residuals_dev, jacobians_dev, &ok, &e, sqrt_info_dev)) {
        set_err(err, errlen, e.c_str());
        return -3;
    }
    for (int k = 0; k < n; k++) ok_dev[k] = ok[(size_t) k];
    return 0;
}

// The body of the two timing entries (profiles/preint_eval_probe.py, profiles/preint_odo_probe.py): the intervals are integrated by one
// *_batch launch (time_p1: `reps` times, every pass marking them dirty again), then evaluated `reps` times (a) by Factor::Evaluate, one call per
// factor, on a HostPool of `threads` threads and (b) by one Obj::evaluateBatch call.  out8: device time of the P1 kernel per call [ms]
// (event-timed mean) and P1 wall seconds (best), both 0 without time_p1; host P2 seconds (best of reps); evaluateBatch wall seconds incl.
// packing and transfers (best); device time of the two P2 kernels per call [ms] (mean over reps, event-timed); max |r_dev - r_host|;
// max |J_dev - J_host|; factors evaluated.
template <class F>
int preint_time_entry(bool time_p1, int variant, int n, const int32_t *offsets, const double *imu, const double *state0, const double *params,
                      const double *eval_point, int threads, int reps, double *out8, char *err, int errlen) {
    typedef typename F::Obj Obj;
    constexpr size_t NS = Obj::NUM_STATE, JAC = Obj::NUM_JAC, POINT = Obj::NUM_POINT;
    if (!Obj::evaluateBatchAvailable()) {
        set_err(err, errlen, (std::string(Obj::EVAL_NAME) + " is not in this build").c_str());
        return -4;
    }
    TempCtx T(0);
    PreintIntervals<F> I(variant, n, offsets, imu, state0, params);
    std::vector<std::unique_ptr<typename F::Factor>> factors;
    for (const auto &p : I.pre) factors.emplace_back(new typename F::Factor(p));
    std::string e;
    double best_p1 = 0;
    if (time_p1)
        best_p1 = best_of(reps, [&](int pass) {
            if (pass == 1) icg_prof_enable(T.ctx, 1); // (the timed passes carry the event records)
            for (auto *p : I.raw) p->reintegration(icg::IntegrationState(p->startState()));
            return Obj::integrateBatch(T.ctx, I.raw, &e);
        });
    else if (!Obj::integrateBatch(T.ctx, I.raw, &e))
        best_p1 = -1;
    if (best_p1 < 0) {
        set_err(err, errlen, e.c_str());
        return -2;
    }
    const size_t N = (size_t) n;
    std::vector<double> rh(NS * N), Jh(JAC * N), rd(NS * N), Jd(JAC * N);
    std::vector<char> okh(N, 0), okd;
    icg::HostPool pool(threads < 1 ? 1 : threads);
    const double best_host = best_of(reps, [&](int) {
        pool.parallelFor(n, [&](int k) {
            const size_t j = (size_t) k;
            okh[j]         = evaluate_on_host(*factors[j], eval_point + POINT * j, rh.data() + NS * j, Jh.data() + JAC * j) ? 1 : 0;
        });
        return true;
    });
    const double best_dev = best_of(reps, [&](int pass) {
        if (pass == 1 && !time_p1) icg_prof_enable(T.ctx, 1);
        return Obj::evaluateBatch(T.ctx, I.craw, eval_point, rd.data(), Jd.data(), &okd, &e);
    });
    if (best_dev < 0) {
        set_err(err, errlen, e.c_str());
        return -3;
    }
    int l1 = 0, l2 = 0;
    double ms1 = 0, ms2 = 0;
    if (time_p1) icg_prof_get(T.ctx, F::P1, &l1, &ms1);
    icg_prof_get(T.ctx, F::S, &l2, &ms2);
    double dr = 0, dJ = 0, evaluated = 0;
    for (size_t k = 0; k < N; k++) {
        if (okh[k] != okd[k]) {
            set_err(err, errlen, ("host and device disagree on whether factor " + std::to_string(k) + " can be evaluated").c_str());
            return -5;
        }
        evaluated += okh[k] ? 1 : 0;
        for (size_t i = 0; i < NS; i++) dr = std::max(dr, std::fabs(rd[NS * k + i] - rh[NS * k + i]));
        for (size_t i = 0; i < JAC; i++) dJ = std::max(dJ, std::fabs(Jd[JAC * k + i] - Jh[JAC * k + i]));
    }
    out8[0] = l1 > 0 ? ms1 / l1 : 0.0, out8[1] = best_p1, out8[2] = best_host, out8[3] = best_dev, out8[4] = l2 > 0 ? ms2 / l2 : 0.0;
    out8[5] = dr, out8[6] = dJ, out8[7] = evaluated;
    return 0;
}

template <class F>
int preint_streams_entry(int n, const int32_t *variant, const int32_t *offsets, const double *imu, const double *state0, const double *params,
                         int mode, int passes, int profile, int n_redo, const int32_t *redo, const double *redo_state, double *members, int32_t *ready,
                         double *pn, int32_t *pn_doubles, double *prof, double *seconds, char *err, int errlen) {
    typedef typename F::Obj Obj;
    if (mode != 0 && mode != 1) throw std::runtime_error("mode " + std::to_string(mode) + " is neither 0 (integrateBatch) nor 1 (integrateStreams)");
    if (n < 1 || passes < 1) throw std::runtime_error("n and passes must be positive");
    constexpr int STATE_W = Obj::STATE0_ROW, PARAM_W = F::PARAMS_W + 4, MEMBER_W = 16 + (Obj::HAS_ODO ? 1 : 0) + Obj::NUM_DELTA + 5 + 3 * Obj::NUM_COV;
    TempCtx T(0);
    std::vector<std::shared_ptr<Obj>> pre;
    std::vector<Obj *> raw;
    for (int k = 0; k < n; k++) {
        const double *row = params + (size_t) PARAM_W * (size_t) k;
        F::checkStreamVariant(variant[k]);
        auto P         = F::params(row);
        P->has_station = row[F::PARAMS_W] != 0;
        P->station     = icg::Vector3d(row[F::PARAMS_W + 1], row[F::PARAMS_W + 2], row[F::PARAMS_W + 3]);
        pre.push_back(F::interval(variant[k], P, offsets, imu, k, state0 + (size_t) STATE_W * (size_t) k));
        raw.push_back(pre.back().get());
    }
    auto available = [&] { return mode == 0 ? Obj::integrateBatchAvailable() : Obj::integrateStreamsAvailable(); };
    auto put       = [&](const Obj &p, double *o) {
        preint_put_state(p.currentState(), o);
        o += 16;
        if (Obj::HAS_ODO) *o++ = p.currentState().sodo;
        Obj::deltaRow(p.deltaState(), o);
        o += Obj::NUM_DELTA;
        o[0] = p.deltaTime(), o[1] = p.currentState().time;
        for (int i = 0; i < 3; i++) o[2 + i] = p.earthRate()[i];
        const std::vector<double> *m[3] = {&p.jacobian(), &p.covariance(), &p.sqrtInformation()};
        for (int b = 0; b < 3; b++) memcpy(o + 5 + Obj::NUM_COV * b, m[b]->data(), sizeof(double) * Obj::NUM_COV);
    };
    if (profile) icg_prof_enable(T.ctx, 1);
    std::string e;
    auto timed = [&](double *out) {
        const auto a  = std::chrono::steady_clock::now();
        const bool ok = mode == 0 ? Obj::integrateBatch(T.ctx, raw, &e) : Obj::integrateStreams(T.ctx, raw, &e);
        *out          = std::chrono::duration<double>(std::chrono::steady_clock::now() - a).count();
        if (!ok) set_err(err, errlen, e.c_str());
        return ok;
    };
    auto counts = [&](double *out4) {
        int l1 = 0, l2 = 0;
        double ms1 = 0, ms2 = 0;
        icg_prof_get(T.ctx, F::P1, &l1, &ms1);
        icg_prof_get(T.ctx, F::S, &l2, &ms2);
        out4[0] = l1, out4[1] = ms1, out4[2] = l2, out4[3] = ms2;
    };
    const size_t total = (size_t) offsets[n];
    auto store         = [&](int stage) {
        for (int k = 0; k < n; k++) {
            const Obj &p = *raw[(size_t) k];
            put(p, members + ((size_t) stage * (size_t) n + (size_t) k) * (size_t) MEMBER_W);
            ready[(size_t) stage * (size_t) n + (size_t) k] = p.ready() ? 1 : 0;
            const std::vector<double> &rows = p.pnRows();
            const size_t room               = 4 * (size_t) (offsets[k + 1] - offsets[k]);
            const size_t cnt                = rows.size() < room ? rows.size() : room;
            pn_doubles[(size_t) stage * (size_t) n + (size_t) k] = (int32_t) rows.size();
            if (cnt) memcpy(pn + 4 * ((size_t) stage * total + (size_t) offsets[k]), rows.data(), sizeof(double) * cnt);
        }
    };
    for (int pass = 0; pass < passes; pass++) {
        if (pass > 0)
            for (int k = 0; k < n; k++) raw[(size_t) k]->reintegration(F::state(state0 + (size_t) STATE_W * (size_t) k));
        if (!timed(seconds + pass)) {
            if (available()) return -2;
            store(0); // (the objects as the refused call left them: not integrated)
            return -4;
        }
    }
    counts(prof);
    store(0);
    if (!timed(seconds + passes)) return -2;
    counts(prof + 4);
    for (int j = 0; j < n_redo; j++) {
        if (redo[j] < 0 || redo[j] >= n) throw std::runtime_error("redo[" + std::to_string(j) + "] = " + std::to_string(redo[j]) + " is not an interval");
        raw[(size_t) redo[j]]->reintegration(F::state(redo_state + (size_t) STATE_W * (size_t) j));
    }
    if (!timed(seconds + passes + 1)) return -2;
    counts(prof + 8);
    store(1);
    seconds[passes + 2] = 0.0;
    if (mode == 0) {
        const auto a = std::chrono::steady_clock::now();
        for (Obj *p : raw) p->recomputeSqrtInformation();
        seconds[passes + 2] = std::chrono::duration<double>(std::chrono::steady_clock::now() - a).count();
    }
    return 0;
}

} // namespace
