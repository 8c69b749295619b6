// The one body of icgh_backend_preint_streams (capi_preint.cc) and icgh_backend_preint_odo_streams (capi_preint_odo.cc): the intervals of
// many streams, every one with a parameter set of its own, integrated by integrateBatch (mode 0) or integrateStreams (mode 1), with every
// member the two must agree on, the launches the context's profiler recorded and the wall time around the integrate call.  A family brings
// a traits struct F:
//   Obj                                  Preintegration / PreintegrationOdo
//   IMU_W, STATE_W, PARAM_W, MEMBER_W    doubles per IMU row, start state, parameter row and member row
//   P1, S                                the profiler's names of the integration and of the square-root-information launches
//   make(variant, param_row, offsets, imu, k, state_row), state(state_row), put(obj, member_row),
//   integrate(mode, ctx, list, err), available(mode)
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
#include <chrono>
#include <string>
#include <vector>

#include "capi_util.h"

namespace {

template <class F>
int preint_streams_entry(int n, const int32_t *variant, const int32_t *offsets, const double *imu, const double *state0, const double *params,
                         int mode, int passes, int profile, int n_redo, const int32_t *redo, const double *redo_state, double *members, int32_t *ready,
                         double *pn, int32_t *pn_doubles, double *prof, double *seconds, char *err, int errlen) {
    typedef typename F::Obj Obj;
    if (mode != 0 && mode != 1) throw std::runtime_error("mode " + std::to_string(mode) + " is neither 0 (integrateBatch) nor 1 (integrateStreams)");
    if (n < 1 || passes < 1) throw std::runtime_error("n and passes must be positive");
    TempCtx T(0);
    std::vector<std::shared_ptr<Obj>> pre;
    std::vector<Obj *> raw;
    for (int k = 0; k < n; k++) {
        pre.push_back(F::make(variant[k], params + (size_t) F::PARAM_W * (size_t) k, offsets, imu, k, state0 + (size_t) F::STATE_W * (size_t) k));
        raw.push_back(pre.back().get());
    }
    if (profile) icg_prof_enable(T.ctx, 1);
    std::string e;
    auto timed = [&](double *out) {
        const auto a  = std::chrono::steady_clock::now();
        const bool ok = F::integrate(mode, T.ctx, raw, &e);
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
            F::put(p, members + ((size_t) stage * (size_t) n + (size_t) k) * (size_t) F::MEMBER_W);
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
            for (int k = 0; k < n; k++) raw[(size_t) k]->reintegration(F::state(state0 + (size_t) F::STATE_W * (size_t) k));
        if (!timed(seconds + pass)) {
            if (F::available(mode)) return -2;
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
        raw[(size_t) redo[j]]->reintegration(F::state(redo_state + (size_t) F::STATE_W * (size_t) j));
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
