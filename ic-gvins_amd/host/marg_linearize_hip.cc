// MarginalizationLinearizer: see marg_linearize_hip.h.  Reference: factors/marginalization_info.h:153-192.
#include "marg_linearize_hip.h"

#include <algorithm>
#include <cstring>
#include <thread>

// A build of this layer on another implementation of the C ABI may not have the entry point: the reference stays weak (null when absent)
// and linearize() reports it; the product library links libicgvins_hip.so, which defines it.
#pragma weak icg_marg_linearize_batch
#pragma weak icg_marg_linearize_batch_keep
#pragma weak icg_marg_linearized_release

namespace icg {

bool MarginalizationLinearizer::available() { return &icg_marg_linearize_batch != nullptr; }

bool MarginalizationLinearizer::keepAvailable() { return &icg_marg_linearize_batch_keep != nullptr && &icg_marg_linearized_release != nullptr; }

void MarginalizationLinearizer::releaseKept(icg_ctx *ctx) {
    if (ctx && keepAvailable()) (void) icg_marg_linearized_release(ctx);
}

uint64_t MarginalizationLinearizer::linearizeKeep(int n_windows, const int32_t *P, const int32_t *m, const double *H, const double *b, double eps,
                                                  double *Hp, double *bp, double *J0, double *e0, double *evals, double *min_ev_m, int32_t *status,
                                                  std::string *err) {
    auto fail = [&](const std::string &what) {
        if (err) *err = what;
        return (uint64_t) 0;
    };
    if (!device_) return fail("MarginalizationLinearizer::linearizeKeep: device mode only");
    if (!keepAvailable()) return fail("icg_marg_linearize_batch_keep is not in this build");
    if (!ctx_) return fail("MarginalizationLinearizer: no context");
    uint64_t id = 0;
    if (icg_marg_linearize_batch_keep(ctx_, n_windows, P, m, H, b, eps, Hp, bp, J0, e0, evals, min_ev_m, status, &id) != ICG_OK)
        return fail(icg_last_error(ctx_));
    return id;
}

MarginalizationLinearizer::MarginalizationLinearizer(bool device, icg_ctx *ctx, int host_threads) : device_(device), ctx_(ctx) {
    host_threads_ = host_threads > 0 ? host_threads : (int) std::min(16u, std::max(1u, std::thread::hardware_concurrency()));
}

bool MarginalizationLinearizer::linearize(int n_windows, const int32_t *P, const int32_t *m, const double *H, const double *b, double eps,
                                          double *Hp, double *bp, double *J0, double *e0, double *evals, double *min_ev_m, int32_t *status,
                                          std::string *err) {
    auto fail = [&](const std::string &what) {
        if (err) *err = what;
        return false;
    };
    if (device_) {
        if (!available()) return fail("icg_marg_linearize_batch is not in this build");
        if (!ctx_) return fail("MarginalizationLinearizer: no context");
        if (icg_marg_linearize_batch(ctx_, n_windows, P, m, H, b, eps, Hp, bp, J0, e0, evals, min_ev_m, status) != ICG_OK)
            return fail(icg_last_error(ctx_));
        return true;
    }
    if (n_windows <= 0 || !P || !m || !H || !b || !J0 || !e0) return fail("MarginalizationLinearizer: invalid argument");
    const size_t W = (size_t) n_windows;
    vector<size_t> h_off(W + 1, 0), b_off(W + 1, 0), r_off(W + 1, 0), rr_off(W + 1, 0);
    for (size_t w = 0; w < W; w++) {
        if (P[w] <= 0 || m[w] < 0 || m[w] >= P[w]) return fail("MarginalizationLinearizer: window " + std::to_string(w) + ": 0 <= m < P does not hold");
        const size_t r = (size_t) (P[w] - m[w]);
        h_off[w + 1] = h_off[w] + (size_t) P[w] * P[w], b_off[w + 1] = b_off[w] + (size_t) P[w];
        r_off[w + 1] = r_off[w] + r, rr_off[w + 1] = rr_off[w] + r * r;
    }
    auto one = [&](int wi) {
        const size_t w = (size_t) wi, r = (size_t) (P[w] - m[w]);
        vector<double> hp, bpv, j0, e0v, ev;
        double mn = 0;
        int st    = 0;
        linearizeReduced(P[w], m[w], H + h_off[w], b + b_off[w], eps, hp, bpv, j0, e0v, &ev, &mn, &st);
        memcpy(J0 + rr_off[w], j0.data(), sizeof(double) * r * r);
        memcpy(e0 + r_off[w], e0v.data(), sizeof(double) * r);
        if (Hp) memcpy(Hp + rr_off[w], hp.data(), sizeof(double) * r * r);
        if (bp) memcpy(bp + r_off[w], bpv.data(), sizeof(double) * r);
        if (evals) memcpy(evals + r_off[w], ev.data(), sizeof(double) * r);
        if (min_ev_m) min_ev_m[w] = mn;
        if (status) status[w] = st;
    };
    if (host_threads_ <= 1 || n_windows < 2) {
        for (int w = 0; w < n_windows; w++) one(w);
        return true;
    }
    if (!pool_) pool_.reset(new HostPool(host_threads_));
    pool_->parallelFor(n_windows, one);
    return true;
}

} // namespace icg
