// M3 for many windows per call: the Schur step on the marginalized pose / mix block and the linearization of the reduced system
// (reference factors/marginalization_info.h:153-192).  Device mode is ONE icg_marg_linearize_batch call (a workgroup per window); host mode
// runs linearizeReduced (factors.h: the arithmetic of MarginalizationInfo) per window on a HostPool.  Both take and return the flat layout
// of the C entry: window w has a P[w] x P[w] row-major H and a b of P[w], concatenated; r = P - m; outputs per window concatenated.
// The C entry is referenced weakly: in a build of this layer on a C ABI without it available() is false and device mode fails by name.
#pragma once
#include <memory>
#include <string>
#include <vector>

#include "factors.h"
#include "host_pool.h"

namespace icg {

class MarginalizationLinearizer {
public:
    static bool available(); // icg_marg_linearize_batch is in this build
    // device: ctx must outlive the calls; host: ctx is not used, host_threads = size of the pool (0: hardware concurrency, at most 16)
    explicit MarginalizationLinearizer(bool device, icg_ctx *ctx = nullptr, int host_threads = 0);
    bool deviceMode() const { return device_; }
    // J0 (sum r^2) and e0 (sum r) are required; Hp, bp, evals (sum r), min_ev_m, status (n_windows) may be null.  status bit 1 (iteration
    // cap) is reported by the device only.  false with *err set on failure; nothing is written then.
    bool linearize(int n_windows, const int32_t *P, const int32_t *m, const double *H, const double *b, double eps, double *Hp, double *bp,
                   double *J0, double *e0, double *evals, double *min_ev_m, int32_t *status, std::string *err = nullptr);
    // Device mode only: the same call through icg_marg_linearize_batch_keep, which also leaves J0 / e0 of every window on the device for
    // MarginalizationPriorSet::set (icg_marg_prior_set_from_kept).  Returns the id of the kept linearization, 0 with *err set on failure.
    // The kept buffer (sum r^2 + sum r doubles) lives until the context's next linearize call of either kind, releaseKept(ctx) or the
    // context's destruction.  The entries are referenced weakly like the one above: keepAvailable() is false on a C ABI without them.
    static bool keepAvailable();
    uint64_t linearizeKeep(int n_windows, const int32_t *P, const int32_t *m, const double *H, const double *b, double eps, double *Hp, double *bp,
                           double *J0, double *e0, double *evals, double *min_ev_m, int32_t *status, std::string *err = nullptr);
    static void releaseKept(icg_ctx *ctx); // icg_marg_linearized_release; nothing without the entry or a context

private:
    bool device_;
    icg_ctx *ctx_;
    int host_threads_;
    std::unique_ptr<HostPool> pool_;
};

} // namespace icg
