// C entry point of libicgvins_host.so for WindowSolverBatch::setDevicePrior: a batch of visual-inertial windows, each optionally with a
// marginalization prior given as plain arrays, solved with the prior on the host pool or resident on the device.  For tests and probes.
// The windows are built and solved by solve_vio_windows (capi_solve_windows.h), shared with the entries of capi_solve_preint.cc,
// capi_solve_preint_odo.cc and capi_solve_nav.cc.
#include "capi_solve_windows.h"

using namespace icg;

extern "C" {

// icgh_backend_solve_vio_batch (capi_solve_parts.cc: the same windows, the same leading arguments) with, per window and optionally, a
// marginalization prior and constant states.
//   prior_r[w]       the prior's retained size, 0 = window w has no prior.  The prior has prior_nb[w] blocks; block b has global size
//                    prior_size[w][b] (7 or 9), first local column prior_index[w][b], and is the parameter block prior_param[w][b] of the
//                    window: 2 k = the pose of state k, 2 k + 1 = its mix block.  prior_x0[w] (the blocks' linearization points,
//                    concatenated), prior_J0[w] (r x r row-major), prior_e0[w] (r): the layout of icg_marg_prior_set for one window.
//   prior_robust[w]  != 0: the prior's residual block gets a Huber loss of that delta (such a prior stays on the pool in every mode)
//   state_const[w]   n_intervals[w] + 1 flags (NULL: none): the pose and mix blocks of a flagged state are constant
//   prior_cost       W x 2: the prior's own cost 0.5 |e|^2 (no loss) from its Evaluate at the start and at the end; 0 without a prior
// mode: 0 = host, 1 = device reduced solve, 2 = that and the device host part, 3 = those and the device prior (setDevicePrior); 3 + 16: the
// prior switch with the reduced solve but WITHOUT setDeviceHostPart, which solve() refuses by name (-3).  A mode whose C entries are not in
// the build computes nothing: -4 and the entry's name.  summary4 is W x 4 as there; *solve_ms: the wall time of the solve alone.
int icgh_backend_solve_prior_batch(int W, const int32_t *n_intervals, const int32_t *const *offsets, const double *const *imu, const double *params9,
                                   double *const *states16, const int32_t *n_fac, const double *const *obs_soa, const int32_t *const *idx_i,
                                   const int32_t *const *idx_j, const int32_t *const *idx_lm, double *const *ext, const int32_t *n_lm, double *const *invdepth,
                                   double *td, const double *const *prior_pose0, const double *const *prior_mix0, double prior_weight, double huber, int iters,
                                   const int32_t *prior_r, const int32_t *prior_nb, const int32_t *const *prior_size, const int32_t *const *prior_index,
                                   const int32_t *const *prior_param, const double *const *prior_x0, const double *const *prior_J0,
                                   const double *const *prior_e0, const double *prior_robust, const int32_t *const *state_const, double *summary4,
                                   double *prior_cost, double *solve_ms, int mode, char *err, int errlen) {
    return guarded(err, errlen, [&] {
        const bool without_parts = mode == 3 + 16;
        if (without_parts) mode = 3;
        if (mode < 0 || mode > 3) {
            set_err(err, errlen, "mode must be 0 (host), 1 (device reduced solve), 2 (and device host part) or 3 (and device prior)");
            return -1;
        }
        const VioBatchArgs a{W,       0,        n_intervals, offsets,  imu,      params9,  nullptr,     nullptr,  nullptr,  nullptr,      nullptr,
                             nullptr, nullptr,  nullptr,     states16, n_fac,    obs_soa,  idx_i,       idx_j,    idx_lm,   ext,          n_lm,
                             invdepth, td,      prior_pose0, prior_mix0, prior_weight, huber, iters,    prior_r,  prior_nb, prior_size,   prior_index,
                             prior_param, prior_x0, prior_J0, prior_e0, prior_robust, nullptr, state_const, 0,     nullptr,  nullptr,      nullptr,
                             nullptr, summary4, prior_cost,  solve_ms, nullptr,  nullptr,  nullptr};
        return solve_vio_windows(a, mode, without_parts, false, err, errlen);
    });
}

} // extern "C"
