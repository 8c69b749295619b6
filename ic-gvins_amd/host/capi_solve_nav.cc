// C entry points of libicgvins_host.so: the navigation factors of the product (nav_factors.h) for tests and probes, alone
// (icgh_backend_nav_eval) and in the batched window solve (icgh_backend_solve_nav_batch: WindowSolverBatch::setDeviceNavFactors).  Flat layouts as
// icg_nav_set / icg_nav_evaluate_resident take them: kind 0..5 per member, its constants at aux + aux_off[f] (aux_off has n + 1 entries),
// its parameter block at points + point_off[f]; results concatenated in member order (nr residuals, nr x width Jacobian entries).
#include <memory>
#include <string>

#include "nav_factors.h"
#include "capi_solve_windows.h"

using namespace icg;

namespace {
std::shared_ptr<ceres::CostFunction> make_nav_factor(int kind, const double *a) {
    switch (kind) {
    case 0: {
        GNSS g;
        g.blh = Vector3d(a[0], a[1], a[2]), g.std = Vector3d(a[3], a[4], a[5]);
        return std::make_shared<GnssFactor>(g, Vector3d(a[6], a[7], a[8]));
    }
    case 1: return std::make_shared<ImuErrorFactor>();
    case 2: return std::make_shared<ImuPosePriorFactor>(a, a + 7);
    case 3: return std::make_shared<ImuMixPriorFactor>(a, a + 9);
    case 4: return std::make_shared<ImuErrorFactor>(2);
    case 5: return std::make_shared<ImuMixPriorFactor>(a, a + 10, 2);
    }
    throw std::runtime_error("kind " + std::to_string(kind) + " is outside 0..5");
}
} // namespace

extern "C" {

// Every member through the product class's Evaluate and, where it is marked, through the Ceres corrector.  Outputs, concatenated: r / J (the
// class's own), r_corr / J_corr (what ResidualBlockInfo::Evaluate holds; equal to r / J for an unmarked member), corr 3 per member
// (sqrt_rho1, alpha_sq_norm, residual_scaling; 1, 0, 1 for an unmarked member), sq_norm per member (sum_k r[k]^2, k ascending), shape 3 per
// member (kind as NavFactor reports it, nr, width).  huber (NULL: no member is marked): huber[f] != 0 marks member f.
//   corr_in == NULL  the marked member carries HuberLoss(huber[f]); r_corr / J_corr are ResidualBlockInfo::Evaluate's, corr is
//                    correctorScalars of that loss at the member's sq_norm
//   corr_in != NULL  the twin of icg_nav_correct_resident: the marked member is corrected with the three scalars at corr_in + 3 f, whatever
//                    they are, in ResidualBlockInfo::Evaluate's operation order; corr returns them
// Any output may be NULL.  -2: a member that is no NavFactor with one block of its width.
int icgh_backend_nav_eval(int n, const int32_t *kind, const int32_t *aux_off, const double *aux, const double *points, const int32_t *point_off,
                          const double *huber, const double *corr_in, double *r, double *J, double *r_corr, double *J_corr, double *corr,
                          double *sq_norm, int32_t *shape, char *err, int errlen) {
    return guarded(err, errlen, [&] {
        size_t ro = 0, jo = 0;
        for (int f = 0; f < n; f++) {
            auto cost       = make_nav_factor(kind[f], aux + aux_off[f]);
            const auto *nav = dynamic_cast<const NavFactor *>(cost.get());
            if (!nav || cost->parameter_block_sizes().size() != 1 || cost->parameter_block_sizes()[0] != nav->navWidth() ||
                cost->num_residuals() != nav->navResiduals()) {
                set_err(err, errlen, ("member " + std::to_string(f) + " is no navigation factor on one block of its width").c_str());
                return -2;
            }
            const int nr = nav->navResiduals(), nc = nav->navWidth();
            if (shape) shape[3 * f] = nav->navKind(), shape[3 * f + 1] = nr, shape[3 * f + 2] = nc;
            vector<double> x(points + point_off[f], points + point_off[f] + nc);
            const double *pp[1] = {x.data()};
            vector<double> rr((size_t) nr), JJ((size_t) nr * nc);
            double *jj[1] = {JJ.data()};
            if (!cost->Evaluate(pp, rr.data(), jj)) return -3;
            {
                vector<double> r2((size_t) nr);
                if (!cost->Evaluate(pp, r2.data(), nullptr) || memcmp(r2.data(), rr.data(), sizeof(double) * (size_t) nr)) return -3;
            }
            double sq = 0;
            for (double v : rr) sq += v * v;
            vector<double> rc = rr, Jc = JJ;
            CorrectorScalars cs{1.0, 0.0, 1.0};
            const bool marked = huber && huber[f] != 0.0;
            if (marked && !corr_in) {
                auto loss = std::make_shared<ceres::HuberLoss>(huber[f]);
                double rho[3];
                loss->Evaluate(sq, rho);
                cs = correctorScalars(sq, rho);
                ResidualBlockInfo info(cost, loss, vector<double *>{x.data()}, vector<int>{});
                if (!info.Evaluate()) return -3;
                rc = info.residuals(), Jc = info.jacobians()[0];
            } else if (marked) {
                cs = CorrectorScalars{corr_in[3 * f], corr_in[3 * f + 1], corr_in[3 * f + 2]};
                for (int c = 0; c < nc; c++) {
                    double rtj = 0;
                    for (int k = 0; k < nr; k++) rtj += rc[(size_t) k] * Jc[(size_t) k * nc + c];
                    for (int k = 0; k < nr; k++) {
                        double &j = Jc[(size_t) k * nc + c];
                        j         = cs.sqrt_rho1 * (j - cs.alpha_sq_norm * rc[(size_t) k] * rtj);
                    }
                }
                for (double &v : rc) v *= cs.residual_scaling;
            }
            if (r) memcpy(r + ro, rr.data(), sizeof(double) * (size_t) nr);
            if (J) memcpy(J + jo, JJ.data(), sizeof(double) * (size_t) nr * nc);
            if (r_corr) memcpy(r_corr + ro, rc.data(), sizeof(double) * (size_t) nr);
            if (J_corr) memcpy(J_corr + jo, Jc.data(), sizeof(double) * (size_t) nr * nc);
            if (corr) corr[3 * f] = cs.sqrt_rho1, corr[3 * f + 1] = cs.alpha_sq_norm, corr[3 * f + 2] = cs.residual_scaling;
            if (sq_norm) sq_norm[f] = sq;
            ro += (size_t) nr, jo += (size_t) nr * nc;
        }
        return 0;
    });
}

// The visual-inertial windows of icgh_backend_solve_preint_batch (variant 0 Normal / 1 Earth: states of 16, mix blocks of 9, the intervals
// integrated here from offsets / imu / params9) and of icgh_backend_solve_preint_odo_batch (variant 2 Odo / 3 EarthOdo: states of 17, mix blocks
// of 10, the integration results GIVEN as delta / jac / cov / dt / iewn / pn_off / pn with params19); the arguments of the variant that is not
// asked for may be NULL.  The same blocks and the same order of the residual blocks as there: the motion factors, the pose prior on state 0,
// the optional marginalization prior, the mix prior on state 0.  With nav_factors != 0 the stand-in priors are the product's navigation
// factors, and two more groups follow:
//   ImuPosePriorFactor(prior_pose0, std 1 / prior_weight) and ImuMixPriorFactor(prior_mix0, std 1 / prior_weight) on state 0
//   an ImuErrorFactor on the last state's mix block
//   a GnssFactor on every state: blh gnss_blh[w] + 3 k, std gnss_std3, lever gnss_lever3, behind HuberLoss(gnss_huber[w]) where that is not 0
// With nav_factors == 0 the windows are exactly those entries' (their stand-in priors, nothing added): the same bits as theirs.
// mode: 0 host; 1 device reduced solve; 2 and device host part; 3 and device prior; 4 = mode 2 plus the device preintegration, 5 = mode 3
// plus it.  device_nav: 1 = setDeviceNavFactors(true); 1 + 16: that switch WITHOUT setDeviceHostPart, which solve() refuses by name (-3).
// nav_on_device (optional out): the navigation factors that were resident on the device in the solve.  states, invdepth, summary4,
// prior_cost, solve_ms as there.  Other modes or variants: -1.  A mode whose C entries are not in the build computes nothing: -4 and the
// entry's name, icg_nav_set's first of all.  -2: the integration failed; -3: solve() failed (err: its message); -5: prepare() or a prior's
// evaluation failed.
int icgh_backend_solve_nav_batch(int W, int variant, const int32_t *n_intervals, const int32_t *const *offsets, const double *const *imu, const double *params9,
                                 const double *const *delta, const double *const *jac, const double *const *cov, const double *const *dt,
                                 const double *const *iewn, const int32_t *const *pn_off, const double *const *pn, const double *params19, double *const *states,
                                 const int32_t *n_fac, const double *const *obs_soa, const int32_t *const *idx_i, const int32_t *const *idx_j,
                                 const int32_t *const *idx_lm, double *const *ext, const int32_t *n_lm, double *const *invdepth, double *td,
                                 const double *const *prior_pose0, const double *const *prior_mix0, double prior_weight, double huber, int iters,
                                 const int32_t *prior_r, const int32_t *prior_nb, const int32_t *const *prior_size, const int32_t *const *prior_index,
                                 const int32_t *const *prior_param, const double *const *prior_x0, const double *const *prior_J0, const double *const *prior_e0,
                                 const int32_t *const *state_const, int nav_factors, const double *const *gnss_blh, const double *gnss_std3,
                                 const double *gnss_lever3, const double *gnss_huber, double *summary4, double *prior_cost, double *solve_ms,
                                 int32_t *nav_on_device, int mode, int device_nav, char *err, int errlen) {
    return guarded(err, errlen, [&] {
        const bool without_parts = device_nav == 1 + 16;
        if (without_parts) device_nav = 1;
        if (mode < 0 || mode > 5 || variant < 0 || variant > 3 || (device_nav != 0 && device_nav != 1)) {
            set_err(err, errlen, "mode must be 0 (host), 1 (device reduced solve), 2 (and device host part), 3 (and device prior), 4 (mode 2 and device "
                                 "preintegration) or 5 (mode 3 and device preintegration); variant 0 .. 3; device_nav 0 or 1 (+ 16)");
            return -1;
        }
        if (nav_on_device) *nav_on_device = 0;
        const VioBatchArgs a{W,       variant,  n_intervals, offsets,  imu,      params9,  delta,       jac,      cov,      dt,           iewn,
                             pn_off,  pn,       params19,    states,   n_fac,    obs_soa,  idx_i,       idx_j,    idx_lm,   ext,          n_lm,
                             invdepth, td,      prior_pose0, prior_mix0, prior_weight, huber, iters,    prior_r,  prior_nb, prior_size,   prior_index,
                             prior_param, prior_x0, prior_J0, prior_e0, nullptr, nullptr,  state_const, nav_factors, gnss_blh, gnss_std3, gnss_lever3,
                             gnss_huber, summary4, prior_cost, solve_ms, nullptr, nullptr, nav_on_device};
        return solve_vio_windows(a, mode, without_parts, device_nav != 0, err, errlen);
    });
}

} // extern "C"
