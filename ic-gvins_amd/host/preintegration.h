// Preintegration of boundary B1 (P1 on device; P2 on host per factor, or batched on device): reference
// preintegration/preintegration{,_base,_normal,_earth}.{h,cc}, preintegration_factor.h.  One class template, PreintegrationT, over a family
// record: the 15-state family (Normal / Earth) is here, the 19-state odometer family in preintegration_odo.h.  Implemented, and instantiated
// for both, in preintegration_hip.cc (its small-matrix helpers in preint_common.h); PreintegrationSetT in preint_set_hip.cc.
#pragma once
#include <cstring>
#include <memory>
#include <string>
#include <utility>
#include <vector>

#include "../../include/icgvins_hip.h"
#include "ceres_compat.h"
#include "types.h"

namespace icg {

using std::vector;

struct IMU { // common/types.h:48-56
    double time, dt;
    Vector3d dtheta, dvel;
    double odovel{0};
};
struct Quaterniond {
    double x{0}, y{0}, z{0}, w{1};
};
struct IntegrationState { // preintegration/integration_state.h:35-52 (fields used by the Normal/Earth variants)
    double time{0};
    Vector3d p;
    Quaterniond q;
    Vector3d v, bg, ba;
    Vector3d sg, sa; // gyroscope / accelerometer scale factors (used by MISC::insMechanization when iswithscale)
    double sodo{0};  // odometer scale factor (written out by MISC::writeNavResult; estimated by the odometer variants, preintegration_odo.h)
    Vector3d s;      // preintegrated distance of the odometer variants (integration_state.h:45); zero elsewhere
};
struct IntegrationParameters { // integration_state.h:67-88
    double acc_vrw{0}, gyr_arw{0}, gyr_bias_std{0}, acc_bias_std{0}, corr_time{1}, gravity{9.8};
    Vector3d iewn; // Earth rotation in the local frame, Earth::iewn(station, p) — explicit here (SURVEY.md hazard H9)
    // when set, every (re)integration derives its own Earth rate from the interval's start position, as
    // PreintegrationEarth::resetState does (preintegration_earth.cc:319-321); otherwise `iewn` above is used as given
    bool has_station{false};
    Vector3d station;
    // the odometer variants only (preintegration_odo.h; integration_state.h:82-86): white noise of the odometer [m/s], random walk of its scale
    // factor, installation angles between the body and the vehicle frame [rad], lever arm of the odometer in the body frame [m]
    Vector3d odo_std;
    double odo_srw{0};
    Vector3d abv, lodo;
};

// The 16 doubles every state row begins with: p3, q4 (x, y, z, w), v3, bg3, ba3.
inline void stateToArray16(const IntegrationState &s, double *a) {
    a[0] = s.p[0], a[1] = s.p[1], a[2] = s.p[2];
    a[3] = s.q.x, a[4] = s.q.y, a[5] = s.q.z, a[6] = s.q.w;
    for (int i = 0; i < 3; i++) {
        a[7 + i]  = s.v[i];
        a[10 + i] = s.bg[i];
        a[13 + i] = s.ba[i];
    }
}
inline void stateFromArray16(const double *a, IntegrationState &s) {
    s.p  = Vector3d(a[0], a[1], a[2]);
    s.q  = Quaterniond{a[3], a[4], a[5], a[6]};
    s.v  = Vector3d(a[7], a[8], a[9]);
    s.bg = Vector3d(a[10], a[11], a[12]);
    s.ba = Vector3d(a[13], a[14], a[15]);
}

// What one preintegration family is: the widths of its rows, its variant numbers, its C entries and what they read of an object.
//   NUM_STATE error state, NUM_MIX mix block, NUM_DELTA delta_state row, IMU_ROW / STATE0_ROW / PARAMS_ROW the rows of the *_batch entries
//   PLAIN_VARIANT / EARTH_VARIANT   the variant without / with pn rows and an Earth-rate quaternion
//   HAS_ODO             the odometer rows (ds, dsodo) behind the 15 common ones
//   PN_EVERY_VARIANT    pn_ takes the rows of the call's buffer for every variant, not for the Earth one alone
//   batchEntry / paramsEntry / evalEntry   the C entry, null when this build has none (only where the reference is weak); *_NAME its name
//   imuRow, state0Row, paramsRow, deltaRow   the rows of the C entries; deltaFromRow the way back (inline: the drivers pack a row per sample)
// The 15-state family: Normal / Earth (the Normal variant keeps the zero pn rows of the call's buffer).
struct PreintegrationFamily {
    enum Variant { NORMAL = 0, EARTH = 1 };
    static constexpr Variant PLAIN_VARIANT = NORMAL, EARTH_VARIANT = EARTH;
    static constexpr int NUM_STATE = 15, NUM_MIX = 9, NUM_DELTA = 16, IMU_ROW = 8, STATE0_ROW = 16, PARAMS_ROW = 9;
    static constexpr bool HAS_ODO = false, PN_EVERY_VARIANT = true;
    static constexpr const char *BATCH_NAME = "icg_preint_batch", *PARAMS_NAME = "icg_preint_batch_params", *EVAL_NAME = "icg_preint_evaluate_batch";
    static decltype(&icg_preint_batch) batchEntry();
    static decltype(&icg_preint_batch_params) paramsEntry();
    static decltype(&icg_preint_evaluate_batch) evalEntry();
    static void imuRow(const IMU &s, double *row8) {
        const double v[8] = {s.time, s.dt, s.dtheta[0], s.dtheta[1], s.dtheta[2], s.dvel[0], s.dvel[1], s.dvel[2]};
        memcpy(row8, v, sizeof v);
    }
    static void state0Row(const IntegrationState &start, double *row16) { stateToArray16(start, row16); }
    static void paramsRow(const IntegrationParameters &P, const Vector3d &iewn, double *row9) {
        const double v[9] = {P.gyr_arw, P.acc_vrw, P.gyr_bias_std, P.acc_bias_std, P.corr_time, P.gravity, iewn[0], iewn[1], iewn[2]};
        memcpy(row9, v, sizeof v);
    }
    static void deltaRow(const IntegrationState &delta, double *row16) { stateToArray16(delta, row16); }
    static void deltaFromRow(const double *row16, IntegrationState &delta) { stateFromArray16(row16, delta); }
};

// One IMU (+ odometer) interval between two time nodes.  (Re)integration of many intervals is ONE batched device call.  With N = NUM_STATE and
// M = NUM_MIX of the family F (15 and 9; 19 and 10 for the odometer family):
template <class F> class PreintegrationT : public F {
public:
    using Variant = typename F::Variant;
    // widths besides the family's: evaluation point (pose0 mix0 pose1 mix1), whitened Jacobians of one factor, jac / cov / sqrt_info
    static constexpr int NUM_POINT = 2 * (7 + F::NUM_MIX), NUM_JAC = F::NUM_STATE * NUM_POINT, NUM_COV = F::NUM_STATE * F::NUM_STATE;
    PreintegrationT(std::shared_ptr<IntegrationParameters> parameters, const IMU &imu0, const IntegrationState &state, Variant v);
    void addNewImu(const IMU &imu) { imu_buffer_.push_back(imu); dirty_ = true; }
    void reintegration(const IntegrationState &state);
    const Vector3d &earthRate() const { return iewn_; }
    // integrate every dirty interval of the list: one *_batch launch per (variant, parameter values) group
    static bool integrateBatch(icg_ctx *ctx, const vector<PreintegrationT *> &list, std::string *err = nullptr);
    static bool integrateBatchAvailable(); // the family's *_batch entry is in this build
    // integrateBatch for the intervals of MANY streams: every dirty interval of the list in ONE *_batch_params call per variant present,
    // whatever the parameter values (each interval brings its own row: its Earth rate, gravity, noise figures), and the square-root
    // information comes down with the result (the device forms it behind the integration; updateSqrtInformation does not run).  Every member
    // is afterwards what integrateBatch leaves, bit for bit.  The C entry is referenced weakly: without it integrateStreamsAvailable() is
    // false and integrateStreams fails by the entry's name and integrates nothing.
    static bool integrateStreams(icg_ctx *ctx, const vector<PreintegrationT *> &list, std::string *err = nullptr);
    static bool integrateStreamsAvailable(); // the family's *_batch_params entry is in this build
    // The object as if integrateBatch had returned this result (delta_state NUM_DELTA and jac / cov N x N in the *_batch entry's layout, pn
    // rows of 4 or null, iewn the interval's Earth rate): the host P2 can then be exercised, and pinned against the reference, without a device.
    void setIntegrationResult(const double *cur16, const double *delta, const double *jac, const double *cov, double delta_time, const double *pn,
                              int pn_rows, const Vector3d &iewn);
    // P2 on the device: residual N (and, unless `jacobians` is null, the Jacobians NUM_JAC = N x 7 | N x M | N x 7 | N x M) of every factor of
    // the list at its evaluation point (points: n x NUM_POINT = pose0[7] mix0[M] pose1[7] mix1[M]) through the *_evaluate_batch entry, one call
    // per variant present.  ok[k] = 0 (and zero rows) for a factor that is not integrated for its current buffer / start state or whose
    // covariance is singular: the two conditions under which evaluate() returns false.  sqrt_info (optional, n x N x N): the square-root
    // information the device formed.  Returns false with *err set when a call fails or the entry point is not in this build.
    static bool evaluateBatch(icg_ctx *ctx, const vector<const PreintegrationT *> &list, const double *points, double *residuals, double *jacobians,
                              vector<char> *ok, std::string *err = nullptr, double *sqrt_info = nullptr);
    static bool evaluateBatchAvailable(); // the family's *_evaluate_batch entry is in this build
    const IntegrationState &startState() const { return start_state_; }
    const IntegrationState &currentState() const { return current_state_; }
    const IntegrationState &deltaState() const { return delta_state_; } // the odometer family: with s and sodo
    double deltaTime() const { return delta_time_; }
    const vector<IMU> &imuBuffer() const { return imu_buffer_; }
    // PreintegrationFactor::Evaluate body (preintegration_factor.h:45-69): residual N, Jacobians N x 7, N x M, N x 7, N x M.  false (and
    // nothing written) while the interval is not integrated or its covariance is singular.
    bool evaluate(const double *const *parameters, double *residuals, double **jacobians) const;
    // The only two places of evaluate() where sin / cos / sqrt enter, as unit quaternions (x, y, z, w), formed with evaluate()'s own
    // expressions: the bias correction of delta q at mix0 (v3, bg3, ba3[, sodo]), rotvec2quat(dq_dbg (bg0 - delta.bg)), and the Earth
    // variant's rotvec2quat(-iewn T), a constant of the integration result (identity, and unused, for the plain variant).
    void correctionQuaternion(const double *mix0, double q_xyzw[4]) const;
    void earthRateQuaternion(double q_xyzw[4]) const;
    // evaluate() with the two quaternions given: everything that is left is + - * / in a fixed order.  evaluate() is
    // correctionQuaternion + earthRateQuaternion + evaluateGiven; a caller that evaluates on the device (the family's *_set /
    // *_evaluate_resident entries) ships the quaternions instead of calling sin / cos there.
    bool evaluateGiven(const double *const *parameters, const double q_corr[4], const double q_nn[4], double *residuals, double **jacobians) const;
    Variant variant() const { return variant_; }
    const vector<double> &sqrtInformation() const { return sqrt_information_; } // N x N row-major; zeros while the covariance is singular
    // what a resident set packs besides deltaState(), deltaTime(), sqrtInformation() and earthRate()
    bool ready() const { return !dirty_ && sqrt_information_ok_; } // integrated for the current buffer / start state, covariance not singular
    // forms the square-root information from the covariance on the host again, as integrateBatch does for every result it brings down (the
    // same arithmetic on the same data: nothing changes); for probes that time that loop
    void recomputeSqrtInformation() { updateSqrtInformation(); }
    const vector<double> &jacobian() const { return jacobian_; }     // N x N row-major
    const vector<double> &covariance() const { return covariance_; } // N x N row-major
    double gravity() const { return parameters_->gravity; }
    const vector<double> &pnRows() const { return pn_; } // Earth variant: rows of 4 (dt, position); evaluate() sums the complete rows

private:
    std::shared_ptr<IntegrationParameters> parameters_;
    Variant variant_;
    vector<IMU> imu_buffer_;
    IntegrationState start_state_, current_state_, delta_state_;
    double delta_time_{0};
    void refreshEarthRate();
    void updateSqrtInformation();
    // setIntegrationResult without the square-root information (integrateStreams takes that from the device)
    void storeIntegrationResult(const double *cur16, const double *delta, const double *jac, const double *cov, double delta_time, const double *pn,
                                int pn_rows, const Vector3d &iewn);
    // the batch drivers' two halves: the rows of the dirty intervals `todo` for one call, and that call's rows back into the objects (S =
    // null: the square-root information is formed here)
    static void stageIntervals(const vector<PreintegrationT *> &todo, vector<int32_t> &offsets, vector<double> &imu, vector<double> &state0);
    static void storeIntervals(const vector<PreintegrationT *> &todo, int variant, const vector<int32_t> &offsets, const vector<double> &cur,
                               const vector<double> &del, const vector<double> &jac, const vector<double> &cov, const vector<double> &dt,
                               const vector<double> &pn, const double *S, const int32_t *status);
    vector<double> jacobian_, covariance_, pn_; // N x N, N x N, (n-1) x 4
    vector<double> sqrt_information_;            // N x N, of covariance_ (zeros until an integration result arrives)
    bool sqrt_information_ok_{false};
    Vector3d iewn_; // this interval's Earth rate: P1 (device) and P2 (evaluate) use the same value
    bool dirty_{true};
};
using Preintegration = PreintegrationT<PreintegrationFamily>;

template <class F> class PreintegrationFactorT : public ceres::CostFunction {
public:
    explicit PreintegrationFactorT(std::shared_ptr<PreintegrationT<F>> preintegration) : preintegration_(std::move(preintegration)) {
        *mutable_parameter_block_sizes() = std::vector<int32_t>{7, F::NUM_MIX, 7, F::NUM_MIX}; // numBlocksParameters (normal :148-150, odo :165-167)
        set_num_residuals(F::NUM_STATE);
    }
    bool Evaluate(const double *const *parameters, double *residuals, double **jacobians) const override {
        return preintegration_->evaluate(parameters, residuals, jacobians);
    }
    // what a solver that evaluates the factor on the device (WindowSolverBatch::setDevicePreintegration) packs its resident set from
    const PreintegrationT<F> &preintegration() const { return *preintegration_; }

private:
    std::shared_ptr<PreintegrationT<F>> preintegration_;
};
using PreintegrationFactor = PreintegrationFactorT<PreintegrationFamily>;

// The preintegration factors of many windows resident on the device for a solve (P = Preintegration: icg_preint_set /
// icg_preint_evaluate_resident; P = PreintegrationOdo: icg_preint_odo_set / icg_preint_odo_evaluate_resident; each family has its own
// resident set in the context, both may be resident at once): set() at the head of the solve, pack() + evaluateResident() per LM point.  The
// device gets the host's square-root information and the two quaternions of P::evaluate that need sin / cos (earthRateQuaternion with the
// set, correctionQuaternion with every point); its residuals, Jacobians and squared norms are then the bits of P::evaluate.  The results stay
// on the device for icg_reproj_host_parts_build_preint*; only one squared norm per factor comes back.  The C entries are referenced weakly,
// per family: in a build of this layer on a C ABI without them available() is false, missingEntry() names the first that is absent and set()
// fails by that name.  Implemented, and instantiated for the two classes, in preint_set_hip.cc.
template <class P> class PreintegrationSetT {
public:
    static bool available();
    static const char *missingEntry(); // nullptr when available()
    // every factor must be ready() (integrated, covariance not singular); the objects must outlive the set's use
    bool set(icg_ctx *ctx, const vector<const P *> &list, std::string *err = nullptr);
    // factor f's evaluation point (pose0[7], mix0, pose1[7], mix1) and its correction quaternion to their places (any thread, before the call)
    void pack(size_t f, const double *const *parameters);
    bool evaluateResident(bool want_jac, double *sq_norm, std::string *err = nullptr);
    int factors() const { return (int) list_.size(); }

private:
    icg_ctx *ctx_{nullptr};
    vector<const P *> list_;
    vector<double> points_, q_corr_;
};
using PreintegrationSet = PreintegrationSetT<Preintegration>;

} // namespace icg
