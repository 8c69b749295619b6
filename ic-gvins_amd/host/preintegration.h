// Preintegration of boundary B1 (P1 on device; P2 on host per factor, or batched on device): reference
// preintegration/preintegration{,_base,_normal,_earth}.{h,cc}, preintegration_factor.h.  Implemented in preintegration_hip.cc
// (the batch drivers and small-matrix helpers shared with PreintegrationOdo in preint_common.h; PreintegrationSetT in preint_set_hip.cc).
#pragma once
#include <memory>
#include <string>
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

// One IMU interval between two time nodes.  (Re)integration of many intervals is ONE batched device call.
class Preintegration {
public:
    enum Variant { NORMAL = 0, EARTH = 1 };
    // widths: error state, mix block, delta_state row, evaluation point (pose0 mix0 pose1 mix1), whitened Jacobians of one factor
    static constexpr int NUM_STATE = 15, NUM_MIX = 9, NUM_DELTA = 16, NUM_POINT = 2 * (7 + NUM_MIX), NUM_JAC = NUM_STATE * NUM_POINT;
    static constexpr Variant EARTH_VARIANT = EARTH; // the variant with pn rows and an Earth-rate quaternion
    static void deltaToArray(const IntegrationState &s, double *a); // the delta_state row of the C entries (NUM_DELTA)
    Preintegration(std::shared_ptr<IntegrationParameters> parameters, const IMU &imu0, const IntegrationState &state, Variant v);
    void addNewImu(const IMU &imu) { imu_buffer_.push_back(imu); dirty_ = true; }
    void reintegration(const IntegrationState &state);
    const Vector3d &earthRate() const { return iewn_; }
    // integrate every dirty interval of the list: one icg_preint_batch launch per (variant, parameter values) group
    static bool integrateBatch(icg_ctx *ctx, const vector<Preintegration *> &list, std::string *err = nullptr);
    // integrateBatch for the intervals of MANY streams: every dirty interval of the list in ONE icg_preint_batch_params call per variant
    // present, whatever the parameter values (each interval brings its own row: its Earth rate, gravity, noise figures), and the
    // square-root information comes down with the result (the device forms it behind the integration; updateSqrtInformation does not
    // run).  Every member is afterwards what integrateBatch leaves, bit for bit.  The C entry is referenced weakly: without it
    // integrateStreamsAvailable() is false and integrateStreams fails by the entry's name and integrates nothing.
    static bool integrateStreams(icg_ctx *ctx, const vector<Preintegration *> &list, std::string *err = nullptr);
    static bool integrateStreamsAvailable(); // icg_preint_batch_params is in this build
    // P2 on the device: residual 15 (and, unless `jacobians` is null, the Jacobians 480 = 15x7 | 15x9 | 15x7 | 15x9) of every factor of the
    // list at its evaluation point (points: n x 32 = pose0[7] mix0[9] pose1[7] mix1[9]) through icg_preint_evaluate_batch, one call per
    // variant present.  ok[k] = 0 (and zero rows) for a factor that is not integrated for its current buffer / start state or whose
    // covariance is singular: the two conditions under which evaluate() returns false.  sqrt_info (optional, n x 225): the square-root
    // information the device formed.  Returns false with *err set when a call fails or the entry point is not in this build.
    static bool evaluateBatch(icg_ctx *ctx, const vector<const Preintegration *> &list, const double *points, double *residuals,
                              double *jacobians, vector<char> *ok, std::string *err = nullptr, double *sqrt_info = nullptr);
    static bool evaluateBatchAvailable(); // icg_preint_evaluate_batch is in this build
    const IntegrationState &currentState() const { return current_state_; }
    const IntegrationState &deltaState() const { return delta_state_; }
    double deltaTime() const { return delta_time_; }
    const vector<IMU> &imuBuffer() const { return imu_buffer_; }
    // PreintegrationFactor::Evaluate body (preintegration_factor.h:45-69): residual 15, Jacobians 15x7,15x9,15x7,15x9
    bool evaluate(const double *const *parameters, double *residuals, double **jacobians) const;
    // The only two places of evaluate() where sin / cos / sqrt enter, as unit quaternions (x, y, z, w), formed with evaluate()'s own
    // expressions: the bias correction of delta q at mix0 (v3, bg3, ba3), rotvec2quat(dq_dbg (bg0 - delta.bg)), and the Earth variant's
    // rotvec2quat(-iewn T), a constant of the integration result (identity, and unused, for the Normal variant).
    void correctionQuaternion(const double *mix0, double q_xyzw[4]) const;
    void earthRateQuaternion(double q_xyzw[4]) const;
    // evaluate() with the two quaternions given: everything that is left is + - * / in a fixed order.  evaluate() is
    // correctionQuaternion + earthRateQuaternion + evaluateGiven; a caller that evaluates on the device (icg_preint_set /
    // icg_preint_evaluate_resident) ships the quaternions instead of calling sin / cos there.
    bool evaluateGiven(const double *const *parameters, const double q_corr[4], const double q_nn[4], double *residuals, double **jacobians) const;
    Variant variant() const { return variant_; }
    const vector<double> &sqrtInformation() const { return sqrt_information_; } // 15x15 row-major; zeros while the covariance is singular
    // what a resident set packs besides deltaState(), deltaTime(), sqrtInformation() and earthRate()
    bool ready() const { return !dirty_ && sqrt_information_ok_; } // integrated for the current buffer / start state, covariance not singular
    // forms the square-root information from the covariance on the host again, as integrateBatch does for every result it brings down (the
    // same arithmetic on the same data: nothing changes); for probes that time that loop
    void recomputeSqrtInformation() { updateSqrtInformation(); }
    const vector<double> &jacobian() const { return jacobian_; }   // 15x15 row-major
    const vector<double> &covariance() const { return covariance_; } // 15x15 row-major
    double gravity() const { return parameters_->gravity; }
    const vector<double> &pnRows() const { return pn_; }           // Earth variant: rows of 4 (dt, position); evaluate() sums the complete rows

private:
    std::shared_ptr<IntegrationParameters> parameters_;
    Variant variant_;
    vector<IMU> imu_buffer_;
    IntegrationState start_state_, current_state_, delta_state_;
    double delta_time_{0};
    void updateSqrtInformation();
    struct Traits; // what the shared batch drivers (preint_common.h) need of this class
    // one integration result of the C entries into the members, without the square-root information
    void storeIntegrationResult(const double *cur16, const double *delta16, const double *jac225, const double *cov225, double delta_time,
                                const double *pn, int pn_rows);
    vector<double> jacobian_, covariance_, pn_; // 15x15, 15x15, (n-1)x4
    vector<double> sqrt_information_;            // 15x15, of covariance_ (formed when an integration result arrives)
    bool sqrt_information_ok_{false};
    Vector3d iewn_; // this interval's Earth rate: P1 (device) and P2 (evaluate) use the same value
    bool dirty_{true};
};

class PreintegrationFactor : public ceres::CostFunction {
public:
    explicit PreintegrationFactor(std::shared_ptr<Preintegration> preintegration);
    bool Evaluate(const double *const *parameters, double *residuals, double **jacobians) const override {
        return preintegration_->evaluate(parameters, residuals, jacobians);
    }
    // what a solver that evaluates the factor on the device (WindowSolverBatch::setDevicePreintegration) packs its resident set from
    const Preintegration &preintegration() const { return *preintegration_; }

private:
    std::shared_ptr<Preintegration> preintegration_;
};

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
