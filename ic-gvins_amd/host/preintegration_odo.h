// Odometer preintegration (P1 on the device; P2 on the host per factor, or batched on the device): reference
// preintegration/preintegration_{odo,earth_odo}.{h,cc} on preintegration_base.{h,cc}, preintegration_factor.h.  A class beside Preintegration
// (preintegration.h), not a widening of it: the error state is 19 wide (dp, dv, dq, dbg, dba, ds, dsodo), the noise has 16 channels and the
// mix block 10 parameters (v, bg, ba, sodo: the odometer scale factor is mix[9], preintegration_odo.cc:169-183).  Implemented in
// preintegration_odo_hip.cc.
// The reference's factory (preintegration/preintegration.h:37-73) maps to the two classes as: Normal -> Preintegration::NORMAL,
// Earth -> Preintegration::EARTH, Odo -> PreintegrationOdo::ODO, EarthOdo -> PreintegrationOdo::EARTH_ODO.
#pragma once
#include <memory>
#include <string>
#include <vector>

#include "preintegration.h"

namespace icg {

// The 10-parameter mix block of the odometer variants (stateToData / stateFromData, preintegration_odo.cc:169-183): v, bg, ba, sodo.
inline void odoStateToMix(const IntegrationState &s, double mix[10]) {
    for (int i = 0; i < 3; i++) mix[i] = s.v[i], mix[3 + i] = s.bg[i], mix[6 + i] = s.ba[i];
    mix[9] = s.sodo;
}
inline void odoStateFromMix(const double mix[10], IntegrationState &s) {
    s.v  = Vector3d(mix[0], mix[1], mix[2]);
    s.bg = Vector3d(mix[3], mix[4], mix[5]);
    s.ba = Vector3d(mix[6], mix[7], mix[8]);
    s.sodo = mix[9];
}

// One IMU + odometer interval between two time nodes.  (Re)integration of many intervals is ONE batched device call.
class PreintegrationOdo {
public:
    enum Variant { ODO = 2, EARTH_ODO = 3 }; // the numbers of icg_preint_odo_batch (the reference's own enum numbers them 1 and 3)
    static constexpr int NUM_STATE = 19, NUM_MIX = 10, NUM_DELTA = 20, NUM_POINT = 2 * (7 + NUM_MIX), NUM_JAC = NUM_STATE * NUM_POINT;
    static constexpr Variant EARTH_VARIANT = EARTH_ODO; // the variant with pn rows and an Earth-rate quaternion
    static void deltaToArray(const IntegrationState &s, double *a); // the delta_state row of the C entries (NUM_DELTA: the 16, s3, sodo)
    PreintegrationOdo(std::shared_ptr<IntegrationParameters> parameters, const IMU &imu0, const IntegrationState &state, Variant v);
    void addNewImu(const IMU &imu) { imu_buffer_.push_back(imu); dirty_ = true; }
    void reintegration(const IntegrationState &state);
    const Vector3d &earthRate() const { return iewn_; }
    // integrate every dirty interval of the list: one icg_preint_odo_batch launch per (variant, parameter values) group
    static bool integrateBatch(icg_ctx *ctx, const vector<PreintegrationOdo *> &list, std::string *err = nullptr);
    // integrateBatch for the intervals of MANY streams: every dirty interval of the list in ONE icg_preint_odo_batch_params call per
    // variant present, whatever the parameter values, with the square-root information formed on the device behind the integration
    // (updateSqrtInformation does not run).  Every member is afterwards what integrateBatch leaves, bit for bit.  Without the (weakly
    // referenced) C entry integrateStreamsAvailable() is false and integrateStreams fails by the entry's name and integrates nothing.
    static bool integrateStreams(icg_ctx *ctx, const vector<PreintegrationOdo *> &list, std::string *err = nullptr);
    static bool integrateStreamsAvailable(); // icg_preint_odo_batch_params is in this build
    // The object as if integrateBatch had returned this result (delta_state 20 and jac / cov 361 in icg_preint_odo_batch's layout, pn rows of
    // 4, iewn the interval's Earth rate): the host P2 can then be exercised, and pinned against the reference, without a device.
    void setIntegrationResult(const double *cur16, const double *delta20, const double *jac361, const double *cov361, double delta_time,
                              const double *pn, int pn_rows, const Vector3d &iewn);
    // P2 on the device: residual 19 (and, unless `jacobians` is null, the Jacobians 646 = 19x7 | 19x10 | 19x7 | 19x10) of every factor of the
    // list at its evaluation point (points: n x 34 = pose0[7] mix0[10] pose1[7] mix1[10]) through icg_preint_odo_evaluate_batch, one call
    // per variant present.  ok[k] = 0 (and zero rows) for a factor that is not integrated or whose covariance is singular.  sqrt_info
    // (optional, n x 361): the square-root information the device formed.  Returns false with *err set when a call fails or the entry point
    // is not in this build.
    static bool evaluateBatch(icg_ctx *ctx, const vector<const PreintegrationOdo *> &list, const double *points, double *residuals,
                              double *jacobians, vector<char> *ok, std::string *err = nullptr, double *sqrt_info = nullptr);
    static bool integrateBatchAvailable(); // icg_preint_odo_batch is in this build
    static bool evaluateBatchAvailable();  // icg_preint_odo_evaluate_batch is in this build
    const IntegrationState &startState() const { return start_state_; }
    const IntegrationState &currentState() const { return current_state_; }
    const IntegrationState &deltaState() const { return delta_state_; } // with s and sodo
    double deltaTime() const { return delta_time_; }
    const vector<IMU> &imuBuffer() const { return imu_buffer_; }
    // PreintegrationFactor::Evaluate body (preintegration_factor.h:45-69): residual 19, Jacobians 19x7, 19x10, 19x7, 19x10.  false (and
    // nothing written) while the interval is not integrated or its covariance is singular.
    bool evaluate(const double *const *parameters, double *residuals, double **jacobians) const;
    // The only two places of evaluate() where sin / cos / sqrt enter, as unit quaternions (x, y, z, w), formed with evaluate()'s own
    // expressions: the bias correction of delta q at mix0 (v3, bg3, ba3, sodo), rotvec2quat(dq_dbg (bg0 - delta.bg)), and the EarthOdo
    // variant's rotvec2quat(-iewn T), a constant of the integration result (identity, and unused, for the Odo variant).
    void correctionQuaternion(const double *mix0, double q_xyzw[4]) const;
    void earthRateQuaternion(double q_xyzw[4]) const;
    // evaluate() with the two quaternions given: everything that is left is + - * / in a fixed order.  evaluate() is
    // correctionQuaternion + earthRateQuaternion + evaluateGiven; a caller that evaluates on the device (icg_preint_odo_set /
    // icg_preint_odo_evaluate_resident) ships the quaternions instead of calling sin / cos there.
    bool evaluateGiven(const double *const *parameters, const double q_corr[4], const double q_nn[4], double *residuals, double **jacobians) const;
    Variant variant() const { return variant_; }
    const vector<double> &sqrtInformation() const { return sqrt_information_; } // 19x19 row-major; zeros while the covariance is singular
    bool ready() const { return !dirty_ && sqrt_information_ok_; }
    // forms the square-root information from the covariance on the host again, as integrateBatch does for every result it brings down (the
    // same arithmetic on the same data: nothing changes); for probes that time that loop
    void recomputeSqrtInformation() { updateSqrtInformation(); }
    const vector<double> &jacobian() const { return jacobian_; }     // 19x19 row-major
    const vector<double> &covariance() const { return covariance_; } // 19x19 row-major
    double gravity() const { return parameters_->gravity; }
    const vector<double> &pnRows() const { return pn_; } // EarthOdo: rows of 4 (dt, position)
    // cvb = euler2matrix(abv)^T row-major (rotation.h:84-88; preintegration_odo.cc:36): formed here, shipped to the device as nine doubles
    static void vehicleRotation(const Vector3d &abv, double cvb[9]);

private:
    std::shared_ptr<IntegrationParameters> parameters_;
    Variant variant_;
    vector<IMU> imu_buffer_;
    IntegrationState start_state_, current_state_, delta_state_;
    double delta_time_{0};
    void updateSqrtInformation();
    struct Traits; // what the shared batch drivers (preint_common.h) need of this class
    // setIntegrationResult without the square-root information (integrateStreams takes that from the device)
    void storeIntegrationResult(const double *cur16, const double *delta20, const double *jac361, const double *cov361, double delta_time,
                                const double *pn, int pn_rows, const Vector3d &iewn);
    vector<double> jacobian_, covariance_, pn_; // 19x19, 19x19, (n-1)x4
    vector<double> sqrt_information_;            // 19x19, of covariance_ (formed when an integration result arrives)
    bool sqrt_information_ok_{false};
    Vector3d iewn_; // this interval's Earth rate: P1 (device) and P2 (evaluate) use the same value
    bool dirty_{true};
};

class PreintegrationOdoFactor : public ceres::CostFunction {
public:
    explicit PreintegrationOdoFactor(std::shared_ptr<PreintegrationOdo> preintegration);
    bool Evaluate(const double *const *parameters, double *residuals, double **jacobians) const override {
        return preintegration_->evaluate(parameters, residuals, jacobians);
    }
    const PreintegrationOdo &preintegration() const { return *preintegration_; }

private:
    std::shared_ptr<PreintegrationOdo> preintegration_;
};

// The odometer preintegration factors of many windows resident on the device: PreintegrationSetT (preintegration.h) for this class.
using PreintegrationOdoSet = PreintegrationSetT<PreintegrationOdo>;

} // namespace icg
