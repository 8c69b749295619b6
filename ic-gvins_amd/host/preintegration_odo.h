// Odometer preintegration (P1 on the device; P2 on the host per factor, or batched on the device): reference
// preintegration/preintegration_{odo,earth_odo}.{h,cc} on preintegration_base.{h,cc}, preintegration_factor.h.  The 19-state family of
// PreintegrationT (preintegration.h): the error state is 19 wide (dp, dv, dq, dbg, dba, ds, dsodo), the noise has 16 channels and the mix
// block 10 parameters (v, bg, ba, sodo: the odometer scale factor is mix[9], preintegration_odo.cc:169-183).
// The reference's factory (preintegration/preintegration.h:37-73) maps to the two classes as: Normal -> Preintegration::NORMAL,
// Earth -> Preintegration::EARTH, Odo -> PreintegrationOdo::ODO, EarthOdo -> PreintegrationOdo::EARTH_ODO.
#pragma once
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

// The 19-state family: Odo / EarthOdo.  Rows of icg_preint_odo_batch: imu 9 (the 8, odovel), state0 17 (the 16, sodo), delta_state 20 (the
// 16, s3, sodo), params 25 (the 9, odo_std 3, odo_srw, cvb 9, lodo 3).
struct PreintegrationOdoFamily {
    enum Variant { ODO = 2, EARTH_ODO = 3 }; // the numbers of icg_preint_odo_batch (the reference's own enum numbers them 1 and 3)
    static constexpr Variant PLAIN_VARIANT = ODO, EARTH_VARIANT = EARTH_ODO;
    static constexpr int NUM_STATE = 19, NUM_MIX = 10, NUM_DELTA = 20, IMU_ROW = 9, STATE0_ROW = 17, PARAMS_ROW = 25;
    static constexpr bool HAS_ODO = true, PN_EVERY_VARIANT = false;
    static constexpr const char *BATCH_NAME = "icg_preint_odo_batch", *PARAMS_NAME = "icg_preint_odo_batch_params",
                                *EVAL_NAME = "icg_preint_odo_evaluate_batch";
    static decltype(&icg_preint_odo_batch) batchEntry();
    static decltype(&icg_preint_odo_batch_params) paramsEntry();
    static decltype(&icg_preint_odo_evaluate_batch) evalEntry();
    static void imuRow(const IMU &s, double *row9) {
        const double v[9] = {s.time, s.dt, s.dtheta[0], s.dtheta[1], s.dtheta[2], s.dvel[0], s.dvel[1], s.dvel[2], s.odovel};
        memcpy(row9, v, sizeof v);
    }
    static void state0Row(const IntegrationState &start, double *row17) {
        stateToArray16(start, row17);
        row17[16] = start.sodo;
    }
    static void paramsRow(const IntegrationParameters &P, const Vector3d &iewn, double *row25) {
        const double v[13] = {P.gyr_arw, P.acc_vrw, P.gyr_bias_std, P.acc_bias_std, P.corr_time, P.gravity, iewn[0], iewn[1], iewn[2],
                              P.odo_std[0], P.odo_std[1], P.odo_std[2], P.odo_srw};
        memcpy(row25, v, sizeof v);
        vehicleRotation(P.abv, row25 + 13);
        row25[22] = P.lodo[0], row25[23] = P.lodo[1], row25[24] = P.lodo[2];
    }
    static void deltaRow(const IntegrationState &delta, double *row20) {
        stateToArray16(delta, row20);
        row20[16] = delta.s[0], row20[17] = delta.s[1], row20[18] = delta.s[2], row20[19] = delta.sodo;
    }
    static void deltaFromRow(const double *row20, IntegrationState &delta) {
        stateFromArray16(row20, delta);
        delta.s    = Vector3d(row20[16], row20[17], row20[18]);
        delta.sodo = row20[19];
    }
    // cvb = euler2matrix(abv)^T row-major (rotation.h:84-88; preintegration_odo.cc:36): formed here, shipped to the device as nine doubles
    static void vehicleRotation(const Vector3d &abv, double cvb[9]);
};
using PreintegrationOdo       = PreintegrationT<PreintegrationOdoFamily>;
using PreintegrationOdoFactor = PreintegrationFactorT<PreintegrationOdoFamily>;

// The odometer preintegration factors of many windows resident on the device: PreintegrationSetT (preintegration.h) for this class.
using PreintegrationOdoSet = PreintegrationSetT<PreintegrationOdo>;

} // namespace icg
