// Preintegration on the HIP C ABI: P1 (the per-sample inner loop) runs batched on the device through icg_preint_batch (integrateBatch: one
// launch per group of equal parameter values, the square-root information formed here) or icg_preint_batch_params (integrateStreams: the
// intervals of many streams in one call per variant, a parameter row per interval, the square-root information formed on the device);
// P2 (residual + Jacobians, preintegration_normal.cc:38-142 / preintegration_earth.cc:37-164, wrapped by
// preintegration_factor.h:45-69) is a handful of 3x3 / 15x15 operations per factor (<= 15 factors per solve) and stays
// on the host, in the Ceres callback thread that asks for it.  evaluateBatch() is the same evaluation for MANY factors at once on the
// device (icg_preint_evaluate_batch): for callers that hold thousands of integrated intervals, not for the per-factor Ceres callback.
// evaluate() is split at its two rotvec2quat calls (correctionQuaternion, earthRateQuaternion) from the rest (evaluateGiven): a driver that
// keeps the factors resident on the device for a solve (PreintegrationSet, preint_set_hip.cc) ships the two quaternions, and the device
// result has evaluate()'s bits.
#include "earth.h"
#include "factors.h"
#include "preint_common.h"

// A build of this layer on another implementation of the C ABI may not have the entry point: the reference stays weak (null when absent)
// and evaluateBatch() reports it; the product library links libicgvins_hip.so, which defines it.
#pragma weak icg_preint_evaluate_batch
#pragma weak icg_preint_batch_params

namespace icg {

using namespace preint_math;

struct Preintegration::Traits {
    typedef Preintegration Class;
    static constexpr int N = NUM_STATE, IMU_ROW = 8, STATE0 = 16, DELTA = NUM_DELTA, PARAMS = 9;
    static constexpr Variant PLAIN = NORMAL, EARTH_V = EARTH;
    static constexpr bool PN_EVERY_VARIANT = true; // (the Normal variant keeps the zero rows of the call's buffer)
    static constexpr const char *batch_name = "icg_preint_batch", *params_name = "icg_preint_batch_params", *eval_name = "icg_preint_evaluate_batch";
    static auto batchEntry() { return &icg_preint_batch; }
    static auto paramsEntry() { return &icg_preint_batch_params; }
    static auto evalEntry() { return &icg_preint_evaluate_batch; }
    static void imuRow(const IMU &s, double *row) {
        const double v[8] = {s.time, s.dt, s.dtheta[0], s.dtheta[1], s.dtheta[2], s.dvel[0], s.dvel[1], s.dvel[2]};
        memcpy(row, v, sizeof v);
    }
    static void state0Row(const Preintegration &p, double *a) { stateToArray16(p.start_state_, a); }
    static void paramsRow(const Preintegration &p, double *out9) {
        const IntegrationParameters &P = *p.parameters_;
        const double v[9] = {P.gyr_arw, P.acc_vrw, P.gyr_bias_std, P.acc_bias_std, P.corr_time, P.gravity, p.iewn_[0], p.iewn_[1], p.iewn_[2]};
        memcpy(out9, v, sizeof v);
    }
    static void deltaRow(const IntegrationState &s, double *a) { deltaToArray(s, a); }
    static bool dirty(const Preintegration &p) { return p.dirty_; }
    static void store(Preintegration &p, const double *cur, const double *del, const double *jac, const double *cov, double dt, const double *pn,
                      int pn_rows) {
        p.storeIntegrationResult(cur, del, jac, cov, dt, pn, pn_rows);
    }
    static void finishHost(Preintegration &p) {
        p.updateSqrtInformation();
        p.dirty_ = false;
    }
    static void finishDevice(Preintegration &p, const double *S, bool ok) {
        p.sqrt_information_.assign(S, S + NUM_STATE * NUM_STATE);
        p.sqrt_information_ok_ = ok;
        p.dirty_               = false;
    }
};

void Preintegration::deltaToArray(const IntegrationState &s, double *a) { stateToArray16(s, a); }

static void refreshEarthRate(const IntegrationParameters &P, const IntegrationState &state, Vector3d &iewn);

Preintegration::Preintegration(std::shared_ptr<IntegrationParameters> parameters, const IMU &imu0, const IntegrationState &state,
                               Variant v)
    : parameters_(std::move(parameters)), variant_(v), start_state_(state), current_state_(state) {
    imu_buffer_.push_back(imu0);
    delta_state_.bg = state.bg;
    delta_state_.ba = state.ba;
    jacobian_.assign(225, 0.0);
    covariance_.assign(225, 0.0);
    for (int i = 0; i < 15; i++) jacobian_[(size_t) i * 16] = 1.0;
    refreshEarthRate(*parameters_, state, iewn_);
}

// preintegration_earth.cc:319-321 (resetState, run by the constructor and by every reintegration)
static void refreshEarthRate(const IntegrationParameters &P, const IntegrationState &state, Vector3d &iewn) {
    iewn = P.has_station ? Earth::iewn(P.station, state.p) : P.iewn;
}

void Preintegration::reintegration(const IntegrationState &state) {
    start_state_ = state;
    dirty_       = true;
    if (variant_ == EARTH) refreshEarthRate(*parameters_, state, iewn_);
}

void Preintegration::storeIntegrationResult(const double *cur16, const double *delta16, const double *jac225, const double *cov225,
                                            double delta_time, const double *pn, int pn_rows) {
    stateFromArray16(cur16, current_state_);
    stateFromArray16(delta16, delta_state_);
    current_state_.time = imu_buffer_.back().time;
    jacobian_.assign(jac225, jac225 + 225);
    covariance_.assign(cov225, cov225 + 225);
    delta_time_ = delta_time;
    pn_.assign(pn, pn + 4 * (size_t) (pn_rows > 0 ? pn_rows : 0));
}

bool Preintegration::integrateBatch(icg_ctx *ctx, const vector<Preintegration *> &list, std::string *err) {
    return integrateBatchT<Traits>(ctx, list, err);
}

bool Preintegration::integrateStreamsAvailable() { return &icg_preint_batch_params != nullptr; }

bool Preintegration::integrateStreams(icg_ctx *ctx, const vector<Preintegration *> &list, std::string *err) {
    return integrateStreamsT<Traits>(ctx, list, err);
}

bool Preintegration::evaluateBatchAvailable() { return &icg_preint_evaluate_batch != nullptr; }

bool Preintegration::evaluateBatch(icg_ctx *ctx, const vector<const Preintegration *> &list, const double *points, double *residuals,
                                   double *jacobians, vector<char> *ok, std::string *err, double *sqrt_info) {
    return evaluateBatchT<Traits>(ctx, list, points, residuals, jacobians, ok, err, sqrt_info);
}

// the square-root information of covariance_ (preint_common.h), formed once when an integration result arrives
void Preintegration::updateSqrtInformation() {
    sqrt_information_.assign(225, 0.0);
    sqrt_information_ok_ = preintSqrtInformation<15>(covariance_.data(), sqrt_information_.data());
}

void Preintegration::correctionQuaternion(const double *mix0, double q_xyzw[4]) const {
    M3 dq_dbg;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) dq_dbg.m[i][j] = jacobian_[(size_t) (6 + i) * 15 + 9 + j];
    V3 bg0{mix0[3], mix0[4], mix0[5]}, dbg0{delta_state_.bg[0], delta_state_.bg[1], delta_state_.bg[2]};
    V3 dbg = bg0 - dbg0;
    Q4 q   = rotvec2quat(mv(dq_dbg, dbg));
    q_xyzw[0] = q.x, q_xyzw[1] = q.y, q_xyzw[2] = q.z, q_xyzw[3] = q.w;
}

void Preintegration::earthRateQuaternion(double q_xyzw[4]) const {
    Q4 q{0, 0, 0, 1};
    if (variant_ == EARTH) {
        V3 iewn{iewn_[0], iewn_[1], iewn_[2]};
        const double T = delta_time_;
        q              = rotvec2quat(-iewn * T);
    }
    q_xyzw[0] = q.x, q_xyzw[1] = q.y, q_xyzw[2] = q.z, q_xyzw[3] = q.w;
}

bool Preintegration::evaluate(const double *const *parameters, double *residuals, double **jacobians) const {
    if (dirty_) return false; // not integrated for the current buffer/start state: evaluation failed, loudly
    if (!sqrt_information_ok_) return false; // singular covariance
    double q_corr[4], q_nn[4];
    correctionQuaternion(parameters[1], q_corr);
    earthRateQuaternion(q_nn);
    return evaluateGiven(parameters, q_corr, q_nn, residuals, jacobians);
}

bool Preintegration::evaluateGiven(const double *const *parameters, const double q_corr[4], const double q_nn[4], double *residuals,
                                   double **jacobians) const {
    if (dirty_) return false;
    if (!sqrt_information_ok_) return false;
    typedef double M15[15][15];
    M15 jac, S;
    memcpy(jac, jacobian_.data(), sizeof jac);
    memcpy(S, sqrt_information_.data(), sizeof S);
    // constructState (normal :162-180)
    const double *pose0 = parameters[0], *mix0 = parameters[1], *pose1 = parameters[2], *mix1 = parameters[3];
    V3 p0{pose0[0], pose0[1], pose0[2]}, p1{pose1[0], pose1[1], pose1[2]};
    Q4 q0{pose0[3], pose0[4], pose0[5], pose0[6]}, q1{pose1[3], pose1[4], pose1[5], pose1[6]};
    V3 v0{mix0[0], mix0[1], mix0[2]}, bg0{mix0[3], mix0[4], mix0[5]}, ba0{mix0[6], mix0[7], mix0[8]};
    V3 v1{mix1[0], mix1[1], mix1[2]}, bg1{mix1[3], mix1[4], mix1[5]}, ba1{mix1[6], mix1[7], mix1[8]};
    V3 gravity{0, 0, parameters_->gravity};
    V3 iewn{iewn_[0], iewn_[1], iewn_[2]};
    const IntegrationState &d = delta_state_;
    V3 dp{d.p[0], d.p[1], d.p[2]}, dv{d.v[0], d.v[1], d.v[2]}, dbg0{d.bg[0], d.bg[1], d.bg[2]}, dba0{d.ba[0], d.ba[1], d.ba[2]};
    Q4 dq{d.q.x, d.q.y, d.q.z, d.q.w};
    auto blk = [&](int r, int c) {
        M3 b;
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) b.m[i][j] = jac[r + i][c + j];
        return b;
    };
    M3 dp_dbg = blk(0, 9), dp_dba = blk(0, 12), dv_dbg = blk(3, 9), dv_dba = blk(3, 12), dq_dbg = blk(6, 9);
    V3 dbg = bg0 - dbg0, dba = ba0 - dba0;
    V3 corrected_p = dp + mv(dp_dba, dba) + mv(dp_dbg, dbg);
    V3 corrected_v = dv + mv(dv_dba, dba) + mv(dv_dbg, dbg);
    Q4 corrected_q = qmul(dq, Q4{q_corr[0], q_corr[1], q_corr[2], q_corr[3]});
    const double T = delta_time_;

    double r[15];
    double J0[15][7], J1[15][9], J2[15][7], J3[15][9];
    memset(J0, 0, sizeof J0);
    memset(J1, 0, sizeof J1);
    memset(J2, 0, sizeof J2);
    memset(J3, 0, sizeof J3);
    auto put = [](auto &J, int r0, int c0, const M3 &b) {
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) J[r0 + i][c0 + j] = b.m[i][j];
    };
    M3 cnb0 = qmat(qinv(q0));
    if (variant_ == NORMAL) {
        V3 dpn = p1 - p0 - v0 * T - 0.5 * gravity * T * T;
        V3 dvn = v1 - v0 - gravity * T;
        V3 rp = qrot(qinv(q0), dpn) - corrected_p, rv = qrot(qinv(q0), dvn) - corrected_v;
        Q4 qe = qmul(qmul(qinv(corrected_q), qinv(q0)), q1);
        r[0] = rp.x, r[1] = rp.y, r[2] = rp.z, r[3] = rv.x, r[4] = rv.y, r[5] = rv.z, r[6] = 2 * qe.x, r[7] = 2 * qe.y, r[8] = 2 * qe.z;
        put(J0, 0, 0, scale(cnb0, -1.0));
        put(J0, 0, 3, skew(qrot(qinv(q0), dpn)));
        put(J0, 3, 3, skew(qrot(qinv(q0), dvn)));
        put(J0, 6, 3, scale(qleft_qright_br(qmul(qinv(q1), q0), corrected_q), -1.0));
        put(J2, 0, 0, cnb0);
        put(J2, 6, 3, qleft_br(qe));
        put(J1, 0, 0, scale(cnb0, -T));
        put(J1, 0, 3, scale(dp_dbg, -1.0));
        put(J1, 0, 6, scale(dp_dba, -1.0));
        put(J1, 3, 0, scale(cnb0, -1.0));
        put(J1, 3, 3, scale(dv_dbg, -1.0));
        put(J1, 3, 6, scale(dv_dba, -1.0));
        put(J1, 6, 3, mul(scale(qleft_br(qmul(qmul(qinv(q1), q0), dq)), -1.0), dq_dbg));
    } else {
        M3 iewn_skew = skew(iewn);
        V3 p_cor{0, 0, 0};
        for (size_t k = 0; k + 3 < pn_.size(); k += 4) p_cor = p_cor + (V3{pn_[k + 1], pn_[k + 2], pn_[k + 3]} - p0) * pn_[k];
        p_cor    = mv(scale(iewn_skew, 2.0), p_cor);
        V3 v_cor = mv(scale(iewn_skew, 2.0), p1 - p0);
        Q4 qnn   = Q4{q_nn[0], q_nn[1], q_nn[2], q_nn[3]};
        V3 dpn   = p1 - p0 - v0 * T - 0.5 * gravity * T * T + p_cor;
        V3 dvn   = v1 - v0 - gravity * T + v_cor;
        Q4 qb0b1 = qmul(qmul(qinv(q1), qnn), q0);
        V3 rp = mv(cnb0, dpn) - corrected_p, rv = mv(cnb0, dvn) - corrected_v;
        Q4 qe = qmul(qb0b1, corrected_q);
        r[0] = rp.x, r[1] = rp.y, r[2] = rp.z, r[3] = rv.x, r[4] = rv.y, r[5] = rv.z, r[6] = 2 * qe.x, r[7] = 2 * qe.y, r[8] = 2 * qe.z;
        put(J0, 0, 0, add(scale(cnb0, -1.0), scale(mul(scale(cnb0, 2.0), iewn_skew), -T)));
        put(J0, 0, 3, skew(mv(cnb0, dpn)));
        put(J0, 3, 0, mul(scale(cnb0, -2.0), iewn_skew));
        put(J0, 3, 3, skew(mv(cnb0, dvn)));
        put(J0, 6, 3, qleft_qright_br(qb0b1, corrected_q));
        put(J2, 0, 0, cnb0);
        put(J2, 3, 0, mul(scale(cnb0, 2.0), iewn_skew));
        put(J2, 6, 3, scale(qright_br(qe), -1.0));
        put(J1, 0, 0, scale(cnb0, -T));
        put(J1, 0, 3, scale(dp_dbg, -1.0));
        put(J1, 0, 6, scale(dp_dba, -1.0));
        put(J1, 3, 0, scale(cnb0, -1.0));
        put(J1, 3, 3, scale(dv_dbg, -1.0));
        put(J1, 3, 6, scale(dv_dba, -1.0));
        put(J1, 6, 3, mul(qleft_br(qmul(qb0b1, dq)), dq_dbg));
    }
    put(J1, 9, 3, scale(eye(), -1.0));
    put(J1, 12, 6, scale(eye(), -1.0));
    put(J3, 3, 0, cnb0);
    put(J3, 9, 3, eye());
    put(J3, 12, 6, eye());
    V3 rbg = bg1 - bg0, rba = ba1 - ba0;
    r[9] = rbg.x, r[10] = rbg.y, r[11] = rbg.z, r[12] = rba.x, r[13] = rba.y, r[14] = rba.z;
    for (int i = 0; i < 15; i++) {
        double s = 0;
        for (int k = 0; k < 15; k++) s += S[i][k] * r[k];
        residuals[i] = s;
    }
    if (jacobians) {
        auto emit = [&](auto &J, int cols, double *out) {
            if (!out) return;
            for (int i = 0; i < 15; i++)
                for (int j = 0; j < cols; j++) {
                    double s = 0;
                    for (int k = 0; k < 15; k++) s += S[i][k] * J[k][j];
                    out[i * cols + j] = s;
                }
        };
        emit(J0, 7, jacobians[0]);
        emit(J1, 9, jacobians[1]);
        emit(J2, 7, jacobians[2]);
        emit(J3, 9, jacobians[3]);
    }
    return true;
}

PreintegrationFactor::PreintegrationFactor(std::shared_ptr<Preintegration> preintegration)
    : preintegration_(std::move(preintegration)) {
    *mutable_parameter_block_sizes() = std::vector<int32_t>{7, 9, 7, 9}; // numBlocksParameters (normal :148-150)
    set_num_residuals(15);
}

} // namespace icg
