// Odometer preintegration on the HIP C ABI: P1 (the per-sample inner loop of PreintegrationOdo / PreintegrationEarthOdo) runs batched on the
// device through icg_preint_odo_batch; P2 (residual 19 + Jacobians, preintegration_odo.cc:40-159 / preintegration_earth_odo.cc:41-183,
// wrapped by preintegration_factor.h:45-69) is evaluated on the host per factor (evaluate) or for many factors at once on the device
// (evaluateBatch, icg_preint_odo_evaluate_batch).  The 19-state twin of preintegration_hip.cc, which stays as it is: the small-matrix helpers
// below repeat that file's (same expressions, same order) so that nothing the 15-state bit-for-bit tests rest on moves.
// evaluate() is split at its two rotvec2quat calls (correctionQuaternion, earthRateQuaternion) from the rest (evaluateGiven), as
// Preintegration::evaluate is: a driver that keeps the factors resident on the device (PreintegrationOdoSet, preint_odo_set_hip.cc) ships
// the two quaternions, and the device is left with + - * / in this file's order.
#include "earth.h"
#include "preint_common.h"
#include "preintegration_odo.h"

// A build of this layer on another implementation of the C ABI (the CPU checker library) does not have the entry points: the references stay
// weak (null when absent) and the callers report it; the product library links libicgvins_hip.so, which defines them.
#pragma weak icg_preint_odo_batch
#pragma weak icg_preint_odo_evaluate_batch
#pragma weak icg_preint_odo_batch_params

namespace icg {

using namespace preint_math;

namespace {
constexpr int N = PreintegrationOdo::NUM_STATE, NN = N * N;

// rows of icg_preint_odo_batch: state0 17 (p3, q4 xyzw, v3, bg3, ba3, sodo), cur_state 16, delta_state 20 (the 16, s3, sodo)
void deltaFromArray20(const double *a, IntegrationState &s) {
    stateFromArray16(a, s);
    s.s    = Vector3d(a[16], a[17], a[18]);
    s.sodo = a[19];
}

// preintegration_earth_odo.cc:364-366 (resetState, run by the constructor and by every reintegration)
void refreshEarthRate(const IntegrationParameters &P, const IntegrationState &state, Vector3d &iewn) {
    iewn = P.has_station ? Earth::iewn(P.station, state.p) : P.iewn;
}
} // namespace

void PreintegrationOdo::vehicleRotation(const Vector3d &abv, double cvb[9]) {
    // R = Rz(abv[2]) Ry(abv[1]) Rx(abv[0]); cvb = R^T
    const double sx = std::sin(abv[0]), cx = std::cos(abv[0]), sy = std::sin(abv[1]), cy = std::cos(abv[1]), sz = std::sin(abv[2]), cz = std::cos(abv[2]);
    const double R[3][3] = {{cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx}, {sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx}, {-sy, cy * sx, cy * cx}};
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) cvb[i * 3 + j] = R[j][i];
}

PreintegrationOdo::PreintegrationOdo(std::shared_ptr<IntegrationParameters> parameters, const IMU &imu0, const IntegrationState &state, Variant v)
    : parameters_(std::move(parameters)), variant_(v), start_state_(state), current_state_(state) {
    imu_buffer_.push_back(imu0);
    delta_state_.bg   = state.bg;
    delta_state_.ba   = state.ba;
    delta_state_.sodo = state.sodo;
    jacobian_.assign(NN, 0.0);
    covariance_.assign(NN, 0.0);
    sqrt_information_.assign(NN, 0.0);
    for (int i = 0; i < N; i++) jacobian_[(size_t) i * (N + 1)] = 1.0;
    refreshEarthRate(*parameters_, state, iewn_);
}

void PreintegrationOdo::reintegration(const IntegrationState &state) {
    start_state_ = state;
    dirty_       = true;
    if (variant_ == EARTH_ODO) refreshEarthRate(*parameters_, state, iewn_);
}

struct PreintegrationOdo::Traits {
    typedef PreintegrationOdo Class;
    static constexpr int N = NUM_STATE, IMU_ROW = 9, STATE0 = 17, DELTA = NUM_DELTA, PARAMS = 25;
    static constexpr Variant PLAIN = ODO, EARTH_V = EARTH_ODO;
    static constexpr bool PN_EVERY_VARIANT = false;
    static constexpr const char *batch_name = "icg_preint_odo_batch", *params_name = "icg_preint_odo_batch_params",
                                *eval_name = "icg_preint_odo_evaluate_batch";
    static auto batchEntry() { return &icg_preint_odo_batch; }
    static auto paramsEntry() { return &icg_preint_odo_batch_params; }
    static auto evalEntry() { return &icg_preint_odo_evaluate_batch; }
    static void imuRow(const IMU &s, double *row) {
        const double v[9] = {s.time, s.dt, s.dtheta[0], s.dtheta[1], s.dtheta[2], s.dvel[0], s.dvel[1], s.dvel[2], s.odovel};
        memcpy(row, v, sizeof v);
    }
    static void state0Row(const PreintegrationOdo &p, double *a) {
        stateToArray16(p.start_state_, a);
        a[16] = p.start_state_.sodo;
    }
    static void paramsRow(const PreintegrationOdo &p, double *out25) {
        const IntegrationParameters &P = *p.parameters_;
        const double v[13] = {P.gyr_arw, P.acc_vrw, P.gyr_bias_std, P.acc_bias_std, P.corr_time, P.gravity, p.iewn_[0], p.iewn_[1], p.iewn_[2],
                              P.odo_std[0], P.odo_std[1], P.odo_std[2], P.odo_srw};
        memcpy(out25, v, sizeof v);
        vehicleRotation(P.abv, out25 + 13);
        out25[22] = P.lodo[0], out25[23] = P.lodo[1], out25[24] = P.lodo[2];
    }
    static void deltaRow(const IntegrationState &s, double *a) { deltaToArray(s, a); }
    static bool dirty(const PreintegrationOdo &p) { return p.dirty_; }
    static void store(PreintegrationOdo &p, const double *cur, const double *del, const double *jac, const double *cov, double dt,
                      const double *pn, int pn_rows) {
        p.storeIntegrationResult(cur, del, jac, cov, dt, pn, pn_rows, p.iewn_);
    }
    static void finishHost(PreintegrationOdo &p) {
        p.updateSqrtInformation();
        p.dirty_ = false;
    }
    static void finishDevice(PreintegrationOdo &p, const double *S, bool ok) {
        p.sqrt_information_.assign(S, S + NN);
        p.sqrt_information_ok_ = ok;
        p.dirty_               = false;
    }
};

void PreintegrationOdo::deltaToArray(const IntegrationState &s, double *a) {
    stateToArray16(s, a);
    a[16] = s.s[0], a[17] = s.s[1], a[18] = s.s[2], a[19] = s.sodo;
}

bool PreintegrationOdo::integrateBatchAvailable() { return &icg_preint_odo_batch != nullptr; }
bool PreintegrationOdo::evaluateBatchAvailable() { return &icg_preint_odo_evaluate_batch != nullptr; }

void PreintegrationOdo::setIntegrationResult(const double *cur16, const double *delta20, const double *jac361, const double *cov361,
                                             double delta_time, const double *pn, int pn_rows, const Vector3d &iewn) {
    storeIntegrationResult(cur16, delta20, jac361, cov361, delta_time, pn, pn_rows, iewn);
    updateSqrtInformation();
    dirty_ = false;
}

void PreintegrationOdo::storeIntegrationResult(const double *cur16, const double *delta20, const double *jac361, const double *cov361,
                                               double delta_time, const double *pn, int pn_rows, const Vector3d &iewn) {
    stateFromArray16(cur16, current_state_);
    current_state_.sodo = start_state_.sodo;
    current_state_.time = imu_buffer_.back().time;
    deltaFromArray20(delta20, delta_state_);
    jacobian_.assign(jac361, jac361 + NN);
    covariance_.assign(cov361, cov361 + NN);
    delta_time_ = delta_time;
    pn_.assign(pn, pn + (pn ? 4 * (size_t) (pn_rows > 0 ? pn_rows : 0) : 0));
    iewn_ = iewn;
}

bool PreintegrationOdo::integrateBatch(icg_ctx *ctx, const vector<PreintegrationOdo *> &list, std::string *err) {
    return integrateBatchT<Traits>(ctx, list, err);
}

bool PreintegrationOdo::integrateStreamsAvailable() { return &icg_preint_odo_batch_params != nullptr; }

bool PreintegrationOdo::integrateStreams(icg_ctx *ctx, const vector<PreintegrationOdo *> &list, std::string *err) {
    return integrateStreamsT<Traits>(ctx, list, err);
}

bool PreintegrationOdo::evaluateBatch(icg_ctx *ctx, const vector<const PreintegrationOdo *> &list, const double *points, double *residuals,
                                      double *jacobians, vector<char> *ok, std::string *err, double *sqrt_info) {
    return evaluateBatchT<Traits>(ctx, list, points, residuals, jacobians, ok, err, sqrt_info);
}

// the square-root information of covariance_ (preint_common.h), formed once when an integration result arrives
void PreintegrationOdo::updateSqrtInformation() {
    sqrt_information_.assign(NN, 0.0);
    sqrt_information_ok_ = preintSqrtInformation<N>(covariance_.data(), sqrt_information_.data());
}

void PreintegrationOdo::correctionQuaternion(const double *mix0, double q_xyzw[4]) const {
    M3 dq_dbg;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) dq_dbg.m[i][j] = jacobian_[(size_t) (6 + i) * N + 9 + j];
    V3 bg0{mix0[3], mix0[4], mix0[5]}, dbg0{delta_state_.bg[0], delta_state_.bg[1], delta_state_.bg[2]};
    V3 dbg = bg0 - dbg0;
    Q4 q   = rotvec2quat(mv(dq_dbg, dbg));
    q_xyzw[0] = q.x, q_xyzw[1] = q.y, q_xyzw[2] = q.z, q_xyzw[3] = q.w;
}

void PreintegrationOdo::earthRateQuaternion(double q_xyzw[4]) const {
    Q4 q{0, 0, 0, 1};
    if (variant_ == EARTH_ODO) {
        V3 iewn{iewn_[0], iewn_[1], iewn_[2]};
        const double T = delta_time_;
        q              = rotvec2quat(-iewn * T);
    }
    q_xyzw[0] = q.x, q_xyzw[1] = q.y, q_xyzw[2] = q.z, q_xyzw[3] = q.w;
}

bool PreintegrationOdo::evaluate(const double *const *parameters, double *residuals, double **jacobians) const {
    if (dirty_) return false;                // not integrated for the current buffer/start state: evaluation failed, loudly
    if (!sqrt_information_ok_) return false; // singular covariance
    double q_corr[4], q_nn[4];
    correctionQuaternion(parameters[1], q_corr);
    earthRateQuaternion(q_nn);
    return evaluateGiven(parameters, q_corr, q_nn, residuals, jacobians);
}

bool PreintegrationOdo::evaluateGiven(const double *const *parameters, const double q_corr[4], const double q_nn[4], double *residuals,
                                      double **jacobians) const {
    if (dirty_) return false;
    if (!sqrt_information_ok_) return false;
    typedef double MN[N][N];
    MN jac, S;
    memcpy(jac, jacobian_.data(), sizeof jac);
    memcpy(S, sqrt_information_.data(), sizeof S);
    // constructState (odo :185-204)
    const double *pose0 = parameters[0], *mix0 = parameters[1], *pose1 = parameters[2], *mix1 = parameters[3];
    V3 p0{pose0[0], pose0[1], pose0[2]}, p1{pose1[0], pose1[1], pose1[2]};
    Q4 q0{pose0[3], pose0[4], pose0[5], pose0[6]}, q1{pose1[3], pose1[4], pose1[5], pose1[6]};
    V3 v0{mix0[0], mix0[1], mix0[2]}, bg0{mix0[3], mix0[4], mix0[5]}, ba0{mix0[6], mix0[7], mix0[8]};
    V3 v1{mix1[0], mix1[1], mix1[2]}, bg1{mix1[3], mix1[4], mix1[5]}, ba1{mix1[6], mix1[7], mix1[8]};
    const double sodo0 = mix0[9], sodo1 = mix1[9];
    V3 gravity{0, 0, parameters_->gravity};
    V3 iewn{iewn_[0], iewn_[1], iewn_[2]};
    const IntegrationState &d = delta_state_;
    V3 dp{d.p[0], d.p[1], d.p[2]}, dv{d.v[0], d.v[1], d.v[2]}, dbg0{d.bg[0], d.bg[1], d.bg[2]}, dba0{d.ba[0], d.ba[1], d.ba[2]};
    V3 dsd{d.s[0], d.s[1], d.s[2]};
    Q4 dq{d.q.x, d.q.y, d.q.z, d.q.w};
    auto blk = [&](int r, int c) {
        M3 b;
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) b.m[i][j] = jac[r + i][c + j];
        return b;
    };
    M3 dp_dbg = blk(0, 9), dp_dba = blk(0, 12), dv_dbg = blk(3, 9), dv_dba = blk(3, 12), dq_dbg = blk(6, 9), ds_dbg = blk(15, 9);
    V3 ds_dsodo{jac[15][18], jac[16][18], jac[17][18]};
    V3 dbg = bg0 - dbg0, dba = ba0 - dba0;
    const double dsodo = sodo0 - d.sodo;
    V3 corrected_p = dp + mv(dp_dba, dba) + mv(dp_dbg, dbg);
    V3 corrected_v = dv + mv(dv_dba, dba) + mv(dv_dbg, dbg);
    Q4 corrected_q = qmul(dq, Q4{q_corr[0], q_corr[1], q_corr[2], q_corr[3]});
    V3 corrected_s = dsd + mv(ds_dbg, dbg) + dsodo * ds_dsodo;
    const double T = delta_time_;

    double r[N];
    double J0[N][7], J1[N][10], J2[N][7], J3[N][10];
    memset(J0, 0, sizeof J0);
    memset(J1, 0, sizeof J1);
    memset(J2, 0, sizeof J2);
    memset(J3, 0, sizeof J3);
    auto put = [](auto &J, int r0, int c0, const M3 &b) {
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) J[r0 + i][c0 + j] = b.m[i][j];
    };
    M3 cnb0 = qmat(qinv(q0));
    V3 rds;
    if (variant_ == ODO) {
        V3 dpn = p1 - p0 - v0 * T - 0.5 * gravity * T * T;
        V3 dvn = v1 - v0 - gravity * T;
        V3 rdp = qrot(qinv(q0), dpn), rdv = qrot(qinv(q0), dvn);
        rds    = qrot(qinv(q0), p1 - p0);
        V3 rp = rdp - corrected_p, rv = rdv - corrected_v;
        Q4 qe = qmul(qmul(qinv(corrected_q), qinv(q0)), q1);
        r[0] = rp.x, r[1] = rp.y, r[2] = rp.z, r[3] = rv.x, r[4] = rv.y, r[5] = rv.z, r[6] = 2 * qe.x, r[7] = 2 * qe.y, r[8] = 2 * qe.z;
        put(J0, 0, 0, scale(cnb0, -1.0));
        put(J0, 0, 3, skew(rdp));
        put(J0, 3, 3, skew(rdv));
        put(J0, 6, 3, scale(qleft_qright_br(qmul(qinv(q1), q0), corrected_q), -1.0));
        put(J2, 0, 0, cnb0);
        put(J2, 6, 3, qleft_br(qe));
        put(J1, 6, 3, mul(scale(qleft_br(qmul(qmul(qinv(q1), q0), dq)), -1.0), dq_dbg));
    } else {
        M3 iewn_skew = skew(iewn);
        V3 p_cor{0, 0, 0};
        for (size_t k = 0; k + 3 < pn_.size(); k += 4) p_cor = p_cor + (V3{pn_[k + 1], pn_[k + 2], pn_[k + 3]} - p0) * pn_[k];
        p_cor    = mv(scale(iewn_skew, 2.0), p_cor);
        V3 v_cor = mv(scale(iewn_skew, 2.0), p1 - p0);
        Q4 qnn{q_nn[0], q_nn[1], q_nn[2], q_nn[3]};
        V3 dpn   = p1 - p0 - v0 * T - 0.5 * gravity * T * T + p_cor;
        V3 dvn   = v1 - v0 - gravity * T + v_cor;
        Q4 qb0b1 = qmul(qmul(qinv(q1), qnn), q0);
        V3 rdp = mv(cnb0, dpn), rdv = mv(cnb0, dvn);
        rds    = mv(cnb0, p1 - p0);
        V3 rp = rdp - corrected_p, rv = rdv - corrected_v;
        Q4 qe = qmul(qb0b1, corrected_q);
        r[0] = rp.x, r[1] = rp.y, r[2] = rp.z, r[3] = rv.x, r[4] = rv.y, r[5] = rv.z, r[6] = 2 * qe.x, r[7] = 2 * qe.y, r[8] = 2 * qe.z;
        put(J0, 0, 0, add(scale(cnb0, -1.0), scale(mul(scale(cnb0, 2.0), iewn_skew), -T)));
        put(J0, 0, 3, skew(rdp));
        put(J0, 3, 0, mul(scale(cnb0, -2.0), iewn_skew));
        put(J0, 3, 3, skew(rdv));
        put(J0, 6, 3, qleft_qright_br(qb0b1, corrected_q));
        put(J2, 0, 0, cnb0);
        put(J2, 3, 0, mul(scale(cnb0, 2.0), iewn_skew));
        put(J2, 6, 3, scale(qright_br(qe), -1.0));
        put(J1, 6, 3, mul(qleft_br(qmul(qb0b1, dq)), dq_dbg));
    }
    put(J0, 15, 0, scale(cnb0, -1.0));
    put(J0, 15, 3, skew(rds));
    put(J2, 15, 0, cnb0);
    put(J1, 0, 0, scale(cnb0, -T));
    put(J1, 0, 3, scale(dp_dbg, -1.0));
    put(J1, 0, 6, scale(dp_dba, -1.0));
    put(J1, 3, 0, scale(cnb0, -1.0));
    put(J1, 3, 3, scale(dv_dbg, -1.0));
    put(J1, 3, 6, scale(dv_dba, -1.0));
    put(J1, 9, 3, scale(eye(), -1.0));
    put(J1, 12, 6, scale(eye(), -1.0));
    put(J1, 15, 3, scale(ds_dbg, -1.0));
    J1[15][9] = ds_dsodo.x * -1.0, J1[16][9] = ds_dsodo.y * -1.0, J1[17][9] = ds_dsodo.z * -1.0;
    J1[18][9] = -1.0;
    put(J3, 3, 0, cnb0);
    put(J3, 9, 3, eye());
    put(J3, 12, 6, eye());
    J3[18][9] = 1.0;
    V3 rbg = bg1 - bg0, rba = ba1 - ba0, rs = rds - corrected_s;
    r[9] = rbg.x, r[10] = rbg.y, r[11] = rbg.z, r[12] = rba.x, r[13] = rba.y, r[14] = rba.z;
    r[15] = rs.x, r[16] = rs.y, r[17] = rs.z, r[18] = sodo1 - sodo0;
    for (int i = 0; i < N; i++) {
        double s = 0;
        for (int k = 0; k < N; k++) s += S[i][k] * r[k];
        residuals[i] = s;
    }
    if (jacobians) {
        auto emit = [&](auto &J, int cols, double *out) {
            if (!out) return;
            for (int i = 0; i < N; i++)
                for (int j = 0; j < cols; j++) {
                    double s = 0;
                    for (int k = 0; k < N; k++) s += S[i][k] * J[k][j];
                    out[i * cols + j] = s;
                }
        };
        emit(J0, 7, jacobians[0]);
        emit(J1, 10, jacobians[1]);
        emit(J2, 7, jacobians[2]);
        emit(J3, 10, jacobians[3]);
    }
    return true;
}

PreintegrationOdoFactor::PreintegrationOdoFactor(std::shared_ptr<PreintegrationOdo> preintegration)
    : preintegration_(std::move(preintegration)) {
    *mutable_parameter_block_sizes() = std::vector<int32_t>{7, 10, 7, 10}; // numBlocksParameters (odo :165-167)
    set_num_residuals(PreintegrationOdo::NUM_STATE);
}

} // namespace icg
