// Preintegration on the HIP C ABI, for both families (PreintegrationT<PreintegrationFamily>: Normal / Earth, 15 states;
// PreintegrationT<PreintegrationOdoFamily>: Odo / EarthOdo, 19 states).  P1 (the per-sample inner loop) runs batched on the device through the
// family's *_batch entry (integrateBatch: one launch per group of equal parameter values, the square-root information formed here) or its
// *_batch_params entry (integrateStreams: the intervals of many streams in one call per variant, a parameter row per interval, the
// square-root information formed on the device).  P2 (residual + Jacobians, preintegration_normal.cc:38-142 / preintegration_earth.cc:37-164 /
// preintegration_odo.cc:40-159 / preintegration_earth_odo.cc:41-183, wrapped by preintegration_factor.h:45-69) is a handful of 3x3 / N x N
// operations per factor (<= 15 factors per solve) and stays on the host, in the Ceres callback thread that asks for it.  evaluateBatch() is
// the same evaluation for MANY factors at once on the device (the *_evaluate_batch entry): for callers that hold thousands of integrated
// intervals, not for the per-factor Ceres callback.
// evaluate() is split at its two rotvec2quat calls (correctionQuaternion, earthRateQuaternion) from the rest (evaluateGiven): a driver that
// keeps the factors resident on the device for a solve (PreintegrationSetT, preint_set_hip.cc) ships the two quaternions, and the device
// result has evaluate()'s bits: evaluateGiven is written ONCE, the odometer rows behind `if constexpr`, and the device kernels of both
// families are held to its operands and its order.
#include "earth.h"
#include "preint_common.h"
#include "preintegration_odo.h"

// A build of this layer on another implementation of the C ABI (the CPU checker library) may not have these entry points: the references
// stay weak (null when absent) and the callers report it; the product library links libicgvins_hip.so, which defines them.
#pragma weak icg_preint_evaluate_batch
#pragma weak icg_preint_batch_params
#pragma weak icg_preint_odo_batch
#pragma weak icg_preint_odo_evaluate_batch
#pragma weak icg_preint_odo_batch_params

namespace icg {

using namespace preint_math;

// ---------------------------------------------------------------- the two family records: what is not inline -----------------------------------
decltype(&icg_preint_batch) PreintegrationFamily::batchEntry() { return &icg_preint_batch; }
decltype(&icg_preint_batch_params) PreintegrationFamily::paramsEntry() { return &icg_preint_batch_params; }
decltype(&icg_preint_evaluate_batch) PreintegrationFamily::evalEntry() { return &icg_preint_evaluate_batch; }

decltype(&icg_preint_odo_batch) PreintegrationOdoFamily::batchEntry() { return &icg_preint_odo_batch; }
decltype(&icg_preint_odo_batch_params) PreintegrationOdoFamily::paramsEntry() { return &icg_preint_odo_batch_params; }
decltype(&icg_preint_odo_evaluate_batch) PreintegrationOdoFamily::evalEntry() { return &icg_preint_odo_evaluate_batch; }
void PreintegrationOdoFamily::vehicleRotation(const Vector3d &abv, double cvb[9]) {
    // R = Rz(abv[2]) Ry(abv[1]) Rx(abv[0]); cvb = R^T
    const double sx = std::sin(abv[0]), cx = std::cos(abv[0]), sy = std::sin(abv[1]), cy = std::cos(abv[1]), sz = std::sin(abv[2]), cz = std::cos(abv[2]);
    const double R[3][3] = {{cz * cy, cz * sy * sx - sz * cx, cz * sy * cx + sz * sx}, {sz * cy, sz * sy * sx + cz * cx, sz * sy * cx - cz * sx}, {-sy, cy * sx, cy * cx}};
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) cvb[i * 3 + j] = R[j][i];
}

// ---------------------------------------------------------------- the object ----------------------------------------------------------------------
template <class F>
PreintegrationT<F>::PreintegrationT(std::shared_ptr<IntegrationParameters> parameters, const IMU &imu0, const IntegrationState &state, Variant v)
    : parameters_(std::move(parameters)), variant_(v), start_state_(state), current_state_(state) {
    imu_buffer_.push_back(imu0);
    delta_state_.bg = state.bg;
    delta_state_.ba = state.ba;
    if constexpr (F::HAS_ODO) delta_state_.sodo = state.sodo;
    jacobian_.assign(NUM_COV, 0.0);
    covariance_.assign(NUM_COV, 0.0);
    sqrt_information_.assign(NUM_COV, 0.0);
    for (int i = 0; i < F::NUM_STATE; i++) jacobian_[(size_t) i * (F::NUM_STATE + 1)] = 1.0;
    refreshEarthRate();
}

// preintegration_earth.cc:319-321, preintegration_earth_odo.cc:364-366 (resetState, run by the constructor and by every reintegration)
template <class F> void PreintegrationT<F>::refreshEarthRate() {
    iewn_ = parameters_->has_station ? Earth::iewn(parameters_->station, start_state_.p) : parameters_->iewn;
}

template <class F> void PreintegrationT<F>::reintegration(const IntegrationState &state) {
    start_state_ = state;
    dirty_       = true;
    if (variant_ == F::EARTH_VARIANT) refreshEarthRate();
}

template <class F>
void PreintegrationT<F>::storeIntegrationResult(const double *cur16, const double *delta, const double *jac, const double *cov, double delta_time,
                                                const double *pn, int pn_rows, const Vector3d &iewn) {
    stateFromArray16(cur16, current_state_);
    if constexpr (F::HAS_ODO) current_state_.sodo = start_state_.sodo;
    current_state_.time = imu_buffer_.back().time;
    F::deltaFromRow(delta, delta_state_);
    jacobian_.assign(jac, jac + NUM_COV);
    covariance_.assign(cov, cov + NUM_COV);
    delta_time_ = delta_time;
    pn_.assign(pn, pn + (pn ? 4 * (size_t) (pn_rows > 0 ? pn_rows : 0) : 0));
    iewn_ = iewn;
}

template <class F>
void PreintegrationT<F>::setIntegrationResult(const double *cur16, const double *delta, const double *jac, const double *cov, double delta_time,
                                              const double *pn, int pn_rows, const Vector3d &iewn) {
    storeIntegrationResult(cur16, delta, jac, cov, delta_time, pn, pn_rows, iewn);
    updateSqrtInformation();
    dirty_ = false;
}

// the square-root information of covariance_ (preint_common.h), formed once when an integration result arrives
template <class F> void PreintegrationT<F>::updateSqrtInformation() {
    sqrt_information_.assign(NUM_COV, 0.0);
    sqrt_information_ok_ = preintSqrtInformation<F::NUM_STATE>(covariance_.data(), sqrt_information_.data());
}

template <class F> bool PreintegrationT<F>::integrateBatchAvailable() { return F::batchEntry() != nullptr; }
template <class F> bool PreintegrationT<F>::integrateStreamsAvailable() { return F::paramsEntry() != nullptr; }
template <class F> bool PreintegrationT<F>::evaluateBatchAvailable() { return F::evalEntry() != nullptr; }

// ---------------------------------------------------------------- the batch drivers ---------------------------------------------------------------
template <class F>
void PreintegrationT<F>::stageIntervals(const vector<PreintegrationT *> &todo, vector<int32_t> &offsets, vector<double> &imu, vector<double> &state0) {
    offsets.assign(1, 0);
    for (auto *p : todo) {
        for (const IMU &s : p->imu_buffer_) {
            double row[F::IMU_ROW];
            F::imuRow(s, row);
            imu.insert(imu.end(), row, row + F::IMU_ROW);
        }
        offsets.push_back((int32_t) (imu.size() / F::IMU_ROW));
        double a[F::STATE0_ROW];
        F::state0Row(p->start_state_, a);
        state0.insert(state0.end(), a, a + F::STATE0_ROW);
    }
}

template <class F>
void PreintegrationT<F>::storeIntervals(const vector<PreintegrationT *> &todo, int variant, const vector<int32_t> &offsets, const vector<double> &cur,
                                        const vector<double> &del, const vector<double> &jac, const vector<double> &cov, const vector<double> &dt,
                                        const vector<double> &pn, const double *S, const int32_t *status) {
    constexpr size_t NN = NUM_COV;
    for (size_t k = 0; k < todo.size(); k++) {
        PreintegrationT &p = *todo[k];
        const int b = offsets[k], cnt = offsets[k + 1] - offsets[k];
        p.storeIntegrationResult(&cur[16 * k], &del[F::NUM_DELTA * k], &jac[NN * k], &cov[NN * k], dt[k],
                                 F::PN_EVERY_VARIANT || variant == (int) F::EARTH_VARIANT ? &pn[4 * (size_t) b] : nullptr, cnt - 1, p.iewn_);
        if (S) {
            p.sqrt_information_.assign(S + NN * k, S + NN * (k + 1));
            p.sqrt_information_ok_ = status[k] == 0;
        } else {
            p.updateSqrtInformation();
        }
        p.dirty_ = false;
    }
}

// one launch per (variant, parameter values): the *_batch entry takes one parameter vector per call, and every interval must be integrated
// with ITS OWN Earth rate (the one evaluate() uses).  Intervals of one estimator share their values in practice.
template <class F> bool PreintegrationT<F>::integrateBatch(icg_ctx *ctx, const vector<PreintegrationT *> &list, std::string *err) {
    constexpr size_t NN = NUM_COV;
    const auto entry    = F::batchEntry();
    if (!entry) {
        if (err) *err = std::string(F::BATCH_NAME) + " is not in this build";
        return false;
    }
    vector<PreintegrationT *> pending;
    for (auto *p : list)
        if (p->dirty_) pending.push_back(p);
    while (!pending.empty()) {
        double params[F::PARAMS_ROW];
        F::paramsRow(*pending[0]->parameters_, pending[0]->iewn_, params);
        const int variant = (int) pending[0]->variant();
        vector<PreintegrationT *> todo, rest;
        for (auto *p : pending) {
            double q[F::PARAMS_ROW];
            F::paramsRow(*p->parameters_, p->iewn_, q);
            ((int) p->variant() == variant && memcmp(q, params, sizeof q) == 0 ? todo : rest).push_back(p);
        }
        pending.swap(rest);
        vector<int32_t> offsets;
        vector<double> imu, state0;
        stageIntervals(todo, offsets, imu, state0);
        const size_t n = todo.size(), total = imu.size() / F::IMU_ROW;
        vector<double> cur(16 * n), del(F::NUM_DELTA * n), jac(NN * n), cov(NN * n), dt(n), pn(4 * total);
        int rc = entry(ctx, variant, (int) n, offsets.data(), imu.data(), state0.data(), params, cur.data(), del.data(), jac.data(), cov.data(),
                       dt.data(), pn.data());
        if (rc != ICG_OK) {
            if (err) *err = icg_last_error(ctx);
            return false;
        }
        storeIntervals(todo, variant, offsets, cur, del, jac, cov, dt, pn, nullptr, nullptr);
    }
    return true;
}

// one call per variant present: every interval brings its own parameter row (its own Earth rate), and the device forms the square-root
// information behind the integration, so updateSqrtInformation does not run
template <class F> bool PreintegrationT<F>::integrateStreams(icg_ctx *ctx, const vector<PreintegrationT *> &list, std::string *err) {
    constexpr size_t NN = NUM_COV;
    const auto entry    = F::paramsEntry();
    if (!entry) {
        if (err) *err = std::string(F::PARAMS_NAME) + " is not in this build";
        return false;
    }
    for (int variant = (int) F::PLAIN_VARIANT; variant <= (int) F::EARTH_VARIANT; variant++) {
        vector<PreintegrationT *> todo;
        for (auto *p : list)
            if (p->dirty_ && (int) p->variant() == variant) todo.push_back(p);
        if (todo.empty()) continue;
        vector<int32_t> offsets;
        vector<double> imu, state0, params;
        stageIntervals(todo, offsets, imu, state0);
        for (auto *p : todo) {
            double row[F::PARAMS_ROW];
            F::paramsRow(*p->parameters_, p->iewn_, row);
            params.insert(params.end(), row, row + F::PARAMS_ROW);
        }
        const size_t n = todo.size(), total = imu.size() / F::IMU_ROW;
        vector<double> cur(16 * n), del(F::NUM_DELTA * n), jac(NN * n), cov(NN * n), dt(n), pn(4 * total), S(NN * n);
        vector<int32_t> status(n);
        int rc = entry(ctx, variant, (int) n, offsets.data(), imu.data(), state0.data(), params.data(), cur.data(), del.data(), jac.data(),
                       cov.data(), dt.data(), pn.data(), S.data(), status.data());
        if (rc != ICG_OK) {
            if (err) *err = icg_last_error(ctx);
            return false;
        }
        storeIntervals(todo, variant, offsets, cur, del, jac, cov, dt, pn, S.data(), status.data());
    }
    return true;
}

// P2 of every integrated factor of the list on the device, one call per variant present; zero rows and ok = 0 for the others
template <class F>
bool PreintegrationT<F>::evaluateBatch(icg_ctx *ctx, const vector<const PreintegrationT *> &list, const double *points, double *residuals,
                                       double *jacobians, vector<char> *ok, std::string *err, double *sqrt_info) {
    constexpr size_t N = F::NUM_STATE, NN = NUM_COV, POINT = NUM_POINT, JAC = NUM_JAC, DELTA = F::NUM_DELTA;
    const auto entry = F::evalEntry();
    if (!entry) {
        if (err) *err = std::string(F::EVAL_NAME) + " is not in this build";
        return false;
    }
    const size_t n_all = list.size();
    if (ok) ok->assign(n_all, 0);
    memset(residuals, 0, sizeof(double) * N * n_all);
    if (jacobians) memset(jacobians, 0, sizeof(double) * JAC * n_all);
    if (sqrt_info) memset(sqrt_info, 0, sizeof(double) * NN * n_all);
    for (int variant = (int) F::PLAIN_VARIANT; variant <= (int) F::EARTH_VARIANT; variant++) {
        vector<size_t> idx; // the integrated factors of this variant, list order
        for (size_t k = 0; k < n_all; k++)
            if ((int) list[k]->variant() == variant && !list[k]->dirty_) idx.push_back(k);
        if (idx.empty()) continue;
        const size_t n   = idx.size();
        const bool earth = variant == (int) F::EARTH_VARIANT;
        vector<double> del(DELTA * n), jac(NN * n), cov(NN * n), dt(n), env(4 * n), pts(POINT * n), pn;
        vector<int32_t> pn_off{0};
        for (size_t j = 0; j < n; j++) {
            const PreintegrationT &p = *list[idx[j]];
            F::deltaRow(p.delta_state_, &del[DELTA * j]);
            memcpy(&jac[NN * j], p.jacobian_.data(), sizeof(double) * NN);
            memcpy(&cov[NN * j], p.covariance_.data(), sizeof(double) * NN);
            dt[j]          = p.delta_time_;
            env[4 * j]     = p.gravity();
            env[4 * j + 1] = p.iewn_[0], env[4 * j + 2] = p.iewn_[1], env[4 * j + 3] = p.iewn_[2];
            memcpy(&pts[POINT * j], points + POINT * idx[j], sizeof(double) * POINT);
            if (earth) {
                pn.insert(pn.end(), p.pn_.begin(), p.pn_.begin() + (long) (p.pn_.size() / 4 * 4));
                pn_off.push_back((int32_t) (pn.size() / 4));
            }
        }
        vector<double> r(N * n), J(jacobians ? JAC * n : 0), S(sqrt_info ? NN * n : 0);
        vector<int32_t> status(n);
        if (pn.empty()) pn.resize(4); // (a valid pointer for a batch without rows)
        int rc = entry(ctx, variant, (int) n, del.data(), jac.data(), cov.data(), dt.data(), env.data(), earth ? pn_off.data() : nullptr,
                       earth ? pn.data() : nullptr, pts.data(), r.data(), jacobians ? J.data() : nullptr, sqrt_info ? S.data() : nullptr,
                       status.data());
        if (rc != ICG_OK) {
            if (err) *err = icg_last_error(ctx);
            return false;
        }
        for (size_t j = 0; j < n; j++) {
            const size_t k = idx[j];
            memcpy(residuals + N * k, &r[N * j], sizeof(double) * N);
            if (jacobians) memcpy(jacobians + JAC * k, &J[JAC * j], sizeof(double) * JAC);
            if (sqrt_info) memcpy(sqrt_info + NN * k, &S[NN * j], sizeof(double) * NN);
            if (ok) (*ok)[k] = status[j] == 0 ? 1 : 0;
        }
    }
    return true;
}

// ---------------------------------------------------------------- P2 on the host ------------------------------------------------------------------
template <class F> void PreintegrationT<F>::correctionQuaternion(const double *mix0, double q_xyzw[4]) const {
    M3 dq_dbg;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) dq_dbg.m[i][j] = jacobian_[(size_t) (6 + i) * F::NUM_STATE + 9 + j];
    V3 bg0{mix0[3], mix0[4], mix0[5]}, dbg0{delta_state_.bg[0], delta_state_.bg[1], delta_state_.bg[2]};
    V3 dbg = bg0 - dbg0;
    Q4 q   = rotvec2quat(mv(dq_dbg, dbg));
    q_xyzw[0] = q.x, q_xyzw[1] = q.y, q_xyzw[2] = q.z, q_xyzw[3] = q.w;
}

template <class F> void PreintegrationT<F>::earthRateQuaternion(double q_xyzw[4]) const {
    Q4 q{0, 0, 0, 1};
    if (variant_ == F::EARTH_VARIANT) {
        V3 iewn{iewn_[0], iewn_[1], iewn_[2]};
        const double T = delta_time_;
        q              = rotvec2quat(-iewn * T);
    }
    q_xyzw[0] = q.x, q_xyzw[1] = q.y, q_xyzw[2] = q.z, q_xyzw[3] = q.w;
}

template <class F> bool PreintegrationT<F>::evaluate(const double *const *parameters, double *residuals, double **jacobians) const {
    if (dirty_) return false;                // not integrated for the current buffer/start state: evaluation failed, loudly
    if (!sqrt_information_ok_) return false; // singular covariance
    double q_corr[4], q_nn[4];
    correctionQuaternion(parameters[1], q_corr);
    earthRateQuaternion(q_nn);
    return evaluateGiven(parameters, q_corr, q_nn, residuals, jacobians);
}

template <class F>
bool PreintegrationT<F>::evaluateGiven(const double *const *parameters, const double q_corr[4], const double q_nn[4], double *residuals,
                                       double **jacobians) const {
    if (dirty_) return false;
    if (!sqrt_information_ok_) return false;
    constexpr int N = F::NUM_STATE, MIX = F::NUM_MIX;
    constexpr bool WITH_ODO = F::HAS_ODO;
    typedef double MN[N][N];
    MN jac, S;
    memcpy(jac, jacobian_.data(), sizeof jac);
    memcpy(S, sqrt_information_.data(), sizeof S);
    // constructState (normal :162-180, odo :185-204)
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
    // the odometer rows (read and written under WITH_ODO alone): the corrected distance, and rds, the travelled distance in the body frame
    [[maybe_unused]] M3 ds_dbg;
    [[maybe_unused]] V3 ds_dsodo, corrected_s, rds;
    if constexpr (WITH_ODO) {
        ds_dbg   = blk(15, 9);
        ds_dsodo = V3{jac[15][18], jac[16][18], jac[17][18]};
        V3 dsd{d.s[0], d.s[1], d.s[2]};
        const double dsodo = mix0[9] - d.sodo;
        corrected_s        = dsd + mv(ds_dbg, dbg) + dsodo * ds_dsodo;
    }
    const double T = delta_time_;

    double r[N];
    double J0[N][7], J1[N][MIX], J2[N][7], J3[N][MIX];
    memset(J0, 0, sizeof J0);
    memset(J1, 0, sizeof J1);
    memset(J2, 0, sizeof J2);
    memset(J3, 0, sizeof J3);
    auto put = [](auto &J, int r0, int c0, const M3 &b) {
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) J[r0 + i][c0 + j] = b.m[i][j];
    };
    M3 cnb0 = qmat(qinv(q0));
    if (variant_ == F::PLAIN_VARIANT) {
        V3 dpn = p1 - p0 - v0 * T - 0.5 * gravity * T * T;
        V3 dvn = v1 - v0 - gravity * T;
        V3 rdp = qrot(qinv(q0), dpn), rdv = qrot(qinv(q0), dvn);
        if constexpr (WITH_ODO) rds = qrot(qinv(q0), p1 - p0);
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
        if constexpr (WITH_ODO) rds = mv(cnb0, p1 - p0);
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
    put(J1, 0, 0, scale(cnb0, -T));
    put(J1, 0, 3, scale(dp_dbg, -1.0));
    put(J1, 0, 6, scale(dp_dba, -1.0));
    put(J1, 3, 0, scale(cnb0, -1.0));
    put(J1, 3, 3, scale(dv_dbg, -1.0));
    put(J1, 3, 6, scale(dv_dba, -1.0));
    put(J1, 9, 3, scale(eye(), -1.0));
    put(J1, 12, 6, scale(eye(), -1.0));
    put(J3, 3, 0, cnb0);
    put(J3, 9, 3, eye());
    put(J3, 12, 6, eye());
    V3 rbg = bg1 - bg0, rba = ba1 - ba0;
    r[9] = rbg.x, r[10] = rbg.y, r[11] = rbg.z, r[12] = rba.x, r[13] = rba.y, r[14] = rba.z;
    if constexpr (WITH_ODO) {
        put(J0, 15, 0, scale(cnb0, -1.0));
        put(J0, 15, 3, skew(rds));
        put(J2, 15, 0, cnb0);
        put(J1, 15, 3, scale(ds_dbg, -1.0));
        J1[15][9] = ds_dsodo.x * -1.0, J1[16][9] = ds_dsodo.y * -1.0, J1[17][9] = ds_dsodo.z * -1.0;
        J1[18][9] = -1.0;
        J3[18][9] = 1.0;
        V3 rs = rds - corrected_s;
        r[15] = rs.x, r[16] = rs.y, r[17] = rs.z, r[18] = mix1[9] - mix0[9];
    }
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
        emit(J1, MIX, jacobians[1]);
        emit(J2, 7, jacobians[2]);
        emit(J3, MIX, jacobians[3]);
    }
    return true;
}

template class PreintegrationT<PreintegrationFamily>;
template class PreintegrationT<PreintegrationOdoFamily>;

} // namespace icg
