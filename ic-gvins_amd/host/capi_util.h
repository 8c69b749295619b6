// Shared by the capi_*.cc files (the extern "C" surface of libicgvins_host.so) and included by nothing else: the guard that owns the
// one try/catch, the temporary device context, the flat-array <-> object converters, the best-of-reps timer and the test-only cost
// functions.  Everything has internal linkage.
#pragma once
#include <chrono>
#include <cstdio>
#include <cstring>
#include <memory>
#include <stdexcept>

#include "factors.h"
#include "misc_hip.h"
#include "preintegration_odo.h"

namespace {

void set_err(char *err, int errlen, const char *msg) {
    if (err && errlen > 0) snprintf(err, (size_t) errlen, "%s", msg);
}

// body() behind the C API's one try/catch: an exception leaves its text in err and returns `thrown`
template <class R, class F>
R guarded(char *err, int errlen, R thrown, F &&body) {
    try {
        return body();
    } catch (const std::exception &e) {
        set_err(err, errlen, e.what());
        return thrown;
    }
}
template <class F>
int guarded(char *err, int errlen, F &&body) {
    return guarded(err, errlen, -1, body);
}

// A small device context of an entry's own.  Declare it BEFORE any object that holds the context (Preintegration batches,
// MarginalizationLinearizer, MarginalizationPriorSet): those are then destroyed first, on every return and on an exception.  A context
// that cannot be created throws icg_last_error's text, which guarded() turns into rc -1.
struct TempCtx {
    icg_ctx *ctx = nullptr;
    explicit TempCtx(int device) {
        icg_ctx_config cfg{};
        cfg.device = device, cfg.width = 64, cfg.height = 64, cfg.n_slots = 1, cfg.max_batch = 1, cfg.max_points = 64;
        if (icg_ctx_create(&cfg, &ctx) != ICG_OK) throw std::runtime_error(icg_last_error(nullptr));
    }
    ~TempCtx() { icg_ctx_destroy(ctx); }
};

// Best wall time of fn(pass) in seconds: reps + 1 passes, the first one (it pages everything in) untimed unless it is the only one.
// fn returns false to stop: the result is then negative.
template <class F>
double best_of(int reps, F &&fn) {
    const int passes = (reps > 0 ? reps : 0) + 1;
    double best      = -1;
    for (int pass = 0; pass < passes; pass++) {
        const auto a = std::chrono::steady_clock::now();
        if (!fn(pass)) return -1;
        const double t = std::chrono::duration<double>(std::chrono::steady_clock::now() - a).count();
        if ((pass > 0 || passes == 1) && (best < 0 || t < best)) best = t;
    }
    return best;
}

// ---- flat arrays <-> objects: imu rows of 8, INS state rows of 23 (see include/icgvins_hip.h), preintegration state rows of 16 --------
icg::IMU ins_imu(const double *p) {
    icg::IMU s;
    s.time = p[0], s.dt = p[1];
    s.dtheta = icg::Vector3d(p[2], p[3], p[4]);
    s.dvel   = icg::Vector3d(p[5], p[6], p[7]);
    return s;
}
void ins_put_imu(const icg::IMU &m, double *r) {
    r[0] = m.time, r[1] = m.dt;
    for (int k = 0; k < 3; k++) r[2 + k] = m.dtheta[k], r[5 + k] = m.dvel[k];
}
icg::IntegrationState ins_state(const double *r) {
    icg::IntegrationState s;
    s.time = r[0];
    for (int k = 0; k < 3; k++) s.p[k] = r[1 + k], s.v[k] = r[8 + k], s.bg[k] = r[11 + k], s.ba[k] = r[14 + k], s.sg[k] = r[17 + k], s.sa[k] = r[20 + k];
    s.q = icg::Quaterniond{r[4], r[5], r[6], r[7]};
    return s;
}
void ins_put_state(const icg::IntegrationState &s, double *r) {
    r[0] = s.time;
    for (int k = 0; k < 3; k++) r[1 + k] = s.p[k], r[8 + k] = s.v[k], r[11 + k] = s.bg[k], r[14 + k] = s.ba[k], r[17 + k] = s.sg[k], r[20 + k] = s.sa[k];
    r[4] = s.q.x, r[5] = s.q.y, r[6] = s.q.z, r[7] = s.q.w;
}
icg::IntegrationConfiguration ins_config(const double *c) {
    icg::IntegrationConfiguration cfg;
    cfg.gravity     = icg::Vector3d(c[0], c[1], c[2]);
    cfg.iewn        = icg::Vector3d(c[3], c[4], c[5]);
    cfg.iswithearth = c[6] != 0, cfg.iswithscale = c[7] != 0;
    return cfg;
}
icg::InsWindow ins_window(int n, const double *imu, const double *states) {
    icg::InsWindow w;
    for (int k = 0; k < n; k++) w.emplace_back(ins_imu(imu + 8 * (size_t) k), states ? ins_state(states + 23 * (size_t) k) : icg::IntegrationState());
    return w;
}
// p3, q4 (xyzw), v3, bg3, ba3
icg::IntegrationState preint_state(const double *s) {
    icg::IntegrationState st;
    st.p = icg::Vector3d(s[0], s[1], s[2]);
    st.q = icg::Quaterniond{s[3], s[4], s[5], s[6]};
    st.v = icg::Vector3d(s[7], s[8], s[9]), st.bg = icg::Vector3d(s[10], s[11], s[12]), st.ba = icg::Vector3d(s[13], s[14], s[15]);
    return st;
}
void preint_put_state(const icg::IntegrationState &c, double *o) {
    o[0] = c.p[0], o[1] = c.p[1], o[2] = c.p[2], o[3] = c.q.x, o[4] = c.q.y, o[5] = c.q.z, o[6] = c.q.w;
    for (int i = 0; i < 3; i++) o[7 + i] = c.v[i], o[10 + i] = c.bg[i], o[13 + i] = c.ba[i];
}
// params9 as icg_preint_batch takes them
std::shared_ptr<icg::IntegrationParameters> preint_params(const double *params9) {
    auto P          = std::make_shared<icg::IntegrationParameters>();
    P->gyr_arw      = params9[0];
    P->acc_vrw      = params9[1];
    P->gyr_bias_std = params9[2];
    P->acc_bias_std = params9[3];
    P->corr_time    = params9[4];
    P->gravity      = params9[5];
    P->iewn         = icg::Vector3d(params9[6], params9[7], params9[8]);
    return P;
}
// interval k of the imu rows (it owns rows [offsets[k], offsets[k+1])) as a Preintegration object from its start state, a row of 16: the first
// sample in the constructor, the rest through addNewImu.  variant: 0 = NORMAL, otherwise EARTH
std::shared_ptr<icg::Preintegration> preint_interval(int variant, const std::shared_ptr<icg::IntegrationParameters> &params, const int32_t *offsets,
                                                     const double *imu, int k, const double *state16) {
    auto p = std::make_shared<icg::Preintegration>(params, ins_imu(imu + 8 * (size_t) offsets[k]), preint_state(state16),
                                                   variant ? icg::Preintegration::EARTH : icg::Preintegration::NORMAL);
    for (int row = offsets[k] + 1; row < offsets[k + 1]; row++) p->addNewImu(ins_imu(imu + 8 * (size_t) row));
    return p;
}
// ---- the odometer family: parameters of 19 ([0..8] as icg_preint_batch, [9..11] odo_std, [12] odo_srw, [13..15] abv, [16..18] lodo; the host
// forms cvb from abv) and objects from GIVEN integration results
std::shared_ptr<icg::IntegrationParameters> odo_params19(const double *params19) {
    using icg::Vector3d;
    auto P     = preint_params(params19);
    P->odo_std = Vector3d(params19[9], params19[10], params19[11]);
    P->odo_srw = params19[12];
    P->abv     = Vector3d(params19[13], params19[14], params19[15]);
    P->lodo    = Vector3d(params19[16], params19[17], params19[18]);
    return P;
}
// a PreintegrationOdo as if integrateBatch had returned the given result (no device, no IMU samples)
std::shared_ptr<icg::PreintegrationOdo> odo_from_result(const std::shared_ptr<icg::IntegrationParameters> &P, int variant, const double *delta20,
                                                        const double *jac361, const double *cov361, double delta_time, const double *pn, int pn_rows,
                                                        const double *iewn3) {
    using namespace icg;
    IntegrationState st;
    st.bg   = Vector3d(delta20[10], delta20[11], delta20[12]);
    st.ba   = Vector3d(delta20[13], delta20[14], delta20[15]);
    st.sodo = delta20[19];
    auto p  = std::make_shared<PreintegrationOdo>(P, IMU(), st, variant == 2 ? PreintegrationOdo::ODO : PreintegrationOdo::EARTH_ODO);
    double cur16[16];
    preint_put_state(st, cur16);
    p->setIntegrationResult(cur16, delta20, jac361, cov361, delta_time, pn_rows > 0 ? pn : nullptr, pn_rows > 0 ? pn_rows : 0,
                            Vector3d(iewn3[0], iewn3[1], iewn3[2]));
    return p;
}
// factor k of the 15 x n observation table (column c of factor k at obs_soa[c * n + k])
std::unique_ptr<icg::ReprojectionFactor> reproj_factor_from_soa(const double *obs_soa, int n, int k) {
    using icg::Vector3d;
    auto o = [&](int c) { return obs_soa[(size_t) c * n + k]; };
    return std::unique_ptr<icg::ReprojectionFactor>(new icg::ReprojectionFactor(Vector3d(o(0), o(1), o(2)), Vector3d(o(3), o(4), o(5)), Vector3d(o(6), o(7), o(8)),
                                                                                 Vector3d(o(9), o(10), o(11)), o(12), o(13), o(14)));
}

// ---- test-only cost functions ----------------------------------------------------------------------------------------------------------
// simple generic host factor used to exercise the non-reprojection path of MarginalizationInfo:
// residual = w * [p - p0 ; 2 vec(q0^-1 q)] on one pose block (6 residuals, 7 parameters)
class PosePriorFactor : public ceres::SizedCostFunction<6, 7> {
public:
    PosePriorFactor(const double *pose0, double weight) : w_(weight) { memcpy(x0_, pose0, sizeof x0_); }
    bool Evaluate(const double *const *parameters, double *residuals, double **jacobians) const override {
        const double *x = parameters[0];
        const double n2 = x0_[3] * x0_[3] + x0_[4] * x0_[4] + x0_[5] * x0_[5] + x0_[6] * x0_[6];
        const double ax = -x0_[3] / n2, ay = -x0_[4] / n2, az = -x0_[5] / n2, aw = x0_[6] / n2;
        const double bx = x[3], by = x[4], bz = x[5], bw = x[6];
        const double dq[4] = {aw * bx + ax * bw + ay * bz - az * by, aw * by + ay * bw + az * bx - ax * bz,
                              aw * bz + az * bw + ax * by - ay * bx, aw * bw - ax * bx - ay * by - az * bz};
        for (int k = 0; k < 3; k++) {
            residuals[k]     = w_ * (x[k] - x0_[k]);
            residuals[3 + k] = w_ * 2.0 * dq[k];
        }
        if (jacobians && jacobians[0]) {
            memset(jacobians[0], 0, sizeof(double) * 42);
            for (int k = 0; k < 3; k++) {
                jacobians[0][k * 7 + k]           = w_;
                jacobians[0][(3 + k) * 7 + 3 + k] = w_ * dq[3]; // d(2 vec(dq * exp(phi/2)))/dphi ~ w I at dq ~ identity
            }
        }
        return true;
    }

private:
    double x0_[7], w_;
};
// a host factor on a one-dimensional block (an inverse depth): residual = w (x - x0).  On a landmark it breaks the structure the
// landmark-eliminated marginalization relies on (tests: that window then takes the dense M2 + M3)
class ScalarPriorFactor : public ceres::SizedCostFunction<1, 1> {
public:
    ScalarPriorFactor(double x0, double weight) : x0_(x0), w_(weight) {}
    bool Evaluate(const double *const *parameters, double *residuals, double **jacobians) const override {
        residuals[0] = w_ * (parameters[0][0] - x0_);
        if (jacobians && jacobians[0]) jacobians[0][0] = w_;
        return true;
    }

private:
    double x0_, w_;
};
// r = w (x - x0) on one 9-vector block (velocity, gyroscope bias, accelerometer bias): stands in for the part of the
// marginalization prior that anchors the first state's velocity and biases
class MixPriorFactor : public ceres::SizedCostFunction<9, 9> {
public:
    MixPriorFactor(const double *x0, double weight) : w_(weight) { memcpy(x0_, x0, sizeof x0_); }
    bool Evaluate(const double *const *parameters, double *residuals, double **jacobians) const override {
        for (int k = 0; k < 9; k++) residuals[k] = w_ * (parameters[0][k] - x0_[k]);
        if (jacobians && jacobians[0]) {
            memset(jacobians[0], 0, sizeof(double) * 81);
            for (int k = 0; k < 9; k++) jacobians[0][k * 9 + k] = w_;
        }
        return true;
    }

private:
    double x0_[9], w_;
};
// the velocity / bias / scale-factor prior on a 10-wide mix block (MixPriorFactor at 10)
class OdoMixPriorFactor : public ceres::SizedCostFunction<10, 10> {
public:
    OdoMixPriorFactor(const double *x0, double weight) : w_(weight) { memcpy(x0_, x0, sizeof x0_); }
    bool Evaluate(const double *const *parameters, double *residuals, double **jacobians) const override {
        for (int k = 0; k < 10; k++) residuals[k] = w_ * (parameters[0][k] - x0_[k]);
        if (jacobians && jacobians[0]) {
            memset(jacobians[0], 0, sizeof(double) * 100);
            for (int k = 0; k < 10; k++) jacobians[0][k * 10 + k] = w_;
        }
        return true;
    }

private:
    double x0_[10], w_;
};
} // namespace
