// TEST INFRASTRUCTURE ONLY — runs the REFERENCE's odometer preintegration (PreintegrationOdo / PreintegrationEarthOdo:
// preintegration/preintegration_{base,odo,earth_odo}.{h,cc}, preintegration_factor.h, common/earth.h, compiled unmodified from where
// they lie, as oracle/ref_build/ref_preint.cc does for the two 15-state variants) behind one C entry point.  Linear algebra comes from
// the Eigen-interface shim of oracle/ref_build/shim.  Built and run by make_preint_odo_golden.py only; no test needs it.
#include "common/earth.h"
#include "preintegration/preintegration_earth_odo.h"
#include "preintegration/preintegration_factor.h"
#include "preintegration/preintegration_odo.h"

#include "preintegration/preintegration_base.cc" // the reference sources themselves (single translation unit)
#include "preintegration/preintegration_earth_odo.cc"
#include "preintegration/preintegration_odo.cc"

namespace {
template <typename Base> struct ProbeT : public Base { // protected state made readable
    using Base::Base;
    const Eigen::MatrixXd &jac() const { return this->jacobian_; }
    const Eigen::MatrixXd &cov() const { return this->covariance_; }
};

IntegrationState make_state(const double *s17) { // p3 q4(xyzw) v3 bg3 ba3 sodo
    IntegrationState st;
    st.time = 0;
    st.p    = Vector3d(s17[0], s17[1], s17[2]);
    st.q    = Quaterniond(s17[6], s17[3], s17[4], s17[5]);
    st.v    = Vector3d(s17[7], s17[8], s17[9]);
    st.bg   = Vector3d(s17[10], s17[11], s17[12]);
    st.ba   = Vector3d(s17[13], s17[14], s17[15]);
    st.sodo = s17[16];
    return st;
}
void put_state(const IntegrationState &st, double *s16) {
    for (int k = 0; k < 3; k++) {
        s16[k]      = st.p[k];
        s16[7 + k]  = st.v[k];
        s16[10 + k] = st.bg[k];
        s16[13 + k] = st.ba[k];
    }
    s16[3] = st.q.x(), s16[4] = st.q.y(), s16[5] = st.q.z(), s16[6] = st.q.w();
}
// params16: gyr_arw, acc_vrw, gyr_bias_std, acc_bias_std, corr_time, gravity, odo_std[3], odo_srw, abv[3], lodo[3]
template <typename P>
std::shared_ptr<P> build_t(int n_imu, const double *imu9, const double *state17, const double *params16, const double *station) {
    auto par          = std::make_shared<IntegrationParameters>();
    par->station      = Vector3d(station[0], station[1], station[2]);
    par->gyr_arw      = params16[0];
    par->acc_vrw      = params16[1];
    par->gyr_bias_std = params16[2];
    par->acc_bias_std = params16[3];
    par->corr_time    = params16[4];
    par->gravity      = params16[5];
    par->odo_std      = Vector3d(params16[6], params16[7], params16[8]);
    par->odo_srw      = params16[9];
    par->abv          = Vector3d(params16[10], params16[11], params16[12]);
    par->lodo         = Vector3d(params16[13], params16[14], params16[15]);
    auto mk = [&](int k) {
        IMU m;
        m.time   = imu9[9 * k];
        m.dt     = imu9[9 * k + 1];
        m.dtheta = Vector3d(imu9[9 * k + 2], imu9[9 * k + 3], imu9[9 * k + 4]);
        m.dvel   = Vector3d(imu9[9 * k + 5], imu9[9 * k + 6], imu9[9 * k + 7]);
        m.odovel = imu9[9 * k + 8];
        return m;
    };
    auto pre = std::make_shared<P>(par, mk(0), make_state(state17));
    for (int k = 1; k < n_imu; k++) pre->addNewImu(mk(k));
    return pre;
}
template <typename P>
int run_t(int n_imu, const double *imu9, const double *state17, const double *params16, const double *station, double *cur16, double *delta20,
          double *jac361, double *cov361, double *delta_time, const double *point34, double *residuals19, double *jacobians646) {
    auto pre = build_t<P>(n_imu, imu9, state17, params16, station);
    put_state(pre->currentState(), cur16);
    const IntegrationState &d = pre->deltaState();
    put_state(d, delta20);
    delta20[16] = d.s[0], delta20[17] = d.s[1], delta20[18] = d.s[2], delta20[19] = d.sodo;
    for (int i = 0; i < 19; i++)
        for (int j = 0; j < 19; j++) {
            jac361[i * 19 + j] = pre->jac().get(i, j);
            cov361[i * 19 + j] = pre->cov().get(i, j);
        }
    *delta_time = pre->deltaTime();
    if (!point34) return 0;
    PreintegrationFactor f(pre);
    if (f.num_residuals() != 19) return 2;
    const double *p[4] = {point34, point34 + 7, point34 + 17, point34 + 24};
    double *J[4]       = {jacobians646, jacobians646 + 133, jacobians646 + 323, jacobians646 + 456};
    return f.Evaluate(p, residuals19, J) ? 0 : 1;
}
} // namespace

extern "C" {
// variant 2 = PreintegrationOdo, 3 = PreintegrationEarthOdo.  imu9: n x 9 (time, dt, dtheta[3], dvel[3], odovel); state17: p3 q4(xyzw) v3
// bg3 ba3 sodo; station: origin (lat, lon, h) of the local frame.  Outputs: cur16; delta20 = the 16, then s[3], then sodo; jac / cov 19 x 19
// row-major; iewn3 = Earth::iewn(station, p0) (the rate EarthOdo derives at resetState, :365); pn (variant 3, (n - 1) x 4): (dt, position)
// after every sample, read as currentState().p of the interval cut after that sample (pn_ itself is private); with point34 (pose0[7]
// mix0[10] pose1[7] mix1[10]) PreintegrationFactor::Evaluate: residuals 19, jacobians 646 = 19x7 | 19x10 | 19x7 | 19x10.
int ref_preint_odo(int variant, int n_imu, const double *imu9, const double *state17, const double *params16, const double *station,
                   double *cur16, double *delta20, double *jac361, double *cov361, double *delta_time, double *iewn3, double *pn,
                   const double *point34, double *residuals19, double *jacobians646) {
    Vector3d w = Earth::iewn(Vector3d(station[0], station[1], station[2]), Vector3d(state17[0], state17[1], state17[2]));
    iewn3[0] = w[0], iewn3[1] = w[1], iewn3[2] = w[2];
    if (variant == 2)
        return run_t<ProbeT<PreintegrationOdo>>(n_imu, imu9, state17, params16, station, cur16, delta20, jac361, cov361, delta_time, point34,
                                                residuals19, jacobians646);
    if (variant != 3) return -1;
    for (int k = 1; pn && k < n_imu; k++) {
        auto cut = build_t<ProbeT<PreintegrationEarthOdo>>(k + 1, imu9, state17, params16, station);
        pn[4 * (k - 1)] = imu9[9 * k + 1];
        for (int c = 0; c < 3; c++) pn[4 * (k - 1) + 1 + c] = cut->currentState().p[c];
    }
    return run_t<ProbeT<PreintegrationEarthOdo>>(n_imu, imu9, state17, params16, station, cur16, delta20, jac361, cov361, delta_time, point34,
                                                 residuals19, jacobians646);
}
}
