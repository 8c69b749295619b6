// P2 of the odometer variants on the HIP C ABI with the factors resident on the device: the 19-state twin of preint_set_hip.cc.
// PreintegrationOdo::evaluate stays what the per-factor Ceres callback runs; PreintegrationOdoSet is the same evaluation for MANY factors per
// call: the integration results cross the link once, an evaluation ships the 34-wide points and the correction quaternions in and one
// squared norm per factor out.
#include <cstring>

#include "preintegration_odo.h"

// A build of this layer on another implementation of the C ABI may not have the entry points: the references stay weak (null when absent)
// and set() reports it; the product library links libicgvins_hip.so, which defines them.
#pragma weak icg_preint_odo_set
#pragma weak icg_preint_odo_evaluate_resident

namespace icg {

const char *PreintegrationOdoSet::missingEntry() {
    if (&icg_preint_odo_set == nullptr) return "icg_preint_odo_set";
    if (&icg_preint_odo_evaluate_resident == nullptr) return "icg_preint_odo_evaluate_resident";
    return nullptr;
}

bool PreintegrationOdoSet::available() { return missingEntry() == nullptr; }

bool PreintegrationOdoSet::set(icg_ctx *ctx, const vector<const PreintegrationOdo *> &list, std::string *err) {
    ctx_ = nullptr;
    list_.clear();
    if (!available()) {
        if (err) *err = std::string(missingEntry()) + " is not in this build";
        return false;
    }
    constexpr size_t NN = (size_t) PreintegrationOdo::NUM_STATE * PreintegrationOdo::NUM_STATE;
    const size_t n      = list.size();
    vector<int32_t> variant(n), pn_off(n + 1, 0);
    vector<double> del(20 * n), jac(NN * n), S(NN * n), dt(n), env(4 * n), qnn(4 * n), pn;
    bool any_earth = false;
    for (size_t f = 0; f < n; f++) {
        const PreintegrationOdo &p = *list[f];
        if (!p.ready()) {
            if (err) *err = "PreintegrationOdoSet::set: factor " + std::to_string(f) + " is not integrated or its covariance is singular";
            return false;
        }
        variant[f] = (int32_t) p.variant();
        any_earth |= p.variant() == PreintegrationOdo::EARTH_ODO;
        const IntegrationState &d = p.deltaState();
        double *a                 = &del[20 * f];
        a[0] = d.p[0], a[1] = d.p[1], a[2] = d.p[2], a[3] = d.q.x, a[4] = d.q.y, a[5] = d.q.z, a[6] = d.q.w;
        for (int i = 0; i < 3; i++) a[7 + i] = d.v[i], a[10 + i] = d.bg[i], a[13 + i] = d.ba[i], a[16 + i] = d.s[i];
        a[19] = d.sodo;
        memcpy(&jac[NN * f], p.jacobian().data(), sizeof(double) * NN);
        memcpy(&S[NN * f], p.sqrtInformation().data(), sizeof(double) * NN);
        dt[f]      = p.deltaTime();
        env[4 * f] = p.gravity();
        for (int i = 0; i < 3; i++) env[4 * f + 1 + i] = p.earthRate()[i];
        p.earthRateQuaternion(&qnn[4 * f]);
        if (p.variant() == PreintegrationOdo::EARTH_ODO) pn.insert(pn.end(), p.pnRows().begin(), p.pnRows().begin() + (long) (p.pnRows().size() / 4 * 4));
        pn_off[f + 1] = (int32_t) (pn.size() / 4);
    }
    if (icg_preint_odo_set(ctx, (int) n, variant.data(), del.data(), jac.data(), S.data(), dt.data(), env.data(), qnn.data(),
                           any_earth ? pn_off.data() : nullptr, pn.empty() ? nullptr : pn.data()) != ICG_OK) {
        if (err) *err = ctx ? icg_last_error(ctx) : "icg_preint_odo_set: no context";
        return false;
    }
    list_ = list;
    points_.assign(34 * n, 0.0), q_corr_.assign(4 * n, 0.0);
    ctx_ = ctx;
    return true;
}

void PreintegrationOdoSet::pack(size_t f, const double *const *parameters) {
    double *pt = &points_[34 * f];
    memcpy(pt, parameters[0], sizeof(double) * 7), memcpy(pt + 7, parameters[1], sizeof(double) * 10);
    memcpy(pt + 17, parameters[2], sizeof(double) * 7), memcpy(pt + 24, parameters[3], sizeof(double) * 10);
    list_[f]->correctionQuaternion(parameters[1], &q_corr_[4 * f]);
}

bool PreintegrationOdoSet::evaluateResident(bool want_jac, double *sq_norm, std::string *err) {
    if (!available() || !ctx_) {
        if (err) *err = !available() ? std::string(missingEntry()) + " is not in this build" : "PreintegrationOdoSet::evaluateResident: no set";
        return false;
    }
    if (icg_preint_odo_evaluate_resident(ctx_, points_.data(), q_corr_.data(), want_jac ? 1 : 0, sq_norm) != ICG_OK) {
        if (err) *err = icg_last_error(ctx_);
        return false;
    }
    return true;
}

} // namespace icg
