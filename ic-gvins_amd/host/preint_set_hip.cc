// P2 on the HIP C ABI for a solve: the preintegration factors of many windows resident on the device, for both families (PreintegrationSet =
// PreintegrationSetT<Preintegration>, PreintegrationOdoSet = PreintegrationSetT<PreintegrationOdo>).  P::evaluate stays what the per-factor
// Ceres callback runs; the set is the same evaluation for MANY factors per call, for a driver that evaluates them at every LM point: the
// integration results cross the link once per solve, an evaluation ships the points and the correction quaternions in and one squared norm
// per factor out.
#include <cstring>

#include "preintegration_odo.h"
#include "resident_call.h"

// A build of this layer on another implementation of the C ABI may not have the entry points: the references stay weak (null when absent)
// and set() reports it; the product library links libicgvins_hip.so, which defines them.
#pragma weak icg_preint_set
#pragma weak icg_preint_evaluate_resident
#pragma weak icg_preint_odo_set
#pragma weak icg_preint_odo_evaluate_resident

namespace icg {

namespace {
// the family's two C entries (null when this build has none), their names and the class's name in messages
template <class P> struct SetEntries;
template <> struct SetEntries<Preintegration> {
    static constexpr const char *set_name = "icg_preint_set", *eval_name = "icg_preint_evaluate_resident", *cls = "PreintegrationSet";
    static auto set() { return &icg_preint_set; }
    static auto eval() { return &icg_preint_evaluate_resident; }
};
template <> struct SetEntries<PreintegrationOdo> {
    static constexpr const char *set_name = "icg_preint_odo_set", *eval_name = "icg_preint_odo_evaluate_resident", *cls = "PreintegrationOdoSet";
    static auto set() { return &icg_preint_odo_set; }
    static auto eval() { return &icg_preint_odo_evaluate_resident; }
};
} // namespace

template <class P> const char *PreintegrationSetT<P>::missingEntry() {
    typedef SetEntries<P> E;
    if (E::set() == nullptr) return E::set_name;
    if (E::eval() == nullptr) return E::eval_name;
    return nullptr;
}

template <class P> bool PreintegrationSetT<P>::available() { return missingEntry() == nullptr; }

template <class P> bool PreintegrationSetT<P>::set(icg_ctx *ctx, const vector<const P *> &list, std::string *err) {
    typedef SetEntries<P> E;
    constexpr size_t NN = (size_t) P::NUM_STATE * P::NUM_STATE, DELTA = P::NUM_DELTA;
    ctx_ = nullptr;
    list_.clear();
    if (!available()) {
        if (err) *err = std::string(missingEntry()) + " is not in this build";
        return false;
    }
    const size_t n = list.size();
    vector<int32_t> variant(n), pn_off(n + 1, 0);
    vector<double> del(DELTA * n), jac(NN * n), S(NN * n), dt(n), env(4 * n), qnn(4 * n), pn;
    bool any_earth = false;
    for (size_t f = 0; f < n; f++) {
        const P &p = *list[f];
        if (!p.ready()) {
            if (err) *err = std::string(E::cls) + "::set: factor " + std::to_string(f) + " is not integrated or its covariance is singular";
            return false;
        }
        variant[f] = (int32_t) p.variant();
        any_earth |= p.variant() == P::EARTH_VARIANT;
        P::deltaRow(p.deltaState(), &del[DELTA * f]);
        memcpy(&jac[NN * f], p.jacobian().data(), sizeof(double) * NN);
        memcpy(&S[NN * f], p.sqrtInformation().data(), sizeof(double) * NN);
        dt[f]      = p.deltaTime();
        env[4 * f] = p.gravity();
        for (int i = 0; i < 3; i++) env[4 * f + 1 + i] = p.earthRate()[i];
        p.earthRateQuaternion(&qnn[4 * f]);
        if (p.variant() == P::EARTH_VARIANT) pn.insert(pn.end(), p.pnRows().begin(), p.pnRows().begin() + (long) (p.pnRows().size() / 4 * 4));
        pn_off[f + 1] = (int32_t) (pn.size() / 4);
    }
    if (!residentCall(nullptr, ctx, std::string(E::set_name) + ": no context", err, [&] {
            return E::set()(ctx, (int) n, variant.data(), del.data(), jac.data(), S.data(), dt.data(), env.data(), qnn.data(), any_earth ? pn_off.data() : nullptr,
                            pn.empty() ? nullptr : pn.data());
        }))
        return false;
    list_ = list;
    points_.assign((size_t) P::NUM_POINT * n, 0.0), q_corr_.assign(4 * n, 0.0);
    ctx_ = ctx;
    return true;
}

template <class P> void PreintegrationSetT<P>::pack(size_t f, const double *const *parameters) {
    constexpr int MIX = P::NUM_MIX;
    double *pt        = &points_[(size_t) P::NUM_POINT * f];
    memcpy(pt, parameters[0], sizeof(double) * 7), memcpy(pt + 7, parameters[1], sizeof(double) * MIX);
    memcpy(pt + 7 + MIX, parameters[2], sizeof(double) * 7), memcpy(pt + 14 + MIX, parameters[3], sizeof(double) * MIX);
    list_[f]->correctionQuaternion(parameters[1], &q_corr_[4 * f]);
}

template <class P> bool PreintegrationSetT<P>::evaluateResident(bool want_jac, double *sq_norm, std::string *err) {
    typedef SetEntries<P> E;
    return residentCall(missingEntry(), ctx_, std::string(E::cls) + "::evaluateResident: no set", err,
                        [&] { return E::eval()(ctx_, points_.data(), q_corr_.data(), want_jac ? 1 : 0, sq_norm); });
}

template class PreintegrationSetT<Preintegration>;
template class PreintegrationSetT<PreintegrationOdo>;

} // namespace icg
