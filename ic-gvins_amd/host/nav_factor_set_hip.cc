// The navigation factors on the HIP C ABI with the members resident on the device: see nav_factor_set.h.
#include <cstring>

#include "nav_factor_set.h"
#include "resident_call.h"

// A build of this layer on another implementation of the C ABI may not have the entry points: the references stay weak (null when absent)
// and set() reports it; the product library links libicgvins_hip.so, which defines them.
#pragma weak icg_nav_set
#pragma weak icg_nav_evaluate_resident
#pragma weak icg_nav_correct_resident

namespace icg {

const char *NavFactorSet::missingEntry() {
    if (&icg_nav_set == nullptr) return "icg_nav_set";
    if (&icg_nav_evaluate_resident == nullptr) return "icg_nav_evaluate_resident";
    if (&icg_nav_correct_resident == nullptr) return "icg_nav_correct_resident";
    return nullptr;
}

bool NavFactorSet::available() { return missingEntry() == nullptr; }

bool NavFactorSet::set(icg_ctx *ctx, const vector<const NavFactor *> &list, std::string *err) {
    ctx_ = nullptr;
    kind_.clear();
    if (!available()) {
        if (err) *err = std::string(missingEntry()) + " is not in this build";
        return false;
    }
    const size_t n = list.size();
    vector<int32_t> kind(n), aux_off(n + 1, 0), point_off(n, 0);
    vector<double> aux;
    size_t at = 0;
    for (size_t f = 0; f < n; f++) {
        kind[f]               = list[f]->navKind();
        const vector<double> a = list[f]->navAux();
        aux.insert(aux.end(), a.begin(), a.end());
        aux_off[f + 1] = (int32_t) aux.size();
        point_off[f]   = (int32_t) at;
        at += (size_t) list[f]->navWidth();
    }
    if (aux.empty()) aux.push_back(0.0); // (a set of error factors reads no constant; the entry still wants a pointer)
    if (!residentCall(nullptr, ctx, "icg_nav_set: no context", err, [&] { return icg_nav_set(ctx, (int) n, kind.data(), aux_off.data(), aux.data()); })) return false;
    kind_.swap(kind), point_off_.swap(point_off);
    points_.assign(at, 0.0);
    ctx_ = ctx;
    return true;
}

void NavFactorSet::pack(size_t f, const double *block) {
    const size_t end = f + 1 < point_off_.size() ? (size_t) point_off_[f + 1] : points_.size();
    memcpy(&points_[(size_t) point_off_[f]], block, sizeof(double) * (end - (size_t) point_off_[f]));
}

bool NavFactorSet::evaluateResident(bool want_jac, double *sq_norm, std::string *err) {
    return residentCall(missingEntry(), ctx_, "NavFactorSet::evaluateResident: no set", err,
                        [&] { return icg_nav_evaluate_resident(ctx_, points_.data(), point_off_.data(), want_jac ? 1 : 0, sq_norm); });
}

bool NavFactorSet::correct(const uint8_t *robust, const double *corr, std::string *err) {
    return residentCall(missingEntry(), ctx_, "NavFactorSet::correct: no set", err, [&] { return icg_nav_correct_resident(ctx_, robust, corr); });
}

} // namespace icg
