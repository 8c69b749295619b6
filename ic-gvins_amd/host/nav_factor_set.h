// The navigation factors of many windows resident on the device (icg_nav_set / icg_nav_evaluate_resident / icg_nav_correct_resident): the
// twin of PreintegrationOdoSet for the small factors of nav_factors.h.  set() once, pack() + evaluateResident() per evaluation point; at a
// linearization the members that carry a loss get the Ceres corrector where their results are (correct(): the three scalars per member are
// the host's, correctorScalars).  Residuals, Jacobians and squared norms are then the bits of the classes' Evaluate (and of
// ResidualBlockInfo::Evaluate for a corrected member), and only one squared norm per member comes back.  The C entries are referenced weakly:
// in a build of this layer on a C ABI without them available() is false, missingEntry() names the first that is absent and set() fails by
// that name.
#pragma once
#include <string>
#include <vector>

#include "nav_factors.h"

namespace icg {

class NavFactorSet {
public:
    static bool available();
    static const char *missingEntry(); // nullptr when available()
    // the objects must outlive the set's use; their constants are read here (a GnssFactor updated afterwards needs a new set())
    bool set(icg_ctx *ctx, const vector<const NavFactor *> &list, std::string *err = nullptr);
    // member f's parameter block to its place (any thread)
    void pack(size_t f, const double *block);
    bool evaluateResident(bool want_jac, double *sq_norm, std::string *err = nullptr);
    // after an evaluation with Jacobians, once: robust[f] != 0 marks a member, corr holds its sqrt_rho1, alpha_sq_norm, residual_scaling at 3 f
    bool correct(const uint8_t *robust, const double *corr, std::string *err = nullptr);
    int factors() const { return (int) kind_.size(); }

private:
    icg_ctx *ctx_{nullptr};
    vector<int32_t> kind_, point_off_;
    vector<double> points_;
};

} // namespace icg
