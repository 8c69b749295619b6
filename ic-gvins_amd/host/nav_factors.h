// The small navigation factors of the GVINS window (tens of blocks per solve):
//   GnssFactor          reference factors/gnss_factor.h:33-80                  3 x 7
//   ImuErrorFactor      reference preintegration/imu_error_factor.h:30-95      6 x 9 (Normal / Earth), 7 x 10 (Odo / EarthOdo)
//   ImuPosePriorFactor  reference preintegration/imu_pose_prior_factor.h:30-72 6 x 7
//   ImuMixPriorFactor   reference preintegration/imu_mix_prior_factor.h:30-80  9 x 9 (Normal / Earth), 10 x 10 (Odo / EarthOdo)
// Same block sizes, residual order and Jacobian layout (row-major, global size) as the reference; the 9-wide forms are pinned against the
// reference's own headers (oracle/_ref/libref_nav.so, tests/golden/nav_ref_golden.npz).  All four are NavFactors: what a solver needs to
// evaluate them somewhere else (csrc/nav.hip restates every Evaluate below operation for operation).
#pragma once
#include <cstring>
#include <vector>

#include "earth.h"
#include "factors.h"

namespace icg {

// What the four classes share besides ceres::CostFunction (a solver finds it with dynamic_cast): the kind, the shape and the constants.
class NavFactor {
public:
    enum Kind { KIND_GNSS = 0, KIND_ERROR = 1, KIND_POSE_PRIOR = 2, KIND_MIX_PRIOR = 3, KIND_ERROR_ODO = 4, KIND_MIX_PRIOR_ODO = 5 };
    virtual ~NavFactor() = default;
    int navKind() const { return kind_; }
    int navResiduals() const { return nr_; }
    int navWidth() const { return width_; } // size of the one parameter block
    // the constants, flat: GNSS = blh3, std3, lever3; pose prior = pose7, std6; mix prior = mix, std (width each); error = none
    virtual std::vector<double> navAux() const = 0;

protected:
    NavFactor(int kind, int nr, int width) : kind_(kind), nr_(nr), width_(width) {}

private:
    int kind_, nr_, width_;
};

// the preintegration option of the reference (Preintegration::PreintegrationOptions): 0 Normal, 1 Earth, 2 Odo, 3 EarthOdo
inline bool navVariantHasOdo(int variant) { return variant == 2 || variant == 3; }

struct GNSS { // common/types.h:35-43
    double time{0};
    Vector3d blh, std;
    bool isyawvalid{false};
    double yaw{0};
};

class GnssFactor : public ceres::SizedCostFunction<3, 7>, public NavFactor {
public:
    GnssFactor(GNSS gnss, Vector3d lever) : NavFactor(KIND_GNSS, 3, 7), gnss_(gnss), lever_(lever) {}
    void updateGnssState(const GNSS &gnss) { gnss_ = gnss; }
    std::vector<double> navAux() const override {
        return {gnss_.blh[0], gnss_.blh[1], gnss_.blh[2], gnss_.std[0], gnss_.std[1], gnss_.std[2], lever_[0], lever_[1], lever_[2]};
    }
    bool Evaluate(const double *const *parameters, double *residuals, double **jacobians) const override {
        const double *x = parameters[0];
        Matrix3d R      = Rotation::quaternion2matrix(Quaterniond{x[3], x[4], x[5], x[6]});
        Vector3d rl     = R * lever_;
        for (int k = 0; k < 3; k++) residuals[k] = (1.0 / gnss_.std[k]) * (x[k] + rl[k] - gnss_.blh[k]);
        if (jacobians && jacobians[0]) {
            double *J = jacobians[0];
            memset(J, 0, sizeof(double) * 21);
            const double S[3][3] = {{0, -lever_[2], lever_[1]}, {lever_[2], 0, -lever_[0]}, {-lever_[1], lever_[0], 0}};
            for (int i = 0; i < 3; i++) {
                const double w = 1.0 / gnss_.std[i];
                J[i * 7 + i]   = w * 1.0;
                for (int j = 0; j < 3; j++) J[i * 7 + 3 + j] = w * -(R(i, 0) * S[0][j] + R(i, 1) * S[1][j] + R(i, 2) * S[2][j]);
            }
        }
        return true;
    }

private:
    GNSS gnss_;
    Vector3d lever_;
};

class ImuErrorFactor : public ceres::CostFunction, public NavFactor {
public:
    explicit ImuErrorFactor(int variant = 0)
        : NavFactor(navVariantHasOdo(variant) ? KIND_ERROR_ODO : KIND_ERROR, navVariantHasOdo(variant) ? 7 : 6, navVariantHasOdo(variant) ? 10 : 9) {
        *mutable_parameter_block_sizes() = std::vector<int32_t>{navWidth()};
        set_num_residuals(navResiduals());
    }
    std::vector<double> navAux() const override { return {}; }
    bool Evaluate(const double *const *parameters, double *residuals, double **jacobians) const override {
        const int nc = navWidth();
        for (int k = 0; k < 3; k++) {
            residuals[k + 0] = parameters[0][k + 3] / IMU_GRY_BIAS_STD;
            residuals[k + 3] = parameters[0][k + 6] / IMU_ACC_BIAS_STD;
        }
        if (nc == 10) residuals[6] = parameters[0][9] / ODO_SCALE_STD;
        if (jacobians && jacobians[0]) {
            memset(jacobians[0], 0, sizeof(double) * (size_t) (navResiduals() * nc));
            for (int k = 0; k < 3; k++) {
                jacobians[0][(k + 0) * nc + k + 3] = 1.0 / IMU_GRY_BIAS_STD;
                jacobians[0][(k + 3) * nc + k + 6] = 1.0 / IMU_ACC_BIAS_STD;
            }
            if (nc == 10) jacobians[0][6 * nc + 9] = 1.0 / ODO_SCALE_STD;
        }
        return true;
    }

    static constexpr double IMU_GRY_BIAS_STD = 7200 / 3600.0 * M_PI / 180.0; // 7200 deg / hr
    static constexpr double IMU_ACC_BIAS_STD = 2.0e4 * 1.0e-5;               // 20000 mGal
    static constexpr double ODO_SCALE_STD    = 2.0e4 * 1.0e-6;               // 0.02
};

class ImuPosePriorFactor : public ceres::SizedCostFunction<6, 7>, public NavFactor {
public:
    ImuPosePriorFactor(const double *pose, const double *std) : NavFactor(KIND_POSE_PRIOR, 6, 7) {
        memcpy(pose_, pose, sizeof(double) * 7);
        memcpy(std_, std, sizeof(double) * 6);
        for (int k = 0; k < 6; k++) w_[k] = 1.0 / std[k];
    }
    std::vector<double> navAux() const override {
        std::vector<double> a(pose_, pose_ + 7);
        a.insert(a.end(), std_, std_ + 6);
        return a;
    }
    bool Evaluate(const double *const *parameters, double *residuals, double **jacobians) const override {
        const double *x = parameters[0];
        for (int k = 0; k < 3; k++) residuals[k] = (x[k] - pose_[k]);
        // d = q^-1 * q_p (Eigen inverse(): conjugate / squared norm)
        const double n2 = x[3] * x[3] + x[4] * x[4] + x[5] * x[5] + x[6] * x[6];
        const double ax = -x[3] / n2, ay = -x[4] / n2, az = -x[5] / n2, aw = x[6] / n2;
        const double bx = pose_[3], by = pose_[4], bz = pose_[5], bw = pose_[6];
        const double dx = aw * bx + ax * bw + ay * bz - az * by;
        const double dy = aw * by + ay * bw + az * bx - ax * bz;
        const double dz = aw * bz + az * bw + ax * by - ay * bx;
        const double dw = aw * bw - ax * bx - ay * by - az * bz;
        residuals[3] = 2 * dx, residuals[4] = 2 * dy, residuals[5] = 2 * dz;
        for (int k = 0; k < 6; k++) residuals[k] = w_[k] * residuals[k];
        if (jacobians && jacobians[0]) {
            double *J = jacobians[0];
            memset(J, 0, sizeof(double) * 42);
            for (int k = 0; k < 3; k++) J[k * 7 + k] = w_[k] * 1.0;
            // -quaternionright(d).bottomRightCorner<3,3>() = -(dw I - skew(d.vec))
            const double B[3][3] = {{dw, dz, -dy}, {-dz, dw, dx}, {dy, -dx, dw}};
            for (int i = 0; i < 3; i++)
                for (int j = 0; j < 3; j++) J[(3 + i) * 7 + 3 + j] = w_[3 + i] * -B[i][j];
        }
        return true;
    }

private:
    double pose_[7], std_[6], w_[6];
};

class ImuMixPriorFactor : public ceres::CostFunction, public NavFactor {
public:
    // mix and mix_std hold 9 values, 10 with an odometer variant
    ImuMixPriorFactor(const double *mix, const double *mix_std, int variant = 0)
        : NavFactor(navVariantHasOdo(variant) ? KIND_MIX_PRIOR_ODO : KIND_MIX_PRIOR, navVariantHasOdo(variant) ? 10 : 9, navVariantHasOdo(variant) ? 10 : 9) {
        *mutable_parameter_block_sizes() = std::vector<int32_t>{navWidth()};
        set_num_residuals(navResiduals());
        memcpy(mix_, mix, sizeof(double) * (size_t) navWidth());
        memcpy(mix_std_, mix_std, sizeof(double) * (size_t) navWidth());
    }
    std::vector<double> navAux() const override {
        std::vector<double> a(mix_, mix_ + navWidth());
        a.insert(a.end(), mix_std_, mix_std_ + navWidth());
        return a;
    }
    bool Evaluate(const double *const *parameters, double *residuals, double **jacobians) const override {
        const int n = navWidth();
        for (int k = 0; k < n; k++) residuals[k] = (parameters[0][k] - mix_[k]) / mix_std_[k];
        if (jacobians && jacobians[0]) {
            memset(jacobians[0], 0, sizeof(double) * (size_t) (n * n));
            for (int k = 0; k < n; k++) jacobians[0][k * n + k] = 1.0 / mix_std_[k];
        }
        return true;
    }

private:
    double mix_[10], mix_std_[10];
};

} // namespace icg
