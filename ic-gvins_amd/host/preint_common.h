// What PreintegrationT (preintegration_hip.cc) rests on that is no member of it:
//   preint_math   the small-matrix helpers of evaluate(): one set of expressions, one order
//   preintSqrtInformation<N> the square-root information of a covariance (updateSqrtInformation)
#pragma once
#include <cmath>
#include <cstring>
#include <utility>

#include "preintegration.h"

namespace icg {

namespace preint_math {
struct V3 {
    double x, y, z;
};
struct Q4 {
    double x, y, z, w;
};
struct M3 {
    double m[3][3];
};
inline V3 operator+(V3 a, V3 b) { return {a.x + b.x, a.y + b.y, a.z + b.z}; }
inline V3 operator-(V3 a, V3 b) { return {a.x - b.x, a.y - b.y, a.z - b.z}; }
inline V3 operator*(V3 a, double s) { return {a.x * s, a.y * s, a.z * s}; }
inline V3 operator*(double s, V3 a) { return {a.x * s, a.y * s, a.z * s}; }
inline V3 operator-(V3 a) { return {-a.x, -a.y, -a.z}; }
inline V3 cross(V3 a, V3 b) { return {a.y * b.z - a.z * b.y, a.z * b.x - a.x * b.z, a.x * b.y - a.y * b.x}; }
inline Q4 qinv(Q4 q) {
    double n2 = q.x * q.x + q.y * q.y + q.z * q.z + q.w * q.w;
    return {-q.x / n2, -q.y / n2, -q.z / n2, q.w / n2};
}
inline Q4 qmul(Q4 a, Q4 b) {
    return {a.w * b.x + a.x * b.w + a.y * b.z - a.z * b.y, a.w * b.y + a.y * b.w + a.z * b.x - a.x * b.z,
            a.w * b.z + a.z * b.w + a.x * b.y - a.y * b.x, a.w * b.w - a.x * b.x - a.y * b.y - a.z * b.z};
}
inline V3 qrot(Q4 q, V3 v) {
    V3 qv{q.x, q.y, q.z};
    V3 uv = cross(qv, v);
    uv    = uv + uv;
    return v + q.w * uv + cross(qv, uv);
}
inline M3 qmat(Q4 q) {
    double tx = 2 * q.x, ty = 2 * q.y, tz = 2 * q.z, twx = tx * q.w, twy = ty * q.w, twz = tz * q.w;
    double txx = tx * q.x, txy = ty * q.x, txz = tz * q.x, tyy = ty * q.y, tyz = tz * q.y, tzz = tz * q.z;
    return M3{{{1 - (tyy + tzz), txy - twz, txz + twy}, {txy + twz, 1 - (txx + tzz), tyz - twx}, {txz - twy, tyz + twx, 1 - (txx + tyy)}}};
}
inline Q4 rotvec2quat(V3 rv) {
    double angle = std::sqrt(rv.x * rv.x + rv.y * rv.y + rv.z * rv.z);
    V3 axis      = rv;
    if (angle > 0) axis = rv * (1.0 / angle);
    double s = std::sin(0.5 * angle), c = std::cos(0.5 * angle);
    return {s * axis.x, s * axis.y, s * axis.z, c};
}
inline M3 skew(V3 v) { return M3{{{0, -v.z, v.y}, {v.z, 0, -v.x}, {-v.y, v.x, 0}}}; }
inline M3 eye() { return M3{{{1, 0, 0}, {0, 1, 0}, {0, 0, 1}}}; }
inline M3 scale(const M3 &a, double s) {
    M3 r;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) r.m[i][j] = a.m[i][j] * s;
    return r;
}
inline M3 add(const M3 &a, const M3 &b) {
    M3 r;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) r.m[i][j] = a.m[i][j] + b.m[i][j];
    return r;
}
inline M3 mul(const M3 &a, const M3 &b) {
    M3 r;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) r.m[i][j] = a.m[i][0] * b.m[0][j] + a.m[i][1] * b.m[1][j] + a.m[i][2] * b.m[2][j];
    return r;
}
inline V3 mv(const M3 &a, V3 v) {
    return {a.m[0][0] * v.x + a.m[0][1] * v.y + a.m[0][2] * v.z, a.m[1][0] * v.x + a.m[1][1] * v.y + a.m[1][2] * v.z,
            a.m[2][0] * v.x + a.m[2][1] * v.y + a.m[2][2] * v.z};
}
inline M3 qleft_br(Q4 q) { return add(scale(eye(), q.w), skew({q.x, q.y, q.z})); }
inline M3 qright_br(Q4 q) { return add(scale(eye(), q.w), scale(skew({q.x, q.y, q.z}), -1.0)); }
inline M3 qleft_qright_br(Q4 a, Q4 b) { // bottom-right 3x3 of quaternionleft(a) * quaternionright(b), rotation.h:103-119
    double L[4][4], R[4][4];
    auto fill = [](double M[4][4], Q4 q, double sgn) {
        M[0][0] = q.w;
        M[0][1] = -q.x, M[0][2] = -q.y, M[0][3] = -q.z;
        M[1][0] = q.x, M[2][0] = q.y, M[3][0] = q.z;
        M3 s = skew({q.x, q.y, q.z});
        for (int i = 0; i < 3; i++)
            for (int j = 0; j < 3; j++) M[1 + i][1 + j] = (i == j ? q.w : 0.0) + sgn * s.m[i][j];
    };
    fill(L, a, 1.0);
    fill(R, b, -1.0);
    M3 out;
    for (int i = 0; i < 3; i++)
        for (int j = 0; j < 3; j++) {
            double s = 0;
            for (int k = 0; k < 4; k++) s += L[1 + i][k] * R[k][1 + j];
            out.m[i][j] = s;
        }
    return out;
}
} // namespace preint_math

// sqrt_information = LLT(cov^-1).matrixL().transpose()  (normal :39-40, earth :39-40, odo :42-43, earth_odo :43-44).  The reference forms it
// inside every evaluate(); it only depends on the covariance, so it is formed once when an integration result arrives (same arithmetic, same
// value): Gauss-Jordan with partial pivoting on the N x 2N augmented matrix, mirrored lower triangle, column Cholesky (the device's
// square-root kernels repeat this arithmetic in this order).  cov, S: N x N row-major; false, and S untouched, for a singular covariance.
template <int N> bool preintSqrtInformation(const double *cov_in, double *S) {
    typedef double MN[N][N];
    MN cov, inv, L;
    memcpy(cov, cov_in, sizeof cov);
    double w[N][2 * N];
    for (int i = 0; i < N; i++)
        for (int j = 0; j < N; j++) {
            w[i][j]     = cov[i][j];
            w[i][N + j] = (i == j) ? 1.0 : 0.0;
        }
    for (int c = 0; c < N; c++) {
        int piv = c;
        for (int r = c + 1; r < N; r++)
            if (std::fabs(w[r][c]) > std::fabs(w[piv][c])) piv = r;
        if (w[piv][c] == 0.0) return false;
        if (piv != c)
            for (int j = 0; j < 2 * N; j++) std::swap(w[c][j], w[piv][j]);
        double d = w[c][c];
        for (int j = 0; j < 2 * N; j++) w[c][j] /= d;
        for (int r = 0; r < N; r++)
            if (r != c) {
                double f = w[r][c];
                if (f != 0.0)
                    for (int j = 0; j < 2 * N; j++) w[r][j] -= f * w[c][j];
            }
    }
    for (int i = 0; i < N; i++)
        for (int j = 0; j < N; j++) inv[i][j] = w[i][N + j];
    for (int i = 0; i < N; i++)
        for (int j = 0; j < i; j++) inv[j][i] = inv[i][j];
    memset(L, 0, sizeof L);
    for (int j = 0; j < N; j++) {
        double s = inv[j][j];
        for (int k = 0; k < j; k++) s -= L[j][k] * L[j][k];
        L[j][j] = std::sqrt(s);
        for (int i = j + 1; i < N; i++) {
            double t = inv[i][j];
            for (int k = 0; k < j; k++) t -= L[i][k] * L[j][k];
            L[i][j] = t / L[j][j];
        }
    }
    for (int i = 0; i < N; i++)
        for (int j = 0; j < N; j++) S[(size_t) i * N + j] = L[j][i];
    return true;
}

} // namespace icg
