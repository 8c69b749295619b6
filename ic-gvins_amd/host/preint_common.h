// What the two preintegration classes share on the host: Preintegration (Normal / Earth, 15-wide error state, preintegration_hip.cc) and
// PreintegrationOdo (Odo / EarthOdo, 19-wide, preintegration_odo_hip.cc).
//   preint_math   the small-matrix helpers of the per-factor evaluate() bodies: one set of expressions, one order, for both classes
//   preintSqrtInformation<N> the square-root information of a covariance (both updateSqrtInformation members)
//   integrateBatchT / integrateStreamsT / evaluateBatchT   the batch drivers, written once against a per-class traits struct
#pragma once
#include <cmath>
#include <cstring>
#include <string>
#include <utility>
#include <vector>

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

// The 16 doubles every state row begins with: p3, q4 (x, y, z, w), v3, bg3, ba3.
inline void stateToArray16(const IntegrationState &s, double *a) {
    a[0] = s.p[0], a[1] = s.p[1], a[2] = s.p[2];
    a[3] = s.q.x, a[4] = s.q.y, a[5] = s.q.z, a[6] = s.q.w;
    for (int i = 0; i < 3; i++) {
        a[7 + i]  = s.v[i];
        a[10 + i] = s.bg[i];
        a[13 + i] = s.ba[i];
    }
}
inline void stateFromArray16(const double *a, IntegrationState &s) {
    s.p  = Vector3d(a[0], a[1], a[2]);
    s.q  = Quaterniond{a[3], a[4], a[5], a[6]};
    s.v  = Vector3d(a[7], a[8], a[9]);
    s.bg = Vector3d(a[10], a[11], a[12]);
    s.ba = Vector3d(a[13], a[14], a[15]);
}

// ---------------------------------------------------------------- the batch drivers ----------------------------------------------------------------
// T is the class's traits struct (a private nested struct, defined beside the class's members):
//   Class; N, IMU_ROW, STATE0, DELTA, PARAMS (row widths of the C entries), PLAIN / EARTH_V (variant numbers), PN_EVERY_VARIANT (pn_ takes
//   the rows of the call's buffer for every variant, not for the Earth one alone)
//   batchEntry / paramsEntry / evalEntry () -> the C entry or null when this build has none, *_name its name
//   imuRow, state0Row, paramsRow, deltaRow   what the entry reads of an object
//   dirty, store (the integration result, without the square-root information), finishHost (updateSqrtInformation) / finishDevice (S, ok)
template <class T> void stageIntervals(const vector<typename T::Class *> &todo, vector<int32_t> &offsets, vector<double> &imu, vector<double> &state0) {
    offsets.assign(1, 0);
    for (auto *p : todo) {
        for (const IMU &s : p->imuBuffer()) {
            double row[T::IMU_ROW];
            T::imuRow(s, row);
            imu.insert(imu.end(), row, row + T::IMU_ROW);
        }
        offsets.push_back((int32_t) (imu.size() / T::IMU_ROW));
        double a[T::STATE0];
        T::state0Row(*p, a);
        state0.insert(state0.end(), a, a + T::STATE0);
    }
}
// the rows of one call back into their objects; S = null: the square-root information is formed here
template <class T>
void storeIntervals(const vector<typename T::Class *> &todo, int variant, const vector<int32_t> &offsets, const vector<double> &cur,
                    const vector<double> &del, const vector<double> &jac, const vector<double> &cov, const vector<double> &dt,
                    const vector<double> &pn, const double *S, const int32_t *status) {
    constexpr size_t NN = (size_t) T::N * T::N;
    for (size_t k = 0; k < todo.size(); k++) {
        const int b = offsets[k], cnt = offsets[k + 1] - offsets[k];
        T::store(*todo[k], &cur[16 * k], &del[T::DELTA * k], &jac[NN * k], &cov[NN * k], dt[k],
                 T::PN_EVERY_VARIANT || variant == (int) T::EARTH_V ? &pn[4 * (size_t) b] : nullptr, cnt - 1);
        if (S)
            T::finishDevice(*todo[k], S + NN * k, status[k] == 0);
        else
            T::finishHost(*todo[k]);
    }
}

// one launch per (variant, parameter values): the *_batch entry takes one parameter vector per call, and every interval must be integrated
// with ITS OWN Earth rate (the one evaluate() uses).  Intervals of one estimator share their values in practice.
template <class T> bool integrateBatchT(icg_ctx *ctx, const vector<typename T::Class *> &list, std::string *err) {
    typedef typename T::Class C;
    constexpr size_t NN = (size_t) T::N * T::N;
    const auto entry    = T::batchEntry();
    if (!entry) {
        if (err) *err = std::string(T::batch_name) + " is not in this build";
        return false;
    }
    vector<C *> pending;
    for (auto *p : list)
        if (T::dirty(*p)) pending.push_back(p);
    while (!pending.empty()) {
        double params[T::PARAMS];
        T::paramsRow(*pending[0], params);
        const int variant = (int) pending[0]->variant();
        vector<C *> todo, rest;
        for (auto *p : pending) {
            double q[T::PARAMS];
            T::paramsRow(*p, q);
            ((int) p->variant() == variant && memcmp(q, params, sizeof q) == 0 ? todo : rest).push_back(p);
        }
        pending.swap(rest);
        vector<int32_t> offsets;
        vector<double> imu, state0;
        stageIntervals<T>(todo, offsets, imu, state0);
        const size_t n = todo.size(), total = imu.size() / T::IMU_ROW;
        vector<double> cur(16 * n), del(T::DELTA * n), jac(NN * n), cov(NN * n), dt(n), pn(4 * total);
        int rc = entry(ctx, variant, (int) n, offsets.data(), imu.data(), state0.data(), params, cur.data(), del.data(), jac.data(), cov.data(),
                       dt.data(), pn.data());
        if (rc != ICG_OK) {
            if (err) *err = icg_last_error(ctx);
            return false;
        }
        storeIntervals<T>(todo, variant, offsets, cur, del, jac, cov, dt, pn, nullptr, nullptr);
    }
    return true;
}

// one call per variant present: every interval brings its own parameter row (its own Earth rate), and the device forms the square-root
// information behind the integration, so updateSqrtInformation does not run
template <class T> bool integrateStreamsT(icg_ctx *ctx, const vector<typename T::Class *> &list, std::string *err) {
    typedef typename T::Class C;
    constexpr size_t NN = (size_t) T::N * T::N;
    const auto entry    = T::paramsEntry();
    if (!entry) {
        if (err) *err = std::string(T::params_name) + " is not in this build";
        return false;
    }
    for (int variant = (int) T::PLAIN; variant <= (int) T::EARTH_V; variant++) {
        vector<C *> todo;
        for (auto *p : list)
            if (T::dirty(*p) && (int) p->variant() == variant) todo.push_back(p);
        if (todo.empty()) continue;
        vector<int32_t> offsets;
        vector<double> imu, state0, params;
        stageIntervals<T>(todo, offsets, imu, state0);
        for (auto *p : todo) {
            double row[T::PARAMS];
            T::paramsRow(*p, row);
            params.insert(params.end(), row, row + T::PARAMS);
        }
        const size_t n = todo.size(), total = imu.size() / T::IMU_ROW;
        vector<double> cur(16 * n), del(T::DELTA * n), jac(NN * n), cov(NN * n), dt(n), pn(4 * total), S(NN * n);
        vector<int32_t> status(n);
        int rc = entry(ctx, variant, (int) n, offsets.data(), imu.data(), state0.data(), params.data(), cur.data(), del.data(), jac.data(),
                       cov.data(), dt.data(), pn.data(), S.data(), status.data());
        if (rc != ICG_OK) {
            if (err) *err = icg_last_error(ctx);
            return false;
        }
        storeIntervals<T>(todo, variant, offsets, cur, del, jac, cov, dt, pn, S.data(), status.data());
    }
    return true;
}

// P2 of every integrated factor of the list on the device, one call per variant present; zero rows and ok = 0 for the others
template <class T>
bool evaluateBatchT(icg_ctx *ctx, const vector<const typename T::Class *> &list, const double *points, double *residuals, double *jacobians,
                    vector<char> *ok, std::string *err, double *sqrt_info) {
    typedef typename T::Class C;
    constexpr size_t N = T::N, NN = N * N, POINT = C::NUM_POINT, NUM_JAC = C::NUM_JAC;
    const auto entry = T::evalEntry();
    if (!entry) {
        if (err) *err = std::string(T::eval_name) + " is not in this build";
        return false;
    }
    const size_t n_all = list.size();
    if (ok) ok->assign(n_all, 0);
    memset(residuals, 0, sizeof(double) * N * n_all);
    if (jacobians) memset(jacobians, 0, sizeof(double) * NUM_JAC * n_all);
    if (sqrt_info) memset(sqrt_info, 0, sizeof(double) * NN * n_all);
    for (int variant = (int) T::PLAIN; variant <= (int) T::EARTH_V; variant++) {
        vector<size_t> idx; // the integrated factors of this variant, list order
        for (size_t k = 0; k < n_all; k++)
            if ((int) list[k]->variant() == variant && !T::dirty(*list[k])) idx.push_back(k);
        if (idx.empty()) continue;
        const size_t n   = idx.size();
        const bool earth = variant == (int) T::EARTH_V;
        vector<double> del(T::DELTA * n), jac(NN * n), cov(NN * n), dt(n), env(4 * n), pts(POINT * n), pn;
        vector<int32_t> pn_off{0};
        for (size_t j = 0; j < n; j++) {
            const C &p = *list[idx[j]];
            T::deltaRow(p.deltaState(), &del[T::DELTA * j]);
            memcpy(&jac[NN * j], p.jacobian().data(), sizeof(double) * NN);
            memcpy(&cov[NN * j], p.covariance().data(), sizeof(double) * NN);
            dt[j]          = p.deltaTime();
            env[4 * j]     = p.gravity();
            env[4 * j + 1] = p.earthRate()[0], env[4 * j + 2] = p.earthRate()[1], env[4 * j + 3] = p.earthRate()[2];
            memcpy(&pts[POINT * j], points + POINT * idx[j], sizeof(double) * POINT);
            if (earth) {
                pn.insert(pn.end(), p.pnRows().begin(), p.pnRows().begin() + (long) (p.pnRows().size() / 4 * 4));
                pn_off.push_back((int32_t) (pn.size() / 4));
            }
        }
        vector<double> r(N * n), J(jacobians ? NUM_JAC * n : 0), S(sqrt_info ? NN * n : 0);
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
            if (jacobians) memcpy(jacobians + NUM_JAC * k, &J[NUM_JAC * j], sizeof(double) * NUM_JAC);
            if (sqrt_info) memcpy(sqrt_info + NN * k, &S[NN * j], sizeof(double) * NN);
            if (ok) (*ok)[k] = status[j] == 0 ? 1 : 0;
        }
    }
    return true;
}

} // namespace icg
