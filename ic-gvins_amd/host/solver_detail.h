// The core shared by WindowSolver (solver_hip.cc) and WindowSolverBatch (solver_batch_hip.cc), which differ only in how they schedule the
// device and host work of an LM step: the problem model of one window (parameter and residual blocks, the column layout of its reduced
// camera system, backup / step / restore of the parameters: Problem), the trust-region rule of one window (TrustRegion), the pose manifold
// step, the reduced-system solve and the accumulation of host-evaluated factors into a window's reduced system.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstring>
#include <memory>
#include <stdexcept>
#include <string>
#include <unordered_map>
#include <vector>

#include "factors.h"

namespace icg {
namespace solver_detail {

struct Options {
    int max_num_iterations{50};
    double initial_trust_region_radius{1e4}, max_trust_region_radius{1e16}, min_trust_region_radius{1e-32};
    double min_relative_decrease{1e-3}, min_lm_diagonal{1e-6}, max_lm_diagonal{1e32};
    double function_tolerance{1e-6}, gradient_tolerance{1e-10}, parameter_tolerance{1e-8};
};
struct Summary {
    double initial_cost{0}, final_cost{0};
    int num_successful_steps{0}, num_unsuccessful_steps{0};
    std::string termination;
    std::string BriefReport() const;
};

struct Block {
    double *values;
    int size, local;
    bool pose, constant;
    int column; // in the reduced (camera) system, -1 for constants and for the eliminated inverse-depth blocks
    bool landmark;
};
struct Residual {
    std::shared_ptr<ceres::CostFunction> cost;
    std::shared_ptr<ceres::LossFunction> loss;
    std::vector<double *> blocks;
    bool removed;
};

// in-place Cholesky solve of the symmetric positive definite n x n system A x = b (row-major, lower triangle used); dense_kernels.cc
bool choleskySolve(int n, std::vector<double> &A, std::vector<double> &b);
// T (nf x nf, upper triangle) += J^T J, g (nf) += J^T r for a dense row-major J (nr x nf); dense_kernels.cc
void accumulateJtJ(int nr, int nf, const double *J, const double *r, double *T, double *g);

// PoseParameterization::Plus (factors/pose_parameterization.h:34-50): p += dp, q = (q * rotvec2quaternion(dtheta)).normalized()
inline void posePlus(double *x, const double *delta) {
    for (int k = 0; k < 3; k++) x[k] += delta[k];
    const double rx = delta[3], ry = delta[4], rz = delta[5];
    const double angle = std::sqrt(rx * rx + ry * ry + rz * rz);
    double ax = rx, ay = ry, az = rz;
    if (angle > 0) ax /= angle, ay /= angle, az /= angle;
    const double sh = std::sin(0.5 * angle), ch = std::cos(0.5 * angle);
    const double bx = sh * ax, by = sh * ay, bz = sh * az, bw = ch;
    const double qx = x[3], qy = x[4], qz = x[5], qw = x[6];
    double nx = qw * bx + qx * bw + qy * bz - qz * by;
    double ny = qw * by + qy * bw + qz * bx - qx * bz;
    double nz = qw * bz + qz * bw + qx * by - qy * bx;
    double nw = qw * bw - qx * bx - qy * by - qz * bz;
    const double nn = std::sqrt(nx * nx + ny * ny + nz * nz + nw * nw);
    x[3] = nx / nn, x[4] = ny / nn, x[5] = nz / nn, x[6] = nw / nn;
}

// cost of one host residual block: 0.5 rho(|r|^2) (apply_loss) or 0.5 |r|^2
inline bool residualCost(const Residual &R, bool apply_loss_function, double *cost) {
    std::vector<double> r((size_t) R.cost->num_residuals());
    if (!R.cost->Evaluate(R.blocks.data(), r.data(), nullptr)) return false;
    double s = 0;
    for (double v : r) s += v * v;
    if (apply_loss_function && R.loss) {
        double rho[3];
        R.loss->Evaluate(s, rho);
        s = rho[0];
    }
    *cost = 0.5 * s;
    return true;
}

// The problem of one window: problem.AddParameterBlock / SetParameterBlockConstant / AddResidualBlock / EvaluateResidualBlock for the
// host-evaluated factors, the column layout of the reduced camera system and the step of its parameters.  `owner` prefixes the messages.
struct Problem {
    const char *owner;
    std::vector<Block> blocks;
    std::unordered_map<const double *, int> block_of;
    std::vector<Residual> residuals;
    std::vector<std::vector<double>> saved; // backup()

    explicit Problem(const char *owner_) : owner(owner_) {}
    [[noreturn]] void fail(const char *what) const { throw std::runtime_error(std::string(owner) + ": " + what); }

    // pose blocks are [p3, q4 xyzw], tangent size 6
    void addParameterBlock(double *values, int size, bool pose_manifold) {
        if (block_of.count(values)) return;
        if (pose_manifold && size != 7) fail("the pose manifold needs a block of size 7");
        block_of[values] = (int) blocks.size();
        blocks.push_back({values, size, pose_manifold ? 6 : size, pose_manifold, false, -1, false});
    }
    void setParameterBlockConstant(double *values) {
        auto it = block_of.find(values);
        if (it == block_of.end()) fail("unknown parameter block");
        blocks[(size_t) it->second].constant = true;
    }
    int addResidualBlock(std::shared_ptr<ceres::CostFunction> cost, std::shared_ptr<ceres::LossFunction> loss, const std::vector<double *> &ptrs) {
        const auto &sizes = cost->parameter_block_sizes();
        if (sizes.size() != ptrs.size()) fail("block count does not match the cost function");
        for (size_t k = 0; k < ptrs.size(); k++) {
            auto it = block_of.find(ptrs[k]);
            if (it == block_of.end()) fail("residual block uses an unknown parameter block");
            if (blocks[(size_t) it->second].size != sizes[k]) fail("parameter block size mismatch");
        }
        residuals.push_back({std::move(cost), std::move(loss), ptrs, false});
        return (int) residuals.size() - 1;
    }
    void removeResidualBlock(int id) { residuals.at((size_t) id).removed = true; }
    bool evaluateResidualBlock(int id, bool apply_loss_function, double *cost) const {
        return residualCost(residuals.at((size_t) id), apply_loss_function, cost);
    }

    // Column layout of the reduced system: the inverse-depth blocks of the visual factors (`landmarks`) are marked, they are eliminated
    // on the device; every other non-constant block gets the next columns, in the order the blocks were added.  -> P, or -1 and *error.
    int assignColumns(const std::vector<double *> &landmarks, std::string *error) {
        for (Block &b : blocks) b.landmark = false, b.column = -1;
        for (double *p : landmarks) {
            auto it = block_of.find(p);
            if (it == block_of.end()) return *error = "an inverse-depth block of a reprojection factor was not added to the solver", -1;
            if (blocks[(size_t) it->second].constant) return *error = "constant inverse-depth blocks are not supported", -1;
            blocks[(size_t) it->second].landmark = true;
        }
        for (const Residual &R : residuals)
            if (!R.removed)
                for (double *p : R.blocks)
                    if (blocks[(size_t) block_of.at(p)].landmark) return *error = "host factors on an eliminated inverse-depth block are not supported", -1;
        int P = 0;
        for (Block &b : blocks)
            if (!b.constant && !b.landmark) {
                b.column = P;
                P += b.local;
            }
        return P;
    }
    // the column of a block of a visual factor (after assignColumns)
    int column(const double *p) const {
        auto it = block_of.find(p);
        if (it == block_of.end()) fail("a block of a reprojection factor was not added to the solver");
        return blocks[(size_t) it->second].column;
    }

    void backup() {
        saved.resize(blocks.size());
        for (size_t k = 0; k < blocks.size(); k++) saved[k].assign(blocks[k].values, blocks[k].values + blocks[k].size);
    }
    void restore() {
        for (size_t k = 0; k < blocks.size(); k++) memcpy(blocks[k].values, saved[k].data(), sizeof(double) * (size_t) blocks[k].size);
    }
    // x = x [+] delta_c on the blocks with a column; the caller steps the eliminated inverse depths
    void applyCameraStep(const double *delta_c) {
        for (Block &b : blocks) {
            if (b.column < 0) continue;
            const double *d = &delta_c[(size_t) b.column];
            if (b.pose)
                posePlus(b.values, d);
            else
                for (int k = 0; k < b.size; k++) b.values[k] += d[k];
        }
    }
};

// The step rule of one window (solver_hip.h: the Ceres trust-region loop without Jacobi scaling).  The callers decide when to relinearize
// and when to re-damp; every function that can end the solve sets the summary's termination and returns true when it does.
struct TrustRegion {
    double radius, decrease_factor{2.0}, cost{0};
    Summary summary;
    explicit TrustRegion(const Options &o) : radius(o.initial_trust_region_radius) { summary.termination = "max_num_iterations"; }

    // dd (the size of diag) = the LM diagonal clamp(diag, min, max) / radius on the leading n columns, zero beyond
    void damp(const Options &o, const std::vector<double> &diag, int n, std::vector<double> &dd) const {
        dd.assign(diag.size(), 0.0);
        for (int k = 0; k < n; k++) dd[(size_t) k] = std::min(std::max(diag[(size_t) k], o.min_lm_diagonal), o.max_lm_diagonal) / radius;
    }
    // max norm of J^T r over the camera columns (the landmark part is bounded by it after elimination in practice and is not fetched)
    bool gradientConverged(const Options &o, const std::vector<double> &s) {
        double gmax = 0;
        for (double v : s) gmax = std::max(gmax, std::fabs(v));
        if (gmax < o.gradient_tolerance) {
            summary.termination = "gradient_tolerance";
            return true;
        }
        return false;
    }
    // an unsuccessful step (failed factorization, non-positive model decrease, rejected trial point)
    bool reject(const Options &o) {
        radius /= decrease_factor;
        decrease_factor *= 2.0;
        summary.num_unsuccessful_steps++;
        if (radius < o.min_trust_region_radius) {
            summary.termination = "min_trust_region_radius";
            return true;
        }
        return false;
    }
    // model decrease 0.5 (delta^T b + delta^T D delta) of the FULL damped system; s is the reduced right-hand side, and
    // delta^T b = delta_c^T s + sum b_l^2/(h_ll+d_l) (lm_terms[0], device), delta^T D delta = delta_c^T Dc delta_c + sum d_l delta_l^2 (lm_terms[1])
    static double modelDecrease(const double *lm_terms, const std::vector<double> &delta_c, const std::vector<double> &s, const std::vector<double> &dd) {
        double t0 = lm_terms[0], t1 = lm_terms[1];
        for (size_t k = 0; k < delta_c.size(); k++) t0 += delta_c[k] * s[k], t1 += dd[k] * delta_c[k] * delta_c[k];
        return 0.5 * (t0 + t1);
    }
    // |delta| <= tol (|x| + tol), x the free blocks of the problem before the step, delta the camera step and the window's n_l landmark steps
    bool parameterConverged(const Options &o, const Problem &p, const std::vector<double> &delta_c, const double *delta_l, size_t n_l) {
        double dn = 0, xn = 0;
        for (double v : delta_c) dn += v * v;
        for (size_t k = 0; k < n_l; k++) dn += delta_l[k] * delta_l[k];
        for (const Block &b : p.blocks)
            if (!b.constant)
                for (int k = 0; k < b.size; k++) xn += b.values[k] * b.values[k];
        if (std::sqrt(dn) <= o.parameter_tolerance * (std::sqrt(xn) + o.parameter_tolerance)) {
            summary.termination = "parameter_tolerance";
            return true;
        }
        return false;
    }
    // the cost at the trial point decides: *accepted (the radius grows) or rejected (p.restore(), then reject())
    bool trial(const Options &o, double new_cost, double model, Problem &p, bool *accepted) {
        const double rho = (cost - new_cost) / model;
        *accepted        = rho > o.min_relative_decrease;
        if (!*accepted) {
            p.restore();
            return reject(o);
        }
        const double change = cost - new_cost;
        cost                = new_cost;
        summary.num_successful_steps++;
        radius          = std::min(o.max_trust_region_radius, radius / std::max(1.0 / 3.0, 1.0 - std::pow(2.0 * rho - 1.0, 3)));
        decrease_factor = 2.0;
        if (std::fabs(change) < o.function_tolerance * cost) {
            summary.termination = "function_tolerance";
            return true;
        }
        return false;
    }
};

// the columns of a host factor inside the window's reduced system: the free local columns of its blocks, in block order (none: every block
// of the factor is constant)
inline void hostBlockColumns(const Problem &p, const Residual &R, std::vector<int> &cols) {
    cols.clear();
    for (size_t a = 0; a < R.blocks.size(); a++) {
        const Block &A = p.blocks[(size_t) p.block_of.at(R.blocks[a])];
        if (A.column < 0) continue;
        for (int x = 0; x < A.local; x++) cols.push_back(A.column + x);
    }
}

// One host factor, evaluated and gathered: *cost += 0.5 rho(|r|^2) from the raw residual, then res (nr, robust-corrected where the factor has a
// loss), cols (hostBlockColumns) and the dense row-major nr x nf Jacobian Jd of those columns.  Jd and res are written at Jd_at / res_at when
// given (nr and nf follow from the problem: the caller sized them), into the vectors otherwise.
// -> -1: the cost function failed; 0: no free column, nothing to accumulate (the cost is counted); 1: the block is there.
inline int gatherHostBlock(const Problem &p, const Residual &R, double *cost, std::vector<int> &cols, std::vector<double> &Jd, std::vector<double> &res,
                           double *Jd_at = nullptr, double *res_at = nullptr) {
    ResidualBlockInfo info(R.cost, nullptr, R.blocks, {});
    if (!info.Evaluate()) return -1;
    double sq = 0;
    for (double v : info.residuals()) sq += v * v;
    if (R.loss) { // cost from the raw residual, then the Ceres corrector (residual_block_info.h:59-87)
        double rho[3];
        R.loss->Evaluate(sq, rho);
        *cost += 0.5 * rho[0];
        ResidualBlockInfo corrected(R.cost, R.loss, R.blocks, {});
        if (!corrected.Evaluate()) return -1;
        info = corrected;
    } else {
        *cost += 0.5 * sq;
    }
    // the blocks are gathered into ONE dense row-major Jacobian (nr x n_free): see accumulateHostBlock
    const int nr      = R.cost->num_residuals();
    const auto &sizes = R.cost->parameter_block_sizes();
    hostBlockColumns(p, R, cols);
    const int nf = (int) cols.size();
    if (nf == 0) return 0;
    if (!Jd_at) Jd.resize((size_t) nr * nf), Jd_at = Jd.data();
    if (!res_at) res.resize((size_t) nr), res_at = res.data();
    int c0 = 0;
    for (size_t a = 0; a < R.blocks.size(); a++) {
        const Block &A = p.blocks[(size_t) p.block_of.at(R.blocks[a])];
        if (A.column < 0) continue;
        gatherJacobianColumns(nr, sizes[a], A.local, info.jacobians()[a].data(), nf, c0, Jd_at);
        c0 += A.local;
    }
    memcpy(res_at, info.residuals().data(), sizeof(double) * (size_t) nr);
    return 1;
}

// S += J^T J, s -= J^T r, diag += diag(J^T J) for one gathered block.  J^T J of the factor's free columns: the triple loop runs with the
// residual index outermost and a contiguous, independent inner index (vectorizable as written); every cell is the sum over k in ascending
// order from zero, as in a cell-by-cell inner product, and is then added to S once.  S is P x P with row stride P.
inline void accumulateHostBlock(int P, const std::vector<int> &cols, int nr, const double *Jd, const double *res, double *S, double *s, double *diag) {
    const int nf = (int) cols.size();
    thread_local std::vector<double> T;
    T.assign((size_t) nf * nf + nf, 0.0);
    double *g = T.data() + (size_t) nf * nf;
    accumulateJtJ(nr, nf, Jd, res, T.data(), g);
    for (int x = 0; x < nf; x++) {
        s[(size_t) cols[(size_t) x]] -= g[x];
        diag[(size_t) cols[(size_t) x]] += T[(size_t) x * nf + x];
        S[(size_t) cols[(size_t) x] * P + cols[(size_t) x]] += T[(size_t) x * nf + x];
        for (int y = x + 1; y < nf; y++) {
            const double v = T[(size_t) x * nf + y];
            S[(size_t) cols[(size_t) x] * P + cols[(size_t) y]] += v;
            S[(size_t) cols[(size_t) y] * P + cols[(size_t) x]] += v;
        }
    }
}

// host factors of one window: S += J^T J, s -= J^T r (robust-corrected), diag, cost += 0.5 rho(|r|^2); S == nullptr: cost only.
// S is P x P with row stride P.
inline bool hostFactors(const Problem &p, int P, double *S, double *s, double *diag, double *cost) {
    thread_local std::vector<double> Jd, res;
    thread_local std::vector<int> cols;
    for (const Residual &R : p.residuals) {
        if (R.removed) continue;
        if (!S) {
            double c;
            if (!residualCost(R, true, &c)) return false;
            *cost += c;
            continue;
        }
        const int got = gatherHostBlock(p, R, cost, cols, Jd, res);
        if (got < 0) return false;
        if (got == 0) continue;
        accumulateHostBlock(P, cols, R.cost->num_residuals(), Jd.data(), res.data(), S, s, diag);
    }
    return true;
}

} // namespace solver_detail
} // namespace icg
