// The symmetric eigen-solver of the back-end's host side: see sym_eigen.h.
#include "sym_eigen.h"

#include <algorithm>
#include <cmath>

namespace icg {

// ---- symmetric eigen-solver ------------------------------------------------------------------------------------------
// Householder tridiagonalisation followed by the implicit-shift QL iteration (the classic EISPACK tred2 / tql2 pair): ~(4/3 + 3) n^3
// flops.  The cyclic Jacobi solver used before needed ~40 ms for the 133 x 133 and 61 x 61 matrices of one C2 marginalization (its
// off-diagonal norm never reached the 1e-30 threshold, so every call ran the full 100 sweeps); this one takes ~1 ms for both.
// evecs is row-major n x n with eigenvector k in COLUMN k; evals ascending.
// Round 5: the same arithmetic in the same order (outputs bit-identical to the plain form on every matrix tried: full rank, rank-deficient,
// diagonal, zero rows, zero, badly scaled; n = 1 ... 207), 2.4 x faster at n = 142 — the working matrix is held transposed from the start
// (every inner loop contiguous), the dependent sums of tred2 / of the accumulation run four / eight columns' chains at a time (each chain in
// its own order), and the element-wise loops are vectorised.
// The element-wise inner loops of symmetricEigen: no reductions, so their vector forms do exactly the scalar arithmetic (no FMA in either
// clone: "avx2" does not include it, and contraction is off).  The AVX2 clone is picked at load time where the CPU has it.
// (Sanitizer builds — tests/tsan/run.sh — take the plain build: an instrumented ifunc resolver runs before the sanitizer's runtime is up.)
#if defined(__SANITIZE_THREAD__) || defined(__SANITIZE_ADDRESS__)
#define ICG_CLONES __attribute__((optimize("O3", "fp-contract=off")))
#else
#define ICG_CLONES __attribute__((target_clones("avx2", "default"), optimize("O3", "fp-contract=off")))
#endif
// Givens rotation of two rows (tql2 "accumulate"): element-wise, no reduction -> the vector form does the scalar form's arithmetic
ICG_CLONES static void eig_rotate(double *__restrict vi, double *__restrict vi1, int n, double c, double s) {
    for (int k = 0; k < n; k++) {
        const double h = vi1[k], a = vi[k];
        vi1[k] = s * a + c * h;
        vi[k]  = c * a - s * h;
    }
}
// col[k] -= f * e[k] + g * d[k], k in [k0, k1)
ICG_CLONES static void eig_rank2(double *__restrict col, const double *__restrict e, const double *__restrict d, int k0, int k1, double f, double g) {
    for (int k = k0; k < k1; k++) col[k] -= (f * e[k] + g * d[k]);
}
// col[k] -= g * d[k], k in [0, k1)
ICG_CLONES static void eig_axpy(double *__restrict col, const double *__restrict d, int k1, double g) {
    for (int k = 0; k < k1; k++) col[k] -= g * d[k];
}

void symmetricEigen(int n, const vector<double> &A, vector<double> &evals, vector<double> &evecs) {
    if (n == 0) {
        evals.clear(), evecs.clear();
        return;
    }
    // W holds the working matrix TRANSPOSED: v(i, j) = W[j * n + i] — every inner loop of the three phases then walks memory contiguously
    vector<double> W((size_t) n * n), d((size_t) n), e((size_t) n);
    for (int i = 0; i < n; i++)
        for (int j = 0; j < n; j++) W[(size_t) j * n + i] = A[(size_t) i * n + j];
    auto v   = [&](int i, int j) -> double & { return W[(size_t) j * n + i]; };
    auto col = [&](int j) -> double * { return &W[(size_t) j * n]; };
    double *dp = d.data(), *ep = e.data();
    // ---- tridiagonalise
    for (int j = 0; j < n; j++) dp[j] = v(n - 1, j);
    for (int i = n - 1; i > 0; i--) {
        double scale = 0.0, h = 0.0;
        for (int k = 0; k < i; k++) scale += std::fabs(dp[k]);
        if (scale == 0.0) {
            ep[i] = dp[i - 1];
            for (int j = 0; j < i; j++) {
                dp[j]   = v(i - 1, j);
                v(i, j) = 0.0;
                v(j, i) = 0.0;
            }
        } else {
            for (int k = 0; k < i; k++) {
                dp[k] /= scale;
                h += dp[k] * dp[k];
            }
            double f = dp[i - 1];
            double g = std::sqrt(h);
            if (f > 0) g = -g;
            ep[i]     = scale * g;
            h         = h - f * g;
            dp[i - 1] = f - g;
            for (int j = 0; j < i; j++) ep[j] = 0.0;
            double *ci = col(i);
            for (int j = 0; j < i; j++) ci[j] = dp[j]; // v(j, i) = d[j]
            // e[k] += v(k, j) d[j] (k > j) and g_j = e[j] + v(j, j) d[j] + sum_{k > j} v(k, j) d[k]: every sum in the order the one-column
            // loop adds it, four columns' (independent) chains in flight
            int j = 0;
            for (; j + 4 <= i; j += 4) {
                const double *c0 = col(j), *c1 = col(j + 1), *c2 = col(j + 2), *c3 = col(j + 3);
                const double f0 = dp[j], f1 = dp[j + 1], f2 = dp[j + 2], f3 = dp[j + 3];
                double g0 = ep[j] + c0[j] * f0;
                g0 += c0[j + 1] * dp[j + 1], ep[j + 1] += c0[j + 1] * f0;
                g0 += c0[j + 2] * dp[j + 2], ep[j + 2] += c0[j + 2] * f0;
                g0 += c0[j + 3] * dp[j + 3], ep[j + 3] += c0[j + 3] * f0;
                double g1 = ep[j + 1] + c1[j + 1] * f1;
                g1 += c1[j + 2] * dp[j + 2], ep[j + 2] += c1[j + 2] * f1;
                g1 += c1[j + 3] * dp[j + 3], ep[j + 3] += c1[j + 3] * f1;
                double g2 = ep[j + 2] + c2[j + 2] * f2;
                g2 += c2[j + 3] * dp[j + 3], ep[j + 3] += c2[j + 3] * f2;
                double g3 = ep[j + 3] + c3[j + 3] * f3;
                for (int k = j + 4; k < i; k++) {
                    const double dk = dp[k];
                    double ek = ep[k];
                    g0 += c0[k] * dk, ek += c0[k] * f0;
                    g1 += c1[k] * dk, ek += c1[k] * f1;
                    g2 += c2[k] * dk, ek += c2[k] * f2;
                    g3 += c3[k] * dk, ek += c3[k] * f3;
                    ep[k] = ek;
                }
                ep[j] = g0, ep[j + 1] = g1, ep[j + 2] = g2, ep[j + 3] = g3;
            }
            for (; j < i; j++) {
                const double *cj = col(j);
                f = dp[j];
                g = ep[j] + cj[j] * f;
                for (int k = j + 1; k <= i - 1; k++) {
                    g += cj[k] * dp[k];
                    ep[k] += cj[k] * f;
                }
                ep[j] = g;
            }
            f = 0.0;
            for (int jj = 0; jj < i; jj++) {
                ep[jj] /= h;
                f += ep[jj] * dp[jj];
            }
            const double hh = f / (h + h);
            for (int jj = 0; jj < i; jj++) ep[jj] -= hh * dp[jj];
            for (int jj = 0; jj < i; jj++) {
                f = dp[jj];
                g = ep[jj];
                double *cj = col(jj);
                eig_rank2(cj, ep, dp, jj, i, f, g);
                // (a later column jj' reads d[k] for k >= jj' > jj only: d[jj] is free to take the next step's value now)
                dp[jj]  = cj[i - 1];
                cj[i]   = 0.0;
            }
        }
        dp[i] = h;
    }
    // ---- accumulate the transformations
    for (int i = 0; i < n - 1; i++) {
        v(n - 1, i) = v(i, i);
        v(i, i)     = 1.0;
        const double h = dp[i + 1];
        if (h != 0.0) {
            const double *u = col(i + 1);
            for (int k = 0; k <= i; k++) dp[k] = u[k] / h;
            int j = 0;
            for (; j + 8 <= i + 1; j += 8) { // eight columns' (independent) sums in flight, each in its own order
                double *c0 = col(j), *c1 = col(j + 1), *c2 = col(j + 2), *c3 = col(j + 3), *c4 = col(j + 4), *c5 = col(j + 5), *c6 = col(j + 6), *c7 = col(j + 7);
                double g0 = 0.0, g1 = 0.0, g2 = 0.0, g3 = 0.0, g4 = 0.0, g5 = 0.0, g6 = 0.0, g7 = 0.0;
                for (int k = 0; k <= i; k++) {
                    const double uk = u[k];
                    g0 += uk * c0[k], g1 += uk * c1[k], g2 += uk * c2[k], g3 += uk * c3[k];
                    g4 += uk * c4[k], g5 += uk * c5[k], g6 += uk * c6[k], g7 += uk * c7[k];
                }
                eig_axpy(c0, dp, i + 1, g0), eig_axpy(c1, dp, i + 1, g1), eig_axpy(c2, dp, i + 1, g2), eig_axpy(c3, dp, i + 1, g3);
                eig_axpy(c4, dp, i + 1, g4), eig_axpy(c5, dp, i + 1, g5), eig_axpy(c6, dp, i + 1, g6), eig_axpy(c7, dp, i + 1, g7);
            }
            for (; j <= i; j++) {
                double *cj = col(j);
                double g = 0.0;
                for (int k = 0; k <= i; k++) g += u[k] * cj[k];
                eig_axpy(cj, dp, i + 1, g);
            }
        }
        double *u = col(i + 1);
        for (int k = 0; k <= i; k++) u[k] = 0.0;
    }
    for (int j = 0; j < n; j++) {
        dp[j]       = v(n - 1, j);
        v(n - 1, j) = 0.0;
    }
    v(n - 1, n - 1) = 1.0;
    ep[0]           = 0.0;
    // ---- implicit QL on the tridiagonal matrix; the Givens rotations act on two columns of V = two rows of W
    for (int i = 1; i < n; i++) ep[i - 1] = ep[i];
    ep[n - 1] = 0.0;
    double f = 0.0, tst1 = 0.0;
    const double eps = 2.220446049250313e-16;
    for (int l = 0; l < n; l++) {
        tst1  = std::max(tst1, std::fabs(dp[l]) + std::fabs(ep[l]));
        int m = l;
        while (m < n) {
            if (std::fabs(ep[m]) <= eps * tst1) break;
            m++;
        }
        if (m > l) {
            int iter = 0;
            do {
                iter++;
                double g = dp[l];
                double p = (dp[l + 1] - g) / (2.0 * ep[l]);
                double r = std::hypot(p, 1.0);
                if (p < 0) r = -r;
                dp[l]     = ep[l] / (p + r);
                dp[l + 1] = ep[l] * (p + r);
                const double dl1 = dp[l + 1];
                double h         = g - dp[l];
                for (int i = l + 2; i < n; i++) dp[i] -= h;
                f += h;
                p        = dp[m];
                double c = 1.0, c2 = c, c3 = c, s = 0.0, s2 = 0.0;
                const double el1 = ep[l + 1];
                for (int i = m - 1; i >= l; i--) {
                    c3 = c2;
                    c2 = c;
                    s2 = s;
                    g  = c * ep[i];
                    h  = c * p;
                    r  = std::hypot(p, ep[i]);
                    ep[i + 1] = s * r;
                    s         = ep[i] / r;
                    c         = p / r;
                    p         = c * dp[i] - s * g;
                    dp[i + 1] = h + s * (c * g + s * dp[i]);
                    eig_rotate(col(i), col(i + 1), n, c, s);
                }
                p     = -s * s2 * c3 * el1 * ep[l] / dl1;
                ep[l] = s * p;
                dp[l] = c * p;
            } while (std::fabs(ep[l]) > eps * tst1 && iter < 60);
        }
        dp[l] = dp[l] + f;
        ep[l] = 0.0;
    }
    vector<int> order((size_t) n);
    for (int i = 0; i < n; i++) order[(size_t) i] = i;
    std::sort(order.begin(), order.end(), [&](int x, int y) { return dp[x] < dp[y]; });
    evals.assign((size_t) n, 0.0);
    evecs.assign((size_t) n * n, 0.0);
    for (int k = 0; k < n; k++) {
        evals[(size_t) k] = dp[order[(size_t) k]];
        const double *src = col(order[(size_t) k]);
        for (int i = 0; i < n; i++) evecs[(size_t) i * n + k] = src[i];
    }
}

} // namespace icg
