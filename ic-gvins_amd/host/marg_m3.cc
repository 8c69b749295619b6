// M3 on plain arrays: see marg_m3.h.  Reference: factors/marginalization_info.h:153-192.
#include "marg_m3.h"

#include <chrono>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <limits>

#include "sym_eigen.h"

namespace icg {

// the symmetrised m-block of the P x P system and its eigen-decomposition: where both forms of the Schur step start
static void eigenOfMarginalizedBlock(int P, int m, const double *H, vector<double> &ev, vector<double> &V) {
    vector<double> Hmm((size_t) m * m);
    for (int i = 0; i < m; i++)
        for (int j = 0; j < m; j++) Hmm[(size_t) i * m + j] = 0.5 * (H[(size_t) i * P + j] + H[(size_t) j * P + i]);
    symmetricEigen(m, Hmm, ev, V);
}

// :170-192 from the eigenvectors on: Hmm^+ = Wv V^T with Wv = V diag(1 / ev) as the caller scaled it (only the lower triangle of the
// symmetric product is formed), T = Hrm Hmm^+, Hp = Hrr - T Hmr, bp = br - T bm.  The one copy of these loops: every sum over k ascending.
static void eliminateMarginalizedBlock(int P, int m, const double *H, const double *b, const vector<double> &V, const vector<double> &Wv,
                                       vector<double> &Hp, vector<double> &bp) {
    const int r = P - m;
    vector<double> Hinv((size_t) m * m, 0.0);
    for (int i = 0; i < m; i++)
        for (int j = 0; j <= i; j++) {
            double s = 0;
            for (int k = 0; k < m; k++) s += Wv[(size_t) i * m + k] * V[(size_t) j * m + k];
            Hinv[(size_t) i * m + j] = Hinv[(size_t) j * m + i] = s;
        }
    vector<double> T((size_t) r * m);
    for (int i = 0; i < r; i++)
        for (int j = 0; j < m; j++) {
            double s = 0;
            for (int k = 0; k < m; k++) s += H[(size_t) (m + i) * P + k] * Hinv[(size_t) k * m + j];
            T[(size_t) i * m + j] = s;
        }
    Hp.assign((size_t) r * r, 0.0);
    bp.assign((size_t) r, 0.0);
    for (int i = 0; i < r; i++) {
        for (int j = 0; j < r; j++) {
            double s = 0;
            for (int k = 0; k < m; k++) s += T[(size_t) i * m + k] * H[(size_t) k * P + m + j];
            Hp[(size_t) i * r + j] = H[(size_t) (m + i) * P + m + j] - s;
        }
        double s = 0;
        for (int k = 0; k < m; k++) s += T[(size_t) i * m + k] * b[(size_t) k];
        bp[(size_t) i] = b[(size_t) m + i] - s;
    }
}

// :170-192 on plain arrays: the m leading columns of the P x P system (H row-major, b) are eliminated
void schurReduce(int P, int m, const double *H, const double *b, double eps, vector<double> &Hp, vector<double> &bp, double *min_ev_m,
                 int *status) {
    vector<double> ev, V;
    auto tA = std::chrono::steady_clock::now();
    eigenOfMarginalizedBlock(P, m, H, ev, V);
    auto tB = std::chrono::steady_clock::now();
    if (getenv("ICG_MARG_DEBUG")) fprintf(stderr, "[schur] eigen(%d) %.3f ms\n", m, std::chrono::duration<double, std::milli>(tB - tA).count());
    if (min_ev_m) *min_ev_m = m > 0 ? ev[0] : std::numeric_limits<double>::infinity();
    if (status && m > 0 && ev[0] <= eps) *status |= 2;
    // Hmm^+ = V diag(1/ev, 0 below EPS) V^T: the thresholded reciprocals once, the scaled copy W = V diag(inv) once
    vector<double> inv((size_t) m), Wv((size_t) m * m);
    for (int k = 0; k < m; k++) inv[(size_t) k] = ev[(size_t) k] > eps ? 1.0 / ev[(size_t) k] : 0.0;
    for (int i = 0; i < m; i++)
        for (int k = 0; k < m; k++) Wv[(size_t) i * m + k] = V[(size_t) i * m + k] * inv[(size_t) k];
    eliminateMarginalizedBlock(P, m, H, b, V, Wv, Hp, bp);
}

bool schurReduceGuarded(int P, int m, const double *H, const double *b, double guard, vector<double> &Hp, vector<double> &bp) {
    vector<double> ev, V;
    eigenOfMarginalizedBlock(P, m, H, ev, V);
    for (int k = 0; k < m; k++)
        if (!(ev[(size_t) k] > guard)) return false;
    vector<double> Wv((size_t) m * m);
    for (int i = 0; i < m; i++)
        for (int k = 0; k < m; k++) Wv[(size_t) i * m + k] = V[(size_t) i * m + k] / ev[(size_t) k];
    eliminateMarginalizedBlock(P, m, H, b, V, Wv, Hp, bp);
    return true;
}

// :153-167 on plain arrays
void linearizePrior(int r, const vector<double> &Hp, const vector<double> &bp, double eps, vector<double> &J0, vector<double> &e0,
                    vector<double> *evals, int *status) {
    vector<double> ev, V;
    symmetricEigen(r, Hp, ev, V);
    J0.assign((size_t) r * r, 0.0);
    e0.assign((size_t) r, 0.0);
    for (int k = 0; k < r; k++) {
        const double S = ev[(size_t) k] > eps ? ev[(size_t) k] : 0.0, Sinv = ev[(size_t) k] > eps ? 1.0 / ev[(size_t) k] : 0.0;
        const double ss = std::sqrt(S), si = std::sqrt(Sinv);
        double vb = 0;
        for (int i = 0; i < r; i++) {
            J0[(size_t) k * r + i] = ss * V[(size_t) i * r + k];
            vb += V[(size_t) i * r + k] * -bp[(size_t) i];
        }
        e0[(size_t) k] = si * vb;
    }
    if (status && r > 0 && ev[0] <= eps) *status |= 4;
    if (evals) evals->swap(ev);
}

void linearizeReduced(int P, int m, const double *H, const double *b, double eps, vector<double> &Hp, vector<double> &bp, vector<double> &J0,
                      vector<double> &e0, vector<double> *evals, double *min_ev_m, int *status) {
    if (status) *status = 0;
    schurReduce(P, m, H, b, eps, Hp, bp, min_ev_m, status);
    linearizePrior(P - m, Hp, bp, eps, J0, e0, evals, status);
}

} // namespace icg
