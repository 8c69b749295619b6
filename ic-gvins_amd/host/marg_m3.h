// M3 on plain arrays (marginalization_info.h:153-192), what MarginalizationInfo::schurElimination / linearization / finishStructured run.
#pragma once
#include <vector>

namespace icg {

using std::vector;

// schurReduce: the m leading columns of the P x P system (H row-major, b) are eliminated through the eigen-decomposition of Hmm with the
// eps floor (m = 0: Hp = H, bp = b).  linearizePrior: Hp = J0^T J0, bp = -J0^T e0 on the eigenvalues above eps (J0 r x r row-major).
// Optional: evals (of Hp, ascending), min_ev_m (smallest eigenvalue of the m-block, +inf for m = 0), status (bits OR-ed in: 2 = an m-block
// eigenvalue <= eps, 4 = an Hp eigenvalue <= eps; linearizeReduced clears it first).
void schurReduce(int P, int m, const double *H, const double *b, double eps, vector<double> &Hp, vector<double> &bp, double *min_ev_m = nullptr,
                 int *status = nullptr);
// The same step where Hmm must be safely positive definite (the landmark-eliminated path, MarginalizationInfo::finishStructured): false,
// with Hp / bp as they were, unless every eigenvalue of the m-block is above `guard`; then the plain inverse, each eigenvector column
// DIVIDED by its eigenvalue (schurReduce multiplies by the rounded reciprocal: the two give different bits).
bool schurReduceGuarded(int P, int m, const double *H, const double *b, double guard, vector<double> &Hp, vector<double> &bp);
void linearizePrior(int r, const vector<double> &Hp, const vector<double> &bp, double eps, vector<double> &J0, vector<double> &e0,
                    vector<double> *evals = nullptr, int *status = nullptr);
void linearizeReduced(int P, int m, const double *H, const double *b, double eps, vector<double> &Hp, vector<double> &bp, vector<double> &J0,
                      vector<double> &e0, vector<double> *evals = nullptr, double *min_ev_m = nullptr, int *status = nullptr);

} // namespace icg
