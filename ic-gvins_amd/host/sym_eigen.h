// The symmetric eigen-solver of the back-end's host side: M3 (marg_m3.cc) runs it on the m-block and on the reduced system.
#pragma once
#include <vector>

namespace icg {

using std::vector;

// symmetric eigen-decomposition (Householder tridiagonalisation + implicit QL), eigenvalues ascending, evecs row-major with eigenvectors in columns
void symmetricEigen(int n, const vector<double> &A, vector<double> &evals, vector<double> &evecs);

} // namespace icg
