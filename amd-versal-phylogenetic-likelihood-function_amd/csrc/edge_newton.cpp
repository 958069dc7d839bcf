// edge_newton.cpp -- see edge_newton.hpp.
#include "edge_newton.hpp"

#include <cmath>

namespace plfx {

EdgeNewton::EdgeNewton(double t0, double tmin, double tmax, int max_evals)
    : max_evals_(max_evals),
      valid_(tmin > 0.0 && tmin <= t0 && t0 <= tmax && std::isfinite(tmax) && max_evals >= 1) {
  s_.init(t0, tmin, tmax);
}

bool EdgeNewton::advance(double d1, double d2) { return s_.advance(d1, d2, max_evals_); }

}  // namespace plfx
