// edge_newton.cpp -- see edge_newton.hpp.
#include "edge_newton.hpp"

#include <cmath>

namespace plfx {

EdgeNewton::EdgeNewton(double t0, double tmin, double tmax, int max_evals)
    : t_(t0), lo_(tmin), hi_(tmax), max_evals_(max_evals),
      valid_(tmin > 0.0 && tmin <= t0 && t0 <= tmax && std::isfinite(tmax) && max_evals >= 1) {}

bool EdgeNewton::advance(double d1, double d2) {
  evals_++;
  if (t_ <= lo_) lo_seen_ = true;
  if (t_ >= hi_) hi_seen_ = true;
  if (d1 > 0.0) {
    lo_ = t_;
    lo_seen_ = true;
  } else {
    hi_ = t_;
    hi_seen_ = true;
  }
  if (last_ || evals_ >= max_evals_) return false;
  double tn = d2 < 0.0 ? t_ - d1 / d2 : 0.0;
  // a Newton step this small is convergence wherever it lands: at the optimum it rounds onto the
  // bracket's end, and bisecting from there would only halve the bracket thirty more times
  if (d2 < 0.0 && std::fabs(tn - t_) <= kTol * t_) return false;
  if (!(d2 < 0.0) || !(tn > lo_ && tn < hi_)) tn = std::sqrt(lo_ * hi_);
  // the bracket has closed (its ends, or a bisection step across it, within kTol)
  const bool closed = hi_ / lo_ < 1.0 + kTol || std::fabs(tn - t_) <= kTol * t_;
  if (closed && !(lo_seen_ && hi_seen_)) {  // d1 never changed sign: the optimum is the unseen end
    t_ = lo_seen_ ? hi_ : lo_;
    last_ = true;
    return true;
  }
  if (closed) return false;
  t_ = tn;
  return true;
}

}  // namespace plfx
