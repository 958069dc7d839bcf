// edge_newton.hpp -- the branch-length stepper of plfx_edge_optimize: a
// bracketed Newton iteration for the zero of d lnL/dt on [tmin, tmax].  Plain
// C++: no GPU, no context (tests/edge_newton_main.cpp drives it on the CPU);
// plfx_api.hip evaluates the derivatives where the stepper asks for them.
//
// After each evaluation (t, d1, d2):
//   1. d1 > 0: lo = t, else hi = t  (the zero of d1 lies in [lo, hi]);
//   2. the proposal is the Newton step t - d1/d2 when d2 < 0;
//   3. when d2 >= 0 or the proposal is not strictly inside (lo, hi), the
//      proposal is the geometric bisection sqrt(lo hi) instead;
//   4. done when the step is <= kTol t (the Newton step is tested before it is
//      compared with the bracket: at the optimum it rounds onto an end), or
//      hi/lo < 1 + kTol, or max_evals evaluations were made.
// A bracket that has closed in on an end that was never evaluated (d1 has one
// sign on all of [tmin, tmax]: the optimum is that end) gets one last
// evaluation at the end itself, so the result is tmin or tmax exactly and the
// last evaluation is always the result's.
//
// The arithmetic is EdgeNewtonStep's (edge_newton_step.hpp), which the device
// loop of plfx_edge_optimize_dev shares; this class adds the argument check
// and the evaluation cap.
#pragma once
#include "edge_newton_step.hpp"

namespace plfx {

class EdgeNewton {
 public:
  static constexpr double kTol = EdgeNewtonStep::kTol;
  // requires 0 < tmin <= t0 <= tmax, max_evals >= 1 (valid() otherwise false)
  EdgeNewton(double t0, double tmin, double tmax, int max_evals);
  bool valid() const { return valid_; }
  // where to evaluate next; after the last advance(), the result
  double t() const { return s_.t; }
  // the derivatives at t(): true = evaluate again at the new t()
  bool advance(double d1, double d2);
  int evals() const { return s_.evals; }
  double lo() const { return s_.lo; }
  double hi() const { return s_.hi; }

 private:
  EdgeNewtonStep s_;
  int max_evals_;
  bool valid_;
};

}  // namespace plfx
