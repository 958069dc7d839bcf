// edge_newton_step.hpp -- the arithmetic of the branch-length stepper
// (edge_newton.hpp states the rules) as a plain struct with inline functions,
// shared by the host class EdgeNewton (plfx_edge_optimize) and the device
// loop of plfx_edge_optimize_dev (plf_edge.hpp edge_opt_kernel): the struct is
// also the per-edge state that kernel keeps in the stream workspace.  Only
// + - * / sqrt and comparisons, no multiply-add to contract; f64 / and sqrt are
// correctly rounded on host and device, so both walk the same t sequence bit
// for bit.
#pragma once
#include <cmath>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define PLFX_HD __host__ __device__
#else
#define PLFX_HD
#endif

namespace plfx {

struct EdgeNewtonStep {
  static constexpr double kTol = 1e-10;
  enum : unsigned {
    kLoSeen = 1u,  // the bracket's lower end was evaluated
    kHiSeen = 2u,  // its upper end
    kLast = 4u,    // the next evaluation is the one at the unseen end: stop after it
    kDone = 8u,    // stopped: t is the result (set by the device loop only)
  };
  double t, lo, hi;  // where to evaluate next (after the stop: the result); the bracket
  int evals;
  unsigned flags;

  // requires 0 < tmin <= t0 <= tmax
  PLFX_HD void init(double t0, double tmin, double tmax) {
    t = t0;
    lo = tmin;
    hi = tmax;
    evals = 0;
    flags = 0u;
  }

  // the derivatives at t: true = evaluate again at the new t
  PLFX_HD bool advance(double d1, double d2, int max_evals) {
    evals++;
    if (t <= lo) flags |= kLoSeen;
    if (t >= hi) flags |= kHiSeen;
    if (d1 > 0.0) {
      lo = t;
      flags |= kLoSeen;
    } else {
      hi = t;
      flags |= kHiSeen;
    }
    if ((flags & kLast) || evals >= max_evals) return false;
    double tn = d2 < 0.0 ? t - d1 / d2 : 0.0;
    // a Newton step this small is convergence wherever it lands: at the optimum it rounds onto the
    // bracket's end, and bisecting from there would only halve the bracket thirty more times
    if (d2 < 0.0 && std::fabs(tn - t) <= kTol * t) return false;
    if (!(d2 < 0.0) || !(tn > lo && tn < hi)) tn = std::sqrt(lo * hi);
    // the bracket has closed (its ends, or a bisection step across it, within kTol)
    const bool closed = hi / lo < 1.0 + kTol || std::fabs(tn - t) <= kTol * t;
    const bool both = (flags & kLoSeen) && (flags & kHiSeen);
    if (closed && !both) {  // d1 never changed sign: the optimum is the unseen end
      t = (flags & kLoSeen) ? hi : lo;
      flags |= kLast;
      return true;
    }
    if (closed) return false;
    t = tn;
    return true;
  }
};

}  // namespace plfx
