// psr_scan_lower.hpp -- from the arguments of a plfx_psr_rate_scan call (plfx.h
// section 12) to what the C ABI issues: the call's checks, the carving of the
// caller's workspace, the tip-tiling launches, the split of the candidates
// into passes of at most `group`, and the launch list of a pass's traversal
// over group * n "virtual sites" (psr_lower.hpp).  Plain C++: device pointers
// are stored and compared, never followed (tests/psr_scan_lower_main.cpp
// drives it on the CPU).
#pragma once
#include <string>
#include <vector>

#include "../../include/plfx.h"
#include "plf_desc.hpp"  // PsrTileDescH
#include "psr_lower.hpp"

namespace plfx {

constexpr size_t kPsrScanAlign = 256;  // of the workspace and of every array carved from it

// Offsets into the workspace, in bytes.  Every array starts on a multiple of
// kPsrScanAlign: CLV k at clv0 + k * clv_stride (group * n * states values),
// tip array k at tip0 + k * row (group * n bytes), scaler row j at sc0 + j *
// row, the category bytes at cat0, the matrices at pm0 (2 * npmats * group *
// states^2 values); end: the size plfx_psr_rate_scan_workspace_gen reports.
struct PsrScanLayout {
  size_t clv0, clv_stride, tip0, row, sc0, cat0, pm0, end;
};

// PLFX_ERR_INVALID for a bad dtype, a negative count or n, a group outside
// 1..PLFX_PSR_MAX_CATS or states other than 4 (plfx.h section 12) and 20 (12b).
int psr_scan_layout(int dtype, int nops, int ntips, int npmats, int64_t n, int group, PsrScanLayout *out,
                    int states = 4);

// The arguments of the call, as plfx.h names them; fuse: the context's PSR
// level-pair switch (PLFX_FUSE), which 20 states ignore (the planner is given
// 0: there is no protein level pair); states: 4 or 20, checked by the caller;
// flags: 0 or PLFX_FMA (section 11d), handed to every pass's PsrCall -- the
// plan does not depend on it.
struct PsrScanCall {
  int dtype;
  const plfx_trav_op *ops;
  int nops;
  const uint8_t *const *tips;
  int nslots;
  const double *blen;
  int npmats;
  const double *eigen;
  const void *EV, *tipvec;
  const double *cand_rates;
  int ncand, group;
  int64_t n;
  void *workspace;
  size_t workspace_bytes;
  int32_t *best_idx;
  double *best_lnl, *all_lnl, *out_lnl;
  int fuse;
  int states = 4;
  int flags = 0;
};

// Candidates [k0, k0 + gc) in one traversal of gc * n virtual sites with gc
// categories; tail: gc < group, the pass runs the `tail` launch list (its
// matrices are gc * states^2 values apart) on prefixes of every array.
struct PsrScanPass {
  int k0, gc;
  bool tail;
};

struct PsrScanPlan {
  PsrScanLayout lay{};
  std::vector<PsrTileDescH> tiles;  // launched in chunks of kMaxBatch, the category bytes with the first
  std::vector<PsrScanPass> passes;
  PsrLaunchList full, tail;  // a pass's node launches: group categories / the last short pass's
  TravPlan trav;
  uint8_t *cat = nullptr;         // group * n category bytes: cat[g * n + i] = g
  void *pmats = nullptr;          // what plfx_pmatrix writes per pass
  const void *root = nullptr;     // the CLV of the last op's parent
  const uint8_t *scalers = nullptr;  // row j at scalers + j * sc_stride
  int64_t sc_stride = 0;
  // the traversal's slot arrays (kept for their capacity)
  std::vector<void *> clv;
  std::vector<const uint8_t *> wtips;
  std::vector<uint8_t *> sc_rows;
  void clear();
};

// Every check of the call, then the plan.  n == 0: no passes, no tiles (the
// caller zeroes out_lnl).  Returns PLFX_OK, PLFX_ERR_UNSUPPORTED for a dense
// leaf or PLFX_ERR_INVALID, the last two with *err set and *out cleared:
// nothing of a refused call is launched.
int lower_psr_scan(const PsrScanCall &c, PsrScanPlan *out, std::string *err);

}  // namespace plfx
