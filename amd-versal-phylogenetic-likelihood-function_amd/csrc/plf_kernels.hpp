// plf_kernels.hpp -- launchers of the fused PLF kernels (internal to libplfx).
#pragma once
#include <hip/hip_runtime.h>
#include <cstdint>

#include "plf_desc.hpp"

namespace plfx {

// Self-resetting workspace of the in-kernel scaler-sum reduction
// (plf_dna.hpp block_ticket_sum): kWsWords 64-bit words, zero at rest.
constexpr int kWsWords = (32 + 1) * 16;

struct DnaArgs {
  const void *x1, *x2;
  void *x3;
  const void *EV, *left, *right;
  const int32_t *wgt;       // may be null (weights = 1)
  uint8_t *scaler;          // may be null
  int64_t *scaler_sum;      // may be null
  unsigned long long *ws;   // ticket words (needed iff scaler_sum); the f64 protein FMA
                            // launch also takes its tile queue from ws + kWsWords when
                            // non-null (2 x kWsWords words, zero at rest)
  int64_t n;
  int segments = -1;        // node kernels' XCD-segmented site mapping: -1 by size, 0 off,
                            // 1 on (plf_kernels.hip segment_grid; PLFX_NODE_SEGMENTS)
  int streams = 1;          // one-node calls the caller keeps in flight (plfx_ctx_set_streams):
                            // the dense DNA node kernels and the protein FMA kernels
                            // take the co-resident blocks / streams
};

// Fused DNA (4 states x 4 Gamma categories) inner-node update.
// Returns the hipError_t of the launch.
hipError_t launch_plf_dna_f32(const DnaArgs &a, int max_blocks, hipStream_t s);
hipError_t launch_plf_dna_f64(const DnaArgs &a, int max_blocks, hipStream_t s);

// sum_j scaler[j]*wgt[j] (host_mem.cpp:384-388), self-resetting ws as above.
// Protein (S=20, C=4) kernel; fma selects fused multiply-add.
hipError_t launch_plf_prot(int dtype, bool fma, const DnaArgs &a, int max_blocks, hipStream_t s,
                           int tips = 0, const void *tipvec = nullptr);
// Protein f64 in FMA mode on the VALU (plf_prot_valu.hip, PLFX_FMA | PLFX_VALU):
// P and EV as wave-uniform scalar operands, LDS holds only the staged child
// tile; bit-identical to the matrix-core FMA kernel, dense children, one node.
hipError_t launch_plf_prot_valu_f64(const DnaArgs &a, int max_blocks, hipStream_t s);
// Protein f64 in exact mode with the matrices as scalar operands
// (plf_prot_valu_exact.hip): bit-identical to the LDS-matrix exact kernel.
hipError_t launch_plf_prot_valu_exact_f64(const DnaArgs &a, int max_blocks, hipStream_t s);

// Batched nodes (<= kMaxBatch per launch) sharing EV, n, wgt.  dtype: 0 f32, 1 f64.
// tips: 0 dense children; 1 x1 of every node is a tip (uint8 state codes);
// 2 x1 and x2 are tips.  tipvec: 16 x 4 tip vectors of dtype (NULL = 0/1 bits).
// The descriptors (NodeDescH, ...) and their limits are plf_desc.hpp's.
hipError_t launch_plf_dna_batch(int dtype, const NodeDescH *nodes, int count, const void *EV,
                                const int32_t *wgt, int64_t n, unsigned long long *ws,
                                int max_blocks, hipStream_t s, int tips = 0,
                                const void *tipvec = nullptr, int share = 1);
// Tip/tip protein nodes from their 576-combination tables (plf_prot.hpp
// prot_tiptip_gather_kernel): x3 / scaler / sum of each node gathered by code pair.
hipError_t launch_prot_tiptip_gather(int dtype, const ProtGatherDescH *d, int count, const int32_t *wgt,
                                     int64_t n, unsigned long long *ws, int max_blocks, hipStream_t s);

// Protein nodes (f64, f32; FMA or exact) whose two children are tip/tip nodes held in
// combination tables (plf_prot.hpp ProtTabDesc), batched as above.
hipError_t launch_prot_tab_batch(int dtype, bool fma, const ProtTabDescH *d, int count, const void *EV,
                                 const int32_t *wgt, int64_t n, unsigned long long *ws, int max_blocks,
                                 hipStream_t s);

// Protein (S = 20) nodes batched the same way; fma as launch_plf_prot.
hipError_t launch_plf_prot_batch(int dtype, bool fma, const NodeDescH *nodes, int count, const void *EV,
                                 const int32_t *wgt, int64_t n, unsigned long long *ws, int max_blocks,
                                 hipStream_t s, int tips, const void *tipvec);

// Root log-likelihood; partials: >= kLnlMaxGrid doubles (one accumulator); ticket: kWsWords u64 (zero at rest).
constexpr int kLnlMaxGrid = 4096;
hipError_t launch_root_lnl(int dtype, int states, const void *x, int64_t n, const double *catw,
                           const double *freq, const int32_t *wgt, const int64_t *scaler_sums,
                           int nsums, double *partials, unsigned long long *ticket, double *out,
                           double *site_lnl, hipStream_t s);

// One branch between two fixed CLVs (plf_edge.hpp; defined in plf_edge.hip =
// libplfx_edge.so, which libplfx.so links).  Sum table: tip != 0 reads
// x1 as uint8 codes through tipvec (required then).  Derivatives: partials
// >= 3 * kLnlMaxGrid doubles, ticket as launch_root_lnl's; lambda, rates (4),
// t: device f64; out: 3 device doubles.
hipError_t launch_edge_sumtable(int dtype, int states, bool tip, const void *x1, const void *x2, int64_t n,
                                const void *tipvec, void *sumtab, int max_blocks, hipStream_t s);
hipError_t launch_edge_derivatives(int dtype, int states, const void *sumtab, int64_t n, const double *lambda,
                                   const double *rates, const double *catw, const int32_t *wgt,
                                   const double *t, const int64_t *scaler_sums, int nsums, double *partials,
                                   unsigned long long *ticket, double *out3, double *site_lnl,
                                   int max_blocks, hipStream_t s);

// The branch-length loop of plfx_edge_optimize_dev for count <= kMaxBatch
// edges that share n, the model and wgt: max_evals launches, one evaluation
// and one step of every unfinished edge each (plf_edge.hpp edge_opt_kernel).
// sumtabs: host array of device tables; t0, t_opt (count), out3 (3 * count, may
// be null), evals (count, may be null): device.  state: kMaxBatch *
// kEdgeStateBytes bytes (no rest state: the first launch writes it); partials
// as above; ws: kMaxBatch regions of kWsWords (zero at rest).
constexpr int kEdgeStateBytes = 32;  // sizeof(EdgeNewtonStep), asserted in plf_edge.hpp
hipError_t launch_edge_optimize(int dtype, int states, const void *const *sumtabs, int count, int64_t n,
                                const double *lambda, const double *rates, const double *catw,
                                const int32_t *wgt, const double *t0, double tmin, double tmax, int max_evals,
                                void *state, double *partials, unsigned long long *ws, double *t_opt,
                                double *out3, int32_t *evals, int max_blocks, hipStream_t s);

// Per-site rate categories (plf_psr.hpp; defined in plf_psr.hip =
// libplfx_psr.so, which libplfx.so links): DNA, one of ncat (1..32) categories
// per site from the device bytes rate_cat, CLVs of n * 4 values.  Node: count
// <= kMaxBatch nodes of one kind per launch, tips bit 0 / 1 = child 1 / 2 of
// every node is coded (its descriptor pointer names uint8 codes), left / right
// of ncat * 16 values, ws as launch_plf_dna_batch's.  Root lnL, sum table and
// edge sums: as their Gamma counterparts above, partials / ticket included.
hipError_t launch_plf_psr(int dtype, int tips, const NodeDescH *nodes, int count, const void *EV,
                          const uint8_t *rate_cat, int ncat, const int32_t *wgt, int64_t n, const void *tipvec,
                          unsigned long long *ws, int max_blocks, hipStream_t s);
// Fused PSR level pairs (plf_psr.hpp plf_psr_triple_kernel): count <=
// kMaxTriples per launch, ws >= 3 * count regions; tips 0 / 1 / 2 = the
// number of coded children of each leaf op, coded child first; every matrix
// of ncat * 16 values.
hipError_t launch_plf_psr_triples(int dtype, int tips, const TripleDescH *t, int count, const void *EV,
                                  const uint8_t *rate_cat, int ncat, const int32_t *wgt, int64_t n,
                                  const void *tipvec, unsigned long long *ws, int max_blocks, hipStream_t s);
hipError_t launch_root_lnl_psr(int dtype, const void *x, int64_t n, const double *freq, const int32_t *wgt,
                               const int64_t *scaler_sums, int nsums, double *partials,
                               unsigned long long *ticket, double *out, double *site_lnl, int max_blocks,
                               hipStream_t s);
hipError_t launch_edge_sumtable_psr(int dtype, bool tip, const void *x1, const void *x2, int64_t n,
                                    const void *tipvec, void *sumtab, int max_blocks, hipStream_t s);
hipError_t launch_edge_derivatives_psr(int dtype, const void *sumtab, int64_t n, const double *lambda,
                                       const double *rates, int ncat, const uint8_t *rate_cat,
                                       const int32_t *wgt, const double *t, const int64_t *scaler_sums, int nsums,
                                       double *partials, unsigned long long *ticket, double *out3,
                                       double *site_lnl, int max_blocks, hipStream_t s);
// count <= kMaxBatch sum tables with one kind of side 1 in one launch (edge =
// blockIdx.y), n >= 1; tip: every x1 names uint8 codes.
hipError_t launch_edge_sumtable_psr_batch(int dtype, bool tip, const PsrEdgeDescH *edges, int count, int64_t n,
                                          const void *tipvec, int max_blocks, hipStream_t s);
// launch_edge_optimize for PSR sum tables (plf_psr.hpp edge_opt_psr_kernel):
// state, partials and ws are the same regions.  A one-edge call has
// launch_edge_derivatives_psr's grid.
hipError_t launch_edge_optimize_psr(int dtype, const void *const *sumtabs, int count, int64_t n,
                                    const double *lambda, const double *rates, int ncat,
                                    const uint8_t *rate_cat, const int32_t *wgt, const double *t0, double tmin,
                                    double tmax, int max_evals, void *state, double *partials,
                                    unsigned long long *ws, double *t_opt, double *out3, int32_t *evals,
                                    int max_blocks, hipStream_t s);

// The per-site rate scan (plfx.h section 12; plf_psr.hpp psr_site_lnl_kernel,
// psr_tile_kernel), n >= 1.  scalers: nsc rows `stride` bytes apart (may be
// NULL with nsc == 0).  site_lnl: one segment, per-site lnL with the site's own
// scaling correction, no workspace.  scan_pass: gc candidates from k0 over
// gc * n virtual sites of x, the running best updated (`first`: started), the
// weighted total into out through partials / ticket when out != NULL.  tile:
// count <= kMaxBatch tips tiled `group` times and, when cat != NULL, the
// group * n category bytes.
hipError_t launch_psr_site_lnl(int dtype, const void *x, int64_t n, const double *freq, const uint8_t *scalers,
                               int nsc, int64_t stride, double *site_lnl, int max_blocks, hipStream_t s);
hipError_t launch_psr_scan_pass(int dtype, const void *x, int64_t n, int gc, const double *freq,
                                const uint8_t *scalers, int nsc, int64_t stride, int k0, bool first,
                                double *all_lnl, double *best_lnl, int32_t *best_idx, const int32_t *wgt,
                                double *partials, unsigned long long *ticket, double *out, int max_blocks,
                                hipStream_t s);
hipError_t launch_psr_tile(const PsrTileDescH *tips, int count, int64_t n, int group, uint8_t *cat, int max_blocks,
                           hipStream_t s);

// All-branch derivatives of a PSR tree (plfx.h section 13; plf_psr_branch.hpp;
// defined in plf_psr_branch.hip = libplfx_psr_branch.so, which libplfx.so
// links): DNA.  Pairs: count <= kMaxPairs ops per launch, ws >= 2 * count
// regions; tips 0 / 1 / 2 = the coded children of each op, coded child first.
// Counts: one chunk of count <= kScaleChunk ops from `first` -- the subtree
// sums (outer_pass false; scaler_sums -> sub) or the outer sums and edge_scale
// (true; wsum, sub -> outer, edge_scale), one block.
hipError_t launch_psr_branch_pairs(int dtype, int tips, const BranchPairDescH *pairs, int count, const void *EV,
                                   const uint8_t *rate_cat, int ncat, const int32_t *wgt, int64_t n,
                                   const void *tipvec, unsigned long long *ws, int max_blocks, hipStream_t s);
hipError_t launch_psr_branch_counts(bool outer_pass, const BranchScaleDescH *ops, int first, int count,
                                    const int64_t *scaler_sums, const int64_t *wsum, int64_t *sub, int64_t *outer,
                                    int64_t *edge_scale, hipStream_t s);
int psr_branch_sites_per_lane(int dtype);  // the pair kernel's sites per lane and trip (dtype 1 = f64)

// Protein per-site rate categories (plfx.h section 11b; plf_psr_prot.hpp;
// defined in plf_psr_prot.hip = libplfx_psr_prot.so, which libplfx.so links):
// CLVs of n * 20 values, every matrix of ncat * 400, tipvec NULL or 24 x 20
// values.  The arguments are launch_plf_psr's and launch_root_lnl_psr's.
hipError_t launch_plf_psr_prot(int dtype, int tips, const NodeDescH *nodes, int count, const void *EV,
                               const uint8_t *rate_cat, int ncat, const int32_t *wgt, int64_t n,
                               const void *tipvec, unsigned long long *ws, int max_blocks, hipStream_t s);
hipError_t launch_root_lnl_psr_prot(int dtype, const void *x, int64_t n, const double *freq, const int32_t *wgt,
                                    const int64_t *scaler_sums, int nsums, double *partials,
                                    unsigned long long *ticket, double *out, double *site_lnl, int max_blocks,
                                    hipStream_t s);
// The same node in FMA mode on the f64 matrix cores (plfx.h section 11d;
// plf_psr_prot_mfma.hpp; defined in plf_psr_prot_mfma.hip =
// libplfx_psr_prot_mfma.so, which libplfx.so links): f64 only, the arguments
// of launch_plf_psr_prot without the dtype.
hipError_t launch_plf_psr_prot_mfma(int tips, const NodeDescH *nodes, int count, const void *EV,
                                    const uint8_t *rate_cat, int ncat, const int32_t *wgt, int64_t n,
                                    const void *tipvec, unsigned long long *ws, int max_blocks, hipStream_t s);
// The branch-length half (plfx.h section 11c): launch_edge_sumtable_psr,
// _psr_batch, launch_edge_derivatives_psr and launch_edge_optimize_psr for
// tables of n * 20 values, tipvec 24 x 20 values; n >= 1 for the sum tables.
hipError_t launch_edge_sumtable_psr_prot(int dtype, bool tip, const void *x1, const void *x2, int64_t n,
                                         const void *tipvec, void *sumtab, int max_blocks, hipStream_t s);
hipError_t launch_edge_sumtable_psr_prot_batch(int dtype, bool tip, const PsrEdgeDescH *edges, int count, int64_t n,
                                               const void *tipvec, int max_blocks, hipStream_t s);
hipError_t launch_edge_derivatives_psr_prot(int dtype, const void *sumtab, int64_t n, const double *lambda,
                                            const double *rates, int ncat, const uint8_t *rate_cat,
                                            const int32_t *wgt, const double *t, const int64_t *scaler_sums,
                                            int nsums, double *partials, unsigned long long *ticket, double *out3,
                                            double *site_lnl, int max_blocks, hipStream_t s);
hipError_t launch_edge_optimize_psr_prot(int dtype, const void *const *sumtabs, int count, int64_t n,
                                         const double *lambda, const double *rates, int ncat,
                                         const uint8_t *rate_cat, const int32_t *wgt, const double *t0, double tmin,
                                         double tmax, int max_evals, void *state, double *partials,
                                         unsigned long long *ws, double *t_opt, double *out3, int32_t *evals,
                                         int max_blocks, hipStream_t s);
// The protein rate scan (plfx.h section 12b; plf_psr_prot.hpp
// psr_site_lnl_prot_kernel): launch_psr_site_lnl and launch_psr_scan_pass over
// rows of 20 values, the same arguments.  The tiling is launch_psr_tile's.
hipError_t launch_psr_site_lnl_prot(int dtype, const void *x, int64_t n, const double *freq, const uint8_t *scalers,
                                    int nsc, int64_t stride, double *site_lnl, int max_blocks, hipStream_t s);
hipError_t launch_psr_scan_pass_prot(int dtype, const void *x, int64_t n, int gc, const double *freq,
                                     const uint8_t *scalers, int nsc, int64_t stride, int k0, bool first,
                                     double *all_lnl, double *best_lnl, int32_t *best_idx, const int32_t *wgt,
                                     double *partials, unsigned long long *ticket, double *out, int max_blocks,
                                     hipStream_t s);

hipError_t launch_scaler_sum(const uint8_t *scaler, const int32_t *wgt, int64_t n,
                             int64_t *out, unsigned long long *ws, int max_blocks,
                             hipStream_t s);

// P matrices from an eigensystem (plf_pmat.hpp).  dtype 0 f32 / 1 f64.
hipError_t launch_pmatrix(int dtype, bool eigen_conv, const double *eigen, int S,
                          const double *rates, int ncat, const double *blen, int64_t nbranch,
                          void *out, hipStream_t s);

// Fused level pairs (plf_dna.hpp TripleDesc), dtype 0 f32 / 1 f64; <= kMaxTriples per
// launch, ws >= 3 * count regions.  tips as plf_dna_f64_triple_kernel's kTips.
hipError_t launch_plf_dna_triples(int dtype, const TripleDescH *t, int count, const void *EV,
                                  const int32_t *wgt, int64_t n, unsigned long long *ws,
                                  int max_blocks, hipStream_t s, int tips, const void *tipvec);

// Fused three-level subtrees (plf_dna.hpp SeptetDesc), dtype 0 f32 / 1 f64; <= kMaxSeptets
// per launch, ws >= 7 * count regions.  tips as plf_dna_f64_septet_kernel's kTips.
hipError_t launch_plf_dna_septets(int dtype, const SeptetDescH *t, int count, const void *EV,
                                  const int32_t *wgt, int64_t n, unsigned long long *ws,
                                  int max_blocks, hipStream_t s, int tips, const void *tipvec);

// Fused complete subtree of depth 4..6 (plf_dna.hpp DeepDesc: 2^depth leaves,
// 2^depth - 1 nodes in heap order by level), dtype 0 f32 / 1 f64, one per
// launch, ws >= 2^depth - 1 regions.  tips: 0 dense leaves; 2 every leaf a tip
// (uint8 state codes), tipvec as launch_plf_dna_batch's.
// the deep passes' chunk queue: this region of the stream workspace (plf_dna.hpp WaveQueue)
constexpr int kDeepQueueRegion = 63;
hipError_t launch_plf_dna_deep(int dtype, int depth, const DeepDescH *t, const void *EV,
                               const int32_t *wgt, int64_t n, unsigned long long *ws, int max_blocks,
                               hipStream_t s, int tips = 0, const void *tipvec = nullptr);

}  // namespace plfx
