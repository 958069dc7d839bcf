/*
 * plfx.h -- C ABI of the MI355X-native PLF engine (libplfx.so).
 *
 * This is the drop-in boundary.  It replaces the two interfaces through which
 * the reference drives its PLF hot path:
 *
 *   (1) the CPU entry point  void plf(float* x1_start, float* x2_start,
 *       float* x3_start, float* EV, const int n, float* left, float* right,
 *       int* wgt, int& scalerIncrement)
 *       -- /root/reference/app/src/plf.h:1-5, defined app/src/plf.cpp:8-68,
 *       called from app/src/host_mem.cpp:418;
 *   (2) the XRT accelerator contract of app/src/host_mem.cpp:108-157,283-394:
 *       per instance an `in_left` bo = [EV16 | P_L64 | CLV_L], an `in_right`
 *       bo = [EV16 | P_R64 | CLV_R] (COMBINED) or [P_R64 | CLV_R] (SEPARATE),
 *       an `out` bo (CLV) and an `out_scaler` bo (char per site), with kernel
 *       arguments mm2sleft/mm2sright(mem, alignment_sites, window_size)
 *       (hls/src/mm2sleft_memDNAwindowComb.cpp:16) and
 *       s2mm(mem, scalerIncrement, alignment_sites, window_size)
 *       (hls/src/s2mm_memDNAwindowComb.cpp:20), and the host-side scaler
 *       reduction sum_j scaler[j]*wgt[j] (host_mem.cpp:384-388).
 *
 * Data layout (identical to the reference): a site is S*C values stored
 * site-major as x[site*16 + cat*4 + state] for DNA (4 Gamma categories x 4
 * states, plf.cpp:21-23); P matrices are left[cat*16 + k*4 + l] (row-major
 * P_c, plf.cpp:37-38); EV is EV[k*4 + l] (plf.cpp:47).
 *
 * Semantics (plf.cpp:19-65): for every site and category
 *   ump_L[k] = sum_l x1[c*4+l]*left[c*16+k*4+l]   (same for right/x2)
 *   x3[c*4+l] = sum_k (ump_L[k]*ump_R[k]) * EV[4k+l]
 * then if every |x3| of the site is < 2^-32 (strict; NaN never scales), all
 * values of the site are multiplied by 2^32, the per-site scaler byte is 1
 * and wgt[site] is added to the scaler increment.  Arithmetic is IEEE with
 * no FMA contraction and the reference's accumulation order, so the f32
 * entry points reproduce the reference bit-for-bit and f64 reproduces the
 * double instantiation of the same loop bit-for-bit.
 *
 * All functions return PLFX_OK (0) or a negative plfx_status; they never
 * throw.  plfx_last_error() gives a message for the last failure on a
 * context.  `stream` arguments are hipStream_t values passed as void* (NULL =
 * the HIP null stream, as everywhere in HIP; plfx_ctx_stream() gives the
 * context's own non-blocking stream).  Device pointers must come from the same HIP
 * device as the context; CLV pointers must be 16-byte aligned.  Every entry
 * point binds the context's device for its duration and restores the
 * caller's current device on return.  Calls on one context from several host
 * threads are serialised by the context (one lock per context, held for the
 * call: host entry points block other threads' calls for their duration;
 * device entry points only for the launch); distinct contexts are independent.
 * plfx_last_error() reports the last failure on the context, whichever thread
 * made it; the string is the calling thread's copy, valid until that thread
 * calls plfx_last_error() again.
 *
 * Streams and the scaler-sum workspace.  Sum-producing launches (scaler_sum
 * outputs, plfx_scaler_sum, plfx_root_lnl) reduce across thread blocks through
 * a small self-resetting device workspace.  The context keeps ONE workspace
 * PER STREAM in use (up to PLFX_MAX_STREAMS at a time), so launches on
 * different streams may run concurrently; launches on one stream are ordered
 * by the stream.  hipStreamPerThread names a different stream in every host
 * thread and gets a workspace per thread.  The first PLFX_WS_POOL streams take
 * workspaces allocated with the context, so their first use may be inside a
 * graph capture; a further stream's first sum-producing use allocates (not
 * inside hipStreamBeginCapture: issue one call on it before capturing).
 * plfx_ctx_release_stream() waits for a stream and returns its workspace to
 * the pool -- call it before destroying a stream used with the context, or
 * when rotating through many streams (not while the stream is being captured:
 * PLFX_ERR_INVALID).  A captured graph keeps the workspace of the stream it
 * was captured on, so its replays must not overlap other work on that
 * workspace, and must not outlive the context; releasing such a stream retires
 * its workspace (no other stream is ever given it) instead of returning it to
 * the pool.  A hipStreamPerThread workspace whose thread exits without
 * releasing it is retired too, and reclaimed (after a device-wide wait, not
 * inside a capture) when the context runs out of workspaces.
 * plfx_ctx_destroy() waits for the context's stream; if a stream other than
 * the context's still holds a workspace, or one was used under a capture, it
 * waits for the whole device (hipDeviceSynchronize, which must not overlap a
 * global-mode capture in another thread) -- it never uses a caller's stream
 * handle, which may already be destroyed.  Release streams before destroy
 * (plfx_ctx_release_stream) to keep destroy off the device-wide wait.  Graph
 * replays still in flight must finish before destroy.
 * The same workspace also holds the tile/chunk queues of the protein f64 FMA
 * kernel (from 2^20 sites) and of the fused six-level tree passes: blocks or
 * waves that run ahead take more of the alignment instead of a fixed share
 * (every site is computed the same way, so results do not change); the queue
 * words, like the sums, reset themselves at the end of each launch.
 * The reduction encodes arrival counts next to the sums: a count is read
 * back exactly for every running sum S of a launch with
 * -2^40 <= S <= 2^40 - 1 and is off by one at S = 2^40 and at S = -2^40 - 1.
 * Every running sum is bounded by sum_j |wgt[j]|, so the contract is
 * sum_j |wgt[j]| < 2^40 per launch (the reference's own scalerIncrement is a
 * 32-bit int); the host entry points check this (PLFX_ERR_INVALID, nothing
 * written; fewer than 512 sites cannot reach the bound), the device entry
 * points cannot check it cheaply and leave it to the caller.  Inside the
 * contract every scaler_sum is the exact int64 sum.
 *
 * No allocation happens per call after warm-up (the host entry points keep
 * grow-only staging buffers in the context).  Each workspace also holds the
 * protein tip/tip combination tables (about 11.8 MB; the pool's
 * PLFX_WS_POOL of them, ~95 MB, are allocated with the context).  A context
 * created with PLFX_CTX_LAZY_TABLES (DNA-only users) allocates a workspace's
 * tables on its first protein tip/tip call instead; that first call may then
 * not be inside a capture (PLFX_ERR_INVALID).
 * Every entry point rejects a parent CLV x3 that shares any byte with a child
 * it reads (PLFX_ERR_INVALID).
 *
 * Timing note: after an idle gap of ~0.3 s or more the MI355X lowers its
 * shader clock to ~1.8-2.0 GHz for the first ~10-15 ms of renewed load
 * (DVFS; measured in-kernel, HISTORY.md section 3.3).  HBM-bound calls (DNA)
 * run <= 4 % slower through it, the protein matrix-core kernels ~10 %.  It
 * is a property of the device's power management, not of a context or a
 * process, so no library-side warm-up can absorb it.
 */
#ifndef PLFX_H
#define PLFX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PLFX_VERSION 10300 /* 1.3.0 */
#define PLFX_MAX_STREAMS 64 /* streams holding a workspace at a time, per context */
#define PLFX_WS_POOL 8      /* workspaces allocated with the context */
#define PLFX_STREAMS_MAX 8  /* plfx_ctx_set_streams */

typedef enum {
  PLFX_OK = 0,
  PLFX_ERR_INVALID = -1,     /* bad argument (null pointer, size, alignment) */
  PLFX_ERR_HIP = -2,         /* HIP runtime failure; see plfx_last_error()   */
  PLFX_ERR_NOMEM = -3,       /* device allocation failed                      */
  PLFX_ERR_NODEV = -4,       /* no such HIP device / not a gfx950 device      */
  PLFX_ERR_UNSUPPORTED = -5  /* states/categories combination not built       */
} plfx_status;

/* Instance-buffer header layout: app/src/include.h:20 (COMBINED, SEPARATE). */
typedef enum { PLFX_LAYOUT_COMBINED = 0, PLFX_LAYOUT_SEPARATE = 1 } plfx_layout;
/* AIE transport of the reference: app/src/include.h:21 (STREAM, WINDOW).
 * Only affects buffer sizing (padding); the GPU needs neither. */
typedef enum { PLFX_AIE_STREAM = 0, PLFX_AIE_WINDOW = 1 } plfx_aie;
typedef enum { PLFX_F32 = 0, PLFX_F64 = 1 } plfx_dtype;

typedef struct plfx_ctx plfx_ctx;

/* ---- context ----------------------------------------------------------- */
/* Replaces acap_info (app/src/include.h:28-147): binds a HIP device and owns
 * a non-blocking stream, the scaler-sum workspace and host staging buffers. */
int plfx_ctx_create(int device, plfx_ctx **ctx);
/* flags: 0 (= plfx_ctx_create) or PLFX_CTX_LAZY_TABLES (see "Streams and the
 * scaler-sum workspace"); other bits are PLFX_ERR_INVALID. */
#define PLFX_CTX_LAZY_TABLES 1u
int plfx_ctx_create_ex(int device, unsigned flags, plfx_ctx **ctx);
int plfx_ctx_destroy(plfx_ctx *ctx);
const char *plfx_last_error(const plfx_ctx *ctx);
int plfx_get_version(void);
/* The context's stream (hipStream_t) and device ordinal. */
void *plfx_ctx_stream(plfx_ctx *ctx);
int plfx_ctx_device(const plfx_ctx *ctx);
/* Synchronise the context's stream. */
int plfx_ctx_synchronize(plfx_ctx *ctx);
/* Wait for `stream` (hipStream_t; NULL = the null stream; hipStreamPerThread =
 * the calling thread's) and return its scaler-sum workspace to the context's
 * pool.  PLFX_OK also when the stream holds none.  (Extension: the reference's
 * XRT queues are fixed per instance, host_mem.cpp:123-127.) */
int plfx_ctx_release_stream(plfx_ctx *ctx, void *stream);
/* One-node calls the caller keeps in flight at once, each on its own stream
 * (default 1; PLFX_STREAMS=1..8 in the environment at context creation,
 * empty = 1, anything else fails plfx_ctx_create with PLFX_ERR_INVALID).  The dense
 * one-node DNA kernels (plfx_plf_dev_f32 / _f64, plfx_plf_dev_gen with 4
 * states, and the host entries' chunks) and the protein FMA kernels
 * (plfx_plf_dev_gen, 20 states, PLFX_FMA; f32 rounds up to whole blocks per
 * CU) then launch the co-resident blocks / streams, and a DNA batch (plfx_plf_batch_dev) the share of them its
 * nodes would take / streams, so the calls in flight fill the GPU together and one call's
 * drain overlaps the others' work: 2^20-site f64 nodes alternating over two
 * streams run 0.80 of the HBM peak instead of 0.78 (0.75 one at a time),
 * f32 0.81 instead of 0.77.  Same bits for any value.
 * A call issued alone with streams > 1 runs on the smaller grid (0.64 for
 * the f64 node at 2): set it to what is actually in flight.  Other entry
 * points ignore it.  For many large nodes, one call per node over two streams
 * beats batches (512 nodes of 2^20 f64 sites: 0.793 vs 0.775 for 32-node
 * batches on two streams, 0.766 on one).  (Extension: the reference's instances run side by side,
 * app/src/include.h:181-195.)  set: PLFX_ERR_INVALID outside 1..8; get: the
 * value, or PLFX_ERR_INVALID for a null context. */
int plfx_ctx_set_streams(plfx_ctx *ctx, int streams);
int plfx_ctx_streams(const plfx_ctx *ctx);

/* ---- (1) drop-in for plf(): host arrays, synchronous -------------------- */
/* Same argument order and meaning as plf() (app/src/plf.h:1-5); `int&` is
 * `int*`.  Copies to the device, runs the fused kernel, copies back.
 * wgt may be NULL (= all ones).  *scalerIncrement is the exact sum of the
 * scaled sites' weights reduced modulo 2^32 to a signed 32-bit int (the
 * reference's `int` accumulation wraps the same way).  sum |wgt| >= 2^40 is
 * refused with PLFX_ERR_INVALID before anything is copied or written. */
int plfx_plf_f32(plfx_ctx *ctx, const float *x1_start, const float *x2_start,
                 float *x3_start, const float *EV, int n, const float *left,
                 const float *right, const int *wgt, int *scalerIncrement);
int plfx_plf_f64(plfx_ctx *ctx, const double *x1_start, const double *x2_start,
                 double *x3_start, const double *EV, int n, const double *left,
                 const double *right, const int *wgt, int *scalerIncrement);

/* ---- (2) the hot path on device-resident CLVs, asynchronous ------------- */
/* All pointers are device pointers.  wgt, scaler (uint8 per site, the s2mm
 * char output) and scaler_sum (int64, = sum scaler*wgt, wgt NULL => 1) are
 * each optional (NULL = not produced / not read).  n may be 0.  From 2^25
 * sites (f32 and f64) the kernel deals the sites to the 8 XCDs as eight
 * contiguous segments instead of one grid-wide stride -- same bits, +1-29 %
 * HBM rate on long CLVs; env PLFX_NODE_SEGMENTS,
 * read at context creation: "1" forces the segments, "0" the one window,
 * "-1" / "auto" / "" keep the choice by size; any other value makes context
 * creation fail with PLFX_ERR_INVALID.  Segments need 8 blocks: under a grid
 * cap below 8 (PLFX_MAX_BLOCKS) the one window runs. */
int plfx_plf_dev_f32(plfx_ctx *ctx, const float *x1, const float *x2, float *x3,
                     const float *EV, int64_t n, const float *left,
                     const float *right, const int32_t *wgt, uint8_t *scaler,
                     int64_t *scaler_sum, void *stream);
int plfx_plf_dev_f64(plfx_ctx *ctx, const double *x1, const double *x2, double *x3,
                     const double *EV, int64_t n, const double *left,
                     const double *right, const int32_t *wgt, uint8_t *scaler,
                     int64_t *scaler_sum, void *stream);

/* ---- (2b) any state count (extension: BASELINE configs[4], protein) ------ */
/* states = 4 (DNA, the kernels above) or 20 (protein); 4 Gamma categories.
 * Layout generalises plf(): x[site*4S + cat*S + state], left/right
 * [cat][k][l] (S*S per category), EV[k][l] (S*S).  flags: PLFX_EXACT keeps
 * plf()'s separate multiply/add and operation order (bit-identical to the
 * double/float instantiation of the reference loop); PLFX_FMA fuses each
 * multiply-add (one rounding per term, within 1e-12 relative in f64; protein
 * only, on the matrix cores -- v_mfma_f64_16x16x4 / v_mfma_f32_16x16x4 are
 * k-ordered fma chains, so the result is bit-identical to a fused VALU loop;
 * DNA is always exact).  PLFX_FMA | PLFX_VALU (protein f64, plfx_plf_dev_gen
 * only): the same fused chains on the VALU, the P matrices as scalar operands
 * -- BASELINE configs[4]'s "matvec, not MFMA" -- bit-identical to PLFX_FMA.
 * Exact mode is always on the VALU (PLFX_VALU accepted, no effect). */
#define PLFX_EXACT 0
#define PLFX_FMA 1
#define PLFX_VALU 2
int plfx_plf_dev_gen(plfx_ctx *ctx, int dtype, int states, int flags, const void *x1,
                     const void *x2, void *x3, const void *EV, int64_t n, const void *left,
                     const void *right, const int32_t *wgt, uint8_t *scaler,
                     int64_t *scaler_sum, void *stream);

/* ---- (3) the accelerator instance-buffer contract ----------------------- */
/* in_left/in_right/out_clv/out_scaler: device buffers exactly as the
 * reference packs them (host_mem.cpp:221-243): in_left = [EV 16 | P_L 64 |
 * CLV_L], in_right = [EV 16 | P_R 64 | CLV_R] (COMBINED) or [P_R 64 | CLV_R]
 * (SEPARATE); element type `dtype`.  Writes alignment_sites CLVs to out_clv
 * and alignment_sites scaler bytes to out_scaler (never the window padding,
 * SURVEY Q4/Q5).  window_size (bytes of an AIE window, a multiple of 16; 0
 * for stream configs) is validated for sizing parity but not needed by the
 * kernel. */
int plfx_instance_run(plfx_ctx *ctx, const void *in_left, const void *in_right,
                      void *out_clv, uint8_t *out_scaler, uint32_t alignment_sites,
                      uint32_t window_size, int layout, int dtype, void *stream);

/* The same contract on HOST buffers, synchronous -- one accelerator instance
 * run as host_mem.cpp:293-318 drives it: write the active prefix of the two
 * input bos (bo.write(..., active bytes), :297-298), run the movers and the
 * graph (:305), read back alignment_sites CLVs and scaler bytes (:313-314).
 * The copies go through the context's device staging and stream; out_scaler
 * may be NULL.  Host buffers may be pageable or page-locked. */
int plfx_instance_run_host(plfx_ctx *ctx, const void *in_left, const void *in_right,
                           void *out_clv, uint8_t *out_scaler, uint32_t alignment_sites,
                           uint32_t window_size, int layout, int dtype);

/* ---- (4) scaler reduction (host_mem.cpp:384-388) on the device ---------- */
/* out_sum (device int64) = sum_j scaler[j] * (wgt ? wgt[j] : 1). */
int plfx_scaler_sum(plfx_ctx *ctx, const uint8_t *scaler, const int32_t *wgt,
                    int64_t n, int64_t *out_sum, void *stream);

/* ---- (6) many inner nodes per launch (extension: the reference evaluates
 * one node per call; BASELINE configs 3 and 4) -------------------------- */
/* One inner-node update: parent x3 from children x1, x2 with this node's P
 * matrices (left/right: C*S*S values, layout of plf.cpp:37-38).  scaler
 * (uint8 per site) and scaler_sum (int64) are optional per node. */
typedef struct {
  const void *x1, *x2;
  void *x3;
  const void *left, *right;
  uint8_t *scaler;
  int64_t *scaler_sum;
} plfx_node;

/* `count` independent nodes sharing EV, n and wgt; all device pointers, the
 * `nodes` array itself is host memory (it travels in the kernel arguments, 32
 * nodes per launch: graph-capture safe).  states 4 (DNA) or 20 (protein,
 * exact mode; up to 32 nodes per launch, node = blockIdx.y, each node with
 * its own scaler-sum workspace region). */
int plfx_plf_batch_dev(plfx_ctx *ctx, int dtype, int states, const plfx_node *nodes, int count,
                       const void *EV, int64_t n, const int32_t *wgt, void *stream);

/* A traversal descriptor (RAxML-style post-order list).  Op j computes CLV
 * slot `parent` from slots `child1`, `child2` with the P-matrix pair `pmat`:
 * left = pmats + (2*pmat)*C*S*S, right = pmats + (2*pmat+1)*C*S*S. */
typedef struct {
  int32_t parent, child1, child2, pmat;
} plfx_trav_op;

/* Executes `ops` in an order equivalent to the sequential one: ops are grouped
 * into dependency levels (an op waits for the ops that write its children and
 * for earlier readers/writers of its parent slot) and each level is issued as
 * batched launches.  clv: host array of `nslots` device CLV pointers;
 * scalers: host array of nops device uint8 pointers (or NULL / NULL entries);
 * scaler_sums: device int64[nops] (or NULL): entry j = op j's scalerIncrement. */
int plfx_traverse(plfx_ctx *ctx, int dtype, int states, const plfx_trav_op *ops, int nops,
                  void *const *clv, int nslots, const void *pmats, int npmats, const void *EV,
                  int64_t n, const int32_t *wgt, uint8_t *const *scalers, int64_t *scaler_sums,
                  void *stream);

/* ---- (8) tip children (extension) ---------------
 * A tip (leaf) is stored as one state code per site -- uint8, bit s set =
 * state s possible (A=1 C=2 G=4 T=8, ambiguity codes are unions, 15 = gap /
 * unknown; the upper nibble is ignored), the RAxML/PLL encoding -- instead of
 * a dense CLV of 16 values per site (16x/32x less traffic for that child).
 * Results are bit-identical to plf() on the expanded dense CLV
 * x[i][c][s] = (code_i >> s) & 1 for every category c.
 *
 * Protein (states = 20, plfx_plf_tips_dev_gen / plfx_traverse_tips): a code is
 * an index into a table of 24 dense rows of 20 values (codes >= 24 read row
 * 23); the default table (tipvec NULL), states in ARNDCQEGHILKMFPSTWYV order:
 * 0..19 one state, 20 = B (N|D), 21 = Z (Q|E), 22 = X, 23 = gap (all states);
 * tipvec = a device table of 24 x 20 values of dtype replaces it.  Exact and
 * FMA modes as plfx_plf_dev_gen, bit-identical to the dense computation on
 * x[i][c][s] = tv[code_i][s] in that mode. */

/* tipvec: NULL, or a device table of 16 x 4 values of dtype -- the dense
 * per-category CLV entry of each code, tipvec[code*4 + s] (the default is the
 * 0/1 state indicator; plfx_model_tip_vectors gives the eigen-convention
 * table).  Results are bit-identical to plf() on x[i][c][s] = tipvec[code_i][s].
 *
 * One node: exactly one of (tip1, x1) and one of (tip2, x2) is non-NULL;
 * the other arguments are those of plfx_plf_dev_f32/f64 (device pointers). */
int plfx_plf_tips_dev(plfx_ctx *ctx, int dtype, const uint8_t *tip1, const void *x1,
                      const uint8_t *tip2, const void *x2, void *x3, const void *EV, int64_t n,
                      const void *left, const void *right, const int32_t *wgt, uint8_t *scaler,
                      int64_t *scaler_sum, const void *tipvec, void *stream);

/* plfx_plf_tips_dev for states 4 or 20 and flags as plfx_plf_dev_gen
 * (PLFX_FMA: protein nodes on the f64 / f32 matrix cores; DNA is always exact). */
int plfx_plf_tips_dev_gen(plfx_ctx *ctx, int dtype, int states, int flags, const uint8_t *tip1,
                          const void *x1, const uint8_t *tip2, const void *x2, void *x3,
                          const void *EV, int64_t n, const void *left, const void *right,
                          const int32_t *wgt, uint8_t *scaler, int64_t *scaler_sum,
                          const void *tipvec, void *stream);

/* plfx_traverse with tip slots and flags: tips is a host array of nslots device
 * pointers (or NULL = no tips); a slot with tips[s] != NULL is a tip (clv[s] is
 * not read) and may not be an op's parent (codes and tipvec as above for the
 * states).  Each level is
 * issued as up to three batched launches (tip/tip, tip/inner, inner/inner),
 * six-level subtrees over dense leaves, three-level subtrees and level pairs
 * fused where possible (bit-identical results; env PLFX_FUSE=2 no six-level
 * passes, 1 pairs only, 0 none).  states 4 or 20; flags as
 * plfx_plf_dev_gen (PLFX_FMA: protein nodes on the f64 / f32 matrix cores;
 * DNA is always exact).  plfx_traverse == flags PLFX_EXACT, no tips, no tipvec.
 * Protein tip/tip nodes (here and in plfx_plf_tips_dev_gen) are evaluated once
 * per code pair (24 x 24) into tables of the stream's workspace (allocated
 * with the workspace, so also a stream's first call inside a capture uses
 * them) and gathered per site: the same values as the direct computation.  In
 * a traversal (exact and FMA modes, f64 and f32), a node whose two children
 * are such nodes of the level before stages its children from their tables
 * instead of reading their CLVs back (the CLVs are still written; the results
 * are the same). */
int plfx_traverse_tips(plfx_ctx *ctx, int dtype, int states, int flags, const plfx_trav_op *ops,
                       int nops, void *const *clv, const uint8_t *const *tips, int nslots,
                       const void *pmats,
                       int npmats, const void *EV, int64_t n, const int32_t *wgt,
                       uint8_t *const *scalers, int64_t *scaler_sums, const void *tipvec,
                       void *stream);

/* The schedule the last plfx_traverse(_tips) or plfx_traverse_psr call on this
 * context chose:
 * counts[i] for i < ncounts (extra entries are not written) of
 *   0: fused six-level passes (63 ops)   1: five-level (31)   2: four-level (15)
 *   3: three-level passes (7 ops)        4: level pairs (3 ops)
 *   5: ops run unfused                   6: kernel launches issued
 * Returns the number of entries written. */
#define PLFX_SCHED_COUNTS 7
int plfx_traverse_schedule(const plfx_ctx *ctx, int *counts, int ncounts);

/* ---- (7) root log-likelihood (extension) -- */
/* lnL = sum_i wgt_i * log( sum_c catw[c] * sum_s freq[s] * x[i][c][s] )
 *       + (sum_{j<nsums} scaler_sums[j]) * log(2^-32)
 * x: device CLV of the root (n sites, states S in {4, 20}, 4 categories);
 * catw (4), freq (S): device f64 arrays or NULL (uniform); wgt NULL = 1;
 * scaler_sums: device int64[nsums] (the inner nodes' scalerIncrements).
 * out_lnl: device double; site_lnl: optional device double[n] (log L_i
 * without the scaling correction).  Deterministic (fixed reduction order). */
int plfx_root_lnl(plfx_ctx *ctx, int dtype, int states, const void *x, int64_t n,
                  const double *catw, const double *freq, const int32_t *wgt,
                  const int64_t *scaler_sums, int nsums, double *out_lnl, double *site_lnl,
                  void *stream);

/* ---- (5) instance sizing: testbench_info (app/src/include.h:150-266) ---- */
/* 64-bit throughout.  `instance` < 0 means "no instance" where the
 * reference has an overload without one. */
typedef struct {
  uint64_t alignment_sites;
  uint32_t parallel_instances;
  uint32_t window_size;  /* bytes, AIE window (include.h:155) */
  int32_t layout;        /* plfx_layout */
  int32_t aie_type;      /* plfx_aie */
} plfx_testbench;

uint64_t plfx_tb_alignments_per_instance(const plfx_testbench *tb, int instance);
uint64_t plfx_tb_alignments_padding(const plfx_testbench *tb);
uint64_t plfx_tb_instance_site_offset(const plfx_testbench *tb, int instance);
uint64_t plfx_tb_elements_per_instance(const plfx_testbench *tb);
uint64_t plfx_tb_instance_elements_left(const plfx_testbench *tb);
uint64_t plfx_tb_instance_elements_right(const plfx_testbench *tb);
uint64_t plfx_tb_instance_elements_out(const plfx_testbench *tb);
uint64_t plfx_tb_instance_active_elements_left(const plfx_testbench *tb, int instance);
uint64_t plfx_tb_instance_active_elements_right(const plfx_testbench *tb, int instance);
uint64_t plfx_tb_num_windows_per_instance(const plfx_testbench *tb);

/* Host packing of one instance's input buffers (host_mem.cpp:221-243) into
 * caller-provided host arrays of instance_elements_{left,right} elements of
 * `dtype`; padding is zero-filled. */
int plfx_pack_instance(const plfx_testbench *tb, int instance, int dtype,
                       const void *EV, const void *left, const void *right,
                       const void *x1_all, const void *x2_all, void *out_left,
                       void *out_right);

/* The reference's partition of `total` items over `parts` (include.h:181-189,
 * offsets host_mem.cpp:229,290-291): n0 = ceil(total/parts), part k covers
 * [k*n0, k*n0 + count), the last part short by n0*parts - total.  Used for
 * sites over instances and for independent inner nodes over ranks (BASELINE
 * configs[3]).  PLFX_ERR_INVALID where the reference's arithmetic underflows
 * (the padding reaches a whole share, e.g. 10 items over 8 parts). */
int plfx_shard(uint64_t total, uint32_t parts, uint32_t k, uint64_t *offset, uint64_t *count);

/* The host_mem.cpp:179-209 input protocol with a fixed seed (the reference
 * uses std::random_device): std::mt19937(seed) + uniform_real_distribution
 * <double>(0,1): EV[16], then left[64]/right[64] interleaved, then x1/x2
 * (16*n each) interleaved, x1 x 1e-12 on every 4th site; wgt (may be NULL)
 * = 1.  Host arrays of `dtype`. */
int plfx_gen_hostmem(int dtype, uint32_t seed, uint64_t n, void *EV, void *left, void *right,
                     void *x1, void *x2, int32_t *wgt);

/* ---- (5b) sw_emu: the accelerator instance emulated on the CPU ----------
 * The reference's software-emulation target (make run TARGET=sw_emu,
 * Makefile:199-220; host_mem.cpp:160-164; BASELINE configs[0]): one instance
 * run as its dataflow on the host, window by window -- mm2sleft/mm2sright
 * (hls/src/mm2s{left,right}_memDNAwindow{Comb,Sep}.cpp, stream:
 * mm2sleft_memDNAstreamComb.cpp) split each 512-bit site word into 4 lane
 * beats and prepend the EV half and the transposed P_c (transpose.cpp:6-24)
 * to every window, each lane runs mmul_branch x2 -> combine -> ev
 * (aie/src/128x9DNAwindow8192Comb/kernels/), and s2mm
 * (hls/src/s2mm_memDNAwindowComb.cpp:45-99) reassembles the 16 values, tests
 * and rescales them with the padding mask.  Host buffers only, no GPU, no
 * context; in_left/in_right must hold the whole padded instance
 * (plfx_tb_instance_elements_left/right).  Writes alignment_sites CLVs and
 * scaler bytes (never the padding, as plfx_instance_run).  Arithmetic in
 * plf()'s order: results are bit-identical to plfx_instance_run.  An explicit
 * target like the reference's, never a fallback of the GPU entry points.
 * aie_type: PLFX_AIE_WINDOW (window_size bytes, a multiple of 32) or
 * PLFX_AIE_STREAM (COMBINED only; window_size ignored). */
int plfx_swemu_instance_run(const void *in_left, const void *in_right, void *out_clv,
                            uint8_t *out_scaler, uint32_t alignment_sites, uint32_t window_size,
                            int layout, int aie_type, int dtype);

/* ---- (9) model setup: P matrices and EV from branch lengths (extension,
 * SURVEY section 8f row 3; the reference's inputs are random or precomputed,
 * host_mem.cpp:189-197, aie/data/inputbranch*) ---------------------------- */
typedef enum { PLFX_PMAT_STATE = 0, PLFX_PMAT_EIGEN = 1 } plfx_pmat_convention;

/* Eigensystem of the time-reversible rate matrix Q_ij = r_ij pi_j (i != j),
 * normalised to one expected substitution per unit time.  exch: S(S-1)/2
 * exchangeabilities, upper triangle row-major (DNA: AC AG AT CG CT GT);
 * freqs: S positive frequencies (normalised here).  eigen (host, S+2S^2
 * doubles) = lambda[S] (descending, lambda_0 = 0) | V[S*S] | Vinv[S*S],
 * row-major, Q = V diag(lambda) Vinv.  Host-only; 2 <= S <= 64. */
int plfx_model_eigen(int states, const double *exch, const double *freqs, double *eigen);

/* Yang (1994) discrete Gamma: ncat equal-probability categories of a
 * Gamma(alpha, alpha) (mean 1); rate = category mean (median = 0) or the
 * median rescaled to mean 1 (median != 0).  Host-only. */
int plfx_gamma_rates(double alpha, int ncat, int median, double *rates);

/* EV (S*S, host) for a convention: STATE -> identity; EIGEN -> EV[k][l] =
 * Vinv[l][k] (CLVs in eigen coordinates, the RAxML form of plf()). */
int plfx_model_ev(int states, int convention, const double *eigen, double *EV);

/* Root weights w (S, host) for plfx_root_lnl's `freq`: STATE -> freqs;
 * EIGEN -> w[k] = sum_s pi_s V[s][k] (the root CLV is in eigen coordinates). */
int plfx_model_root_weights(int states, int convention, const double *eigen, const double *freqs,
                            double *w);

/* Tip vectors (host, 16 x S doubles; DNA: S = 4) for plfx_plf_tips_dev /
 * plfx_traverse_tips: STATE -> tv[code][s] = bit s of code; EIGEN -> tv[code]
 * = Vinv . bits(code) (tips in eigen coordinates). */
int plfx_model_tip_vectors(int states, int convention, const double *eigen, double *tv);

/* Device: pmats[b][c][k][l] (nbranch * ncat * S * S values of dtype) from the
 * eigensystem (device, S+2S^2 doubles, as plfx_model_eigen), category rates
 * (device, ncat doubles) and branch lengths (device, nbranch doubles):
 *   STATE: P_c(t_b) = V diag(exp(lambda r_c t_b)) Vinv;
 *   EIGEN: V[k][l] exp(lambda_l r_c t_b).
 * Branch 2j / 2j+1 are P-matrix pair j's left / right (the traverse layout).
 * f64 arithmetic (device exp, within a few ulp of the host libm). */
int plfx_pmatrix(plfx_ctx *ctx, int dtype, int states, int convention, const double *eigen,
                 const double *rates, int ncat, const double *blen, int64_t nbranch, void *pmats,
                 void *stream);

/* ---- (10) one branch between two fixed CLVs: the sum table, the edge
 * log-likelihood with d/dt and d2/dt2, and the branch-length optimum
 * (extension: RAxML's makenewz, next to plf() = newview and (7) = evaluate) --
 * The CLVs MUST be in the eigen convention (PLFX_PMAT_EIGEN: P matrices from
 * plfx_pmatrix, EV from plfx_model_ev, tips through plfx_model_tip_vectors).
 * With V = Pi^-1/2 U (plfx_model_eigen) V^T Pi V = I, so for the CLVs a, b at
 * the two ends of a branch of length t
 *   L_i(t) = sum_c catw[c] * sum_k a[i][c][k] * b[i][c][k] * exp(lambda_k r_c t)
 * with no further weights; a and b stay fixed while t varies.  STATE-
 * convention CLVs give meaningless results (not detected).
 *
 * Sum table: sumtab[i][c][k] = x1[i][c][k] * x2[i][c][k], one multiply
 * rounded in dtype; the layout is the CLV layout (n * 4 * states values),
 * states 4 or 20.  Side 1 is either dense (x1) or a coded tip (tip1: uint8
 * codes as in section 8, then x1[i][c][k] = tipvec[row][k] with row =
 * code & 15 of 16 x 4 for DNA and min(code, 23) of 24 x 20 for protein);
 * exactly one of tip1 / x1 is non-NULL and tipvec is required with tip1 (the
 * default 0/1 table is not in eigen coordinates).  Only side 1 may be coded:
 * the product is symmetric, so pass the tip first.  x1, x2, sumtab: 16-byte
 * aligned; sumtab may not share a byte with x1 or x2.  f32 products of two
 * very small entries may underflow (as RAxML's f32 sum table would): the
 * table is not rescaled.  Asynchronous, capture-safe. */
int plfx_edge_sumtable(plfx_ctx *ctx, int dtype, int states, const uint8_t *tip1, const void *x1,
                       const void *x2, int64_t n, const void *tipvec, void *sumtab, void *stream);

/* out3 (3 device doubles), all arithmetic in f64, with x_ck = lambda_k r_c,
 * e = exp(x t), e1 = e x, e2 = e1 x and L, L1, L2 = sum_c catw[c] sum_k
 * sumtab[i][c][k] * {e, e1, e2} (ascending k, then ascending c):
 *   out3[0] = sum_i wgt_i log L_i + (sum_{j<nsums} scaler_sums[j]) * log(2^-32)
 *   out3[1] = sum_i wgt_i L1/L                   (d lnL / dt)
 *   out3[2] = sum_i wgt_i (L2/L - (L1/L)^2)      (d2 lnL / dt2)
 * Scaling cancels in out3[1], out3[2].  eigen: the device array plfx_pmatrix
 * takes (only lambda is read); rates: device, ncat doubles; ncat must be 4
 * (PLFX_ERR_UNSUPPORTED otherwise); t: one device double; catw, wgt,
 * scaler_sums as in plfx_root_lnl (NULL: uniform, 1, none); site_lnl:
 * optional device double[n], log L_i.  n == 0: out3 = {correction, 0, 0}.
 * Deterministic (the fixed reduction order of (7)); asynchronous, uses the
 * stream's workspace, capture-safe as plfx_root_lnl. */
int plfx_edge_derivatives(plfx_ctx *ctx, int dtype, int states, const void *sumtab, int64_t n,
                          const double *eigen, const double *rates, int ncat, const double *catw,
                          const int32_t *wgt, const double *t, const int64_t *scaler_sums, int nsums,
                          double *out3, double *site_lnl, void *stream);

/* The branch length in [tmin, tmax] that maximises the edge log-likelihood: a
 * bracketed Newton iteration on d lnL/dt from t0.  After each evaluation
 * d1 > 0 raises the lower end of the bracket to t, else the upper end drops
 * to t; the next t is the Newton step t - d1/d2 when d2 < 0 and the step
 * lands strictly inside the bracket, else the geometric mean of the bracket's
 * ends; it stops when the step is <= 1e-10 t, the bracket's ends are within
 * 1 + 1e-10 of each other, or after max_evals evaluations.  When d1 has one
 * sign on the whole interval the result is tmin or tmax itself.  Host-
 * synchronous (24 bytes come back per evaluation through a buffer of the
 * context; nothing is allocated): PLFX_ERR_INVALID on a capturing stream and
 * unless 0 < tmin <= t0 <= tmax, max_evals >= 1.  t_opt, out3_host (may be
 * NULL; lnL without scaling correction, d1, d2 at t_opt) and evals (may be
 * NULL; evaluations made) are host pointers; the rest as above. */
int plfx_edge_optimize(plfx_ctx *ctx, int dtype, int states, const void *sumtab, int64_t n,
                       const double *eigen, const double *rates, int ncat, const double *catw,
                       const int32_t *wgt, double t0, double tmin, double tmax, int max_evals,
                       double *t_opt, double *out3_host, int *evals, void *stream);

/* The same iteration for nedges independent branches with the loop kept on
 * the device: asynchronous, allocates nothing, legal on a capturing stream
 * (the stream's workspace, as plfx_root_lnl; so a stream's first use may be
 * the capture while pool entries last).  sumtabs: HOST array of nedges device
 * sum tables (n * 4 * states values of dtype each, 16-byte aligned, none
 * NULL; the pointers travel in kernel arguments, as plfx_node's do, so the
 * array may be reused after the call); n, eigen, rates, catw and wgt are
 * shared by all edges.  t0: device, nedges doubles, read by the call's first
 * launch -- so an earlier call's t_opt can be the next call's t0 with no host
 * in between; a t0[j] outside [tmin, tmax] is clamped into it (the host
 * cannot check it).  t_opt: device, nedges doubles.  out3: device, 3 * nedges
 * doubles or NULL: edge j's lnL (no scaling correction), d1, d2 at t_opt[j].
 * evals: device int32[nedges] or NULL: evaluations made.  Every edge walks
 * the t sequence plfx_edge_optimize walks from the same start, bit for bit
 * (one stepper, correctly rounded f64 arithmetic on both sides), and a
 * one-edge call sums in plfx_edge_derivatives' order, so its t_opt, out3 and
 * evals are plfx_edge_optimize's.  Deterministic.
 * Mechanism: exactly max_evals launches per group of up to 32 edges, each one
 * evaluation and one step of every edge of the group that has not stopped (a
 * stopped edge's blocks return at entry); no grid-wide barrier.  max_evals
 * therefore bounds the launches as well as the evaluations:
 * PLFX_ERR_INVALID unless 1 <= max_evals <= PLFX_EDGE_MAX_EVALS, 0 < tmin <=
 * tmax < infinity, nedges >= 1, t0 and t_opt non-NULL and every table
 * non-NULL and aligned; PLFX_ERR_UNSUPPORTED as plfx_edge_derivatives. */
#define PLFX_EDGE_MAX_EVALS 256
int plfx_edge_optimize_dev(plfx_ctx *ctx, int dtype, int states, const void *const *sumtabs, int nedges,
                           int64_t n, const double *eigen, const double *rates, int ncat,
                           const double *catw, const int32_t *wgt, const double *t0, double tmin,
                           double tmax, int max_evals, double *t_opt, double *out3, int32_t *evals,
                           void *stream);

/* ---- (11) per-site rate categories (PSR) -- the GTRCAT model of RAxML /
 * ExaML next to the Gamma model of every section above (extension) ----------
 * Every site belongs to exactly ONE of ncat rate categories, so a PSR CLV is
 * x[site*4 + state] -- n * 4 values, a quarter of the Gamma layout, 16-byte
 * aligned -- and a node's P matrices are chosen per site.  DNA (4 states),
 * f32 and f64; the entry points of this section have no states argument (the
 * Python binding answers a protein request to them with
 * PLFX_ERR_UNSUPPORTED).  Section (11b) has the node, the traversal and the
 * root lnL for protein.
 *   rate_cat: device uint8[n]; site i uses category min(rate_cat[i], ncat-1)
 *             (the clamp of protein tip codes >= 24: no index leaves a table);
 *   ncat:     1 <= ncat <= PLFX_PSR_MAX_CATS, else PLFX_ERR_INVALID;
 *   left, right: ncat * 16 values of dtype, [c][k][l] -- what plfx_pmatrix
 *             writes per branch for `ncat` rates.
 * Node update, with c the site's category, in plf()'s operation order and
 * with no FMA contraction:
 *   umpL[k]  = sum_l x1[i][l] * left[c*16 + k*4 + l]     (same for right / x2)
 *   x3[i][l] = sum_k (umpL[k] * umpR[k]) * EV[4k + l]
 * then, if all FOUR |x3[i][.]| < 2^-32 (strict; NaN never scales), they are
 * multiplied by 2^32, scaler[i] = 1 and wgt[i] is added to the node's scaler
 * sum: plf()'s loop with one category, run on each category's sites with that
 * category's matrices, bit for bit.  A child is dense or coded as in section
 * (8): uint8 codes, x[i][s] = tipvec[(code & 15)*4 + s], tipvec a device table
 * of 16 x 4 values of dtype or NULL (the 0/1 indicator); results are
 * bit-identical to the dense computation on the expanded child. */
#define PLFX_PSR_MAX_CATS 32

/* One PSR node: exactly one of tip1 / x1 and one of tip2 / x2 is non-NULL;
 * scaler (uint8 per site) and scaler_sum (int64) are optional.  All device
 * pointers. */
typedef struct {
  const uint8_t *tip1;
  const void *x1;
  const uint8_t *tip2;
  const void *x2;
  void *x3;
  const void *left, *right;
  uint8_t *scaler;
  int64_t *scaler_sum;
} plfx_psr_node;

/* count >= 1 independent nodes sharing EV, n, rate_cat, wgt and tipvec.  The
 * `nodes` array is host memory and travels in the kernel arguments (nodes of
 * one kind of children, up to 32 per launch, node = blockIdx.y, as
 * plfx_plf_batch_dev): asynchronous, allocates nothing, capture-safe as
 * plfx_plf_batch_dev; count == 1 is the one-node call.  Every check runs
 * before the first launch: PLFX_ERR_INVALID for count < 1, n < 0, ncat out of
 * range, a null EV / rate_cat / nodes, and per node for both or neither of
 * tip / dense on a side, a null x3 / left / right, a dense child or x3 not
 * 16-byte aligned, and an x3 that shares a byte with a child it reads.  n ==
 * 0: nothing is launched and the nodes' scaler sums are zeroed. */
int plfx_plf_psr_dev(plfx_ctx *ctx, int dtype, const plfx_psr_node *nodes, int count, const void *EV,
                     int64_t n, const uint8_t *rate_cat, int ncat, const int32_t *wgt, const void *tipvec,
                     void *stream);

/* plfx_traverse_tips for PSR CLVs: a whole post-order op list in one call.
 * ops, clv, tips, nslots, scalers, scaler_sums as there (a slot with tips[s]
 * != NULL is a coded tip and may not be a parent; tips NULL = no tips); EV,
 * rate_cat, ncat, wgt, tipvec and the CLV layout (n * 4 values) as in
 * plfx_plf_psr_dev.  Op j's matrices are left = pmats + (2*pmat) * ncat*16 and
 * right = pmats + (2*pmat + 1) * ncat*16 values of dtype: what plfx_pmatrix
 * writes for 2 * npmats branches and ncat rates.
 * The ops are levelled as in plfx_traverse_tips; per level, ops a, b whose
 * outputs are the two children of an op p of the next level (a and b with the
 * same number of coded children) run with p as one fused level-pair launch
 * (up to 10 triples each) that never reads a's and b's CLVs back, and the
 * other ops as plfx_plf_psr_dev batches.  Whatever the schedule, every CLV,
 * scaler byte and scaler_sums[j] is bit-identical to running the ops one by
 * one in list order as one-node plfx_plf_psr_dev calls.  Level pairs are
 * formed when the environment's PLFX_FUSE is >= 1 (deeper fused passes do not
 * exist for PSR).  PLFX_FUSE=0 or unset runs every op unfused: unlike the
 * Gamma traversals, fusion is not the default here, because level pairs are
 * faster on large alignments only (at 2^20 sites, not at 2^14).
 * plfx_traverse_schedule reports the call: entries 0..3 are 0, 4 the level
 * pairs, 5 the unfused ops, 6 the launches.
 * Asynchronous, allocates nothing, descriptors in the kernel arguments,
 * capture-safe as plfx_plf_psr_dev.  Every check runs before the first launch
 * (PLFX_ERR_INVALID, nothing is launched): the op list's (slot / pmat range,
 * a parent that is a child of its op or a tip), ncat, n < 0, a null EV /
 * rate_cat / pmats / clv, per op the node checks of plfx_plf_psr_dev (a null
 * CLV of a non-tip slot, alignment, a parent sharing a byte with a child it
 * reads), and per level pair that none of its three outputs shares a byte
 * with another of them or with one of its four leaves.  n == 0 or nops == 0:
 * nothing is launched and scaler_sums[0..nops) is zeroed. */
int plfx_traverse_psr(plfx_ctx *ctx, int dtype, const plfx_trav_op *ops, int nops, void *const *clv,
                      const uint8_t *const *tips, int nslots, const void *pmats, int npmats,
                      const void *EV, int64_t n, const uint8_t *rate_cat, int ncat, const int32_t *wgt,
                      uint8_t *const *scalers, int64_t *scaler_sums, const void *tipvec, void *stream);

/* lnL = sum_i wgt_i * log( sum_s freq[s] * x[i][s] )
 *       + (sum_{j<nsums} scaler_sums[j]) * log(2^-32)
 * x: the root's PSR CLV; the other arguments, the fixed-order reduction and
 * the capture rules are plfx_root_lnl's (freq NULL = 1/4 each; there are no
 * category weights: a site has one category). */
int plfx_root_lnl_psr(plfx_ctx *ctx, int dtype, const void *x, int64_t n, const double *freq,
                      const int32_t *wgt, const int64_t *scaler_sums, int nsums, double *out_lnl,
                      double *site_lnl, void *stream);

/* Section (10) for a PSR branch; the CLVs must be in the eigen convention as
 * there.  Sum table: sumtab[i][k] = x1[i][k] * x2[i][k], one multiply rounded
 * in dtype, n * 4 values; side 1 dense or coded (tipvec required with tip1),
 * alignment and overlap rules of plfx_edge_sumtable. */
int plfx_edge_sumtable_psr(plfx_ctx *ctx, int dtype, const uint8_t *tip1, const void *x1, const void *x2,
                           int64_t n, const void *tipvec, void *sumtab, void *stream);

/* out3 as plfx_edge_derivatives', in f64, with x_k = lambda_k * rates[c_i], e
 * = exp(x_k t), and L, L1, L2 = sum_k sumtab[i][k] * {e, e x, e x x}
 * (ascending k).  rates: device, ncat doubles; rate_cat, ncat as above
 * (PLFX_ERR_INVALID outside 1..PLFX_PSR_MAX_CATS); the factors are formed
 * from the device t once per thread block.  n == 0: out3 = {correction, 0, 0}.
 * Deterministic, asynchronous, capture-safe as plfx_edge_derivatives. */
int plfx_edge_derivatives_psr(plfx_ctx *ctx, int dtype, const void *sumtab, int64_t n, const double *eigen,
                              const double *rates, int ncat, const uint8_t *rate_cat, const int32_t *wgt,
                              const double *t, const int64_t *scaler_sums, int nsums, double *out3,
                              double *site_lnl, void *stream);

/* plfx_edge_optimize over plfx_edge_derivatives_psr: the same bracketed Newton
 * iteration, stop rules, argument rules and refusal of a capturing stream;
 * host-synchronous. */
int plfx_edge_optimize_psr(plfx_ctx *ctx, int dtype, const void *sumtab, int64_t n, const double *eigen,
                           const double *rates, int ncat, const uint8_t *rate_cat, const int32_t *wgt,
                           double t0, double tmin, double tmax, int max_evals, double *t_opt,
                           double *out3_host, int *evals, void *stream);

/* plfx_edge_optimize_dev for PSR branches: the contract of section (10)'s
 * device loop with the PSR arguments of plfx_edge_derivatives_psr.  sumtabs:
 * HOST array of nedges device PSR sum tables (n * 4 values of dtype each,
 * 16-byte aligned, none NULL; the pointers travel in the kernel arguments);
 * n, eigen, rates, ncat, rate_cat and wgt are shared by all edges.  t0
 * (device, read by the first launch, clamped into [tmin, tmax], a NaN starts
 * at tmin), t_opt, out3 and evals (device; the last two may be NULL) as
 * there.  Exactly max_evals launches per group of up to 32 edges, edge =
 * blockIdx.y, groups one after the other on the stream; asynchronous,
 * allocates nothing, legal on a capturing stream; the stream's workspace
 * regions are the ones plfx_edge_optimize_dev uses.  Every edge walks the t
 * sequence plfx_edge_optimize_psr walks from the same start, and a one-edge
 * call has plfx_edge_derivatives_psr's grid, slots and summation order, so
 * its t_opt, out3 and evals are plfx_edge_optimize_psr's bit for bit.  In a
 * group of `count` edges each edge gets at most 4096 / count blocks, so with
 * many edges of many sites the sums are formed in another (fixed) order.
 * Deterministic.  n == 0 is accepted (rate_cat may then be NULL): every edge
 * walks the host loop's sequence on the sums {0, 0, 0}.
 * PLFX_ERR_INVALID, before the first launch: what plfx_edge_derivatives_psr
 * refuses of dtype, ncat (outside 1..PLFX_PSR_MAX_CATS), n, eigen, rates,
 * rate_cat and each table; nedges < 1; a NULL sumtabs, t0 or t_opt; anything
 * but 0 < tmin <= tmax < infinity and 1 <= max_evals <= PLFX_EDGE_MAX_EVALS.
 * There is no PLFX_ERR_UNSUPPORTED case. */
int plfx_edge_optimize_psr_dev(plfx_ctx *ctx, int dtype, const void *const *sumtabs, int nedges,
                               int64_t n, const double *eigen, const double *rates, int ncat,
                               const uint8_t *rate_cat, const int32_t *wgt, const double *t0,
                               double tmin, double tmax, int max_evals, double *t_opt,
                               double *out3, int32_t *evals, void *stream);

/* One branch of plfx_edge_sumtable_psr_batch: exactly one of tip1 / x1 is
 * non-NULL.  All device pointers. */
typedef struct {
  const uint8_t *tip1; /* exactly one of tip1 / x1 */
  const void *x1;
  const void *x2;
  void *sumtab;
} plfx_psr_edge;

/* The sum tables of nedges >= 1 PSR branches sharing n and tipvec: edge j's
 * table is exactly what plfx_edge_sumtable_psr writes for the same arguments
 * (one multiply rounded in dtype, no other byte written).  `edges` is host
 * memory and travels in the kernel arguments: the edges with a dense side 1
 * first, then those with a coded one, each kind in the caller's order in
 * launches of up to 32 edges (edge = blockIdx.y).  Asynchronous, allocates
 * nothing, needs no workspace, capture-safe.  With plfx_edge_optimize_psr_dev
 * a batch of branches goes from CLVs to optima in 1-2 + max_evals launches
 * per 32 branches with no host wait.
 * Every check runs before the first launch (PLFX_ERR_INVALID, nothing is
 * launched): nedges < 1, a NULL edges, n < 0, a bad dtype; per edge the rules
 * of plfx_edge_sumtable_psr (both or neither of tip1 / x1, a NULL x2 or
 * sumtab, a dense side or a table not 16-byte aligned, a coded side with
 * tipvec NULL, a table sharing a byte with its own x1 / tip1 or x2); across
 * the call a table that shares a byte with another edge's table (the same
 * table listed twice included) or with any edge's input.  Inputs may repeat
 * freely: one CLV is an end of three branches.  n == 0 runs the call-level
 * checks only and launches nothing. */
int plfx_edge_sumtable_psr_batch(plfx_ctx *ctx, int dtype, const plfx_psr_edge *edges, int nedges,
                                 int64_t n, const void *tipvec, void *stream);

/* ---- (11b) per-site rate categories for protein: the likelihood half ------
 * (PROTCAT: the node, a whole traversal, the root lnL; extension).  The three
 * entry points below are their section-(11) namesakes with a `states`
 * argument, as plfx_plf_dev_gen stands beside plfx_plf_dev_f64: states == 4 is
 * section (11) itself (the same kernels, the same bits), states == 20 is the
 * protein path described here, any other value PLFX_ERR_UNSUPPORTED.  The
 * branch-length half (the protein versions of plfx_edge_*_psr) is section
 * (11c), the rate scan section (12b), the FMA mode on the f64 matrix cores
 * section (11d); an f32 FMA form of the protein node and rate scan does not
 * exist yet.
 * With 20 states a PSR CLV is x[site*20 + state] -- n * 20 values of dtype
 * (f32 or f64), a quarter of the Gamma protein layout, base 16-byte aligned;
 *   left, right: ncat * 400 values [c][k][l] -- what plfx_pmatrix(states = 20)
 *             writes per branch for `ncat` rates;
 *   rate_cat, the clamp c = min(rate_cat[i], ncat-1) and 1 <= ncat <=
 *             PLFX_PSR_MAX_CATS as in section (11).
 * Node update -- plf()'s loop with one category, run on each category's sites
 * with that category's matrices; no FMA contraction: the entry points of
 * this section run exact mode (section (11d) has the fused one):
 *   umpL[k]  = sum_l x1[i][l] * left[c*400 + k*20 + l]    from +0.0, ascending l
 *                                                         (same for right / x2)
 *   x3[i][l] = sum_k (umpL[k] * umpR[k]) * EV[20k + l]    from +0.0, ascending k
 * then, if all TWENTY |x3[i][.]| < 2^-32 (strict; NaN never scales), they are
 * multiplied by 2^32, scaler[i] = 1 and wgt[i] enters the node's scaler sum.
 * A coded child is as in section (8) protein: uint8 codes, row min(code, 23)
 * of a 24 x 20 table of dtype, tipvec NULL = the default table of section
 * (8); results are bit-identical to the dense computation on the expanded
 * child.
 *
 * SITE ORDER.  The kernel makes the category uniform across a wave of 64
 * consecutive sites by looping: a wave whose 64 sites share one category makes
 * one pass over its matrices, a wave with k distinct categories k passes.  The
 * results are the same bits for any order of the sites; the time is not: sort
 * the site patterns by category once, after plfx_psr_categorize (site patterns
 * are exchangeable: permute every tip's codes, wgt and rate_cat alike).
 * plfx_psr_site_order gives the permutation.  DESIGN.md section 3.8b has the
 * measured cost of unsorted sites. */

/* plfx_plf_psr_dev with a state count: the same plfx_psr_node array, checks
 * (all before the first launch; the overlap check uses n * states values per
 * CLV), n == 0 rule, launches of at most 32 nodes of one kind of children
 * (node = blockIdx.y, a ticket region each), asynchronous, allocates nothing,
 * descriptors in the kernel arguments, capture-safe.  tipvec: 16 x 4 values
 * (states 4) or 24 x 20 (states 20), or NULL. */
int plfx_plf_psr_dev_gen(plfx_ctx *ctx, int dtype, int states, const plfx_psr_node *nodes, int count,
                         const void *EV, int64_t n, const uint8_t *rate_cat, int ncat, const int32_t *wgt,
                         const void *tipvec, void *stream);

/* plfx_traverse_psr with a state count.  Op j's matrices are left = pmats +
 * (2*pmat) * ncat * states^2 and right = pmats + (2*pmat + 1) * ncat * states^2
 * values of dtype.  With states == 20 there is no fused level pair, whatever
 * PLFX_FUSE says: every level runs as batches by kind of children, and
 * plfx_traverse_schedule reports entry 4 = 0, entry 5 = nops, entry 6 = the
 * launches.  Every CLV, scaler byte and scaler_sums[j] is bit-identical to
 * the ops run one by one as one-node plfx_plf_psr_dev_gen calls. */
int plfx_traverse_psr_gen(plfx_ctx *ctx, int dtype, int states, const plfx_trav_op *ops, int nops,
                          void *const *clv, const uint8_t *const *tips, int nslots, const void *pmats,
                          int npmats, const void *EV, int64_t n, const uint8_t *rate_cat, int ncat,
                          const int32_t *wgt, uint8_t *const *scalers, int64_t *scaler_sums, const void *tipvec,
                          void *stream);

/* plfx_root_lnl_psr with a state count:
 *   lnL = sum_i wgt_i * log( sum_s freq[s] * x[i][s] )
 *         + (sum_{j<nsums} scaler_sums[j]) * log(2^-32)
 * over `states` values per site, in f64; freq NULL = 1/states each; site_lnl
 * optional; the fixed-order reduction and the rules of plfx_root_lnl_psr. */
int plfx_root_lnl_psr_gen(plfx_ctx *ctx, int dtype, int states, const void *x, int64_t n, const double *freq,
                          const int32_t *wgt, const int64_t *scaler_sums, int nsums, double *out_lnl,
                          double *site_lnl, void *stream);

/* Host only: perm[j] = the site that goes to position j when the n sites are
 * sorted by clamped category min(rate_cat[i], ncat-1), stably (sites of one
 * category keep their order) -- a counting sort.  rate_cat and perm are host
 * arrays of n entries.  PLFX_ERR_INVALID for a NULL pointer, n < 0 or ncat
 * outside 1..PLFX_PSR_MAX_CATS; n == 0 writes nothing. */
int plfx_psr_site_order(const uint8_t *rate_cat, int64_t n, int ncat, int64_t *perm);

/* ---- (11c) per-site rate categories for protein: the branch-length half ----
 * (PROTCAT: the sum table, one and batched, the edge derivatives and the two
 * Newton loops; extension).  The five entry points below are their
 * section-(11) namesakes with a `states` argument after dtype, as section
 * (11b)'s are: states == 4 is section (11) itself (the same launchers, the
 * same bits), states == 20 the protein path described here, any other value
 * PLFX_ERR_UNSUPPORTED.  The CLVs must be in the eigen convention, as in
 * section (10).  With 20 states a sum table is n * 20 values of dtype, 16-byte
 * aligned; tipvec is the 24 x 20 table of dtype a coded side indexes by
 * min(code, 23); eigen is what plfx_pmatrix(states = 20) takes, of which only
 * lambda[0..19] is read; rates, rate_cat, the clamp c_i = min(rate_cat[i],
 * ncat-1) and 1 <= ncat <= PLFX_PSR_MAX_CATS as in section (11).
 *
 * SITE ORDER.  Unlike the node of section (11b), the edge kernels make no pass
 * per category: a lane owns a site and reads its category's 60 factors from a
 * table in the block's local memory, whose rows are padded so that lanes in
 * different categories read different banks.  Every site's terms are the same
 * bits for any order of the sites, and so is the time: measured at 2^14, 2^18
 * and 2^20 f64 sites with 25 categories, uniformly random categories and
 * shuffled whole runs of 64 sites both take 0.98 to 1.00 of the sorted time
 * (DESIGN.md section 4).  Sorting the sites, which the node needs, does not
 * matter to the calls of this section. */

/* plfx_edge_sumtable_psr with a state count: sumtab[i][k] = x1[i][k] *
 * x2[i][k], one multiply rounded in dtype, n * states values.  Side 1 is dense
 * or coded; with states == 20 a coded side reads row min(code, 23) of the 24 x
 * 20 tipvec, which is required with tip1.  The 16-byte alignment and overlap
 * rules are plfx_edge_sumtable_psr's, the overlap check over n * states
 * values. */
int plfx_edge_sumtable_psr_gen(plfx_ctx *ctx, int dtype, int states, const uint8_t *tip1, const void *x1,
                               const void *x2, int64_t n, const void *tipvec, void *sumtab, void *stream);

/* plfx_edge_sumtable_psr_batch with a state count: the same plfx_psr_edge
 * array, dense-side edges first, then coded ones, in launches of up to 32 with
 * edge = blockIdx.y; each table is exactly what the one-edge call writes.
 * Every check runs before the first launch; the byte-overlap sweep across the
 * edges spans n * states values per CLV and table. */
int plfx_edge_sumtable_psr_batch_gen(plfx_ctx *ctx, int dtype, int states, const plfx_psr_edge *edges,
                                     int nedges, int64_t n, const void *tipvec, void *stream);

/* plfx_edge_derivatives_psr with a state count: out3 as there, in f64, with
 * x_k = lambda_k * rates[c_i], e = exp(x_k t), and L, L1, L2 = sum_k
 * sumtab[i][k] * {e, e x, e x x} over k = 0..states-1, from +0.0, ascending k.
 * site_lnl, wgt, scaler_sums and n == 0 (out3 = {correction, 0, 0}) as in
 * section (11); the fixed-order reduction: deterministic, asynchronous,
 * capture-safe. */
int plfx_edge_derivatives_psr_gen(plfx_ctx *ctx, int dtype, int states, const void *sumtab, int64_t n,
                                  const double *eigen, const double *rates, int ncat, const uint8_t *rate_cat,
                                  const int32_t *wgt, const double *t, const int64_t *scaler_sums, int nsums,
                                  double *out3, double *site_lnl, void *stream);

/* plfx_edge_optimize_psr over plfx_edge_derivatives_psr_gen: host-synchronous,
 * refuses a capturing stream. */
int plfx_edge_optimize_psr_gen(plfx_ctx *ctx, int dtype, int states, const void *sumtab, int64_t n,
                               const double *eigen, const double *rates, int ncat, const uint8_t *rate_cat,
                               const int32_t *wgt, double t0, double tmin, double tmax, int max_evals,
                               double *t_opt, double *out3_host, int *evals, void *stream);

/* plfx_edge_optimize_psr_dev with a state count: the same contract -- exactly
 * max_evals launches per group of up to 32 edges, the same workspace regions,
 * at most 4096 / count blocks per edge of a group; a one-edge call has
 * plfx_edge_derivatives_psr_gen's grid, slots and summation order, so its
 * t_opt, out3 and evals are plfx_edge_optimize_psr_gen's bit for bit. */
int plfx_edge_optimize_psr_dev_gen(plfx_ctx *ctx, int dtype, int states, const void *const *sumtabs, int nedges,
                                   int64_t n, const double *eigen, const double *rates, int ncat,
                                   const uint8_t *rate_cat, const int32_t *wgt, const double *t0, double tmin,
                                   double tmax, int max_evals, double *t_opt, double *out3, int32_t *evals,
                                   void *stream);

/* ---- (12) the PSR rate scan and rate categorisation (extension) -----------
 * Section (11) takes rate_cat and the category rates as inputs; this section
 * produces them, as RAxML / ExaML do for GTRCAT: every site gets the rate it
 * likes best on the current tree out of a grid of candidates, and the chosen
 * rates are binned into at most max_cats categories.
 *
 * Per-site lnL with the site's own scaling correction:
 *   L_i    = sum_s freq[s] * x[i][s]                (plfx_root_lnl_psr's L_i)
 *   cnt_i  = number of j < nsc with scalers[j*stride + i] != 0
 *   site_lnl[i] = log(L_i) + cnt_i * log(2^-32)     (one multiply, one add)
 * x: a PSR CLV (n * 4 values of dtype, 16-byte aligned), freq: device, 4
 * doubles or NULL (1/4 each).  scalers: ONE device block holding nsc scaler
 * rows, row j at scalers + j*stride bytes (stride >= n): point
 * plfx_traverse_psr's scalers[j] into it.  nsc == 0 (scalers may be NULL)
 * gives plfx_root_lnl_psr's site_lnl bit for bit.  Asynchronous, no
 * workspace, capture-safe.  PLFX_ERR_INVALID before any launch: a bad dtype,
 * n < 0, a NULL or misaligned x, a NULL site_lnl, nsc < 0, nsc > 0 with NULL
 * scalers, stride < n.  n == 0 launches nothing. */
int plfx_site_lnl_psr(plfx_ctx *ctx, int dtype, const void *x, int64_t n, const double *freq,
                      const uint8_t *scalers, int nsc, int64_t stride, double *site_lnl, void *stream);

/* The rate scan: for each of ncand candidate rates r_k, the per-site lnL of
 * the whole tree with EVERY site at rate r_k; per site the best candidate.
 *   all_lnl[k*n + i] = lnL of site i under r_k (scaling correction included)
 *   best_idx[i] = the k of the largest all_lnl[k*n + i] (ties: the lowest k;
 *                 a NaN never wins; all NaN: 0), best_lnl[i] = that value
 *                 (-inf if none won), out_lnl = sum_i wgt_i * best_lnl[i]
 *                 (plfx_root_lnl's fixed-order reduction).
 * ops, tips, nslots (HOST arrays) as in plfx_traverse_psr; the root is the
 * parent of the last op.  Every slot an op reads must be a coded tip
 * (tips[s] != NULL) or the parent of an earlier op: a dense leaf gives
 * PLFX_ERR_UNSUPPORTED.  blen: device, 2*npmats doubles, branches 2m and 2m+1
 * of pair m; eigen as plfx_pmatrix; EV, tipvec (required) in the eigen
 * convention; freq: device root weights (4 doubles, plfx_model_root_weights
 * in the eigen convention) or NULL; cand_rates: device, ncand doubles, 1 <=
 * ncand <= PLFX_PSR_SCAN_MAX_RATES; wgt: device int32[n] or NULL (used for
 * out_lnl only).  Outputs, all device: best_idx int32[n], best_lnl double[n],
 * all_lnl double[ncand*n] or NULL, out_lnl one double or NULL.
 * Mechanism: `group` (1..PLFX_PSR_MAX_CATS) candidates are evaluated per
 * traversal, as the categories of a "virtual alignment" of group*n sites
 * (virtual site g*n + i = site i under candidate g).  The tip codes and the
 * category bytes are tiled once; then per pass of gc = min(group, candidates
 * left): plfx_pmatrix (EIGEN, ncat = gc) into the workspace, the
 * plfx_traverse_psr launches over gc*n virtual sites with every op's scaler
 * row, and one kernel that forms the per-site lnL and updates the running
 * best.  group sizes the workspace and the launches and nothing else: every
 * output has the same bits for every group and for either PLFX_FUSE setting,
 * and row k of all_lnl is what plfx_traverse_psr (rate_cat all k) +
 * plfx_site_lnl_psr give.
 * workspace: one device block, 256-byte aligned, of at least
 * plfx_psr_rate_scan_workspace(dtype, nops, ntips, npmats, n, group) bytes,
 * ntips the number of non-NULL tips[]; its contents are scratch.
 * Asynchronous, allocates nothing, legal on a capturing stream under
 * plfx_root_lnl_psr's workspace rules.  Every check runs before the first
 * launch: the op-list checks of plfx_traverse_psr, the ranges above, NULL
 * pointers, the workspace's alignment and size (PLFX_ERR_INVALID).  n == 0
 * launches nothing and zeroes out_lnl if given. */
#define PLFX_PSR_SCAN_MAX_RATES 1024
int plfx_psr_rate_scan(plfx_ctx *ctx, int dtype, const plfx_trav_op *ops, int nops,
                       const uint8_t *const *tips, int nslots, const double *blen, int npmats,
                       const double *eigen, const void *EV, const void *tipvec, const double *cand_rates,
                       int ncand, int group, const double *freq, const int32_t *wgt, int64_t n,
                       void *workspace, size_t workspace_bytes, int32_t *best_idx, double *best_lnl,
                       double *all_lnl, double *out_lnl, void *stream);

/* Host only.  *bytes = the size of the scan's workspace, the sum of these
 * parts, each array rounded up to 256 bytes: nops CLVs of group*n*4 values of
 * dtype, ntips code arrays of group*n bytes, nops scaler rows of group*n
 * bytes, group*n category bytes, 2*npmats*group*16 matrix values.
 * PLFX_ERR_INVALID for a bad dtype, a negative count or n, group outside
 * 1..PLFX_PSR_MAX_CATS or a NULL bytes. */
int plfx_psr_rate_scan_workspace(int dtype, int nops, int ntips, int npmats, int64_t n, int group,
                                 size_t *bytes);

/* Host only, no context: from the scan's best_idx to rate_cat and the category
 * rates.  w_i = wgt ? wgt[i] : 1; W_k = the sum of w_i over the sites with
 * best_idx[i] == k; used = the candidates some site chose (a site of weight 0
 * counts).  kept = used if it has at most max_cats members, else its max_cats
 * members of largest W_k (ties: the lower k).  Categories are numbered by
 * ascending cand_rates[k] over kept (ties: by k).  A site whose candidate is
 * kept gets that category; any other site the kept category whose rate is
 * nearest to its candidate's, |cand_rates[best_idx[i]] - cand_rates[kept]|
 * (ties: the lower category).  *scale = (sum_i w_i) / (sum_i w_i * rate_i),
 * both sums in f64 in site order, and cat_rates[c] = cand_rates[kept_c] *
 * *scale: the weighted mean rate is 1.  rate_cat: uint8[n]; cat_rates:
 * max_cats doubles, entries from *ncat on are not written.
 * PLFX_ERR_INVALID (nothing written): a NULL pointer other than wgt, n < 1,
 * ncand < 1, max_cats outside 1..PLFX_PSR_MAX_CATS, an index outside [0,
 * ncand), a candidate that is not finite and > 0, a negative weight, a weight
 * sum of 0.  Deterministic. */
int plfx_psr_categorize(const double *cand_rates, int ncand, const int32_t *best_idx, const int32_t *wgt,
                        int64_t n, int max_cats, uint8_t *rate_cat, double *cat_rates, int *ncat,
                        double *scale);

/* ---- (12b) the rate scan with a state count (PROTCAT; extension) -----------
 * The three entry points below are their section-(12) namesakes with a
 * `states` argument after dtype (the workspace query has no ctx: dtype comes
 * first there, then states), as sections (11b) and (11c) do it: states == 4
 * is section (12) itself -- one
 * code path, the same launchers, the same bits --, states == 20 the protein
 * path described here, any other value PLFX_ERR_UNSUPPORTED.  What the scan
 * produces feeds plfx_psr_categorize, plfx_psr_site_order and then every call
 * of sections (11b) and (11c). */

/* plfx_site_lnl_psr with a state count: x holds n * states values of dtype
 * (16-byte aligned), freq `states` doubles or NULL (1/states each);
 *   L_i = sum_s freq[s] * x[i][s]      from +0.0, ascending s, in f64
 *   site_lnl[i] = log(L_i) + cnt_i * log(2^-32)        one multiply, one add
 * with cnt_i over the nsc scaler rows as in section (12).  With nsc == 0 it
 * gives plfx_root_lnl_psr_gen's site_lnl bit for bit.  The checks and the
 * n == 0 rule are plfx_site_lnl_psr's. */
int plfx_site_lnl_psr_gen(plfx_ctx *ctx, int dtype, int states, const void *x, int64_t n, const double *freq,
                          const uint8_t *scalers, int nsc, int64_t stride, double *site_lnl, void *stream);

/* plfx_psr_rate_scan with a state count.  With states == 20: eigen is what
 * plfx_pmatrix(states = 20) takes, EV holds 400 values of dtype, tipvec
 * (required) is a 24 x 20 table of dtype in the eigen convention, freq holds
 * 20 root weights or is NULL (1/20 each), and the tips are protein codes (row
 * min(code, 23)).  The outputs, the tie and NaN rules (strict >: ties keep the
 * lower k, a NaN never wins, all NaN gives best_idx 0 and best_lnl -inf) and
 * out_lnl's fixed-order reduction are section (12)'s.  The mechanism too: the
 * codes and category bytes tiled once, then per pass plfx_pmatrix (EIGEN,
 * states, ncat = gc), the plfx_traverse_psr_gen launches over gc * n virtual
 * sites -- which arrive sorted by category by construction, the order the
 * protein node kernel is fast in; with 20 states no level pair is fused,
 * whatever PLFX_FUSE says -- and one kernel for the per-site lnL and the
 * running best.  Row k of all_lnl is bit for bit what plfx_traverse_psr_gen
 * (rate_cat all k) followed by plfx_site_lnl_psr_gen gives, and every output
 * has the same bits for every group.  workspace: at least
 * plfx_psr_rate_scan_workspace_gen(dtype, states, ...) bytes, 256-byte
 * aligned: one sized for 4 states is refused for 20.  Asynchronous, allocates
 * nothing, capture-safe; every check runs before the first launch, with
 * section (12)'s codes. */
int plfx_psr_rate_scan_gen(plfx_ctx *ctx, int dtype, int states, const plfx_trav_op *ops, int nops,
                           const uint8_t *const *tips, int nslots, const double *blen, int npmats,
                           const double *eigen, const void *EV, const void *tipvec, const double *cand_rates,
                           int ncand, int group, const double *freq, const int32_t *wgt, int64_t n,
                           void *workspace, size_t workspace_bytes, int32_t *best_idx, double *best_lnl,
                           double *all_lnl, double *out_lnl, void *stream);

/* Host only.  *bytes = section (12)'s formula with `states` in place of 4 and
 * states^2 in place of 16, each array rounded up to 256 bytes: nops CLVs of
 * group*n*states values of dtype, ntips + nops + 1 rows of group*n bytes (the
 * code arrays, the scaler rows, the category bytes), 2*npmats*group*states^2
 * matrix values.  With 20 states the CLVs are five times the DNA size and
 * they are nearly all of it: `group` is what sizes the workspace -- choose it
 * to fit, the results do not depend on it.  PLFX_ERR_UNSUPPORTED for states
 * other than 4 and 20; PLFX_ERR_INVALID as plfx_psr_rate_scan_workspace. */
int plfx_psr_rate_scan_workspace_gen(int dtype, int states, int nops, int ntips, int npmats, int64_t n, int group,
                                     size_t *bytes);

/* ---- (11d) PROTCAT FMA mode: the protein PSR node on the f64 matrix cores ----
 * (extension).  The three entry points below are their _gen namesakes of
 * sections (11b) and (12b) with an `int flags` argument after states, named
 * like plfx_ctx_create_ex.  flags: 0 or PLFX_FMA; any other bit is
 * PLFX_ERR_INVALID.  flags == 0 is the _gen call -- one code path, the same
 * bits.  states == 4 is section (11) / (12) bit for bit whatever the flag
 * (DNA is always exact).  states == 20 with PLFX_FMA and dtype f32 is
 * PLFX_ERR_UNSUPPORTED (not built); PLFX_VALU is not a flag of these calls.
 *
 * FMA mode for a protein PSR node is plf()'s loop with one category, run on
 * each category's sites with that category's matrices, every multiply-add
 * fused, in the order of the Gamma PLFX_FMA mode of section (2b).  With
 * c = min(rate_cat[i], ncat-1):
 *   umpL[k]  : u = +0.0; for l = 0..19 ascending: u = fma(x1[i][l], left[c*400 + 20k + l], u)
 *                                                         (same for right / x2)
 *   p[k]     = umpL[k] * umpR[k]                          one rounding
 *   x3[i][l] : a = +0.0; for k = 0..19 ascending: a = fma(p[k], EV[20k + l], a)
 * The scale rule is section (11b)'s unchanged: all twenty |x3| < 2^-32 strict,
 * NaN never scales, x 2^32, scaler byte, wgt into the node's sum.  A coded
 * child is the row min(code, 23) of the 24 x 20 tip table put through the
 * same arithmetic: bit-identical to the dense call on the expanded child;
 * there is no (category, code) table.  On random inputs the values differ in
 * bits from exact mode on about three quarters of the entries and agree to
 * about 6e-13 relative.
 *
 * The kernel (csrc/plf_psr_prot_mfma.hpp) makes the category uniform across a
 * wave of 64 consecutive sites by looping, as the exact one does: the same
 * bits for any order of the sites, and section (11b)'s SITE ORDER paragraph
 * holds -- sort the sites by category.  plfx_root_lnl_psr_gen,
 * plfx_site_lnl_psr_gen and all of section (11c) do not depend on the mode.
 *
 * Every other check, the n == 0 rule, "every check before the first launch, a
 * refused call enqueues nothing", asynchrony, no allocation and capture safety
 * are as in the _gen calls. */

/* plfx_plf_psr_dev_gen with flags. */
int plfx_plf_psr_dev_ex(plfx_ctx *ctx, int dtype, int states, int flags, const plfx_psr_node *nodes, int count,
                        const void *EV, int64_t n, const uint8_t *rate_cat, int ncat, const int32_t *wgt,
                        const void *tipvec, void *stream);

/* plfx_traverse_psr_gen with flags: the launch list is the exact call's, only
 * the node kernel differs.  Every CLV, scaler byte and scaler_sums[j] is
 * bit-identical to the ops run one by one as one-node plfx_plf_psr_dev_ex
 * calls with the same flags.  There is no level pair for 20 states. */
int plfx_traverse_psr_ex(plfx_ctx *ctx, int dtype, int states, int flags, const plfx_trav_op *ops, int nops,
                         void *const *clv, const uint8_t *const *tips, int nslots, const void *pmats, int npmats,
                         const void *EV, int64_t n, const uint8_t *rate_cat, int ncat, const int32_t *wgt,
                         uint8_t *const *scalers, int64_t *scaler_sums, const void *tipvec, void *stream);

/* plfx_psr_rate_scan_gen with flags: the same workspace
 * (plfx_psr_rate_scan_workspace_gen), passes and outputs, every pass's
 * traversal in the mode of flags.  The same bits for every group; equal bit
 * for bit to the per-candidate composition plfx_pmatrix + plfx_traverse_psr_ex
 * (same flags) + plfx_root_lnl_psr_gen / plfx_site_lnl_psr_gen. */
int plfx_psr_rate_scan_ex(plfx_ctx *ctx, int dtype, int states, int flags, const plfx_trav_op *ops, int nops,
                          const uint8_t *const *tips, int nslots, const double *blen, int npmats,
                          const double *eigen, const void *EV, const void *tipvec, const double *cand_rates,
                          int ncand, int group, const double *freq, const int32_t *wgt, int64_t n, void *workspace,
                          size_t workspace_bytes, int32_t *best_idx, double *best_lnl, double *all_lnl,
                          double *out_lnl, void *stream);

/* ---- (13) all-branch derivatives of a PSR tree: outer CLVs and the sum table
 * of every branch in one call (extension) -------------------------------------
 * Sections (11) / (11c) differentiate the one branch between two CLVs the
 * caller holds, and a traversal only makes post-order CLVs: the branch the
 * tree is rooted on.  This section makes, for EVERY branch, the CLV of
 * everything outside the subtree below it and the branch's sum table, ready
 * for plfx_edge_optimize_psr_dev_gen / plfx_edge_derivatives_psr_gen.
 *
 * INPUT.  A post-order op list ops[0..nops) of ONE rooted binary tree after
 * plfx_traverse_psr_ex has run on it with the same ops, clv, tips, nslots,
 * pmats, npmats, EV, n, rate_cat, ncat, wgt and tipvec: clv[] and
 * scaler_sums[0..nops) are inputs here, and no byte of clv[] is written.
 * The CLVs must be in the eigen convention of section (10).
 *
 * TREE RULES (else PLFX_ERR_INVALID): every parent slot is written once; every
 * written slot but the last op's parent is read by exactly one later op; no
 * slot is read twice; the last op is the root op; a slot that no op writes is
 * a tip, dense (clv[slot]) or coded (tips[slot]), and only read; the root
 * op's two children are not both coded tips.
 *
 * EDGES.  Edge e = 2*j + s is the branch of op j to its child s (0 = child1 /
 * left, 1 = child2 / right); its length is the one blen[2*ops[j].pmat + s]
 * that made the op's matrix.  The root op's two branches are ONE edge of the
 * summed length: both of its entries carry the same table and the same count.
 *
 * OUTER CLV W(c), for a child c of op j: the PSR CLV of everything outside
 * c's subtree, located at c's parent node.
 *   root op (r, a, b):  W(a) is slot b itself and W(b) slot a; nothing is copied.
 *   op j = (v, c1, c2): W(c1) = node(x1 = W(v), left = Pup(v), x2 = slot c2, right = op j's right matrix)
 *                       W(c2) = node(x1 = W(v), left = Pup(v), x2 = slot c1, right = op j's left matrix)
 *   Pup(v) is the matrix of v's branch in the op that reads v -- or, when that
 *   op is the root op, root_pmat: ncat * states^2 values the caller makes with
 *   plfx_pmatrix for the joined root length (both root branches summed).
 * Each W is bit for bit what a one-node plfx_plf_psr_dev_ex call with those
 * arguments and the call's flags writes, the 2^-32 rescale and the node's
 * weighted scaler sum included.
 *
 * SUM TABLE of edge e to child c: plfx_edge_sumtable_psr_gen(side 1 = slot c,
 * dense or coded; x2 = W(c)) bit for bit; the root edge is x_a * x_b with a
 * coded child as side 1.  A coded tip anywhere needs tipvec.
 *
 * edge_scale[e] (device int64[2*nops], may be NULL): the scaler count of edge
 * e's lnL -- scaler_sums over c's subtree, the sums of every W on the way up
 * (W(c)'s own, W(v)'s, ...) and scaler_sums of the sibling subtrees hanging
 * off that path: lnL(e) = out3[0] + edge_scale[e] * log(2^-32).  Integer sums,
 * formed on the device.  NULL: no count is formed, scaler_sums is not read.
 *
 * SCHEDULE.  The ops are levelled by depth from the root op; level by level,
 * an op with 4 states and a dense W(v) runs as ONE fused sibling-pair launch
 * (up to 16 ops each) that reads W(v) and both children once and writes both
 * W and both tables; every other op (20 states; PLFX_BRANCH_NOFUSE; W(v) a
 * coded tip, which happens only under a root child whose sibling is coded) as
 * plfx_plf_psr_dev_ex batches followed by plfx_edge_sumtable_psr_batch_gen
 * launches.  The W of a coded child exists only for its table: unfused it has
 * a slab of the workspace, fused it is never written.  Results are the same
 * bits whatever the schedule.
 *
 * flags: 0, PLFX_FMA (20 states: the W nodes in the mode plfx_traverse_psr_ex
 * runs them in; refused as there), PLFX_BRANCH_NOFUSE; any other bit is
 * PLFX_ERR_INVALID.  states: 4 or 20, else PLFX_ERR_UNSUPPORTED.
 *
 * The workspace (device, 256-byte aligned, >= plfx_branch_sumtables_psr_workspace
 * bytes) holds slabs of slab = n * states * sizeof(dtype) rounded up to 256
 * bytes: W of edge e < 2*(nops-1) at byte e * slab (readable after the call;
 * a coded child's is scratch or untouched), then the 2*nops - 1 tables, then
 * the counters, int64: the weighted scaler sum of W of edge e at counter e,
 * written when edge_scale is given.  It must share no byte with a slot.
 * sumtabs_out: HOST array of 2*nops device pointers into the workspace, filled
 * before the call returns.  Asynchronous, allocates nothing, descriptors in
 * the kernel arguments, capture-safe.  Every check runs before the first
 * launch: a refused call enqueues nothing and leaves sumtabs_out as it was.
 * n == 0: nothing is launched and edge_scale is zeroed.  After branch lengths
 * change the caller re-runs the traversal and this call. */
#define PLFX_BRANCH_NOFUSE 4

int plfx_branch_sumtables_psr_workspace(int dtype, int states, int nops, int64_t n, size_t *bytes);

int plfx_branch_sumtables_psr(plfx_ctx *ctx, int dtype, int states, int flags, const plfx_trav_op *ops, int nops,
                              void *const *clv, const uint8_t *const *tips, int nslots, const void *pmats,
                              int npmats, const void *root_pmat, const void *EV, int64_t n,
                              const uint8_t *rate_cat, int ncat, const int32_t *wgt, const int64_t *scaler_sums,
                              const void *tipvec, void *workspace, size_t workspace_bytes, void **sumtabs_out,
                              int64_t *edge_scale, void *stream);

/* Sites per lane and trip of the fused sibling-pair kernel (dtype PLFX_F32 /
 * PLFX_F64; 0 for anything else): a block covers 256 times as many sites. */
int plfx_branch_pair_sites_per_lane(int dtype);

#ifdef __cplusplus
} /* extern "C" */
#endif

#endif /* PLFX_H */
