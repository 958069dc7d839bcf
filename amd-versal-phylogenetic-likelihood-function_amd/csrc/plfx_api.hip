// plfx_api.hip -- the C ABI of include/plfx.h over the HIP kernels.
//
// Replaces the reference host's XRT layer (app/src/host_mem.cpp:108-157
// kernel/bo/run setup, :283-394 run loop) and its CPU entry point plf()
// (app/src/plf.h:1-5).  No C++ exception crosses this boundary; every entry
// point returns a plfx_status.
#include <hip/hip_runtime.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <algorithm>
#include <new>
#include <string>
#include <mutex>
#include <vector>

#include "../../include/plfx.h"
#include "edge_newton.hpp"
#include "plf_kernels.hpp"
#include "branch_plan.hpp"
#include "psr_edge_lower.hpp"
#include "psr_lower.hpp"
#include "psr_scan_lower.hpp"
#include "stream_ws.hpp"
#include "testbench.hpp"
#include "trav_lower.hpp"
#include "trav_plan.hpp"

constexpr int kHostChunksMax = 16;

// The per-stream reduction workspaces (stream_ws.hpp: who holds which entry
// and when it may change hands) are allocated here: kWsPool entries with the
// context, further ones stream-ordered on the stream that needs one.
// plfx_ctx_destroy never touches a caller's stream handle (the stream may be
// gone by then): an entry still held by a stream other than the context's is
// waited for device-wide.  (An event recorded after each call cannot stand
// in: HIP rejects waiting on an event whose stream was destroyed -- an exited
// thread's hipStreamPerThread gave hipErrorCapturedEvent (907) on the box.)
using plfx::StreamWs;
using plfx::aligned16;
using plfx::clv_bytes_of;
using plfx::overlap;
constexpr int kWsPool = PLFX_WS_POOL;

struct plfx_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  int max_blocks = 0;               // grid cap for the grid-stride kernels (0 = resident blocks)
  int node_segments = -1;           // node kernels' XCD-segmented mapping: -1 by size, 0 off, 1 on
                                    // (PLFX_NODE_SEGMENTS; plf_kernels.hip segment_grid)
  int streams = 1;                  // one-node calls kept in flight (plfx_ctx_set_streams, PLFX_STREAMS)
  int fuse = 3;  // traverse: 3 six-level subtrees before 2's, 2 three-level subtrees +
                 // level pairs, 1 level pairs, 0 none (PLFX_FUSE)
  int psr_fuse = 0;  // traverse_psr: >= 1 level pairs, 0 none.  PLFX_FUSE when it is set; unset means 0 here
                     // (level pairs lose at 2^14 sites), not `fuse`'s default
  bool lazy_tables = false;         // PLFX_CTX_LAZY_TABLES
  plfx::WsPool wss{hipStreamPerThread};  // per-stream workspaces
  std::vector<void *> ws_blocks;    // their allocations (the pool's, then one per extra entry)
  uint8_t *tt_codes = nullptr;      // the tip/tip tables' two constant 576-code arrays (kTtCodeBytes)
  double *edge_buf = nullptr;       // plfx_edge_optimize: the trial t and the three results (kEdgeBufBytes)
  int sched[PLFX_SCHED_COUNTS] = {};  // schedule of the last traverse
  plfx::LaunchList lowered;         // the launches of the call in progress (kept for its capacity)
  plfx::PsrLaunchList psr_lowered;  // the same for plfx_plf_psr_dev and plfx_traverse_psr
  plfx::PsrEdgeLaunchList psr_edges_lowered;  // and for plfx_edge_sumtable_psr_batch
  plfx::PsrScanPlan psr_scan;       // and for plfx_psr_rate_scan
  plfx::BranchPlan branches;        // and for plfx_branch_sumtables_psr
  // grow-only staging for the synchronous host entry points
  void *d_buf = nullptr;
  size_t d_cap = 0;
  // host entry pipelining: D2H of chunk i on its own stream while chunk i+1 uploads
  hipStream_t d2h_stream = nullptr;
  hipEvent_t chunk_done[kHostChunksMax] = {};
  std::string err;
  // calls on one context from several host threads are serialised (recursive:
  // entry points call each other, e.g. instance_run_host -> instance_run)
  mutable std::recursive_mutex mu;
};

namespace {

// Every entry point runs with the context's device current and gives the
// caller's current device back (hipSetDevice is per host thread).
struct DeviceGuard {
  int prev = -1;
  explicit DeviceGuard(int dev) {
    if (hipGetDevice(&prev) != hipSuccess) prev = -1;
    if (prev != dev) (void)hipSetDevice(dev);
    else prev = -1;  // nothing to restore
  }
  ~DeviceGuard() {
    if (prev >= 0) (void)hipSetDevice(prev);
  }
  DeviceGuard(const DeviceGuard &) = delete;
  DeviceGuard &operator=(const DeviceGuard &) = delete;
};

#define PLFX_BIND(ctx)                                              \
  if (!(ctx)) return PLFX_ERR_INVALID;                              \
  std::lock_guard<std::recursive_mutex> plfx_lock_((ctx)->mu);      \
  DeviceGuard plfx_guard_((ctx)->device)

constexpr size_t kWsRegions = std::max({(size_t)plfx::kMaxBatch, (size_t)7 * plfx::kMaxSeptets,
                                        (size_t)plfx::kDeepNodes, (size_t)plfx::kDeepQueueRegion + 1});
constexpr size_t kWsBytes = kWsRegions * plfx::kWsWords * sizeof(unsigned long long);
// three accumulators per block (the edge derivatives; the root lnL uses the first kLnlMaxGrid)
constexpr size_t kLnlPartialBytes = 3 * (size_t)plfx::kLnlMaxGrid * sizeof(double);
constexpr size_t kEdgeBufBytes = 4 * sizeof(double);
constexpr size_t kLnlTicketBytes = plfx::kWsWords * sizeof(unsigned long long);
// plfx_edge_optimize_dev: the stepper state of each edge of a launch group
constexpr size_t kEdgeStateRegionBytes = (size_t)plfx::kMaxBatch * plfx::kEdgeStateBytes;

int fail(plfx_ctx *ctx, int code, const char *fmt, ...) {
  if (ctx) {
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    ctx->err = buf;
  }
  return code;
}

int hip_fail(plfx_ctx *ctx, hipError_t e, const char *what) {
  return fail(ctx, PLFX_ERR_HIP, "%s: %s (%d)", what, hipGetErrorString(e), (int)e);
}

#define PLFX_HIP(ctx, call)                          \
  do {                                               \
    hipError_t e_ = (call);                          \
    if (e_ != hipSuccess) return hip_fail(ctx, e_, #call); \
  } while (0)

int check_dtype(plfx_ctx *ctx, int dtype) {
  if (dtype != PLFX_F32 && dtype != PLFX_F64) return fail(ctx, PLFX_ERR_INVALID, "bad dtype %d", dtype);
  return PLFX_OK;
}

// NULL is the HIP null stream, as in every HIP API; pass plfx_ctx_stream(ctx)
// to run on the context's own stream.
hipStream_t pick(void *stream) { return reinterpret_cast<hipStream_t>(stream); }

constexpr size_t kWsEntryBytes = kWsBytes + kLnlPartialBytes + kLnlTicketBytes + kEdgeStateRegionBytes;

// Tip/tip protein combination tables (plf_prot.hpp prot_tiptip_gather_kernel):
// per node of a launch group, a 576 x 80 table of the node's dtype and 576
// scaler bytes, in every workspace entry (written by the table kernel before
// each use, so never zeroed), and the two constant 576-code arrays (combo
// k = code1 * 24 + code2) once per context.  Allocated with the entries, so
// a stream's first tip/tip call -- also inside a capture -- takes the tables;
// under PLFX_CTX_LAZY_TABLES they are allocated on an entry's first tip/tip
// call instead, and that first call is refused (PLFX_ERR_INVALID) inside a
// capture.
constexpr size_t kTtCodeBytes = 2048;
constexpr size_t kTtEntryBytes = (size_t)plfx::kMaxBatch * (plfx::kTtTabBytes + plfx::kTtScBytes);

bool capturing(hipStream_t s) {
  hipStreamCaptureStatus cap = hipStreamCaptureStatusNone;
  return s && hipStreamIsCapturing(s, &cap) == hipSuccess && cap != hipStreamCaptureStatusNone;
}

// Threads that took a hipStreamPerThread workspace of a live context: when
// such a thread exits without releasing it, its entry is retired (its stream
// is gone with the thread, so nothing may wait on it) and reclaimed, after a
// device synchronisation, when the context runs out of entries.
std::mutex g_live_mu;
std::vector<plfx_ctx *> g_live;  // contexts not yet destroyed

// the calling thread's id for the workspace pool: an address of its own
thread_local char t_tag;

struct PerThreadEntries {
  std::vector<plfx_ctx *> ctxs;
  ~PerThreadEntries() {
    std::lock_guard<std::mutex> l(g_live_mu);
    for (plfx_ctx *c : ctxs)
      if (std::find(g_live.begin(), g_live.end(), c) != g_live.end()) {
        std::lock_guard<std::recursive_mutex> lock(c->mu);
        c->wss.orphan(&t_tag);
      }
  }
};
thread_local PerThreadEntries t_entries;

void ws_carve(StreamWs &w, void *base, void *tt) {
  char *b = static_cast<char *>(base);
  w.ws = reinterpret_cast<unsigned long long *>(b);
  w.lnl_partials = reinterpret_cast<double *>(b + kWsBytes);
  w.lnl_ticket = reinterpret_cast<unsigned long long *>(b + kWsBytes + kLnlPartialBytes);
  w.edge_state = b + kWsBytes + kLnlPartialBytes + kLnlTicketBytes;
  w.tt = static_cast<char *>(tt);
}

// A further entry, allocated and zeroed stream-ordered on s: usable by s's
// next launch with no host wait (and freed stream-ordered at destroy, which a
// plain hipFree would turn into a wait for the whole device)
int ws_allocate(plfx_ctx *ctx, hipStream_t s) {
  void *block = nullptr;
  const size_t bytes = kWsEntryBytes + (ctx->lazy_tables ? 0 : kTtEntryBytes);
  hipError_t e = hipMallocAsync(&block, bytes, s);
  if (e != hipSuccess)
    return fail(ctx, PLFX_ERR_NOMEM, "workspace hipMallocAsync(%zu): %s", bytes, hipGetErrorString(e));
  e = hipMemsetAsync(block, 0, kWsEntryBytes, s);
  if (e != hipSuccess) {
    (void)hipFreeAsync(block, s);
    return hip_fail(ctx, e, "workspace memset");
  }
  ctx->ws_blocks.push_back(block);
  StreamWs w;
  ws_carve(w, block, ctx->lazy_tables ? nullptr : static_cast<char *>(block) + kWsEntryBytes);
  ctx->wss.add(w);
  return PLFX_OK;
}

// The workspace of stream s: its own, else a free pool entry (zero at rest),
// else a retired per-thread entry reclaimed after a device synchronisation,
// else a new allocation -- neither of the last two inside a stream capture
// (WsPool::acquire decides).  A hipStreamPerThread entry is remembered by the
// thread that takes it (retired at its exit).
StreamWs *ws_for(plfx_ctx *ctx, hipStream_t s, int *rc) {
  *rc = PLFX_OK;
  const bool cap = capturing(s);
  for (;;) {
    const plfx::WsPool::Acquired a = ctx->wss.acquire(s, &t_tag, cap);
    switch (a.answer) {
      case plfx::WsPool::kTaken:
        if (s == hipStreamPerThread &&
            std::find(t_entries.ctxs.begin(), t_entries.ctxs.end(), ctx) == t_entries.ctxs.end())
          t_entries.ctxs.push_back(ctx);
        [[fallthrough]];
      case plfx::WsPool::kHeld:
        return a.entry;
      case plfx::WsPool::kReclaim:
        if (hipError_t e = hipDeviceSynchronize(); e != hipSuccess)
          *rc = hip_fail(ctx, e, "reclaiming workspaces of exited threads");
        else
          ctx->wss.reclaim();
        break;
      case plfx::WsPool::kAllocate:
        *rc = ws_allocate(ctx, s);
        break;
      case plfx::WsPool::kTooMany:
        *rc = fail(ctx, PLFX_ERR_INVALID,
                   "more than %d streams in use with one context (release idle ones with "
                   "plfx_ctx_release_stream)", PLFX_MAX_STREAMS);
        break;
      case plfx::WsPool::kCapturing:
        *rc = fail(ctx, PLFX_ERR_INVALID,
                   "more than %d streams in use and this one is being captured: issue one call on "
                   "the stream before capturing (its reduction workspace is allocated then)", kWsPool);
        break;
    }
    if (*rc != PLFX_OK) return nullptr;  // else an entry is free now: acquire again
  }
}

// the workspace of stream s as `out`; returns from the caller on failure
#define PLFX_WS(ctx, s, out)                      \
  StreamWs *out = nullptr;                        \
  do {                                            \
    int wrc_ = PLFX_OK;                           \
    out = ws_for((ctx), (s), &wrc_);              \
    if (!out) return wrc_;                        \
  } while (0)

// clv_bytes: bytes of one CLV of the call (n * 4 categories * states * element
// size); a tip child is n code bytes.  The parent may not share a byte with
// either child: every site's children are read by other blocks than the one
// writing that site's parent.
int check_dev_args(plfx_ctx *ctx, const void *x1, const void *x2, const void *x3, const void *EV,
                   int64_t n, const void *left, const void *right, size_t clv_bytes) {
  if (!ctx) return PLFX_ERR_INVALID;
  if (n < 0) return fail(ctx, PLFX_ERR_INVALID, "n < 0 (%lld)", (long long)n);
  if (n == 0) return PLFX_OK;
  if (!x1 || !x2 || !x3 || !EV || !left || !right)
    return fail(ctx, PLFX_ERR_INVALID, "null CLV/matrix pointer");
  if (!aligned16(x1) || !aligned16(x2) || !aligned16(x3))
    return fail(ctx, PLFX_ERR_INVALID, "CLV pointers must be 16-byte aligned");
  if (overlap(x3, clv_bytes, x1, clv_bytes) || overlap(x3, clv_bytes, x2, clv_bytes))
    return fail(ctx, PLFX_ERR_INVALID, "x3 may not overlap x1/x2");
  return PLFX_OK;
}

// n == 0: nothing is launched; the count scaler sums at sums (may be NULL) are
// zero -- 8 zero bytes each, so root_lnl's f64 result goes through here too
int zero_sums(plfx_ctx *ctx, hipStream_t s, void *sums, int count) {
  if (sums && count > 0) PLFX_HIP(ctx, hipMemsetAsync(sums, 0, (size_t)count * sizeof(int64_t), s));
  return PLFX_OK;
}

// n == 0 for a batch of nodes: the sum of each (may be NULL) is zero
template <typename Node>
int zero_node_sums(plfx_ctx *ctx, hipStream_t s, const Node *nodes, int count) {
  for (int i = 0; i < count; i++)
    if (int rc = zero_sums(ctx, s, nodes[i].scaler_sum, 1); rc != PLFX_OK) return rc;
  return PLFX_OK;
}

// one DNA node of dtype (PLFX_F32 / PLFX_F64, checked by the caller)
int plf_dev(plfx_ctx *ctx, int dtype, const void *x1, const void *x2, void *x3, const void *EV, int64_t n,
            const void *left, const void *right, const int32_t *wgt, uint8_t *scaler,
            int64_t *scaler_sum, void *stream) {
  int rc = check_dev_args(ctx, x1, x2, x3, EV, n, left, right,
                          (size_t)n * 16 * (dtype == PLFX_F32 ? 4 : 8));
  if (rc != PLFX_OK) return rc;
  hipStream_t s = pick(stream);
  if (n == 0) return zero_sums(ctx, s, scaler_sum, 1);
  PLFX_WS(ctx, s, w);
  plfx::DnaArgs a{x1, x2, x3, EV, left, right, wgt, scaler, scaler_sum, w->ws, n, ctx->node_segments};
  a.streams = ctx->streams;
  hipError_t e = dtype == PLFX_F32 ? plfx::launch_plf_dna_f32(a, ctx->max_blocks, s)
                                   : plfx::launch_plf_dna_f64(a, ctx->max_blocks, s);
  if (e != hipSuccess) return hip_fail(ctx, e, "plf_dna launch");
  return PLFX_OK;
}

int ensure_dbuf(plfx_ctx *ctx, size_t bytes) {
  if (bytes <= ctx->d_cap) return PLFX_OK;
  if (ctx->d_buf) {
    // the last call's downloads (d2h_stream) and launches (stream) read it
    if (ctx->d2h_stream) PLFX_HIP(ctx, hipStreamSynchronize(ctx->d2h_stream));
    PLFX_HIP(ctx, hipStreamSynchronize(ctx->stream));
    PLFX_HIP(ctx, hipFreeAsync(ctx->d_buf, ctx->stream));
    ctx->d_buf = nullptr;
    ctx->d_cap = 0;
  }
  hipError_t e = hipMallocAsync(&ctx->d_buf, bytes, ctx->stream);
  if (e != hipSuccess) return fail(ctx, PLFX_ERR_NOMEM, "hipMallocAsync(%zu): %s", bytes, hipGetErrorString(e));
  ctx->d_cap = bytes;
  return PLFX_OK;
}

size_t round_up(size_t v, size_t a) { return (v + a - 1) / a * a; }

// plf()-shaped synchronous host entry (the reference's hm / msm / mh regions,
// host_mem.cpp:293-318): H2D -> fused kernel -> D2H, pipelined over up to
// kHostChunksMax site chunks -- chunk i's results go back on a second stream
// while chunk i+1 uploads, so the two PCIe directions overlap (the reference
// overlaps its two uploads and its two downloads, host_mem.cpp:297-314).  The
// chunks are independent sites; the scaler sum is the sum of the chunk sums.
template <typename T>
int plf_host(plfx_ctx *ctx, const T *x1, const T *x2, T *x3, const T *EV, int n, const T *left,
             const T *right, const int *wgt, int *scalerIncrement) {
  if (!ctx) return PLFX_ERR_INVALID;
  if (n < 0) return fail(ctx, PLFX_ERR_INVALID, "n < 0 (%d)", n);
  if (n > 0 && (!x1 || !x2 || !x3 || !EV || !left || !right))
    return fail(ctx, PLFX_ERR_INVALID, "null argument");
  if (wgt && n >= 512) {  // the reduction's bound (plfx.h): sum |wgt| < 2^40; 511 weights cannot reach it
    int64_t tot = 0;
    for (int i = 0; i < n; i++) tot += wgt[i] < 0 ? -(int64_t)wgt[i] : (int64_t)wgt[i];
    if (tot >= (int64_t(1) << 40)) return fail(ctx, PLFX_ERR_INVALID, "sum |wgt| >= 2^40");
  }
  constexpr int64_t kMinChunk = 1 << 17;  // sites; smaller chunks pay per-copy overheads
  const int nch = (int)std::max<int64_t>(1, std::min<int64_t>(kHostChunksMax, n / kMinChunk));
  const int64_t chunk = ((int64_t)n + nch - 1) / nch;
  const size_t clv = (size_t)n * 16 * sizeof(T);
  const size_t o_x1 = 0, o_x2 = round_up(clv, 256), o_x3 = o_x2 + round_up(clv, 256);
  const size_t o_mat = o_x3 + round_up(clv, 256);  // EV 16 | left 64 | right 64
  const size_t o_wgt = o_mat + round_up(144 * sizeof(T), 256);
  const size_t o_sum = o_wgt + round_up((size_t)n * sizeof(int32_t), 256);  // int64 per chunk
  const size_t total = o_sum + round_up(kHostChunksMax * sizeof(int64_t), 256);
  int rc = ensure_dbuf(ctx, total);
  if (rc != PLFX_OK) return rc;
  if (!ctx->d2h_stream) {
    PLFX_HIP(ctx, hipStreamCreateWithFlags(&ctx->d2h_stream, hipStreamNonBlocking));
    for (hipEvent_t &e : ctx->chunk_done) PLFX_HIP(ctx, hipEventCreateWithFlags(&e, hipEventDisableTiming));
  }
  char *d = static_cast<char *>(ctx->d_buf);
  hipStream_t s = ctx->stream, s2 = ctx->d2h_stream;
  const T *dm = reinterpret_cast<const T *>(d + o_mat);
  int64_t *dsum = reinterpret_cast<int64_t *>(d + o_sum);
  if (n > 0) {
    PLFX_HIP(ctx, hipMemcpyAsync(d + o_mat, EV, 16 * sizeof(T), hipMemcpyHostToDevice, s));
    PLFX_HIP(ctx, hipMemcpyAsync(d + o_mat + 16 * sizeof(T), left, 64 * sizeof(T), hipMemcpyHostToDevice, s));
    PLFX_HIP(ctx, hipMemcpyAsync(d + o_mat + 80 * sizeof(T), right, 64 * sizeof(T), hipMemcpyHostToDevice, s));
  }
  int used = 0;
  for (int64_t lo = 0; lo < n || (n == 0 && used == 0); lo += chunk, used++) {
    const int64_t m = std::min<int64_t>(chunk, n - lo);
    const size_t off = (size_t)lo * 16 * sizeof(T), bytes = (size_t)m * 16 * sizeof(T);
    if (m > 0) {
      PLFX_HIP(ctx, hipMemcpyAsync(d + o_x1 + off, x1 + lo * 16, bytes, hipMemcpyHostToDevice, s));
      PLFX_HIP(ctx, hipMemcpyAsync(d + o_x2 + off, x2 + lo * 16, bytes, hipMemcpyHostToDevice, s));
      if (wgt)
        PLFX_HIP(ctx, hipMemcpyAsync(d + o_wgt + lo * 4, wgt + lo, (size_t)m * 4, hipMemcpyHostToDevice, s));
    }
    rc = plf_dev(ctx, sizeof(T) == 4 ? PLFX_F32 : PLFX_F64, d + o_x1 + off, d + o_x2 + off, d + o_x3 + off,
                 dm, std::max<int64_t>(m, 0), dm + 16, dm + 80,
                 wgt ? reinterpret_cast<const int32_t *>(d + o_wgt + lo * 4) : nullptr, nullptr,
                 dsum + used, s);
    if (rc != PLFX_OK) return rc;
    if (m > 0) {
      PLFX_HIP(ctx, hipEventRecord(ctx->chunk_done[used], s));
      PLFX_HIP(ctx, hipStreamWaitEvent(s2, ctx->chunk_done[used], 0));
      PLFX_HIP(ctx, hipMemcpyAsync(x3 + lo * 16, d + o_x3 + off, bytes, hipMemcpyDeviceToHost, s2));
    }
    if (n == 0) break;
  }
  int64_t sums[kHostChunksMax] = {};
  PLFX_HIP(ctx, hipMemcpyAsync(sums, dsum, (size_t)used * sizeof(int64_t), hipMemcpyDeviceToHost, s));
  PLFX_HIP(ctx, hipStreamSynchronize(s));
  PLFX_HIP(ctx, hipStreamSynchronize(s2));
  int64_t sum = 0;
  for (int i = 0; i < used; i++) sum += sums[i];
  // plf()'s int: the exact sum modulo 2^32 as a signed 32-bit value (plfx.h), as the reference's own
  // int accumulation wraps
  if (scalerIncrement) *scalerIncrement = (int)sum;
  return PLFX_OK;
}

// What the launches of one call share: the entry point's arguments.
struct ExecCall {
  int dtype, states, flags;
  const void *EV;
  int64_t n;
  const int32_t *wgt;
  const void *tipvec;  // may be NULL
  hipStream_t s;
  int streams;  // DNA batches share the resident grid with the batches of this many streams in flight
};

// PLFX_CTX_LAZY_TABLES: the tip/tip tables of workspace entry w on its first
// tip/tip use, before the call is lowered (its descriptors point into them)
int ensure_tables(plfx_ctx *ctx, StreamWs *w, hipStream_t s) {
  if (w->tt) return PLFX_OK;
  if (w->capturing_now())
    return fail(ctx, PLFX_ERR_INVALID,
                "protein tip/tip tables: the context was created with PLFX_CTX_LAZY_TABLES and "
                "this stream has not made a tip/tip call outside a capture yet");
  void *t = nullptr;
  hipError_t e = hipMallocAsync(&t, kTtEntryBytes, s);
  if (e != hipSuccess)
    return fail(ctx, PLFX_ERR_NOMEM, "tip/tip tables hipMallocAsync(%zu): %s", kTtEntryBytes,
                hipGetErrorString(e));
  ctx->ws_blocks.push_back(t);
  w->tt = static_cast<char *>(t);
  return PLFX_OK;
}

// The launches of a lowered call (trav_lower.hpp), in list order.
int execute(plfx_ctx *ctx, const plfx::LaunchList &l, const ExecCall &c, unsigned long long *ws) {
  const bool fma = (c.flags & PLFX_FMA) != 0;
  const int mb = ctx->max_blocks;
  for (const plfx::LaunchItem &it : l.items) {
    hipError_t e = hipSuccess;
    const char *what = "";
    switch (it.kind) {
      case plfx::kLaunchDeep:
        what = "fused deep-subtree launch";
        e = plfx::launch_plf_dna_deep(c.dtype, it.depth, &l.deeps[it.first], c.EV, c.wgt, c.n, ws, mb, c.s,
                                      it.tips, c.tipvec);
        break;
      case plfx::kLaunchSeptets:
        what = "fused three-level launch";
        e = plfx::launch_plf_dna_septets(c.dtype, &l.septets[it.first], it.count, c.EV, c.wgt, c.n, ws, mb, c.s,
                                         it.tips, c.tipvec);
        break;
      case plfx::kLaunchTriples:
        what = "fused level-pair launch";
        e = plfx::launch_plf_dna_triples(c.dtype, &l.triples[it.first], it.count, c.EV, c.wgt, c.n, ws, mb, c.s,
                                         it.tips, c.tipvec);
        break;
      case plfx::kLaunchDnaBatch:
        what = "plf batch launch";
        e = plfx::launch_plf_dna_batch(c.dtype, &l.nodes[it.first], it.count, c.EV, c.wgt, c.n, ws, mb, c.s,
                                       it.tips, c.tipvec, c.streams);
        break;
      case plfx::kLaunchProtNode: {
        what = "plf_prot launch";
        const plfx::NodeDescH &d = l.nodes[it.first];
        plfx::DnaArgs a{d.x1, d.x2, d.x3, c.EV, d.left, d.right, c.wgt, d.scaler, d.scaler_sum, ws, c.n};
        e = plfx::launch_plf_prot(c.dtype, fma, a, mb, c.s, it.tips, c.tipvec);
        break;
      }
      case plfx::kLaunchProtBatch:
        what = "plf_prot batch launch";
        e = plfx::launch_plf_prot_batch(c.dtype, fma, &l.nodes[it.first], it.count, c.EV, c.wgt, c.n, ws, mb, c.s,
                                        it.tips, c.tipvec);
        break;
      case plfx::kLaunchProtTipTip:
        what = "plf_prot combination tables";
        e = plfx::launch_plf_prot_batch(c.dtype, fma, &l.combs[it.first], it.count, c.EV, nullptr,
                                        plfx::kProtCombos, ws, mb, c.s, 2, c.tipvec);
        if (e != hipSuccess) break;
        what = "plf_prot tip/tip gather";
        e = plfx::launch_prot_tiptip_gather(c.dtype, &l.gathers[it.first], it.count, c.wgt, c.n, ws, mb, c.s);
        break;
      case plfx::kLaunchProtTab:
        what = "plf_prot table-children launch";
        e = plfx::launch_prot_tab_batch(c.dtype, fma, &l.tabs[it.first], it.count, c.EV, c.wgt, c.n, ws, mb, c.s);
        break;
    }
    if (e != hipSuccess) return hip_fail(ctx, e, what);
  }
  return PLFX_OK;
}

// Nodes of one kind (tips = number of tip children, tip child first):
// lowered (trav_lower.hpp lower_batch), then launched.
int run_batch(plfx_ctx *ctx, const ExecCall &c, const plfx_node *nodes, int count, int tips) {
  if (count < 0 || c.n < 0 || (count > 0 && (!nodes || !c.EV)))
    return fail(ctx, PLFX_ERR_INVALID, "bad batch arguments");
  if (c.n == 0) return zero_node_sums(ctx, c.s, nodes, count);
  if (count == 0) return PLFX_OK;
  PLFX_WS(ctx, c.s, w);
  if (c.states == 20 && tips == 2)
    if (int rc = ensure_tables(ctx, w, c.s); rc != PLFX_OK) return rc;
  std::string err;
  const plfx::LowerCall lc{c.dtype, c.states, c.n, w->tt, ctx->tt_codes};
  if (plfx::lower_batch(lc, nodes, count, tips, nullptr, &ctx->lowered, &err) != PLFX_OK)
    return fail(ctx, PLFX_ERR_INVALID, "%s", err.c_str());
  return execute(ctx, ctx->lowered, c, w->ws);
}

// The launches of a lowered per-site-rate call (psr_lower.hpp), in list order.
int execute_psr(plfx_ctx *ctx, const plfx::PsrLaunchList &l, const plfx::PsrCall &c, const int32_t *wgt,
                const void *tipvec, hipStream_t s, unsigned long long *ws) {
  static_assert(3 * plfx::kMaxTriples <= kWsRegions, "three ticket regions per level pair");
  for (const plfx::PsrLaunch &it : l.items) {
    const bool triples = it.kind == plfx::kPsrTriples;
    if (c.states == 20) {  // section 11b: node batches only (the lowering emits no level pair)
      // section 11d: PLFX_FMA runs the same list on the matrix-core kernel (f64, checked by the entry point)
      hipError_t e = hipErrorInvalidValue;
      if (!triples)
        e = (c.flags & PLFX_FMA)
                ? plfx::launch_plf_psr_prot_mfma(it.tips, &l.nodes[it.first], it.count, c.EV, c.rate_cat, c.ncat, wgt,
                                                 c.n, tipvec, ws, ctx->max_blocks, s)
                : plfx::launch_plf_psr_prot(c.dtype, it.tips, &l.nodes[it.first], it.count, c.EV, c.rate_cat, c.ncat,
                                            wgt, c.n, tipvec, ws, ctx->max_blocks, s);
      if (e != hipSuccess) return hip_fail(ctx, e, "plf_psr protein launch");
      continue;
    }
    const hipError_t e =
        triples ? plfx::launch_plf_psr_triples(c.dtype, it.tips, &l.triples[it.first], it.count, c.EV, c.rate_cat,
                                               c.ncat, wgt, c.n, tipvec, ws, ctx->max_blocks, s)
                : plfx::launch_plf_psr(c.dtype, it.tips, &l.nodes[it.first], it.count, c.EV, c.rate_cat, c.ncat, wgt,
                                       c.n, tipvec, ws, ctx->max_blocks, s);
    if (e != hipSuccess) return hip_fail(ctx, e, triples ? "plf_psr level-pair launch" : "plf_psr launch");
  }
  return PLFX_OK;
}

// The plan of a traversal call: levels and fused groups from the op list and
// the tip slots alone.
int plan_call(plfx_ctx *ctx, const plfx_trav_op *ops, int nops, const uint8_t *const *tips, int nslots, int npmats,
              int states, int fuse, plfx::TravPlan *plan) {
  std::vector<unsigned char> tip_mask;
  if (nops > 0 && tips)
    for (int sl = 0; sl < nslots; sl++) tip_mask.push_back(tips[sl] != nullptr);
  std::string err;
  if (plfx::plan_traversal(ops, nops, nslots, npmats, tip_mask.empty() ? nullptr : tip_mask.data(), states, fuse,
                           plan, &err) != PLFX_OK)
    return fail(ctx, PLFX_ERR_INVALID, "%s", err.c_str());
  return PLFX_OK;
}

// The end of a traversal call that was not refused: its schedule as
// plfx_traverse_schedule reports it from now on (launches 0: nothing to launch).
int publish_sched(plfx_ctx *ctx, const plfx::TravPlan &plan, int launches) {
  static_assert(PLFX_SCHED_COUNTS == 7, "the plan's six counts, then the launches");
  std::copy(plan.counts, plan.counts + 6, ctx->sched);
  ctx->sched[6] = launches;
  return PLFX_OK;
}

// The arguments of plfx_edge_sumtable and plfx_edge_sumtable_psr after dtype
// and states; clv_bytes of one CLV of the call.  n == 0 passes: the caller
// returns then.
int check_sumtable_args(plfx_ctx *ctx, const uint8_t *tip1, const void *x1, const void *x2, int64_t n,
                        const void *tipvec, const void *sumtab, size_t clv_bytes) {
  if ((tip1 != nullptr) == (x1 != nullptr))
    return fail(ctx, PLFX_ERR_INVALID, "side 1 needs exactly one of tip / CLV");
  if (tip1 && !tipvec)
    return fail(ctx, PLFX_ERR_INVALID, "a coded side needs tipvec (the default 0/1 table is not in eigen coordinates)");
  if (n < 0) return fail(ctx, PLFX_ERR_INVALID, "n < 0 (%lld)", (long long)n);
  if (n == 0) return PLFX_OK;
  if (!x2 || !sumtab) return fail(ctx, PLFX_ERR_INVALID, "null CLV / sum table pointer");
  if ((x1 && !aligned16(x1)) || !aligned16(x2) || !aligned16(sumtab))
    return fail(ctx, PLFX_ERR_INVALID, "CLV pointers must be 16-byte aligned");
  if (overlap(sumtab, clv_bytes, tip1 ? (const void *)tip1 : x1, tip1 ? (size_t)n : clv_bytes) ||
      overlap(sumtab, clv_bytes, x2, clv_bytes))
    return fail(ctx, PLFX_ERR_INVALID, "sumtab may not overlap x1/x2");
  return PLFX_OK;
}

// What the root-lnL and edge-derivative entry points (`who`) check last:
// `required` -- their own pointers and sizes -- and the scaler sums.
int check_sums_args(plfx_ctx *ctx, const char *who, bool required, const int64_t *scaler_sums, int nsums) {
  if (!required || nsums < 0 || (nsums > 0 && !scaler_sums))
    return fail(ctx, PLFX_ERR_INVALID, "bad %s arguments", who);
  return PLFX_OK;
}

// The environment's settings of a new context; false for a value that is refused.
bool env_settings(plfx_ctx *ctx) {
  // Grid cap: 0 = as many blocks as are co-resident (occupancy x CUs);
  // PLFX_MAX_BLOCKS overrides it for experiments.
  if (const char *env = std::getenv("PLFX_MAX_BLOCKS")) {
    int v = std::atoi(env);
    if (v > 0) ctx->max_blocks = v;
  }
  if (const char *env = std::getenv("PLFX_FUSE")) ctx->fuse = ctx->psr_fuse = std::atoi(env);
  // PLFX_NODE_SEGMENTS: "1" on, "0" off, "-1" / "auto" / unset by size; any
  // other value is refused (a typo must not silently switch the mapping)
  if (const char *env = std::getenv("PLFX_NODE_SEGMENTS")) {
    if (!std::strcmp(env, "1")) ctx->node_segments = 1;
    else if (!std::strcmp(env, "0")) ctx->node_segments = 0;
    else if (!std::strcmp(env, "-1") || !std::strcmp(env, "auto") || !*env) ctx->node_segments = -1;
    else return false;
  }
  // PLFX_STREAMS: one-node calls kept in flight, "1".."8" (PLFX_STREAMS_MAX), empty
  // = 1; anything else is refused like PLFX_NODE_SEGMENTS
  const char *env = std::getenv("PLFX_STREAMS");
  if (env && *env) {
    static_assert(PLFX_STREAMS_MAX <= 9, "PLFX_STREAMS is parsed as one digit");
    const int v = (env[0] >= '1' && env[0] <= '0' + PLFX_STREAMS_MAX && !env[1]) ? env[0] - '0' : 0;
    if (!v) return false;
    ctx->streams = v;
  }
  return true;
}

// the arguments plfx_edge_derivatives and plfx_edge_optimize share
int check_edge_args(plfx_ctx *ctx, int dtype, int states, const void *sumtab, int64_t n,
                           const double *eigen, const double *rates, int ncat) {
  if (int rc = check_dtype(ctx, dtype); rc != PLFX_OK) return rc;
  if (states != 4 && states != 20) return fail(ctx, PLFX_ERR_UNSUPPORTED, "edge: states=%d not built (4, 20)", states);
  if (ncat != 4) return fail(ctx, PLFX_ERR_UNSUPPORTED, "edge: ncat=%d not built (4)", ncat);
  if (n < 0) return fail(ctx, PLFX_ERR_INVALID, "n < 0 (%lld)", (long long)n);
  if (!eigen || !rates || (n > 0 && !sumtab)) return fail(ctx, PLFX_ERR_INVALID, "edge: null sum table / eigen / rates");
  if (!aligned16(sumtab)) return fail(ctx, PLFX_ERR_INVALID, "the sum table must be 16-byte aligned");
  return PLFX_OK;
}

// the arguments plfx_edge_derivatives_psr and plfx_edge_optimize_psr share
int check_psr_edge_args(plfx_ctx *ctx, int dtype, const void *sumtab, int64_t n, const double *eigen,
                        const double *rates, int ncat, const uint8_t *rate_cat) {
  if (int rc = check_dtype(ctx, dtype); rc != PLFX_OK) return rc;
  if (ncat < 1 || ncat > PLFX_PSR_MAX_CATS)
    return fail(ctx, PLFX_ERR_INVALID, "psr edge: ncat=%d outside 1..%d", ncat, PLFX_PSR_MAX_CATS);
  if (n < 0) return fail(ctx, PLFX_ERR_INVALID, "n < 0 (%lld)", (long long)n);
  if (!eigen || !rates || (n > 0 && (!sumtab || !rate_cat)))
    return fail(ctx, PLFX_ERR_INVALID, "psr edge: null sum table / eigen / rates / rate_cat");
  if (!aligned16(sumtab)) return fail(ctx, PLFX_ERR_INVALID, "the sum table must be 16-byte aligned");
  return PLFX_OK;
}

// The host-synchronous bracketed Newton of plfx_edge_optimize and
// plfx_edge_optimize_psr (edge_newton.hpp) from t0 on stream s: eval(d_t,
// d_out) enqueues one evaluation of the three sums at the device double d_t
// into the device doubles d_out, both in the context's edge_buf.
template <typename Eval>
int edge_newton_loop(plfx_ctx *ctx, const char *who, double t0, double tmin, double tmax, int max_evals,
                     double *t_opt, double *out3_host, int *evals, hipStream_t s, Eval eval) {
  if (!t_opt) return fail(ctx, PLFX_ERR_INVALID, "%s: null t_opt", who);
  plfx::EdgeNewton step(t0, tmin, tmax, max_evals);
  if (!step.valid())
    return fail(ctx, PLFX_ERR_INVALID, "%s: needs 0 < tmin <= t0 <= tmax and max_evals >= 1", who);
  if (capturing(s))
    return fail(ctx, PLFX_ERR_INVALID, "%s waits for every evaluation: not on a capturing stream", who);
  double *d_t = ctx->edge_buf, *d_out = ctx->edge_buf + 1;
  double t = 0.0, out[3] = {0.0, 0.0, 0.0};
  for (bool more = true; more;) {
    t = step.t();  // read by the upload until the wait below
    PLFX_HIP(ctx, hipMemcpyAsync(d_t, &t, sizeof t, hipMemcpyHostToDevice, s));
    if (int rc = eval(d_t, d_out); rc != PLFX_OK) return rc;
    PLFX_HIP(ctx, hipMemcpyAsync(out, d_out, sizeof out, hipMemcpyDeviceToHost, s));
    PLFX_HIP(ctx, hipStreamSynchronize(s));
    more = step.advance(out[1], out[2]);
  }
  *t_opt = t;
  if (out3_host) std::copy(out, out + 3, out3_host);
  if (evals) *evals = step.evals();
  return PLFX_OK;
}

// The device-resident Newton of plfx_edge_optimize_dev and
// plfx_edge_optimize_psr_dev_gen (`who`): check_table(sumtab) checks one table
// with the call's model arguments, launch(g, c, w, s) enqueues the c edges
// from edge g on stream s with the stream's workspace w.
template <typename Check, typename Launch>
int edge_optimize_dev(plfx_ctx *ctx, const char *who, const void *const *sumtabs, int nedges, const double *t0,
                      double tmin, double tmax, int max_evals, double *t_opt, void *stream, Check check_table,
                      Launch launch) {
  if (nedges < 1 || !sumtabs) return fail(ctx, PLFX_ERR_INVALID, "%s: nedges=%d / null sumtabs", who, nedges);
  for (int j = 0; j < nedges; j++) {
    if (!sumtabs[j]) return fail(ctx, PLFX_ERR_INVALID, "%s: sum table %d is null", who, j);
    if (int rc = check_table(sumtabs[j]); rc != PLFX_OK) return rc;
  }
  if (!t0 || !t_opt) return fail(ctx, PLFX_ERR_INVALID, "%s: null t0 / t_opt", who);
  if (!(tmin > 0.0 && tmin <= tmax && std::isfinite(tmax)) || max_evals < 1 || max_evals > PLFX_EDGE_MAX_EVALS)
    return fail(ctx, PLFX_ERR_INVALID, "%s: needs 0 < tmin <= tmax < inf and 1 <= max_evals <= %d", who,
                PLFX_EDGE_MAX_EVALS);
  hipStream_t s = pick(stream);
  PLFX_WS(ctx, s, w);
  // groups of kMaxBatch edges, one after the other on the stream: a group's
  // launches are done with the state, ticket and partial regions before the
  // next group's first launch rewrites the state
  for (int g = 0; g < nedges; g += plfx::kMaxBatch) {
    hipError_t e = launch(g, std::min(nedges - g, plfx::kMaxBatch), w, s);
    if (e != hipSuccess) return hip_fail(ctx, e, (std::string(who) + " launch").c_str());
  }
  return PLFX_OK;
}

// the state counts the per-site-rate entry points are built for
int check_psr_states(plfx_ctx *ctx, int states) {
  if (states != 4 && states != 20)
    return fail(ctx, PLFX_ERR_UNSUPPORTED, "per-site rate categories: states=%d not built (4, 20)", states);
  return PLFX_OK;
}

// The flags of the plfx_*_psr_ex entry points (plfx.h section 11d), after the
// states check: what the call runs with -- 0 for 4 states ("DNA is always
// exact") -- into *mode.  who: the entry point, for the message.
int check_psr_flags(plfx_ctx *ctx, const char *who, int dtype, int states, int flags, int *mode) {
  if (flags & ~PLFX_FMA) return fail(ctx, PLFX_ERR_INVALID, "%s: bad flags %d", who, flags);
  *mode = states == 20 ? flags : 0;
  if (*mode && dtype == PLFX_F32)
    return fail(ctx, PLFX_ERR_UNSUPPORTED, "%s: PLFX_FMA with 20 states is built for f64 only", who);
  return PLFX_OK;
}

}  // namespace

extern "C" {

int plfx_get_version(void) { return PLFX_VERSION; }

int plfx_ctx_create(int device, plfx_ctx **out) { return plfx_ctx_create_ex(device, 0u, out); }

int plfx_ctx_create_ex(int device, unsigned flags, plfx_ctx **out) {
  if (!out) return PLFX_ERR_INVALID;
  if (flags & ~(unsigned)PLFX_CTX_LAZY_TABLES) return PLFX_ERR_INVALID;
  *out = nullptr;
  int count = 0;
  if (hipGetDeviceCount(&count) != hipSuccess || device < 0 || device >= count)
    return PLFX_ERR_NODEV;
  hipDeviceProp_t prop;
  if (hipGetDeviceProperties(&prop, device) != hipSuccess) return PLFX_ERR_NODEV;
  if (std::strncmp(prop.gcnArchName, "gfx950", 6) != 0) return PLFX_ERR_NODEV;
  plfx_ctx *ctx = new (std::nothrow) plfx_ctx();
  if (!ctx) return PLFX_ERR_NOMEM;
  ctx->device = device;
  ctx->lazy_tables = (flags & PLFX_CTX_LAZY_TABLES) != 0;
  DeviceGuard guard(device);  // the caller's current device is restored on return
  // the settings first: until the stream exists only the context is to undo
  int rc = PLFX_OK;
  if (!env_settings(ctx)) rc = PLFX_ERR_INVALID;
  else if (hipStreamCreateWithFlags(&ctx->stream, hipStreamNonBlocking) != hipSuccess) rc = PLFX_ERR_HIP;
  if (rc != PLFX_OK) {
    delete ctx;
    return rc;
  }
  // the workspace pool: kWsPool entries (reduction words zeroed before return,
  // tip/tip tables), and the tables' constant code arrays
  auto undo = [&](int code) {
    for (void *b : ctx->ws_blocks) (void)hipFreeAsync(b, ctx->stream);
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipStreamDestroy(ctx->stream);
    delete ctx;
    return code;
  };
  void *pool = nullptr, *tabs = nullptr, *codes = nullptr, *edge = nullptr;
  if (hipMallocAsync(&pool, kWsPool * kWsEntryBytes, ctx->stream) != hipSuccess) return undo(PLFX_ERR_NOMEM);
  ctx->ws_blocks.push_back(pool);
  if (!ctx->lazy_tables) {
    if (hipMallocAsync(&tabs, kWsPool * kTtEntryBytes, ctx->stream) != hipSuccess) return undo(PLFX_ERR_NOMEM);
    ctx->ws_blocks.push_back(tabs);
  }
  if (hipMallocAsync(&codes, kTtCodeBytes, ctx->stream) != hipSuccess) return undo(PLFX_ERR_NOMEM);
  ctx->ws_blocks.push_back(codes);
  if (hipMallocAsync(&edge, kEdgeBufBytes, ctx->stream) != hipSuccess) return undo(PLFX_ERR_NOMEM);
  ctx->ws_blocks.push_back(edge);
  ctx->edge_buf = static_cast<double *>(edge);
  uint8_t cc[kTtCodeBytes] = {};
  for (int k = 0; k < plfx::kProtCombos; k++) {
    cc[k] = (uint8_t)(k / 24);
    cc[1024 + k] = (uint8_t)(k % 24);
  }
  if (hipMemsetAsync(pool, 0, kWsPool * kWsEntryBytes, ctx->stream) != hipSuccess ||
      hipMemcpyAsync(codes, cc, kTtCodeBytes, hipMemcpyHostToDevice, ctx->stream) != hipSuccess ||
      hipStreamSynchronize(ctx->stream) != hipSuccess)
    return undo(PLFX_ERR_HIP);
  ctx->tt_codes = static_cast<uint8_t *>(codes);
  for (int i = 0; i < kWsPool; i++) {
    StreamWs w;
    ws_carve(w, static_cast<char *>(pool) + i * kWsEntryBytes,
             tabs ? static_cast<char *>(tabs) + i * kTtEntryBytes : nullptr);
    ctx->wss.add(w);
  }
  {
    std::lock_guard<std::mutex> l(g_live_mu);
    g_live.push_back(ctx);
  }
  *out = ctx;
  return PLFX_OK;
}

int plfx_ctx_destroy(plfx_ctx *ctx) {
  if (!ctx) return PLFX_OK;
  {
    // no exiting thread may retire entries of this context from here on
    std::lock_guard<std::mutex> l(g_live_mu);
    g_live.erase(std::remove(g_live.begin(), g_live.end(), ctx), g_live.end());
  }
  {
    DeviceGuard guard(ctx->device);
    (void)hipStreamSynchronize(ctx->stream);
    // the staging buffer's last downloads run on d2h_stream: done before the
    // free.  All device memory of the context is stream-ordered
    // (hipMallocAsync): freed on its stream below, since hipFree would wait for
    // the whole device
    if (ctx->d2h_stream) {
      (void)hipStreamSynchronize(ctx->d2h_stream);
      (void)hipStreamDestroy(ctx->d2h_stream);
    }
    if (ctx->d_buf) (void)hipFreeAsync(ctx->d_buf, ctx->stream);
    for (hipEvent_t e : ctx->chunk_done)
      if (e) (void)hipEventDestroy(e);
    // Workspace entries still held by a stream other than the context's:
    // their last launches must be done before the free.  The caller's stream
    // handle is never used here -- the stream may already be destroyed (e.g.
    // a context collected after its user's streams) -- so the device is
    // waited for; releasing streams (plfx_ctx_release_stream) before destroy
    // avoids that wait.  An entry used under a capture needs it anyway (its
    // graph may still be replaying on any stream).
    if (ctx->wss.needs_device_wait(ctx->stream)) (void)hipDeviceSynchronize();
    for (void *b : ctx->ws_blocks) (void)hipFreeAsync(b, ctx->stream);
    (void)hipStreamSynchronize(ctx->stream);
    (void)hipStreamDestroy(ctx->stream);
  }
  delete ctx;
  return PLFX_OK;
}

// A copy taken under the context's lock, so another thread's failure cannot
// free the string under the caller; valid until this thread's next call.
const char *plfx_last_error(const plfx_ctx *ctx) {
  if (!ctx) return "null context";
  thread_local std::string copy;
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  copy = ctx->err;
  return copy.c_str();
}

void *plfx_ctx_stream(plfx_ctx *ctx) { return ctx ? reinterpret_cast<void *>(ctx->stream) : nullptr; }

int plfx_ctx_device(const plfx_ctx *ctx) { return ctx ? ctx->device : -1; }

int plfx_ctx_synchronize(plfx_ctx *ctx) {
  PLFX_BIND(ctx);
  PLFX_HIP(ctx, hipStreamSynchronize(ctx->stream));
  return PLFX_OK;
}

int plfx_ctx_release_stream(plfx_ctx *ctx, void *stream) {
  PLFX_BIND(ctx);
  hipStream_t s = pick(stream);
  StreamWs *w = ctx->wss.find(s, &t_tag);
  if (!w) return PLFX_OK;  // no workspace held: nothing to release
  if (capturing(s))  // a wait on a capturing stream would invalidate the capture
    return fail(ctx, PLFX_ERR_INVALID, "stream is being captured: release it after the capture ends");
  // the stream's last sum-producing launch must be done before another stream
  // may take the entry (it is zero again once that launch has finished)
  PLFX_HIP(ctx, hipStreamSynchronize(s));
  // a graph captured through the entry keeps using its words (sum tickets,
  // queue heads, tip/tip tables): retired, never handed to another stream
  ctx->wss.release(w);
  return PLFX_OK;
}

int plfx_ctx_set_streams(plfx_ctx *ctx, int streams) {
  if (!ctx) return PLFX_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  if (streams < 1 || streams > PLFX_STREAMS_MAX)
    return fail(ctx, PLFX_ERR_INVALID, "streams %d not in 1..%d", streams, PLFX_STREAMS_MAX);
  ctx->streams = streams;
  return PLFX_OK;
}

int plfx_ctx_streams(const plfx_ctx *ctx) {
  if (!ctx) return PLFX_ERR_INVALID;
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  return ctx->streams;
}

int plfx_plf_f32(plfx_ctx *ctx, const float *x1, const float *x2, float *x3, const float *EV, int n,
                 const float *left, const float *right, const int *wgt, int *scalerIncrement) {
  PLFX_BIND(ctx);
  return plf_host<float>(ctx, x1, x2, x3, EV, n, left, right, wgt, scalerIncrement);
}

int plfx_plf_f64(plfx_ctx *ctx, const double *x1, const double *x2, double *x3, const double *EV,
                 int n, const double *left, const double *right, const int *wgt,
                 int *scalerIncrement) {
  PLFX_BIND(ctx);
  return plf_host<double>(ctx, x1, x2, x3, EV, n, left, right, wgt, scalerIncrement);
}

int plfx_plf_dev_f32(plfx_ctx *ctx, const float *x1, const float *x2, float *x3, const float *EV,
                     int64_t n, const float *left, const float *right, const int32_t *wgt,
                     uint8_t *scaler, int64_t *scaler_sum, void *stream) {
  PLFX_BIND(ctx);
  return plf_dev(ctx, PLFX_F32, x1, x2, x3, EV, n, left, right, wgt, scaler, scaler_sum, stream);
}

int plfx_plf_dev_f64(plfx_ctx *ctx, const double *x1, const double *x2, double *x3,
                     const double *EV, int64_t n, const double *left, const double *right,
                     const int32_t *wgt, uint8_t *scaler, int64_t *scaler_sum, void *stream) {
  PLFX_BIND(ctx);
  return plf_dev(ctx, PLFX_F64, x1, x2, x3, EV, n, left, right, wgt, scaler, scaler_sum, stream);
}

int plfx_plf_dev_gen(plfx_ctx *ctx, int dtype, int states, int flags, const void *x1,
                     const void *x2, void *x3, const void *EV, int64_t n, const void *left,
                     const void *right, const int32_t *wgt, uint8_t *scaler,
                     int64_t *scaler_sum, void *stream) {
  PLFX_BIND(ctx);
  if (int rc = check_dtype(ctx, dtype); rc != PLFX_OK) return rc;
  if (flags & ~(PLFX_FMA | PLFX_VALU)) return fail(ctx, PLFX_ERR_INVALID, "bad flags %d", flags);
  const bool valu = (flags & PLFX_VALU) != 0;
  if (valu && (states != 20 || dtype != PLFX_F64))
    return fail(ctx, PLFX_ERR_INVALID, "PLFX_VALU: protein (states 20), f64 only");
  if (states == 4) return plf_dev(ctx, dtype, x1, x2, x3, EV, n, left, right, wgt, scaler, scaler_sum, stream);
  if (states != 20) return fail(ctx, PLFX_ERR_UNSUPPORTED, "states=%d not built (4, 20)", states);
  int rc = check_dev_args(ctx, x1, x2, x3, EV, n, left, right,
                          (size_t)n * 80 * (dtype == PLFX_F32 ? 4 : 8));
  if (rc != PLFX_OK) return rc;
  hipStream_t s = pick(stream);
  if (n == 0) return zero_sums(ctx, s, scaler_sum, 1);
  PLFX_WS(ctx, s, w);
  plfx::DnaArgs a{x1, x2, x3, EV, left, right, wgt, scaler, scaler_sum, w->ws, n};
  a.streams = ctx->streams;
  // f64 exact: the scalar-operand kernel (plf_prot_valu_exact.hip, 3 waves per
  // SIMD; +10 % over the LDS-matrix kernel, same bits) with or without PLFX_VALU
  const bool fma = (flags & PLFX_FMA) != 0;
  hipError_t e = dtype == PLFX_F64 && !fma ? plfx::launch_plf_prot_valu_exact_f64(a, ctx->max_blocks, s)
                 : valu                    ? plfx::launch_plf_prot_valu_f64(a, ctx->max_blocks, s)
                                           : plfx::launch_plf_prot(dtype, fma, a, ctx->max_blocks, s);
  if (e != hipSuccess) return hip_fail(ctx, e, valu ? "plf_prot_valu launch" : "plf_prot launch");
  return PLFX_OK;
}

int plfx_instance_run(plfx_ctx *ctx, const void *in_left, const void *in_right, void *out_clv,
                      uint8_t *out_scaler, uint32_t alignment_sites, uint32_t window_size,
                      int layout, int dtype, void *stream) {
  PLFX_BIND(ctx);
  if (layout != PLFX_LAYOUT_COMBINED && layout != PLFX_LAYOUT_SEPARATE)
    return fail(ctx, PLFX_ERR_INVALID, "bad layout %d", layout);
  if (int rc = check_dtype(ctx, dtype); rc != PLFX_OK) return rc;
  if (window_size % 16 != 0) return fail(ctx, PLFX_ERR_INVALID, "window_size %u not a multiple of 16", window_size);
  if (!in_left || !in_right) return fail(ctx, PLFX_ERR_INVALID, "null instance buffer");
  // Header words: in_left = [EV | P_L] (mm2sleft reads mem[0], mem[1..4]);
  // in_right = [EV | P_R] (COMBINED, mem[1..4]) or [P_R] (SEPARATE, mem[0..3]).
  const size_t es = dtype == PLFX_F32 ? 4 : 8;
  const char *L = static_cast<const char *>(in_left);
  const char *R = static_cast<const char *>(in_right);
  const size_t rhdr = layout == PLFX_LAYOUT_COMBINED ? 80 : 64;
  const void *EV = L;
  const void *left = L + 16 * es;
  const void *x1 = L + 80 * es;
  const void *right = R + (rhdr - 64) * es;
  const void *x2 = R + rhdr * es;
  return plf_dev(ctx, dtype, x1, x2, out_clv, EV, alignment_sites, left, right, nullptr, out_scaler, nullptr,
                 stream);
}

int plfx_instance_run_host(plfx_ctx *ctx, const void *in_left, const void *in_right,
                           void *out_clv, uint8_t *out_scaler, uint32_t alignment_sites,
                           uint32_t window_size, int layout, int dtype) {
  PLFX_BIND(ctx);
  if (layout != PLFX_LAYOUT_COMBINED && layout != PLFX_LAYOUT_SEPARATE)
    return fail(ctx, PLFX_ERR_INVALID, "bad layout %d", layout);
  if (int rc = check_dtype(ctx, dtype); rc != PLFX_OK) return rc;
  if (!in_left || !in_right || (alignment_sites > 0 && !out_clv))
    return fail(ctx, PLFX_ERR_INVALID, "null instance buffer");
  const size_t es = dtype == PLFX_F32 ? 4 : 8, n = alignment_sites;
  const size_t lbytes = (80 + 16 * n) * es;                                        // active prefix of in_left
  const size_t rbytes = ((layout == PLFX_LAYOUT_COMBINED ? 80 : 64) + 16 * n) * es;  // and of in_right
  const size_t obytes = 16 * n * es;
  const size_t o_l = 0, o_r = round_up(lbytes, 256), o_o = o_r + round_up(rbytes, 256);
  const size_t o_s = o_o + round_up(obytes, 256);
  int rc = ensure_dbuf(ctx, o_s + round_up(std::max<size_t>(n, 1), 256));
  if (rc != PLFX_OK) return rc;
  char *d = static_cast<char *>(ctx->d_buf);
  hipStream_t s = ctx->stream;
  PLFX_HIP(ctx, hipMemcpyAsync(d + o_l, in_left, lbytes, hipMemcpyHostToDevice, s));
  PLFX_HIP(ctx, hipMemcpyAsync(d + o_r, in_right, rbytes, hipMemcpyHostToDevice, s));
  rc = plfx_instance_run(ctx, d + o_l, d + o_r, d + o_o, out_scaler ? (uint8_t *)(d + o_s) : nullptr,
                         alignment_sites, window_size, layout, dtype, s);
  if (rc != PLFX_OK) return rc;
  if (n > 0) {
    PLFX_HIP(ctx, hipMemcpyAsync(out_clv, d + o_o, obytes, hipMemcpyDeviceToHost, s));
    if (out_scaler) PLFX_HIP(ctx, hipMemcpyAsync(out_scaler, d + o_s, n, hipMemcpyDeviceToHost, s));
  }
  PLFX_HIP(ctx, hipStreamSynchronize(s));
  return PLFX_OK;
}

int plfx_plf_batch_dev(plfx_ctx *ctx, int dtype, int states, const plfx_node *nodes, int count,
                       const void *EV, int64_t n, const int32_t *wgt, void *stream) {
  PLFX_BIND(ctx);
  if (int rc = check_dtype(ctx, dtype); rc != PLFX_OK) return rc;
  if (states != 4 && states != 20)
    return fail(ctx, PLFX_ERR_UNSUPPORTED, "batched nodes: states=%d not built (4, 20)", states);
  // DNA batches share the resident grid with the batches of the other
  // streams in flight (plfx_ctx_set_streams)
  const ExecCall call{dtype, states, PLFX_EXACT, EV, n, wgt, /*tipvec*/ nullptr, pick(stream), ctx->streams};
  return run_batch(ctx, call, nodes, count, 0);
}

int plfx_plf_tips_dev_gen(plfx_ctx *ctx, int dtype, int states, int flags, const uint8_t *tip1,
                          const void *x1, const uint8_t *tip2, const void *x2, void *x3,
                          const void *EV, int64_t n, const void *left, const void *right,
                          const int32_t *wgt, uint8_t *scaler, int64_t *scaler_sum,
                          const void *tipvec, void *stream) {
  PLFX_BIND(ctx);
  if (int rc = check_dtype(ctx, dtype); rc != PLFX_OK) return rc;
  if (states != 4 && states != 20)
    return fail(ctx, PLFX_ERR_UNSUPPORTED, "states=%d not built (4, 20)", states);
  if (flags & ~PLFX_FMA) return fail(ctx, PLFX_ERR_INVALID, "bad flags %d", flags);
  if ((tip1 != nullptr) == (x1 != nullptr) || (tip2 != nullptr) == (x2 != nullptr))
    return fail(ctx, PLFX_ERR_INVALID, "each child needs exactly one of tip / CLV");
  // dense/tip runs as tip/dense: u1*u2 == u2*u1 exactly
  const plfx::OpNode o = plfx::tip_first({{tip1 ? (const void *)tip1 : x1, tip2 ? (const void *)tip2 : x2, x3, left,
                                           right, scaler, scaler_sum}, tip1 != nullptr, tip2 != nullptr});
  const ExecCall call{dtype, states, flags, EV, n, wgt, tipvec, pick(stream), /*streams*/ 1};
  return run_batch(ctx, call, &o.nd, 1, o.t1 + o.t2);
}

int plfx_plf_tips_dev(plfx_ctx *ctx, int dtype, const uint8_t *tip1, const void *x1,
                      const uint8_t *tip2, const void *x2, void *x3, const void *EV, int64_t n,
                      const void *left, const void *right, const int32_t *wgt, uint8_t *scaler,
                      int64_t *scaler_sum, const void *tipvec, void *stream) {
  return plfx_plf_tips_dev_gen(ctx, dtype, 4, PLFX_EXACT, tip1, x1, tip2, x2, x3, EV, n, left,
                               right, wgt, scaler, scaler_sum, tipvec, stream);
}

int plfx_traverse(plfx_ctx *ctx, int dtype, int states, const plfx_trav_op *ops, int nops,
                  void *const *clv, int nslots, const void *pmats, int npmats, const void *EV,
                  int64_t n, const int32_t *wgt, uint8_t *const *scalers, int64_t *scaler_sums,
                  void *stream) {
  return plfx_traverse_tips(ctx, dtype, states, PLFX_EXACT, ops, nops, clv, nullptr, nslots, pmats,
                            npmats, EV, n, wgt, scalers, scaler_sums, nullptr, stream);
}

int plfx_traverse_tips(plfx_ctx *ctx, int dtype, int states, int flags, const plfx_trav_op *ops,
                       int nops,
                       void *const *clv, const uint8_t *const *tips, int nslots, const void *pmats,
                       int npmats, const void *EV, int64_t n, const int32_t *wgt,
                       uint8_t *const *scalers, int64_t *scaler_sums, const void *tipvec,
                       void *stream) {
  PLFX_BIND(ctx);
  for (int &c : ctx->sched) c = 0;
  if (states != 4 && states != 20)
    return fail(ctx, PLFX_ERR_UNSUPPORTED, "traverse: states=%d not built (4, 20)", states);
  if (int rc = check_dtype(ctx, dtype); rc != PLFX_OK) return rc;
  if (flags & ~PLFX_FMA) return fail(ctx, PLFX_ERR_INVALID, "bad flags %d", flags);
  if (nops < 0 || (nops > 0 && (!ops || !clv || !pmats || !EV)))
    return fail(ctx, PLFX_ERR_INVALID, "bad traverse arguments");
  if (n < 0) return fail(ctx, PLFX_ERR_INVALID, "n < 0 (%lld)", (long long)n);
  plfx::TravPlan plan;
  if (int rc = plan_call(ctx, ops, nops, tips, nslots, npmats, states, ctx->fuse, &plan); rc != PLFX_OK) return rc;
  hipStream_t s = pick(stream);
  if (n == 0 || nops == 0) {  // nothing to launch
    const int rc = zero_sums(ctx, s, scaler_sums, nops);
    return rc != PLFX_OK ? rc : publish_sched(ctx, plan, 0);
  }
  // lower: every node checked, every descriptor filled, before the first launch
  PLFX_WS(ctx, s, w);
  const plfx::TravArrays arrays{ops, nops, clv, tips, pmats, scalers, scaler_sums};
  if (plfx::traversal_uses_tables(arrays, states))
    if (int rc = ensure_tables(ctx, w, s); rc != PLFX_OK) return rc;
  const plfx::LowerCall lc{dtype, states, n, w->tt, ctx->tt_codes};
  std::string err;
  if (plfx::lower_traversal(plan, arrays, lc, &ctx->lowered, &err) != PLFX_OK)
    return fail(ctx, PLFX_ERR_INVALID, "%s", err.c_str());
  // execute: level by level, the level's fused groups first
  const ExecCall call{dtype, states, flags, EV, n, wgt, tipvec, s, /*streams*/ 1};
  if (int rc = execute(ctx, ctx->lowered, call, w->ws); rc != PLFX_OK) return rc;
  return publish_sched(ctx, plan, ctx->lowered.launches());
}

int plfx_traverse_schedule(const plfx_ctx *ctx, int *counts, int ncounts) {
  if (!ctx || (ncounts > 0 && !counts)) return 0;
  std::lock_guard<std::recursive_mutex> lock(ctx->mu);
  const int m = std::min(ncounts, PLFX_SCHED_COUNTS);
  for (int i = 0; i < m; i++) counts[i] = ctx->sched[i];
  return m < 0 ? 0 : m;
}

int plfx_root_lnl(plfx_ctx *ctx, int dtype, int states, const void *x, int64_t n,
                  const double *catw, const double *freq, const int32_t *wgt,
                  const int64_t *scaler_sums, int nsums, double *out_lnl, double *site_lnl,
                  void *stream) {
  PLFX_BIND(ctx);
  if (int rc = check_dtype(ctx, dtype); rc != PLFX_OK) return rc;
  if (states != 4 && states != 20) return fail(ctx, PLFX_ERR_UNSUPPORTED, "lnl: states=%d", states);
  if (int rc = check_sums_args(ctx, "root_lnl", out_lnl && n >= 0 && (n == 0 || x), scaler_sums, nsums); rc != PLFX_OK)
    return rc;
  hipStream_t s = pick(stream);
  if (n == 0) {
    const int rc = zero_sums(ctx, s, out_lnl, 1);
    if (rc != PLFX_OK || nsums == 0) return rc;
  }
  PLFX_WS(ctx, s, w);
  hipError_t e = plfx::launch_root_lnl(dtype, states, x, n, catw, freq, wgt, scaler_sums, nsums,
                                       w->lnl_partials, w->lnl_ticket, out_lnl, site_lnl, s);
  if (e != hipSuccess) return hip_fail(ctx, e, "root_lnl launch");
  return PLFX_OK;
}

int plfx_scaler_sum(plfx_ctx *ctx, const uint8_t *scaler, const int32_t *wgt, int64_t n,
                    int64_t *out_sum, void *stream) {
  PLFX_BIND(ctx);
  if (!out_sum || n < 0 || (n > 0 && !scaler)) return fail(ctx, PLFX_ERR_INVALID, "bad scaler_sum args");
  hipStream_t s = pick(stream);
  if (n == 0) return zero_sums(ctx, s, out_sum, 1);
  PLFX_WS(ctx, s, w);
  hipError_t e = plfx::launch_scaler_sum(scaler, wgt, n, out_sum, w->ws, ctx->max_blocks, s);
  if (e != hipSuccess) return hip_fail(ctx, e, "scaler_sum launch");
  return PLFX_OK;
}

int plfx_pmatrix(plfx_ctx *ctx, int dtype, int states, int convention, const double *eigen,
                 const double *rates, int ncat, const double *blen, int64_t nbranch, void *pmats,
                 void *stream) {
  PLFX_BIND(ctx);
  if (int rc = check_dtype(ctx, dtype); rc != PLFX_OK) return rc;
  if (convention != PLFX_PMAT_STATE && convention != PLFX_PMAT_EIGEN)
    return fail(ctx, PLFX_ERR_INVALID, "bad convention %d", convention);
  if (states < 2 || states > 64 || ncat < 1 || nbranch < 0)
    return fail(ctx, PLFX_ERR_INVALID, "bad pmatrix sizes (states %d, ncat %d)", states, ncat);
  if (nbranch == 0) return PLFX_OK;
  if (!eigen || !rates || !blen || !pmats) return fail(ctx, PLFX_ERR_INVALID, "null pmatrix pointer");
  hipError_t e = plfx::launch_pmatrix(dtype, convention == PLFX_PMAT_EIGEN, eigen, states, rates,
                                      ncat, blen, nbranch, pmats, pick(stream));
  if (e != hipSuccess) return hip_fail(ctx, e, "pmatrix launch");
  return PLFX_OK;
}

int plfx_edge_sumtable(plfx_ctx *ctx, int dtype, int states, const uint8_t *tip1, const void *x1,
                       const void *x2, int64_t n, const void *tipvec, void *sumtab, void *stream) {
  PLFX_BIND(ctx);
  if (int rc = check_dtype(ctx, dtype); rc != PLFX_OK) return rc;
  if (states != 4 && states != 20)
    return fail(ctx, PLFX_ERR_UNSUPPORTED, "edge_sumtable: states=%d not built (4, 20)", states);
  const int rc = check_sumtable_args(ctx, tip1, x1, x2, n, tipvec, sumtab, clv_bytes_of(dtype, states, n));
  if (rc != PLFX_OK || n == 0) return rc;
  hipError_t e = plfx::launch_edge_sumtable(dtype, states, tip1 != nullptr, tip1 ? (const void *)tip1 : x1, x2,
                                            n, tipvec, sumtab, ctx->max_blocks, pick(stream));
  if (e != hipSuccess) return hip_fail(ctx, e, "edge_sumtable launch");
  return PLFX_OK;
}

int plfx_edge_derivatives(plfx_ctx *ctx, int dtype, int states, const void *sumtab, int64_t n,
                          const double *eigen, const double *rates, int ncat, const double *catw,
                          const int32_t *wgt, const double *t, const int64_t *scaler_sums, int nsums,
                          double *out3, double *site_lnl, void *stream) {
  PLFX_BIND(ctx);
  if (int rc = check_edge_args(ctx, dtype, states, sumtab, n, eigen, rates, ncat); rc != PLFX_OK) return rc;
  if (int rc = check_sums_args(ctx, "edge_derivatives", t && out3, scaler_sums, nsums); rc != PLFX_OK) return rc;
  hipStream_t s = pick(stream);
  PLFX_WS(ctx, s, w);
  // n == 0 launches too: one block, out3 = {correction, 0, 0}
  hipError_t e = plfx::launch_edge_derivatives(dtype, states, sumtab, n, eigen, rates, catw, wgt, t, scaler_sums,
                                               nsums, w->lnl_partials, w->lnl_ticket, out3, site_lnl,
                                               ctx->max_blocks, s);
  if (e != hipSuccess) return hip_fail(ctx, e, "edge_derivatives launch");
  return PLFX_OK;
}

int plfx_edge_optimize(plfx_ctx *ctx, int dtype, int states, const void *sumtab, int64_t n,
                       const double *eigen, const double *rates, int ncat, const double *catw,
                       const int32_t *wgt, double t0, double tmin, double tmax, int max_evals,
                       double *t_opt, double *out3_host, int *evals, void *stream) {
  PLFX_BIND(ctx);
  if (int rc = check_edge_args(ctx, dtype, states, sumtab, n, eigen, rates, ncat); rc != PLFX_OK) return rc;
  return edge_newton_loop(ctx, "edge_optimize", t0, tmin, tmax, max_evals, t_opt, out3_host, evals, pick(stream),
                          [&](const double *d_t, double *d_out) {
                            return plfx_edge_derivatives(ctx, dtype, states, sumtab, n, eigen, rates, ncat, catw, wgt,
                                                         d_t, nullptr, 0, d_out, nullptr, stream);
                          });
}

int plfx_edge_optimize_dev(plfx_ctx *ctx, int dtype, int states, const void *const *sumtabs, int nedges,
                           int64_t n, const double *eigen, const double *rates, int ncat, const double *catw,
                           const int32_t *wgt, const double *t0, double tmin, double tmax, int max_evals,
                           double *t_opt, double *out3, int32_t *evals, void *stream) {
  PLFX_BIND(ctx);
  return edge_optimize_dev(
      ctx, "edge_optimize_dev", sumtabs, nedges, t0, tmin, tmax, max_evals, t_opt, stream,
      [&](const void *st) { return check_edge_args(ctx, dtype, states, st, n, eigen, rates, ncat); },
      [&](int g, int c, StreamWs *w, hipStream_t s) {
        return plfx::launch_edge_optimize(dtype, states, sumtabs + g, c, n, eigen, rates, catw, wgt, t0 + g, tmin, tmax,
                                          max_evals, w->edge_state, w->lnl_partials, w->ws, t_opt + g,
                                          out3 ? out3 + 3 * (size_t)g : nullptr, evals ? evals + g : nullptr,
                                          ctx->max_blocks, s);
      });
}

// ---- (11) per-site rate categories; (11b), (11c) the same with a state count ----

// Each entry point of section 11 is its _gen twin with 4 states.  The _gen
// entry points: states 4 runs plf_psr.hip's launchers, states 20
// plf_psr_prot.hip's; the checks, the host loop and the workspace regions are
// shared.

int plfx_plf_psr_dev(plfx_ctx *ctx, int dtype, const plfx_psr_node *nodes, int count, const void *EV,
                     int64_t n, const uint8_t *rate_cat, int ncat, const int32_t *wgt, const void *tipvec,
                     void *stream) {
  return plfx_plf_psr_dev_gen(ctx, dtype, 4, nodes, count, EV, n, rate_cat, ncat, wgt, tipvec, stream);
}

int plfx_traverse_psr(plfx_ctx *ctx, int dtype, const plfx_trav_op *ops, int nops, void *const *clv,
                      const uint8_t *const *tips, int nslots, const void *pmats, int npmats,
                      const void *EV, int64_t n, const uint8_t *rate_cat, int ncat, const int32_t *wgt,
                      uint8_t *const *scalers, int64_t *scaler_sums, const void *tipvec, void *stream) {
  return plfx_traverse_psr_gen(ctx, dtype, 4, ops, nops, clv, tips, nslots, pmats, npmats, EV, n, rate_cat, ncat, wgt,
                               scalers, scaler_sums, tipvec, stream);
}

int plfx_root_lnl_psr(plfx_ctx *ctx, int dtype, const void *x, int64_t n, const double *freq,
                      const int32_t *wgt, const int64_t *scaler_sums, int nsums, double *out_lnl,
                      double *site_lnl, void *stream) {
  return plfx_root_lnl_psr_gen(ctx, dtype, 4, x, n, freq, wgt, scaler_sums, nsums, out_lnl, site_lnl, stream);
}

int plfx_edge_sumtable_psr(plfx_ctx *ctx, int dtype, const uint8_t *tip1, const void *x1, const void *x2,
                           int64_t n, const void *tipvec, void *sumtab, void *stream) {
  return plfx_edge_sumtable_psr_gen(ctx, dtype, 4, tip1, x1, x2, n, tipvec, sumtab, stream);
}

int plfx_edge_derivatives_psr(plfx_ctx *ctx, int dtype, const void *sumtab, int64_t n, const double *eigen,
                              const double *rates, int ncat, const uint8_t *rate_cat, const int32_t *wgt,
                              const double *t, const int64_t *scaler_sums, int nsums, double *out3,
                              double *site_lnl, void *stream) {
  return plfx_edge_derivatives_psr_gen(ctx, dtype, 4, sumtab, n, eigen, rates, ncat, rate_cat, wgt, t, scaler_sums,
                                       nsums, out3, site_lnl, stream);
}

int plfx_edge_optimize_psr(plfx_ctx *ctx, int dtype, const void *sumtab, int64_t n, const double *eigen,
                           const double *rates, int ncat, const uint8_t *rate_cat, const int32_t *wgt,
                           double t0, double tmin, double tmax, int max_evals, double *t_opt,
                           double *out3_host, int *evals, void *stream) {
  return plfx_edge_optimize_psr_gen(ctx, dtype, 4, sumtab, n, eigen, rates, ncat, rate_cat, wgt, t0, tmin, tmax,
                                    max_evals, t_opt, out3_host, evals, stream);
}

int plfx_edge_optimize_psr_dev(plfx_ctx *ctx, int dtype, const void *const *sumtabs, int nedges, int64_t n,
                               const double *eigen, const double *rates, int ncat, const uint8_t *rate_cat,
                               const int32_t *wgt, const double *t0, double tmin, double tmax, int max_evals,
                               double *t_opt, double *out3, int32_t *evals, void *stream) {
  return plfx_edge_optimize_psr_dev_gen(ctx, dtype, 4, sumtabs, nedges, n, eigen, rates, ncat, rate_cat, wgt, t0, tmin,
                                        tmax, max_evals, t_opt, out3, evals, stream);
}

int plfx_edge_sumtable_psr_batch(plfx_ctx *ctx, int dtype, const plfx_psr_edge *edges, int nedges, int64_t n,
                                 const void *tipvec, void *stream) {
  return plfx_edge_sumtable_psr_batch_gen(ctx, dtype, 4, edges, nedges, n, tipvec, stream);
}

int plfx_plf_psr_dev_gen(plfx_ctx *ctx, int dtype, int states, const plfx_psr_node *nodes, int count,
                         const void *EV, int64_t n, const uint8_t *rate_cat, int ncat, const int32_t *wgt,
                         const void *tipvec, void *stream) {
  return plfx_plf_psr_dev_ex(ctx, dtype, states, 0, nodes, count, EV, n, rate_cat, ncat, wgt, tipvec, stream);
}

// ---- (11d) the _ex entry points: the _gen calls with flags; flags 0 is the _gen call ----

int plfx_plf_psr_dev_ex(plfx_ctx *ctx, int dtype, int states, int flags, const plfx_psr_node *nodes, int count,
                        const void *EV, int64_t n, const uint8_t *rate_cat, int ncat, const int32_t *wgt,
                        const void *tipvec, void *stream) {
  PLFX_BIND(ctx);
  if (int rc = check_psr_states(ctx, states); rc != PLFX_OK) return rc;
  int mode;
  if (int rc = check_psr_flags(ctx, "plf_psr_dev_ex", dtype, states, flags, &mode); rc != PLFX_OK) return rc;
  static_assert(PLFX_PSR_MAX_CATS <= 256, "a category is one byte");
  std::string err;
  const plfx::PsrCall call{dtype, n, ncat, EV, rate_cat, states, mode};
  if (plfx::lower_psr(call, nodes, count, &ctx->psr_lowered, &err) != PLFX_OK)
    return fail(ctx, PLFX_ERR_INVALID, "%s", err.c_str());
  hipStream_t s = pick(stream);
  if (n == 0) return zero_node_sums(ctx, s, nodes, count);
  PLFX_WS(ctx, s, w);
  return execute_psr(ctx, ctx->psr_lowered, call, wgt, tipvec, s, w->ws);
}

int plfx_traverse_psr_gen(plfx_ctx *ctx, int dtype, int states, const plfx_trav_op *ops, int nops,
                          void *const *clv, const uint8_t *const *tips, int nslots, const void *pmats,
                          int npmats, const void *EV, int64_t n, const uint8_t *rate_cat, int ncat,
                          const int32_t *wgt, uint8_t *const *scalers, int64_t *scaler_sums, const void *tipvec,
                          void *stream) {
  return plfx_traverse_psr_ex(ctx, dtype, states, 0, ops, nops, clv, tips, nslots, pmats, npmats, EV, n, rate_cat,
                              ncat, wgt, scalers, scaler_sums, tipvec, stream);
}

int plfx_traverse_psr_ex(plfx_ctx *ctx, int dtype, int states, int flags, const plfx_trav_op *ops, int nops,
                         void *const *clv, const uint8_t *const *tips, int nslots, const void *pmats, int npmats,
                         const void *EV, int64_t n, const uint8_t *rate_cat, int ncat, const int32_t *wgt,
                         uint8_t *const *scalers, int64_t *scaler_sums, const void *tipvec, void *stream) {
  PLFX_BIND(ctx);
  if (int rc = check_psr_states(ctx, states); rc != PLFX_OK) return rc;
  int mode;
  if (int rc = check_psr_flags(ctx, "traverse_psr_ex", dtype, states, flags, &mode); rc != PLFX_OK) return rc;
  for (int &c : ctx->sched) c = 0;
  if (nops < 0 || (nops > 0 && (!ops || !clv))) return fail(ctx, PLFX_ERR_INVALID, "bad traverse_psr arguments");
  // level pairs alone: the deeper passes of entries 0..3 of the schedule are not built for PSR;
  // with 20 states there is no level pair either, whatever PLFX_FUSE says
  plfx::TravPlan plan;
  const int fuse = states == 4 ? std::min(ctx->psr_fuse, 1) : 0;
  if (int rc = plan_call(ctx, ops, nops, tips, nslots, npmats, states, fuse, &plan); rc != PLFX_OK) return rc;
  // lower: the call, every op and every level pair checked, every descriptor
  // filled, before the first launch
  const plfx::TravArrays arrays{ops, nops, clv, tips, pmats, scalers, scaler_sums};
  const plfx::PsrCall call{dtype, n, ncat, EV, rate_cat, states, mode};
  std::string err;
  if (plfx::lower_psr_traversal(plan, arrays, call, &ctx->psr_lowered, &err) != PLFX_OK)
    return fail(ctx, PLFX_ERR_INVALID, "%s", err.c_str());
  hipStream_t s = pick(stream);
  if (n == 0 || nops == 0) {  // nothing to launch
    const int rc = zero_sums(ctx, s, scaler_sums, nops);
    return rc != PLFX_OK ? rc : publish_sched(ctx, plan, 0);
  }
  PLFX_WS(ctx, s, w);
  if (int rc = execute_psr(ctx, ctx->psr_lowered, call, wgt, tipvec, s, w->ws); rc != PLFX_OK) return rc;
  return publish_sched(ctx, plan, ctx->psr_lowered.launches());
}

int plfx_root_lnl_psr_gen(plfx_ctx *ctx, int dtype, int states, const void *x, int64_t n, const double *freq,
                          const int32_t *wgt, const int64_t *scaler_sums, int nsums, double *out_lnl,
                          double *site_lnl, void *stream) {
  PLFX_BIND(ctx);
  if (int rc = check_psr_states(ctx, states); rc != PLFX_OK) return rc;
  if (int rc = check_dtype(ctx, dtype); rc != PLFX_OK) return rc;
  if (int rc = check_sums_args(ctx, "root_lnl_psr", out_lnl && n >= 0 && (n == 0 || x), scaler_sums, nsums);
      rc != PLFX_OK)
    return rc;
  if (!aligned16(x)) return fail(ctx, PLFX_ERR_INVALID, "the CLV must be 16-byte aligned");
  hipStream_t s = pick(stream);
  if (n == 0) {
    const int rc = zero_sums(ctx, s, out_lnl, 1);
    if (rc != PLFX_OK || nsums == 0) return rc;
  }
  PLFX_WS(ctx, s, w);
  const auto launch = states == 4 ? plfx::launch_root_lnl_psr : plfx::launch_root_lnl_psr_prot;
  hipError_t e = launch(dtype, x, n, freq, wgt, scaler_sums, nsums, w->lnl_partials, w->lnl_ticket, out_lnl,
                        site_lnl, ctx->max_blocks, s);
  if (e != hipSuccess) return hip_fail(ctx, e, "root_lnl_psr launch");
  return PLFX_OK;
}

int plfx_edge_sumtable_psr_gen(plfx_ctx *ctx, int dtype, int states, const uint8_t *tip1, const void *x1,
                               const void *x2, int64_t n, const void *tipvec, void *sumtab, void *stream) {
  PLFX_BIND(ctx);
  if (int rc = check_psr_states(ctx, states); rc != PLFX_OK) return rc;
  if (int rc = check_dtype(ctx, dtype); rc != PLFX_OK) return rc;
  const int rc = check_sumtable_args(ctx, tip1, x1, x2, n, tipvec, sumtab, plfx::psr_clv_bytes(dtype, n, states));
  if (rc != PLFX_OK || n == 0) return rc;
  const auto launch = states == 4 ? plfx::launch_edge_sumtable_psr : plfx::launch_edge_sumtable_psr_prot;
  hipError_t e = launch(dtype, tip1 != nullptr, tip1 ? (const void *)tip1 : x1, x2, n, tipvec, sumtab,
                        ctx->max_blocks, pick(stream));
  if (e != hipSuccess) return hip_fail(ctx, e, "edge_sumtable_psr launch");
  return PLFX_OK;
}

int plfx_edge_sumtable_psr_batch_gen(plfx_ctx *ctx, int dtype, int states, const plfx_psr_edge *edges, int nedges,
                                     int64_t n, const void *tipvec, void *stream) {
  PLFX_BIND(ctx);
  if (int rc = check_psr_states(ctx, states); rc != PLFX_OK) return rc;
  std::string err;
  plfx::PsrEdgeLaunchList &l = ctx->psr_edges_lowered;
  if (plfx::lower_psr_edges(dtype, n, tipvec, edges, nedges, &l, &err, states) != PLFX_OK)
    return fail(ctx, PLFX_ERR_INVALID, "%s", err.c_str());
  hipStream_t s = pick(stream);
  const auto launch = states == 4 ? plfx::launch_edge_sumtable_psr_batch : plfx::launch_edge_sumtable_psr_prot_batch;
  for (const plfx::PsrEdgeLaunch &it : l.items) {  // none when n == 0
    hipError_t e = launch(dtype, it.tip != 0, &l.edges[it.first], it.count, n, tipvec, ctx->max_blocks, s);
    if (e != hipSuccess) return hip_fail(ctx, e, "edge_sumtable_psr_batch launch");
  }
  return PLFX_OK;
}

int plfx_edge_derivatives_psr_gen(plfx_ctx *ctx, int dtype, int states, const void *sumtab, int64_t n,
                                  const double *eigen, const double *rates, int ncat, const uint8_t *rate_cat,
                                  const int32_t *wgt, const double *t, const int64_t *scaler_sums, int nsums,
                                  double *out3, double *site_lnl, void *stream) {
  PLFX_BIND(ctx);
  if (int rc = check_psr_states(ctx, states); rc != PLFX_OK) return rc;
  if (int rc = check_psr_edge_args(ctx, dtype, sumtab, n, eigen, rates, ncat, rate_cat); rc != PLFX_OK) return rc;
  if (int rc = check_sums_args(ctx, "edge_derivatives_psr", t && out3, scaler_sums, nsums); rc != PLFX_OK) return rc;
  hipStream_t s = pick(stream);
  PLFX_WS(ctx, s, w);
  // n == 0 launches too: one block, out3 = {correction, 0, 0}
  const auto launch = states == 4 ? plfx::launch_edge_derivatives_psr : plfx::launch_edge_derivatives_psr_prot;
  hipError_t e = launch(dtype, sumtab, n, eigen, rates, ncat, rate_cat, wgt, t, scaler_sums, nsums, w->lnl_partials,
                        w->lnl_ticket, out3, site_lnl, ctx->max_blocks, s);
  if (e != hipSuccess) return hip_fail(ctx, e, "edge_derivatives_psr launch");
  return PLFX_OK;
}

int plfx_edge_optimize_psr_gen(plfx_ctx *ctx, int dtype, int states, const void *sumtab, int64_t n,
                               const double *eigen, const double *rates, int ncat, const uint8_t *rate_cat,
                               const int32_t *wgt, double t0, double tmin, double tmax, int max_evals,
                               double *t_opt, double *out3_host, int *evals, void *stream) {
  PLFX_BIND(ctx);
  if (int rc = check_psr_states(ctx, states); rc != PLFX_OK) return rc;
  if (int rc = check_psr_edge_args(ctx, dtype, sumtab, n, eigen, rates, ncat, rate_cat); rc != PLFX_OK) return rc;
  return edge_newton_loop(ctx, "edge_optimize_psr", t0, tmin, tmax, max_evals, t_opt, out3_host, evals, pick(stream),
                          [&](const double *d_t, double *d_out) {
                            return plfx_edge_derivatives_psr_gen(ctx, dtype, states, sumtab, n, eigen, rates, ncat,
                                                                 rate_cat, wgt, d_t, nullptr, 0, d_out, nullptr,
                                                                 stream);
                          });
}

int plfx_edge_optimize_psr_dev_gen(plfx_ctx *ctx, int dtype, int states, const void *const *sumtabs, int nedges,
                                   int64_t n, const double *eigen, const double *rates, int ncat,
                                   const uint8_t *rate_cat, const int32_t *wgt, const double *t0, double tmin,
                                   double tmax, int max_evals, double *t_opt, double *out3, int32_t *evals,
                                   void *stream) {
  PLFX_BIND(ctx);
  if (int rc = check_psr_states(ctx, states); rc != PLFX_OK) return rc;
  // the groups run in the regions and under the ordering rule of plfx_edge_optimize_dev
  const auto launch_group = states == 4 ? plfx::launch_edge_optimize_psr : plfx::launch_edge_optimize_psr_prot;
  return edge_optimize_dev(
      ctx, "edge_optimize_psr_dev", sumtabs, nedges, t0, tmin, tmax, max_evals, t_opt, stream,
      [&](const void *st) { return check_psr_edge_args(ctx, dtype, st, n, eigen, rates, ncat, rate_cat); },
      [&](int g, int c, StreamWs *w, hipStream_t s) {
        return launch_group(dtype, sumtabs + g, c, n, eigen, rates, ncat, rate_cat, wgt, t0 + g, tmin, tmax, max_evals,
                            w->edge_state, w->lnl_partials, w->ws, t_opt + g, out3 ? out3 + 3 * (size_t)g : nullptr,
                            evals ? evals + g : nullptr, ctx->max_blocks, s);
      });
}

// ---- (13) all-branch derivatives of a PSR tree ----

int plfx_branch_pair_sites_per_lane(int dtype) {
  return dtype == PLFX_F32 || dtype == PLFX_F64 ? plfx::psr_branch_sites_per_lane(dtype) : 0;
}

int plfx_branch_sumtables_psr_workspace(int dtype, int states, int nops, int64_t n, size_t *bytes) {
  if (int rc = check_psr_states(nullptr, states); rc != PLFX_OK) return rc;
  plfx::BranchLayout lay;
  if (!bytes || plfx::branch_layout(dtype, states, nops, n, &lay) != PLFX_OK) return PLFX_ERR_INVALID;
  *bytes = lay.bytes;
  return PLFX_OK;
}

int plfx_branch_sumtables_psr(plfx_ctx *ctx, int dtype, int states, int flags, const plfx_trav_op *ops, int nops,
                              void *const *clv, const uint8_t *const *tips, int nslots, const void *pmats,
                              int npmats, const void *root_pmat, const void *EV, int64_t n,
                              const uint8_t *rate_cat, int ncat, const int32_t *wgt, const int64_t *scaler_sums,
                              const void *tipvec, void *workspace, size_t workspace_bytes, void **sumtabs_out,
                              int64_t *edge_scale, void *stream) {
  PLFX_BIND(ctx);
  if (int rc = check_psr_states(ctx, states); rc != PLFX_OK) return rc;
  if (flags & ~(PLFX_FMA | PLFX_BRANCH_NOFUSE))
    return fail(ctx, PLFX_ERR_INVALID, "branch_sumtables_psr: bad flags %d", flags);
  int mode;  // the W nodes run in the mode plfx_traverse_psr_ex runs the ops in, and are refused as there
  if (int rc = check_psr_flags(ctx, "branch_sumtables_psr", dtype, states, flags & PLFX_FMA, &mode); rc != PLFX_OK)
    return rc;
  if (!sumtabs_out) return fail(ctx, PLFX_ERR_INVALID, "branch_sumtables_psr: null sumtabs_out");
  // plan: the tree, the call, every node and table checked, every descriptor filled, before the first launch
  plfx::BranchPlan &pl = ctx->branches;
  const plfx::BranchCall call{dtype, states,   flags,        ops,         nops,   clv,       tips,
                              nslots, pmats,   npmats,       root_pmat,   EV,     n,         rate_cat,
                              ncat,   scaler_sums, tipvec,   workspace,   workspace_bytes,   edge_scale};
  std::string err;
  if (plfx::plan_branches(call, &pl, &err) != PLFX_OK) return fail(ctx, PLFX_ERR_INVALID, "%s", err.c_str());
  hipStream_t s = pick(stream);
  if (n == 0) {  // nothing to launch
    if (int rc = zero_sums(ctx, s, edge_scale, 2 * nops); rc != PLFX_OK) return rc;
    std::copy(pl.tab.begin(), pl.tab.end(), sumtabs_out);
    return PLFX_OK;
  }
  PLFX_WS(ctx, s, w);
  std::copy(pl.tab.begin(), pl.tab.end(), sumtabs_out);
  static_assert(2 * plfx::kMaxPairs <= kWsRegions, "two ticket regions per sibling pair");
  int64_t *wsum = reinterpret_cast<int64_t *>(static_cast<char *>(workspace) + pl.lay.cnt_off);
  for (const plfx::BranchLaunch &it : pl.items) {
    hipError_t e = hipErrorInvalidValue;
    switch (it.kind) {
      case plfx::kBranchPairs:
        e = plfx::launch_psr_branch_pairs(dtype, it.tips, &pl.pairs[it.first], it.count, EV, rate_cat, ncat, wgt, n,
                                          tipvec, w->ws, ctx->max_blocks, s);
        break;
      case plfx::kBranchNodes:
        if (states == 20)
          e = mode ? plfx::launch_plf_psr_prot_mfma(it.tips, &pl.nodes[it.first], it.count, EV, rate_cat, ncat, wgt, n,
                                                    tipvec, w->ws, ctx->max_blocks, s)
                   : plfx::launch_plf_psr_prot(dtype, it.tips, &pl.nodes[it.first], it.count, EV, rate_cat, ncat, wgt,
                                               n, tipvec, w->ws, ctx->max_blocks, s);
        else
          e = plfx::launch_plf_psr(dtype, it.tips, &pl.nodes[it.first], it.count, EV, rate_cat, ncat, wgt, n, tipvec,
                                   w->ws, ctx->max_blocks, s);
        break;
      case plfx::kBranchTables:
        e = (states == 4 ? plfx::launch_edge_sumtable_psr_batch : plfx::launch_edge_sumtable_psr_prot_batch)(
            dtype, it.tips != 0, &pl.edges[it.first], it.count, n, tipvec, ctx->max_blocks, s);
        break;
      case plfx::kBranchSub:
      case plfx::kBranchScale:
        e = plfx::launch_psr_branch_counts(it.kind == plfx::kBranchScale, &pl.scale[it.first], it.first, it.count,
                                           scaler_sums, wsum, pl.sub, pl.outer, edge_scale, s);
        break;
    }
    if (e != hipSuccess) return hip_fail(ctx, e, "branch_sumtables_psr launch");
  }
  return PLFX_OK;
}

// ---- (12) the PSR rate scan; (12b) the same with a state count ----

// Each entry point of section 12 is its _gen twin with 4 states, as section
// 11's are.  The _gen entry points: states 4 runs plf_psr.hip's lnL / argmax
// launchers, states 20 plf_psr_prot.hip's; the checks, the lowering, the
// tiling launch and the pass loop are shared.

int plfx_site_lnl_psr(plfx_ctx *ctx, int dtype, const void *x, int64_t n, const double *freq,
                      const uint8_t *scalers, int nsc, int64_t stride, double *site_lnl, void *stream) {
  return plfx_site_lnl_psr_gen(ctx, dtype, 4, x, n, freq, scalers, nsc, stride, site_lnl, stream);
}

int plfx_psr_rate_scan_workspace(int dtype, int nops, int ntips, int npmats, int64_t n, int group, size_t *bytes) {
  return plfx_psr_rate_scan_workspace_gen(dtype, 4, nops, ntips, npmats, n, group, bytes);
}

int plfx_psr_rate_scan(plfx_ctx *ctx, int dtype, const plfx_trav_op *ops, int nops, const uint8_t *const *tips,
                       int nslots, const double *blen, int npmats, const double *eigen, const void *EV,
                       const void *tipvec, const double *cand_rates, int ncand, int group, const double *freq,
                       const int32_t *wgt, int64_t n, void *workspace, size_t workspace_bytes, int32_t *best_idx,
                       double *best_lnl, double *all_lnl, double *out_lnl, void *stream) {
  return plfx_psr_rate_scan_gen(ctx, dtype, 4, ops, nops, tips, nslots, blen, npmats, eigen, EV, tipvec, cand_rates,
                                ncand, group, freq, wgt, n, workspace, workspace_bytes, best_idx, best_lnl, all_lnl,
                                out_lnl, stream);
}

int plfx_site_lnl_psr_gen(plfx_ctx *ctx, int dtype, int states, const void *x, int64_t n, const double *freq,
                          const uint8_t *scalers, int nsc, int64_t stride, double *site_lnl, void *stream) {
  PLFX_BIND(ctx);
  if (int rc = check_psr_states(ctx, states); rc != PLFX_OK) return rc;
  if (int rc = check_dtype(ctx, dtype); rc != PLFX_OK) return rc;
  if (n < 0 || !x || !aligned16(x) || !site_lnl || nsc < 0 || (nsc > 0 && !scalers) || stride < n)
    return fail(ctx, PLFX_ERR_INVALID,
                "site_lnl_psr: needs n >= 0, a 16-byte aligned x, site_lnl, nsc >= 0 rows (non-NULL when nsc > 0) and "
                "stride >= n");
  if (n == 0) return PLFX_OK;
  const auto launch = states == 4 ? plfx::launch_psr_site_lnl : plfx::launch_psr_site_lnl_prot;
  hipError_t e = launch(dtype, x, n, freq, scalers, nsc, stride, site_lnl, ctx->max_blocks, pick(stream));
  if (e != hipSuccess) return hip_fail(ctx, e, "site_lnl_psr launch");
  return PLFX_OK;
}

int plfx_psr_rate_scan_workspace_gen(int dtype, int states, int nops, int ntips, int npmats, int64_t n, int group,
                                     size_t *bytes) {
  if (int rc = check_psr_states(nullptr, states); rc != PLFX_OK) return rc;
  plfx::PsrScanLayout lay;
  if (!bytes || plfx::psr_scan_layout(dtype, nops, ntips, npmats, n, group, &lay, states) != PLFX_OK)
    return PLFX_ERR_INVALID;
  *bytes = lay.end;
  return PLFX_OK;
}

int plfx_psr_rate_scan_gen(plfx_ctx *ctx, int dtype, int states, const plfx_trav_op *ops, int nops,
                           const uint8_t *const *tips, int nslots, const double *blen, int npmats,
                           const double *eigen, const void *EV, const void *tipvec, const double *cand_rates,
                           int ncand, int group, const double *freq, const int32_t *wgt, int64_t n,
                           void *workspace, size_t workspace_bytes, int32_t *best_idx, double *best_lnl,
                           double *all_lnl, double *out_lnl, void *stream) {
  return plfx_psr_rate_scan_ex(ctx, dtype, states, 0, ops, nops, tips, nslots, blen, npmats, eigen, EV, tipvec,
                               cand_rates, ncand, group, freq, wgt, n, workspace, workspace_bytes, best_idx, best_lnl,
                               all_lnl, out_lnl, stream);
}

int plfx_psr_rate_scan_ex(plfx_ctx *ctx, int dtype, int states, int flags, const plfx_trav_op *ops, int nops,
                          const uint8_t *const *tips, int nslots, const double *blen, int npmats,
                          const double *eigen, const void *EV, const void *tipvec, const double *cand_rates,
                          int ncand, int group, const double *freq, const int32_t *wgt, int64_t n, void *workspace,
                          size_t workspace_bytes, int32_t *best_idx, double *best_lnl, double *all_lnl,
                          double *out_lnl, void *stream) {
  PLFX_BIND(ctx);
  if (int rc = check_psr_states(ctx, states); rc != PLFX_OK) return rc;
  int mode;
  if (int rc = check_psr_flags(ctx, "psr_rate_scan_ex", dtype, states, flags, &mode); rc != PLFX_OK) return rc;
  // lower: every check, the workspace carved, the passes and each pass's launch list, before the first launch
  plfx::PsrScanPlan &pl = ctx->psr_scan;
  const plfx::PsrScanCall call{dtype,  ops,        nops,  tips,  nslots, blen,      npmats,          eigen,
                               EV,     tipvec,     cand_rates,   ncand,  group,     n,               workspace,
                               workspace_bytes,    best_idx,     best_lnl,          all_lnl,         out_lnl,
                               ctx->psr_fuse,      states,       mode};
  std::string err;
  if (int rc = plfx::lower_psr_scan(call, &pl, &err); rc != PLFX_OK) return fail(ctx, rc, "%s", err.c_str());
  hipStream_t s = pick(stream);
  if (n == 0) return zero_sums(ctx, s, out_lnl, 1);
  PLFX_WS(ctx, s, w);
  // set-up: the tip codes and the category bytes over the whole group
  const int ntile = (int)pl.tiles.size();
  for (int i = 0; i == 0 || i < ntile; i += plfx::kMaxBatch) {
    hipError_t e = plfx::launch_psr_tile(ntile ? &pl.tiles[(size_t)i] : nullptr, std::min(plfx::kMaxBatch, ntile - i),
                                         n, group, i == 0 ? pl.cat : nullptr, ctx->max_blocks, s);
    if (e != hipSuccess) return hip_fail(ctx, e, "psr_rate_scan tiling launch");
  }
  // passes, one after the other on the stream: each reuses the CLVs, scaler rows and matrices
  const auto launch_pass = states == 4 ? plfx::launch_psr_scan_pass : plfx::launch_psr_scan_pass_prot;
  for (size_t p = 0; p < pl.passes.size(); p++) {
    const plfx::PsrScanPass &ps = pl.passes[p];
    hipError_t e = plfx::launch_pmatrix(dtype, true, eigen, states, cand_rates + ps.k0, ps.gc, blen,
                                        2 * (int64_t)npmats, pl.pmats, s);
    if (e != hipSuccess) return hip_fail(ctx, e, "psr_rate_scan pmatrix launch");
    const plfx::PsrCall pc{dtype, (int64_t)ps.gc * n, ps.gc, EV, pl.cat, states, call.flags};
    if (int rc = execute_psr(ctx, ps.tail ? pl.tail : pl.full, pc, nullptr, tipvec, s, w->ws); rc != PLFX_OK) return rc;
    const bool last = p + 1 == pl.passes.size();
    e = launch_pass(dtype, pl.root, n, ps.gc, freq, pl.scalers, nops, pl.sc_stride, ps.k0, p == 0, all_lnl, best_lnl,
                    best_idx, wgt, w->lnl_partials, w->lnl_ticket, last ? out_lnl : nullptr, ctx->max_blocks, s);
    if (e != hipSuccess) return hip_fail(ctx, e, "psr_rate_scan lnl launch");
  }
  return PLFX_OK;
}

}  // extern "C"
