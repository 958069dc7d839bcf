// stream_ws.hpp -- the per-stream reduction workspaces of a context: which
// stream holds which entry, and when an entry may change hands (plfx.h,
// "Streams and the scaler-sum workspace").  Plain C++: no GPU, no context; a
// stream is an opaque handle and the device pointers of an entry are stored,
// never followed (tests/stream_ws_main.cpp drives it on the CPU).
// plfx_api.hip does what the answers here ask for: the device wait, the
// allocation, the error texts.  Not thread-safe: the caller holds the
// context's lock.
#pragma once
#include <deque>

namespace plfx {

// Scaler-sum / lnL reduction workspace of one stream (plf_dna.hpp
// block_ticket_sum, plf_lnl.hpp): zero at rest, restored to zero by the last
// arriving block of every launch.
class StreamWs {
 public:
  unsigned long long *ws = nullptr;  // kWsRegions x kWsWords u64
  double *lnl_partials = nullptr;    // 3 x kLnlMaxGrid doubles (plf_edge.hpp sums three values per block)
  unsigned long long *lnl_ticket = nullptr;
  void *edge_state = nullptr;  // plfx_edge_optimize_dev: kMaxBatch per-edge stepper states (no rest state)
  // tip/tip protein combination tables (kTtEntryBytes): allocated with the
  // entry, or on first use with PLFX_CTX_LAZY_TABLES (nullptr until then)
  char *tt = nullptr;

  // the stream of the acquire() that returned this entry was capturing
  bool capturing_now() const { return cap_now; }

 private:
  friend class WsPool;
  const void *stream = nullptr;
  const void *tid = nullptr;  // owning thread for the per-thread handle, else none
  bool in_use = false;
  bool captured = false;  // used while its stream was capturing
  bool retired = false;   // released after a capture, or its thread exited
  bool cap_now = false;
};

// One entry per stream, so sum-producing launches on different streams of one
// context may overlap.  The per-thread handle (hipStreamPerThread) is one
// value that names a different stream in every host thread, so its entries
// are keyed by (handle, thread).  The first PLFX_WS_POOL entries are added
// with the context (no allocation on a call path for the first PLFX_WS_POOL
// streams, so a stream's first use may be inside a graph capture); release()
// makes an entry free again -- unless a graph was captured through it: the
// graph's replays keep using the entry's words, so it is retired (never
// handed to another stream).  An entry whose thread exited is retired too,
// but may be reclaimed once the device has been waited for: its stream is
// gone with the thread, so nothing else can wait for its last launches.
class WsPool {
 public:
  enum Answer {
    kHeld,       // entry: the stream's own
    kTaken,      // entry: a free one, now keyed to the stream
    kReclaim,    // wait for the device, reclaim(), acquire again
    kAllocate,   // allocate an entry, add() it, acquire again
    kTooMany,    // refused: PLFX_MAX_STREAMS entries exist and none is free
    kCapturing,  // refused: none is free and a capturing stream may not allocate
  };
  struct Acquired {
    Answer answer;
    StreamWs *entry;  // kHeld, kTaken; else nullptr
  };

  // per_thread: the stream handle that names a stream per host thread
  explicit WsPool(const void *per_thread) : per_thread_(per_thread) {}

  // The entry of `stream` for a call from thread `tid`, or what stands in the
  // way.  An entry returned while capturing is marked: the graph keeps using
  // it after the capture.
  Acquired acquire(const void *stream, const void *tid, bool capturing);
  // frees the entries of exited threads that no graph was captured through;
  // the caller has waited for the device
  void reclaim();
  // a new free entry with w's device pointers
  void add(const StreamWs &w);
  // the entry held by `stream` (for the per-thread handle: by thread `tid`), or nullptr
  StreamWs *find(const void *stream, const void *tid);
  // the holder is done with w (its last launch has finished): free, or
  // retired if a graph was captured through it
  void release(StreamWs *w);
  // thread `tid` exits: its per-thread entries are retired
  void orphan(const void *tid);
  // destroying the context must wait for the whole device, not only for
  // own_stream: an entry is held by another stream, retired, or was captured
  // through (its graph may still be replaying on any stream)
  bool needs_device_wait(const void *own_stream) const;

  int size() const { return (int)wss_.size(); }
  const StreamWs &at(int i) const { return wss_[i]; }

 private:
  const void *key_tid(const void *stream, const void *tid) const {
    return stream == per_thread_ ? tid : nullptr;
  }
  const void *per_thread_;
  std::deque<StreamWs> wss_;  // stable addresses
};

}  // namespace plfx
