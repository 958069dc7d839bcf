// stream_ws.cpp -- see stream_ws.hpp.
#include "stream_ws.hpp"

#include "../../include/plfx.h"

namespace plfx {

StreamWs *WsPool::find(const void *stream, const void *tid) {
  tid = key_tid(stream, tid);
  for (StreamWs &w : wss_)
    if (w.in_use && !w.retired && w.stream == stream && w.tid == tid) return &w;
  return nullptr;
}

WsPool::Acquired WsPool::acquire(const void *stream, const void *tid, bool capturing) {
  Answer how = kHeld;
  StreamWs *got = find(stream, tid);
  if (!got)
    for (StreamWs &w : wss_)
      if (!w.in_use) {
        w.in_use = true;
        w.retired = false;
        w.captured = false;
        w.stream = stream;
        w.tid = key_tid(stream, tid);
        how = kTaken;
        got = &w;
        break;
      }
  if (got) {
    got->captured = got->captured || capturing;
    got->cap_now = capturing;
    return {how, got};
  }
  // entries of exited threads' per-thread streams (not captured: those stay
  // retired): their last launches must be done before reuse, and the thread's
  // stream is gone -- so the device is waited for, which a capture forbids
  if (!capturing)
    for (const StreamWs &w : wss_)
      if (w.in_use && w.retired && !w.captured) return {kReclaim, nullptr};
  if ((int)wss_.size() >= PLFX_MAX_STREAMS) return {kTooMany, nullptr};
  if (capturing) return {kCapturing, nullptr};
  return {kAllocate, nullptr};
}

void WsPool::reclaim() {
  for (StreamWs &w : wss_)
    if (w.in_use && w.retired && !w.captured) w.in_use = false;
}

void WsPool::add(const StreamWs &w) {
  StreamWs e;
  e.ws = w.ws;
  e.lnl_partials = w.lnl_partials;
  e.lnl_ticket = w.lnl_ticket;
  e.edge_state = w.edge_state;
  e.tt = w.tt;
  wss_.push_back(e);
}

void WsPool::release(StreamWs *w) {
  if (w->captured) w->retired = true;
  else w->in_use = false;
  w->stream = nullptr;
  w->tid = nullptr;
}

void WsPool::orphan(const void *tid) {
  for (StreamWs &w : wss_)
    if (w.in_use && !w.retired && w.stream == per_thread_ && w.tid == tid) {
      w.retired = true;
      w.stream = nullptr;
      w.tid = nullptr;
    }
}

bool WsPool::needs_device_wait(const void *own_stream) const {
  for (const StreamWs &w : wss_)
    if (w.in_use && (w.captured || w.retired || w.stream != own_stream)) return true;
  return false;
}

}  // namespace plfx
