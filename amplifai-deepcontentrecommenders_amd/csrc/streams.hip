// Side streams and the orders between streams. A training step is a chain of small kernels, each far
// from filling 256 CUs; the independent branches run concurrently: the user tower beside the item tower
// (forward and backward), and each conv layer's weight gradient beside the dgrad chain of the layers
// below (alternating between two streams, each with its own partial-sum buffers). Forks and joins are
// ordered against the caller's stream -- by events, or on plans by signal words (Edge) -- so the calls
// stay stream-ordered (and capturable).
#include <atomic>

#include "dcue_internal.h"

namespace dcue {

unsigned sync_event_flags() { return hipEventDisableTiming | hipEventReleaseToDevice; }

SidePool* side_pool() {
  static SidePool pools[64];
  int dev = 0;
  if (hipGetDevice(&dev) != hipSuccess || dev < 0 || dev >= 64) return nullptr;
  SidePool& p = pools[dev];
  if (!p.st[0]) {
    for (int i = 0; i < 3; ++i)
      if (hipStreamCreateWithFlags(&p.st[i], hipStreamNonBlocking) != hipSuccess) return nullptr;
    for (auto& e : p.ev)
      if (hipEventCreateWithFlags(&e, sync_event_flags()) != hipSuccess) return nullptr;
  }
  return &p;
}

// A point on `from` that other streams can wait for later (wait_point): a ring event is recorded
// now. The ring is long enough that no event is re-recorded before its waits are enqueued
// (a step records fewer than 16 points).
int fork_point(SidePool* p, hipStream_t from, hipEvent_t* ev) {
  hipEvent_t e = ring_event(p);
  DCUE_HIP_CHECK(hipEventRecord(e, from));
  *ev = e;
  return DCUE_OK;
}

hipEvent_t ring_event(SidePool* p) {
  return p->ev[p->next.fetch_add(1, std::memory_order_relaxed) % SidePool::kEvents];
}

LaunchTag& launch_tag() {
  thread_local LaunchTag t;
  return t;
}
static std::atomic<int64_t> g_launches{0};
void count_launch() { g_launches.fetch_add(1, std::memory_order_relaxed); }
int64_t launches_counted() { return g_launches.load(std::memory_order_relaxed); }
bool& capturing_step() {
  thread_local bool c = false;
  return c;
}

ForkAfter::ForkAfter(SidePool* p, hipStream_t s, hipEvent_t* ev)
    : s_(s), out_(ev), e_(ev ? ring_event(p) : nullptr) {
  if (!ev) return;  // a point nobody waits for: nothing bound, nothing recorded
  saved_ = launch_tag();
  if (!capturing_step()) {
    launch_tag() = LaunchTag{nullptr, e_, 0, false};
    armed_ = true;
  }
}

void ForkAfter::restore() {
  if (!armed_) return;
  const int n = launch_tag().launches;
  launch_tag() = saved_;
  if (n && saved_.stop) launch_tag().missed = true;
  armed_ = false;
}

int ForkAfter::done() {
  if (finished_ || !out_) return DCUE_OK;
  finished_ = true;
  const bool bound = armed_ && launch_tag().launches > 0 && !launch_tag().missed;
  restore();
  if (!bound) DCUE_HIP_CHECK(hipEventRecord(e_, s_));
  *out_ = e_;
  return DCUE_OK;
}

ForkAfter::~ForkAfter() { restore(); }

// Plans leave the user table's Adam step (and its rolling flush slice) running on the user stream
// past the end of a step; entry points that touch the table from the caller's stream join it first.
int join_user_stream(hipStream_t s) {
  SidePool* sp = side_pool();
  if (!sp) return DCUE_ERR_HIP;
  return stream_wait(sp, s, sp->st[0]);
}

bool xq_edge_on(int group) {
  static const bool on[3] = {
      !env_is(getenv("DCUE_XQ_START"), '0'), !env_is(getenv("DCUE_XQ_FORK"), '0'), !env_is(getenv("DCUE_XQ_LATE"), '0')};
  return group >= 0 && group < 3 && on[group];
}

int wait_point(hipStream_t to, hipEvent_t ev) {
  DCUE_HIP_CHECK(hipStreamWaitEvent(to, ev, 0));
  return DCUE_OK;
}

// `to` waits for everything enqueued on `from` so far. An event is re-recorded only after the
// wait on its previous record has been enqueued, so a small ring of events suffices.
int stream_wait(SidePool* p, hipStream_t to, hipStream_t from) {
  hipEvent_t e = ring_event(p);
  DCUE_HIP_CHECK(hipEventRecord(e, from));
  DCUE_HIP_CHECK(hipStreamWaitEvent(to, e, 0));
  return DCUE_OK;
}

int wait_edges(hipStream_t to, const Edge* e, int n) {
  DevWait w[kWaitSignalsMax] = {};
  int k = 0;
  for (int i = 0; i < n; ++i)
    if (e[i].dev()) {
      if (k == kWaitSignalsMax) return DCUE_ERR_INVALID;
      w[k++] = e[i].sig;
    }
  TRY(launch_wait_signals(w, k, to));
  for (int i = 0; i < n; ++i)
    if (!e[i].dev() && e[i].ev) TRY(wait_point(to, e[i].ev));
  return DCUE_OK;
}
int wait_or_poll(hipStream_t to, const Edge& e, DevWait* poll) {
  *poll = e.sig;
  return e.dev() || !e.ev ? DCUE_OK : wait_point(to, e.ev);
}
DevWait next_signal(unsigned* sig, unsigned* issued, int slot, unsigned n) {
  return DevWait{sig + slot, issued[slot] += n, user_fwd_fail_flag()};
}

}  // namespace dcue
