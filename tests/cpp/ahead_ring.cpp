// The ahead ring's bookkeeping (pvw_rs_amd/csrc/pvw_ahead_ring.h) against a model of the two streams, on the CPU.
//
// The model: the caller's stream is a sequence of operations numbered as they are enqueued; an event record on it holds the
// number of the last operation in front of it; the side stream runs in order, so it has waited for the largest record it was
// told to wait for.  encrypt_enqueue's use of the ring is restated in Sim::ahead_call.  What must hold for every sequence of
// calls:
//   - a prologue that writes set j stands behind a wait that covers the last MAC that read set j;
//   - a MAC reads the set its own prologue wrote, and no later prologue has written that set in between;
//   - guards are recorded on the caller's stream at most once per R ahead calls that reach their MAC (the MAC launches of the
//     other calls stay adjacent in the queue), plus once for every call that failed on a bank's last set.
// Prints AHEAD_RING_OK; built with -fsanitize=address,undefined by tests/test_ahead_ring_host.py.
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "pvw_ahead_ring.h"

using pvw::AheadRing;

static int g_fail = 0;
#define CHECK(cond, ...)                                  \
  do {                                                    \
    if (!(cond)) {                                        \
      ++g_fail;                                           \
      printf("FAIL %s:%d %s: ", __FILE__, __LINE__, #cond); \
      printf(__VA_ARGS__);                                \
      printf("\n");                                       \
    }                                                     \
  } while (0)

struct Sim {
  AheadRing ring;
  uint64_t seq = 0;                    // operations enqueued on the caller's stream so far
  uint64_t guard[2] = {0, 0};          // what each bank's guard holds (the seq at its last record)
  bool guard_recorded[2] = {false, false};
  uint64_t side_waited = 0;            // the side stream has waited for every caller-stream operation up to here
  std::vector<uint64_t> last_read;     // per set: seq of the last MAC that read it (0: none)
  std::vector<uint64_t> content;       // per set: id of the call whose prologue wrote it last
  uint64_t calls = 0, taken = 0, macs_ahead = 0, records = 0, records_first = 0;   // taken: sets handed out

  explicit Sim(unsigned R) {
    ring.reset(R);
    last_read.assign(ring.slots(), 0);
    content.assign(ring.slots(), 0);
  }
  void record(unsigned bank) {
    guard[bank] = seq;
    guard_recorded[bank] = true;
    ++records;
  }
  // a call that stays in order: prologue and MAC on the caller's stream, into the workspace's own buffers
  void in_order_call() {
    ++calls;
    seq += 2;
  }
  // other work of the caller's on its stream
  void other_work(unsigned ops) { seq += ops; }
  // fail_before_mac: the call returns an error between the prologue and the MAC (nothing reads the set)
  // timed_out: the host gave up polling and put a wait in front of the MAC -- no difference to the ring
  void ahead_call(bool fail_before_mac = false, bool timed_out = false) {
    const uint64_t id = ++calls;
    const AheadRing::Step st = ring.begin();
    ++taken;
    CHECK(st.slot < ring.slots() && st.bank == st.slot / ring.R, "slot %u bank %u", st.slot, st.bank);
    if (st.record_first) {
      record(st.bank);
      ++records_first;
    }
    if (st.wait_guard) {
      CHECK(guard_recorded[st.bank], "call %llu waits for a guard that was never recorded", (unsigned long long)id);
      if (guard[st.bank] > side_waited) side_waited = guard[st.bank];
    }
    // the prologue writes the set now (as far as the side stream's order goes)
    CHECK(last_read[st.slot] <= side_waited, "call %llu writes set %u, last read by operation %llu, side stream waited for %llu",
          (unsigned long long)id, st.slot, (unsigned long long)last_read[st.slot], (unsigned long long)side_waited);
    content[st.slot] = id;
    if (fail_before_mac) return;
    if (timed_out) ++seq;              // the wait packet
    ++seq;                             // the MAC
    CHECK(content[st.slot] == id, "call %llu reads set %u written by call %llu", (unsigned long long)id, st.slot,
          (unsigned long long)content[st.slot]);
    last_read[st.slot] = seq;
    ++macs_ahead;
    if (ring.finish(st.slot)) record(st.bank);
  }
  // every set a queued MAC still has to read keeps its content: the host may be ahead of the GPU by every call whose MAC the
  // side stream has not been made to wait for
  void check_pending_intact() const {
    for (unsigned j = 0; j < last_read.size(); ++j)
      if (last_read[j] > side_waited) CHECK(content[j] != 0, "set %u", j);
  }
};

static uint32_t g_rng = 12345;
static uint32_t rnd() {
  g_rng = g_rng * 1664525u + 1013904223u;
  return g_rng >> 8;
}

int main() {
  for (unsigned R = 1; R <= AheadRing::MAX_R; ++R) {
    // ---- a straight run of ahead calls through several wraps: one record per R calls, no record_first ----
    {
      Sim s(R);
      const unsigned N = 7 * 2 * R + 3;
      for (unsigned i = 0; i < N; ++i) {
        const uint64_t before = s.records;
        s.ahead_call();
        CHECK(s.records - before == ((i + 1) % R == 0 ? 1u : 0u), "R=%u call %u: %llu records", R, i, (unsigned long long)(s.records - before));
      }
      CHECK(s.records == N / R && s.records_first == 0, "R=%u records %llu", R, (unsigned long long)s.records);
      // the sets come round in order
      Sim t(R);
      for (unsigned i = 0; i < 5 * 2 * R; ++i) {
        const unsigned want = i % (2 * R);
        CHECK(t.ring.pos == want, "R=%u call %u pos %u", R, i, t.ring.pos);
        t.ahead_call();
      }
    }
    // ---- the first lap waits for nothing (no MAC has read any set) ----
    {
      Sim s(R);
      for (unsigned i = 0; i < 2 * R; ++i) s.ahead_call();
      CHECK(s.side_waited == 0, "R=%u first lap waited for %llu", R, (unsigned long long)s.side_waited);
      const uint64_t g0 = s.guard[0], bank0_last = s.last_read[R - 1];
      s.ahead_call();                  // the wrap: bank 0 again, behind the guard of its first fill
      CHECK(s.side_waited == g0 && g0 >= bank0_last && bank0_last > 0, "R=%u wrap", R);
    }
    // ---- mixed: ahead, in-order and other work, timeouts in the middle, at every phase of the ring ----
    for (unsigned phase = 0; phase < 2 * R; ++phase) {
      Sim s(R);
      for (unsigned i = 0; i < phase; ++i) s.ahead_call();
      s.in_order_call();
      s.other_work(3);
      s.ahead_call(false, true);       // a timed-out call in the middle of a sequence
      s.in_order_call();
      for (unsigned i = 0; i < 4 * R + 1; ++i) s.ahead_call(false, i % 3 == 1);
      CHECK(s.records_first == 0, "R=%u phase %u", R, phase);
      CHECK(s.records == s.macs_ahead / R, "R=%u phase %u records %llu macs %llu", R, phase, (unsigned long long)s.records,
            (unsigned long long)s.macs_ahead);
    }
    // ---- a call that fails before its MAC, at every set: the guard is made up on the next entry where it was due ----
    for (unsigned at = 0; at < 2 * R; ++at) {
      Sim s(R);
      for (unsigned i = 0; i < 2 * R + at; ++i) s.ahead_call();
      s.ahead_call(true);
      const uint64_t before = s.records_first;
      for (unsigned i = 0; i < 6 * R; ++i) s.ahead_call();
      CHECK(s.records_first - before == (at % R == R - 1 ? 1u : 0u), "R=%u at %u: %llu", R, at, (unsigned long long)(s.records_first - before));
    }
    // ---- random sequences ----
    for (unsigned run = 0; run < 200; ++run) {
      Sim s(R);
      uint64_t failed_last = 0;
      for (unsigned i = 0; i < 300; ++i) {
        const uint32_t x = rnd() % 16;
        if (x < 9) s.ahead_call(false, x == 8);
        else if (x < 12) s.in_order_call();
        else if (x < 15) s.other_work(1 + rnd() % 4);
        else {
          if (s.ring.pos % R == R - 1) ++failed_last;
          s.ahead_call(true);
        }
        s.check_pending_intact();
      }
      CHECK(s.records_first <= failed_last, "R=%u run %u: %llu late records for %llu failures", R, run,
            (unsigned long long)s.records_first, (unsigned long long)failed_last);
      CHECK(s.records - s.records_first <= s.taken / R, "R=%u run %u", R, run);   // one per bank filled
    }
  }
  // ---- reset() clamps R and forgets the guards ----
  {
    AheadRing r;
    r.reset(0);
    CHECK(r.R == 1 && r.slots() == 2, "R=%u", r.R);
    r.reset(100);
    CHECK(r.R == AheadRing::MAX_R, "R=%u", r.R);
    for (unsigned i = 0; i < r.slots(); ++i) r.finish(r.begin().slot);
    r.reset(2);
    CHECK(r.pos == 0 && !r.recorded[0] && !r.recorded[1] && !r.open[0] && !r.open[1], "reset");
    CHECK(!r.begin().wait_guard, "fresh ring waits");
  }
  if (g_fail) {
    printf("AHEAD_RING_FAILED %d\n", g_fail);
    return 1;
  }
  printf("AHEAD_RING_OK\n");
  return 0;
}
