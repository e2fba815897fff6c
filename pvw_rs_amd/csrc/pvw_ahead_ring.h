// pvw_ahead_ring.h -- bookkeeping of the (r-hat, e_small) sets that a seed-mode encrypt's prologue fills AHEAD of its MAC, on a
// side stream (encrypt_enqueue, pvw_capi.hip).  No HIP types: the caller owns the buffers, the streams and the events; this
// says which set a call takes and which event operations protect it.  tests/cpp/ahead_ring.cpp walks it on the CPU.
//
// 2R sets in two banks of R.  A call takes the next set in order; calls that stay in order (idle stream, _rs, explicit
// randomness, capture) do not touch the ring.  One GUARD event per bank tells the side stream when the MACs that read the bank
// have finished: it is recorded on the CALLER's stream behind the MAC that reads the bank's LAST set, and the side stream waits
// for it in front of the prologue that writes the bank's FIRST set the next time round (the side stream runs in order, so the
// bank's other sets stand behind that wait too).  A bank is left only through its last set, so when it is entered again every
// MAC that read it is older than the guard.  The library ships R = 1: two sets, every call records its bank's guard.  R > 1
// (one record per R calls) measured the same step as R = 1; it stays, behind the tuning build's PVW_AHEAD_R, so that the runs
// recorded in profiles/r09_prologue_ahead_ab.txt can be repeated.
//
// A call that took a set and failed before its MAC was enqueued never reaches finish().  Where that was a bank's last set, the
// guard is missing: the next call that enters the bank records it first (record_first) -- on the caller's stream at that
// moment, behind everything that could still read the bank -- and waits for that.
#pragma once

namespace pvw {

struct AheadRing {
  static constexpr unsigned MAX_R = 8;
  unsigned R = 0;                       // sets per bank (0: the ring has not been set up)
  unsigned pos = 0;                     // the next call's set, in [0, 2R)
  bool recorded[2] = {false, false};    // bank's guard has been recorded at least once
  bool open[2] = {false, false};        // sets of the bank handed out since its guard was last recorded

  struct Step {
    unsigned slot = 0, bank = 0;
    bool record_first = false;          // record the bank's guard on the caller's stream before anything else
    bool wait_guard = false;            // the side stream waits for the bank's guard in front of the prologue
  };

  void reset(unsigned r) {
    R = r < 1 ? 1 : (r > MAX_R ? MAX_R : r);
    pos = 0;
    recorded[0] = recorded[1] = open[0] = open[1] = false;
  }
  unsigned slots() const { return 2 * R; }

  // the set of the call that is about to launch its prologue
  Step begin() {
    Step s;
    s.slot = pos;
    s.bank = pos / R;
    if (pos % R == 0) {                 // entering the bank
      s.record_first = open[s.bank];
      s.wait_guard = open[s.bank] || recorded[s.bank];
      if (s.record_first) {
        recorded[s.bank] = true;
        open[s.bank] = false;
      }
    }
    open[s.bank] = true;
    pos = (pos + 1) % slots();
    return s;
  }
  // the MAC that reads set `slot` has been enqueued on the caller's stream; true: record the bank's guard behind it now
  bool finish(unsigned slot) {
    if (slot % R != R - 1) return false;
    const unsigned bank = slot / R;
    recorded[bank] = true;
    open[bank] = false;
    return true;
  }
};

}  // namespace pvw
