// tail_wait.h — how the host waits for the row of a result tail, and which
// profile event pairs are out with statements whose times are not read yet.
//
// The last kernel of a one-row aggregate stores the row in the engine's mapped
// buffer (result_tail.h) and ends with one release store at system scope: the
// statement's ticket, at kTailTicketOffset.  TailWait spins on that word, so
// the host reads the row the moment it is complete and the stream drains
// behind its back; past a spin budget it blocks on the stream, as ToHost
// always did.  A ticket is a 64-bit count that is never reused and never 0
// (the buffer is zeroed when it is allocated), and only the wanted value is
// taken: an older or a younger one is not the statement's row.  The caller
// reads the error word and the cells only after TailWait said the ticket is in.
//
// Plain C++, no HIP: the executor instantiates the wait with the mapped
// buffer, steady_clock and hipStreamSynchronize, a host test with threads.
#pragma once
#include <cstddef>
#include <cstdint>
#include <vector>

#if defined(__x86_64__) || defined(__i386__)
#include <immintrin.h>
#endif

namespace mbx {

inline void TailSpinPause() {
#if defined(__x86_64__) || defined(__i386__)
  _mm_pause();
#elif defined(__aarch64__)
  __asm__ __volatile__("yield");
#endif
}

// duckdb_mbx_tail_wait_stats
struct TailWaitStats {
  int64_t polled = 0;   // statements whose ticket the spin saw
  int64_t blocked = 0;  // statements that went to the blocking wait
  int64_t wait_ns = 0;  // in TailWait, both kinds
};

enum class TailWaitOutcome {
  kPolled,   // the spin saw the wanted ticket
  kBlocked,  // the blocking wait returned and the ticket is the wanted one
  kLost      // the blocking wait returned and the ticket is another: no row may be handed out
};

// how many looks at the ticket lie between two looks at the clock
constexpr int kTailSpinsPerClock = 16;

// load():  the ticket word, with acquire
// now():   a monotonic clock in nanoseconds
// block(): waits until everything queued before it has run (it raises its own
//          errors); called at most once
// spin_ns <= 0: never spins, never looks at the ticket before block().
template <class Load, class Now, class Block>
TailWaitOutcome TailWait(uint64_t want, int64_t spin_ns, Load &&load, Now &&now, Block &&block, TailWaitStats &st) {
  const int64_t t0 = now();
  if (spin_ns > 0) {
    for (;;) {
      for (int i = 0; i < kTailSpinsPerClock; i++) {
        if (load() == want) {
          st.polled++;
          st.wait_ns += now() - t0;
          return TailWaitOutcome::kPolled;
        }
        TailSpinPause();
      }
      if (now() - t0 >= spin_ns) break;
    }
  }
  st.blocked++;
  block();
  const bool ok = load() == want;
  st.wait_ns += now() - t0;
  return ok ? TailWaitOutcome::kBlocked : TailWaitOutcome::kLost;
}

// The profile's event pairs by index.  A statement takes pairs as it launches
// (Take); when it ends they are either read at once or left out with it
// (Defer) until the engine settles (Settle, oldest statement first), and only
// then go back to be handed out again.  The pool therefore holds what one
// statement needs plus what the unsettled ones hold, and no more.
class EventPairLedger {
 public:
  // an index no statement holds; == Made() before the call when the caller has to create the pair
  size_t Take() {
    size_t i;
    if (!free_.empty()) {
      i = free_.back();
      free_.pop_back();
    } else {
      i = made_++;
    }
    current_.push_back(i);
    return i;
  }
  // the running statement ends unread (it raised, or a new one begins): its pairs are free again
  void DropCurrent() {
    free_.insert(free_.end(), current_.rbegin(), current_.rend());
    current_.clear();
  }
  // the running statement's pairs stay out until Settle; returns its place in the order
  uint64_t Defer() {
    pending_.push_back(std::move(current_));
    current_.clear();
    return first_serial_ + pending_.size() - 1;
  }
  // fn(serial, pair index) for every pair of every deferred statement, in
  // statement order and, within one, in the order taken; then they are free
  template <class Fn>
  void Settle(Fn &&fn) {
    for (size_t s = 0; s < pending_.size(); s++) {
      for (size_t i : pending_[s]) fn(first_serial_ + s, i);
      free_.insert(free_.end(), pending_[s].rbegin(), pending_[s].rend());
    }
    first_serial_ += pending_.size();
    pending_.clear();
  }
  size_t Made() const { return made_; }
  size_t PendingStatements() const { return pending_.size(); }
  size_t Held() const {
    size_t n = current_.size();
    for (auto &p : pending_) n += p.size();
    return n;
  }

 private:
  std::vector<size_t> free_, current_;
  std::vector<std::vector<size_t>> pending_;
  uint64_t first_serial_ = 0;
  size_t made_ = 0;
};

}  // namespace mbx
