// Stand-alone host check of csrc/tail_wait.h (tests/test_tail_wait_host.py
// builds it once under AddressSanitizer + UBSan and once under
// ThreadSanitizer): the ticket wait the executor instantiates, here against a
// writer thread that plays the emitting kernel, and the ledger of profile
// event pairs.
#include <atomic>
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <thread>
#include <vector>

#include "result_tail.h"
#include "tail_wait.h"

using namespace mbx;

#define CHECK(x)                                                   \
  do {                                                             \
    if (!(x)) {                                                    \
      fprintf(stderr, "%s:%d: CHECK(%s) failed\n", __FILE__, __LINE__, #x); \
      exit(1);                                                     \
    }                                                              \
  } while (0)

static int64_t SteadyNow() {
  return (int64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(
             std::chrono::steady_clock::now().time_since_epoch())
      .count();
}

// a clock the test moves: every look advances it by `step`
struct FakeClock {
  int64_t t = 0, step = 0, looks = 0;
  int64_t operator()() {
    looks++;
    t += step;
    return t;
  }
};

// The mapped buffer's first lines as the kernel and the host see them: plain
// cells and error word, the ticket an atomic at kTailTicketOffset.
struct alignas(64) Mapped {
  int32_t err;
  int32_t pad;
  std::atomic<uint64_t> ticket;
  char fill[48];
  uint64_t cell[3];
};
static_assert(offsetof(Mapped, ticket) == kTailTicketOffset, "the ticket's home");
static_assert(offsetof(Mapped, cell) == 64, "cells begin on the second line");

// Ordering: the writer stores the cells, then the error word, then the ticket
// with release; the reader takes the row after TailWait and must never see a
// cell of an older statement.  The reader hands the row back through `taken`,
// as the next statement is only launched after the host has read this one.
static void Ordering(int handovers) {
  static Mapped M;
  M.err = 0;
  M.ticket.store(0);
  std::atomic<uint64_t> taken{0};
  std::thread writer([&] {
    for (uint64_t k = 1; k <= (uint64_t)handovers; k++) {
      while (taken.load(std::memory_order_acquire) != k - 1) TailSpinPause();
      M.cell[0] = k * 3;
      M.cell[1] = ~k;
      M.cell[2] = k * k;
      M.err = (int32_t)(k & 0x7fff);
      M.ticket.store(k, std::memory_order_release);
    }
  });
  TailWaitStats st;
  int blocks = 0;
  for (uint64_t k = 1; k <= (uint64_t)handovers; k++) {
    const TailWaitOutcome w = TailWait(
        k, (int64_t)60 * 1000 * 1000 * 1000, [&] { return M.ticket.load(std::memory_order_acquire); }, SteadyNow,
        [&] { blocks++; }, st);
    CHECK(w == TailWaitOutcome::kPolled);
    CHECK(M.err == (int32_t)(k & 0x7fff));
    CHECK(M.cell[0] == k * 3 && M.cell[1] == ~k && M.cell[2] == k * k);
    taken.store(k, std::memory_order_release);
  }
  writer.join();
  CHECK(blocks == 0);
  CHECK(st.polled == handovers && st.blocked == 0 && st.wait_ns >= 0);
}

// A ticket of want - 1 or want + 1 is never accepted: the spin runs its budget
// out on it, and after the blocking wait it is an error.
static void StaleTickets() {
  for (uint64_t have : {(uint64_t)6, (uint64_t)8, (uint64_t)0, ~(uint64_t)0}) {
    FakeClock clk;
    clk.step = 10;
    TailWaitStats st;
    int blocks = 0;
    int64_t loads = 0;
    const TailWaitOutcome w = TailWait(
        7, 1000, [&] { loads++; return have; }, clk, [&] { blocks++; }, st);
    CHECK(w == TailWaitOutcome::kLost);
    CHECK(blocks == 1);
    CHECK(loads > 1);
    CHECK(st.polled == 0 && st.blocked == 1);
  }
}

// Budget expiry: block() is called exactly once, and a ticket that the
// blocking wait brought is taken; one it did not bring is kLost (no row).
static void BudgetExpiry() {
  {
    FakeClock clk;
    clk.step = 100;
    TailWaitStats st;
    int blocks = 0;
    uint64_t word = 41;
    const TailWaitOutcome w = TailWait(
        42, 5000, [&] { return word; }, clk, [&] { blocks++; word = 42; }, st);
    CHECK(w == TailWaitOutcome::kBlocked);
    CHECK(blocks == 1);
    CHECK(st.polled == 0 && st.blocked == 1);
    CHECK(st.wait_ns >= 5000);
  }
  {
    FakeClock clk;
    clk.step = 100;
    TailWaitStats st;
    int blocks = 0;
    const TailWaitOutcome w = TailWait(
        42, 5000, [&] { return (uint64_t)41; }, clk, [&] { blocks++; }, st);
    CHECK(w == TailWaitOutcome::kLost);
    CHECK(blocks == 1);
  }
  {  // the spin ends between two looks at the clock, not only on one
    FakeClock clk;
    clk.step = 1;
    TailWaitStats st;
    int blocks = 0;
    int64_t loads = 0;
    const TailWaitOutcome w = TailWait(
        9, 1000000, [&] { return ++loads == 40 ? (uint64_t)9 : (uint64_t)8; }, clk, [&] { blocks++; }, st);
    CHECK(w == TailWaitOutcome::kPolled && blocks == 0 && loads == 40);
  }
}

// Budget 0 never spins: the ticket is not looked at before block(), and once after.
static void BudgetZero() {
  for (int64_t budget : {(int64_t)0, (int64_t)-5}) {
    FakeClock clk;
    clk.step = 7;
    TailWaitStats st;
    int blocks = 0, loads_before = 0, loads_after = 0;
    const TailWaitOutcome w = TailWait(
        3, budget,
        [&] {
          (blocks ? loads_after : loads_before)++;
          return (uint64_t)3;  // (already there: a spin would have taken it)
        },
        clk, [&] { blocks++; }, st);
    CHECK(w == TailWaitOutcome::kBlocked);
    CHECK(blocks == 1 && loads_before == 0 && loads_after == 1);
    CHECK(clk.looks == 2);
    CHECK(st.polled == 0 && st.blocked == 1 && st.wait_ns == 7);
  }
}

// Counters: polled + blocked = statements, wait_ns the sum of every wait.
static void Counters() {
  FakeClock clk;
  clk.step = 5;
  TailWaitStats st;
  int blocks = 0;
  int64_t expect_ns = 0;
  uint64_t word = 0;
  for (uint64_t k = 1; k <= 100; k++) {
    const bool late = k % 4 == 0;  // every fourth arrives only with the blocking wait
    if (!late) word = k;
    const int64_t t0 = clk.t;
    const TailWaitOutcome w = TailWait(
        k, 200, [&] { return word; }, clk, [&] { blocks++; word = k; }, st);
    expect_ns += clk.t - (t0 + clk.step);
    CHECK(w == (late ? TailWaitOutcome::kBlocked : TailWaitOutcome::kPolled));
  }
  CHECK(st.polled == 75 && st.blocked == 25 && blocks == 25);
  CHECK(st.polled + st.blocked == 100);
  CHECK(st.wait_ns == expect_ns);
}

// The ledger: a pair a pending statement holds is not handed out again, the
// settle order is the statement order, and the pool stops growing.
static void Ledger() {
  EventPairLedger L;
  // statement 0 takes 2 pairs and is deferred
  const size_t a0 = L.Take(), a1 = L.Take();
  CHECK(a0 == 0 && a1 == 1 && L.Made() == 2);
  CHECK(L.Defer() == 0);
  // statement 1 must not get 0 or 1
  const size_t b0 = L.Take(), b1 = L.Take(), b2 = L.Take();
  CHECK(b0 == 2 && b1 == 3 && b2 == 4);
  CHECK(L.Defer() == 1);
  // statement 2 raised: its pairs are free at once, statement 3 gets them, not a pending one
  const size_t c0 = L.Take();
  CHECK(c0 == 5);
  L.DropCurrent();
  const size_t d0 = L.Take();
  CHECK(d0 == 5 && L.Made() == 6);
  CHECK(L.Defer() == 2);
  CHECK(L.PendingStatements() == 3 && L.Held() == 6);
  std::vector<std::pair<uint64_t, size_t>> seen;
  L.Settle([&](uint64_t s, size_t i) { seen.push_back({s, i}); });
  const std::vector<std::pair<uint64_t, size_t>> want = {{0, 0}, {0, 1}, {1, 2}, {1, 3}, {1, 4}, {2, 5}};
  CHECK(seen == want);
  CHECK(L.PendingStatements() == 0 && L.Held() == 0);
  // serials go on, and settled pairs are handed out again: the pool does not grow
  for (int s = 0; s < 10000; s++) {
    const size_t i = L.Take();
    CHECK(i < 6);
    CHECK(L.Defer() == (uint64_t)(3 + s));
    int n = 0;
    L.Settle([&](uint64_t serial, size_t j) { n++; CHECK(serial == (uint64_t)(3 + s) && j == i); });
    CHECK(n == 1);
  }
  CHECK(L.Made() == 6);
  // k statements pending need k pairs and no more
  for (int s = 0; s < 4; s++) {
    L.Take();
    L.Defer();
  }
  CHECK(L.Made() == 6 && L.Held() == 4);
  L.Settle([](uint64_t, size_t) {});
  // an empty statement keeps its place in the order
  L.Defer();
  L.Take();
  L.Defer();
  std::vector<uint64_t> serials;
  L.Settle([&](uint64_t s, size_t) { serials.push_back(s); });
  CHECK(serials.size() == 1 && serials[0] == 10008);
}

int main(int argc, char **argv) {
  const int handovers = argc > 1 ? atoi(argv[1]) : 100000;
  Ordering(handovers);
  StaleTickets();
  BudgetExpiry();
  BudgetZero();
  Counters();
  Ledger();
  printf("tail wait: ok (%d handovers)\n", handovers);
  return 0;
}
