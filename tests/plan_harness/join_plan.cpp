// Stand-alone host check of csrc/join_plan.h (tests/test_join_plan_host.py
// builds and runs it): the join table's hash, sizing and probe sequence through
// the header's own insert and lookup -- key sets whose first slots collide
// (found here by brute force against the header's hash), the keys at the ends
// of int64 and the multiples of 2^32, capacities 1, 2 and the power of two
// just above 2n, a lookup of an absent key that walks a full cluster and
// stops, and the bounded-walk verdict on a table without an empty slot.
// Prints "join plan: ok" or the first failed check.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "join_plan.h"

using namespace mbx;

#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
      exit(1);                                                \
    }                                                         \
  } while (0)

// what the device does with atomicCAS, single-threaded
static bool Claim(uint32_t *w, uint32_t v) {
  if (*w != 0) return false;
  *w = v;
  return true;
}

struct Table {
  std::vector<JoinEntry> e;
  int64_t cap;
  explicit Table(int64_t c) : e((size_t)c), cap(c) {
    for (auto &x : e) x = JoinEntry{0, 0, 0};
  }
  int64_t Insert(int64_t key, int32_t start, uint32_t len) { return JoinInsert(e.data(), cap, key, start, len, Claim); }
  int64_t Find(int64_t key, JoinEntry *out) const { return JoinLookup(e.data(), cap, key, out); }
};

// inserts keys[i] with start = i and len = i + 1 and finds every one again
static void RoundTrip(const std::vector<int64_t> &keys, int64_t cap) {
  Table t(cap);
  std::set<int64_t> slots;
  for (size_t i = 0; i < keys.size(); i++) {
    const int64_t s = t.Insert(keys[i], (int32_t)i, (uint32_t)i + 1);
    CHECK(s >= 0 && s < cap);
    CHECK(slots.insert(s).second);  // every key owns a slot of its own
  }
  for (size_t i = 0; i < keys.size(); i++) {
    JoinEntry got = {0, 0, 0};
    const int64_t s = t.Find(keys[i], &got);
    CHECK(s >= 0 && s < cap);
    CHECK(got.key == keys[i] && got.start == (int32_t)i && got.len == (uint32_t)i + 1);
  }
}

static void Capacity() {
  CHECK(JoinCapacity(0) == 1);
  CHECK(JoinCapacity(1) == 2);
  CHECK(JoinCapacity(2) == 4);
  CHECK(JoinCapacity(3) == 8);
  CHECK(JoinCapacity(4) == 8);
  CHECK(JoinCapacity(5) == 16);
  CHECK(JoinCapacity(70001) == 262144);
  CHECK(JoinCapacity(kJoinMaxBuildRows) == (int64_t)1 << 32);
  for (int64_t n = 1; n < 5000; n++) {
    const int64_t c = JoinCapacity(n);
    CHECK((c & (c - 1)) == 0 && c >= 2 * n && c / 2 < 2 * n);
  }
  static_assert(sizeof(JoinEntry) == 16 && alignof(JoinEntry) == 16, "one 16-byte load per probe step");
}

static void ProbeSequence() {
  // every slot of the table exactly once, whatever the hash
  for (int64_t cap : {1, 2, 8, 64}) {
    for (uint64_t h : {0ull, 1ull, 63ull, ~0ull, 0x8000000000000000ull}) {
      std::set<int64_t> seen;
      for (int64_t i = 0; i < cap; i++) {
        const int64_t s = JoinSlot(h, i, cap);
        CHECK(s >= 0 && s < cap);
        seen.insert(s);
      }
      CHECK((int64_t)seen.size() == cap);
    }
  }
}

static void EdgeKeys() {
  std::vector<int64_t> keys = {0, -1, INT64_MIN, INT64_MAX, 1, -2, INT64_MIN + 1, INT64_MAX - 1};
  for (int64_t m = 1; m <= 64; m++) keys.push_back(m << 32);        // multiples of 2^32: equal low words
  for (int64_t m = 1; m <= 64; m++) keys.push_back(-(m << 32));
  for (int64_t m = 1; m <= 16; m++) keys.push_back((m << 32) | 7);
  RoundTrip(keys, JoinCapacity((int64_t)keys.size()));
  // the multiples of 2^32 do not all land in one slot: the hash reads the high word
  std::set<int64_t> first;
  for (int64_t m = 0; m < 256; m++) first.insert(JoinSlot(JoinHash(m << 32), 0, 1024));
  CHECK(first.size() > 128);
  // a key and its negation, 0 and -1, the two ends: different hashes
  CHECK(JoinHash(0) != JoinHash(-1) && JoinHash(INT64_MIN) != JoinHash(INT64_MAX) && JoinHash(5) != JoinHash(-5));
}

// n keys whose first probe slot in a table of `cap` is `slot`
static std::vector<int64_t> Colliding(int64_t cap, int64_t slot, size_t n, int64_t from) {
  std::vector<int64_t> out;
  for (int64_t k = from; out.size() < n; k++)
    if (JoinSlot(JoinHash(k), 0, cap) == slot) out.push_back(k);
  return out;
}

static void Collisions() {
  const int64_t cap = 64;
  // 20 keys that all start at slot 60: the cluster wraps past the end of the table
  std::vector<int64_t> keys = Colliding(cap, 60, 20, -1000);
  RoundTrip(keys, cap);
  Table t(cap);
  for (size_t i = 0; i < keys.size(); i++) CHECK(t.Insert(keys[i], (int32_t)i, 1) == JoinSlot(60, (int64_t)i, cap));
  // an absent key that starts at the head of the cluster walks all of it and stops at the empty slot behind
  const int64_t absent = Colliding(cap, 60, 21, -1000).back();
  JoinEntry got = {0, 0, 0};
  CHECK(t.Find(absent, &got) == kJoinAbsent);
  // one that starts at an empty slot stops at once
  const int64_t lone = Colliding(cap, 30, 1, 0)[0];
  CHECK(t.Find(lone, &got) == kJoinAbsent);
  // a mixed set at the capacity the executor would choose
  std::vector<int64_t> mixed = Colliding(128, 5, 10, 0);
  for (int64_t k : Colliding(128, 6, 10, 0)) mixed.push_back(k);
  for (int64_t k : Colliding(128, 127, 10, 0)) mixed.push_back(k);
  for (int64_t k = 1000000; (int64_t)mixed.size() < 64; k++) mixed.push_back(k * 7919);
  RoundTrip(mixed, JoinCapacity((int64_t)mixed.size()));
}

static void SmallTables() {
  JoinEntry got = {0, 0, 0};
  {  // capacity 1: the table of an empty build side, and one that is full with a single key
    Table t(1);
    CHECK(t.Find(42, &got) == kJoinAbsent);
    CHECK(t.Insert(42, 3, 9) == 0);
    CHECK(t.Find(42, &got) == 0 && got.start == 3 && got.len == 9);
    CHECK(t.Find(43, &got) == kJoinTableFull);
    CHECK(t.Insert(43, 0, 1) == kJoinTableFull);
  }
  {  // capacity 2 = JoinCapacity(1)
    Table t(2);
    CHECK(t.Insert(INT64_MIN, 0, 1) >= 0);
    CHECK(t.Find(INT64_MIN, &got) >= 0 && got.key == INT64_MIN);
    CHECK(t.Find(INT64_MAX, &got) == kJoinAbsent);
    CHECK(t.Find(0, &got) == kJoinAbsent);
  }
  // the power of two just above 2n, n keys
  for (int64_t n : {1, 2, 3, 5, 31, 32, 33, 1000}) {
    std::vector<int64_t> keys;
    for (int64_t i = 0; i < n; i++) keys.push_back(i * 0x100000001ll - n / 2);
    RoundTrip(keys, JoinCapacity(n));
  }
}

// a table without an empty slot (a sizing bug or a corrupted table on the
// device): every walk ends after cap steps with the verdict, none spins
static void FullTable() {
  const int64_t cap = 16;
  Table t(cap);
  for (int64_t k = 0; k < cap; k++) CHECK(t.Insert(k * 3 + 1, (int32_t)k, 1) >= 0);
  JoinEntry got = {0, 0, 0};
  for (int64_t k = 0; k < cap; k++) CHECK(t.Find(k * 3 + 1, &got) >= 0 && got.start == (int32_t)k);
  CHECK(t.Find(2, &got) == kJoinTableFull);
  CHECK(t.Find(-1, &got) == kJoinTableFull);
  CHECK(t.Insert(1000, 0, 1) == kJoinTableFull);
  for (int64_t k = 0; k < cap; k++) CHECK(t.e[(size_t)k].len == 1);  // the refused insert wrote nothing
}

int main() {
  Capacity();
  ProbeSequence();
  EdgeKeys();
  Collisions();
  SmallTables();
  FullTable();
  printf("join plan: ok\n");
  return 0;
}
