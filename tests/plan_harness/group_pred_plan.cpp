// Stand-alone host check of csrc/group_pred_plan.h (tests/test_group_pred_plan.py
// builds and runs it): the predicate plan of the partitioned GROUP BY -- its
// verdicts, the clamp to the zone map, lo / span at the ends of INT64, the
// operands that coincide with a key or value column, and a brute-force check
// of every produced entry.  Prints "group pred plan: ok" or the first failed
// check.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "group_pred_plan.h"

using namespace mbx;
typedef __int128 i128;

static int g_dummy[8];  // (the plan only carries the data pointers)

#define CHECK(c)                                                \
  do {                                                          \
    if (!(c)) {                                                 \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);   \
      exit(1);                                                  \
    }                                                           \
  } while (0)

static const i128 kMin = (i128)INT64_MIN, kMax = (i128)INT64_MAX;

// column `col` with zone map [zmin, zmax] and the range [lo, hi]
static GroupPredIn In(int col, int phys, i128 zmin, i128 zmax, i128 lo, i128 hi) {
  GroupPredIn p = {};
  p.col = col;
  p.data = &g_dummy[col & 7];
  p.phys = phys;
  p.has_validity = false;
  p.stats_valid = true;
  p.imin = zmin;
  p.imax = zmax;
  p.null_count = 0;
  p.lo = lo;
  p.hi = hi;
  return p;
}

// one BIGINT key (column 0), one value (column 1)
static GroupPredShape OneKey() {
  GroupPredShape s = {};
  s.nkeys = 1;
  s.code = false;
  s.key_cols[0] = 0;
  s.nv = 1;
  s.val_cols[0] = 1;
  return s;
}

// the device test of an entry
static bool Pass(const GroupPredEntry &e, int64_t x) { return (uint64_t)x - (uint64_t)e.lo <= e.span; }

// Every entry of the plan against its original range: for a few hundred values
// of the zone map around both bounds, both zone-map edges and zero, the device
// test equals lo0 <= x <= hi0.  (Outside its zone map a column holds no value.)
static void BruteForce(const std::vector<GroupPredIn> &in, const GroupPredPlan &p) {
  for (int j = 0; j < p.set.n; j++) {
    const GroupPredEntry &e = p.set.p[j];
    const GroupPredIn *c = nullptr;
    for (auto &x : in)
      if (x.data == e.data) c = &x;
    CHECK(c);
    CHECK((i128)e.lo >= c->imin && (i128)e.lo + (i128)e.span <= c->imax);  // clamped
    const i128 around[5] = {c->lo, c->hi, c->imin, c->imax, 0};
    int tested = 0;
    for (i128 mid : around)
      for (int d = -40; d <= 40; d++) {
        const i128 x = mid + d;
        if (x < c->imin || x > c->imax) continue;
        CHECK(Pass(e, (int64_t)x) == (c->lo <= x && x <= c->hi));
        tested++;
      }
    CHECK(tested > 0);
  }
}

static GroupPredPlan Plan(const std::vector<GroupPredIn> &in, const GroupPredShape &s) {
  const GroupPredPlan p = PlanGroupPreds(in.data(), (int)in.size(), s);
  CHECK(p.set.n >= 0 && p.set.n <= GROUP_MAX_PRED);
  CHECK((p.verdict == GroupPredVerdict::Filter) == (p.set.n > 0));
  CHECK((p.verdict == GroupPredVerdict::Empty) == (p.set.empty == 1));
  if (p.verdict == GroupPredVerdict::Filter) BruteForce(in, p);
  else CHECK(p.own_bytes == 0);
  return p;
}

int main() {
  const GroupPredShape one = OneKey();
  // ---- Filter: x > 24 over x in 1..50, clamped to the zone map
  {
    GroupPredPlan p = Plan({In(2, P_I64, 1, 50, 25, kMax)}, one);
    CHECK(p.verdict == GroupPredVerdict::Filter && p.set.n == 1);
    CHECK(p.set.p[0].lo == 25 && p.set.p[0].span == 25 && p.set.p[0].src == kPredOwn && p.set.p[0].phys == P_I64);
    CHECK(p.set.p[0].data == &g_dummy[2] && p.own_bytes == 8);
    p = Plan({In(2, P_I32, 1, 50, kMin, 24)}, one);  // x <= 24, INT32
    CHECK(p.verdict == GroupPredVerdict::Filter && p.set.p[0].lo == 1 && p.set.p[0].span == 23 && p.own_bytes == 4);
  }
  // ---- an = predicate: span 0; BETWEEN; two ranges on one column (RangeConj
  // intersects them before the plan sees them: x > 10 AND x <= 30)
  {
    GroupPredPlan p = Plan({In(2, P_I64, 1, 50, 25, 25)}, one);
    CHECK(p.verdict == GroupPredVerdict::Filter && p.set.p[0].lo == 25 && p.set.p[0].span == 0);
    p = Plan({In(2, P_I64, 1, 50, 10, 20)}, one);
    CHECK(p.verdict == GroupPredVerdict::Filter && p.set.p[0].lo == 10 && p.set.p[0].span == 10);
    p = Plan({In(2, P_I64, 1, 50, 11, 30)}, one);
    CHECK(p.verdict == GroupPredVerdict::Filter && p.set.p[0].lo == 11 && p.set.p[0].span == 19);
  }
  // ---- Empty: lo > hi (x > 30 AND x < 20 intersected; a comparison with NULL
  // gives [1, 0]), and a range wholly outside the zone map on either side
  {
    CHECK(Plan({In(2, P_I64, 1, 50, 31, 19)}, one).verdict == GroupPredVerdict::Empty);
    CHECK(Plan({In(2, P_I64, 1, 50, 1, 0)}, one).verdict == GroupPredVerdict::Empty);
    CHECK(Plan({In(2, P_I64, 1, 50, 51, kMax)}, one).verdict == GroupPredVerdict::Empty);
    CHECK(Plan({In(2, P_I64, 1, 50, kMin, 0)}, one).verdict == GroupPredVerdict::Empty);
    // an empty range empties the result whatever its column is (a NULL fails it too)
    GroupPredIn nn = In(2, P_I64, 1, 50, 1, 0);
    nn.has_validity = true, nn.null_count = 3;
    CHECK(Plan({nn}, one).verdict == GroupPredVerdict::Empty);
    // one fitting predicate and one outside its zone map
    CHECK(Plan({In(2, P_I64, 1, 50, 25, kMax), In(3, P_I64, 0, 9, 10, 12)}, one).verdict == GroupPredVerdict::Empty);
  }
  // ---- a range just inside and just outside a zone-map edge, on both sides
  {
    GroupPredPlan p = Plan({In(2, P_I64, 1, 50, 50, kMax)}, one);  // x >= 50: the top value alone
    CHECK(p.verdict == GroupPredVerdict::Filter && p.set.p[0].lo == 50 && p.set.p[0].span == 0);
    CHECK(Plan({In(2, P_I64, 1, 50, 51, kMax)}, one).verdict == GroupPredVerdict::Empty);  // x >= 51
    p = Plan({In(2, P_I64, 1, 50, kMin, 1)}, one);  // x <= 1: the bottom value alone
    CHECK(p.verdict == GroupPredVerdict::Filter && p.set.p[0].lo == 1 && p.set.p[0].span == 0);
    CHECK(Plan({In(2, P_I64, 1, 50, kMin, 0)}, one).verdict == GroupPredVerdict::Empty);  // x <= 0
    CHECK(Plan({In(2, P_I64, 1, 50, 1, kMax)}, one).verdict == GroupPredVerdict::All);    // x >= 1 covers
    p = Plan({In(2, P_I64, 1, 50, 2, kMax)}, one);                                        // x >= 2 does not
    CHECK(p.verdict == GroupPredVerdict::Filter && p.set.p[0].lo == 2 && p.set.p[0].span == 48);
    CHECK(Plan({In(2, P_I64, 1, 50, kMin, 50)}, one).verdict == GroupPredVerdict::All);  // x <= 50 covers
    p = Plan({In(2, P_I64, 1, 50, kMin, 49)}, one);
    CHECK(p.verdict == GroupPredVerdict::Filter && p.set.p[0].lo == 1 && p.set.p[0].span == 48);
  }
  // ---- All: every range covers its zone map; the whole INT64 range does not overflow
  {
    GroupPredPlan p = Plan({In(2, P_I64, 1, 50, 0, kMax), In(3, P_I32, -5, 5, -5, 5)}, one);
    CHECK(p.verdict == GroupPredVerdict::All && p.set.n == 0 && p.own_bytes == 0);
    CHECK(Plan({In(2, P_I64, kMin, kMax, kMin, kMax)}, one).verdict == GroupPredVerdict::All);
    CHECK(Plan({}, one).verdict == GroupPredVerdict::All);
  }
  // ---- lo / span at INT64_MIN and INT64_MAX, and __int128 bounds outside int64
  {
    GroupPredPlan p = Plan({In(2, P_I64, kMin, kMax, kMin, kMax - 1)}, one);
    CHECK(p.verdict == GroupPredVerdict::Filter && p.set.p[0].lo == INT64_MIN && p.set.p[0].span == UINT64_MAX - 1);
    CHECK(Pass(p.set.p[0], INT64_MIN) && Pass(p.set.p[0], INT64_MAX - 1) && !Pass(p.set.p[0], INT64_MAX));
    p = Plan({In(2, P_I64, kMin, kMax, kMin + 1, kMax)}, one);
    CHECK(p.verdict == GroupPredVerdict::Filter && p.set.p[0].lo == INT64_MIN + 1 && p.set.p[0].span == UINT64_MAX - 1);
    CHECK(!Pass(p.set.p[0], INT64_MIN) && Pass(p.set.p[0], INT64_MIN + 1) && Pass(p.set.p[0], INT64_MAX));
    p = Plan({In(2, P_I64, kMin, kMax, kMax, kMax)}, one);  // x = INT64_MAX
    CHECK(p.verdict == GroupPredVerdict::Filter && p.set.p[0].lo == INT64_MAX && p.set.p[0].span == 0);
    p = Plan({In(2, P_I64, kMin, kMax, kMin, kMin)}, one);  // x = INT64_MIN
    CHECK(p.verdict == GroupPredVerdict::Filter && p.set.p[0].lo == INT64_MIN && p.set.p[0].span == 0);
    // bounds beyond int64 (a HUGEINT constant): clamped to the zone map first
    p = Plan({In(2, P_I64, kMin, kMax, kMin - 1000, 7)}, one);
    CHECK(p.verdict == GroupPredVerdict::Filter && p.set.p[0].lo == INT64_MIN &&
          p.set.p[0].span == (uint64_t)7 - (uint64_t)INT64_MIN);
    p = Plan({In(2, P_I64, kMin, kMax, -7, kMax + ((i128)1 << 70))}, one);
    CHECK(p.verdict == GroupPredVerdict::Filter && p.set.p[0].lo == -7 && p.set.p[0].span == (uint64_t)INT64_MAX + 7);
    CHECK(Plan({In(2, P_I64, -100, 100, kMax + 1, kMax + 5)}, one).verdict == GroupPredVerdict::Empty);
    CHECK(Plan({In(2, P_I64, -100, 100, kMin - 5, kMin - 1)}, one).verdict == GroupPredVerdict::Empty);
    CHECK(Plan({In(2, P_I64, -100, 100, kMin - 5, kMax + 5)}, one).verdict == GroupPredVerdict::All);
    p = Plan({In(2, P_I32, INT32_MIN, INT32_MAX, kMin - 5, -1)}, one);
    CHECK(p.verdict == GroupPredVerdict::Filter && p.set.p[0].lo == INT32_MIN && p.set.p[0].span == (uint64_t)INT32_MAX);
  }
  // ---- Unfit: a fourth predicate column; three ranges of which one covers
  // its zone map leave two entries; four of which one covers leave three
  {
    std::vector<GroupPredIn> four = {In(2, P_I64, 1, 50, 25, kMax), In(3, P_I32, 0, 999, kMin, 499),
                                     In(4, P_I64, -9, 9, 0, 0), In(5, P_I32, 0, 99, 10, 20)};
    CHECK(Plan(four, one).verdict == GroupPredVerdict::Unfit);
    std::vector<GroupPredIn> three(four.begin(), four.begin() + 3);
    GroupPredPlan p = Plan(three, one);
    CHECK(p.verdict == GroupPredVerdict::Filter && p.set.n == 3 && p.own_bytes == 8 + 4 + 8);
    three[1] = In(3, P_I32, 0, 999, kMin, 999);  // covers
    p = Plan(three, one);
    CHECK(p.verdict == GroupPredVerdict::Filter && p.set.n == 2 && p.own_bytes == 16);
    CHECK(p.set.p[0].data == &g_dummy[2] && p.set.p[1].data == &g_dummy[4]);
    four[1] = three[1];
    p = Plan(four, one);
    CHECK(p.verdict == GroupPredVerdict::Filter && p.set.n == 3 && p.own_bytes == 8 + 8 + 4);
  }
  // ---- Unfit: not INT32 / INT64, a bitmap, NULLs, no zone map, no data
  {
    CHECK(Plan({In(2, P_I16, 1, 50, 25, kMax)}, one).verdict == GroupPredVerdict::Unfit);
    CHECK(Plan({In(2, P_I128, 1, 50, 25, kMax)}, one).verdict == GroupPredVerdict::Unfit);
    CHECK(Plan({In(2, P_F64, 1, 50, 25, kMax)}, one).verdict == GroupPredVerdict::Unfit);
    CHECK(Plan({In(2, P_U64, 1, 50, 25, kMax)}, one).verdict == GroupPredVerdict::Unfit);
    GroupPredIn a = In(2, P_I64, 1, 50, 25, kMax);
    a.has_validity = true;
    CHECK(Plan({a}, one).verdict == GroupPredVerdict::Unfit);
    a = In(2, P_I64, 1, 50, 25, kMax);
    a.null_count = 1;
    CHECK(Plan({a}, one).verdict == GroupPredVerdict::Unfit);
    a = In(2, P_I64, 1, 50, 25, kMax);
    a.stats_valid = false;
    CHECK(Plan({a}, one).verdict == GroupPredVerdict::Unfit);
    a = In(2, P_I64, 1, 50, 25, kMax);
    a.data = nullptr;
    CHECK(Plan({a}, one).verdict == GroupPredVerdict::Unfit);
    // ... even beside a predicate that covers its zone map
    a = In(3, P_I64, 1, 50, 25, kMax);
    a.has_validity = true;
    CHECK(Plan({In(2, P_I64, 1, 50, 0, 99), a}, one).verdict == GroupPredVerdict::Unfit);
  }
  // ---- operands that coincide, and the bytes counted once
  {
    // on the key and on the value of the single-key shape
    GroupPredPlan p = Plan({In(0, P_I64, 0, 2999, 1500, kMax), In(1, P_I64, -1000000, 999999, kMin, -1)}, one);
    CHECK(p.verdict == GroupPredVerdict::Filter && p.set.n == 2 && p.own_bytes == 0);
    CHECK(p.set.p[0].src == kPredKey && p.set.p[1].src == kPredV0);
    CHECK(p.set.p[0].lo == 1500 && p.set.p[0].span == 1499 && p.set.p[1].lo == -1000000 && p.set.p[1].span == 999999);
    // key, own INT32 and own INT64 column: only the own ones count
    p = Plan({In(0, P_I64, 0, 2999, 1500, kMax), In(2, P_I32, 1, 50, 25, kMax), In(3, P_I64, 1, 50, 25, kMax)}, one);
    CHECK(p.set.n == 3 && p.own_bytes == 12 && p.set.p[1].src == kPredOwn && p.set.p[2].src == kPredOwn);
    // composite keys (a, b) = columns 4, 5, two value columns 1 and 6
    GroupPredShape ab = {};
    ab.nkeys = 2, ab.code = true, ab.key_cols[0] = 4, ab.key_cols[1] = 5, ab.nv = 2, ab.val_cols[0] = 1,
    ab.val_cols[1] = 6;
    p = Plan({In(5, P_I32, -50, 49, kMin, -11), In(6, P_I64, 0, 999, kMin, 499), In(2, P_I64, 1, 50, 25, kMax)}, ab);
    CHECK(p.verdict == GroupPredVerdict::Filter && p.set.n == 3 && p.own_bytes == 8);
    CHECK(p.set.p[0].src == kPredCodeKey + 1 && p.set.p[1].src == kPredV1 && p.set.p[2].src == kPredOwn);
    p = Plan({In(4, P_I32, 0, 299, 100, 100)}, ab);
    CHECK(p.set.p[0].src == kPredCodeKey + 0 && p.own_bytes == 0);
    // a one-key group code (a NULL-able key is another column than its predicate's)
    GroupPredShape nk = {};
    nk.nkeys = 1, nk.code = true, nk.key_cols[0] = 7, nk.nv = 0;
    p = Plan({In(1, P_I64, -1000000, 999999, kMin, -1)}, nk);  // no value column: v is its own column here
    CHECK(p.set.p[0].src == kPredOwn && p.own_bytes == 8);
    // a covered predicate on an own column costs nothing (All)
    p = Plan({In(2, P_I64, 1, 50, 1, kMax)}, ab);
    CHECK(p.verdict == GroupPredVerdict::All && p.own_bytes == 0);
  }
  printf("group pred plan: ok\n");
  return 0;
}
