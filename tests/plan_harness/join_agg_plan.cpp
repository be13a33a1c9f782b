// Stand-alone host check of csrc/join_agg_plan.h (tests/test_join_agg_plan.py
// builds and runs it): the decision of the fused probe-and-aggregate on every
// reason to decline and on the boundary of the run limit, and the merge of two
// partial records against constants worked out in Python (they stand beside
// each check): low words that carry, sums of values at +-(2^63 - 1), an empty
// side in both orders, min / max of negatives.  With a file of records as its
// argument (first line: the expected merge of all that follow, written by the
// test from Python integers) it merges them left to right, right to left, as a
// pairwise tree and in the strided-then-tree shape of the fold kernel; all four
// must give the expected record.  Prints "join agg plan: ok" or the first
// failed check.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "join_agg_plan.h"

using namespace mbx;

#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
      exit(1);                                                \
    }                                                         \
  } while (0)

static JoinAggFacts Takes() {
  JoinAggFacts f;
  f.n_aggs = 2;
  f.max_aggs = 12;
  f.max_run = 1;
  f.max_run_limit = 8;
  return f;
}

static void Declines(const JoinAggFacts &f, const char *word) {
  const JoinAggChoice c = JoinAggDecide(f);
  CHECK(!c.take);
  CHECK(strstr(c.reason, word) != nullptr);
}

static void Decisions() {
  JoinAggFacts f = Takes();
  CHECK(JoinAggDecide(f).take);
  CHECK(std::string(JoinAggDecide(f).reason).empty());
  f = Takes(), f.enabled = false, Declines(f, "mbx_join_agg=false");
  f = Takes(), f.distinct = true, Declines(f, "DISTINCT");
  f = Takes(), f.varchar = true, Declines(f, "VARCHAR");
  f = Takes(), f.minmax_128 = true, Declines(f, "128-bit");
  f = Takes(), f.n_aggs = 13, Declines(f, "more aggregates");
  f = Takes(), f.n_aggs = 12;
  CHECK(JoinAggDecide(f).take);
  f = Takes(), f.n_aggs = 0;
  CHECK(JoinAggDecide(f).take);
  f = Takes(), f.compile_failed = true, Declines(f, "compiler");
  // the run limit: at it the statement is taken, one above it is not
  for (int64_t limit : {(int64_t)1, (int64_t)8, (int64_t)1024, (int64_t)2147483647}) {
    f = Takes(), f.max_run_limit = limit, f.max_run = limit;
    CHECK(JoinAggDecide(f).take);
    f.max_run = limit + 1;
    Declines(f, "mbx_join_agg_max_run");
    f.max_run = 0;  // an empty build side has no run
    CHECK(JoinAggDecide(f).take);
  }
  // the first reason that applies is the one given
  f = Takes(), f.enabled = false, f.distinct = true, f.max_run = 100, Declines(f, "mbx_join_agg=false");
}

// the record of one 64-bit integer value
static JoinAggRec One(int64_t v) {
  JoinAggRec r = JoinAggEmpty();
  r.count = 1;
  r.sum_lo = (uint64_t)v;
  r.sum_hi = v >> 63;
  r.min_i = r.max_i = v;
  return r;
}

static bool Same(const JoinAggRec &a, const JoinAggRec &b) {
  return a.count == b.count && a.sum_lo == b.sum_lo && a.sum_hi == b.sum_hi && a.min_i == b.min_i && a.max_i == b.max_i &&
         memcmp(&a.sum_f, &b.sum_f, 8) == 0 && a.min_f == b.min_f && a.max_f == b.max_f;
}

static void Merges() {
  const int64_t big = INT64_MAX;  // 2^63 - 1
  // (2^64 - 1) + 1 = 2^64: the low word wraps to 0 and carries
  JoinAggRec a = JoinAggEmpty(), b = One(1);
  a.count = 1, a.sum_lo = 0xFFFFFFFFFFFFFFFFull, a.sum_hi = 0;
  JoinAggMerge(a, b);
  CHECK(a.count == 2 && a.sum_lo == 0 && a.sum_hi == 1);
  // -1 + 1 = 0: the carry out of the low word cancels the high word of -1
  a = One(-1), JoinAggMerge(a, One(1));
  CHECK(a.count == 2 && a.sum_lo == 0 && a.sum_hi == 0 && a.min_i == -1 && a.max_i == 1);
  // 3 * (2^63 - 1) = 0x1_7FFFFFFFFFFFFFFD
  a = One(big), JoinAggMerge(a, One(big)), JoinAggMerge(a, One(big));
  CHECK(a.count == 3 && a.sum_lo == 0x7FFFFFFFFFFFFFFDull && a.sum_hi == 1);
  // 3 * -(2^63 - 1) = -0x1_7FFFFFFFFFFFFFFD = hi -2, lo 0x8000000000000003
  a = One(-big), JoinAggMerge(a, One(-big)), JoinAggMerge(a, One(-big));
  CHECK(a.count == 3 && a.sum_lo == 0x8000000000000003ull && a.sum_hi == -2);
  CHECK(a.min_i == -big && a.max_i == -big);
  // 1000 * (2^63 - 1) + 1000 * -(2^63 - 1) = 0, whatever the order
  a = JoinAggEmpty();
  for (int i = 0; i < 1000; i++) JoinAggMerge(a, One(i % 3 == 0 ? big : -big));
  for (int i = 0; i < 1000; i++) JoinAggMerge(a, One(i % 3 == 0 ? -big : big));
  CHECK(a.count == 2000 && a.sum_lo == 0 && a.sum_hi == 0 && a.min_i == -big && a.max_i == big);
  // 667 * (2^63 - 1) = 0x14D_7FFFFFFFFFFFFD65 (667 = 0x29B)
  a = JoinAggEmpty();
  for (int i = 0; i < 667; i++) JoinAggMerge(a, One(big));
  CHECK(a.sum_hi == 0x14D && a.sum_lo == 0x7FFFFFFFFFFFFD65ull);

  // an empty side, in both orders: the other side as it stands, min / max of negatives included
  JoinAggRec neg = One(-7);
  JoinAggMerge(neg, One(-3));
  CHECK(neg.min_i == -7 && neg.max_i == -3 && neg.sum_lo == (uint64_t)-10 && neg.sum_hi == -1);
  neg.sum_f = -0.0, neg.min_f = 5, neg.max_f = 9;
  a = neg, JoinAggMerge(a, JoinAggEmpty());
  CHECK(Same(a, neg));
  a = JoinAggEmpty(), JoinAggMerge(a, neg);
  CHECK(Same(a, neg));
  // a side without values whose other fields are not the initial ones still changes nothing
  JoinAggRec junk = JoinAggEmpty();
  junk.min_i = INT64_MIN, junk.max_i = INT64_MAX, junk.sum_lo = 99, junk.min_f = 0, junk.max_f = ~0ull;
  a = neg, JoinAggMerge(a, junk);
  CHECK(Same(a, neg));
  // two empty sides stay empty: the count decides NULL
  a = JoinAggEmpty(), JoinAggMerge(a, JoinAggEmpty());
  CHECK(Same(a, JoinAggEmpty()) && a.count == 0);
  // min / max of negatives, and of the order-encoded doubles
  a = One(-5), JoinAggMerge(a, One(INT64_MIN)), JoinAggMerge(a, One(-1));
  CHECK(a.min_i == INT64_MIN && a.max_i == -1);
  a = One(0), b = One(0);
  a.min_f = 10, a.max_f = 20, b.min_f = 3, b.max_f = 15, a.sum_f = 1.5, b.sum_f = -4.0;
  JoinAggMerge(a, b);
  CHECK(a.min_f == 3 && a.max_f == 20 && a.sum_f == -2.5);
}

static JoinAggRec ReadRec(FILE *f) {
  JoinAggRec r;
  uint64_t fbits;
  CHECK(fscanf(f, "%" SCNu64 " %" SCNu64 " %" SCNd64 " %" SCNd64 " %" SCNd64 " %" SCNu64 " %" SCNu64 " %" SCNu64, &r.count,
               &r.sum_lo, &r.sum_hi, &r.min_i, &r.max_i, &fbits, &r.min_f, &r.max_f) == 8);
  memcpy(&r.sum_f, &fbits, 8);
  return r;
}

static JoinAggRec Tree(const std::vector<JoinAggRec> &v, size_t lo, size_t hi) {
  if (hi - lo == 1) return v[lo];
  JoinAggRec a = Tree(v, lo, lo + (hi - lo) / 2);
  JoinAggMerge(a, Tree(v, lo + (hi - lo) / 2, hi));
  return a;
}

static void Orders(const char *path) {
  FILE *f = fopen(path, "r");
  CHECK(f);
  int n;
  CHECK(fscanf(f, "%d", &n) == 1 && n >= 2);
  const JoinAggRec want = ReadRec(f);
  std::vector<JoinAggRec> v;
  for (int i = 0; i < n; i++) v.push_back(ReadRec(f));
  fclose(f);
  JoinAggRec a = JoinAggEmpty();
  for (int i = 0; i < n; i++) JoinAggMerge(a, v[i]);
  CHECK(Same(a, want));
  a = JoinAggEmpty();
  for (int i = n - 1; i >= 0; i--) {
    JoinAggRec x = v[i];
    JoinAggMerge(x, a);
    a = x;
  }
  CHECK(Same(a, want));
  CHECK(Same(Tree(v, 0, v.size()), want));
  // the fold kernel's shape: lane t takes records t, t + 256, ..., then the lanes halve
  std::vector<JoinAggRec> lane(256, JoinAggEmpty());
  for (int t = 0; t < 256; t++)
    for (int i = t; i < n; i += 256) JoinAggMerge(lane[t], v[i]);
  for (int h = 128; h >= 1; h >>= 1)
    for (int t = 0; t < h; t++) JoinAggMerge(lane[t], lane[t + h]);
  CHECK(Same(lane[0], want));
}

int main(int argc, char **argv) {
  Decisions();
  Merges();
  if (argc > 1) Orders(argv[1]);
  printf("join agg plan: ok\n");
  return 0;
}
