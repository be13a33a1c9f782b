// join_agg_plan.h — the fused probe-and-aggregate of a global aggregate over
// an inner join (join.cpp: JoinAggregate; join_kernels.hip: join_probe_agg,
// join_agg_fold): whether a statement takes it, and how two partial records of
// one aggregate merge.
//
// The fused kernel interprets the residual, the WHERE and the aggregate
// arguments for every pair while the pair exists only in registers, so it
// takes what the tile interpreter can evaluate and what fits its states; a
// tile costs as many interpreter passes as the longest build run among its 256
// probe rows, so a build side with a long run goes to the materialising path,
// which lays its work out by pairs.
// No HIP types: the functions also build in a plain host program
// (tests/plan_harness/join_agg_plan.cpp).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MBX_JA_HD __host__ __device__ __forceinline__
#else
#define MBX_JA_HD inline
#endif

namespace mbx {

// What JoinAggregate knows about a statement and its build side when it chooses
struct JoinAggFacts {
  bool enabled = true;          // mbx_join_agg
  bool distinct = false;        // a DISTINCT aggregate
  bool varchar = false;         // a VARCHAR column, argument or predicate in the residual, the WHERE or an argument
  bool minmax_128 = false;      // MIN / MAX of a 128-bit value
  bool membership = false;      // an IN (subquery) leaf in the residual, the WHERE or an argument
  int n_aggs = 0;
  int max_aggs = 0;             // VM_MAX_OUT
  bool compile_failed = false;  // VmCompiler refused one of the three stages
  int64_t max_run = 0;          // the longest run of equal keys on the build side
  int64_t max_run_limit = 0;    // mbx_join_agg_max_run
};

struct JoinAggChoice {
  bool take;
  const char *reason;  // why not (for a debug print); "" when taken
};

inline JoinAggChoice JoinAggDecide(const JoinAggFacts &f) {
  if (!f.enabled) return {false, "mbx_join_agg=false"};
  if (f.distinct) return {false, "a DISTINCT aggregate"};
  if (f.varchar) return {false, "a VARCHAR column, argument or predicate"};
  if (f.minmax_128) return {false, "MIN/MAX of a 128-bit value"};
  if (f.membership) return {false, "an IN (subquery) leaf, which is lowered to a column first"};
  if (f.n_aggs > f.max_aggs) return {false, "more aggregates than the program has outputs"};
  if (f.compile_failed) return {false, "the expression compiler refused a stage"};
  if (f.max_run > f.max_run_limit) return {false, "a build run longer than mbx_join_agg_max_run"};
  return {true, ""};
}

// One aggregate's statistics over some of the pairs; the layout of
// dev::AggState, so the fold writes the emit's input as it stands.
struct JoinAggRec {
  uint64_t count;         // non-NULL argument values
  uint64_t sum_lo;        // their int128 sum
  int64_t sum_hi;
  int64_t min_i, max_i;   // signed min / max (64-bit classes)
  double sum_f;           // double sum
  uint64_t min_f, max_f;  // min / max of order-encoded doubles
};

// the record of no value: what dev::InitAggStates writes
MBX_JA_HD JoinAggRec JoinAggEmpty() {
  JoinAggRec r;
  r.count = 0;
  r.sum_lo = 0;
  r.sum_hi = 0;
  r.min_i = INT64_MAX;
  r.max_i = INT64_MIN;
  r.sum_f = 0;
  r.min_f = 0xFFFFFFFFFFFFFFFFull;
  r.max_f = 0;
  return r;
}

// a <- a merged with b.  The int128 add carries from the low word; a side
// without values leaves the other as it is (its min / max, and the sign of a
// zero double sum); the count, which decides NULL, adds.
MBX_JA_HD void JoinAggMerge(JoinAggRec &a, const JoinAggRec &b) {
  if (b.count == 0) return;
  if (a.count == 0) {
    a = b;
    return;
  }
  a.count += b.count;
  const uint64_t lo = a.sum_lo + b.sum_lo;
  a.sum_hi = (int64_t)((uint64_t)a.sum_hi + (uint64_t)b.sum_hi + (lo < a.sum_lo ? 1u : 0u));
  a.sum_lo = lo;
  a.min_i = b.min_i < a.min_i ? b.min_i : a.min_i;
  a.max_i = b.max_i > a.max_i ? b.max_i : a.max_i;
  a.sum_f += b.sum_f;
  a.min_f = b.min_f < a.min_f ? b.min_f : a.min_f;
  a.max_f = b.max_f > a.max_f ? b.max_f : a.max_f;
}

}  // namespace mbx
