// group_pred_plan.h — the predicate plan of the partitioned GROUP BY
// (group_part.hip): a WHERE that is a conjunction of integer range comparisons
// (RangeConj: column -> inclusive [lo, hi]) becomes at most GROUP_MAX_PRED
// entries {data, phys, lo, span} that the hist and scatter passes test per row
// as (uint64_t)(x - lo) <= span, so rows that fail never become records.
// Every range is judged against its column's zone map first: a range the zone
// map rules out empties the result, one that covers the zone map drops out,
// and what stays is clamped to the zone map before it narrows to 64 bits.
// An entry whose column is a key or value column of the shape names that
// operand (src) and is compared in the register its load already filled.
// No HIP types: the planning function also builds in a plain host program
// (tests/plan_harness/group_pred_plan.cpp).
#pragma once
#include <stdint.h>

#include "group_direct_plan.h"  // GROUP_MAX_PRED
#include "phys.h"

namespace mbx {

// where the compared value of an entry comes from
enum GroupPredSrc : int32_t {
  kPredOwn = 0,      // its own column, loaded for the predicate alone
  kPredKey = 1,      // the key column (single-key shapes)
  kPredV0 = 2,       // value column 0
  kPredV1 = 3,       // value column 1
  kPredCodeKey = 4,  // + q: key column q of the group code
};

struct GroupPredEntry {
  const void *data;
  int32_t phys;  // P_I32 / P_I64
  int32_t src;   // GroupPredSrc
  int64_t lo;
  uint64_t span;  // a row passes when (uint64_t)(x - lo) <= span
};

// passed by value to the kernels; n, the widths and the bounds are wave-uniform
struct GroupPredSet {
  int32_t n;      // entries in use; 0: no predicate (the kernels without one run)
  int32_t empty;  // 1: no row can pass (the passes are skipped)
  GroupPredEntry p[GROUP_MAX_PRED];
};

enum class GroupPredVerdict {
  Unfit,   // the partitioned GROUP BY declines the statement
  Empty,   // no row can pass
  All,     // every row passes: no predicate is left
  Filter,  // set.n entries remain
};

// one range of the conjunction and what the planner knows of its column
struct GroupPredIn {
  int col;  // the column's index in the relation
  const void *data;
  int phys;
  bool has_validity;  // the column carries a validity bitmap
  bool stats_valid;
  __int128 imin, imax;  // zone map
  int64_t null_count;
  __int128 lo, hi;  // inclusive; lo > hi: empty (a comparison with NULL)
};

// the key and value columns of the shape (indices in the relation)
struct GroupPredShape {
  int nkeys;  // 1 with code = false: the single-key kernels
  bool code;  // the keys fold into a group code (PgCode)
  int key_cols[4];
  int nv;
  int val_cols[2];
};

struct GroupPredPlan {
  GroupPredVerdict verdict;
  GroupPredSet set;
  int own_bytes;  // bytes per row of predicate columns that are no key or value column of the shape
};

inline GroupPredPlan PlanGroupPreds(const GroupPredIn *in, int nin, const GroupPredShape &shape) {
  GroupPredPlan out = {};
  out.verdict = GroupPredVerdict::Unfit;
  // an empty range selects nothing, whatever its column is
  for (int i = 0; i < nin; i++)
    if (in[i].lo > in[i].hi) {
      out.verdict = GroupPredVerdict::Empty;
      out.set.empty = 1;
      return out;
    }
  bool outside = false;
  GroupPredSet set = {};
  int own_bytes = 0;
  for (int i = 0; i < nin; i++) {
    const GroupPredIn &c = in[i];
    if ((c.phys != P_I32 && c.phys != P_I64) || !c.data || c.has_validity || c.null_count != 0 || !c.stats_valid ||
        c.imin > c.imax || c.imin < (__int128)INT64_MIN || c.imax > (__int128)INT64_MAX)
      return out;  // Unfit
    if (c.lo > c.imax || c.hi < c.imin) {
      outside = true;
      continue;
    }
    if (c.lo <= c.imin && c.hi >= c.imax) continue;  // covers the zone map: no predicate
    if (set.n == GROUP_MAX_PRED) return out;         // a fourth column: Unfit
    const __int128 lo = c.lo > c.imin ? c.lo : c.imin, hi = c.hi < c.imax ? c.hi : c.imax;
    GroupPredEntry &e = set.p[set.n++];
    e.data = c.data;
    e.phys = c.phys;
    e.lo = (int64_t)lo;
    e.span = (uint64_t)(int64_t)hi - (uint64_t)(int64_t)lo;
    e.src = kPredOwn;
    for (int q = 0; q < shape.nkeys && q < 4; q++)
      if (shape.key_cols[q] == c.col) e.src = shape.code ? kPredCodeKey + q : kPredKey;
    if (e.src == kPredOwn)
      for (int j = 0; j < shape.nv && j < 2; j++)
        if (shape.val_cols[j] == c.col) {
          e.src = j == 0 ? kPredV0 : kPredV1;
          break;
        }
    if (e.src == kPredOwn) own_bytes += c.phys == P_I64 ? 8 : 4;
  }
  if (outside) {
    out.verdict = GroupPredVerdict::Empty;
    out.set.empty = 1;
    return out;
  }
  out.set = set;
  out.own_bytes = set.n ? own_bytes : 0;
  out.verdict = set.n ? GroupPredVerdict::Filter : GroupPredVerdict::All;
  return out;
}

}  // namespace mbx
