// join_mark_plan.h — the mark join behind x IN (subquery) (executor.cpp:
// MarkLowering; join_kernels.hip: join_probe_mark): SQL's three-valued
// membership as one cell function, and what the host decides before a launch.
//
// The subquery's rows are the set S.  Its non-NULL keys go into the table of
// join_plan.h; whether S has any row at all and whether it holds a NULL are two
// facts beside the table.  A probe row's mark is then a function of four bits:
//
//   S has no row at all                      -> FALSE (even for a NULL x)
//   x is NULL                                -> NULL
//   x equals a member                        -> TRUE
//   x equals no member, S holds a NULL       -> NULL
//   x equals no member, S holds no NULL      -> FALSE
//
// NOT IN is the VM's three-valued NOT over the mark column.  The kernel and the
// host both call JoinMarkCell; neither keeps a second copy of the table above.
// No HIP types: the functions also build in a plain host program
// (tests/plan_harness/join_mark_plan.cpp).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MBX_JM_HD __host__ __device__ __forceinline__
#else
#define MBX_JM_HD inline
#endif

namespace mbx {

struct JoinMarkCellValue {
  uint8_t value;  // the BOOLEAN column's byte (0 where the cell is NULL)
  bool valid;     // the cell's validity bit
};

MBX_JM_HD JoinMarkCellValue JoinMarkCell(bool found, bool key_valid, bool set_empty, bool set_has_null) {
  if (set_empty) return {0, true};
  if (!key_valid) return {0, false};
  if (found) return {1, true};
  return {0, !set_has_null};
}

// What the host knows once the subquery has run
struct JoinMarkFacts {
  int64_t set_rows = 0;         // rows of the subquery, NULL keys included
  int64_t set_nulls = 0;        // of them NULL
  bool probe_nullable = false;  // the probe key column has a validity bitmap
};

struct JoinMarkPlan {
  bool constant_false;  // S is empty: every cell is FALSE and nothing is launched
  bool validity;        // the mark column needs a validity bitmap of its own
  bool lookup;          // S has a non-NULL key: there is a table to probe
  bool set_has_null;
};

inline JoinMarkPlan JoinMarkDecide(const JoinMarkFacts &f) {
  JoinMarkPlan p;
  p.constant_false = f.set_rows <= 0;
  p.set_has_null = !p.constant_false && f.set_nulls > 0;
  // a cell is NULL only for a NULL probe key or for a miss against a set that holds a NULL
  p.validity = !p.constant_false && (f.probe_nullable || p.set_has_null);
  p.lookup = !p.constant_false && f.set_rows > f.set_nulls;
  return p;
}

}  // namespace mbx
