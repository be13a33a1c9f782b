// Stand-alone host check of csrc/join_mark_plan.h (tests/test_join_mark_plan.py
// builds and runs it): the cell function of x IN (subquery) on all 16
// combinations of its four inputs against a truth table written out below
// (SQL's three-valued IN, as DuckDB answers it), and the host plan's verdicts:
// when the mark column is the constant FALSE, when it needs a validity bitmap
// of its own, when there is a table to probe.  Prints "join mark plan: ok" or
// the first failed check.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "join_mark_plan.h"

using namespace mbx;

#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
      exit(1);                                                \
    }                                                         \
  } while (0)

enum Cell { F, T, N };  // FALSE, TRUE, NULL

// index: found * 8 + key_valid * 4 + set_empty * 2 + set_has_null
// (an empty set that "holds a NULL", or a key "found" in an empty set or for
// a NULL key, cannot come from the executor; the function still has to answer
// by the first rule that applies: empty set, then NULL key, then found)
static const Cell kTruth[16] = {
    /* found=0 valid=0 empty=0 null=0 */ N,
    /* found=0 valid=0 empty=0 null=1 */ N,
    /* found=0 valid=0 empty=1 null=0 */ F,
    /* found=0 valid=0 empty=1 null=1 */ F,
    /* found=0 valid=1 empty=0 null=0 */ F,
    /* found=0 valid=1 empty=0 null=1 */ N,
    /* found=0 valid=1 empty=1 null=0 */ F,
    /* found=0 valid=1 empty=1 null=1 */ F,
    /* found=1 valid=0 empty=0 null=0 */ N,
    /* found=1 valid=0 empty=0 null=1 */ N,
    /* found=1 valid=0 empty=1 null=0 */ F,
    /* found=1 valid=0 empty=1 null=1 */ F,
    /* found=1 valid=1 empty=0 null=0 */ T,
    /* found=1 valid=1 empty=0 null=1 */ T,
    /* found=1 valid=1 empty=1 null=0 */ F,
    /* found=1 valid=1 empty=1 null=1 */ F,
};

static void Cells() {
  for (int i = 0; i < 16; i++) {
    const JoinMarkCellValue c = JoinMarkCell((i & 8) != 0, (i & 4) != 0, (i & 2) != 0, (i & 1) != 0);
    const Cell got = !c.valid ? N : c.value ? T : F;
    CHECK(got == kTruth[i]);
    CHECK(c.value == 0 || c.value == 1);
    CHECK(c.valid || c.value == 0);  // a NULL cell's byte is 0, like every other BOOLEAN writer's
  }
}

static JoinMarkFacts Facts(int64_t rows, int64_t nulls, bool nullable) {
  JoinMarkFacts f;
  f.set_rows = rows;
  f.set_nulls = nulls;
  f.probe_nullable = nullable;
  return f;
}

static void Plans() {
  // no row at all: the constant FALSE, nothing else asked for, whatever the probe side is
  for (bool nullable : {false, true}) {
    const JoinMarkPlan p = JoinMarkDecide(Facts(0, 0, nullable));
    CHECK(p.constant_false && !p.validity && !p.lookup && !p.set_has_null);
  }
  // rows, no NULL on either side: bytes only
  JoinMarkPlan p = JoinMarkDecide(Facts(1, 0, false));
  CHECK(!p.constant_false && !p.validity && p.lookup && !p.set_has_null);
  p = JoinMarkDecide(Facts(1000000, 0, false));
  CHECK(!p.constant_false && !p.validity && p.lookup && !p.set_has_null);
  // a NULL-able probe key alone asks for validity
  p = JoinMarkDecide(Facts(3, 0, true));
  CHECK(!p.constant_false && p.validity && p.lookup && !p.set_has_null);
  // a NULL in the set alone asks for validity
  p = JoinMarkDecide(Facts(3, 1, false));
  CHECK(!p.constant_false && p.validity && p.lookup && p.set_has_null);
  p = JoinMarkDecide(Facts(3, 1, true));
  CHECK(!p.constant_false && p.validity && p.lookup && p.set_has_null);
  // a set of NULLs only: not empty (no constant), nothing to probe, every cell NULL
  p = JoinMarkDecide(Facts(2, 2, false));
  CHECK(!p.constant_false && p.validity && !p.lookup && p.set_has_null);
  p = JoinMarkDecide(Facts(1, 1, true));
  CHECK(!p.constant_false && p.validity && !p.lookup && p.set_has_null);
  // the plan and the cell function agree: without validity no input the plan admits gives a NULL cell
  for (int rows : {0, 1, 5})
    for (int nulls = 0; nulls <= rows; nulls++)
      for (bool nullable : {false, true}) {
        const JoinMarkPlan q = JoinMarkDecide(Facts(rows, nulls, nullable));
        for (int found = 0; found < 2; found++)
          for (int valid = 0; valid < 2; valid++) {
            if (!nullable && !valid) continue;   // a column without a bitmap has no NULL key
            if (found && (!q.lookup || !valid)) continue;  // only a valid key is looked up, and only in a table
            const JoinMarkCellValue c = JoinMarkCell(found, valid, q.constant_false, q.set_has_null);
            if (!q.validity) CHECK(c.valid);
            if (q.constant_false) CHECK(c.valid && c.value == 0);
          }
      }
}

int main() {
  Cells();
  Plans();
  printf("join mark plan: ok\n");
  return 0;
}
