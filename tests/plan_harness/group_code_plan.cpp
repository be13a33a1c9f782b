// Stand-alone host check of csrc/group_code.h (tests/test_group_code_plan.py
// builds and runs it): the group-code plan of 1..4 integer keys, its refusals,
// and encode -> decode round trips.  Prints "group code plan: ok" or the first
// failed check.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "group_code.h"

using namespace mbx;
typedef __int128 i128;

static int g_dummy;  // (the plan only carries the data pointers)

#define CHECK(c)                                                \
  do {                                                          \
    if (!(c)) {                                                 \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);   \
      exit(1);                                                  \
    }                                                           \
  } while (0)

static GroupCodeKeyIn Key(int phys, i128 lo, i128 hi, bool nullable, bool stats = true) {
  static const uint64_t words[1] = {0};
  GroupCodeKeyIn k;
  k.data = &g_dummy;
  k.validity = nullable ? words : nullptr;
  k.phys = phys;
  k.stats_valid = stats;
  k.imin = lo;
  k.imax = hi;
  return k;
}

// every combination of {min, max, NULL} per key encodes to a code in
// [0, total) and decodes to itself; distinct combinations get distinct codes
static void RoundTrip(const std::vector<GroupCodeKeyIn> &in) {
  GroupCodePlan p;
  const int ng = (int)in.size();
  CHECK(PlanGroupCode(in.data(), ng, &p));
  CHECK(p.nkeys == ng);
  int combos = 1;
  for (int q = 0; q < ng; q++) combos *= 3;
  std::vector<int64_t> seen;
  for (int c = 0; c < combos; c++) {
    bool valid[kGroupCodeMaxKeys], skip = false;
    int64_t v[kGroupCodeMaxKeys];
    for (int q = 0, r = c; q < ng; q++, r /= 3) {
      const int pick = r % 3;  // 0: min, 1: max, 2: NULL
      valid[q] = pick != 2;
      v[q] = pick == 0 ? (int64_t)in[q].imin : pick == 1 ? (int64_t)in[q].imax : 0;
      if (pick == 2 && !in[q].validity) skip = true;
      if (pick == 1 && in[q].imax == in[q].imin) skip = true;  // (the same value as pick 0)
    }
    if (skip) continue;
    const int64_t code = GroupCodeOf(p, valid, v);
    CHECK(code >= 0 && code < p.total);
    for (int64_t s : seen) CHECK(s != code);
    seen.push_back(code);
    for (int q = 0; q < ng; q++) {
      bool dv;
      int64_t dk;
      GroupCodeDecode(p, code, q, &dv, &dk);
      CHECK(dv == valid[q]);
      if (dv) CHECK(dk == v[q]);
    }
  }
}

int main() {
  const i128 two62 = (i128)1 << 62;
  GroupCodePlan p;
  // ---- total and strides: last key fastest, +1 digit per NULL-able key
  {
    GroupCodeKeyIn in[3] = {Key(P_I32, 0, 299, false), Key(P_I64, -50, 49, true), Key(P_I32, 7, 7, false)};
    CHECK(PlanGroupCode(in, 3, &p));
    CHECK(p.k[0].radix == 300 && p.k[1].radix == 101 && p.k[2].radix == 1);
    CHECK(p.k[2].stride == 1 && p.k[1].stride == 1 && p.k[0].stride == 101);
    CHECK(p.total == 300 * 101);
    CHECK(p.k[1].nullable == 1 && p.k[0].nullable == 0 && p.k[1].kmin == -50);
    const bool valid[3] = {true, false, true};
    const int64_t v[3] = {2, 0, 7};
    CHECK(GroupCodeOf(p, valid, v) == 2 * 101 + 100);  // NULL: the last digit
  }
  {
    GroupCodeKeyIn in[4] = {Key(P_I64, 10, 19, false), Key(P_I32, 0, 4, false), Key(P_I32, -3, 3, false),
                            Key(P_I64, 100, 101, true)};
    CHECK(PlanGroupCode(in, 4, &p));
    CHECK(p.k[3].stride == 1 && p.k[2].stride == 3 && p.k[1].stride == 21 && p.k[0].stride == 105);
    CHECK(p.total == 1050);
    // codes ascend with the keys compared left to right, NULL after every value
    const bool va[4] = {true, true, true, true}, vb[4] = {true, true, true, false};
    const int64_t a[4] = {10, 4, 3, 101}, b[4] = {10, 4, 3, 0}, c[4] = {11, 0, -3, 100};
    CHECK(GroupCodeOf(p, va, a) < GroupCodeOf(p, vb, b));
    CHECK(GroupCodeOf(p, vb, b) < GroupCodeOf(p, va, c));
  }
  // ---- round trips at every key's min, max and NULL digit, 1..4 keys
  RoundTrip({Key(P_I64, -5, 5, false)});
  RoundTrip({Key(P_I64, -5, 5, true)});
  RoundTrip({Key(P_I64, INT64_MIN, INT64_MIN + 1000, true)});
  RoundTrip({Key(P_I64, INT64_MAX - 1000, INT64_MAX, true)});
  RoundTrip({Key(P_I64, INT64_MIN, INT64_MIN + (int64_t)(two62 - 3), true)});  // total = 2^62 - 1
  RoundTrip({Key(P_I32, 0, 299, false), Key(P_I32, -50, 49, false)});
  RoundTrip({Key(P_I32, 0, 299, true), Key(P_I64, -50, 49, true)});
  RoundTrip({Key(P_I32, INT32_MIN, INT32_MAX, true), Key(P_I64, 1, 1 << 20, false)});
  RoundTrip({Key(P_I64, 0, 999 * (i128)1000003, false), Key(P_I32, 0, 49, true), Key(P_I32, 3, 3, true)});
  RoundTrip({Key(P_I32, -10, 9, true), Key(P_I64, (i128)1 << 33, ((i128)1 << 33) + 29, false),
             Key(P_I64, 0, 6, true), Key(P_I32, -5, 5, false)});
  RoundTrip({Key(P_I64, -(1 << 14), 1 << 14, true), Key(P_I64, -(1 << 14), 1 << 14, true),
             Key(P_I64, -(1 << 14), 1 << 14, true), Key(P_I64, -(1 << 14), 1 << 14, true)});
  // ---- refusals
  {
    GroupCodeKeyIn a = Key(P_I64, 0, two62 - 1, false);  // one key, radix 2^62
    CHECK(!PlanGroupCode(&a, 1, &p));
    GroupCodeKeyIn b = Key(P_I64, 0, two62 - 2, false);  // radix 2^62 - 1
    CHECK(PlanGroupCode(&b, 1, &p) && p.total == (int64_t)(two62 - 1));
    GroupCodeKeyIn c = Key(P_I64, 0, two62 - 2, true);  // ... + the NULL digit
    CHECK(!PlanGroupCode(&c, 1, &p));
    GroupCodeKeyIn d[2] = {Key(P_I64, 0, ((i128)1 << 31) - 1, false), Key(P_I64, 0, ((i128)1 << 31) - 1, false)};
    CHECK(!PlanGroupCode(d, 2, &p));  // 2^31 x 2^31
    d[1] = Key(P_I64, 0, ((i128)1 << 31) - 2, false);
    CHECK(PlanGroupCode(d, 2, &p));
    GroupCodeKeyIn e[2] = {Key(P_I64, 0, (i128)1 << 40, false), Key(P_I64, -((i128)1 << 39), (i128)1 << 39, false)};
    CHECK(!PlanGroupCode(e, 2, &p));  // two sparse keys spanning 2^40 each
    // the whole INT64 range: a radix of 2^64 (+ 1), computed without overflow
    GroupCodeKeyIn f = Key(P_I64, INT64_MIN, INT64_MAX, false), g = Key(P_I64, INT64_MIN, INT64_MAX, true);
    CHECK(!PlanGroupCode(&f, 1, &p) && !PlanGroupCode(&g, 1, &p));
    GroupCodeKeyIn h[4] = {f, f, f, f};  // 2^256 would wrap to 0
    CHECK(!PlanGroupCode(h, 4, &p));
    // an empty zone map (every value NULL): radix < 1 without the NULL digit
    GroupCodeKeyIn z = Key(P_I64, 0, -1, false);
    CHECK(!PlanGroupCode(&z, 1, &p));
    // not a plain INT32 / INT64 column with a zone map; too many / no keys
    GroupCodeKeyIn s = Key(P_I16, 0, 9, false), t = Key(P_F64, 0, 9, false), u = Key(P_I64, 0, 9, false, false);
    CHECK(!PlanGroupCode(&s, 1, &p) && !PlanGroupCode(&t, 1, &p) && !PlanGroupCode(&u, 1, &p));
    GroupCodeKeyIn five[5] = {b, b, b, b, b};
    for (auto &k : five) k = Key(P_I32, 0, 1, false);
    CHECK(!PlanGroupCode(five, 5, &p) && !PlanGroupCode(five, 0, &p) && PlanGroupCode(five, 4, &p));
  }
  printf("group code plan: ok\n");
  return 0;
}
