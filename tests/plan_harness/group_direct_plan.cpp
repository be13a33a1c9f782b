// Stand-alone host check of csrc/group_direct_plan.h (tests/test_group_direct_plan.py
// builds and runs it): invariants of the direct GROUP BY's launch plan over a
// sweep of shapes, the plan's LDS layout against the kernels' own arithmetic
// (kernels.hip: group_direct_kernel, group_direct_lds_kernel), and worked
// shapes at 256 CUs.  Prints "group direct plan: ok" or the first failed check.
#include <cstdio>
#include <cstdlib>
#include <initializer_list>

#include "group_direct_plan.h"

using namespace mbx;
typedef unsigned __int128 u128;
typedef GroupDirectForm F;

static const GroupDirectShape *g_shape;  // the shape under check, printed on failure
static void Describe() {
  const GroupDirectShape &s = *g_shape;
  fprintf(stderr, "shape: n=%lld nk=%d key=%d val=%d nv=%d mm=%d vm=%d maxabs=0x%llx%016llx npred=%d own=%d cus=%d\n",
          (long long)s.n, s.nk, s.key_bytes, s.val_bytes, s.nv, (int)s.mm, s.vm, (unsigned long long)(s.maxabs >> 64),
          (unsigned long long)s.maxabs, s.npred, s.npred_own, s.num_cus);
}
#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
      if (g_shape) Describe();                                \
      exit(1);                                                \
    }                                                         \
  } while (0)

static size_t Align16(size_t b) { return (b + 15) & ~(size_t)15; }

// ---- the kernels' own layout, restated from their bodies -------------------
// group_direct_lds_kernel<TK, TV, NV, MM, DEPTH, VN>: bytes of a ring slot
// (KB + NV * VB, VN: + 3 validity steps of 32 B, + the predicates' slices)
static size_t KernelSlot(const GroupDirectShape &s) {
  const int KB = 256 * s.key_bytes, VB = 256 * s.val_bytes;
  const int SBD = KB + s.nv * VB, NVW = s.vm ? 3 : 0, SB0 = SBD + 32 * NVW;
  int PB = 0;
  for (int j = 0; j < s.npred_own; j++) PB += 256 * s.pred_bytes[j];
  return SB0 + PB;
}
// the byte after the last table either kernel touches with R replicas: cnt
// (VN: cnt64), sum0 at the next 16 B, sum1 / mn0 / mx0 / mn1 / mx1 behind it,
// VN: vcnt1 after those
static size_t KernelTablesEnd(const GroupDirectShape &s, int R, bool vn) {
  const size_t nslot = (size_t)s.nk * R, cols = s.nv >= 2 ? 2 : 1;
  const size_t sum0 = Align16(nslot * (vn ? 8 : 4));
  const size_t vcnt1 = sum0 + cols * nslot * 8 + (s.mm ? 2 * cols * nslot * 8 : 0);
  return vcnt1 + (vn ? 4 * nslot : 0);
}

static bool Pow2(int x) { return x > 0 && (x & (x - 1)) == 0; }

static long g_forms[4];
static void Invariants(const GroupDirectShape &s) {
  g_shape = &s;
  const GroupDirectPlan p = PlanGroupDirect(s);
  const GroupDirectReplicas rep = PlanGroupDirectReplicas(s);
  g_forms[(int)p.form]++;
  CHECK((p.form == F::Unfit) == !rep.fit);
  if (p.form == F::Unfit) return;
  CHECK(Pow2(p.R) && p.R <= 64 && p.R <= rep.R);
  CHECK(p.seg_rows > 0);
  CHECK(p.ring_off % 16 == 0 && p.lds_bytes % 16 == 0);
  CHECK(p.records == (p.record_bytes != 0));
  if (p.records) {
    CHECK(p.form == F::LdsOneFlush && s.records_offered && s.nk <= kGroupPartialKeys);
    CHECK(p.record_bytes == (size_t)s.nk * p.grid * GroupPartialWords(s.nv, s.mm) * 8);
  }
  // a replica's int64 sum cannot overflow between flushes
  if (s.maxabs > 0) CHECK((u128)(p.seg_rows / p.R) * s.maxabs <= (u128)1 << 62);
  if (p.form == F::LdsOneFlush) {
    CHECK(p.depth == 2 || p.depth == 3);
    CHECK(p.gpc >= 1 && p.grid == s.num_cus * p.gpc);
    CHECK(p.lds_bytes <= GroupDirectLdsCap(p.gpc));
    // halving for the ring keeps the rows per replica
    CHECK(p.seg_rows * 64 / p.R == rep.seg_rows * 64 / rep.R);
    // one flush is enough: no workgroup sees more rows than the replicas absorb
    const int64_t waves = (int64_t)p.grid * 4, steps = ((s.n >> 8) + waves - 1) / waves;
    CHECK(steps * 4 * 256 + 256 <= p.seg_rows);
    // the layout is the kernel's
    CHECK(p.slot_bytes == KernelSlot(s));
    CHECK(KernelTablesEnd(s, p.R, s.vm != 0) <= p.table_bytes && p.table_bytes <= p.ring_off);
    CHECK(p.lds_bytes == p.ring_off + 4 * (size_t)p.depth * p.slot_bytes);
  }
  if (p.form == F::Segmented) {
    CHECK(s.vm == 0 && s.npred == 0);
    CHECK(!p.records);
    CHECK(p.chunk > 0 && p.chunk % 4 == 0 && p.seg_rows % 4 == 0 && p.seg_rows <= p.chunk);
    CHECK(p.grid >= 1 && (int64_t)p.grid * p.chunk >= s.n && (int64_t)(p.grid - 1) * p.chunk < s.n);
    CHECK(p.grid <= s.num_cus * 4);
    CHECK(KernelTablesEnd(s, p.R, false) <= p.table_bytes && p.lds_bytes == p.table_bytes);
    CHECK(p.lds_bytes <= 64 * 1024);
  }
}

static void Sweep() {
  const u128 one = 1;
  const u128 maxabs[] = {0, 1, 1000, one << 39, one << 50, one << 56, one << 62, one << 63};
  const int64_t rows[] = {1, 255, 256, 257, 4099, 1000003, 1000000000, (int64_t)1 << 30};
  for (int nk = 1; nk <= 1025; nk++)
    for (int nv = 0; nv <= 2; nv++)
      for (int mm = 0; mm < 2; mm++)
        for (int vm = 0; vm < 8; vm++)
          for (int kb : {4, 8})
            for (int vb : {4, 8})
              for (int np = 0; np <= GROUP_MAX_PRED; np++)
                for (u128 ma : maxabs)
                  for (int64_t n : rows)
                    for (int cus : {256, 64}) {
                      GroupDirectShape s;
                      s.n = n;
                      s.nk = nk;
                      s.key_bytes = kb;
                      s.val_bytes = vb;
                      s.nv = nv;
                      s.mm = mm != 0;
                      s.vm = vm;
                      s.maxabs = ma;
                      s.npred = s.npred_own = np;
                      for (int j = 0; j < np; j++) s.pred_bytes[j] = j == 1 ? 4 : 8;
                      s.num_cus = cus;
                      s.records_offered = true;
                      Invariants(s);
                    }
  for (int f = 0; f < 4; f++) CHECK(g_forms[f] > 0);  // the sweep reaches every form
}

// a shape at 256 CUs with a records buffer on offer
static GroupDirectShape Shape(int64_t n, int nk, int key_bytes, int nv, bool mm, int vm, u128 maxabs) {
  GroupDirectShape s;
  s.n = n;
  s.nk = nk;
  s.key_bytes = key_bytes;
  s.nv = nv;
  s.mm = mm;
  s.vm = vm;
  s.maxabs = maxabs;
  s.num_cus = 256;
  s.records_offered = true;
  return s;
}

// the knobs go through the same invariants
static void Knobs() {
  for (int nk : {1, 32, 100, 301, 1000})
    for (int nv = 0; nv <= 2; nv++)
      for (int vm : {0, 4, 7})
        for (int np = 0; np <= 2; np++)
          for (int own = 0; own <= np; own++)
            for (int64_t n : {4099, 1000000000})
              for (int variant = 0; variant < 6; variant++)
                for (int r : {0, 1, 8})
                  for (int atomic = 0; atomic < 2; atomic++) {
                    GroupDirectShape s = Shape(n, nk, 4, nv, nv > 0, vm, nv ? (u128)1 << 50 : 0);
                    s.npred = np;
                    s.npred_own = own;
                    for (int j = 0; j < own; j++) s.pred_bytes[j] = 8;
                    const int dg[6][2] = {{0, 0}, {0, 0}, {2, 1}, {2, 2}, {3, 3}, {5, 2}};
                    s.knobs.seg = variant == 1;
                    s.knobs.depth = dg[variant][0];
                    s.knobs.gpc = dg[variant][1];
                    s.knobs.r_cap = r;
                    s.knobs.atomic_flush = atomic != 0;
                    Invariants(s);
                    const GroupDirectPlan p = PlanGroupDirect(s);
                    if (p.form == F::LdsOneFlush) {
                      if (variant >= 2) CHECK(p.gpc == dg[variant][1] && p.depth == (dg[variant][0] <= 2 ? 2 : 3));
                      if (r) CHECK(p.R <= r);
                      if (atomic) CHECK(!p.records);
                    }
                    if (variant == 1 && np == 0) CHECK(p.form != F::LdsOneFlush);
                  }
}

// Worked shapes (256 CUs), each recomputed from the decisions as they stood
// in aggregate.cpp and GroupByDirectStates before this header held them.
static void Pinned() {
  g_shape = nullptr;
  const u128 one = 1;
  {  // C3-like: 100 int32 keys, one int64 value
    const GroupDirectPlan p = PlanGroupDirect(Shape(1000000000, 100, 4, 1, false, 0, 1000000));
    CHECK(p.form == F::LdsOneFlush && p.R == 32 && p.depth == 2 && p.gpc == 1 && p.grid == 256);
    CHECK(p.seg_rows == (int64_t)32 << 30);
    CHECK(p.table_bytes == 38400 && p.ring_off == 38400 && p.slot_bytes == 3072 && p.lds_bytes == 62976);
    CHECK(p.records && p.record_bytes == 100 * 256 * 4 * 8);
  }
  {  // NULL-able int32 key, MIN / MAX: the ring takes R from 4 to 2; too many keys for records
    const GroupDirectShape s = Shape(4099, 301, 4, 1, true, 4, 1000000);
    const GroupDirectPlan p = PlanGroupDirect(s);
    CHECK(PlanGroupDirectReplicas(s).R == 4);
    CHECK(p.form == F::LdsOneFlush && p.R == 2 && p.depth == 2 && p.gpc == 3 && p.grid == 768);
    CHECK(p.seg_rows == (int64_t)2 << 30);
    CHECK(p.ring_off == 21680 && p.slot_bytes == 3168 && p.lds_bytes == 47024 && !p.records);
  }
  {  // a predicate on a third (int64) column: a 3-deep ring
    GroupDirectShape s = Shape(4099, 300, 4, 1, false, 0, 1000000);
    s.npred = s.npred_own = 1;
    s.pred_bytes[0] = 8;
    const GroupDirectPlan p = PlanGroupDirect(s);
    CHECK(p.form == F::LdsOneFlush && p.R == 8 && p.depth == 3 && p.gpc == 1 && p.grid == 256);
    CHECK(p.ring_off == 28800 && p.slot_bytes == 5120 && p.lds_bytes == 90240 && !p.records);
  }
  {  // NULL-able everything at 1000 keys: 109920 B at R = 1, above 64 KiB at 3 workgroups per CU
    const GroupDirectPlan p = PlanGroupDirect(Shape(1000000000, 1000, 8, 2, true, 7, 1000000));
    CHECK(p.form == F::Refused && p.R == 1 && p.lds_bytes == 109920);
  }
  {  // values up to 2^50: 262144 rows per flush, below a workgroup's 3906816
    const GroupDirectPlan p = PlanGroupDirect(Shape(1000000000, 40, 8, 1, false, 0, one << 50));
    CHECK(p.form == F::Segmented && p.R == 64 && p.seg_rows == 262144);
    CHECK(p.grid == 1024 && p.chunk == 976564 && p.table_bytes == 30720 && p.lds_bytes == 30720 && !p.records);
  }
  {  // COUNT only
    const GroupDirectPlan p = PlanGroupDirect(Shape(1000000000, 32, 4, 0, false, 0, 0));
    CHECK(p.form == F::LdsOneFlush && p.R == 64 && p.depth == 2 && p.gpc == 3 && p.grid == 768);
    CHECK(p.ring_off == 24576 && p.lds_bytes == 32768 && p.records && p.record_bytes == 32 * 768 * 1 * 8);
  }
  // values up to 2^62: one row per replica
  CHECK(PlanGroupDirect(Shape(1000000000, 40, 8, 2, true, 0, one << 62)).form == F::Unfit);
  {  // the 1 000 003-row table of the GPU suite's f2_segmented: 4096 rows per flush, cut to the chunk
    const GroupDirectPlan p = PlanGroupDirect(Shape(1000003, 40, 8, 1, false, 0, one << 56));
    CHECK(p.form == F::Segmented && p.R == 64 && p.grid == 1021 && p.chunk == 980 && p.seg_rows == 980);
  }
  {  // ... and of f2_refused: 1000 int32 keys and the NULL group, two NULL-able int64 columns, MIN / MAX
    const GroupDirectPlan p = PlanGroupDirect(Shape(4099, 1001, 4, 2, true, 7, 1000000));
    CHECK(p.form == F::Refused && p.R == 1 && p.ring_off == 60080 && p.lds_bytes == 101808);
  }
  {  // "seg" asks for the segmented kernel ...
    GroupDirectShape s = Shape(1000000000, 100, 4, 1, false, 0, 1000000);
    s.knobs.seg = true;
    GroupDirectPlan p = PlanGroupDirect(s);
    CHECK(p.form == F::Segmented && p.R == 32 && p.grid == 1024 && p.chunk == 976564 && p.seg_rows == 976564);
    // ... and is ignored when a predicate is present (here one on the key)
    s.npred = 1;
    p = PlanGroupDirect(s);
    CHECK(p.form == F::LdsOneFlush && p.R == 32 && p.depth == 2 && p.gpc == 1 && p.lds_bytes == 62976 && p.records);
    // NULL-able columns have no segmented kernel to go to
    s.npred = 0;
    s.vm = 1;
    CHECK(PlanGroupDirect(s).form == F::Refused);
  }
}

int main() {
  Pinned();
  Knobs();
  Sweep();
  printf("group direct plan: ok\n");
  return 0;
}
