// group_direct_plan.h — the launch plan of the fused GROUP BY on a small-range
// integer key (group_direct / group_direct_lds in kernels.hip; path F2, config
// C3): how many table replicas, how many rows a replica may absorb before its
// int64 sums could overflow, the ring depth and workgroups per CU, the LDS
// layout, and which form runs.  The callers (aggregate.cpp) plan once, branch
// on the form and size their buffers from the plan; GroupDirectLaunch only
// launches what the plan says.  The MBX_GD_* switches mean what this header
// does with GroupDirectKnobs.
// No HIP types and no environment: the planning also builds in a plain host
// program (tests/plan_harness/group_direct_plan.cpp).
#pragma once
#include <stddef.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define MBX_GD_HD __host__ __device__ constexpr
#else
#define MBX_GD_HD constexpr
#endif

#define GROUP_MAX_PRED 3  // range predicates fused into the scan

namespace mbx {

// Per-workgroup partial records of group_direct_lds (key-major, GroupPartialWords
// u64 each: COUNT(*), then per value column its valid-row count, sum lo / hi
// and, with MIN/MAX, min / max), reduced by GroupPartialsCompact.
constexpr int kGroupPartialKeys = 128;
MBX_GD_HD int GroupPartialWords(int nv, bool mm) { return 1 + nv * (mm ? 5 : 3); }

// ---- LDS layout: the replicated tables, then every wave's ring -------------
// Tables of nk * R slots: COUNT(*) as u32 (vm: u64, value 0's valid rows in the
// high half), 16-aligned; an int64 sum per value column (one column's room for
// COUNT only); with MIN/MAX a min and a max per column; vm: value 1's valid
// rows as u32.  vm: NULL-able columns (bit 0 value 0, bit 1 value 1, bit 2 the
// key).
MBX_GD_HD size_t GroupDirectLds(int nk, int R, int nv, bool mm, int vm = 0) {
  const size_t nslot = (size_t)nk * R, cols = nv >= 2 ? 2 : 1;
  size_t b = (nslot * (vm ? 8 : 4) + 15) & ~(size_t)15;
  b += nslot * 8 * cols;
  if (mm) b += nslot * 8 * 2 * cols;
  if (vm) b += 4 * ((nslot + 3) & ~(size_t)3);
  return (b + 15) & ~(size_t)15;
}
// One ring slot (a wave's 256-row step): the key slice, the value slices, vm:
// three 32-B steps of validity words, then the predicates' own column slices.
MBX_GD_HD size_t GroupDirectSlot(int key_bytes, int val_bytes, int nv, int vm, int npred_own, const int *pred_bytes) {
  size_t b = 256 * (size_t)key_bytes + (size_t)nv * 256 * val_bytes + (vm ? 3 * 32 : 0);
  for (int j = 0; j < npred_own; j++) b += 256 * (size_t)pred_bytes[j];
  return b;
}
// LDS one workgroup may ask for at gpc workgroups per CU (160 KiB per CU)
MBX_GD_HD size_t GroupDirectLdsCap(int gpc) { return gpc <= 1 ? 150 * 1024 : gpc == 2 ? 76 * 1024 : 64 * 1024; }

// MBX_GD_VARIANT="d<2|3>_g<workgroups per CU>" (depth, gpc) or anything else
// ("seg": the segmented kernel; ignored when predicates are present, which
// only the LDS-DMA kernel evaluates); MBX_GD_R=<r>: at most r replicas;
// MBX_GD_XCD=1: XCD-grouped step windows; MBX_GD_ATOMIC_FLUSH: no records.
struct GroupDirectKnobs {
  int depth = 0, gpc = 0;  // 0: the defaults
  bool seg = false;
  int r_cap = 0;
  bool xcd = false;
  bool atomic_flush = false;
};

struct GroupDirectShape {
  int64_t n = 0;                         // rows
  int nk = 0;                            // key slots (the NULL group's included)
  int key_bytes = 8, val_bytes = 8;      // 4 or 8; val_bytes is 8 when nv == 0
  int nv = 0;                            // value columns, 0..2
  bool mm = false;                       // MIN / MAX wanted
  int vm = 0;                            // NULL-able columns (GroupDirectLds)
  unsigned __int128 maxabs = 0;          // zone-map bound on |value|, 0: no values
  int npred = 0;                         // range predicates in all
  int npred_own = 0;                     // ... of which on columns of their own,
  int pred_bytes[GROUP_MAX_PRED] = {};   // with these widths
  int num_cus = 0;
  bool records_offered = false;          // the caller can take per-workgroup records
  GroupDirectKnobs knobs;
};

enum class GroupDirectForm {
  Unfit,        // not a shape of this path: the caller tries the next one
  Refused,      // a shape of this path that no form can run
  LdsOneFlush,  // group_direct_lds: every workgroup flushes its table once
  Segmented,    // group_direct: a flush every seg_rows rows
};

struct GroupDirectPlan {
  GroupDirectForm form = GroupDirectForm::Unfit;
  int R = 0;             // table replicas (lane % R picks one)
  int64_t seg_rows = 0;  // rows R replicas may absorb between flushes
  int depth = 0, gpc = 0, grid = 0;
  size_t table_bytes = 0, ring_off = 0, slot_bytes = 0, lds_bytes = 0;
  int64_t chunk = 0;  // Segmented: rows per workgroup
  bool records = false;  // LdsOneFlush: records (record_bytes of them) instead of the atomic flush
  size_t record_bytes = 0;
  bool xcd = false;
};

// The replicas and the overflow bound: 64 replicas, halved while the table is
// above 48 KiB; a replica's int64 sum holds 2^62 / maxabs rows; a bound above
// 2^31 rows per replica (its count is a u32) becomes 2^30.  fit: the table
// fits 64 KiB and R replicas hold 4096 rows.
struct GroupDirectReplicas {
  bool fit;
  int R;
  int64_t seg_rows;
};
inline GroupDirectReplicas PlanGroupDirectReplicas(const GroupDirectShape &s) {
  GroupDirectReplicas r = {false, 64, 0};
  while (r.R > 1 && GroupDirectLds(s.nk, r.R, s.nv, s.mm, s.vm) > 48 * 1024) r.R >>= 1;
  if (GroupDirectLds(s.nk, r.R, s.nv, s.mm, s.vm) > 64 * 1024) return r;
  const int64_t cap = (int64_t)r.R << 30;
  r.seg_rows = cap;
  if (s.maxabs > 0) {
    const unsigned __int128 seg128 = (((unsigned __int128)1 << 62) / s.maxabs) * r.R;
    if (seg128 < 4096) return r;
    if (seg128 <= (unsigned __int128)cap * 2) r.seg_rows = (int64_t)seg128;
  }
  r.fit = true;
  return r;
}

inline GroupDirectPlan PlanGroupDirect(const GroupDirectShape &s) {
  typedef GroupDirectForm F;
  GroupDirectPlan p;
  if (s.n <= 0 || s.nk < 1 || s.nk > 1025 || s.nv < 0 || s.nv > 2 || s.npred_own > GROUP_MAX_PRED) return p;
  const GroupDirectReplicas rep = PlanGroupDirectReplicas(s);
  if (!rep.fit) return p;
  p.R = rep.R;
  p.seg_rows = rep.seg_rows;
  p.xcd = s.knobs.xcd;
  p.form = F::Refused;
  const bool vv = s.vm != 0;
  if (((s.vm & 1) && s.nv < 1) || ((s.vm & 2) && s.nv < 2)) return p;
  // Defaults from profiles/r02_group_sweep.log (after the table atomics stopped
  // draining the DMA ring): d2_g1 for value aggregates (C3 1.735-1.77 ms, 2-6 %
  // under d2_g3 on two boxes) and d2_g3 for COUNT-only tables (0.56 ms vs 0.62
  // on the segmented kernel).  NULL-able columns: three 2-deep workgroups per
  // CU -- the validity words' extra LDS reads and selects per step want more
  // waves to hide them (C3 with NULLs 1.90 ms at d2_g3 vs 2.13 at d2_g2 and
  // 2.32 at d2_g1, profiles/r06_gd_nulls/).  Predicate slices of their own: a
  // deeper ring (c3_where: d3 3.00 vs d2 3.32 ms).
  p.depth = s.npred_own ? 3 : 2;
  p.gpc = s.nv > 0 ? (vv ? 3 : 1) : 3;
  if (s.knobs.depth || s.knobs.gpc) {
    p.depth = s.knobs.depth;
    p.gpc = s.knobs.gpc;
  }
  const bool use_lds = !s.knobs.seg || s.npred != 0;
  if (vv && !use_lds) return p;  // the segmented kernel has no validity words
  if (use_lds) {
    for (; s.knobs.r_cap > 0 && p.R > s.knobs.r_cap; p.R >>= 1) p.seg_rows >>= 1;
    p.depth = p.depth <= 2 ? 2 : 3;  // the kernel is built for 2- and 3-deep rings
    p.grid = s.num_cus * p.gpc;
    const int64_t nsteps = s.n >> 8, waves = (int64_t)p.grid * 4;
    const int64_t rows_per_block = ((nsteps + waves - 1) / waves) * 4 * 256 + 256;
    p.slot_bytes = GroupDirectSlot(s.key_bytes, s.val_bytes, s.nv, s.vm, s.npred_own, s.pred_bytes);
    const size_t lds_cap = GroupDirectLdsCap(p.gpc);
    auto layout = [&] {
      p.table_bytes = p.ring_off = GroupDirectLds(s.nk, p.R, s.nv, s.mm, s.vm);  // (16-aligned)
      p.lds_bytes = p.ring_off + 4 * (size_t)p.depth * p.slot_bytes;
    };
    // wide slots: trade table replicas for ring space; seg_rows scales with R
    // (rows per replica stay the same)
    for (layout(); p.lds_bytes > lds_cap && p.R > 1; layout()) {
      p.R >>= 1;
      p.seg_rows >>= 1;
    }
    // one flush at the end must be overflow-safe (else the segmented kernel)
    if (p.seg_rows >= rows_per_block && p.lds_bytes <= lds_cap) {
      p.form = F::LdsOneFlush;
      // records reduced by group_partials_compact instead of the flush's global
      // atomics (every workgroup hitting the same nk states at once)
      p.records = s.records_offered && s.nk <= kGroupPartialKeys && !s.knobs.atomic_flush;
      if (p.records) p.record_bytes = (size_t)s.nk * p.grid * GroupPartialWords(s.nv, s.mm) * 8;
      return p;
    }
  }
  if (vv || s.npred) return p;  // validity words and predicates need the LDS-DMA kernel
  p.form = F::Segmented;
  p.depth = p.gpc = 0;
  p.ring_off = p.slot_bytes = 0;
  p.grid = s.num_cus * 4;
  p.chunk = ((s.n + p.grid - 1) / p.grid + 3) & ~(int64_t)3;
  p.grid = (int)((s.n + p.chunk - 1) / p.chunk);
  if (p.seg_rows > p.chunk) p.seg_rows = p.chunk;
  p.seg_rows = (p.seg_rows + 3) & ~(int64_t)3;
  p.table_bytes = p.lds_bytes = GroupDirectLds(s.nk, p.R, s.nv, s.mm);
  return p;
}

}  // namespace mbx
