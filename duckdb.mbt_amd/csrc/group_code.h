// group_code.h — the group code of a GROUP BY over 1..4 integer key columns:
// every key's zone map bounds a digit (value - min, or radix - 1 for NULL), and
// the digits fold, last key fastest, into one non-negative 64-bit code.  The
// partitioned GROUP BY (group_part.hip) computes the code in registers in its
// hist and scatter passes and the emit kernel decodes it back into the key
// columns (EmitDesc::kc carries the same kmin / radix / stride).
// No HIP types: the planning function also builds in a plain host program.
#pragma once
#include <stdint.h>

#include "phys.h"

#if defined(__HIPCC__)
#define MBX_GC_HD __host__ __device__ __forceinline__
#else
#define MBX_GC_HD inline
#endif

namespace mbx {

constexpr int kGroupCodeMaxKeys = 4;  // (EMIT_MAX_CKEYS)

struct GroupCodeKey {
  const void *data;
  const uint64_t *validity;  // bit r & 63 of word r >> 6; null when !nullable
  int32_t phys;              // P_I32 / P_I64
  int32_t nullable;
  int64_t kmin, radix, stride;
};

struct GroupCodePlan {
  int32_t nkeys;
  int64_t total;  // codes lie in [0, total), total < 2^62
  GroupCodeKey k[kGroupCodeMaxKeys];
};

// what the planner knows of one key column
struct GroupCodeKeyIn {
  const void *data;
  const uint64_t *validity;  // null: the column has no validity bitmap
  int phys;
  bool stats_valid;
  __int128 imin, imax;  // zone map of the non-NULL values
};

// false: the keys have no plan (not 1..4 plain P_I32 / P_I64 columns with zone
// maps, an empty zone map, or total >= 2^62)
inline bool PlanGroupCode(const GroupCodeKeyIn *in, int ng, GroupCodePlan *out) {
  if (ng < 1 || ng > kGroupCodeMaxKeys) return false;
  GroupCodePlan p = {};
  p.nkeys = ng;
  const __int128 limit = (__int128)1 << 62;
  __int128 total = 1;
  for (int i = 0; i < ng; i++) {
    const GroupCodeKeyIn &c = in[i];
    if ((c.phys != P_I32 && c.phys != P_I64) || !c.stats_valid || !c.data) return false;
    const __int128 radix = c.imax - c.imin + 1 + (c.validity ? 1 : 0);
    if (c.imax < c.imin || radix < 1 || radix >= limit) return false;
    if (c.imin < (__int128)INT64_MIN || c.imax > (__int128)INT64_MAX) return false;
    total *= radix;  // (< 2^124)
    if (total >= limit) return false;
    GroupCodeKey &k = p.k[i];
    k.data = c.data;
    k.validity = c.validity;
    k.phys = c.phys;
    k.nullable = c.validity ? 1 : 0;
    k.kmin = (int64_t)c.imin;
    k.radix = (int64_t)radix;
  }
  int64_t stride = 1;
  for (int i = ng - 1; i >= 0; i--) {  // last key fastest
    p.k[i].stride = stride;
    stride *= p.k[i].radix;
  }
  p.total = (int64_t)total;
  *out = p;
  return true;
}

// ---- reference restatements of the encode and decode, one row at a time.
// The kernels do not call these: the scatter folds eight rows column by column
// in 32- or 64-bit registers (PgCode::rows, group_part.hip) and the emit
// decodes from EmitDesc::kc (emit_agg_body, kernels.hip), each with this
// arithmetic.  The host test of the plan uses them to check that a plan's
// kmin / radix / stride round-trip; the kernels' own arithmetic is covered by
// the GPU tests.
// digit of one key value (valid = 0: the NULL digit)
MBX_GC_HD int64_t GroupCodeDigit(const GroupCodeKey &k, bool valid, int64_t v) {
  return valid ? (int64_t)((uint64_t)v - (uint64_t)k.kmin) : k.radix - 1;
}

// the code of one row's key values
MBX_GC_HD int64_t GroupCodeOf(const GroupCodePlan &p, const bool *valid, const int64_t *v) {
  int64_t code = 0;
  for (int q = 0; q < p.nkeys; q++) code += GroupCodeDigit(p.k[q], valid[q], v[q]) * p.k[q].stride;
  return code;
}

// key q of a code: *valid = false for the NULL digit, else *v = the key value
MBX_GC_HD void GroupCodeDecode(const GroupCodePlan &p, int64_t code, int q, bool *valid, int64_t *v) {
  const GroupCodeKey &k = p.k[q];
  const int64_t dg = (code / k.stride) % k.radix;
  *valid = !(k.nullable && dg == k.radix - 1);
  *v = *valid ? (int64_t)((uint64_t)k.kmin + (uint64_t)dg) : 0;
}

}  // namespace mbx
