// scan_hist.h — the code histogram of a column that keeps a bit-plane image
// (scan_planes.h): 1 << b counters of uint64_t, b = code_planes, counter c the
// number of rows in [0, code_rows) whose code value - code_base is c.  One per
// column, over all its rows.  Ingest counts the codes while it builds the
// planes (scan_encode_planes, kernels.hip), so the histogram lives and dies
// with the image.  For the queries the plane scan serves (a range on the column,
// aggregates over the same column, all its rows) COUNT, SUM, MIN and MAX are
// exact functions of the counters, and the fold below answers them from at most
// 2 KiB in place of a pass over the planes.
// The range [clo, chi] is PlanScanPlanes's; nothing here derives it again.
// Like scan_planes.h this header has no HIP types: the kernel and the host
// test run the same functions.
#pragma once
#include <stdint.h>

#include "scan_planes.h"

namespace mbx {

// counters, and bytes, of the histogram of b-bit codes
MBX_SC_HD int64_t ScanHistBins(int b) { return (int64_t)1 << b; }
MBX_SC_HD int64_t ScanHistBytes(int b) { return ScanHistBins(b) * 8; }

// What the counters of some codes in range add up to: their rows, the sum of
// their codes (rows < 2^40 and codes <= 255: below 2^48), and the smallest and
// largest code that has a row (mx < 0: none has).
struct ScanHistFold {
  uint64_t cnt, sum;
  int32_t mn, mx;
};
MBX_SC_HD ScanHistFold ScanHistNone() { return ScanHistFold{0, 0, INT32_MAX, -1}; }
// counter h of code c under the range clo <= c <= chi
MBX_SC_HD ScanHistFold ScanHistBin(uint32_t c, uint64_t h, uint32_t clo, uint32_t chi) {
  if (c < clo || c > chi || h == 0) return ScanHistNone();
  return ScanHistFold{h, (uint64_t)c * h, (int32_t)c, (int32_t)c};
}
MBX_SC_HD ScanHistFold ScanHistMerge(const ScanHistFold &a, const ScanHistFold &b) {
  return ScanHistFold{a.cnt + b.cnt, a.sum + b.sum, a.mn < b.mn ? a.mn : b.mn, a.mx > b.mx ? a.mx : b.mx};
}
// the whole fold, one counter of the range after another (the kernel gives
// thread c counter c and merges through its block reduction instead)
MBX_SC_HD ScanHistFold ScanHistFoldRange(const uint64_t *h, int b, uint32_t clo, uint32_t chi) {
  ScanHistFold f = ScanHistNone();
  for (uint32_t c = clo; c <= chi && c < (uint32_t)ScanHistBins(b); c++)
    f = ScanHistMerge(f, ScanHistBin(c, h[c], clo, chi));
  return f;
}

// The fold in values: the count, SUM = sum of codes + count x base in int128
// (as filter_agg_planes forms it once per lane), MIN and MAX = base + code, or
// INT64_MAX / INT64_MIN where no row passes.
struct ScanHistValues {
  uint64_t cnt, slo;
  int64_t shi, mn, mx;
};
MBX_SC_HD ScanHistValues ScanHistValuesOf(const ScanHistFold &f, int64_t base) {
  const __int128 s = (__int128)(unsigned __int128)f.sum + (__int128)(unsigned __int128)f.cnt * (__int128)base;
  ScanHistValues v;
  v.cnt = f.cnt;
  v.slo = (uint64_t)s;
  v.shi = (int64_t)(s >> 64);
  v.mn = f.mx >= 0 ? (int64_t)((uint64_t)base + (uint64_t)f.mn) : INT64_MAX;
  v.mx = f.mx >= 0 ? (int64_t)((uint64_t)base + (uint64_t)f.mx) : INT64_MIN;
  return v;
}

}  // namespace mbx
