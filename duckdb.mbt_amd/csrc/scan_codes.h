// scan_codes.h — the code image of a narrow-range integer table column:
// code[i] = (uintW)(value[i] - imin), W = 1 or 2 bytes, chosen from the
// column's zone map.  The fused filter-aggregate (kernels.hip) streams the
// image instead of the 4- or 8-byte values; the values buffer stays the
// column's truth.  This header holds the planning: the width choice, the
// translation of a predicate range into a code range, and the packed compare
// (several codes per 32-bit word) that the kernels use when every code of the
// column is below half its width's range.
// No HIP types: the planning also builds in a plain host program.  All range
// arithmetic is in __int128 or unsigned, so bases at INT64_MIN / INT64_MAX
// cannot overflow.
#pragma once
#include <stdint.h>

#include "phys.h"

#if defined(__HIPCC__)
#define MBX_SC_HD __host__ __device__ __forceinline__
#else
#define MBX_SC_HD inline
#endif

namespace mbx {

// Code width in bytes of a column with the zone map [imin, imax], 0: no image.
// A code is at most a quarter of the physical width: 1 or 2 bytes for an
// 8-byte column, 1 byte for a 4-byte one.
inline int ScanCodeWidth(int phys, __int128 imin, __int128 imax) {
  if (phys != P_I32 && phys != P_I64) return 0;
  if (imax < imin || imin < (__int128)INT64_MIN || imax > (__int128)INT64_MAX) return 0;
  const unsigned __int128 range = (unsigned __int128)(imax - imin) + 1;  // distinct values the map admits
  if (range <= 256) return 1;
  if (phys == P_I64 && range <= 65536) return 2;
  return 0;
}

struct ScanCodeRange {
  bool empty;      // no value of the zone map passes: nothing to launch
  uint32_t clo;    // passing codes: clo <= code <= clo + cspan
  uint32_t cspan;
  bool packed;     // every code of the column is below 128 (W = 1) / 32768 (W = 2)
};

// The predicate lo <= value <= hi over a column coded with base imin and width
// `width` (ScanCodeWidth of the same zone map), clamped to the zone map.
inline ScanCodeRange PlanScanCodeRange(int width, __int128 imin, __int128 imax, int64_t lo, int64_t hi) {
  ScanCodeRange r = {true, 0, 0, false};
  if (lo > hi || (__int128)hi < imin || (__int128)lo > imax) return r;
  const __int128 l = (__int128)lo > imin ? (__int128)lo : imin;
  const __int128 h = (__int128)hi < imax ? (__int128)hi : imax;
  r.empty = false;
  r.clo = (uint32_t)(unsigned __int128)(l - imin);
  r.cspan = (uint32_t)(unsigned __int128)(h - l);
  const unsigned __int128 top = (unsigned __int128)(imax - imin);  // the largest code
  r.packed = top < (width == 1 ? 128u : 32768u);
  return r;
}

// ---- packed compare.  With every code c of a 32-bit word below H / 1 (the
// top bit of its field clear), (c + A) has the field's top bit set exactly
// when c >= clo for A = top - clo, and (B - c) has it set exactly when
// c <= chi for B = top + chi; neither carries nor borrows across fields
// (c + A <= 2 top - 1, B - c >= 1).  The mask's set bits count the passing
// codes of the word.
MBX_SC_HD uint32_t ScanPackedTop(int width) { return width == 1 ? 0x80808080u : 0x80008000u; }
MBX_SC_HD uint32_t ScanPackedA(int width, uint32_t clo) {
  return width == 1 ? (0x80u - clo) * 0x01010101u : (0x8000u - clo) * 0x00010001u;
}
MBX_SC_HD uint32_t ScanPackedB(int width, uint32_t chi) {
  return width == 1 ? (0x80u + chi) * 0x01010101u : (0x8000u + chi) * 0x00010001u;
}
// top bit of every field of w whose code lies in [clo, chi]
MBX_SC_HD uint32_t ScanPackedMask(uint32_t w, uint32_t A, uint32_t B, uint32_t H) { return (w + A) & (B - w) & H; }

}  // namespace mbx
