// scan_codes.h — the code image of a narrow-range integer table column:
// code[i] = value[i] - imin, packed F to a 32-bit word in fields of
// Bf = 32 / F bits (code i lives in word i / F at bit (i mod F) * Bf; the bits
// above F * Bf and the fields of rows past the end are zero).  F follows from
// the bit length of the zone map's span; F = 4 and F = 2 are the plain 1- and
// 2-byte images.  The fused filter-aggregate (kernels.hip) streams the image
// instead of the 4- or 8-byte values; the values buffer stays the column's
// truth.  This header holds the planning: the field choice, the layout, the
// translation of a predicate range into a code range, and the word-parallel
// compares that the kernels run on whole 32-bit words.
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

// Fields per 32-bit word for the same zone map, 0: no image.  b = bit length
// of imax - imin picks the most fields whose width holds b bits: 32, 16, 10, 8,
// 6, 5 fields for b = 1..6, 4 for 7-8, 3 for 9-10, 2 for 11-16.  Without
// `bit_fields` (a table below the connection's mbx_scan_codes_bits_min_rows)
// a field is a whole byte or two: 4 or 2 fields.
inline int ScanCodeFields(int phys, __int128 imin, __int128 imax, bool bit_fields) {
  const int w = ScanCodeWidth(phys, imin, imax);
  if (!w || !bit_fields) return w ? 4 / w : 0;
  const uint32_t top = (uint32_t)(unsigned __int128)(imax - imin);  // below 65536
  int b = 1;
  while ((top >> b) != 0) b++;
  return b <= 2 ? 32 / b : b == 3 ? 10 : b == 4 ? 8 : b == 5 ? 6 : b == 6 ? 5 : b <= 8 ? 4 : b <= 10 ? 3 : 2;
}

// ---- layout
MBX_SC_HD constexpr int ScanFieldBits(int fields) { return 32 / fields; }
MBX_SC_HD constexpr uint32_t ScanFieldMax(int fields) { return fields == 1 ? ~0u : (1u << (32 / fields)) - 1u; }
MBX_SC_HD int64_t ScanCodeWord(int fields, int64_t row) { return row / fields; }
MBX_SC_HD int ScanCodeShift(int fields, int64_t row) { return (int)(row % fields) * ScanFieldBits(fields); }
MBX_SC_HD int64_t ScanCodeWords(int fields, int64_t rows) { return (rows + fields - 1) / fields; }
MBX_SC_HD constexpr int64_t ScanPieceRows(int fields) { return 256 * (int64_t)fields; }  // a 1-KiB ring piece
MBX_SC_HD uint32_t ScanCodeAt(const uint32_t *words, int fields, int64_t row) {
  return (words[ScanCodeWord(fields, row)] >> ScanCodeShift(fields, row)) & ScanFieldMax(fields);
}
// Bytes of the image of `rows` rows as the profile reports them: the words'
// bytes; a 1- or 2-byte image is counted by its codes, rows x 1 or rows x 2.
inline int64_t ScanCodeBytes(int fields, int64_t rows) {
  return fields == 4 || fields == 2 ? rows * (4 / fields) : 4 * ScanCodeWords(fields, rows);
}

// ---- which compare a scan runs on the words of an image
enum ScanCompare {
  SC_PER_CODE = 0,  // extract every field: always valid (MIN / MAX use it)
  SC_GUARD,         // ScanPackedMask: the largest code is below 2^(Bf-1), so every field has a spare top bit
  SC_GE,            // ScanFieldsGe alone: the clamped range reaches the largest code
  SC_LE,            // ScanFieldsLe alone: the clamped range starts at code 0
  SC_BOTH,          // ScanFieldsGe & ScanFieldsLe
};

struct ScanCodeRange {
  bool empty;      // no value of the zone map passes: nothing to launch
  uint32_t clo;    // passing codes: clo <= code <= clo + cspan
  uint32_t cspan;
  bool packed;     // every code of the column is below half its field's range (form == SC_GUARD)
  int form;        // the cheapest word-parallel ScanCompare that is valid
};

// The predicate lo <= value <= hi over a column coded with base imin in
// `fields` fields per word (ScanCodeFields of the same zone map), clamped to
// the zone map.
inline ScanCodeRange PlanScanFieldRange(int fields, __int128 imin, __int128 imax, int64_t lo, int64_t hi) {
  ScanCodeRange r = {true, 0, 0, false, SC_PER_CODE};
  if (lo > hi || (__int128)hi < imin || (__int128)lo > imax) return r;
  const __int128 l = (__int128)lo > imin ? (__int128)lo : imin;
  const __int128 h = (__int128)hi < imax ? (__int128)hi : imax;
  r.empty = false;
  r.clo = (uint32_t)(unsigned __int128)(l - imin);
  r.cspan = (uint32_t)(unsigned __int128)(h - l);
  const unsigned __int128 top = (unsigned __int128)(imax - imin);  // the largest code
  r.packed = top < ((unsigned __int128)1 << (ScanFieldBits(fields) - 1));
  r.form = r.packed ? SC_GUARD : h == imax ? SC_GE : l == imin ? SC_LE : SC_BOTH;
  return r;
}
// the same by the byte width of a 1- or 2-byte image
inline ScanCodeRange PlanScanCodeRange(int width, __int128 imin, __int128 imax, int64_t lo, int64_t hi) {
  return PlanScanFieldRange(4 / width, imin, imax, lo, hi);
}

// ---- per-field constants of a word: v in every one of the F fields, the
// fields' top bits, and the fields' bits below the top
MBX_SC_HD constexpr uint32_t ScanFieldRep(int fields, uint32_t v) {
  uint32_t r = 0;
  for (int e = 0; e < fields; e++) r |= v << (e * (32 / fields));
  return r;
}
MBX_SC_HD constexpr uint32_t ScanFieldTop(int fields) { return ScanFieldRep(fields, 1u << (32 / fields - 1)); }
MBX_SC_HD constexpr uint32_t ScanFieldLow(int fields) { return ScanFieldRep(fields, (1u << (32 / fields - 1)) - 1u); }

// ---- guard compare.  With every code c of a 32-bit word below H / 1 (the
// top bit of its field clear), (c + A) has the field's top bit set exactly
// when c >= clo for A = top - clo, and (B - c) has it set exactly when
// c <= chi for B = top + chi; neither carries nor borrows across fields
// (c + A <= 2 top - 1, B - c >= 1).  The mask's set bits count the passing
// codes of the word.
MBX_SC_HD uint32_t ScanGuardA(int fields, uint32_t clo) { return ScanFieldRep(fields, (1u << (32 / fields - 1)) - clo); }
MBX_SC_HD uint32_t ScanGuardB(int fields, uint32_t chi) { return ScanFieldRep(fields, (1u << (32 / fields - 1)) + chi); }
MBX_SC_HD uint32_t ScanPackedTop(int width) { return ScanFieldTop(4 / width); }
MBX_SC_HD uint32_t ScanPackedA(int width, uint32_t clo) { return ScanGuardA(4 / width, clo); }
MBX_SC_HD uint32_t ScanPackedB(int width, uint32_t chi) { return ScanGuardB(4 / width, chi); }
// top bit of every field of w whose code lies in [clo, chi]
MBX_SC_HD uint32_t ScanPackedMask(uint32_t w, uint32_t A, uint32_t B, uint32_t H) { return (w + A) & (B - w) & H; }

// ---- compares for fields with no spare bit (any code below 2^Bf).  A field
// is its top bit and its low part.  (w | H) - (k & L) sets each field's top
// bit, subtracts the low part of k from the low part of the code, and leaves
// the top bit standing exactly when low(c) >= low(k); no field borrows from
// its neighbour because every minuend field is at least 2^(Bf-1).  Then
// c >= k when top(c) > top(k), or the tops are equal and low(c) >= low(k):
// with a constant k that is (c | t) for top(k) = 0 and (c & t) for top(k) = 1,
// the bitwise majority of c, t and Z = ~0 / 0.  c <= k is the mirror image
// with ~c.  The constants are word-uniform; the result has exactly one bit,
// its field's top bit, per passing field, and none above the F-th field.
struct ScanFieldCmp {
  uint32_t kl;  // Ge: low parts of clo.         Le: H | low parts of chi
  uint32_t z;   // Ge: top(clo) ? 0 : ~0.         Le: top(chi) ? ~0 : 0
};
MBX_SC_HD ScanFieldCmp ScanFieldsGeK(int fields, uint32_t clo) {
  const uint32_t hb = 1u << (32 / fields - 1);
  return ScanFieldCmp{ScanFieldRep(fields, clo & (hb - 1u)), (clo & hb) ? 0u : ~0u};
}
MBX_SC_HD ScanFieldCmp ScanFieldsLeK(int fields, uint32_t chi) {
  const uint32_t hb = 1u << (32 / fields - 1);
  return ScanFieldCmp{ScanFieldRep(fields, hb | (chi & (hb - 1u))), (chi & hb) ? ~0u : 0u};
}
MBX_SC_HD uint32_t ScanMajority(uint32_t a, uint32_t b, uint32_t c) { return (a & b) | ((a | b) & c); }
// top bit of every field of w whose code is >= clo (H, L: ScanFieldTop / ScanFieldLow)
MBX_SC_HD uint32_t ScanFieldsGe(uint32_t w, ScanFieldCmp k, uint32_t H) {
  const uint32_t t = (w | H) - k.kl;
  return ScanMajority(w, t, k.z) & H;
}
// top bit of every field of w whose code is <= chi
MBX_SC_HD uint32_t ScanFieldsLe(uint32_t w, ScanFieldCmp k, uint32_t H, uint32_t L) {
  const uint32_t t = k.kl - (w & L);
  return ScanMajority(~w, t, k.z) & H;
}

// Everything a scan needs to compare the words of one image against
// [clo, chi], by any form.
struct ScanWordCmp {
  uint32_t H, L, A, B;
  ScanFieldCmp ge, le;
};
MBX_SC_HD ScanWordCmp ScanWordCmpOf(int fields, int form, uint32_t clo, uint32_t chi) {
  ScanWordCmp c;
  c.H = ScanFieldTop(fields);
  c.L = ScanFieldLow(fields);
  c.A = ScanGuardA(fields, form == SC_GUARD ? clo : 0);
  c.B = ScanGuardB(fields, form == SC_GUARD ? chi : 0);
  c.ge = ScanFieldsGeK(fields, clo);
  c.le = ScanFieldsLeK(fields, chi);
  return c;
}
// one bit, the field's top bit, per field of w whose code lies in [clo, chi]
MBX_SC_HD uint32_t ScanWordMask(int form, uint32_t w, const ScanWordCmp &c) {
  if (form == SC_GUARD) return ScanPackedMask(w, c.A, c.B, c.H);
  if (form == SC_GE) return ScanFieldsGe(w, c.ge, c.H);
  if (form == SC_LE) return ScanFieldsLe(w, c.le, c.H, c.L);
  return ScanFieldsGe(w, c.ge, c.H) & ScanFieldsLe(w, c.le, c.H, c.L);
}
// all bits of fields 0, 2, 4, ...
MBX_SC_HD constexpr uint32_t ScanEvenFields(int fields) {
  uint32_t r = 0;
  for (int e = 0; e < fields; e += 2) r |= ScanFieldMax(fields) << (e * (32 / fields));
  return r;
}
// a mask of top bits widened to the whole of each marked field
MBX_SC_HD uint32_t ScanFieldsOf(int fields, uint32_t m) {
  return (m >> (32 / fields - 1)) * ScanFieldMax(fields);
}

}  // namespace mbx
