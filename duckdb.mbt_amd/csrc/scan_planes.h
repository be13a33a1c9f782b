// scan_planes.h — the bit-plane image of a narrow-range integer table column
// (BitWeaving/V): code[i] = value[i] - imin has b <= 8 bits, and bit j of every
// code is stored apart, in plane j.  A plane is 32-bit words: bit r mod 32 of
// word r / 32 is bit j of code r.  Rows are cut into segments of
// kScanPlaneSegRows = 2^20 rows; a segment holds its b planes one after
// another, most significant first (plane position k is plane b - 1 - k),
// 128 KiB each, and the buffer holds whole segments.  A range predicate needs
// only the planes down to the lowest set bit of its lower bound (the lowest
// clear bit of its upper bound): those are a prefix of every segment, and the
// fused filter-aggregate (kernels.hip) streams that prefix alone, in 1-KiB
// ring pieces of 8192 rows per plane.  The bits of rows past the end are zero
// up to the end of the word that holds the last row; beyond that word nothing
// is promised and no scan reads it.
// This header holds the planning: eligibility, the layout, which planes a
// predicate reads, and the word-parallel compare, sum, min and max that the
// kernels run on the words of the planes.  Like scan_codes.h it has no HIP
// types, and all range arithmetic is in __int128 or unsigned.
#pragma once
#include <stdint.h>

#include "scan_codes.h"

namespace mbx {

constexpr int kScanPlaneMaxBits = 8;                       // wider codes keep a field image
constexpr int64_t kScanPlaneSegRows = (int64_t)1 << 20;    // S: rows of a segment
constexpr int64_t kScanPlanePieceRows = 8192;              // rows of a 1-KiB ring piece of one plane
constexpr int64_t kScanPlaneSegPieces = kScanPlaneSegRows / kScanPlanePieceRows;  // 128
constexpr int64_t kScanPlaneBytes = kScanPlaneSegRows / 8;  // one plane of one segment: 128 KiB

// Bits per code, 1..8, of a column with the zone map [imin, imax]: the bit
// length of imax - imin, at least 1.  0: no plane image (the column has no code
// image at all, or its codes are wider than kScanPlaneMaxBits).
inline int ScanPlaneBits(int phys, __int128 imin, __int128 imax) {
  if (!ScanCodeWidth(phys, imin, imax)) return 0;
  const uint32_t top = (uint32_t)(unsigned __int128)(imax - imin);  // below 65536
  int b = 1;
  while ((top >> b) != 0) b++;
  return b <= kScanPlaneMaxBits ? b : 0;
}

// ---- layout
// byte at which the 1-KiB ring piece q of plane position k starts
MBX_SC_HD int64_t ScanPlanePieceByte(int b, int k, int64_t q) {
  return (((q >> 7) * b + k) * kScanPlaneSegPieces + (q & (kScanPlaneSegPieces - 1))) * 1024;
}
// index, in 32-bit words from the start of the buffer, of the word of plane
// position k that holds `row`, and the row's bit in it
MBX_SC_HD int64_t ScanPlaneWord(int b, int k, int64_t row) {
  return ScanPlanePieceByte(b, k, row / kScanPlanePieceRows) / 4 + (row % kScanPlanePieceRows) / 32;
}
MBX_SC_HD int ScanPlaneBit(int64_t row) { return (int)(row & 31); }
MBX_SC_HD int64_t ScanPlaneWords(int64_t rows) { return (rows + 31) / 32; }  // words of one plane that hold rows
// bytes of the buffer of a column with room for `cap` rows: whole segments
inline int64_t ScanPlaneBufferBytes(int b, int64_t cap) {
  return (cap + kScanPlaneSegRows - 1) / kScanPlaneSegRows * b * kScanPlaneBytes;
}
// bytes of a scan of `rows` rows over `planes_read` planes as the profile reports them
inline int64_t ScanPlaneScanBytes(int planes_read, int64_t rows) { return planes_read * 4 * ScanPlaneWords(rows); }
// code of `row`, gathered from the b planes
MBX_SC_HD uint32_t ScanPlaneCodeAt(const uint32_t *words, int b, int64_t row) {
  uint32_t c = 0;
  for (int k = 0; k < b; k++) c = (c << 1) | ((words[ScanPlaneWord(b, k, row)] >> ScanPlaneBit(row)) & 1u);
  return c;
}
// the rows of the word that holds row n - 1 (n > 0): all 32, or the n mod 32 below the end
MBX_SC_HD uint32_t ScanPlaneLastWordMask(int64_t n) { return (n & 31) ? (1u << (n & 31)) - 1u : ~0u; }

// ---- which planes a scan reads
struct ScanPlanePlan {
  bool empty;         // no value of the zone map passes: nothing to launch
  uint32_t clo, chi;  // passing codes: clo <= code <= chi
  bool ge, le;        // which sides are tested: clo > 0, chi < the largest code
  int t;              // the lowest plane a compare reads (b: no side is tested)
  int planes;         // planes read: positions 0 .. planes - 1
};
MBX_SC_HD int ScanPlaneCtz(uint32_t x) {  // x != 0
  int n = 0;
  while (!((x >> n) & 1u)) n++;
  return n;
}
// The predicate lo <= value <= hi over a column of b-bit codes with the zone
// map [imin, imax], clamped to the zone map.  c >= k does not depend on the
// bits below k's lowest set bit, c <= k not on those below k's lowest clear
// bit, so a COUNT(*) reads planes b - 1 .. t only; `values` (SUM, MIN or MAX
// of the passing values) reads all b.  planes == 0: every row passes and
// nothing but their number is asked.
inline ScanPlanePlan PlanScanPlanes(int b, __int128 imin, __int128 imax, int64_t lo, int64_t hi, bool values) {
  ScanPlanePlan r = {true, 0, 0, false, false, b, 0};
  if (lo > hi || (__int128)hi < imin || (__int128)lo > imax) return r;
  const __int128 l = (__int128)lo > imin ? (__int128)lo : imin;
  const __int128 h = (__int128)hi < imax ? (__int128)hi : imax;
  const uint32_t top = (uint32_t)(unsigned __int128)(imax - imin);  // the largest code
  r.empty = false;
  r.clo = (uint32_t)(unsigned __int128)(l - imin);
  r.chi = (uint32_t)(unsigned __int128)(h - imin);
  r.ge = r.clo > 0;
  r.le = r.chi < top;
  if (r.ge && ScanPlaneCtz(r.clo) < r.t) r.t = ScanPlaneCtz(r.clo);
  if (r.le && ScanPlaneCtz(r.chi + 1u) < r.t) r.t = ScanPlaneCtz(r.chi + 1u);
  r.planes = values ? b : b - r.t;
  return r;
}

// ---- word-parallel primitives.  p[0 .. np - 1] are the words of the np most
// significant planes at one word index, most significant first: 32 rows.  k is
// the bound's same np bits (the code bound shifted right by b - np).
// bit r set: code r >= k
MBX_SC_HD uint32_t ScanPlanesGe(const uint32_t *p, int np, uint32_t k) {
  uint32_t gt = 0, eq = ~0u;
  for (int i = 0; i < np; i++) {
    const uint32_t K = ((k >> (np - 1 - i)) & 1u) ? ~0u : 0u;
    gt |= eq & p[i] & ~K;
    eq &= ~(p[i] ^ K);
  }
  return gt | eq;
}
// bit r set: code r <= k
MBX_SC_HD uint32_t ScanPlanesLe(const uint32_t *p, int np, uint32_t k) {
  uint32_t lt = 0, eq = ~0u;
  for (int i = 0; i < np; i++) {
    const uint32_t K = ((k >> (np - 1 - i)) & 1u) ? ~0u : 0u;
    lt |= eq & ~p[i] & K;
    eq &= ~(p[i] ^ K);
  }
  return lt | eq;
}
// sum of the codes of the rows of m (p holds all np = b planes): at most 32 x 255
MBX_SC_HD uint32_t ScanPlanesSum(const uint32_t *p, int np, uint32_t m) {
  uint32_t s = 0;
  for (int i = 0; i < np; i++) s += (uint32_t)__builtin_popcount(p[i] & m) << (np - 1 - i);
  return s;
}
// largest / smallest code among the rows of m != 0: the candidates narrow from
// the top plane down, to those with the bit set (clear) wherever one has it
MBX_SC_HD uint32_t ScanPlanesMax(const uint32_t *p, int np, uint32_t m) {
  uint32_t v = 0;
  for (int i = 0; i < np; i++) {
    const uint32_t c = m & p[i];
    m = c ? c : m;
    v = (v << 1) | (c ? 1u : 0u);
  }
  return v;
}
MBX_SC_HD uint32_t ScanPlanesMin(const uint32_t *p, int np, uint32_t m) {
  uint32_t v = 0;
  for (int i = 0; i < np; i++) {
    const uint32_t c = m & ~p[i];
    m = c ? c : m;
    v = (v << 1) | (c ? 0u : 1u);
  }
  return v;
}

}  // namespace mbx
