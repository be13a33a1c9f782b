// Stand-alone host check of csrc/scan_codes.h (tests/test_scan_codes_plan.py
// builds and runs it): the code width of a zone map, the translation of a
// predicate range into a code range against a brute-force loop over every
// value of small zone maps, and the packed compare against the per-element
// compare.  Prints "scan codes plan: ok" or the first failed check.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "scan_codes.h"

using namespace mbx;
typedef __int128 i128;

#define CHECK(c)                                                \
  do {                                                          \
    if (!(c)) {                                                 \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);   \
      exit(1);                                                  \
    }                                                           \
  } while (0)

// width of a zone map holding `range` distinct values, at several bases
static void Widths() {
  const i128 bases[] = {0, -100, (i128)INT64_MIN, 1000000007};
  struct {
    i128 range;
    int w64, w32;
  } cases[] = {{1, 1, 1}, {128, 1, 1}, {129, 1, 1}, {256, 1, 1}, {257, 2, 0}, {65536, 2, 0}, {65537, 0, 0}};
  for (i128 b : bases)
    for (auto &c : cases) {
      CHECK(ScanCodeWidth(P_I64, b, b + c.range - 1) == c.w64);
      // an INT32 column's values fit int32; its width never exceeds 1
      const i128 b32 = b < (i128)INT32_MIN ? (i128)INT32_MIN : b;
      CHECK(ScanCodeWidth(P_I32, b32, b32 + c.range - 1) == c.w32);
      // the top of the int64 range
      CHECK(ScanCodeWidth(P_I64, (i128)INT64_MAX - (c.range - 1), (i128)INT64_MAX) == c.w64);
    }
  CHECK(ScanCodeWidth(P_I64, (i128)INT64_MIN, (i128)INT64_MAX) == 0);
  CHECK(ScanCodeWidth(P_I64, 5, 4) == 0);                              // empty zone map
  CHECK(ScanCodeWidth(P_I64, (i128)INT64_MIN - 1, (i128)INT64_MIN) == 0);  // outside int64
  CHECK(ScanCodeWidth(P_I64, (i128)INT64_MAX, (i128)INT64_MAX + 1) == 0);
  CHECK(ScanCodeWidth(P_F64, 0, 10) == 0);
  CHECK(ScanCodeWidth(P_STR, 0, 10) == 0);
}

// every value v of [imin, imax]: lo <= v <= hi exactly when its code lies in
// the planned code range; the plan is `empty` exactly when no value passes
static void Translate(i128 imin, i128 imax) {
  const int w = ScanCodeWidth(P_I64, imin, imax);
  CHECK(w == 1 || w == 2);
  std::vector<int64_t> pts = {INT64_MIN, INT64_MIN + 1, -1, 0, 1, INT64_MAX - 1, INT64_MAX};
  for (i128 d = -3; d <= 3; d++)
    for (i128 at : {imin, imax, (imin + imax) / 2}) {
      const i128 p = at + d;
      if (p >= (i128)INT64_MIN && p <= (i128)INT64_MAX) pts.push_back((int64_t)p);
    }
  for (int64_t lo : pts)
    for (int64_t hi : pts) {
      const ScanCodeRange r = PlanScanCodeRange(w, imin, imax, lo, hi);
      int64_t pass = 0;
      for (i128 v = imin; v <= imax; v++) {
        const bool want = (i128)lo <= v && v <= (i128)hi;
        pass += want;
        if (r.empty) {
          CHECK(!want);
          continue;
        }
        const uint32_t code = (uint32_t)(unsigned __int128)(v - imin);
        const bool got = code - r.clo <= r.cspan;
        CHECK(got == want);
      }
      CHECK(r.empty == (pass == 0));
      if (!r.empty) {
        CHECK((i128)r.clo + r.cspan <= imax - imin);  // clamped to the zone map
        CHECK(r.packed == (imax - imin < (w == 1 ? 128 : 32768)));
      }
    }
}

static void Translations() {
  const i128 bases[] = {(i128)INT64_MIN, (i128)INT64_MAX - 49, 0, -100, -25};
  for (i128 b : bases) {
    Translate(b, b + 49);
    Translate(b, b);  // a constant column
  }
  Translate(-100, 100);                         // W = 1, codes above 127
  Translate(0, 255);
  Translate(100, 5000);                         // W = 2
  Translate((i128)INT64_MAX - 65535, (i128)INT64_MAX);  // W = 2, full code range at the top
  Translate((i128)INT64_MIN, (i128)INT64_MIN + 300);
  // lo > hi is empty whatever the map
  CHECK(PlanScanCodeRange(1, 0, 49, 10, 9).empty);
}

// the packed mask of a word of codes against the per-element compare
static void PackedWord(int w, const uint32_t *codes, uint32_t clo, uint32_t chi) {
  const int cpw = 4 / w, bits = 8 * w;
  uint32_t word = 0, want = 0;
  for (int e = 0; e < cpw; e++) {
    word |= codes[e] << (bits * e);
    if (codes[e] >= clo && codes[e] <= chi) want |= 1u << (bits * e + bits - 1);
  }
  const uint32_t got = ScanPackedMask(word, ScanPackedA(w, clo), ScanPackedB(w, chi), ScanPackedTop(w));
  CHECK(got == want);
}

static void Packed() {
  // 8-bit: every clo <= chi below 128, every code in every byte position, the
  // other bytes at the extremes that could carry or borrow into it
  for (uint32_t clo = 0; clo < 128; clo++)
    for (uint32_t chi = clo; chi < 128; chi++)
      for (uint32_t c = 0; c < 128; c++)
        for (uint32_t other : {0u, 127u}) {
          for (int pos = 0; pos < 4; pos++) {
            uint32_t codes[4] = {other, other, other, other};
            codes[pos] = c;
            PackedWord(1, codes, clo, chi);
          }
        }
  // 16-bit: a sample of ranges and codes below 32768, both positions
  const uint32_t pts[] = {0, 1, 2, 99, 127, 128, 255, 256, 4900, 16383, 16384, 32766, 32767};
  for (uint32_t clo : pts)
    for (uint32_t chi : pts) {
      if (chi < clo) continue;
      for (uint32_t c : pts)
        for (uint32_t d = 0; d < 3; d++)
          for (uint32_t other : {0u, 32767u}) {
            const uint32_t cc = c + d > 32767 ? 32767 : c + d;
            uint32_t a[2] = {cc, other}, b[2] = {other, cc};
            PackedWord(2, a, clo, chi);
            PackedWord(2, b, clo, chi);
          }
    }
  uint32_t seed = 12345;
  for (int it = 0; it < 200000; it++) {
    auto next = [&]() { return (seed = seed * 1664525u + 1013904223u) >> 17; };  // 15 bits
    uint32_t clo = next(), chi = next(), codes[2] = {next(), next()};
    if (chi < clo) {
      const uint32_t t = clo;
      clo = chi;
      chi = t;
    }
    PackedWord(2, codes, clo, chi);
  }
}

int main() {
  Widths();
  Translations();
  Packed();
  printf("scan codes plan: ok\n");
  return 0;
}
