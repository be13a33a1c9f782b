// Stand-alone host check of the bit-packed code images of csrc/scan_codes.h
// (tests/test_scan_codes_bits_plan.py builds and runs it): the field count of
// a zone map, the layout of codes in words, which compare the plan picks, and
// every word-parallel compare against a per-field loop.  Prints
// "scan codes bits plan: ok" or the first failed check.
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

static const int kFields[] = {32, 16, 10, 8, 6, 5, 4, 3, 2};

// fields per word of a zone map holding `range` distinct values
static void Widths() {
  const i128 bases[] = {0, -100, (i128)INT64_MIN, 1000000007};
  struct {
    i128 range;
    int f64, f32;  // with sub-byte fields allowed
  } cases[] = {{1, 32, 32},  {2, 32, 32},  {3, 16, 16}, {4, 16, 16}, {5, 10, 10},  {8, 10, 10},    {9, 8, 8},
               {16, 8, 8},   {17, 6, 6},   {32, 6, 6},  {33, 5, 5},  {64, 5, 5},   {65, 4, 4},     {128, 4, 4},
               {129, 4, 4},  {256, 4, 4},  {257, 3, 0}, {1024, 3, 0}, {1025, 2, 0}, {65536, 2, 0}, {65537, 0, 0}};
  for (i128 b : bases)
    for (auto &c : cases) {
      const i128 b32 = b < (i128)INT32_MIN ? (i128)INT32_MIN : b;
      const i128 tops[] = {b, (i128)INT64_MAX - (c.range - 1)};
      for (i128 lo : tops) {
        CHECK(ScanCodeFields(P_I64, lo, lo + c.range - 1, true) == c.f64);
        // below the floor a range that fits a byte keeps whole bytes
        CHECK(ScanCodeFields(P_I64, lo, lo + c.range - 1, false) == (c.f64 >= 4 ? 4 : c.f64 == 3 ? 2 : c.f64));
      }
      CHECK(ScanCodeFields(P_I32, b32, b32 + c.range - 1, true) == c.f32);
      CHECK(ScanCodeFields(P_I32, b32, b32 + c.range - 1, false) == (c.f32 >= 4 ? 4 : c.f32));
      // the byte view of the same map agrees
      const int w = ScanCodeWidth(P_I64, b, b + c.range - 1);
      CHECK(w == (c.f64 == 0 ? 0 : c.f64 <= 3 ? 2 : 1));
    }
  // the field holds the largest code, and is at most a quarter of the physical width
  for (i128 range = 1; range <= 65536; range++) {
    const int f = ScanCodeFields(P_I64, 7, 7 + range - 1, true), f32 = ScanCodeFields(P_I32, 7, 7 + range - 1, true);
    CHECK(f > 0 && (uint32_t)(range - 1) <= ScanFieldMax(f) && ScanFieldBits(f) <= 16);
    // ... and no larger field count would
    const int more = f == 2 ? 3 : f == 3 ? 4 : f == 4 ? 5 : f == 5 ? 6 : f == 6 ? 8 : f == 8 ? 10 : f == 10 ? 16 : 32;
    CHECK(f == 32 || (uint32_t)(range - 1) > ScanFieldMax(more));
    CHECK(f32 == (range <= 256 ? f : 0));
  }
  CHECK(ScanCodeFields(P_I64, (i128)INT64_MIN, (i128)INT64_MAX, true) == 0);
  CHECK(ScanCodeFields(P_I64, 5, 4, true) == 0);
  CHECK(ScanCodeFields(P_F64, 0, 10, true) == 0);
  CHECK(ScanCodeFields(P_STR, 0, 10, true) == 0);
}

static void Layout() {
  for (int f : kFields) {
    const int bf = ScanFieldBits(f);
    CHECK(bf == 32 / f && f * bf <= 32 && ScanFieldMax(f) == (1u << bf) - 1u);
    CHECK(ScanPieceRows(f) == 256 * f);  // 1 KiB of words; a lane's 16 bytes are 4 f rows
    CHECK(ScanCodeWords(f, 0) == 0);
    const int64_t rows[] = {1, f - 1, f, f + 1, 4 * f + 1, 256 * f - 1, 256 * f, 256 * f + 1, 2000003, ((int64_t)1 << 40) - 1};
    for (int64_t n : rows) {
      if (n <= 0) continue;
      CHECK(ScanCodeWords(f, n) == (n + f - 1) / f);
      CHECK(ScanCodeWord(f, n - 1) == ScanCodeWords(f, n) - 1);  // the last row lives in the last word
      CHECK(ScanCodeBytes(f, n) == (f == 4 ? n : f == 2 ? 2 * n : 4 * ScanCodeWords(f, n)));
    }
    // an image built field by field reads back, with the padding zero
    const int64_t n = 3 * f + 2;
    std::vector<uint32_t> img(ScanCodeWords(f, n), 0);
    uint32_t seed = 7u * f;
    std::vector<uint32_t> codes(n);
    for (int64_t i = 0; i < n; i++) {
      codes[i] = ((seed = seed * 1664525u + 1013904223u) >> 9) & ScanFieldMax(f);
      CHECK(ScanCodeWord(f, i) == i / f && ScanCodeShift(f, i) == (int)(i % f) * bf);
      CHECK(ScanCodeShift(f, i) + bf <= 32);
      img[ScanCodeWord(f, i)] |= codes[i] << ScanCodeShift(f, i);
    }
    for (int64_t i = 0; i < n; i++) CHECK(ScanCodeAt(img.data(), f, i) == codes[i]);
    if (f * bf < 32)
      for (uint32_t w : img) CHECK((w >> (f * bf)) == 0);
    // the constants of a word
    uint32_t top = 0, low = 0, even = 0;
    for (int e = 0; e < f; e++) {
      top |= 1u << (e * bf + bf - 1);
      low |= ((1u << (bf - 1)) - 1u) << (e * bf);
      if (e % 2 == 0) even |= ScanFieldMax(f) << (e * bf);
    }
    CHECK(ScanFieldTop(f) == top && ScanFieldLow(f) == low && ScanEvenFields(f) == even);
    if (f == 4 || f == 2) {  // the byte views
      CHECK(ScanPackedTop(4 / f) == top);
      CHECK(ScanPackedA(4 / f, 3) == ScanGuardA(f, 3) && ScanPackedB(4 / f, 3) == ScanGuardB(f, 3));
    }
  }
}

// which form the plan picks, and that the byte view plans the same
static void Forms() {
  for (int f : kFields) {
    const uint32_t max = ScanFieldMax(f), half = 1u << (ScanFieldBits(f) - 1);
    const uint32_t tops[] = {0, half - 1 < max ? half - 1 : 0, half <= max ? half : max, max};
    for (uint32_t top : tops)
      for (i128 base : {(i128)INT64_MIN, (i128)-25, (i128)INT64_MAX - top}) {
        const i128 imin = base, imax = base + top;
        for (i128 lo = imin - 2; lo <= imax + 2 && lo <= imin + 40; lo++)
          for (i128 hi = lo; hi <= imax + 2 && hi <= lo + 40; hi++) {
            if (lo < (i128)INT64_MIN || hi > (i128)INT64_MAX) continue;
            const ScanCodeRange r = PlanScanFieldRange(f, imin, imax, (int64_t)lo, (int64_t)hi);
            CHECK(r.empty == (hi < imin || lo > imax));
            if (r.empty) continue;
            const i128 l = lo > imin ? lo : imin, h = hi < imax ? hi : imax;
            CHECK(r.clo == (uint32_t)(l - imin) && r.cspan == (uint32_t)(h - l) && r.clo + r.cspan <= top);
            CHECK(r.packed == (top < half));
            CHECK(r.form == (top < half ? SC_GUARD : h == imax ? SC_GE : l == imin ? SC_LE : SC_BOTH));
            if (f == 4 || f == 2) {
              const ScanCodeRange b = PlanScanCodeRange(4 / f, imin, imax, (int64_t)lo, (int64_t)hi);
              CHECK(b.clo == r.clo && b.cspan == r.cspan && b.packed == r.packed && b.form == r.form);
            }
          }
      }
  }
}

static long g_words = 0;

// every valid form's mask of one word against a per-field loop: exactly the
// top bit of each passing field, so its popcount is the count and the fields
// it widens to select the sum
static void Word(int f, uint32_t top, uint32_t clo, uint32_t chi, uint32_t w) {
  const int bf = ScanFieldBits(f);
  uint32_t want = 0, cnt = 0, sum = 0;
  for (int e = 0; e < f; e++) {
    const uint32_t c = (w >> (e * bf)) & ScanFieldMax(f);
    if (c >= clo && c <= chi) want |= 1u << (e * bf + bf - 1), cnt++, sum += c;
  }
  int forms[4], nf = 0;
  forms[nf++] = SC_BOTH;
  if (top < (1u << (bf - 1))) forms[nf++] = SC_GUARD;
  if (chi == top) forms[nf++] = SC_GE;
  if (clo == 0) forms[nf++] = SC_LE;
  for (int i = 0; i < nf; i++) {
    const ScanWordCmp k = ScanWordCmpOf(f, forms[i], clo, chi);
    const uint32_t m = ScanWordMask(forms[i], w, k);
    CHECK(m == want);
    CHECK((uint32_t)__builtin_popcount(m) == cnt);
    const uint32_t sel = w & ScanFieldsOf(f, m);
    // the kernel's sum: even and odd fields in lanes of 2 bf bits
    const uint32_t ev = sel & ScanEvenFields(f), od = (sel >> bf) & ScanEvenFields(f);
    uint32_t s = 0;
    for (int e = 0; e < (f + 1) / 2; e++) {
      const uint32_t lane = 2 * bf >= 32 ? ~0u : (1u << (2 * bf)) - 1u;
      s += ((ev >> (2 * bf * e)) & lane) + ((od >> (2 * bf * e)) & lane);
    }
    CHECK(s == sum);
  }
  g_words++;
}

// the word patterns of one (f, top, clo, chi): each field position holding
// every code while the others hold 0, the largest code, and random codes (the
// rows past the end of a last word are zero fields: the `others = 0` pattern)
static void Patterns(int f, uint32_t top, uint32_t clo, uint32_t chi, const std::vector<uint32_t> &vals, uint32_t &seed) {
  const int bf = ScanFieldBits(f);
  auto rnd = [&]() { return (uint32_t)(((uint64_t)((seed = seed * 1664525u + 1013904223u) >> 8) * (top + 1)) >> 24); };
  for (int fill = 0; fill < 3; fill++) {
    uint32_t bg = 0;
    for (int e = 0; e < f; e++) bg |= (fill == 0 ? 0u : fill == 1 ? top : rnd()) << (e * bf);
    for (int pos = 0; pos < f; pos++)
      for (uint32_t c : vals) Word(f, top, clo, chi, (bg & ~(ScanFieldMax(f) << (pos * bf))) | (c << (pos * bf)));
  }
}

static void Compares() {
  uint32_t seed = 2024;
  // every largest code and every clo <= chi of the sub-byte fields
  for (int f : {32, 16, 10, 8, 6, 5}) {
    const uint32_t max = ScanFieldMax(f);
    for (uint32_t top = 0; top <= max; top++) {
      std::vector<uint32_t> vals;
      for (uint32_t c = 0; c <= top; c++) vals.push_back(c);
      for (uint32_t clo = 0; clo <= top; clo++)
        for (uint32_t chi = clo; chi <= top; chi++) {
          Patterns(f, top, clo, chi, vals, seed);
        }
    }
  }
  // bytes, 10 and 16 bits: a sample of largest codes, bounds and codes
  for (int f : {4, 3, 2}) {
    const uint32_t max = ScanFieldMax(f), half = (max + 1) / 2;
    const uint32_t tops[] = {0, 1, 49, half - 1, half, half + 1, max - 1, max};
    for (uint32_t top : tops) {
      std::vector<uint32_t> pts;
      for (uint32_t p : {0u, 1u, 2u, 24u, 49u, 99u, half - 2, half - 1, half, half + 1, top / 2, top - 1, top})
        if (p <= top) pts.push_back(p);  // top - 1 wraps above top at top = 0 and is dropped
      for (uint32_t clo : pts)
        for (uint32_t chi : pts)
          if (clo <= chi) Patterns(f, top, clo, chi, pts, seed);
    }
  }
  // random words, bounds and largest codes of every field width
  for (int f : kFields)
    for (int it = 0; it < 200000; it++) {
      auto next = [&]() { return seed = seed * 1664525u + 1013904223u; };
      const uint32_t top = (next() >> 7) & ScanFieldMax(f);
      uint32_t clo = (uint32_t)(((uint64_t)(next() >> 8) * (top + 1)) >> 24), chi = (uint32_t)(((uint64_t)(next() >> 8) * (top + 1)) >> 24);
      if (chi < clo) {
        const uint32_t t = clo;
        clo = chi;
        chi = t;
      }
      if (it & 1) chi = top;
      if (it & 2) clo = 0;
      uint32_t w = 0;
      for (int e = 0; e < f; e++) w |= (uint32_t)(((uint64_t)(next() >> 8) * (top + 1)) >> 24) << (e * ScanFieldBits(f));
      Word(f, top, clo, chi, w);
    }
}

int main() {
  Widths();
  Layout();
  Forms();
  Compares();
  printf("scan codes bits plan: ok (%ld words)\n", g_words);
  return 0;
}
