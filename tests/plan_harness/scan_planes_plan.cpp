// Stand-alone host check of the bit-plane code images of csrc/scan_planes.h
// (tests/test_scan_planes_plan.py builds and runs it): the layout of rows in
// plane words, pieces and segments, which planes the plan reads for a
// predicate, and the word-parallel compare, sum, min and max against a per-row
// loop.  Prints "scan planes plan: ok" or the first failed check.
#include <cstdio>
#include <cstdlib>
#include <set>
#include <vector>

#include "scan_planes.h"

using namespace mbx;
typedef __int128 i128;

#define CHECK(c)                                                \
  do {                                                          \
    if (!(c)) {                                                 \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c);   \
      exit(1);                                                  \
    }                                                           \
  } while (0)

static uint64_t g_seed = 0x9E3779B97F4A7C15ull;
static uint32_t Rand() {
  g_seed ^= g_seed << 13;
  g_seed ^= g_seed >> 7;
  g_seed ^= g_seed << 17;
  return (uint32_t)(g_seed >> 16);
}

static void Eligibility() {
  const i128 bases[] = {0, -100, (i128)INT64_MIN, 1000000007};
  for (i128 base : bases)
    for (int64_t range = 1; range <= 70000; range += range < 600 ? 1 : 997) {
      int b = 1;
      while (((range - 1) >> b) != 0) b++;
      const i128 lows[] = {base, (i128)INT64_MAX - (range - 1)};
      for (i128 lo : lows) CHECK(ScanPlaneBits(P_I64, lo, lo + range - 1) == (b <= 8 ? b : 0));
      const i128 b32 = base < (i128)INT32_MIN ? (i128)INT32_MIN : base;
      CHECK(ScanPlaneBits(P_I32, b32, b32 + range - 1) == (b <= 8 ? b : 0));
    }
  CHECK(ScanPlaneBits(P_I64, (i128)INT64_MIN, (i128)INT64_MAX) == 0);
  CHECK(ScanPlaneBits(P_I64, 5, 4) == 0);
  CHECK(ScanPlaneBits(P_F64, 0, 10) == 0);
}

// row -> word, bit and piece offset; buffer and reported bytes
static void Layout() {
  CHECK(kScanPlaneSegRows == (1 << 20) && kScanPlanePieceRows == 8192 && kScanPlaneBytes == 128 * 1024);
  const int64_t S = kScanPlaneSegRows;
  const int64_t rows[] = {0, 1, 31, 32, 33, 8191, 8192, 8193, 24 * 8192 + 7, S - 33, S - 1, S, S + 1, 2 * S + 8192 + 33,
                          999999999, ((int64_t)1 << 40) - 1};
  for (int b = 1; b <= 8; b++) {
    for (int64_t r : rows)
      for (int k = 0; k < b; k++) {
        const int64_t q = r / 8192;
        // the piece formula of the design, written out
        const int64_t piece = (((q >> 7) * b + k) * 128 + (q & 127)) * 1024;
        CHECK(ScanPlanePieceByte(b, k, q) == piece);
        // by segments: segment r / S, then plane position k, then the row's word within the segment's plane
        const int64_t byte = (r / S * b + k) * (S / 8) + (r % S) / 32 * 4;
        CHECK(ScanPlaneWord(b, k, r) * 4 == byte);
        CHECK(byte >= piece && byte < piece + 1024 && byte - piece == (r % 8192) / 32 * 4);
        CHECK(ScanPlaneBit(r) == (int)(r % 32));
        CHECK(byte + 4 <= ScanPlaneBufferBytes(b, r + 1));
      }
    // the planes a scan reads are one prefix of every segment; the rest is one run of (b - np) x 128 KiB
    for (int np = 1; np <= b; np++)
      for (int64_t q : {(int64_t)0, (int64_t)127, (int64_t)128, (int64_t)300}) {
        CHECK(ScanPlanePieceByte(b, np - 1, q) / kScanPlaneBytes % b == np - 1);
        CHECK(ScanPlanePieceByte(b, 0, q + 128) - ScanPlanePieceByte(b, 0, q) == b * kScanPlaneBytes);
      }
    const int64_t caps[] = {1, S - 1, S, S + 1, 5 * S, 1000000000};
    for (int64_t cap : caps) {
      CHECK(ScanPlaneBufferBytes(b, cap) == (cap + S - 1) / S * b * 128 * 1024);
      CHECK(ScanPlaneBufferBytes(b, cap) % 256 == 0);
    }
    for (int64_t n : rows)
      for (int np = 0; np <= b; np++) CHECK(ScanPlaneScanBytes(np, n) == np * 4 * ((n + 31) / 32));
  }
  CHECK(ScanPlaneScanBytes(3, 1000000000) == 375000000);
  // no two (row / 32, plane) pairs share a word, over three segments of 3 planes
  {
    std::set<int64_t> seen;
    for (int64_t r = 0; r < 3 * S; r += 32)
      for (int k = 0; k < 3; k++) CHECK(seen.insert(ScanPlaneWord(3, k, r)).second);
    CHECK(*seen.rbegin() * 4 + 4 == ScanPlaneBufferBytes(3, 3 * S));
  }
  for (int64_t n = 1; n <= 130; n++) {
    const uint32_t m = ScanPlaneLastWordMask(n);
    for (int r = 0; r < 32; r++) CHECK(((m >> r) & 1u) == ((n - 1) / 32 * 32 + r < n ? 1u : 0u));
  }
  // a code read back from a small image written bit by bit
  {
    const int b = 6;
    const int64_t n = S + 100;
    std::vector<uint32_t> img(ScanPlaneBufferBytes(b, n) / 4, 0u), codes(n);
    for (int64_t r = 0; r < n; r++) {
      codes[r] = Rand() % 50;
      for (int k = 0; k < b; k++)
        img[ScanPlaneWord(b, k, r)] |= ((codes[r] >> (b - 1 - k)) & 1u) << ScanPlaneBit(r);
    }
    for (int64_t r = 0; r < n; r += 7) CHECK(ScanPlaneCodeAt(img.data(), b, r) == codes[r]);
    CHECK(ScanPlaneCodeAt(img.data(), b, n - 1) == codes[n - 1]);
  }
}

// plane words of the 32 codes c0 .. c0 + 31: P[j] is plane j
static void CodeBlock(uint32_t c0, uint32_t P[8]) {
  for (int j = 0; j < 8; j++) {
    P[j] = 0;
    for (int r = 0; r < 32; r++) P[j] |= (((c0 + r) >> j) & 1u) << r;
  }
}

// bit r set: lo <= blk * 32 + r <= hi, by a loop over the 32 codes of the block
static uint32_t BlockRangeLoop(uint32_t blk, uint32_t lo, uint32_t hi) {
  uint32_t m = 0;
  for (int r = 0; r < 32; r++)
    if (blk * 32 + r >= lo && blk * 32 + r <= hi) m |= 1u << r;
  return m;
}
// the same from a table filled once by that loop: [blk][lo][hi] for codes below 256
static uint32_t BlockRange(uint32_t blk, uint32_t lo, uint32_t hi) {
  static std::vector<uint32_t> tab;
  if (tab.empty()) {
    tab.resize(8 * 256 * 256);
    for (uint32_t k = 0; k < 8; k++)
      for (uint32_t l = 0; l < 256; l++)
        for (uint32_t h = 0; h < 256; h++) tab[(k * 256 + l) * 256 + h] = BlockRangeLoop(k, l, h);
  }
  return tab[(blk * 256 + lo) * 256 + hi];
}

// The plan against the definition, for every b, every largest code `top` of
// that bit length and every clo <= chi <= top: with the planned-out planes
// removed (only planes b - 1 .. t go into the compares, and only the tested
// sides run), the answer over every code 0 .. top is that of clo <= c <= chi;
// and no skipped plane matters: flipping its bit in any code never changes
// whether the code passes.
static void Plan() {
  uint32_t blocks[8][8];
  for (int blk = 0; blk < 8; blk++) CodeBlock(blk * 32, blocks[blk]);
  const i128 imin = -17;
  for (int b = 1; b <= 8; b++)
    for (uint32_t top = b == 1 ? 0 : 1u << (b - 1); top < (1u << b); top++) {
      const i128 imax = imin + top;
      CHECK(ScanPlaneBits(P_I64, imin, imax) == b);
      for (uint32_t clo = 0; clo <= top; clo++)
        for (uint32_t chi = clo; chi <= top; chi++) {
          const ScanPlanePlan p = PlanScanPlanes(b, imin, imax, (int64_t)(imin + clo), (int64_t)(imin + chi), false);
          CHECK(!p.empty && p.clo == clo && p.chi == chi);
          CHECK(p.ge == (clo > 0) && p.le == (chi < top));
          int t = b;
          if (p.ge) t = ScanPlaneCtz(clo) < t ? ScanPlaneCtz(clo) : t;
          if (p.le) t = ScanPlaneCtz(chi + 1) < t ? ScanPlaneCtz(chi + 1) : t;
          CHECK(p.t == t && p.planes == b - t && t >= 0 && t <= b);
          CHECK((p.planes == 0) == (!p.ge && !p.le));
          const int np = p.planes;
          for (uint32_t blk = 0; blk * 32 <= top; blk++) {
            uint32_t w[8];
            for (int k = 0; k < np; k++) w[k] = blocks[blk][b - 1 - k];
            const uint32_t truth = BlockRange(blk, clo, chi), valid = BlockRange(blk, 0, top);
            uint32_t m = ~0u;
            if (p.ge) m &= ScanPlanesGe(w, np, clo >> t);
            if (p.le) m &= ScanPlanesLe(w, np, chi >> t);
            CHECK((m & valid) == truth);
          }
          for (int j = 0; j < t; j++)
            for (uint32_t c = 0; c <= top; c++) {
              const uint32_t d = c ^ (1u << j);
              if (d <= top) CHECK((c >= clo && c <= chi) == (d >= clo && d <= chi));
            }
        }
    }
  // values asked: all planes; clamping and empty ranges; bases at the ends of int64
  const i128 mins[] = {(i128)INT64_MIN, -3, (i128)INT64_MAX - 49};
  for (i128 lo : mins) {
    const i128 hi = lo + 49;
    const int64_t l64 = (int64_t)lo, h64 = (int64_t)hi;
    ScanPlanePlan p = PlanScanPlanes(6, lo, hi, l64 + 24, INT64_MAX, false);  // the C2 shape: code >= 24
    CHECK(!p.empty && p.clo == 24 && p.chi == 49 && p.ge && !p.le && p.t == 3 && p.planes == 3);
    p = PlanScanPlanes(6, lo, hi, l64 + 24, INT64_MAX, true);
    CHECK(!p.empty && p.t == 3 && p.planes == 6);
    p = PlanScanPlanes(6, lo, hi, INT64_MIN, INT64_MAX, false);
    CHECK(!p.empty && !p.ge && !p.le && p.planes == 0 && p.clo == 0 && p.chi == 49);
    p = PlanScanPlanes(6, lo, hi, INT64_MIN, INT64_MAX, true);
    CHECK(!p.empty && !p.ge && !p.le && p.planes == 6);
    p = PlanScanPlanes(6, lo, hi, l64 + 8, l64 + 39, false);  // two sides: ctz(8) = 3, ctz(40) = 3
    CHECK(p.ge && p.le && p.t == 3 && p.planes == 3);
    p = PlanScanPlanes(6, lo, hi, l64 + 23, INT64_MAX, false);
    CHECK(p.t == 0 && p.planes == 6);
    p = PlanScanPlanes(6, lo, hi, l64 + 16, INT64_MAX, false);
    CHECK(p.t == 4 && p.planes == 2);
    CHECK(PlanScanPlanes(6, lo, hi, l64 + 5, l64 + 4, false).empty);
    if (lo > (i128)INT64_MIN) CHECK(PlanScanPlanes(6, lo, hi, INT64_MIN, l64 - 1, false).empty);
    if (hi < (i128)INT64_MAX) CHECK(PlanScanPlanes(6, lo, hi, h64 + 1, INT64_MAX, false).empty);
  }
}

// one word of 32 codes through the primitives against a loop over its rows
static void CheckWord(int b, const uint32_t codes[32], uint32_t rows, uint32_t clo, uint32_t chi) {
  uint32_t w[8];
  for (int k = 0; k < b; k++) {
    w[k] = 0;
    for (int r = 0; r < 32; r++) w[k] |= ((codes[r] >> (b - 1 - k)) & 1u) << r;
  }
  uint32_t ge = 0, le = 0, sum = 0, mn = ~0u, mx = 0, cnt = 0;
  for (int r = 0; r < 32; r++) {
    if (codes[r] >= clo) ge |= 1u << r;
    if (codes[r] <= chi) le |= 1u << r;
    if (((rows >> r) & 1u) && codes[r] >= clo && codes[r] <= chi) {
      cnt++;
      sum += codes[r];
      mn = codes[r] < mn ? codes[r] : mn;
      mx = codes[r] > mx ? codes[r] : mx;
    }
  }
  CHECK(ScanPlanesGe(w, b, clo) == ge);
  CHECK(ScanPlanesLe(w, b, chi) == le);
  const uint32_t m = rows & ge & le;
  CHECK((uint32_t)__builtin_popcount(m) == cnt);
  CHECK(ScanPlanesSum(w, b, m) == sum);
  if (m) {
    CHECK(ScanPlanesMin(w, b, m) == mn);
    CHECK(ScanPlanesMax(w, b, m) == mx);
  }
  // a compare that leaves out the low s planes is the compare of the codes shifted by s
  for (int s = 1; s < b; s++) {
    uint32_t g2 = 0, l2 = 0;
    for (int r = 0; r < 32; r++) {
      if ((codes[r] >> s) >= (clo >> s)) g2 |= 1u << r;
      if ((codes[r] >> s) <= (chi >> s)) l2 |= 1u << r;
    }
    CHECK(ScanPlanesGe(w, b - s, clo >> s) == g2);
    CHECK(ScanPlanesLe(w, b - s, chi >> s) == l2);
  }
}

static void Primitives() {
  for (int b = 1; b <= 8; b++) {
    const uint32_t top = (1u << b) - 1u;
    // bounds: all of them up to 5 bits; above, a sample: the three lowest and highest, powers of
    // two, powers of two less one, multiples of 23 (Plan() runs every bound pair over every code)
    std::vector<uint32_t> ks;
    for (uint32_t k = 0; k <= top; k++)
      if (b <= 5 || k < 3 || k + 3 > top || (k & (k - 1)) == 0 || ((k + 1) & k) == 0 || k % 23 == 0) ks.push_back(k);
    // every code at every bit position of the word, against two bounds drawn from ks, against
    // itself as both bounds, and under every last-word mask
    for (int fill = 0; fill < 3; fill++)  // the rest of the word: 0, top, seeded random
      for (int pos = 0; pos < 32; pos++)
        for (uint32_t c = 0; c <= top; c++) {
          uint32_t codes[32];
          for (int r = 0; r < 32; r++) codes[r] = fill == 0 ? 0 : fill == 1 ? top : Rand() & top;
          codes[pos] = c;
          const uint32_t clo = ks[Rand() % ks.size()], chi = ks[Rand() % ks.size()];
          CheckWord(b, codes, ~0u, clo, chi);
          CheckWord(b, codes, ~0u, c, c);
          CheckWord(b, codes, ScanPlaneLastWordMask(pos + 1), clo < chi ? clo : chi, clo < chi ? chi : clo);
        }
    for (uint32_t clo : ks)
      for (uint32_t chi : ks) {
        uint32_t codes[32];
        for (int r = 0; r < 32; r++) codes[r] = Rand() & top;
        CheckWord(b, codes, ~0u, clo, chi);
        CheckWord(b, codes, Rand(), clo, chi);
        CheckWord(b, codes, ScanPlaneLastWordMask(1 + Rand() % 64), clo, chi);
      }
  }
}

int main() {
  Eligibility();
  Layout();
  Plan();
  Primitives();
  printf("scan planes plan: ok\n");
  return 0;
}
