// Stand-alone host check of the code histogram of csrc/scan_hist.h
// (tests/test_scan_hist_plan.py builds and runs it): the fold of the counters
// under a code range, and the values it stands for, against a loop over the
// rows the counters were counted from.  Prints "scan hist plan: ok" or the
// first failed check.
#include <cstdio>
#include <cstdlib>
#include <vector>

#include "scan_hist.h"

using namespace mbx;
typedef __int128 i128;
typedef unsigned __int128 u128;

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

// The rows of a column as the test knows them: `times` rows of code `code`
// (times is 1 wherever the rows can be written out; the columns of near 2^40
// rows cannot, and keep their rows as runs).
struct Run {
  uint32_t code;
  uint64_t times;
};
typedef std::vector<Run> Rows;

static std::vector<uint64_t> Count(const Rows &rows, int b) {
  std::vector<uint64_t> h((size_t)ScanHistBins(b), 0);
  for (const Run &r : rows) {
    CHECK(r.code < h.size());
    h[r.code] += r.times;
  }
  return h;
}

static const i128 kBases[] = {(i128)INT64_MIN, (i128)INT64_MAX - 255, 0};

// the fold and its values over [clo, chi] against the loop over the rows
static void CheckRange(const Rows &rows, const std::vector<uint64_t> &h, int b, uint32_t clo, uint32_t chi) {
  uint64_t cnt = 0;
  u128 sum = 0;
  int mn = -1, mx = -1;
  for (const Run &r : rows) {
    if (r.code < clo || r.code > chi || r.times == 0) continue;
    cnt += r.times;
    sum += (u128)r.code * r.times;
    if (mn < 0 || (int)r.code < mn) mn = (int)r.code;
    if ((int)r.code > mx) mx = (int)r.code;
  }
  const ScanHistFold f = ScanHistFoldRange(h.data(), b, clo, chi);
  CHECK(f.cnt == cnt);
  CHECK((u128)f.sum == sum);
  CHECK(f.mx == mx);
  CHECK(cnt == 0 ? f.mn == INT32_MAX : f.mn == mn);
  for (i128 base : kBases) {
    const ScanHistValues v = ScanHistValuesOf(f, (int64_t)base);
    const i128 want = (i128)sum + (i128)cnt * base;  // |.| < 2^40 x 2^63 + 2^48
    CHECK(v.cnt == cnt);
    CHECK(v.slo == (uint64_t)want && v.shi == (int64_t)(want >> 64));
    CHECK(v.mn == (cnt ? (int64_t)(base + mn) : INT64_MAX));
    CHECK(v.mx == (cnt ? (int64_t)(base + mx) : INT64_MIN));
  }
}

// the histograms of a column of b-bit codes whose largest code is `top`
static std::vector<Rows> Columns(int b, uint32_t top) {
  std::vector<Rows> cols;
  cols.push_back(Rows());  // no row: every counter zero
  cols.push_back(Rows(7, Run{top, 1}));  // one code only
  Rows once;
  for (uint32_t c = 0; c <= top; c++) once.push_back(Run{c, 1});
  cols.push_back(once);
  Rows rnd;  // seeded random, the largest code among them
  for (int i = 0; i < 40; i++) rnd.push_back(Run{Rand() % (top + 1), 1});
  rnd.push_back(Run{top, 1});
  cols.push_back(rnd);
  // near 2^40 rows: all in one code, and spread over every code
  const uint64_t n = ((uint64_t)1 << 40) - 1;
  cols.push_back(Rows(1, Run{top, n}));
  Rows spread;
  for (uint32_t c = 0; c <= top; c++) spread.push_back(Run{c, n / (top + 1) + (c == 0 ? n % (top + 1) : 0)});
  cols.push_back(spread);
  (void)b;
  return cols;
}

static void Folds() {
  for (int b = 1; b <= 8; b++)
    for (uint32_t top = b == 1 ? 0 : 1u << (b - 1); top < (1u << b); top++) {
      CHECK(ScanPlaneBits(P_I64, 0, top) == b || (b == 1 && top == 0));
      for (const Rows &rows : Columns(b, top)) {
        const std::vector<uint64_t> h = Count(rows, b);
        CHECK((int64_t)h.size() == ScanHistBins(b) && ScanHistBytes(b) == (int64_t)h.size() * 8);
        for (uint32_t clo = 0; clo <= top; clo++)
          for (uint32_t chi = clo; chi <= top; chi++) CheckRange(rows, h, b, clo, chi);
      }
    }
}

// Through the plan: the predicate lo <= value <= hi over values base + code,
// with the range PlanScanPlanes gives, against the loop over the values.
static void Predicates() {
  for (int b = 1; b <= 8; b++)
    for (uint32_t top : {b == 1 ? 0u : 1u << (b - 1), (1u << b) - 1u})
      for (i128 base : kBases) {
        const i128 imin = base, imax = base + top;
        Rows rows;
        for (int i = 0; i < 64; i++) rows.push_back(Run{Rand() % (top + 1), 1});
        rows.push_back(Run{0, 1});
        rows.push_back(Run{top, 1});
        const std::vector<uint64_t> h = Count(rows, b);
        std::vector<int64_t> bounds = {INT64_MIN, INT64_MAX, 0, -1, 1};
        for (i128 d = -2; d <= (i128)top + 2; d++)
          if (base + d >= (i128)INT64_MIN && base + d <= (i128)INT64_MAX) bounds.push_back((int64_t)(base + d));
        for (int64_t lo : bounds)
          for (int64_t hi : bounds)
            for (bool values : {false, true}) {
              const ScanPlanePlan pp = PlanScanPlanes(b, imin, imax, lo, hi, values);
              uint64_t cnt = 0;
              i128 sum = 0, mn = 0, mx = 0;
              for (const Run &r : rows) {
                const i128 v = base + r.code;
                if (v < (i128)lo || v > (i128)hi) continue;
                if (!cnt || v < mn) mn = v;
                if (!cnt || v > mx) mx = v;
                cnt++;
                sum += v;
              }
              if (pp.empty) {
                CHECK(cnt == 0);
                continue;
              }
              const ScanHistValues v = ScanHistValuesOf(ScanHistFoldRange(h.data(), b, pp.clo, pp.chi), (int64_t)base);
              CHECK(v.cnt == cnt);
              CHECK(v.slo == (uint64_t)sum && v.shi == (int64_t)(sum >> 64));
              CHECK(v.mn == (cnt ? (int64_t)mn : INT64_MAX) && v.mx == (cnt ? (int64_t)mx : INT64_MIN));
              if (pp.planes == 0) CHECK(cnt == rows.size());  // every row passes: the count is known
            }
      }
}

int main() {
  Folds();
  Predicates();
  printf("scan hist plan: ok\n");
  return 0;
}
