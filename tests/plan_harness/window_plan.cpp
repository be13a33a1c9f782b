// Stand-alone host check of csrc/window_plan.h (tests/test_window_plan.py
// builds and runs it): the frame resolution on every (function, ORDER BY,
// frame) combination, the grouping of calls by specification, and the
// segmented operator of every state kind.  Its argument is a file the test
// writes: N elements (segment flag, NULL flag, an int64, a double, a 128-bit
// value) and beside each the running values computed in Python.  Every kind
// is folded four ways -- a left fold, a right-nested fold
// x0 (+) (x1 (+) (... (+) xi)), and the three-launch tile scan with tiles of 7
// and of 256 -- and each must give exactly those running values, element by
// element.  Prints "window plan: ok" or the first failed check.
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "window_plan.h"

using namespace mbx;

#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
      exit(1);                                                \
    }                                                         \
  } while (0)

static void Frames() {
  // aggregates: [has ORDER BY][frame as written]
  static const WinTarget want[2][WFS_NSPECS] = {
      // none         ROWS..CURRENT  RANGE..CURRENT  ROWS..UNBOUNDED  RANGE..UNBOUNDED
      {WT_PART_END, WT_SELF, WT_PART_END, WT_PART_END, WT_PART_END},
      {WT_PEER_END, WT_SELF, WT_PEER_END, WT_PART_END, WT_PART_END},
  };
  int seen = 0;
  for (int k = 0; k < W_NKINDS; k++)
    for (int ob = 0; ob < 2; ob++)
      for (int f = 0; f < WFS_NSPECS; f++) {
        const bool agg = k == W_COUNT_STAR || k == W_COUNT || k == W_SUM || k == W_MIN || k == W_MAX || k == W_AVG;
        CHECK(WinIsAggregate((WinKind)k) == agg);
        const WinTarget t = WinResolveFrame((WinKind)k, ob != 0, (WinFrameSpec)f);
        CHECK(t == (agg ? want[ob][f] : WT_SELF));  // the ranks, LAG and LEAD ignore the frame
        seen++;
      }
  CHECK(seen == 11 * 2 * 5);
  CHECK(strstr(WinTargetName(WT_SELF), "ROWS") && strstr(WinTargetName(WT_PEER_END), "RANGE") &&
        strstr(WinTargetName(WT_PART_END), "WHOLE"));
}

static void Specs() {
  const int key[] = {3, 1, 3, 2, 1, 3};
  int spec[6];
  CHECK(WinGroupSpecs(6, [&](int a, int b) { return key[a] == key[b]; }, spec) == 3);
  const int want[] = {0, 1, 0, 2, 1, 0};
  for (int i = 0; i < 6; i++) CHECK(spec[i] == want[i]);
  CHECK(WinGroupSpecs(0, [](int, int) { return true; }, spec) == 0);
  CHECK(WinGroupSpecs(3, [](int, int) { return false; }, spec) == 3 && spec[2] == 2);
  CHECK(WinGroupSpecs(3, [](int, int) { return true; }, spec) == 1 && spec[2] == 0);
  // tiles
  CHECK(kWinTile == kWinBlock * kWinItems && WinTiles(0) == 0 && WinTiles(1) == 1 && WinTiles(kWinTile) == 1 &&
        WinTiles(kWinTile + 1) == 2);
}

struct Row {
  uint32_t flag, valid;
  int64_t v;
  double d;
  uint64_t hlo;
  int64_t hhi;
  // the running values
  uint64_t cnt, slo;
  int64_t shi;
  uint64_t fbits, mn64, mx64, mn128lo;
  int64_t mn128hi;
  uint64_t mx128lo;
  int64_t mx128hi, pos;
};

// folds xs four ways; same(i, state) compares with the expected running value
template <typename Op, typename Same>
static void FourWays(const std::vector<WinElem<Op>> &xs, Same same) {
  const int64_t n = (int64_t)xs.size();
  {  // left fold
    WinElem<Op> r = WinIdentity<Op>();
    for (int64_t i = 0; i < n; i++) {
      WinCombine<Op>(r, xs[i]);
      CHECK(same(i, r.s));
      CHECK(r.flag == 1u);  // element 0 is flagged
    }
  }
  for (int64_t i = 0; i < n; i++) {  // right-nested
    WinElem<Op> r = xs[i];
    for (int64_t j = i - 1; j >= 0; j--) {
      WinElem<Op> l = xs[j];
      WinCombine<Op>(l, r);
      r = l;
    }
    CHECK(same(i, r.s));
  }
  for (int64_t tile : {(int64_t)7, (int64_t)256}) {
    std::vector<WinElem<Op>> x = xs, carry((size_t)WinTiles(n, tile));
    WinTileScan<Op>(x.data(), n, tile, carry.data());
    for (int64_t i = 0; i < n; i++) CHECK(same(i, x[i].s));
  }
}

int main(int argc, char **argv) {
  Frames();
  Specs();
  CHECK(argc == 2);
  FILE *f = fopen(argv[1], "r");
  CHECK(f);
  long n = 0;
  CHECK(fscanf(f, "%ld", &n) == 1 && n > 0);
  std::vector<Row> rows((size_t)n);
  for (Row &r : rows) {
    uint64_t dbits;
    CHECK(fscanf(f, "%u %u %" SCNd64 " %" SCNu64 " %" SCNu64 " %" SCNd64 " %" SCNu64 " %" SCNu64 " %" SCNd64 " %" SCNu64
                    " %" SCNu64 " %" SCNu64 " %" SCNu64 " %" SCNd64 " %" SCNu64 " %" SCNd64 " %" SCNd64,
                 &r.flag, &r.valid, &r.v, &dbits, &r.hlo, &r.hhi, &r.cnt, &r.slo, &r.shi, &r.fbits, &r.mn64, &r.mx64,
                 &r.mn128lo, &r.mn128hi, &r.mx128lo, &r.mx128hi, &r.pos) == 17);
    memcpy(&r.d, &dbits, 8);
  }
  fclose(f);
  CHECK(rows[0].flag == 1);

  std::vector<WinElem<WinCount>> xc;
  std::vector<WinElem<WinPosMin>> xp;
  std::vector<WinElem<WinSum128>> xs;
  std::vector<WinElem<WinSumF>> xf;
  std::vector<WinElem<WinMinMax64<false>>> xmn;
  std::vector<WinElem<WinMinMax64<true>>> xmx;
  std::vector<WinElem<WinMinMax128<false>>> xmn8;
  std::vector<WinElem<WinMinMax128<true>>> xmx8;
  for (long i = 0; i < n; i++) {
    const Row &r = rows[(size_t)i];
    const uint64_t key = (uint64_t)r.v ^ 0x8000000000000000ull;
    xc.push_back({r.flag, r.valid ? 1u : 0u});
    xp.push_back({r.flag, (int64_t)i});
    xs.push_back({r.flag, r.valid ? WinSum128::Of(r.v, r.v >> 63) : WinSum128::Identity()});
    xf.push_back({r.flag, r.valid ? WinSumF::Of(r.d) : WinSumF::Identity()});
    xmn.push_back({r.flag, r.valid ? WinMinMax64<false>::Of(key) : WinMinMax64<false>::Identity()});
    xmx.push_back({r.flag, r.valid ? WinMinMax64<true>::Of(key) : WinMinMax64<true>::Identity()});
    xmn8.push_back({r.flag, r.valid ? WinMinMax128<false>::Of((int64_t)r.hlo, r.hhi) : WinMinMax128<false>::Identity()});
    xmx8.push_back({r.flag, r.valid ? WinMinMax128<true>::Of((int64_t)r.hlo, r.hhi) : WinMinMax128<true>::Identity()});
  }
  FourWays<WinCount>(xc, [&](int64_t i, uint64_t s) { return s == rows[i].cnt; });
  FourWays<WinPosMin>(xp, [&](int64_t i, int64_t s) { return s == rows[i].pos; });
  FourWays<WinSum128>(xs, [&](int64_t i, const WinSum128::State &s) {
    return s.count == rows[i].cnt && s.lo == rows[i].slo && s.hi == rows[i].shi;
  });
  FourWays<WinSumF>(xf, [&](int64_t i, const WinSumF::State &s) {
    uint64_t b;
    memcpy(&b, &s.sum, 8);
    return s.count == rows[i].cnt && b == rows[i].fbits;
  });
  FourWays<WinMinMax64<false>>(xmn, [&](int64_t i, const WinMinMax64<false>::State &s) {
    return s.count == rows[i].cnt && s.key == rows[i].mn64;
  });
  FourWays<WinMinMax64<true>>(xmx, [&](int64_t i, const WinMinMax64<true>::State &s) {
    return s.count == rows[i].cnt && s.key == rows[i].mx64;
  });
  FourWays<WinMinMax128<false>>(xmn8, [&](int64_t i, const WinMinMax128<false>::State &s) {
    return s.count == rows[i].cnt && s.lo == rows[i].mn128lo && s.hi == rows[i].mn128hi;
  });
  FourWays<WinMinMax128<true>>(xmx8, [&](int64_t i, const WinMinMax128<true>::State &s) {
    return s.count == rows[i].cnt && s.lo == rows[i].mx128lo && s.hi == rows[i].mx128hi;
  });
  printf("window plan: ok\n");
  return 0;
}
