// Stand-alone host check of csrc/emit_cell.h (tests/test_emit_cell_host.py
// builds and runs it): the cell every aggregate kind forms from an integer
// state, against __int128 arithmetic written out here; the correctly rounded
// int128 -> double against values whose double is known and against a
// round-to-nearest-even done by hand; and the path of the histogram's host
// answer, fold -> values -> cells -> the result buffer's layout, against a byte
// buffer of which nothing but the cells and the validity words may change.
// Prints "emit cell: ok" or the first failed check.
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "emit_cell.h"
#include "result_tail.h"
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

struct State {
  unsigned long long count, sum_lo;
  long long sum_hi, min_i, max_i;
};

static int64_t Bits(double d) {
  int64_t b;
  memcpy(&b, &d, 8);
  return b;
}

// round to nearest, ties to even, by hand: the 53 leading bits, then the rest
// against half a unit in the last place
static double RefU128ToDouble(u128 m) {
  int len = 0;
  while (len < 128 && (m >> len) != 0) len++;
  if (len <= 53) return (double)(uint64_t)m;
  const int sh = len - 53;
  uint64_t q = (uint64_t)(m >> sh);
  const u128 rem = m & (((u128)1 << sh) - 1), half = (u128)1 << (sh - 1);
  if (rem > half || (rem == half && (q & 1))) q++;
  return std::ldexp((double)q, sh);  // (q <= 2^53: exact)
}
static double RefI128ToDouble(i128 v) { return v < 0 ? -RefU128ToDouble((u128)0 - (u128)v) : RefU128ToDouble((u128)v); }

static State StateOf(uint64_t count, i128 sum, int64_t mn, int64_t mx) {
  State s;
  s.count = count;
  s.sum_lo = (uint64_t)(u128)sum;
  s.sum_hi = (int64_t)(sum >> 64);
  s.min_i = mn;
  s.max_i = mx;
  return s;
}

// every kind's cell from (count, sum, mn, mx) against the arithmetic written out
static void CheckCells(uint64_t cstar, uint64_t count, i128 sum, int64_t mn, int64_t mx, int scale) {
  const State s = StateOf(count, sum, mn, mx);
  for (int kind = 0; kind <= 5; kind++) {
    int64_t lo = 0x5555, hi = 0x5555;
    const bool valid = dev::emit_cell_int(kind, scale, cstar, kind == 0 ? (const State *)nullptr : &s, lo, hi);
    bool ev = true;
    int64_t elo = 0, ehi = 0;
    switch (kind) {
      case 0: elo = (int64_t)cstar; break;
      case 1: elo = (int64_t)count; break;
      case 2:
        ev = count > 0;
        if (ev) {
          elo = (int64_t)(uint64_t)(u128)sum;
          ehi = (int64_t)(uint64_t)((u128)sum >> 64);
        }
        break;
      case 3:
      case 4:
        ev = count > 0;
        if (ev) {
          elo = kind == 3 ? mn : mx;
          ehi = elo < 0 ? -1 : 0;
        }
        break;
      default:
        ev = count > 0;
        if (ev) {
          double div = (double)count;  // the definition: the count, times ten `scale` times
          for (int k = 0; k < scale; k++) div *= 10.0;
          elo = Bits(RefI128ToDouble(sum) / div);
        }
        break;
    }
    CHECK(valid == ev);
    CHECK(lo == elo);
    CHECK(hi == ehi);
  }
}

static void CheckToDouble() {
  const u128 p53 = (u128)1 << 53, p64 = (u128)1 << 64, p11 = (u128)1 << 11;
  struct {
    u128 m;
    double d;
  } known[] = {
      {0, 0.0},
      {1, 1.0},
      {p53, 9007199254740992.0},
      {p53 + 1, 9007199254740992.0},  // a tie: to even
      {p53 + 2, 9007199254740994.0},
      {p53 + 3, 9007199254740996.0},  // a tie: to even, upwards
      {(u128)UINT64_MAX, 18446744073709551616.0},
      {p64, std::ldexp(1.0, 64)},
      {p64 + p11 - 1, std::ldexp(1.0, 64)},
      {p64 + p11, std::ldexp(1.0, 64)},  // a tie: the even neighbour is below
      {p64 + p11 + 1, std::ldexp(1.0, 64) + std::ldexp(1.0, 12)},
      {p64 + 3 * p11 - 1, std::ldexp(1.0, 64) + std::ldexp(1.0, 12)},
      {p64 + 3 * p11, std::ldexp(1.0, 64) + std::ldexp(1.0, 13)},  // a tie: the even neighbour is above
      {p64 + 3 * p11 + 1, std::ldexp(1.0, 64) + std::ldexp(1.0, 13)},
      {((u128)1 << 103) - 1, std::ldexp(1.0, 103)},
      {((u128)1 << 127) - 1, std::ldexp(1.0, 127)},
  };
  for (auto &k : known) {
    CHECK(Bits(dev::u128_to_double(k.m)) == Bits(k.d));
    CHECK(Bits(RefU128ToDouble(k.m)) == Bits(k.d));
    if (k.m <= (((u128)1 << 127) - 1)) {
      CHECK(Bits(dev::i128_to_double((i128)k.m)) == Bits(k.d));
      if (k.m) CHECK(Bits(dev::i128_to_double(-(i128)k.m)) == Bits(-k.d));
    }
  }
  CHECK(Bits(dev::i128_to_double((i128)((u128)1 << 127))) == Bits(-std::ldexp(1.0, 127)));  // INT128_MIN
  // around every power of two and every half-way point above 2^53, against the hand rounding
  for (int e = 53; e < 127; e++)
    for (int lowbit = 0; lowbit < e - 52 + 1 && lowbit < 70; lowbit++)
      for (int d = -1; d <= 1; d++) {
        const u128 m = ((u128)1 << e) + ((u128)3 << lowbit) + (u128)(i128)d;
        CHECK(Bits(dev::u128_to_double(m)) == Bits(RefU128ToDouble(m)));
        CHECK(Bits(dev::i128_to_double(-(i128)m)) == Bits(-RefU128ToDouble(m)));
      }
}

static void CheckStore() {
  // store_phys writes the cell's own bytes and no other
  const int phys[] = {P_U8, P_I8, P_I16, P_U16, P_I32, P_U32, P_I64, P_U64, P_I128, P_F32, P_F64};
  const int size[] = {1, 1, 2, 2, 4, 4, 8, 8, 16, 4, 8};
  for (size_t i = 0; i < sizeof(phys) / sizeof(phys[0]); i++) {
    alignas(16) uint8_t buf[64];
    memset(buf, 0xAB, sizeof(buf));
    const double dv = -2.5;
    const int64_t lo = phys[i] == P_F32 || phys[i] == P_F64 ? Bits(dv) : (int64_t)0x8877665544332211ll, hi = -2;
    dev::store_phys(buf, phys[i], 1, lo, hi);
    for (int b = 0; b < 64; b++)
      if (b < size[i] || b >= 2 * size[i]) CHECK(buf[b] == 0xAB);
    uint8_t exp[16];
    if (phys[i] == P_F32) {
      const float f = (float)dv;
      memcpy(exp, &f, 4);
    } else {
      memcpy(exp, &lo, 8);
      memcpy(exp + 8, &hi, 8);
    }
    CHECK(memcmp(buf + size[i], exp, (size_t)size[i]) == 0);
  }
}

// fold -> values -> cells -> the result buffer, as the host answer goes: ncols
// aggregates (kind j % 6) over the codes of [clo, chi] of a b-bit histogram
static void CheckRow(int ncols, int b, i128 base, uint32_t clo, uint32_t chi, int scale) {
  std::vector<uint64_t> h((size_t)ScanHistBins(b));
  uint64_t cnt = 0;
  i128 sum = 0;
  int mn = -1, mx = -1;
  for (uint32_t c = 0; c < h.size(); c++) {
    h[c] = c % 3 == 1 ? 0 : (uint64_t)c * 1000003ull + 1;
    if (c < clo || c > chi || !h[c]) continue;
    cnt += h[c];
    sum += ((i128)c + base) * (i128)h[c];
    if (mn < 0) mn = (int)c;
    mx = (int)c;
  }
  const ScanHistValues v = ScanHistValuesOf(ScanHistFoldRange(h.data(), b, clo, chi), (int64_t)base);
  State s;
  s.count = v.cnt;
  s.sum_lo = v.slo;
  s.sum_hi = v.shi;
  s.min_i = v.mn;
  s.max_i = v.mx;
  const int kind_phys[6] = {P_I64, P_I64, P_I128, P_I64, P_I64, P_F64};
  const int kind_size[6] = {8, 8, 16, 8, 8, 8};
  int cell[8];
  bool has_valid[8];
  ResultColLayout off[8];
  for (int j = 0; j < ncols; j++) {
    cell[j] = kind_size[j % 6];
    has_valid[j] = true;
  }
  const size_t need = ResultBufferLayout((size_t)ncols, cell, has_valid, 1, 1, false, off);
  std::vector<uint8_t> buf(need + 64, 0xCD), touched(need + 64, 0);
  for (int j = 0; j < ncols; j++) {
    int64_t lo, hi;
    const bool valid = dev::emit_cell_int(j % 6, scale, s.count, &s, lo, hi);
    CHECK(off[j].data_off >= 64 && off[j].data_off + (size_t)cell[j] <= need);
    CHECK(off[j].valid_off >= 64 && off[j].valid_off + 8 <= need);
    dev::store_phys(buf.data() + off[j].data_off, kind_phys[j % 6], 0, lo, hi);
    const uint64_t vw = valid ? 1 : 0;
    memcpy(buf.data() + off[j].valid_off, &vw, 8);
    // what the arithmetic written out says
    uint8_t exp[16] = {0};
    bool ev = true;
    switch (j % 6) {
      case 0:
      case 1: memcpy(exp, &cnt, 8); break;
      case 2:
        ev = cnt > 0;
        if (ev) memcpy(exp, &sum, 16);
        break;
      case 3:
      case 4: {
        ev = cnt > 0;
        const int64_t m = (int64_t)(base + (j % 6 == 3 ? mn : mx));
        if (ev) memcpy(exp, &m, 8);
        break;
      }
      default: {
        ev = cnt > 0;
        double div = (double)cnt;
        for (int k = 0; k < scale; k++) div *= 10.0;
        const double a = RefI128ToDouble(sum) / div;
        if (ev) memcpy(exp, &a, 8);
        break;
      }
    }
    CHECK(vw == (ev ? 1u : 0u));
    CHECK(memcmp(buf.data() + off[j].data_off, exp, (size_t)cell[j]) == 0);
    for (int k = 0; k < cell[j]; k++) touched[off[j].data_off + (size_t)k]++;
    for (int k = 0; k < 8; k++) touched[off[j].valid_off + (size_t)k]++;
  }
  for (size_t i = 0; i < buf.size(); i++) {
    CHECK(touched[i] <= 1);  // no two pieces overlap
    if (!touched[i]) CHECK(buf[i] == 0xCD);
  }
}

int main() {
  CheckToDouble();
  CheckStore();
  const i128 p63 = (i128)1 << 63, p64 = (i128)1 << 64, p103m = ((i128)1 << 103) - 1;
  const i128 sums[] = {0, 1, -1, 12345, p63, -p63, p63 - 1, p64, -p64, p64 + 1, p103m, -p103m, p103m - 1};
  const uint64_t counts[] = {0, 1, 3, 1000003, ((uint64_t)1 << 40) - 1};
  const int scales[] = {0, 2, 18};
  const i128 bases[] = {(i128)INT64_MIN, 0, (i128)INT64_MAX - 255};
  for (i128 sum : sums)
    for (uint64_t count : counts)
      for (int scale : scales)
        for (i128 base : bases) {
          // MIN / MAX as the fold gives them: base + code, or the identities where no row passed
          const int64_t mn = count ? (int64_t)base : INT64_MAX, mx = count ? (int64_t)(base + 255) : INT64_MIN;
          CheckCells(count, count, sum, mn, mx, scale);
          CheckCells(count + 7, count, sum, mn, mx, scale);  // (COUNT(*) reads cstar, COUNT the state)
        }
  for (int ncols : {1, 6})
    for (int b : {1, 6, 8})
      for (i128 base : bases)
        for (int scale : scales) {
          const uint32_t top = (uint32_t)ScanHistBins(b) - 1;
          CheckRow(ncols, b, base, 0, top, scale);
          CheckRow(ncols, b, base, top, top, scale);
          CheckRow(ncols, b, base, 1, 1, scale);  // a code no row has: NULL for all but the counts
          if (b > 1) CheckRow(ncols, b, base, 2, top - 1, scale);
        }
  printf("emit cell: ok\n");
  return 0;
}
