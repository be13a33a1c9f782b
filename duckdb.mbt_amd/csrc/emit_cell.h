// emit_cell.h — how an aggregate's output cell is formed from its state, and
// how a cell is stored: the one definition the emit kernels (emit_cell in
// kernels.hip), the run-time compiled kernels, the host folder (binder.cpp) and
// the host answer of a histogram range aggregate (aggregate.cpp) all compile.
// A cell is the pair {lo, hi}: the value's low and high 64 bits, a double's
// bits in lo.  Here: store_phys, the correctly rounded int128 -> double, and
// the cells of the integer class (COUNT(*), COUNT, SUM, MIN / MAX of at most
// 64 bits, AVG with the DECIMAL scale of its argument); floating-point states
// and 128-bit MIN / MAX stay with emit_cell.
// AVG is sum / div in IEEE doubles after one exact rounding of the integer
// sum, and div is a product of exactly representable factors, so the host and
// the device give the same bits (tests/plan_harness/emit_cell.cpp holds the
// host to __int128 arithmetic written out, tests/test_gpu_scan_hist_host.py
// the two to each other).
// Like scan_hist.h this header has no HIP types.
#pragma once
#include <stdint.h>
#if !defined(__HIPCC_RTC__)
#include <math.h>
#endif

#include "phys.h"

#ifndef MBX_SC_HD
#if defined(__HIPCC__) || defined(__HIPCC_RTC__)
#define MBX_SC_HD __host__ __device__ __forceinline__
#else
#define MBX_SC_HD inline
#endif
#endif

namespace mbx {
namespace dev {

// the bits of a double and back (a bit cast every compiler here takes)
MBX_SC_HD int64_t f64_bits(double d) { return __builtin_bit_cast(int64_t, d); }
MBX_SC_HD double bits_f64(int64_t b) { return __builtin_bit_cast(double, b); }

MBX_SC_HD void store_phys(void *data, int phys, int64_t row, int64_t lo, int64_t hi) {
  switch (phys) {
    case P_U8: ((uint8_t *)data)[row] = (uint8_t)lo; break;
    case P_I8: ((int8_t *)data)[row] = (int8_t)lo; break;
    case P_I16: ((int16_t *)data)[row] = (int16_t)lo; break;
    case P_U16: ((uint16_t *)data)[row] = (uint16_t)lo; break;
    case P_I32: ((int32_t *)data)[row] = (int32_t)lo; break;
    case P_U32: ((uint32_t *)data)[row] = (uint32_t)lo; break;
    case P_I64: case P_U64: case P_F64: case P_STR: ((int64_t *)data)[row] = lo; break;
    case P_I128: {
      int64_t *p = (int64_t *)data + 2 * row;
      p[0] = lo;
      p[1] = hi;
      break;
    }
    case P_F32: ((float *)data)[row] = (float)bits_f64(lo); break;
    default: break;
  }
}

// int128 -> double through the magnitude, correctly rounded: the top 64
// significant bits with a sticky bit for the rest are rounded once, and the
// power-of-two scaling is exact.
MBX_SC_HD double u128_to_double(unsigned __int128 m) {
  uint64_t hi = (uint64_t)(m >> 64), lo = (uint64_t)m;
  if (hi == 0) return (double)lo;
  int sh = __builtin_clzll(hi);
  uint64_t top = sh ? (hi << sh) | (lo >> (64 - sh)) : hi;
  if (lo << sh) top |= 1;  // sticky bit: the discarded low bits only matter as "non-zero"
  return ldexp((double)top, 64 - sh);
}
MBX_SC_HD double i128_to_double(__int128 v) {
  if (v < 0) return -u128_to_double((unsigned __int128)0 - (unsigned __int128)v);
  return u128_to_double((unsigned __int128)v);
}

// The cell {lo, hi} of an aggregate of the integer class: kind is the AggKind
// (0 COUNT(*), 1 COUNT, 2 SUM, 3 MIN, 4 MAX, 5 AVG), cstar the slot's rows
// (COUNT(*) only), *S the state (count, sum_lo / sum_hi the int128 sum, min_i,
// max_i; not read for COUNT(*)), avg_scale the DECIMAL scale of AVG's
// argument.  false: the cell is NULL (and {0, 0}).
template <class State>
MBX_SC_HD bool emit_cell_int(int kind, int avg_scale, unsigned long long cstar, const State *S, int64_t &lo,
                             int64_t &hi) {
  lo = 0;
  hi = 0;
  switch (kind) {
    case 0: /*COUNT_STAR*/ lo = (int64_t)cstar; return true;
    case 1: /*COUNT*/ lo = (int64_t)S->count; return true;
    case 2: /*SUM*/
      if (!S->count) return false;
      lo = (int64_t)S->sum_lo;
      hi = S->sum_hi;
      return true;
    case 3: /*MIN*/
    case 4: /*MAX*/
      if (!S->count) return false;
      lo = kind == 3 ? S->min_i : S->max_i;
      hi = lo >> 63;
      return true;
    default: /*AVG*/ {
      if (!S->count) return false;
      const double sum =
          i128_to_double((__int128)(((unsigned __int128)(uint64_t)S->sum_hi << 64) | (uint64_t)S->sum_lo));
      double div = (double)S->count;
      for (int k = 0; k < avg_scale; k++) div *= 10.0;
      lo = f64_bits(sum / div);
      return true;
    }
  }
}

}  // namespace dev
}  // namespace mbx
