// window_kernels.hip — window functions on the device (executor: window.cpp;
// the operator, the states and the scan's shape: window_plan.h).
//
//   window_bounds        sorted position i compares the key columns at perm[i]
//                        and perm[i - 1] through the sort's key encoding and
//                        writes two bits: a partition / a peer group starts here
//   window_scan_reduce   a segmented inclusive scan over the sorted positions in
//   window_scan_carry    three launches: every tile of kWinTile positions reduced
//   window_scan_apply    to its (flag, state) carry; one workgroup scans the
//                        carries, kWinCarryLanes at a time; every tile scanned
//                        again with what it receives.  No workgroup waits for
//                        another: no look-back, no grid barrier, no spin.
//   window_emit          per call: the value at the position its frame names,
//                        written with its validity bit at perm[i]
//
// A lane owns kWinItems consecutive positions; a tile is combined lane by lane
// in LDS (a Hillis-Steele scan of the lanes' totals), always in the same order,
// so a DOUBLE running sum depends on the row count alone.  Wave64.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <type_traits>

#include "device.h"
#include "phys.h"
#include "types.h"
#include "vm.h"
#include "vm_device.h"
#include "window_plan.h"

namespace mbx {
namespace dev {

namespace {

int RowGrid(int64_t n) {
  const int64_t want = (n + kWinBlock * 4 - 1) / (kWinBlock * 4);
  return (int)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)NumCUs() * 8));
}

// the key word ORDER BY sorts by (sort_key_kernel, before DESC's complement,
// which keeps equality): -0.0 = +0.0, every NaN one key
__device__ __forceinline__ uint64_t key_word(const void *data, int phys, int64_t r) {
  int64_t lo, hi;
  load_phys(data, phys, r, lo, hi);
  if (phys == P_F64 || phys == P_F32) {
    double d = __longlong_as_double(lo);
    if (d == 0) d = 0.0;
    return f64_order(d);
  }
  return (uint64_t)lo;
}

__global__ void __launch_bounds__(kWinBlock) window_bounds_kernel(WinKeys K, const int64_t *__restrict__ perm, int64_t n,
                                                                  uint8_t *__restrict__ flags) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    if (i == 0) {
      flags[0] = kWinPartStart | kWinPeerStart;
      continue;
    }
    const int64_t r1 = perm ? perm[i] : i, r0 = perm ? perm[i - 1] : i - 1;
    bool part = false, peer = false;
    for (int q = 0; q < K.nkeys; q++) {
      const bool v0 = bit_valid(K.k[q].valid, r0), v1 = bit_valid(K.k[q].valid, r1);
      bool diff = v0 != v1;
      if (v0 && v1) diff = key_word(K.k[q].data, K.k[q].phys, r0) != key_word(K.k[q].data, K.k[q].phys, r1);
      if (diff) {
        if (q < K.npart) part = true;
        peer = true;
      }
    }
    flags[i] = (uint8_t)((part ? kWinPartStart : 0) | ((part || peer) ? kWinPeerStart : 0));
  }
}

// ---- the scan --------------------------------------------------------------
// the element of logical position j (the scan's order); i is its place in memory
template <typename Op>
__device__ __forceinline__ WinElem<Op> load_elem(const WinScanDesc &D, int64_t j) {
  const int64_t i = D.backward ? D.n - 1 - j : j;
  WinElem<Op> x;
  if (j == 0) x.flag = 1u;
  else x.flag = (D.flags[D.backward ? i + 1 : i] & D.seg_bit) ? 1u : 0u;
  if constexpr (std::is_same<Op, WinPosMin>::value) {
    x.s = j;
  } else if constexpr (std::is_same<Op, WinCount>::value) {
    if (D.src == WSRC_PEER) {
      x.s = (D.flags[i] & kWinPeerStart) ? 1u : 0u;
    } else {
      x.s = bit_valid(D.valid, D.perm ? D.perm[i] : i) ? 1u : 0u;
    }
  } else {
    const int64_t r = D.perm ? D.perm[i] : i;
    if (!bit_valid(D.valid, r)) {
      x.s = Op::Identity();
    } else {
      int64_t lo, hi;
      load_phys(D.data, D.phys, r, lo, hi);
      if constexpr (std::is_same<Op, WinSumF>::value) {
        x.s = Op::Of(__longlong_as_double(lo));
      } else if constexpr (std::is_same<Op, WinMinMax64<false>>::value || std::is_same<Op, WinMinMax64<true>>::value) {
        uint64_t k;
        if (D.phys == P_F64 || D.phys == P_F32) k = f64_order(__longlong_as_double(lo));
        else if (D.phys == P_U8 || D.phys == P_U16 || D.phys == P_U32 || D.phys == P_U64) k = (uint64_t)lo;
        else k = (uint64_t)lo ^ 0x8000000000000000ull;
        x.s = Op::Of(k);
      } else {
        x.s = Op::Of(lo, hi);
      }
    }
  }
  return x;
}

template <typename Op>
__device__ __forceinline__ void store_elem(const WinScanDesc &D, int64_t j, const WinElem<Op> &x) {
  const int64_t i = D.backward ? D.n - 1 - j : j;
  if constexpr (std::is_same<Op, WinPosMin>::value) {
    ((int32_t *)D.out)[i] = (int32_t)(D.backward ? D.n - 1 - x.s : x.s);
  } else {
    ((typename Op::State *)D.out)[i] = x.s;
  }
}

// Inclusive scan of one element per lane over the workgroup, in LDS.  Returns
// the buffer that holds the result; every lane may read all of it.
template <typename Op>
__device__ __forceinline__ const WinElem<Op> *block_scan(WinElem<Op> (*buf)[kWinBlock], const WinElem<Op> &mine) {
  const int t = threadIdx.x;
  buf[0][t] = mine;
  __syncthreads();
  int cur = 0;
  for (int d = 1; d < kWinBlock; d <<= 1) {
    WinElem<Op> v = buf[cur][t];
    if (t >= d) {
      WinElem<Op> l = buf[cur][t - d];
      WinCombine<Op>(l, v);
      v = l;
    }
    buf[cur ^ 1][t] = v;
    __syncthreads();
    cur ^= 1;
  }
  return buf[cur];
}

// kReduce: only the tile's carry is written; else the tile is finished from the carry it receives
template <typename Op, bool kReduce>
__global__ void __launch_bounds__(kWinBlock) window_scan_tile_kernel(WinScanDesc D) {
  __shared__ WinElem<Op> buf[2][kWinBlock];
  const int64_t tile = blockIdx.x;
  const int64_t j0 = tile * kWinTile + (int64_t)threadIdx.x * kWinItems;
  WinElem<Op> e[kWinItems];
  WinElem<Op> acc = WinIdentity<Op>();
#pragma unroll
  for (int k = 0; k < kWinItems; k++) {
    e[k] = j0 + k < D.n ? load_elem<Op>(D, j0 + k) : WinIdentity<Op>();
    WinCombine<Op>(acc, e[k]);
  }
  const WinElem<Op> *sc = block_scan<Op>(buf, acc);
  if constexpr (kReduce) {
    if (threadIdx.x == kWinBlock - 1) ((WinElem<Op> *)D.carry)[tile] = sc[kWinBlock - 1];
  } else {
    WinElem<Op> run = ((const WinElem<Op> *)D.carry)[tile];
    if (threadIdx.x > 0) WinCombine<Op>(run, sc[threadIdx.x - 1]);
#pragma unroll
    for (int k = 0; k < kWinItems; k++) {
      if (j0 + k < D.n) {
        WinCombine<Op>(run, e[k]);
        store_elem<Op>(D, j0 + k, run);
      }
    }
  }
}

// carry[t] <- the combination of every tile before t; one workgroup, kWinCarryLanes tiles at a time
template <typename Op>
__global__ void __launch_bounds__(kWinCarryLanes) window_scan_carry_kernel(WinScanDesc D, int64_t ntiles) {
  static_assert(kWinCarryLanes == kWinBlock, "block_scan is sized by kWinBlock");
  __shared__ WinElem<Op> buf[2][kWinBlock];
  WinElem<Op> *carry = (WinElem<Op> *)D.carry;
  WinElem<Op> run = WinIdentity<Op>();
  for (int64_t base = 0; base < ntiles; base += kWinCarryLanes) {
    const int64_t t = base + threadIdx.x;
    const WinElem<Op> mine = t < ntiles ? carry[t] : WinIdentity<Op>();
    const WinElem<Op> *sc = block_scan<Op>(buf, mine);
    WinElem<Op> before = run;
    if (threadIdx.x > 0) WinCombine<Op>(before, sc[threadIdx.x - 1]);
    if (t < ntiles) carry[t] = before;
    WinCombine<Op>(run, sc[kWinBlock - 1]);
    __syncthreads();  // the next round rewrites the buffers
  }
}

// ---- emit ---------------------------------------------------------------------
__global__ void __launch_bounds__(kWinBlock) window_emit_kernel(WinEmitDesc D) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < D.n; i += (int64_t)gridDim.x * blockDim.x) {
    const int64_t r = D.perm ? D.perm[i] : i;
    int64_t t = i;
    if (D.target == WT_PEER_END) t = D.peer_last[i];
    else if (D.target == WT_PART_END) t = D.part_last[i];
    int64_t lo = 0, hi = 0;
    bool valid = true;
    switch (D.kind) {
      case W_ROW_NUMBER: lo = i - D.part_first[i] + 1; break;
      case W_RANK: lo = (int64_t)D.peer_first[i] - D.part_first[i] + 1; break;
      case W_DENSE_RANK: lo = (int64_t)((const uint64_t *)D.state)[i]; break;
      case W_COUNT_STAR: lo = t - D.part_first[i] + 1; break;
      case W_COUNT: lo = (int64_t)((const uint64_t *)D.state)[t]; break;
      case W_SUM:
        if (D.op == WOP_SUMF) {
          const WinSumF::State s = ((const WinSumF::State *)D.state)[t];
          valid = s.count != 0;
          lo = __double_as_longlong(s.sum);
        } else {
          const WinSum128::State s = ((const WinSum128::State *)D.state)[t];
          valid = s.count != 0;
          lo = (int64_t)s.lo;
          hi = s.hi;
        }
        break;
      case W_AVG: {
        // the conversion of the aggregates' emit (emit_cell)
        double v = 0;
        if (D.op == WOP_SUMF) {
          const WinSumF::State s = ((const WinSumF::State *)D.state)[t];
          valid = s.count != 0;
          if (valid) v = s.sum / (double)s.count;
        } else {
          const WinSum128::State s = ((const WinSum128::State *)D.state)[t];
          valid = s.count != 0;
          if (valid) {
            const double sum = i128_to_double(mk128((int64_t)s.lo, s.hi));
            double div = (double)s.count;
            for (int k = 0; k < D.avg_scale; k++) div *= 10.0;
            v = sum / div;
          }
        }
        lo = __double_as_longlong(v);
        break;
      }
      case W_MIN:
      case W_MAX:
        if (D.op == WOP_MIN128 || D.op == WOP_MAX128) {
          const WinMinMax128<false>::State s = ((const WinMinMax128<false>::State *)D.state)[t];
          valid = s.count != 0;
          lo = (int64_t)s.lo;
          hi = s.hi;
        } else {
          const WinMinMax64<false>::State s = ((const WinMinMax64<false>::State *)D.state)[t];
          valid = s.count != 0;
          const int p = D.in_phys;
          if (p == P_F64 || p == P_F32) lo = __double_as_longlong(f64_unorder(s.key));
          else if (p == P_U8 || p == P_U16 || p == P_U32 || p == P_U64) lo = (int64_t)s.key;
          else lo = (int64_t)(s.key ^ 0x8000000000000000ull);
        }
        break;
      default: {  // LAG / LEAD: a read at perm[i -/+ offset], inside the partition
        valid = false;
        int64_t j = -1;
        if (D.kind == W_LAG) {
          if (D.offset <= i - D.part_first[i]) j = i - D.offset;
        } else {
          if (D.offset <= (int64_t)D.part_last[i] - i) j = i + D.offset;
        }
        if (j >= 0 && j < D.n) {
          const int64_t rj = D.perm ? D.perm[j] : j;
          if (bit_valid(D.valid, rj)) {
            valid = true;
            load_phys(D.data, D.in_phys, rj, lo, hi);
          }
        }
        break;
      }
    }
    if (!valid) lo = hi = 0;
    store_phys(D.out, D.out_phys, r, lo, hi);
    if (D.out_valid && valid) atomicOr(&D.out_valid[r >> 5], 1u << (r & 31));
  }
}

template <typename F>
void ByOp(int op, F f) {
  switch (op) {
    case WOP_POS: f(WinPosMin()); break;
    case WOP_COUNT: f(WinCount()); break;
    case WOP_SUM128: f(WinSum128()); break;
    case WOP_SUMF: f(WinSumF()); break;
    case WOP_MIN64: f(WinMinMax64<false>()); break;
    case WOP_MAX64: f(WinMinMax64<true>()); break;
    case WOP_MIN128: f(WinMinMax128<false>()); break;
    default: f(WinMinMax128<true>()); break;
  }
}

}  // namespace

void WindowBounds(const WinKeys &K, const int64_t *perm, int64_t n, uint8_t *flags, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(window_bounds_kernel, dim3(RowGrid(n)), dim3(kWinBlock), 0, s, K, perm, n, flags);
  (void)hipGetLastError();
}

size_t WinStateBytes(int op) {
  size_t b = 0;
  ByOp(op, [&](auto o) { b = sizeof(typename decltype(o)::State); });
  return b;
}

size_t WinCarryBytes(int op) {
  size_t b = 0;
  ByOp(op, [&](auto o) { b = sizeof(WinElem<decltype(o)>); });
  return b;
}

void WindowScanReduce(const WinScanDesc &D, hipStream_t s) {
  if (D.n <= 0) return;
  const int64_t nt = WinTiles(D.n);
  ByOp(D.op, [&](auto o) {
    hipLaunchKernelGGL((window_scan_tile_kernel<decltype(o), true>), dim3((unsigned)nt), dim3(kWinBlock), 0, s, D);
  });
  (void)hipGetLastError();
}

void WindowScanCarry(const WinScanDesc &D, hipStream_t s) {
  if (D.n <= 0) return;
  const int64_t nt = WinTiles(D.n);
  ByOp(D.op, [&](auto o) {
    hipLaunchKernelGGL((window_scan_carry_kernel<decltype(o)>), dim3(1), dim3(kWinCarryLanes), 0, s, D, nt);
  });
  (void)hipGetLastError();
}

void WindowScanApply(const WinScanDesc &D, hipStream_t s) {
  if (D.n <= 0) return;
  const int64_t nt = WinTiles(D.n);
  ByOp(D.op, [&](auto o) {
    hipLaunchKernelGGL((window_scan_tile_kernel<decltype(o), false>), dim3((unsigned)nt), dim3(kWinBlock), 0, s, D);
  });
  (void)hipGetLastError();
}

void WindowEmit(const WinEmitDesc &D, hipStream_t s) {
  if (D.n <= 0) return;
  hipLaunchKernelGGL(window_emit_kernel, dim3(RowGrid(D.n)), dim3(kWinBlock), 0, s, D);
  (void)hipGetLastError();
}

}  // namespace dev
}  // namespace mbx
