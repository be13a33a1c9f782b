// kernels.hip — hand-written gfx950 (CDNA4) kernels of the columnar backend.
//
// All of this is HBM-bound integer/byte work: no MFMA.  Design rules applied
// (cdna_hip_programming.md §6 G2/G7/G11/G12/G13):
//   * 16-byte vector loads (global_load_dwordx4), several in flight per lane;
//   * wave64 ballot / mbcnt for predicate compaction and bit packing;
//   * per-thread -> per-wave (DPP/shuffle) -> per-block (LDS) reduction and
//     ONE global atomic per block and aggregate (128-bit sums as a carry-correct
//     pair of 64-bit atomics, exact in any order);
//   * GROUP BY on small key ranges in LDS-privatised replicated tables
//     (one replica per lane index -> no same-address conflicts inside a wave).
#include <hip/hip_runtime.h>
#include <hipcub/hipcub.hpp>
#include <algorithm>
#include <limits>
#include <stdexcept>
#include <string>
#include <stdint.h>
#include <type_traits>

#include "device.h"
#include "types.h"

// ---------------------------------------------------------------------------
// In-kernel clock stamps (diagnostic build only: make clockdiag compiles this
// file with MBX_CLOCK_STAMPS=1 into libduckdb_mb_amd_clk.so; in the product
// library no stamp instruction exists).  Thread 0 of each of the first
// kClkSlots workgroups of filter_agg_lds, group_direct_lds and the two-array
// ring read records the shader-clock counter (s_memtime) and the 100 MHz
// reference counter (s_memrealtime) once when its main loop starts and once
// when it has drained, with ordinary vector stores.  Clock of a workgroup =
// d(memtime) / d(realtime) x 100 MHz (MI355X_MICROARCH.md, DVFS item 6).
// ---------------------------------------------------------------------------
namespace mbx {
namespace dev {
constexpr int kClkSlots = 1024;
}
}  // namespace mbx
#if MBX_CLOCK_STAMPS
__device__ unsigned long long g_clk_stamps[mbx::dev::kClkSlots * 4];
__device__ __forceinline__ void clk_stamp(int part) {
  if (threadIdx.x == 0 && blockIdx.x < mbx::dev::kClkSlots) {
    const unsigned long long c = __builtin_amdgcn_s_memtime();
    const unsigned long long r = __builtin_amdgcn_s_memrealtime();
    g_clk_stamps[blockIdx.x * 4 + part * 2] = c;
    g_clk_stamps[blockIdx.x * 4 + part * 2 + 1] = r;
  }
}
#define MBX_CLK(part) clk_stamp(part)
#else
#define MBX_CLK(part)
#endif
#include "vm.h"
#include "vm_device.h"
#include "vm_lds.h"
#include "knobs.h"
#include "group_hash.h"

namespace mbx {
namespace dev {

typedef __int128 i128;
typedef unsigned __int128 u128;

#define CHECK_LAUNCH() (void)hipGetLastError()

// hipCUB reports a refused launch or a bad argument through its return value:
// a sort or scan that did not run must not pass for one that did
static inline void CubCheck(hipError_t err, const char *what) {
  if (err != hipSuccess) throw std::runtime_error(std::string("hipcub ") + what + ": " + hipGetErrorString(err));
}
#define CUB_CHECK(call, what) CubCheck((call), what)

static int g_num_cus = 0;
int NumCUs() {
  if (!g_num_cus) {
    int d = 0;
    (void)hipGetDevice(&d);
    hipDeviceProp_t pr;
    if (hipGetDeviceProperties(&pr, d) == hipSuccess) g_num_cus = pr.multiProcessorCount;
    if (g_num_cus <= 0) g_num_cus = 256;
  }
  return g_num_cus;
}

static inline int GridFor(int64_t work_items, int per_block, int max_blocks) {
  int64_t b = (work_items + per_block - 1) / per_block;
  if (b < 1) b = 1;
  if (b > max_blocks) b = max_blocks;
  return (int)b;
}

// ---------------------------------------------------------------------------
// expression VM (tile interpreter)
// ---------------------------------------------------------------------------
// (register planes, LdsRF and vm_exec: vm_lds.h, shared with join_kernels.hip)

__global__ __launch_bounds__(256) void vm_filter_kernel(VmProgram P, VmCols C, int64_t nrows, int64_t rs,
                                                        int64_t rstep, uint64_t *__restrict__ bits,
                                                        uint32_t *__restrict__ tile_counts, int32_t *err) {
  extern __shared__ __attribute__((aligned(16))) unsigned char vm_lds[];
  VmLds R = vm_regs(vm_lds, P.n_regs);
  __shared__ uint32_t wcnt[4];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int64_t ntiles = (nrows + VM_TILE - 1) / VM_TILE;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    int64_t row = tile * VM_TILE + t;
    bool active = row < nrows;
    vm_exec(P, C, row, active, rs, rstep, R, t, err);
    const int pr = P.pred_reg;
    bool sel = active && !R.nl[(pr) * VM_TILE + t] && R.lo[(pr) * VM_TILE + t] != 0;
    uint64_t m = __ballot(sel);
    if (lane == 0) {
      bits[tile * 4 + w] = m;
      wcnt[w] = (uint32_t)__popcll(m);
    }
    __syncthreads();
    if (t == 0) tile_counts[tile] = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
    __syncthreads();
  }
}

__global__ __launch_bounds__(256) void vm_project_kernel(VmProgram P, VmCols C, int64_t nrows, int64_t rs,
                                                         int64_t rstep, const uint64_t *__restrict__ bits,
                                                         const int64_t *__restrict__ tile_off, VmOuts O,
                                                         int32_t *err) {
  extern __shared__ __attribute__((aligned(16))) unsigned char vm_lds[];
  VmLds R = vm_regs(vm_lds, P.n_regs);
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int64_t ntiles = (nrows + VM_TILE - 1) / VM_TILE;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    int64_t row = tile * VM_TILE + t;
    bool sel;
    int64_t out_idx;
    if (bits) {
      const uint64_t *tb = bits + tile * 4;
      uint64_t b0 = tb[0], b1 = tb[1], b2 = tb[2], b3 = tb[3];
      if ((b0 | b1 | b2 | b3) == 0) continue;  // uniform across the block
      uint64_t mine = w == 0 ? b0 : w == 1 ? b1 : w == 2 ? b2 : b3;
      int before = (w > 0 ? __popcll(b0) : 0) + (w > 1 ? __popcll(b1) : 0) + (w > 2 ? __popcll(b2) : 0);
      sel = (mine >> lane) & 1ull;
      uint64_t lt = lane ? (mine & ((1ull << lane) - 1ull)) : 0ull;
      out_idx = tile_off[tile] + before + __popcll(lt);
    } else {
      sel = row < nrows;
      out_idx = row;
    }
    vm_exec(P, C, row, sel, rs, rstep, R, t, err);
    if (sel) {
      for (int o = 0; o < P.n_out; o++) {
        const int r = P.out_reg[o];
        store_phys(O.data[o], P.out_phys[o], out_idx, R.lo[(r) * VM_TILE + t], R.hi[(r) * VM_TILE + t]);
        if (R.nl[(r) * VM_TILE + t] && O.nullbits[o]) {
          atomicOr(&O.nullbits[o][out_idx >> 5], 1u << (out_idx & 31));
          if (O.anynull) O.anynull[o] = 1;
        }
      }
    }
  }
}

void VmFilter(const VmProgram &p, const VmCols &cols, int64_t nrows, int64_t range_start, int64_t range_step,
              uint64_t *sel_bits, uint32_t *tile_counts, int32_t *err, hipStream_t s) {
  if (nrows <= 0) return;
  int64_t ntiles = (nrows + VM_TILE - 1) / VM_TILE;
  int grid = GridFor(ntiles, 1, NumCUs() * 8);
  hipLaunchKernelGGL(vm_filter_kernel, dim3(grid), dim3(256), VmLdsBytes(p.n_regs), s, p, cols, nrows, range_start,
                     range_step, sel_bits,
                     tile_counts, err);
  CHECK_LAUNCH();
}

void VmProject(const VmProgram &p, const VmCols &cols, int64_t nrows, int64_t range_start, int64_t range_step,
               const uint64_t *sel_bits, const int64_t *tile_offsets, const VmOuts &outs, int32_t *err,
               hipStream_t s) {
  if (nrows <= 0) return;
  int64_t ntiles = (nrows + VM_TILE - 1) / VM_TILE;
  int grid = GridFor(ntiles, 1, NumCUs() * 8);
  hipLaunchKernelGGL(vm_project_kernel, dim3(grid), dim3(256), VmLdsBytes(p.n_regs), s, p, cols, nrows, range_start,
                     range_step,
                     sel_bits, tile_offsets, outs, err);
  CHECK_LAUNCH();
}

__global__ void invert_bits_kernel(uint64_t *bits, int64_t n) {
  const int64_t words = (n + 63) >> 6;
  for (int64_t w = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; w < words; w += (int64_t)gridDim.x * blockDim.x) {
    uint64_t v = ~bits[w];
    if (w == words - 1 && (n & 63)) v &= (1ull << (n & 63)) - 1ull;
    bits[w] = v;
  }
}

void InvertNullBits(uint64_t *bits, int64_t n, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(invert_bits_kernel, dim3(GridFor((n + 63) >> 6, 256, NumCUs() * 4)), dim3(256), 0, s, bits, n);
  CHECK_LAUNCH();
}

__global__ void scan_total_kernel(const uint32_t *counts, const int64_t *offsets, int64_t n, int64_t *total) {
  *total = n ? offsets[n - 1] + (int64_t)counts[n - 1] : 0;
}

struct U32ToI64 {
  __host__ __device__ int64_t operator()(uint32_t x) const { return (int64_t)x; }
};

void ScanTileCounts(const uint32_t *counts, int64_t *offsets, int64_t n, int64_t *total, hipStream_t s) {
  if (n <= 0) {
    (void)hipMemsetAsync(total, 0, sizeof(int64_t), s);
    return;
  }
  hipcub::TransformInputIterator<int64_t, U32ToI64, const uint32_t *> it(counts, U32ToI64());
  size_t tmp = 0;
  CUB_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp, it, offsets, (int)n, s), "ExclusiveSum");
  void *d_tmp = nullptr;
  d_tmp = TempAlloc(tmp);
  CUB_CHECK(hipcub::DeviceScan::ExclusiveSum(d_tmp, tmp, it, offsets, (int)n, s), "ExclusiveSum");
  TempFree(d_tmp, tmp);
  hipLaunchKernelGGL(scan_total_kernel, dim3(1), dim3(1), 0, s, counts, offsets, n, total);
}

// selected rows of a 256-row step = popcount of its four ballot words
struct StepPopc {
  const unsigned long long *b;
  __host__ __device__ int64_t operator()(int64_t i) const {
    return (int64_t)(__popcll(b[4 * i]) + __popcll(b[4 * i + 1]) + __popcll(b[4 * i + 2]) + __popcll(b[4 * i + 3]));
  }
};

__global__ void scan_bits_total_kernel(const unsigned long long *bits, const int64_t *offsets, int64_t n,
                                       int64_t *total) {
  *total = n ? offsets[n - 1] + StepPopc{bits}(n - 1) : 0;
}

void ScanStepBits(const unsigned long long *bits, int64_t *offsets, int64_t steps, int64_t *total, hipStream_t s) {
  if (steps <= 0) {
    (void)hipMemsetAsync(total, 0, sizeof(int64_t), s);
    return;
  }
  hipcub::CountingInputIterator<int64_t> idx(0);
  hipcub::TransformInputIterator<int64_t, StepPopc, hipcub::CountingInputIterator<int64_t>> it(idx, StepPopc{bits});
  size_t tmp = 0;
  CUB_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp, it, offsets, (int)steps, s), "ExclusiveSum");
  void *d_tmp = TempAlloc(tmp);
  CUB_CHECK(hipcub::DeviceScan::ExclusiveSum(d_tmp, tmp, it, offsets, (int)steps, s), "ExclusiveSum");
  TempFree(d_tmp, tmp);
  hipLaunchKernelGGL(scan_bits_total_kernel, dim3(1), dim3(1), 0, s, bits, offsets, steps, total);
}

// ---------------------------------------------------------------------------
// fused scan -> filter -> aggregate (configs C2 and C5)
// ---------------------------------------------------------------------------
// Per-thread accumulators: count, int128 sum (lo/hi with carry), min, max.
struct Acc {
  uint64_t cnt;
  uint64_t slo;
  int64_t shi;
  int64_t mn, mx;
};

__device__ __forceinline__ void acc_add(Acc &A, bool ok, int64_t v) {
  A.cnt += ok;
  int64_t vv = ok ? v : 0;
  uint64_t nlo = A.slo + (uint64_t)vv;
  A.shi += (vv >> 63) + (nlo < A.slo ? 1 : 0);
  A.slo = nlo;
  A.mn = ok && v < A.mn ? v : A.mn;
  A.mx = ok && v > A.mx ? v : A.mx;
}

__device__ __forceinline__ void acc_merge(Acc &A, const Acc &B) {
  A.cnt += B.cnt;
  uint64_t nlo = A.slo + B.slo;
  A.shi += B.shi + (nlo < A.slo ? 1 : 0);
  A.slo = nlo;
  A.mn = B.mn < A.mn ? B.mn : A.mn;
  A.mx = B.mx > A.mx ? B.mx : A.mx;
}

__device__ __forceinline__ uint64_t shfl_xor_u64(uint64_t v, int m) {
  return (uint64_t)__shfl_xor((long long)v, m, 64);
}

__device__ __forceinline__ void acc_wave_reduce(Acc &A) {
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    Acc B;
    B.cnt = shfl_xor_u64(A.cnt, m);
    B.slo = shfl_xor_u64(A.slo, m);
    B.shi = (int64_t)shfl_xor_u64((uint64_t)A.shi, m);
    B.mn = (int64_t)shfl_xor_u64((uint64_t)A.mn, m);
    B.mx = (int64_t)shfl_xor_u64((uint64_t)A.mx, m);
    acc_merge(A, B);
  }
}

__device__ __forceinline__ void agg_state_atomic(AggState *st, const Acc &A) {
  atomicAdd(&st->count, (unsigned long long)A.cnt);
  unsigned long long old = atomicAdd(&st->sum_lo, (unsigned long long)A.slo);
  unsigned long long carry = (old + (unsigned long long)A.slo) < old ? 1ull : 0ull;
  atomicAdd((unsigned long long *)&st->sum_hi, (unsigned long long)A.shi + carry);
  atomicMin(&st->min_i, (long long)A.mn);
  atomicMax(&st->max_i, (long long)A.mx);
}

// Block-level finish: wave shuffle reduction, LDS across the 4 waves, one
// set of atomics per block.
__device__ __forceinline__ void acc_block_commit(Acc &A, AggState *st, unsigned long long *cstar, bool count_is_star) {
  __shared__ Acc part[4];
  acc_wave_reduce(A);
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) part[w] = A;
  __syncthreads();
  if (threadIdx.x == 0) {
    Acc T = part[0];
    for (int i = 1; i < (int)(blockDim.x >> 6); i++) acc_merge(T, part[i]);
    if (cstar) atomicAdd(cstar, (unsigned long long)T.cnt);
    if (st) agg_state_atomic(st, T);
  }
  (void)count_is_star;
}

typedef long long v2i64 __attribute__((ext_vector_type(2)));
typedef int v4i32 __attribute__((ext_vector_type(4)));
// Row-pair loads: lane l of a wave reads rows {2l, 2l+1} of a 128-row wave
// step, so ONE load instruction covers a contiguous 1 KiB (int64) or 512 B
// (int32) with no holes — every cache line is requested once.
typedef int v2i32 __attribute__((ext_vector_type(2)));
template <typename T, bool NT>
struct Pair;
template <bool NT>
struct Pair<int64_t, NT> {
  static __device__ __forceinline__ void load(const int64_t *__restrict__ p, int64_t pi, int64_t &a, int64_t &b) {
    const v2i64 *q = (const v2i64 *)p + pi;
    v2i64 v = NT ? __builtin_nontemporal_load(q) : *q;
    a = v.x;
    b = v.y;
  }
};
template <bool NT>
struct Pair<int32_t, NT> {
  static __device__ __forceinline__ void load(const int32_t *__restrict__ p, int64_t pi, int64_t &a, int64_t &b) {
    const v2i32 *q = (const v2i32 *)p + pi;
    v2i32 v = NT ? __builtin_nontemporal_load(q) : *q;
    a = v.x;
    b = v.y;
  }
};

__device__ __forceinline__ void acc_count(Acc &A, bool ok) { A.cnt += ok; }

// Register-load filter-aggregate for the one shape filter_agg_lds below does
// not take: a predicate column and an aggregated column of different widths
// (MODE 1, TP != TA).  UNROLL row-pair loads in flight per lane, non-temporal,
// one contiguous slice of pairs per workgroup (CHUNK): the best register-load
// shape of the sweep in profiles/r01_filter_sweep_lds.json.  The loop is
// written for any MODE / CHUNK; the constants below pick the shape that runs.
template <typename TP, typename TA>
__global__ __launch_bounds__(256) void filter_agg_kernel(const TP *__restrict__ p, const TA *__restrict__ a, int64_t n,
                                                         int64_t lo, uint64_t span, AggState *st,
                                                         unsigned long long *cstar) {
  constexpr int MODE = 1, UNROLL = 8;
  constexpr bool NT = true, CHUNK = true;
  Acc A;
  A.cnt = 0; A.slo = 0; A.shi = 0; A.mn = INT64_MAX; A.mx = INT64_MIN;
  const int64_t npairs = n >> 1;
  int64_t g, gend, stride;
  if (CHUNK) {
    const int64_t per = (npairs + gridDim.x - 1) / gridDim.x;
    g = (int64_t)blockIdx.x * per + threadIdx.x;
    gend = (int64_t)blockIdx.x * per + per;
    if (gend > npairs) gend = npairs;
    stride = blockDim.x;
  } else {
    g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    gend = npairs;
    stride = (int64_t)gridDim.x * blockDim.x;
  }
  for (; g + (UNROLL - 1) * stride < gend; g += UNROLL * stride) {
    int64_t p0[UNROLL], p1[UNROLL], a0[UNROLL], a1[UNROLL];
#pragma unroll
    for (int u = 0; u < UNROLL; u++) {
      Pair<TP, NT>::load(p, g + u * stride, p0[u], p1[u]);
      if (MODE == 1) Pair<TA, NT>::load(a, g + u * stride, a0[u], a1[u]);
    }
#pragma unroll
    for (int u = 0; u < UNROLL; u++) {
      bool ok0 = (uint64_t)(p0[u]) - (uint64_t)(lo) <= span, ok1 = (uint64_t)(p1[u]) - (uint64_t)(lo) <= span;
      if (MODE == 2) {
        acc_count(A, ok0);
        acc_count(A, ok1);
      } else if (MODE == 1) {
        acc_add(A, ok0, a0[u]);
        acc_add(A, ok1, a1[u]);
      } else {
        acc_add(A, ok0, p0[u]);
        acc_add(A, ok1, p1[u]);
      }
    }
  }
  for (; g < gend; g += stride) {
    int64_t x0, x1, y0 = 0, y1 = 0;
    Pair<TP, NT>::load(p, g, x0, x1);
    if (MODE == 1) Pair<TA, NT>::load(a, g, y0, y1);
    bool ok0 = (uint64_t)(x0) - (uint64_t)(lo) <= span, ok1 = (uint64_t)(x1) - (uint64_t)(lo) <= span;
    if (MODE == 2) {
      acc_count(A, ok0);
      acc_count(A, ok1);
    } else {
      acc_add(A, ok0, MODE == 1 ? y0 : x0);
      acc_add(A, ok1, MODE == 1 ? y1 : x1);
    }
  }
  // odd last row: first thread of block 0
  if ((n & 1) && blockIdx.x == 0 && threadIdx.x == 0) {
    int64_t x = p[n - 1];
    bool ok = (uint64_t)(x) - (uint64_t)(lo) <= span;
    if (MODE == 2) acc_count(A, ok);
    else acc_add(A, ok, MODE == 1 ? (int64_t)a[n - 1] : x);
  }
  acc_block_commit(A, MODE == 2 ? nullptr : st, cstar, true);
}

// LDS-DMA streaming version: each wave owns a ring of DEPTH slots of 1 KiB
// (64 lanes x 16 B, global_load_lds_dwordx4) per column; waves walk the
// column's 1-KiB pieces grid-stride, so the whole chip streams through one
// contiguous window.  The oldest slot is consumed once at most DEPTH-1 newer
// pieces are pending (counted vmcnt, never 0 in the loop).  All LDS — ring
// and the final block reduction — lives in ONE __shared__ array (a second
// __shared__ object makes hipcc drain vmcnt before every ds_read).
// A piece is 128 int64 rows or 256 int32 rows; rows past the last whole
// piece are handled by wave 0 of block 0.  MODE 1 needs TP == TA here.
// MM: MIN/MAX requested.  NARROW: the host proved from the column's zone map
// that no lane's int64 partial sum can overflow, so the per-row int128 carry
// chain collapses to one int64 add (sign-extended once, before the reduce).
__device__ __forceinline__ void acc_row(Acc &A, bool ok, int64_t v, bool mm, bool narrow) {
  if (!narrow) {
    if (mm) {
      acc_add(A, ok, v);
    } else {
      A.cnt += ok;
      int64_t vv = ok ? v : 0;
      uint64_t nlo = A.slo + (uint64_t)vv;
      A.shi += (vv >> 63) + (nlo < A.slo ? 1 : 0);
      A.slo = nlo;
    }
    return;
  }
  A.cnt += ok;
  A.slo += (uint64_t)(ok ? v : 0);
  if (mm) {
    A.mn = ok && v < A.mn ? v : A.mn;
    A.mx = ok && v > A.mx ? v : A.mx;
  }
}

// MM: 0 no MIN/MAX, 1 int64 MIN/MAX, 2 int32 MIN/MAX (the zone map bounds |value|
// below 2^31: one v_min_i32 / v_max_i32 per row instead of 64-bit compare pairs)
template <typename T, int MODE, int DEPTH, int MM, bool NARROW>
__global__ __launch_bounds__(256) void filter_agg_lds_kernel(const T *__restrict__ p, const T *__restrict__ a, int64_t n,
                                                             int64_t lo, uint64_t span, AggState *st,
                                                             unsigned long long *cstar, AggPartial *partials) {
  constexpr int NS = MODE == 1 ? 2 : 1;
  constexpr int RPL = 16 / (int)sizeof(T);
  constexpr int64_t RP = 64 * RPL;
  __shared__ __attribute__((aligned(16))) v2i64 ring[4 * NS * DEPTH * 64];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t npieces = n / RP;
  const int64_t nw = (int64_t)gridDim.x * 4;
  int64_t pc = (int64_t)blockIdx.x * 4 + w;
  v2i64 *slot0 = ring + w * NS * DEPTH * 64;
  const v2i64 *P = (const v2i64 *)p, *A2 = (const v2i64 *)a;
  Acc A;
  A.cnt = 0; A.slo = 0; A.shi = 0; A.mn = INT64_MAX; A.mx = INT64_MIN;
  int32_t mn32 = INT32_MAX, mx32 = INT32_MIN;
  auto row = [&](bool ok, int64_t v) {
    acc_row(A, ok, v, MM == 1, NARROW);
    if (MM == 2) {
      mn32 = min(mn32, ok ? (int32_t)v : INT32_MAX);
      mx32 = max(mx32, ok ? (int32_t)v : INT32_MIN);
    }
  };
#pragma unroll
  for (int d = 0; d < DEPTH; d++) {
    int64_t q = pc + d * nw;
    q = q < npieces ? q : 0;  // keep the per-slot load count uniform (dummy piece 0)
    if (npieces > 0) {
      __builtin_amdgcn_global_load_lds((const void *)(P + q * 64 + lane), (void *)(slot0 + d * 64), 16, 0, 2);
      if (NS == 2)
        __builtin_amdgcn_global_load_lds((const void *)(A2 + q * 64 + lane), (void *)(slot0 + (DEPTH + d) * 64), 16, 0, 2);
    }
  }
  int k = 0;
  MBX_CLK(0);
  for (; pc < npieces; pc += nw) {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NS * (DEPTH - 1)) : "memory");
    v2i64 x = slot0[k * 64 + lane];
    v2i64 y;
    if (NS == 2) y = slot0[(DEPTH + k) * 64 + lane];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    int64_t q = pc + DEPTH * nw;
    q = q < npieces ? q : pc;  // past the end: re-read the piece just consumed
    __builtin_amdgcn_global_load_lds((const void *)(P + q * 64 + lane), (void *)(slot0 + k * 64), 16, 0, 2);
    if (NS == 2)
      __builtin_amdgcn_global_load_lds((const void *)(A2 + q * 64 + lane), (void *)(slot0 + (DEPTH + k) * 64), 16, 0, 2);
    if (sizeof(T) == 8) {
      bool ok0 = (uint64_t)(x.x) - (uint64_t)(lo) <= span, ok1 = (uint64_t)(x.y) - (uint64_t)(lo) <= span;
      if (MODE == 2) {
        acc_count(A, ok0);
        acc_count(A, ok1);
      } else {
        row(ok0, MODE == 1 ? y.x : x.x);
        row(ok1, MODE == 1 ? y.y : x.y);
      }
    } else {
      const int *xi = (const int *)&x, *yi = (const int *)&y;
#pragma unroll
      for (int e = 0; e < 4; e++) {
        bool ok = (uint64_t)((int64_t)xi[e]) - (uint64_t)(lo) <= span;
        if (MODE == 2) acc_count(A, ok);
        else row(ok, (int64_t)(MODE == 1 ? yi[e] : xi[e]));
      }
    }
    k = k + 1 == DEPTH ? 0 : k + 1;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  MBX_CLK(1);
  if (blockIdx.x == 0 && w == 0) {
    for (int64_t i = npieces * RP + lane; i < n; i += 64) {
      int64_t xv = p[i];
      bool ok = (uint64_t)(xv) - (uint64_t)(lo) <= span;
      if (MODE == 2) acc_count(A, ok);
      else row(ok, MODE == 1 ? (int64_t)a[i] : xv);
    }
  }
  if (MM == 2) {  // no selected row leaves INT32_MAX / INT32_MIN: the emit reads a count of 0 as NULL
    A.mn = mn32;
    A.mx = mx32;
  }
  if (NARROW) A.shi = (int64_t)A.slo >> 63;
  // block reduction through the same LDS array
  acc_wave_reduce(A);
  __syncthreads();
  Acc *part = (Acc *)ring;
  if (lane == 0) part[w] = A;
  __syncthreads();
  if (threadIdx.x == 0) {
    Acc T0 = part[0];
    for (int i = 1; i < 4; i++) acc_merge(T0, part[i]);
    if (partials) {
      partials[blockIdx.x] = AggPartial{T0.cnt, T0.slo, T0.shi, T0.mn, T0.mx};
    } else {
      if (cstar) atomicAdd(cstar, (unsigned long long)T0.cnt);
      if (MODE != 2 && st) agg_state_atomic(st, T0);
    }
  }
}

// The same ring over a column's code image (scan_codes.h): F codes of
// value - base per 32-bit word in fields of Bf = 32 / F bits, a 1-KiB piece is
// 256 F rows, 4 F codes per lane.  The predicate is clo <= code <= clo + cspan.
// MODE 2 counts; MODE 0 also sums the passing codes.  FORM (ScanCompare, chosen
// by PlanScanFieldRange) is the compare: a word-parallel one leaves one bit per
// passing field, the count is a popcount, and the sum adds the masked word's
// even and odd fields into 2 Bf-bit lanes that are folded once per piece (four
// words: at most 4 (2^Bf - 1) per lane; a 1-bit code sums by popcount, a byte
// by v_sad_u8).  SC_PER_CODE extracts every field and also takes the passing
// codes' min / max.  Per piece a lane adds at most 16 x 65535 to 32-bit piece
// totals, folded into 64-bit lane totals; the value sum is codes + count x base
// in int128, once per lane, so the partial records are exactly those of the
// 8-byte kernel.
template <int F, int MODE, int DEPTH, int FORM>
__global__ __launch_bounds__(256) void filter_agg_codes_kernel(const uint32_t *__restrict__ codes, int64_t n,
                                                               uint32_t clo, uint32_t cspan, int64_t base,
                                                               AggPartial *partials) {
  constexpr int BF = ScanFieldBits(F);
  constexpr int64_t RP = ScanPieceRows(F);
  constexpr bool MM = FORM == SC_PER_CODE;
  constexpr uint32_t EVEN = ScanEvenFields(F);
  __shared__ __attribute__((aligned(16))) v4i32 ring[4 * DEPTH * 64];
  static_assert(sizeof(v4i32) * 4 * DEPTH * 64 >= 4 * sizeof(Acc), "the block reduction reuses the ring");
  static_assert(F * BF <= 32 && 16ull * F * ScanFieldMax(F) < (1ull << 32), "a piece's totals fit 32 bits");
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t npieces = n / RP;
  const int64_t nw = (int64_t)gridDim.x * 4;
  int64_t pc = (int64_t)blockIdx.x * 4 + w;
  v4i32 *slot0 = ring + w * DEPTH * 64;
  const v4i32 *P = (const v4i32 *)codes;
  const ScanWordCmp K = ScanWordCmpOf(F, FORM, clo, clo + cspan);
  uint64_t cnt = 0, sum = 0;
  int32_t mn = INT32_MAX, mx = -1;  // codes are below 2^16
  auto one = [&](uint32_t c, uint32_t &pcnt, uint32_t &psum) {
    const bool ok = c - clo <= cspan;
    pcnt += ok;
    if (MODE == 0) psum += ok ? c : 0u;
    if (MM) {
      mn = min(mn, ok ? (int32_t)c : INT32_MAX);
      mx = max(mx, ok ? (int32_t)c : -1);
    }
  };
  // ev / od: the piece's passing codes of the even and the odd fields, in lanes of 2 BF bits
  auto word = [&](uint32_t x, uint32_t &pcnt, uint32_t &psum, uint32_t &ev, uint32_t &od) {
    if (FORM != SC_PER_CODE) {
      const uint32_t m = ScanWordMask(FORM, x, K);
      pcnt += __builtin_popcount(m);
      if (MODE == 0) {
        if (BF == 1) {
          psum += __builtin_popcount(x & m);
        } else if (BF == 8) {
          psum = __builtin_amdgcn_sad_u8(x & ScanFieldsOf(F, m), 0u, psum);
        } else {
          const uint32_t t = x & ScanFieldsOf(F, m);
          ev += t & EVEN;
          od += (t >> BF) & EVEN;
        }
      }
    } else {
#pragma unroll
      for (int e = 0; e < F; e++) one((x >> (BF * e)) & ScanFieldMax(F), pcnt, psum);
    }
  };
  auto fold = [&](uint32_t ev, uint32_t od, uint32_t &psum) {
    if (MODE != 0 || FORM == SC_PER_CODE || BF == 1 || BF == 8) return;
    if (BF == 2) {  // a 4-bit lane holds 4 x 3, not 8 x 3: fold the two halves apart
#pragma unroll
      for (int e = 0; e < 8; e++) psum += ((ev >> (4 * e)) & 0xFu) + ((od >> (4 * e)) & 0xFu);
    } else if constexpr (BF == 16) {
      psum += ev + od;
    } else {
      const uint32_t t = ev + od;
#pragma unroll
      for (int e = 0; e < (F + 1) / 2; e++) psum += (t >> (2 * BF * e)) & ((1u << (2 * BF)) - 1u);
    }
  };
#pragma unroll
  for (int d = 0; d < DEPTH; d++) {
    int64_t q = pc + d * nw;
    q = q < npieces ? q : 0;  // keep the per-slot load count uniform (dummy piece 0)
    if (npieces > 0) __builtin_amdgcn_global_load_lds((const void *)(P + q * 64 + lane), (void *)(slot0 + d * 64), 16, 0, 2);
  }
  int k = 0;
  for (; pc < npieces; pc += nw) {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(DEPTH - 1) : "memory");
    v4i32 x = slot0[k * 64 + lane];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    int64_t q = pc + DEPTH * nw;
    q = q < npieces ? q : pc;  // past the end: re-read the piece just consumed
    __builtin_amdgcn_global_load_lds((const void *)(P + q * 64 + lane), (void *)(slot0 + k * 64), 16, 0, 2);
    uint32_t pcnt = 0, psum = 0, ev = 0, od = 0;
    word((uint32_t)x.x, pcnt, psum, ev, od);
    word((uint32_t)x.y, pcnt, psum, ev, od);
    word((uint32_t)x.z, pcnt, psum, ev, od);
    word((uint32_t)x.w, pcnt, psum, ev, od);
    fold(ev, od, psum);
    cnt += pcnt;
    sum += psum;
    k = k + 1 == DEPTH ? 0 : k + 1;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (blockIdx.x == 0 && w == 0) {
    uint32_t pcnt = 0, psum = 0;
    for (int64_t i = npieces * RP + lane; i < n; i += 64) one(ScanCodeAt(codes, F, i), pcnt, psum);
    cnt += pcnt;
    sum += psum;
  }
  Acc A;
  A.cnt = cnt;
  {
    const __int128 s = (__int128)(unsigned __int128)sum + (__int128)(unsigned __int128)cnt * (__int128)base;
    A.slo = (uint64_t)s;
    A.shi = (int64_t)(s >> 64);
  }
  A.mn = MM && mx >= 0 ? (int64_t)((uint64_t)base + (uint64_t)mn) : INT64_MAX;
  A.mx = MM && mx >= 0 ? (int64_t)((uint64_t)base + (uint64_t)mx) : INT64_MIN;
  acc_wave_reduce(A);
  __syncthreads();
  Acc *part = (Acc *)ring;
  if (lane == 0) part[w] = A;
  __syncthreads();
  if (threadIdx.x == 0) {
    Acc T0 = part[0];
    for (int i = 1; i < 4; i++) acc_merge(T0, part[i]);
    partials[blockIdx.x] = AggPartial{T0.cnt, T0.slo, T0.shi, T0.mn, T0.mx};
  }
}

// Builds the words of the code image that hold rows [begin, end): every word
// from begin / F on is made whole from the values (the fields of rows >= end
// stay zero), so extending an image never reads it back.  A block takes tiles
// of 512 words: the 512 F values come in as coalesced 16-byte loads, their
// codes go to LDS, and each thread packs two words from F neighbouring codes
// and stores them, so no two threads ever write the same word.  The words
// before the first tile (it starts at a word that is a multiple of 4, which
// keeps the 16-byte loads aligned for every F) and after the last are packed
// one per thread straight from the values.
template <typename T, int F>
__global__ __launch_bounds__(256) void scan_encode_kernel(const T *__restrict__ v, uint32_t *__restrict__ words,
                                                          int64_t begin, int64_t end, uint64_t base) {
  constexpr int BF = ScanFieldBits(F);
  constexpr int R = 16 / (int)sizeof(T);  // rows per 16-byte load
  constexpr int TW = 512;                 // words per tile
  constexpr int UNITS = TW * F / R;       // 16-byte loads per tile
  __shared__ __attribute__((aligned(16))) uint16_t lds[TW * F];
  const int64_t w0 = begin / F, wend = ScanCodeWords(F, end), wfull = end / F;
  int64_t wa = (w0 + 3) & ~(int64_t)3;
  if (wa > wfull) wa = wfull;
  const int64_t ntiles = (wfull - wa) / TW;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const v4i32 *src = (const v4i32 *)(v + (wa + t * TW) * F);
#pragma unroll 4
    for (int u = threadIdx.x; u < UNITS; u += 256) {
      const v4i32 x = __builtin_nontemporal_load(src + u);
      if (sizeof(T) == 8) {
        const uint64_t c0 = ((uint64_t)(uint32_t)x.x | ((uint64_t)(uint32_t)x.y << 32)) - base;
        const uint64_t c1 = ((uint64_t)(uint32_t)x.z | ((uint64_t)(uint32_t)x.w << 32)) - base;
        ((uint32_t *)lds)[u] = (uint32_t)(uint16_t)c0 | ((uint32_t)(uint16_t)c1 << 16);
      } else {
        const uint32_t c0 = (uint16_t)((uint64_t)(int64_t)x.x - base), c1 = (uint16_t)((uint64_t)(int64_t)x.y - base);
        const uint32_t c2 = (uint16_t)((uint64_t)(int64_t)x.z - base), c3 = (uint16_t)((uint64_t)(int64_t)x.w - base);
        ((uint2 *)lds)[u] = make_uint2(c0 | (c1 << 16), c2 | (c3 << 16));
      }
    }
    __syncthreads();
#pragma unroll
    for (int h = 0; h < TW / 256; h++) {
      const int wi = h * 256 + threadIdx.x;
      uint32_t o = 0;
#pragma unroll
      for (int e = 0; e < F; e++) o |= (uint32_t)lds[wi * F + e] << (BF * e);
      words[wa + t * TW + wi] = o;
    }
    __syncthreads();
  }
  const int64_t nhead = wa - w0, t0 = wa + ntiles * TW, nslow = nhead + (wend - t0);
  for (int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x; j < nslow; j += (int64_t)gridDim.x * 256) {
    const int64_t wi = j < nhead ? w0 + j : t0 + (j - nhead);
    uint32_t o = 0;
#pragma unroll
    for (int e = 0; e < F; e++) {
      const int64_t row = wi * F + e;
      if (row < end) o |= ((uint32_t)((uint64_t)(int64_t)v[row] - base) & ScanFieldMax(F)) << (BF * e);
    }
    words[wi] = o;
  }
}

// The same ring over a column's bit-plane image (scan_planes.h): a wave's work
// item is piece q, 8192 rows, and it issues one 16-B-per-lane LDS-DMA load per
// plane read, NP of them, into its own slot: the 1 KiB of every plane position
// 0 .. NP - 1 that holds those rows.  A lane then has four words, 128 rows, of
// every plane.  SIDES (bit 0: code >= clo, bit 1: code <= chi) are the
// bit-serial compares over the NP planes, klo / khi the bounds' same NP bits.
// MODE 2 counts; MODE 0 (NP is then all b planes) also sums the passing codes
// by popcounts, and MM takes their min / max by narrowing a candidate mask.
// Per piece a lane adds at most 128 to its count and 128 x 255 to its sum in
// 32-bit piece totals, folded into 64-bit lane totals; the value sum is codes
// + count x base in int128, once per lane, so the partial records are exactly
// those of the 8-byte kernel.  The rows past the last whole piece go to wave 0
// of block 0, by plain loads, the last word masked to n.
// A wave keeps DEPTH pieces of NP KiB in flight: at least the 6 KiB of the
// other rings, in a block of at most 64 KiB (DESIGN.md §3 has the depths tried).
// MBX_SCAN_PLANES_RING_KIB is a build-time knob kept only so that those depth
// trials can be repeated (make OPT="-O3 -DMBX_SCAN_PLANES_RING_KIB=12"); the
// shipped library is built without it.
#ifndef MBX_SCAN_PLANES_RING_KIB
#define MBX_SCAN_PLANES_RING_KIB 6
#endif
constexpr int ScanPlanesDepth(int np) {
  int d = (MBX_SCAN_PLANES_RING_KIB + np - 1) / np;
  if (d > 16 / np) d = 16 / np;
  return d < 2 ? 2 : d;
}
template <int NP, int SIDES, int MODE, bool MM>
__global__ __launch_bounds__(256) void filter_agg_planes_kernel(const uint32_t *__restrict__ planes, int64_t n, int b,
                                                                uint32_t klo, uint32_t khi, int64_t base,
                                                                AggPartial *partials) {
  constexpr int DEPTH = ScanPlanesDepth(NP);
  __shared__ __attribute__((aligned(16))) v4i32 ring[4 * DEPTH * NP * 64];
  static_assert(sizeof(v4i32) * 4 * DEPTH * NP * 64 <= 65536 && NP * (DEPTH - 1) <= 63, "the ring fits a block and vmcnt");
  static_assert(sizeof(v4i32) * 4 * DEPTH * NP * 64 >= 4 * sizeof(Acc), "the block reduction reuses the ring");
  static_assert(MODE == 0 || (MODE == 2 && !MM && SIDES != 0), "MIN / MAX come with the sum; a count tests a side");
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const int64_t npieces = n / kScanPlanePieceRows;
  const int64_t nw = (int64_t)gridDim.x * 4;
  int64_t pc = (int64_t)blockIdx.x * 4 + w;
  v4i32 *slot0 = ring + w * DEPTH * NP * 64;
  const char *P = (const char *)planes + lane * 16;
  uint64_t cnt = 0, sum = 0;
  int32_t mn = INT32_MAX, mx = -1;  // codes are below 2^8
  // the 32 rows `rows` of one word index: p[k] is the word of plane position k
  auto word = [&](const uint32_t *p, uint32_t rows, uint32_t &pcnt, uint32_t &psum) {
    uint32_t m = rows;
    if (SIDES & 1) m &= ScanPlanesGe(p, NP, klo);
    if (SIDES & 2) m &= ScanPlanesLe(p, NP, khi);
    pcnt += __builtin_popcount(m);
    if (MODE == 0) psum += ScanPlanesSum(p, NP, m);
    if (MM) {
      mn = min(mn, m ? (int32_t)ScanPlanesMin(p, NP, m) : INT32_MAX);
      mx = max(mx, m ? (int32_t)ScanPlanesMax(p, NP, m) : -1);
    }
  };
  auto issue = [&](int64_t q, int d) {
#pragma unroll
    for (int k = 0; k < NP; k++)
      __builtin_amdgcn_global_load_lds((const void *)(P + ScanPlanePieceByte(b, k, q)), (void *)(slot0 + (d * NP + k) * 64),
                                       16, 0, 2);
  };
#pragma unroll
  for (int d = 0; d < DEPTH; d++) {
    int64_t q = pc + d * nw;
    q = q < npieces ? q : 0;  // keep the per-slot load count uniform (dummy piece 0)
    if (npieces > 0) issue(q, d);
  }
  int kk = 0;
  for (; pc < npieces; pc += nw) {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NP * (DEPTH - 1)) : "memory");
    v4i32 x[NP];
#pragma unroll
    for (int k = 0; k < NP; k++) x[k] = slot0[(kk * NP + k) * 64 + lane];
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    int64_t q = pc + DEPTH * nw;
    q = q < npieces ? q : pc;  // past the end: re-read the piece just consumed
    issue(q, kk);
    uint32_t pcnt = 0, psum = 0;
#pragma unroll
    for (int e = 0; e < 4; e++) {
      uint32_t p[NP];
#pragma unroll
      for (int k = 0; k < NP; k++) p[k] = (uint32_t)x[k][e];
      word(p, ~0u, pcnt, psum);
    }
    cnt += pcnt;
    sum += psum;
    kk = kk + 1 == DEPTH ? 0 : kk + 1;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (blockIdx.x == 0 && w == 0) {
    const int64_t r0 = npieces * kScanPlanePieceRows, tw = ScanPlaneWords(n - r0);  // at most 256 words a plane
    uint32_t pcnt = 0, psum = 0;
    for (int64_t i = lane; i < tw; i += 64) {
      uint32_t p[NP];
#pragma unroll
      for (int k = 0; k < NP; k++) p[k] = planes[ScanPlaneWord(b, k, r0 + i * 32)];
      word(p, i == tw - 1 ? ScanPlaneLastWordMask(n) : ~0u, pcnt, psum);
    }
    cnt += pcnt;
    sum += psum;
  }
  Acc A;
  A.cnt = cnt;
  {
    const __int128 s = (__int128)(unsigned __int128)sum + (__int128)(unsigned __int128)cnt * (__int128)base;
    A.slo = (uint64_t)s;
    A.shi = (int64_t)(s >> 64);
  }
  A.mn = MM && mx >= 0 ? (int64_t)((uint64_t)base + (uint64_t)mn) : INT64_MAX;
  A.mx = MM && mx >= 0 ? (int64_t)((uint64_t)base + (uint64_t)mx) : INT64_MIN;
  acc_wave_reduce(A);
  __syncthreads();
  Acc *part = (Acc *)ring;
  if (lane == 0) part[w] = A;
  __syncthreads();
  if (threadIdx.x == 0) {
    Acc T0 = part[0];
    for (int i = 1; i < 4; i++) acc_merge(T0, part[i]);
    partials[blockIdx.x] = AggPartial{T0.cnt, T0.slo, T0.shi, T0.mn, T0.mx};
  }
}

// Builds the words of every plane of the bit-plane image that hold rows
// [begin, end): each plane's words from begin / 32 on are made whole from the
// values (the bits of rows >= end stay zero) and never read back.  A block
// takes one piece of 8192 rows at a time: the values come in as coalesced
// 16-byte loads (singly where a load would cross `end`), their codes go to LDS
// as bytes, and thread t gathers the 32 codes of word t into one word per
// plane, four rows at a time: the multiply moves bit 0 of the four bytes of
// ((d >> j) & 0x01010101) to bits 24 .. 27.  So a block owns whole words, the
// 256 threads store 1 KiB of each plane side by side, and a piece lands at
// ScanPlanePieceByte whichever segment it is in.
// HIST: the block also counts the codes it holds into the column's histogram
// (scan_hist.h), rows [begin, end) only: the word that holds `begin` is
// rebuilt from its first row, and the rows of it before `begin` were counted
// when they came in; the padding past `end` never counts.  Thread t adds the
// codes of its word to a 32-bit LDS table, kept in kScanHistRep copies picked
// by the lane (a constant column would otherwise put all 64 lanes of every add
// on one address), and when the block's pieces are done thread c adds counter
// c, where it is not zero, to the global one: at most 256 64-bit atomics a
// block.  ScanEncodePlanes sizes the grid so that a block never counts 2^32
// rows.
#ifndef MBX_SCAN_HIST_REP
#define MBX_SCAN_HIST_REP 8
#endif
constexpr int kScanHistRep = MBX_SCAN_HIST_REP;  // a power of two, at most 64
constexpr int64_t kScanHistBlockPieces = (int64_t)1 << 18;  // pieces a block may count: 2^31 rows
template <typename T, bool HIST>
__global__ __launch_bounds__(256) void scan_encode_planes_kernel(const T *__restrict__ v, uint32_t *__restrict__ planes,
                                                                 int b, int64_t begin, int64_t end, uint64_t base,
                                                                 unsigned long long *__restrict__ hist) {
  constexpr int R = 16 / (int)sizeof(T);                   // rows per 16-byte load
  constexpr int UNITS = (int)kScanPlanePieceRows / R;      // 16-byte loads per piece
  __shared__ __attribute__((aligned(16))) uint8_t lds[kScanPlanePieceRows];
  __shared__ uint32_t tab[HIST ? 256 * kScanHistRep : 1];
  if (HIST) {
    for (int i = threadIdx.x; i < 256 * kScanHistRep; i += 256) tab[i] = 0;  // the piece loop's first barrier orders it
  }
  const int64_t w0 = begin / 32;
  const int64_t q0 = begin / kScanPlanePieceRows, q1 = (end + kScanPlanePieceRows - 1) / kScanPlanePieceRows;
  for (int64_t q = q0 + blockIdx.x; q < q1; q += gridDim.x) {
    const int64_t r0 = q * kScanPlanePieceRows;
    for (int u = threadIdx.x; u < UNITS; u += 256) {
      const int64_t r = r0 + (int64_t)u * R;
      uint32_t c[R];
      if (r + R <= end) {
        const v4i32 x = __builtin_nontemporal_load((const v4i32 *)(v + r));
        if (sizeof(T) == 8) {
          c[0] = (uint32_t)x.x - (uint32_t)base;  // the low byte of value - base needs the low words only
          c[1 % R] = (uint32_t)x.z - (uint32_t)base;
        } else {
#pragma unroll
          for (int e = 0; e < R; e++) c[e] = (uint32_t)x[e] - (uint32_t)base;
        }
      } else {
#pragma unroll
        for (int e = 0; e < R; e++) c[e] = r + e < end ? (uint32_t)(uint64_t)(int64_t)v[r + e] - (uint32_t)base : 0u;
      }
      if (sizeof(T) == 8) {
        ((uint16_t *)lds)[u] = (uint16_t)((c[0] & 0xFFu) | ((c[1 % R] & 0xFFu) << 8));
      } else {
        ((uint32_t *)lds)[u] = (c[0] & 0xFFu) | ((c[1 % R] & 0xFFu) << 8) | ((c[2 % R] & 0xFFu) << 16) | (c[3 % R] << 24);
      }
    }
    __syncthreads();
    const int64_t row = r0 + (int64_t)threadIdx.x * 32, wi = row / 32;
    if (row < end && wi >= w0) {
      uint32_t d[8];
      const uint4 lo = ((const uint4 *)lds)[threadIdx.x * 2], hi = ((const uint4 *)lds)[threadIdx.x * 2 + 1];
      d[0] = lo.x; d[1] = lo.y; d[2] = lo.z; d[3] = lo.w;
      d[4] = hi.x; d[5] = hi.y; d[6] = hi.z; d[7] = hi.w;
      for (int k = 0; k < b; k++) {
        const int j = b - 1 - k;
        uint32_t o = 0;
#pragma unroll
        for (int i = 0; i < 8; i++) o |= ((((d[i] >> j) & 0x01010101u) * 0x01020408u) >> 24) << (4 * i);
        planes[ScanPlaneWord(b, k, row)] = o;
      }
      if (HIST) {
        uint32_t *mine = tab + (threadIdx.x & (kScanHistRep - 1));
        if (row >= begin && row + 32 <= end) {
#pragma unroll
          for (int i = 0; i < 32; i++) atomicAdd(mine + ((d[i >> 2] >> (8 * (i & 3))) & 0xFFu) * kScanHistRep, 1u);
        } else {
          for (int i = 0; i < 32; i++)
            if (row + i >= begin && row + i < end) atomicAdd(mine + ((d[i >> 2] >> (8 * (i & 3))) & 0xFFu) * kScanHistRep, 1u);
        }
      }
    }
    __syncthreads();
  }
  if (HIST) {
    __syncthreads();
    if ((int)threadIdx.x < (1 << b)) {
      unsigned long long t = 0;
#pragma unroll
      for (int r = 0; r < kScanHistRep; r++) t += tab[threadIdx.x * kScanHistRep + r];
      if (t) atomicAdd(hist + threadIdx.x, t);
    }
  }
}

// The plane scan's answer from the column's code histogram (scan_hist.h): one
// block, thread c folds counter c under clo <= c <= chi into the values of an
// accumulator, and the block reduction and the one partial record are those
// the scans end with.  With emit, thread 0 then writes the one-row relation
// from the accumulator it holds (emit_one_row), where emit_agg_kernel would
// read the record back in a launch of its own.
__device__ __forceinline__ void emit_one_row(const EmitDesc &D, const Acc &T0, int32_t err);
__global__ __launch_bounds__(256) void filter_agg_hist_kernel(const unsigned long long *__restrict__ hist, int b,
                                                              uint32_t clo, uint32_t chi, int64_t base,
                                                              AggPartial *partials, EmitDesc D, int emit) {
  __shared__ Acc part[4];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  const uint32_t c = threadIdx.x;
  // (the device error word for the host tail, fetched beside the counters)
  int32_t err = 0;
  if (emit && threadIdx.x == 0 && D.host.err_dst) err = *D.host.err_src;
  const ScanHistValues hv =
      ScanHistValuesOf(c < (uint32_t)ScanHistBins(b) ? ScanHistBin(c, hist[c], clo, chi) : ScanHistNone(), base);
  Acc A;
  A.cnt = hv.cnt;
  A.slo = hv.slo;
  A.shi = hv.shi;
  A.mn = hv.mn;
  A.mx = hv.mx;
  acc_wave_reduce(A);
  if (lane == 0) part[w] = A;
  __syncthreads();
  if (threadIdx.x == 0) {
    Acc T0 = part[0];
    for (int i = 1; i < 4; i++) acc_merge(T0, part[i]);
    partials[0] = AggPartial{T0.cnt, T0.slo, T0.shi, T0.mn, T0.mx};
    if (emit) emit_one_row(D, T0, err);
  }
}

// Multi-column version of the LDS-DMA filter-aggregate.  A wave step covers
// 256 consecutive rows; each column's slice (1 KiB for int32, 2 KiB for
// int64) lands in the wave's ring slot through global_load_lds; each lane
// then owns 4 consecutive rows of every column.  A NULL-able column adds its
// step's 4 validity words (one exec-masked LDS-DMA instruction); a row counts
// only where every such column is non-NULL (the host admits a NULL-able
// aggregated column only where that is the SQL answer).
//
// Compile-time layout of filter_multi_t: NC columns, bit c of WM = column c is
// 8 bytes wide (else 4); slices at fixed offsets, then the NULL-able columns'
// 32-B validity words (runtime: which columns, at the end of the slot).
template <int NC, int WM>
struct FmCols {
  static constexpr int w(int c) { return (WM >> c) & 1 ? 8 : 4; }
  static constexpr int off(int c) { return c == 0 ? 0 : off(c - 1) + w(c - 1) * 256; }
  static constexpr int ni() { return off(NC) / 1024; }
};
template <int N>
__device__ __forceinline__ void fm_wait() {
  asm volatile("s_waitcnt vmcnt(%0)" ::"n"(N) : "memory");
}

// The column layout is a template parameter (a kernel that decided widths and
// predicate roles per column and row at run time had ≈865 instructions in its
// loop region, exec-mask branches for each short-circuit and SGPR spills; it
// won on no shape, profiles/r02_filter_multi_templated.log, and was
// removed).  Every slice read has a fixed offset and width, predicates
// combine bitwise, and only the NULL-able columns (0..NC, their validity
// words one exec-masked LDS-DMA instruction each) stay run-time: a scalar
// switch picks the exact counted vmcnt for their number.
// The host puts the aggregated column first and gives every column that is
// not a predicate the always-true range [INT64_MIN, +2^64), so a row's test
// is the same branch-free compare for every column.  MODE: 0 COUNT only,
// 1 SUM (+COUNT) accumulated in int64 (no MIN/MAX; the grid bounds the sum),
// 3 the same plus MIN/MAX in int32 (the zone map bounds |value| < 2^31),
// 2 general (run-time MIN/MAX, int128 SUM, int32 MIN/MAX).
template <int NC, int WM, int DEPTH, int MODE>
__global__ __launch_bounds__(256) void filter_multi_t_kernel(FilterMultiDesc D, int64_t n, AggPartial *partials,
                                                             int slot_bytes) {
  typedef FmCols<NC, WM> L;
  extern __shared__ __attribute__((aligned(16))) unsigned char fmt_lds[];
  constexpr int NIC = L::ni();
  const int SB = slot_bytes;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  unsigned char *ring = fmt_lds + (size_t)w * DEPTH * SB;
  int voff[NC];
  bool hv[NC];
  int64_t lo[NC];
  uint64_t span[NC];
  const unsigned char *colp[NC];
  int nvw = 0;
#pragma unroll
  for (int c = 0; c < NC; c++) {
    hv[c] = D.col[c].valid != nullptr;
    voff[c] = L::off(NC) + 32 * nvw;
    nvw += hv[c];
    lo[c] = D.col[c].lo;
    span[c] = D.col[c].span;
    colp[c] = (const unsigned char *)D.col[c].data + lane * 16;
  }
  const int64_t nsteps = n >> 8;
  const int64_t nw = (int64_t)gridDim.x * 4;
  int64_t st = (int64_t)blockIdx.x * 4 + w;
  auto issue = [&](int64_t q, int d) {
    unsigned char *dst = ring + d * SB;
#pragma unroll
    for (int c = 0; c < NC; c++) {
      const unsigned char *src = colp[c] + q * (L::w(c) * 256);
      __builtin_amdgcn_global_load_lds((const void *)src, (void *)(dst + L::off(c)), 16, 0, 2);
      if (L::w(c) == 8)
        __builtin_amdgcn_global_load_lds((const void *)(src + 1024), (void *)(dst + L::off(c) + 1024), 16, 0, 2);
    }
#pragma unroll
    for (int c = 0; c < NC; c++)
      if (hv[c] && lane < 2)
        __builtin_amdgcn_global_load_lds((const void *)(D.col[c].valid + q * 4 + lane * 2), (void *)(dst + voff[c]), 16,
                                         0, 0);
  };
  Acc A;
  A.cnt = 0; A.slo = 0; A.shi = 0; A.mn = INT64_MAX; A.mx = INT64_MIN;
  const bool mm32 = D.mm && D.mm32, mm = D.mm && !mm32, narrow = D.narrow;
  int32_t mn32 = INT32_MAX, mx32 = INT32_MIN;
  if (nsteps > 0) {
#pragma unroll
    for (int d = 0; d < DEPTH; d++) {
      int64_t q = st + d * nw;
      issue(q < nsteps ? q : 0, d);
    }
  }
  int k = 0;
  for (; st < nsteps; st += nw) {
    switch (nvw) {  // wave-uniform: the exact count of the slots issued after this one
      case 0: fm_wait<NIC * (DEPTH - 1)>(); break;
      case 1: fm_wait<(NIC + 1) * (DEPTH - 1)>(); break;
      case 2: fm_wait<(NIC + 2) * (DEPTH - 1)>(); break;
      case 3: fm_wait<(NIC + 3) * (DEPTH - 1)>(); break;
      default: fm_wait<(NIC + 4) * (DEPTH - 1)>(); break;
    }
    const unsigned char *src = ring + k * SB;
    int64_t v[NC][4];
#pragma unroll
    for (int c = 0; c < NC; c++) {
      if (L::w(c) == 8) {
        v2i64 x0 = *(const v2i64 *)(src + L::off(c) + lane * 32), x1 = *(const v2i64 *)(src + L::off(c) + lane * 32 + 16);
        v[c][0] = x0.x; v[c][1] = x0.y; v[c][2] = x1.x; v[c][3] = x1.y;
      } else {
        v4i32 x = *(const v4i32 *)(src + L::off(c) + lane * 16);
        v[c][0] = x.x; v[c][1] = x.y; v[c][2] = x.z; v[c][3] = x.w;
      }
    }
    unsigned vm = 0xFu;  // rows 4 lane + e where every NULL-able column is valid
#pragma unroll
    for (int c = 0; c < NC; c++)
      if (hv[c]) vm &= (unsigned)(*(const uint64_t *)(src + voff[c] + (lane >> 4) * 8) >> (4 * (lane & 15))) & 0xFu;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    int64_t q = st + DEPTH * nw;
    issue(q < nsteps ? q : st, k);
#pragma unroll
    for (int e = 0; e < 4; e++) {
      bool ok = (vm >> e) & 1u;
#pragma unroll
      for (int c = 0; c < NC; c++) ok = ok & ((uint64_t)(v[c][e]) - (uint64_t)(lo[c]) <= span[c]);
      const int64_t val = v[0][e];
      if constexpr (MODE == 0) {
        acc_count(A, ok);
      } else if constexpr (MODE == 1 || MODE == 3) {
        A.cnt += ok;
        A.slo += (uint64_t)(ok ? val : 0);
        if constexpr (MODE == 3) {
          mn32 = min(mn32, ok ? (int32_t)val : INT32_MAX);
          mx32 = max(mx32, ok ? (int32_t)val : INT32_MIN);
        }
      } else {
        acc_row(A, ok, val, mm, narrow);
        if (mm32) {
          mn32 = min(mn32, ok ? (int32_t)val : INT32_MAX);
          mx32 = max(mx32, ok ? (int32_t)val : INT32_MIN);
        }
      }
    }
    k = k + 1 == DEPTH ? 0 : k + 1;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (blockIdx.x == 0 && w == 0) {
    for (int64_t i = (nsteps << 8) + lane; i < n; i += 64) {
      bool ok = true;
      int64_t val = 0;
      for (int c = 0; c < D.ncol; c++) {
        int64_t x = D.col[c].phys == P_I64 ? ((const int64_t *)D.col[c].data)[i] : (int64_t)((const int32_t *)D.col[c].data)[i];
        if (D.col[c].is_pred) ok = ok && (uint64_t)(x) - (uint64_t)(D.col[c].lo) <= D.col[c].span;
        if (D.col[c].valid) ok = ok && ((D.col[c].valid[i >> 6] >> (i & 63)) & 1);
        if (c == D.agg) val = x;
      }
      if (D.agg < 0) {
        acc_count(A, ok);
      } else {
        acc_row(A, ok, val, mm, narrow);
        if (mm32) {
          mn32 = min(mn32, ok ? (int32_t)val : INT32_MAX);
          mx32 = max(mx32, ok ? (int32_t)val : INT32_MIN);
        }
      }
    }
  }
  if (mm32) {  // a count of 0 makes the emit write NULL whatever these hold
    A.mn = mn32;
    A.mx = mx32;
  }
  if (narrow) A.shi = (int64_t)A.slo >> 63;
  acc_wave_reduce(A);
  __syncthreads();
  Acc *part = (Acc *)fmt_lds;
  if (lane == 0) part[w] = A;
  __syncthreads();
  if (threadIdx.x == 0) {
    Acc T0 = part[0];
    for (int i = 1; i < 4; i++) acc_merge(T0, part[i]);
    partials[blockIdx.x] = AggPartial{T0.cnt, T0.slo, T0.shi, T0.mn, T0.mx};
  }
}

namespace {
// Ring depth by the columns' LDS-DMA instructions per step: 6 for one, 3 for
// two, 2 above (profiles/r02_filter_multi_sweep.log).
template <int NC, int WM, int MODE>
void FmtLaunchM(const FilterMultiDesc &d, int64_t nrows, AggPartial *partials, int slot, int grid, hipStream_t s) {
  constexpr int ni = FmCols<NC, WM>::ni();
  constexpr int DP = ni <= 1 ? 6 : ni == 2 ? 3 : 2;
  hipLaunchKernelGGL((filter_multi_t_kernel<NC, WM, DP, MODE>), dim3(grid), dim3(256), (size_t)4 * DP * slot, s, d,
                     nrows, partials, slot);
}
template <int NC, int WM>
void FmtLaunch(const FilterMultiDesc &d, int mode, int64_t nrows, AggPartial *partials, int slot, int grid,
               hipStream_t s) {
  if (mode == 0) FmtLaunchM<NC, WM, 0>(d, nrows, partials, slot, grid, s);
  else if (mode == 1) FmtLaunchM<NC, WM, 1>(d, nrows, partials, slot, grid, s);
  else if (mode == 3) FmtLaunchM<NC, WM, 3>(d, nrows, partials, slot, grid, s);
  else FmtLaunchM<NC, WM, 2>(d, nrows, partials, slot, grid, s);
}
template <int NC, int WM = 0>
void FmtDispatch(const FilterMultiDesc &d, int wm, int mode, int64_t nrows, AggPartial *partials, int slot, int grid,
                 hipStream_t s) {
  if constexpr (WM < (1 << NC)) {
    if (wm == WM) return FmtLaunch<NC, WM>(d, mode, nrows, partials, slot, grid, s);
    FmtDispatch<NC, WM + 1>(d, wm, mode, nrows, partials, slot, grid, s);
  }
}
}  // namespace

int FilterMultiPartials(const FilterMultiDesc &d_in, int64_t nrows, AggPartial *partials, hipStream_t s) {
  FilterMultiDesc d = d_in;
  if (d.ncol < 1 || d.ncol > FM_MAX) throw std::runtime_error("FilterMultiPartials: shape");
  int slot = 0;
  for (int c = 0; c < d.ncol; c++) slot += (d.col[c].phys == P_I64 ? 2048 : 1024) + (d.col[c].valid ? 32 : 0);
  slot = (slot + 15) & ~15;
  int grid = 0;
  auto plan = [&](int gpc) {
    grid = NumCUs() * gpc;
    int64_t need = (nrows >> 8) / 4 + 1;
    if (grid > need) grid = (int)need;
    if (grid > kMaxAggPartials) grid = kMaxAggPartials;
    // a lane sees at most (ceil(steps / waves) + 1) x 4 rows, tail included
    const int64_t waves = (int64_t)grid * 4, steps = nrows >> 8;
    const unsigned __int128 rows_per_lane = (unsigned __int128)(((steps + waves - 1) / waves + 1) * 4);
    d.narrow = d.maxabs <= (uint64_t)INT64_MAX &&
               (unsigned __int128)d.maxabs * rows_per_lane < ((unsigned __int128)1 << 63);
    const char *e32 = Knob("MBX_FA_MM32");
    d.mm32 = d.mm && d.narrow && d.maxabs < ((uint64_t)1 << 31) && !(e32 && e32[0] == '0');
  };
  auto mode_of = [&] { return d.agg < 0 ? 0 : (!d.mm && d.narrow) ? 1 : (d.mm32 && d.narrow) ? 3 : 2; };
  // Workgroups per CU: 1 for the compile-time modes (COUNT, narrow SUM, narrow
  // SUM + int32 MIN/MAX) and 3 for the general mode and one-column SUMs
  // (profiles/r02_filter_multi_modes.log).
  const char *e = Knob("MBX_FM_BLOCKS_PER_CU");
  const int gpc_env = e && *e ? atoi(e) : 0;
  if (gpc_env > 0) {
    plan(gpc_env);
  } else {
    plan(1);
    const int m1 = mode_of();
    if (m1 == 2 || (m1 == 1 && d.ncol == 1)) plan(3);
  }
  // aggregated column first; non-predicates always true
  if (d.agg > 0) {
    std::swap(d.col[0], d.col[d.agg]);
    d.agg = 0;
  }
  for (int c = 0; c < d.ncol; c++)
    if (!d.col[c].is_pred) {
      d.col[c].lo = INT64_MIN;
      d.col[c].span = ~0ull;
    }
  const int mode = mode_of();
  int wm = 0;
  for (int c = 0; c < d.ncol; c++)
    if (d.col[c].phys == P_I64) wm |= 1 << c;
  switch (d.ncol) {
    case 1: FmtDispatch<1>(d, wm, mode, nrows, partials, slot, grid, s); break;
    case 2: FmtDispatch<2>(d, wm, mode, nrows, partials, slot, grid, s); break;
    case 3: FmtDispatch<3>(d, wm, mode, nrows, partials, slot, grid, s); break;
    default: FmtDispatch<4>(d, wm, mode, nrows, partials, slot, grid, s); break;
  }
  CHECK_LAUNCH();
  return grid;
}

__global__ void init_agg_states_kernel(AggState *st, int64_t n) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    AggState z;
    z.count = 0; z.sum_lo = 0; z.sum_hi = 0;
    z.min_i = INT64_MAX; z.max_i = INT64_MIN;
    z.sum_f = 0; z.min_f = 0xFFFFFFFFFFFFFFFFull; z.max_f = 0;
    st[i] = z;
  }
}

__global__ void init_states_counts_kernel(AggState *st, int64_t n, unsigned long long *cs, int64_t nc,
                                          unsigned long long count) {
  for (int64_t i = blockIdx.x * (int64_t)blockDim.x + threadIdx.x; i < n || i < nc; i += (int64_t)gridDim.x * blockDim.x) {
    if (i < n) {
      AggState z;
      z.count = 0; z.sum_lo = 0; z.sum_hi = 0;
      z.min_i = INT64_MAX; z.max_i = INT64_MIN;
      z.sum_f = 0; z.min_f = 0xFFFFFFFFFFFFFFFFull; z.max_f = 0;
      st[i] = z;
    }
    if (i < nc) cs[i] = count;
  }
}

void InitAggStatesCounts(AggState *st, int64_t n, unsigned long long *cs, int64_t nc, hipStream_t s,
                         unsigned long long count) {
  int64_t m = n > nc ? n : nc;
  if (m <= 0) return;
  hipLaunchKernelGGL(init_states_counts_kernel, dim3(GridFor(m, 256, 1024)), dim3(256), 0, s, st, n, cs, nc, count);
  CHECK_LAUNCH();
}

void InitAggStates(AggState *st, int64_t n, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(init_agg_states_kernel, dim3(GridFor(n, 256, 1024)), dim3(256), 0, s, st, n);
  CHECK_LAUNCH();
}

// Fused filter-aggregate over one or two columns.  The LDS-DMA stream with 6
// x 1 KiB slots per wave and one 256-thread workgroup per CU (one wave per
// SIMD) takes every shape but one — 6.90 TB/s median on the 1e9-row COUNT vs
// 6.80 at depth 8 and 6.06 for the best register-load shape
// (profiles/r01_filter_sweep_lds.json, r01_filter_sweep_depth.json).  An
// aggregated column of another width than the predicate column does not fit
// its equal-width slots and runs filter_agg_kernel.
struct FaLaunch {
  bool mm;               // MIN/MAX requested
  bool narrow;           // no lane's int64 partial sum can overflow (zone map)
  bool mm32;             // MIN/MAX in int32 (zone map: |value| < 2^31)
  AggPartial *partials;  // per-workgroup records, or nullptr: atomics into st / cstar
};

template <typename T, int MODE>
static void LaunchFALds(const FaLaunch &L, const void *p, const void *a, int64_t n, int64_t lo, uint64_t span,
                        AggState *st, unsigned long long *cstar, int grid, hipStream_t s) {
#define FAL(MM, NW)                                                                                         \
  hipLaunchKernelGGL((filter_agg_lds_kernel<T, MODE, 6, MM, NW>), dim3(grid), dim3(256), 0, s, (const T *)p, \
                     (const T *)a, n, lo, span, st, cstar, L.partials)
  if (MODE == 2) FAL(0, false);
  else if (L.mm) { if (L.mm32) FAL(2, true); else if (L.narrow) FAL(1, true); else FAL(1, false); }
  else { if (L.narrow) FAL(0, true); else FAL(0, false); }
#undef FAL
  CHECK_LAUNCH();
}

// true when LaunchFilterAgg takes the LDS-DMA kernel for this shape
static bool FaUsesLds(int mode, int pphys, int aphys) { return mode != 1 || pphys == aphys; }

template <typename TP, typename TA, int MODE>
static void LaunchFilterAgg(const FaLaunch &L, const void *p, const void *a, int64_t n, int64_t lo, uint64_t span,
                            AggState *st, unsigned long long *cstar, int grid, hipStream_t s) {
  if constexpr (MODE != 1 || sizeof(TP) == sizeof(TA)) {
    LaunchFALds<TP, MODE>(L, p, a, n, lo, span, st, cstar, grid, s);
  } else {
    hipLaunchKernelGGL((filter_agg_kernel<TP, TA>), dim3(grid), dim3(256), 0, s, (const TP *)p, (const TA *)a, n, lo,
                       span, st, cstar);
    CHECK_LAUNCH();
  }
}

int FilterAggStates(const void *pcol, int pphys, int64_t lo, int64_t hi, bool has_pred, const void *acol, int aphys,
                    int64_t nrows, AggState *st, unsigned long long *cstar, int grid_blocks, hipStream_t s,
                    bool need_minmax, uint64_t sum_maxabs, AggPartial *partials) {
  if (nrows <= 0) {
    InitAggStatesCounts(st, 1, cstar, 1, s);
    return 0;
  }
  uint64_t span = has_pred ? (uint64_t)hi - (uint64_t)lo : ~0ull;
  if (!has_pred) lo = INT64_MIN;
  const int mode = acol == nullptr ? 2 : (acol == pcol ? 0 : 1);
  int grid = grid_blocks > 0 ? grid_blocks : NumCUs();
  int64_t groups = (nrows >> 2) + 1;
  if (grid > groups) grid = (int)groups;
  const bool use_partials = partials && FaUsesLds(mode, pphys, aphys) && grid <= kMaxAggPartials;
  if (!use_partials) InitAggStatesCounts(st, 1, cstar, 1, s);
  FaLaunch L;
  L.mm = need_minmax;
  L.partials = use_partials ? partials : nullptr;
  // LDS-DMA kernel: a lane sees at most (ceil(pieces / waves) + 1) pieces of
  // 16 B, i.e. that many times 2 (int64) or 4 (int32) rows, tail included.
  {
    const int64_t rp = 64 * (16 / (pphys == P_I64 ? 8 : 4));
    const int64_t waves = (int64_t)grid * 4, pieces = nrows / rp;
    const int64_t rows_per_lane = ((pieces + waves - 1) / waves + 1) * (16 / (pphys == P_I64 ? 8 : 4));
    L.narrow = sum_maxabs <= (uint64_t)INT64_MAX &&
               (unsigned __int128)sum_maxabs * (unsigned __int128)rows_per_lane < ((unsigned __int128)1 << 63);
    // MIN/MAX in int32 when the zone map bounds |value| below 2^31 (MBX_FA_MM32=0 disables)
    const char *e32 = Knob("MBX_FA_MM32");
    L.mm32 = L.narrow && sum_maxabs < ((uint64_t)1 << 31) && !(e32 && e32[0] == '0');
  }
  if (pphys == P_I64) {
    if (mode == 0) LaunchFilterAgg<int64_t, int64_t, 0>(L, pcol, acol, nrows, lo, span, st, cstar, grid, s);
    else if (mode == 2) LaunchFilterAgg<int64_t, int64_t, 2>(L, pcol, acol, nrows, lo, span, st, cstar, grid, s);
    else if (aphys == P_I64) LaunchFilterAgg<int64_t, int64_t, 1>(L, pcol, acol, nrows, lo, span, st, cstar, grid, s);
    else LaunchFilterAgg<int64_t, int32_t, 1>(L, pcol, acol, nrows, lo, span, st, cstar, grid, s);
  } else {
    if (mode == 0) LaunchFilterAgg<int32_t, int32_t, 0>(L, pcol, acol, nrows, lo, span, st, cstar, grid, s);
    else if (mode == 2) LaunchFilterAgg<int32_t, int32_t, 2>(L, pcol, acol, nrows, lo, span, st, cstar, grid, s);
    else if (aphys == P_I64) LaunchFilterAgg<int32_t, int64_t, 1>(L, pcol, acol, nrows, lo, span, st, cstar, grid, s);
    else LaunchFilterAgg<int32_t, int32_t, 1>(L, pcol, acol, nrows, lo, span, st, cstar, grid, s);
  }
  return use_partials ? grid : 0;
}

template <int F>
static void LaunchFilterAggCodes(const void *codes, int64_t base, uint32_t clo, uint32_t cspan, int form, bool sum,
                                 int64_t nrows, AggPartial *partials, int grid, hipStream_t s) {
#define FAC(MODE, FORM)                                                                                    \
  hipLaunchKernelGGL((filter_agg_codes_kernel<F, MODE, 6, FORM>), dim3(grid), dim3(256), 0, s,              \
                     (const uint32_t *)codes, nrows, clo, cspan, base, partials)
#define FAC_M(MODE)                                \
  switch (form) {                                  \
    case SC_GUARD: FAC(MODE, SC_GUARD); break;     \
    case SC_GE: FAC(MODE, SC_GE); break;           \
    case SC_LE: FAC(MODE, SC_LE); break;           \
    default: FAC(MODE, SC_BOTH); break;            \
  }
  if (!sum) { FAC_M(2) }
  else if (form == SC_PER_CODE) FAC(0, SC_PER_CODE);
  else { FAC_M(0) }
#undef FAC_M
#undef FAC
}

// Every field count ScanCodeFields can return.
#define MBX_SCAN_FIELDS(X) X(32) X(16) X(10) X(8) X(6) X(5) X(4) X(3) X(2)

int FilterAggCodes(const void *codes, int fields, int64_t base, uint32_t clo, uint32_t cspan, int form, bool sum,
                   bool need_minmax, int64_t nrows, AggPartial *partials, hipStream_t s) {
  int grid = NumCUs();
  if (grid > kMaxAggPartials) grid = kMaxAggPartials;
  const int64_t pieces = nrows / ScanPieceRows(fields) + 1;
  if ((int64_t)grid * 4 > pieces) grid = (int)((pieces + 3) / 4);
  if (sum && need_minmax) form = SC_PER_CODE;
  switch (fields) {
#define X(F) case F: LaunchFilterAggCodes<F>(codes, base, clo, cspan, form, sum, nrows, partials, grid, s); break;
    MBX_SCAN_FIELDS(X)
#undef X
    default: throw std::runtime_error("FilterAggCodes: no kernel for " + std::to_string(fields) + " fields per word");
  }
  CHECK_LAUNCH();
  return grid;
}

void ScanEncode(const void *values, int phys, void *codes, int fields, int64_t base, int64_t begin, int64_t end,
                hipStream_t s) {
  if (end <= begin) return;
  const int64_t tiles = (end - begin) / (512 * (int64_t)fields) + 1;  // a block packs 512 words per trip
  const int grid = (int)std::min<int64_t>(tiles, (int64_t)NumCUs() * 8);
  switch (fields) {
#define X(F)                                                                                                       \
  case F:                                                                                                          \
    if (phys == P_I64)                                                                                             \
      hipLaunchKernelGGL((scan_encode_kernel<int64_t, F>), dim3(grid), dim3(256), 0, s, (const int64_t *)values,   \
                         (uint32_t *)codes, begin, end, (uint64_t)base);                                           \
    else                                                                                                           \
      hipLaunchKernelGGL((scan_encode_kernel<int32_t, F>), dim3(grid), dim3(256), 0, s, (const int32_t *)values,   \
                         (uint32_t *)codes, begin, end, (uint64_t)base);                                           \
    break;
    MBX_SCAN_FIELDS(X)
#undef X
    default: throw std::runtime_error("ScanEncode: no kernel for " + std::to_string(fields) + " fields per word");
  }
  CHECK_LAUNCH();
}

template <int NP>
static void LaunchFilterAggPlanes(const void *planes, int b, int sides, uint32_t klo, uint32_t khi, int64_t base,
                                  bool sum, bool mm, int64_t nrows, AggPartial *partials, int grid, hipStream_t s) {
#define FAP(SIDES, MODE, MM)                                                                              \
  hipLaunchKernelGGL((filter_agg_planes_kernel<NP, SIDES, MODE, MM>), dim3(grid), dim3(256), 0, s,        \
                     (const uint32_t *)planes, nrows, b, klo, khi, base, partials)
#define FAP_S(MODE, MM)                   \
  switch (sides) {                        \
    case 1: FAP(1, MODE, MM); break;      \
    case 2: FAP(2, MODE, MM); break;      \
    default: FAP(3, MODE, MM); break;     \
  }
  // a COUNT(*) that tests no side reads no plane and never gets here (FilterAggPlanes)
  if (sides == 0) {
    if (mm) FAP(0, 0, true);
    else FAP(0, 0, false);
  } else if (!sum) { FAP_S(2, false) }
  else if (mm) { FAP_S(0, true) }
  else { FAP_S(0, false) }
#undef FAP_S
#undef FAP
}

int FilterAggPlanes(const void *planes, int b, int planes_read, bool ge, bool le, uint32_t clo, uint32_t chi,
                    int64_t base, bool sum, bool need_minmax, int64_t nrows, AggPartial *partials, hipStream_t s) {
  if (planes_read < 1 || planes_read > b || b > kScanPlaneMaxBits || (sum && planes_read != b) || (!sum && !ge && !le))
    throw std::runtime_error("FilterAggPlanes: no kernel for " + std::to_string(planes_read) + " of " +
                             std::to_string(b) + " planes");
  int grid = NumCUs();
  if (grid > kMaxAggPartials) grid = kMaxAggPartials;
  const int64_t pieces = nrows / kScanPlanePieceRows + 1;
  if ((int64_t)grid * 4 > pieces) grid = (int)((pieces + 3) / 4);
  const int sides = (ge ? 1 : 0) | (le ? 2 : 0), shift = b - planes_read;
  switch (planes_read) {
#define X(NP)                                                                                                  \
  case NP:                                                                                                     \
    LaunchFilterAggPlanes<NP>(planes, b, sides, clo >> shift, chi >> shift, base, sum, sum && need_minmax,     \
                              nrows, partials, grid, s);                                                       \
    break;
    X(1) X(2) X(3) X(4) X(5) X(6) X(7) X(8)
#undef X
  }
  CHECK_LAUNCH();
  return grid;
}

int FilterAggHist(const void *hist, int b, uint32_t clo, uint32_t chi, int64_t base, AggPartial *partials,
                  hipStream_t s, const EmitDesc *emit) {
  if (!hist || b < 1 || b > kScanPlaneMaxBits)
    throw std::runtime_error("FilterAggHist: no histogram of " + std::to_string(b) + "-bit codes");
  EmitDesc D;
  if (emit) D = *emit;
  else memset(&D, 0, sizeof(D));
  hipLaunchKernelGGL(filter_agg_hist_kernel, dim3(1), dim3(256), 0, s, (const unsigned long long *)hist, b, clo, chi,
                     base, partials, D, emit ? 1 : 0);
  CHECK_LAUNCH();
  return 1;
}

void ScanEncodePlanes(const void *values, int phys, void *planes, int b, int64_t base, int64_t begin, int64_t end,
                      void *hist, hipStream_t s) {
  if (end <= begin) return;
  if (b < 1 || b > kScanPlaneMaxBits || (phys != P_I64 && phys != P_I32))
    throw std::runtime_error("ScanEncodePlanes: no kernel for " + std::to_string(b) + "-bit codes of this column");
  const int64_t pieces = (end + kScanPlanePieceRows - 1) / kScanPlanePieceRows - begin / kScanPlanePieceRows;
  int grid = (int)std::min<int64_t>(pieces, (int64_t)NumCUs() * 8);
  // a block's 32-bit histogram table counts at most kScanHistBlockPieces pieces
  if (hist && pieces > grid * kScanHistBlockPieces) grid = (int)((pieces + kScanHistBlockPieces - 1) / kScanHistBlockPieces);
#define SEP(T, HIST)                                                                                        \
  hipLaunchKernelGGL((scan_encode_planes_kernel<T, HIST>), dim3(grid), dim3(256), 0, s, (const T *)values, \
                     (uint32_t *)planes, b, begin, end, (uint64_t)base, (unsigned long long *)hist)
  if (phys == P_I64) {
    if (hist) SEP(int64_t, true);
    else SEP(int64_t, false);
  } else {
    if (hist) SEP(int32_t, true);
    else SEP(int32_t, false);
  }
#undef SEP
  CHECK_LAUNCH();
}

__global__ __launch_bounds__(256) void copy_kernel(const float4 *__restrict__ in, float4 *__restrict__ out, int64_t n) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    out[i] = in[i];
}

// ---------------------------------------------------------------------------
// HBM calibration: a float4 copy and an int64 read-reduce, timed with events
// ---------------------------------------------------------------------------
template <bool NT>
__global__ __launch_bounds__(256) void read_sum_kernel(const v2i64 *__restrict__ in, int64_t n, unsigned long long *out) {
  long long acc = 0;
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i + 3 * stride < n; i += 4 * stride) {
    v2i64 a, b, c, d;
    if (NT) {
      a = __builtin_nontemporal_load(in + i);
      b = __builtin_nontemporal_load(in + i + stride);
      c = __builtin_nontemporal_load(in + i + 2 * stride);
      d = __builtin_nontemporal_load(in + i + 3 * stride);
    } else {
      a = in[i]; b = in[i + stride]; c = in[i + 2 * stride]; d = in[i + 3 * stride];
    }
    acc += a.x ^ a.y ^ b.x ^ b.y ^ c.x ^ c.y ^ d.x ^ d.y;
  }
  for (; i < n; i += stride) acc += in[i].x ^ in[i].y;
  if (acc == 0x123456789) atomicAdd(out, 1ull);  // keeps the loads live
}

// the read shape of the hot kernels: one workgroup of 4 waves per CU, each
// wave an LDS-DMA ring of DEPTH x 1 KiB slots (16 B per lane, non-temporal)
template <int DEPTH>
__global__ __launch_bounds__(256) void ring_read_kernel(const unsigned char *__restrict__ in, int64_t nsteps,
                                                        unsigned long long *flag) {
  extern __shared__ __attribute__((aligned(16))) unsigned char rr_lds[];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  unsigned char *ring = rr_lds + w * DEPTH * 1024;
  const int64_t nw = (int64_t)gridDim.x * 4;
  int64_t st = (int64_t)blockIdx.x * 4 + w;
  auto issue = [&](int64_t q, int d) {
    __builtin_amdgcn_global_load_lds((const void *)(in + q * 1024 + lane * 16), (void *)(ring + d * 1024), 16, 0, 2);
  };
#pragma unroll
  for (int d = 0; d < DEPTH; d++) issue(st + d * nw < nsteps ? st + d * nw : 0, d);
  long long acc = 0;
  int k = 0;
  for (; st < nsteps; st += nw) {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(DEPTH - 1) : "memory");
    v2i64 x = *(const v2i64 *)(ring + k * 1024 + lane * 16);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    const int64_t q = st + DEPTH * nw;
    issue(q < nsteps ? q : st, k);
    acc += x.x ^ x.y;
    k = k + 1 == DEPTH ? 0 : k + 1;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (acc == 0x123456789) atomicAdd(flag, 1ull);
}

// the read shape of C3's group_direct_lds (d2_g1): one workgroup of 4 waves
// per CU; a wave step pulls 256 rows of a 4-byte column (1 KiB) and of an
// 8-byte column (2 KiB) into a DEPTH-deep ring of 3 KiB slots; no atomics
template <int DEPTH>
__global__ __launch_bounds__(256) void ring_read2_kernel(const unsigned char *__restrict__ k4,
                                                         const unsigned char *__restrict__ v8, int64_t nsteps,
                                                         unsigned long long *flag) {
  extern __shared__ __attribute__((aligned(16))) unsigned char r2_lds[];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  unsigned char *ring = r2_lds + w * DEPTH * 3072;
  const int64_t nw = (int64_t)gridDim.x * 4;
  int64_t st = (int64_t)blockIdx.x * 4 + w;
  auto issue = [&](int64_t q, int d) {
    unsigned char *dst = ring + d * 3072;
    __builtin_amdgcn_global_load_lds((const void *)(k4 + q * 1024 + lane * 16), (void *)dst, 16, 0, 2);
    __builtin_amdgcn_global_load_lds((const void *)(v8 + q * 2048 + lane * 16), (void *)(dst + 1024), 16, 0, 2);
    __builtin_amdgcn_global_load_lds((const void *)(v8 + q * 2048 + 1024 + lane * 16), (void *)(dst + 2048), 16, 0, 2);
  };
#pragma unroll
  for (int d = 0; d < DEPTH; d++) issue(st + d * nw < nsteps ? st + d * nw : 0, d);
  long long acc = 0;
  int k = 0;
  MBX_CLK(0);
  for (; st < nsteps; st += nw) {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(3 * (DEPTH - 1)) : "memory");
    const unsigned char *src = ring + k * 3072;
    v4i32 a = *(const v4i32 *)(src + lane * 16);
    v2i64 b = *(const v2i64 *)(src + 1024 + lane * 32), c = *(const v2i64 *)(src + 1024 + lane * 32 + 16);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    const int64_t q = st + DEPTH * nw;
    issue(q < nsteps ? q : st, k);
    acc += (a.x ^ a.w) + (b.x ^ c.y);
    k = k + 1 == DEPTH ? 0 : k + 1;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  MBX_CLK(1);
  if (acc == 0x123456789) atomicAdd(flag, 1ull);
}

// 16-B copy with 4 independent loads in flight per lane, non-temporal both ways
__global__ __launch_bounds__(256) void copy_nt4_kernel(const v4i32 *__restrict__ in, v4i32 *__restrict__ out, int64_t n) {
  const int64_t stride = (int64_t)gridDim.x * blockDim.x;
  int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  for (; i + 3 * stride < n; i += 4 * stride) {
    v4i32 a = __builtin_nontemporal_load(in + i), b = __builtin_nontemporal_load(in + i + stride);
    v4i32 c = __builtin_nontemporal_load(in + i + 2 * stride), d = __builtin_nontemporal_load(in + i + 3 * stride);
    __builtin_nontemporal_store(a, out + i);
    __builtin_nontemporal_store(b, out + i + stride);
    __builtin_nontemporal_store(c, out + i + 2 * stride);
    __builtin_nontemporal_store(d, out + i + 3 * stride);
  }
  for (; i < n; i += stride) out[i] = in[i];
}

// the same ring with every slot written back out (non-temporal 16-B stores):
// the copy shape of the materialising kernels.  Stores count in vmcnt too, so
// the wait allows the DEPTH-1 younger loads and as many stores.
// HALF: only lanes 0..31 store, packed (512 B per 1 KiB read): the 2:1
// read:write mix of a compaction at ~50 % selectivity
template <int DEPTH, bool HALF>
__global__ __launch_bounds__(256) void ring_copy_kernel(const unsigned char *__restrict__ in, unsigned char *__restrict__ out,
                                                        int64_t nsteps) {
  extern __shared__ __attribute__((aligned(16))) unsigned char rc_lds[];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  unsigned char *ring = rc_lds + w * DEPTH * 1024;
  const int64_t nw = (int64_t)gridDim.x * 4;
  int64_t st = (int64_t)blockIdx.x * 4 + w;
  auto issue = [&](int64_t q, int d) {
    __builtin_amdgcn_global_load_lds((const void *)(in + q * 1024 + lane * 16), (void *)(ring + d * 1024), 16, 0, 2);
  };
#pragma unroll
  for (int d = 0; d < DEPTH; d++) issue(st + d * nw < nsteps ? st + d * nw : 0, d);
  int k = 0;
  for (; st < nsteps; st += nw) {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(2 * (DEPTH - 1)) : "memory");
    v4i32 x = *(const v4i32 *)(ring + k * 1024 + lane * 16);
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    const int64_t q = st + DEPTH * nw;
    issue(q < nsteps ? q : st, k);
    if (!HALF) __builtin_nontemporal_store(x, (v4i32 *)(out + st * 1024 + lane * 16));
    else if (lane < 32) __builtin_nontemporal_store(x, (v4i32 *)(out + st * 512 + lane * 16));
    k = k + 1 == DEPTH ? 0 : k + 1;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
}

// out: [0] float4 copy, [1] non-temporal int64 read, [2] plain read, [3] the
// hot kernels' LDS-DMA ring read, [4] unrolled non-temporal 16-B copy, [5] the
// LDS-DMA ring copy, [6] the ring copy writing half of what it reads, [7] C3's
// two-array ring read (a 4-byte and an 8-byte column, 2-deep 3 KiB slots)
// (GB/s; a copy counts its read and its write)
void HbmCalibrate(void *buf_a, void *buf_b, int64_t bytes, int iters, double out[kCalibrateShapes], hipStream_t s) {
  hipEvent_t e0, e1;
  (void)hipEventCreate(&e0);
  (void)hipEventCreate(&e1);
  unsigned long long *flag = (unsigned long long *)buf_b;
  int64_t n16 = bytes / 16;
  int grid = NumCUs() * 8;
  const int64_t nsteps = bytes / 1024;
  const int64_t nsteps3 = bytes / 3072;  // [7]: 256-row steps of 4 + 8 bytes per row
  for (int k = 0; k < kCalibrateShapes; k++) {
    float best = 1e30f;
    for (int it = 0; it < iters + 1; it++) {
      (void)hipEventRecord(e0, s);
      if (k == 0) hipLaunchKernelGGL(copy_kernel, dim3(grid), dim3(256), 0, s, (const float4 *)buf_a, (float4 *)buf_b, n16);
      else if (k == 1) hipLaunchKernelGGL(read_sum_kernel<true>, dim3(grid), dim3(256), 0, s, (const v2i64 *)buf_a, n16, flag);
      else if (k == 2) hipLaunchKernelGGL(read_sum_kernel<false>, dim3(grid), dim3(256), 0, s, (const v2i64 *)buf_a, n16, flag);
      else if (k == 3)
        hipLaunchKernelGGL(ring_read_kernel<6>, dim3(NumCUs()), dim3(256), 4 * 6 * 1024, s, (const unsigned char *)buf_a,
                           nsteps, flag);
      else if (k == 4)
        hipLaunchKernelGGL(copy_nt4_kernel, dim3(grid), dim3(256), 0, s, (const v4i32 *)buf_a, (v4i32 *)buf_b, n16);
      else if (k == 5)
        hipLaunchKernelGGL((ring_copy_kernel<6, false>), dim3(NumCUs()), dim3(256), 4 * 6 * 1024, s,
                           (const unsigned char *)buf_a, (unsigned char *)buf_b, nsteps);
      else if (k == 7)
        hipLaunchKernelGGL(ring_read2_kernel<2>, dim3(NumCUs()), dim3(256), 4 * 2 * 3072, s,
                           (const unsigned char *)buf_a, (const unsigned char *)buf_a + nsteps3 * 1024, nsteps3, flag);
      else
        hipLaunchKernelGGL((ring_copy_kernel<6, true>), dim3(NumCUs()), dim3(256), 4 * 6 * 1024, s,
                           (const unsigned char *)buf_a, (unsigned char *)buf_b, nsteps);
      (void)hipEventRecord(e1, s);
      (void)hipEventSynchronize(e1);
      float ms = 0;
      (void)hipEventElapsedTime(&ms, e0, e1);
      if (it > 0 && ms < best) best = ms;  // first launch is a warm-up
    }
    double moved = (k == 7 ? (double)nsteps3 * 3072 / (double)bytes : k == 6 ? 1.5 : k == 0 || (k >= 4 && k < 7) ? 2.0 : 1.0) *
                   (double)bytes;
    out[k] = moved / (best * 1e-3) / 1e9;
  }
  (void)hipEventDestroy(e0);
  (void)hipEventDestroy(e1);
}

// The clock stamps of the last stamped launch (diagnostic build): up to cap
// workgroups' {memtime start, realtime start, memtime end, realtime end};
// returns the count copied, 0 in the product library (no stamps compiled).
int ReadClockStamps(uint64_t *out, int cap, hipStream_t s) {
#if MBX_CLOCK_STAMPS
  const int n = std::min(cap, kClkSlots);
  if (n <= 0) return 0;
  if (hipStreamSynchronize(s) != hipSuccess) return 0;
  if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_clk_stamps), (size_t)n * 4 * 8, 0, hipMemcpyDeviceToHost) != hipSuccess)
    return 0;
  return n;
#else
  (void)out, (void)cap, (void)s;
  return 0;
#endif
}

// ---------------------------------------------------------------------------
// fused GROUP BY on a small integer key range (config C3)
// ---------------------------------------------------------------------------
// LDS table with R replicas per key: replica = lane % R, so the 64 lanes of a
// wave never hit the same address in one ds_add.  Partial sums are int64
// (the host sizes seg_rows from the column statistics so they cannot
// overflow) and are folded into int128 global slots at every segment flush.
template <typename TK, typename TV, int NV, bool MM>
__global__ __launch_bounds__(256) void group_direct_kernel(const TK *__restrict__ keys, const TV *__restrict__ v0,
                                                           const TV *__restrict__ v1, int64_t n, int64_t kmin, int nk,
                                                           int R, int64_t chunk, int64_t seg_rows,
                                                           unsigned long long *cstar, AggState *st0, AggState *st1) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  const int nslot = nk * R;
  unsigned int *cnt = (unsigned int *)lds_raw;
  long long *sum0 = (long long *)(lds_raw + ((nslot * 4 + 15) & ~15));
  long long *sum1 = sum0 + nslot;
  long long *mn0 = sum0 + (NV >= 2 ? 2 : 1) * nslot;
  long long *mx0 = mn0 + nslot;
  long long *mn1 = mx0 + nslot;
  long long *mx1 = mn1 + nslot;
  const int t = threadIdx.x, lane = t & 63;
  const int rep = lane % R;
  auto zero = [&]() {
    for (int i = t; i < nslot; i += blockDim.x) {
      cnt[i] = 0;
      if (NV >= 1) sum0[i] = 0;
      if (NV >= 2) sum1[i] = 0;
      if (MM) {
        mn0[i] = INT64_MAX; mx0[i] = INT64_MIN;
        if (NV >= 2) { mn1[i] = INT64_MAX; mx1[i] = INT64_MIN; }
      }
    }
  };
  auto flush = [&]() {
    __syncthreads();
    for (int k = t; k < nk; k += blockDim.x) {
      unsigned long long c = 0;
      i128 s0 = 0, s1 = 0;
      long long a0 = INT64_MAX, b0 = INT64_MIN, a1 = INT64_MAX, b1 = INT64_MIN;
      for (int r = 0; r < R; r++) {
        int sl = k * R + r;
        c += cnt[sl];
        if (NV >= 1) s0 += (i128)sum0[sl];
        if (NV >= 2) s1 += (i128)sum1[sl];
        if (MM) {
          a0 = mn0[sl] < a0 ? mn0[sl] : a0; b0 = mx0[sl] > b0 ? mx0[sl] : b0;
          if (NV >= 2) { a1 = mn1[sl] < a1 ? mn1[sl] : a1; b1 = mx1[sl] > b1 ? mx1[sl] : b1; }
        }
      }
      if (c) {
        atomicAdd(&cstar[k], c);
        Acc A;
        A.cnt = c;
        if (NV >= 1) {
          int64_t lo, hi;
          sp128(s0, lo, hi);
          A.slo = (uint64_t)lo; A.shi = hi; A.mn = MM ? a0 : INT64_MAX; A.mx = MM ? b0 : INT64_MIN;
          agg_state_atomic(&st0[k], A);
        }
        if (NV >= 2) {
          int64_t lo, hi;
          sp128(s1, lo, hi);
          A.slo = (uint64_t)lo; A.shi = hi; A.mn = MM ? a1 : INT64_MAX; A.mx = MM ? b1 : INT64_MIN;
          agg_state_atomic(&st1[k], A);
        }
      }
    }
    __syncthreads();
    zero();
    __syncthreads();
  };
  zero();
  __syncthreads();
  int64_t begin = (int64_t)blockIdx.x * chunk;
  int64_t end = begin + chunk < n ? begin + chunk : n;
  for (int64_t seg = begin; seg < end; seg += seg_rows) {
    int64_t seg_end = seg + seg_rows < end ? seg + seg_rows : end;
    // row-pair body (chunk/seg boundaries are multiples of 4): each load
    // instruction covers a contiguous 512 B (int32) / 1 KiB (int64) span;
    // GU pairs per lane are loaded before any LDS atomic is issued.
    constexpr int GU = 4;
    int64_t g0 = seg >> 1, g1 = seg_end >> 1;
    auto row = [&](int64_t k, int64_t a, int64_t b) {
      int sl = (int)(k - kmin) * R + rep;
      atomicAdd(&cnt[sl], 1u);
      if (NV >= 1) atomicAdd((unsigned long long *)&sum0[sl], (unsigned long long)a);
      if (NV >= 2) atomicAdd((unsigned long long *)&sum1[sl], (unsigned long long)b);
      if (MM) {
        atomicMin(&mn0[sl], (long long)a); atomicMax(&mx0[sl], (long long)a);
        if (NV >= 2) { atomicMin(&mn1[sl], (long long)b); atomicMax(&mx1[sl], (long long)b); }
      }
    };
    int64_t g = g0 + t;
    for (; g + (GU - 1) * (int64_t)blockDim.x < g1; g += GU * (int64_t)blockDim.x) {
      int64_t k0[GU], k1[GU], a0[GU], a1[GU], b0[GU], b1[GU];
#pragma unroll
      for (int u = 0; u < GU; u++) {
        int64_t gi = g + u * (int64_t)blockDim.x;
        Pair<TK, true>::load(keys, gi, k0[u], k1[u]);
        if (NV >= 1) Pair<TV, true>::load(v0, gi, a0[u], a1[u]);
        if (NV >= 2) Pair<TV, true>::load(v1, gi, b0[u], b1[u]);
      }
#pragma unroll
      for (int u = 0; u < GU; u++) {
        row(k0[u], NV >= 1 ? a0[u] : 0, NV >= 2 ? b0[u] : 0);
        row(k1[u], NV >= 1 ? a1[u] : 0, NV >= 2 ? b1[u] : 0);
      }
    }
    for (; g < g1; g += blockDim.x) {
      int64_t k0, k1, a0 = 0, a1 = 0, b0 = 0, b1 = 0;
      Pair<TK, true>::load(keys, g, k0, k1);
      if (NV >= 1) Pair<TV, true>::load(v0, g, a0, a1);
      if (NV >= 2) Pair<TV, true>::load(v1, g, b0, b1);
      row(k0, a0, b0);
      row(k1, a1, b1);
    }
    // odd last row (end is odd only at n)
    for (int64_t i = (g1 << 1) + t; i < seg_end; i += blockDim.x) {
      int sl = (int)((int64_t)keys[i] - kmin) * R + rep;
      atomicAdd(&cnt[sl], 1u);
      if (NV >= 1) atomicAdd((unsigned long long *)&sum0[sl], (unsigned long long)(int64_t)v0[i]);
      if (NV >= 2) atomicAdd((unsigned long long *)&sum1[sl], (unsigned long long)(int64_t)v1[i]);
      if (MM) {
        atomicMin(&mn0[sl], (long long)v0[i]); atomicMax(&mx0[sl], (long long)v0[i]);
        if (NV >= 2) { atomicMin(&mn1[sl], (long long)v1[i]); atomicMax(&mx1[sl], (long long)v1[i]); }
      }
    }
    flush();
  }
}

// LDS-DMA version of group_direct (the default when one flush at the end is
// overflow-safe).  A wave step covers 256 consecutive rows: the key slice and
// every value column's slice are pulled into the wave's ring slot with
// 16-B/lane global_load_lds (1 KiB per instruction, no VGPR staging); each
// lane then owns 4 consecutive rows.  Waves walk steps grid-stride.  The
// replicated LDS tables and the rings share ONE dynamic __shared__ array.
// Each row takes a ds_add_u32 for its COUNT and a ds_add_u64 for its SUM.  (A
// packed form -- the COUNT in the low bits of one ds_add_u64 per row, drained
// into registers every few thousand steps -- bounded this kernel while the
// compiler drained the ring before every LDS atomic; with the asm atomics
// below the plain form is faster: C3 1.684 vs 1.744 ms,
// profiles/r02_group_unpacked.log, so it was removed.)
// LDS atomics of the table as inline-asm ds_* ops that return nothing: the
// compiler puts an s_waitcnt vmcnt(0) in front of every atomic LDS access
// while LDS-DMA is in flight (it cannot prove the table and the ring do not
// alias), which drained the whole ring at every step.  The table is read only
// behind an explicit lgkmcnt(0) + barrier.
__device__ __forceinline__ uint32_t gd_lds(const void *p) {
  return (uint32_t)(uintptr_t)(const __attribute__((address_space(3))) void *)p;
}
__device__ __forceinline__ void gd_add_u32(unsigned int *p, unsigned int v) {
  asm volatile("ds_add_u32 %0, %1" ::"v"(gd_lds(p)), "v"(v) : "memory");
}
__device__ __forceinline__ void gd_add_u64(long long *p, unsigned long long v) {
  asm volatile("ds_add_u64 %0, %1" ::"v"(gd_lds(p)), "v"(v) : "memory");
}
__device__ __forceinline__ void gd_min_i64(long long *p, long long v) {
  asm volatile("ds_min_i64 %0, %1" ::"v"(gd_lds(p)), "v"(v) : "memory");
}
__device__ __forceinline__ void gd_max_i64(long long *p, long long v) {
  asm volatile("ds_max_i64 %0, %1" ::"v"(gd_lds(p)), "v"(v) : "memory");
}

// VN: some of the key and value columns hold NULLs (gv says which; the
// choice is wave-uniform, so it costs scalar branches, not one kernel per
// mask).  Three 32-B steps of validity words (key, value 0, value 1: 256 rows
// each) ride the ring slot after the value slices, one exec-masked glds each;
// a column without NULLs re-reads a present column's words (an L2 hit, no HBM
// bytes), so every step issues the same count of loads for the counted wait.
// COUNT(*) takes one ds_add_u32 per row; a NULL-able value column's valid rows
// are counted in its own vcnt table, and its SUM / MIN / MAX see the valid rows
// only; a row whose key is NULL goes to the last key slot (nk - 1, the NULL
// group); a predicate on a NULL-able column fails on NULL.
template <typename TK, typename TV, int NV, bool MM, int DEPTH, bool VN = false>
__global__ __launch_bounds__(256) void group_direct_lds_kernel(const TK *__restrict__ keys, const TV *__restrict__ v0,
                                                               const TV *__restrict__ v1, int64_t n, int64_t kmin,
                                                               int nk, int R, size_t ring_off,
                                                               unsigned long long *cstar, AggState *st0,
                                                               AggState *st1, GroupPreds pr, GroupValidity gv,
                                                               unsigned long long *gpart) {
  const bool KN = VN && gv.key, V0N = VN && NV >= 1 && gv.v0, V1N = VN && NV >= 2 && gv.v1;
  constexpr int NVW = VN ? 3 : 0;  // validity steps per ring slot
  const uint64_t *const anyv = VN ? (gv.key ? gv.key : gv.v0 ? gv.v0 : gv.v1) : nullptr;
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  constexpr int KB = 256 * (int)sizeof(TK), VB = 256 * (int)sizeof(TV);  // bytes per step
  constexpr int SBD = KB + NV * VB;                                        // key + value slices
  constexpr int OKV = SBD, OV0 = OKV + 32, OV1 = OV0 + 32;  // validity words
  constexpr int SB0 = SBD + 32 * NVW;
  // NLD counts the glds of a step without the optional predicate slice: with
  // one, the counted wait below is merely conservative (loads retire in order)
  constexpr int NLD = SBD / 1024 + NVW;
  // extra slices for predicate columns of their own, after the key/value slices
  int poff[GROUP_MAX_PRED];
  int PB = 0;
#pragma unroll
  for (int j = 0; j < GROUP_MAX_PRED; j++) {
    poff[j] = SB0 + PB;
    if (j < pr.n && pr.p[j].src == 1) PB += 256 * (pr.p[j].phys == P_I64 ? 8 : 4);
  }
  const int SB = SB0 + PB;
  const int nslot = nk * R;
  const int null_key = (nk - 1) * R;  // KN: the NULL group's slots
  unsigned int *cnt = (unsigned int *)lds_raw;
  unsigned long long *cnt64 = (unsigned long long *)lds_raw;  // VN: {COUNT(*), valid rows of value 0}
  long long *sum0 = (long long *)(lds_raw + ((nslot * (VN ? 8 : 4) + 15) & ~15));
  long long *sum1 = sum0 + nslot;
  long long *mn0 = sum0 + (NV >= 2 ? 2 : 1) * nslot;
  long long *mx0 = mn0 + nslot;
  long long *mn1 = mx0 + nslot;
  long long *mx1 = mn1 + nslot;
  // valid-row counts per slot of the NULL-able value columns, after the table
  // (GroupDirectLds sizes them)
  unsigned int *vcnt1 = (unsigned int *)(sum0 + (NV >= 2 ? 2 : 1) * nslot + (MM ? 2 * (NV >= 2 ? 2 : 1) * nslot : 0));
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int rep = lane % R;
  unsigned char *ring = lds_raw + ring_off + (size_t)w * DEPTH * SB;
  for (int i = t; i < nslot; i += blockDim.x) {
    if (VN) cnt64[i] = 0;
    else cnt[i] = 0;
    if (V1N) vcnt1[i] = 0;
    if (NV >= 1) sum0[i] = 0;
    if (NV >= 2) sum1[i] = 0;
    if (MM) {
      mn0[i] = INT64_MAX; mx0[i] = INT64_MIN;
      if (NV >= 2) { mn1[i] = INT64_MAX; mx1[i] = INT64_MIN; }
    }
  }
  __syncthreads();
  // one row: its key slot (the NULL group's when kv is false), COUNT(*), and
  // each value column's sum / min / max over its valid rows
  auto row = [&](int64_t k, int64_t a, int64_t b, bool kv, bool va, bool vb) {
    const int sl = (KN && !kv) ? null_key + rep : (int)(k - kmin) * R + rep;
    if (VN) {
      // branch-free: a NULL value adds 0 to its sum and the neutral element to
      // its min / max, so every lane issues the same LDS ops (no exec-mask
      // juggling per row)
      const bool a_ok = !V0N || va, b_ok = !V1N || vb;
      gd_add_u64((long long *)&cnt64[sl], 1ull + (a_ok ? (1ull << 32) : 0ull));
      if (NV >= 1) {
        gd_add_u64(&sum0[sl], a_ok ? (unsigned long long)a : 0ull);
        if (MM) { gd_min_i64(&mn0[sl], a_ok ? (long long)a : INT64_MAX); gd_max_i64(&mx0[sl], a_ok ? (long long)a : INT64_MIN); }
      }
      if (NV >= 2) {
        if (V1N) gd_add_u32(&vcnt1[sl], b_ok ? 1u : 0u);
        gd_add_u64(&sum1[sl], b_ok ? (unsigned long long)b : 0ull);
        if (MM) { gd_min_i64(&mn1[sl], b_ok ? (long long)b : INT64_MAX); gd_max_i64(&mx1[sl], b_ok ? (long long)b : INT64_MIN); }
      }
      return;
    }
    gd_add_u32(&cnt[sl], 1u);
    if (NV >= 1) {
      gd_add_u64(&sum0[sl], (unsigned long long)a);
      if (MM) { gd_min_i64(&mn0[sl], (long long)a); gd_max_i64(&mx0[sl], (long long)a); }
    }
    if (NV >= 2) {
      gd_add_u64(&sum1[sl], (unsigned long long)b);
      if (MM) { gd_min_i64(&mn1[sl], (long long)b); gd_max_i64(&mx1[sl], (long long)b); }
    }
  };
  const int64_t nsteps = n >> 8;
  const int64_t nw = (int64_t)gridDim.x * 4;
  // pr.xcd: blocks are dealt round-robin over the 8 XCDs, so block b's logical
  // index (b % 8) * (grid / 8) + b / 8 gives each XCD one contiguous eighth of
  // every grid-stride window instead of every eighth 1-KiB piece of it
  int64_t bl = blockIdx.x;
  if (pr.xcd && (gridDim.x & 7) == 0) bl = (int64_t)(blockIdx.x & 7) * (gridDim.x >> 3) + (blockIdx.x >> 3);
  int64_t st = bl * 4 + w;
  // issue one step's glds into slot d: key slice, each value slice, the validity words
  auto issue = [&](int64_t q, int d) {
    unsigned char *dst = ring + d * SB;
    const unsigned char *kp = (const unsigned char *)keys + q * KB;
#pragma unroll
    for (int j = 0; j < KB / 1024; j++)
      __builtin_amdgcn_global_load_lds((const void *)(kp + j * 1024 + lane * 16), (void *)(dst + j * 1024), 16, 0, 2);
    if (NV >= 1) {
      const unsigned char *vp = (const unsigned char *)v0 + q * VB;
#pragma unroll
      for (int j = 0; j < VB / 1024; j++)
        __builtin_amdgcn_global_load_lds((const void *)(vp + j * 1024 + lane * 16), (void *)(dst + KB + j * 1024), 16, 0, 2);
    }
    if (NV >= 2) {
      const unsigned char *vp = (const unsigned char *)v1 + q * VB;
#pragma unroll
      for (int j = 0; j < VB / 1024; j++)
        __builtin_amdgcn_global_load_lds((const void *)(vp + j * 1024 + lane * 16), (void *)(dst + KB + VB + j * 1024), 16,
                                         0, 2);
    }
    if (VN && lane < 2) {
      __builtin_amdgcn_global_load_lds((const void *)((KN ? gv.key : anyv) + q * 4 + lane * 2), (void *)(dst + OKV), 16,
                                       0, 2);
      __builtin_amdgcn_global_load_lds((const void *)((V0N ? gv.v0 : anyv) + q * 4 + lane * 2), (void *)(dst + OV0), 16,
                                       0, 2);
      __builtin_amdgcn_global_load_lds((const void *)((V1N ? gv.v1 : anyv) + q * 4 + lane * 2), (void *)(dst + OV1), 16,
                                       0, 2);
    }
#pragma unroll
    for (int j = 0; j < GROUP_MAX_PRED; j++) {
      if (j >= pr.n || pr.p[j].src != 1) continue;
      const int B = pr.p[j].phys == P_I64 ? 2048 : 1024;
      const unsigned char *pp = (const unsigned char *)pr.p[j].col + q * B;
      __builtin_amdgcn_global_load_lds((const void *)(pp + lane * 16), (void *)(dst + poff[j]), 16, 0, 2);
      if (B == 2048)
        __builtin_amdgcn_global_load_lds((const void *)(pp + 1024 + lane * 16), (void *)(dst + poff[j] + 1024), 16, 0,
                                         2);
    }
  };
  if (nsteps > 0) {
#pragma unroll
    for (int d = 0; d < DEPTH; d++) {
      int64_t q = st + d * nw;
      issue(q < nsteps ? q : 0, d);
    }
  }
  int k = 0;
  MBX_CLK(0);
  // this lane's 4 rows' bits of a step's validity words at byte offset o
  auto vbits = [&](const unsigned char *src, int o) {
    return (unsigned)(*(const uint64_t *)(src + o + (lane >> 4) * 8) >> (4 * (lane & 15))) & 0xFu;
  };
  for (; st < nsteps; st += nw) {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NLD * (DEPTH - 1)) : "memory");
    const unsigned char *src = ring + k * SB;
    int64_t kk[4], a[4], b[4];
    if (sizeof(TK) == 4) {
      v4i32 kv = *(const v4i32 *)(src + lane * 16);
      kk[0] = kv.x; kk[1] = kv.y; kk[2] = kv.z; kk[3] = kv.w;
    } else {
      v2i64 k0 = *(const v2i64 *)(src + lane * 32), k1 = *(const v2i64 *)(src + lane * 32 + 16);
      kk[0] = k0.x; kk[1] = k0.y; kk[2] = k1.x; kk[3] = k1.y;
    }
#pragma unroll
    for (int c = 0; c < NV; c++) {
      const unsigned char *vs = src + KB + c * VB;
      int64_t *o = c == 0 ? a : b;
      if (sizeof(TV) == 4) {
        v4i32 x = *(const v4i32 *)(vs + lane * 16);
        o[0] = x.x; o[1] = x.y; o[2] = x.z; o[3] = x.w;
      } else {
        v2i64 x0 = *(const v2i64 *)(vs + lane * 32), x1 = *(const v2i64 *)(vs + lane * 32 + 16);
        o[0] = x0.x; o[1] = x0.y; o[2] = x1.x; o[3] = x1.y;
      }
    }
    bool ok[4] = {true, true, true, true};
    const unsigned km = KN ? vbits(src, OKV) : 0xFu, am = V0N ? vbits(src, OV0) : 0xFu,
                   bm = V1N ? vbits(src, OV1) : 0xFu;
#pragma unroll
    for (int j = 0; j < GROUP_MAX_PRED; j++) {
      if (j >= pr.n) break;
      const GroupPred &g = pr.p[j];
      int64_t pv[4];
      if (g.src == 2) {
        pv[0] = kk[0]; pv[1] = kk[1]; pv[2] = kk[2]; pv[3] = kk[3];
      } else if (g.src == 3) {
        pv[0] = a[0]; pv[1] = a[1]; pv[2] = a[2]; pv[3] = a[3];
      } else if (g.phys != P_I64) {
        v4i32 x = *(const v4i32 *)(src + poff[j] + lane * 16);
        pv[0] = x.x; pv[1] = x.y; pv[2] = x.z; pv[3] = x.w;
      } else {
        v2i64 x0 = *(const v2i64 *)(src + poff[j] + lane * 32), x1 = *(const v2i64 *)(src + poff[j] + lane * 32 + 16);
        pv[0] = x0.x; pv[1] = x0.y; pv[2] = x1.x; pv[3] = x1.y;
      }
#pragma unroll
      for (int e = 0; e < 4; e++) ok[e] = ok[e] && (uint64_t)(pv[e]) - (uint64_t)(g.lo) <= g.span;
      // a predicate on a NULL-able key / value column fails on NULL
      const unsigned pm = g.src == 2 ? km : g.src == 3 ? am : 0xFu;
#pragma unroll
      for (int e = 0; e < 4; e++) ok[e] = ok[e] && ((pm >> e) & 1u);
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    int64_t q = st + DEPTH * nw;
    issue(q < nsteps ? q : st, k);
#pragma unroll
    for (int e = 0; e < 4; e++)
      if (ok[e])
        row(kk[e], NV >= 1 ? a[e] : 0, NV >= 2 ? b[e] : 0, ((km >> e) & 1u) != 0, ((am >> e) & 1u) != 0,
            ((bm >> e) & 1u) != 0);
    k = k + 1 == DEPTH ? 0 : k + 1;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  MBX_CLK(1);
  if (blockIdx.x == 0) {
    auto bit = [](const uint64_t *v, int64_t i) { return ((v[i >> 6] >> (i & 63)) & 1) != 0; };
    for (int64_t i = (nsteps << 8) + t; i < n; i += blockDim.x) {
      int64_t kv = (int64_t)keys[i], av = NV >= 1 ? (int64_t)v0[i] : 0;
      const bool kr = !KN || bit(gv.key, i), ar = !V0N || bit(gv.v0, i), br = !V1N || bit(gv.v1, i);
      bool okr = true;
      for (int j = 0; j < pr.n; j++) {
        const GroupPred &g = pr.p[j];
        int64_t pv = g.src == 2 ? kv : g.src == 3 ? av
                   : (g.phys == P_I64 ? ((const int64_t *)g.col)[i] : (int64_t)((const int32_t *)g.col)[i]);
        okr = okr && (uint64_t)(pv) - (uint64_t)(g.lo) <= g.span && (g.src != 3 || ar) && (g.src != 2 || kr);
      }
      if (okr) row(kv, av, NV >= 2 ? (int64_t)v1[i] : 0, kr, ar, br);
    }
  }
  asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // this thread's table atomics (asm) have landed
  __syncthreads();
  for (int kq = t; kq < nk; kq += blockDim.x) {
    unsigned long long c = 0, vc0 = 0, vc1 = 0;
    i128 s0 = 0, s1 = 0;
    long long a0 = INT64_MAX, b0 = INT64_MIN, a1 = INT64_MAX, b1 = INT64_MIN;
    for (int r = 0; r < R; r++) {
      int sl = kq * R + r;
      if (VN) {
        c += cnt64[sl] & 0xFFFFFFFFull;
        vc0 += cnt64[sl] >> 32;
      } else {
        c += cnt[sl];
      }
      if (V1N) vc1 += vcnt1[sl];
      if (NV >= 1) s0 += (i128)sum0[sl];
      if (NV >= 2) s1 += (i128)sum1[sl];
      if (MM) {
        a0 = mn0[sl] < a0 ? mn0[sl] : a0; b0 = mx0[sl] > b0 ? mx0[sl] : b0;
        if (NV >= 2) { a1 = mn1[sl] < a1 ? mn1[sl] : a1; b1 = mx1[sl] > b1 ? mx1[sl] : b1; }
      }
    }
    if (!V0N) vc0 = c;
    if (!V1N) vc1 = c;
    if (gpart) {
      // this workgroup's record of key kq (key-major: group_partials_compact
      // reads one key's records contiguously); no global atomics
      unsigned long long *o = gpart + ((size_t)kq * gridDim.x + blockIdx.x) * GroupPartialWords(NV, MM);
      o[0] = c;
      int f = 1;
      if (NV >= 1) {
        int64_t lo, hi;
        sp128(s0, lo, hi);
        o[f++] = vc0;
        o[f++] = (unsigned long long)lo; o[f++] = (unsigned long long)hi;
        if (MM) { o[f++] = (unsigned long long)a0; o[f++] = (unsigned long long)b0; }
      }
      if (NV >= 2) {
        int64_t lo, hi;
        sp128(s1, lo, hi);
        o[f++] = vc1;
        o[f++] = (unsigned long long)lo; o[f++] = (unsigned long long)hi;
        if (MM) { o[f++] = (unsigned long long)a1; o[f++] = (unsigned long long)b1; }
      }
      continue;
    }
    if (c) atomicAdd(&cstar[kq], c);
    if (NV >= 1 && vc0) {
      Acc A;
      int64_t lo, hi;
      sp128(s0, lo, hi);
      A.cnt = vc0; A.slo = (uint64_t)lo; A.shi = hi; A.mn = MM ? a0 : INT64_MAX; A.mx = MM ? b0 : INT64_MIN;
      agg_state_atomic(&st0[kq], A);
    }
    if (NV >= 2 && vc1) {
      Acc A;
      int64_t lo, hi;
      sp128(s1, lo, hi);
      A.cnt = vc1; A.slo = (uint64_t)lo; A.shi = hi; A.mn = MM ? a1 : INT64_MAX; A.mx = MM ? b1 : INT64_MIN;
      agg_state_atomic(&st1[kq], A);
    }
  }
}

GroupDirectKnobs GroupDirectKnobsFromEnv() {
  GroupDirectKnobs k;
  const char *e = Knob("MBX_GD_VARIANT");
  if (e && *e) {
    int depth, gpc;
    if (sscanf(e, "d%d_g%d", &depth, &gpc) == 2) {
      k.depth = depth;
      k.gpc = gpc;
    } else {
      k.seg = true;
    }
  }
  if (const char *er = Knob("MBX_GD_R")) k.r_cap = atoi(er);
  if (const char *ex = Knob("MBX_GD_XCD")) k.xcd = atoi(ex) != 0;
  k.atomic_flush = Knob("MBX_GD_ATOMIC_FLUSH") != nullptr;
  return k;
}

// The kernels' template arguments resolved once from the shape: f is called
// with tags of (TK, TV, NV, MM, DEPTH, VN).  COUNT only (nv == 0) has no value
// type and no MIN / MAX: TV = int64_t, MM = false.
template <typename T>
struct GdType {
  typedef T type;
};
template <typename F>
static void GroupDirectDispatch(const GroupDirectShape &sh, int depth, F &&f) {
  auto ring = [&](auto tk, auto tv, auto nv, auto mm) {
    auto vn = [&](auto d) {
      if (sh.vm) f(tk, tv, nv, mm, d, std::true_type());
      else f(tk, tv, nv, mm, d, std::false_type());
    };
    if (depth == 3) vn(std::integral_constant<int, 3>());
    else vn(std::integral_constant<int, 2>());
  };
  auto values = [&](auto tk) {
    auto cols = [&](auto tv) {
      auto minmax = [&](auto nv) {
        if (sh.mm) ring(tk, tv, nv, std::true_type());
        else ring(tk, tv, nv, std::false_type());
      };
      if (sh.nv == 1) minmax(std::integral_constant<int, 1>());
      else minmax(std::integral_constant<int, 2>());
    };
    if (sh.nv == 0) ring(tk, GdType<int64_t>(), std::integral_constant<int, 0>(), std::false_type());
    else if (sh.val_bytes == 8) cols(GdType<int64_t>());
    else cols(GdType<int32_t>());
  };
  if (sh.key_bytes == 4) values(GdType<int32_t>());
  else values(GdType<int64_t>());
}

bool GroupDirectLaunch(const GroupDirectArgs &a, const GroupDirectPlan &p, hipStream_t s) {
  const GroupDirectShape &sh = a.shape;
  const bool seg = p.form == GroupDirectForm::Segmented;
  if (!seg && p.form != GroupDirectForm::LdsOneFlush) return false;
  // the atomic forms need the states zeroed first; the records form writes
  // every one at the end (GroupPartialsCompact)
  if (a.init_state_slots > 0 && !p.records) InitAggStatesCounts(a.st0, a.init_state_slots, a.cstar, sh.nk, s);
  GroupPreds pr = a.preds;
  pr.xcd = p.xcd;
  unsigned long long *const gpart = p.records ? (unsigned long long *)a.records : nullptr;
  GroupDirectDispatch(sh, p.depth, [&](auto tk, auto tv, auto nv, auto mm, auto depth, auto vn) {
    typedef typename decltype(tk)::type TK;
    typedef typename decltype(tv)::type TV;
    constexpr int NV = decltype(nv)::value, DEPTH = decltype(depth)::value;
    constexpr bool MM = decltype(mm)::value, VN = decltype(vn)::value;
    if (seg) {
      hipLaunchKernelGGL((group_direct_kernel<TK, TV, NV, MM>), dim3(p.grid), dim3(256), p.lds_bytes, s,
                         (const TK *)a.keys, (const TV *)a.v0, (const TV *)a.v1, sh.n, a.kmin, sh.nk, p.R, p.chunk,
                         p.seg_rows, a.cstar, a.st0, a.st1);
      return;
    }
    if (p.lds_bytes > 64 * 1024)  // deep rings at one or two workgroups per CU
      (void)hipFuncSetAttribute((const void *)group_direct_lds_kernel<TK, TV, NV, MM, DEPTH, VN>,
                                hipFuncAttributeMaxDynamicSharedMemorySize, 150 * 1024);
    hipLaunchKernelGGL((group_direct_lds_kernel<TK, TV, NV, MM, DEPTH, VN>), dim3(p.grid), dim3(256), p.lds_bytes, s,
                       (const TK *)a.keys, (const TV *)a.v0, (const TV *)a.v1, sh.n, a.kmin, sh.nk, p.R, p.ring_off,
                       a.cstar, a.st0, a.st1, pr, a.valid, gpart);
  });
  CHECK_LAUNCH();
  return true;
}

// ---------------------------------------------------------------------------
// generic aggregation over compacted columns
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void reduce_column_kernel(const void *col, int phys, const uint64_t *valid, int64_t n,
                                                            AggState *st) {
  Acc A;
  A.cnt = 0; A.slo = 0; A.shi = 0; A.mn = INT64_MAX; A.mx = INT64_MIN;
  double sf = 0;
  uint64_t fmn = ~0ull, fmx = 0;
  const bool isf = phys == P_F64 || phys == P_F32;
  const bool is128 = phys == P_I128 || phys == P_U64;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    if (!bit_valid(valid, i)) continue;
    int64_t lo, hi;
    load_phys(col, phys, i, lo, hi);
    if (isf) {
      double d = __longlong_as_double(lo);
      A.cnt++;
      sf += d;
      uint64_t k = f64_order(d);
      fmn = k < fmn ? k : fmn;
      fmx = k > fmx ? k : fmx;
    } else if (is128) {
      A.cnt++;
      uint64_t nlo = A.slo + (uint64_t)lo;
      A.shi += hi + (nlo < A.slo ? 1 : 0);
      A.slo = nlo;
      // the least and the greatest HIGH word: the first half of a 128-bit MIN / MAX (reduce_minmax128_kernel)
      A.mn = hi < A.mn ? hi : A.mn;
      A.mx = hi > A.mx ? hi : A.mx;
    } else {
      acc_add(A, true, lo);
    }
  }
  // floats: reduce separately
  __shared__ double sfs[4];
  __shared__ unsigned long long fmns[4], fmxs[4];
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    sf += __shfl_xor(sf, m, 64);
    uint64_t o = shfl_xor_u64(fmn, m);
    fmn = o < fmn ? o : fmn;
    o = shfl_xor_u64(fmx, m);
    fmx = o > fmx ? o : fmx;
  }
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  if (lane == 0) {
    sfs[w] = sf;
    fmns[w] = fmn;
    fmxs[w] = fmx;
  }
  acc_block_commit(A, st, nullptr, false);
  if (threadIdx.x == 0 && isf) {
    double s = 0;
    unsigned long long a = ~0ull, b = 0;
    for (int i = 0; i < (int)(blockDim.x >> 6); i++) {
      s += sfs[i];
      a = fmns[i] < a ? fmns[i] : a;
      b = fmxs[i] > b ? fmxs[i] : b;
    }
    atomicAdd(&st->sum_f, s);
    atomicMin(&st->min_f, a);
    atomicMax(&st->max_f, b);
  }
}

void ReduceColumn(const void *col, int phys, const uint64_t *valid, int64_t n, AggState *out, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(reduce_column_kernel, dim3(GridFor(n, 256 * 16, NumCUs() * 4)), dim3(256), 0, s, col, phys, valid,
                     n, out);
  CHECK_LAUNCH();
}

// MIN / MAX of a 128-bit column, the second half (no atomic is 128 bits wide):
// reduce_column_kernel has left the least and the greatest high word in min_i /
// max_i; among the rows that have that high word the low words order the values,
// unsigned, and fold into min_f / max_f (which a 128-bit column does not use
// otherwise, and which InitAggStates leaves at ~0 / 0).
__global__ __launch_bounds__(256) void reduce_minmax128_kernel(const void *col, int phys, const uint64_t *valid,
                                                               int64_t n, AggState *st) {
  const int64_t hmin = st->min_i, hmax = st->max_i;
  uint64_t mn = ~0ull, mx = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    if (!bit_valid(valid, i)) continue;
    int64_t lo, hi;
    load_phys(col, phys, i, lo, hi);
    if (hi == hmin) mn = (uint64_t)lo < mn ? (uint64_t)lo : mn;
    if (hi == hmax) mx = (uint64_t)lo > mx ? (uint64_t)lo : mx;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    uint64_t o = shfl_xor_u64(mn, m);
    mn = o < mn ? o : mn;
    o = shfl_xor_u64(mx, m);
    mx = o > mx ? o : mx;
  }
  if ((threadIdx.x & 63) == 0) {
    atomicMin(&st->min_f, (unsigned long long)mn);
    atomicMax(&st->max_f, (unsigned long long)mx);
  }
}

void ReduceMinMax128(const void *col, int phys, const uint64_t *valid, int64_t n, AggState *out, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(reduce_minmax128_kernel, dim3(GridFor(n, 256 * 16, NumCUs() * 4)), dim3(256), 0, s, col, phys,
                     valid, n, out);
  CHECK_LAUNCH();
}

__global__ void key_range_kernel(const void *col, int phys, const uint64_t *valid, int64_t n, long long *out3) {
  long long mn = INT64_MAX, mx = INT64_MIN, c = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    if (!bit_valid(valid, i)) continue;
    int64_t lo, hi;
    load_phys(col, phys, i, lo, hi);
    mn = lo < mn ? lo : mn;
    mx = lo > mx ? lo : mx;
    c++;
  }
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    long long o = __shfl_xor(mn, m, 64);
    mn = o < mn ? o : mn;
    o = __shfl_xor(mx, m, 64);
    mx = o > mx ? o : mx;
    c += __shfl_xor(c, m, 64);
  }
  if ((threadIdx.x & 63) == 0) {
    atomicMin(&out3[0], mn);
    atomicMax(&out3[1], mx);
    atomicAdd((unsigned long long *)&out3[2], (unsigned long long)c);
  }
}

__global__ void init3_kernel(long long *o) {
  o[0] = INT64_MAX;
  o[1] = INT64_MIN;
  o[2] = 0;
}

// Zone map (min, max, non-NULL count) of an INT32 / INT64 column at HBM speed:
// the LDS-DMA ring of filter_agg_lds.  A wave step covers 256 rows: the
// step's values (1 KiB for int32, 2 KiB for int64) and, for a NULL-able
// column, its 4 validity words (one exec-masked LDS-DMA instruction) land in
// the wave's ring slot by global_load_lds, DEPTH steps in flight with a
// counted vmcnt (never 0 in the loop); each lane then owns 4 consecutive rows.
// Min / max stay in T's width.  Ring and reduction scratch share one
// __shared__ array; one atomic set per block.  Rows past the last whole step
// are done by wave 0 of block 0.  p is 16-B aligned; valid (if any) starts at
// row 0 of p.
template <typename T, bool VAL, int DEPTH>
__global__ __launch_bounds__(256) void zone_map_lds_kernel(const T *__restrict__ p, const uint64_t *__restrict__ valid,
                                                           int64_t n, long long *out3) {
  constexpr int VB = 256 * (int)sizeof(T);  // value bytes per step
  constexpr int SB = VB + (VAL ? 32 : 0);   // slot bytes
  constexpr int NI = (sizeof(T) == 8 ? 2 : 1) + (VAL ? 1 : 0);
  constexpr T TMAX = std::numeric_limits<T>::max();
  constexpr T TMIN = std::numeric_limits<T>::min();
  __shared__ __attribute__((aligned(16))) unsigned char ring[4 * DEPTH * SB];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  unsigned char *slot0 = ring + w * DEPTH * SB;
  const int64_t nsteps = n >> 8;
  const int64_t nw = (int64_t)gridDim.x * 4;
  int64_t st = (int64_t)blockIdx.x * 4 + w;
  auto issue = [&](int64_t q, int d) {
    unsigned char *dst = slot0 + d * SB;
    const unsigned char *src = (const unsigned char *)p + q * VB;
    __builtin_amdgcn_global_load_lds((const void *)(src + lane * 16), (void *)dst, 16, 0, 2);
    if (sizeof(T) == 8) __builtin_amdgcn_global_load_lds((const void *)(src + 1024 + lane * 16), (void *)(dst + 1024), 16, 0, 2);
    if (VAL && lane < 2) __builtin_amdgcn_global_load_lds((const void *)(valid + q * 4 + lane * 2), (void *)(dst + VB), 16, 0, 0);
  };
  T mn = TMAX, mx = TMIN;
  uint32_t c = 0;
  if (nsteps > 0) {
#pragma unroll
    for (int d = 0; d < DEPTH; d++) {
      const int64_t q = st + d * nw;
      issue(q < nsteps ? q : 0, d);  // keep the per-slot load count uniform (dummy step 0)
    }
  }
  int k = 0;
  for (; st < nsteps; st += nw) {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NI * (DEPTH - 1)) : "memory");
    const unsigned char *src = slot0 + k * SB;
    T v[4];
    if (sizeof(T) == 8) {
      const v2i64 a = ((const v2i64 *)src)[2 * lane], b = ((const v2i64 *)src)[2 * lane + 1];
      v[0] = (T)a.x; v[1] = (T)a.y; v[2] = (T)b.x; v[3] = (T)b.y;
    } else {
      const v4i32 a = ((const v4i32 *)src)[lane];
      v[0] = (T)a.x; v[1] = (T)a.y; v[2] = (T)a.z; v[3] = (T)a.w;
    }
    uint32_t vb = 0xFu;
    if (VAL) vb = (uint32_t)(((const uint64_t *)(src + VB))[lane >> 4] >> ((lane & 15) * 4)) & 0xFu;
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    int64_t q = st + DEPTH * nw;
    q = q < nsteps ? q : st;  // past the end: re-read the step just consumed
    issue(q, k);
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const bool ok = !VAL || ((vb >> e) & 1u);
      mn = ok && v[e] < mn ? v[e] : mn;
      mx = ok && v[e] > mx ? v[e] : mx;
      c += ok ? 1u : 0u;
    }
    k = k + 1 == DEPTH ? 0 : k + 1;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (blockIdx.x == 0 && w == 0) {
    for (int64_t i = nsteps * 256 + lane; i < n; i += 64) {
      if (VAL && !((valid[i >> 6] >> (i & 63)) & 1ull)) continue;
      const T x = p[i];
      mn = x < mn ? x : mn;
      mx = x > mx ? x : mx;
      c++;
    }
  }
  long long lmn = (long long)mn, lmx = (long long)mx;
  unsigned long long lc = c;
#pragma unroll
  for (int m = 32; m >= 1; m >>= 1) {
    long long o = __shfl_xor(lmn, m, 64);
    lmn = o < lmn ? o : lmn;
    o = __shfl_xor(lmx, m, 64);
    lmx = o > lmx ? o : lmx;
    lc += __shfl_xor(lc, m, 64);
  }
  __syncthreads();  // every wave is done with its ring slots
  long long *part = (long long *)ring;
  if (lane == 0) {
    part[3 * w] = lmn;
    part[3 * w + 1] = lmx;
    part[3 * w + 2] = (long long)lc;
  }
  __syncthreads();
  if (threadIdx.x == 0) {
    long long a = part[0], b = part[1], cc = part[2];
    for (int i = 1; i < 4; i++) {
      a = part[3 * i] < a ? part[3 * i] : a;
      b = part[3 * i + 1] > b ? part[3 * i + 1] : b;
      cc += part[3 * i + 2];
    }
    if (cc > 0) {
      atomicMin(&out3[0], a);
      atomicMax(&out3[1], b);
      atomicAdd((unsigned long long *)&out3[2], (unsigned long long)cc);
    }
  }
}

template <typename T, bool VAL>
static void LaunchZoneMap(const void *col, const uint64_t *valid, int64_t n, long long *out3, hipStream_t s) {
  const int64_t steps = n >> 8;
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>((int64_t)NumCUs(), (steps + 3) / 4));
  hipLaunchKernelGGL((zone_map_lds_kernel<T, VAL, 6>), dim3(grid), dim3(256), 0, s, (const T *)col, valid, n, out3);
}

void KeyRange(const void *col, int phys, const uint64_t *valid, int64_t n, long long *out3, hipStream_t s) {
  hipLaunchKernelGGL(init3_kernel, dim3(1), dim3(1), 0, s, out3);
  if (n <= 0) {
    CHECK_LAUNCH();
    return;
  }
  const int sz = phys == P_I64 ? 8 : phys == P_I32 ? 4 : 0;
  const uintptr_t mis = (uintptr_t)col % 16;
  if (sz && n >= 1024 && (mis == 0 || (!valid && mis % sz == 0))) {
    // an appended range may start mid-vector: its first rows go through the
    // element-wise kernel, the 16-B aligned rest through the ring
    const int64_t head = mis ? (int64_t)((16 - mis) / sz) : 0;
    if (head)
      hipLaunchKernelGGL(key_range_kernel, dim3(1), dim3(64), 0, s, col, phys, (const uint64_t *)nullptr, head, out3);
    const void *body = (const char *)col + head * sz;
    if (sz == 8) {
      if (valid) LaunchZoneMap<int64_t, true>(body, valid, n - head, out3, s);
      else LaunchZoneMap<int64_t, false>(body, nullptr, n - head, out3, s);
    } else {
      if (valid) LaunchZoneMap<int32_t, true>(body, valid, n - head, out3, s);
      else LaunchZoneMap<int32_t, false>(body, nullptr, n - head, out3, s);
    }
    CHECK_LAUNCH();
    return;
  }
  hipLaunchKernelGGL(key_range_kernel, dim3(GridFor(n, 256 * 16, NumCUs() * 4)), dim3(256), 0, s, col, phys, valid,
                     n, out3);
  CHECK_LAUNCH();
}

void ColumnStats(const void *col, int phys, const uint64_t *valid, int64_t n, long long *out3, hipStream_t s) {
  KeyRange(col, phys, valid, n, out3, s);
}

__global__ void group_assign_kernel(const void *kcol, int kphys, const uint64_t *kvalid, int64_t kmin, int64_t nslots,
                                    int64_t n, int32_t *slot_of_row, unsigned long long *count_star) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    int32_t sl;
    if (!bit_valid(kvalid, i)) sl = (int32_t)(nslots - 1);
    else {
      int64_t lo, hi;
      load_phys(kcol, kphys, i, lo, hi);
      sl = (int32_t)(lo - kmin);
    }
    slot_of_row[i] = sl;
    atomicAdd(&count_star[sl], 1ull);
  }
}

void GroupAssign(const void *kcol, int kphys, const uint64_t *kvalid, int64_t kmin, int64_t nslots, int64_t n,
                 int32_t *slot_of_row, unsigned long long *count_star, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(group_assign_kernel, dim3(GridFor(n, 256 * 8, NumCUs() * 8)), dim3(256), 0, s, kcol, kphys,
                     kvalid, kmin, nslots, n, slot_of_row, count_star);
  CHECK_LAUNCH();
}

__global__ void group_reduce_kernel(const int32_t *slot_of_row, const void *col, int phys, const uint64_t *valid,
                                    int64_t n, AggState *states) {
  const bool isf = phys == P_F64 || phys == P_F32;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    if (!bit_valid(valid, i)) continue;
    AggState *st = &states[slot_of_row[i]];
    int64_t lo, hi;
    load_phys(col, phys, i, lo, hi);
    atomicAdd(&st->count, 1ull);
    if (isf) {
      double d = __longlong_as_double(lo);
      atomicAdd(&st->sum_f, d);
      uint64_t k = f64_order(d);
      atomicMin(&st->min_f, (unsigned long long)k);
      atomicMax(&st->max_f, (unsigned long long)k);
    } else {
      unsigned long long old = atomicAdd(&st->sum_lo, (unsigned long long)lo);
      unsigned long long carry = (old + (unsigned long long)lo) < old ? 1ull : 0ull;
      atomicAdd((unsigned long long *)&st->sum_hi, (unsigned long long)hi + carry);
      // a 128-bit value (UBIGINT: 64 unsigned bits under a zero high word) orders by its
      // HIGH word first: the first half of its MIN / MAX (group_minmax128_kernel)
      const long long m = phys == P_I128 || phys == P_U64 ? hi : lo;
      atomicMin(&st->min_i, m);
      atomicMax(&st->max_i, m);
    }
  }
}

void GroupReduceColumn(const int32_t *slot_of_row, const void *col, int phys, const uint64_t *valid, int64_t n,
                       AggState *states, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(group_reduce_kernel, dim3(GridFor(n, 256 * 8, NumCUs() * 8)), dim3(256), 0, s, slot_of_row, col,
                     phys, valid, n, states);
  CHECK_LAUNCH();
}

// MIN / MAX of a 128-bit column per slot, the second half (reduce_minmax128_kernel
// with a slot per row): group_reduce_kernel has left every slot's least and
// greatest high word in min_i / max_i; the unsigned low words of the rows that
// have their slot's high word fold into min_f / max_f.
__global__ void group_minmax128_kernel(const int32_t *slot_of_row, const void *col, int phys, const uint64_t *valid,
                                       int64_t n, AggState *states) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    if (!bit_valid(valid, i)) continue;
    AggState *st = &states[slot_of_row[i]];
    int64_t lo, hi;
    load_phys(col, phys, i, lo, hi);
    if (hi == st->min_i) atomicMin(&st->min_f, (unsigned long long)lo);
    if (hi == st->max_i) atomicMax(&st->max_f, (unsigned long long)lo);
  }
}

void GroupMinMax128(const int32_t *slot_of_row, const void *col, int phys, const uint64_t *valid, int64_t n,
                    AggState *states, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(group_minmax128_kernel, dim3(GridFor(n, 256 * 8, NumCUs() * 8)), dim3(256), 0, s, slot_of_row,
                     col, phys, valid, n, states);
  CHECK_LAUNCH();
}

__global__ __launch_bounds__(1024) void compact_slots_kernel(const unsigned long long *count_star, int64_t nslots,
                                                             int32_t *slot_list, int64_t *n_out) {
  __shared__ int wsum[16];
  __shared__ long long base;
  if (threadIdx.x == 0) base = 0;
  __syncthreads();
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  for (int64_t off = 0; off < nslots; off += blockDim.x) {
    int64_t i = off + threadIdx.x;
    bool f = i < nslots && count_star[i] > 0;
    uint64_t m = __ballot(f);
    if (lane == 0) wsum[w] = __popcll(m);
    __syncthreads();
    int before = 0;
    for (int k = 0; k < w; k++) before += wsum[k];
    int total = 0;
    for (int k = 0; k < (int)(blockDim.x >> 6); k++) total += wsum[k];
    uint64_t lt = lane ? (m & ((1ull << lane) - 1ull)) : 0ull;
    if (f) slot_list[base + before + __popcll(lt)] = (int32_t)i;
    __syncthreads();
    if (threadIdx.x == 0) base += total;
    __syncthreads();
  }
  if (threadIdx.x == 0) *n_out = base;
}

__global__ void slot_flags_kernel(const unsigned long long *count_star, int64_t nslots, int32_t *flag) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nslots; i += (int64_t)gridDim.x * blockDim.x)
    flag[i] = count_star[i] > 0;
}

__global__ void slot_scatter_kernel(const int32_t *flag, const int32_t *pos, int64_t nslots, int32_t *slot_list,
                                    int64_t *n_out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < nslots; i += (int64_t)gridDim.x * blockDim.x) {
    if (flag[i]) slot_list[pos[i]] = (int32_t)i;
    if (i == nslots - 1) *n_out = (int64_t)pos[i] + flag[i];
  }
}

// Ordered list of the non-empty slots.  One workgroup for small tables; a
// device-wide scan (flags -> hipCUB exclusive sum -> scatter) for large ones.
// Writes the aggregate relation [key?, agg0, agg1, ...] from per-slot states,
// as workgroup `bid` of `nb` (emit_agg_kernel; the one workgroup of
// group_partials_compact_kernel).  Validity bitmaps are written as whole 64-bit
// words from a wave ballot (each wave owns 64 consecutive output rows), so the
// output bitmaps need no zeroing and no atomics.  part: LDS room for one Acc
// per wave (the partials reduction).
// The cell {lo, hi} of aggregate A for a slot with cstar rows and state *S
// (not read for COUNT(*)); false: the cell is NULL.
__device__ __forceinline__ bool emit_cell(const EmitAgg &A, unsigned long long cstar, const AggState *S, int64_t &lo,
                                          int64_t &hi) {
  // the integer class (the counts whatever the class) is emit_cell.h's, which
  // the host compiles too; floating-point states and 128-bit MIN / MAX are here
  const bool minmax = A.kind == 3 || A.kind == 4;
  if (A.kind <= 1 || (A.in_class != VC_F64 && !(minmax && A.wide_minmax)))
    return emit_cell_int(A.kind, A.avg_scale, cstar, S, lo, hi);
  lo = 0;
  hi = 0;
  if (!S->count) return false;
  switch (A.kind) {
    case 2: /*SUM*/ lo = f64_bits(S->sum_f); return true;
    case 3: /*MIN*/
    case 4: /*MAX*/
      if (A.in_class == VC_F64) lo = f64_bits(f64_unorder(A.kind == 3 ? S->min_f : S->max_f));
      else { lo = (int64_t)(A.kind == 3 ? S->min_f : S->max_f); hi = A.kind == 3 ? S->min_i : S->max_i; }
      return true;
    default: /*AVG*/ lo = f64_bits(S->sum_f / (double)S->count); return true;
  }
}

// The one-row relation of a fused scan from the accumulator T0 that one thread
// holds (the scan's partials merged; every aggregate reads the same integer
// column): slot 0's count and states are written as the shard combine and later
// readers expect them, and the row is emitted from registers, with no trip
// through memory in between.  With the host tail (D.host), err is the device
// error word, read by the caller while it waited for its own loads.
__device__ __forceinline__ void emit_one_row(const EmitDesc &D, const Acc &T0, int32_t err) {
  ((unsigned long long *)D.cstar)[0] = T0.cnt;
  AggState S;
  S.count = T0.cnt; S.sum_lo = T0.slo; S.sum_hi = T0.shi;
  S.min_i = T0.mn; S.max_i = T0.mx;
  S.sum_f = 0; S.min_f = 0xFFFFFFFFFFFFFFFFull; S.max_f = 0;
  const bool host = D.host.err_dst != nullptr;
  for (int j = 0; j < D.nagg; j++) {
    const EmitAgg &A = D.a[j];
    if (AggState *G = A.states) {
      G->count = S.count; G->sum_lo = S.sum_lo; G->sum_hi = S.sum_hi;
      G->min_i = S.min_i; G->max_i = S.max_i;
    }
    int64_t lo, hi;
    const bool valid = emit_cell(A, T0.cnt, &S, lo, hi);
    store_phys(A.out, A.out_phys, 0, lo, hi);
    A.valid[0] = valid ? 1u : 0u;
    if (host) {
      store_phys(D.host.out[j], A.out_phys, 0, lo, hi);
      *D.host.valid[j] = valid ? 1ull : 0ull;
    }
  }
  if (host) {
    *D.host.err_dst = err;
    __threadfence_system();
    // the ticket, last: this thread alone wrote the cells, the validity words
    // and the error word above (its callers run it on thread 0 of the one
    // workgroup that emits), so a host that sees the ticket sees them all
    __hip_atomic_store(D.host.ticket_dst, D.host.ticket, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

__device__ __forceinline__ void emit_agg_body(const EmitDesc &D, Acc *part, int64_t bid, int64_t nb) {
  if (D.npartials > 0) {
    // the one row of a fused scan (EmitOneRow) from its per-workgroup
    // partials: one workgroup, slot 0, no keys
    int32_t err = 0;
    if (threadIdx.x == 0 && D.host.err_dst) err = *D.host.err_src;
    Acc A;
    A.cnt = 0; A.slo = 0; A.shi = 0; A.mn = INT64_MAX; A.mx = INT64_MIN;
    for (int i = threadIdx.x; i < D.npartials; i += blockDim.x) {
      const AggPartial &q = D.partials[i];
      Acc B;
      B.cnt = q.cnt; B.slo = q.slo; B.shi = q.shi; B.mn = q.mn; B.mx = q.mx;
      acc_merge(A, B);
    }
    acc_wave_reduce(A);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = A;
    __syncthreads();
    if (threadIdx.x == 0) {
      Acc T0 = part[0];
      for (int i = 1; i < (int)(blockDim.x >> 6); i++) acc_merge(T0, part[i]);
      emit_one_row(D, T0, err);
    }
    return;
  }
  const int64_t n = D.slot_list ? *D.n_list : D.nslots;
  const int lane = threadIdx.x & 63;
  const int64_t stride = nb * blockDim.x;
  for (int64_t base = bid * blockDim.x + (threadIdx.x & ~63); base < n; base += stride) {
    const int64_t i = base + lane;
    const bool in = i < n;
    const int64_t sl = in ? (D.slot_list ? D.slot_list[i] : i) : 0;
    if (D.has_key) {
      bool kv = in && sl != D.null_slot;
      if (in) {
        int64_t k = D.key_msb ? (int64_t)(D.key_msb[sl] ^ 0x8000000000000000ull) : D.kmin + sl;
        if (kv) store_phys(D.key_out, D.key_phys, i, k, k >> 63);
        else store_phys(D.key_out, D.key_phys, i, 0, 0);
      }
      uint64_t m = __ballot(kv);
      if (lane == 0) {
        D.key_valid[base >> 5] = (uint32_t)m;
        if (base + 32 < n) D.key_valid[(base >> 5) + 1] = (uint32_t)(m >> 32);
      }
    }
    for (int q = 0; q < D.nkeys_c; q++) {
      const auto &K = D.kc[q];
      bool kv = in;
      if (in) {
        const int64_t code = D.code_msb ? (int64_t)(D.code_msb[sl] ^ 0x8000000000000000ull) : sl;
        const int64_t dg = (code / K.stride) % K.radix;
        kv = !(K.nullable && dg == K.radix - 1);
        const int64_t k = kv ? K.kmin + dg : 0;
        store_phys(K.out, K.phys, i, k, k >> 63);
      }
      uint64_t m = __ballot(kv);
      if (lane == 0) {
        K.valid[base >> 5] = (uint32_t)m;
        if (base + 32 < n) K.valid[(base >> 5) + 1] = (uint32_t)(m >> 32);
      }
    }
    for (int j = 0; j < D.nagg; j++) {
      const EmitAgg &A = D.a[j];
      bool valid = in;
      int64_t lo = 0, hi = 0;
      if (in) {
        if (A.kind == 0 /*COUNT_STAR*/) valid = emit_cell(A, D.cstar[sl], nullptr, lo, hi);
        else valid = emit_cell(A, 0, A.states + sl, lo, hi);
        store_phys(A.out, A.out_phys, i, lo, hi);  // (0 for a NULL cell)
        if (D.host.err_dst && i == 0) store_phys(D.host.out[j], A.out_phys, 0, lo, hi);
      }
      uint64_t m = __ballot(valid);
      if (lane == 0) {
        A.valid[base >> 5] = (uint32_t)m;
        if (base + 32 < n) A.valid[(base >> 5) + 1] = (uint32_t)(m >> 32);
        if (D.host.err_dst && base == 0) *D.host.valid[j] = m;
      }
    }
  }
  if (D.host.err_dst) {
    // the host tail: the cells and validity words above went to the mapped
    // buffer too; the error word follows them (one workgroup, one row: thread 0
    // stored every one), then the ticket, by the same thread: the launch is one
    // workgroup (EmitAggRelation refuses any other shape with a host tail), row
    // 0 is thread 0's, and so is word 0 of every bitmap, so thread 0 is the
    // tail's only writer and its release orders all of it before the ticket
    if (bid == 0 && threadIdx.x == 0) *D.host.err_dst = *D.host.err_src;
    __threadfence_system();
    if (bid == 0 && threadIdx.x == 0)
      __hip_atomic_store(D.host.ticket_dst, D.host.ticket, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_SYSTEM);
  }
}

__global__ __launch_bounds__(256) void emit_agg_kernel(EmitDesc D) {
  __shared__ Acc part[4];
  emit_agg_body(D, part, blockIdx.x, gridDim.x);
}

// The group_direct_lds partials of nb workgroups reduced per key (one wave per
// key at a time, its lanes over the records, carry-correct int128 sums), every
// key's state and COUNT(*) slot written (empty keys as the initialisation
// leaves them), then the non-empty keys compacted in key order as
// compact_slots_kernel does, from the counts kept in LDS.
template <int NV, bool MM>
__global__ __launch_bounds__(1024) void group_partials_compact_kernel(const unsigned long long *gpart, int nb, int nk,
                                                                      unsigned long long *count_star, AggState *st0,
                                                                      AggState *st1, int32_t *slot_list,
                                                                      int64_t *n_out, EmitDesc D, int emit) {
  constexpr int W = GroupPartialWords(NV, MM);
  __shared__ unsigned long long kc[kGroupPartialKeys];
  __shared__ int wsum[16];
  __shared__ Acc part[16];
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
  for (int kq = w; kq < nk; kq += nw) {
    unsigned long long c = 0;
    Acc A[NV > 0 ? NV : 1];
    for (int j = 0; j < (NV > 0 ? NV : 1); j++) {
      A[j].cnt = 0; A[j].slo = 0; A[j].shi = 0; A[j].mn = INT64_MAX; A[j].mx = INT64_MIN;
    }
#pragma unroll 4
    for (int b = lane; b < nb; b += 64) {  // (unrolled: a lane's records load together)
      const unsigned long long *o = gpart + ((size_t)kq * nb + b) * W;
      c += o[0];
      int f = 1;
#pragma unroll
      for (int j = 0; j < NV; j++) {
        Acc B;
        B.cnt = o[f]; B.slo = o[f + 1]; B.shi = (int64_t)o[f + 2];
        B.mn = MM ? (int64_t)o[f + 3] : INT64_MAX;
        B.mx = MM ? (int64_t)o[f + 4] : INT64_MIN;
        f += MM ? 5 : 3;
        acc_merge(A[j], B);
      }
    }
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) c += shfl_xor_u64(c, m);
#pragma unroll
    for (int j = 0; j < NV; j++) acc_wave_reduce(A[j]);
    if (lane == 0) {
      kc[kq] = c;
      count_star[kq] = c;
      for (int j = 0; j < 2; j++) {
        AggState z;
        z.count = 0; z.sum_lo = 0; z.sum_hi = 0;
        z.min_i = INT64_MAX; z.max_i = INT64_MIN;
        z.sum_f = 0; z.min_f = 0xFFFFFFFFFFFFFFFFull; z.max_f = 0;
        if (j < NV && A[j].cnt) {
          z.count = A[j].cnt; z.sum_lo = A[j].slo; z.sum_hi = A[j].shi;
          if (MM) { z.min_i = A[j].mn; z.max_i = A[j].mx; }
        }
        (j == 0 ? st0 : st1)[kq] = z;
      }
    }
  }
  __syncthreads();
  // compaction of the non-empty keys (one pass: nk <= blockDim.x)
  const int i = threadIdx.x;
  const bool f = i < nk && kc[i] > 0;
  const uint64_t m = __ballot(f);
  if (lane == 0) wsum[w] = __popcll(m);
  __syncthreads();
  int before = 0, total = 0;
  for (int k = 0; k < nw; k++) {
    before += k < w ? wsum[k] : 0;
    total += wsum[k];
  }
  const uint64_t lt = lane ? (m & ((1ull << lane) - 1ull)) : 0ull;
  if (f) slot_list[before + __popcll(lt)] = (int32_t)i;
  if (threadIdx.x == 0) *n_out = total;
  if (!emit) return;
  // the relation of the compacted keys (D reads the states, slot list and
  // count just written by this workgroup)
  __threadfence_block();
  __syncthreads();
  emit_agg_body(D, part, 0, 1);
}

void GroupPartialsCompact(const void *records, int blocks, int nv, bool mm, int nk, unsigned long long *count_star,
                          AggState *st0, AggState *st1, int32_t *slot_list, int64_t *n_out, hipStream_t s,
                          const EmitDesc *emit) {
  EmitDesc D;
  if (emit) D = *emit;
  else memset(&D, 0, sizeof(D));
#define GPC(NV, MM)                                                                                               \
  hipLaunchKernelGGL((group_partials_compact_kernel<NV, MM>), dim3(1), dim3(1024), 0, s,                          \
                     (const unsigned long long *)records, blocks, nk, count_star, st0, st1, slot_list, n_out, D,   \
                     emit ? 1 : 0)
  if (nv == 0) GPC(0, false);
  else if (nv == 1) { if (mm) GPC(1, true); else GPC(1, false); }
  else { if (mm) GPC(2, true); else GPC(2, false); }
#undef GPC
  CHECK_LAUNCH();
}

void CompactSlots(const unsigned long long *count_star, int64_t nslots, int32_t *slot_list, int64_t *n_out,
                  hipStream_t s) {
  if (nslots <= (1 << 16)) {
    hipLaunchKernelGGL(compact_slots_kernel, dim3(1), dim3(1024), 0, s, count_star, nslots, slot_list, n_out);
    CHECK_LAUNCH();
    return;
  }
  int32_t *flag = (int32_t *)TempAlloc((size_t)nslots * 4);
  int32_t *pos = (int32_t *)TempAlloc((size_t)nslots * 4);
  const int grid = GridFor(nslots, 256 * 4, NumCUs() * 8);
  hipLaunchKernelGGL(slot_flags_kernel, dim3(grid), dim3(256), 0, s, count_star, nslots, flag);
  CHECK_LAUNCH();
  size_t tmp = 0;
  CUB_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp, flag, pos, (int)nslots, s), "ExclusiveSum");
  void *d_tmp = TempAlloc(tmp ? tmp : 16);
  CUB_CHECK(hipcub::DeviceScan::ExclusiveSum(d_tmp, tmp, flag, pos, (int)nslots, s), "ExclusiveSum");
  hipLaunchKernelGGL(slot_scatter_kernel, dim3(grid), dim3(256), 0, s, flag, pos, nslots, slot_list, n_out);
  CHECK_LAUNCH();
  TempFree(d_tmp, tmp ? tmp : 16);
  TempFree(pos, (size_t)nslots * 4);
  TempFree(flag, (size_t)nslots * 4);
}

// ---------------------------------------------------------------------------
// sort / gather
// ---------------------------------------------------------------------------
__global__ void sort_key_kernel(const void *col, int phys, const uint64_t *valid, int64_t n, const int64_t *perm,
                                bool desc, bool nulls_first, uint64_t *keys) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t r = perm ? perm[i] : i;
    uint64_t k;
    // NULL placement is a separate stable 1-bit pass (SortKeyNull), so the
    // full 64-bit value range stays distinct here
    if (!bit_valid(valid, r)) {
      k = 0ull;
    } else {
      int64_t lo, hi;
      load_phys(col, phys, r, lo, hi);
      if (phys == P_F64 || phys == P_F32) {
        // -0.0 = +0.0 for ORDER BY (as V_CMP_F has it); f64_order itself keeps
        // them apart, which MIN / MAX rely on to round-trip the sign
        double d = __longlong_as_double(lo);
        if (d == 0) d = 0.0;
        k = f64_order(d);
      } else if (phys == P_U8 || phys == P_U16 || phys == P_U32 || phys == P_U64) k = (uint64_t)lo;
      else k = (uint64_t)lo ^ 0x8000000000000000ull;
      if (desc) k = ~k;
    }
    (void)nulls_first;
    keys[i] = k;
  }
}

void SortKeyU64(const void *col, int phys, const uint64_t *valid, int64_t n, const int64_t *perm, bool desc,
                bool nulls_first, uint64_t *keys, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(sort_key_kernel, dim3(GridFor(n, 256 * 4, NumCUs() * 8)), dim3(256), 0, s, col, phys, valid, n,
                     perm, desc, nulls_first, keys);
  CHECK_LAUNCH();
}

void SortPairs(uint64_t *keys_in, int64_t *vals_in, uint64_t *keys_out, int64_t *vals_out, int64_t n, hipStream_t s,
               int end_bit) {
  if (n <= 0) return;
  size_t tmp = 0;
  CUB_CHECK(hipcub::DeviceRadixSort::SortPairs(nullptr, tmp, keys_in, keys_out, vals_in, vals_out, (int)n, 0, end_bit, s),
            "SortPairs");
  void *d_tmp = nullptr;
  d_tmp = TempAlloc(tmp);
  CUB_CHECK(hipcub::DeviceRadixSort::SortPairs(d_tmp, tmp, keys_in, keys_out, vals_in, vals_out, (int)n, 0, end_bit, s),
            "SortPairs");
  TempFree(d_tmp, tmp);
}

// 1-bit NULL-placement key: the last (most significant) pass of each ORDER BY key
__global__ void sort_key_null_kernel(const uint64_t *valid, int64_t n, const int64_t *perm, bool nulls_first,
                                     uint64_t *keys) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    bool isnull = !bit_valid(valid, perm ? perm[i] : i);
    keys[i] = (isnull != nulls_first) ? 1ull : 0ull;
  }
}

void SortKeyNull(const uint64_t *valid, int64_t n, const int64_t *perm, bool nulls_first, uint64_t *keys,
                 hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(sort_key_null_kernel, dim3(GridFor(n, 256 * 4, NumCUs() * 8)), dim3(256), 0, s, valid, n, perm,
                     nulls_first, keys);
  CHECK_LAUNCH();
}

// VARCHAR ORDER BY: LSD over 8-byte chunks.  Chunk p of a string is its bytes
// [8p, 8p+8) big-endian, zero-padded (so a prefix sorts first); sorting the
// chunks from last to first with stable passes gives byte-wise (C collation)
// order.
__global__ void sort_key_str_kernel(const int64_t *offsets, const char *chars, const uint64_t *valid, int64_t n,
                                    const int64_t *perm, int64_t chunk, bool desc, uint64_t *keys) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t r = perm ? perm[i] : i;
    uint64_t k = 0;
    if (bit_valid(valid, r)) {
      int64_t b = offsets[r], e = offsets[r + 1];
      for (int j = 0; j < 8; j++) {
        int64_t at = b + chunk * 8 + j;
        k = (k << 8) | (at < e ? (uint8_t)chars[at] : 0u);
      }
      if (desc) k = ~k;
    }
    keys[i] = k;
  }
}

void SortKeyStr(const int64_t *offsets, const char *chars, const uint64_t *valid, int64_t n, const int64_t *perm,
                int64_t chunk, bool desc, uint64_t *keys, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(sort_key_str_kernel, dim3(GridFor(n, 256 * 4, NumCUs() * 8)), dim3(256), 0, s, offsets, chars,
                     valid, n, perm, chunk, desc, keys);
  CHECK_LAUNCH();
}

__global__ void str_max_len_kernel(const int64_t *offsets, int64_t n, unsigned long long *out) {
  unsigned long long m = 0;
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    unsigned long long l = (unsigned long long)(offsets[i + 1] - offsets[i]);
    m = l > m ? l : m;
  }
  for (int o = 32; o > 0; o >>= 1) {
    unsigned long long x = __shfl_xor(m, o);
    m = x > m ? x : m;
  }
  if ((threadIdx.x & 63) == 0) atomicMax(out, m);
}

void StrMaxLen(const int64_t *offsets, int64_t n, unsigned long long *out, hipStream_t s) {
  (void)hipMemsetAsync(out, 0, 8, s);
  if (n <= 0) return;
  hipLaunchKernelGGL(str_max_len_kernel, dim3(GridFor(n, 256 * 4, NumCUs() * 4)), dim3(256), 0, s, offsets, n, out);
  CHECK_LAUNCH();
}

__global__ void iota_kernel(int64_t *p, int64_t n, int64_t start) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    p[i] = start + i;
}

void Iota(int64_t *p, int64_t n, int64_t start, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(iota_kernel, dim3(GridFor(n, 256 * 4, NumCUs() * 8)), dim3(256), 0, s, p, n, start);
  CHECK_LAUNCH();
}

__global__ void gather_fixed_kernel(const void *in, int phys, const uint64_t *in_valid, const int64_t *idx, int64_t n,
                                    void *out, uint32_t *out_valid) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t r = idx[i];
    int64_t lo, hi;
    load_phys(in, phys, r, lo, hi);
    if (phys == P_F32) {  // keep exact float bits
      ((float *)out)[i] = ((const float *)in)[r];
    } else if (phys == P_INTERVAL) {
      ((int64_t *)out)[2 * i] = ((const int64_t *)in)[2 * r];
      ((int64_t *)out)[2 * i + 1] = ((const int64_t *)in)[2 * r + 1];
    } else {
      store_phys(out, phys, i, lo, hi);
    }
    if (out_valid && bit_valid(in_valid, r)) atomicOr(&out_valid[i >> 5], 1u << (i & 31));
  }
}

void GatherFixed(const void *in, int phys, const uint64_t *in_valid, const int64_t *idx, int64_t n, void *out,
                 uint32_t *out_valid, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(gather_fixed_kernel, dim3(GridFor(n, 256 * 4, NumCUs() * 8)), dim3(256), 0, s, in, phys, in_valid,
                     idx, n, out, out_valid);
  CHECK_LAUNCH();
}

__global__ void gather_slots_kernel(const unsigned char *in, int eb, const int32_t *idx, int64_t n, unsigned char *out) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const unsigned char *src = in + (int64_t)idx[i] * eb;
    unsigned char *dst = out + i * eb;
    for (int k = 0; k < eb; k++) dst[k] = src[k];
  }
}

void GatherSlots(const void *in, int elem_bytes, const int32_t *idx, int64_t n, void *out, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(gather_slots_kernel, dim3(GridFor(n, 256, 1024)), dim3(256), 0, s, (const unsigned char *)in,
                     elem_bytes, idx, n, (unsigned char *)out);
  CHECK_LAUNCH();
}

// ---------------------------------------------------------------------------
// strings
// ---------------------------------------------------------------------------
__global__ void str_len_kernel(const int64_t *codes, const uint64_t *valid, int64_t n, const int64_t *src_off,
                               const int64_t *pool_off, int64_t *lens) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    int64_t c = codes[i];
    int64_t L = 0;
    if (bit_valid(valid, i)) {
      if (c >= 0) L = src_off[c + 1] - src_off[c];
      else L = pool_off[-c] - pool_off[-c - 1];
    }
    lens[i] = L;
  }
}

void StringLengths(const int64_t *codes, const uint64_t *valid, int64_t n, const int64_t *src_off,
                   const int64_t *pool_off, int64_t *lens, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(str_len_kernel, dim3(GridFor(n, 256 * 4, NumCUs() * 8)), dim3(256), 0, s, codes, valid, n, src_off,
                     pool_off, lens);
  CHECK_LAUNCH();
}

void ScanLengths(const int64_t *lens, int64_t *offsets, int64_t n, hipStream_t s) {
  // offsets[0] = 0, offsets[i+1] = inclusive sum
  (void)hipMemsetAsync(offsets, 0, sizeof(int64_t), s);
  if (n <= 0) return;
  size_t tmp = 0;
  CUB_CHECK(hipcub::DeviceScan::InclusiveSum(nullptr, tmp, lens, offsets + 1, (int)n, s), "InclusiveSum");
  void *d_tmp = nullptr;
  d_tmp = TempAlloc(tmp);
  CUB_CHECK(hipcub::DeviceScan::InclusiveSum(d_tmp, tmp, lens, offsets + 1, (int)n, s), "InclusiveSum");
  TempFree(d_tmp, tmp);
}

__global__ void str_copy_kernel(const int64_t *codes, const uint64_t *valid, int64_t n, const int64_t *src_off,
                                const char *src_chars, const int64_t *pool_off, const char *pool_chars,
                                const int64_t *out_off, char *out_chars) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    if (!bit_valid(valid, i)) continue;
    int64_t c = codes[i];
    const char *src;
    int64_t L;
    if (c >= 0) {
      src = src_chars + src_off[c];
      L = src_off[c + 1] - src_off[c];
    } else {
      src = pool_chars + pool_off[-c - 1];
      L = pool_off[-c] - pool_off[-c - 1];
    }
    char *dst = out_chars + out_off[i];
    for (int64_t k = 0; k < L; k++) dst[k] = src[k];
  }
}

void StringCopy(const int64_t *codes, const uint64_t *valid, int64_t n, const int64_t *src_off, const char *src_chars,
                const int64_t *pool_off, const char *pool_chars, const int64_t *out_off, char *out_chars,
                hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(str_copy_kernel, dim3(GridFor(n, 256 * 4, NumCUs() * 8)), dim3(256), 0, s, codes, valid, n,
                     src_off, src_chars, pool_off, pool_chars, out_off, out_chars);
  CHECK_LAUNCH();
}

// ---------------------------------------------------------------------------
// ingest helpers
// ---------------------------------------------------------------------------
template <typename T>
__global__ void synth_kernel(T *out, int64_t n, uint64_t seed, int64_t start, uint64_t m, int64_t add) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    out[i] = (T)((int64_t)(splitmix64(seed + (uint64_t)(start + i)) % m) + add);
}

void Synth(void *out, int phys, int64_t n, int64_t seed, int64_t start, int64_t m, int64_t add, hipStream_t s) {
  if (n <= 0) return;
  int grid = GridFor(n, 256 * 8, NumCUs() * 8);
  if (phys == P_I32)
    hipLaunchKernelGGL(synth_kernel<int32_t>, dim3(grid), dim3(256), 0, s, (int32_t *)out, n, (uint64_t)seed, start,
                       (uint64_t)m, add);
  else
    hipLaunchKernelGGL(synth_kernel<int64_t>, dim3(grid), dim3(256), 0, s, (int64_t *)out, n, (uint64_t)seed, start,
                       (uint64_t)m, add);
  CHECK_LAUNCH();
}

__global__ void bitmap_append_kernel(uint64_t *dst, int64_t dst_off, const uint64_t *src, int64_t n) {
  // one thread per destination word touched
  int64_t first = dst_off >> 6, last = (dst_off + n - 1) >> 6;
  for (int64_t wi = first + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; wi <= last;
       wi += (int64_t)gridDim.x * blockDim.x) {
    uint64_t word = 0;
    int64_t b0 = wi << 6;
    for (int k = 0; k < 64; k++) {
      int64_t db = b0 + k;
      if (db < dst_off || db >= dst_off + n) {
        word |= dst[wi] & (1ull << k);
        continue;
      }
      int64_t sb = db - dst_off;
      uint64_t bit = src ? ((src[sb >> 6] >> (sb & 63)) & 1ull) : 1ull;
      word |= bit << k;
    }
    dst[wi] = word;
  }
}

void BitmapAppend(uint64_t *dst, int64_t dst_off, const uint64_t *src, int64_t n, hipStream_t s) {
  if (n <= 0) return;
  int64_t words = ((dst_off + n - 1) >> 6) - (dst_off >> 6) + 1;
  hipLaunchKernelGGL(bitmap_append_kernel, dim3(GridFor(words, 256, 4096)), dim3(256), 0, s, dst, dst_off, src, n);
  CHECK_LAUNCH();
}

void CopyKernel(const void *in, void *out, int64_t nbytes, hipStream_t s) {
  int64_t n = nbytes / 16;
  hipLaunchKernelGGL(copy_kernel, dim3(NumCUs() * 8), dim3(256), 0, s, (const float4 *)in, (float4 *)out, n);
  CHECK_LAUNCH();
}

}  // namespace dev
}  // namespace mbx

namespace mbx {
namespace dev {

void EmitAggRelation(const EmitDesc &d, hipStream_t s) {
  if (d.host.err_dst && (d.nslots != 1 || d.slot_list))
    throw std::runtime_error("EmitAggRelation: the host tail takes exactly one row");
  if (d.host.err_dst && (!d.host.ticket_dst || !d.host.ticket))
    throw std::runtime_error("EmitAggRelation: a host tail without a ticket");
  hipLaunchKernelGGL(emit_agg_kernel, dim3(d.npartials > 0 ? 1 : GridFor(d.nslots, 256, 1024)), dim3(256), 0, s, d);
  CHECK_LAUNCH();
}

// ---------------------------------------------------------------------------
// hash GROUP BY
// ---------------------------------------------------------------------------
// The table's arithmetic -- the hash of a key row, the entry packing, the
// insert walk -- is group_hash.h, shared with the host
// (tests/plan_harness/group_hash.cpp).

// key value as (up to) 128 bits; floats normalised so -0.0 groups with 0.0
// and every NaN with every other NaN
__device__ __forceinline__ void key_bits(const HashKeyCol &c, int64_t r, uint64_t &w0, uint64_t &w1) {
  int64_t lo, hi;
  load_phys(c.data, c.phys, r, lo, hi);
  w0 = (c.phys == P_F64 || c.phys == P_F32) ? GroupFloatBits((uint64_t)lo) : (uint64_t)lo;
  w1 = (uint64_t)hi;
}

__device__ uint64_t row_hash(const HashKeys &K, int64_t r) {
  uint64_t h = kGroupHashSeed;
  for (int j = 0; j < K.nk; j++) {
    const HashKeyCol &c = K.k[j];
    if (!bit_valid(c.validity, r)) {
      h = GroupHashNull(h);
      continue;
    }
    if (c.phys == P_STR) {
      const int64_t b = c.offsets[r], e = c.offsets[r + 1];
      h = GroupHashString(h, c.chars + b, e - b);
    } else {
      uint64_t w0, w1;
      key_bits(c, r, w0, w1);
      h = GroupHashWords(h, w0, w1);
    }
  }
  return h;
}

__device__ bool rows_equal(const HashKeys &K, int64_t a, int64_t b) {
  for (int j = 0; j < K.nk; j++) {
    const HashKeyCol &c = K.k[j];
    bool va = bit_valid(c.validity, a), vb = bit_valid(c.validity, b);
    if (va != vb) return false;
    if (!va) continue;
    if (c.phys == P_STR) {
      const int64_t ab = c.offsets[a], ae = c.offsets[a + 1], bb = c.offsets[b], be = c.offsets[b + 1];
      if (!GroupStringsEqual(c.chars + ab, ae - ab, c.chars + bb, be - bb)) return false;
    } else {
      uint64_t a0, a1, b0, b1;
      key_bits(c, a, a0, a1);
      key_bits(c, b, b0, b1);
      if (a0 != b0 || a1 != b1) return false;
    }
  }
  return true;
}

__global__ __launch_bounds__(256) void hash_insert_kernel(HashKeys K, int64_t n, unsigned long long *table,
                                                          uint64_t mask, int32_t *entry_of, int32_t *err) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
    const int64_t got = GroupInsert(
        row_hash(K, r), r, mask,
        [&](uint64_t e) -> uint64_t {
          return __hip_atomic_load(&table[e], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        },
        [&](uint64_t e, uint64_t expected, uint64_t desired) -> uint64_t {
          return atomicCAS(&table[e], (unsigned long long)expected, (unsigned long long)desired);
        },
        [&](int64_t other) { return rows_equal(K, other, r); });
    if (got < 0) atomicCAS(err, 0, E_HASH_FULL);  // cannot happen with cap >= 2n; never loops forever
    entry_of[r] = got < 0 ? 0 : (int32_t)got;
  }
}

__global__ void hash_occupancy_kernel(const unsigned long long *table, int64_t cap, int32_t *flag) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cap; i += (int64_t)gridDim.x * blockDim.x)
    flag[i] = table[i] != kGroupEmpty;
}

// pos = exclusive scan of the occupancy flags: entry e (occupied) -> group pos[e]
__global__ void hash_groups_kernel(const unsigned long long *table, const int32_t *flag, const int32_t *pos,
                                   int64_t cap, int32_t *gid_of_entry, int64_t *rep_row, int64_t *ngroups) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cap; i += (int64_t)gridDim.x * blockDim.x) {
    if (flag[i]) {
      gid_of_entry[i] = pos[i];
      rep_row[pos[i]] = GroupEntryRow(table[i]);
    }
    if (i == cap - 1) *ngroups = (int64_t)pos[i] + flag[i];
  }
}

__global__ void hash_slots_kernel(int32_t *slot_of_row, const int32_t *gid_of_entry, int64_t n,
                                  unsigned long long *count_star) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x) {
    int32_t g = gid_of_entry[slot_of_row[r]];
    slot_of_row[r] = g;
    if (count_star) atomicAdd(&count_star[g], 1ull);
  }
}

__global__ void count_slots_kernel(const int32_t *slot_of_row, int64_t n, unsigned long long *count_star) {
  for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < n; r += (int64_t)gridDim.x * blockDim.x)
    atomicAdd(&count_star[slot_of_row[r]], 1ull);
}

void CountSlots(const int32_t *slot_of_row, int64_t n, unsigned long long *count_star, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(count_slots_kernel, dim3(GridFor(n, 256 * 4, NumCUs() * 8)), dim3(256), 0, s, slot_of_row, n,
                     count_star);
  CHECK_LAUNCH();
}

void HashGroupAssign(const HashKeys &k, int64_t n, unsigned long long *table, int64_t cap, int32_t *slot_of_row,
                     int32_t *gid_of_entry, int64_t *rep_row, unsigned long long *count_star, int64_t *ngroups,
                     int32_t *err, hipStream_t s) {
  // table must hold kGroupEmpty, count_star zeros (caller); gid_of_entry doubles as scan scratch
  if (n <= 0) {
    (void)hipMemsetAsync(ngroups, 0, 8, s);
    return;
  }
  const int grid = GridFor(n, 256 * 4, NumCUs() * 8);
  hipLaunchKernelGGL(hash_insert_kernel, dim3(grid), dim3(256), 0, s, k, n, table, (uint64_t)(cap - 1), slot_of_row,
                     err);
  CHECK_LAUNCH();
  int32_t *flag = nullptr, *pos = nullptr;
  flag = (int32_t *)TempAlloc((size_t)cap * 4);
  pos = (int32_t *)TempAlloc((size_t)cap * 4);
  const int cgrid = GridFor(cap, 256 * 4, NumCUs() * 8);
  hipLaunchKernelGGL(hash_occupancy_kernel, dim3(cgrid), dim3(256), 0, s, table, cap, flag);
  CHECK_LAUNCH();
  size_t tmp = 0;
  CUB_CHECK(hipcub::DeviceScan::ExclusiveSum(nullptr, tmp, flag, pos, (int)cap, s), "ExclusiveSum");
  void *d_tmp = nullptr;
  d_tmp = TempAlloc(tmp ? tmp : 16);
  CUB_CHECK(hipcub::DeviceScan::ExclusiveSum(d_tmp, tmp, flag, pos, (int)cap, s), "ExclusiveSum");
  hipLaunchKernelGGL(hash_groups_kernel, dim3(cgrid), dim3(256), 0, s, table, flag, pos, cap, gid_of_entry, rep_row,
                     ngroups);
  CHECK_LAUNCH();
  hipLaunchKernelGGL(hash_slots_kernel, dim3(grid), dim3(256), 0, s, slot_of_row, gid_of_entry, n, count_star);
  CHECK_LAUNCH();
  TempFree(d_tmp, tmp ? tmp : 16);
  TempFree(pos, (size_t)cap * 4);
  TempFree(flag, (size_t)cap * 4);
}

__global__ __launch_bounds__(256) void host_copy_kernel(HostCopyDesc D) {
  if ((int)blockIdx.x < D.nseg) {
    const HostCopySeg g = D.seg[blockIdx.x];
    const int64_t words = ((((uintptr_t)g.src | (uintptr_t)g.dst) & 7) == 0) ? g.bytes >> 3 : 0;
    const uint64_t *s8 = (const uint64_t *)g.src;
    uint64_t *d8 = (uint64_t *)g.dst;
    for (int64_t i = threadIdx.x; i < words; i += blockDim.x) d8[i] = s8[i];
    const uint8_t *s1 = (const uint8_t *)g.src;
    uint8_t *d1 = (uint8_t *)g.dst;
    for (int64_t i = (words << 3) + threadIdx.x; i < g.bytes; i += blockDim.x) d1[i] = s1[i];
  }
  if (blockIdx.x == 0 && threadIdx.x == 0) *D.err_dst = *D.err_src;
  __threadfence_system();
}

void HostCopy(const HostCopyDesc &d, hipStream_t s) {
  hipLaunchKernelGGL(host_copy_kernel, dim3(d.nseg > 0 ? d.nseg : 1), dim3(256), 0, s, d);
  CHECK_LAUNCH();
}

// Arrow wire layout of one fixed-width column (reference duckdb_native.c
// :2572-2797, the *_nullable getters): values with NULL slots zeroed, then one
// validity byte per row (1 = valid).  Rows are independent; each thread does
// one row per grid-stride step, so loads and stores are coalesced.
template <typename T>
__global__ void arrow_wire_kernel(const T *__restrict__ src, const uint64_t *__restrict__ valid, int64_t n,
                                  T *__restrict__ vals, uint8_t *__restrict__ vbytes) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
    const bool ok = valid == nullptr || ((valid[i >> 6] >> (i & 63)) & 1);
    vals[i] = ok ? src[i] : (T)0;
    if (vbytes) vbytes[i] = ok ? 1 : 0;
  }
}

void ArrowWire(const void *src, const uint64_t *valid, int64_t n, int width, void *vals, uint8_t *vbytes,
               hipStream_t s) {
  if (n <= 0) return;
  const dim3 g(GridFor(n, 256 * 4, 4096)), b(256);
  switch (width) {
    case 1: hipLaunchKernelGGL(arrow_wire_kernel<uint8_t>, g, b, 0, s, (const uint8_t *)src, valid, n, (uint8_t *)vals, vbytes); break;
    case 4: hipLaunchKernelGGL(arrow_wire_kernel<uint32_t>, g, b, 0, s, (const uint32_t *)src, valid, n, (uint32_t *)vals, vbytes); break;
    case 8: hipLaunchKernelGGL(arrow_wire_kernel<uint64_t>, g, b, 0, s, (const uint64_t *)src, valid, n, (uint64_t *)vals, vbytes); break;
    default: return;
  }
  CHECK_LAUNCH();
}

__global__ void rebase_kernel(const int64_t *src, int64_t *dst, int64_t n, int64_t delta) {
  for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x)
    dst[i] = src[i] + delta;
}

void RebaseOffsets(const int64_t *src, int64_t *dst, int64_t n, int64_t delta, hipStream_t s) {
  if (n <= 0) return;
  hipLaunchKernelGGL(rebase_kernel, dim3(GridFor(n, 256 * 4, 4096)), dim3(256), 0, s, src, dst, n, delta);
  CHECK_LAUNCH();
}


// ---------------------------------------------------------------------------
// Filter -> compaction, two streaming passes (see device.h).  A one-pass form
// with a decoupled look-back over 2048/4096-row tiles measured slower on this
// chip (sel 4.1-9.8 ms vs 2-pass JIT 5.3 ms at 1e9 rows): a tile routinely
// finishes loading before its predecessor (4 predecessor polls per tile), so
// every workgroup waits out the slowest recent load while holding its slot.
// Both passes here stream with no inter-workgroup waits.
// ---------------------------------------------------------------------------

// pass 1: NI LDS-DMA instructions per wave step (1 per KiB of predicate
// slices, 1 per nullable column for its 4 validity words), DEPTH steps in flight
template <int NI, int DEPTH>
__global__ __launch_bounds__(256) void filter_bits_lds_kernel(FilterMultiDesc D, int64_t n, unsigned long long *bits,
                                                              int slot_bytes) {
  extern __shared__ __attribute__((aligned(16))) unsigned char fb_lds[];
  const int SB = slot_bytes;
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  unsigned char *ring = fb_lds + (size_t)w * DEPTH * SB;
  int off[FM_MAX], voff[FM_MAX];
  {
    int o = 0;
#pragma unroll
    for (int c = 0; c < FM_MAX; c++) {
      off[c] = o;
      if (c < D.ncol) o += D.col[c].phys == P_I64 ? 2048 : 1024;
    }
#pragma unroll
    for (int c = 0; c < FM_MAX; c++) {
      voff[c] = o;
      if (c < D.ncol && D.col[c].valid) o += 32;
    }
  }
  const int64_t nsteps = n >> 8;
  const int64_t nw = (int64_t)gridDim.x * 4;
  int64_t st = (int64_t)blockIdx.x * 4 + w;
  auto issue = [&](int64_t q, int d) {
    unsigned char *dst = ring + d * SB;
#pragma unroll
    for (int c = 0; c < FM_MAX; c++) {
      if (c >= D.ncol) break;
      const int B = D.col[c].phys == P_I64 ? 2048 : 1024;
      const unsigned char *src = (const unsigned char *)D.col[c].data + q * B;
      __builtin_amdgcn_global_load_lds((const void *)(src + lane * 16), (void *)(dst + off[c]), 16, 0, 2);
      if (B == 2048)
        __builtin_amdgcn_global_load_lds((const void *)(src + 1024 + lane * 16), (void *)(dst + off[c] + 1024), 16, 0, 2);
      // the step's 4 validity words: lanes 0-1, 16 B each (exec-masked, still one vmcnt)
      if (D.col[c].valid && lane < 2)
        __builtin_amdgcn_global_load_lds((const void *)(D.col[c].valid + q * 4 + lane * 2), (void *)(dst + voff[c]), 16,
                                         0, 0);
    }
  };
  // one step's 4 ballot words: lanes 0..3 store a word each (32 contiguous bytes)
  auto emit = [&](int64_t step, const bool ok[4]) {
    unsigned long long b[4];
#pragma unroll
    for (int e = 0; e < 4; e++) b[e] = __ballot(ok[e]);
    const unsigned long long mine = lane == 0 ? b[0] : lane == 1 ? b[1] : lane == 2 ? b[2] : b[3];
    if (lane < 4) __builtin_nontemporal_store(mine, bits + step * 4 + lane);
  };
  if (nsteps > 0) {
#pragma unroll
    for (int d = 0; d < DEPTH; d++) {
      int64_t q = st + d * nw;
      issue(q < nsteps ? q : 0, d);
    }
  }
  int k = 0;
  for (; st < nsteps; st += nw) {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NI * (DEPTH - 1)) : "memory");
    const unsigned char *src = ring + k * SB;
    int64_t v[FM_MAX][4];
    unsigned vm = 0xFu;  // rows 4 lane + e whose predicate columns are all non-NULL
#pragma unroll
    for (int c = 0; c < FM_MAX; c++) {
      if (c >= D.ncol) break;
      if (D.col[c].phys == P_I64) {
        v2i64 x0 = *(const v2i64 *)(src + off[c] + lane * 32), x1 = *(const v2i64 *)(src + off[c] + lane * 32 + 16);
        v[c][0] = x0.x; v[c][1] = x0.y; v[c][2] = x1.x; v[c][3] = x1.y;
      } else {
        v4i32 x = *(const v4i32 *)(src + off[c] + lane * 16);
        v[c][0] = x.x; v[c][1] = x.y; v[c][2] = x.z; v[c][3] = x.w;
      }
      if (D.col[c].valid)
        vm &= (unsigned)(*(const uint64_t *)(src + voff[c] + (lane >> 4) * 8) >> (4 * (lane & 15))) & 0xFu;
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    int64_t q = st + DEPTH * nw;
    issue(q < nsteps ? q : st, k);
    bool ok[4];
#pragma unroll
    for (int e = 0; e < 4; e++) {
      ok[e] = (vm >> e) & 1u;
#pragma unroll
      for (int c = 0; c < FM_MAX; c++)
        if (c < D.ncol) ok[e] = ok[e] && (uint64_t)(v[c][e]) - (uint64_t)(D.col[c].lo) <= D.col[c].span;
    }
    emit(st, ok);
    k = k + 1 == DEPTH ? 0 : k + 1;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  // the partial last step (n % 256 rows): block 0, wave 0, scalar loads
  if (blockIdx.x == 0 && w == 0 && (n & 255)) {
    bool ok[4];
#pragma unroll
    for (int e = 0; e < 4; e++) {
      const int64_t i = (nsteps << 8) + 4 * lane + e;
      ok[e] = i < n;
      for (int c = 0; c < D.ncol && ok[e]; c++) {
        const int64_t x = D.col[c].phys == P_I64 ? ((const int64_t *)D.col[c].data)[i]
                                                 : (int64_t)((const int32_t *)D.col[c].data)[i];
        ok[e] = (uint64_t)(x) - (uint64_t)(D.col[c].lo) <= D.col[c].span &&
                (!D.col[c].valid || ((D.col[c].valid[i >> 6] >> (i & 63)) & 1));
      }
    }
    emit(nsteps, ok);
  }
}

void FilterBits(const FilterMultiDesc &d, int64_t nrows, unsigned long long *bits, hipStream_t s) {
  if (nrows <= 0) return;
  int ni = 0, slot = 0;
  for (int c = 0; c < d.ncol; c++) {
    ni += d.col[c].phys == P_I64 ? 2 : 1;
    slot += d.col[c].phys == P_I64 ? 2048 : 1024;
    if (d.col[c].valid) {
      ni++;
      slot += 32;
    }
  }
  slot = (slot + 15) & ~15;
  int gpc = 3;
  if (const char *e = Knob("MBX_FB_BLOCKS_PER_CU")) gpc = atoi(e) > 0 ? atoi(e) : 3;
  int grid = NumCUs() * gpc;
  const int64_t need = (nrows >> 8) / 4 + 1;
  if (grid > need) grid = (int)need;
#define FB(L, DP)                                                                                           \
  hipLaunchKernelGGL((filter_bits_lds_kernel<L, DP>), dim3(grid), dim3(256), (size_t)4 * DP * slot, s, d, \
                     nrows, bits, slot)
  switch (ni) {  // the executor keeps ni <= 8
    case 1: FB(1, 6); break;
    case 2: FB(2, 3); break;
    case 3: FB(3, 2); break;
    case 4: FB(4, 2); break;
    case 5: FB(5, 2); break;
    case 6: FB(6, 2); break;
    case 7: FB(7, 2); break;
    default: FB(8, 2); break;
  }
#undef FB
  CHECK_LAUNCH();
}

// Validity of the compacted rows.  A wave owns a chunk of CV_CHUNK (8) consecutive
// 256-row steps and prefetches the chunk's ballot words, validity words and
// step offsets with one load each per lane.  Per step, each lane writes the
// validity bytes of its selected rows (rows 4 lane + e) at their rank into the
// wave's 256-byte LDS staging row; four ballots over the staged bytes give the
// step's 256-bit run of output validity (run word q = ballot of bytes 64 q + lane).
// The run lands at bit offset[step] of the output through a carry word kept
// across the chunk's steps, so output words are written once with plain
// stores; only a chunk's first word (when a previous chunk may share it) and
// its final carry are ORed atomically: device-scope atomics leave the XCD's L2
// and are slow, so they are kept to about two per chunk.
#define CV_CHUNK 8
__device__ __forceinline__ uint64_t readlane64(uint64_t x, int l) {
  const uint32_t lo = __builtin_amdgcn_readlane((int)(uint32_t)x, l);
  const uint32_t hi = __builtin_amdgcn_readlane((int)(uint32_t)(x >> 32), l);
  return (uint64_t)hi << 32 | lo;
}

__global__ __launch_bounds__(256) void compact_validity_kernel(const unsigned long long *bits, const int64_t *offs,
                                                               int64_t n, const uint64_t *vin, uint64_t *vout) {
  __shared__ __attribute__((aligned(16))) uint8_t stage_lds[4][256];
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  uint8_t *stage = stage_lds[w];
  const uint64_t lt = (1ull << lane) - 1;
  const int64_t steps = (n + 255) >> 8, nwords = (n + 63) >> 6;
  const int64_t nchunks = (steps + CV_CHUNK - 1) / CV_CHUNK;
  for (int64_t ch = (int64_t)blockIdx.x * 4 + w; ch < nchunks; ch += (int64_t)gridDim.x * 4) {
    const int64_t s0 = ch * CV_CHUNK;
    // the chunk's 4 x 32 ballot words and validity words: 2 of each per lane
    const int64_t bw = 4 * s0 + 2 * lane;
    const bool in0 = bw < 4 * steps, in1 = bw + 1 < 4 * steps;
    const uint64_t pb0 = in0 ? bits[bw] : 0, pb1 = in1 ? bits[bw + 1] : 0;
    const uint64_t pv0 = bw < nwords ? vin[bw] : 0, pv1 = bw + 1 < nwords ? vin[bw + 1] : 0;
    const int64_t po = lane < CV_CHUNK && s0 + lane < steps ? offs[s0 + lane] : 0;
    int64_t carry_idx = -1, first_word = -1;
    uint64_t carry_val = 0;
    bool first_shared = false;
    auto put = [&](int64_t W, uint64_t val) {  // one complete (or final) output word
      if (W == first_word && first_shared) {
        if (val) atomicOr((unsigned long long *)&vout[W], (unsigned long long)val);
      } else {
        vout[W] = val;
      }
    };
    for (int j = 0; j < CV_CHUNK && s0 + j < steps; j++) {
      const uint64_t b0 = readlane64(pb0, 2 * j), b1 = readlane64(pb1, 2 * j);
      const uint64_t b2 = readlane64(pb0, 2 * j + 1), b3 = readlane64(pb1, 2 * j + 1);
      const int cnt = __popcll(b0) + __popcll(b1) + __popcll(b2) + __popcll(b3);
      if (cnt == 0) continue;  // wave-uniform
      const int64_t o = readlane64((uint64_t)po, j);
      // this lane's validity word: chunk word 4 j + (lane >> 4), held by lane (4 j + (lane >> 4)) / 2
      const int src = (4 * j + (lane >> 4)) >> 1;
      const uint64_t v0 = __shfl(pv0, src), v1 = __shfl(pv1, src);
      const uint64_t vword = ((lane >> 4) & 1) ? v1 : v0;
      const unsigned m = (unsigned)((b0 >> lane) & 1) | (unsigned)((b1 >> lane) & 1) << 1 |
                         (unsigned)((b2 >> lane) & 1) << 2 | (unsigned)((b3 >> lane) & 1) << 3;
      const int r0 = __popcll(b0 & lt) + __popcll(b1 & lt) + __popcll(b2 & lt) + __popcll(b3 & lt);
      const unsigned vb = (unsigned)(vword >> (4 * (lane & 15))) & 0xFu;
      int r = r0;
#pragma unroll
      for (int e = 0; e < 4; e++)
        if ((m >> e) & 1u) stage[r++] = (uint8_t)((vb >> e) & 1u);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      uint64_t R[4];  // run word q, bit i = staged byte 64 q + i
#pragma unroll
      for (int qw = 0; qw < 4; qw++) R[qw] = __ballot(64 * qw + lane < cnt && stage[64 * qw + lane]);
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // staging reads done before the next step's writes
      const int64_t w0 = o >> 6, w1 = (o + cnt - 1) >> 6;
      if (first_word < 0) {
        first_word = w0;
        first_shared = (o & 63) != 0;
      }
      if (carry_idx >= 0 && carry_idx != w0) {  // the carry word is complete
        if (lane == 0) put(carry_idx, carry_val);
        carry_idx = -1;
      }
      const int64_t W = w0 + lane;
      uint64_t val = 0;
      if (lane <= 4 && W <= w1) {
        const int64_t sh = 64 * W - o;  // run bit at output bit 64 W; in [-63, 256)
        if (sh < 0) {
          val = R[0] << (-sh);
        } else {
          const int qw = (int)(sh >> 6), rb = (int)(sh & 63);
          const uint64_t a0 = qw == 0 ? R[0] : qw == 1 ? R[1] : qw == 2 ? R[2] : R[3];
          const uint64_t a1 = qw == 0 ? R[1] : qw == 1 ? R[2] : qw == 2 ? R[3] : 0;
          val = rb ? (a0 >> rb) | (a1 << (64 - rb)) : a0;
        }
        if (W == carry_idx) val |= carry_val;
        if (W < w1) put(W, val);
      }
      carry_val = readlane64(val, (int)(w1 - w0));
      carry_idx = w1;
    }
    if (carry_idx >= 0 && lane == 0 && carry_val)  // the next chunk may share it
      atomicOr((unsigned long long *)&vout[carry_idx], (unsigned long long)carry_val);
  }
}

void CompactValidity(const unsigned long long *bits, const int64_t *step_offsets, int64_t nrows,
                     const uint64_t *valid_in, uint64_t *valid_out, hipStream_t s) {
  if (nrows <= 0) return;
  const int64_t chunks = ((nrows + 255) >> 8) / CV_CHUNK + 1;
  hipLaunchKernelGGL(compact_validity_kernel, dim3(GridFor(chunks, 4, NumCUs() * 32)), dim3(256), 0, s, bits,
                     step_offsets, nrows, valid_in, valid_out);
  CHECK_LAUNCH();
}

// pass 2: NLD KiB of output slices per wave step
template <int NLD, int DEPTH>
__global__ __launch_bounds__(256) void compact_lds_kernel(CompactDesc D, int64_t n, const unsigned long long *bits,
                                                          const int64_t *offs) {
  extern __shared__ __attribute__((aligned(16))) unsigned char cp_lds[];
  constexpr int SB = NLD * 1024 + 64;  // output slices + the step's metadata (4 ballot words, offset pair)
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  unsigned char *ring = cp_lds + (size_t)w * DEPTH * SB;
  unsigned char *stage = cp_lds + (size_t)4 * DEPTH * SB + (size_t)w * 2048;  // 256 rows x 8 B per wave
  int off[FC_MAX_OUT];
  {
    int o = 0;
#pragma unroll
    for (int c = 0; c < FC_MAX_OUT; c++) {
      off[c] = o;
      if (c < D.nout) o += D.ow[c] * 256;
    }
  }
  const uint64_t lt = (1ull << lane) - 1;
  const int64_t nsteps = n >> 8;
  const int64_t nw = (int64_t)gridDim.x * 4;
  int64_t st = (int64_t)blockIdx.x * 4 + w;
  // one step into slot d: every output slice, then the metadata in one
  // exec-masked LDS-DMA (lanes 0-1: the 32 B of ballot words, lane 2: the
  // 16-B aligned offset pair holding offs[q]) — NLD + 1 loads per step
  auto issue = [&](int64_t q, int d) {
    unsigned char *dst = ring + d * SB;
#pragma unroll
    for (int c = 0; c < FC_MAX_OUT; c++) {
      if (c >= D.nout) break;
      const int B = D.ow[c] * 256;
      const unsigned char *src = (const unsigned char *)D.src[c] + q * B;
      __builtin_amdgcn_global_load_lds((const void *)(src + lane * 16), (void *)(dst + off[c]), 16, 0, 2);
      if (B == 2048)
        __builtin_amdgcn_global_load_lds((const void *)(src + 1024 + lane * 16), (void *)(dst + off[c] + 1024), 16, 0, 2);
    }
    const unsigned char *msrc = lane < 2 ? (const unsigned char *)(bits + q * 4) + lane * 16
                                         : (const unsigned char *)(offs + (q & ~(int64_t)1));
    if (lane < 3) __builtin_amdgcn_global_load_lds((const void *)msrc, (void *)(dst + NLD * 1024), 16, 0, 0);
  };
  if (nsteps > 0) {
#pragma unroll
    for (int d = 0; d < DEPTH; d++) {
      int64_t q = st + d * nw;
      issue(q < nsteps ? q : 0, d);
    }
  }
  int k = 0;
  for (; st < nsteps; st += nw) {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"((NLD + 1) * (DEPTH - 1)) : "memory");
    const unsigned char *src = ring + k * SB;
    const unsigned long long *meta = (const unsigned long long *)(src + NLD * 1024);
    const unsigned long long b0 = meta[0], b1 = meta[1], b2 = meta[2], b3 = meta[3];
    const int64_t o0 = (int64_t)meta[4 + (st & 1)];
    int64_t v[FC_MAX_OUT][4];
#pragma unroll
    for (int c = 0; c < FC_MAX_OUT; c++) {
      if (c >= D.nout) break;
      if (D.ow[c] == 8) {
        v2i64 x0 = *(const v2i64 *)(src + off[c] + lane * 32), x1 = *(const v2i64 *)(src + off[c] + lane * 32 + 16);
        v[c][0] = x0.x; v[c][1] = x0.y; v[c][2] = x1.x; v[c][3] = x1.y;
      } else {
        v4i32 x = *(const v4i32 *)(src + off[c] + lane * 16);
        v[c][0] = x.x; v[c][1] = x.y; v[c][2] = x.z; v[c][3] = x.w;
      }
    }
    asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
    int64_t q = st + DEPTH * nw;
    issue(q < nsteps ? q : st, k);
    const unsigned m = (unsigned)((b0 >> lane) & 1) | (unsigned)((b1 >> lane) & 1) << 1 |
                       (unsigned)((b2 >> lane) & 1) << 2 | (unsigned)((b3 >> lane) & 1) << 3;
    // rank of this lane's first selected row inside the step; step total
    const int r0 = __popcll(b0 & lt) + __popcll(b1 & lt) + __popcll(b2 & lt) + __popcll(b3 & lt);
    const int cnt = __popcll(b0) + __popcll(b1) + __popcll(b2) + __popcll(b3);
    // each column: selected values -> the wave's staging area at their rank,
    // then consecutive lanes store consecutive rows
#pragma unroll
    for (int c = 0; c < FC_MAX_OUT; c++) {
      if (c >= D.nout) break;
      int r = r0;
      if (D.ow[c] == 8) {
#pragma unroll
        for (int e = 0; e < 4; e++)
          if ((m >> e) & 1u) ((int64_t *)stage)[r++] = v[c][e];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        for (int i = lane; i < cnt; i += 64) ((int64_t *)D.dst[c])[o0 + i] = ((const int64_t *)stage)[i];
      } else {
#pragma unroll
        for (int e = 0; e < 4; e++)
          if ((m >> e) & 1u) ((int32_t *)stage)[r++] = (int32_t)v[c][e];
        asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
        for (int i = lane; i < cnt; i += 64) ((int32_t *)D.dst[c])[o0 + i] = ((const int32_t *)stage)[i];
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // reads done before the next column overwrites
    }
    k = k + 1 == DEPTH ? 0 : k + 1;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  // the partial last step: block 0, wave 0, scalar loads
  if (blockIdx.x == 0 && w == 0 && (n & 255)) {
    const unsigned long long b0 = bits[nsteps * 4], b1 = bits[nsteps * 4 + 1], b2 = bits[nsteps * 4 + 2],
                             b3 = bits[nsteps * 4 + 3];
    const unsigned m = (unsigned)((b0 >> lane) & 1) | (unsigned)((b1 >> lane) & 1) << 1 |
                       (unsigned)((b2 >> lane) & 1) << 2 | (unsigned)((b3 >> lane) & 1) << 3;
    int64_t pos = offs[nsteps] + __popcll(b0 & lt) + __popcll(b1 & lt) + __popcll(b2 & lt) + __popcll(b3 & lt);
    for (int e = 0; e < 4; e++) {
      const int64_t i = (nsteps << 8) + 4 * lane + e;
      if (!((m >> e) & 1u)) continue;  // rows past n are never selected
      for (int c = 0; c < D.nout; c++) {
        if (D.ow[c] == 8) ((int64_t *)D.dst[c])[pos] = ((const int64_t *)D.src[c])[i];
        else ((int32_t *)D.dst[c])[pos] = ((const int32_t *)D.src[c])[i];
      }
      pos++;
    }
  }
}

// copies row `row` of a w-byte column to position `pos` of another
__device__ __forceinline__ void fc_copy_row(const void *src, void *dst, int w, int64_t row, int64_t pos) {
  switch (w) {
    case 1: ((uint8_t *)dst)[pos] = ((const uint8_t *)src)[row]; break;
    case 2: ((uint16_t *)dst)[pos] = ((const uint16_t *)src)[row]; break;
    case 4: ((uint32_t *)dst)[pos] = ((const uint32_t *)src)[row]; break;
    case 8: ((uint64_t *)dst)[pos] = ((const uint64_t *)src)[row]; break;
    default: ((v4i32 *)dst)[pos] = ((const v4i32 *)src)[row]; break;
  }
}

// pass 2 for any mix of 1/2/4/8/16-byte outputs: every column's slice of a
// step (256 x w bytes, 1-4 LDS-DMA instructions; 1- and 2-byte slices use 16
// and 32 lanes) lands in the ring; each column's selected rows are copied
// slot -> per-wave staging area (LDS to LDS, at their rank) and stored out with
// consecutive lanes on consecutive rows; the slot is refilled after the last
// column.  NI = LDS-DMA instructions per step (compile time: the counted wait).
template <int NI, int DEPTH>
__global__ __launch_bounds__(256) void compact_any_lds_kernel(CompactDesc D, int64_t n, const unsigned long long *bits,
                                                              const int64_t *offs, int slot_bytes) {
  extern __shared__ __attribute__((aligned(16))) unsigned char ca_lds[];
  const int SB = slot_bytes;  // Σ 256 w + 64 (metadata), a multiple of 16
  const int w = threadIdx.x >> 6, lane = threadIdx.x & 63;
  unsigned char *ring = ca_lds + (size_t)w * DEPTH * SB;
  unsigned char *stage = ca_lds + (size_t)4 * DEPTH * SB + (size_t)w * 4096;  // 256 rows x 16 B per wave
  int off[FC_MAX_OUT];
  int meta_off = 0;
  {
    int o = 0;
#pragma unroll
    for (int c = 0; c < FC_MAX_OUT; c++) {
      off[c] = o;
      if (c < D.nout) o += D.ow[c] * 256;
    }
    meta_off = o;
  }
  const uint64_t lt = (1ull << lane) - 1;
  const int64_t nsteps = n >> 8;
  const int64_t nw = (int64_t)gridDim.x * 4;
  int64_t st = (int64_t)blockIdx.x * 4 + w;
  auto issue = [&](int64_t q, int d) {
    unsigned char *dst = ring + d * SB;
#pragma unroll
    for (int c = 0; c < FC_MAX_OUT; c++) {
      if (c >= D.nout) break;
      const int B = D.ow[c] * 256;
      const unsigned char *src = (const unsigned char *)D.src[c] + q * B;
      for (int j = 0; j < B; j += 1024)
        if (j + lane * 16 < B)
          __builtin_amdgcn_global_load_lds((const void *)(src + j + lane * 16), (void *)(dst + off[c] + j), 16, 0, 2);
    }
    const unsigned char *msrc = lane < 2 ? (const unsigned char *)(bits + q * 4) + lane * 16
                                         : (const unsigned char *)(offs + (q & ~(int64_t)1));
    if (lane < 3) __builtin_amdgcn_global_load_lds((const void *)msrc, (void *)(dst + meta_off), 16, 0, 0);
  };
  if (nsteps > 0) {
#pragma unroll
    for (int d = 0; d < DEPTH; d++) {
      int64_t q = st + d * nw;
      issue(q < nsteps ? q : 0, d);
    }
  }
  int k = 0;
  for (; st < nsteps; st += nw) {
    asm volatile("s_waitcnt vmcnt(%0)" ::"n"(NI * (DEPTH - 1)) : "memory");
    const unsigned char *src = ring + k * SB;
    const unsigned long long *meta = (const unsigned long long *)(src + meta_off);
    const unsigned long long b0 = meta[0], b1 = meta[1], b2 = meta[2], b3 = meta[3];
    const int64_t o0 = (int64_t)meta[4 + (st & 1)];
    const unsigned m = (unsigned)((b0 >> lane) & 1) | (unsigned)((b1 >> lane) & 1) << 1 |
                       (unsigned)((b2 >> lane) & 1) << 2 | (unsigned)((b3 >> lane) & 1) << 3;
    const int r0 = __popcll(b0 & lt) + __popcll(b1 & lt) + __popcll(b2 & lt) + __popcll(b3 & lt);
    const int cnt = __popcll(b0) + __popcll(b1) + __popcll(b2) + __popcll(b3);
#pragma unroll 1
    for (int c = 0; c < D.nout; c++) {
      const int ow = D.ow[c];
      const unsigned char *cs = src + off[c];
      int r = r0;
#pragma unroll
      for (int e = 0; e < 4; e++) {
        if (!((m >> e) & 1u)) continue;
        const int row = 4 * lane + e;
        switch (ow) {
          case 1: stage[r] = cs[row]; break;
          case 2: ((uint16_t *)stage)[r] = ((const uint16_t *)cs)[row]; break;
          case 4: ((uint32_t *)stage)[r] = ((const uint32_t *)cs)[row]; break;
          case 8: ((uint64_t *)stage)[r] = ((const uint64_t *)cs)[row]; break;
          default: ((v4i32 *)stage)[r] = ((const v4i32 *)cs)[row]; break;
        }
        r++;
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");
      unsigned char *dst = (unsigned char *)D.dst[c];
      switch (ow) {
        case 1: for (int i = lane; i < cnt; i += 64) dst[o0 + i] = stage[i]; break;
        case 2: for (int i = lane; i < cnt; i += 64) ((uint16_t *)dst)[o0 + i] = ((const uint16_t *)stage)[i]; break;
        case 4: for (int i = lane; i < cnt; i += 64) ((uint32_t *)dst)[o0 + i] = ((const uint32_t *)stage)[i]; break;
        case 8: for (int i = lane; i < cnt; i += 64) ((uint64_t *)dst)[o0 + i] = ((const uint64_t *)stage)[i]; break;
        default: for (int i = lane; i < cnt; i += 64) ((v4i32 *)dst)[o0 + i] = ((const v4i32 *)stage)[i]; break;
      }
      asm volatile("s_waitcnt lgkmcnt(0)" ::: "memory");  // staging reads done before the next column
    }
    int64_t q = st + DEPTH * nw;
    issue(q < nsteps ? q : st, k);
    k = k + 1 == DEPTH ? 0 : k + 1;
  }
  asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
  if (blockIdx.x == 0 && w == 0 && (n & 255)) {  // the partial last step
    const unsigned long long b0 = bits[nsteps * 4], b1 = bits[nsteps * 4 + 1], b2 = bits[nsteps * 4 + 2],
                             b3 = bits[nsteps * 4 + 3];
    const unsigned m = (unsigned)((b0 >> lane) & 1) | (unsigned)((b1 >> lane) & 1) << 1 |
                       (unsigned)((b2 >> lane) & 1) << 2 | (unsigned)((b3 >> lane) & 1) << 3;
    int64_t pos = offs[nsteps] + __popcll(b0 & lt) + __popcll(b1 & lt) + __popcll(b2 & lt) + __popcll(b3 & lt);
    for (int e = 0; e < 4; e++) {
      const int64_t i = (nsteps << 8) + 4 * lane + e;
      if (!((m >> e) & 1u)) continue;
      for (int c = 0; c < D.nout; c++) fc_copy_row(D.src[c], D.dst[c], D.ow[c], i, pos);
      pos++;
    }
  }
}

static void CompactAny(const CompactDesc &d, int64_t nrows, const unsigned long long *bits, const int64_t *step_offsets,
                       int grid, hipStream_t s) {
  int ni = 1, sb = 64;
  for (int c = 0; c < d.nout; c++) {
    ni += (d.ow[c] * 256 + 1023) / 1024;
    sb += d.ow[c] * 256;
  }
  const size_t lds = (size_t)4 * 2 * sb + 4 * 4096;
#define CA(N)                                                                                               \
  hipLaunchKernelGGL((compact_any_lds_kernel<N, 2>), dim3(grid), dim3(256), lds, s, d, nrows, bits, step_offsets, sb)
  switch (ni) {
    case 2: CA(2); break;
    case 3: CA(3); break;
    case 4: CA(4); break;
    case 5: CA(5); break;
    case 6: CA(6); break;
    case 7: CA(7); break;
    case 8: CA(8); break;
    default: CA(9); break;
  }
#undef CA
  CHECK_LAUNCH();
}

void CompactColumns(const CompactDesc &d, int64_t nrows, const unsigned long long *bits, const int64_t *step_offsets,
                    hipStream_t s) {
  if (nrows <= 0 || d.nout <= 0) return;
  bool any = false;
  for (int c = 0; c < d.nout; c++) any |= d.ow[c] != 4 && d.ow[c] != 8;
  if (any) {
    int gpc = 3;
    if (const char *e = Knob("MBX_CP_BLOCKS_PER_CU")) gpc = atoi(e) > 0 ? atoi(e) : 3;
    int grid = NumCUs() * gpc;
    const int64_t need = (nrows >> 8) / 4 + 1;
    if (grid > need) grid = (int)need;
    CompactAny(d, nrows, bits, step_offsets, grid, s);
    return;
  }
  int nld = 0;
  for (int c = 0; c < d.nout; c++) nld += d.ow[c] / 4;
  if (nld > 8) throw std::runtime_error("CompactColumns: more than 8 KiB of outputs per step");
  int gpc = 3;
  if (const char *e = Knob("MBX_CP_BLOCKS_PER_CU")) gpc = atoi(e) > 0 ? atoi(e) : 3;
  int grid = NumCUs() * gpc;
  const int64_t need = (nrows >> 8) / 4 + 1;
  if (grid > need) grid = (int)need;
#define CP(L, DP)                                                                                              \
  hipLaunchKernelGGL((compact_lds_kernel<L, DP>), dim3(grid), dim3(256), (size_t)4 * DP * (L * 1024 + 64) + 4 * 2048, s, d, \
                     nrows, bits, step_offsets)
  switch (nld) {
    case 1: CP(1, 6); break;
    case 2: CP(2, 3); break;
    case 3: CP(3, 2); break;
    case 4: CP(4, 2); break;
    case 5: CP(5, 2); break;
    case 6: CP(6, 2); break;
    case 7: CP(7, 2); break;
    default: CP(8, 2); break;
  }
#undef CP
  CHECK_LAUNCH();
}

}  // namespace dev
}  // namespace mbx
