// join_kernels.hip — the inner equi-join on the device (executor: join.cpp).
//
//   join_keys         build keys of any integer width -> int64 (sign- or
//                     zero-extended) and, beside them, their row numbers
//   join_build        over the SORTED build keys: the first row of every run of
//                     equal keys inserts {key, run start, run length} into the
//                     open-addressing table of join_plan.h (one CAS per key)
//   join_probe_count  per probe row: hash, walk, write the match count (int64)
//                     and the run start (int32); no atomics on this side
//   join_probe_mark   x IN (subquery): per probe row the lookup, then the mark's
//                     byte and, where the plan asks for one, its validity bit
//                     (join_mark_plan.h); one wave64 ballot is one validity word
//   join_expand       per OUTPUT row j in [0, total): the probe row whose
//                     [offsets[p], offsets[p + 1]) holds j and the build row at
//                     that place of its run
//   join_probe_agg    a global aggregate over the join without the pairs: per
//                     probe row the lookup, then one interpreter pass per build
//                     row of its run over a program of three stages (residual,
//                     WHERE, aggregate arguments); per-workgroup partial records
//   join_agg_fold     the partial records merged in a fixed order into the
//                     AggState array and the counts the emit reads
//
// Every lane owns two consecutive rows, so 8-byte columns move as 16 bytes per
// lane.  join_expand is laid out by output rows, not by probe rows: a probe
// row with a million matches is a million output rows spread over as many
// lanes as any other million, and nothing is written outside [0, total).
// Every table walk is bounded by the capacity (join_plan.h); a walk that runs
// out raises E_JOIN_FULL in the device error word.
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include <algorithm>
#include <stdexcept>
#include <string>

#include "device.h"
#include "join_agg_plan.h"
#include "join_mark_plan.h"
#include "join_plan.h"
#include "phys.h"
#include "types.h"
#include "vm.h"
#include "vm_device.h"
#include "vm_lds.h"

namespace mbx {
namespace dev {

namespace {

constexpr int kJoinBlock = 256;
constexpr int kJoinBlocksPerCU = 8;
constexpr int kExpandTile = 2 * kJoinBlock;  // output rows of a workgroup step

int PairGrid(int64_t n) {
  const int64_t pairs = (n + 1) / 2;
  const int64_t want = (pairs + kJoinBlock - 1) / kJoinBlock;
  return (int)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)NumCUs() * kJoinBlocksPerCU));
}

__device__ __forceinline__ bool row_valid(const uint64_t *__restrict__ valid, int64_t i) {
  return !valid || ((valid[i >> 6] >> (i & 63)) & 1);
}

// rows i0, i0 + 1 of a column as int64; 8-byte columns with one 16-B load
template <typename T>
__device__ __forceinline__ void load_pair(const T *__restrict__ col, int64_t i0, bool both, int64_t &a, int64_t &b) {
  if constexpr (sizeof(T) == 8) {
    if (both && (((uintptr_t)col & 15) == 0)) {
      const longlong2 v = *(const longlong2 *)(col + i0);
      a = v.x, b = v.y;
      return;
    }
  }
  a = (int64_t)col[i0];
  b = both ? (int64_t)col[i0 + 1] : a;
}

__device__ __forceinline__ void store_pair(int64_t *__restrict__ out, int64_t i0, bool both, int64_t a, int64_t b) {
  if (both && (((uintptr_t)out & 15) == 0)) {
    *(longlong2 *)(out + i0) = make_longlong2(a, b);
  } else {
    out[i0] = a;
    if (both) out[i0 + 1] = b;
  }
}

template <typename T>
__global__ __launch_bounds__(kJoinBlock) void join_keys_kernel(const T *__restrict__ col, const int64_t n,
                                                               int64_t *__restrict__ keys, int64_t *__restrict__ rows) {
  const int64_t stride = (int64_t)gridDim.x * kJoinBlock;
  for (int64_t t = (int64_t)blockIdx.x * kJoinBlock + threadIdx.x; 2 * t < n; t += stride) {
    const int64_t i0 = 2 * t;
    const bool both = i0 + 1 < n;
    int64_t a, b;
    load_pair(col, i0, both, a, b);
    store_pair(keys, i0, both, a, b);
    if (rows) store_pair(rows, i0, both, i0, i0 + 1);
  }
}

// rows of the run of equal keys that starts at i: gallop, then bisect
__device__ __forceinline__ int64_t run_length(const int64_t *__restrict__ keys, int64_t n, int64_t i, int64_t k) {
  int64_t step = 1;
  while (i + step < n && keys[i + step] == k) step <<= 1;
  // keys[i + step / 2] == k (or step == 1); the run ends in (i + step / 2, min(i + step, n)]
  int64_t lo = i + (step >> 1), hi = std::min<int64_t>(i + step, n);  // keys[lo] == k; hi: first index known not in the run
  while (hi - lo > 1) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (keys[mid] == k) lo = mid;
    else hi = mid;
  }
  return hi - i;
}

__device__ __forceinline__ void insert_run(const int64_t *__restrict__ keys, int64_t n, int64_t i, int64_t k,
                                           JoinEntry *__restrict__ tab, int64_t cap, int32_t *__restrict__ err,
                                           uint32_t *max_run) {
  const int64_t len = run_length(keys, n, i, k);
  // the longest run, for the fused aggregate's choice (a word still 0 after a build stands for 1):
  // runs of one row touch nothing, a longer one reads the word with a plain load first, so that
  // it is not one atomic per key on this one address
  if (max_run && len > 1 && (uint32_t)len > *max_run) atomicMax(max_run, (uint32_t)len);
  const int64_t s = JoinInsert(tab, cap, k, (int32_t)i, (uint32_t)len,
                               [](uint32_t *w, uint32_t v) { return atomicCAS(w, 0u, v) == 0u; });
  if (s < 0) atomicCAS(err, 0, (int32_t)E_JOIN_FULL);
}

__global__ __launch_bounds__(kJoinBlock) void join_build_kernel(const int64_t *__restrict__ keys, const int64_t n,
                                                                JoinEntry *__restrict__ tab, const int64_t cap,
                                                                int32_t *__restrict__ err, uint32_t *max_run) {
  const int64_t stride = (int64_t)gridDim.x * kJoinBlock;
  for (int64_t t = (int64_t)blockIdx.x * kJoinBlock + threadIdx.x; 2 * t < n; t += stride) {
    const int64_t i0 = 2 * t;
    const bool both = i0 + 1 < n;
    int64_t k0, k1;
    load_pair(keys, i0, both, k0, k1);
    if (i0 == 0 || keys[i0 - 1] != k0) insert_run(keys, n, i0, k0, tab, cap, err, max_run);
    if (both && k1 != k0) insert_run(keys, n, i0 + 1, k1, tab, cap, err, max_run);
  }
}

template <typename T>
__global__ __launch_bounds__(kJoinBlock) void join_probe_count_kernel(const T *__restrict__ col,
                                                                      const uint64_t *__restrict__ valid, const int64_t n,
                                                                      const JoinEntry *__restrict__ tab, const int64_t cap,
                                                                      int64_t *__restrict__ counts,
                                                                      int32_t *__restrict__ starts,
                                                                      int32_t *__restrict__ err) {
  const int64_t stride = (int64_t)gridDim.x * kJoinBlock;
  for (int64_t t = (int64_t)blockIdx.x * kJoinBlock + threadIdx.x; 2 * t < n; t += stride) {
    const int64_t i0 = 2 * t;
    const bool both = i0 + 1 < n;
    int64_t k[2];
    load_pair(col, i0, both, k[0], k[1]);
    int64_t cnt[2] = {0, 0};
    int32_t st[2] = {0, 0};
#pragma unroll
    for (int r = 0; r < 2; r++) {
      if (r == 1 && !both) break;
      if (!row_valid(valid, i0 + r)) continue;  // a NULL key matches nothing
      JoinEntry e;
      const int64_t s = JoinLookup(tab, cap, k[r], &e);
      if (s >= 0) {
        cnt[r] = (int64_t)e.len;
        st[r] = e.start;
      } else if (s == kJoinTableFull) {
        atomicCAS(err, 0, (int32_t)E_JOIN_FULL);
      }
    }
    store_pair(counts, i0, both, cnt[0], cnt[1]);
    starts[i0] = st[0];
    if (both) starts[i0 + 1] = st[1];
  }
}

// x IN (subquery).  A wave owns kMarkGroups x 64 consecutive rows at a time:
// lane t takes rows base + 64 g + t, so a group's keys are one contiguous
// wave-wide load, its marks one contiguous run of bytes, and its validity bits
// exactly one word, which the ballot assembles and lane 0 stores whole (base
// is a multiple of 64 x kMarkGroups).  The first entry of every group's probe
// sequence is loaded before any is looked at: kMarkGroups independent 16-B
// table reads per lane are in flight.  A key whose first slot holds another
// key walks on with JoinLookup.  Rows at or past n vote 0, which leaves the
// last word's unused bits clear like every other validity writer's; a word
// wholly past n is not written.  tab may be null with cap == 0 (a set of
// NULLs only): nothing is found.
constexpr int kMarkGroups = 4;
constexpr int kMarkBlocksPerCU = 4;
constexpr int kMarkWaveRows = 64 * kMarkGroups;

template <typename T>
__global__ __launch_bounds__(kJoinBlock) void join_probe_mark_kernel(const T *__restrict__ col,
                                                                     const uint64_t *__restrict__ valid, const int64_t n,
                                                                     const JoinEntry *__restrict__ tab, const int64_t cap,
                                                                     const bool set_has_null, uint8_t *__restrict__ mark,
                                                                     uint64_t *__restrict__ mark_valid,
                                                                     int32_t *__restrict__ err) {
  const int lane = threadIdx.x & 63;
  const int64_t wave = (int64_t)blockIdx.x * (kJoinBlock / 64) + (threadIdx.x >> 6);
  const int64_t nwaves = (int64_t)gridDim.x * (kJoinBlock / 64);
  const int64_t nchunks = (n + kMarkWaveRows - 1) / kMarkWaveRows;
  for (int64_t chunk = wave; chunk < nchunks; chunk += nwaves) {
    const int64_t base = chunk * kMarkWaveRows;
    int64_t k[kMarkGroups];
    bool live[kMarkGroups], kv[kMarkGroups];
    JoinEntry first[kMarkGroups];
#pragma unroll
    for (int g = 0; g < kMarkGroups; g++) {
      const int64_t row = base + 64 * g + lane;
      live[g] = row < n;
      k[g] = live[g] ? (int64_t)col[row] : 0;
      kv[g] = live[g] && row_valid(valid, row);
    }
#pragma unroll
    for (int g = 0; g < kMarkGroups; g++) {
      first[g].len = 0;
      if (kv[g] && cap > 0) first[g] = tab[JoinSlot(JoinHash(k[g]), 0, cap)];
    }
#pragma unroll
    for (int g = 0; g < kMarkGroups; g++) {
      if (base + 64 * g >= n) break;  // (the whole wave leaves together)
      bool found = false;
      if (first[g].len != 0) {
        found = first[g].key == k[g];
        if (!found) {
          JoinEntry e;
          const int64_t s = JoinLookup(tab, cap, k[g], &e);
          found = s >= 0;
          if (s == kJoinTableFull) atomicCAS(err, 0, (int32_t)E_JOIN_FULL);
        }
      }
      const JoinMarkCellValue c = JoinMarkCell(found, kv[g], false, set_has_null);
      const int64_t row = base + 64 * g + lane;
      if (live[g]) mark[row] = c.value;
      if (mark_valid) {
        const uint64_t word = __ballot(live[g] && c.valid);
        if (lane == 0) mark_valid[(base >> 6) + g] = word;
      }
    }
  }
}

// the largest p in [lo, hi) with offs[p] <= j; needs offs[lo] <= j < offs[hi]
__device__ __forceinline__ int64_t owner_row(const int64_t *__restrict__ offs, int64_t lo, int64_t hi, int64_t j) {
  while (hi - lo > 1) {
    const int64_t mid = lo + ((hi - lo) >> 1);
    if (offs[mid] <= j) lo = mid;
    else hi = mid;
  }
  return lo;
}

// offs: the n + 1 exclusive offsets of the probe rows' counts (offs[n] ==
// total); starts: each probe row's run start; build_rows: the build row
// numbers in sorted-key order.  Output row j belongs to the probe row p with
// offs[p] <= j < offs[p + 1] and is the (j - offs[p])-th row of p's run.
__global__ __launch_bounds__(kJoinBlock) void join_expand_kernel(const int64_t *__restrict__ offs,
                                                                 const int32_t *__restrict__ starts, const int64_t n,
                                                                 const int64_t total,
                                                                 const int64_t *__restrict__ build_rows,
                                                                 int64_t *__restrict__ out_probe,
                                                                 int64_t *__restrict__ out_build) {
  __shared__ int64_t s_lo, s_hi;
  const int64_t ntiles = (total + kExpandTile - 1) / kExpandTile;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t j0 = tile * kExpandTile, j1 = std::min<int64_t>(j0 + kExpandTile, total);
    // the tile's probe rows lie between the owners of its first and last output row
    if (threadIdx.x == 0) s_lo = owner_row(offs, 0, n, j0);
    if (threadIdx.x == 64) s_hi = owner_row(offs, 0, n, j1 - 1);
    __syncthreads();
    const int64_t j = j0 + 2 * (int64_t)threadIdx.x;
    if (j < j1) {
      const bool both = j + 1 < j1;
      const int64_t p0 = owner_row(offs, s_lo, s_hi + 1, j);
      int64_t p1 = p0;
      if (both && j + 1 >= offs[p0 + 1]) p1 = owner_row(offs, p0 + 1, s_hi + 1, j + 1);
      const int64_t b0 = build_rows[(int64_t)starts[p0] + (j - offs[p0])];
      const int64_t b1 = both ? build_rows[(int64_t)starts[p1] + (j + 1 - offs[p1])] : b0;
      store_pair(out_probe, j, both, p0, p1);
      store_pair(out_build, j, both, b0, b1);
    }
    __syncthreads();  // s_lo / s_hi are rewritten by the next tile
  }
}

// ---- the fused probe-and-aggregate ------------------------------------------------------------------
static_assert(sizeof(JoinAggRec) == sizeof(AggState) && offsetof(JoinAggRec, sum_hi) == offsetof(AggState, sum_hi) &&
                  offsetof(JoinAggRec, min_i) == offsetof(AggState, min_i) &&
                  offsetof(JoinAggRec, sum_f) == offsetof(AggState, sum_f) &&
                  offsetof(JoinAggRec, max_f) == offsetof(AggState, max_f),
              "join_agg_fold writes JoinAggRec records where the emit reads AggState");
static_assert(VM_MAX_COLS <= 32, "JoinAggArgs::build_mask has one bit per VmCols slot");

__device__ __forceinline__ uint64_t wave_add(uint64_t v) {
  for (int d = 32; d >= 1; d >>= 1) v += (uint64_t)__shfl_xor((unsigned long long)v, d);
  return v;
}

// One 256-row tile of probe rows per workgroup step.  Every lane looks its
// key up and keeps its run's start and length; a wave then makes as many
// interpreter passes as its longest run has rows, lane t active while j <
// len, its pair (probe row, build_rows[start + j]) living in the LDS register
// planes only.  A V_LOADCOL of a build-side slot reads at the build row,
// everything else at the probe row.  `active` narrows after the residual and
// after the WHERE, so the argument stage raises only for pairs both keep.
// The waves share nothing inside the loop (the planes are per lane, the
// accumulators per wave, touched by lane 0 only): no barrier until the end,
// where the four waves' records merge into the workgroup's partials.
__global__ __launch_bounds__(kJoinBlock) void join_probe_agg_kernel(VmProgram P, VmCols C, JoinAggArgs A,
                                                                    JoinAggRec *__restrict__ partials,
                                                                    unsigned long long *__restrict__ block_counts,
                                                                    int32_t *err) {
  extern __shared__ __attribute__((aligned(16))) unsigned char vm_lds[];
  const VmLds R = vm_regs(vm_lds, P.n_regs);
  __shared__ JoinAggRec s_acc[kJoinBlock / 64][VM_MAX_OUT];
  __shared__ unsigned long long s_cnt[kJoinBlock / 64][2];
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  if (lane == 0)
    for (int o = 0; o < P.n_out; o++) s_acc[w][o] = JoinAggEmpty();
  LdsRF rf{R, t};
  uint64_t pairs = 0, kept = 0;
  const int64_t ntiles = (A.n + VM_TILE - 1) / VM_TILE;
  for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
    const int64_t row = tile * VM_TILE + t;
    int len = 0;
    int64_t start = 0;
    if (row < A.n && bit_valid(A.key_valid, row)) {  // a NULL key matches nothing
      int64_t k, khi;
      load_phys(A.key, A.key_phys, row, k, khi);
      JoinEntry e;
      const int64_t s = JoinLookup(A.tab, A.cap, k, &e);
      if (s >= 0) {
        len = (int)e.len;
        start = e.start;
      } else if (s == kJoinTableFull) {
        atomicCAS(err, 0, (int32_t)E_JOIN_FULL);
      }
    }
    pairs += (uint64_t)len;  // counted before the residual: the limit is on the join's own pairs
    int wmax = len;
    for (int d = 32; d >= 1; d >>= 1) {
      const int other = __shfl_xor(wmax, d);
      wmax = other > wmax ? other : wmax;
    }
    for (int j = 0; j < wmax; j++) {
      bool active = j < len;
      const int64_t brow = active ? A.build_rows[start + j] : 0;
      int k = 0;
#pragma unroll 1
      for (int stage = 0; stage < 3; stage++) {
        const int kend = stage == 0 ? A.end_residual : stage == 1 ? A.end_where : P.n_ins;
        for (; k < kend; k++) {
          const VmIns I = P.ins[k];
          const bool bside = I.op == V_LOADCOL && ((A.build_mask >> I.a) & 1u);
          vm_step(P, C, I.op, I.dst, I.a, I.b, I.c, I.aux, bside ? brow : row, active, 0, 1, rf, err);
        }
        const int pr = stage == 0 ? A.residual_reg : stage == 1 ? A.where_reg : 255;
        if (pr != 255) active = active && !rf.nl(pr) && rf.lo(pr) != 0;
      }
      kept += active ? 1u : 0u;
      for (int o = 0; o < P.n_out; o++) {
        const int r = P.out_reg[o];
        if (r == 255) continue;  // COUNT(*): the kept pairs
        const bool has = active && !rf.nl(r);
        const uint64_t m = __ballot(has);
        if (!m) continue;  // wave-uniform
        const int stats = P.out_phys[o];  // bit 0: sum, bit 1: min / max (COUNT: neither)
        JoinAggRec b = JoinAggEmpty();
        b.count = (uint64_t)__popcll(m);
        if (P.out_class[o] == VC_F64) {
          const double v = __longlong_as_double(rf.lo(r));
          if (stats & 1) {
            double sum = has ? v : 0.0;
            for (int d = 32; d >= 1; d >>= 1) sum += __shfl_xor(sum, d);
            b.sum_f = sum;
          }
          if (stats & 2) {
            const uint64_t key = f64_order(v);
            uint64_t mn = has ? key : ~0ull, mx = has ? key : 0ull;
            for (int d = 32; d >= 1; d >>= 1) {
              const uint64_t on = (uint64_t)__shfl_xor((unsigned long long)mn, d);
              const uint64_t ox = (uint64_t)__shfl_xor((unsigned long long)mx, d);
              mn = on < mn ? on : mn;
              mx = ox > mx ? ox : mx;
            }
            b.min_f = mn;
            b.max_f = mx;
          }
        } else {
          // a 64-bit class register's high plane is not its sign: only 128-bit values carry one
          const int64_t v = rf.lo(r), vh = P.out_class[o] == VC_I128 ? rf.hi(r) : (v >> 63);
          if (stats & 1) {
            uint64_t lo = has ? (uint64_t)v : 0, hi = has ? (uint64_t)vh : 0;
            for (int d = 32; d >= 1; d >>= 1) {
              const uint64_t ol = (uint64_t)__shfl_xor((unsigned long long)lo, d);
              const uint64_t oh = (uint64_t)__shfl_xor((unsigned long long)hi, d);
              const uint64_t nl = lo + ol;
              hi += oh + (nl < lo ? 1u : 0u);
              lo = nl;
            }
            b.sum_lo = lo;
            b.sum_hi = (int64_t)hi;
          }
          if (stats & 2) {
            long long mn = has ? v : INT64_MAX, mx = has ? v : INT64_MIN;
            for (int d = 32; d >= 1; d >>= 1) {
              const long long on = __shfl_xor(mn, d), ox = __shfl_xor(mx, d);
              mn = on < mn ? on : mn;
              mx = ox > mx ? ox : mx;
            }
            b.min_i = mn;
            b.max_i = mx;
          }
        }
        if (lane == 0) JoinAggMerge(s_acc[w][o], b);
      }
    }
  }
  pairs = wave_add(pairs);
  kept = wave_add(kept);
  if (lane == 0) {
    s_cnt[w][0] = pairs;
    s_cnt[w][1] = kept;
  }
  __syncthreads();
  if (t < P.n_out) {
    JoinAggRec a = s_acc[0][t];
    for (int v = 1; v < kJoinBlock / 64; v++) JoinAggMerge(a, s_acc[v][t]);
    partials[(size_t)blockIdx.x * P.n_out + t] = a;
  }
  if (t < 2) {
    unsigned long long c = 0;
    for (int v = 0; v < kJoinBlock / 64; v++) c += s_cnt[v][t];
    block_counts[(size_t)blockIdx.x * 2 + t] = c;
  }
}

// One workgroup: thread t merges the records of blocks t, t + 256, ... in
// ascending order, then the 256 partial merges fold as a tree whose shape
// depends on nothing but the block count; a double sum therefore comes out
// the same for the same grid.  counts_out[0] = kept pairs (the COUNT(*) word
// of the emit), counts_out[1] = the join's pairs.
__global__ __launch_bounds__(kJoinBlock) void join_agg_fold_kernel(const JoinAggRec *__restrict__ partials,
                                                                   const unsigned long long *__restrict__ block_counts,
                                                                   const int blocks, const int n_out,
                                                                   JoinAggRec *__restrict__ states,
                                                                   unsigned long long *__restrict__ counts_out) {
  __shared__ JoinAggRec s_rec[kJoinBlock];
  __shared__ unsigned long long s_c[kJoinBlock][2];
  const int t = threadIdx.x;
  unsigned long long c0 = 0, c1 = 0;
  for (int b = t; b < blocks; b += kJoinBlock) {
    c0 += block_counts[(size_t)b * 2];
    c1 += block_counts[(size_t)b * 2 + 1];
  }
  s_c[t][0] = c0;
  s_c[t][1] = c1;
  __syncthreads();
  for (int h = kJoinBlock / 2; h >= 1; h >>= 1) {
    if (t < h) {
      s_c[t][0] += s_c[t + h][0];
      s_c[t][1] += s_c[t + h][1];
    }
    __syncthreads();
  }
  if (t == 0) {
    counts_out[0] = s_c[0][1];
    counts_out[1] = s_c[0][0];
  }
  for (int o = 0; o < n_out; o++) {
    JoinAggRec a = JoinAggEmpty();
    for (int b = t; b < blocks; b += kJoinBlock) JoinAggMerge(a, partials[(size_t)b * n_out + o]);
    s_rec[t] = a;
    __syncthreads();
    for (int h = kJoinBlock / 2; h >= 1; h >>= 1) {
      if (t < h) {
        JoinAggRec x = s_rec[t];
        JoinAggMerge(x, s_rec[t + h]);
        s_rec[t] = x;
      }
      __syncthreads();
    }
    if (t == 0) states[o] = s_rec[0];
    __syncthreads();  // s_rec is rewritten by the next aggregate
  }
}

template <typename T>
void launch_keys(const void *col, int64_t n, int64_t *keys, int64_t *rows, hipStream_t s) {
  hipLaunchKernelGGL((join_keys_kernel<T>), dim3(PairGrid(n)), dim3(kJoinBlock), 0, s, (const T *)col, n, keys, rows);
}

template <typename T>
void launch_probe(const void *col, const uint64_t *valid, int64_t n, const JoinEntry *tab, int64_t cap, int64_t *counts,
                  int32_t *starts, int32_t *err, hipStream_t s) {
  hipLaunchKernelGGL((join_probe_count_kernel<T>), dim3(PairGrid(n)), dim3(kJoinBlock), 0, s, (const T *)col, valid, n,
                     tab, cap, counts, starts, err);
}

template <typename T>
void launch_mark(const void *col, const uint64_t *valid, int64_t n, const JoinEntry *tab, int64_t cap, bool set_has_null,
                 uint8_t *mark, uint64_t *mark_valid, int32_t *err, hipStream_t s) {
  const int64_t nchunks = (n + kMarkWaveRows - 1) / kMarkWaveRows;
  const int64_t want = (nchunks + kJoinBlock / 64 - 1) / (kJoinBlock / 64);
  const int grid = (int)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)NumCUs() * kMarkBlocksPerCU));
  hipLaunchKernelGGL((join_probe_mark_kernel<T>), dim3(grid), dim3(kJoinBlock), 0, s, (const T *)col, valid, n, tab, cap,
                     set_has_null, mark, mark_valid, err);
}

void CheckLaunch(const char *what) {
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) throw std::runtime_error(std::string(what) + ": " + hipGetErrorString(e));
}

}  // namespace

void JoinKeys(const void *col, int phys, int64_t n, int64_t *keys, int64_t *rows, hipStream_t s) {
  if (n <= 0) return;
  switch (phys) {
    case P_U8: launch_keys<uint8_t>(col, n, keys, rows, s); break;
    case P_I8: launch_keys<int8_t>(col, n, keys, rows, s); break;
    case P_I16: launch_keys<int16_t>(col, n, keys, rows, s); break;
    case P_U16: launch_keys<uint16_t>(col, n, keys, rows, s); break;
    case P_I32: launch_keys<int32_t>(col, n, keys, rows, s); break;
    case P_U32: launch_keys<uint32_t>(col, n, keys, rows, s); break;
    case P_I64: launch_keys<int64_t>(col, n, keys, rows, s); break;
    case P_U64: launch_keys<uint64_t>(col, n, keys, rows, s); break;
    default: throw std::runtime_error("join_keys: not an integer column");
  }
  CheckLaunch("join_keys");
}

void JoinBuild(const int64_t *sorted_keys, int64_t n, JoinEntry *tab, int64_t cap, int32_t *err, hipStream_t s,
               uint32_t *max_run) {
  if (n <= 0) return;
  hipLaunchKernelGGL(join_build_kernel, dim3(PairGrid(n)), dim3(kJoinBlock), 0, s, sorted_keys, n, tab, cap, err,
                     max_run);
  CheckLaunch("join_build");
}

void JoinProbeCount(const void *col, int phys, const uint64_t *valid, int64_t n, const JoinEntry *tab, int64_t cap,
                    int64_t *counts, int32_t *starts, int32_t *err, hipStream_t s) {
  if (n <= 0) return;
  switch (phys) {
    case P_U8: launch_probe<uint8_t>(col, valid, n, tab, cap, counts, starts, err, s); break;
    case P_I8: launch_probe<int8_t>(col, valid, n, tab, cap, counts, starts, err, s); break;
    case P_I16: launch_probe<int16_t>(col, valid, n, tab, cap, counts, starts, err, s); break;
    case P_U16: launch_probe<uint16_t>(col, valid, n, tab, cap, counts, starts, err, s); break;
    case P_I32: launch_probe<int32_t>(col, valid, n, tab, cap, counts, starts, err, s); break;
    case P_U32: launch_probe<uint32_t>(col, valid, n, tab, cap, counts, starts, err, s); break;
    case P_I64: launch_probe<int64_t>(col, valid, n, tab, cap, counts, starts, err, s); break;
    case P_U64: launch_probe<uint64_t>(col, valid, n, tab, cap, counts, starts, err, s); break;
    default: throw std::runtime_error("join_probe_count: not an integer column");
  }
  CheckLaunch("join_probe_count");
}

void JoinProbeMark(const void *col, int phys, const uint64_t *valid, int64_t n, const JoinEntry *tab, int64_t cap,
                   bool set_has_null, uint8_t *mark, uint64_t *mark_valid, int32_t *err, hipStream_t s) {
  if (n <= 0) return;
  if (!tab) cap = 0;
  switch (phys) {
    case P_U8: launch_mark<uint8_t>(col, valid, n, tab, cap, set_has_null, mark, mark_valid, err, s); break;
    case P_I8: launch_mark<int8_t>(col, valid, n, tab, cap, set_has_null, mark, mark_valid, err, s); break;
    case P_I16: launch_mark<int16_t>(col, valid, n, tab, cap, set_has_null, mark, mark_valid, err, s); break;
    case P_U16: launch_mark<uint16_t>(col, valid, n, tab, cap, set_has_null, mark, mark_valid, err, s); break;
    case P_I32: launch_mark<int32_t>(col, valid, n, tab, cap, set_has_null, mark, mark_valid, err, s); break;
    case P_U32: launch_mark<uint32_t>(col, valid, n, tab, cap, set_has_null, mark, mark_valid, err, s); break;
    case P_I64: launch_mark<int64_t>(col, valid, n, tab, cap, set_has_null, mark, mark_valid, err, s); break;
    case P_U64: launch_mark<uint64_t>(col, valid, n, tab, cap, set_has_null, mark, mark_valid, err, s); break;
    default: throw std::runtime_error("join_probe_mark: not an integer column");
  }
  CheckLaunch("join_probe_mark");
}

void JoinExpand(const int64_t *offsets, const int32_t *starts, int64_t n, int64_t total, const int64_t *build_rows,
                int64_t *out_probe, int64_t *out_build, hipStream_t s) {
  if (n <= 0 || total <= 0) return;
  const int64_t ntiles = (total + kExpandTile - 1) / kExpandTile;
  const int grid = (int)std::min<int64_t>(ntiles, (int64_t)NumCUs() * kJoinBlocksPerCU);
  hipLaunchKernelGGL(join_expand_kernel, dim3(grid), dim3(kJoinBlock), 0, s, offsets, starts, n, total, build_rows,
                     out_probe, out_build);
  CheckLaunch("join_expand");
}

int JoinProbeAggBlocks(int64_t n) {
  const int64_t ntiles = (n + VM_TILE - 1) / VM_TILE;
  return (int)std::max<int64_t>(1, std::min<int64_t>(ntiles, (int64_t)NumCUs() * kJoinBlocksPerCU));
}

void JoinProbeAgg(const VmProgram &p, const VmCols &cols, const JoinAggArgs &a, JoinAggRec *partials,
                  unsigned long long *block_counts, int blocks, int32_t *err, hipStream_t s) {
  if (a.key_phys > P_U64) throw std::runtime_error("join_probe_agg: not an integer column");
  if (blocks != JoinProbeAggBlocks(a.n)) throw std::runtime_error("join_probe_agg: partials sized for another grid");
  hipLaunchKernelGGL(join_probe_agg_kernel, dim3(blocks), dim3(kJoinBlock), VmLdsBytes(p.n_regs), s, p, cols, a, partials,
                     block_counts, err);
  CheckLaunch("join_probe_agg");
}

void JoinAggFold(const JoinAggRec *partials, const unsigned long long *block_counts, int blocks, int n_out,
                 AggState *states, unsigned long long *counts_out, hipStream_t s) {
  hipLaunchKernelGGL(join_agg_fold_kernel, dim3(1), dim3(kJoinBlock), 0, s, partials, block_counts, blocks, n_out,
                     (JoinAggRec *)states, counts_out);
  CheckLaunch("join_agg_fold");
}

}  // namespace dev
}  // namespace mbx
