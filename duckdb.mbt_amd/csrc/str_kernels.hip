// str_kernels.hip — VARCHAR predicates on the device: a string column against
// a constant (comparisons, LIKE and its prefix / suffix / contains forms) and
// two string columns against each other.  One byte per row comes out, 0 or 1,
// the layout of a BOOLEAN column; the executor (LowerStringPredicates) hands
// that column to the expression VM like any other.  The matching itself is
// str_match.h, the same functions the binder folds constants with.
//
// str_match: a wave step owns 256 consecutive rows, four per lane.  String
// offsets never decrease, so the step's bytes are the one span
// chars[off[r0] .. off[r0 + 256]): the wave streams it into its LDS region
// with 16 bytes per lane and load, from the span start rounded down to 16, and
// every lane then reads its four rows out of LDS.  One lane reading its rows
// byte by byte from global memory would use a few bytes of every 64- or 128-B
// line it touches per load.  A step whose span does not fit the region (one
// string of about 12 KiB is enough) evaluates its rows from global memory
// instead, decided per step and uniformly for the wave.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>

#include "device.h"
#include "str_minmax.h"

namespace mbx {
namespace dev {

namespace {

constexpr int kStepRows = 256;  // rows of a wave step
constexpr int kStrWaves = 4;    // waves of a workgroup, each with a region of its own
// A wave's LDS region.  12 KiB holds a step whose rows average 48 bytes, above
// the 5-30 bytes the path is for.  Four regions and the plan's 512 bytes make
// a 48.5 KiB workgroup, so LDS admits three workgroups (12 waves) on a CU's
// 160 KiB; a larger region would take the third away for spans that are rare.
// A wave has its whole span and 2 KiB of offsets in flight at once, about
// 6.5 KiB at 17 bytes a row, some 78 KiB per CU with 12 waves.  This is
// arithmetic, not a measurement: the 32-64 KiB per CU it was sized against is
// an estimate of HBM latency x bandwidth over 256 CUs, and the occupancy the
// launches reach was not read from counters.  Registers do not cap it below
// LDS: the compiler's kernel-resource-usage remarks give 60-74 VGPRs (74 for
// GENERAL), no spills, no scratch and 3 waves per SIMD for every staged kernel.
constexpr int kSpanBytes = 12 << 10;
constexpr int kStrBlocksPerCU = 3;

struct Row4 {
  int64_t b[4], e[4];  // the lane's rows: chars[b, e), clamped to [0, chars_len]
  int64_t s0, s1;      // the step's span
};

// The 257 offsets of a step: two 16-B loads and the next lane's first offset
// for a full step, clamped indices for the last one (rows past n are empty).
__device__ __forceinline__ Row4 load_offsets(const int64_t *__restrict__ off, int64_t chars_len, int64_t n,
                                             int64_t r0, bool full, int lane) {
  int64_t o[5];
  if (full && (((uintptr_t)off & 15) == 0)) {
    const longlong2 a = *(const longlong2 *)(off + r0), c = *(const longlong2 *)(off + r0 + 2);
    o[0] = a.x, o[1] = a.y, o[2] = c.x, o[3] = c.y;
    o[4] = off[r0 + 4];
  } else {
#pragma unroll
    for (int k = 0; k < 5; k++) o[k] = off[min(r0 + k, n)];
  }
  // whatever the offsets say, no row reaches outside chars
  Row4 r;
#pragma unroll
  for (int k = 0; k < 4; k++) {
    r.b[k] = min(max(o[k], (int64_t)0), chars_len);
    r.e[k] = min(max(o[k + 1], r.b[k]), chars_len);
  }
  r.s0 = __shfl(r.b[0], 0);
  r.s1 = __shfl(r.e[3], 63);
  return r;
}

// 16 bytes at address g, zero where they lie outside [lo, hi).  The low side
// (g < lo: a span start rounded down to before chars) is defensive only: every
// chars buffer the engine makes is at least 16-B aligned, so no test reaches it.
__device__ __forceinline__ uint4 load_piece(uintptr_t g, uintptr_t lo, uintptr_t hi) {
  if (g >= lo && g + 16 <= hi) return *(const uint4 *)g;
  uint32_t w[4] = {0, 0, 0, 0};
  for (int j = 0; j < 16; j++) {
    const uintptr_t a = g + j;
    if (a >= lo && a < hi) w[j >> 2] |= (uint32_t)(*(const uint8_t *)a) << (8 * (j & 3));
  }
  return make_uint4(w[0], w[1], w[2], w[3]);
}

template <int FORM, int OP, bool GLOBAL>
__global__ __launch_bounds__(kStrWaves * 64) void str_match_kernel(const StrMatchPlan plan, const StrCol col,
                                                                   const int64_t n, uint8_t *__restrict__ out) {
  __shared__ __attribute__((aligned(16))) uint8_t lds[GLOBAL ? 16 : kStrWaves * kSpanBytes];
  __shared__ uint8_t pb[kStrMatchCap + 1], pk[kStrMatchCap + 1];
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  pb[t] = plan.bytes[t];
  pk[t] = plan.kind[t];
  __syncthreads();
  const int plen = plan.len;
  const int64_t nsteps = (n + kStepRows - 1) / kStepRows;
  const uintptr_t base = (uintptr_t)col.chars, limit = base + (uintptr_t)col.chars_len;
  uint8_t *const region = lds + (GLOBAL ? 0 : wave * kSpanBytes);
  // every wave of the workgroup makes the same number of rounds (the barrier)
  for (int64_t bs = blockIdx.x; bs * kStrWaves < nsteps; bs += gridDim.x) {
    const int64_t step = bs * kStrWaves + wave;
    const bool active = step < nsteps;
    const int64_t r0 = step * kStepRows + lane * 4;
    Row4 r;
    uintptr_t from = 0;  // the address region[0] holds
    bool staged = false;
    if (active) {
      r = load_offsets(col.offsets, col.chars_len, n, r0, step * kStepRows + kStepRows <= n, lane);
      from = (base + (uintptr_t)r.s0) & ~(uintptr_t)15;
      const int64_t span = (int64_t)(base + (uintptr_t)r.s1 - from);
      staged = !GLOBAL && span <= kSpanBytes;
      if (staged) {
        // four 16-B loads per lane in flight, then their LDS stores
        for (int64_t c = 0; c < span; c += 4096) {
          uint4 v[4];
#pragma unroll
          for (int u = 0; u < 4; u++) {
            const int64_t p = c + u * 1024 + lane * 16;
            if (p < span) v[u] = load_piece(from + (uintptr_t)p, base, limit);
          }
#pragma unroll
          for (int u = 0; u < 4; u++) {
            const int64_t p = c + u * 1024 + lane * 16;
            if (p < span) *(uint4 *)(region + p) = v[u];
          }
        }
      }
    }
    if (!GLOBAL) __syncthreads();  // the span is in LDS before any lane reads another lane's bytes
    if (!active) continue;
    uint32_t bits = 0;
    if (staged) {
      const uint8_t *const s = region - (from - base);  // s + b = the staged copy of chars[b]
#pragma unroll
      for (int k = 0; k < 4; k++)
        bits |= (uint32_t)StrMatchRowT<FORM, OP>(pb, pk, plen, s + r.b[k], r.e[k] - r.b[k]) << (8 * k);
    } else {
      const uint8_t *const s = (const uint8_t *)col.chars;
#pragma unroll
      for (int k = 0; k < 4; k++)
        bits |= (uint32_t)StrMatchRowT<FORM, OP>(pb, pk, plen, s + r.b[k], r.e[k] - r.b[k]) << (8 * k);
    }
    if (r0 >= n) continue;
    if constexpr (OP == SM_DISTINCT || OP == SM_NOT_DISTINCT) {
      if (col.valid) {  // NULL is a value: distinct from every constant
        const uint32_t v4 = (uint32_t)(col.valid[r0 >> 6] >> (r0 & 63)) & 0xFu;
#pragma unroll
        for (int k = 0; k < 4; k++)
          if (!((v4 >> k) & 1u)) bits = (bits & ~(0xFFu << (8 * k))) | ((OP == SM_DISTINCT ? 1u : 0u) << (8 * k));
      }
    }
    if (r0 + 4 <= n && (((uintptr_t)out & 3) == 0)) {
      *(uint32_t *)(out + r0) = bits;
    } else {
      for (int k = 0; k < 4 && r0 + k < n; k++) out[r0 + k] = (uint8_t)(bits >> (8 * k));
    }
  }
}

template <int FORM, int OP>
void launch_match(const StrMatchPlan &plan, const StrCol &a, int64_t n, uint8_t *out, bool global_form, hipStream_t s) {
  const int64_t nsteps = (n + kStepRows - 1) / kStepRows;
  const int64_t want = (nsteps + kStrWaves - 1) / kStrWaves;
  const int grid = (int)std::min<int64_t>(want, (int64_t)NumCUs() * kStrBlocksPerCU);
  if (global_form)
    hipLaunchKernelGGL((str_match_kernel<FORM, OP, true>), dim3(grid), dim3(kStrWaves * 64), 0, s, plan, a, n, out);
  else
    hipLaunchKernelGGL((str_match_kernel<FORM, OP, false>), dim3(grid), dim3(kStrWaves * 64), 0, s, plan, a, n, out);
}

// ---- two columns: one row per lane, read from global memory (the two spans of
// a step are unrelated, and the shape is rare next to column-against-constant)
template <int OP>
__global__ __launch_bounds__(256) void str_compare_cols_kernel(const StrCol a, const StrCol b, const int64_t n,
                                                               uint8_t *__restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= n) return;
  const int64_t ab = min(max(a.offsets[i], (int64_t)0), a.chars_len);
  const int64_t ae = min(max(a.offsets[i + 1], ab), a.chars_len);
  const int64_t bb = min(max(b.offsets[i], (int64_t)0), b.chars_len);
  const int64_t be = min(max(b.offsets[i + 1], bb), b.chars_len);
  const uint8_t *const sa = (const uint8_t *)a.chars + ab, *const sb = (const uint8_t *)b.chars + bb;
  bool res;
  if constexpr (OP == SM_EQ || OP == SM_NE || OP == SM_DISTINCT || OP == SM_NOT_DISTINCT) {
    const bool eq = ae - ab == be - bb && StrBytesEqual(sa, sb, ae - ab);
    res = (OP == SM_EQ || OP == SM_NOT_DISTINCT) ? eq : !eq;
  } else {
    res = StrCompareOp(OP, StrCompare(sa, ae - ab, sb, be - bb));
  }
  if constexpr (OP == SM_DISTINCT || OP == SM_NOT_DISTINCT) {
    const bool va = !a.valid || ((a.valid[i >> 6] >> (i & 63)) & 1), vb = !b.valid || ((b.valid[i >> 6] >> (i & 63)) & 1);
    if (!va || !vb) res = (OP == SM_DISTINCT) ? (va != vb) : (va == vb);
  }
  out[i] = res;
}

__global__ void and_words_kernel(const uint64_t *__restrict__ a, const uint64_t *__restrict__ b, int64_t words,
                                 uint64_t *__restrict__ o) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < words) o[i] = a[i] & b[i];
}

template <int OP>
void launch_cols(const StrCol &a, const StrCol &b, int64_t n, uint8_t *out, hipStream_t s) {
  hipLaunchKernelGGL((str_compare_cols_kernel<OP>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, a, b, n, out);
}

}  // namespace

void StrMatch(const StrMatchPlan &plan, const StrCol &a, int64_t n, uint8_t *out, bool global_form, hipStream_t s) {
  if (n <= 0) return;
  switch (plan.form) {
    case SF_COMPARE:
      switch (plan.op) {
        case SM_EQ: return launch_match<SF_COMPARE, SM_EQ>(plan, a, n, out, global_form, s);
        case SM_NE: return launch_match<SF_COMPARE, SM_NE>(plan, a, n, out, global_form, s);
        case SM_LT: return launch_match<SF_COMPARE, SM_LT>(plan, a, n, out, global_form, s);
        case SM_LE: return launch_match<SF_COMPARE, SM_LE>(plan, a, n, out, global_form, s);
        case SM_GT: return launch_match<SF_COMPARE, SM_GT>(plan, a, n, out, global_form, s);
        case SM_GE: return launch_match<SF_COMPARE, SM_GE>(plan, a, n, out, global_form, s);
        case SM_DISTINCT: return launch_match<SF_COMPARE, SM_DISTINCT>(plan, a, n, out, global_form, s);
        default: return launch_match<SF_COMPARE, SM_NOT_DISTINCT>(plan, a, n, out, global_form, s);
      }
    case SF_EXACT: return launch_match<SF_EXACT, SM_LIKE>(plan, a, n, out, global_form, s);
    case SF_PREFIX: return launch_match<SF_PREFIX, SM_LIKE>(plan, a, n, out, global_form, s);
    case SF_SUFFIX: return launch_match<SF_SUFFIX, SM_LIKE>(plan, a, n, out, global_form, s);
    case SF_CONTAINS: return launch_match<SF_CONTAINS, SM_LIKE>(plan, a, n, out, global_form, s);
    case SF_ALL:  // every non-NULL row matches: no kernel (the executor does not even ask)
      (void)hipMemsetAsync(out, 1, (size_t)n, s);
      return;
    default: return launch_match<SF_GENERAL, SM_LIKE>(plan, a, n, out, global_form, s);
  }
}

void StrCompareCols(int op, const StrCol &a, const StrCol &b, int64_t n, uint8_t *out, uint64_t *out_valid,
                    hipStream_t s) {
  if (n <= 0) return;
  switch (op) {
    case SM_EQ: launch_cols<SM_EQ>(a, b, n, out, s); break;
    case SM_NE: launch_cols<SM_NE>(a, b, n, out, s); break;
    case SM_LT: launch_cols<SM_LT>(a, b, n, out, s); break;
    case SM_LE: launch_cols<SM_LE>(a, b, n, out, s); break;
    case SM_GT: launch_cols<SM_GT>(a, b, n, out, s); break;
    case SM_GE: launch_cols<SM_GE>(a, b, n, out, s); break;
    case SM_DISTINCT: launch_cols<SM_DISTINCT>(a, b, n, out, s); break;
    default: launch_cols<SM_NOT_DISTINCT>(a, b, n, out, s); break;
  }
  if (out_valid && a.valid && b.valid) {
    const int64_t words = (n + 63) / 64;
    hipLaunchKernelGGL(and_words_kernel, dim3((unsigned)((words + 255) / 256)), dim3(256), 0, s, a.valid, b.valid, words,
                       out_valid);
  }
}

// ---- MIN / MAX over VARCHAR (str_minmax.h): rounds of 64-bit atomicMin /
// atomicMax into one word per group and kind.  str_minmax_key (round 0) and
// str_minmax_live stream the offsets and the first 8 bytes of every row the way
// str_match walks a column, a wave step of 256 rows, four consecutive rows per
// lane, the offsets read once; the later rounds (str_minmax_round) read the
// candidates that str_minmax_live left.  No kernel waits for another
// workgroup: every loop below runs over rows or candidates.
namespace {

constexpr int kMmWaves = 4;
constexpr int kMmBlocksPerCU = 8;

// words: [0, nslots) MIN's, [nslots, 2 nslots) MAX's
__global__ void str_minmax_init_kernel(uint64_t *__restrict__ words, int64_t nslots, int r, int chunks) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i < 2 * nslots) words[i] = StrMinMaxInitWord(i < nslots ? SMM_MIN : SMM_MAX, r, chunks);
}

// The offer: a plain look at the word first, the atomic only for a key that
// would change it (Guideline 12; insert_run of join_kernels.hip does the same
// for max_run).  The word only moves towards better keys, so a stale look can
// cost an atomic and never drops one.
__device__ __forceinline__ void mm_offer(uint64_t *w, bool least, uint64_t key) {
  const uint64_t cur = __hip_atomic_load(w, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  if (!StrMinMaxImproves(least, key, cur)) return;
  if (least) atomicMin((unsigned long long *)w, (unsigned long long)key);
  else atomicMax((unsigned long long *)w, (unsigned long long)key);
}

__device__ __forceinline__ uint64_t wave_min_u64(uint64_t v) {
  for (int o = 32; o > 0; o >>= 1) {
    const uint64_t x = __shfl_xor(v, o);
    v = x < v ? x : v;
  }
  return v;
}
__device__ __forceinline__ uint64_t wave_max_u64(uint64_t v) {
  for (int o = 32; o > 0; o >>= 1) {
    const uint64_t x = __shfl_xor(v, o);
    v = x > v ? x : v;
  }
  return v;
}

// the lane's four rows of a step: which are valid rows of the column, their slots
struct MmRows {
  uint32_t v4;
  int32_t g[4];
};
__device__ __forceinline__ MmRows mm_rows(const StrMinMaxRun &A, int64_t r0) {
  MmRows m;
  m.v4 = 0;
#pragma unroll
  for (int k = 0; k < 4; k++) m.g[k] = 0;
  if (r0 >= A.n) return m;
  m.v4 = A.col.valid ? (uint32_t)(A.col.valid[r0 >> 6] >> (r0 & 63)) & 0xFu : 0xFu;  // r0 is a multiple of 4
  if (r0 + 4 > A.n) m.v4 &= (1u << (A.n - r0)) - 1u;
  if (A.slot_of) {
    if (r0 + 4 <= A.n && (((uintptr_t)A.slot_of & 15) == 0)) {
      const int4 q = *(const int4 *)(A.slot_of + r0);
      m.g[0] = q.x, m.g[1] = q.y, m.g[2] = q.z, m.g[3] = q.w;
    } else {
#pragma unroll
      for (int k = 0; k < 4; k++)
        if (r0 + k < A.n) m.g[k] = A.slot_of[r0 + k];
    }
    // a slot outside the words is never followed
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (m.g[k] < 0 || m.g[k] >= A.nslots) m.v4 &= ~(1u << k);
  }
  return m;
}

// Round 0 over every row.  GROUPED: each row offers to its slot's words.
// Otherwise the lane keeps its least and greatest key over all its steps, the
// wave reduces them with shuffles and issues one atomic per kind.
template <bool GROUPED>
__global__ __launch_bounds__(kMmWaves * 64) void str_minmax_key_kernel(const StrMinMaxRun A,
                                                                        uint64_t *__restrict__ words) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t nsteps = (A.n + kStepRows - 1) / kStepRows;
  const uint8_t *const chars = (const uint8_t *)A.col.chars;
  uint64_t lo = ~0ull, hi = 0;
  for (int64_t step = (int64_t)blockIdx.x * kMmWaves + wave; step < nsteps; step += (int64_t)gridDim.x * kMmWaves) {
    const int64_t r0 = step * kStepRows + lane * 4;
    const Row4 r = load_offsets(A.col.offsets, A.col.chars_len, A.n, r0, step * kStepRows + kStepRows <= A.n, lane);
    const MmRows m = mm_rows(A, r0);
#pragma unroll
    for (int k = 0; k < 4; k++) {
      if (!((m.v4 >> k) & 1u)) continue;
      const uint64_t key = StrMinMaxChunkKey(chars + r.b[k], r.e[k] - r.b[k], A.col.chars_len - r.b[k], 0);
      if constexpr (GROUPED) {
        if (A.kinds & kStrMinMaxWantMin) mm_offer(words + m.g[k], true, key);
        if (A.kinds & kStrMinMaxWantMax) mm_offer(words + A.nslots + m.g[k], false, key);
      } else {
        lo = key < lo ? key : lo;
        hi = key > hi ? key : hi;
      }
    }
  }
  if constexpr (!GROUPED) {
    // (a wave without a valid row offers the initial values, which change nothing)
    lo = wave_min_u64(lo);
    hi = wave_max_u64(hi);
    if (lane == 0) {
      if (A.kinds & kStrMinMaxWantMin) mm_offer(words, true, lo);
      if (A.kinds & kStrMinMaxWantMax) mm_offer(words + A.nslots, false, hi);
    }
  }
}

// The rows whose round-0 key is their slot's word, for either kind, compacted
// into cand (room for n entries; the order is whatever the waves' turns at the
// counter give: no round depends on it).  ctr[0]: their number, ctr[1]: the
// length of the longest.
__global__ __launch_bounds__(kMmWaves * 64) void str_minmax_live_kernel(const StrMinMaxRun A,
                                                                         const uint64_t *__restrict__ words,
                                                                         uint64_t *__restrict__ cand,
                                                                         unsigned long long *__restrict__ ctr) {
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int64_t nsteps = (A.n + kStepRows - 1) / kStepRows;
  const uint8_t *const chars = (const uint8_t *)A.col.chars;
  uint64_t maxlen = 0;
  for (int64_t step = (int64_t)blockIdx.x * kMmWaves + wave; step < nsteps; step += (int64_t)gridDim.x * kMmWaves) {
    const int64_t r0 = step * kStepRows + lane * 4;
    const Row4 r = load_offsets(A.col.offsets, A.col.chars_len, A.n, r0, step * kStepRows + kStepRows <= A.n, lane);
    const MmRows m = mm_rows(A, r0);
    int live[4];
    int mine = 0;
#pragma unroll
    for (int k = 0; k < 4; k++) {
      live[k] = 0;
      if (!((m.v4 >> k) & 1u)) continue;
      const uint64_t key = StrMinMaxChunkKey(chars + r.b[k], r.e[k] - r.b[k], A.col.chars_len - r.b[k], 0);
      if ((A.kinds & kStrMinMaxWantMin) && StrMinMaxStaysLive(key, words[m.g[k]])) live[k] |= kStrMinMaxWantMin;
      if ((A.kinds & kStrMinMaxWantMax) && StrMinMaxStaysLive(key, words[A.nslots + m.g[k]]))
        live[k] |= kStrMinMaxWantMax;
      if (live[k]) {
        mine++;
        const uint64_t len = (uint64_t)(r.e[k] - r.b[k]);
        maxlen = len > maxlen ? len : maxlen;
      }
    }
    // the lanes' counts scanned across the wave, one turn at the counter per step
    int before = mine;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
      const int x = __shfl_up(before, o);
      if (lane >= o) before += x;
    }
    const int total = __shfl(before, 63);
    if (total == 0) continue;  // (uniform)
    before -= mine;
    unsigned long long base = 0;
    if (lane == 0) base = atomicAdd(ctr, (unsigned long long)total);
    base = __shfl(base, 0);
    int64_t at = (int64_t)base + before;
#pragma unroll
    for (int k = 0; k < 4; k++)
      if (live[k] && at < A.n) cand[at++] = StrMinMaxCand(r0 + k, live[k]);
  }
  maxlen = wave_max_u64(maxlen);
  if (lane == 0 && maxlen > 0) mm_offer((uint64_t *)(ctr + 1), false, maxlen);
}

// Round r >= 1 over the candidates: a candidate that was live for a kind
// stays so if its key of round r - 1 is the slot's word of that round (prev),
// and then offers its key of round r (cur).  Its live bits are written back.
// Without slots the wave reduces the live lanes' keys first.
__global__ __launch_bounds__(256) void str_minmax_round_kernel(const StrMinMaxRun A, uint64_t *__restrict__ cand,
                                                                const int64_t ncand, const int r, const int chunks,
                                                                const uint64_t *__restrict__ prev,
                                                                uint64_t *__restrict__ cur) {
  const int lane = threadIdx.x & 63;
  const uint8_t *const chars = (const uint8_t *)A.col.chars;
  const int64_t stride = (int64_t)gridDim.x * 256;
  // whole waves make the same number of turns (the shuffles below)
  for (int64_t i0 = (int64_t)blockIdx.x * 256 + (threadIdx.x & ~63); i0 < ncand; i0 += stride) {
    const int64_t i = i0 + lane;
    int live = 0, was = 0;
    uint64_t key = 0;
    int64_t g = 0;
    if (i < ncand) {
      const uint64_t cd = cand[i];
      const int64_t row = StrMinMaxCandRow(cd);
      was = StrMinMaxCandLive(cd) & A.kinds;
      if (row < A.n && was) {
        g = A.slot_of ? A.slot_of[row] : 0;
        if (g >= 0 && g < A.nslots) {
          const int64_t b = min(max(A.col.offsets[row], (int64_t)0), A.col.chars_len);
          const int64_t e = min(max(A.col.offsets[row + 1], b), A.col.chars_len);
          const uint64_t pkey = StrMinMaxKey(r - 1, chunks, chars + b, e - b, A.col.chars_len - b, row);
          key = StrMinMaxKey(r, chunks, chars + b, e - b, A.col.chars_len - b, row);
          if ((was & kStrMinMaxWantMin) && StrMinMaxStaysLive(pkey, prev[g])) live |= kStrMinMaxWantMin;
          if ((was & kStrMinMaxWantMax) && StrMinMaxStaysLive(pkey, prev[A.nslots + g])) live |= kStrMinMaxWantMax;
        }
      }
      if (live != StrMinMaxCandLive(cd)) cand[i] = StrMinMaxCand(row, live);
    }
#pragma unroll
    for (int k = 0; k < SMM_KINDS; k++) {
      const bool on = (live >> k) & 1;
      const bool least = StrMinMaxTakesLeast(k, r, chunks);
      uint64_t *const w = cur + (k == SMM_MAX ? A.nslots : 0);
      if (A.slot_of) {
        if (on) mm_offer(w + g, least, key);
      } else {
        // (a lane that is not live offers the word's initial value: no change)
        const uint64_t mine = on ? key : StrMinMaxInitWord(k, r, chunks);
        const uint64_t best = least ? wave_min_u64(mine) : wave_max_u64(mine);
        if (lane == 0 && (A.kinds >> k & 1)) mm_offer(w, least, best);
      }
    }
  }
}

// Output row i is slot slot_list[i] (or i): its winner's row number from the
// last round's words, row 0 and a clear validity bit where the slot has none
// (or, defensively, a word that is no row of the column).
__global__ __launch_bounds__(256) void str_minmax_rows_kernel(const uint64_t *__restrict__ words,
                                                               const int32_t *__restrict__ slot_list,
                                                               const int64_t nout, const int64_t nslots,
                                                               const int64_t n, int64_t *__restrict__ rows,
                                                               uint64_t *__restrict__ valid) {
  const int lane = threadIdx.x & 63;
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  bool ok = false;
  if (i < nout) {
    const int64_t sl = slot_list ? slot_list[i] : i;
    uint64_t w = kStrMinMaxNoRow;
    if (sl >= 0 && sl < nslots) w = words[sl];
    ok = w != kStrMinMaxNoRow && w < (uint64_t)n;
    rows[i] = ok ? (int64_t)w : 0;
  }
  const uint64_t m = __ballot(ok);
  if (lane == 0 && i < nout) valid[i >> 6] = m;
}

int mm_grid(int64_t n) {
  const int64_t nsteps = (n + kStepRows - 1) / kStepRows;
  const int64_t want = (nsteps + kMmWaves - 1) / kMmWaves;
  return (int)std::max<int64_t>(1, std::min<int64_t>(want, (int64_t)NumCUs() * kMmBlocksPerCU));
}

}  // namespace

void StrMinMaxInitWords(uint64_t *words, int64_t nslots, int r, int chunks, hipStream_t s) {
  if (nslots <= 0) return;
  hipLaunchKernelGGL(str_minmax_init_kernel, dim3((unsigned)((2 * nslots + 255) / 256)), dim3(256), 0, s, words,
                     nslots, r, chunks);
}

void StrMinMaxKeyPass(const StrMinMaxRun &run, uint64_t *words, hipStream_t s) {
  if (run.n <= 0 || run.nslots <= 0) return;
  if (run.slot_of)
    hipLaunchKernelGGL((str_minmax_key_kernel<true>), dim3(mm_grid(run.n)), dim3(kMmWaves * 64), 0, s, run, words);
  else
    hipLaunchKernelGGL((str_minmax_key_kernel<false>), dim3(mm_grid(run.n)), dim3(kMmWaves * 64), 0, s, run, words);
}

void StrMinMaxLivePass(const StrMinMaxRun &run, const uint64_t *words, uint64_t *cand, unsigned long long *ctr,
                       hipStream_t s) {
  (void)hipMemsetAsync(ctr, 0, 16, s);
  if (run.n <= 0 || run.nslots <= 0) return;
  hipLaunchKernelGGL(str_minmax_live_kernel, dim3(mm_grid(run.n)), dim3(kMmWaves * 64), 0, s, run, words, cand, ctr);
}

void StrMinMaxRoundPass(const StrMinMaxRun &run, uint64_t *cand, int64_t ncand, int r, int chunks,
                        const uint64_t *prev, uint64_t *cur, hipStream_t s) {
  if (ncand <= 0 || run.nslots <= 0 || r < 1) return;
  const int grid = (int)std::min<int64_t>((ncand + 255) / 256, (int64_t)NumCUs() * 16);
  hipLaunchKernelGGL(str_minmax_round_kernel, dim3(grid), dim3(256), 0, s, run, cand, ncand, r, chunks, prev, cur);
}

void StrMinMaxRowsPass(const uint64_t *words, const int32_t *slot_list, int64_t nout, int64_t nslots, int64_t n,
                       int64_t *rows, uint64_t *valid, hipStream_t s) {
  if (nout <= 0) return;
  hipLaunchKernelGGL(str_minmax_rows_kernel, dim3((unsigned)((nout + 255) / 256)), dim3(256), 0, s, words, slot_list,
                     nout, nslots, n, rows, valid);
}

}  // namespace dev
}  // namespace mbx
