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

}  // namespace dev
}  // namespace mbx
