// window_plan.h — what the window stage (window.cpp, window_kernels.hip)
// decides and computes without a GPU: which position of the sorted order a
// call reads its value at (frame resolution), which calls share one sort
// (grouping by specification), and the segmented scan's operator with the
// running state of each kind of call.
//
// The scan runs over sorted positions.  An element is (flag, state): the flag
// says that a segment (a partition) starts here.  The operator is
//
//   (fa, a) (+) (fb, b) = (fa | fb, fb ? b : merge(a, b))
//
// which is associative whenever merge is, so tiles can be reduced, their
// carries scanned and the tiles finished in three launches, with no
// workgroup waiting for another.  WinTileScan is that three-step shape on the
// host; the kernels follow it step by step.
// No HIP types: the functions also build in a plain host program
// (tests/plan_harness/window_plan.cpp).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MBX_WN_HD __host__ __device__ __forceinline__
#else
#define MBX_WN_HD inline
#endif

namespace mbx {

// ---- functions and frames ---------------------------------------------------
enum WinKind : uint8_t {
  W_ROW_NUMBER, W_RANK, W_DENSE_RANK, W_COUNT_STAR, W_COUNT, W_SUM, W_MIN, W_MAX, W_AVG, W_LAG, W_LEAD,
  W_NKINDS
};

// the frame as written: none, or a unit with its end (the start is always UNBOUNDED PRECEDING)
enum WinFrameSpec : uint8_t {
  WFS_NONE, WFS_ROWS_CURRENT, WFS_RANGE_CURRENT, WFS_ROWS_UNBOUNDED, WFS_RANGE_UNBOUNDED,
  WFS_NSPECS
};

// the sorted position whose running state is the call's value at position i
enum WinTarget : uint8_t {
  WT_SELF,      // i itself: ROWS to CURRENT ROW; the rank functions, LAG and LEAD ignore the frame
  WT_PEER_END,  // the last row of i's peer group: RANGE to CURRENT ROW
  WT_PART_END,  // the last row of i's partition: the whole partition
};

MBX_WN_HD bool WinIsAggregate(WinKind k) { return k >= W_COUNT_STAR && k <= W_AVG; }

MBX_WN_HD WinTarget WinResolveFrame(WinKind k, bool has_order, WinFrameSpec f) {
  if (!WinIsAggregate(k)) return WT_SELF;
  switch (f) {
    case WFS_NONE: return has_order ? WT_PEER_END : WT_PART_END;
    case WFS_ROWS_CURRENT: return WT_SELF;
    // without ORDER BY every row of a partition is a peer of every other
    case WFS_RANGE_CURRENT: return has_order ? WT_PEER_END : WT_PART_END;
    default: return WT_PART_END;
  }
}

inline const char *WinTargetName(WinTarget t) {
  return t == WT_SELF ? "ROWS TO CURRENT ROW" : t == WT_PEER_END ? "RANGE TO CURRENT ROW" : "WHOLE PARTITION";
}

// Calls with one (partition keys, order items) specification share its sort
// and its boundaries.  spec_of[i] <- the dense number of call i's
// specification, in order of first appearance; returns how many there are.
template <typename Same>
inline int WinGroupSpecs(int n, Same same, int *spec_of) {
  int nspec = 0;
  for (int i = 0; i < n; i++) {
    spec_of[i] = -1;
    for (int j = 0; j < i && spec_of[i] < 0; j++)
      if (same(j, i)) spec_of[i] = spec_of[j];
    if (spec_of[i] < 0) spec_of[i] = nspec++;
  }
  return nspec;
}

// ---- running states ------------------------------------------------------------
// Each is as narrow as its calls need; `Of` makes the state of one input row.

// COUNT(x), DENSE_RANK (a count of peer-group starts)
struct WinCount {
  typedef uint64_t State;
  static MBX_WN_HD State Identity() { return 0; }
  static MBX_WN_HD void Merge(State &a, const State &b) { a += b; }
};

// the first position of a segment: a minimum over positions
struct WinPosMin {
  typedef int64_t State;
  static MBX_WN_HD State Identity() { return INT64_MAX; }
  static MBX_WN_HD void Merge(State &a, const State &b) { a = b < a ? b : a; }
};

// SUM / AVG of integers and DECIMALs: the count of values and their carrying int128 sum
struct WinSum128 {
  struct State {
    uint64_t count, lo;
    int64_t hi;
  };
  static MBX_WN_HD State Identity() { return {0, 0, 0}; }
  static MBX_WN_HD State Of(int64_t lo, int64_t hi) { return {1, (uint64_t)lo, hi}; }
  // the add carries from the low word into the high one (as JoinAggMerge's)
  static MBX_WN_HD void Merge(State &a, const State &b) {
    a.count += b.count;
    const uint64_t lo = a.lo + b.lo;
    a.hi = (int64_t)((uint64_t)a.hi + (uint64_t)b.hi + (lo < a.lo ? 1u : 0u));
    a.lo = lo;
  }
};

// SUM / AVG of DOUBLE.  An empty side leaves the other as it is, the sign of a zero included.
struct WinSumF {
  struct State {
    uint64_t count;
    double sum;
  };
  static MBX_WN_HD State Identity() { return {0, 0.0}; }
  static MBX_WN_HD State Of(double v) { return {1, v}; }
  static MBX_WN_HD void Merge(State &a, const State &b) {
    if (b.count == 0) return;
    if (a.count == 0) {
      a = b;
      return;
    }
    a.count += b.count;
    a.sum += b.sum;
  }
};

// MIN / MAX of a value of at most 64 bits as an order-preserving unsigned key
// (signed: value ^ 2^63; unsigned: the value; DOUBLE: the order encoding)
template <bool kMax>
struct WinMinMax64 {
  struct State {
    uint64_t count, key;
  };
  static MBX_WN_HD State Identity() { return {0, kMax ? 0ull : 0xFFFFFFFFFFFFFFFFull}; }
  static MBX_WN_HD State Of(uint64_t key) { return {1, key}; }
  static MBX_WN_HD void Merge(State &a, const State &b) {
    a.count += b.count;
    if (kMax ? b.key > a.key : b.key < a.key) a.key = b.key;
  }
};

// MIN / MAX of HUGEINT and wide DECIMAL: signed high word, unsigned low word
template <bool kMax>
struct WinMinMax128 {
  struct State {
    uint64_t count, lo;
    int64_t hi;
  };
  static MBX_WN_HD State Identity() {
    return kMax ? State{0, 0, INT64_MIN} : State{0, 0xFFFFFFFFFFFFFFFFull, INT64_MAX};
  }
  static MBX_WN_HD State Of(int64_t lo, int64_t hi) { return {1, (uint64_t)lo, hi}; }
  static MBX_WN_HD void Merge(State &a, const State &b) {
    a.count += b.count;
    const bool less = b.hi < a.hi || (b.hi == a.hi && b.lo < a.lo);
    const bool more = b.hi > a.hi || (b.hi == a.hi && b.lo > a.lo);
    if (kMax ? more : less) {
      a.lo = b.lo;
      a.hi = b.hi;
    }
  }
};

// ---- the segmented operator and the scan's shape ----------------------------------
template <typename Op>
struct WinElem {
  uint32_t flag;
  typename Op::State s;
};

// a <- a (+) b
template <typename Op>
MBX_WN_HD void WinCombine(WinElem<Op> &a, const WinElem<Op> &b) {
  if (b.flag) {
    a.s = b.s;
  } else {
    Op::Merge(a.s, b.s);
  }
  a.flag |= b.flag;
}

template <typename Op>
MBX_WN_HD WinElem<Op> WinIdentity() {
  return {0u, Op::Identity()};
}

// The scan's tile, in rows, and the lanes of the one workgroup that scans the
// tiles' carries (it loops when there are more tiles than lanes).  Both fix the
// order in which values are combined, so a DOUBLE running sum depends on the
// row count alone.
constexpr int kWinBlock = 256;
constexpr int kWinItems = 4;
constexpr int kWinTile = kWinBlock * kWinItems;
constexpr int kWinCarryLanes = 256;

MBX_WN_HD int64_t WinTiles(int64_t n, int64_t tile = kWinTile) { return (n + tile - 1) / tile; }

// The three launches on the host, in place over x[0 .. n): (1) every tile's
// elements reduced to its carry, (2) the carries scanned to what each tile
// receives, (3) every tile scanned with what it received.  carry: room for
// WinTiles(n, tile) elements.
template <typename Op>
inline void WinTileScan(WinElem<Op> *x, int64_t n, int64_t tile, WinElem<Op> *carry) {
  const int64_t nt = WinTiles(n, tile);
  for (int64_t t = 0; t < nt; t++) {
    WinElem<Op> r = WinIdentity<Op>();
    for (int64_t i = t * tile; i < n && i < (t + 1) * tile; i++) WinCombine<Op>(r, x[i]);
    carry[t] = r;
  }
  WinElem<Op> run = WinIdentity<Op>();
  for (int64_t t = 0; t < nt; t++) {
    const WinElem<Op> mine = carry[t];
    carry[t] = run;
    WinCombine<Op>(run, mine);
  }
  for (int64_t t = 0; t < nt; t++) {
    WinElem<Op> r = carry[t];
    for (int64_t i = t * tile; i < n && i < (t + 1) * tile; i++) {
      WinCombine<Op>(r, x[i]);
      x[i] = r;
    }
  }
}

}  // namespace mbx
