// join_plan.h — the hash table of the inner equi-join (join_kernels.hip): its
// hash, its sizing and its probe sequence, the same functions on the host and
// on the device.
//
// The build side's keys are normalised to int64 and sorted, so equal keys form
// a run of the sorted array; the table holds one entry per DISTINCT key: the
// key and the run's start and length.  Open addressing, linear probing, a
// capacity that is a power of two >= 2 x build rows.  Every key is inserted
// once, so an inserter never compares keys: it claims the first empty slot on
// its probe sequence with one compare-and-swap on the entry's 32-bit length
// word (0 = empty; a run has at least one row) and then fills in the rest.
// Build and probe are separate launches: a lookup never sees a half-written
// entry.  One entry is 16 bytes, one load per probe step.
//
// Every walk is bounded by the capacity: an insert into a full table and a
// lookup that meets neither its key nor an empty slot return kJoinTableFull
// (the kernels raise E_JOIN_FULL) and never spin.
// No HIP types: the functions also build in a plain host program
// (tests/plan_harness/join_plan.cpp).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MBX_JP_HD __host__ __device__ __forceinline__
#else
#define MBX_JP_HD inline
#endif

namespace mbx {

struct alignas(16) JoinEntry {
  int64_t key;
  int32_t start;  // of the key's run in the sorted build arrays
  uint32_t len;   // rows of the run; 0: the slot is empty (the claim word)
};

constexpr int64_t kJoinAbsent = -1;     // lookup: the key is not in the table
constexpr int64_t kJoinTableFull = -2;  // no empty slot within `cap` steps
constexpr int64_t kJoinMaxBuildRows = 2147483647;

// murmur3's 64-bit finaliser: every input bit reaches every output bit, so
// keys that differ only above bit 32 (or only in the sign) spread like any
constexpr MBX_JP_HD uint64_t JoinHash(int64_t key) {
  uint64_t h = (uint64_t)key;
  h ^= h >> 33;
  h *= 0xff51afd7ed558ccdull;
  h ^= h >> 33;
  h *= 0xc4ceb9fe1a85ec53ull;
  h ^= h >> 33;
  return h;
}

// the smallest power of two >= 2 x rows (1 for an empty build side)
constexpr MBX_JP_HD int64_t JoinCapacity(int64_t build_rows) {
  int64_t cap = 1;
  while (cap < 2 * build_rows) cap <<= 1;
  return cap;
}

// step `i` of key's probe sequence in a table of `cap` slots (a power of two)
constexpr MBX_JP_HD int64_t JoinSlot(uint64_t hash, int64_t i, int64_t cap) {
  return (int64_t)((hash + (uint64_t)i) & (uint64_t)(cap - 1));
}

// Inserts a key that is not in the table yet.  claim(&len, run_len) stores
// run_len into a length word that is 0 and says whether it did (atomically on
// the device).  Returns the slot, or kJoinTableFull.
template <class Claim>
MBX_JP_HD int64_t JoinInsert(JoinEntry *tab, int64_t cap, int64_t key, int32_t start, uint32_t len, Claim claim) {
  const uint64_t h = JoinHash(key);
  for (int64_t i = 0; i < cap; i++) {
    const int64_t s = JoinSlot(h, i, cap);
    if (claim(&tab[s].len, len)) {
      tab[s].key = key;
      tab[s].start = start;
      return s;
    }
  }
  return kJoinTableFull;
}

// The slot that holds `key`, kJoinAbsent when its probe sequence reaches an
// empty slot first, kJoinTableFull when it reaches neither within cap steps.
// *out is the entry found.
MBX_JP_HD int64_t JoinLookup(const JoinEntry *tab, int64_t cap, int64_t key, JoinEntry *out) {
  const uint64_t h = JoinHash(key);
  for (int64_t i = 0; i < cap; i++) {
    const int64_t s = JoinSlot(h, i, cap);
    const JoinEntry e = tab[s];
    if (e.len == 0) return kJoinAbsent;
    if (e.key == key) {
      *out = e;
      return s;
    }
  }
  return kJoinTableFull;
}

}  // namespace mbx
