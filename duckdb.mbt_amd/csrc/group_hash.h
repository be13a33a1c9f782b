// group_hash.h — the hash table of the hash GROUP BY (hash_insert_kernel in
// kernels.hip, HashAggregate in aggregate.cpp): the hash of a key row, the
// packing of an entry, the sizing and the insert walk, the same functions on
// the host and on the device.
//
// One 64-bit word per slot: the top 24 bits of the row's hash (the tag) over
// the 40-bit index of the group's representative row; all ones is the empty
// word (row 2^40 - 1 never exists: the path takes at most 2^30 rows).  Open
// addressing, linear probing, a capacity that is a power of two: 1024, then
// the power of two >= 2 x rows, at most 2^30.  Every row inserts its own key:
// it claims the first empty slot on its probe sequence with one
// compare-and-swap, or stops at the first entry whose tag and key equal its
// own.  A row that loses the compare-and-swap examines the winner's entry: the
// winner may hold the same key.  The tag is compared before the keys, so most
// foreign entries cost no key load.
//
// The hash of a row folds its keys in order into one 64-bit state with hmix
// (splitmix64's finaliser).  A fixed-width key gives two words (the value's
// low and high 64 bits, sign- or zero-extended by load_phys); a float key is
// canonical first: -0.0 becomes 0.0 and every NaN the one quiet NaN, so that
// equal keys in SQL's sense have equal bits.  A string gives FNV-1a over its
// bytes, read as unsigned, seeded with its length; a NULL gives a constant, so
// '' and NULL differ, and ('ab','c') and ('a','bc') do as well.
//
// The walk is bounded by the capacity: an insert into a table without an empty
// slot and without the key returns kGroupTableFull (the kernel raises
// E_HASH_FULL) and never spins.
// No HIP types: the functions also build in a plain host program
// (tests/plan_harness/group_hash.cpp).
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MBX_GH_HD __host__ __device__ __forceinline__
#else
#define MBX_GH_HD inline
#endif

namespace mbx {

constexpr uint64_t kGroupEmpty = 0xFFFFFFFFFFFFFFFFull;
constexpr int kGroupTagShift = 40;  // a 24-bit tag over a 40-bit row
constexpr uint64_t kGroupRowMask = (1ull << kGroupTagShift) - 1;
constexpr int64_t kGroupTableFull = -1;  // no empty slot and no equal key within `cap` steps
constexpr int64_t kGroupMinCapacity = 1024;
constexpr int64_t kGroupMaxCapacity = (int64_t)1 << 30;  // the table's scan counts in int32
constexpr int64_t kGroupMaxRows = (int64_t)1 << 30;      // one entry per row at most: they always fit

constexpr uint64_t kGroupHashSeed = 0x9E3779B97F4A7C15ull;
constexpr uint64_t kGroupNullWord = 0x5BD1E9955BD1E995ull;
constexpr uint64_t kGroupHighWordAdd = 0x632BE59BD9B4E019ull;
constexpr uint64_t kGroupStrSeed = 0xCBF29CE484222325ull;  // FNV-1a, 64 bits
constexpr uint64_t kGroupStrPrime = 0x100000001B3ull;
constexpr uint64_t kGroupQuietNaN = 0x7FF8000000000000ull;

constexpr MBX_GH_HD uint64_t hmix(uint64_t z) {
  z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
  z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
  return z ^ (z >> 31);
}

// the canonical bits of a DOUBLE key (a FLOAT key arrives widened to double):
// -0.0 groups with 0.0 and every NaN with every other NaN
MBX_GH_HD uint64_t GroupFloatBits(uint64_t bits) {
  double d;
  __builtin_memcpy(&d, &bits, 8);
  if (d == 0.0) d = 0.0;
  if (d != d) return kGroupQuietNaN;
  __builtin_memcpy(&bits, &d, 8);
  return bits;
}

// ---- folding one key into the row's hash --------------------------------------------------------
constexpr MBX_GH_HD uint64_t GroupHashNull(uint64_t h) { return hmix(h ^ kGroupNullWord); }

// a fixed-width key: its low and high words
constexpr MBX_GH_HD uint64_t GroupHashWords(uint64_t h, uint64_t w0, uint64_t w1) {
  h = hmix(h ^ w0);
  return hmix(h ^ (w1 + kGroupHighWordAdd));
}

// a string: FNV-1a over the bytes, the length folded into the seed
constexpr MBX_GH_HD uint64_t GroupStrBegin(int64_t len) { return kGroupStrSeed ^ (uint64_t)len; }
constexpr MBX_GH_HD uint64_t GroupStrByte(uint64_t f, uint8_t byte) { return (f ^ byte) * kGroupStrPrime; }
MBX_GH_HD uint64_t GroupHashString(uint64_t h, const char *chars, int64_t len) {
  uint64_t f = GroupStrBegin(len);
  for (int64_t i = 0; i < len; i++) f = GroupStrByte(f, (uint8_t)chars[i]);
  return hmix(h ^ f);
}

MBX_GH_HD bool GroupStringsEqual(const char *a, int64_t alen, const char *b, int64_t blen) {
  if (alen != blen) return false;
  for (int64_t i = 0; i < alen; i++)
    if (a[i] != b[i]) return false;
  return true;
}

// ---- the entry ------------------------------------------------------------------------------------
constexpr MBX_GH_HD uint64_t GroupTag(uint64_t hash) { return hash >> kGroupTagShift; }
constexpr MBX_GH_HD uint64_t GroupEntry(uint64_t tag, int64_t row) { return (tag << kGroupTagShift) | (uint64_t)row; }
constexpr MBX_GH_HD uint64_t GroupEntryTag(uint64_t entry) { return entry >> kGroupTagShift; }
constexpr MBX_GH_HD int64_t GroupEntryRow(uint64_t entry) { return (int64_t)(entry & kGroupRowMask); }

// ---- the table ------------------------------------------------------------------------------------
// 1024, then the power of two >= 2 x rows, at most 2^30
constexpr MBX_GH_HD int64_t GroupCapacity(int64_t rows) {
  int64_t cap = kGroupMinCapacity;
  while (cap < 2 * rows && cap < kGroupMaxCapacity) cap <<= 1;
  return cap;
}

// Inserts row `row`, whose key hashes to `hash`, into a table of mask + 1 slots
// (a power of two).  load(slot) reads a slot (relaxed on the device);
// cas(slot, expected, desired) stores `desired` into a slot that holds
// `expected` and returns what the slot held (atomically on the device);
// equal(other_row) says whether `other_row` has the key of `row`.  Returns the
// slot of the row's group -- claimed by this call, or found to hold an equal
// key -- or kGroupTableFull.
template <class Load, class Cas, class Equal>
MBX_GH_HD int64_t GroupInsert(uint64_t hash, int64_t row, uint64_t mask, Load load, Cas cas, Equal equal) {
  const uint64_t tag = GroupTag(hash);
  const uint64_t mine = GroupEntry(tag, row);
  uint64_t e = hash & mask;
  for (uint64_t probe = 0; probe <= mask; probe++) {
    uint64_t cur = load(e);
    if (cur == kGroupEmpty) {
      const uint64_t prev = cas(e, kGroupEmpty, mine);
      if (prev == kGroupEmpty) return (int64_t)e;
      cur = prev;  // lost: the winner may hold this row's key
    }
    if (GroupEntryTag(cur) == tag && equal(GroupEntryRow(cur))) return (int64_t)e;
    e = (e + 1) & mask;
  }
  return kGroupTableFull;
}

}  // namespace mbx
