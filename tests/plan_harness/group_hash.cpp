// Stand-alone host check of csrc/group_hash.h (tests/test_group_hash_plan.py
// builds and runs it): the hash GROUP BY's table through the header's own
// insert walk with a single-threaded claim -- the capacity rule, the entry
// packing, chains of keys that share the last slot of the table and wrap to
// slot 0, pairs of different keys with equal tag and equal home slot (both
// found here by brute force against the header's hash, for BIGINT keys and for
// 8-byte strings), what makes two fixed-width, float or string keys equal,
// a lost compare-and-swap, and the bounded-walk verdict on a table without an
// empty slot.  Prints "group hash: ok" or the first failed check.  With the
// argument `hashes` it prints the 64-bit hash of a fixed list of key rows
// instead (tests/hash_group_model.py restates them).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <limits>
#include <set>
#include <string>
#include <utility>
#include <vector>

#include "group_hash.h"

using namespace mbx;

#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
      exit(1);                                                \
    }                                                         \
  } while (0)

// ---- key rows as the kernel sees them --------------------------------------------------------------
struct Cell {
  enum Kind { NUL, WORDS, FLOAT, STR } kind;
  uint64_t w0, w1;
  std::string s;
};
typedef std::vector<Cell> Row;

static Cell Null() { return Cell{Cell::NUL, 0, 0, ""}; }
static Cell Words(uint64_t lo, uint64_t hi) { return Cell{Cell::WORDS, lo, hi, ""}; }
static Cell BigInt(int64_t v) { return Words((uint64_t)v, (uint64_t)(v >> 63)); }  // load_phys: sign-extended
static Cell Str(const std::string &s) { return Cell{Cell::STR, 0, 0, s}; }
static uint64_t Bits(double d) {
  uint64_t b;
  memcpy(&b, &d, 8);
  return b;
}
static Cell DoubleBits(uint64_t bits) { return Cell{Cell::FLOAT, bits, 0, ""}; }
static Cell Double(double d) { return DoubleBits(Bits(d)); }

// key_bits of kernels.hip
static void KeyBits(const Cell &c, uint64_t &w0, uint64_t &w1) {
  w0 = c.kind == Cell::FLOAT ? GroupFloatBits(c.w0) : c.w0;
  w1 = c.w1;
}

// row_hash of kernels.hip
static uint64_t RowHash(const Row &r) {
  uint64_t h = kGroupHashSeed;
  for (const Cell &c : r) {
    if (c.kind == Cell::NUL) {
      h = GroupHashNull(h);
    } else if (c.kind == Cell::STR) {
      h = GroupHashString(h, c.s.data(), (int64_t)c.s.size());
    } else {
      uint64_t w0, w1;
      KeyBits(c, w0, w1);
      h = GroupHashWords(h, w0, w1);
    }
  }
  return h;
}

// rows_equal of kernels.hip
static bool RowsEqual(const Row &a, const Row &b) {
  CHECK(a.size() == b.size());
  for (size_t j = 0; j < a.size(); j++) {
    const bool va = a[j].kind != Cell::NUL, vb = b[j].kind != Cell::NUL;
    if (va != vb) return false;
    if (!va) continue;
    CHECK(a[j].kind == b[j].kind);
    if (a[j].kind == Cell::STR) {
      if (!GroupStringsEqual(a[j].s.data(), (int64_t)a[j].s.size(), b[j].s.data(), (int64_t)b[j].s.size())) return false;
    } else {
      uint64_t a0, a1, b0, b1;
      KeyBits(a[j], a0, a1);
      KeyBits(b[j], b0, b1);
      if (a0 != b0 || a1 != b1) return false;
    }
  }
  return true;
}

// ---- the table: what the device does with a relaxed load and atomicCAS, single-threaded ----------
struct Table {
  std::vector<uint64_t> slot;
  std::vector<Row> rows;
  int64_t loads = 0;
  explicit Table(int64_t cap) : slot((size_t)cap, kGroupEmpty) { CHECK(cap > 0 && (cap & (cap - 1)) == 0); }
  int64_t cap() const { return (int64_t)slot.size(); }
  // appends the row and inserts it; the slot of its group or kGroupTableFull
  int64_t Insert(const Row &r) {
    rows.push_back(r);
    const int64_t me = (int64_t)rows.size() - 1;
    return GroupInsert(
        RowHash(r), me, (uint64_t)cap() - 1,
        [&](uint64_t e) {
          loads++;
          return slot[e];
        },
        [&](uint64_t e, uint64_t expected, uint64_t desired) {
          const uint64_t prev = slot[e];
          if (prev == expected) slot[e] = desired;
          return prev;
        },
        [&](int64_t other) { return RowsEqual(rows[(size_t)other], rows[(size_t)me]); });
  }
  int64_t Occupied() const { return (int64_t)std::count_if(slot.begin(), slot.end(), [](uint64_t v) { return v != kGroupEmpty; }); }
};

static int64_t Home(const Row &r, int64_t cap) { return (int64_t)(RowHash(r) & (uint64_t)(cap - 1)); }

// n distinct keys -> n entries, and each key a second time -> its own entry again
static void Distinct(const std::vector<Row> &keys, int64_t cap) {
  Table t(cap);
  std::vector<int64_t> at;
  std::set<int64_t> seen;
  for (const Row &k : keys) {
    const int64_t s = t.Insert(k);
    CHECK(s >= 0 && s < cap);
    CHECK(seen.insert(s).second);  // every key owns an entry
    CHECK(GroupEntryRow(t.slot[(size_t)s]) == (int64_t)t.rows.size() - 1);
    CHECK(GroupEntryTag(t.slot[(size_t)s]) == GroupTag(RowHash(k)));
    at.push_back(s);
  }
  for (size_t i = keys.size(); i-- > 0;) CHECK(t.Insert(keys[i]) == at[i]);
  CHECK(t.Occupied() == (int64_t)keys.size());
}

// ---- the checks ---------------------------------------------------------------------------------------
static void Capacity() {
  CHECK(GroupCapacity(0) == 1024);
  CHECK(GroupCapacity(1) == 1024);
  CHECK(GroupCapacity(512) == 1024);
  CHECK(GroupCapacity(513) == 2048);
  CHECK(GroupCapacity(1024) == 2048);
  CHECK(GroupCapacity(1025) == 4096);
  CHECK(GroupCapacity(70001) == 262144);
  for (int64_t n = 0; n <= 512; n++) CHECK(GroupCapacity(n) == 1024);
  for (int64_t n = 513; n < 70000; n += 7) {
    const int64_t c = GroupCapacity(n);
    CHECK((c & (c - 1)) == 0 && c >= 2 * n && c / 2 < 2 * n);
  }
  const int64_t top = (int64_t)1 << 30;
  CHECK(GroupCapacity(top / 2 - 1) == top);
  CHECK(GroupCapacity(top / 2) == top);
  CHECK(GroupCapacity(top / 2 + 1) == top);
  CHECK(GroupCapacity(top) == top);
  CHECK(GroupCapacity(top + 1) == top);  // (HashAggregate refuses more than kGroupMaxRows rows)
  CHECK(GroupCapacity(std::numeric_limits<int64_t>::max() / 2) == top);
  CHECK(kGroupMaxRows == top && kGroupMaxCapacity == top && kGroupMinCapacity == 1024);
}

static void Packing() {
  CHECK(kGroupTagShift == 40 && kGroupRowMask == 0xFFFFFFFFFFull && kGroupEmpty == ~0ull);
  const uint64_t h = 0xABCDEF0123456789ull;
  CHECK(GroupTag(h) == 0xABCDEFull);
  const uint64_t e = GroupEntry(GroupTag(h), 0x12345678);
  CHECK(e == 0xABCDEF0012345678ull);
  CHECK(GroupEntryTag(e) == 0xABCDEFull && GroupEntryRow(e) == 0x12345678);
  // no row the path admits packs to the empty word, whatever its tag
  CHECK(GroupEntry(0xFFFFFF, kGroupMaxRows - 1) != kGroupEmpty);
  CHECK(GroupEntryRow(GroupEntry(0xFFFFFF, kGroupMaxRows - 1)) == kGroupMaxRows - 1);
  CHECK(GroupEntry(0, 0) == 0);
}

// the candidates of the searches: i * 1000003, or the 8-digit decimal spelling of i
static Row Candidate(bool str, int64_t i) {
  if (!str) return Row{BigInt(i * 1000003)};
  char buf[16];
  snprintf(buf, sizeof buf, "%08lld", (long long)i);
  return Row{Str(buf)};
}
constexpr int64_t kSearch = (int64_t)1 << 22;

// >= 250 keys whose home is the last slot of a 1024-entry table: the chain wraps to slot 0
static void WrappingChain(bool str) {
  const int64_t cap = 1024;
  std::vector<Row> keys;
  for (int64_t i = 0; i < kSearch && keys.size() < 300; i++) {
    Row r = Candidate(str, i);
    if (Home(r, cap) == cap - 1) keys.push_back(r);
  }
  CHECK(keys.size() >= 250);
  Distinct(keys, cap);
  Table t(cap);
  for (size_t i = 0; i < keys.size(); i++) CHECK(t.Insert(keys[i]) == (int64_t)((cap - 1 + i) % cap));
  // each key again, the twins far apart: the same entries, no new one
  for (size_t i = 0; i < keys.size(); i++) CHECK(t.Insert(keys[i]) == (int64_t)((cap - 1 + i) % cap));
  CHECK(t.Occupied() == (int64_t)keys.size());
  CHECK(t.slot[1023] != kGroupEmpty && t.slot[0] != kGroupEmpty && t.slot[keys.size() - 1] == kGroupEmpty);
}

// >= 100 pairs of different keys with equal tag and equal home slot: only rows_equal tells them apart
static void TagPairs(bool str) {
  const int64_t cap = 1024;
  std::vector<std::pair<uint64_t, int64_t>> byhash;
  byhash.reserve((size_t)kSearch);
  for (int64_t i = 0; i < kSearch; i++) {
    const uint64_t h = RowHash(Candidate(str, i));
    byhash.push_back({(GroupTag(h) << kGroupTagShift) | (h & (uint64_t)(cap - 1)), i});
  }
  std::sort(byhash.begin(), byhash.end());
  std::vector<std::pair<Row, Row>> pairs;
  for (size_t j = 0; j + 1 < byhash.size(); j++) {
    if (byhash[j].first == byhash[j + 1].first) {
      pairs.push_back({Candidate(str, byhash[j].second), Candidate(str, byhash[j + 1].second)});
      j++;
    }
  }
  CHECK(pairs.size() >= 100);
  Table t(GroupCapacity((int64_t)pairs.size() * 3));
  for (auto &p : pairs) {
    CHECK(!RowsEqual(p.first, p.second));
    CHECK(GroupTag(RowHash(p.first)) == GroupTag(RowHash(p.second)));
    const int64_t before = t.Occupied();
    const int64_t a = t.Insert(p.first), b = t.Insert(p.second);
    CHECK(a >= 0 && b >= 0 && a != b);
    CHECK(t.Occupied() == before + 2);
    CHECK(t.Insert(p.second) == b && t.Insert(p.first) == a);  // a repeated key gets no entry
    CHECK(t.Occupied() == before + 2);
  }
  // and in one 1024-entry table, where the two share the home slot itself
  for (size_t i = 0; i < 100; i++) {
    Table s(cap);
    const int64_t a = s.Insert(pairs[i].first), b = s.Insert(pairs[i].second);
    CHECK(a == Home(pairs[i].first, cap) && b == (a + 1) % cap);
    CHECK(s.Insert(pairs[i].first) == a && s.Insert(pairs[i].second) == b && s.Occupied() == 2);
  }
}

static void FixedWidthKeys() {
  const uint64_t m1 = ~0ull;
  // (lo, hi): -1 as HUGEINT, 2^64 - 1, 2^64, 0
  Distinct({Row{Words(m1, m1)}, Row{Words(m1, 0)}, Row{Words(0, 1)}, Row{Words(0, 0)}}, 1024);
  std::set<uint64_t> hs = {RowHash(Row{Words(m1, m1)}), RowHash(Row{Words(m1, 0)}), RowHash(Row{Words(0, 1)}),
                           RowHash(Row{Words(0, 0)}), RowHash(Row{Words(1, 0)}), RowHash(Row{Words(1, 1)})};
  CHECK(hs.size() == 6);  // the high word reaches the hash
  // UBIGINT 2^63 (hi = 0) and BIGINT -2^63 (hi = -1) are different words
  CHECK(!RowsEqual(Row{Words(1ull << 63, 0)}, Row{BigInt(std::numeric_limits<int64_t>::min())}));

  // DOUBLE: one zero, one NaN
  const double inf = std::numeric_limits<double>::infinity();
  const uint64_t qnan = 0x7FF8000000000000ull, nnan = 0xFFF8000000000000ull, pnan = 0xFFF8000000000001ull,
                 snan = 0x7FF0000000000001ull;
  CHECK(GroupFloatBits(Bits(-0.0)) == 0 && GroupFloatBits(Bits(0.0)) == 0);
  for (uint64_t n : {qnan, nnan, pnan, snan}) CHECK(GroupFloatBits(n) == kGroupQuietNaN);
  for (double d : {inf, -inf, 5e-324, -5e-324, 1.5, -2.5, 1e300, std::numeric_limits<double>::min()})
    CHECK(GroupFloatBits(Bits(d)) == Bits(d));
  CHECK(RowsEqual(Row{Double(0.0)}, Row{Double(-0.0)}) && RowHash(Row{Double(0.0)}) == RowHash(Row{Double(-0.0)}));
  for (uint64_t n : {nnan, pnan, snan}) {
    CHECK(RowsEqual(Row{DoubleBits(qnan)}, Row{DoubleBits(n)}));
    CHECK(RowHash(Row{DoubleBits(qnan)}) == RowHash(Row{DoubleBits(n)}));
  }
  {
    Table t(1024);
    const int64_t z = t.Insert(Row{Double(0.0)}), n = t.Insert(Row{DoubleBits(qnan)});
    CHECK(t.Insert(Row{Double(-0.0)}) == z);
    CHECK(t.Insert(Row{DoubleBits(nnan)}) == n && t.Insert(Row{DoubleBits(pnan)}) == n);
    CHECK(t.Occupied() == 2);
  }
  Distinct({Row{Double(0.0)}, Row{DoubleBits(qnan)}, Row{Double(inf)}, Row{Double(-inf)}, Row{Double(5e-324)},
            Row{Double(1.5)}, Row{Double(-1.5)}, Row{Double(-5e-324)}}, 1024);

  // FLOAT: load_phys widens to double; the widened value is its own canonical form
  for (float f : {16777216.0f, 16777218.0f, 0.1f, 1e-45f, -1e-45f, 3.4028235e38f, -16777216.0f}) {
    const double d = f;
    CHECK(GroupFloatBits(Bits(d)) == Bits(d) && (float)d == f);
  }
  CHECK(GroupFloatBits(Bits((double)-0.0f)) == 0);
  CHECK(GroupFloatBits(Bits((double)std::numeric_limits<float>::quiet_NaN())) == kGroupQuietNaN);
  CHECK(GroupFloatBits(Bits((double)-std::numeric_limits<float>::quiet_NaN())) == kGroupQuietNaN);
  Distinct({Row{Double(16777216.0f)}, Row{Double(16777218.0f)}, Row{Double(0.1f)}, Row{Double(0.1)}}, 1024);
}

static void Strings() {
  // '' is a key of its own, and not NULL
  CHECK(!RowsEqual(Row{Str("")}, Row{Null()}));
  CHECK(RowHash(Row{Str("")}) != RowHash(Row{Null()}));
  Distinct({Row{Str("")}, Row{Null()}, Row{Str("ab")}, Row{Str("abc")}, Row{Str("abd")}, Row{Str("bbc")},
            Row{Str(std::string(4097, 'x'))}, Row{Str(std::string(4096, 'x') + "y")}, Row{Str(std::string(4096, 'x'))}},
           1024);
  CHECK(GroupStringsEqual("abc", 3, "abc", 3) && GroupStringsEqual("", 0, "x", 0));
  CHECK(!GroupStringsEqual("ab", 2, "abc", 3) && !GroupStringsEqual("abc", 3, "ab", 2));
  CHECK(!GroupStringsEqual("abc", 3, "abd", 3) && !GroupStringsEqual("abc", 3, "bbc", 3));
  // the length is in the hash: a string and its prefix start from different seeds
  CHECK(GroupStrBegin(2) != GroupStrBegin(3));
  CHECK(RowHash(Row{Str("ab")}) != RowHash(Row{Str("abc")}));
  // bytes >= 0x80 hash as unsigned: FNV-1a by hand, with the byte zero-extended
  const std::string hi = "\xff\x80\xc3\xa9";
  uint64_t f = 0xCBF29CE484222325ull ^ 4;
  for (unsigned v : {0xFFu, 0x80u, 0xC3u, 0xA9u}) f = (f ^ (uint64_t)v) * 0x100000001B3ull;
  CHECK(RowHash(Row{Str(hi)}) == hmix(kGroupHashSeed ^ f));
  CHECK(GroupStrByte(1, (uint8_t)'\xff') == (1ull ^ 0xFFull) * 0x100000001B3ull);
  // two-key rows whose bytes concatenate alike, with '' and NULL on either side
  const std::vector<Row> seven = {Row{Str("ab"), Str("c")},  Row{Str("a"), Str("bc")}, Row{Str(""), Str("abc")},
                                  Row{Null(), Str("abc")},   Row{Str("abc"), Null()},  Row{Null(), Null()},
                                  Row{Str(""), Null()}};
  Distinct(seven, 1024);
  std::set<uint64_t> hs;
  for (const Row &r : seven) hs.insert(RowHash(r));
  CHECK(hs.size() == 7);
}

// a row that loses the compare-and-swap examines the winner's entry
static void LostClaim() {
  const Row mine = {Str("walnut")}, other = {Str("cherry")};
  for (int same = 0; same < 2; same++) {
    std::vector<uint64_t> slot(1024, kGroupEmpty);
    // row 0: the winner (the same key, or another); row 1: the loser
    std::vector<Row> rows = {same ? mine : other, mine};
    const uint64_t h = RowHash(mine), home = h & 1023;
    // the winner's entry as the device would have written it; with the loser's tag in the other-key case too,
    // so that only the key compare can tell them apart
    const uint64_t winner = GroupEntry(GroupTag(h), 0);
    int cas_calls = 0;
    const int64_t got = GroupInsert(
        h, 1, 1023, [&](uint64_t e) { return slot[e]; },
        [&](uint64_t e, uint64_t expected, uint64_t desired) {
          if (cas_calls++ == 0) {  // between this row's load and its swap, the winner stored
            CHECK(e == home && expected == kGroupEmpty);
            slot[e] = winner;
          }
          const uint64_t prev = slot[e];
          if (prev == expected) slot[e] = desired;
          return prev;
        },
        [&](int64_t o) { return RowsEqual(rows[(size_t)o], rows[1]); });
    if (same) {
      CHECK(got == (int64_t)home && cas_calls == 1);  // joined the winner's group
      CHECK(slot[(home + 1) & 1023] == kGroupEmpty);
    } else {
      CHECK(got == (int64_t)((home + 1) & 1023) && cas_calls == 2);
      CHECK(slot[home] == winner && GroupEntryRow(slot[(home + 1) & 1023]) == 1);
    }
  }
}

// a table without an empty slot (a sizing bug on the device): the walk ends after cap steps
static void FullTable() {
  const int64_t cap = 16;
  Table t(cap);
  std::vector<int64_t> at;
  for (int64_t k = 0; k < cap; k++) {
    at.push_back(t.Insert(Row{BigInt(k * 3 + 1)}));
    CHECK(at.back() >= 0);
  }
  CHECK(t.Occupied() == cap);
  const std::vector<uint64_t> before = t.slot;
  t.loads = 0;
  CHECK(t.Insert(Row{BigInt(1000)}) == kGroupTableFull);
  CHECK(t.loads == cap);  // one load per slot, then the verdict
  CHECK(t.Insert(Row{Str("x")}) == kGroupTableFull);
  CHECK(t.slot == before);  // the refused inserts wrote nothing
  for (int64_t k = 0; k < cap; k++) CHECK(t.Insert(Row{BigInt(k * 3 + 1)}) == at[(size_t)k]);  // present keys are found
  CHECK(t.slot == before);
}

// the fixed list of hash_group_model.HASHED_ROWS, in its order
static void PrintHashes() {
  const uint64_t m1 = ~0ull;
  const std::vector<Row> rows = {
      Row{BigInt(0)},
      Row{BigInt(-1)},
      Row{BigInt(std::numeric_limits<int64_t>::min())},
      Row{BigInt(std::numeric_limits<int64_t>::max())},
      Row{BigInt(12345 * 1000003ll)},
      Row{Words(1, 1)},        // HUGEINT 2^64 + 1
      Row{Words(m1, 0)},       // 2^64 - 1
      Row{Words(m1, m1)},      // -1
      Row{Words(1ull << 63, 0)},  // UBIGINT 2^63
      Row{Double(1.5)},
      Row{Double(-0.0)},
      Row{DoubleBits(0xFFF8000000000001ull)},
      Row{Double(5e-324)},
      Row{Str("")},
      Row{Str("a")},
      Row{Str("abc")},
      Row{Str("\xff\x80\xc3\xa9")},
      Row{Str("00001234")},
      Row{Str("seventeen bytes!!")},
      Row{Null()},
      Row{Str("ab"), Null(), BigInt(7)},
  };
  for (const Row &r : rows) printf("%016llx\n", (unsigned long long)RowHash(r));
}

int main(int argc, char **argv) {
  if (argc > 1 && strcmp(argv[1], "hashes") == 0) {
    PrintHashes();
    return 0;
  }
  Capacity();
  Packing();
  for (bool str : {false, true}) {
    WrappingChain(str);
    TagPairs(str);
  }
  FixedWidthKeys();
  Strings();
  LostClaim();
  FullTable();
  printf("group hash: ok\n");
  return 0;
}
