// Stand-alone host check of csrc/str_minmax.h (tests/test_str_minmax_plan.py
// builds and runs it): the rounds of MIN / MAX over VARCHAR, run in one thread
// with the functions the kernels call and in the kernels' order -- round 0 over
// every row, the rows that are live after it as candidates, the later chunk
// rounds over the candidates with two word buffers in turn, the length tie,
// the row tie -- against a direct StrCompare scan (str_match.h) that keeps the
// lowest row among equal strings.  Strings lie in one character buffer, as a
// column's do, so both forms of the chunk key run: the 8-byte load and, near
// the buffer's end, the byte loop.  Prints "str minmax plan: ok" or the first
// failed check.
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "str_match.h"
#include "str_minmax.h"

using namespace mbx;

#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
      exit(1);                                                \
    }                                                         \
  } while (0)

struct Row {
  bool valid;
  std::string s;
};
static Row V(const std::string &s) { return Row{true, s}; }
static Row Null() { return Row{false, ""}; }

struct Column {
  std::vector<int64_t> off;
  std::vector<uint8_t> chars;  // exactly chars_len bytes: ASan sees a read past them
  std::vector<bool> valid;
};
static Column ColumnOf(const std::vector<Row> &rows) {
  Column c;
  c.off.push_back(0);
  for (auto &r : rows) {
    if (r.valid) c.chars.insert(c.chars.end(), r.s.begin(), r.s.end());
    c.off.push_back((int64_t)c.chars.size());
    c.valid.push_back(r.valid);
  }
  c.chars.shrink_to_fit();
  return c;
}

struct Winners {
  int64_t row[SMM_KINDS];  // -1: none
  int chunks;              // of the run
};

static uint64_t KeyOf(const Column &c, int r, int chunks, int64_t row) {
  const int64_t b = c.off[row], len = c.off[row + 1] - b;
  return StrMinMaxKey(r, chunks, c.chars.data() + b, len, (int64_t)c.chars.size() - b, row);
}

// the rounds, as the executor launches them
static Winners Run(const Column &c) {
  const int64_t n = (int64_t)c.valid.size();
  uint64_t words[2][SMM_KINDS];
  // round 0 over every row (the number of chunks is not known yet and does not matter to it)
  for (int k = 0; k < SMM_KINDS; k++) words[0][k] = StrMinMaxInitWord(k, 0, 1);
  for (int64_t i = 0; i < n; i++) {
    if (!c.valid[i]) continue;
    const uint64_t key = KeyOf(c, 0, 1, i);
    for (int k = 0; k < SMM_KINDS; k++)
      words[0][k] = StrMinMaxOffer(StrMinMaxTakesLeast(k, 0, 1), key, words[0][k]);
  }
  // the candidates and their longest string
  std::vector<uint64_t> cand;
  int64_t maxlen = 0;
  for (int64_t i = 0; i < n; i++) {
    if (!c.valid[i]) continue;
    const uint64_t key = KeyOf(c, 0, 1, i);
    int live = 0;
    for (int k = 0; k < SMM_KINDS; k++) live |= StrMinMaxStaysLive(key, words[0][k]) ? 1 << k : 0;
    if (!live) continue;
    cand.push_back(StrMinMaxCand(i, live));
    maxlen = std::max<int64_t>(maxlen, c.off[i + 1] - c.off[i]);
  }
  Winners w;
  w.chunks = StrMinMaxChunks(maxlen);
  const int rounds = StrMinMaxRounds(w.chunks);
  CHECK(rounds == w.chunks + 2);
  for (int r = 1; r < rounds; r++) {
    uint64_t *prev = words[(r - 1) & 1], *cur = words[r & 1];
    for (int k = 0; k < SMM_KINDS; k++) cur[k] = StrMinMaxInitWord(k, r, w.chunks);
    for (auto &cd : cand) {
      const int64_t row = StrMinMaxCandRow(cd);
      int live = StrMinMaxCandLive(cd);
      const uint64_t pkey = KeyOf(c, r - 1, w.chunks, row), key = KeyOf(c, r, w.chunks, row);
      for (int k = 0; k < SMM_KINDS; k++) {
        if (!(live >> k & 1)) continue;
        if (!StrMinMaxStaysLive(pkey, prev[k])) {
          live &= ~(1 << k);
          continue;
        }
        const bool least = StrMinMaxTakesLeast(k, r, w.chunks);
        // (the kernels skip the atomic exactly when this is false)
        if (StrMinMaxImproves(least, key, cur[k])) cur[k] = StrMinMaxOffer(least, key, cur[k]);
      }
      cd = StrMinMaxCand(row, live);
    }
  }
  const uint64_t *last = words[(rounds - 1) & 1];
  for (int k = 0; k < SMM_KINDS; k++) {
    // (a run with a single round: cannot happen, rounds >= 3)
    w.row[k] = last[k] == kStrMinMaxNoRow ? -1 : (int64_t)last[k];
    if (cand.empty()) CHECK(w.row[k] == -1);
  }
  return w;
}

static Winners Direct(const std::vector<Row> &rows) {
  Winners w;
  w.row[0] = w.row[1] = -1;
  w.chunks = 0;
  for (int64_t i = 0; i < (int64_t)rows.size(); i++) {
    if (!rows[i].valid) continue;
    for (int k = 0; k < SMM_KINDS; k++) {
      if (w.row[k] < 0) {
        w.row[k] = i;
        continue;
      }
      const std::string &a = rows[i].s, &b = rows[w.row[k]].s;
      const int cmp = StrCompare((const uint8_t *)a.data(), (int64_t)a.size(), (const uint8_t *)b.data(), (int64_t)b.size());
      if (k == SMM_MIN ? cmp < 0 : cmp > 0) w.row[k] = i;  // strictly better only: the lowest row of equals stays
    }
  }
  return w;
}

static Winners Check(const std::vector<Row> &rows) {
  const Winners got = Run(ColumnOf(rows)), want = Direct(rows);
  for (int k = 0; k < SMM_KINDS; k++) {
    if (got.row[k] != want.row[k])
      fprintf(stderr, "kind %d: row %lld, expected %lld (%zu rows)\n", k, (long long)got.row[k], (long long)want.row[k],
              rows.size());
    CHECK(got.row[k] == want.row[k]);
  }
  return got;
}

static std::string Rep(char ch, int n) { return std::string((size_t)n, ch); }

int main() {
  // the functions themselves
  CHECK(StrMinMaxChunks(0) == 1 && StrMinMaxChunks(1) == 1 && StrMinMaxChunks(8) == 1 && StrMinMaxChunks(9) == 2);
  CHECK(StrMinMaxChunks(16) == 2 && StrMinMaxChunks(17) == 3 && StrMinMaxChunks(24) == 3 && StrMinMaxChunks(25) == 4);
  CHECK(StrMinMaxInitWord(SMM_MIN, 0, 1) == ~0ull && StrMinMaxInitWord(SMM_MAX, 0, 1) == 0);
  CHECK(StrMinMaxInitWord(SMM_MIN, 1, 1) == ~0ull && StrMinMaxInitWord(SMM_MAX, 1, 1) == 0);  // the length
  CHECK(StrMinMaxInitWord(SMM_MIN, 2, 1) == ~0ull && StrMinMaxInitWord(SMM_MAX, 2, 1) == ~0ull);  // the row
  {
    const uint8_t b[12] = {'a', 'b', 'c', 'd', 'e', 'f', 'g', 'h', 'i', 0x80, 0xFF, 'z'};
    CHECK(StrMinMaxChunkKey(b, 0, 12, 0) == 0);
    CHECK(StrMinMaxChunkKey(b, 1, 12, 0) == 0x6100000000000000ull);
    CHECK(StrMinMaxChunkKey(b, 1, 1, 0) == 0x6100000000000000ull);  // the byte loop
    CHECK(StrMinMaxChunkKey(b, 8, 12, 0) == 0x6162636465666768ull);
    CHECK(StrMinMaxChunkKey(b, 8, 8, 0) == 0x6162636465666768ull);
    CHECK(StrMinMaxChunkKey(b, 11, 12, 1) == 0x6980FF0000000000ull);  // bytes past the buffer's 8-byte reach: loop
    CHECK(StrMinMaxChunkKey(b, 12, 12, 1) == 0x6980FF7A00000000ull);
    CHECK(StrMinMaxChunkKey(b, 12, 12, 2) == 0);
    for (int len = 0; len <= 12; len++)
      for (int c = 0; c < 3; c++)
        CHECK(StrMinMaxChunkKey(b, len, 12, c) == StrMinMaxChunkKey(b, len, len, c));  // both forms agree
  }
  // every length around the chunk borders, distinct strings and a shared first letter
  {
    std::vector<Row> rows;
    for (int len : {0, 1, 7, 8, 9, 15, 16, 17, 24, 25}) rows.push_back(V(Rep('m', len)));
    Winners w = Check(rows);
    CHECK(w.row[SMM_MIN] == 0 && w.row[SMM_MAX] == 9 && w.chunks == 4);
    for (int len : {0, 1, 7, 8, 9, 15, 16, 17, 24, 25}) {
      Check({V(Rep('q', len))});
      Check({V(Rep('q', len)), V(Rep('q', len) + "a"), V(Rep('q', len) + "b")});
      Check({V(Rep('q', len) + "b"), V(Rep('q', len)), Null(), V(Rep('q', len) + "a")});
    }
  }
  // ties on the first 8 and on the first 16 bytes
  Check({V("prefix08b"), V("prefix08a"), V("prefix08c"), V("prefix08")});
  Check({V("prefix08prefix16y"), V("prefix08prefix16x"), V("prefix08prefix16z"), V("prefix08prefix16")});
  Check({V("prefix08prefix16y"), V("prefix08b"), V("prefix08prefix16x"), V("prefix07")});
  // trailing NUL bytes: equal keys in every chunk, the length decides
  {
    const std::string a("a"), a0("a\0", 2), a00("a\0\0", 3);
    Winners w = Check({V(a0), V(a), V(a00)});
    CHECK(w.row[SMM_MIN] == 1 && w.row[SMM_MAX] == 2);
    w = Check({V(a00), V(a0), V(a), V(a00), V(a)});
    CHECK(w.row[SMM_MIN] == 2 && w.row[SMM_MAX] == 0);
    Check({V(std::string("\0", 1)), V(""), V(std::string("\0\0", 2))});
    Check({V(Rep('k', 8) + std::string("\0", 1)), V(Rep('k', 8)), V(Rep('k', 8) + std::string("\0\0", 2))});
  }
  // unsigned bytes: 0x80 and above are greater than ASCII
  {
    Winners w = Check({V("z"), V("\xC3\xA9"), V("\xE6\x97\xA5\xE6\x9C\xAC"), V("a")});
    CHECK(w.row[SMM_MIN] == 3 && w.row[SMM_MAX] == 2);
    Check({V("\x80"), V("\x7F"), V("\xFF"), V("")});
  }
  // eight 0xFF bytes: the MIN word's initial value is this row's key
  {
    Winners w = Check({V(Rep('\xFF', 8))});
    CHECK(w.row[SMM_MIN] == 0 && w.row[SMM_MAX] == 0);
    Check({V(Rep('\xFF', 8)), V(Rep('\xFF', 8))});
    Check({V(Rep('\xFF', 9)), V(Rep('\xFF', 8)), V(Rep('\xFF', 16))});
  }
  // '' only: the MAX word's initial value is this row's key
  {
    Winners w = Check({Null(), V(""), V("")});
    CHECK(w.row[SMM_MIN] == 1 && w.row[SMM_MAX] == 1);
    Check({V("")});
    Check({V(""), Null(), V("a")});
  }
  // all equal: the lowest row
  {
    Winners w = Check({Null(), V("same string, 21 bytes"), V("same string, 21 bytes"), V("same string, 21 bytes")});
    CHECK(w.row[SMM_MIN] == 1 && w.row[SMM_MAX] == 1);
  }
  // no non-NULL row: no winner
  {
    Winners w = Check({Null(), Null()});
    CHECK(w.row[SMM_MIN] == -1 && w.row[SMM_MAX] == -1);
    Check({});
  }
  // seeded random sets over a small alphabet: many ties in every round
  uint64_t seed = 0x9E3779B97F4A7C15ull;
  auto next = [&]() {
    seed = seed * 6364136223846793005ull + 1442695040888963407ull;
    return (uint32_t)(seed >> 33);
  };
  for (int set = 0; set < 200; set++) {
    std::vector<Row> rows;
    const int n = 1 + (int)(next() % 40);
    for (int i = 0; i < n; i++) {
      if (next() % 8 == 0) {
        rows.push_back(Null());
        continue;
      }
      const int len = (int)(next() % 21);
      std::string s;
      // long common prefixes: a letter is repeated with probability 3/4
      for (int j = 0; j < len; j++) s.push_back(j > 0 && next() % 4 ? s[j - 1] : (char)('a' + next() % 3));
      rows.push_back(V(s));
    }
    Check(rows);
  }
  printf("str minmax plan: ok\n");
  return 0;
}
