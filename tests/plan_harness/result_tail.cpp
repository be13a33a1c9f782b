// Stand-alone host check of csrc/result_tail.h (tests/test_result_tail_plan.py
// builds and runs it).  The layout: ResultBufferLayout against the arithmetic
// ToHost used before the header existed, written out here once more (the error
// word at 0, the first column at 64, every piece padded to 64 bytes), for 1, 2,
// 15 and 16 columns of 1-, 4-, 8- and 16-byte cells, with and without validity,
// one row and many, with and without the device row count; and against offsets
// worked out by hand.  The decision: ResultTailDecide on every statement shape
// it must refuse, the column-count boundary and the mapped buffer's size.
// Prints "result tail plan: ok" or the first failed check.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "result_tail.h"

using namespace mbx;

#define CHECK(c)                                              \
  do {                                                        \
    if (!(c)) {                                               \
      fprintf(stderr, "%s:%d: %s\n", __FILE__, __LINE__, #c); \
      exit(1);                                                \
    }                                                         \
  } while (0)

// the offsets as ToHostPinned computed them in place
static size_t Before(size_t ncols, const int *cell, const bool *has_valid, int64_t n, int64_t words, bool count_word,
                     std::vector<size_t> &data_off, std::vector<size_t> &valid_off) {
  size_t need = count_word ? 128 : 64;
  for (size_t c = 0; c < ncols; c++) {
    need += ((size_t)n * cell[c] + 63) & ~(size_t)63;
    if (has_valid[c]) need += ((size_t)words * 8 + 63) & ~(size_t)63;
  }
  data_off.assign(ncols, 0);
  valid_off.assign(ncols, 0);
  size_t at = 64;
  if (count_word) at += 64;
  for (size_t c = 0; c < ncols; c++) {
    size_t bytes = (size_t)n * cell[c];
    data_off[c] = at;
    at += (bytes + 63) & ~(size_t)63;
    if (has_valid[c]) {
      valid_off[c] = at;
      size_t vb = (size_t)words * 8;
      at += (vb + 63) & ~(size_t)63;
    }
  }
  CHECK(at == need);
  return need;
}

static void Layouts() {
  const int widths[4] = {1, 4, 8, 16};
  int checked = 0;
  for (size_t ncols : {(size_t)1, (size_t)2, (size_t)15, (size_t)16})
    for (int w0 = 0; w0 < 4; w0++)
      for (int valid = 0; valid < 3; valid++)  // none, all, every other column
        for (int64_t n : {(int64_t)1, (int64_t)0, (int64_t)63, (int64_t)65, (int64_t)1000})
          for (int count_word = 0; count_word < 2; count_word++) {
            int cell[16];
            bool has_valid[16];
            for (size_t c = 0; c < ncols; c++) {
              cell[c] = widths[(w0 + c) % 4];  // w0 first, then the other widths in turn
              has_valid[c] = valid == 1 || (valid == 2 && c % 2 == 0);
            }
            const int64_t words = (n + 63) / 64;
            std::vector<size_t> d, v;
            const size_t need = Before(ncols, cell, has_valid, n, words, count_word != 0, d, v);
            ResultColLayout off[16];
            CHECK(ResultBufferLayout(ncols, cell, has_valid, n, words, count_word != 0, off) == need);
            for (size_t c = 0; c < ncols; c++) {
              CHECK(off[c].data_off == d[c]);
              CHECK(off[c].valid_off == v[c]);
              CHECK(off[c].data_off % 64 == 0 && off[c].valid_off % 64 == 0);
              CHECK(has_valid[c] == (off[c].valid_off != 0));
            }
            // one width for every column: the same check with uniform cells
            for (size_t c = 0; c < ncols; c++) cell[c] = widths[w0];
            const size_t need1 = Before(ncols, cell, has_valid, n, words, count_word != 0, d, v);
            CHECK(ResultBufferLayout(ncols, cell, has_valid, n, words, count_word != 0, off) == need1);
            for (size_t c = 0; c < ncols; c++) CHECK(off[c].data_off == d[c] && off[c].valid_off == v[c]);
            checked++;
          }
  CHECK(checked == 4 * 4 * 3 * 5 * 2);
  // by hand: one row of {8-byte, 16-byte, 4-byte} cells, each with validity:
  // 64 cells, 128 validity, 192, 256, 320, 384; 448 bytes in all
  const int cell[3] = {8, 16, 4};
  const bool hv[3] = {true, true, true};
  ResultColLayout off[3];
  CHECK(ResultBufferLayout(3, cell, hv, 1, 1, false, off) == 448);
  CHECK(off[0].data_off == 64 && off[0].valid_off == 128 && off[1].data_off == 192 && off[1].valid_off == 256 &&
        off[2].data_off == 320 && off[2].valid_off == 384);
  // 16 one-row columns with validity: 64 + 16 * 128 = 2112 bytes
  int c16[16];
  bool v16[16];
  for (int i = 0; i < 16; i++) c16[i] = 16, v16[i] = true;
  ResultColLayout o16[16];
  CHECK(ResultBufferLayout(16, c16, v16, 1, 1, false, o16) == 2112);
  CHECK(o16[15].data_off == 64 + 15 * 128 && o16[15].valid_off == 64 + 15 * 128 + 64);
  CHECK(ResultPad(0) == 0 && ResultPad(1) == 64 && ResultPad(64) == 64 && ResultPad(65) == 128);
}

static ResultTailFacts Takes() {
  ResultTailFacts f;
  f.shape.own_result = true;
  f.ncols = 1;
  f.max_cols = 16;
  f.need = 192;
  f.mapped_bytes = (size_t)64 << 10;
  f.max_segs = 32;
  return f;
}

static void Declines(const ResultTailFacts &f, const char *word) {
  const ResultTailChoice c = ResultTailDecide(f);
  CHECK(!c.take);
  CHECK(strstr(c.reason, word) != nullptr);
}

static void Decisions() {
  ResultTailFacts f = Takes();
  CHECK(ResultTailDecide(f).take);
  CHECK(ResultTailDecide(f).reason[0] == 0);
  CHECK(RelationReachesHostUnchanged(f.shape));
  f = Takes(), f.enabled = false, Declines(f, "mbx_result_tail=false");
  // a subquery's, a device result's, an INSERT's or a CREATE TABLE AS's relation
  f = Takes(), f.shape.own_result = false, Declines(f, "own result");
  CHECK(!RelationReachesHostUnchanged(f.shape));
  f = Takes(), f.shape.having = true, Declines(f, "HAVING");
  CHECK(!RelationReachesHostUnchanged(f.shape));
  f = Takes(), f.shape.order_by = true, Declines(f, "ORDER BY");
  CHECK(!RelationReachesHostUnchanged(f.shape));
  f = Takes(), f.shape.limit = true, Declines(f, "LIMIT");
  CHECK(!RelationReachesHostUnchanged(f.shape));
  f = Takes(), f.shape.offset = true, Declines(f, "OFFSET");
  CHECK(!RelationReachesHostUnchanged(f.shape));
  f = Takes(), f.shape.union_all = true, Declines(f, "UNION");
  CHECK(!RelationReachesHostUnchanged(f.shape));
  f = Takes(), f.shape.computed_output = true, Declines(f, "computed");
  CHECK(!RelationReachesHostUnchanged(f.shape));
  f = Takes(), f.grouped = true, Declines(f, "GROUP BY");
  CHECK(RelationReachesHostUnchanged(f.shape));  // (a GROUP BY may still leave its count on the device)
  f = Takes(), f.varchar = true, Declines(f, "VARCHAR");
  f = Takes(), f.no_hostcopy = true, Declines(f, "mapped buffer");
  // the column boundary: 15 columns are 31 pieces with the error word, 16 are 33
  f = Takes(), f.ncols = 15;
  CHECK(ResultTailDecide(f).take);
  f = Takes(), f.ncols = 16, Declines(f, "mapped buffer");
  f = Takes(), f.ncols = 16, f.max_segs = 33;
  CHECK(ResultTailDecide(f).take);
  f = Takes(), f.ncols = 17, f.max_segs = 64, Declines(f, "more columns");
  f = Takes(), f.ncols = 0, Declines(f, "more columns");
  // the buffer's size: at it the result is taken, one byte above it is not
  f = Takes(), f.need = f.mapped_bytes;
  CHECK(ResultTailDecide(f).take);
  f.need++;
  Declines(f, "mapped buffer");
  // the same decision ToHost makes
  CHECK(ResultFitsMapped(64, 15, 65536, 32, false) && !ResultFitsMapped(64, 16, 65536, 32, false));
  CHECK(ResultFitsMapped(65536, 1, 65536, 32, false) && !ResultFitsMapped(65537, 1, 65536, 32, false));
  CHECK(!ResultFitsMapped(64, 1, 65536, 32, true));
  // the first reason that applies is the one given
  f = Takes(), f.enabled = false, f.shape.having = true, f.grouped = true, Declines(f, "mbx_result_tail=false");
}

int main() {
  Layouts();
  Decisions();
  printf("result tail plan: ok\n");
  return 0;
}
