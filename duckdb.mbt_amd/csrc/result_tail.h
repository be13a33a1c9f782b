// result_tail.h — how a small fixed-width result lies in a host buffer, and
// which statements may have their last kernel write it there.
//
// ToHost lands every column of a result in one host buffer (the coherent
// mapped buffer for small results, the pinned arena otherwise) and waits on
// the stream once.  The layout: the device error word at byte 0, the device
// row count at 64 when it rides along, then for every column its cells and,
// where it has a validity bitmap, its 64-bit validity words; every piece is
// padded to 64 bytes.
//
// The one-row relation of an aggregate without GROUP BY is written by one
// workgroup (emit_agg_body).  Where that relation is the statement's own
// result and goes to the host as it stands, the workgroup stores the cells
// straight into the mapped buffer in this layout (EmitDesc::host) and ToHost
// waits and reads, with no copy kernel in between: the result tail.
// ResultTailDecide says which statements take it; ResultFitsMapped is the
// copy decision ToHost makes, shared so the two cannot drift apart.
//
//
// The first 64-byte line holds the error word at [0, 4) and, at
// [kTailTicketOffset, kTailTicketOffset + 8), the ticket of the result tail:
// the 64-bit count of the statement whose row the buffer holds, stored last by
// the emitting thread with release at system scope (EmitDesc::host.ticket_dst,
// tail_wait.h).  Nothing else writes that word: host_copy_kernel leaves it
// alone, and the buffer is zeroed when it is allocated, so it reads 0 until
// the first tail.  ResultBufferLayout never places a column below byte 64.
//
// Plain C++, no HIP: the executor includes it, and so does a host test.
#pragma once
#include <cstddef>
#include <cstdint>

namespace mbx {

constexpr size_t kTailTicketOffset = 8;

constexpr size_t ResultPad(size_t bytes) { return (bytes + 63) & ~(size_t)63; }

struct ResultColLayout {
  size_t data_off;
  size_t valid_off;  // 0: the column has no validity bitmap
};

// The offsets of ncols columns of n rows each (cell_bytes[c] bytes a cell,
// valid_words 64-bit validity words where has_valid[c]) into off[0 .. ncols);
// count_word: the device row count rides at byte 64.  Returns the bytes the
// buffer needs.
inline size_t ResultBufferLayout(size_t ncols, const int *cell_bytes, const bool *has_valid, int64_t n,
                                 int64_t valid_words, bool count_word, ResultColLayout *off) {
  size_t at = count_word ? 128 : 64;
  for (size_t c = 0; c < ncols; c++) {
    off[c].data_off = at;
    at += ResultPad((size_t)n * (size_t)cell_bytes[c]);
    off[c].valid_off = 0;
    if (has_valid[c]) {
      off[c].valid_off = at;
      at += ResultPad((size_t)valid_words * 8);
    }
  }
  return at;
}

// The copy decision: a result of `need` bytes in ncols columns goes through
// the mapped buffer (one kernel writes every piece and the error word, at most
// max_segs pieces) and not by one DMA per piece.
inline bool ResultFitsMapped(size_t need, size_t ncols, size_t mapped_bytes, size_t max_segs, bool no_hostcopy) {
  return need <= mapped_bytes && ncols * 2 + 1 <= max_segs && !no_hostcopy;
}

// A statement whose aggregate relation reaches the host unchanged: the
// top-level SELECT of a materialized query (not a subquery, a device result, an
// INSERT's or a CREATE TABLE AS's input), no HAVING, ORDER BY, LIMIT / OFFSET
// or UNION, every output a column of the aggregate.
struct StatementShape {
  bool own_result = false;  // the relation is the statement's own and ToHost takes it
  bool having = false, order_by = false, limit = false, offset = false, union_all = false;
  bool computed_output = false;  // an output is not a plain column of the aggregate
};
inline bool RelationReachesHostUnchanged(const StatementShape &s) {
  return s.own_result && !s.having && !s.order_by && !s.limit && !s.offset && !s.union_all && !s.computed_output;
}

struct ResultTailFacts {
  bool enabled = true;  // mbx_result_tail
  StatementShape shape;
  bool grouped = false;  // GROUP BY: many rows, their count still on the device
  bool varchar = false;  // a VARCHAR output
  int ncols = 0;         // aggregates = columns of the relation
  int max_cols = 0;      // what one emit descriptor holds
  size_t need = 0;       // ResultBufferLayout of the one row
  size_t mapped_bytes = 0, max_segs = 0;
  bool no_hostcopy = false;  // MBX_NO_HOSTCOPY
};
struct ResultTailChoice {
  bool take;
  const char *reason;  // why not ("" when taken)
};
inline ResultTailChoice ResultTailDecide(const ResultTailFacts &f) {
  if (!f.enabled) return {false, "mbx_result_tail=false"};
  if (!f.shape.own_result) return {false, "not the statement's own result on its way to the host"};
  if (f.shape.having) return {false, "HAVING"};
  if (f.shape.order_by) return {false, "ORDER BY"};
  if (f.shape.limit) return {false, "LIMIT"};
  if (f.shape.offset) return {false, "OFFSET"};
  if (f.shape.union_all) return {false, "UNION"};
  if (f.shape.computed_output) return {false, "an output computed from the aggregates"};
  if (f.grouped) return {false, "GROUP BY"};
  if (f.varchar) return {false, "VARCHAR output"};
  if (f.ncols < 1 || f.ncols > f.max_cols) return {false, "more columns than one emit holds"};
  if (!ResultFitsMapped(f.need, (size_t)f.ncols, f.mapped_bytes, f.max_segs, f.no_hostcopy))
    return {false, "the result does not go through the mapped buffer"};
  return {true, ""};
}

}  // namespace mbx
