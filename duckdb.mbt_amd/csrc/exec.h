// exec.h — what the executor's translation units share (executor.cpp,
// aggregate.cpp, join.cpp, window.cpp, ingest.cpp, sharded.cpp): the engine state, device buffers
// and relations, and the functions that cross between the units.  Internal to
// those six files: the engine and the C-ABI shim see engine.h only.
#pragma once
#include <hip/hip_runtime.h>

#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <string>
#include <utility>
#include <vector>

#include "device.h"
#include "engine.h"
#include "result_tail.h"
#include "tail_wait.h"

namespace mbx {
#define HIPCHK(x)                                                                            \
  do {                                                                                       \
    hipError_t e_ = (x);                                                                     \
    if (e_ != hipSuccess) ThrowError("IO", std::string("HIP error: ") + hipGetErrorString(e_) + " at " #x); \
  } while (0)

// ---------------------------------------------------------------------------
// engine state
// ---------------------------------------------------------------------------
struct ProfEvent {
  std::string name;
  hipEvent_t a, b;
  double bytes;
  int64_t rows;
};

// Caching device allocator for every intermediate buffer of a connection
// (hipMalloc underneath; the stream-ordered hipMallocAsync pool is not used).
// Blocks are bucketed — powers of two up to 1 MiB, then steps of 1/8 of the
// size's power of two (>= 2 MiB) — and recycled on the connection's single
// stream, so reuse is stream-ordered by construction.  Cached bytes above
// kLimit are released after a stream synchronisation.
struct DevicePool {
  static constexpr size_t kLimit = (size_t)64 << 30;
  std::map<size_t, std::vector<void *>> free_;
  size_t cached = 0;
  hipStream_t s = nullptr;
  int device = 0;
  void Free(void *p) { (void)hipFree(p); }
  static size_t Bucket(size_t bytes) {
    if (bytes <= 256) return 256;
    size_t p2 = 256;
    while (p2 < bytes) p2 <<= 1;
    if (p2 <= ((size_t)1 << 20)) return p2;
    size_t step = std::max<size_t>(p2 / 16, (size_t)2 << 20);  // p2/2 < bytes <= p2: steps of p2/16 = (1/8 of floor pow2)
    return (bytes + step - 1) / step * step;
  }
  void ReleaseAll() {
    if (s) (void)hipStreamSynchronize(s);
    for (auto &kv : free_)
      for (void *p : kv.second) Free(p);
    free_.clear();
    cached = 0;
  }
  void *Get(size_t b) {
    auto it = free_.find(b);
    if (it != free_.end() && !it->second.empty()) {
      void *p = it->second.back();
      it->second.pop_back();
      cached -= b;
      return p;
    }
    void *p = nullptr;
    if (hipMalloc(&p, b) != hipSuccess) {
      (void)hipGetLastError();
      ReleaseAll();  // give cached blocks back and retry once
      if (hipMalloc(&p, b) != hipSuccess) {
        (void)hipGetLastError();
        return nullptr;
      }
    }
    return p;
  }
  void Put(size_t b, void *p) {
    if (cached + b > kLimit) {
      if (s) (void)hipStreamSynchronize(s);
      Free(p);
      return;
    }
    free_[b].push_back(p);
    cached += b;
  }
  ~DevicePool() { ReleaseAll(); }
};

struct DevBuf;

struct Engine {
  int device = 0;
  std::shared_ptr<DevicePool> pool;
  bool has_gpu = false;
  hipStream_t stream = nullptr;
  int32_t *d_err = nullptr;
  int64_t *d_scratch = nullptr;  // small device scratch (counts)
  // select_rounds control block (abort word, total, {count, epoch} granules):
  // zeroed when (re)allocated, then reused with a fresh epoch per launch
  unsigned long long *d_rounds = nullptr;
  size_t rounds_bytes = 0;
  uint32_t rounds_epoch = 0;
  void *d_small = nullptr;       // 64 KB scratch for small states
  dev::AggPartial *d_partials = nullptr;  // per-workgroup partials of the fused filter-aggregate
  const void *defer_count_for = nullptr;  // the top-level BoundSelect whose GROUP BY count may stay on the device
  // pinned host staging for small results: every D2H of a query lands here
  // and the query pays ONE stream synchronisation
  // set around the query of CREATE TABLE AS / INSERT ... SELECT: select_rounds
  // then also returns its outputs' zone maps (DCol::zn), so the append needs no
  // statistics pass
  bool want_zone_maps = false;
  uint8_t *h_pinned = nullptr;
  size_t h_pinned_bytes = 0;
  // grows the arena (power of two, up to kPinnedMax) so a query result of
  // that size still lands in pinned memory with one synchronisation
  static constexpr size_t kPinnedMax = (size_t)512 << 20;
  bool EnsurePinned(size_t need) {
    if (need <= h_pinned_bytes) return true;
    if (need > kPinnedMax) return false;
    size_t b = h_pinned_bytes ? h_pinned_bytes : 1 << 20;
    while (b < need) b <<= 1;
    HIPCHK(hipStreamSynchronize(stream));
    if (h_pinned) HIPCHK(hipHostFree(h_pinned));
    h_pinned = nullptr;
    h_pinned_bytes = 0;
    HIPCHK(hipHostMalloc((void **)&h_pinned, b, hipHostMallocDefault));
    h_pinned_bytes = b;
    return true;
  }
  // coherent pinned buffer for small results, written by host_copy_kernel or,
  // for a one-row aggregate, by the emit itself (result_tail.h)
  static constexpr size_t kMappedBytes = (size_t)64 << 10;
  uint8_t *h_mapped = nullptr;
  // mbx_result_tail (set by Eng); the statement count that dates a relation's
  // ResultTailMark (ExecuteSelect advances it, so no mark outlives its
  // statement); results ToHost read straight from the emit's host tail, and
  // results it copied with HostCopy (duckdb_mbx_result_tail_stats)
  bool result_tail = true;
  uint64_t tail_serial = 0;
  int64_t tail_results = 0, hostcopy_results = 0;
  // The result tail's ticket (tail_wait.h): EmitOneRow advances it each time it
  // takes the tail and hands the new value to the emit, which stores it at
  // h_mapped + kTailTicketOffset after the row; ToHost waits for exactly that
  // value, spinning for up to tail_spin_ns (mbx_tail_spin_us, set by Eng; 0:
  // block on the stream at once).  stream_draining: the last statement
  // returned on its ticket, so its kernel's last instructions and the
  // profile's closing event may still be on the stream.
  uint64_t tail_ticket = 0;
  int64_t tail_spin_ns = 0;
  bool stream_draining = false;
  TailWaitStats tail_wait;  // duckdb_mbx_tail_wait_stats
  // H2D ingest ring: host rows are copied into a pinned slot while the DMA of
  // the previous slot runs (bulk appender path)
  static constexpr int kStageSlots = 4;
  static constexpr size_t kStageBytes = (size_t)16 << 20;
  uint8_t *h_stage[kStageSlots] = {nullptr, nullptr, nullptr, nullptr};
  hipEvent_t stage_ev[kStageSlots] = {nullptr, nullptr, nullptr, nullptr};
  // zone-map statistics of appends still in flight (appender's pinned double
  // buffer): the stats reduction's 3 values land in a pinned slot and are
  // folded into the column by SettlePending before the next device statement
  struct PendingStat {
    DevColumn *col;
    long long *h;  // pinned: min, max, non-null count
    int64_t n;
    bool first_rows;
    int64_t rows;  // the table's row count after this append
  };
  std::vector<PendingStat> pending_stats;
  std::vector<long long *> stat_slots;  // free pinned 3-value slots
  // an async append's DMA from a pinned appender buffer is in flight: the next
  // SettlePending waits for it, so the buffer is never refilled under the DMA
  bool inflight_h2d = false;
  // select_rounds outcomes (duckdb_mbx_engine_stats): launches, launches that
  // gave up because a workgroup was never scheduled (the two-pass form reran
  // the query), launches that failed to start
  int64_t sr_launches = 0, sr_aborts = 0, sr_launch_failures = 0;
  // the connection's mbx_scan_codes / mbx_scan_codes_min_rows /
  // mbx_scan_codes_bits_min_rows / mbx_scan_codes_planes_min_rows /
  // mbx_scan_hist / mbx_scan_hist_min_rows (set by Eng)
  bool scan_codes = true, scan_hist = true;
  int64_t scan_hist_min_rows = 0;
  // mbx_scan_hist_host / mbx_scan_hist_host_min_rows (set by Eng), and what
  // became of the statements they cover (duckdb_mbx_scan_hist_host_stats):
  // answered on the host with no launch; fetches of a column's histogram
  // mirror; statements that wanted the host answer and took the device path,
  // with the reason of the last one
  bool scan_hist_host = true;
  int64_t scan_hist_host_min_rows = 0;
  struct ScanHistHostStats {
    int64_t answered = 0, fetches = 0, declined = 0;
    const char *last_reason = "";
  } hist_host;
  int64_t scan_codes_min_rows = 0, scan_codes_bits_min_rows = 0, scan_codes_planes_min_rows = 0;
  // IN (subquery): the sets of the running statement, each subquery run and
  // its table built once however often its leaf is lowered (MarkSetScope)
  struct MarkSet {
    std::shared_ptr<const BoundSelect> sub;
    int64_t rows = 0, nulls = 0;  // of the subquery; of them NULL keys
    std::shared_ptr<struct DevBuf> tab;  // null: no non-NULL key
    int64_t cap = 0;
  };
  std::vector<MarkSet> mark_sets;
  int mark_depth = 0;
  Connection *mark_conn = nullptr;  // the connection the subqueries run on
  bool profile = false;
  std::vector<ProfEvent> events;
  // kernels timed on shard engines during this query (gpu_devices)
  std::mutex shard_mu;
  std::vector<QueryProfile::Kernel> shard_kernels;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;  // reused across queries
  // which pairs of ev_pool are out: with the running statement, or with
  // statements whose profile is not settled yet (pending_prof, oldest first;
  // SettleProfile reads them and gives their pairs back)
  EventPairLedger ev_ledger;
  struct PendingProfile {
    std::vector<ProfEvent> events;
    std::vector<QueryProfile::Kernel> shard_kernels;
  };
  std::vector<PendingProfile> pending_prof;
  // The per-kernel profile's event pairs: timing only (SettleProfile reads them
  // after waiting for the last one), so without the system-scope fence a
  // recorded event otherwise performs (an L2 writeback and invalidate around
  // each timestamp, which also delays the next launch on the stream).  A pair
  // that a pending statement holds is not handed out.
  std::pair<hipEvent_t, hipEvent_t> NextEvents() {
    const size_t i = ev_ledger.Take();
    if (i == ev_pool.size()) {
      hipEvent_t a, b;
      (void)hipEventCreateWithFlags(&a, hipEventDisableSystemFence);
      (void)hipEventCreateWithFlags(&b, hipEventDisableSystemFence);
      ev_pool.push_back({a, b});
    }
    return ev_pool[i];
  }
  // a statement begins (or ends unread): the running statement's events go
  void ResetEvents() {
    events.clear();
    ev_ledger.DropCurrent();
  }
  ~Engine() {
    if (has_gpu) {
      hipSetDevice(device);
      if (stream) hipStreamSynchronize(stream);
      pool->s = nullptr;  // tables may hold pool blocks past this engine (adopted results)
      pool.reset();       // returns cached buffers before the stream goes away
      for (auto &e : ev_pool) {
        hipEventDestroy(e.first);
        hipEventDestroy(e.second);
      }
      if (d_err) hipFree(d_err);
      if (d_scratch) hipFree(d_scratch);
      if (d_rounds) hipFree(d_rounds);
      if (d_small) hipFree(d_small);
      if (d_partials) hipFree(d_partials);
      if (h_pinned) hipHostFree(h_pinned);
      if (h_mapped) hipHostFree(h_mapped);
      for (auto &ps : pending_stats) stat_slots.push_back(ps.h);
      for (auto *h : stat_slots) hipHostFree(h);
      for (int i = 0; i < kStageSlots; i++) {
        if (h_stage[i]) hipHostFree(h_stage[i]);
        if (stage_ev[i]) hipEventDestroy(stage_ev[i]);
      }
      if (stream) hipStreamDestroy(stream);
    }
  }
};

struct ProfScope {
  Engine &e;
  bool on;
  size_t idx;
  ProfScope(Engine &en, const char *name, double bytes, int64_t rows) : e(en), on(en.profile) {
    if (!on) return;
    ProfEvent pe;
    pe.name = name;
    pe.bytes = bytes;
    pe.rows = rows;
    auto ev = e.NextEvents();
    pe.a = ev.first;
    pe.b = ev.second;
    hipEventRecord(pe.a, e.stream);
    e.events.push_back(pe);
    idx = e.events.size() - 1;
  }
  // the event's name, once the scope knows which kernel it launched
  void Rename(const char *name) {
    if (on) e.events[idx].name = name;
  }
  ~ProfScope() {
    if (on) hipEventRecord(e.events[idx].b, e.stream);
  }
};

// Around a statement's run: the membership sets made inside are dropped when
// the outermost scope ends, however it ends.
struct MarkSetScope {
  Engine &e;
  Connection *prev;
  MarkSetScope(Engine &en, Connection &c) : e(en), prev(en.mark_conn) {
    if (e.mark_depth++ == 0) e.mark_sets.clear();
    e.mark_conn = &c;
  }
  ~MarkSetScope() {
    e.mark_conn = prev;
    if (--e.mark_depth == 0) e.mark_sets.clear();
  }
};

// ---------------------------------------------------------------------------
// device buffers and relations
// ---------------------------------------------------------------------------
// Every intermediate device buffer comes from the connection's DevicePool
// and returns to it when its last owner lets go.
struct DevBuf {
  void *p = nullptr;
  size_t bytes = 0;
  std::shared_ptr<DevicePool> pool;
  ~DevBuf() {
    if (p && pool) pool->Put(bytes, p);
  }
};
typedef std::shared_ptr<DevBuf> DevBufPtr;

struct DCol {
  LogicalType type;
  Phys phys = P_I64;
  void *data = nullptr;
  uint64_t *validity = nullptr;
  int64_t *offsets = nullptr;  // strings
  char *chars = nullptr;
  int64_t chars_len = 0;
  std::vector<DevBufPtr> owners;
  // statistics when the column is a table column
  const DevColumn *table_col = nullptr;
  // the table column's buffer owners, when the data is read in place
  std::vector<std::shared_ptr<void>> pins;
  // zone map the producing kernel computed over its zn rows (select_rounds
  // under Engine::want_zone_maps): min / max of the non-NULL values, their count
  int64_t zn = -1, zvalid = 0;
  i128 zmin = 0, zmax = 0;
};

// What the emit of a one-row aggregate already stored in the engine's mapped
// buffer (EmitDesc::host): the relation's column buffers and where their cells
// lie.  ToHost trusts it only for exactly these buffers, whole, in the
// statement that made it.
struct ResultTailMark {
  uint64_t serial = 0;  // Engine::tail_serial when it was made
  uint64_t ticket = 0;  // what the emit stores behind the row (Engine::tail_ticket)
  // the host itself stored the row and a zero error word (a histogram range
  // aggregate answered from the mirror): no kernel ran, there is no ticket to
  // wait for, and the relation's device columns were never written
  bool host_filled = false;
  size_t ncols = 0;
  const void *data[EMIT_MAX_AGGS];
  const void *valid[EMIT_MAX_AGGS];
  ResultColLayout off[EMIT_MAX_AGGS];
};

struct DRel {
  std::shared_ptr<const ResultTailMark> tail;  // column passthroughs keep it; every other operator drops it
  std::vector<DCol> cols;
  int64_t n = 0;
  bool range = false;  // column 0 is the virtual range column
  int64_t rs = 0, rstep = 1;
  // the row count is still on the device (n is its upper bound; the columns
  // hold n rows): only the top-level aggregate of ExecuteSelect leaves it so,
  // for ToHost to read with the rows in one copy; SettleCount otherwise
  const int64_t *n_dev = nullptr;
  std::shared_ptr<void> n_owner;
};

inline int64_t Words64(int64_t n) { return (n + 63) / 64; }

// ---- executor.cpp
Engine &Eng(Connection &c);
void FoldStats(DevColumn &c, int64_t n, int64_t nvalid, i128 mn, i128 mx, bool first_rows);
void SettlePending(Engine &e);
DevBufPtr Alloc(Engine &e, size_t bytes, bool zero = false);
DCol ColFromTable(const DevColumn &c);
void CheckError(Engine &e);
void RaiseDeviceError(Engine &e, int32_t err);
void SettleCount(Engine &e, DRel &r);
void UploadHostColumn(Engine &e, const HostColumn &hc, int64_t n, DCol &d);
DRel UploadRows(Engine &e, const std::vector<std::vector<Value>> &rows, const std::vector<LogicalType> &types);
DCol AllocOut(Engine &e, const LogicalType &t, int64_t n, bool with_valid, bool zero_valid = true);
DRel FilterProject(Engine &e, const DRel &rel, const BExprPtr &pred, const std::vector<BExprPtr> &exprs);
// Evaluates every leaf of `trees` (entries may be null) that the VM cannot
// compute -- a VARCHAR predicate, with the str_match kernels; x IN (subquery),
// with the mark join (join_probe_mark) -- into BOOLEAN columns appended to a
// copy of rel (`lowered`) and rewrites the trees, copy on write, to read those
// columns.  false: no tree has such a leaf; trees and lowered are untouched.
bool LowerStringPredicates(Engine &e, const DRel &rel, std::vector<BExprPtr> &trees, DRel &lowered);
const BExpr *StripWidening(const BExpr *x);
bool RangePredicate(const BExpr &p, int *col, i128 *lo, i128 *hi);
bool RangeConj(const BExpr &p, std::map<int, std::pair<i128, i128>> &ranges);
bool FastIntCol(const DRel &rel, int c);
DRel GatherRel(Engine &e, const DRel &r, const int64_t *perm, int64_t n);
DevBufPtr SortPerm(Engine &e, const DRel &r, const std::vector<BoundOrder> &order);
DRel ConcatRels(Engine &e, std::vector<DRel> &parts);
ResultPtr ToHost(Engine &e, const DRel &r, const std::vector<std::string> &names, int64_t offset, int64_t limit,
                 size_t ncols, bool text = false);
DRel SourceRel(Engine &e, Connection &c, const BoundSource &src);
DRel RunBranch(Engine &e, Connection &c, const BoundSelect &s);
size_t VisibleCols(const BoundSelect &s);
DRel RunSelectDev(Engine &e, Connection &c, const BoundSelect &s, bool top = false);
bool IsHostConstantSelect(const BoundSelect &s);
ResultPtr HostConstantSelect(const BoundSelect &s);
// The statement's profile: total_ms now; its kernels' times at once, or, where
// the statement returned on its ticket with the stream still draining
// (Engine::stream_draining), when SettleProfile next runs.
void FinishProfile(Connection &c, Engine &e, double total_ms);
// Reads the event pairs of every statement FinishProfile left pending into
// last_profile and profile_history, in statement order (waits for the last
// event).  At the start of every statement that resets the engine's events,
// before the profile getters answer, and before the engine goes away.
void SettleProfile(Connection &c, Engine &e);
// a statement begins: SettleProfile, then e.profile from the connection and no events
void BeginProfile(Connection &c, Engine &e);
// ---- aggregate.cpp
DRel Aggregate(Engine &e, const DRel &src, const BoundSelect &s);
// the one-row relation of s's aggregates (no GROUP BY) from states[j] and the COUNT(*) word
DRel EmitGlobalStates(Engine &e, const BoundSelect &s, const unsigned long long *cstar, dev::AggState *states);
// ---- join.cpp
// A join up to and including its table: both inputs run to relations (ranges
// made real), the side choice, the probe side's key column, the build side's
// sorted row numbers and the table of its distinct keys.
struct JoinPrepared {
  DRel in[2];             // the left and the right input
  int b = 1, p = 0;       // which of them builds and which probes
  bool empty = false;     // an input, or the build side without its NULL keys, has no row: no pair
  DCol pkey;              // the probe side's key column
  DevBufPtr rows2, tab;   // build row numbers in sorted-key order; the table (JoinEntry x cap)
  int64_t nb = 0, cap = 0;
  DevBufPtr max_run;      // with want_max_run: a device word, the longest run of equal build keys
};
JoinPrepared JoinPrepare(Engine &e, Connection &c, const BoundSource &src, bool want_max_run = false);
// a key expression over r as a column: a bare column read in place, anything else evaluated
DCol KeyColumn(Engine &e, const DRel &r, const BExprPtr &k);
// The build half, shared by the join and by IN (subquery): the n keys of an
// integer column, NULLs filtered out, as sorted row numbers and the table of
// the distinct keys (join_keys, radix_sort, join_build).  nb == 0 (no non-NULL
// key): no buffers.
struct JoinTable {
  DevBufPtr rows2, tab, max_run;
  int64_t nb = 0, cap = 0;  // non-NULL keys; table slots
  int64_t nulls = 0;        // keys that were NULL
};
JoinTable JoinBuildTable(Engine &e, DCol bkey, int64_t n, bool want_max_run = false);
// the rest: counts, offsets, the limit, the row numbers of the pairs, the gathers, the residual
DRel JoinPairs(Engine &e, Connection &c, const BoundSource &src, const JoinPrepared &j);
DRel JoinRel(Engine &e, Connection &c, const BoundSource &src);  // JoinPairs(JoinPrepare(...))
// s: an aggregate without GROUP BY whose source is a join.  The aggregate
// relation (before HAVING and the outputs): from the fused
// probe-and-aggregate where join_agg_plan.h takes the statement, else from
// JoinPairs on the same prepared join and Aggregate()
DRel JoinAggregate(Engine &e, Connection &c, const BoundSelect &s);
// ---- window.cpp
// s: a select with window calls; src: its source relation.  The relation of s's outputs, in source order.
DRel WindowBranch(Engine &e, const BoundSelect &s, const DRel &src);
// ---- ingest.cpp
void UpdateScanCodes(Engine &e, DevColumn &c, int64_t nrows);
void AppendCast(Engine &e, Table &t, DRel r, const std::vector<int> &col_map);
// ---- sharded.cpp
void KeyBytes(const Value &v, std::string &out);
int CompareValues(const Value &a, const Value &b);
DRel ShardedBranch(Engine &e, Connection &c, const BoundSelect &s);
ResultPtr ShardedAggregateHost(Connection &c, const BoundSelect &s);
int TargetPart(const Connection &c, const Table &t);
void SyncRows(Table &t);
void ShardedInsertSelect(Connection &c, Table &t, const BoundSelect &s, const std::vector<int> &col_map);

template <typename T>
T ReadDev(Engine &e, const void *p) {
  // through the pinned arena: a pageable destination would take HIP's staged copy
  static_assert(sizeof(T) <= 64, "small device words only");
  HIPCHK(hipMemcpyAsync(e.h_pinned, p, sizeof(T), hipMemcpyDeviceToHost, e.stream));
  HIPCHK(hipStreamSynchronize(e.stream));
  T v;
  memcpy(&v, e.h_pinned, sizeof(T));
  return v;
}

}  // namespace mbx
