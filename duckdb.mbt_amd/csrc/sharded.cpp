// sharded.cpp — multi-device plans (gpu_devices): shard workers, partial
// aggregates and their host or RCCL combine, sharded branches and inserts.
#include <algorithm>
#include <atomic>
#include <chrono>
#include <cmath>
#include <condition_variable>
#include <functional>
#include <map>
#include <thread>

#include "exec.h"
#include "knobs.h"
#include "rccl_combine.h"

namespace mbx {
// ---------------------------------------------------------------------------
// sharded tables (gpu_devices): every table is split into contiguous row runs,
// one per shard connection (own device, stream, pool).  A query over a sharded
// table runs its scan -> filter -> (partial) aggregate on every shard at once,
// each on its own host thread, and this connection's engine combines:
//   * aggregates: each shard computes decomposable partials per group
//     (COUNT, SUM as int128/DECIMAL(38)/DOUBLE, MIN, MAX; AVG as SUM + COUNT),
//     copied back in one small D2H each and merged exactly on the host, then
//     HAVING / outputs / ORDER BY / LIMIT run on the combining device;
//   * row results: each shard's rows are copied device to device (xGMI peer
//     DMA between different devices) and concatenated in part order.
// The cross-process form of the same combine (one process per GPU) is the
// RCCL all-reduce / all-gather in distributed.py.
// ---------------------------------------------------------------------------
// One persistent host thread per shard 1..n-1 (shard 0 runs on the calling
// thread).  A dispatch bumps a generation word; a worker that finished its
// last job spins on it for up to kSpinUs (back-to-back queries re-dispatch
// within tens of microseconds) and otherwise sleeps on the condition
// variable.  Each worker keeps its shard's device current (HIP's current
// device and the scratch allocator are per thread).
struct ShardWorkers {
  // MBX_SHARD_SPIN_US (0 = sleep at once): with 8 shards, 7 spinning workers
  // compete with the host merge and the appender's copy threads
  const int kSpinUs = [] {
    const char *e = Knob("MBX_SHARD_SPIN_US");
    return e ? atoi(e) : 300;
  }();
  const int n;
  std::vector<std::thread> th;
  std::mutex mu;
  std::condition_variable cv;
  std::atomic<uint64_t> gen{0};
  std::atomic<int> left{0};
  std::atomic<bool> stop{false};
  const std::function<void(int)> *job = nullptr;
  std::vector<std::exception_ptr> errs;
  explicit ShardWorkers(int nshards) : n(nshards), errs(nshards) {
    for (int i = 1; i < n; i++) th.emplace_back([this, i] { Loop(i); });
  }
  void Loop(int i) {
    uint64_t seen = 0;
    for (;;) {
      const auto t0 = std::chrono::steady_clock::now();
      int k = 0;
      while (gen.load(std::memory_order_acquire) == seen && !stop.load(std::memory_order_acquire)) {
        if ((++k & 63) == 0 &&
            std::chrono::steady_clock::now() - t0 > std::chrono::microseconds(kSpinUs)) {
          std::unique_lock<std::mutex> lk(mu);
          cv.wait(lk, [&] { return gen.load(std::memory_order_acquire) != seen || stop.load(); });
          break;
        }
        __builtin_ia32_pause();
      }
      if (stop.load(std::memory_order_acquire)) return;
      seen = gen.load(std::memory_order_acquire);
      try {
        (*job)(i);
      } catch (...) {
        errs[i] = std::current_exception();
      }
      left.fetch_sub(1, std::memory_order_acq_rel);
    }
  }
  void Run(const std::function<void(int)> &f) {
    for (auto &x : errs) x = nullptr;
    job = &f;
    left.store(n - 1, std::memory_order_release);
    {
      std::lock_guard<std::mutex> g(mu);
      gen.fetch_add(1, std::memory_order_acq_rel);
    }
    cv.notify_all();
    try {
      f(0);
    } catch (...) {
      errs[0] = std::current_exception();
    }
    for (int k = 0; left.load(std::memory_order_acquire) > 0; k++) {
      if (k < 4096) __builtin_ia32_pause();
      else std::this_thread::yield();
    }
    for (auto &x : errs)
      if (x) std::rethrow_exception(x);
  }
  ~ShardWorkers() {
    {
      std::lock_guard<std::mutex> g(mu);
      stop.store(true, std::memory_order_release);
    }
    cv.notify_all();
    for (auto &t : th) t.join();
  }
};

// us since the current dispatch of c started (per-shard timings)
static double SinceDispatch(const Connection &c) {
  return (double)(std::chrono::steady_clock::now().time_since_epoch().count() - c.shard_stats_t0) * 1e-3;
}
// a shard's plan and launches are queued (called on its worker thread)
static void MarkLaunched(Connection &c, int i) {
  if (i < (int)c.shard_stats.last.size()) c.shard_stats.last[i].launch_us = SinceDispatch(c);
}

// Runs f(i) for every shard i at once (shard 0 on the calling thread).  Each
// shard's times land in shard_stats.last; an error raised on a shard comes
// back naming the shard and its device.
static void ForShards(Connection &c, const std::function<void(int)> &f) {
  static_assert(std::is_same<std::chrono::steady_clock::duration, std::chrono::nanoseconds>::value, "ns clock");
  const auto t0 = std::chrono::steady_clock::now();
  c.shard_stats_t0 = t0.time_since_epoch().count();
  if (!c.workers) c.workers = std::make_shared<ShardWorkers>((int)c.shards.size());
  c.shard_stats.dispatches++;
  const int nsh = (int)c.shards.size();
  c.shard_stats.last.assign(nsh, ShardStats::Timing());
  const std::function<void(int)> g = [&](int i) {
    ShardStats::Timing &T = c.shard_stats.last[i];
    T.device = c.shards[i]->opts.device;
    T.wake_us = SinceDispatch(c);
    try {
      f(i);
    } catch (std::exception &ex) {
      throw EngineError(std::string(ex.what()) + " (shard " + std::to_string(i) + " of " + std::to_string(nsh) +
                        ", device " + std::to_string(T.device) + ")");
    }
    if (T.launch_us == 0) T.launch_us = SinceDispatch(c);
    T.done_us = SinceDispatch(c);
  };
  c.workers->Run(g);
  c.shard_stats.last_dispatch_us =
      std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
}

static Engine &ShardEngine(Connection &top, Connection &sc) {
  Engine &se = Eng(sc);
  // (a shard engine takes no result tail, so none of its statements leaves a
  // profile pending: ShardCollect reads its events after a stream wait)
  se.profile = top.opts.profile;
  se.ResetEvents();
  return se;
}

// a shard's work is done: wait for it, raise its device errors (unless the
// shard's result copy already read its error word after a synchronisation),
// and hand its kernel timings to the combining engine's profile
static void ShardCollect(Engine &top, Engine &se, int shard, bool checked = false) {
  if (!checked) {
    HIPCHK(hipStreamSynchronize(se.stream));
    CheckError(se);
  }
  if (!se.profile) return;
  std::vector<QueryProfile::Kernel> ks;
  for (auto &ev : se.events) {
    float ms = 0;
    hipEventElapsedTime(&ms, ev.a, ev.b);
    QueryProfile::Kernel k;
    k.name = ev.name;
    k.ms = ms;
    k.bytes = ev.bytes;
    k.rows = ev.rows;
    k.shard = shard;
    k.device = se.device;
    ks.push_back(k);
  }
  se.ResetEvents();
  std::lock_guard<std::mutex> g(top.shard_mu);
  top.shard_kernels.insert(top.shard_kernels.end(), ks.begin(), ks.end());
}

// r (on src's device, src's stream idle) as buffers of dst's device, copied by
// peer DMA on dst's stream (xGMI between MI355X devices); the caller
// synchronises dst's stream once for all the moves it queued.  Shards on the
// same device share r as is, unless the connection forces the peer path
// (mbx_force_peer, tests).
static DRel MoveRelAsync(Connection &conn, Engine &dst, Engine &src, const DRel &r) {
  if (dst.device == src.device && !conn.opts.force_peer) return r;
  DRel out;
  out.n = r.n;
  const int64_t n = r.n;
  for (auto &c : r.cols) {
    DCol d;
    d.type = c.type;
    d.phys = c.phys;
    auto peer = [&](const void *sp, size_t bytes) -> void * {
      auto b = Alloc(dst, std::max<size_t>(bytes, 16));
      if (bytes) {
        HIPCHK(hipMemcpyPeerAsync(b->p, dst.device, sp, src.device, bytes, dst.stream));
        conn.shard_stats.peer_copies++;
        conn.shard_stats.peer_bytes += (int64_t)bytes;
      }
      d.owners.push_back(b);
      return b->p;
    };
    if (c.phys == P_STR) {
      d.offsets = (int64_t *)peer(c.offsets, (size_t)(n + 1) * 8);
      d.chars = (char *)peer(c.chars, (size_t)c.chars_len);
      d.chars_len = c.chars_len;
    } else if (c.data) {
      d.data = peer(c.data, (size_t)n * PhysSize(c.phys));
    }
    if (c.validity) d.validity = (uint64_t *)peer(c.validity, (size_t)Words64(n) * 8);
    out.cols.push_back(d);
  }
  return out;
}

static DRel MoveRel(Connection &c, Engine &dst, Engine &src, const DRel &r) {
  DRel out = MoveRelAsync(c, dst, src, r);
  HIPCHK(hipStreamSynchronize(dst.stream));
  return out;
}

// every row of a sharded table on e's device, in part order (the fallback for
// shapes the partial aggregation does not decompose): every shard's pending
// work settled, then all parts' peer copies queued and waited for once
static DRel GatherShards(Engine &e, Connection &c, const Table &t) {
  std::vector<DRel> parts(t.parts.size());
  for (size_t i = 0; i < t.parts.size(); i++) {
    Engine &se = Eng(*c.shards[i]);
    HIPCHK(hipStreamSynchronize(se.stream));
  }
  Eng(c);  // back on the combining device
  for (size_t i = 0; i < t.parts.size(); i++) {
    const Table &p = *t.parts[i];
    DRel r;
    r.n = p.nrows;
    for (auto &col : p.cols) r.cols.push_back(ColFromTable(col));
    parts[i] = MoveRelAsync(c, e, *c.shards[i]->engine, r);
  }
  HIPCHK(hipStreamSynchronize(e.stream));
  return ConcatRels(e, parts);
}

static LogicalType SumTypeOf(const LogicalType &at) {
  if (at.id == T_DECIMAL) return LogicalType::Decimal(38, at.scale);
  if (at.id == T_FLOAT || at.id == T_DOUBLE) return LogicalType(T_DOUBLE);
  return LogicalType(T_HUGEINT);
}

// the per-shard partial select of an aggregate branch: the same source,
// WHERE and groups; aggregates decomposed; outputs = the whole aggregate
// relation.  false when an aggregate does not decompose (COUNT(DISTINCT)).
static bool PartialSelect(const BoundSelect &s, BoundSelect &p, std::vector<int> &first) {
  p = s;
  p.having.reset();
  p.order.clear();
  p.limit = -1;
  p.offset = 0;
  p.union_all.clear();
  p.distinct = false;
  p.aggs.clear();
  p.outputs.clear();
  p.names.clear();
  const int ng = (int)s.groups.size();
  for (auto &a : s.aggs) {
    if (a.distinct) return false;
    first.push_back(ng + (int)p.aggs.size());
    if (a.kind == A_AVG) {
      AggSpec sum = a, cnt = a;
      sum.kind = A_SUM;
      sum.type = SumTypeOf(a.arg->type);
      cnt.kind = A_COUNT;
      cnt.type = LogicalType(T_BIGINT);
      p.aggs.push_back(sum);
      p.aggs.push_back(cnt);
    } else {
      p.aggs.push_back(a);
    }
  }
  for (int j = 0; j < ng + (int)p.aggs.size(); j++) {
    auto col = std::make_shared<BExpr>();
    col->kind = BExpr::COL;
    col->col = j;
    col->type = j < ng ? s.groups[j]->type : p.aggs[j - ng].type;
    p.outputs.push_back(col);
    p.names.push_back("__p" + std::to_string(j));
  }
  return true;
}

// int128 -> double exactly as the emit kernel's AVG does (through the magnitude)
static double I128ToDoubleLikeDevice(i128 v) {
  const bool neg = v < 0;
  const u128 m = neg ? (u128)0 - (u128)v : (u128)v;
  const uint64_t hi = (uint64_t)(m >> 64), lo = (uint64_t)m;
  const double d = hi == 0 ? (double)lo : (double)hi * 18446744073709551616.0 + (double)lo;
  return neg ? -d : d;
}

int CompareValues(const Value &a, const Value &b) {  // non-NULL values of one type
  switch (ClassOf(a.type)) {
    case VC_F64: {  // NaN sorts above every number, as DuckDB orders it
      const bool an = std::isnan(a.d), bn = std::isnan(b.d);
      if (an || bn) return an == bn ? 0 : an ? 1 : -1;
      return a.d < b.d ? -1 : a.d > b.d ? 1 : 0;
    }
    case VC_STR: return a.s < b.s ? -1 : a.s > b.s ? 1 : 0;
    default: return a.i < b.i ? -1 : a.i > b.i ? 1 : 0;
  }
}

void KeyBytes(const Value &v, std::string &out) {
  out.push_back(v.is_null ? '\0' : '\1');
  if (v.is_null) return;
  switch (ClassOf(v.type)) {
    case VC_F64: {
      // one group per value, as on one device: -0.0 joins 0.0, every NaN one NaN
      double d = v.d == 0.0 ? 0.0 : v.d;
      if (std::isnan(d)) d = std::numeric_limits<double>::quiet_NaN();
      out.append((const char *)&d, 8);
      break;
    }
    case VC_STR: {
      const uint64_t n = v.s.size();
      out.append((const char *)&n, 8);
      out += v.s;
      break;
    }
    default: out.append((const char *)&v.i, 16); break;
  }
  if (v.type.id == T_INTERVAL) out.append((const char *)&v.iv, sizeof(v.iv));
}

// One group's running merge of the shards' partials, per aggregate.
struct ShardAcc {
  int64_t cnt = 0;
  bool has = false;
  i128 si = 0;
  double sd = 0;
  Value mv;
};

// folds one partial row (get(col) = its column col) into the group's accumulators
static void FoldPartial(const BoundSelect &s, const std::vector<int> &first, std::vector<ShardAcc> &accs,
                        const std::function<Value(int)> &get) {
  for (size_t q = 0; q < s.aggs.size(); q++) {
    const AggSpec &a = s.aggs[q];
    ShardAcc &A = accs[q];
    const Value v = get(first[q]);
    switch (a.kind) {
      case A_COUNT_STAR:
      case A_COUNT: A.cnt += (int64_t)v.i; break;
      case A_SUM:
        if (v.is_null) break;
        A.has = true;
        if (ClassOf(a.type) == VC_F64) A.sd += v.d;
        else A.si += v.i;
        break;
      case A_MIN:
      case A_MAX:
        if (v.is_null) break;
        if (!A.has || (a.kind == A_MIN ? CompareValues(v, A.mv) < 0 : CompareValues(v, A.mv) > 0)) A.mv = v;
        A.has = true;
        break;
      case A_AVG: {
        const Value n = get(first[q] + 1);
        if (v.is_null) break;
        A.has = true;
        A.cnt += (int64_t)n.i;
        if (ClassOf(SumTypeOf(a.arg->type)) == VC_F64) A.sd += v.d;
        else A.si += v.i;
        break;
      }
    }
  }
}

// the merged group's aggregate values (AVG finished as the emit kernel does)
static void FinishAccs(const BoundSelect &s, const std::vector<ShardAcc> &accs, std::vector<Value> &row) {
  for (size_t q = 0; q < s.aggs.size(); q++) {
    const AggSpec &a = s.aggs[q];
    const ShardAcc &A = accs[q];
    Value v = Value::Null(a.type);
    switch (a.kind) {
      case A_COUNT_STAR:
      case A_COUNT: v = Value::Int(T_BIGINT, A.cnt); break;
      case A_SUM:
        if (!A.has) break;
        v.is_null = false;
        if (ClassOf(a.type) == VC_F64) v.d = A.sd;
        else v.i = A.si;
        break;
      case A_MIN:
      case A_MAX:
        if (A.has) v = A.mv;
        break;
      case A_AVG: {
        if (!A.has || A.cnt == 0) break;
        if (ClassOf(SumTypeOf(a.arg->type)) == VC_F64) {
          v = Value::Double(A.sd / (double)A.cnt);
        } else {
          double div = (double)A.cnt;
          const int scale = a.arg->type.id == T_DECIMAL ? a.arg->type.scale : 0;
          for (int k = 0; k < scale; k++) div *= 10.0;
          v = Value::Double(I128ToDoubleLikeDevice(A.si) / div);
        }
        break;
      }
    }
    row.push_back(v);
  }
}

static Value LanesValue(const LogicalType &t, int64_t lo, int64_t hi, bool valid) {
  if (!valid) return Value::Null(t);
  Value v;
  v.type = t;
  v.is_null = false;
  v.i = (i128)(((u128)(uint64_t)hi << 64) | (u128)(uint64_t)lo);
  return v;
}

// mbx_combine=rccl: a sharded global aggregate whose partials are integers
// (COUNT, SUM as HUGEINT / DECIMAL(38,s), integer MIN / MAX; AVG over
// integers) is combined by RCCL on the shard devices: every shard packs its
// one partial row into int64 lanes (combine.h) and takes part in one
// collective on its own stream -- an ncclInt64 reduce to device 0 when every partial
// is a COUNT, else an all-gather finished by the carry-correct combine kernel
// on device 0 -- and device 0's answer (with every rank's error word) comes
// back in one small D2H.  false (the host merge runs instead, the reason in
// shard_stats.rccl_note) for other shapes or without distinct devices.
// How each partial column of p combines across ranks (combine.h kinds) and
// whether every one is a COUNT; false and *why for partials RCCL does not
// combine (floating point, non-integer MIN/MAX, too many columns).
static bool RcclKinds(const BoundSelect &p, rc::CombineDesc &cd, bool &counts_only, std::string *why) {
  const int ncols = (int)p.aggs.size();
  if (ncols < 1 || ncols > rc::kMaxCols) return *why = "partial row wider than the RCCL lane block", false;
  memset(&cd, 0, sizeof(cd));
  counts_only = true;
  for (int k = 0; k < ncols; k++) {
    const AggSpec &a = p.aggs[k];
    const VClass vc = ClassOf(a.type);
    switch (a.kind) {
      case A_COUNT_STAR:
      case A_COUNT: cd.kind[k] = rc::K_SUM; break;
      case A_SUM:
        if (vc != VC_I64 && vc != VC_I128) return *why = "floating-point SUM: host merge", false;
        cd.kind[k] = rc::K_SUM, counts_only = false;
        break;
      case A_MIN:
      case A_MAX:
        if ((vc != VC_I64 && vc != VC_I128) || PhysOf(a.type) == P_STR || PhysOf(a.type) == P_INTERVAL)
          return *why = "non-integer MIN/MAX: host merge", false;
        cd.kind[k] = a.kind == A_MIN ? rc::K_MIN : rc::K_MAX, counts_only = false;
        break;
      default: return *why = "aggregate without an integer partial: host merge", false;
    }
  }
  cd.ncols = ncols;
  return true;
}

static bool DistinctDevices(const std::vector<int> &devs) {
  for (size_t i = 0; i < devs.size(); i++)
    for (size_t j = i + 1; j < devs.size(); j++)
      if (devs[i] == devs[j]) return false;
  return true;
}

// Whether the RCCL combine can run over c's shard layout at all (one rank per
// device: distinct devices, unless the test loopback stands in); false and the
// reason in shard_stats.rccl_note (counted as rccl_unsupported)
static bool RcclLayout(Connection &c) {
  if (c.opts.rccl_loopback || DistinctDevices(c.opts.devices)) return true;
  c.shard_stats.rccl_note = "shard devices are not distinct (RCCL takes one rank per device): host merge";
  return false;
}

// Starts opening the communicators of a sharded connection over distinct
// devices at connect (mbx_combine=rccl): ncclCommInitAll and its check run on
// a helper thread while the tables are built, so the first aggregate waits
// only for what is left (rc::Prepare)
static void RcclPrepare(Connection &c) {
  if (!c.opts.combine_rccl || c.opts.rccl_loopback || !DistinctDevices(c.opts.devices)) return;
  if (!rc::ApiProblem().empty()) return;  // (RcclReady reports it)
  c.rccl_init = rc::Prepare(c.opts.devices);
  c.shard_stats.rccl_prepared_at_connect = true;
}

// the connection's communicators (the open started at connect, or now; the
// loopback when the test mode asks for it); false and the reason in
// shard_stats.rccl_note
static bool RcclReady(Connection &c) {
  ShardStats &st = c.shard_stats;
  if (c.rccl && rc::IsLoopback(*c.rccl) != c.opts.rccl_loopback) c.rccl.reset(), c.rccl_tried = false;
  if (c.rccl && c.rccl->dead) {  // failed on another connection sharing them: host merge from now on
    c.rccl.reset();
    st.rccl_note = "RCCL communicators of these devices failed earlier in this process: host merge";
    return false;
  }
  if (!c.rccl_tried) {
    c.rccl_tried = true;
    std::string note;
    if (c.opts.rccl_loopback) {
      c.rccl = rc::OpenLoopback(c.opts.devices);
    } else {
      note = rc::ApiProblem();
      if (note.empty()) {
        if (!c.rccl_init) c.rccl_init = rc::Prepare(c.opts.devices);
        double waited = 0;
        c.rccl = rc::Wait(c.rccl_init, &note, &waited);
        st.rccl_first_wait_ms = waited;
      }
    }
    if (!c.rccl) st.rccl_note = note;
  }
  if (!c.rccl && st.rccl_note.empty()) st.rccl_note = "RCCL unavailable";
  return c.rccl != nullptr;
}

// what the last combine ran (duckdb_mbx_rccl_info)
static void CountCollective(Connection &c, bool reduce) {
  ShardStats &st = c.shard_stats;
  (reduce ? st.rccl_reduces : st.rccl_allgathers)++;
  st.last_collective = std::string(c.rccl->loopback ? "loopback " : "") +
                       (reduce ? "ncclReduce (int64 sum to device 0)" : "ncclAllGather");
}

// Waits (bounded) for every rank's stream after a collective; false when it
// timed out, after the communicators were aborted (this connection keeps the
// host merge from then on: rccl_tried stays set).
static bool RcclWait(Connection &c, const std::vector<hipStream_t> &streams,
                     std::chrono::steady_clock::time_point t0) {
  if (c.rccl->loopback) return true;
  static const int timeout_ms = [] {
    const char *v = Knob("MBX_RCCL_TIMEOUT_MS");
    return v ? std::max(1, atoi(v)) : 20000;
  }();
  const auto deadline = t0 + std::chrono::milliseconds(timeout_ms);
  for (size_t i = 0; i < streams.size();) {
    const hipError_t q = hipStreamQuery(streams[i]);
    if (q != hipErrorNotReady) {  // done (or an error, raised by the synchronisation after)
      i++;
      continue;
    }
    if (std::chrono::steady_clock::now() > deadline) {
      rc::Abort(*c.rccl, "an RCCL collective did not complete within " + std::to_string(timeout_ms) + " ms");
      for (size_t k = 0; k < streams.size(); k++) {
        Eng(*c.shards[k]);
        (void)hipStreamSynchronize(streams[k]);
      }
      Eng(c);
      c.rccl.reset();
      c.shard_stats.rccl_timeouts++;
      c.shard_stats.rccl_note = "an RCCL collective did not complete within " + std::to_string(timeout_ms) +
                                " ms: communicators aborted, host merge from now on";
      return false;
    }
    __builtin_ia32_pause();
  }
  return true;
}

static bool ShardedAggregateRccl(Connection &c, const BoundSelect &s, const BoundSelect &p,
                                 const std::vector<int> &first, std::vector<std::vector<Value>> &rows,
                                 std::vector<LogicalType> &types) {
  ShardStats &st = c.shard_stats;
  if (!c.opts.combine_rccl) return false;
  auto fallback = [&](const std::string &why) {
    st.rccl_fallbacks++;
    st.rccl_note = why;
    return false;
  };
  auto unsupported = [&](const std::string &why) {  // a shape or layout RCCL never combines
    st.rccl_unsupported++;
    st.rccl_note = why;
    return false;
  };
  if (!s.groups.empty()) return false;  // (GROUP BY: ShardedAggregateRows, GroupRcclCombine)
  const int ncols = (int)p.aggs.size();
  rc::CombineDesc cd;
  bool counts_only = true;
  std::string why;
  if (!RcclLayout(c)) return unsupported(st.rccl_note);
  if (!RcclKinds(p, cd, counts_only, &why)) return unsupported(why);
  if (!RcclReady(c)) return fallback(st.rccl_note);
  const Table &t = *s.src.table;
  const int nsh = (int)t.parts.size();
  if (nsh != (int)c.rccl->devs.size()) return fallback("table parts do not match the shard devices: host merge");
  const int P = rc::LanesPerRank(ncols, counts_only);
  const size_t recv_lanes = counts_only ? (size_t)P : (size_t)nsh * P;
  cd.ncols = ncols;
  cd.nranks = nsh;
  Engine &e = *c.engine;
  std::vector<int64_t> host(recv_lanes + 3 * ncols);
  // Phase 1, on every shard at once: the partial row, its shape checks, the
  // lane buffers and the pack.  Anything that can fail happens here, before
  // any rank enters the collective, so an error cannot leave the other ranks
  // waiting inside it (ForShards re-raises it naming the shard).
  std::vector<DRel> rel(nsh);
  std::vector<DevBufPtr> sendb(nsh), recvb(nsh), scrb(nsh);
  ForShards(c, [&](int i) {
    Connection &sc = *c.shards[i];
    Engine &se = ShardEngine(c, sc);
    BoundSelect pi = p;
    pi.src.table = t.parts[i];
    rel[i] = RunBranch(se, sc, pi);
    const DRel &r = rel[i];
    if (r.n != 1 || (int)r.cols.size() < ncols) ThrowError("Internal", "RCCL combine: partial row shape");
    rc::PackDesc pd;
    memset(&pd, 0, sizeof(pd));
    for (int k = 0; k < ncols; k++) {
      const DCol &d = r.cols[k];
      if (d.phys == P_STR || d.phys == P_F32 || d.phys == P_F64 || d.phys == P_INTERVAL || !d.data)
        ThrowError("Internal", "RCCL combine: partial column type");
      pd.data[k] = d.data;
      pd.valid[k] = d.validity;
      pd.phys[k] = d.phys;
    }
    pd.ncols = ncols;
    pd.counts_only = counts_only;
    pd.err = se.d_err;
    sendb[i] = Alloc(se, (size_t)P * 8);
    recvb[i] = Alloc(se, recv_lanes * 8);
    if (counts_only && c.rccl->loopback && i == 0) scrb[i] = Alloc(se, (size_t)nsh * P * 8);
    // shard 0: the combined lanes (+ its own counts); every other shard: its counts (reduce form)
    if (!se.EnsurePinned(i == 0 ? (host.size() + P) * 8 : (size_t)P * 8))
      ThrowError("IO", "RCCL combine: pinned staging");
    rc::Pack(pd, (int64_t *)sendb[i]->p, se.stream);
    HIPCHK(hipGetLastError());
    MarkLaunched(c, i);
  });
  // Phase 2, on this thread: the one collective over every rank's stream
  const auto tc0 = std::chrono::steady_clock::now();
  std::vector<const int64_t *> sp(nsh);
  std::vector<int64_t *> rp(nsh), xp(nsh);
  std::vector<hipStream_t> streams(nsh);
  for (int i = 0; i < nsh; i++) {
    sp[i] = (const int64_t *)sendb[i]->p;
    rp[i] = (int64_t *)recvb[i]->p;
    xp[i] = scrb[i] ? (int64_t *)scrb[i]->p : nullptr;
    streams[i] = c.shards[i]->engine->stream;
  }
  std::string cerr;
  // connections over the same devices share the communicators: one collective
  // (and its wait) at a time; `comms` keeps them alive if RcclWait drops them
  const std::shared_ptr<rc::Comms> comms = c.rccl;
  std::unique_lock<std::mutex> coll_lock(comms->mu);
  const bool cok = rc::Collective(*comms, counts_only, sp, rp, xp, streams, (size_t)P, &cerr);
  // A collective that does not complete in time (a rank that cannot reach the
  // others, a broken link) must not hang the connection: the communicators
  // are aborted and the host merge answers this statement and the next ones.
  // The wait is bounded also when the group reported an error: some ranks'
  // parts may have been enqueued before it.
  if (!RcclWait(c, streams, tc0)) {
    coll_lock.unlock();
    for (int k = 0; k < nsh; k++) sendb[k].reset(), recvb[k].reset(), scrb[k].reset(), rel[k] = DRel();
    return fallback(st.rccl_note);
  }
  coll_lock.unlock();
  // Phase 3: device 0 finishes (combine kernel, one D2H); every rank's stream
  // is drained before its lane buffers go back to its pool.  The reduce form
  // also reads back each rank's own counts (its partial row), in the D2H that
  // drains it.
  std::vector<int64_t> own(counts_only ? (size_t)nsh * P : 0);
  std::exception_ptr first_err;
  for (int i = 0; i < nsh; i++) {
    Engine &se = Eng(*c.shards[i]);
    try {
      if (cok && i == 0) {
        DevBufPtr out;
        if (!counts_only) {
          out = Alloc(se, (size_t)3 * ncols * 8);
          rc::Combine(cd, (const int64_t *)recvb[0]->p, (int64_t *)out->p, se.stream);
          HIPCHK(hipGetLastError());
        }
        HIPCHK(hipMemcpyAsync(se.h_pinned, recvb[0]->p, recv_lanes * 8, hipMemcpyDeviceToHost, se.stream));
        if (out)
          HIPCHK(hipMemcpyAsync(se.h_pinned + recv_lanes * 8, out->p, (size_t)3 * ncols * 8, hipMemcpyDeviceToHost,
                                se.stream));
        if (counts_only)
          HIPCHK(hipMemcpyAsync(se.h_pinned + host.size() * 8, sendb[0]->p, (size_t)P * 8, hipMemcpyDeviceToHost,
                                se.stream));
        HIPCHK(hipStreamSynchronize(se.stream));  // every rank's part of the collective has landed
        memcpy(host.data(), se.h_pinned, host.size() * 8);
        if (counts_only) memcpy(own.data(), se.h_pinned + host.size() * 8, (size_t)P * 8);
        out.reset();
      } else {
        if (cok && counts_only)
          HIPCHK(hipMemcpyAsync(se.h_pinned, sendb[i]->p, (size_t)P * 8, hipMemcpyDeviceToHost, se.stream));
        HIPCHK(hipStreamSynchronize(se.stream));
        if (cok && counts_only) memcpy(own.data() + (size_t)i * P, se.h_pinned, (size_t)P * 8);
      }
      ShardCollect(e, se, i, true);
    } catch (...) {
      if (!first_err) first_err = std::current_exception();
    }
    sendb[i].reset(), recvb[i].reset(), scrb[i].reset();
    rel[i] = DRel();
  }
  Eng(c);
  const double t_coll = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - tc0).count();
  if (first_err) std::rethrow_exception(first_err);
  if (!cok) {  // the host merge recomputes the partials, for this statement and the next ones
    const std::string why = "RCCL collective failed (" + cerr + "): communicators dropped, host merge from now on";
    rc::MarkDead(*c.rccl, why);
    c.rccl.reset();
    return fallback(why);
  }
  CountCollective(c, counts_only);
  const auto t_merge = std::chrono::steady_clock::now();
  // every rank's device error word, raised as that shard's error; every
  // shard that reported one is cleared, so no stale error reaches its next query
  std::vector<int32_t> errs(nsh, 0);
  if (counts_only) {
    for (int i = 0; i < nsh; i++) errs[i] = (int32_t)own[(size_t)i * P + P - 1];
  } else {
    for (int i = 0; i < nsh; i++) errs[i] = (int32_t)host[(size_t)i * P + P - 1];
  }
  int bad = -1;
  for (int i = 0; i < nsh; i++) {
    if (!errs[i]) continue;
    if (bad < 0) bad = i;
    Engine &se = Eng(*c.shards[i]);
    HIPCHK(hipMemsetAsync(se.d_err, 0, sizeof(int32_t), se.stream));
    HIPCHK(hipStreamSynchronize(se.stream));
  }
  Eng(c);
  if (bad >= 0) {
    st.rccl_errors++;
    try {
      RaiseDeviceError(e, errs[bad]);
    } catch (std::exception &ex) {
      throw EngineError(std::string(ex.what()) + " (shard " + std::to_string(bad) + " of " + std::to_string(nsh) +
                        ", device " + std::to_string(c.shards[bad]->opts.device) + ")");
    }
    ThrowError("Internal", "RCCL combine: a shard reported a device error");
  }
  // the combined partial row, then the aggregates finished as the host merge does
  std::vector<Value> part(ncols);
  for (int k = 0; k < ncols; k++) {
    const LogicalType &pt = p.aggs[k].type;
    if (counts_only) part[k] = Value::Int(T_BIGINT, (i128)host[k]);
    else {
      const int64_t *o = host.data() + recv_lanes + 3 * k;
      part[k] = LanesValue(pt, o[0], o[1], o[2] & 1);
    }
  }
  std::vector<ShardAcc> accs(s.aggs.size());
  FoldPartial(s, first, accs, [&](int col) { return part[col]; });
  types.clear();
  for (auto &a : s.aggs) types.push_back(a.type);
  rows.assign(1, std::vector<Value>());
  FinishAccs(s, accs, rows[0]);
  // each rank's partial row, as the host merge keeps them (the all-gather's
  // blocks, or each rank's own count lanes of the reduce)
  st.last_partials.clear();
  for (int i = 0; i < nsh; i++) {
    auto res = std::make_shared<MaterializedResult>();
    res->nrows = 1;
    for (int k = 0; k < ncols; k++) {
      HostColumn hc;
      hc.name = p.names[k];
      hc.type = p.aggs[k].type;
      hc.phys = PhysOf(hc.type);
      if (counts_only) {
        HostColumnPush(hc, Value::Int(T_BIGINT, (i128)own[(size_t)i * P + k]));
      } else {
        const int64_t *x = host.data() + (size_t)i * P + 3 * k;
        HostColumnPush(hc, LanesValue(hc.type, x[0], x[1], x[2] & 1));
      }
      res->cols.push_back(std::move(hc));
    }
    st.last_partials.push_back(res);
  }
  st.rccl_combines++;
  if (c.rccl->loopback) st.rccl_loopbacks++;
  st.rccl_note.clear();
  st.last_rccl_us = t_coll;
  st.last_combine_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_merge).count();
  return true;
}

// mbx_combine=rccl for a sharded GROUP BY on one integer key (SURVEY.md
// §8(e): the GROUP BY partials travel by the same all-gather).  Each shard's
// partial relation (its groups, already on its device) is packed into dense
// key slots -- slot = key - kmin over the union of the shards' key ranges,
// the NULL key last -- with {lo, hi, valid} lanes per partial column
// (PackRows); one all-gather of the blocks; combine_slots_kernel on device 0
// ORs presence and combines each column as the global combine does; one D2H
// of the combined slots (and of the gathered blocks, for the per-shard
// partials).  Groups come out in key order, NULL last, as the direct-index
// paths emit them.  false (the caller merges the same partials on the host)
// when the key range is wider than kMaxGroupSlots or a collective fails.
static constexpr int64_t kMaxGroupSlots = 4096;
static bool GroupRcclEligible(Connection &c, const BoundSelect &s, const BoundSelect &p, rc::CombineDesc &cd) {
  ShardStats &st = c.shard_stats;
  if (!c.opts.combine_rccl) return false;
  auto fallback = [&](const std::string &why) {
    st.rccl_fallbacks++;
    st.rccl_note = why;
    return false;
  };
  auto unsupported = [&](const std::string &why) {  // a shape or layout RCCL never combines
    st.rccl_unsupported++;
    st.rccl_note = why;
    return false;
  };
  if (s.groups.empty()) return false;  // (a global aggregate: ShardedAggregateRccl)
  if (s.groups.size() != 1) return unsupported("GROUP BY over several keys: host merge");
  const LogicalType &kt = s.groups[0]->type;
  const Phys kp = PhysOf(kt);
  if (!RcclLayout(c)) return unsupported(st.rccl_note);
  if (kp != P_I8 && kp != P_I16 && kp != P_I32 && kp != P_I64 && kp != P_U8 && kp != P_U16 && kp != P_U32)
    return unsupported("GROUP BY key is not an integer column of <= 64 bits: host merge");
  bool counts_only = false;
  std::string why;
  if (!RcclKinds(p, cd, counts_only, &why)) return unsupported(why);
  if (!RcclReady(c)) return fallback(st.rccl_note);
  if ((int)s.src.table->parts.size() != (int)c.rccl->devs.size())
    return fallback("table parts do not match the shard devices: host merge");
  return true;
}

static bool GroupRcclCombine(Connection &c, const BoundSelect &s, const BoundSelect &p, const std::vector<int> &first,
                             rc::CombineDesc cd, std::vector<DRel> &rel, const std::vector<std::array<long long, 3>> &kr,
                             std::vector<std::vector<Value>> &rows, std::vector<LogicalType> &types) {
  ShardStats &st = c.shard_stats;
  auto fallback = [&](const std::string &why) {
    st.rccl_fallbacks++;
    st.rccl_note = why;
    return false;
  };
  const int nsh = (int)rel.size(), ncols = cd.ncols;
  // the union of the shards' key ranges (the NULL key always has its slot)
  bool any = false;
  i128 kmin = 0, kmax = 0;
  for (int i = 0; i < nsh; i++) {
    if (kr[i][2] > 0) {
      if (!any || (i128)kr[i][0] < kmin) kmin = kr[i][0];
      if (!any || (i128)kr[i][1] > kmax) kmax = kr[i][1];
      any = true;
    }
  }
  const i128 range = any ? kmax - kmin + 1 : 0;
  if (range > kMaxGroupSlots) {  // a shape the slots do not cover
    st.rccl_unsupported++;
    st.rccl_note = "GROUP BY key range wider than 4096: host merge";
    return false;
  }
  const int64_t nslot = (int64_t)range + 1;  // + the NULL key's slot
  const int64_t SL = rc::SlotLanes(ncols), P = nslot * SL + 1, recv_lanes = (int64_t)nsh * P;
  const int64_t out_lanes = nslot * SL + nsh;
  cd.nranks = nsh;
  Engine &e = *c.engine;
  std::vector<DevBufPtr> sendb(nsh), recvb(nsh);
  std::vector<const int64_t *> sp(nsh);
  std::vector<int64_t *> rp(nsh), xp(nsh, nullptr);
  std::vector<hipStream_t> streams(nsh);
  // pack every rank's block (the partial relations are on their devices)
  for (int i = 0; i < nsh; i++) {
    Engine &se = Eng(*c.shards[i]);
    const DRel &r = rel[i];
    rc::PackRowsDesc pd;
    memset(&pd, 0, sizeof(pd));
    pd.key = r.cols[0].data;
    pd.key_valid = r.cols[0].validity;
    pd.key_phys = (uint8_t)r.cols[0].phys;
    for (int k = 0; k < ncols; k++) {
      const DCol &d = r.cols[1 + k];
      if (d.phys == P_STR || d.phys == P_F32 || d.phys == P_F64 || d.phys == P_INTERVAL || !d.data)
        ThrowError("Internal", "RCCL combine: partial column type");
      pd.data[k] = d.data;
      pd.valid[k] = d.validity;
      pd.phys[k] = (uint8_t)d.phys;
    }
    pd.ncols = ncols;
    pd.nrows = r.n;
    pd.kmin = (int64_t)kmin;
    pd.nslot = nslot;
    pd.err = se.d_err;
    sendb[i] = Alloc(se, (size_t)P * 8);
    recvb[i] = Alloc(se, (size_t)recv_lanes * 8);
    rc::PackRows(pd, (int64_t *)sendb[i]->p, se.stream);
    HIPCHK(hipGetLastError());
    sp[i] = (const int64_t *)sendb[i]->p;
    rp[i] = (int64_t *)recvb[i]->p;
    streams[i] = se.stream;
  }
  const auto tc0 = std::chrono::steady_clock::now();
  std::string cerr;
  const std::shared_ptr<rc::Comms> comms = c.rccl;  // (shared: one collective at a time, as above)
  std::unique_lock<std::mutex> coll_lock(comms->mu);
  const bool cok = rc::Collective(*comms, false, sp, rp, xp, streams, (size_t)P, &cerr);
  if (!RcclWait(c, streams, tc0)) return fallback(st.rccl_note);  // (bounded also after a reported error)
  coll_lock.unlock();
  // device 0 combines; one D2H of the combined slots and of the gathered blocks
  const bool keep_parts = recv_lanes * 8 <= ((int64_t)4 << 20);  // the per-shard partials, when small
  std::vector<int64_t> host((size_t)out_lanes + (keep_parts ? (size_t)recv_lanes : 0));
  std::exception_ptr first_err;
  for (int i = 0; i < nsh; i++) {
    Engine &se = Eng(*c.shards[i]);
    try {
      if (cok && i == 0) {
        DevBufPtr out = Alloc(se, (size_t)out_lanes * 8);
        rc::CombineSlots(cd, nslot, (const int64_t *)recvb[0]->p, (int64_t *)out->p, se.stream);
        HIPCHK(hipGetLastError());
        if (!se.EnsurePinned(host.size() * 8)) ThrowError("IO", "RCCL combine: pinned staging");
        HIPCHK(hipMemcpyAsync(se.h_pinned, out->p, (size_t)out_lanes * 8, hipMemcpyDeviceToHost, se.stream));
        if (keep_parts)
          HIPCHK(hipMemcpyAsync(se.h_pinned + out_lanes * 8, recvb[0]->p, (size_t)recv_lanes * 8,
                                hipMemcpyDeviceToHost, se.stream));
        HIPCHK(hipStreamSynchronize(se.stream));
        memcpy(host.data(), se.h_pinned, host.size() * 8);
      } else {
        HIPCHK(hipStreamSynchronize(se.stream));
      }
      ShardCollect(e, se, i, true);
    } catch (...) {
      if (!first_err) first_err = std::current_exception();
    }
    sendb[i].reset(), recvb[i].reset();
  }
  Eng(c);
  const double t_coll = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - tc0).count();
  if (first_err) std::rethrow_exception(first_err);
  if (!cok) {
    const std::string why = "RCCL all-gather failed (" + cerr + "): communicators dropped, host merge from now on";
    rc::MarkDead(*c.rccl, why);
    c.rccl.reset();
    return fallback(why);
  }
  CountCollective(c, false);
  const auto t_merge = std::chrono::steady_clock::now();
  // every rank's device error word: the first raised naming its shard, all cleared
  int bad = -1;
  std::vector<int32_t> errs(nsh);
  for (int i = 0; i < nsh; i++) {
    errs[i] = (int32_t)host[(size_t)nslot * SL + i];
    if (!errs[i]) continue;
    if (bad < 0) bad = i;
    Engine &se = Eng(*c.shards[i]);
    HIPCHK(hipMemsetAsync(se.d_err, 0, sizeof(int32_t), se.stream));
    HIPCHK(hipStreamSynchronize(se.stream));
  }
  Eng(c);
  if (bad >= 0) {
    st.rccl_errors++;
    try {
      RaiseDeviceError(e, errs[bad]);
    } catch (std::exception &ex) {
      throw EngineError(std::string(ex.what()) + " (shard " + std::to_string(bad) + " of " + std::to_string(nsh) +
                        ", device " + std::to_string(c.shards[bad]->opts.device) + ")");
    }
    ThrowError("Internal", "RCCL combine: a shard reported a device error");
  }
  // the merged groups in key order (the NULL key last), aggregates finished as the host merge does
  const LogicalType &kt = s.groups[0]->type;
  auto key_value = [&](int64_t sl) {
    if (sl == nslot - 1) return Value::Null(kt);
    const i128 k = kmin + sl;
    return LanesValue(kt, (int64_t)k, (int64_t)(k >> 64), true);
  };
  types.clear();
  types.push_back(kt);
  for (auto &a : s.aggs) types.push_back(a.type);
  rows.clear();
  std::vector<Value> part(1 + ncols);
  for (int64_t sl = 0; sl < nslot; sl++) {
    const int64_t *o = host.data() + sl * SL;
    if (!o[0]) continue;
    part[0] = key_value(sl);
    for (int k = 0; k < ncols; k++) part[1 + k] = LanesValue(p.aggs[k].type, o[1 + 3 * k], o[2 + 3 * k], o[3 + 3 * k] & 1);
    std::vector<ShardAcc> accs(s.aggs.size());
    FoldPartial(s, first, accs, [&](int col) { return part[col]; });
    std::vector<Value> row;
    row.push_back(part[0]);
    FinishAccs(s, accs, row);
    rows.push_back(std::move(row));
  }
  // each rank's partial groups as they were gathered
  st.last_partials.clear();
  if (keep_parts) {
    for (int i = 0; i < nsh; i++) {
      const int64_t *g = host.data() + out_lanes + (size_t)i * P;
      auto res = std::make_shared<MaterializedResult>();
      HostColumn kc;
      kc.name = p.names[0];
      kc.type = kt;
      kc.phys = PhysOf(kt);
      std::vector<HostColumn> vc(ncols);
      for (int k = 0; k < ncols; k++) {
        vc[k].name = p.names[1 + k];
        vc[k].type = p.aggs[k].type;
        vc[k].phys = PhysOf(vc[k].type);
      }
      for (int64_t sl = 0; sl < nslot; sl++) {
        const int64_t *o = g + sl * SL;
        if (!o[0]) continue;
        HostColumnPush(kc, key_value(sl));
        for (int k = 0; k < ncols; k++)
          HostColumnPush(vc[k], LanesValue(vc[k].type, o[1 + 3 * k], o[2 + 3 * k], o[3 + 3 * k] & 1));
        res->nrows++;
      }
      res->cols.push_back(std::move(kc));
      for (auto &h : vc) res->cols.push_back(std::move(h));
      st.last_partials.push_back(res);
    }
  }
  st.rccl_combines++;
  st.rccl_group_combines++;
  if (c.rccl->loopback) st.rccl_loopbacks++;
  st.rccl_note.clear();
  st.last_rccl_us = t_coll;
  st.last_combine_us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_merge).count();
  return true;
}

// The host merge when every group key is an integer-like column (the C3
// shape): the partial rows are keyed by their raw int128 keys (NULL last, as
// the direct-index paths order them), sorted once, and each run of equal keys
// folded -- no per-row key strings, hash map or Value keys (8 shards x 32
// groups: see profiles/r04_shard_overhead*.json).  false for other key types
// (VARCHAR, floating point, INTERVAL) or more than two keys.
static bool MergeIntKeys(const BoundSelect &s, const std::vector<int> &first, const std::vector<ResultPtr> &partial,
                         int ng, std::vector<std::vector<Value>> &rows, std::vector<LogicalType> &types) {
  if (ng < 1 || ng > 2) return false;
  for (const auto &m : partial)
    for (int g = 0; g < ng; g++) {
      const Phys p = m->cols[g].phys;
      if (p == P_STR || p == P_F32 || p == P_F64 || p == P_INTERVAL) return false;
    }
  struct Ent {
    i128 k[2];
    uint8_t nul[2];
    int32_t shard;
    int64_t row;
  };
  std::vector<Ent> ents;
  size_t total = 0;
  for (const auto &m : partial) total += (size_t)m->nrows;
  ents.reserve(total);
  for (int i = 0; i < (int)partial.size(); i++) {
    const MaterializedResult &m = *partial[i];
    for (int64_t row = 0; row < m.nrows; row++) {
      Ent e;
      e.k[1] = 0;
      e.nul[1] = 0;
      for (int g = 0; g < ng; g++) {
        const HostColumn &hc = m.cols[g];
        e.nul[g] = hc.IsNull(row);
        e.k[g] = e.nul[g] ? 0 : hc.Get(row).i;
      }
      e.shard = i;
      e.row = row;
      ents.push_back(e);
    }
  }
  auto less = [&](const Ent &a, const Ent &b) {
    for (int g = 0; g < ng; g++) {
      if (a.nul[g] != b.nul[g]) return b.nul[g] != 0;  // NULL keys last
      if (!a.nul[g] && a.k[g] != b.k[g]) return a.k[g] < b.k[g];
    }
    return false;
  };
  std::stable_sort(ents.begin(), ents.end(), less);
  types.clear();
  for (auto &g : s.groups) types.push_back(g->type);
  for (auto &a : s.aggs) types.push_back(a.type);
  rows.clear();
  std::vector<ShardAcc> accs(s.aggs.size());
  for (size_t i = 0; i < ents.size();) {
    size_t j = i;
    for (auto &a : accs) a = ShardAcc();
    while (j < ents.size() && !less(ents[i], ents[j])) {
      const MaterializedResult &m = *partial[ents[j].shard];
      const int64_t row = ents[j].row;
      FoldPartial(s, first, accs, [&](int col) { return m.cols[col].Get(row); });
      j++;
    }
    std::vector<Value> out;
    out.reserve(ng + s.aggs.size());
    const MaterializedResult &m0 = *partial[ents[i].shard];
    for (int g = 0; g < ng; g++) out.push_back(m0.cols[g].Get(ents[i].row));
    FinishAccs(s, accs, out);
    rows.push_back(std::move(out));
    i = j;
  }
  return true;
}

// The aggregate relation of a sharded aggregate branch (groups in key order,
// then one column per aggregate) as host rows: every shard computes its
// decomposable partials (one small D2H each, on its own worker thread), and
// the host merges them by key exactly (int128 sums) -- or, with
// mbx_combine=rccl, RCCL combines a global aggregate on the devices.
static void ShardedAggregateRows(Connection &c, const BoundSelect &s, const BoundSelect &p,
                                 const std::vector<int> &first, std::vector<std::vector<Value>> &rows,
                                 std::vector<LogicalType> &types) {
  if (ShardedAggregateRccl(c, s, p, first, rows, types)) return;
  const Table &t = *s.src.table;
  const int nsh = (int)t.parts.size(), ng = (int)s.groups.size();
  std::vector<ResultPtr> partial(nsh);
  Engine &e = *c.engine;
  // mbx_combine=rccl over a GROUP BY on one integer key: the partials stay on
  // their devices for GroupRcclCombine (each shard reads back only its key range)
  rc::CombineDesc gcd;
  const bool grp_rccl = GroupRcclEligible(c, s, p, gcd);
  std::vector<DRel> rel(grp_rccl ? nsh : 0);
  std::vector<std::array<long long, 3>> kr(nsh, std::array<long long, 3>{0, 0, 0});
  ForShards(c, [&](int i) {
    Connection &sc = *c.shards[i];
    Engine &se = ShardEngine(c, sc);
    BoundSelect pi = p;
    pi.src.table = t.parts[i];
    DRel r = RunBranch(se, sc, pi);
    MarkLaunched(c, i);
    if (grp_rccl) {
      if (r.n > 0) {
        long long *o3 = (long long *)((char *)se.d_small + 3072);
        dev::KeyRange(r.cols[0].data, r.cols[0].phys, r.cols[0].validity, r.n, o3, se.stream);
        HIPCHK(hipMemcpyAsync(se.h_pinned, o3, 24, hipMemcpyDeviceToHost, se.stream));
        HIPCHK(hipStreamSynchronize(se.stream));
        memcpy(kr[i].data(), se.h_pinned, 24);
      }
      rel[i] = std::move(r);
      return;
    }
    partial[i] = ToHost(se, r, pi.names, 0, -1, pi.names.size());  // synchronises and raises device errors
    ShardCollect(e, se, i, true);
  });
  Eng(c);
  if (grp_rccl) {
    if (GroupRcclCombine(c, s, p, first, gcd, rel, kr, rows, types)) return;
    // the host merge of the same partials
    ForShards(c, [&](int i) {
      Engine &se = Eng(*c.shards[i]);
      partial[i] = ToHost(se, rel[i], p.names, 0, -1, p.names.size());
      ShardCollect(e, se, i, true);
    });
    Eng(c);
  }
  c.shard_stats.last_partials = partial;
  const auto t_merge = std::chrono::steady_clock::now();
  if (MergeIntKeys(s, first, partial, ng, rows, types)) {
    c.shard_stats.last_combine_us =
        std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_merge).count();
    return;
  }
  // merge by group key, exactly (int128 sums)
  size_t total_rows = 0;
  for (int i = 0; i < nsh; i++) total_rows += (size_t)partial[i]->nrows;
  std::unordered_map<std::string, size_t> index;
  index.reserve(total_rows * 2 + 1);
  std::vector<std::vector<Value>> keys;
  std::vector<std::vector<ShardAcc>> accs;
  keys.reserve(total_rows);
  accs.reserve(total_rows);
  std::string kb;
  std::vector<Value> kv(ng);
  for (int i = 0; i < nsh; i++) {
    const MaterializedResult &m = *partial[i];
    for (int64_t row = 0; row < m.nrows; row++) {
      kb.clear();
      for (int g = 0; g < ng; g++) {
        kv[g] = m.cols[g].Get(row);
        KeyBytes(kv[g], kb);
      }
      auto it = index.find(kb);
      size_t gi;
      if (it == index.end()) {
        gi = keys.size();
        index.emplace(kb, gi);
        keys.push_back(kv);
        accs.emplace_back(s.aggs.size());
      } else {
        gi = it->second;
      }
      FoldPartial(s, first, accs[gi], [&](int col) { return m.cols[col].Get(row); });
    }
  }
  // groups in key order (NULL keys last), as the direct-index paths emit them
  std::vector<size_t> order(keys.size());
  for (size_t i = 0; i < order.size(); i++) order[i] = i;
  std::sort(order.begin(), order.end(), [&](size_t x, size_t y) {
    for (int g = 0; g < ng; g++) {
      const Value &a = keys[x][g], &b = keys[y][g];
      if (a.is_null != b.is_null) return b.is_null;
      if (a.is_null) continue;
      const int r = CompareValues(a, b);
      if (r) return r < 0;
    }
    return false;
  });
  types.clear();
  for (auto &g : s.groups) types.push_back(g->type);
  for (auto &a : s.aggs) types.push_back(a.type);
  rows.clear();
  for (size_t oi : order) {
    std::vector<Value> row = keys[oi];
    FinishAccs(s, accs[oi], row);
    rows.push_back(std::move(row));
  }
  if (ng == 0 && rows.empty()) {  // a global aggregate always has one row
    std::vector<Value> row;
    for (auto &a : s.aggs)
      row.push_back(a.kind == A_COUNT_STAR || a.kind == A_COUNT ? Value::Int(T_BIGINT, 0) : Value::Null(a.type));
    rows.push_back(row);
  }
  c.shard_stats.last_combine_us =
      std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t_merge).count();
}

static DRel ShardedAggregate(Engine &e, Connection &c, const BoundSelect &s, const BoundSelect &p,
                             const std::vector<int> &first) {
  std::vector<std::vector<Value>> rows;
  std::vector<LogicalType> types;
  ShardedAggregateRows(c, s, p, first, rows, types);
  return UploadRows(e, rows, types);
}

// A top-level SELECT over a sharded table whose result is exactly its merged
// aggregate relation, columns picked in any order (no HAVING, ORDER BY,
// LIMIT, UNION or expressions over the aggregates): the merged rows become
// the host result directly, without a round trip through the combining
// device.  nullptr when the statement does not have that shape.
ResultPtr ShardedAggregateHost(Connection &c, const BoundSelect &s) {
  if (!(s.src.kind == BoundSource::TABLE && s.src.table && s.src.table->sharded() && s.is_agg)) return nullptr;
  if (s.having || !s.order.empty() || s.limit >= 0 || s.offset > 0 || !s.union_all.empty() || s.distinct)
    return nullptr;
  if ((int)s.src.table->parts.size() != (int)c.shards.size()) return nullptr;
  const size_t nvis = VisibleCols(s);
  const size_t nagg = s.groups.size() + s.aggs.size();
  for (size_t k = 0; k < nvis; k++) {
    const BExpr &o = *s.outputs[k];
    if (o.kind != BExpr::COL || o.col < 0 || (size_t)o.col >= nagg) return nullptr;
    const LogicalType &src = o.col < (int)s.groups.size() ? s.groups[o.col]->type : s.aggs[o.col - s.groups.size()].type;
    if (!(src == o.type)) return nullptr;
  }
  BoundSelect p;
  std::vector<int> first;
  if (!PartialSelect(s, p, first)) return nullptr;
  std::vector<std::vector<Value>> rows;
  std::vector<LogicalType> types;
  ShardedAggregateRows(c, s, p, first, rows, types);
  auto res = std::make_shared<MaterializedResult>();
  res->nrows = (int64_t)rows.size();
  for (size_t k = 0; k < nvis; k++) {
    const int j = s.outputs[k]->col;
    HostColumn hc;
    hc.name = s.names[k];
    hc.type = types[j];
    hc.phys = PhysOf(hc.type);
    if (hc.phys == P_STR) hc.offsets.push_back(0);
    for (auto &row : rows) HostColumnPush(hc, row[j]);
    res->cols.push_back(std::move(hc));
  }
  c.shard_stats.host_results++;
  return res;
}

DRel ShardedBranch(Engine &e, Connection &c, const BoundSelect &s) {
  const Table &t = *s.src.table;
  if ((int)t.parts.size() != (int)c.shards.size())
    ThrowError("Internal", "sharded table \"" + t.name + "\" does not match the connection's shards");
  if (s.is_agg) {
    BoundSelect p;
    std::vector<int> first;
    if (PartialSelect(s, p, first)) {
      DRel agg = ShardedAggregate(e, c, s, p, first);
      return FilterProject(e, agg, s.having, s.outputs);
    }
    DRel src = GatherShards(e, c, t);
    DRel agg = Aggregate(e, src, s);
    return FilterProject(e, agg, s.having, s.outputs);
  }
  // row results: filter/project on every shard, concatenated in part order
  const int nsh = (int)t.parts.size();
  std::vector<DRel> parts(nsh);
  ForShards(c, [&](int i) {
    Connection &sc = *c.shards[i];
    Engine &se = ShardEngine(c, sc);
    BoundSelect si = s;
    si.src.table = t.parts[i];
    si.union_all.clear();
    si.order.clear();
    si.limit = -1;
    si.offset = 0;
    parts[i] = RunBranch(se, sc, si);
    MarkLaunched(c, i);
    ShardCollect(e, se, i);
  });
  Eng(c);
  for (int i = 0; i < nsh; i++) parts[i] = MoveRelAsync(c, e, *c.shards[i]->engine, parts[i]);
  HIPCHK(hipStreamSynchronize(e.stream));
  return ConcatRels(e, parts);
}

// the part that takes appended rows: the last non-empty part while it has room
// (mbx_shard_rows; 0 = unbounded), else the next one -- row order stays part order
int TargetPart(const Connection &c, const Table &t) {
  const int n = (int)t.parts.size();
  int last = 0;
  for (int i = 0; i < n; i++)
    if (t.parts[i]->nrows > 0) last = i;
  if (c.opts.shard_rows > 0 && t.parts[last]->nrows >= c.opts.shard_rows && last + 1 < n) return last + 1;
  return last;
}

void SyncRows(Table &t) {
  int64_t n = 0;
  for (auto &p : t.parts) n += p->nrows;
  t.nrows = n;
}

void ShardedInsertSelect(Connection &c, Table &t, const BoundSelect &s, const std::vector<int> &col_map) {
  const int nsh = (int)t.parts.size();
  bool empty = true;
  for (auto &p : t.parts) empty = empty && p->nrows == 0;
  const bool plain = !s.is_agg && s.union_all.empty() && s.order.empty() && s.limit < 0 && s.offset == 0 &&
                     !s.distinct;
  if (empty && plain && s.src.kind == BoundSource::RANGE) {
    // generated rows: contiguous sub-ranges, one per part, built on every shard at once
    const int64_t n = s.src.RangeCount();
    ForShards(c, [&](int i) {
      const int64_t lo = (int64_t)((__int128)n * i / nsh), hi = (int64_t)((__int128)n * (i + 1) / nsh);
      BoundSelect si = s;
      si.src.range_start = s.src.range_start + lo * s.src.range_step;
      si.src.range_stop = s.src.range_start + hi * s.src.range_step;
      si.src.range_inclusive = false;
      ExecuteInsertSelect(*c.shards[i], *t.parts[i], si, col_map);
    });
    SyncRows(t);
    return;
  }
  if (empty && plain && s.src.kind == BoundSource::TABLE && s.src.table && s.src.table->sharded() &&
      (int)s.src.table->parts.size() == nsh) {
    // a sharded source: every part from the same shard's part of the source
    ForShards(c, [&](int i) {
      BoundSelect si = s;
      si.src.table = s.src.table->parts[i];
      ExecuteInsertSelect(*c.shards[i], *t.parts[i], si, col_map);
    });
    SyncRows(t);
    return;
  }
  // anything else: evaluated on the combining device, appended to the target part
  Engine &e = Eng(c);
  e.profile = false;
  DRel r;
  if (IsHostConstantSelect(s)) {
    ResultPtr hr = HostConstantSelect(s);
    r.n = hr->nrows;
    for (auto &hc : hr->cols) {
      DCol d;
      UploadHostColumn(e, hc, hr->nrows, d);
      r.cols.push_back(d);
    }
  } else {
    r = RunSelectDev(e, c, s);
  }
  HIPCHK(hipStreamSynchronize(e.stream));
  CheckError(e);
  const int k = TargetPart(c, t);
  Engine &se = Eng(*c.shards[k]);
  se.profile = false;
  AppendCast(se, *t.parts[k], MoveRel(c, se, e, r), col_map);
  HIPCHK(hipStreamSynchronize(se.stream));
  SyncRows(t);
}

void OpenShards(Connection &c) {
  if (c.opts.devices.size() < 2) return;
  for (int d : c.opts.devices) {
    auto sc = std::make_unique<Connection>();
    sc->opts = c.opts;
    sc->opts.devices.clear();
    sc->opts.device = d;
    sc->engine = CreateEngine(d, false);
    sc->catalog.device = d;
    c.shards.push_back(std::move(sc));
  }
  // peer access between every pair of distinct devices (xGMI on an MI355X
  // node), so row results move by peer DMA without host staging
  std::vector<int> devs = c.opts.devices;
  std::sort(devs.begin(), devs.end());
  devs.erase(std::unique(devs.begin(), devs.end()), devs.end());
  for (int a : devs)
    for (int b : devs) {
      if (a == b) continue;
      int can = 0;
      hipSetDevice(a);
      if (hipDeviceCanAccessPeer(&can, a, b) == hipSuccess && can) {
        const hipError_t r = hipDeviceEnablePeerAccess(b, 0);
        if (r == hipSuccess || r == hipErrorPeerAccessAlreadyEnabled) c.shard_stats.peer_links++;
      }
    }
  (void)hipGetLastError();  // "already enabled" is not an error here
  hipSetDevice(c.engine->device);
  c.workers = std::make_shared<ShardWorkers>((int)c.shards.size());
  RcclPrepare(c);
}

static std::string JsonStr(const std::string &v) {
  std::string o = "\"";
  for (unsigned char ch : v) {
    if (ch == '"' || ch == '\\') o += '\\', o += (char)ch;
    else if (ch < 0x20) {
      char b[8];
      snprintf(b, sizeof(b), "\\u%04x", ch);
      o += b;
    } else o += (char)ch;
  }
  return o + "\"";
}

static std::string JsonRanks(const std::vector<int> &devs, const std::vector<int> &count,
                             const std::vector<int> &user_rank, const std::vector<int> &cu_device) {
  std::string j = "[";
  for (size_t i = 0; i < devs.size(); i++) {
    auto at = [&](const std::vector<int> &v) { return i < v.size() ? v[i] : -1; };
    j += std::string(i ? "," : "") + "{\"device\":" + std::to_string(devs[i]) +
         ",\"count\":" + std::to_string(at(count)) + ",\"user_rank\":" + std::to_string(at(user_rank)) +
         ",\"cu_device\":" + std::to_string(at(cu_device)) + "}";
  }
  return j + "]";
}

std::string RcclInfoJson(Connection &c) {
  const ShardStats &st = c.shard_stats;
  const char *state = "none";
  if (c.rccl && c.rccl->loopback) state = "loopback";
  else if (c.rccl) state = c.rccl->dead ? "failed" : "ready";
  else if (c.rccl_init) state = rc::InitState(*c.rccl_init);
  else if (c.rccl_tried) state = "failed";
  std::string j = "{";
  j += "\"mode\":" + JsonStr(!c.opts.combine_rccl ? "host" : c.opts.rccl_loopback ? "rccl_loopback" : "rccl");
  j += ",\"state\":" + JsonStr(state);
  j += ",\"devices\":[";
  for (size_t i = 0; i < c.opts.devices.size(); i++) j += (i ? "," : "") + std::to_string(c.opts.devices[i]);
  j += "],\"prepared_at_connect\":" + std::string(st.rccl_prepared_at_connect ? "true" : "false");
  char b[256];
  snprintf(b, sizeof(b), ",\"first_wait_ms\":%.3f", st.rccl_first_wait_ms);
  j += b;
  if (c.rccl && !c.rccl->loopback) {
    snprintf(b, sizeof(b), ",\"init_s\":%.6f,\"check_us\":%.1f", c.rccl->init_s, c.rccl->check_us);
    j += b;
    j += ",\"ranks\":" + JsonRanks(c.rccl->devs, c.rccl->count, c.rccl->user_rank, c.rccl->cu_device);
  }
  j += ",\"combines\":" + std::to_string(st.rccl_combines) + ",\"fallbacks\":" + std::to_string(st.rccl_fallbacks) +
       ",\"unsupported\":" + std::to_string(st.rccl_unsupported) + ",\"loopbacks\":" +
       std::to_string(st.rccl_loopbacks) + ",\"group_combines\":" + std::to_string(st.rccl_group_combines) +
       ",\"timeouts\":" + std::to_string(st.rccl_timeouts) + ",\"errors\":" + std::to_string(st.rccl_errors) +
       ",\"reduces\":" + std::to_string(st.rccl_reduces) + ",\"allgathers\":" + std::to_string(st.rccl_allgathers);
  j += ",\"last_collective\":" + JsonStr(st.last_collective) + ",\"note\":" + JsonStr(st.rccl_note) + "}";
  return j;
}

std::string RcclSelfTestJson(const std::vector<int> &devs, std::string *err, double *us) {
  rc::SelfTestInfo info;
  const auto t0 = std::chrono::steady_clock::now();
  *err = rc::SelfTest(devs, &info);
  *us = std::chrono::duration<double, std::micro>(std::chrono::steady_clock::now() - t0).count();
  std::string j = "{\"ok\":" + std::string(err->empty() ? "true" : "false") + ",\"error\":" + JsonStr(*err) +
                  ",\"devices\":[";
  for (size_t i = 0; i < devs.size(); i++) j += (i ? "," : "") + std::to_string(devs[i]);
  char b[160];
  snprintf(b, sizeof(b), "],\"init_us\":%.1f,\"check_us\":%.1f,\"total_us\":%.1f", info.init_us, info.check_us, *us);
  j += b;
  j += ",\"ranks\":" + (err->empty() ? JsonRanks(devs, info.count, info.user_rank, info.cu_device) : "[]") + "}";
  return j;
}
}  // namespace mbx
