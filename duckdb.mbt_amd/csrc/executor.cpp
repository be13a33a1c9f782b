// executor.cpp — runs bound plans on the MI355X.
//
// Replaces the work libduckdb does inside duckdb_query for the recognised
// shapes (reference call sites /root/reference/src/duckdb_native.c:159, :2246,
// :1003, :381): scan -> filter -> project -> aggregate -> sort over
// device-resident column chunks.  Every pass over table rows is a kernel in
// kernels.hip; the host only plans, allocates and copies the (small) final
// result back.  There is no CPU execution path: without a device, any plan
// that touches rows raises.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <type_traits>
#include <cmath>
#include <condition_variable>
#include <cstring>
#include <functional>
#include <limits>
#include <map>
#include <unordered_map>
#include <mutex>
#include <sstream>
#include <thread>

#include "device.h"
#include "jit.h"
#include "engine.h"
#include "hostlink.h"
#include "vm.h"
#include "knobs.h"
#include "rccl_combine.h"

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
  // coherent pinned buffer for small results, written by host_copy_kernel
  static constexpr size_t kMappedBytes = (size_t)64 << 10;
  uint8_t *h_mapped = nullptr;
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
  // the connection's mbx_scan_codes / mbx_scan_codes_min_rows (set by Eng)
  bool scan_codes = true;
  int64_t scan_codes_min_rows = 0;
  bool profile = false;
  std::vector<ProfEvent> events;
  // kernels timed on shard engines during this query (gpu_devices)
  std::mutex shard_mu;
  std::vector<QueryProfile::Kernel> shard_kernels;
  std::vector<std::pair<hipEvent_t, hipEvent_t>> ev_pool;  // reused across queries
  size_t ev_used = 0;
  // The per-kernel profile's event pairs: timing only (FinishProfile reads them
  // after a stream synchronisation), so without the system-scope fence a
  // recorded event otherwise performs (an L2 writeback and invalidate around
  // each timestamp, which also delays the next launch on the stream)
  std::pair<hipEvent_t, hipEvent_t> NextEvents() {
    if (ev_used == ev_pool.size()) {
      hipEvent_t a, b;
      (void)hipEventCreateWithFlags(&a, hipEventDisableSystemFence);
      (void)hipEventCreateWithFlags(&b, hipEventDisableSystemFence);
      ev_pool.push_back({a, b});
    }
    return ev_pool[ev_used++];
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

int DeviceCount() {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

// scratch for the device helpers (hipcub temp storage, hash flags) from the
// calling connection's pool
static void *TempAllocCb(size_t bytes, void *ctx) {
  DevicePool *p = (DevicePool *)ctx;
  return p->Get(DevicePool::Bucket(bytes ? bytes : 16));
}
static void TempFreeCb(void *ptr, size_t bytes, void *ctx) {
  if (ptr) ((DevicePool *)ctx)->Put(DevicePool::Bucket(bytes ? bytes : 16), ptr);
}

std::shared_ptr<Engine> CreateEngine(int device, bool allow_no_gpu) {
  auto e = std::make_shared<Engine>();
  int n = DeviceCount();
  if (n <= 0) {
    if (!allow_no_gpu)
      ThrowError("IO", "no AMD GPU visible: the MI355X backend requires a gfx950 device (HIP reports 0 devices)");
    e->has_gpu = false;
    return e;
  }
  if (device < 0) HIPCHK(hipGetDevice(&device));
  if (device >= n) ThrowError("IO", "gpu_device " + std::to_string(device) + " out of range (" + std::to_string(n) + " devices)");
  e->device = device;
  HIPCHK(hipSetDevice(device));
  HIPCHK(hipStreamCreateWithFlags(&e->stream, hipStreamNonBlocking));
  e->pool = std::make_shared<DevicePool>();
  e->pool->s = e->stream;
  e->pool->device = device;
  dev::SetTempAllocator(&TempAllocCb, &TempFreeCb, e->pool.get());
  HIPCHK(hipMalloc(&e->d_err, 256));
  HIPCHK(hipMalloc(&e->d_scratch, 4096));
  HIPCHK(hipMalloc(&e->d_small, 1 << 16));
  HIPCHK(hipMalloc(&e->d_partials, sizeof(dev::AggPartial) * dev::kMaxAggPartials));
  HIPCHK(hipMemset(e->d_err, 0, 256));
  e->h_pinned_bytes = 1 << 20;
  HIPCHK(hipHostMalloc((void **)&e->h_pinned, e->h_pinned_bytes, hipHostMallocDefault));
  HIPCHK(hipHostMalloc((void **)&e->h_mapped, Engine::kMappedBytes, hipHostMallocCoherent | hipHostMallocMapped));
  e->has_gpu = true;
  return e;
}

// n appended rows, nvalid of them non-NULL with values in [mn, mx], folded
// into the column's zone map
static void FoldStats(DevColumn &c, int64_t n, int64_t nvalid, i128 mn, i128 mx, bool first_rows) {
  c.null_count += n - nvalid;
  if (nvalid > 0) {
    if (first_rows || !c.stats_valid) {
      c.imin = mn;
      c.imax = mx;
    } else {
      c.imin = std::min<i128>(c.imin, mn);
      c.imax = std::max<i128>(c.imax, mx);
    }
  }
}

static void UpdateScanCodes(Engine &e, DevColumn &c, int64_t nrows);

// folds the zone-map statistics of in-flight appends into their columns
// (after the stream has drained: their DMAs and reductions are done), then
// brings the columns' code images up to the appended rows
static void SettlePending(Engine &e) {
  if (e.pending_stats.empty() && !e.inflight_h2d) return;
  HIPCHK(hipStreamSynchronize(e.stream));
  e.inflight_h2d = false;
  for (auto &ps : e.pending_stats) {
    const long long *h = ps.h;
    FoldStats(*ps.col, ps.n, h[2], h[0], h[1], ps.first_rows);
    e.stat_slots.push_back(ps.h);
  }
  std::vector<std::pair<DevColumn *, int64_t>> cols;  // each column once, at its last row count
  for (auto &ps : e.pending_stats) {
    auto it = std::find_if(cols.begin(), cols.end(), [&](const std::pair<DevColumn *, int64_t> &x) { return x.first == ps.col; });
    if (it == cols.end()) cols.push_back({ps.col, ps.rows});
    else it->second = std::max(it->second, ps.rows);
  }
  e.pending_stats.clear();
  for (auto &cr : cols) UpdateScanCodes(e, *cr.first, cr.second);
}

static Engine &Eng(Connection &c) {
  Engine &e = *c.engine;
  if (!e.has_gpu)
    ThrowError("IO", "this statement reads table rows and needs the MI355X device, but no GPU is available");
  hipSetDevice(e.device);
  dev::SetTempAllocator(&TempAllocCb, &TempFreeCb, e.pool.get());
  e.scan_codes = c.opts.scan_codes;
  e.scan_codes_min_rows = c.opts.scan_codes_min_rows;
  SettlePending(e);  // a statement never sees a column before its appended stats
  return e;
}

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
  ~ProfScope() {
    if (on) hipEventRecord(e.events[idx].b, e.stream);
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

static DevBufPtr Alloc(Engine &e, size_t bytes, bool zero = false) {
  auto b = std::make_shared<DevBuf>();
  if (bytes == 0) bytes = 16;
  b->bytes = DevicePool::Bucket(bytes);
  b->pool = e.pool;
  b->p = e.pool->Get(b->bytes);
  if (!b->p) ThrowError("Out of Memory", "device allocation of " + std::to_string(b->bytes) + " bytes failed");
  if (zero) HIPCHK(hipMemsetAsync(b->p, 0, b->bytes, e.stream));
  return b;
}

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

struct DRel {
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

static DCol ColFromTable(const DevColumn &c) {
  DCol d;
  for (const auto *o : {&c.data_owner, &c.validity_owner, &c.offsets_owner, &c.chars_owner, &c.codes_owner})
    if (*o) d.pins.push_back(*o);
  d.type = c.type;
  d.phys = c.phys;
  d.data = c.data;
  d.validity = c.validity;
  d.offsets = c.offsets;
  d.chars = c.chars;
  d.chars_len = c.chars_len;
  d.table_col = &c;
  return d;
}

static int64_t Words64(int64_t n) { return (n + 63) / 64; }

static void RaiseDeviceError(Engine &e, int32_t err);

static void CheckError(Engine &e) {
  // through the pinned arena: a pageable destination would take HIP's staged copy
  HIPCHK(hipMemcpyAsync(e.h_pinned, e.d_err, sizeof(int32_t), hipMemcpyDeviceToHost, e.stream));
  HIPCHK(hipStreamSynchronize(e.stream));
  int32_t err;
  memcpy(&err, e.h_pinned, sizeof(err));
  RaiseDeviceError(e, err);
}

static void RaiseDeviceError(Engine &e, int32_t err) {
  if (err) {
    HIPCHK(hipMemsetAsync(e.d_err, 0, sizeof(int32_t), e.stream));
    switch (err) {
      case E_OVF_ADD: ThrowError("Out of Range", "Overflow in addition!");
      case E_OVF_SUB: ThrowError("Out of Range", "Overflow in subtraction!");
      case E_OVF_MUL: ThrowError("Out of Range", "Overflow in multiplication!");
      case E_OVF_NEG: ThrowError("Out of Range", "Overflow in negation!");
      case E_CAST_RANGE: ThrowError("Conversion", "Value out of range for the destination type in CAST");
      case E_HASH_FULL: ThrowError("Internal", "hash aggregate table overflow");
      case E_KEY_RANGE: ThrowError("Internal", "GROUP BY key outside its column statistics");
      default: ThrowError("Out of Range", "Decimal value out of range");
    }
  }
}

template <typename T>
static T ReadDev(Engine &e, const void *p) {
  // through the pinned arena: a pageable destination would take HIP's staged copy
  static_assert(sizeof(T) <= 64, "small device words only");
  HIPCHK(hipMemcpyAsync(e.h_pinned, p, sizeof(T), hipMemcpyDeviceToHost, e.stream));
  HIPCHK(hipStreamSynchronize(e.stream));
  T v;
  memcpy(&v, e.h_pinned, sizeof(T));
  return v;
}

// a row count left on the device (DRel::n_dev) read back
static void SettleCount(Engine &e, DRel &r) {
  if (!r.n_dev) return;
  r.n = ReadDev<int64_t>(e, r.n_dev);
  r.n_dev = nullptr;
  r.n_owner.reset();
}

// ---------------------------------------------------------------------------
// host -> device upload of constant rows (VALUES, host-constant subqueries)
// ---------------------------------------------------------------------------
static void UploadHostColumn(Engine &e, const HostColumn &hc, int64_t n, DCol &d) {
  d.type = hc.type;
  d.phys = hc.phys;
  if (hc.phys == P_STR) {
    auto ob = Alloc(e, (n + 1) * sizeof(int64_t));
    auto cb = Alloc(e, std::max<size_t>(hc.chars.size(), 1));
    HIPCHK(hipMemcpyAsync(ob->p, hc.offsets.data(), (n + 1) * sizeof(int64_t), hipMemcpyHostToDevice, e.stream));
    if (!hc.chars.empty())
      HIPCHK(hipMemcpyAsync(cb->p, hc.chars.data(), hc.chars.size(), hipMemcpyHostToDevice, e.stream));
    d.offsets = (int64_t *)ob->p;
    d.chars = (char *)cb->p;
    d.chars_len = (int64_t)hc.chars.size();
    d.owners.push_back(ob);
    d.owners.push_back(cb);
  } else {
    size_t bytes = (size_t)n * PhysSize(hc.phys);
    auto db = Alloc(e, bytes);
    if (bytes) HIPCHK(hipMemcpyAsync(db->p, hc.data.data(), bytes, hipMemcpyHostToDevice, e.stream));
    d.data = db->p;
    d.owners.push_back(db);
  }
  bool anynull = false;
  for (int64_t i = 0; i < n; i++)
    if (hc.IsNull(i)) anynull = true;
  if (anynull) {
    std::vector<uint64_t> bm(Words64(n), 0);
    for (int64_t i = 0; i < n; i++)
      if (!hc.IsNull(i)) bm[i >> 6] |= 1ull << (i & 63);
    auto vb = Alloc(e, bm.size() * 8);
    HIPCHK(hipMemcpyAsync(vb->p, bm.data(), bm.size() * 8, hipMemcpyHostToDevice, e.stream));
    d.validity = (uint64_t *)vb->p;
    d.owners.push_back(vb);
  }
  // keep host staging alive until the copies are done
  HIPCHK(hipStreamSynchronize(e.stream));
}

static DRel UploadRows(Engine &e, const std::vector<std::vector<Value>> &rows, const std::vector<LogicalType> &types) {
  DRel r;
  r.n = (int64_t)rows.size();
  for (size_t c = 0; c < types.size(); c++) {
    HostColumn hc;
    hc.type = types[c];
    hc.phys = PhysOf(types[c]);
    if (hc.phys == P_STR) hc.offsets.push_back(0);
    for (auto &row : rows) HostColumnPush(hc, CastValue(row[c], types[c]));
    DCol d;
    UploadHostColumn(e, hc, r.n, d);
    r.cols.push_back(d);
  }
  return r;
}

// ---------------------------------------------------------------------------
// VM compiler: bound expressions -> tile program
// ---------------------------------------------------------------------------
struct StrPool {
  std::vector<std::string> s;
  int Add(const std::string &x) {
    for (size_t i = 0; i < s.size(); i++)
      if (s[i] == x) return (int)i;
    s.push_back(x);
    return (int)s.size() - 1;
  }
};

struct VmCompiler {
  VmProgram P;
  const DRel &rel;
  std::vector<int> colmap;  // rel col -> VmCols index
  dev::VmCols cols;
  bool used[VM_MAX_REGS] = {};
  int high = 0;
  StrPool *pool;
  int str_src_col = -1;  // the one source string column referenced by string outputs

  VmCompiler(const DRel &r, StrPool *p) : rel(r), pool(p) {
    memset(&P, 0, sizeof(P));
    memset(&cols, 0, sizeof(cols));
    colmap.assign(r.cols.size(), -1);
  }
  int Reg() {
    for (int i = 0; i < VM_MAX_REGS; i++)
      if (!used[i]) {
        used[i] = true;
        high = std::max(high, i + 1);
        return i;
      }
    ThrowError("Not implemented", "expression too complex for the device VM (registers)");
  }
  void Free(int r) {
    if (r >= 0 && r < VM_MAX_REGS) used[r] = false;
  }
  void Emit(uint8_t op, int d, int a = 0, int b = 0, int c = 0, int aux = 0) {
    if (P.n_ins >= VM_MAX_INS) ThrowError("Not implemented", "expression too complex for the device VM (instructions)");
    VmIns &I = P.ins[P.n_ins++];
    I.op = op;
    I.dst = (uint8_t)d;
    I.a = (uint8_t)a;
    I.b = (uint8_t)b;
    I.c = (uint8_t)c;
    I.aux = (uint16_t)aux;
  }
  // unary step consuming register a
  int Step1(uint8_t op, int a, int b = 0, int c = 0, int aux = 0) {
    int d = Reg();
    Emit(op, d, a, b, c, aux);
    Free(a);
    return d;
  }
  // binary step consuming registers a, b
  int Step2(uint8_t op, int a, int b, int aux = 0) {
    int d = Reg();
    Emit(op, d, a, b, 0, aux);
    Free(a);
    Free(b);
    return d;
  }
  int Const(i128 v, bool isnull = false) {
    int64_t lo = (int64_t)(uint64_t)(u128)v, hi = (int64_t)(uint64_t)((u128)v >> 64);
    for (int i = 0; i < P.n_const; i++)
      if (P.consts[i].lo == lo && P.consts[i].hi == hi && P.consts[i].isnull == (int)isnull) return i;
    if (P.n_const >= VM_MAX_CONST) ThrowError("Not implemented", "too many constants for the device VM");
    P.consts[P.n_const].lo = lo;
    P.consts[P.n_const].hi = hi;
    P.consts[P.n_const].isnull = isnull;
    return P.n_const++;
  }
  int ConstF(double d) {
    int64_t bits;
    memcpy(&bits, &d, 8);
    return Const((i128)bits);
  }
  int LoadConst(int k) {
    int d = Reg();
    Emit(V_CONST, d, k);
    return d;
  }
  int ColIdx(int c) {
    if (colmap[c] < 0) {
      if (cols.n >= VM_MAX_COLS) ThrowError("Not implemented", "too many columns in one device expression program");
      const DCol &d = rel.cols[c];
      cols.c[cols.n].data = d.phys == P_STR ? nullptr : d.data;
      cols.c[cols.n].validity = d.validity;
      cols.c[cols.n].phys = d.phys;
      colmap[c] = cols.n++;
    }
    return colmap[c];
  }

  // register class conversion without value checks
  int ToClass(int r, VClass from, VClass to) {
    if (from == to) return r;
    if (from == VC_I64 && to == VC_I128) return Step1(V_I2L, r);
    if (from == VC_I128 && to == VC_I64) return Step1(V_L2I, r, 255, 255);
    if (from == VC_I64 && to == VC_F64) return Step1(V_I2F, r);
    if (from == VC_I128 && to == VC_F64) return Step1(V_L2F, r);
    ThrowError("Not implemented", "unsupported register class conversion on device");
  }

  int RangeCheck(int r, VClass vc, i128 lo, i128 hi) {
    return Step1(vc == VC_I128 ? V_CHECK_L : V_CHECK_I, r, Const(lo), Const(hi));
  }

  int ToFloat32(int r) {
    int z = LoadConst(ConstF(0.0));
    return Step2(V_ADD_F, r, z, 1);
  }

  int CompileCast(const BExpr &e) {
    const LogicalType &from = e.ch[0]->type, &to = e.type;
    VClass fc = ClassOf(from), tc = ClassOf(to);
    if (fc == VC_STR || tc == VC_STR) {
      if (fc == VC_STR && tc == VC_STR) return Compile(*e.ch[0]);
      ThrowError("Not implemented", "casts between VARCHAR and " + (fc == VC_STR ? to : from).ToString() +
                                         " are not supported on the MI355X device path");
    }
    if (from.id == T_DATE || from.id == T_TIMESTAMP || from.id == T_TIME || to.id == T_DATE || to.id == T_TIMESTAMP ||
        to.id == T_TIME || from.id == T_INTERVAL || to.id == T_INTERVAL) {
      if (from.id == T_DATE && to.id == T_TIMESTAMP) {
        int r = Compile(*e.ch[0]);
        int k = LoadConst(Const(86400000000LL));
        return Step2(V_MUL_I, r, k);
      }
      ThrowError("Not implemented", "cast " + from.ToString() + " -> " + to.ToString() + " is not supported on device");
    }
    int r = Compile(*e.ch[0]);
    bool fint = IsIntegral(from.id) || from.id == T_BOOLEAN, tint = IsIntegral(to.id);
    bool fdec = from.id == T_DECIMAL, tdec = to.id == T_DECIMAL;
    bool ff = from.id == T_FLOAT || from.id == T_DOUBLE, tf = to.id == T_FLOAT || to.id == T_DOUBLE;
    if (to.id == T_BOOLEAN) return Step1(ff ? V_TOBOOL_F : V_TOBOOL_I, r);
    if (fint && tint) {
      i128 lo, hi, flo, fhi;
      IntegralRange(to.id, &lo, &hi);
      IntegralRange(from.id, &flo, &fhi);
      if (flo >= lo && fhi <= hi) {
        if (from.id == T_UBIGINT) return r;  // already 128-bit class
        return ToClass(r, fc, tc);
      }
      if (fc == VC_I128 && tc == VC_I64) return Step1(V_L2I, r, Const(lo), Const(hi));
      int x = ToClass(r, fc, tc);
      return RangeCheck(x, tc, lo, hi);
    }
    if ((fint || fdec) && tdec) {
      int fs = fdec ? from.scale : 0;
      int x = ToClass(r, fc, tc);
      int ds = to.scale - fs;
      if (ds > 0) x = Step1(tc == VC_I128 ? V_SCALEUP_L : V_SCALEUP_I, x, 0, 0, ds);
      else if (ds < 0) x = Step1(tc == VC_I128 ? V_SCALEDN_L : V_SCALEDN_I, x, 0, 0, -ds);
      i128 lim = Pow10(to.width) - 1;
      return RangeCheck(x, tc, -lim, lim);
    }
    if (fdec && tint) {
      int x = r;
      if (from.scale) x = Step1(fc == VC_I128 ? V_SCALEDN_L : V_SCALEDN_I, x, 0, 0, from.scale);
      i128 lo, hi;
      IntegralRange(to.id, &lo, &hi);
      if (fc == VC_I128 && tc == VC_I64) return Step1(V_L2I, x, Const(lo), Const(hi));
      x = ToClass(x, fc, tc);
      return RangeCheck(x, tc, lo, hi);
    }
    if ((fint || fdec) && tf) {
      int d;
      if (fdec) d = Step1(fc == VC_I128 ? V_DEC2F_L : V_DEC2F_I, r, 0, 0, from.scale);
      else d = Step1(fc == VC_I128 ? V_L2F : V_I2F, r);
      return to.id == T_FLOAT ? ToFloat32(d) : d;
    }
    if (ff && tf) return to.id == T_FLOAT ? ToFloat32(r) : r;
    if (ff && tint) {
      i128 lo, hi;
      IntegralRange(to.id, &lo, &hi);
      return Step1(tc == VC_I128 ? V_F2L : V_F2I, r, Const(lo), Const(hi));
    }
    if (ff && tdec) {
      i128 lim = Pow10(to.width) - 1;
      return Step1(tc == VC_I128 ? V_F2DEC_L : V_F2DEC_I, r, Const(-lim), Const(lim), to.scale);
    }
    ThrowError("Not implemented", "cast " + from.ToString() + " -> " + to.ToString() + " is not supported on device");
  }

  int Compile(const BExpr &e) {
    switch (e.kind) {
      case BExpr::CONST: {
        const Value &v = e.cval;
        VClass vc = ClassOf(e.type);
        if (v.is_null) return LoadConst(Const(0, true));
        if (vc == VC_F64) return LoadConst(ConstF(v.d));
        if (vc == VC_STR) {
          if (!pool) ThrowError("Not implemented", "string constants are not supported in this device context");
          return LoadConst(Const(-(i128)(pool->Add(v.s) + 1)));
        }
        if (e.type.id == T_INTERVAL) ThrowError("Not implemented", "INTERVAL values are not supported on device");
        return LoadConst(Const(v.i));
      }
      case BExpr::COL: {
        int d = Reg();
        if (rel.range && e.col == 0) {
          Emit(V_LOADRANGE, d);
          return d;
        }
        const DCol &c = rel.cols[e.col];
        if (c.phys == P_STR) {
          if (str_src_col >= 0 && str_src_col != e.col)
            ThrowError("Not implemented", "an expression mixing two VARCHAR columns is not supported on device");
          str_src_col = e.col;
        }
        if (c.phys == P_INTERVAL) ThrowError("Not implemented", "INTERVAL columns are not supported on device");
        Emit(V_LOADCOL, d, ColIdx(e.col), 0, 0, c.phys);
        return d;
      }
      default:
        break;
    }
    const LogicalType &t = e.type;
    VClass vc = ClassOf(t);
    switch (e.op) {
      case B_CAST: return CompileCast(e);
      case B_CASE: {
        size_t n = e.ch.size();
        int acc = (n % 2 == 1) ? Compile(*e.ch[n - 1]) : LoadConst(Const(0, true));
        for (int i = (int)(n / 2) - 1; i >= 0; i--) {
          int c = Compile(*e.ch[2 * i]);
          int v = Compile(*e.ch[2 * i + 1]);
          int d = Reg();
          Emit(V_SELECT, d, c, v, acc);
          Free(c);
          Free(v);
          Free(acc);
          acc = d;
        }
        return acc;
      }
      case B_COALESCE: {
        int acc = Compile(*e.ch.back());
        for (int i = (int)e.ch.size() - 2; i >= 0; i--) {
          int a = Compile(*e.ch[i]);
          acc = Step2(V_COALESCE, a, acc);
        }
        return acc;
      }
      case B_AND: case B_OR: {
        int a = Compile(*e.ch[0]), b = Compile(*e.ch[1]);
        return Step2(e.op == B_AND ? V_AND : V_OR, a, b);
      }
      case B_NOT: return Step1(V_NOT, Compile(*e.ch[0]));
      case B_ISNULL: return Step1(V_ISNULL, Compile(*e.ch[0]));
      case B_ISNOTNULL: return Step1(V_ISNOTNULL, Compile(*e.ch[0]));
      case B_SYNTH: {
        int a = Compile(*e.ch[0]), b = Compile(*e.ch[1]), c = Compile(*e.ch[2]);
        int d = Reg();
        Emit(V_SYNTH, d, a, b, c);
        Free(a);
        Free(b);
        Free(c);
        return d;
      }
      case B_EQ: case B_NE: case B_LT: case B_LE: case B_GT: case B_GE:
      case B_DISTINCT: case B_NOT_DISTINCT: {
        VClass cc = ClassOf(e.ch[0]->type);
        if (cc == VC_STR) ThrowError("Not implemented", "VARCHAR comparisons are not supported on the MI355X device path");
        if (e.ch[0]->type.id == T_INTERVAL) ThrowError("Not implemented", "INTERVAL comparisons are not supported on device");
        int a = Compile(*e.ch[0]), b = Compile(*e.ch[1]);
        if (e.op == B_DISTINCT || e.op == B_NOT_DISTINCT)
          return Step2(cc == VC_F64 ? V_DISTINCT_F : cc == VC_I128 ? V_DISTINCT_L : V_DISTINCT_I, a, b,
                       e.op == B_NOT_DISTINCT ? 1 : 0);
        int k = e.op == B_EQ ? 0 : e.op == B_NE ? 1 : e.op == B_LT ? 2 : e.op == B_LE ? 3 : e.op == B_GT ? 4 : 5;
        return Step2(cc == VC_F64 ? V_CMP_F : cc == VC_I128 ? V_CMP_L : V_CMP_I, a, b, k);
      }
      case B_NEG: case B_ABS: {
        int a = Compile(*e.ch[0]);
        uint8_t op = e.op == B_NEG ? (vc == VC_F64 ? V_NEG_F : vc == VC_I128 ? V_NEG_L : V_NEG_I)
                                   : (vc == VC_F64 ? V_ABS_F : vc == VC_I128 ? V_ABS_L : V_ABS_I);
        int d = Step1(op, a);
        if (vc == VC_I64 && IsIntegral(t.id) && t.id != T_BIGINT) {
          i128 lo, hi;
          IntegralRange(t.id, &lo, &hi);
          return RangeCheck(d, vc, lo, hi);
        }
        return d;
      }
      case B_ADD: case B_SUB: case B_MUL: case B_DIV: case B_IDIV: case B_MOD: {
        if (t.id == T_DATE || t.id == T_TIMESTAMP || t.id == T_INTERVAL)
          ThrowError("Not implemented", "date/interval arithmetic is not supported on the MI355X device path");
        if (vc == VC_STR) ThrowError("Not implemented", "string arithmetic is not supported on device");
        int a = Compile(*e.ch[0]);
        a = ToClass(a, ClassOf(e.ch[0]->type), vc);
        int b = Compile(*e.ch[1]);
        b = ToClass(b, ClassOf(e.ch[1]->type), vc);
        uint8_t op;
        if (vc == VC_F64) {
          op = e.op == B_ADD ? V_ADD_F : e.op == B_SUB ? V_SUB_F : e.op == B_MUL ? V_MUL_F : e.op == B_DIV ? V_DIV_F
               : e.op == B_MOD ? V_MOD_F : V_IDIV_F;
          return Step2(op, a, b, t.id == T_FLOAT ? 1 : 0);
        }
        if (vc == VC_I128) op = e.op == B_ADD ? V_ADD_L : e.op == B_SUB ? V_SUB_L : e.op == B_MUL ? V_MUL_L
                                : e.op == B_MOD ? V_MOD_L : V_DIV_L;
        else op = e.op == B_ADD ? V_ADD_I : e.op == B_SUB ? V_SUB_I : e.op == B_MUL ? V_MUL_I
                  : e.op == B_MOD ? V_MOD_I : V_DIV_I;
        int d = Step2(op, a, b);
        if (vc == VC_I64 && IsIntegral(t.id) && t.id != T_BIGINT) {
          i128 lo, hi;
          IntegralRange(t.id, &lo, &hi);
          return RangeCheck(d, vc, lo, hi);
        }
        return d;
      }
      default:
        ThrowError("Not implemented", "function " + ExprToString(e) + " is not supported on the MI355X device path");
    }
  }
};

// Does the expression (transitively) only reference columns, and which?
static void CollectCols(const BExpr &e, std::vector<int> &out) {
  if (e.kind == BExpr::COL) out.push_back(e.col);
  for (auto &c : e.ch) CollectCols(*c, out);
}

// ---------------------------------------------------------------------------
// filter + project
// ---------------------------------------------------------------------------
struct StrOut {
  int out_idx;
  int src_col;  // -1: pool only
};

static DCol AllocOut(Engine &e, const LogicalType &t, int64_t n, bool with_valid, bool zero_valid = true) {
  DCol d;
  d.type = t;
  d.phys = PhysOf(t);
  int sz = d.phys == P_STR ? 8 : PhysSize(d.phys);
  auto b = Alloc(e, (size_t)std::max<int64_t>(n, 1) * sz);
  d.data = b->p;
  d.owners.push_back(b);
  if (with_valid) {
    auto v = Alloc(e, Words64(std::max<int64_t>(n, 1)) * 8, zero_valid);
    d.validity = (uint64_t *)v->p;
    d.owners.push_back(v);
  }
  return d;
}

static void MaterializeStrings(Engine &e, DCol &out, const DCol *src, const StrPool &pool, int64_t n) {
  // out.data holds int64 codes; build offsets + chars
  std::vector<int64_t> poff(1, 0);
  std::string pchars;
  for (auto &s : pool.s) {
    pchars += s;
    poff.push_back((int64_t)pchars.size());
  }
  auto pob = Alloc(e, poff.size() * 8);
  auto pcb = Alloc(e, std::max<size_t>(pchars.size(), 1));
  HIPCHK(hipMemcpyAsync(pob->p, poff.data(), poff.size() * 8, hipMemcpyHostToDevice, e.stream));
  if (!pchars.empty()) HIPCHK(hipMemcpyAsync(pcb->p, pchars.data(), pchars.size(), hipMemcpyHostToDevice, e.stream));
  auto lens = Alloc(e, std::max<int64_t>(n, 1) * 8);
  auto offs = Alloc(e, (n + 1) * 8);
  const int64_t *soff = src ? src->offsets : nullptr;
  const char *schars = src ? src->chars : nullptr;
  dev::StringLengths((const int64_t *)out.data, out.validity, n, soff, (const int64_t *)pob->p, (int64_t *)lens->p,
                     e.stream);
  dev::ScanLengths((const int64_t *)lens->p, (int64_t *)offs->p, n, e.stream);
  int64_t total = ReadDev<int64_t>(e, (int64_t *)offs->p + n);
  auto chars = Alloc(e, std::max<int64_t>(total, 1));
  dev::StringCopy((const int64_t *)out.data, out.validity, n, soff, schars, (const int64_t *)pob->p,
                  (const char *)pcb->p, (const int64_t *)offs->p, (char *)chars->p, e.stream);
  HIPCHK(hipStreamSynchronize(e.stream));  // pool staging buffers go out of scope
  out.offsets = (int64_t *)offs->p;
  out.chars = (char *)chars->p;
  out.chars_len = total;
  out.owners.push_back(offs);
  out.owners.push_back(chars);
  out.data = nullptr;
}

static bool TryFilterCompact(Engine &e, const DRel &rel, const BExpr &pred, const std::vector<BExprPtr> &exprs,
                             DRel &out);

// Evaluates `pred` (may be null) and `exprs` over `rel`; returns the
// projected relation of the selected rows.
static DRel FilterProject(Engine &e, const DRel &rel, const BExprPtr &pred, const std::vector<BExprPtr> &exprs) {
  const int64_t n = rel.n;
  if (rel.n_dev) {  // only a column passthrough may carry a row count still on the device
    bool pt = !pred;
    for (auto &x : exprs) pt &= x->kind == BExpr::COL && !(rel.range && x->col == 0);
    if (!pt) ThrowError("Internal", "a relation with its row count on the device reached a projection");
  }
  {
    DRel fused;
    if (pred && pred->kind != BExpr::CONST && TryFilterCompact(e, rel, *pred, exprs, fused)) return fused;
  }
  // pure column passthrough, no predicate, no virtual range column
  bool passthrough = !pred;
  for (auto &x : exprs)
    if (x->kind != BExpr::COL || (rel.range && x->col == 0)) passthrough = false;
  if (passthrough) {
    DRel out;
    out.n = n;
    out.n_dev = rel.n_dev;
    out.n_owner = rel.n_owner;
    for (auto &x : exprs) out.cols.push_back(rel.cols[x->col]);
    return out;
  }

  const int64_t ntiles = (n + VM_TILE - 1) / VM_TILE;
  DevBufPtr bits, offs;
  int64_t nsel = n;
  if (pred) {
    if (pred->kind == BExpr::CONST) {
      bool keep = !pred->cval.is_null && pred->cval.i;
      if (!keep) nsel = 0;
    } else {
      StrPool dummy;
      VmCompiler vc(rel, nullptr);
      int r = vc.Compile(*pred);
      vc.P.pred_reg = (uint8_t)r;
      vc.P.n_regs = vc.high;
      bits = Alloc(e, std::max<int64_t>(ntiles, 1) * 4 * 8);
      auto counts = Alloc(e, std::max<int64_t>(ntiles, 1) * 4);
      offs = Alloc(e, std::max<int64_t>(ntiles, 1) * 8);
      {
        ProfScope ps(e, "vm_filter", 0, n);
        if (!jit::VmFilter(vc.P, vc.cols, n, rel.rs, rel.rstep, (uint64_t *)bits->p, (uint32_t *)counts->p, e.d_err,
                           e.stream))
          dev::VmFilter(vc.P, vc.cols, n, rel.rs, rel.rstep, (uint64_t *)bits->p, (uint32_t *)counts->p, e.d_err,
                        e.stream);
      }
      dev::ScanTileCounts((const uint32_t *)counts->p, (int64_t *)offs->p, ntiles, e.d_scratch, e.stream);
      nsel = ReadDev<int64_t>(e, e.d_scratch);
      CheckError(e);
    }
  }
  DRel out;
  out.n = nsel;
  if (exprs.empty()) return out;
  // compile all outputs into one program (split into chunks of VM_MAX_OUT)
  for (size_t base = 0; base < exprs.size(); base += VM_MAX_OUT) {
    size_t cnt = std::min<size_t>(VM_MAX_OUT, exprs.size() - base);
    StrPool pool;
    std::vector<DCol> outs;
    std::vector<StrOut> strs;
    // one program per chunk; string outputs each need their own program (src column tracking)
    VmCompiler vc(rel, &pool);
    std::vector<int> src_cols(cnt, -1);
    for (size_t k = 0; k < cnt; k++) {
      const BExpr &x = *exprs[base + k];
      int prev_src = vc.str_src_col;
      if (ClassOf(x.type) == VC_STR) vc.str_src_col = -1;
      int r = vc.Compile(x);
      if (ClassOf(x.type) == VC_STR) {
        src_cols[k] = vc.str_src_col;
      }
      vc.str_src_col = prev_src < 0 ? vc.str_src_col : prev_src;
      vc.P.out_reg[k] = (uint8_t)r;
      vc.P.out_phys[k] = ClassOf(x.type) == VC_STR ? (uint8_t)P_I64 : (uint8_t)PhysOf(x.type);
      vc.P.out_class[k] = ClassOf(x.type);
      // r stays allocated (pinned) until the end of the program
    }
    vc.P.n_out = (int)cnt;
    vc.P.n_regs = vc.high;
    auto anynull = Alloc(e, VM_MAX_OUT * 4, true);
    dev::VmOuts vo;
    memset(&vo, 0, sizeof(vo));
    vo.anynull = (int32_t *)anynull->p;
    for (size_t k = 0; k < cnt; k++) {
      DCol d = AllocOut(e, exprs[base + k]->type, nsel, true);  // zeroed: the NULL bitmap until inverted
      vo.data[k] = d.data;
      vo.nullbits[k] = (uint32_t *)d.validity;
      outs.push_back(d);
    }
    if (nsel > 0) {
      ProfScope ps(e, "vm_project", 0, n);
      if (!jit::VmProject(vc.P, vc.cols, n, rel.rs, rel.rstep, bits ? (const uint64_t *)bits->p : nullptr,
                     offs ? (const int64_t *)offs->p : nullptr, vo, e.d_err, e.stream))
        dev::VmProject(vc.P, vc.cols, n, rel.rs, rel.rstep, bits ? (const uint64_t *)bits->p : nullptr,
                     offs ? (const int64_t *)offs->p : nullptr, vo, e.d_err, e.stream);
    }
    int32_t an[VM_MAX_OUT];
    HIPCHK(hipMemcpyAsync(an, anynull->p, sizeof(an), hipMemcpyDeviceToHost, e.stream));
    CheckError(e);
    for (size_t k = 0; k < cnt; k++) {
      DCol &d = outs[k];
      if (!an[k]) d.validity = nullptr;  // all valid: drop the bitmap (owner freed with the column)
      else dev::InvertNullBits(d.validity, nsel, e.stream);
      if (ClassOf(exprs[base + k]->type) == VC_STR) {
        const DCol *src = src_cols[k] >= 0 ? &rel.cols[src_cols[k]] : nullptr;
        MaterializeStrings(e, d, src, pool, nsel);
        d.phys = P_STR;
      }
      out.cols.push_back(d);
    }
  }
  return out;
}

// ---------------------------------------------------------------------------
// aggregation
// ---------------------------------------------------------------------------
// Column-vs-constant predicate that is a conjunction of comparisons on ONE
// integer column: folded to lo <= col <= hi (inclusive).
static const BExpr *StripWidening(const BExpr *x) {
  while (x->kind == BExpr::FUNC && x->op == B_CAST) {
    const LogicalType &f = x->ch[0]->type, &t = x->type;
    bool ok = false;
    if ((IsIntegral(f.id) || f.id == T_BOOLEAN) && IsIntegral(t.id)) {
      i128 a, b, c, d;
      IntegralRange(f.id, &a, &b);
      IntegralRange(t.id, &c, &d);
      ok = a >= c && b <= d;
    } else if (f.id == T_DECIMAL && t.id == T_DECIMAL && f.scale == t.scale && t.width >= f.width) {
      ok = true;
    }
    if (!ok) return x;
    x = x->ch[0].get();
  }
  return x;
}

static bool RangePredicate(const BExpr &p, int *col, i128 *lo, i128 *hi) {
  if (p.kind == BExpr::FUNC && p.op == B_AND) {
    return RangePredicate(*p.ch[0], col, lo, hi) && RangePredicate(*p.ch[1], col, lo, hi);
  }
  if (p.kind != BExpr::FUNC) return false;
  if (p.op != B_EQ && p.op != B_LT && p.op != B_LE && p.op != B_GT && p.op != B_GE) return false;
  const BExpr *a = StripWidening(p.ch[0].get()), *b = StripWidening(p.ch[1].get());
  BOp op = p.op;
  if (a->kind == BExpr::CONST && b->kind == BExpr::COL) {
    std::swap(a, b);
    op = op == B_LT ? B_GT : op == B_LE ? B_GE : op == B_GT ? B_LT : op == B_GE ? B_LE : op;
  }
  if (a->kind != BExpr::COL || b->kind != BExpr::CONST) return false;
  if (ClassOf(p.ch[0]->type) != VC_I64 && ClassOf(p.ch[0]->type) != VC_I128) return false;
  if (p.ch[0]->type.id == T_DOUBLE || p.ch[0]->type.id == T_FLOAT) return false;
  if (*col >= 0 && *col != a->col) return false;
  *col = a->col;
  if (b->cval.is_null) {  // comparison with NULL selects nothing
    *lo = 1;
    *hi = 0;
    return true;
  }
  i128 c = b->cval.i;
  switch (op) {
    case B_EQ: *lo = std::max(*lo, c); *hi = std::min(*hi, c); break;
    case B_GT: *lo = std::max(*lo, c + 1); break;
    case B_GE: *lo = std::max(*lo, c); break;
    case B_LT: *hi = std::min(*hi, c - 1); break;
    case B_LE: *hi = std::min(*hi, c); break;
    default: return false;
  }
  return true;
}

// Conjunction of range predicates over several integer columns: per column
// lo <= col <= hi (inclusive).  false if any leaf is not such a comparison.
static bool RangeConj(const BExpr &p, std::map<int, std::pair<i128, i128>> &ranges) {
  if (p.kind == BExpr::FUNC && p.op == B_AND) return RangeConj(*p.ch[0], ranges) && RangeConj(*p.ch[1], ranges);
  int col = -1;
  i128 lo = (i128)INT64_MIN, hi = (i128)INT64_MAX;
  if (!RangePredicate(p, &col, &lo, &hi) || col < 0) return false;
  auto it = ranges.find(col);
  if (it == ranges.end()) {
    ranges[col] = {lo, hi};
  } else {
    it->second.first = std::max(it->second.first, lo);
    it->second.second = std::min(it->second.second, hi);
  }
  return true;
}

static bool FastIntCol(const DRel &rel, int c) {
  if (rel.range && c == 0) return false;
  const DCol &d = rel.cols[c];
  return d.validity == nullptr && (d.phys == P_I32 || d.phys == P_I64) && d.data != nullptr;
}

// One-pass forms of the compaction below, for 4/8-byte columns, at most
// SL_MAX_COL distinct loaded columns (predicates ∪ outputs) and SL_MAX_OUT
// outputs.  NULL-able columns take the round-synchronous form only: a NULL
// fails a predicate, and a NULL-able output's validity comes back as one byte
// per output row, packed into its bitmap afterwards (dev::PackValidityBytes).  Each loaded column is read from HBM once; outputs are
// allocated for every row (the count is known only afterwards), so the form
// is used while that upper bound stays under MBX_SL_MAX_GB (default 64).
//  * default (n >= MBX_SR_MIN_ROWS, default 2^22): dev::SelectRounds, the
//    round-synchronous kernel (one persistent workgroup per CU).  Engines that
//    share a device (gpu_devices=0,0) take turns through a per-device lock, so
//    two persistent grids never compete for the CUs; should a workgroup never
//    be scheduled anyway, the kernel gives up after 100 ms without progress
//    and the two-pass form runs instead.
//  * MBX_SL=0: never (the count-first / ballot-bits two-pass forms).  (A
//    decoupled look-back one-pass kernel measured 2-9x slower than the
//    two-pass forms and was removed, profiles/r02_select_onepass.log.)
static std::mutex g_rounds_mu[64];

static bool TrySelectOnePass(Engine &e, const DRel &rel, const dev::FilterMultiDesc &F,
                             const std::vector<BExprPtr> &exprs, DRel &out) {
  const char *env = Knob("MBX_SL");
  const int mode = env ? atoi(env) : 1;
  if (mode == 0) return false;
  int64_t min_rows = (int64_t)1 << 22;
  if (const char *m = Knob("MBX_SR_MIN_ROWS")) min_rows = atoll(m);
  if (rel.n < min_rows) return false;
  if ((int)exprs.size() > SL_MAX_OUT) return false;
  dev::SelectDesc S;
  memset(&S, 0, sizeof(S));
  auto slot_of = [&](const void *data, int w) -> int {
    for (int i = 0; i < S.ncol; i++)
      if (S.col[i].data == data) return S.col[i].w == w ? i : -2;
    if (S.ncol >= SL_MAX_COL) return -1;
    S.col[S.ncol].data = data;
    S.col[S.ncol].w = w;
    return S.ncol++;
  };
  bool any_valid = false;
  for (int j = 0; j < F.ncol; j++) {
    if (F.col[j].valid && (uintptr_t)F.col[j].valid % 16) return false;
    const int i = slot_of(F.col[j].data, F.col[j].phys == P_I64 ? 8 : 4);
    if (i < 0) return false;
    S.col[i].valid = F.col[j].valid;
    any_valid |= F.col[j].valid != nullptr;
    S.col[i].is_pred = 1;
    S.col[i].lo = F.col[j].lo;
    S.col[i].span = F.col[j].span;
  }
  double out_bytes = 0;
  const char *nenv = Knob("MBX_SR_NARROW");
  const bool narrow_ok = !(nenv && atoi(nenv) == 0);
  const char *senv = Knob("MBX_SR_SENT");  // MBX_SR_SENT=0: NULL-able outputs stage validity bytes (A/B)
  const bool sent_off = senv && atoi(senv) == 0;
  for (auto &x : exprs) {
    const DCol &c = rel.cols[x->col];
    if (c.validity && (uintptr_t)c.validity % 16) return false;
    const int w = PhysSize(c.phys);
    if (w != 4 && w != 8) return false;
    const int i = slot_of(c.data, w);
    if (i < 0) return false;
    S.col[i].valid = c.validity;
    any_valid |= c.validity != nullptr;
    S.out_col[S.nout++] = i;
    out_bytes += (double)rel.n * (w + (c.validity ? 1 : 0));
    // an INT64 table column whose zone map fits int32 is staged in 4 bytes (the
    // map covers the valid rows; a NULL row's staged value is never read)
    const DevColumn *tc = c.table_col;
    if (narrow_ok && w == 8 && tc && tc->stats_valid && tc->imin >= (i128)INT32_MIN && tc->imax <= (i128)INT32_MAX)
      S.col[i].narrow = 1;
    // a NULL-able output whose zone map leaves a value of the staged width
    // unused stages NULL rows as that value instead of staging a validity byte
    // per row: the staging rows are as wide as without NULLs, so the shape
    // keeps the loader count and ring of its NULL-free form
    if (c.validity && tc && tc->stats_valid && !sent_off) {
      const bool w4 = w == 4 || S.col[i].narrow;
      const i128 tmax = w4 ? (i128)INT32_MAX : (i128)INT64_MAX, tmin = w4 ? (i128)INT32_MIN : (i128)INT64_MIN;
      if (tc->imax < tmax) S.col[i].vsent = 1, S.col[i].sent = (int64_t)tmax;
      else if (tc->imin > tmin) S.col[i].vsent = 1, S.col[i].sent = (int64_t)tmin;
    }
  }
  if (any_valid) {  // MBX_SR_NULLS=0: NULL-able shapes keep the two-pass form (A/B tests)
    const char *nv = Knob("MBX_SR_NULLS");
    if (nv && atoi(nv) == 0) return false;
  }
  int ni = 0;
  for (int i = 0; i < S.ncol; i++) ni += S.col[i].w / 4;
  if (ni > 8) return false;
  double cap_gb = 64;
  if (const char *c = Knob("MBX_SL_MAX_GB")) cap_gb = atof(c);
  if (out_bytes > cap_gb * 1e9) return false;
  const int64_t n = rel.n;
  const dev::SelectRoundsPlan plan = dev::PlanSelectRounds(S, n);
  if (!plan.ok) return false;
  std::vector<DCol> cols;
  std::vector<DevBufPtr> vbytes(exprs.size());  // NULL-able outputs: one validity byte per output row
  for (int k = 0; k < (int)exprs.size(); k++) {
    const bool nullable = rel.cols[exprs[k]->col].validity != nullptr;
    cols.push_back(AllocOut(e, exprs[k]->type, n, nullable, false));
    S.dst[k] = cols[k].data;
    if (nullable) {
      vbytes[k] = Alloc(e, (size_t)std::max<int64_t>(n, 1) + 64);
      S.vdst[k] = (uint8_t *)vbytes[k]->p;
    }
  }
  double bytes = 0;
  for (int i = 0; i < S.ncol; i++) bytes += (double)n * S.col[i].w + (S.col[i].valid ? n / 8.0 : 0);
  int64_t nsel = 0;
  int32_t rounds_err = -1;  // the error word read with the round total (-1: not read)
  {
    std::unique_lock<std::mutex> lk(g_rounds_mu[e.device & 63]);
    const size_t need = dev::SelectRoundsCtlBytes(plan);
    if (need > e.rounds_bytes) {
      HIPCHK(hipStreamSynchronize(e.stream));
      if (e.d_rounds) HIPCHK(hipFree(e.d_rounds));
      e.d_rounds = nullptr;
      size_t b = 1 << 20;
      while (b < need) b <<= 1;
      HIPCHK(hipMalloc((void **)&e.d_rounds, b));
      HIPCHK(hipMemsetAsync(e.d_rounds, 0, b, e.stream));
      e.rounds_bytes = b;
      e.rounds_epoch = 0;
    }
    if (++e.rounds_epoch == 0) {  // 2^32 launches: start over from a zeroed block
      HIPCHK(hipMemsetAsync(e.d_rounds, 0, e.rounds_bytes, e.stream));
      e.rounds_epoch = 1;
    }
    const uint32_t epoch = e.rounds_epoch;
    DevBufPtr dbgbuf, tsbuf;
    if (Knob("MBX_SR_DEBUG")) {
      dbgbuf = Alloc(e, 256, true);
      HIPCHK(hipMemsetAsync(dbgbuf->p, 0, 256, e.stream));
      S.dbg = (unsigned long long *)dbgbuf->p;
      if (atoi(Knob("MBX_SR_DEBUG")) == 2) {
        tsbuf = Alloc(e, (size_t)plan.nrounds * plan.G * 8, true);
        S.dbg_ts = (unsigned long long *)tsbuf->p;
      }
    }
    const char *zk = Knob("MBX_SR_ZONE");  // 0: the append's own zone-map pass instead (A/B)
    if (e.want_zone_maps && !(zk && atoi(zk) == 0)) {
      for (int k = 0; k < S.nout; k++) {
        const Phys ph = rel.cols[exprs[k]->col].phys;
        if (ph == P_I32 || ph == P_I64) S.zmask |= 1 << S.out_col[k];
      }
      if (S.zmask) {  // {INT64_MAX, INT64_MIN, 0} per column, from the pinned arena (synchronised below)
        S.zstats = (long long *)((char *)e.d_small + 4096);
        // which role folds the map: with 4 loaders the storers have slack and
        // fold it for free while copying (CTAS SELECT k, v ... WHERE x > 24:
        // 4.59 ms, as the selection alone; loaders 5.00); 8 loaders keep their
        // storers busy, so the loaders fold it (SELECT x ... WHERE x > 24:
        // 2.21 ms; storers 2.35)
        S.zstore = plan.NL == 4;  // (each kernel instance compiles the map in that role only)
        long long *z0 = (long long *)(e.h_pinned + 256);
        for (int c = 0; c < SL_MAX_COL; c++) z0[3 * c] = LLONG_MAX, z0[3 * c + 1] = LLONG_MIN, z0[3 * c + 2] = 0;
        HIPCHK(hipMemcpyAsync(S.zstats, z0, SL_MAX_COL * 3 * sizeof(long long), hipMemcpyHostToDevice, e.stream));
      }
    }
    hipError_t launch;
    {
      ProfScope ps(e, "select_rounds", bytes, n);  // algorithmic: inputs once (+ the selected rows' outputs, added below)
      launch = dev::SelectRounds(S, plan, n, e.d_rounds, epoch, e.stream);
    }
    e.sr_launches++;
    if (launch != hipSuccess) {  // nothing ran: the control block still holds the last launch's total
      e.sr_launch_failures++;
      if (e.profile && !e.events.empty() && e.events.back().name == "select_rounds")
        e.events.back().name = "select_rounds_launch_failed";
      return false;  // the two-pass form instead
    }
    if (dbgbuf) {
      unsigned long long h[14];
      HIPCHK(hipMemcpyAsync(h, dbgbuf->p, sizeof(h), hipMemcpyDeviceToHost, e.stream));
      HIPCHK(hipStreamSynchronize(e.stream));
      const double L = (double)plan.G * plan.NL, Ls = (double)plan.G * plan.NS, C = (double)plan.G;
      fprintf(stderr, "[select_rounds] G %d rounds %lld S %d stg %d depth %d | per loader: cycles %.0f dma_wait %.0f "
              "staging_wait %.0f meta_wait %.0f | per storer: cycles %.0f base_wait %.0f copy %.0f | per coordinator: cycles %.0f "
              "polls %.1f no_progress %.1f poll_load_cycles %.0f (%.0f per poll) rounds %.1f max/poll %llu "
              "publish->resolve %.0f cycles/round\n",
              plan.G, (long long)plan.nrounds, plan.S, plan.stg, plan.depth, h[0] / L, h[1] / L, h[2] / L, h[3] / L,
              h[4] / Ls, h[5] / Ls, h[13] / Ls, h[6] / C, h[7] / C, h[8] / C, h[9] / C, h[7] ? (double)h[9] / h[7] : 0.0, h[10] / C,
              h[11], h[10] ? (double)h[12] / h[10] : 0.0);
      if (tsbuf) {  // publish-time spread per round (10 ns ticks): how far the last workgroup trails
        std::vector<unsigned long long> ts((size_t)plan.nrounds * plan.G);
        HIPCHK(hipMemcpy(ts.data(), tsbuf->p, ts.size() * 8, hipMemcpyDeviceToHost));
        std::vector<double> spread, late_med;
        std::vector<double> wg_late(plan.G, 0.0);
        for (int64_t r = 0; r < plan.nrounds; r++) {
          std::vector<unsigned long long> v(ts.begin() + r * plan.G, ts.begin() + (r + 1) * plan.G);
          std::vector<unsigned long long> srt = v;
          std::sort(srt.begin(), srt.end());
          spread.push_back((double)(srt.back() - srt.front()));
          late_med.push_back((double)(srt.back() - srt[srt.size() / 2]));
          for (int gg = 0; gg < plan.G; gg++) wg_late[gg] += (double)(v[gg] - srt[srt.size() / 2]);
        }
        auto mean = [](const std::vector<double> &x) { double a = 0; for (double y : x) a += y; return x.empty() ? 0 : a / x.size(); };
        std::sort(spread.begin(), spread.end());
        int worst = 0;
        for (int gg = 1; gg < plan.G; gg++) if (wg_late[gg] > wg_late[worst]) worst = gg;
        std::vector<double> wl = wg_late;
        std::sort(wl.begin(), wl.end());
        fprintf(stderr, "[select_rounds] publish spread per round (us): mean %.2f median %.2f p90 %.2f max %.2f | "
                "last - median mean %.2f | round period %.2f us | per-WG mean lateness vs median (us): min %.2f "
                "median %.2f max %.2f (wg %d)\n",
                mean(spread) / 100, spread[spread.size() / 2] / 100, spread[spread.size() * 9 / 10] / 100,
                spread.back() / 100, mean(late_med) / 100,
                plan.nrounds > 1 ? (double)(ts[(plan.nrounds - 1) * plan.G] - ts[0]) / 100 / (plan.nrounds - 1) : 0.0,
                wl.front() / plan.nrounds / 100, wl[wl.size() / 2] / plan.nrounds / 100, wl.back() / plan.nrounds / 100,
                worst);
      }
    }
    // {abort word, total} and the device error word in one synchronisation
    // (pinned arena: a pageable destination would take HIP's staged copy)
    unsigned long long h[2];
    HIPCHK(hipMemcpyAsync(e.h_pinned, e.d_rounds, sizeof(h), hipMemcpyDeviceToHost, e.stream));
    HIPCHK(hipMemcpyAsync(e.h_pinned + 16, e.d_err, sizeof(int32_t), hipMemcpyDeviceToHost, e.stream));
    if (S.zmask)
      HIPCHK(hipMemcpyAsync(e.h_pinned + 64, S.zstats, SL_MAX_COL * 3 * sizeof(long long), hipMemcpyDeviceToHost,
                            e.stream));
    HIPCHK(hipStreamSynchronize(e.stream));
    memcpy(h, e.h_pinned, sizeof(h));
    memcpy(&rounds_err, e.h_pinned + 16, sizeof(rounds_err));
    if (S.zmask && h[0] != (unsigned long long)epoch) {
      const long long *z = (const long long *)(e.h_pinned + 64);
      for (int k = 0; k < S.nout; k++) {
        const int oc = S.out_col[k];
        if (!((S.zmask >> oc) & 1)) continue;
        cols[k].zn = (int64_t)h[1];
        cols[k].zmin = z[3 * oc];
        cols[k].zmax = z[3 * oc + 1];
        cols[k].zvalid = S.col[oc].valid ? z[3 * oc + 2] : (int64_t)h[1];  // (counted for NULL-able columns only)
      }
    }
    lk.unlock();
    if (h[0] == (unsigned long long)epoch) {  // a workgroup was never scheduled: two-pass form instead
      e.sr_aborts++;
      if (e.profile && !e.events.empty() && e.events.back().name == "select_rounds") e.events.back().name = "select_rounds_abort";
      return false;
    }
    nsel = (int64_t)h[1];
  }
  if (e.profile && !e.events.empty() && e.events.back().name == "select_rounds") {
    double ob = 0;
    for (int k = 0; k < S.nout; k++) ob += (double)nsel * (S.col[S.out_col[k]].w + (S.vdst[k] ? 1 : 0));
    e.events.back().bytes += ob;
  }
  for (int k = 0; k < S.nout; k++) {
    if (!S.vdst[k]) continue;
    ProfScope ps(e, "pack_validity", (double)nsel + nsel / 8.0, nsel);
    dev::PackValidityBytes(S.vdst[k], nsel, cols[k].validity, e.stream);
  }
  out = DRel();
  out.n = nsel;
  out.cols = cols;
  bool packed = false;
  for (int k = 0; k < S.nout; k++) packed |= S.vdst[k] != nullptr;
  if (rounds_err >= 0 && !packed) RaiseDeviceError(e, rounds_err);  // nothing ran after that read
  else CheckError(e);
  return true;
}

// Count-first two-pass compaction (dev::FilterCountChunks, scan,
// dev::CompactRecompute) when every predicate column is also an output and all
// columns are NULL-free 4/8-byte ones (SELECT x FROM t WHERE x > 24): pass 1
// writes one count per 2048-row chunk instead of per-row ballot bits, and pass 2
// evaluates the predicates again on the slices it loads anyway, each wave
// storing its chunk as one contiguous run.  MBX_CC=0 keeps the bits form.
static bool TryCountFirst(Engine &e, const DRel &rel, const dev::FilterMultiDesc &F,
                          const std::vector<BExprPtr> &exprs, DRel &out) {
  const char *env = Knob("MBX_CC");
  if (env && atoi(env) == 0) return false;
  if ((int)exprs.size() > FC_MAX_OUT) return false;
  dev::CompactDesc C;
  memset(&C, 0, sizeof(C));
  int nld = 0;
  for (auto &x : exprs) {
    const DCol &c = rel.cols[x->col];
    const int w = PhysSize(c.phys);
    if (c.validity || (w != 4 && w != 8)) return false;
    C.src[C.nout] = c.data;
    C.ow[C.nout] = w;
    C.nout++;
    nld += w / 4;
  }
  if (nld > 8) return false;
  for (int j = 0; j < F.ncol; j++) {
    if (F.col[j].valid) return false;
    const int w = F.col[j].phys == P_I64 ? 8 : 4;
    int k = -1;
    for (int i = 0; i < C.nout && k < 0; i++)
      if (C.src[i] == F.col[j].data && C.ow[i] == w) k = i;
    if (k < 0) return false;
    C.pred_out[C.npred] = k;
    C.pred_lo[C.npred] = F.col[j].lo;
    C.pred_span[C.npred] = F.col[j].span;
    C.npred++;
  }
  const int64_t n = rel.n;
  const int64_t chunks = dev::CountEntries(n);
  auto counts = Alloc(e, (size_t)(chunks + 1) * 4);
  auto offs = Alloc(e, (size_t)(chunks + 1) * 8);
  double pbytes = 0;
  for (int j = 0; j < F.ncol; j++) pbytes += (double)n * (F.col[j].phys == P_I64 ? 8 : 4);
  {
    ProfScope ps(e, "filter_count", pbytes + (double)(chunks + 1) * 4, n);
    dev::FilterCountChunks(F, n, (uint32_t *)counts->p, e.stream);
  }
  dev::ScanTileCounts((const uint32_t *)counts->p, (int64_t *)offs->p, chunks + 1, e.d_scratch, e.stream);
  const int64_t nsel = ReadDev<int64_t>(e, e.d_scratch);
  out = DRel();
  out.n = nsel;
  std::vector<DCol> cols;
  for (int k = 0; k < (int)exprs.size(); k++) {
    cols.push_back(AllocOut(e, exprs[k]->type, nsel, false));
    C.dst[k] = cols[k].data;
  }
  if (nsel > 0) {
    double bytes = (double)(chunks + 1) * 8;
    for (int k = 0; k < C.nout; k++) bytes += (double)n * C.ow[k] + (double)nsel * C.ow[k];
    ProfScope ps(e, "compact", bytes, n);
    dev::CompactRecompute(C, n, (const int64_t *)offs->p, e.stream);
  }
  out.cols = cols;
  CheckError(e);
  return true;
}

// WHERE <range conjunction over int columns> with plain 1/2/4/8/16-byte output
// columns: two streaming passes (dev::FilterBits, scan, dev::CompactColumns,
// plus dev::CompactValidity per nullable output) instead of vm_filter + scan +
// vm_project.  A NULL in a predicate column fails the row.  MBX_FC=0 disables it.
static bool TryFilterCompact(Engine &e, const DRel &rel, const BExpr &pred, const std::vector<BExprPtr> &exprs,
                             DRel &out) {
  const char *fc = Knob("MBX_FC");
  if ((fc && atoi(fc) == 0) || rel.range || rel.n <= 0 || exprs.empty()) return false;
  std::map<int, std::pair<i128, i128>> ranges;
  if (!RangeConj(pred, ranges) || ranges.empty() || ranges.size() > FM_MAX) return false;
  dev::FilterMultiDesc F;
  memset(&F, 0, sizeof(F));
  F.agg = -1;
  bool empty = false;
  int ninstr = 0;  // LDS-DMA instructions per 256-row step of FilterBits
  for (auto &kv : ranges) {
    const DCol &c = rel.cols[kv.first];
    if (!c.data || (c.phys != P_I32 && c.phys != P_I64)) return false;
    const bool wide = c.phys == P_I64;
    if ((uintptr_t)c.data % 16 || (uintptr_t)c.validity % 16) return false;  // 16-B LDS-DMA lanes
    ninstr += (wide ? 2 : 1) + (c.validity ? 1 : 0);
    dev::FilterMultiCol &fc_ = F.col[F.ncol++];
    fc_.data = c.data;
    fc_.valid = c.validity;
    fc_.phys = c.phys;
    fc_.is_pred = 1;
    const i128 lo = std::max<i128>(kv.second.first, wide ? (i128)INT64_MIN : (i128)INT32_MIN);
    const i128 hi = std::min<i128>(kv.second.second, wide ? (i128)INT64_MAX : (i128)INT32_MAX);
    if (lo > hi) empty = true;
    fc_.lo = (int64_t)lo;
    fc_.span = lo > hi ? 0 : (uint64_t)(int64_t)hi - (uint64_t)(int64_t)lo;
  }
  if (ninstr > 8) return false;
  for (auto &x : exprs) {
    if (x->kind != BExpr::COL || (rel.range && x->col == 0)) return false;
    const DCol &c = rel.cols[x->col];
    if (!c.data || c.phys == P_STR) return false;
    const int w = PhysSize(c.phys);
    if ((w != 1 && w != 2 && w != 4 && w != 8 && w != 16) || (uintptr_t)c.data % 16) return false;
  }
  out = DRel();
  const int64_t n = rel.n;
  if (empty) {  // nothing passes: typed empty columns
    for (auto &x : exprs) out.cols.push_back(AllocOut(e, x->type, 0, rel.cols[x->col].validity != nullptr));
    return true;
  }
  if (TrySelectOnePass(e, rel, F, exprs, out)) return true;
  if (TryCountFirst(e, rel, F, exprs, out)) return true;
  const int64_t steps = (n + 255) / 256;
  auto bits = Alloc(e, (size_t)steps * 32);
  auto offs = Alloc(e, (size_t)(steps + 2) * 8);  // compact reads offsets in 16-B aligned pairs
  double pbytes = 0;
  for (int j = 0; j < F.ncol; j++) pbytes += (double)n * (F.col[j].phys == P_I64 ? 8 : 4) + (F.col[j].valid ? n / 8.0 : 0);
  {
    ProfScope ps(e, "filter_bits", pbytes + (double)steps * 32, n);
    dev::FilterBits(F, n, (unsigned long long *)bits->p, e.stream);
  }
  dev::ScanStepBits((const unsigned long long *)bits->p, (int64_t *)offs->p, steps, e.d_scratch, e.stream);
  const int64_t nsel = ReadDev<int64_t>(e, e.d_scratch);
  out.n = nsel;
  std::vector<DCol> cols;
  for (auto &x : exprs) cols.push_back(AllocOut(e, x->type, nsel, rel.cols[x->col].validity != nullptr));
  if (nsel > 0) {
    // output columns in groups of at most 8 LDS-DMA instructions (8 KiB) per 256-row step
    size_t k = 0;
    while (k < exprs.size()) {
      dev::CompactDesc C;
      memset(&C, 0, sizeof(C));
      int kib = 0;
      double bytes = (double)steps * 40;
      for (; k < exprs.size() && C.nout < FC_MAX_OUT; k++) {
        const DCol &c = rel.cols[exprs[k]->col];
        const int w = PhysSize(c.phys);
        const int cost = (256 * w + 1023) / 1024;
        if (kib + cost > 8) break;
        kib += cost;
        C.src[C.nout] = c.data;
        C.dst[C.nout] = cols[k].data;
        C.ow[C.nout] = w;
        C.nout++;
        bytes += (double)n * w + (double)nsel * w;
      }
      ProfScope ps(e, "compact", bytes, n);
      dev::CompactColumns(C, n, (const unsigned long long *)bits->p, (const int64_t *)offs->p, e.stream);
    }
    for (size_t j = 0; j < exprs.size(); j++) {
      const DCol &c = rel.cols[exprs[j]->col];
      if (!c.validity) continue;
      ProfScope ps(e, "compact_validity", (double)steps * 40 + n / 8.0 + nsel / 8.0, n);
      dev::CompactValidity((const unsigned long long *)bits->p, (const int64_t *)offs->p, n, c.validity,
                           cols[j].validity, e.stream);
    }
  }
  out.cols = cols;
  CheckError(e);
  return true;
}

static dev::EmitAgg EmitFor(const AggSpec &a, VClass in_class, dev::AggState *states, DCol &out) {
  dev::EmitAgg ea;
  memset(&ea, 0, sizeof(ea));
  ea.kind = a.kind;
  ea.in_class = in_class;
  ea.out_phys = PhysOf(a.type);
  ea.avg_scale = a.arg && a.arg->type.id == T_DECIMAL ? a.arg->type.scale : 0;
  ea.states = states;
  ea.out = out.data;
  ea.valid = (uint32_t *)out.validity;
  return ea;
}

static void DropEmptyValidity(Engine &e, DRel &r) {
  // aggregates: keep bitmaps (cheap, tiny relations); nothing to do
  (void)e;
  (void)r;
}

static DRel GatherRel(Engine &e, const DRel &r, const int64_t *perm, int64_t n);

// LDS direct-index reduction (group_direct kernels): rows with an integer key
// in [kmin, kmin + nk) (no NULL keys) and <= 2 integer value columns of one
// physical type without NULLs.  Fills cs (COUNT(*) per key) and s0/s1 (one
// AggState per key for each value column).  maxabs bounds |value| (zone map
// or a device min/max pass); false = the shape does not fit.
struct DirectStates {
  DevBufPtr cs, s0, s1;
};
static bool DirectReduce(Engine &e, const void *kdata, Phys kphys, int64_t kmin, int64_t nk, int64_t n,
                         const std::vector<const DCol *> &vals, i128 maxabs, bool mm, DirectStates &out) {
  const int nv = (int)vals.size();
  if (nk < 1 || nk > 1024 || nv > 2 || n <= 0) return false;
  if (kphys != P_I32 && kphys != P_I64) return false;
  for (auto *v : vals)
    if ((v->phys != P_I32 && v->phys != P_I64) || v->validity || v->phys != vals[0]->phys) return false;
  int R = 64;
  while (R > 1 && dev::GroupDirectLds((int)nk, R, nv, mm) > 48 * 1024) R >>= 1;
  if (dev::GroupDirectLds((int)nk, R, nv, mm) > 64 * 1024) return false;
  int64_t seg = 0;  // whole chunk
  if (maxabs > 0) {
    i128 per_rep = ((i128)1 << 62) / maxabs;  // rows one replica may absorb
    i128 seg128 = per_rep * R;
    if (seg128 < 4096) return false;
    if (seg128 < (i128)INT64_MAX / 2) seg = (int64_t)seg128;
  }
  if ((int64_t)R * ((int64_t)1 << 31) < seg || seg == 0) {
    // u32 replica counts: cap segment length
    int64_t cap = (int64_t)R * ((int64_t)1 << 30);
    if (seg == 0 || seg > cap) seg = cap;
  }
  size_t st_bytes = (size_t)nk * sizeof(dev::AggState);
  out.cs = Alloc(e, nk * 8, true);
  out.s0 = Alloc(e, st_bytes);
  out.s1 = Alloc(e, st_bytes);
  dev::InitAggStates((dev::AggState *)out.s0->p, nk, e.stream);
  dev::InitAggStates((dev::AggState *)out.s1->p, nk, e.stream);
  const Phys vphys = nv ? vals[0]->phys : P_I64;
  double bytes = (double)n * PhysSize(kphys);
  for (auto *v : vals) bytes += (double)n * PhysSize(v->phys);
  ProfScope ps(e, "group_direct", bytes, n);
  dev::GroupByDirectStates(kdata, kphys, kmin, (int)nk, nv > 0 ? vals[0]->data : nullptr,
                           nv > 1 ? vals[1]->data : nullptr, vphys, nv, mm, n, seg, R,
                           (unsigned long long *)out.cs->p, (dev::AggState *)out.s0->p, (dev::AggState *)out.s1->p, 0,
                           e.stream, nullptr, maxabs < ((i128)1 << 62) ? (uint64_t)maxabs : ~0ull);
  return true;
}

// max |x| over an integer column without NULLs (one device min/max pass)
static i128 DeviceMaxAbs(Engine &e, const DCol &c, int64_t n) {
  long long *o3 = (long long *)((char *)e.d_small + 3072);
  dev::KeyRange(c.data, c.phys, c.validity, n, o3, e.stream);
  long long h[3];
  HIPCHK(hipMemcpyAsync(h, o3, sizeof(h), hipMemcpyDeviceToHost, e.stream));
  HIPCHK(hipStreamSynchronize(e.stream));
  if (!h[2]) return 0;
  i128 a = h[0] < 0 ? -(i128)h[0] : (i128)h[0], b = h[1] < 0 ? -(i128)h[1] : (i128)h[1];
  return a > b ? a : b;
}

// Value columns of the generic aggregate paths reduced through DirectReduce
// in pairs; states_of[j] = AggState array of aggregate j (nullptr for
// COUNT(*)), count_star = the per-key COUNT(*).  false: not applicable.
static bool DirectReduceAll(Engine &e, const void *kdata, Phys kphys, int64_t kmin, int64_t nk, int64_t n,
                            const DRel &tmp, const BoundSelect &s, const std::vector<int> &arg_idx,
                            std::vector<DevBufPtr> &keep, std::vector<dev::AggState *> &states_of,
                            const unsigned long long **count_star) {
  const int na = (int)s.aggs.size();
  std::vector<int> cols;
  bool mm = false;
  for (int j = 0; j < na; j++) {
    if (arg_idx[j] < 0) continue;
    if (s.aggs[j].distinct) return false;
    const DCol &c = tmp.cols[arg_idx[j]];
    if ((c.phys != P_I32 && c.phys != P_I64) || c.validity || ClassOf(c.type) != VC_I64) return false;
    if (s.aggs[j].kind == A_MIN || s.aggs[j].kind == A_MAX) mm = true;
    if (std::find(cols.begin(), cols.end(), arg_idx[j]) == cols.end()) cols.push_back(arg_idx[j]);
  }
  // pairs of one physical type
  std::vector<std::vector<int>> groups;
  for (Phys ph : {P_I32, P_I64}) {
    std::vector<int> g;
    for (int c : cols)
      if (tmp.cols[c].phys == ph) g.push_back(c);
    for (size_t i = 0; i < g.size(); i += 2)
      groups.push_back(std::vector<int>(g.begin() + i, g.begin() + std::min(g.size(), i + 2)));
  }
  if (groups.empty()) groups.push_back({});
  states_of.assign(na, nullptr);
  *count_star = nullptr;
  for (auto &g : groups) {
    std::vector<const DCol *> vals;
    i128 maxabs = 0;
    for (int c : g) {
      vals.push_back(&tmp.cols[c]);
      maxabs = std::max(maxabs, DeviceMaxAbs(e, tmp.cols[c], n));
    }
    DirectStates ds;
    if (!DirectReduce(e, kdata, kphys, kmin, nk, n, vals, maxabs, mm, ds)) return false;
    keep.push_back(ds.cs);
    keep.push_back(ds.s0);
    keep.push_back(ds.s1);
    if (!*count_star) *count_star = (const unsigned long long *)ds.cs->p;
    for (int j = 0; j < na; j++) {
      if (arg_idx[j] < 0) continue;
      if (!g.empty() && arg_idx[j] == g[0]) states_of[j] = (dev::AggState *)ds.s0->p;
      if (g.size() > 1 && arg_idx[j] == g[1]) states_of[j] = (dev::AggState *)ds.s1->p;
    }
  }
  return true;
}

// GROUP BY through the device hash table (HashGroupAssign): works for any
// number of keys of any fixed-width or VARCHAR type.  Keys are emitted by
// gathering each group's representative row; groups come out in table
// order (DuckDB's hash aggregate has no defined order either).
static DRel HashAggregate(Engine &e, const DRel &tmp, const BoundSelect &s, const std::vector<int> &arg_idx) {
  const int ng = (int)s.groups.size();
  const int na = (int)s.aggs.size();
  if (ng > HASH_MAX_KEYS) ThrowError("Not implemented", "GROUP BY with more than 8 keys");
  dev::HashKeys hk;
  memset(&hk, 0, sizeof(hk));
  hk.nk = ng;
  for (int g = 0; g < ng; g++) {
    const DCol &c = tmp.cols[g];
    if (c.phys == P_INTERVAL) ThrowError("Not implemented", "GROUP BY on INTERVAL keys is not supported on device");
    if (c.phys == P_STR && (!c.offsets || !c.chars))
      ThrowError("Internal", "GROUP BY VARCHAR key without materialised strings");
    hk.k[g] = dev::HashKeyCol{c.data, c.validity, c.offsets, c.chars, (int32_t)c.phys};
  }
  const int64_t n = tmp.n;
  // a table of >= 2n entries, at most 2^30 (its scan counts in int32: a 2^31-entry
  // table silently lost every group above 5.4e8 rows); at most one entry per
  // row is ever claimed, so n <= 2^30 rows always fit
  int64_t cap = 1024;
  while (cap < 2 * n && cap < ((int64_t)1 << 30)) cap <<= 1;
  if (n > ((int64_t)1 << 30)) ThrowError("Not implemented", "GROUP BY input above 2^30 rows on the hash path");
  auto table = Alloc(e, (size_t)cap * 8);
  HIPCHK(hipMemsetAsync(table->p, 0xFF, (size_t)cap * 8, e.stream));
  auto slot_of = Alloc(e, (size_t)std::max<int64_t>(n, 1) * 4);
  auto gid = Alloc(e, (size_t)cap * 4);
  auto rep = Alloc(e, (size_t)std::max<int64_t>(n, 1) * 8);
  {
    double kb = 0;
    for (int g = 0; g < ng; g++) kb += (double)n * (tmp.cols[g].phys == P_STR ? 16 : PhysSize(tmp.cols[g].phys));
    ProfScope ps(e, "hash_group_assign", kb, n);
    dev::HashGroupAssign(hk, n, (unsigned long long *)table->p, cap, (int32_t *)slot_of->p, (int32_t *)gid->p,
                         (int64_t *)rep->p, nullptr, e.d_scratch, e.d_err, e.stream);
  }
  const int64_t ngroups = ReadDev<int64_t>(e, e.d_scratch);
  CheckError(e);
  table.reset();
  gid.reset();
  std::vector<DevBufPtr> states(na);
  std::vector<DevBufPtr> keep;
  std::vector<dev::AggState *> st_of(na, nullptr);
  const unsigned long long *cstar = nullptr;
  DevBufPtr cs;
  // few groups: LDS-privatised reduction keyed by the dense group id
  bool lds = ngroups >= 1 && ngroups <= 1024 &&
             DirectReduceAll(e, slot_of->p, P_I32, 0, ngroups, n, tmp, s, arg_idx, keep, st_of, &cstar);
  if (!lds) {
    cs = Alloc(e, (size_t)std::max<int64_t>(ngroups, 1) * 8, true);
    dev::CountSlots((const int32_t *)slot_of->p, n, (unsigned long long *)cs->p, e.stream);
    cstar = (const unsigned long long *)cs->p;
  }
  for (int j = 0; j < na && !lds; j++) {
    if (arg_idx[j] < 0) continue;
    const DCol &c = tmp.cols[arg_idx[j]];
    const void *data = c.data;
    int phys = c.phys;
    if (c.phys == P_STR) {
      if (s.aggs[j].kind != A_COUNT)
        ThrowError("Not implemented", "SUM/MIN/MAX/AVG over VARCHAR are not supported on device");
      data = c.offsets;
      phys = P_I64;
    }
    states[j] = Alloc(e, (size_t)std::max<int64_t>(ngroups, 1) * sizeof(dev::AggState));
    dev::InitAggStates((dev::AggState *)states[j]->p, ngroups, e.stream);
    ProfScope ps(e, "group_reduce", (double)n * (PhysSize((Phys)phys) + 4), n);
    dev::GroupReduceColumn((const int32_t *)slot_of->p, data, phys, c.validity, n, (dev::AggState *)states[j]->p,
                           e.stream);
    st_of[j] = (dev::AggState *)states[j]->p;
  }
  DRel keys;
  keys.n = n;
  for (int g = 0; g < ng; g++) keys.cols.push_back(tmp.cols[g]);
  DRel out = GatherRel(e, keys, (const int64_t *)rep->p, ngroups);
  for (int g = 0; g < ng; g++) out.cols[g].type = s.groups[g]->type;
  dev::EmitDesc D;
  memset(&D, 0, sizeof(D));
  D.nagg = na;
  D.cstar = cstar;
  D.nslots = ngroups;
  D.null_slot = -1;
  for (int j = 0; j < na; j++) {
    DCol oc = AllocOut(e, s.aggs[j].type, ngroups, true, false);
    VClass ic = arg_idx[j] >= 0 ? ClassOf(tmp.cols[arg_idx[j]].type) : VC_I64;
    D.a[j] = EmitFor(s.aggs[j], ic, st_of[j], oc);
    out.cols.push_back(oc);
  }
  if (ngroups > 0) dev::EmitAggRelation(D, e.stream);
  HIPCHK(hipStreamSynchronize(e.stream));
  out.n = ngroups;
  return out;
}

// F1m: no GROUP BY, a conjunction of range predicates over >= 2 int columns
// (or one predicate column of another width than the aggregated column),
// aggregates over one int column or COUNT(*): one LDS-DMA pass over all the
// columns (filter_multi_lds).  The single-column shape stays on F1.
// NULL-able columns take this kernel too (their validity words ride the ring):
// a NULL fails a predicate; a NULL-able aggregated column that carries no
// predicate is admitted only without COUNT(*), so that "every NULL-able column
// valid" is exactly the set of rows each aggregate sees.
static bool FmIntCol(const DRel &rel, int c) {
  if (rel.range && c == 0) return false;
  const DCol &d = rel.cols[c];
  return d.data && (d.phys == P_I32 || d.phys == P_I64) && (uintptr_t)d.data % 16 == 0 &&
         (uintptr_t)d.validity % 16 == 0;
}

static bool FilterMultiAggregate(Engine &e, const DRel &src, const BoundSelect &s, DRel &out) {
  if (!s.where || src.n <= 0) return false;
  std::map<int, std::pair<i128, i128>> ranges;
  if (!RangeConj(*s.where, ranges)) return false;
  int acol = -1;
  bool need_mm = false, count_star = false;
  for (auto &a : s.aggs) {
    if (a.kind == A_COUNT_STAR) {
      count_star = true;
      continue;
    }
    if (a.distinct) return false;
    const BExpr *x = a.arg ? StripWidening(a.arg.get()) : nullptr;
    if (!x || x->kind != BExpr::COL || !FmIntCol(src, x->col)) return false;
    if (a.arg->type.id == T_DOUBLE || a.arg->type.id == T_FLOAT) return false;
    if (acol >= 0 && acol != x->col) return false;
    acol = x->col;
    need_mm |= a.kind == A_MIN || a.kind == A_MAX;
  }
  bool nullable = false;
  int ninstr = 0;
  for (auto &kv : ranges) {
    if (!FmIntCol(src, kv.first)) return false;
    nullable |= src.cols[kv.first].validity != nullptr;
    ninstr += (src.cols[kv.first].phys == P_I64 ? 2 : 1) + (src.cols[kv.first].validity ? 1 : 0);
  }
  if (acol >= 0 && !ranges.count(acol)) {
    if (src.cols[acol].validity && count_star) return false;
    nullable |= src.cols[acol].validity != nullptr;
    ninstr += (src.cols[acol].phys == P_I64 ? 2 : 1) + (src.cols[acol].validity ? 1 : 0);
  }
  if (ninstr > 8) return false;
  const bool single = ranges.size() == 1 && (acol < 0 || acol == ranges.begin()->first ||
                                             src.cols[acol].phys == src.cols[ranges.begin()->first].phys);
  if (single && !nullable) return false;  // F1 proper
  dev::FilterMultiDesc d;
  memset(&d, 0, sizeof(d));
  d.agg = -1;
  double bytes = 0;
  for (auto &kv : ranges) {
    if (d.ncol == FM_MAX) return false;
    i128 lo = std::max<i128>(kv.second.first, INT64_MIN), hi = std::min<i128>(kv.second.second, INT64_MAX);
    dev::FilterMultiCol &c = d.col[d.ncol];
    c.data = src.cols[kv.first].data;
    c.phys = src.cols[kv.first].phys;
    c.valid = src.cols[kv.first].validity;
    c.is_pred = 1;
    if (lo > hi) return false;  // an empty range: the generic path answers it
    c.lo = (int64_t)lo;
    c.span = (uint64_t)(int64_t)hi - (uint64_t)(int64_t)lo;
    if (kv.first == acol) d.agg = d.ncol;
    bytes += (double)src.n * PhysSize(src.cols[kv.first].phys) + (c.valid ? src.n / 8.0 : 0);
    d.ncol++;
  }
  if (acol >= 0 && d.agg < 0) {
    if (d.ncol == FM_MAX) return false;
    dev::FilterMultiCol &c = d.col[d.ncol];
    c.data = src.cols[acol].data;
    c.phys = src.cols[acol].phys;
    c.valid = src.cols[acol].validity;
    c.is_pred = 0;
    d.agg = d.ncol++;
    bytes += (double)src.n * PhysSize(src.cols[acol].phys) + (c.valid ? src.n / 8.0 : 0);
  }
  d.mm = need_mm;
  uint64_t maxabs = ~0ull;
  if (acol >= 0 && src.cols[acol].table_col && src.cols[acol].table_col->stats_valid) {
    const DevColumn *tc = src.cols[acol].table_col;
    i128 m1 = tc->imin < 0 ? -tc->imin : tc->imin, m2 = tc->imax < 0 ? -tc->imax : tc->imax;
    i128 m = m1 > m2 ? m1 : m2;
    if (m <= (i128)INT64_MAX) maxabs = (uint64_t)m;
  }
  d.maxabs = maxabs;  // FilterMultiPartials decides the int64-partial (narrow) mode from it
  const int na = (int)s.aggs.size();
  dev::AggState *st = (dev::AggState *)e.d_small;
  unsigned long long *cstar = (unsigned long long *)((char *)e.d_small + 1024);
  int npartials;
  {
    ProfScope ps(e, "filter_multi", bytes, src.n);
    npartials = dev::FilterMultiPartials(d, src.n, e.d_partials, e.stream);
  }
  out.n = 1;
  dev::EmitDesc D;
  memset(&D, 0, sizeof(D));
  D.nagg = na;
  D.cstar = cstar;
  D.nslots = 1;
  D.null_slot = -1;
  D.partials = e.d_partials;
  D.npartials = npartials;
  for (int j = 0; j < na; j++) {
    DCol oc = AllocOut(e, s.aggs[j].type, 1, true, false);
    D.a[j] = EmitFor(s.aggs[j], VC_I64, s.aggs[j].kind == A_COUNT_STAR ? nullptr : st, oc);
    out.cols.push_back(oc);
  }
  dev::EmitAggRelation(D, e.stream);
  return true;
}

// Run-time specialised scan -> filter -> project -> aggregate (no GROUP BY):
// one kernel evaluates the WHERE program and every aggregate argument and
// accumulates in registers (jit::VmAggregate); nothing is materialised.  false
// while the kernel is still compiling, or for shapes it does not take
// (DISTINCT, VARCHAR arguments, MIN/MAX of 128-bit values).
static bool JitAggregate(Engine &e, const DRel &src, const BoundSelect &s, DRel &out) {
  const int na = (int)s.aggs.size();
  if (na > VM_MAX_OUT || src.n <= 0) return false;
  VmCompiler vc(src, nullptr);
  try {
    vc.P.pred_reg = 255;
    if (s.where) vc.P.pred_reg = (uint8_t)vc.Compile(*s.where);
    for (int j = 0; j < na; j++) {
      const AggSpec &a = s.aggs[j];
      if (a.distinct) return false;
      if (a.kind == A_COUNT_STAR) {
        vc.P.out_reg[j] = 255;
        continue;
      }
      VClass c = ClassOf(a.arg->type);
      if (c == VC_STR) return false;
      if (c == VC_I128 && (a.kind == A_MIN || a.kind == A_MAX)) return false;
      vc.P.out_reg[j] = (uint8_t)vc.Compile(*a.arg);
      vc.P.out_class[j] = (uint8_t)c;
      // statistics the kernel accumulates: bit0 sum (SUM/AVG), bit1 min/max; COUNT only counts
      vc.P.out_phys[j] = a.kind == A_SUM || a.kind == A_AVG ? 1 : a.kind == A_MIN || a.kind == A_MAX ? 2 : 4;
    }
  } catch (std::exception &) {
    return false;  // the VM path raises the same error if it applies
  }
  vc.P.n_out = na;
  vc.P.n_regs = vc.high;
  auto states = Alloc(e, (size_t)std::max(na, 1) * sizeof(dev::AggState));
  dev::InitAggStates((dev::AggState *)states->p, std::max(na, 1), e.stream);
  auto cs = Alloc(e, 8, true);
  bool ok;
  {
    ProfScope ps(e, "jit_aggregate", 0, src.n);
    ok = jit::VmAggregate(vc.P, vc.cols, src.n, src.rs, src.rstep, states->p, (unsigned long long *)cs->p, e.d_err,
                          e.stream);
  }
  if (!ok) return false;
  out.n = 1;
  dev::EmitDesc D;
  memset(&D, 0, sizeof(D));
  D.nagg = na;
  D.cstar = (const unsigned long long *)cs->p;
  D.nslots = 1;
  D.null_slot = -1;
  for (int j = 0; j < na; j++) {
    DCol oc = AllocOut(e, s.aggs[j].type, 1, true, false);
    VClass ic = s.aggs[j].kind == A_COUNT_STAR ? VC_I64 : ClassOf(s.aggs[j].arg->type);
    D.a[j] = EmitFor(s.aggs[j], ic, (dev::AggState *)states->p + j, oc);
    out.cols.push_back(oc);
  }
  dev::EmitAggRelation(D, e.stream);
  HIPCHK(hipStreamSynchronize(e.stream));  // states / count buffers released after the emit
  return true;
}

// Fused GROUP BY (jit::VmGroupAggregate): up to JIT_MAX_KEYS integer key
// columns whose statistics bound a composite slot table of <= 4096 slots,
// any WHERE program, integer aggregate arguments of any expression.  One
// pass over the columns; nothing is materialised.  Groups come out in key
// order (NULL keys last), like the direct-index path.
static bool JitGroupAggregate(Engine &e, const DRel &src, const BoundSelect &s, DRel &out) {
  const int ng = (int)s.groups.size(), na = (int)s.aggs.size();
  if (ng < 1 || ng > JIT_MAX_KEYS || ng > EMIT_MAX_CKEYS || na > VM_MAX_OUT || src.n <= 0 || src.range) return false;
  jit::GroupSpec g;
  memset(&g, 0, sizeof(g));
  g.nkeys = ng;
  i128 nslots = 1;
  for (int i = 0; i < ng; i++) {
    const BExpr *x = StripWidening(s.groups[i].get());
    if (x->kind != BExpr::COL || ClassOf(s.groups[i]->type) != VC_I64) return false;
    const DCol &c = src.cols[x->col];
    if (!c.table_col || !c.table_col->stats_valid || c.table_col->data != c.data) return false;
    if (c.phys != P_I8 && c.phys != P_I16 && c.phys != P_I32 && c.phys != P_I64 && c.phys != P_U8 &&
        c.phys != P_U16 && c.phys != P_U32)
      return false;
    const Phys kp = PhysOf(s.groups[i]->type);
    if (kp == P_STR || kp == P_F32 || kp == P_F64 || kp == P_I128 || kp == P_INTERVAL || kp == P_U64) return false;
    const i128 range = c.table_col->imax - c.table_col->imin + 1;
    if (range < 1 || range > 4096) return false;
    g.key_nullable[i] = c.validity != nullptr;
    g.kmin[i] = (int64_t)c.table_col->imin;
    g.radix[i] = (int64_t)range + (g.key_nullable[i] ? 1 : 0);
    nslots *= g.radix[i];
    if (nslots > 4096) return false;
  }
  g.nslots = (int32_t)nslots;
  int64_t stride = 1;
  for (int i = ng - 1; i >= 0; i--) {
    g.stride[i] = stride;
    stride *= g.radix[i];
  }
  VmCompiler vc(src, nullptr);
  try {
    vc.P.pred_reg = 255;
    if (s.where) vc.P.pred_reg = (uint8_t)vc.Compile(*s.where);
    for (int i = 0; i < ng; i++) g.key_reg[i] = (uint8_t)vc.Compile(*s.groups[i]);
    for (int j = 0; j < na; j++) {
      const AggSpec &a = s.aggs[j];
      if (a.distinct) return false;
      if (a.kind == A_COUNT_STAR) {
        vc.P.out_reg[j] = 255;
        continue;
      }
      if (ClassOf(a.arg->type) != VC_I64) return false;
      vc.P.out_reg[j] = (uint8_t)vc.Compile(*a.arg);
      vc.P.out_class[j] = (uint8_t)VC_I64;
      vc.P.out_phys[j] = a.kind == A_SUM || a.kind == A_AVG ? 1 : a.kind == A_MIN || a.kind == A_MAX ? 2 : 4;
    }
  } catch (std::exception &) {
    return false;  // the VM path raises the same error if it applies
  }
  vc.P.n_out = na;
  vc.P.n_regs = vc.high;
  const int64_t ns = g.nslots;
  auto states = Alloc(e, (size_t)std::max(na, 1) * ns * sizeof(dev::AggState));
  dev::InitAggStates((dev::AggState *)states->p, std::max(na, 1) * ns, e.stream);
  auto cs = Alloc(e, (size_t)ns * 8, true);
  bool ok;
  {
    ProfScope ps(e, "jit_group", 0, src.n);
    ok = jit::VmGroupAggregate(vc.P, vc.cols, g, src.n, src.rs, src.rstep, states->p, (unsigned long long *)cs->p,
                               e.d_err, e.stream);
  }
  if (!ok) return false;
  auto list = Alloc(e, (size_t)ns * 4);
  dev::CompactSlots((const unsigned long long *)cs->p, ns, (int32_t *)list->p, e.d_scratch, e.stream);
  const int64_t ngroups = ReadDev<int64_t>(e, e.d_scratch);
  CheckError(e);
  dev::EmitDesc D;
  memset(&D, 0, sizeof(D));
  D.nagg = na;
  D.cstar = (const unsigned long long *)cs->p;
  D.slot_list = (const int32_t *)list->p;
  D.n_list = e.d_scratch;
  D.nslots = ngroups;
  D.null_slot = -1;
  D.nkeys_c = ng;
  out.n = ngroups;
  for (int i = 0; i < ng; i++) {
    DCol kc = AllocOut(e, s.groups[i]->type, ngroups, true, false);
    D.kc[i].out = kc.data;
    D.kc[i].valid = (uint32_t *)kc.validity;
    D.kc[i].phys = PhysOf(s.groups[i]->type);
    D.kc[i].nullable = g.key_nullable[i];
    D.kc[i].kmin = g.kmin[i];
    D.kc[i].radix = g.radix[i];
    D.kc[i].stride = g.stride[i];
    out.cols.push_back(kc);
  }
  for (int j = 0; j < na; j++) {
    DCol oc = AllocOut(e, s.aggs[j].type, ngroups, true, false);
    dev::AggState *st = s.aggs[j].kind == A_COUNT_STAR ? nullptr : (dev::AggState *)states->p + (size_t)j * ns;
    D.a[j] = EmitFor(s.aggs[j], VC_I64, st, oc);
    out.cols.push_back(oc);
  }
  if (ngroups > 0) dev::EmitAggRelation(D, e.stream);
  HIPCHK(hipStreamSynchronize(e.stream));  // state buffers released after the emit
  DropEmptyValidity(e, out);
  return true;
}

static ResultPtr ToHost(Engine &e, const DRel &r, const std::vector<std::string> &names, int64_t offset, int64_t limit,
                        size_t ncols, bool text = false);
static void KeyBytes(const Value &v, std::string &out);
static DRel Aggregate(Engine &e, const DRel &src, const BoundSelect &s);

// COUNT(DISTINCT arg) (the binder keeps DISTINCT only on COUNT; MIN/MAX
// DISTINCT are plain MIN/MAX).  Per distinct aggregate, two device
// aggregations: the distinct (groups..., arg) pairs of the filtered source (a
// GROUP BY with no aggregates of its own), then COUNT(arg) of those pairs per
// group (a NULL arg is one pair and is not counted).  The other aggregates
// come from one pass with COUNT(arg) in the distinct ones' places; the
// per-group distinct counts (one row per group) are merged into that relation
// on the host by group key (KeyBytes, as the sharded combine does) and the
// relation is uploaded back in the main pass's group order.  This merge is a
// host slow path: it costs a D2H of the main relation and of every distinct
// count, O(groups log groups) host work and an upload, so a high-cardinality
// GROUP BY with COUNT(DISTINCT) is bound by the host (and a sharded table
// gathers its parts first); it is off the measured hot path.
static DRel DistinctAggregate(Engine &e, const DRel &src, const BoundSelect &s) {
  const int ng = (int)s.groups.size(), na = (int)s.aggs.size();
  BoundSelect m = s;
  for (auto &a : m.aggs) a.distinct = false;
  const DRel main = Aggregate(e, src, m);
  std::vector<std::string> names(ng + na, "");
  const ResultPtr mh = ToHost(e, main, names, 0, -1, (size_t)(ng + na));
  std::vector<std::vector<Value>> rows((size_t)mh->nrows);
  std::vector<std::string> keys((size_t)mh->nrows);
  std::map<std::string, size_t> at;
  for (int64_t r = 0; r < mh->nrows; r++) {
    for (int c = 0; c < ng + na; c++) rows[r].push_back(mh->cols[c].Get(r));
    for (int c = 0; c < ng; c++) KeyBytes(rows[r][c], keys[r]);
    at[keys[r]] = (size_t)r;
  }
  for (int j = 0; j < na; j++) {
    if (!s.aggs[j].distinct) continue;
    BoundSelect p;
    p.where = s.where;
    p.is_agg = true;
    p.groups = s.groups;
    p.groups.push_back(s.aggs[j].arg);
    AggSpec cs;
    cs.kind = A_COUNT_STAR;
    cs.type = LogicalType(T_BIGINT);
    p.aggs.push_back(cs);
    const DRel pairs = Aggregate(e, src, p);  // [groups..., arg, COUNT(*)]
    BoundSelect q;
    q.is_agg = true;
    for (int c = 0; c <= ng; c++) {
      auto col = std::make_shared<BExpr>();
      col->kind = BExpr::COL;
      col->col = c;
      col->type = c < ng ? s.groups[c]->type : s.aggs[j].arg->type;
      if (c < ng) q.groups.push_back(col);
      else {
        AggSpec cnt;
        cnt.kind = A_COUNT;
        cnt.arg = col;
        cnt.type = LogicalType(T_BIGINT);
        q.aggs.push_back(cnt);
      }
    }
    const DRel per = Aggregate(e, pairs, q);  // [groups..., COUNT(DISTINCT arg)]
    std::vector<std::string> pn(ng + 1, "");
    const ResultPtr ph = ToHost(e, per, pn, 0, -1, (size_t)(ng + 1));
    for (auto &row : rows) row[ng + j] = Value::Int(T_BIGINT, 0);  // groups whose args are all NULL
    for (int64_t r = 0; r < ph->nrows; r++) {
      std::string kb;
      for (int c = 0; c < ng; c++) KeyBytes(ph->cols[c].Get(r), kb);
      auto it = at.find(kb);
      if (it != at.end()) rows[it->second][ng + j] = Value::Int(T_BIGINT, (int64_t)ph->cols[ng].Get(r).i);
    }
  }
  std::vector<LogicalType> types;
  for (auto &g : s.groups) types.push_back(g->type);
  for (auto &a : s.aggs) types.push_back(a.type);
  return UploadRows(e, rows, types);
}

// The top-level SELECT of ExecuteSelect whose relation goes to the host
// unchanged (no HAVING, ORDER BY, LIMIT / OFFSET or UNION; every output a
// column of the aggregate): its GROUP BY may leave the group count on the
// device, so the rows and the count come back in one copy (DRel::n_dev).
static bool CountMayStayOnDevice(const Engine &e, const BoundSelect &s) {
  if (e.defer_count_for != (const void *)&s || s.having || !s.union_all.empty() || !s.order.empty() ||
      s.limit >= 0 || s.offset > 0)
    return false;
  for (auto &x : s.outputs)
    if (x->kind != BExpr::COL) return false;
  return true;
}

// ---- the partitioned GROUP BY (group_part.hip): F3 (dense), F3h (hashed), and
// both over the group code of composite / NULL-able keys.  The shared parts:
// The value columns of the shape: COUNT / SUM / MIN / MAX / AVG over <= 2
// integer columns of one phys without NULLs, zone maps bounding |v| < 2^62.
struct PartGroupValues {
  std::vector<int> vcols;
  bool mm = false;
  i128 maxabs = 0;
};
static bool PartGroupValueCols(const DRel &src, const BoundSelect &s, PartGroupValues &v) {
  for (auto &a : s.aggs) {
    if (a.kind == A_COUNT_STAR) continue;
    if (a.distinct) return false;
    const BExpr *x = a.arg ? StripWidening(a.arg.get()) : nullptr;
    if (!x || x->kind != BExpr::COL || !FastIntCol(src, x->col) || a.arg->type.id == T_DOUBLE ||
        a.arg->type.id == T_FLOAT)
      return false;
    if (a.kind == A_MIN || a.kind == A_MAX) v.mm = true;
    if (std::find(v.vcols.begin(), v.vcols.end(), x->col) == v.vcols.end()) v.vcols.push_back(x->col);
  }
  const int nv = (int)v.vcols.size();
  if (nv > 2 || (nv == 2 && src.cols[v.vcols[0]].phys != src.cols[v.vcols[1]].phys)) return false;
  for (int c : v.vcols) {
    const DevColumn *vs = src.cols[c].table_col;
    if (!vs || !vs->stats_valid) return false;
    v.maxabs = std::max(v.maxabs, std::max(vs->imax < 0 ? -vs->imax : vs->imax, vs->imin < 0 ? -vs->imin : vs->imin));
  }
  return v.maxabs < ((i128)1 << 62);
}

// The run's buffers (count and states per slot, the hashed tables' keys, the
// passes' scratch) and its descriptor, all but the key fields.
struct PartGroupRun {
  DevBufPtr cs, stb, gk, hist, startb, rows, scan;
  dev::PartGroupDesc d;
  int64_t nslots = 0;
};
static void PartGroupPrepare(Engine &e, const DRel &src, const PartGroupValues &v, int64_t dense_range,
                             PartGroupRun &r) {
  const int nv = (int)v.vcols.size();
  const bool hashed = dense_range <= 0;
  const Phys vphys = nv ? src.cols[v.vcols[0]].phys : P_I64;
  r.nslots = hashed ? dev::PartGroupHashedSlots() : dense_range;
  size_t hb = 0, sb = 0, rb = 0, cb = 0;
  if (hashed) dev::PartGroupHashedScratch(src.n, nv, &hb, &sb, &rb, &cb);
  else dev::PartGroupScratch(src.n, r.nslots, nv, v.mm, vphys, &hb, &sb, &rb, &cb);
  r.cs = Alloc(e, r.nslots * 8);
  r.stb = Alloc(e, (size_t)(nv >= 2 ? 2 : 1) * r.nslots * sizeof(dev::AggState));
  if (hashed) r.gk = Alloc(e, r.nslots * 8);
  r.hist = Alloc(e, hb), r.startb = Alloc(e, sb), r.rows = Alloc(e, rb), r.scan = Alloc(e, cb);
  dev::PartGroupDesc &d = r.d;
  memset(&d, 0, sizeof(d));
  d.v0 = nv > 0 ? src.cols[v.vcols[0]].data : nullptr;
  d.v1 = nv > 1 ? src.cols[v.vcols[1]].data : nullptr;
  d.vphys = vphys;
  d.nv = nv;
  d.mm = v.mm;
  d.n = src.n;
  d.vmaxabs = nv ? (uint64_t)std::max<i128>(v.maxabs, 1) : 0;
  d.cstar = (unsigned long long *)r.cs->p;
  d.st0 = (dev::AggState *)r.stb->p;
  d.scratch_hist = r.hist->p, d.scratch_start = r.startb->p, d.scratch_rows = r.rows->p, d.scratch_scan = r.scan->p;
  d.scratch_scan_bytes = cb;
}

// algorithmic bytes of the value columns
static double PartGroupValueBytes(const DRel &src, const PartGroupValues &v) {
  double bytes = 0;
  for (int c : v.vcols) bytes += (double)src.n * PhysSize(src.cols[c].phys);
  return bytes;
}

// The non-empty slots compacted and emitted; D carries the key fields and
// out.cols the key columns (each allocated for r.nslots rows).  The count stays
// on the device where the statement allows (CountMayStayOnDevice).
static void PartGroupEmit(Engine &e, const BoundSelect &s, const PartGroupValues &v, const PartGroupRun &r,
                          dev::EmitDesc &D, DRel &out) {
  const int na = (int)s.aggs.size();
  const int64_t nslots = r.nslots;
  auto list = Alloc(e, nslots * 4);
  const bool defer = CountMayStayOnDevice(e, s);
  DevBufPtr nbuf = defer ? Alloc(e, 8) : nullptr;
  int64_t *const n_out = defer ? (int64_t *)nbuf->p : e.d_scratch;
  dev::CompactSlots((const unsigned long long *)r.cs->p, nslots, (int32_t *)list->p, n_out, e.stream);
  D.nagg = na;
  D.cstar = (const unsigned long long *)r.cs->p;
  D.slot_list = (const int32_t *)list->p;
  D.n_list = n_out;
  D.nslots = nslots;
  D.null_slot = -1;
  for (int j = 0; j < na; j++) {
    DCol oc = AllocOut(e, s.aggs[j].type, nslots, true, false);
    dev::AggState *stp = nullptr;
    if (s.aggs[j].kind != A_COUNT_STAR)
      stp = StripWidening(s.aggs[j].arg.get())->col == v.vcols[0] ? r.d.st0 : r.d.st0 + nslots;
    D.a[j] = EmitFor(s.aggs[j], VC_I64, stp, oc);
    out.cols.push_back(oc);
  }
  dev::EmitAggRelation(D, e.stream);
  if (defer) {
    out.n = nslots;  // the columns hold every slot; the count follows the rows to the host
    out.n_dev = n_out;
    out.n_owner = nbuf;
  } else {
    out.n = ReadDev<int64_t>(e, n_out);
  }
}

// The hashed passes over r.d (its key fields set); false: the launch was
// refused or a table filled up (more groups than the tables hold) -- the
// caller's hash path answers.
static bool PartGroupHashedRun(Engine &e, const DRel &src, PartGroupRun &r, double bytes) {
  int32_t *ovf = (int32_t *)((char *)e.d_small + 3584);
  {
    ProfScope ps(e, "group_part_hashed", bytes, src.n);
    if (!dev::PartGroupHashed(r.d, (unsigned long long *)r.gk->p, ovf, e.stream)) {
      if (Knob("MBX_PG_DEBUG")) fprintf(stderr, "[mbx] F3h: launch refused\n");
      return false;
    }
  }
  if (const int32_t o = ReadDev<int32_t>(e, ovf)) {  // more groups than the tables hold
    if (Knob("MBX_PG_DEBUG")) fprintf(stderr, "[mbx] F3h: table overflow flag %d\n", o);
    return false;
  }
  return true;
}

// One key column of slot keys (F3: kmin + slot, F3h: the table's key words)
static void PartGroupOneKeyOut(Engine &e, const BoundSelect &s, const PartGroupRun &r, dev::EmitDesc &D, DRel &out) {
  D.has_key = 1;
  D.key_phys = PhysOf(s.groups[0]->type);
  DCol kc = AllocOut(e, s.groups[0]->type, r.nslots, true, false);
  D.key_out = kc.data;
  D.key_valid = (uint32_t *)kc.validity;
  out.cols.clear();
  out.cols.push_back(kc);
}

// F3h: the wide GROUP BY over hashed partitions (group_part.hip); groups come
// out in hash-table order (DuckDB's hash aggregate order is unspecified too).
// false: a table filled up (more groups than the tables hold) -- the caller's
// hash path answers.
static bool PartGroupHashedAggregate(Engine &e, const DRel &src, const BoundSelect &s, const DCol &K,
                                     const PartGroupValues &v, DRel &out) {
  PartGroupRun r;
  PartGroupPrepare(e, src, v, 0, r);
  r.d.key = K.data;
  r.d.kphys = K.phys;
  if (!PartGroupHashedRun(e, src, r, (double)src.n * PhysSize(K.phys) + PartGroupValueBytes(src, v))) return false;
  dev::EmitDesc D;
  memset(&D, 0, sizeof(D));
  D.key_msb = (const unsigned long long *)r.gk->p;
  PartGroupOneKeyOut(e, s, r, D, out);
  PartGroupEmit(e, s, v, r, D, out);
  return true;
}

// F3: GROUP BY one integer key (no NULLs) whose zone-map range is too wide for
// F2's LDS tables but dense enough for per-key state arrays (1024 < range <=
// PartGroupMaxRange, range <= 4 n), no WHERE, COUNT / SUM / MIN / MAX / AVG over
// <= 2 integer columns of one phys without NULLs: rows partitioned by key
// range, each partition reduced in LDS (group_part.hip), then the non-empty
// keys compacted and emitted in key order as F2 does.  false: the shape does
// not fit (the hash path or the run-time compiled kernel takes it).
static bool PartGroupAggregate(Engine &e, const DRel &src, const BoundSelect &s, DRel &out) {
  if (const char *k = Knob("MBX_PART_GROUP"))  // MBX_PART_GROUP=0: the hash path (A/B)
    if (atoi(k) == 0) return false;
  if (s.groups.size() != 1 || s.where || src.range || src.n <= 0 || src.n >= ((int64_t)1 << 32)) return false;
  if (s.groups[0]->kind != BExpr::COL || !FastIntCol(src, s.groups[0]->col)) return false;
  const DCol &K = src.cols[s.groups[0]->col];
  const DevColumn *ks = K.table_col;
  if (!ks || !ks->stats_valid || ks->null_count != 0) return false;
  const i128 range = ks->imax - ks->imin + 1;
  PartGroupValues v;
  if (!PartGroupValueCols(src, s, v) || range <= 1024) return false;
  const int nv = (int)v.vcols.size();
  // keys too sparse for dense per-key states: hashed partitions (F3h), from
  // 2^16 rows (below, the hash path's table is small) with at most one value column
  if (range > dev::PartGroupMaxRange(nv, v.mm) || range > 4 * (i128)src.n)
    return nv <= 1 && src.n >= ((int64_t)1 << 16) && PartGroupHashedAggregate(e, src, s, K, v, out);
  PartGroupRun r;
  PartGroupPrepare(e, src, v, (int64_t)range, r);
  r.d.key = K.data;
  r.d.kphys = K.phys;
  r.d.kmin = (int64_t)ks->imin;
  r.d.range = r.nslots;
  {
    // algorithmic bytes: the key and value columns once
    ProfScope ps(e, "group_part", (double)src.n * PhysSize(K.phys) + PartGroupValueBytes(src, v), src.n);
    if (!dev::PartGroup(r.d, e.stream)) return false;
  }
  dev::EmitDesc D;
  memset(&D, 0, sizeof(D));
  D.kmin = (int64_t)ks->imin;
  PartGroupOneKeyOut(e, s, r, D, out);
  PartGroupEmit(e, s, v, r, D, out);
  return true;
}

// The same over the group code of 1..4 integer key columns and their validity
// (group_code.h): GROUP BY k1, k2[, k3[, k4]], or one NULL-able key too wide
// for F2's LDS tables.  No WHERE, at least 2^16 rows, more than 4096 codes (so
// the shape never competes with F2 or the run-time compiled jit_group); values
// as F3 / F3h take them.  Dense codes (total <= PartGroupMaxRange and <= 4 n)
// come out in code order -- key order, NULLs last per key, as F2 and jit_group
// emit; else hashed partitions, groups in table order (<= 1 value column).
// false: the shape does not fit or the hashed tables filled up.
static bool CodeGroupAggregate(Engine &e, const DRel &src, const BoundSelect &s, DRel &out) {
  const int ng = (int)s.groups.size();
  if (const char *k = Knob("MBX_PART_GROUP"))
    if (atoi(k) == 0) return false;
  if (ng < 1 || ng > kGroupCodeMaxKeys || s.where || src.range || src.n < ((int64_t)1 << 16) ||
      src.n >= ((int64_t)1 << 32))
    return false;
  GroupCodeKeyIn in[kGroupCodeMaxKeys];
  bool nullable = false;
  for (int i = 0; i < ng; i++) {
    const BExpr *x = StripWidening(s.groups[i].get());
    // integer types only (DECIMAL / DATE keys keep the hash path); the emitted
    // key column is a fixed-width integer of at most 64 bits
    if (x->kind != BExpr::COL || !IsIntegral(s.groups[i]->type.id) || !IsIntegral(x->type.id) ||
        ClassOf(s.groups[i]->type) != VC_I64)
      return false;
    const Phys kp = PhysOf(s.groups[i]->type);
    if (kp == P_I128 || kp == P_U64) return false;
    const DCol &c = src.cols[x->col];
    if (!c.table_col || c.table_col->data != c.data) return false;
    in[i].data = c.data;
    in[i].validity = c.validity;
    in[i].phys = c.phys;
    in[i].stats_valid = c.table_col->stats_valid;
    in[i].imin = c.table_col->imin;
    in[i].imax = c.table_col->imax;
    nullable |= c.validity != nullptr;
  }
  if (ng == 1 && !nullable) return false;  // F3's own shape
  GroupCodePlan plan;
  if (!PlanGroupCode(in, ng, &plan) || plan.total <= 4096) return false;
  PartGroupValues v;
  if (!PartGroupValueCols(src, s, v)) return false;
  const int nv = (int)v.vcols.size();
  const bool dense = plan.total <= dev::PartGroupMaxRange(nv, v.mm) && (i128)plan.total <= 4 * (i128)src.n;
  if (!dense && nv > 1) return false;
  // algorithmic bytes: every key column, n / 8 per validity bitmap, every value column
  double bytes = PartGroupValueBytes(src, v);
  for (int i = 0; i < ng; i++)
    bytes += (double)src.n * PhysSize((Phys)in[i].phys) + (in[i].validity ? (double)src.n / 8 : 0);
  PartGroupRun r;
  PartGroupPrepare(e, src, v, dense ? plan.total : 0, r);
  r.d.code = &plan;
  if (dense) {
    r.d.range = plan.total;
    ProfScope ps(e, "group_part", bytes, src.n);
    if (!dev::PartGroup(r.d, e.stream)) return false;
  } else if (!PartGroupHashedRun(e, src, r, bytes)) {
    return false;
  }
  dev::EmitDesc D;
  memset(&D, 0, sizeof(D));
  if (!dense) D.code_msb = (const unsigned long long *)r.gk->p;
  D.nkeys_c = ng;
  out.cols.clear();
  for (int i = 0; i < ng; i++) {
    DCol kc = AllocOut(e, s.groups[i]->type, r.nslots, true, false);
    D.kc[i].out = kc.data;
    D.kc[i].valid = (uint32_t *)kc.validity;
    D.kc[i].phys = PhysOf(s.groups[i]->type);
    D.kc[i].nullable = plan.k[i].nullable;
    D.kc[i].kmin = plan.k[i].kmin;
    D.kc[i].radix = plan.k[i].radix;
    D.kc[i].stride = plan.k[i].stride;
    out.cols.push_back(kc);
  }
  PartGroupEmit(e, s, v, r, D, out);
  return true;
}

static DRel Aggregate(Engine &e, const DRel &src, const BoundSelect &s) {
  const int ng = (int)s.groups.size();
  const int na = (int)s.aggs.size();
  if (na > EMIT_MAX_AGGS) ThrowError("Not implemented", "too many aggregates in one query for the device path");
  for (auto &a : s.aggs)
    if (a.distinct) return DistinctAggregate(e, src, s);
  DRel out;
  // ---- fast path F1: no GROUP BY, range predicate on one int column, all
  //      aggregates over one int column (or COUNT(*)).
  if (ng == 0 && !src.range) {
    DRel multi_out;
    if (FilterMultiAggregate(e, src, s, multi_out)) return multi_out;
    int pcol = -1;
    i128 lo = (i128)INT64_MIN, hi = (i128)INT64_MAX;
    bool pred_ok = !s.where || RangePredicate(*s.where, &pcol, &lo, &hi);
    if (pred_ok && pcol >= 0 && !FastIntCol(src, pcol)) pred_ok = false;
    int acol = -1;
    bool aggs_ok = pred_ok;
    for (auto &a : s.aggs) {
      if (a.kind == A_COUNT_STAR) continue;
      if (a.distinct) aggs_ok = false;
      const BExpr *x = a.arg ? StripWidening(a.arg.get()) : nullptr;
      if (!x || x->kind != BExpr::COL || !FastIntCol(src, x->col)) {
        aggs_ok = false;
        break;
      }
      if (a.arg->type.id == T_DOUBLE || a.arg->type.id == T_FLOAT) aggs_ok = false;
      if (acol >= 0 && acol != x->col) aggs_ok = false;
      acol = x->col;
    }
    if (aggs_ok && src.n > 0) {
      if (lo < (i128)INT64_MIN) lo = INT64_MIN;
      if (hi > (i128)INT64_MAX) hi = INT64_MAX;
      bool empty = lo > hi;
      dev::AggState *st = (dev::AggState *)e.d_small;
      unsigned long long *cstar = (unsigned long long *)((char *)e.d_small + 1024);
      int npartials = 0;
      if (empty) dev::InitAggStatesCounts(st, 1, cstar, 1, e.stream);
      if (!empty) {
        const DCol *P = pcol >= 0 ? &src.cols[pcol] : nullptr;
        const DCol *A = acol >= 0 ? &src.cols[acol] : nullptr;
        if (!P && A) {
          // no predicate: use the aggregate column as the (always-true) predicate column
          P = A;
        }
        if (!P) P = nullptr;
        double bytes = 0;
        if (P) bytes += (double)src.n * PhysSize(P->phys);
        if (A && A != P) bytes += (double)src.n * PhysSize(A->phys);
        // The predicate column's code image stands in for its values when it
        // covers exactly these rows and the aggregates, if any, read the same
        // column; a slice, an intermediate or a second column reads the values.
        const DevColumn *tc = P ? P->table_col : nullptr;
        const bool by_codes = e.scan_codes && tc && tc->codes && P->data == tc->data && src.n == tc->code_rows &&
                              (!A || A == P) && src.n < ((int64_t)1 << 40);
        bool need_mm = false;
        for (auto &a : s.aggs) need_mm |= a.kind == A_MIN || a.kind == A_MAX;
        if (by_codes) {
          const ScanCodeRange cr = PlanScanCodeRange(tc->code_width, (i128)tc->code_base, tc->imax, (int64_t)lo, (int64_t)hi);
          if (cr.empty) {
            // the zone map rules every row out: no scan (the entry keeps the
            // profile at one filter_agg per statement, with nothing read)
            ProfScope ps(e, "filter_agg", 0, src.n);
            dev::InitAggStatesCounts(st, 1, cstar, 1, e.stream);
          } else {
            ProfScope ps(e, "filter_agg", (double)src.n * tc->code_width, src.n);
            npartials = dev::FilterAggCodes(tc->codes, tc->code_width, tc->code_base, cr.clo, cr.cspan, cr.packed,
                                            A != nullptr, need_mm, src.n, e.d_partials, e.stream);
          }
        } else if (P) {
          ProfScope ps(e, "filter_agg", bytes, src.n);
          // zone-map bound on |value| of the aggregated column (lets the kernel
          // keep int64 per-lane partial sums; ~0 = unknown)
          uint64_t maxabs = ~0ull;
          if (A && A->table_col && A->table_col->stats_valid) {
            i128 m1 = A->table_col->imin < 0 ? -A->table_col->imin : A->table_col->imin;
            i128 m2 = A->table_col->imax < 0 ? -A->table_col->imax : A->table_col->imax;
            i128 m = m1 > m2 ? m1 : m2;
            if (m <= (i128)INT64_MAX) maxabs = (uint64_t)m;
          }
          npartials = dev::FilterAggStates(P->data, P->phys, (int64_t)lo, (int64_t)hi, pcol >= 0, A ? A->data : nullptr,
                                           A ? A->phys : P_I64, src.n, st, cstar, 0, e.stream, need_mm, maxabs,
                                           e.d_partials);
        } else {
          // COUNT(*) without predicate: the row count is known
          dev::InitAggStatesCounts(st, 1, cstar, 1, e.stream);
          unsigned long long c = (unsigned long long)src.n;
          HIPCHK(hipMemcpyAsync(cstar, &c, 8, hipMemcpyHostToDevice, e.stream));
          HIPCHK(hipStreamSynchronize(e.stream));
        }
      }
      out.n = 1;
      dev::EmitDesc D;
      memset(&D, 0, sizeof(D));
      D.nagg = na;
      D.cstar = cstar;
      D.nslots = 1;
      D.null_slot = -1;
      D.partials = e.d_partials;
      D.npartials = npartials;
      for (int j = 0; j < na; j++) {
        DCol oc = AllocOut(e, s.aggs[j].type, 1, true, false);
        D.a[j] = EmitFor(s.aggs[j], VC_I64, s.aggs[j].kind == A_COUNT_STAR ? nullptr : st, oc);
        out.cols.push_back(oc);
      }
      dev::EmitAggRelation(D, e.stream);
      return out;
    }
  }
  // ---- fast path F2: GROUP BY one small-range int key column, aggregates
  //      over <= 2 int columns of one phys, no predicate.
  //      (plus: up to GROUP_MAX_PRED range predicates on int columns, fused)
  // Filtered shapes run here too: since its table atomics stopped draining
  // the DMA ring, group_direct_lds beats the run-time compiled jit_group at
  // 1e9 rows (c3_where 3.00 vs 3.34 ms, c3_where2 3.66 vs 4.06 ms,
  // profiles/r02_group_where_sweep.log); jit_group takes the shapes F2 does not.
  std::map<int, std::pair<i128, i128>> f2_ranges;
  bool f2_pred_ok = !s.where || (RangeConj(*s.where, f2_ranges) && f2_ranges.size() <= GROUP_MAX_PRED);
  for (auto &kv : f2_ranges)
    if (!FastIntCol(src, kv.first) || kv.second.first > kv.second.second) f2_pred_ok = false;
  // NULL-able key and value columns ride along: their validity words are loaded
  // with the step (group_direct_lds VM), a NULL key is its own group
  auto int_col = [&](int c) {
    const DCol &d = src.cols[c];
    return FastIntCol(src, c) ||
           (!(src.range && c == 0) && d.validity && (d.phys == P_I32 || d.phys == P_I64) && d.data &&
            (uintptr_t)d.validity % 16 == 0);
  };
  const char *gd_nulls = Knob("MBX_GD_NULLS");  // MBX_GD_NULLS=0: NULL-able columns keep the generic paths
  const bool nulls_ok = !(gd_nulls && atoi(gd_nulls) == 0);
  if (ng == 1 && f2_pred_ok && !src.range && s.groups[0]->kind == BExpr::COL &&
      (FastIntCol(src, s.groups[0]->col) || (nulls_ok && int_col(s.groups[0]->col)))) {
    const DCol &K = src.cols[s.groups[0]->col];
    const DevColumn *ks = K.table_col;
    std::vector<int> vcols;
    const bool knull = K.validity != nullptr;
    bool ok = ks && ks->stats_valid && (knull || ks->null_count == 0) && src.n > 0;
    bool mm = false;
    for (auto &a : s.aggs) {
      if (a.kind == A_COUNT_STAR) continue;
      if (a.distinct) ok = false;
      const BExpr *x = a.arg ? StripWidening(a.arg.get()) : nullptr;
      if (!x || x->kind != BExpr::COL || !int_col(x->col) || a.arg->type.id == T_DOUBLE) {
        ok = false;
        break;
      }
      if (a.kind == A_MIN || a.kind == A_MAX) mm = true;
      if (std::find(vcols.begin(), vcols.end(), x->col) == vcols.end()) vcols.push_back(x->col);
    }
    dev::GroupValidity gval;
    memset(&gval, 0, sizeof(gval));
    gval.key = knull ? K.validity : nullptr;
    for (size_t j = 0; j < vcols.size() && j < 2; j++)
      if (src.cols[vcols[j]].validity) {
        if (!nulls_ok) ok = false;
        (j == 0 ? gval.v0 : gval.v1) = src.cols[vcols[j]].validity;
      }
    const int vm = (gval.v0 ? 1 : 0) | (gval.v1 ? 2 : 0) | (gval.key ? 4 : 0);
    if (ok && vcols.size() <= 2) {
      if (vcols.size() == 2 && src.cols[vcols[0]].phys != src.cols[vcols[1]].phys) ok = false;
      i128 range = ks->imax - ks->imin + 1;
      if (range > 1024 || range < 1) ok = false;
      // overflow-free int64 partial sums: seg_rows / R rows per replica
      i128 maxabs = 0;
      for (int c : vcols) {
        const DevColumn *vs = src.cols[c].table_col;
        if (!vs || !vs->stats_valid) ok = false;
        else maxabs = std::max(maxabs, std::max(vs->imax < 0 ? -vs->imax : vs->imax, vs->imin < 0 ? -vs->imin : vs->imin));
      }
      if (ok) {
        int nk = (int)range + (knull ? 1 : 0);  // + the NULL group's slot, last
        int nv = (int)vcols.size();
        int R = 64;
        while (R > 1 && dev::GroupDirectLds(nk, R, nv, mm, vm) > 48 * 1024) R >>= 1;
        if (dev::GroupDirectLds(nk, R, nv, mm, vm) > 64 * 1024) ok = false;
        int64_t seg = 0;  // whole chunk
        if (maxabs > 0) {
          i128 per_rep = ((i128)1 << 62) / maxabs;  // rows one replica may absorb
          i128 seg128 = per_rep * R;
          if (seg128 < 4096) ok = false;
          if (seg128 < (i128)INT64_MAX / 2) seg = (int64_t)seg128;
        }
        if ((int64_t)R * ((int64_t)1 << 31) < seg || seg == 0) {
          // u32 replica counts: cap segment length
          int64_t cap = (int64_t)R * ((int64_t)1 << 30);
          if (seg == 0 || seg > cap) seg = cap;
        }
        if (ok) {
          int64_t nslots = nk;
          size_t st_bytes = (size_t)nslots * sizeof(dev::AggState);
          // both value columns' states in one block, zeroed with the COUNT(*) slots
          // by one launch ahead of the scan
          auto cs = Alloc(e, nslots * 8);
          auto sb = Alloc(e, 2 * st_bytes);
          dev::AggState *const s0p = (dev::AggState *)sb->p, *const s1p = s0p + nslots;
          // GroupByDirectStates initialises the states for its atomic forms, or
          // has every workgroup write a record of its table (up to
          // kGroupPartialKeys keys) that GroupPartialsCompact reduces
          DevBufPtr gparts;
          dev::GroupPartialsOut po;
          memset(&po, 0, sizeof(po));
          po.state_slots = 2 * nslots;
          if (nk <= dev::kGroupPartialKeys) {
            po.bytes = (size_t)nk * dev::NumCUs() * 3 * dev::GroupPartialWords(2, true) * 8;
            gparts = Alloc(e, po.bytes);
            po.buf = gparts->p;
          }
          Phys vphys = nv ? src.cols[vcols[0]].phys : P_I64;
          double bytes = (double)src.n * PhysSize(K.phys);
          for (int c : vcols) bytes += (double)src.n * PhysSize(src.cols[c].phys);
          bytes += __builtin_popcount(vm) * (src.n / 8.0);  // validity words
          dev::GroupPreds gp;
          memset(&gp, 0, sizeof(gp));
          for (auto &kv : f2_ranges) {
            const int kcol = s.groups[0]->col, pc = kv.first;
            dev::GroupPred &g = gp.p[gp.n++];
            g.src = pc == kcol ? 2 : (nv > 0 && pc == vcols[0]) ? 3 : 1;
            g.phys = src.cols[pc].phys;
            g.col = src.cols[pc].data;
            g.lo = (int64_t)std::max<i128>(kv.second.first, INT64_MIN);
            g.span = (uint64_t)((int64_t)std::min<i128>(kv.second.second, INT64_MAX)) - (uint64_t)g.lo;
            if (g.src == 1) bytes += (double)src.n * PhysSize(src.cols[pc].phys);
          }
          bool launched;
          {
            ProfScope ps(e, "group_direct", bytes, src.n);
            launched = dev::GroupByDirectStates(K.data, K.phys, (int64_t)ks->imin, nk,
                                                nv > 0 ? src.cols[vcols[0]].data : nullptr,
                                                nv > 1 ? src.cols[vcols[1]].data : nullptr, vphys, nv, mm, src.n, seg,
                                                R, (unsigned long long *)cs->p, s0p,
                                                s1p, 0, e.stream, gp.n ? &gp : nullptr,
                                                maxabs < ((i128)1 << 62) ? (uint64_t)maxabs : ~0ull,
                                                vm ? &gval : nullptr, &po);
          }
          if (!launched) goto generic;
          auto list = Alloc(e, nslots * 4);
          // the group count: left on the device for ToHost when this is the
          // statement's own result (CountMayStayOnDevice), else read below
          const bool defer = CountMayStayOnDevice(e, s);
          DevBufPtr nbuf = defer ? Alloc(e, 8) : nullptr;
          int64_t *const n_out = defer ? (int64_t *)nbuf->p : e.d_scratch;
          if (!po.used)
            dev::CompactSlots((const unsigned long long *)cs->p, nslots, (int32_t *)list->p, n_out, e.stream);
          // outputs sized for every slot (<= 1024 rows): the emit reads the group
          // count from the device, so the query waits on the stream once, after it
          dev::EmitDesc D;
          memset(&D, 0, sizeof(D));
          D.nagg = na;
          D.cstar = (const unsigned long long *)cs->p;
          D.slot_list = (const int32_t *)list->p;
          D.n_list = n_out;
          D.nslots = nslots;
          D.has_key = 1;
          D.key_phys = PhysOf(s.groups[0]->type);
          D.kmin = (int64_t)ks->imin;
          D.null_slot = knull ? nk - 1 : -1;
          DCol kc = AllocOut(e, s.groups[0]->type, nslots, true, false);
          D.key_out = kc.data;
          D.key_valid = (uint32_t *)kc.validity;
          out.cols.push_back(kc);
          for (int j = 0; j < na; j++) {
            DCol oc = AllocOut(e, s.aggs[j].type, nslots, true, false);
            dev::AggState *stp = nullptr;
            if (s.aggs[j].kind != A_COUNT_STAR) {
              int c = StripWidening(s.aggs[j].arg.get())->col;
              stp = c == vcols[0] ? s0p : s1p;
            }
            D.a[j] = EmitFor(s.aggs[j], VC_I64, stp, oc);
            out.cols.push_back(oc);
          }
          if (po.used)  // records reduced, keys compacted and the relation written by one launch
            dev::GroupPartialsCompact(po, nv, mm, nk, (unsigned long long *)cs->p, s0p, s1p, (int32_t *)list->p,
                                      n_out, e.stream, &D);
          else
            dev::EmitAggRelation(D, e.stream);
          if (defer) {
            out.n = nslots;  // the columns hold every slot; the count follows the rows to the host
            out.n_dev = n_out;
            out.n_owner = nbuf;
          } else {
            out.n = ReadDev<int64_t>(e, n_out);
          }
          return out;
        }
      }
    }
  }
  // ---- fast path F3: one integer key over a wide range, partitioned
  if (ng == 1) {
    DRel part_out;
    if (PartGroupAggregate(e, src, s, part_out)) return part_out;
  }
generic:
  // ---- generic path: compact [groups..., agg args...] then reduce
  std::vector<BExprPtr> exprs = s.groups;
  std::vector<int> arg_idx(na, -1);
  for (int j = 0; j < na; j++) {
    if (s.aggs[j].kind == A_COUNT_STAR) continue;
    arg_idx[j] = (int)exprs.size();
    exprs.push_back(s.aggs[j].arg);
  }
  if (jit::Enabled()) {
    DRel fused;
    if (ng == 0 ? JitAggregate(e, src, s, fused) : JitGroupAggregate(e, src, s, fused)) return fused;
  }
  // ---- composite / NULL-able integer keys over more than 4096 codes: the
  //      partitioned GROUP BY over the keys' group code
  if (ng >= 1) {
    DRel code_out;
    if (CodeGroupAggregate(e, src, s, code_out)) return code_out;
  }
  DRel tmp = FilterProject(e, src, s.where, exprs);
  if (ng == 0) {
    size_t st_bytes = std::max(na, 1) * sizeof(dev::AggState);
    auto sb = Alloc(e, st_bytes);
    dev::InitAggStates((dev::AggState *)sb->p, std::max(na, 1), e.stream);
    auto cs = Alloc(e, 8);
    unsigned long long cn = (unsigned long long)tmp.n;
    HIPCHK(hipMemcpyAsync(cs->p, &cn, 8, hipMemcpyHostToDevice, e.stream));
    for (int j = 0; j < na; j++) {
      if (arg_idx[j] < 0) continue;
      const DCol &c = tmp.cols[arg_idx[j]];
      const void *data = c.data;
      int phys = c.phys;
      if (c.phys == P_STR) {
        // COUNT(varchar) only needs the validity: scan the offsets as int64
        if (s.aggs[j].kind != A_COUNT)
          ThrowError("Not implemented", "SUM/MIN/MAX/AVG over VARCHAR are not supported on device");
        data = c.offsets;
        phys = P_I64;
      }
      ProfScope ps(e, "reduce_column", (double)tmp.n * PhysSize((Phys)phys), tmp.n);
      dev::ReduceColumn(data, phys, c.validity, tmp.n, (dev::AggState *)sb->p + j, e.stream);
    }
    dev::EmitDesc D;
    memset(&D, 0, sizeof(D));
    D.nagg = na;
    D.cstar = (const unsigned long long *)cs->p;
    D.nslots = 1;
    D.null_slot = -1;
    out.n = 1;
    for (int j = 0; j < na; j++) {
      DCol oc = AllocOut(e, s.aggs[j].type, 1, true, false);
      VClass ic = arg_idx[j] >= 0 ? ClassOf(tmp.cols[arg_idx[j]].type) : VC_I64;
      D.a[j] = EmitFor(s.aggs[j], ic, (dev::AggState *)sb->p + j, oc);
      out.cols.push_back(oc);
    }
    dev::EmitAggRelation(D, e.stream);
    HIPCHK(hipStreamSynchronize(e.stream));
    return out;
  }
  // one integer key with a narrow range: direct-index slots; anything else
  // (several keys, VARCHAR/float keys, wide ranges): the hash table
  const DCol &K = tmp.cols[0];
  bool direct = ng == 1 && ClassOf(K.type) == VC_I64 && K.phys != P_STR && K.phys != P_F64 && K.phys != P_F32 &&
                K.phys != P_I128 && K.phys != P_INTERVAL;
  int64_t kmin = 0;
  i128 range = 0;
  if (direct) {
    long long *kr = (long long *)((char *)e.d_small + 2048);
    dev::KeyRange(K.data, K.phys, K.validity, tmp.n, kr, e.stream);
    long long krh[3];
    HIPCHK(hipMemcpyAsync(krh, kr, sizeof(krh), hipMemcpyDeviceToHost, e.stream));
    HIPCHK(hipStreamSynchronize(e.stream));
    kmin = krh[2] ? krh[0] : 0;
    range = krh[2] ? (i128)krh[1] - krh[0] + 1 : 0;
    if (range > (1 << 24) || range > 4 * (i128)std::max<int64_t>(tmp.n, 1024)) direct = false;
  }
  if (!direct) return HashAggregate(e, tmp, s, arg_idx);
  if (!K.validity && range <= 1024 && range >= 1) {
    // filtered / projected input, small key range: LDS-privatised reduction
    std::vector<DevBufPtr> keep;
    std::vector<dev::AggState *> st_of;
    const unsigned long long *cstar = nullptr;
    if (DirectReduceAll(e, K.data, K.phys, kmin, (int64_t)range, tmp.n, tmp, s, arg_idx, keep, st_of, &cstar)) {
      const int64_t nk = (int64_t)range;
      auto list = Alloc(e, nk * 4);
      dev::CompactSlots(cstar, nk, (int32_t *)list->p, e.d_scratch, e.stream);
      int64_t ngroups = ReadDev<int64_t>(e, e.d_scratch);
      dev::EmitDesc D;
      memset(&D, 0, sizeof(D));
      D.nagg = na;
      D.cstar = cstar;
      D.slot_list = (const int32_t *)list->p;
      D.n_list = e.d_scratch;
      D.nslots = ngroups;
      D.has_key = 1;
      D.key_phys = PhysOf(s.groups[0]->type);
      D.kmin = kmin;
      D.null_slot = -1;
      DCol kc = AllocOut(e, s.groups[0]->type, ngroups, true, false);
      D.key_out = kc.data;
      D.key_valid = (uint32_t *)kc.validity;
      out.n = ngroups;
      out.cols.push_back(kc);
      for (int j = 0; j < na; j++) {
        DCol oc = AllocOut(e, s.aggs[j].type, ngroups, true, false);
        D.a[j] = EmitFor(s.aggs[j], VC_I64, st_of[j], oc);
        out.cols.push_back(oc);
      }
      if (ngroups > 0) dev::EmitAggRelation(D, e.stream);
      HIPCHK(hipStreamSynchronize(e.stream));
      return out;
    }
  }
  int64_t nslots = (int64_t)range + 1;  // + NULL group
  auto slot_of = Alloc(e, std::max<int64_t>(tmp.n, 1) * 4);
  auto cs = Alloc(e, nslots * 8, true);
  {
    ProfScope ps(e, "group_assign", (double)tmp.n * PhysSize(K.phys), tmp.n);
    dev::GroupAssign(K.data, K.phys, K.validity, kmin, nslots, tmp.n, (int32_t *)slot_of->p,
                     (unsigned long long *)cs->p, e.stream);
  }
  std::vector<DevBufPtr> states(na);
  for (int j = 0; j < na; j++) {
    if (arg_idx[j] < 0) continue;
    const DCol &c = tmp.cols[arg_idx[j]];
    const void *data = c.data;
    int phys = c.phys;
    if (c.phys == P_STR) {
      if (s.aggs[j].kind != A_COUNT)
        ThrowError("Not implemented", "SUM/MIN/MAX/AVG over VARCHAR are not supported on device");
      data = c.offsets;
      phys = P_I64;
    }
    states[j] = Alloc(e, nslots * sizeof(dev::AggState));
    dev::InitAggStates((dev::AggState *)states[j]->p, nslots, e.stream);
    ProfScope ps(e, "group_reduce", (double)tmp.n * (PhysSize((Phys)phys) + 4), tmp.n);
    dev::GroupReduceColumn((const int32_t *)slot_of->p, data, phys, c.validity, tmp.n,
                           (dev::AggState *)states[j]->p, e.stream);
  }
  auto list = Alloc(e, nslots * 4);
  dev::CompactSlots((const unsigned long long *)cs->p, nslots, (int32_t *)list->p, e.d_scratch, e.stream);
  int64_t ngroups = ReadDev<int64_t>(e, e.d_scratch);
  dev::EmitDesc D;
  memset(&D, 0, sizeof(D));
  D.nagg = na;
  D.cstar = (const unsigned long long *)cs->p;
  D.slot_list = (const int32_t *)list->p;
  D.n_list = e.d_scratch;
  D.nslots = ngroups;
  D.has_key = 1;
  D.key_phys = PhysOf(s.groups[0]->type);
  D.kmin = kmin;
  D.null_slot = nslots - 1;
  DCol kc = AllocOut(e, s.groups[0]->type, ngroups, true, false);
  D.key_out = kc.data;
  D.key_valid = (uint32_t *)kc.validity;
  out.n = ngroups;
  out.cols.push_back(kc);
  for (int j = 0; j < na; j++) {
    DCol oc = AllocOut(e, s.aggs[j].type, ngroups, true, false);
    VClass ic = arg_idx[j] >= 0 ? ClassOf(tmp.cols[arg_idx[j]].type) : VC_I64;
    D.a[j] = EmitFor(s.aggs[j], ic, states[j] ? (dev::AggState *)states[j]->p : nullptr, oc);
    out.cols.push_back(oc);
  }
  dev::EmitAggRelation(D, e.stream);
  HIPCHK(hipStreamSynchronize(e.stream));
  DropEmptyValidity(e, out);
  return out;
}

// ---------------------------------------------------------------------------
// sort, limit, union
// ---------------------------------------------------------------------------
static DRel GatherRel(Engine &e, const DRel &r, const int64_t *perm, int64_t n) {
  DRel out;
  out.n = n;
  for (const DCol &c : r.cols) {
    if (c.phys == P_STR) {
      // gather codes = perm, then materialize strings from the source column
      DCol d;
      d.type = c.type;
      d.phys = P_STR;
      auto codes = Alloc(e, std::max<int64_t>(n, 1) * 8);
      HIPCHK(hipMemcpyAsync(codes->p, perm, n * 8, hipMemcpyDeviceToDevice, e.stream));
      d.data = codes->p;
      d.owners.push_back(codes);
      if (c.validity) {
        auto v = Alloc(e, Words64(std::max<int64_t>(n, 1)) * 8, true);
        // validity gather through a fixed-width gather of a dummy u8 column
        auto dummy = Alloc(e, std::max<int64_t>(r.n, 1));
        auto dout = Alloc(e, std::max<int64_t>(n, 1));
        dev::GatherFixed(dummy->p, P_U8, c.validity, perm, n, dout->p, (uint32_t *)v->p, e.stream);
        d.validity = (uint64_t *)v->p;
        d.owners.push_back(v);
        d.owners.push_back(dummy);
        d.owners.push_back(dout);
      }
      StrPool empty;
      MaterializeStrings(e, d, &c, empty, n);
      out.cols.push_back(d);
      continue;
    }
    DCol d = AllocOut(e, c.type, n, c.validity != nullptr);
    dev::GatherFixed(c.data, c.phys, c.validity, perm, n, d.data, (uint32_t *)d.validity, e.stream);
    out.cols.push_back(d);
  }
  return out;
}

static DRel SortRel(Engine &e, const DRel &r, const std::vector<BoundOrder> &order) {
  int64_t n = r.n;
  if (n <= 1 || order.empty()) return r;
  auto perm = Alloc(e, n * 8), perm2 = Alloc(e, n * 8);
  auto keys = Alloc(e, n * 8), keys2 = Alloc(e, n * 8);
  dev::Iota((int64_t *)perm->p, n, 0, e.stream);
  // LSD over the ORDER BY keys (last key first); each key is one or more
  // stable 64-bit radix passes, then a stable 1-bit pass placing its NULLs
  auto pass = [&](int end_bit) {
    ProfScope ps(e, "radix_sort", (double)n * 16, n);
    dev::SortPairs((uint64_t *)keys->p, (int64_t *)perm->p, (uint64_t *)keys2->p, (int64_t *)perm2->p, n, e.stream,
                   end_bit);
    std::swap(perm, perm2);
  };
  for (int k = (int)order.size() - 1; k >= 0; k--) {
    const BoundOrder &o = order[k];
    const DCol &c = r.cols[o.expr->col];
    if (c.phys == P_I128 || c.phys == P_INTERVAL)
      ThrowError("Not implemented", "ORDER BY a " + c.type.ToString() + " column is not supported on device yet");
    if (c.phys == P_STR) {
      if (!c.offsets || !c.chars) ThrowError("Internal", "ORDER BY VARCHAR without materialised strings");
      dev::StrMaxLen(c.offsets, n, (unsigned long long *)e.d_scratch, e.stream);
      int64_t maxlen = ReadDev<int64_t>(e, e.d_scratch);
      for (int64_t ch = (maxlen + 7) / 8 - 1; ch >= 0; ch--) {
        dev::SortKeyStr(c.offsets, c.chars, c.validity, n, (const int64_t *)perm->p, ch, o.desc, (uint64_t *)keys->p,
                        e.stream);
        pass(64);
      }
    } else {
      dev::SortKeyU64(c.data, c.phys, c.validity, n, (const int64_t *)perm->p, o.desc, o.nulls_first,
                      (uint64_t *)keys->p, e.stream);
      pass(64);
    }
    if (c.validity) {
      dev::SortKeyNull(c.validity, n, (const int64_t *)perm->p, o.nulls_first, (uint64_t *)keys->p, e.stream);
      pass(1);
    }
  }
  DRel out = GatherRel(e, r, (const int64_t *)perm->p, n);
  HIPCHK(hipStreamSynchronize(e.stream));
  return out;
}

static DRel ConcatRels(Engine &e, std::vector<DRel> &parts) {
  DRel out;
  int64_t total = 0;
  for (auto &p : parts) total += p.n;
  out.n = total;
  size_t nc = parts[0].cols.size();
  for (size_t c = 0; c < nc; c++) {
    const DCol &c0 = parts[0].cols[c];
    bool anyv = false;
    for (auto &p : parts)
      if (p.cols[c].validity) anyv = true;
    DCol d;
    d.type = c0.type;
    d.phys = c0.phys;
    if (anyv) {
      auto v = Alloc(e, Words64(std::max<int64_t>(total, 1)) * 8, true);
      d.validity = (uint64_t *)v->p;
      d.owners.push_back(v);
    }
    if (c0.phys == P_STR) {
      int64_t chars = 0;
      for (auto &p : parts) chars += p.cols[c].chars_len;
      auto ob = Alloc(e, (total + 1) * 8), cb = Alloc(e, std::max<int64_t>(chars, 1));
      int64_t row = 0, cpos = 0;
      for (auto &p : parts) {
        const DCol &s = p.cols[c];
        if (p.n) {
          dev::RebaseOffsets(s.offsets, (int64_t *)ob->p + row, p.n + 1, cpos, e.stream);
          if (s.chars_len)
            HIPCHK(hipMemcpyAsync((char *)cb->p + cpos, s.chars, s.chars_len, hipMemcpyDeviceToDevice, e.stream));
        }
        row += p.n;
        cpos += s.chars_len;
      }
      if (total == 0) HIPCHK(hipMemsetAsync(ob->p, 0, 8, e.stream));
      d.offsets = (int64_t *)ob->p;
      d.chars = (char *)cb->p;
      d.chars_len = chars;
      d.owners.push_back(ob);
      d.owners.push_back(cb);
    } else {
      int sz = PhysSize(c0.phys);
      auto db = Alloc(e, std::max<int64_t>(total, 1) * sz);
      int64_t row = 0;
      for (auto &p : parts) {
        if (p.n) HIPCHK(hipMemcpyAsync((char *)db->p + row * sz, p.cols[c].data, p.n * sz, hipMemcpyDeviceToDevice, e.stream));
        row += p.n;
      }
      d.data = db->p;
      d.owners.push_back(db);
    }
    if (anyv) {
      int64_t row = 0;
      for (auto &p : parts) {
        dev::BitmapAppend(d.validity, row, p.cols[c].validity, p.n, e.stream);
        row += p.n;
      }
    }
    out.cols.push_back(d);
  }
  HIPCHK(hipStreamSynchronize(e.stream));
  return out;
}

// ---------------------------------------------------------------------------
// device -> host
// ---------------------------------------------------------------------------
// Small fixed-width results: every column (values + validity words) and the
// device error word are copied into the pinned arena and the query waits on
// the stream once.  Returns nullptr when the result does not qualify.
// Rows [start, start + n) of every column land in the pinned arena (grown on
// demand) with ONE synchronisation; the device error word rides along.
// Large results pulled cell by cell (duckdb_mb_query, stream batches) bring
// their integer / BOOLEAN / DECIMAL / HUGEINT cells' text along: the text
// kernels format the rows on the device (lengths -> scan -> write, as the
// Arrow string getters do) and the lengths and the NUL-separated text ride the
// same D2H as the values, so duckdb_mb_result_value / duckdb_mb_chunk_value
// only copy bytes.  From kTextRows rows (smaller results keep host formatting).
constexpr int64_t kTextRows = 65536;

static bool TextCol(const DCol &d, int64_t start, dev::TextCol &tc) {
  if (!d.data || d.phys > P_I128) return false;
  switch (d.type.id) {
    case T_BOOLEAN: case T_TINYINT: case T_SMALLINT: case T_INTEGER: case T_BIGINT: case T_UTINYINT:
    case T_USMALLINT: case T_UINTEGER: case T_UBIGINT: case T_HUGEINT: case T_DECIMAL:
      break;
    default:
      return false;
  }
  if (d.validity && (start & 63)) return false;  // validity words must start at the first row
  tc.data = (const char *)d.data + (size_t)start * PhysSize(d.phys);
  tc.valid = d.validity ? d.validity + (start >> 6) : nullptr;
  tc.phys = d.phys;
  tc.kind = d.type.id == T_BOOLEAN ? dev::TEXT_BOOL : d.type.id == T_DECIMAL ? dev::TEXT_DECIMAL : dev::TEXT_INT;
  tc.scale = d.type.id == T_DECIMAL ? d.type.scale : 0;
  return true;
}

static ResultPtr ToHostPinned(Engine &e, const DRel &r, const std::vector<std::string> &names, size_t ncols,
                              int64_t start, int64_t n, bool text = false, const int64_t *count_dev = nullptr) {
  // count_dev: the true row count (<= n) is on the device: it rides the one
  // mapped copy with the n rows, which are trimmed to it (nullptr when that copy
  // does not apply, before anything is launched)
  if (count_dev && (start != 0 || (text && n >= kTextRows))) return nullptr;
  size_t need = count_dev ? 128 : 64;
  const int64_t w0 = start >> 6, w1 = (start + n + 63) >> 6;
  for (size_t c = 0; c < ncols; c++) {
    const DCol &d = r.cols[c];
    if (d.phys == P_STR) return nullptr;
    need += ((size_t)n * PhysSize(d.phys) + 63) & ~(size_t)63;
    if (d.validity) need += ((size_t)(w1 - w0) * 8 + 63) & ~(size_t)63;
  }
  // device text: per eligible column, lengths and an exclusive scan (the
  // totals read back with one synchronisation), then the text itself
  struct TextJob {
    size_t c;
    dev::TextCol tc;
    DevBufPtr lens, offs, chars;
    int64_t total = 0;
    size_t len_off = 0, chr_off = 0;
  };
  std::vector<TextJob> tj;
  if (text && n >= kTextRows && n < ((int64_t)1 << 31)) {
    for (size_t c = 0; c < ncols && tj.size() < 64; c++) {
      TextJob j;
      j.c = c;
      if (!TextCol(r.cols[c], start, j.tc)) continue;
      j.lens = Alloc(e, (size_t)n * 4);  // (reused for the 32-bit offsets of a direct copy)
      j.offs = Alloc(e, (size_t)(n + 1) * 8);
      {
        ProfScope ps(e, "text_lengths", (double)n * PhysSize(r.cols[c].phys), n);
        dev::TextLengths(j.tc, n, (uint32_t *)j.lens->p, e.stream);
      }
      dev::ScanTileCounts((const uint32_t *)j.lens->p, (int64_t *)j.offs->p, n, e.d_scratch + 64 + tj.size(),
                          e.stream);
      tj.push_back(j);
    }
    if (!tj.empty()) {
      HIPCHK(hipMemcpyAsync(e.h_pinned, e.d_scratch + 64, tj.size() * 8, hipMemcpyDeviceToHost, e.stream));
      HIPCHK(hipStreamSynchronize(e.stream));
      for (size_t k = 0; k < tj.size(); k++) memcpy(&tj[k].total, e.h_pinned + 8 * k, 8);
      tj.erase(std::remove_if(tj.begin(), tj.end(), [](const TextJob &j) { return j.total > (int64_t)UINT32_MAX; }),
               tj.end());  // 32-bit text offsets on the host
      for (size_t k = 0; k < tj.size(); k++) {
        tj[k].chars = Alloc(e, (size_t)std::max<int64_t>(tj[k].total, 16));
        ProfScope ps(e, "text_write", (double)n * PhysSize(r.cols[tj[k].c].phys) + (double)tj[k].total, n);
        dev::TextWrite(tj[k].tc, n, (const int64_t *)tj[k].offs->p, (char *)tj[k].chars->p, nullptr, e.stream);
        need += (((size_t)n * 4 + 63) & ~(size_t)63) + (((size_t)tj[k].total + 63) & ~(size_t)63);
      }
    }
  }
  // small results: one copy kernel into the coherent mapped buffer instead of
  // one DMA per buffer; larger ones: DMA into the (growable) pinned arena
  const bool mapped = tj.empty() && need <= Engine::kMappedBytes && ncols * 2 + 1 <= HOSTCOPY_MAX &&
                      !Knob("MBX_NO_HOSTCOPY");
  if (count_dev && !mapped) return nullptr;
  if (!mapped && !e.EnsurePinned(need)) return nullptr;
  uint8_t *const H = mapped ? e.h_mapped : e.h_pinned;
  // large results: the value columns and the device-formatted text go by DMA
  // straight into the result's own host buffers (page-locked blocks of the
  // result block cache) instead of through the pinned arena and a host copy
  const bool direct = !mapped && need >= ((size_t)4 << 20) && !Knob("MBX_RESULT_STAGED");
  std::vector<HostColumn> dcols(direct ? ncols : 0);
  std::vector<size_t> data_off(ncols), valid_off(ncols, 0);
  dev::HostCopyDesc hd;
  memset(&hd, 0, sizeof(hd));
  auto seg = [&](const void *src, size_t off, size_t bytes) {
    if (mapped) hd.seg[hd.nseg++] = dev::HostCopySeg{src, H + off, (int64_t)bytes};
    else HIPCHK(hipMemcpyAsync(H + off, src, bytes, hipMemcpyDeviceToHost, e.stream));
  };
  size_t at = 64;  // [0, 4): error word; [64, 72): the device row count (count_dev)
  if (!mapped) HIPCHK(hipMemcpyAsync(H, e.d_err, 4, hipMemcpyDeviceToHost, e.stream));
  if (count_dev) {
    seg(count_dev, at, 8);
    at += 64;
  }
  for (size_t c = 0; c < ncols; c++) {
    const DCol &d = r.cols[c];
    const int sz = PhysSize(d.phys);
    size_t bytes = (size_t)n * sz;
    data_off[c] = at;
    if (bytes && direct) {
      dcols[c].data.resize(bytes);  // (ResultAlloc: no zero fill)
      HIPCHK(hipMemcpyAsync(dcols[c].data.data(), (const char *)d.data + (size_t)start * sz, bytes,
                            hipMemcpyDeviceToHost, e.stream));
    } else if (bytes) {
      seg((const char *)d.data + (size_t)start * sz, at, bytes);
    }
    at += (bytes + 63) & ~(size_t)63;
    if (d.validity) {
      valid_off[c] = at;
      size_t vb = (size_t)(w1 - w0) * 8;
      if (n > 0) seg(d.validity + w0, at, vb);
      at += (vb + 63) & ~(size_t)63;
    }
  }
  for (auto &j : tj) {
    j.len_off = at;
    if (direct) {  // the host's 32-bit offsets made on the device, straight into the result
      // (the scan wrote offsets [0, n); entry n, the total, is set on the host)
      dev::OffsetsU32((const int64_t *)j.offs->p, (uint32_t *)j.lens->p, n, e.stream);
      dcols[j.c].text_off.resize((size_t)n + 1);
      HIPCHK(hipMemcpyAsync(dcols[j.c].text_off.data(), j.lens->p, (size_t)n * 4, hipMemcpyDeviceToHost, e.stream));
      dcols[j.c].text_off[n] = (uint32_t)j.total;
    } else {
      seg(j.lens->p, at, (size_t)n * 4);
    }
    at += ((size_t)n * 4 + 63) & ~(size_t)63;
    j.chr_off = at;
    if (j.total && direct) {
      dcols[j.c].text.resize((size_t)j.total);
      HIPCHK(hipMemcpyAsync(dcols[j.c].text.data(), j.chars->p, (size_t)j.total, hipMemcpyDeviceToHost, e.stream));
    } else if (j.total) {
      seg(j.chars->p, at, (size_t)j.total);
    }
    at += ((size_t)j.total + 63) & ~(size_t)63;
  }
  if (mapped) {
    hd.err_src = e.d_err;
    hd.err_dst = (int32_t *)H;
    dev::HostCopy(hd, e.stream);
  }
  HIPCHK(hipStreamSynchronize(e.stream));
  int32_t err;
  memcpy(&err, (const void *)H, 4);
  RaiseDeviceError(e, err);
  if (count_dev) {
    int64_t cnt;
    memcpy(&cnt, (const void *)(H + 64), 8);
    if (cnt < 0 || cnt > n) ThrowError("Internal", "device row count out of range");
    n = cnt;
  }
  auto res = std::make_shared<MaterializedResult>();
  res->nrows = n;
  for (size_t c = 0; c < ncols; c++) {
    const DCol &d = r.cols[c];
    HostColumn hc;
    hc.name = names[c];
    hc.type = d.type;
    hc.phys = d.phys;
    size_t bytes = (size_t)n * PhysSize(d.phys);
    if (direct) {
      hc.data = std::move(dcols[c].data);
      hc.data.resize(bytes);  // (a device row count below n trims)
    } else {
      hc.data.assign(H + data_off[c], H + data_off[c] + bytes);
    }
    if (d.validity && n > 0) {
      const uint64_t *bm = (const uint64_t *)(H + valid_off[c]);
      const int64_t sh = start - (w0 << 6);
      hc.valid.resize(n);
      for (int64_t i = 0; i < n; i++) hc.valid[i] = (bm[(i + sh) >> 6] >> ((i + sh) & 63)) & 1;
    }
    for (auto &j : tj) {
      if (j.c != c) continue;
      if (direct) {
        hc.text_off = std::move(dcols[c].text_off);
        hc.text = std::move(dcols[c].text);
        continue;
      }
      const uint32_t *len = (const uint32_t *)(H + j.len_off);
      hc.text_off.resize((size_t)n + 1);
      uint32_t o = 0;
      for (int64_t i = 0; i < n; i++) {
        hc.text_off[i] = o;
        o += len[i];
      }
      hc.text_off[n] = o;
      hc.text.assign((const char *)H + j.chr_off, (const char *)H + j.chr_off + (size_t)j.total);
    }
    res->cols.push_back(std::move(hc));
  }
  return res;
}

static ResultPtr ToHost(Engine &e, const DRel &r, const std::vector<std::string> &names, int64_t offset, int64_t limit,
                        size_t ncols, bool text) {
  if (r.n_dev) {
    // the rows (all n of the upper bound) and the count in one copy; else read the count first
    if (offset <= 0 && limit < 0)
      if (ResultPtr p = ToHostPinned(e, r, names, ncols, 0, r.n, text, r.n_dev)) return p;
    DRel settled = r;
    SettleCount(e, settled);
    return ToHost(e, settled, names, offset, limit, ncols, text);
  }
  int64_t start = std::min(std::max<int64_t>(offset, 0), r.n);
  int64_t n = r.n - start;
  if (limit >= 0) n = std::min(n, limit);
  {
    ResultPtr p = ToHostPinned(e, r, names, ncols, start, n, text);
    if (p) return p;
  }
  auto res = std::make_shared<MaterializedResult>();
  res->nrows = n;
  for (size_t c = 0; c < ncols; c++) {
    const DCol &d = r.cols[c];
    HostColumn hc;
    hc.name = names[c];
    hc.type = d.type;
    hc.phys = d.phys;
    if (d.phys == P_STR) {
      std::vector<int64_t> off(n + 1);
      if (n > 0) {
        HIPCHK(hipMemcpyAsync(off.data(), d.offsets + start, (n + 1) * 8, hipMemcpyDeviceToHost, e.stream));
        HIPCHK(hipStreamSynchronize(e.stream));
        int64_t base = off[0], len = off[n] - off[0];
        hc.chars.resize(len);
        if (len) HIPCHK(hipMemcpyAsync(&hc.chars[0], d.chars + base, len, hipMemcpyDeviceToHost, e.stream));
        for (auto &o : off) o -= base;
      } else {
        off[0] = 0;
      }
      hc.offsets = off;
    } else {
      int sz = PhysSize(d.phys);
      hc.data.resize((size_t)n * sz);
      if (n > 0) HIPCHK(hipMemcpyAsync(hc.data.data(), (char *)d.data + start * sz, (size_t)n * sz, hipMemcpyDeviceToHost, e.stream));
    }
    if (d.validity && n > 0) {
      int64_t w0 = start >> 6, w1 = (start + n + 63) >> 6;
      std::vector<uint64_t> bm(w1 - w0);
      HIPCHK(hipMemcpyAsync(bm.data(), d.validity + w0, bm.size() * 8, hipMemcpyDeviceToHost, e.stream));
      HIPCHK(hipStreamSynchronize(e.stream));
      hc.valid.resize(n);
      for (int64_t i = 0; i < n; i++) {
        int64_t b = start + i - (w0 << 6);
        hc.valid[i] = (bm[b >> 6] >> (b & 63)) & 1;
      }
    }
    res->cols.push_back(std::move(hc));
  }
  HIPCHK(hipStreamSynchronize(e.stream));
  CheckError(e);
  return res;
}

// ---------------------------------------------------------------------------
// select
// ---------------------------------------------------------------------------
static ResultPtr HostConstantSelect(const BoundSelect &s);

static DRel RunSelectDev(Engine &e, Connection &c, const BoundSelect &s, bool top = false);

static DRel SourceRel(Engine &e, Connection &c, const BoundSource &src) {
  DRel r;
  switch (src.kind) {
    case BoundSource::ONE_ROW:
      r.n = 1;
      break;
    case BoundSource::RANGE: {
      r.n = src.RangeCount();
      r.range = true;
      r.rs = src.range_start;
      r.rstep = src.range_step;
      DCol d;
      d.type = LogicalType(T_BIGINT);
      d.phys = P_I64;
      r.cols.push_back(d);
      break;
    }
    case BoundSource::TABLE: {
      r.n = src.table->nrows;
      for (auto &col : src.table->cols) r.cols.push_back(ColFromTable(col));
      break;
    }
    case BoundSource::VALUES:
      r = UploadRows(e, src.rows, src.col_types);
      break;
    case BoundSource::SUBQUERY:
      r = RunSelectDev(e, c, *src.sub);
      // hidden order keys of the subquery are dropped by RunSelectDev
      break;
  }
  return r;
}

static DRel ShardedBranch(Engine &e, Connection &c, const BoundSelect &s);

static DRel RunBranch(Engine &e, Connection &c, const BoundSelect &s) {
  if (s.src.kind == BoundSource::TABLE && s.src.table && s.src.table->sharded()) return ShardedBranch(e, c, s);
  if (IsHostConstantSelect(s) && s.union_all.empty()) {
    ResultPtr hr = HostConstantSelect(s);
    DRel r;
    r.n = hr->nrows;
    for (auto &hc : hr->cols) {
      DCol d;
      UploadHostColumn(e, hc, hr->nrows, d);
      r.cols.push_back(d);
    }
    return r;
  }
  DRel src = SourceRel(e, c, s.src);
  if (s.is_agg) {
    DRel agg = Aggregate(e, src, s);
    return FilterProject(e, agg, s.having, s.outputs);
  }
  return FilterProject(e, src, s.where, s.outputs);
}

static size_t VisibleCols(const BoundSelect &s) {
  size_t n = 0;
  for (auto &nm : s.names)
    if (nm.rfind("__order_", 0) != 0) n++;
  return n;
}

// top: the statement's own result (handed to the host or kept as a device
// result), not a subquery's or an INSERT's input
static DRel RunSelectDev(Engine &e, Connection &c, const BoundSelect &s, bool top) {
  DRel r = RunBranch(e, c, s);
  if (!top || !s.union_all.empty() || !s.order.empty() || s.limit >= 0 || s.offset > 0) SettleCount(e, r);
  if (!s.union_all.empty()) {
    std::vector<DRel> parts;
    parts.push_back(r);
    for (auto &u : s.union_all) parts.push_back(RunBranch(e, c, *u));
    r = ConcatRels(e, parts);
  }
  if (!s.order.empty()) r = SortRel(e, r, s.order);
  if (s.limit >= 0 || s.offset > 0) {
    int64_t start = std::min(s.offset, r.n);
    int64_t n = r.n - start;
    if (s.limit >= 0) n = std::min(n, s.limit);
    // a top-level result's fixed-width columns are sliced in place (their
    // owners / pins keep the buffers alive; only element-wise kernels and
    // copies read a result, so the slice's 4/8-B alignment is enough); strings,
    // the virtual range column and a bitmap that would start mid-word take the
    // gather
    bool slice = top && !r.range;
    for (auto &d : r.cols) slice &= d.phys != P_STR && d.data && (!d.validity || start % 64 == 0);
    if (slice) {
      for (auto &d : r.cols) {
        d.data = (char *)d.data + (size_t)start * PhysSize(d.phys);
        if (d.validity) d.validity += start / 64;
      }
      r.n = n;
      r.cols.resize(VisibleCols(s));
      return r;
    }
    auto perm = Alloc(e, std::max<int64_t>(n, 1) * 8);
    dev::Iota((int64_t *)perm->p, n, start, e.stream);
    r = GatherRel(e, r, (const int64_t *)perm->p, n);
  }
  r.cols.resize(VisibleCols(s));
  return r;
}

// ---- host-constant selects (no FROM): the binder folded every expression
static ResultPtr HostConstantSelect(const BoundSelect &s) {
  std::vector<std::vector<Value>> rows;
  std::function<void(const BoundSelect &)> add = [&](const BoundSelect &b) {
    bool keep = true;
    if (b.where) {
      Value w = EvalConst(*b.where);
      keep = !w.is_null && w.i;
    }
    if (b.is_agg) {
      // aggregates over the single constant row
      std::vector<Value> aggvals;
      for (auto &g : b.groups) aggvals.push_back(EvalConst(*g));
      for (auto &a : b.aggs) {
        Value v;
        Value x = a.arg ? EvalConst(*a.arg) : Value::Int(T_BIGINT, 1);
        bool has = keep && (!a.arg || !x.is_null);
        switch (a.kind) {
          case A_COUNT_STAR: v = Value::Int(T_BIGINT, keep ? 1 : 0); break;
          case A_COUNT: v = Value::Int(T_BIGINT, has ? 1 : 0); break;
          case A_AVG: v = has ? CastValue(x, LogicalType(T_DOUBLE)) : Value::Null(a.type); break;
          default: v = has ? CastValue(x, a.type) : Value::Null(a.type); break;
        }
        aggvals.push_back(v);
      }
      if (!b.groups.empty() && !keep) return;
      // bind outputs over the aggregate row
      std::function<Value(const BExpr &)> ev = [&](const BExpr &x) -> Value {
        if (x.kind == BExpr::COL) return aggvals[x.col];
        if (x.kind == BExpr::CONST) return EvalConst(x);
        BExpr copy = x;
        for (auto &ch : copy.ch) {
          Value v = ev(*ch);
          auto c = std::make_shared<BExpr>();
          c->kind = BExpr::CONST;
          c->cval = v;
          c->type = ch->type;
          ch = c;
        }
        return EvalConst(copy);
      };
      if (b.having) {
        Value h = ev(*b.having);
        if (h.is_null || !h.i) return;
      }
      std::vector<Value> row;
      for (auto &o : b.outputs) row.push_back(CastValue(ev(*o), o->type));
      rows.push_back(row);
      return;
    }
    if (!keep) return;
    std::vector<Value> row;
    for (auto &o : b.outputs) row.push_back(CastValue(EvalConst(*o), o->type));
    rows.push_back(row);
  };
  add(s);
  for (auto &u : s.union_all) add(*u);
  // ORDER BY / LIMIT over constant rows (tiny): the rows are already values
  if (!s.order.empty()) {
    std::stable_sort(rows.begin(), rows.end(), [&](const std::vector<Value> &a, const std::vector<Value> &b) {
      for (auto &o : s.order) {
        const Value &x = a[o.expr->col], &y = b[o.expr->col];
        if (x.is_null || y.is_null) {
          if (x.is_null && y.is_null) continue;
          bool xfirst = x.is_null == o.nulls_first;
          return xfirst;
        }
        Value xc = x, yc = y;
        int c;
        if (ClassOf(x.type) == VC_F64) c = x.d < y.d ? -1 : x.d > y.d ? 1 : 0;
        else if (ClassOf(x.type) == VC_STR) c = x.s < y.s ? -1 : x.s > y.s ? 1 : 0;
        else c = x.i < y.i ? -1 : x.i > y.i ? 1 : 0;
        if (c) return o.desc ? c > 0 : c < 0;
      }
      return false;
    });
  }
  int64_t start = std::min<int64_t>(s.offset, (int64_t)rows.size());
  int64_t n = (int64_t)rows.size() - start;
  if (s.limit >= 0) n = std::min(n, s.limit);
  auto res = std::make_shared<MaterializedResult>();
  res->nrows = n;
  size_t nvis = VisibleCols(s);
  for (size_t c = 0; c < nvis; c++) {
    HostColumn hc;
    hc.name = s.names[c];
    hc.type = s.outputs[c]->type;
    hc.phys = PhysOf(hc.type);
    if (hc.phys == P_STR) hc.offsets.push_back(0);
    for (int64_t i = 0; i < n; i++) HostColumnPush(hc, rows[start + i][c]);
    res->cols.push_back(std::move(hc));
  }
  return res;
}

static ResultPtr ShardedAggregateHost(Connection &c, const BoundSelect &s);

static void FinishProfile(Connection &c, Engine &e, double total_ms) {
  QueryProfile &p = c.last_profile;
  p.kernels.clear();
  p.total_ms = total_ms;
  if (!e.profile) {
    e.shard_kernels.clear();
    return;
  }
  hipStreamSynchronize(e.stream);
  for (auto &ev : e.events) {
    float ms = 0;
    hipEventElapsedTime(&ms, ev.a, ev.b);
    QueryProfile::Kernel k;
    k.name = ev.name;
    k.ms = ms;
    k.bytes = ev.bytes;
    k.rows = ev.rows;
    p.kernels.push_back(k);
    if (c.profile_history.size() < 100000) c.profile_history.push_back(k);
  }
  for (auto &k : e.shard_kernels) {
    p.kernels.push_back(k);
    if (c.profile_history.size() < 100000) c.profile_history.push_back(k);
  }
  e.shard_kernels.clear();
  e.events.clear();
  e.ev_used = 0;
}

ResultPtr ExecuteSelect(Connection &c, const BoundSelect &s) {
  auto t0 = std::chrono::steady_clock::now();
  if (IsHostConstantSelect(s)) {
    ResultPtr r = HostConstantSelect(s);
    c.last_profile = QueryProfile();
    return r;
  }
  Engine &e = Eng(c);
  e.profile = c.opts.profile;
  e.events.clear();
  e.ev_used = 0;
  if (c.sharded()) {
    if (ResultPtr hr = ShardedAggregateHost(c, s)) {
      double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
      FinishProfile(c, e, ms);
      return hr;
    }
  }
  struct DeferScope {  // the statement's own aggregate may leave its group count on the device
    Engine &e;
    DeferScope(Engine &en, const BoundSelect &s) : e(en) { e.defer_count_for = &s; }
    ~DeferScope() { e.defer_count_for = nullptr; }
  } defer(e, s);
  DRel r = RunSelectDev(e, c, s, true);
  std::vector<std::string> names(s.names.begin(), s.names.begin() + VisibleCols(s));
  ResultPtr res = ToHost(e, r, names, 0, -1, names.size(), true);  // raises pending device errors
  double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  FinishProfile(c, e, ms);
  return res;
}

// ---- device-resident results for streams ----------------------------------
struct DeviceResult {
  DRel r;
  std::vector<std::string> names;
};

// nullptr for host-constant SELECTs (the caller materializes those)
DeviceResultPtr ExecuteSelectDevice(Connection &c, const BoundSelect &s, StreamSource *meta) {
  if (IsHostConstantSelect(s)) return nullptr;
  auto t0 = std::chrono::steady_clock::now();
  Engine &e = Eng(c);
  e.profile = c.opts.profile;
  e.events.clear();
  e.ev_used = 0;
  auto d = std::make_shared<DeviceResult>();
  d->r = RunSelectDev(e, c, s, true);
  d->names.assign(s.names.begin(), s.names.begin() + VisibleCols(s));
  CheckError(e);  // (its copy of the error word waits for the whole stream)
  meta->names = d->names;
  meta->types.clear();
  for (size_t i = 0; i < d->names.size(); i++) meta->types.push_back(d->r.cols[i].type);
  meta->nrows = d->r.n;
  double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
  FinishProfile(c, e, ms);
  return d;
}

ResultPtr FetchDeviceRows(Connection &c, DeviceResult &d, int64_t start, int64_t n) {
  Engine &e = Eng(c);
  return ToHost(e, d.r, d.names, start, n, d.names.size(), true);
}

bool DeviceColumnWireOk(const DeviceResult &d, int col, int phys) {
  if (col < 0 || col >= (int)d.r.cols.size()) return false;
  const DCol &dc = d.r.cols[col];
  const int w = PhysSize(dc.phys);
  return dc.phys == phys && dc.data && (w == 1 || w == 4 || w == 8) && dc.phys != P_STR;
}

// Device -> fresh pageable host memory (a getter's Bytes) at link rate
// (hostlink.cpp); the source is complete (its stream was synchronised).
static void LinkCopy(Engine &e, void *dst, const void *src, size_t n) {
  const std::string err = LinkD2H(e.device, dst, src, n);
  if (!err.empty()) ThrowError("IO", err);
}

// The Arrow wire form of one device column (values with NULLs zeroed, then
// validity bytes when vbytes != nullptr), built by one kernel in a device
// staging buffer and copied out with one DMA per part.
bool CopyDeviceColumnWire(Connection &c, DeviceResult &d, int col, int phys, void *vals, uint8_t *vbytes) {
  if (!DeviceColumnWireOk(d, col, phys)) return false;
  const DCol &dc = d.r.cols[col];
  Engine &e = Eng(c);
  const int64_t n = d.r.n;
  const int w = PhysSize(dc.phys);
  if (n <= 0) return true;
  if (!dc.validity) {  // nothing to zero: the column is already the wire layout
    HIPCHK(hipStreamSynchronize(e.stream));
    LinkCopy(e, vals, dc.data, (size_t)n * w);
    if (vbytes) memset(vbytes, 1, (size_t)n);
    return true;
  }
  auto buf = Alloc(e, (size_t)n * (w + 1) + 16);
  uint8_t *dv = (uint8_t *)buf->p, *db = dv + (size_t)n * w;
  dev::ArrowWire(dc.data, dc.validity, n, w, dv, vbytes ? db : nullptr, e.stream);
  HIPCHK(hipStreamSynchronize(e.stream));
  CheckError(e);
  LinkCopy(e, vals, dv, (size_t)n * w);
  if (vbytes) LinkCopy(e, vbytes, db, (size_t)n);
  return true;
}

bool DeviceColumnTextOk(const DeviceResult &d, int col) {
  if (col < 0 || col >= (int)d.r.cols.size()) return false;
  const DCol &dc = d.r.cols[col];
  if (!dc.data || dc.phys > P_I128) return false;
  switch (dc.type.id) {
    case T_BOOLEAN: case T_TINYINT: case T_SMALLINT: case T_INTEGER: case T_BIGINT: case T_UTINYINT:
    case T_USMALLINT: case T_UINTEGER: case T_UBIGINT: case T_HUGEINT: case T_DECIMAL:
      return true;
    default:
      return false;
  }
}

bool CopyDeviceColumnText(Connection &c, DeviceResult &d, int col, const std::function<uint8_t *(int64_t)> &dst,
                          bool vbytes) {
  if (!DeviceColumnTextOk(d, col)) return false;
  const DCol &dc = d.r.cols[col];
  Engine &e = Eng(c);
  const int64_t n = d.r.n;
  dev::TextCol tc;
  tc.data = dc.data;
  tc.valid = dc.validity;
  tc.phys = dc.phys;
  tc.kind = dc.type.id == T_BOOLEAN ? dev::TEXT_BOOL : dc.type.id == T_DECIMAL ? dev::TEXT_DECIMAL : dev::TEXT_INT;
  tc.scale = dc.type.id == T_DECIMAL ? dc.type.scale : 0;
  auto lens = Alloc(e, (size_t)std::max<int64_t>(n, 1) * 4);
  auto offs = Alloc(e, (size_t)(n + 1) * 8);
  {
    ProfScope ps(e, "text_lengths", (double)n * PhysSize(dc.phys), n);
    dev::TextLengths(tc, n, (uint32_t *)lens->p, e.stream);
  }
  dev::ScanTileCounts((const uint32_t *)lens->p, (int64_t *)offs->p, n, e.d_scratch, e.stream);
  const int64_t chars = ReadDev<int64_t>(e, e.d_scratch);
  uint8_t *host = dst(chars);
  if (!host) return false;
  const size_t out_bytes = (size_t)chars + (vbytes ? (size_t)n : 0);
  auto buf = Alloc(e, std::max<size_t>(out_bytes, 16));
  {
    ProfScope ps(e, "text_write", (double)n * PhysSize(dc.phys) + (double)out_bytes, n);
    dev::TextWrite(tc, n, (const int64_t *)offs->p, (char *)buf->p, vbytes ? (uint8_t *)buf->p + chars : nullptr,
                   e.stream);
  }
  HIPCHK(hipStreamSynchronize(e.stream));
  CheckError(e);
  if (out_bytes) LinkCopy(e, host, buf->p, out_bytes);
  if (e.profile) {  // a getter runs after its query's profile was taken: its kernels go to the drain history
    for (auto &ev : e.events) {
      float ms = 0;
      hipEventElapsedTime(&ms, ev.a, ev.b);
      QueryProfile::Kernel k;
      k.name = ev.name;
      k.ms = ms;
      k.bytes = ev.bytes;
      k.rows = ev.rows;
      if (c.profile_history.size() < 100000) c.profile_history.push_back(k);
    }
    e.events.clear();
    e.ev_used = 0;
  }
  return true;
}

// ---------------------------------------------------------------------------
// tables: creation, append, stats
// ---------------------------------------------------------------------------
Table::~Table() {}  // column buffers go with their owners (a live result may still hold them)

TablePtr CreateDeviceTable(Connection &c, const std::string &name, const std::vector<std::string> &names,
                           const std::vector<LogicalType> &types) {
  if (c.sharded()) {
    auto t = std::make_shared<Table>();
    t->name = name;
    t->col_names = names;
    t->device = c.engine->device;
    for (auto &ty : types) {
      DevColumn dc;
      dc.type = ty;
      dc.phys = PhysOf(ty);
      t->cols.push_back(dc);
    }
    std::string key = name;
    for (auto &ch : key) ch = (char)tolower((unsigned char)ch);
    for (auto &sc : c.shards) {
      TablePtr p = CreateDeviceTable(*sc, name, names, types);
      sc->catalog.tables[key] = p;
      t->parts.push_back(p);
    }
    return t;
  }
  auto t = std::make_shared<Table>();
  t->name = name;
  t->col_names = names;
  t->device = c.engine->device;
  for (auto &ty : types) {
    DevColumn dc;
    dc.type = ty;
    dc.phys = PhysOf(ty);
    dc.stats_valid = true;
    dc.imin = 0;
    dc.imax = 0;
    t->cols.push_back(dc);
  }
  return t;
}

void DropDeviceTable(Table &t) { (void)t; }

// a table buffer from hipMalloc, freed when its last holder lets go (the
// column, or a result reading it in place; possibly on another thread)
static std::shared_ptr<void> DevOwned(Engine &e, void *p) {
  const int dev = e.device;
  return std::shared_ptr<void>(p, [dev](void *q) {
    int prev = -1;
    (void)hipGetDevice(&prev);
    if (prev != dev) (void)hipSetDevice(dev);
    (void)hipFree(q);
    if (prev != dev && prev >= 0) (void)hipSetDevice(prev);
  });
}

static void Grow(Engine &e, DevColumn &c, int64_t nrows_old, int64_t need) {
  if (need <= c.capacity && (c.phys != P_STR || c.offsets)) return;
  int64_t cap = std::max<int64_t>(need, std::max<int64_t>(1024, c.capacity * 2));
  if (c.phys == P_STR) {
    int64_t *no = nullptr;
    HIPCHK(hipMalloc(&no, (cap + 1) * 8));
    if (c.offsets) HIPCHK(hipMemcpyAsync(no, c.offsets, (nrows_old + 1) * 8, hipMemcpyDeviceToDevice, e.stream));
    else HIPCHK(hipMemsetAsync(no, 0, 8, e.stream));
    HIPCHK(hipStreamSynchronize(e.stream));
    c.offsets_owner = DevOwned(e, no);
    c.offsets = no;
  } else {
    void *nd = nullptr;
    int sz = PhysSize(c.phys);
    HIPCHK(hipMalloc(&nd, (size_t)cap * sz));
    if (c.data && nrows_old) HIPCHK(hipMemcpyAsync(nd, c.data, (size_t)nrows_old * sz, hipMemcpyDeviceToDevice, e.stream));
    HIPCHK(hipStreamSynchronize(e.stream));
    c.data_owner = DevOwned(e, nd);
    c.data = nd;
  }
  if (c.validity) {
    uint64_t *nv = nullptr;
    HIPCHK(hipMalloc(&nv, Words64(cap) * 8));
    HIPCHK(hipMemsetAsync(nv, 0xFF, Words64(cap) * 8, e.stream));
    HIPCHK(hipMemcpyAsync(nv, c.validity, Words64(nrows_old) * 8, hipMemcpyDeviceToDevice, e.stream));
    HIPCHK(hipStreamSynchronize(e.stream));
    c.validity_owner = DevOwned(e, nv);
    c.validity = nv;
  }
  c.capacity = cap;
}

// Brings c's code image (scan_codes.h) up to nrows rows, once the zone map of
// every row is folded: the appended tail when the map still fits the image's
// base and width, all rows when the base or the width changed, and no image
// when the column does not qualify.  A column is never left partly coded
// beyond this call: code_rows is nrows or the image is gone.
static void UpdateScanCodes(Engine &e, DevColumn &c, int64_t nrows) {
  int w = 0;
  if (e.scan_codes && nrows > 0 && nrows >= e.scan_codes_min_rows && c.stats_valid && !c.validity &&
      c.null_count == 0 && c.data)
    w = ScanCodeWidth(c.phys, c.imin, c.imax);
  if (!w) {
    c.codes = nullptr;
    c.codes_owner.reset();
    c.code_width = 0;
    c.code_base = c.code_rows = c.code_cap = 0;
    return;
  }
  const bool extend = c.codes && c.code_width == w && c.code_base == (int64_t)c.imin && c.code_rows <= nrows;
  const int64_t begin = extend ? c.code_rows : 0;
  if (begin == nrows) return;
  if (!extend || c.code_cap < nrows) {
    const int64_t cap = std::max<int64_t>(nrows, c.capacity);
    void *nc = nullptr;
    HIPCHK(hipMalloc(&nc, (size_t)cap * w));
    if (begin > 0) {
      HIPCHK(hipMemcpyAsync(nc, c.codes, (size_t)begin * w, hipMemcpyDeviceToDevice, e.stream));
      HIPCHK(hipStreamSynchronize(e.stream));  // before the old image goes
    }
    c.codes_owner = DevOwned(e, nc);
    c.codes = nc;
    c.code_cap = cap;
    c.code_width = w;
    c.code_base = (int64_t)c.imin;
  }
  {
    ProfScope ps(e, "scan_encode", (double)(nrows - begin) * (PhysSize(c.phys) + w), nrows - begin);
    dev::ScanEncode(c.data, c.phys, c.codes, w, c.code_base, begin, nrows, e.stream);
  }
  c.code_rows = nrows;
}

static void EnsureValidity(Engine &e, DevColumn &c, int64_t nrows_old) {
  if (c.validity) return;
  int64_t cap = std::max<int64_t>(c.capacity, 1);
  HIPCHK(hipMalloc(&c.validity, Words64(cap) * 8));
  c.validity_owner = DevOwned(e, c.validity);
  HIPCHK(hipMemsetAsync(c.validity, 0xFF, Words64(cap) * 8, e.stream));
  (void)nrows_old;
}

// the zone map the producing kernel left on d (DCol::zn), folded in instead of
// a statistics pass over the appended rows
static bool FoldKernelStats(DevColumn &c, const DCol &d, int64_t n, bool first_rows) {
  if (d.zn != n || d.phys != c.phys || (c.phys != P_I32 && c.phys != P_I64)) return false;
  FoldStats(c, n, d.zvalid, d.zmin, d.zmax, first_rows);
  return true;
}

static void UpdateStats(Engine &e, DevColumn &c, int64_t off, int64_t n, bool first_rows, bool async = false) {
  if (n <= 0) return;
  if (c.phys == P_STR || c.phys == P_F32 || c.phys == P_F64 || c.phys == P_I128 || c.phys == P_U64 ||
      c.phys == P_INTERVAL) {
    c.stats_valid = false;
    return;
  }
  long long *o3 = (long long *)((char *)e.d_small + 3072);
  int sz = PhysSize(c.phys);
  // stats over the appended range; validity offsets are bit offsets, so use a
  // validity-free pass when the column has no NULLs
  const uint64_t *v = nullptr;
  if (c.validity && (off & 63) == 0) v = c.validity + (off >> 6);
  else if (c.validity) {
    c.stats_valid = false;
    return;
  }
  {
    ProfScope ps(e, "zone_map", (double)n * sz + (v ? n / 8.0 : 0), n);
    dev::ColumnStats((const char *)c.data + off * sz, c.phys, v, n, o3, e.stream);
  }
  if (async) {
    long long *slot = nullptr;
    if (!e.stat_slots.empty()) {
      slot = e.stat_slots.back();
      e.stat_slots.pop_back();
    } else {
      HIPCHK(hipHostMalloc((void **)&slot, 3 * sizeof(long long), hipHostMallocDefault));
    }
    HIPCHK(hipMemcpyAsync(slot, o3, 3 * sizeof(long long), hipMemcpyDeviceToHost, e.stream));
    e.pending_stats.push_back({&c, slot, n, first_rows, off + n});
    return;
  }
  long long h[3];
  HIPCHK(hipMemcpyAsync(h, o3, sizeof(h), hipMemcpyDeviceToHost, e.stream));
  HIPCHK(hipStreamSynchronize(e.stream));
  FoldStats(c, n, h[2], h[0], h[1], first_rows);
}

// An empty fixed-width table column takes over the pool blocks of a result
// column (values, and the bitmap when there is one) instead of allocating and
// copying: CREATE TABLE AS / INSERT ... SELECT into a new table then costs the
// query plus the zone-map pass.  A block is adopted at most once per append
// (SELECT x, x) and only when it starts at the column's pointer; string
// columns and blocks far larger than the rows still take the copy.
static bool AdoptResultColumn(DevColumn &c, const DCol &d, int64_t n, std::vector<const void *> &taken) {
  if (c.phys == P_STR || d.phys != c.phys || c.data || c.validity || c.capacity) return false;
  auto owner_of = [&](const void *p) -> DevBufPtr {
    if (!p) return nullptr;
    for (auto &o : d.owners)
      if (o && o->p == p && o->pool) return o;
    return nullptr;
  };
  DevBufPtr db = owner_of(d.data), vb = owner_of(d.validity);
  if (!db || (d.validity && !vb)) return false;
  for (const void *p : taken)
    if (p == db->p || (vb && p == vb->p)) return false;
  int64_t cap = (int64_t)(db->bytes / PhysSize(c.phys));
  if (vb) cap = std::min<int64_t>(cap, (int64_t)(vb->bytes / 8) * 64);
  // (a selective filter's output block is sized for every input row: keep at
  // most twice what the rows need, as Grow's doubling would)
  if (cap < n || db->bytes > 2 * (size_t)n * PhysSize(c.phys) + ((size_t)2 << 20)) return false;
  taken.push_back(db->p);
  c.data = db->p;
  c.data_owner = db;
  if (vb) {
    taken.push_back(vb->p);
    c.validity = (uint64_t *)vb->p;
    c.validity_owner = vb;
  }
  c.capacity = cap;
  return true;
}

static void AppendDRel(Engine &e, Table &t, const DRel &r, const std::vector<int> &col_map) {
  int64_t n = r.n, old = t.nrows;
  if (n <= 0) return;
  std::vector<const void *> taken;
  for (size_t tc = 0; tc < t.cols.size(); tc++) {
    DevColumn &c = t.cols[tc];
    int src = col_map[tc];
    if (old == 0 && src >= 0 && AdoptResultColumn(c, r.cols[src], n, taken)) {
      if (!FoldKernelStats(c, r.cols[src], n, true)) UpdateStats(e, c, 0, n, true);
      continue;
    }
    Grow(e, c, old, old + n);
    if (src < 0) {
      // column not provided: NULLs
      EnsureValidity(e, c, old);
      auto zeros = Alloc(e, Words64(n) * 8, true);
      dev::BitmapAppend(c.validity, old, (const uint64_t *)zeros->p, n, e.stream);
      if (c.phys == P_STR) {
        std::vector<int64_t> offs(n + 1, c.chars_len);
        // offsets already hold old entries; append n equal offsets
        HIPCHK(hipMemcpyAsync(c.offsets + old + 1, offs.data(), n * 8, hipMemcpyHostToDevice, e.stream));
      }
      HIPCHK(hipStreamSynchronize(e.stream));
      c.null_count += n;
      continue;
    }
    const DCol &d = r.cols[src];
    if (d.phys != c.phys) ThrowError("Internal", "append: physical type mismatch");
    if (c.phys == P_STR) {
      int64_t need = c.chars_len + d.chars_len;
      if (need > c.chars_cap) {
        int64_t cap = std::max<int64_t>(need, std::max<int64_t>(4096, c.chars_cap * 2));
        char *nc = nullptr;
        HIPCHK(hipMalloc(&nc, cap));
        if (c.chars_len) HIPCHK(hipMemcpyAsync(nc, c.chars, c.chars_len, hipMemcpyDeviceToDevice, e.stream));
        HIPCHK(hipStreamSynchronize(e.stream));
        c.chars_owner = DevOwned(e, nc);
        c.chars = nc;
        c.chars_cap = cap;
      }
      if (d.chars_len) HIPCHK(hipMemcpyAsync(c.chars + c.chars_len, d.chars, d.chars_len, hipMemcpyDeviceToDevice, e.stream));
      dev::RebaseOffsets(d.offsets + 1, c.offsets + old + 1, n, c.chars_len, e.stream);
      c.chars_len += d.chars_len;
    } else {
      int sz = PhysSize(c.phys);
      ProfScope ps(e, "append_copy", 2.0 * n * sz, n);
      HIPCHK(hipMemcpyAsync((char *)c.data + old * sz, d.data, (size_t)n * sz, hipMemcpyDeviceToDevice, e.stream));
    }
    if (d.validity) {
      EnsureValidity(e, c, old);
      dev::BitmapAppend(c.validity, old, d.validity, n, e.stream);
    } else if (c.validity) {
      dev::BitmapAppend(c.validity, old, nullptr, n, e.stream);
    }
    if (!FoldKernelStats(c, d, n, old == 0)) UpdateStats(e, c, old, n, old == 0);
  }
  HIPCHK(hipStreamSynchronize(e.stream));
  t.nrows = old + n;
  for (auto &c : t.cols) UpdateScanCodes(e, c, t.nrows);
}

static void AppendCast(Engine &e, Table &t, DRel r, const std::vector<int> &col_map);
static void ShardedInsertSelect(Connection &c, Table &t, const BoundSelect &s, const std::vector<int> &col_map);

void ExecuteInsertSelect(Connection &c, Table &t, const BoundSelect &s, const std::vector<int> &col_map) {
  if (t.sharded()) return ShardedInsertSelect(c, t, s, col_map);
  auto t0 = std::chrono::steady_clock::now();
  Engine &e = Eng(c);
  e.profile = c.opts.profile;  // the statement's kernels (query, append copy, zone map) become last_profile
  e.events.clear();
  e.ev_used = 0;
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
    struct Want {
      Engine &e;
      ~Want() { e.want_zone_maps = false; }
    } want{e};
    e.want_zone_maps = true;
    r = RunSelectDev(e, c, s);
  }
  AppendCast(e, t, r, col_map);
  FinishProfile(c, e, std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count());
}

// r's columns (col_map[table column] = column of r, or -1) cast to the table
// types on the device where they differ, then appended
static void AppendCast(Engine &e, Table &t, DRel r, const std::vector<int> &col_map) {
  // cast columns to the table types on device when they differ
  std::vector<BExprPtr> casts;
  bool need = false;
  for (size_t tc = 0; tc < t.cols.size(); tc++) {
    int src = col_map[tc];
    if (src < 0) continue;
    if (!(r.cols[src].type == t.cols[tc].type)) need = true;
  }
  if (need) {
    std::vector<BExprPtr> exprs;
    std::vector<int> map2(t.cols.size(), -1);
    for (size_t tc = 0; tc < t.cols.size(); tc++) {
      int src = col_map[tc];
      if (src < 0) continue;
      auto col = std::make_shared<BExpr>();
      col->kind = BExpr::COL;
      col->col = src;
      col->type = r.cols[src].type;
      BExprPtr x = col;
      if (!(col->type == t.cols[tc].type)) {
        auto cst = std::make_shared<BExpr>();
        cst->kind = BExpr::FUNC;
        cst->op = B_CAST;
        cst->type = t.cols[tc].type;
        cst->ch = {col};
        x = cst;
      }
      map2[tc] = (int)exprs.size();
      exprs.push_back(x);
    }
    r = FilterProject(e, r, nullptr, exprs);
    AppendDRel(e, t, r, map2);
  } else {
    AppendDRel(e, t, r, col_map);
  }
  CheckError(e);
}


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
  se.profile = top.opts.profile;
  se.events.clear();
  se.ev_used = 0;
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
  se.events.clear();
  se.ev_used = 0;
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

static int CompareValues(const Value &a, const Value &b) {  // non-NULL values of one type
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

static void KeyBytes(const Value &v, std::string &out) {
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
static ResultPtr ShardedAggregateHost(Connection &c, const BoundSelect &s) {
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

static DRel ShardedBranch(Engine &e, Connection &c, const BoundSelect &s) {
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
static int TargetPart(const Connection &c, const Table &t) {
  const int n = (int)t.parts.size();
  int last = 0;
  for (int i = 0; i < n; i++)
    if (t.parts[i]->nrows > 0) last = i;
  if (c.opts.shard_rows > 0 && t.parts[last]->nrows >= c.opts.shard_rows && last + 1 < n) return last + 1;
  return last;
}

static void SyncRows(Table &t) {
  int64_t n = 0;
  for (auto &p : t.parts) n += p->nrows;
  t.nrows = n;
}

static void ShardedInsertSelect(Connection &c, Table &t, const BoundSelect &s, const std::vector<int> &col_map) {
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

void EngineCounters(const Connection &c, int64_t out[3]) {
  if (c.engine) {
    out[0] += c.engine->sr_launches;
    out[1] += c.engine->sr_aborts;
    out[2] += c.engine->sr_launch_failures;
  }
  for (auto &sc : c.shards) EngineCounters(*sc, out);
}

void HbmCalibrateConn(Connection &c, int64_t bytes, int iters, double out[8]) {
  Engine &e = Eng(c);
  bytes &= ~(int64_t)1023;  // whole 1 KiB ring slots
  void *a = nullptr, *b = nullptr;
  HIPCHK(hipMalloc(&a, bytes));
  HIPCHK(hipMalloc(&b, bytes));
  HIPCHK(hipMemsetAsync(a, 1, bytes, e.stream));
  HIPCHK(hipMemsetAsync(b, 0, bytes, e.stream));
  dev::HbmCalibrate(a, b, bytes, iters, out, e.stream);
  HIPCHK(hipStreamSynchronize(e.stream));
  HIPCHK(hipFree(a));
  HIPCHK(hipFree(b));
}

int ClockStampsConn(Connection &c, uint64_t *out, int cap) {
  Engine &e = Eng(c);
  return dev::ReadClockStamps(out, cap, e.stream);
}

// memcpy split over a few host threads (one thread tops out near 10 GB/s)
static void ParallelMemcpy(void *dst, const void *src, size_t bytes) {
  const size_t kMinPart = (size_t)2 << 20;
  int nt = (int)std::min<size_t>(8, bytes / kMinPart);
  if (nt <= 1) {
    memcpy(dst, src, bytes);
    return;
  }
  std::vector<std::thread> th;
  size_t part = (bytes / nt + 63) & ~(size_t)63;
  for (int i = 0; i < nt; i++) {
    size_t b = (size_t)i * part;
    if (b >= bytes) break;
    size_t len = std::min(part, bytes - b);
    th.emplace_back([=] { memcpy((char *)dst + b, (const char *)src + b, len); });
  }
  for (auto &t : th) t.join();
}

// Host -> device through the pinned ring: slot k is refilled only after its
// previous DMA (event) has completed, so copy-in and DMA overlap.
static void StageH2D(Engine &e, void *dst, const void *src, size_t bytes) {
  // Default: hand the pageable source to the runtime's own staged DMA — 14.5
  // GB/s on the C4 ingest vs 12.6 for this ring with 8 copy threads
  // (MI355X box, 1e8 INT64 rows).  MBX_INGEST=staged selects the ring.
  const char *mode = Knob("MBX_INGEST");
  if (!mode || strcmp(mode, "staged") != 0) {
    HIPCHK(hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, e.stream));
    return;
  }
  if (!e.h_stage[0]) {
    for (int i = 0; i < Engine::kStageSlots; i++) {
      HIPCHK(hipHostMalloc((void **)&e.h_stage[i], Engine::kStageBytes, hipHostMallocDefault));
      HIPCHK(hipEventCreateWithFlags(&e.stage_ev[i], hipEventDisableTiming));
      HIPCHK(hipEventRecord(e.stage_ev[i], e.stream));
    }
  }
  size_t done = 0;
  int slot = 0;
  while (done < bytes) {
    size_t b = std::min(Engine::kStageBytes, bytes - done);
    HIPCHK(hipEventSynchronize(e.stage_ev[slot]));
    ParallelMemcpy(e.h_stage[slot], (const char *)src + done, b);
    HIPCHK(hipMemcpyAsync((char *)dst + done, e.h_stage[slot], b, hipMemcpyHostToDevice, e.stream));
    HIPCHK(hipEventRecord(e.stage_ev[slot], e.stream));
    done += b;
    slot = (slot + 1) % Engine::kStageSlots;
  }
}

// Bulk appender (duckdb_mbx_append_column / _commit): every column arrives in
// its physical layout and is DMA'd straight to its place at the table's end
// (no intermediate device relation, no D2D append copy).
void AppendRawColumns(Connection &c, Table &t, const std::vector<const void *> &vals,
                      const std::vector<const uint8_t *> &valid, int64_t n, bool sync) {
  if (t.sharded()) {  // into the target part(s), split where a part fills up
    // the caller reuses the buffer of its previous flush once this returns, and
    // that flush may have gone to another shard's stream: settle every shard
    // (Eng of the target shard alone would wait only for its own stream)
    SettleAppends(c);
    int64_t off = 0;
    while (off < n) {
      const int k = TargetPart(c, t);
      int64_t m = n - off;
      if (c.opts.shard_rows > 0 && k + 1 < (int)t.parts.size())
        m = std::min<int64_t>(m, std::max<int64_t>(1, c.opts.shard_rows - t.parts[k]->nrows));
      std::vector<const void *> v2;
      std::vector<const uint8_t *> b2;
      for (size_t tc = 0; tc < t.cols.size(); tc++) {
        v2.push_back((const char *)vals[tc] + (size_t)off * PhysSize(t.cols[tc].phys));
        b2.push_back(valid[tc] ? valid[tc] + off : nullptr);
      }
      AppendRawColumns(*c.shards[k], *t.parts[k], v2, b2, m, sync);
      off += m;
      SyncRows(t);
    }
    return;
  }
  Engine &e = Eng(c);
  const int64_t old = t.nrows;
  if (n <= 0) return;
  for (size_t tc = 0; tc < t.cols.size(); tc++)
    if (t.cols[tc].phys == P_STR || t.cols[tc].phys == P_INTERVAL)
      ThrowError("Invalid Input", "append_column: only fixed-width columns are supported");
  for (size_t tc = 0; tc < t.cols.size(); tc++) {
    DevColumn &col = t.cols[tc];
    Grow(e, col, old, old + n);
    const int sz = PhysSize(col.phys);
    StageH2D(e, (char *)col.data + (size_t)old * sz, vals[tc], (size_t)n * sz);
    const uint8_t *vb = valid[tc];
    if (vb && memchr(vb, 0, (size_t)n) != nullptr) {
      std::vector<uint64_t> bm(Words64(n), 0);
      for (int64_t i = 0; i < n; i++)
        if (vb[i]) bm[i >> 6] |= 1ull << (i & 63);
      auto tmp = Alloc(e, bm.size() * 8);
      HIPCHK(hipMemcpyAsync(tmp->p, bm.data(), bm.size() * 8, hipMemcpyHostToDevice, e.stream));
      EnsureValidity(e, col, old);
      dev::BitmapAppend(col.validity, old, (const uint64_t *)tmp->p, n, e.stream);
      HIPCHK(hipStreamSynchronize(e.stream));  // bm / tmp lifetime
    } else if (col.validity) {
      dev::BitmapAppend(col.validity, old, nullptr, n, e.stream);
    }
    UpdateStats(e, col, old, n, old == 0, !sync);
  }
  t.nrows = old + n;
  if (!sync) {  // DMA + stats in flight; SettlePending waits for them and folds the stats
    e.inflight_h2d = true;
    return;
  }
  HIPCHK(hipStreamSynchronize(e.stream));
  for (auto &col : t.cols) UpdateScanCodes(e, col, t.nrows);
  CheckError(e);
}

void SettleAppends(Connection &c) {
  if (c.engine && c.engine->has_gpu) SettlePending(*c.engine);
  for (auto &sc : c.shards) SettleAppends(*sc);
}

void *HostPinnedAlloc(size_t bytes) {
  void *p = nullptr;
  HIPCHK(hipHostMalloc(&p, bytes ? bytes : 16, hipHostMallocPortable));  // any device of the process
  return p;
}
void HostPinnedFree(void *p) {
  if (p) (void)hipHostFree(p);
}

void AppendHostBatch(Connection &c, Table &t, const HostBatch &b) {
  if (t.sharded()) {
    const int k = TargetPart(c, t);
    AppendHostBatch(*c.shards[k], *t.parts[k], b);
    SyncRows(t);
    return;
  }
  Engine &e = Eng(c);
  DRel r;
  r.n = b.nrows;
  std::vector<int> map;
  for (size_t i = 0; i < b.cols.size(); i++) {
    DCol d;
    UploadHostColumn(e, b.cols[i], b.nrows, d);
    r.cols.push_back(d);
    map.push_back((int)i);
  }
  AppendDRel(e, t, r, map);
}

}  // namespace mbx
