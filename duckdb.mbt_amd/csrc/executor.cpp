// executor.cpp — runs bound plans on the MI355X.
//
// Does the work of a query for the recognised shapes: scan -> filter ->
// project -> aggregate -> sort over device-resident column chunks.  Every pass
// over table rows is a kernel in kernels.hip; the host only plans, allocates
// and copies the (small) final result back.  There is no CPU execution path:
// without a device, any plan that touches rows raises.
//
// This unit holds the engine and its pool, uploads, the filter / project /
// select pipeline, sort, concat, the copies to the host and the statement
// entry points; aggregate.cpp the aggregation paths, ingest.cpp table growth
// and appends, sharded.cpp the multi-device plans (exec.h is what they share).
#include <algorithm>
#include <array>
#include <atomic>
#include <chrono>
#include <type_traits>
#include <cmath>
#include <condition_variable>
#include <functional>
#include <limits>
#include <unordered_map>
#include <sstream>
#include <thread>

#include "exec.h"
#include "jit.h"
#include "join_mark_plan.h"
#include "join_plan.h"
#include "hostlink.h"
#include "vm_compile.h"
#include "knobs.h"

namespace mbx {

int DeviceCount() {
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess) return 0;
  return n;
}

// scratch for the device helpers (hipcub temp storage, hash flags) from the
// calling connection's pool
static thread_local DevicePool *g_temp_pool = nullptr;
void *dev::TempAlloc(size_t bytes) {
  if (!g_temp_pool) throw std::runtime_error("device scratch allocator not set");
  void *p = g_temp_pool->Get(DevicePool::Bucket(bytes ? bytes : 16));
  if (!p) throw std::runtime_error("device scratch allocation failed");
  return p;
}
void dev::TempFree(void *ptr, size_t bytes) {
  if (ptr && g_temp_pool) g_temp_pool->Put(DevicePool::Bucket(bytes ? bytes : 16), ptr);
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
  g_temp_pool = e->pool.get();
  HIPCHK(hipMalloc(&e->d_err, 256));
  HIPCHK(hipMalloc(&e->d_scratch, 4096));
  HIPCHK(hipMalloc(&e->d_small, 1 << 16));
  HIPCHK(hipMalloc(&e->d_partials, sizeof(dev::AggPartial) * dev::kMaxAggPartials));
  HIPCHK(hipMemset(e->d_err, 0, 256));
  e->h_pinned_bytes = 1 << 20;
  HIPCHK(hipHostMalloc((void **)&e->h_pinned, e->h_pinned_bytes, hipHostMallocDefault));
  HIPCHK(hipHostMalloc((void **)&e->h_mapped, Engine::kMappedBytes, hipHostMallocCoherent | hipHostMallocMapped));
  memset(e->h_mapped, 0, Engine::kMappedBytes);  // the ticket word reads 0, which no statement's ticket is
  e->has_gpu = true;
  return e;
}

// n appended rows, nvalid of them non-NULL with values in [mn, mx], folded
// into the column's zone map
void FoldStats(DevColumn &c, int64_t n, int64_t nvalid, i128 mn, i128 mx, bool first_rows) {
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

// folds the zone-map statistics of in-flight appends into their columns
// (after the stream has drained: their DMAs and reductions are done), then
// brings the columns' code images up to the appended rows
void SettlePending(Engine &e) {
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

Engine &Eng(Connection &c) {
  Engine &e = *c.engine;
  if (!e.has_gpu)
    ThrowError("IO", "this statement reads table rows and needs the MI355X device, but no GPU is available");
  hipSetDevice(e.device);
  g_temp_pool = e.pool.get();
  e.scan_codes = c.opts.scan_codes;
  e.scan_codes_min_rows = c.opts.scan_codes_min_rows;
  e.scan_codes_bits_min_rows = c.opts.scan_codes_bits_min_rows;
  e.scan_codes_planes_min_rows = c.opts.scan_codes_planes_min_rows;
  e.scan_hist = c.opts.scan_hist;
  e.scan_hist_min_rows = c.opts.scan_hist_min_rows;
  e.scan_hist_host = c.opts.scan_hist_host;
  e.scan_hist_host_min_rows = c.opts.scan_hist_host_min_rows;
  e.result_tail = c.opts.result_tail;
  e.tail_spin_ns = c.opts.tail_spin_us * 1000;
  SettlePending(e);  // a statement never sees a column before its appended stats
  return e;
}

DevBufPtr Alloc(Engine &e, size_t bytes, bool zero) {
  auto b = std::make_shared<DevBuf>();
  if (bytes == 0) bytes = 16;
  b->bytes = DevicePool::Bucket(bytes);
  b->pool = e.pool;
  b->p = e.pool->Get(b->bytes);
  if (!b->p) ThrowError("Out of Memory", "device allocation of " + std::to_string(b->bytes) + " bytes failed");
  if (zero) HIPCHK(hipMemsetAsync(b->p, 0, b->bytes, e.stream));
  return b;
}

DCol ColFromTable(const DevColumn &c) {
  DCol d;
  for (const auto *o : {&c.data_owner, &c.validity_owner, &c.offsets_owner, &c.chars_owner, &c.codes_owner,
                        &c.code_hist_owner})
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


void CheckError(Engine &e) {
  // through the pinned arena: a pageable destination would take HIP's staged copy
  HIPCHK(hipMemcpyAsync(e.h_pinned, e.d_err, sizeof(int32_t), hipMemcpyDeviceToHost, e.stream));
  HIPCHK(hipStreamSynchronize(e.stream));
  int32_t err;
  memcpy(&err, e.h_pinned, sizeof(err));
  RaiseDeviceError(e, err);
}

void RaiseDeviceError(Engine &e, int32_t err) {
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
      case E_JOIN_FULL: ThrowError("Internal", "join table full");
      default: ThrowError("Out of Range", "Decimal value out of range");
    }
  }
}

// a row count left on the device (DRel::n_dev) read back
void SettleCount(Engine &e, DRel &r) {
  if (!r.n_dev) return;
  r.n = ReadDev<int64_t>(e, r.n_dev);
  r.n_dev = nullptr;
  r.n_owner.reset();
}

// ---------------------------------------------------------------------------
// host -> device upload of constant rows (VALUES, host-constant subqueries)
// ---------------------------------------------------------------------------
void UploadHostColumn(Engine &e, const HostColumn &hc, int64_t n, DCol &d) {
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

DRel UploadRows(Engine &e, const std::vector<std::vector<Value>> &rows, const std::vector<LogicalType> &types) {
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

DCol AllocOut(Engine &e, const LogicalType &t, int64_t n, bool with_valid, bool zero_valid) {
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

// ---------------------------------------------------------------------------
// VARCHAR predicates: lowered to BOOLEAN columns before the expression VM
// ---------------------------------------------------------------------------
// The VM has no string instructions.  A string predicate leaf -- a comparison
// of a VARCHAR column with a VARCHAR constant (either order) or with another
// VARCHAR column of the relation, B_LIKE, prefix / suffix / contains with a
// constant -- is evaluated by the str_match kernels (str_kernels.hip) into a
// one-byte-per-row BOOLEAN column appended to a copy of the relation, and the
// tree is rebuilt with a reference to that column in the leaf's place.  The
// bound plan itself is never changed: a prepared statement patches new
// constants into its nodes, and the next execute must read them here.
//
// x IN (subquery) is the same kind of leaf.  The subquery runs once per
// statement and its non-NULL keys go into the join's table (MarkSetOf); the
// left operand becomes a key column the way a join key does, and
// join_probe_mark writes the mark's byte and, where join_mark_plan.h asks for
// one, its validity.  NOT IN is the VM's NOT over that column.
namespace {

// the same tree: kinds, types, columns, constants, and the subqueries of membership leaves
bool SameTree(const BExpr &a, const BExpr &b) {
  if (a.kind != b.kind || a.type != b.type) return false;
  if (a.kind == BExpr::COL) return a.col == b.col;
  if (a.kind == BExpr::CONST)
    return a.cval.is_null == b.cval.is_null && (a.cval.is_null || FormatValue(a.cval) == FormatValue(b.cval));
  if (a.op != b.op || a.ch.size() != b.ch.size() || (bool)a.sub != (bool)b.sub) return false;
  for (size_t i = 0; i < a.ch.size(); i++)
    if (!SameTree(*a.ch[i], *b.ch[i])) return false;
  return !a.sub || a.sub == b.sub || BoundSelectEq(*a.sub, *b.sub);
}

// The set of a membership subquery in the running statement: the subquery is
// run and its table built the first time any leaf asks, whichever lowering
// that is in.  (By value: a nested subquery's set may be added meanwhile.)
Engine::MarkSet MarkSetOf(Engine &e, const std::shared_ptr<BoundSelect> &sub) {
  if (!e.mark_conn) ThrowError("Internal", "an IN (subquery) leaf outside a statement's run");
  for (auto &m : e.mark_sets)
    if (m.sub == sub) return m;
  for (auto &m : e.mark_sets)
    if (BoundSelectEq(*m.sub, *sub)) return m;
  Engine::MarkSet m;
  m.sub = sub;
  DRel r = RunSelectDev(e, *e.mark_conn, *sub);
  m.rows = r.n;
  if (r.n > 0) {
    auto k = std::make_shared<BExpr>();
    k->kind = BExpr::COL;
    k->col = 0;
    k->type = r.cols[0].type;
    const JoinTable t = JoinBuildTable(e, KeyColumn(e, r, k), r.n);
    m.nulls = t.nulls;
    m.tab = t.tab;
    m.cap = t.tab ? t.cap : 0;
  }
  e.mark_sets.push_back(m);
  return m;
}

bool IsStrColumn(const DRel &rel, const BExpr &x) {
  return x.kind == BExpr::COL && x.col >= 0 && x.col < (int)rel.cols.size() && !(rel.range && x.col == 0) &&
         rel.cols[x.col].phys == P_STR && (rel.n == 0 || rel.cols[x.col].offsets) && ClassOf(x.type) == VC_STR;
}
bool IsStrConst(const BExpr &x) { return x.kind == BExpr::CONST && (ClassOf(x.type) == VC_STR || x.cval.is_null); }

bool IsStrLeaf(const DRel &rel, const BExpr &x) {
  if (x.kind != BExpr::FUNC) return false;
  switch (x.op) {
    case B_EQ: case B_NE: case B_LT: case B_LE: case B_GT: case B_GE: case B_DISTINCT: case B_NOT_DISTINCT: {
      if (x.ch.size() != 2 || ClassOf(x.ch[0]->type) != VC_STR) return false;
      const bool lc = IsStrColumn(rel, *x.ch[0]), rc = IsStrColumn(rel, *x.ch[1]);
      return (lc && (rc || IsStrConst(*x.ch[1]))) || (rc && IsStrConst(*x.ch[0]));
    }
    case B_LIKE: case B_PREFIX: case B_SUFFIX: case B_CONTAINS: {
      if (x.ch.size() < 2 || !IsStrColumn(rel, *x.ch[0])) return false;
      for (size_t i = 1; i < x.ch.size(); i++)
        if (!IsStrConst(*x.ch[i])) return false;
      return true;
    }
    default:
      return false;
  }
}

// the same leaf: operator, columns and constant bytes
bool SameStrLeaf(const BExpr &a, const BExpr &b) {
  if (a.op != b.op || a.ch.size() != b.ch.size()) return false;
  for (size_t i = 0; i < a.ch.size(); i++) {
    const BExpr &x = *a.ch[i], &y = *b.ch[i];
    if (x.kind != y.kind) return false;
    if (x.kind == BExpr::COL ? x.col != y.col : (x.cval.is_null != y.cval.is_null || x.cval.s != y.cval.s)) return false;
  }
  return true;
}

BExprPtr BoolConst(bool v, bool is_null) {
  auto c = std::make_shared<BExpr>();
  c->kind = BExpr::CONST;
  c->type = LogicalType(T_BOOLEAN);
  c->cval = is_null ? Value::Null(c->type) : Value::Bool(v);
  return c;
}
BExprPtr BoolFunc(BOp op, std::vector<BExprPtr> ch) {
  auto f = std::make_shared<BExpr>();
  f->kind = BExpr::FUNC;
  f->op = op;
  f->type = LogicalType(T_BOOLEAN);
  f->ch = std::move(ch);
  return f;
}

dev::StrCol StrColOf(const DCol &c) { return {c.offsets, c.chars, c.chars_len, c.validity}; }

// MBX_STR_GLOBAL=1: every step of str_match reads its rows from global memory
// (the A/B of tools/str_match_bench.py); read per launch so one process can alternate
bool StrGlobalForm() {
  const char *k = Knob("MBX_STR_GLOBAL");
  return k && k[0] == '1';
}

struct StrLowering {
  Engine &e;
  const DRel &rel;
  DRel out;  // rel + the BOOLEAN columns, once a leaf was lowered
  bool lowered = false;
  std::vector<std::pair<BExprPtr, BExprPtr>> done;  // leaf -> its replacement

  StrLowering(Engine &en, const DRel &r) : e(en), rel(r) {}

  // a BOOLEAN column for the kernels to fill; `share` lends its validity words
  // (and what keeps them alive), so the result is NULL where that input is
  DCol NewBool(const DCol *share) {
    DCol d = AllocOut(e, LogicalType(T_BOOLEAN), rel.n, false);
    if (share && share->validity) {
      d.validity = share->validity;
      d.owners.insert(d.owners.end(), share->owners.begin(), share->owners.end());
      d.pins.insert(d.pins.end(), share->pins.begin(), share->pins.end());
    }
    return d;
  }
  BExprPtr Append(const DCol &d) {
    if (!lowered) {
      out = rel;
      lowered = true;
    }
    out.cols.push_back(d);
    auto c = std::make_shared<BExpr>();
    c->kind = BExpr::COL;
    c->col = (int)out.cols.size() - 1;
    c->type = LogicalType(T_BOOLEAN);
    return c;
  }
  void Match(const StrMatchPlan &plan, const DCol &c, DCol &d) {
    ProfScope ps(e, "str_match", (double)rel.n * 9 + (double)c.chars_len, rel.n);
    dev::StrMatch(plan, StrColOf(c), rel.n, (uint8_t *)d.data, StrGlobalForm(), e.stream);
  }

  BExprPtr Leaf(const BExpr &x) {
    const bool distinct = x.op == B_DISTINCT || x.op == B_NOT_DISTINCT;
    if (x.op == B_LIKE || x.op == B_PREFIX || x.op == B_SUFFIX || x.op == B_CONTAINS) {
      for (size_t i = 1; i < x.ch.size(); i++)
        if (x.ch[i]->cval.is_null) return BoolConst(false, true);
      StrMatchPlan plan;
      PlanStringMatch(x, &plan);
      const DCol &c = rel.cols[x.ch[0]->col];
      if (plan.form == SF_ALL) {  // true for every non-NULL row: nothing to launch
        if (!c.validity) return BoolConst(true, false);
        return BoolFunc(B_CASE, {BoolFunc(B_ISNOTNULL, {x.ch[0]}), BoolConst(true, false)});
      }
      DCol d = NewBool(&c);
      Match(plan, c, d);
      return Append(d);
    }
    const bool lc = x.ch[0]->kind == BExpr::COL, rc = x.ch[1]->kind == BExpr::COL;
    const uint8_t op = x.op == B_EQ ? SM_EQ : x.op == B_NE ? SM_NE : x.op == B_LT ? SM_LT : x.op == B_LE ? SM_LE
                       : x.op == B_GT ? SM_GT : x.op == B_GE ? SM_GE : x.op == B_DISTINCT ? SM_DISTINCT : SM_NOT_DISTINCT;
    if (lc && rc) {
      const DCol &a = rel.cols[x.ch[0]->col], &b = rel.cols[x.ch[1]->col];
      const bool both = a.validity && b.validity && !distinct;
      DCol d = NewBool(distinct || both ? nullptr : a.validity ? &a : &b);
      if (both) {
        auto v = Alloc(e, Words64(std::max<int64_t>(rel.n, 1)) * 8);
        d.validity = (uint64_t *)v->p;
        d.owners.push_back(v);
      }
      ProfScope ps(e, "str_match", (double)rel.n * 17 + (double)a.chars_len + (double)b.chars_len, rel.n);
      dev::StrCompareCols(op, StrColOf(a), StrColOf(b), rel.n, (uint8_t *)d.data, both ? d.validity : nullptr, e.stream);
      return Append(d);
    }
    const BExprPtr &colx = lc ? x.ch[0] : x.ch[1];
    const BExpr &k = lc ? *x.ch[1] : *x.ch[0];
    if (k.cval.is_null) {
      // x <op> NULL is NULL; IS [NOT] DISTINCT FROM NULL is the column's NULL test
      if (!distinct) return BoolConst(false, true);
      return BoolFunc(x.op == B_DISTINCT ? B_ISNOTNULL : B_ISNULL, {colx});
    }
    StrMatchPlan plan;
    if (PlanStrCompare(lc ? op : StrFlipOp(op), (const uint8_t *)k.cval.s.data(), (int64_t)k.cval.s.size(), &plan) != SP_OK)
      ThrowError("Not implemented", "a VARCHAR comparison with a constant of more than " + std::to_string(kStrMatchCap) +
                                        " bytes is not supported by the MI355X backend");
    const DCol &c = rel.cols[colx->col];
    DCol d = NewBool(distinct ? nullptr : &c);
    Match(plan, c, d);
    return Append(d);
  }

  // x IN (subquery): the mark column (join_mark_plan.h)
  BExprPtr MarkLeaf(const BExpr &x) {
    const Engine::MarkSet set = MarkSetOf(e, x.sub);
    JoinMarkFacts f;
    f.set_rows = set.rows;
    f.set_nulls = set.nulls;
    if (JoinMarkDecide(f).constant_false) {  // FALSE for every row, a NULL key included: nothing to launch
      const JoinMarkCellValue c = JoinMarkCell(false, false, true, false);
      return BoolConst(c.value != 0, !c.valid);
    }
    const DCol key = KeyColumn(e, rel, x.ch[0]);
    if (key.phys > P_U64) ThrowError("Internal", "IN (subquery) key is not stored as an integer");
    f.probe_nullable = key.validity != nullptr;
    const JoinMarkPlan plan = JoinMarkDecide(f);
    DCol d = NewBool(nullptr);
    if (plan.validity) {
      auto v = Alloc(e, Words64(std::max<int64_t>(rel.n, 1)) * 8);
      d.validity = (uint64_t *)v->p;
      d.owners.push_back(v);
    }
    // per row: the key, one 16-B entry, the mark's byte and its validity bit
    ProfScope ps(e, "join_probe_mark",
                 (double)rel.n * (PhysSize(key.phys) + sizeof(JoinEntry) + 1 + (plan.validity ? 1.0 / 8 : 0)), rel.n);
    dev::JoinProbeMark(key.data, key.phys, key.validity, rel.n, plan.lookup ? (const JoinEntry *)set.tab->p : nullptr,
                       plan.lookup ? set.cap : 0, plan.set_has_null, (uint8_t *)d.data, d.validity, e.d_err, e.stream);
    return Append(d);
  }

  BExprPtr Rewrite(const BExprPtr &x) {
    if (!x || x->kind != BExpr::FUNC) return x;
    if (x->op == B_IN_SUBQUERY && x->sub) {
      for (auto &p : done)
        if (p.first->op == B_IN_SUBQUERY && SameTree(*p.first, *x)) return p.second;
      BExprPtr r = MarkLeaf(*x);
      done.push_back({x, r});
      return r;
    }
    if (IsStrLeaf(rel, *x)) {
      for (auto &p : done)
        if (p.first->op != B_IN_SUBQUERY && SameStrLeaf(*p.first, *x)) return p.second;
      BExprPtr r = Leaf(*x);
      done.push_back({x, r});
      return r;
    }
    std::vector<BExprPtr> ch;
    bool changed = false;
    for (auto &c : x->ch) {
      ch.push_back(Rewrite(c));
      changed |= ch.back() != c;
    }
    if (!changed) return x;
    auto n = std::make_shared<BExpr>(*x);
    n->ch = std::move(ch);
    return n;
  }
};

}  // namespace

bool LowerStringPredicates(Engine &e, const DRel &rel, std::vector<BExprPtr> &trees, DRel &lowered) {
  if (rel.n_dev) return false;  // only a column passthrough may follow (FilterProject)
  StrLowering low(e, rel);
  std::vector<BExprPtr> out;
  bool changed = false;
  for (auto &t : trees) {
    out.push_back(low.Rewrite(t));
    changed |= out.back() != t;
  }
  if (!changed) return false;
  trees = std::move(out);
  lowered = low.lowered ? low.out : rel;
  return true;
}

static bool TryFilterCompact(Engine &e, const DRel &rel, const BExpr &pred, const std::vector<BExprPtr> &exprs,
                             DRel &out);

// Evaluates `pred` (may be null) and `exprs` over `rel`; returns the
// projected relation of the selected rows.
DRel FilterProject(Engine &e, const DRel &rel, const BExprPtr &pred, const std::vector<BExprPtr> &exprs) {
  {  // VARCHAR predicates become BOOLEAN columns of a copy of rel first
    std::vector<BExprPtr> trees = exprs;
    trees.push_back(pred);
    DRel low;
    if (LowerStringPredicates(e, rel, trees, low)) {
      const BExprPtr p = trees.back();
      trees.pop_back();
      return FilterProject(e, low, p, trees);
    }
  }
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
    out.tail = rel.tail;  // (ToHost compares the columns with it)
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
        if (jit::VmFilter(vc.P, vc.cols, n, rel.rs, rel.rstep, (uint64_t *)bits->p, (uint32_t *)counts->p, e.d_err,
                          e.stream))
          ps.Rename("jit_filter");  // the specialised kernel ran, not the interpreter
        else
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
      if (jit::VmProject(vc.P, vc.cols, n, rel.rs, rel.rstep, bits ? (const uint64_t *)bits->p : nullptr,
                     offs ? (const int64_t *)offs->p : nullptr, vo, e.d_err, e.stream))
        ps.Rename("jit_project");
      else
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
const BExpr *StripWidening(const BExpr *x) {
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

bool RangePredicate(const BExpr &p, int *col, i128 *lo, i128 *hi) {
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
bool RangeConj(const BExpr &p, std::map<int, std::pair<i128, i128>> &ranges) {
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

bool FastIntCol(const DRel &rel, int c) {
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
  const int64_t chunks = dev::CountChunks(n);
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

// ---------------------------------------------------------------------------
// sort, limit, union
// ---------------------------------------------------------------------------
DRel GatherRel(Engine &e, const DRel &r, const int64_t *perm, int64_t n) {
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

// The stable permutation that sorts r by `order` (whose expressions are
// columns of r); null when there is nothing to sort: the identity.
DevBufPtr SortPerm(Engine &e, const DRel &r, const std::vector<BoundOrder> &order) {
  int64_t n = r.n;
  if (n <= 1 || order.empty()) return nullptr;
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
      // (a column of empty strings and NULLs only has offsets and no character buffer: no chunk pass runs)
      if (!c.offsets || (!c.chars && c.chars_len > 0))
        ThrowError("Internal", "ORDER BY VARCHAR without materialised strings");
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
  return perm;
}

static DRel SortRel(Engine &e, const DRel &r, const std::vector<BoundOrder> &order) {
  DevBufPtr perm = SortPerm(e, r, order);
  if (!perm) return r;
  DRel out = GatherRel(e, r, (const int64_t *)perm->p, r.n);
  HIPCHK(hipStreamSynchronize(e.stream));
  return out;
}

DRel ConcatRels(Engine &e, std::vector<DRel> &parts) {
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
  const int64_t w0 = start >> 6, w1 = (start + n + 63) >> 6;
  std::vector<int> cell(ncols);
  std::unique_ptr<bool[]> has_valid(new bool[ncols ? ncols : 1]);
  std::vector<ResultColLayout> lay(ncols);
  for (size_t c = 0; c < ncols; c++) {
    const DCol &d = r.cols[c];
    if (d.phys == P_STR) return nullptr;
    cell[c] = PhysSize(d.phys);
    has_valid[c] = d.validity != nullptr;
  }
  const size_t cols_end =
      ResultBufferLayout(ncols, cell.data(), has_valid.get(), n, w1 - w0, count_dev != nullptr, lay.data());
  size_t need = cols_end;
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
  const bool mapped =
      tj.empty() && ResultFitsMapped(need, ncols, Engine::kMappedBytes, HOSTCOPY_MAX, Knob("MBX_NO_HOSTCOPY"));
  // the emit of a one-row aggregate already stored this very relation, whole,
  // in the mapped buffer (EmitOneRow): nothing is left to copy
  bool tail = mapped && r.tail && r.tail->serial == e.tail_serial && r.tail->ncols == ncols && start == 0 && n == 1 &&
              !count_dev;
  for (size_t c = 0; tail && c < ncols; c++)
    tail = r.cols[c].data == r.tail->data[c] && r.cols[c].validity == r.tail->valid[c] &&
           lay[c].data_off == r.tail->off[c].data_off && lay[c].valid_off == r.tail->off[c].valid_off;
  // a relation the host itself filled (the histogram's host answer) is in the
  // mapped buffer and nowhere else: its device columns were never written
  const bool host_filled = r.tail && r.tail->host_filled;
  if (host_filled && !tail)
    ThrowError("Internal", "a host-filled relation reached the host by another way than its tail");
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
  // [0, 4): error word; [64, 72): the device row count (count_dev); then the columns (result_tail.h)
  if (!mapped) HIPCHK(hipMemcpyAsync(H, e.d_err, 4, hipMemcpyDeviceToHost, e.stream));
  if (count_dev) seg(count_dev, 64, 8);
  for (size_t c = 0; c < ncols; c++) {
    const DCol &d = r.cols[c];
    const int sz = PhysSize(d.phys);
    size_t bytes = (size_t)n * sz;
    data_off[c] = lay[c].data_off;
    valid_off[c] = lay[c].valid_off;
    if (tail) continue;
    if (bytes && direct) {
      dcols[c].data.resize(bytes);  // (ResultAlloc: no zero fill)
      HIPCHK(hipMemcpyAsync(dcols[c].data.data(), (const char *)d.data + (size_t)start * sz, bytes,
                            hipMemcpyDeviceToHost, e.stream));
    } else if (bytes) {
      seg((const char *)d.data + (size_t)start * sz, data_off[c], bytes);
    }
    if (d.validity && n > 0) seg(d.validity + w0, valid_off[c], (size_t)(w1 - w0) * 8);
  }
  size_t at = cols_end;
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
  if (tail) {
    if (!host_filled) e.tail_results++;  // (the host's own rows: duckdb_mbx_scan_hist_host_stats)
  } else if (mapped) {
    hd.err_src = e.d_err;
    hd.err_dst = (int32_t *)H;
    dev::HostCopy(hd, e.stream);
    e.hostcopy_results++;
  }
  if (host_filled) {
    // nothing ran, so there is nothing to wait for: no ticket was taken, and
    // the stream is not draining on this statement's account
  } else if (tail) {
    // the row's ticket, not the stream: the emit stored it last, with release
    // (tail_wait.h); the error word and the cells are read only after it
    const uint64_t *tk = (const uint64_t *)(H + kTailTicketOffset);
    const TailWaitOutcome w = TailWait(
        r.tail->ticket, e.tail_spin_ns, [&] { return __atomic_load_n(tk, __ATOMIC_ACQUIRE); },
        [] {
          return (int64_t)std::chrono::duration_cast<std::chrono::nanoseconds>(
                     std::chrono::steady_clock::now().time_since_epoch())
              .count();
        },
        [&] { HIPCHK(hipStreamSynchronize(e.stream)); }, e.tail_wait);
    if (w == TailWaitOutcome::kLost) ThrowError("Internal", "the result tail's ticket did not arrive with the stream");
    e.stream_draining = w == TailWaitOutcome::kPolled;
  } else {
    HIPCHK(hipStreamSynchronize(e.stream));
  }
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

ResultPtr ToHost(Engine &e, const DRel &r, const std::vector<std::string> &names, int64_t offset, int64_t limit,
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
  if (r.tail && r.tail->host_filled)
    ThrowError("Internal", "a host-filled relation reached the host by another way than its tail");
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
DRel SourceRel(Engine &e, Connection &c, const BoundSource &src) {
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
    case BoundSource::JOIN:
      r = JoinRel(e, c, src);
      break;
  }
  return r;
}

DRel RunBranch(Engine &e, Connection &c, const BoundSelect &s) {
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
  // a global aggregate over a join: fused into the probe where it can be (join.cpp)
  if (s.is_agg && s.groups.empty() && s.src.kind == BoundSource::JOIN)
    return FilterProject(e, JoinAggregate(e, c, s), s.having, s.outputs);
  DRel src = SourceRel(e, c, s.src);
  if (s.is_agg) {
    DRel agg = Aggregate(e, src, s);
    return FilterProject(e, agg, s.having, s.outputs);
  }
  if (!s.windows.empty()) return WindowBranch(e, s, src);
  return FilterProject(e, src, s.where, s.outputs);
}

size_t VisibleCols(const BoundSelect &s) {
  size_t n = 0;
  for (auto &nm : s.names)
    if (nm.rfind("__order_", 0) != 0) n++;
  return n;
}

// top: the statement's own result (handed to the host or kept as a device
// result), not a subquery's or an INSERT's input
DRel RunSelectDev(Engine &e, Connection &c, const BoundSelect &s, bool top) {
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
ResultPtr HostConstantSelect(const BoundSelect &s) {
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

void FinishProfile(Connection &c, Engine &e, double total_ms) {
  const bool draining = e.stream_draining;
  e.stream_draining = false;
  if (!e.profile) {
    QueryProfile &p = c.last_profile;
    p.kernels.clear();
    p.total_ms = total_ms;
    e.shard_kernels.clear();
    return;
  }
  // the statement's events and its shards' times wait with the engine, their
  // event pairs out of circulation, until SettleProfile reads them
  SettleProfile(c, e);  // (nothing is pending where the statement began with BeginProfile; else keep the order)
  Engine::PendingProfile pp;
  pp.events.swap(e.events);
  pp.shard_kernels.swap(e.shard_kernels);
  e.pending_prof.push_back(std::move(pp));
  e.ev_ledger.Defer();
  c.last_profile.kernels.clear();
  c.last_profile.total_ms = total_ms;
  // a statement that ended in a stream wait reads its times at once, as ever;
  // one that returned on its ticket leaves the closing event to run out behind it
  if (!draining) SettleProfile(c, e);
}

void SettleProfile(Connection &c, Engine &e) {
  if (e.pending_prof.empty()) return;
  QueryProfile &p = c.last_profile;
  for (size_t i = e.pending_prof.size(); i-- > 0;)  // the last event recorded: every other one is before it on the stream
    if (!e.pending_prof[i].events.empty()) {
      hipEventSynchronize(e.pending_prof[i].events.back().b);
      break;
    }
  for (auto &pp : e.pending_prof) {
    p.kernels.clear();
    for (auto &ev : pp.events) {
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
    for (auto &k : pp.shard_kernels) {
      p.kernels.push_back(k);
      if (c.profile_history.size() < 100000) c.profile_history.push_back(k);
    }
  }
  e.pending_prof.clear();
  e.ev_ledger.Settle([](uint64_t, size_t) {});
}

// A statement begins: what earlier ones left pending is read first (their
// event pairs come back), then the engine's events start empty.
void BeginProfile(Connection &c, Engine &e) {
  SettleProfile(c, e);
  e.profile = c.opts.profile;
  e.stream_draining = false;
  e.ResetEvents();
}

ResultPtr ExecuteSelect(Connection &c, const BoundSelect &s) {
  auto t0 = std::chrono::steady_clock::now();
  if (IsHostConstantSelect(s)) {
    ResultPtr r = HostConstantSelect(s);
    SettleConnProfile(c);  // (an earlier statement's pending times belong in front of this empty profile)
    c.last_profile = QueryProfile();
    return r;
  }
  Engine &e = Eng(c);
  BeginProfile(c, e);
  e.tail_serial++;  // no ResultTailMark of an earlier statement matches from here on
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
  MarkSetScope marks(e, c);
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
  BeginProfile(c, e);
  e.tail_serial++;
  auto d = std::make_shared<DeviceResult>();
  MarkSetScope marks(e, c);
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
    SettleProfile(c, e);  // (behind those of every statement before it)
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
    e.ResetEvents();
  }
  return true;
}

void EngineCounters(const Connection &c, int64_t out[3]) {
  if (c.engine) {
    out[0] += c.engine->sr_launches;
    out[1] += c.engine->sr_aborts;
    out[2] += c.engine->sr_launch_failures;
  }
  for (auto &sc : c.shards) EngineCounters(*sc, out);
}

void TailWaitCounters(const Connection &c, int64_t out[4]) {
  if (c.engine) {
    out[0] += c.engine->tail_wait.polled;
    out[1] += c.engine->tail_wait.blocked;
    out[2] += c.engine->tail_wait.wait_ns;
    out[3] += (int64_t)c.engine->ev_pool.size();
  }
  for (auto &sc : c.shards) TailWaitCounters(*sc, out);
}

const char *ScanHistHostCounters(const Connection &c, int64_t out[3]) {
  // (shard engines take no tail and so never answer on the host: the connection's own engine only)
  if (!c.engine) return "";
  out[0] += c.engine->hist_host.answered;
  out[1] += c.engine->hist_host.fetches;
  out[2] += c.engine->hist_host.declined;
  return c.engine->hist_host.last_reason;
}

void SettleConnProfile(Connection &c) {
  if (c.engine && c.engine->has_gpu && !c.engine->pending_prof.empty()) {
    hipSetDevice(c.engine->device);
    SettleProfile(c, *c.engine);
  }
}

void ResultTailCounters(const Connection &c, int64_t out[2]) {
  if (c.engine) {
    out[0] += c.engine->tail_results;
    out[1] += c.engine->hostcopy_results;
  }
  for (auto &sc : c.shards) ResultTailCounters(*sc, out);
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
}  // namespace mbx
