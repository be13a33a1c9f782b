// aggregate.cpp — the aggregation paths of the executor: Aggregate() tries
// them in order (the fused scans, the LDS direct-index GROUP BY, the
// partitioned GROUP BY, the run-time compiled kernels, then filter / project
// and the generic reductions).
#include <algorithm>
#include <functional>
#include <map>

#include "emit_cell.h"
#include "exec.h"
#include "group_hash.h"
#include "jit.h"
#include "str_minmax.h"
#include "vm_compile.h"
#include "knobs.h"

namespace mbx {

static dev::EmitAgg EmitFor(const AggSpec &a, VClass in_class, dev::AggState *states, DCol &out,
                            bool wide_minmax = false) {
  dev::EmitAgg ea;
  memset(&ea, 0, sizeof(ea));
  ea.kind = a.kind;
  ea.in_class = in_class;
  ea.wide_minmax = wide_minmax;
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

// What the emit reads for one aggregate: its states (nullptr: COUNT(*), from
// the slot counts) and the class of the values they accumulated.
struct EmitIn {
  dev::AggState *states;
  VClass in_class;
  bool wide_minmax = false;  // the states hold a 128-bit MIN / MAX (GlobalReduce)
};
typedef std::function<EmitIn(int)> EmitInOf;

// an emit descriptor with every field clear but the COUNT(*) slots, the slot
// (or group) count and "no NULL slot"
static dev::EmitDesc EmitDescOf(const unsigned long long *cstar, int64_t nslots) {
  dev::EmitDesc D;
  memset(&D, 0, sizeof(D));
  D.cstar = cstar;
  D.nslots = nslots;
  D.null_slot = -1;
  return D;
}

// The columns of the aggregates that have no AggState: MIN / MAX over VARCHAR
// (StrMinMaxColumns), each the argument column gathered at the winners' rows.
// has[j]: aggregate j is one, col[j] its column; the emit passes those by.
struct GatheredAggs {
  std::vector<DCol> col;
  std::vector<char> has;
  bool any = false;
};

// The aggregates' output columns, `rows` rows each, appended to out in the
// aggregates' order.  Those the emit writes are entered in D; a gathered one
// (`gathered`, or none) is put at its place as it is.
static void EmitAggCols(Engine &e, const BoundSelect &s, int64_t rows, const EmitInOf &in_of, dev::EmitDesc &D,
                        DRel &out, const GatheredAggs *gathered = nullptr) {
  const int na = (int)s.aggs.size();
  D.nagg = 0;
  for (int j = 0; j < na; j++) {
    if (gathered && gathered->any && gathered->has[j]) {
      out.cols.push_back(gathered->col[j]);
      continue;
    }
    DCol oc = AllocOut(e, s.aggs[j].type, rows, true, false);
    const EmitIn in = in_of(j);
    D.a[D.nagg++] = EmitFor(s.aggs[j], in.in_class, in.states, oc, in.wide_minmax);
    out.cols.push_back(oc);
  }
}

// What result_tail.h asks about a statement: own_result is the top-level
// SELECT of ExecuteSelect, whose relation ToHost takes.
static StatementShape ShapeOf(const Engine &e, const BoundSelect &s) {
  StatementShape h;
  h.own_result = e.defer_count_for == (const void *)&s;
  h.having = (bool)s.having;
  h.order_by = !s.order.empty();
  h.limit = s.limit >= 0;
  h.offset = s.offset > 0;
  h.union_all = !s.union_all.empty();
  for (auto &x : s.outputs) h.computed_output |= x->kind != BExpr::COL;
  return h;
}

// Whether the one-row relation of s's aggregates takes the result tail, and
// where its cells lie in the mapped buffer (mark.off): every column's physical
// type is its aggregate's, and AllocOut gives every one a validity bitmap.
static ResultTailChoice OneRowTail(const Engine &e, const BoundSelect &s, ResultTailMark &mark) {
  const int na = (int)s.aggs.size();
  ResultTailFacts f;
  f.enabled = e.result_tail;
  f.shape = ShapeOf(e, s);
  f.grouped = !s.groups.empty();
  f.ncols = na;
  f.max_cols = EMIT_MAX_AGGS;
  f.mapped_bytes = Engine::kMappedBytes;
  f.max_segs = HOSTCOPY_MAX;
  f.no_hostcopy = Knob("MBX_NO_HOSTCOPY");
  int cell[EMIT_MAX_AGGS];
  bool has_valid[EMIT_MAX_AGGS];
  for (int j = 0; j < na && j < EMIT_MAX_AGGS; j++) {
    const Phys p = PhysOf(s.aggs[j].type);
    f.varchar |= p == P_STR;
    cell[j] = PhysSize(p);
    has_valid[j] = true;
  }
  if (na <= EMIT_MAX_AGGS) f.need = ResultBufferLayout((size_t)na, cell, has_valid, 1, 1, false, mark.off);
  return ResultTailDecide(f);
}

// The one-row relation of an aggregate without GROUP BY, emitted from the
// states (and, for the fused scans, the workgroups' partials).
// launch: what runs the emit (EmitAggRelation unless the caller's own last
// kernel takes the descriptor).  Where the statement allows
// (OneRowTail), the emit also stores the row in the mapped buffer and the
// relation says so (DRel::tail), so ToHost has nothing left to copy.
static DRel EmitOneRow(Engine &e, const BoundSelect &s, const unsigned long long *cstar, const EmitInOf &in_of,
                       const dev::AggPartial *partials = nullptr, int npartials = 0,
                       const std::function<void(const dev::EmitDesc &)> &launch = nullptr,
                       const GatheredAggs *gathered = nullptr) {
  DRel out;
  out.n = 1;
  dev::EmitDesc D = EmitDescOf(cstar, 1);
  D.partials = partials;
  D.npartials = npartials;
  EmitAggCols(e, s, 1, in_of, D, out, gathered);
  auto mark = std::make_shared<ResultTailMark>();
  // (a gathered column is VARCHAR, which the tail declines: below, D.a and out.cols run in step)
  if (OneRowTail(e, s, *mark).take) {
    mark->serial = e.tail_serial;
    mark->ncols = (size_t)D.nagg;
    for (int j = 0; j < D.nagg; j++) {
      mark->data[j] = out.cols[j].data;
      mark->valid[j] = out.cols[j].validity;
      D.host.out[j] = e.h_mapped + mark->off[j].data_off;
      D.host.valid[j] = (uint64_t *)(e.h_mapped + mark->off[j].valid_off);
    }
    D.host.err_src = e.d_err;
    D.host.err_dst = (int32_t *)e.h_mapped;
    // a fresh ticket for this row (never 0, never reused): ToHost waits for it
    D.host.ticket_dst = (uint64_t *)(e.h_mapped + kTailTicketOffset);
    D.host.ticket = ++e.tail_ticket;
    mark->ticket = D.host.ticket;
    out.tail = mark;
  }
  if (launch) launch(D);
  else dev::EmitAggRelation(D, e.stream);
  return out;
}

// ---- the host answer (mbx_scan_hist_host) ---------------------------------
// A range aggregate that the code histogram answers is a function of at most
// 2 KiB of counters that change only when the table is written.  Where its row
// is the statement's own result (OneRowTail), the host folds a mirror of the
// counters with the functions the kernel runs (scan_hist.h), forms the cells
// with the emit's own definition (emit_cell.h) and stores them where the emit
// would have: nothing is launched and ToHost has nothing to wait for.

// the state emit_cell_int reads, from the fold's values
struct HostCellState {
  unsigned long long count, sum_lo;
  long long sum_hi, min_i, max_i;
};

// c's histogram mirror, fetched if it is none or describes another state of
// the column: one copy behind the encode that counted the rows, one wait.
static const uint64_t *HistMirror(Engine &e, const DevColumn &c) {
  if (!c.HistMirrorValid()) {
    const size_t bytes = (size_t)ScanHistBytes(c.code_planes);
    if (!e.EnsurePinned(bytes)) return nullptr;
    HIPCHK(hipMemcpyAsync(e.h_pinned, c.code_hist, bytes, hipMemcpyDeviceToHost, e.stream));
    HIPCHK(hipStreamSynchronize(e.stream));
    c.hist_mirror.resize(bytes / 8);
    memcpy(c.hist_mirror.data(), e.h_pinned, bytes);
    c.hist_mirror_rows = c.code_rows;
    c.hist_mirror_base = c.code_base;
    c.hist_mirror_planes = c.code_planes;
    e.hist_host.fetches++;
  }
  return c.hist_mirror.data();
}

// The one-row relation of s's aggregates from v, stored by the host in the
// mapped buffer in the tail's layout (mark, from OneRowTail) with a zero error
// word: nothing of this statement ran on the device.  The relation's device
// columns are allocated, as every relation's are, and never written: ToHost
// takes the mark or raises.
static DRel HostEmitOneRow(Engine &e, const BoundSelect &s, const ScanHistValues &v,
                           const std::shared_ptr<ResultTailMark> &mark) {
  const int na = (int)s.aggs.size();
  HostCellState S;
  S.count = v.cnt;
  S.sum_lo = v.slo;
  S.sum_hi = v.shi;
  S.min_i = v.mn;
  S.max_i = v.mx;
  DRel out;
  out.n = 1;
  mark->serial = e.tail_serial;
  mark->ncols = (size_t)na;
  mark->host_filled = true;
  for (int j = 0; j < na; j++) {
    DCol oc = AllocOut(e, s.aggs[j].type, 1, true, false);
    const dev::EmitAgg A = EmitFor(s.aggs[j], VC_I64, nullptr, oc);
    int64_t lo, hi;
    const bool valid = dev::emit_cell_int((int)A.kind, (int)A.avg_scale, S.count, &S, lo, hi);
    dev::store_phys(e.h_mapped + mark->off[j].data_off, A.out_phys, 0, lo, hi);
    const uint64_t vw = valid ? 1ull : 0ull;
    memcpy(e.h_mapped + mark->off[j].valid_off, &vw, 8);
    mark->data[j] = oc.data;
    mark->valid[j] = oc.validity;
    out.cols.push_back(oc);
  }
  const int32_t no_err = 0;
  memcpy(e.h_mapped, &no_err, 4);
  out.tail = mark;
  e.hist_host.answered++;
  return out;
}

// Answers s on the host where the option and the floor allow it, the
// statement takes the tail and, with hist_col, that column's mirror is valid
// after at most one fetch: from the fold of the mirror's counters over
// [clo, chi], or without hist_col from `known` rows that pass (the zone map
// rules every row out; every row passes and only their number is asked).
// false: the caller's device path answers, and the counters say why.
static bool HostAnswer(Engine &e, const BoundSelect &s, int64_t n, const DevColumn *hist_col, uint32_t clo,
                       uint32_t chi, uint64_t known, DRel &out) {
  if (!e.scan_hist_host || n < e.scan_hist_host_min_rows) return false;  // (not wanted: nothing is counted)
  auto mark = std::make_shared<ResultTailMark>();
  const ResultTailChoice ch = OneRowTail(e, s, *mark);
  if (!ch.take) {
    e.hist_host.declined++;
    e.hist_host.last_reason = ch.reason;
    return false;
  }
  // ToHost takes the mark only for the relation's own columns, each once and in
  // order; the emit's row can still be copied where it does not, this one cannot
  bool own_cols = s.outputs.size() == s.aggs.size() && VisibleCols(s) == s.aggs.size();
  for (size_t i = 0; own_cols && i < s.outputs.size(); i++)
    own_cols = s.outputs[i]->kind == BExpr::COL && s.outputs[i]->col == (int)i;
  if (!own_cols) {
    e.hist_host.declined++;
    e.hist_host.last_reason = "the outputs are not the aggregates, each once and in order";
    return false;
  }
  ScanHistFold f = ScanHistFold{known, 0, INT32_MAX, -1};
  int64_t base = 0;
  if (hist_col) {
    const uint64_t *h = HistMirror(e, *hist_col);
    if (!h) {
      e.hist_host.declined++;
      e.hist_host.last_reason = "no page-locked memory for the mirror's fetch";
      return false;
    }
    f = ScanHistFoldRange(h, hist_col->code_planes, clo, chi);
    base = hist_col->code_base;
  }
  out = HostEmitOneRow(e, s, ScanHistValuesOf(f, base), mark);
  return true;
}

DRel EmitGlobalStates(Engine &e, const BoundSelect &s, const unsigned long long *cstar, dev::AggState *states) {
  return EmitOneRow(e, s, cstar, [&](int j) {
    return EmitIn{states + j, s.aggs[j].kind == A_COUNT_STAR ? VC_I64 : ClassOf(s.aggs[j].arg->type)};
  });
}

// The relation of a GROUP BY on one integer key whose groups are slots (key =
// kmin + slot, null_slot the NULL key's or -1): D filled, the key column and
// the aggregates' columns allocated for `rows` rows, which is also D.nslots
// (the emit reads the live count from n_list).  Nothing is launched and out.n
// is the caller's: the sites differ in both.
static DRel KeyedEmit(Engine &e, const BoundSelect &s, const LogicalType &key_type, int64_t kmin, int64_t null_slot,
                      const unsigned long long *cstar, const int32_t *slot_list, const int64_t *n_list, int64_t rows,
                      const EmitInOf &in_of, dev::EmitDesc &D, const GatheredAggs *gathered = nullptr) {
  D = EmitDescOf(cstar, rows);
  D.slot_list = slot_list;
  D.n_list = n_list;
  D.has_key = 1;
  D.key_phys = PhysOf(key_type);
  D.kmin = kmin;
  D.null_slot = null_slot;
  DRel out;
  DCol kc = AllocOut(e, key_type, rows, true, false);
  D.key_out = kc.data;
  D.key_valid = (uint32_t *)kc.validity;
  out.cols.push_back(kc);
  EmitAggCols(e, s, rows, in_of, D, out, gathered);
  return out;
}

// The shape of a direct GROUP BY for group_direct_plan.h (the predicates are
// the caller's to add)
static GroupDirectShape DirectShape(int64_t n, int nk, Phys kphys, Phys vphys, int nv, bool mm, int vm, i128 maxabs) {
  GroupDirectShape sh;
  sh.n = n;
  sh.nk = nk;
  sh.key_bytes = PhysSize(kphys);
  sh.val_bytes = PhysSize(vphys);
  sh.nv = nv;
  sh.mm = mm;
  sh.vm = vm;
  sh.maxabs = (unsigned __int128)maxabs;
  sh.num_cus = dev::NumCUs();
  sh.knobs = dev::GroupDirectKnobsFromEnv();
  return sh;
}

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
  dev::GroupDirectArgs a{};
  a.shape = DirectShape(n, (int)nk, kphys, nv ? vals[0]->phys : P_I64, nv, mm, 0, maxabs);
  const GroupDirectPlan plan = PlanGroupDirect(a.shape);
  // (no NULLs and no predicates: one of the two kernels always takes a shape that fits)
  if (plan.form != GroupDirectForm::LdsOneFlush && plan.form != GroupDirectForm::Segmented) return false;
  size_t st_bytes = (size_t)nk * sizeof(dev::AggState);
  out.cs = Alloc(e, nk * 8, true);
  out.s0 = Alloc(e, st_bytes);
  out.s1 = Alloc(e, st_bytes);
  dev::InitAggStates((dev::AggState *)out.s0->p, nk, e.stream);
  dev::InitAggStates((dev::AggState *)out.s1->p, nk, e.stream);
  double bytes = (double)n * PhysSize(kphys);
  for (auto *v : vals) bytes += (double)n * PhysSize(v->phys);
  ProfScope ps(e, "group_direct", bytes, n);
  a.keys = kdata;
  a.v0 = nv > 0 ? vals[0]->data : nullptr;
  a.v1 = nv > 1 ? vals[1]->data : nullptr;
  a.kmin = kmin;
  a.cstar = (unsigned long long *)out.cs->p;
  a.st0 = (dev::AggState *)out.s0->p;
  a.st1 = (dev::AggState *)out.s1->p;
  dev::GroupDirectLaunch(a, plan, e.stream);
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

// MIN / MAX of a 128-bit value (UBIGINT: 64 unsigned bits, ordered like one) takes two passes: no atomic
// is 128 bits wide (ReduceMinMax128, GroupMinMax128); the emit then reads the pairs (EmitAgg::wide_minmax)
static bool WideMinMax(const AggSpec &a, int phys) {
  return (a.kind == A_MIN || a.kind == A_MAX) && (phys == P_I128 || phys == P_U64);
}

// The generic paths work on tmp = [groups..., agg args...] of the filtered
// source (FilterProject); arg_idx[j] is aggregate j's column in it, -1 for
// COUNT(*).  A VARCHAR argument is counted through its offsets, or it is the
// argument of MIN / MAX, which have a path of their own (StrMinMaxColumns) and
// never come here; the binder refuses every other aggregate over VARCHAR.
static void ReduceInput(const DCol &c, const AggSpec &a, const void **data, int *phys) {
  *data = c.data;
  *phys = c.phys;
  if (c.phys == P_STR) {
    // COUNT(varchar) only needs the validity: scan the offsets as int64
    if (a.kind != A_COUNT) ThrowError("Internal", "an aggregate over VARCHAR other than COUNT / MIN / MAX reached the device");
    *data = c.offsets;
    *phys = P_I64;
  }
}

static bool StrMinMaxAgg(const AggSpec &a, const DCol &c) {
  return c.phys == P_STR && (a.kind == A_MIN || a.kind == A_MAX);
}

// a VARCHAR column of `rows` NULLs
static DCol NullStrings(Engine &e, const LogicalType &type, int64_t rows) {
  DCol d;
  d.type = type;
  d.phys = P_STR;
  auto off = Alloc(e, (size_t)(rows + 1) * 8, true);
  auto v = Alloc(e, (size_t)Words64(std::max<int64_t>(rows, 1)) * 8, true);
  d.offsets = (int64_t *)off->p;
  d.validity = (uint64_t *)v->p;
  d.owners.push_back(off);
  d.owners.push_back(v);
  return d;
}

// MIN / MAX over the VARCHAR arguments of s (str_minmax.h): for every such
// aggregate the argument column gathered at its groups' winner rows.  The rows
// of tmp are in slot slot_of[row] of nslots (slot_of null: one slot, no GROUP
// BY); output row i is slot slot_list[i] (null: slot i) of nout.  MIN and MAX
// of one argument share the passes.  What the passes move, per row of tmp:
// str_minmax_key and str_minmax_live each the offset, the first 8 bytes of the
// string, the slot and the validity bit; str_minmax_round, per candidate and
// round, the entry, two offsets, the slot, two chunks and the words.
static GatheredAggs StrMinMaxColumns(Engine &e, const DRel &tmp, const BoundSelect &s, const std::vector<int> &arg_idx,
                                     const int32_t *slot_of, int64_t nslots, const int32_t *slot_list, int64_t nout) {
  const int na = (int)s.aggs.size();
  GatheredAggs G;
  G.col.resize(na);
  G.has.assign(na, 0);
  for (int j = 0; j < na; j++)
    if (arg_idx[j] >= 0 && StrMinMaxAgg(s.aggs[j], tmp.cols[arg_idx[j]])) G.has[j] = 1, G.any = true;
  const int64_t n = tmp.n;
  for (int j = 0; j < na; j++) {
    if (!G.has[j] || G.col[j].phys == P_STR) continue;  // (done with an earlier aggregate of the same argument)
    const int a = arg_idx[j];
    const DCol &c = tmp.cols[a];
    int kinds = 0;
    for (int q = j; q < na; q++)
      if (G.has[q] && arg_idx[q] == a) kinds |= s.aggs[q].kind == A_MIN ? kStrMinMaxWantMin : kStrMinMaxWantMax;
    DCol result[SMM_KINDS];
    if (n <= 0 || nout <= 0 || nslots <= 0) {
      // no row to offer: nothing is launched (the entry keeps the profile at one
      // str_minmax_key per argument, with nothing read)
      ProfScope ps(e, "str_minmax_key", 0, 0);
      for (int k = 0; k < SMM_KINDS; k++) result[k] = NullStrings(e, c.type, nout);
    } else {
      // (a column whose strings are all NULL or '' has offsets and no characters: no byte of it is read)
      if (!c.offsets || (!c.chars && c.chars_len > 0))
        ThrowError("Internal", "MIN / MAX over VARCHAR without materialised strings");
      dev::StrMinMaxRun run;
      run.col = dev::StrCol{c.offsets, c.chars, c.chars_len, c.validity};
      run.n = n;
      run.slot_of = slot_of;
      run.nslots = nslots;
      run.kinds = kinds;
      DevBufPtr words[2] = {Alloc(e, (size_t)nslots * 16), Alloc(e, (size_t)nslots * 16)};
      auto cand = Alloc(e, (size_t)n * 8);
      auto ctr = Alloc(e, 16);
      const double row_bytes = 8 + (double)std::min<int64_t>(c.chars_len, 8 * n) / (double)n + (slot_of ? 4 : 0) +
                               (c.validity ? 0.125 : 0);
      {
        ProfScope ps(e, "str_minmax_key", (double)n * row_bytes, n);
        dev::StrMinMaxInitWords((uint64_t *)words[0]->p, nslots, 0, 1, e.stream);
        dev::StrMinMaxKeyPass(run, (uint64_t *)words[0]->p, e.stream);
      }
      {
        ProfScope ps(e, "str_minmax_live", (double)n * row_bytes, n);
        dev::StrMinMaxLivePass(run, (const uint64_t *)words[0]->p, (uint64_t *)cand->p,
                               (unsigned long long *)ctr->p, e.stream);
      }
      struct Live {
        uint64_t count, maxlen;
      };
      const Live live = ReadDev<Live>(e, ctr->p);
      const int64_t ncand = (int64_t)std::min<uint64_t>(live.count, (uint64_t)n);
      // the rounds stop with the longest candidate: no live row has a byte past its chunks
      const int chunks = StrMinMaxChunks((int64_t)live.maxlen);
      const int rounds = StrMinMaxRounds(chunks);
      for (int r = 1; r < rounds; r++) {
        ProfScope ps(e, "str_minmax_round", (double)ncand * (8 + 16 + (slot_of ? 4 : 0) + 16 + 16), ncand);
        dev::StrMinMaxInitWords((uint64_t *)words[r & 1]->p, nslots, r, chunks, e.stream);
        dev::StrMinMaxRoundPass(run, (uint64_t *)cand->p, ncand, r, chunks, (const uint64_t *)words[(r - 1) & 1]->p,
                                (uint64_t *)words[r & 1]->p, e.stream);
      }
      const uint64_t *last = (const uint64_t *)words[(rounds - 1) & 1]->p;
      DRel arg;
      arg.n = n;
      arg.cols.push_back(c);
      arg.cols[0].validity = nullptr;  // a winner is never NULL; the cells' validity is the rows pass's
      for (int k = 0; k < SMM_KINDS; k++) {
        if (!(kinds >> k & 1)) continue;
        auto rows = Alloc(e, (size_t)nout * 8);
        auto valid = Alloc(e, (size_t)Words64(nout) * 8);
        {
          ProfScope ps(e, "str_minmax_rows", (double)nout * (8 + 8 + (slot_list ? 4 : 0)), nout);
          dev::StrMinMaxRowsPass(last + (k == SMM_MAX ? nslots : 0), slot_list, nout, nslots, n, (int64_t *)rows->p,
                                 (uint64_t *)valid->p, e.stream);
        }
        // (every row number is in [0, n): a slot without a winner gathers row 0 under a clear bit)
        DRel g = GatherRel(e, arg, (const int64_t *)rows->p, nout);
        result[k] = g.cols[0];
        result[k].validity = (uint64_t *)valid->p;
        result[k].owners.push_back(valid);
      }
      HIPCHK(hipStreamSynchronize(e.stream));  // the run's buffers are released after its last pass
    }
    for (int q = j; q < na; q++)
      if (G.has[q] && arg_idx[q] == a) {
        G.col[q] = result[s.aggs[q].kind == A_MIN ? SMM_MIN : SMM_MAX];
        G.col[q].type = s.aggs[q].type;
        G.col[q].phys = P_STR;
      }
  }
  return G;
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
    // (as the sort requires them: a VARCHAR column without rows has no offsets, one whose strings are all
    // NULL or '' has no characters; the kernels read `length` bytes, so neither pointer is followed there)
    if (c.phys == P_STR && tmp.n > 0 && (!c.offsets || (!c.chars && c.chars_len > 0)))
      ThrowError("Internal", "GROUP BY VARCHAR key without materialised strings");
    hk.k[g] = dev::HashKeyCol{c.data, c.validity, c.offsets, c.chars, (int32_t)c.phys};
  }
  const int64_t n = tmp.n;
  // a table of >= 2n entries, at most 2^30 (its scan counts in int32: a 2^31-entry
  // table silently lost every group above 5.4e8 rows); at most one entry per
  // row is ever claimed, so n <= 2^30 rows always fit (group_hash.h)
  const int64_t cap = GroupCapacity(n);
  if (n > kGroupMaxRows) ThrowError("Not implemented", "GROUP BY input above 2^30 rows on the hash path");
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
  std::vector<char> wide(std::max(na, 1), 0);
  const unsigned long long *cstar = nullptr;
  DevBufPtr cs;
  // few groups: LDS-privatised reduction keyed by the dense group id
  // (a MIN / MAX over VARCHAR is a non-integer column to it: the whole select then takes the branch below)
  bool lds = ngroups >= 1 && ngroups <= 1024 &&
             DirectReduceAll(e, slot_of->p, P_I32, 0, ngroups, n, tmp, s, arg_idx, keep, st_of, &cstar);
  if (!lds) {
    cs = Alloc(e, (size_t)std::max<int64_t>(ngroups, 1) * 8, true);
    dev::CountSlots((const int32_t *)slot_of->p, n, (unsigned long long *)cs->p, e.stream);
    cstar = (const unsigned long long *)cs->p;
  }
  GatheredAggs gathered;
  if (!lds) gathered = StrMinMaxColumns(e, tmp, s, arg_idx, (const int32_t *)slot_of->p, ngroups, nullptr, ngroups);
  for (int j = 0; j < na && !lds; j++) {
    if (arg_idx[j] < 0 || gathered.has[j]) continue;
    const DCol &c = tmp.cols[arg_idx[j]];
    const void *data;
    int phys;
    ReduceInput(c, s.aggs[j], &data, &phys);
    states[j] = Alloc(e, (size_t)std::max<int64_t>(ngroups, 1) * sizeof(dev::AggState));
    dev::InitAggStates((dev::AggState *)states[j]->p, ngroups, e.stream);
    wide[j] = WideMinMax(s.aggs[j], phys);
    ProfScope ps(e, "group_reduce", (double)n * (PhysSize((Phys)phys) + 4) * (wide[j] ? 2 : 1), n);
    dev::GroupReduceColumn((const int32_t *)slot_of->p, data, phys, c.validity, n, (dev::AggState *)states[j]->p,
                           e.stream);
    // MIN / MAX of a 128-bit value: a second pass over the column for the low words
    if (wide[j])
      dev::GroupMinMax128((const int32_t *)slot_of->p, data, phys, c.validity, n, (dev::AggState *)states[j]->p,
                          e.stream);
    st_of[j] = (dev::AggState *)states[j]->p;
  }
  DRel keys;
  keys.n = n;
  for (int g = 0; g < ng; g++) keys.cols.push_back(tmp.cols[g]);
  DRel out = GatherRel(e, keys, (const int64_t *)rep->p, ngroups);
  for (int g = 0; g < ng; g++) out.cols[g].type = s.groups[g]->type;
  // (no key in the descriptor: the key columns are the gathered ones)
  dev::EmitDesc D = EmitDescOf(cstar, ngroups);
  EmitAggCols(e, s, ngroups, [&](int j) {
    return EmitIn{st_of[j], arg_idx[j] >= 0 ? ClassOf(tmp.cols[arg_idx[j]].type) : VC_I64, wide[j] != 0};
  }, D, out, &gathered);
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
  dev::AggState *st = (dev::AggState *)e.d_small;
  unsigned long long *cstar = (unsigned long long *)((char *)e.d_small + 1024);
  int npartials;
  {
    ProfScope ps(e, "filter_multi", bytes, src.n);
    npartials = dev::FilterMultiPartials(d, src.n, e.d_partials, e.stream);
  }
  out = EmitOneRow(
      e, s, cstar, [&](int j) { return EmitIn{s.aggs[j].kind == A_COUNT_STAR ? nullptr : st, VC_I64}; }, e.d_partials,
      npartials);
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
    vc.P.pred_ins = (uint8_t)vc.P.n_ins;
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
  out = EmitOneRow(e, s, (const unsigned long long *)cs->p, [&](int j) {
    return EmitIn{(dev::AggState *)states->p + j,
                  s.aggs[j].kind == A_COUNT_STAR ? VC_I64 : ClassOf(s.aggs[j].arg->type)};
  });
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
    vc.P.pred_ins = (uint8_t)vc.P.n_ins;
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
  dev::EmitDesc D = EmitDescOf((const unsigned long long *)cs->p, ngroups);
  D.slot_list = (const int32_t *)list->p;
  D.n_list = e.d_scratch;
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
  EmitAggCols(e, s, ngroups, [&](int j) {
    return EmitIn{s.aggs[j].kind == A_COUNT_STAR ? nullptr : (dev::AggState *)states->p + (size_t)j * ns, VC_I64};
  }, D, out);
  if (ngroups > 0) dev::EmitAggRelation(D, e.stream);
  HIPCHK(hipStreamSynchronize(e.stream));  // state buffers released after the emit
  DropEmptyValidity(e, out);
  return true;
}


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
  return RelationReachesHostUnchanged(ShapeOf(e, s));
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

// The statement's WHERE as the passes take it (group_pred_plan.h): a
// conjunction of integer range comparisons, planned against the zone maps of
// this relation's columns.  keys: the key column(s) of the shape (code: they
// fold into a group code).  false: not such a conjunction or the plan is Unfit
// -- the path declines as it always did for a WHERE.
static bool PartGroupPreds(const DRel &src, const BoundSelect &s, const std::vector<int> &keys, bool code,
                           const PartGroupValues &v, GroupPredPlan &plan) {
  plan = GroupPredPlan{};
  plan.verdict = GroupPredVerdict::All;
  if (!s.where) return true;
  std::map<int, std::pair<i128, i128>> ranges;
  if (!RangeConj(*s.where, ranges)) return false;
  std::vector<GroupPredIn> in;
  for (auto &kv : ranges) {
    if (src.range && kv.first == 0) return false;
    const DCol &c = src.cols[kv.first];
    const DevColumn *tc = c.table_col;
    GroupPredIn p = {};
    p.col = kv.first;
    p.data = c.data;
    p.phys = c.phys;
    p.has_validity = c.validity != nullptr;
    p.stats_valid = tc && tc->stats_valid;
    p.imin = tc ? tc->imin : 0;
    p.imax = tc ? tc->imax : 0;
    p.null_count = tc ? tc->null_count : 1;
    p.lo = kv.second.first;
    p.hi = kv.second.second;
    in.push_back(p);
  }
  GroupPredShape shape = {};
  shape.nkeys = (int)keys.size();
  shape.code = code;
  for (size_t i = 0; i < keys.size() && i < 4; i++) shape.key_cols[i] = keys[i];
  shape.nv = (int)v.vcols.size();
  for (size_t j = 0; j < v.vcols.size() && j < 2; j++) shape.val_cols[j] = v.vcols[j];
  plan = PlanGroupPreds(in.data(), (int)in.size(), shape);
  return plan.verdict != GroupPredVerdict::Unfit;
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
  const int64_t nslots = r.nslots;
  auto list = Alloc(e, nslots * 4);
  const bool defer = CountMayStayOnDevice(e, s);
  DevBufPtr nbuf = defer ? Alloc(e, 8) : nullptr;
  int64_t *const n_out = defer ? (int64_t *)nbuf->p : e.d_scratch;
  dev::CompactSlots((const unsigned long long *)r.cs->p, nslots, (int32_t *)list->p, n_out, e.stream);
  // (D arrives with its key fields set and is completed here, not built anew)
  D.cstar = (const unsigned long long *)r.cs->p;
  D.slot_list = (const int32_t *)list->p;
  D.n_list = n_out;
  D.nslots = nslots;
  D.null_slot = -1;
  EmitAggCols(e, s, nslots, [&](int j) {
    dev::AggState *stp = nullptr;
    if (s.aggs[j].kind != A_COUNT_STAR)
      stp = StripWidening(s.aggs[j].arg.get())->col == v.vcols[0] ? r.d.st0 : r.d.st0 + nslots;
    return EmitIn{stp, VC_I64};
  }, D, out);
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
                                     const PartGroupValues &v, const GroupPredPlan &preds, DRel &out) {
  PartGroupRun r;
  PartGroupPrepare(e, src, v, 0, r);
  r.d.key = K.data;
  r.d.kphys = K.phys;
  r.d.pred = preds.set;
  if (!PartGroupHashedRun(e, src, r,
                          (double)src.n * (PhysSize(K.phys) + preds.own_bytes) + PartGroupValueBytes(src, v)))
    return false;
  dev::EmitDesc D;
  memset(&D, 0, sizeof(D));
  D.key_msb = (const unsigned long long *)r.gk->p;
  PartGroupOneKeyOut(e, s, r, D, out);
  PartGroupEmit(e, s, v, r, D, out);
  return true;
}

// F3: GROUP BY one integer key (no NULLs) whose zone-map range is too wide for
// F2's LDS tables but dense enough for per-key state arrays (1024 < range <=
// PartGroupMaxRange, range <= 4 n), COUNT / SUM / MIN / MAX / AVG over
// <= 2 integer columns of one phys without NULLs: rows partitioned by key
// range, each partition reduced in LDS (group_part.hip), then the non-empty
// keys compacted and emitted in key order as F2 does.  A WHERE that is a
// conjunction of integer range comparisons on up to GROUP_MAX_PRED columns
// without NULLs is tested inside the hist and scatter passes (PartGroupPreds);
// any other WHERE declines.  false: the shape does not fit (the hash path or
// the run-time compiled kernel takes it).
static bool PartGroupAggregate(Engine &e, const DRel &src, const BoundSelect &s, DRel &out) {
  if (const char *k = Knob("MBX_PART_GROUP"))  // MBX_PART_GROUP=0: the hash path (A/B)
    if (atoi(k) == 0) return false;
  if (s.groups.size() != 1 || src.range || src.n <= 0 || src.n >= ((int64_t)1 << 32)) return false;
  if (s.groups[0]->kind != BExpr::COL || !FastIntCol(src, s.groups[0]->col)) return false;
  const DCol &K = src.cols[s.groups[0]->col];
  const DevColumn *ks = K.table_col;
  if (!ks || !ks->stats_valid || ks->null_count != 0) return false;
  const i128 range = ks->imax - ks->imin + 1;
  PartGroupValues v;
  if (!PartGroupValueCols(src, s, v) || range <= 1024) return false;
  GroupPredPlan preds;
  if (!PartGroupPreds(src, s, {s.groups[0]->col}, false, v, preds)) return false;
  const int nv = (int)v.vcols.size();
  // keys too sparse for dense per-key states: hashed partitions (F3h), from
  // 2^16 rows (below, the hash path's table is small) with at most one value column
  if (range > dev::PartGroupMaxRange(nv, v.mm) || range > 4 * (i128)src.n)
    return nv <= 1 && src.n >= ((int64_t)1 << 16) && PartGroupHashedAggregate(e, src, s, K, v, preds, out);
  PartGroupRun r;
  PartGroupPrepare(e, src, v, (int64_t)range, r);
  r.d.key = K.data;
  r.d.kphys = K.phys;
  r.d.kmin = (int64_t)ks->imin;
  r.d.range = r.nslots;
  r.d.pred = preds.set;
  {
    // algorithmic bytes: the key, the value and the predicates' own columns once
    ProfScope ps(e, "group_part",
                 (double)src.n * (PhysSize(K.phys) + preds.own_bytes) + PartGroupValueBytes(src, v), src.n);
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
// for F2's LDS tables.  A WHERE as F3 takes it, at least 2^16 rows, more than 4096 codes (so
// the shape never competes with F2 or the run-time compiled jit_group); values
// as F3 / F3h take them.  Dense codes (total <= PartGroupMaxRange and <= 4 n)
// come out in code order -- key order, NULLs last per key, as F2 and jit_group
// emit; else hashed partitions, groups in table order (<= 1 value column).
// false: the shape does not fit or the hashed tables filled up.
static bool CodeGroupAggregate(Engine &e, const DRel &src, const BoundSelect &s, DRel &out) {
  const int ng = (int)s.groups.size();
  if (const char *k = Knob("MBX_PART_GROUP"))
    if (atoi(k) == 0) return false;
  if (ng < 1 || ng > kGroupCodeMaxKeys || src.range || src.n < ((int64_t)1 << 16) ||
      src.n >= ((int64_t)1 << 32))
    return false;
  GroupCodeKeyIn in[kGroupCodeMaxKeys];
  std::vector<int> kcols;
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
    kcols.push_back(x->col);
  }
  if (ng == 1 && !nullable) return false;  // F3's own shape
  GroupCodePlan plan;
  if (!PlanGroupCode(in, ng, &plan) || plan.total <= 4096) return false;
  PartGroupValues v;
  if (!PartGroupValueCols(src, s, v)) return false;
  const int nv = (int)v.vcols.size();
  const bool dense = plan.total <= dev::PartGroupMaxRange(nv, v.mm) && (i128)plan.total <= 4 * (i128)src.n;
  if (!dense && nv > 1) return false;
  GroupPredPlan preds;
  if (!PartGroupPreds(src, s, kcols, true, v, preds)) return false;
  // algorithmic bytes: every key column, n / 8 per validity bitmap, every value
  // column, the predicates' own columns
  double bytes = PartGroupValueBytes(src, v) + (double)src.n * preds.own_bytes;
  for (int i = 0; i < ng; i++)
    bytes += (double)src.n * PhysSize((Phys)in[i].phys) + (in[i].validity ? (double)src.n / 8 : 0);
  PartGroupRun r;
  PartGroupPrepare(e, src, v, dense ? plan.total : 0, r);
  r.d.code = &plan;
  r.d.pred = preds.set;
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

// F1: no GROUP BY, a range predicate on one int column (or none), all
// aggregates over one int column (or COUNT(*)): the fused filter_agg scan, over
// the predicate column's code image where it has one.
static bool ScanAggregate(Engine &e, const DRel &src, const BoundSelect &s, DRel &out) {
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
  if (!aggs_ok || src.n <= 0) return false;
  if (lo < (i128)INT64_MIN) lo = INT64_MIN;
  if (hi > (i128)INT64_MAX) hi = INT64_MAX;
  bool empty = lo > hi;
  dev::AggState *st = (dev::AggState *)e.d_small;
  unsigned long long *cstar = (unsigned long long *)((char *)e.d_small + 1024);
  int npartials = 0;
  const EmitInOf in_of = [&](int j) { return EmitIn{s.aggs[j].kind == A_COUNT_STAR ? nullptr : st, VC_I64}; };
  if (empty) dev::InitAggStatesCounts(st, 1, cstar, 1, e.stream);
  if (!empty) {
    const DCol *P = pcol >= 0 ? &src.cols[pcol] : nullptr;
    const DCol *A = acol >= 0 ? &src.cols[acol] : nullptr;
    if (!P && A) {
      // no predicate: use the aggregate column as the (always-true) predicate column
      P = A;
    }
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
    auto known_count = [&]() {  // every row passes and only their number is asked
      dev::InitAggStatesCounts(st, 1, cstar, 1, e.stream, (unsigned long long)src.n);
    };
    if (by_codes && tc->code_planes > 0) {
      const ScanPlanePlan pp =
          PlanScanPlanes(tc->code_planes, (i128)tc->code_base, tc->imax, (int64_t)lo, (int64_t)hi, A != nullptr);
      // the column's code histogram answers what the planes would (scan_hist.h)
      const bool by_hist = e.scan_hist && tc->code_hist && !pp.empty && pp.planes > 0;
      // the host answers what needs no pass over the rows (no launch, no profile entry)
      if ((pp.empty || pp.planes == 0 || by_hist) &&
          HostAnswer(e, s, src.n, by_hist ? tc : nullptr, pp.clo, pp.chi, pp.empty ? 0 : (uint64_t)src.n, out))
        return true;
      ProfScope ps(e, "filter_agg",
                   pp.empty  ? 0
                   : by_hist ? (double)ScanHistBytes(tc->code_planes)
                             : (double)ScanPlaneScanBytes(pp.planes, src.n),
                   src.n);
      if (pp.empty) {
        dev::InitAggStatesCounts(st, 1, cstar, 1, e.stream);  // the zone map rules every row out, as below
      } else if (pp.planes == 0) {
        known_count();  // it lets every row in: no plane is read
      } else if (by_hist) {
        // one launch folds the histogram, writes its partial record (the shard
        // combine reads it) and emits the row from it
        out = EmitOneRow(e, s, cstar, in_of, e.d_partials, 1, [&](const dev::EmitDesc &D) {
          dev::FilterAggHist(tc->code_hist, tc->code_planes, pp.clo, pp.chi, tc->code_base, e.d_partials, e.stream,
                             &D);
        });
        return true;
      } else {
        npartials = dev::FilterAggPlanes(tc->codes, tc->code_planes, pp.planes, pp.ge, pp.le, pp.clo, pp.chi,
                                         tc->code_base, A != nullptr, need_mm, src.n, e.d_partials, e.stream);
      }
    } else if (by_codes) {
      const ScanCodeRange cr = PlanScanFieldRange(tc->code_fields, (i128)tc->code_base, tc->imax, (int64_t)lo, (int64_t)hi);
      if (cr.empty && HostAnswer(e, s, src.n, nullptr, 0, 0, 0, out)) return true;
      if (cr.empty) {
        // the zone map rules every row out: no scan (the entry keeps the
        // profile at one filter_agg per statement, with nothing read)
        ProfScope ps(e, "filter_agg", 0, src.n);
        dev::InitAggStatesCounts(st, 1, cstar, 1, e.stream);
      } else {
        ProfScope ps(e, "filter_agg", (double)ScanCodeBytes(tc->code_fields, src.n), src.n);
        npartials = dev::FilterAggCodes(tc->codes, tc->code_fields, tc->code_base, cr.clo, cr.cspan, cr.form,
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
      if (HostAnswer(e, s, src.n, nullptr, 0, 0, (uint64_t)src.n, out)) return true;
      known_count();
    }
  }
  out = EmitOneRow(e, s, cstar, in_of, e.d_partials, npartials);
  return true;
}

// F2: GROUP BY one small-range int key column (zone-map range <= 1024, plus
// the NULL key's slot), aggregates over <= 2 int columns of one phys, up to
// GROUP_MAX_PRED range predicates on int columns, fused: group_direct_lds.
// Filtered shapes run here too: since its table atomics stopped draining
// the DMA ring, group_direct_lds beats the run-time compiled jit_group at
// 1e9 rows (c3_where 3.00 vs 3.34 ms, c3_where2 3.66 vs 4.06 ms,
// profiles/r02_group_where_sweep.log); jit_group takes the shapes F2 does not.
// false: the shape does not fit, or (*refused set) it fits and the launch was
// refused -- the caller then goes past the partitioned GROUP BY as well.
static bool DirectGroupAggregate(Engine &e, const DRel &src, const BoundSelect &s, DRel &out, bool *refused) {
  *refused = false;
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
  if (!(s.groups.size() == 1 && f2_pred_ok && !src.range && s.groups[0]->kind == BExpr::COL &&
        (FastIntCol(src, s.groups[0]->col) || (nulls_ok && int_col(s.groups[0]->col)))))
    return false;
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
  if (!ok || vcols.size() > 2) return false;
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
  if (!ok) return false;
  int nk = (int)range + (knull ? 1 : 0);  // + the NULL group's slot, last
  int nv = (int)vcols.size();
  dev::GroupDirectArgs a{};
  a.shape = DirectShape(src.n, nk, K.phys, nv ? src.cols[vcols[0]].phys : P_I64, nv, mm, vm, maxabs);
  a.shape.records_offered = true;
  double bytes = (double)src.n * PhysSize(K.phys);
  for (int c : vcols) bytes += (double)src.n * PhysSize(src.cols[c].phys);
  bytes += __builtin_popcount(vm) * (src.n / 8.0);  // validity words
  for (auto &kv : f2_ranges) {
    const int kcol = s.groups[0]->col, pc = kv.first;
    dev::GroupPred &g = a.preds.p[a.preds.n++];
    g.src = pc == kcol ? 2 : (nv > 0 && pc == vcols[0]) ? 3 : 1;
    g.phys = src.cols[pc].phys;
    g.col = src.cols[pc].data;
    g.lo = (int64_t)std::max<i128>(kv.second.first, INT64_MIN);
    g.span = (uint64_t)((int64_t)std::min<i128>(kv.second.second, INT64_MAX)) - (uint64_t)g.lo;
    if (g.src == 1) {
      bytes += (double)src.n * PhysSize(src.cols[pc].phys);
      a.shape.pred_bytes[a.shape.npred_own++] = PhysSize(src.cols[pc].phys);
    }
  }
  a.shape.npred = a.preds.n;
  const GroupDirectPlan plan = PlanGroupDirect(a.shape);
  if (plan.form == GroupDirectForm::Unfit) return false;
  if (plan.form == GroupDirectForm::Refused) {
    // (the profile keeps the group_direct entry a refused launch has always left)
    ProfScope ps(e, "group_direct", bytes, src.n);
    *refused = true;
    return false;
  }
  int64_t nslots = nk;
  size_t st_bytes = (size_t)nslots * sizeof(dev::AggState);
  // both value columns' states in one block; the launch zeroes them with the
  // COUNT(*) slots for its atomic forms, or has every workgroup write a record
  // of its table that GroupPartialsCompact reduces
  auto cs = Alloc(e, nslots * 8);
  auto sb = Alloc(e, 2 * st_bytes);
  dev::AggState *const s0p = (dev::AggState *)sb->p, *const s1p = s0p + nslots;
  DevBufPtr gparts = plan.records ? Alloc(e, plan.record_bytes) : nullptr;
  a.keys = K.data;
  a.v0 = nv > 0 ? src.cols[vcols[0]].data : nullptr;
  a.v1 = nv > 1 ? src.cols[vcols[1]].data : nullptr;
  a.kmin = (int64_t)ks->imin;
  a.valid = gval;
  a.cstar = (unsigned long long *)cs->p;
  a.st0 = s0p;
  a.st1 = s1p;
  a.init_state_slots = 2 * nslots;
  a.records = plan.records ? gparts->p : nullptr;
  {
    ProfScope ps(e, "group_direct", bytes, src.n);
    dev::GroupDirectLaunch(a, plan, e.stream);
  }
  auto list = Alloc(e, nslots * 4);
  // the group count: left on the device for ToHost when this is the
  // statement's own result (CountMayStayOnDevice), else read below
  const bool defer = CountMayStayOnDevice(e, s);
  DevBufPtr nbuf = defer ? Alloc(e, 8) : nullptr;
  int64_t *const n_out = defer ? (int64_t *)nbuf->p : e.d_scratch;
  if (!plan.records)
    dev::CompactSlots((const unsigned long long *)cs->p, nslots, (int32_t *)list->p, n_out, e.stream);
  // outputs sized for every slot (<= 1024 rows), unlike the generic paths'
  // (sized for the groups): the emit reads the group count from the device, so
  // the query waits on the stream once, after it
  dev::EmitDesc D;
  out = KeyedEmit(
      e, s, s.groups[0]->type, (int64_t)ks->imin, knull ? nk - 1 : -1, (const unsigned long long *)cs->p,
      (const int32_t *)list->p, n_out, nslots,
      [&](int j) {
        dev::AggState *stp = nullptr;
        if (s.aggs[j].kind != A_COUNT_STAR) stp = StripWidening(s.aggs[j].arg.get())->col == vcols[0] ? s0p : s1p;
        return EmitIn{stp, VC_I64};
      },
      D);
  if (plan.records)  // records reduced, keys compacted and the relation written by one launch
    dev::GroupPartialsCompact(gparts->p, plan.grid, nv, mm, nk, (unsigned long long *)cs->p, s0p, s1p,
                              (int32_t *)list->p, n_out, e.stream, &D);
  else
    dev::EmitAggRelation(D, e.stream);
  if (defer) {
    out.n = nslots;  // the columns hold every slot; the count follows the rows to the host
    out.n_dev = n_out;
    out.n_owner = nbuf;
  } else {
    out.n = ReadDev<int64_t>(e, n_out);
  }
  return true;
}

// no GROUP BY: one reduce_column per aggregate
static DRel GlobalReduce(Engine &e, const DRel &tmp, const BoundSelect &s, const std::vector<int> &arg_idx) {
  const int na = (int)s.aggs.size();
  size_t st_bytes = std::max(na, 1) * sizeof(dev::AggState);
  auto sb = Alloc(e, st_bytes);
  dev::InitAggStates((dev::AggState *)sb->p, std::max(na, 1), e.stream);
  auto cs = Alloc(e, 8);
  unsigned long long cn = (unsigned long long)tmp.n;
  HIPCHK(hipMemcpyAsync(cs->p, &cn, 8, hipMemcpyHostToDevice, e.stream));
  std::vector<char> wide(std::max(na, 1), 0);
  const GatheredAggs gathered = StrMinMaxColumns(e, tmp, s, arg_idx, nullptr, 1, nullptr, 1);
  for (int j = 0; j < na; j++) {
    if (arg_idx[j] < 0 || gathered.has[j]) continue;
    const DCol &c = tmp.cols[arg_idx[j]];
    const void *data;
    int phys;
    ReduceInput(c, s.aggs[j], &data, &phys);
    wide[j] = WideMinMax(s.aggs[j], phys);
    ProfScope ps(e, "reduce_column", (double)tmp.n * PhysSize((Phys)phys) * (wide[j] ? 2 : 1), tmp.n);
    dev::ReduceColumn(data, phys, c.validity, tmp.n, (dev::AggState *)sb->p + j, e.stream);
    // MIN / MAX of a 128-bit value: a second pass over the column for the low word
    if (wide[j]) dev::ReduceMinMax128(data, phys, c.validity, tmp.n, (dev::AggState *)sb->p + j, e.stream);
  }
  DRel out = EmitOneRow(e, s, (const unsigned long long *)cs->p, [&](int j) {
    return EmitIn{(dev::AggState *)sb->p + j, arg_idx[j] >= 0 ? ClassOf(tmp.cols[arg_idx[j]].type) : VC_I64, wide[j] != 0};
  }, nullptr, 0, nullptr, &gathered);
  HIPCHK(hipStreamSynchronize(e.stream));
  return out;
}

// GROUP BY one integer key whose values in tmp span a narrow range (a device
// min/max pass): direct-index slots, reduced in LDS (group_direct) where the
// key has no NULLs and at most 1024 values, else by group_assign +
// group_reduce.  false: anything else (several keys, VARCHAR / float keys,
// wide ranges) -- the hash table.
static bool SlotGroupAggregate(Engine &e, const DRel &tmp, const BoundSelect &s, const std::vector<int> &arg_idx,
                               DRel &out) {
  const DCol &K = tmp.cols[0];
  if (!(s.groups.size() == 1 && ClassOf(K.type) == VC_I64 && K.phys != P_STR && K.phys != P_F64 && K.phys != P_F32 &&
        K.phys != P_I128 && K.phys != P_INTERVAL))
    return false;
  long long *kr = (long long *)((char *)e.d_small + 2048);
  dev::KeyRange(K.data, K.phys, K.validity, tmp.n, kr, e.stream);
  long long krh[3];
  HIPCHK(hipMemcpyAsync(krh, kr, sizeof(krh), hipMemcpyDeviceToHost, e.stream));
  HIPCHK(hipStreamSynchronize(e.stream));
  const int64_t kmin = krh[2] ? krh[0] : 0;
  const i128 range = krh[2] ? (i128)krh[1] - krh[0] + 1 : 0;
  if (range > (1 << 24) || range > 4 * (i128)std::max<int64_t>(tmp.n, 1024)) return false;
  dev::EmitDesc D;
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
      out = KeyedEmit(e, s, s.groups[0]->type, kmin, -1, cstar, (const int32_t *)list->p, e.d_scratch, ngroups,
                      [&](int j) { return EmitIn{st_of[j], VC_I64}; }, D);
      out.n = ngroups;
      if (ngroups > 0) dev::EmitAggRelation(D, e.stream);
      HIPCHK(hipStreamSynchronize(e.stream));
      return true;
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
  const int na = (int)s.aggs.size();
  std::vector<DevBufPtr> states(na);
  std::vector<char> wide(std::max(na, 1), 0);
  // (which aggregates are gathered is known before their columns are: those need the slot list below)
  std::vector<char> is_gathered(std::max(na, 1), 0);
  for (int j = 0; j < na; j++)
    is_gathered[j] = arg_idx[j] >= 0 && StrMinMaxAgg(s.aggs[j], tmp.cols[arg_idx[j]]);
  for (int j = 0; j < na; j++) {
    if (arg_idx[j] < 0 || is_gathered[j]) continue;
    const DCol &c = tmp.cols[arg_idx[j]];
    const void *data;
    int phys;
    ReduceInput(c, s.aggs[j], &data, &phys);
    states[j] = Alloc(e, nslots * sizeof(dev::AggState));
    dev::InitAggStates((dev::AggState *)states[j]->p, nslots, e.stream);
    wide[j] = WideMinMax(s.aggs[j], phys);
    ProfScope ps(e, "group_reduce", (double)tmp.n * (PhysSize((Phys)phys) + 4) * (wide[j] ? 2 : 1), tmp.n);
    dev::GroupReduceColumn((const int32_t *)slot_of->p, data, phys, c.validity, tmp.n,
                           (dev::AggState *)states[j]->p, e.stream);
    // MIN / MAX of a 128-bit value: a second pass over the column for the low words
    if (wide[j])
      dev::GroupMinMax128((const int32_t *)slot_of->p, data, phys, c.validity, tmp.n, (dev::AggState *)states[j]->p,
                          e.stream);
  }
  auto list = Alloc(e, nslots * 4);
  dev::CompactSlots((const unsigned long long *)cs->p, nslots, (int32_t *)list->p, e.d_scratch, e.stream);
  int64_t ngroups = ReadDev<int64_t>(e, e.d_scratch);
  // (the passes of StrMinMaxColumns use d_scratch for nothing, so the emit still finds the count there)
  const GatheredAggs gathered =
      StrMinMaxColumns(e, tmp, s, arg_idx, (const int32_t *)slot_of->p, nslots, (const int32_t *)list->p, ngroups);
  out = KeyedEmit(e, s, s.groups[0]->type, kmin, nslots - 1, (const unsigned long long *)cs->p,
                  (const int32_t *)list->p, e.d_scratch, ngroups,
                  [&](int j) {
                    return EmitIn{states[j] ? (dev::AggState *)states[j]->p : nullptr,
                                  arg_idx[j] >= 0 ? ClassOf(tmp.cols[arg_idx[j]].type) : VC_I64, wide[j] != 0};
                  },
                  D, &gathered);
  out.n = ngroups;
  // (launched for no groups as well, unlike the LDS form above: kept as it was)
  dev::EmitAggRelation(D, e.stream);
  HIPCHK(hipStreamSynchronize(e.stream));
  DropEmptyValidity(e, out);
  return true;
}

// The plan of an aggregate: the paths in the order they are tried.  Each
// returns false, having left `out` alone, for a shape it does not take.
DRel Aggregate(Engine &e, const DRel &src, const BoundSelect &s) {
  const int ng = (int)s.groups.size();
  const int na = (int)s.aggs.size();
  if (na > EMIT_MAX_AGGS) ThrowError("Not implemented", "too many aggregates in one query for the device path");
  {  // VARCHAR predicates in WHERE, the keys or the arguments become BOOLEAN columns first
    std::vector<BExprPtr> trees = s.groups;
    for (auto &a : s.aggs) trees.push_back(a.arg);
    trees.push_back(s.where);
    DRel low;
    if (LowerStringPredicates(e, src, trees, low)) {
      // The bound plan stays as it is.  The aggregation reads only the WHERE,
      // the keys and the aggregates of its select, so s2 carries just those;
      // not being the statement's own select, it reads its group count back
      // instead of leaving it on the device (CountMayStayOnDevice).
      BoundSelect s2;
      s2.is_agg = true;
      s2.groups.assign(trees.begin(), trees.begin() + ng);
      s2.aggs = s.aggs;
      for (int j = 0; j < na; j++) s2.aggs[j].arg = trees[ng + j];
      s2.where = trees[ng + na];
      return Aggregate(e, low, s2);
    }
  }
  for (auto &a : s.aggs)
    if (a.distinct) return DistinctAggregate(e, src, s);
  DRel out;
  // no GROUP BY, range predicates on int columns, one aggregated int column:
  // the fused scans, F1m (several columns, NULLs) before F1 (one column)
  if (ng == 0 && !src.range) {
    if (FilterMultiAggregate(e, src, s, out)) return out;
    if (ScanAggregate(e, src, s, out)) return out;
  }
  // one int key: F2 (zone-map range <= 1024, in LDS), then F3 / F3h (wider,
  // partitioned); a shape F2 takes but could not launch skips F3 as well
  if (ng == 1) {
    bool f2_refused;
    if (DirectGroupAggregate(e, src, s, out, &f2_refused)) return out;
    if (!f2_refused && PartGroupAggregate(e, src, s, out)) return out;
  }
  // any WHERE and argument expressions, up to 4096 key slots: run-time compiled
  if (jit::Enabled() && (ng == 0 ? JitAggregate(e, src, s, out) : JitGroupAggregate(e, src, s, out))) return out;
  // composite / NULL-able integer keys over more than 4096 codes: the
  // partitioned GROUP BY over the keys' group code
  if (ng >= 1 && CodeGroupAggregate(e, src, s, out)) return out;
  // everything else: compact [groups..., agg args...] then reduce
  std::vector<BExprPtr> exprs = s.groups;
  std::vector<int> arg_idx(na, -1);
  // MIN and MAX of one VARCHAR column read one column of tmp: they share the passes (StrMinMaxColumns)
  auto str_minmax_of_col = [&](const AggSpec &a) {
    return (a.kind == A_MIN || a.kind == A_MAX) && a.arg->kind == BExpr::COL && PhysOf(a.arg->type) == P_STR;
  };
  for (int j = 0; j < na; j++) {
    if (s.aggs[j].kind == A_COUNT_STAR) continue;
    for (int q = 0; q < j && arg_idx[j] < 0 && str_minmax_of_col(s.aggs[j]); q++)
      if (s.aggs[q].kind != A_COUNT_STAR && str_minmax_of_col(s.aggs[q]) && s.aggs[q].arg->col == s.aggs[j].arg->col)
        arg_idx[j] = arg_idx[q];
    if (arg_idx[j] >= 0) continue;
    arg_idx[j] = (int)exprs.size();
    exprs.push_back(s.aggs[j].arg);
  }
  const DRel tmp = FilterProject(e, src, s.where, exprs);
  if (ng == 0) return GlobalReduce(e, tmp, s, arg_idx);
  if (SlotGroupAggregate(e, tmp, s, arg_idx, out)) return out;
  return HashAggregate(e, tmp, s, arg_idx);
}

}  // namespace mbx
