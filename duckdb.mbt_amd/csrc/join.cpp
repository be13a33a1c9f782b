// join.cpp — the inner equi-join as a source of the executor: SourceRel hands
// a BoundSource::JOIN here and gets back one relation, the left input's
// columns followed by the right input's, that every later stage (WHERE,
// Aggregate, sort, concat, results, CTAS) reads like any other.
//
// Both inputs are run to relations.  The one with fewer rows is the build
// side (the right one on a tie): its keys are widened to int64, sorted with
// their row numbers (SortPairs is stable, so rows ascend within a key), and
// every distinct key goes into the table of join_plan.h with its run's start
// and length.  The other input probes: a count per row, ScanLengths for the
// offsets and the total, then join_expand writes the two row-number arrays of
// the result, probe-row-major with build rows ascending, and GatherRel fetches
// the columns of each side.  The ON clause's other conjuncts (the residual)
// filter the joined relation.  The kernels are join_kernels.hip.
//
// JoinBuildTable is the build half on its own (x IN (subquery) builds its set
// with it, executor.cpp).  JoinPrepare runs a join up to its table, JoinPairs does the rest.  An
// aggregate without GROUP BY over a join (JoinAggregate) prepares the join and,
// where join_agg_plan.h takes the statement, never makes the pairs: one kernel
// probes and interprets the residual, the WHERE and the aggregate arguments per
// pair (join_probe_agg), one folds the workgroups' records (join_agg_fold).
#include "exec.h"
#include "join_agg_plan.h"
#include "join_plan.h"
#include "knobs.h"
#include "vm_compile.h"

namespace mbx {

namespace {

BExprPtr ColRef(int c, const LogicalType &t) {
  auto x = std::make_shared<BExpr>();
  x->kind = BExpr::COL;
  x->col = c;
  x->type = t;
  return x;
}

std::vector<BExprPtr> AllCols(const DRel &r) {
  std::vector<BExprPtr> out;
  for (size_t i = 0; i < r.cols.size(); i++) out.push_back(ColRef((int)i, r.cols[i].type));
  return out;
}

// no row of either side: the columns of both, empty
DRel EmptyJoin(Engine &e, const DRel &l, const DRel &r) {
  auto none = Alloc(e, 16);
  DRel out = GatherRel(e, l, (const int64_t *)none->p, 0);
  DRel rr = GatherRel(e, r, (const int64_t *)none->p, 0);
  out.cols.insert(out.cols.end(), rr.cols.begin(), rr.cols.end());
  return out;
}

}  // namespace

// a key that is a bare column is read in place; anything else is evaluated
DCol KeyColumn(Engine &e, const DRel &r, const BExprPtr &k) {
  if (k->kind == BExpr::COL && !(r.range && k->col == 0)) return r.cols[k->col];
  return FilterProject(e, r, nullptr, {k}).cols[0];
}

// The build half of a join: `bkey`'s n keys as int64 beside their row numbers
// (NULL keys leave first), sorted, and every distinct key in the table.
JoinTable JoinBuildTable(Engine &e, DCol bkey, int64_t n, bool want_max_run) {
  JoinTable t;
  if (n > kJoinMaxBuildRows)
    ThrowError("Out of Range", "join input of " + std::to_string(n) + " rows, more than the 2147483647 a join side may have");
  if (bkey.phys > P_U64) ThrowError("Internal", "join key is not stored as an integer");
  int64_t nb = n;
  if (nb == 0) return t;
  auto keys = Alloc(e, nb * 8), keys2 = Alloc(e, nb * 8);
  t.rows2 = Alloc(e, nb * 8);
  DevBufPtr rows_buf;
  int64_t *rows = nullptr;
  DRel kept;  // owns the filtered key and row columns
  if (bkey.validity) {
    DRel kr;
    kr.n = nb;
    kr.cols.push_back(bkey);
    DCol rc = AllocOut(e, LogicalType(T_BIGINT), nb, false);
    dev::Iota((int64_t *)rc.data, nb, 0, e.stream);
    kr.cols.push_back(rc);
    auto notnull = std::make_shared<BExpr>();
    notnull->kind = BExpr::FUNC;
    notnull->op = B_ISNOTNULL;
    notnull->type = LogicalType(T_BOOLEAN);
    notnull->ch.push_back(ColRef(0, bkey.type));
    kept = FilterProject(e, kr, notnull, AllCols(kr));
    nb = kept.n;
    t.nulls = n - nb;
    if (nb == 0) return t;
    bkey = kept.cols[0];
    rows = (int64_t *)kept.cols[1].data;
    ProfScope ps(e, "join_keys", (double)nb * (PhysSize(bkey.phys) + 8), nb);
    dev::JoinKeys(bkey.data, bkey.phys, nb, (int64_t *)keys->p, nullptr, e.stream);
  } else {
    rows_buf = Alloc(e, nb * 8);
    rows = (int64_t *)rows_buf->p;
    ProfScope ps(e, "join_keys", (double)nb * (PhysSize(bkey.phys) + 16), nb);
    dev::JoinKeys(bkey.data, bkey.phys, nb, (int64_t *)keys->p, rows, e.stream);
  }
  {
    ProfScope ps(e, "radix_sort", (double)nb * 16 * 2, nb);
    dev::SortPairs((uint64_t *)keys->p, rows, (uint64_t *)keys2->p, (int64_t *)t.rows2->p, nb, e.stream);
  }
  t.nb = nb;
  t.cap = JoinCapacity(nb);
  t.tab = Alloc(e, (size_t)t.cap * sizeof(JoinEntry), true);
  if (want_max_run) t.max_run = Alloc(e, sizeof(uint32_t), true);
  {
    ProfScope ps(e, "join_build", (double)nb * 8 + (double)t.cap * sizeof(JoinEntry), nb);
    dev::JoinBuild((const int64_t *)keys2->p, nb, (JoinEntry *)t.tab->p, t.cap, e.d_err, e.stream,
                   t.max_run ? (uint32_t *)t.max_run->p : nullptr);
  }
  return t;
}

JoinPrepared JoinPrepare(Engine &e, Connection &c, const BoundSource &src, bool want_max_run) {
  JoinPrepared j;
  j.in[0] = SourceRel(e, c, *src.left);
  j.in[1] = SourceRel(e, c, *src.right);
  for (DRel &r : j.in) {
    SettleCount(e, r);
    // the virtual column of a range relation becomes a real one: the gather reads it by row number
    if (r.range) r = FilterProject(e, r, nullptr, AllCols(r));
  }
  if (j.in[0].n == 0 || j.in[1].n == 0) {
    j.empty = true;
    return j;
  }

  j.b = j.in[0].n < j.in[1].n ? 0 : 1, j.p = 1 - j.b;  // build side: fewer rows, the right input on a tie
  const DRel &build = j.in[j.b], &probe = j.in[j.p];
  if (build.n > kJoinMaxBuildRows || probe.n > kJoinMaxBuildRows)
    ThrowError("Out of Range", "join input of " + std::to_string(std::max(build.n, probe.n)) +
                                   " rows, more than the 2147483647 a join side may have");
  DCol bkey = KeyColumn(e, build, j.b == 0 ? src.left_key : src.right_key);
  j.pkey = KeyColumn(e, probe, j.p == 0 ? src.left_key : src.right_key);
  if (bkey.phys > P_U64 || j.pkey.phys > P_U64) ThrowError("Internal", "join key is not stored as an integer");

  const JoinTable t = JoinBuildTable(e, bkey, build.n, want_max_run);
  if (t.nb == 0) {  // every build key was NULL
    j.empty = true;
    return j;
  }
  j.rows2 = t.rows2, j.tab = t.tab, j.max_run = t.max_run;
  j.nb = t.nb, j.cap = t.cap;
  return j;
}

DRel JoinPairs(Engine &e, Connection &c, const BoundSource &src, const JoinPrepared &j) {
  if (j.empty) return EmptyJoin(e, j.in[0], j.in[1]);
  const int b = j.b, p = j.p;
  const DRel &build = j.in[b], &probe = j.in[p];
  const DCol &pkey = j.pkey;
  const int64_t cap = j.cap;

  // probe: counts, their offsets, the total
  const int64_t np = probe.n;
  auto counts = Alloc(e, np * 8), offs = Alloc(e, (np + 1) * 8), starts = Alloc(e, np * 4);
  {
    ProfScope ps(e, "join_probe_count", (double)np * (PhysSize(pkey.phys) + 12 + sizeof(JoinEntry)), np);
    dev::JoinProbeCount(pkey.data, pkey.phys, pkey.validity, np, (const JoinEntry *)j.tab->p, cap, (int64_t *)counts->p,
                        (int32_t *)starts->p, e.d_err, e.stream);
  }
  dev::ScanLengths((const int64_t *)counts->p, (int64_t *)offs->p, np, e.stream);
  const int64_t total = ReadDev<int64_t>(e, (const int64_t *)offs->p + np);
  CheckError(e);
  if (total > c.opts.join_max_rows)
    ThrowError("Out of Range", "join produces " + std::to_string(total) + " rows, more than mbx_join_max_rows");
  if (total == 0) return EmptyJoin(e, j.in[0], j.in[1]);

  // the result's row numbers on each side, then its columns
  auto pidx = Alloc(e, total * 8), bidx = Alloc(e, total * 8);
  {
    ProfScope ps(e, "join_expand", (double)total * 24 + (double)np * 12, total);
    dev::JoinExpand((const int64_t *)offs->p, (const int32_t *)starts->p, np, total, (const int64_t *)j.rows2->p,
                    (int64_t *)pidx->p, (int64_t *)bidx->p, e.stream);
  }
  DRel side[2];
  {
    // per output row and fixed-width column: the row number, the value read, the value written
    double gbytes = 0;
    for (const DRel *r : {&probe, &build})
      for (const DCol &d : r->cols)
        if (d.phys != P_STR) gbytes += (double)total * (8 + 2 * PhysSize(d.phys));
    ProfScope ps(e, "join_gather", gbytes, total);
    side[p] = GatherRel(e, probe, (const int64_t *)pidx->p, total);
    side[b] = GatherRel(e, build, (const int64_t *)bidx->p, total);
  }
  DRel out;
  out.n = total;
  out.cols = side[0].cols;
  out.cols.insert(out.cols.end(), side[1].cols.begin(), side[1].cols.end());
  if (src.residual) out = FilterProject(e, out, src.residual, AllCols(out));
  return out;
}

DRel JoinRel(Engine &e, Connection &c, const BoundSource &src) { return JoinPairs(e, c, src, JoinPrepare(e, c, src)); }

// ---------------------------------------------------------------------------
// the fused probe-and-aggregate (join_agg_plan.h)
// ---------------------------------------------------------------------------
namespace {

// a VARCHAR value anywhere in the tree: a column, a constant, an argument, an operand of a predicate
bool HasVarchar(const BExprPtr &x) {
  if (!x) return false;
  if (ClassOf(x->type) == VC_STR) return true;
  for (auto &ch : x->ch)
    if (HasVarchar(ch)) return true;
  return false;
}

// The program of the three stages over `joined` (the left input's columns, then
// the right one's, in place), or false where the compiler refuses one.
struct JoinAggProgram {
  VmProgram P;
  dev::VmCols cols;
  int end_residual = 0, end_where = 0, residual_reg = 255, where_reg = 255;
  uint32_t build_mask = 0;
  double probe_bytes = 0, build_bytes = 0;  // the referenced columns of each side, per pair
};

bool CompileJoinAgg(const DRel &joined, size_t nleft, int build_side, const BoundSource &src, const BoundSelect &s,
                    JoinAggProgram &out) {
  const int na = (int)s.aggs.size();
  VmCompiler vc(joined, nullptr);
  try {
    if (src.residual) out.residual_reg = vc.Compile(*src.residual);
    out.end_residual = vc.P.n_ins;
    if (s.where) out.where_reg = vc.Compile(*s.where);
    out.end_where = vc.P.n_ins;
    // the predicates' registers stay allocated: a later stage must not reuse them before they are read
    for (int j = 0; j < na; j++) {
      const AggSpec &a = s.aggs[j];
      if (a.kind == A_COUNT_STAR) {
        vc.P.out_reg[j] = 255;
        continue;
      }
      vc.P.out_reg[j] = (uint8_t)vc.Compile(*a.arg);
      vc.P.out_class[j] = (uint8_t)ClassOf(a.arg->type);
      // statistics the kernel accumulates: bit0 sum (SUM/AVG), bit1 min/max; COUNT only counts
      vc.P.out_phys[j] = a.kind == A_SUM || a.kind == A_AVG ? 1 : a.kind == A_MIN || a.kind == A_MAX ? 2 : 4;
    }
  } catch (std::exception &) {
    return false;  // the materialising path raises the same error if it applies
  }
  vc.P.pred_reg = (uint8_t)out.where_reg;
  vc.P.pred_ins = (uint8_t)out.end_where;
  vc.P.n_out = na;
  vc.P.n_regs = vc.high;
  out.P = vc.P;
  out.cols = vc.cols;
  for (size_t col = 0; col < vc.colmap.size(); col++) {
    if (vc.colmap[col] < 0) continue;
    const bool on_build = (col >= nleft) == (build_side == 1);
    const double bytes = PhysSize(joined.cols[col].phys) + (joined.cols[col].validity ? 1.0 / 8 : 0);
    if (on_build) out.build_mask |= 1u << vc.colmap[col];
    (on_build ? out.build_bytes : out.probe_bytes) += bytes;
  }
  return true;
}

}  // namespace

DRel JoinAggregate(Engine &e, Connection &c, const BoundSelect &s) {
  const BoundSource &src = s.src;
  const int na = (int)s.aggs.size();
  JoinAggFacts f;
  f.enabled = c.opts.join_agg;
  f.n_aggs = na;
  f.max_aggs = VM_MAX_OUT;
  f.max_run_limit = c.opts.join_agg_max_run;
  f.varchar = HasVarchar(src.residual) || HasVarchar(s.where);
  f.membership = HasMembership(src.residual) || HasMembership(s.where);
  for (auto &a : s.aggs) {
    f.membership |= HasMembership(a.arg);
    f.distinct |= a.distinct;
    f.varchar |= HasVarchar(a.arg);
    f.minmax_128 |= a.arg && (a.kind == A_MIN || a.kind == A_MAX) && ClassOf(a.arg->type) == VC_I128;
  }
  // what the statement itself decides is known before anything runs; the
  // compiler's verdict and the longest run need the prepared join
  bool take = JoinAggDecide(f).take;
  const JoinPrepared j = JoinPrepare(e, c, src, take);
  take = take && !j.empty;  // no pair: the aggregate over no rows, from the path that has always given it
  JoinAggProgram prog;
  if (take) {
    DRel joined;  // virtual: both inputs' columns where they are, un-gathered
    joined.cols = j.in[0].cols;
    joined.cols.insert(joined.cols.end(), j.in[1].cols.begin(), j.in[1].cols.end());
    joined.n = j.in[j.p].n;
    f.compile_failed = !CompileJoinAgg(joined, j.in[0].cols.size(), j.b, src, s, prog);
    // the longest run comes back with the error word of the build
    HIPCHK(hipMemcpyAsync(e.h_pinned, e.d_err, sizeof(int32_t), hipMemcpyDeviceToHost, e.stream));
    HIPCHK(hipMemcpyAsync(e.h_pinned + 8, j.max_run->p, sizeof(uint32_t), hipMemcpyDeviceToHost, e.stream));
    HIPCHK(hipStreamSynchronize(e.stream));
    int32_t err;
    uint32_t max_run;
    memcpy(&err, e.h_pinned, sizeof(err));
    memcpy(&max_run, e.h_pinned + 8, sizeof(max_run));
    RaiseDeviceError(e, err);
    f.max_run = std::max<uint32_t>(max_run, 1);  // runs of one row leave the word alone
    const JoinAggChoice ch = JoinAggDecide(f);
    take = ch.take;
    if (!take && Knob("MBX_JOIN_AGG_DEBUG")) fprintf(stderr, "join_probe_agg declined: %s\n", ch.reason);
  }
  if (!take) return Aggregate(e, JoinPairs(e, c, src, j), s);

  const DRel &probe = j.in[j.p];
  const int blocks = dev::JoinProbeAggBlocks(probe.n);
  const int nrec = std::max(na, 1);
  auto partials = Alloc(e, (size_t)blocks * nrec * sizeof(JoinAggRec));
  auto block_counts = Alloc(e, (size_t)blocks * 2 * 8);
  auto states = Alloc(e, (size_t)nrec * sizeof(dev::AggState));
  auto counts = Alloc(e, 2 * 8);
  dev::JoinAggArgs A;
  memset(&A, 0, sizeof(A));
  A.key = j.pkey.data;
  A.key_phys = j.pkey.phys;
  A.key_valid = j.pkey.validity;
  A.n = probe.n;
  A.tab = (const JoinEntry *)j.tab->p;
  A.cap = j.cap;
  A.build_rows = (const int64_t *)j.rows2->p;
  A.end_residual = prog.end_residual;
  A.end_where = prog.end_where;
  A.residual_reg = prog.residual_reg;
  A.where_reg = prog.where_reg;
  A.build_mask = prog.build_mask;
  const double partial_bytes = (double)blocks * (na * sizeof(JoinAggRec) + 16);
  size_t ev = 0;
  {
    // the key and one entry per probe row and the partials; the pairs' share is added once their count is known
    ProfScope ps(e, "join_probe_agg", (double)probe.n * (PhysSize(j.pkey.phys) + sizeof(JoinEntry)) + partial_bytes,
                 probe.n);
    if (ps.on) ev = ps.idx;
    dev::JoinProbeAgg(prog.P, prog.cols, A, (JoinAggRec *)partials->p, (unsigned long long *)block_counts->p, blocks,
                      e.d_err, e.stream);
  }
  {
    ProfScope ps(e, "join_agg_fold", partial_bytes + (double)na * sizeof(dev::AggState) + 16, blocks);
    dev::JoinAggFold((const JoinAggRec *)partials->p, (const unsigned long long *)block_counts->p, blocks, na,
                     (dev::AggState *)states->p, (unsigned long long *)counts->p, e.stream);
  }
  // the pair count and the error word in one copy: the limit is raised before
  // any expression's error, as where the pairs are materialised, and the error
  // word is clear after either
  HIPCHK(hipMemcpyAsync(e.h_pinned, counts->p, 16, hipMemcpyDeviceToHost, e.stream));
  HIPCHK(hipMemcpyAsync(e.h_pinned + 16, e.d_err, sizeof(int32_t), hipMemcpyDeviceToHost, e.stream));
  HIPCHK(hipStreamSynchronize(e.stream));
  uint64_t kept_pairs[2];
  int32_t err;
  memcpy(kept_pairs, e.h_pinned, 16);
  memcpy(&err, e.h_pinned + 16, sizeof(err));
  const uint64_t pairs = kept_pairs[1];
  if (e.profile) e.events[ev].bytes += (double)pairs * (8 + prog.probe_bytes + prog.build_bytes);
  if (pairs > (uint64_t)c.opts.join_max_rows) {
    if (err) HIPCHK(hipMemsetAsync(e.d_err, 0, sizeof(int32_t), e.stream));
    ThrowError("Out of Range", "join produces " + std::to_string(pairs) + " rows, more than mbx_join_max_rows");
  }
  RaiseDeviceError(e, err);
  DRel out = EmitGlobalStates(e, s, (const unsigned long long *)counts->p, (dev::AggState *)states->p);
  HIPCHK(hipStreamSynchronize(e.stream));  // states / count buffers released after the emit
  return out;
}

}  // namespace mbx
