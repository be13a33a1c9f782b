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
#include "exec.h"
#include "join_plan.h"

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

// a key that is a bare column is read in place; anything else is evaluated
DCol KeyColumn(Engine &e, const DRel &r, const BExprPtr &k) {
  if (k->kind == BExpr::COL && !(r.range && k->col == 0)) return r.cols[k->col];
  return FilterProject(e, r, nullptr, {k}).cols[0];
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

DRel JoinRel(Engine &e, Connection &c, const BoundSource &src) {
  DRel in[2] = {SourceRel(e, c, *src.left), SourceRel(e, c, *src.right)};
  for (DRel &r : in) {
    SettleCount(e, r);
    // the virtual column of a range relation becomes a real one: the gather reads it by row number
    if (r.range) r = FilterProject(e, r, nullptr, AllCols(r));
  }
  if (in[0].n == 0 || in[1].n == 0) return EmptyJoin(e, in[0], in[1]);

  const int b = in[0].n < in[1].n ? 0 : 1, p = 1 - b;  // build side: fewer rows, the right input on a tie
  const DRel &build = in[b], &probe = in[p];
  if (build.n > kJoinMaxBuildRows || probe.n > kJoinMaxBuildRows)
    ThrowError("Out of Range", "join input of " + std::to_string(std::max(build.n, probe.n)) +
                                   " rows, more than the 2147483647 a join side may have");
  DCol bkey = KeyColumn(e, build, b == 0 ? src.left_key : src.right_key);
  const DCol pkey = KeyColumn(e, probe, p == 0 ? src.left_key : src.right_key);
  if (bkey.phys > P_U64 || pkey.phys > P_U64) ThrowError("Internal", "join key is not stored as an integer");

  // build keys as int64 beside their row numbers; NULL keys leave first
  int64_t nb = build.n;
  auto keys = Alloc(e, nb * 8), keys2 = Alloc(e, nb * 8), rows2 = Alloc(e, nb * 8);
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
    if (nb == 0) return EmptyJoin(e, in[0], in[1]);
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
    dev::SortPairs((uint64_t *)keys->p, rows, (uint64_t *)keys2->p, (int64_t *)rows2->p, nb, e.stream);
  }
  const int64_t cap = JoinCapacity(nb);
  auto tab = Alloc(e, (size_t)cap * sizeof(JoinEntry), true);
  {
    ProfScope ps(e, "join_build", (double)nb * 8 + (double)cap * sizeof(JoinEntry), nb);
    dev::JoinBuild((const int64_t *)keys2->p, nb, (JoinEntry *)tab->p, cap, e.d_err, e.stream);
  }

  // probe: counts, their offsets, the total
  const int64_t np = probe.n;
  auto counts = Alloc(e, np * 8), offs = Alloc(e, (np + 1) * 8), starts = Alloc(e, np * 4);
  {
    ProfScope ps(e, "join_probe_count", (double)np * (PhysSize(pkey.phys) + 12 + sizeof(JoinEntry)), np);
    dev::JoinProbeCount(pkey.data, pkey.phys, pkey.validity, np, (const JoinEntry *)tab->p, cap, (int64_t *)counts->p,
                        (int32_t *)starts->p, e.d_err, e.stream);
  }
  dev::ScanLengths((const int64_t *)counts->p, (int64_t *)offs->p, np, e.stream);
  const int64_t total = ReadDev<int64_t>(e, (const int64_t *)offs->p + np);
  CheckError(e);
  if (total > c.opts.join_max_rows)
    ThrowError("Out of Range", "join produces " + std::to_string(total) + " rows, more than mbx_join_max_rows");
  if (total == 0) return EmptyJoin(e, in[0], in[1]);

  // the result's row numbers on each side, then its columns
  auto pidx = Alloc(e, total * 8), bidx = Alloc(e, total * 8);
  {
    ProfScope ps(e, "join_expand", (double)total * 24 + (double)np * 12, total);
    dev::JoinExpand((const int64_t *)offs->p, (const int32_t *)starts->p, np, total, (const int64_t *)rows2->p,
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

}  // namespace mbx
