// window.cpp — window functions: f(arg) OVER (PARTITION BY .. ORDER BY .. frame)
// in the select list of a non-aggregate select (kernels: window_kernels.hip;
// the operator, the states and the frame resolution: window_plan.h).
//
//   1. FilterProject gives the base relation: the source columns after WHERE
//      and, appended, one evaluated column per distinct key or argument
//      expression (a bare column is read where it is).
//   2. Once per specification (partition keys, order items): the stable LSD
//      sort's permutation of the base rows (SortPerm; OVER () has none, the
//      identity), then window_bounds marks where partitions and peer groups
//      start, comparing neighbours through the sort's own key encoding.
//   3. Per specification the extents its calls need (a partition's / peer
//      group's first and last position) and per call its running state, each a
//      segmented scan of three launches; then window_emit writes the call's
//      column at every row's ORIGINAL position: the rows do not move.
//   4. FilterProject evaluates the select's outputs over [source columns,
//      window columns].
#include <algorithm>
#include <map>
#include <string>
#include <vector>

#include "exec.h"
#include "window_plan.h"

namespace mbx {

namespace {

// the columns of the base relation that key and argument expressions read
struct BaseCols {
  int nsrc = 0;
  std::vector<BExprPtr> extra;  // evaluated behind the source columns
  std::map<std::string, int> slot;
  int Of(const BExprPtr &x) {
    if (x->kind == BExpr::COL) return x->col;
    const std::string key = ExprToString(*x) + " :: " + x->type.ToString();
    auto it = slot.find(key);
    if (it != slot.end()) return it->second;
    extra.push_back(x);
    return slot[key] = nsrc + (int)extra.size() - 1;
  }
};

BExprPtr ColExpr(int c, const LogicalType &t) {
  auto x = std::make_shared<BExpr>();
  x->kind = BExpr::COL;
  x->col = c;
  x->type = t;
  return x;
}

// one specification's sort and what was derived from it so far
struct SpecState {
  bool ready = false;
  DevBufPtr perm, flags;  // perm null: the identity
  DevBufPtr ext[4];       // part_first, part_last, peer_first, peer_last (int32), made on demand
};

struct WindowRun {
  Engine &e;
  int64_t n;
  DevBufPtr carry;  // every scan's carries: one buffer, reused on the stream

  // a segmented scan: its three launches
  void Scan(dev::WinScanDesc D) {
    D.n = n;
    D.carry = carry->p;
    const double state_bytes = (double)n * (D.op == dev::WOP_POS ? 4 : dev::WinStateBytes(D.op));
    double in_bytes = (double)n;  // the flags
    if (D.src == dev::WSRC_COL) in_bytes += (double)n * ((D.perm ? 8 : 0) + PhysSize((Phys)D.phys));
    const double carry_bytes = (double)WinTiles(n) * dev::WinCarryBytes(D.op);
    {
      ProfScope ps(e, "window_scan_reduce", in_bytes + carry_bytes, n);
      dev::WindowScanReduce(D, e.stream);
    }
    {
      ProfScope ps(e, "window_scan_carry", 2 * carry_bytes, WinTiles(n));
      dev::WindowScanCarry(D, e.stream);
    }
    {
      ProfScope ps(e, "window_scan_apply", in_bytes + carry_bytes + state_bytes, n);
      dev::WindowScanApply(D, e.stream);
    }
  }

  const int32_t *Extent(SpecState &sp, int which) {
    if (!sp.ext[which]) {
      sp.ext[which] = Alloc(e, n * 4);
      dev::WinScanDesc D;
      memset(&D, 0, sizeof(D));
      D.op = dev::WOP_POS;
      D.src = dev::WSRC_POS;
      D.backward = which & 1;
      D.seg_bit = which < 2 ? dev::kWinPartStart : dev::kWinPeerStart;
      D.flags = (const uint8_t *)sp.flags->p;
      D.out = sp.ext[which]->p;
      Scan(D);
    }
    return (const int32_t *)sp.ext[which]->p;
  }
};

}  // namespace

DRel WindowBranch(Engine &e, const BoundSelect &s, const DRel &src) {
  BaseCols bc;
  bc.nsrc = (int)src.cols.size();
  // ---- 1. the base relation
  struct CallCols {
    int arg = -1;
    std::vector<int> keys;  // partition keys, then order keys
  };
  std::vector<CallCols> cc(s.windows.size());
  for (size_t i = 0; i < s.windows.size(); i++) {
    const WindowCall &w = s.windows[i];
    if (w.arg) cc[i].arg = bc.Of(w.arg);
    for (auto &p : w.partition) cc[i].keys.push_back(bc.Of(p));
    for (auto &o : w.order) cc[i].keys.push_back(bc.Of(o.expr));
    if (cc[i].keys.size() > WIN_MAX_KEYS)
      ThrowError("Not implemented", "a window with more than " + std::to_string(WIN_MAX_KEYS) +
                                        " PARTITION BY and ORDER BY keys is not supported by the MI355X backend");
  }
  std::vector<BExprPtr> cols;
  for (int c = 0; c < bc.nsrc; c++) cols.push_back(ColExpr(c, src.cols[c].type));
  DRel base;
  if (s.where) {
    std::vector<BExprPtr> all = cols;
    all.insert(all.end(), bc.extra.begin(), bc.extra.end());
    base = FilterProject(e, src, s.where, all);
  } else {
    base = FilterProject(e, src, nullptr, cols);  // in place, but for a range's virtual column
    base.n = src.n;
    if (!bc.extra.empty()) {
      DRel x = FilterProject(e, src, nullptr, bc.extra);
      base.cols.insert(base.cols.end(), x.cols.begin(), x.cols.end());
    }
  }
  base.tail = nullptr;
  const int64_t n = base.n;
  if (n > INT32_MAX)
    ThrowError("Out of Range", "window functions over more than 2^31 - 1 rows are not supported by the MI355X backend");

  // ---- 2. and 3.
  WindowRun run{e, n, nullptr};
  size_t carry_elem = 0;
  for (int op = dev::WOP_POS; op <= dev::WOP_MAX128; op++) carry_elem = std::max(carry_elem, dev::WinCarryBytes(op));
  if (n > 0) run.carry = Alloc(e, (size_t)WinTiles(n) * carry_elem);
  std::map<int, SpecState> specs;
  DRel rel;
  rel.n = n;
  for (int c = 0; c < bc.nsrc; c++) rel.cols.push_back(base.cols[c]);
  for (size_t i = 0; i < s.windows.size(); i++) {
    const WindowCall &w = s.windows[i];
    const bool never_null = w.kind <= W_COUNT;  // the ranks and the counts
    DCol out = AllocOut(e, w.type, n, !never_null);
    if (n == 0) {
      rel.cols.push_back(out);
      continue;
    }
    SpecState &sp = specs[w.spec];
    if (!sp.ready) {
      std::vector<BoundOrder> order;
      for (size_t k = 0; k < cc[i].keys.size(); k++) {
        BoundOrder bo;
        if (k >= w.partition.size()) bo = w.order[k - w.partition.size()];
        bo.expr = ColExpr(cc[i].keys[k], base.cols[cc[i].keys[k]].type);
        order.push_back(bo);
      }
      sp.perm = SortPerm(e, base, order);
      dev::WinKeys K;
      memset(&K, 0, sizeof(K));
      K.nkeys = (int32_t)cc[i].keys.size();
      K.npart = (int32_t)w.partition.size();
      double key_bytes = 0;
      for (int k = 0; k < K.nkeys; k++) {
        const DCol &kc = base.cols[cc[i].keys[k]];
        if (kc.phys == P_STR || kc.phys == P_I128 || kc.phys == P_INTERVAL || !kc.data)
          ThrowError("Internal", "a window key the binder should have refused");
        K.k[k].data = kc.data;
        K.k[k].valid = kc.validity;
        K.k[k].phys = kc.phys;
        key_bytes += 2.0 * PhysSize(kc.phys);
      }
      sp.flags = Alloc(e, n);
      {
        ProfScope ps(e, "window_bounds", (double)n * (key_bytes + (sp.perm ? 8 : 0) + 1), n);
        dev::WindowBounds(K, sp.perm ? (const int64_t *)sp.perm->p : nullptr, n, (uint8_t *)sp.flags->p, e.stream);
      }
      sp.ready = true;
    }
    const int64_t *perm = sp.perm ? (const int64_t *)sp.perm->p : nullptr;

    dev::WinEmitDesc E;
    memset(&E, 0, sizeof(E));
    E.kind = w.kind;
    E.target = w.target;
    E.n = n;
    E.perm = perm;
    E.offset = w.offset;
    E.out = out.data;
    E.out_phys = out.phys;
    E.out_valid = (uint32_t *)out.validity;
    DevBufPtr state;
    const DCol *arg = cc[i].arg >= 0 ? &base.cols[cc[i].arg] : nullptr;
    if (arg && (arg->phys == P_STR || arg->phys == P_INTERVAL || !arg->data))
      ThrowError("Internal", "a window argument the binder should have refused");
    if (arg) E.in_phys = arg->phys;
    // the running state, where the call has one
    int op = -1, scan_src = dev::WSRC_COL;
    switch (w.kind) {
      case W_DENSE_RANK: op = dev::WOP_COUNT, scan_src = dev::WSRC_PEER; break;
      case W_COUNT: op = dev::WOP_COUNT; break;
      case W_SUM:
      case W_AVG: op = (arg->phys == P_F64 || arg->phys == P_F32) ? dev::WOP_SUMF : dev::WOP_SUM128; break;
      case W_MIN: op = arg->phys == P_I128 ? dev::WOP_MIN128 : dev::WOP_MIN64; break;
      case W_MAX: op = arg->phys == P_I128 ? dev::WOP_MAX128 : dev::WOP_MAX64; break;
      default: break;
    }
    if (op >= 0) {
      state = Alloc(e, (size_t)n * dev::WinStateBytes(op));
      dev::WinScanDesc D;
      memset(&D, 0, sizeof(D));
      D.op = op;
      D.src = scan_src;
      D.seg_bit = dev::kWinPartStart;
      D.flags = (const uint8_t *)sp.flags->p;
      D.perm = perm;
      if (scan_src == dev::WSRC_COL) {
        D.data = arg->data;
        D.valid = arg->validity;
        D.phys = arg->phys;
      }
      D.out = state->p;
      run.Scan(D);
      E.op = op;
      E.state = state->p;
    }
    if (w.kind == W_AVG && w.arg->type.id == T_DECIMAL) E.avg_scale = w.arg->type.scale;
    // the extents the emit reads
    const bool part_first = w.kind == W_ROW_NUMBER || w.kind == W_RANK || w.kind == W_COUNT_STAR || w.kind == W_LAG;
    if (part_first) E.part_first = run.Extent(sp, 0);
    if (w.target == WT_PART_END || w.kind == W_LEAD) E.part_last = run.Extent(sp, 1);
    if (w.kind == W_RANK) E.peer_first = run.Extent(sp, 2);
    if (w.target == WT_PEER_END) E.peer_last = run.Extent(sp, 3);
    if (w.kind == W_LAG || w.kind == W_LEAD) {
      E.data = arg->data;
      E.valid = arg->validity;
    }
    {
      const double bytes = (double)n * ((perm ? 8 : 0) + PhysSize(out.phys) + (op >= 0 ? dev::WinStateBytes(op) : 0) +
                                        4.0 * (!!E.part_first + !!E.part_last + !!E.peer_first + !!E.peer_last));
      ProfScope ps(e, "window_emit", bytes, n);
      dev::WindowEmit(E, e.stream);
    }
    rel.cols.push_back(out);
  }
  // ---- 4. the select's outputs
  return FilterProject(e, rel, nullptr, s.outputs);
}

}  // namespace mbx
