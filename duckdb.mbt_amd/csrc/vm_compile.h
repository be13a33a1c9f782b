// vm_compile.h -- bound expressions compiled to a tile program of the device VM
// (vm.h); shared by the filter / project pipeline (executor.cpp) and the
// run-time compiled aggregates (aggregate.cpp).
#pragma once
#include "exec.h"
#include "vm.h"

namespace mbx {

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

  // errcode: what a value outside [lo, hi] raises (a cast: E_CAST_RANGE; the
  // result of an arithmetic step: that step's overflow code, as the host folder)
  int RangeCheck(int r, VClass vc, i128 lo, i128 hi, int errcode = E_CAST_RANGE) {
    return Step1(vc == VC_I128 ? V_CHECK_L : V_CHECK_I, r, Const(lo), Const(hi), errcode);
  }
  // Result check of integer arithmetic in a type narrower than its register
  // class: TINYINT..INTEGER and the unsigned types in 64 bits, UBIGINT in 128.
  int CheckArith(int d, VClass vc, const LogicalType &t, int errcode) {
    bool narrow = vc == VC_I64 ? (IsIntegral(t.id) && t.id != T_BIGINT) : (vc == VC_I128 && t.id == T_UBIGINT);
    if (!narrow) return d;
    i128 lo, hi;
    IntegralRange(t.id, &lo, &hi);
    return RangeCheck(d, vc, lo, hi, errcode);
  }

  // rounds to FLOAT: x * 1.0 keeps the sign of a zero (x + 0.0 would not)
  int ToFloat32(int r) {
    int z = LoadConst(ConstF(1.0));
    return Step2(V_MUL_F, r, z, 1);
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
      // rescale in the wider of the two classes: a 128-bit value may fit the
      // 64-bit target only after it has been scaled down
      VClass wc = fc == VC_I128 ? fc : tc;
      int x = ToClass(r, fc, wc);
      int ds = to.scale - fs;
      if (ds > 0) x = Step1(wc == VC_I128 ? V_SCALEUP_L : V_SCALEUP_I, x, 0, 0, ds);
      else if (ds < 0) x = Step1(wc == VC_I128 ? V_SCALEDN_L : V_SCALEDN_I, x, 0, 0, -ds);
      i128 lim = Pow10(to.width) - 1;
      if (wc != tc) return Step1(V_L2I, x, Const(-lim), Const(lim));
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
        // a VARCHAR column against a constant or another column never gets here (LowerStringPredicates)
        if (cc == VC_STR)
          ThrowError("Not implemented", "a VARCHAR comparison whose operand is a string expression (lower(s), s || 'x', a "
                                        "cast) is not supported on the MI355X device path: " + ExprToString(e));
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
        return CheckArith(Step1(op, a), vc, t, E_OVF_NEG);
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
        return CheckArith(Step2(op, a, b), vc, t,
                          e.op == B_ADD ? E_OVF_ADD : e.op == B_SUB ? E_OVF_SUB : e.op == B_MUL ? E_OVF_MUL : E_OVF_NEG);
      }
      case B_LIKE: case B_PREFIX: case B_SUFFIX: case B_CONTAINS:
        // over a VARCHAR column these never get here (LowerStringPredicates)
        ThrowError("Not implemented", "a VARCHAR match over anything but a VARCHAR column of the scanned relation is not "
                                      "supported on the MI355X device path: " + ExprToString(e));
      case B_IN_SUBQUERY:
        // lowered to a BOOLEAN column before any program is compiled (LowerStringPredicates)
        ThrowError("Internal", "an IN (subquery) leaf reached the expression compiler: " + ExprToString(e));
      default:
        ThrowError("Not implemented", "function " + ExprToString(e) + " is not supported on the MI355X device path");
    }
  }
};

}  // namespace mbx
