// str_match.h — VARCHAR predicates: the byte-wise comparison and the LIKE
// matcher, once, for the binder's constant folder and for the str_match
// kernels (str_kernels.hip).  A predicate over one string column and a constant
// is a StrMatchPlan, made on the host and passed to the kernel by value: the
// operator, the form the host chose for it and the constant's bytes.
//
// Semantics: strings are byte strings.  The order is byte-wise
// on unsigned bytes, a proper prefix is smaller (DuckDB's binary collation).
// In a LIKE pattern '%' matches any run of bytes, '_' one UTF-8 code point (a
// byte and the 10xxxxxx continuation bytes after it), the escape byte makes the
// next pattern byte literal, every other byte matches itself.
// No HIP types: the header also builds in a plain host program.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__)
#define MBX_SM_HD __host__ __device__ __forceinline__
#else
#define MBX_SM_HD inline
#endif

namespace mbx {

enum StrOp : uint8_t { SM_EQ = 0, SM_NE, SM_LT, SM_LE, SM_GT, SM_GE, SM_DISTINCT, SM_NOT_DISTINCT, SM_LIKE };
// What the row loop runs.  SF_COMPARE: `op` against the constant; the others are
// LIKE patterns by shape: no wildcard, 'abc%', '%abc', '%abc%', only '%'s,
// anything else.
enum StrForm : uint8_t { SF_COMPARE = 0, SF_EXACT, SF_PREFIX, SF_SUFFIX, SF_CONTAINS, SF_ALL, SF_GENERAL, SF_FORMS };
enum StrTok : uint8_t { ST_LIT = 0, ST_ANY = 1, ST_ONE = 2 };  // a literal byte, '%', '_'

constexpr int kStrMatchCap = 255;  // longest constant / pattern in bytes

struct StrMatchPlan {
  uint8_t op;    // StrOp
  uint8_t form;  // StrForm
  uint8_t has_escape, escape;
  int32_t len;                      // bytes[0 .. len)
  uint8_t bytes[kStrMatchCap + 1];  // the constant; the literal of EXACT .. CONTAINS; GENERAL: the pattern, unescaped,
  uint8_t kind[kStrMatchCap + 1];   // ... with the StrTok of every position ('%%' collapsed to one ST_ANY)
};

enum StrPlanStatus { SP_OK = 0, SP_TRAILING_ESCAPE = 1, SP_TOO_LONG = 2 };

// -1 / 0 / 1: unsigned bytes, then the shorter string first
MBX_SM_HD int StrCompare(const uint8_t *a, int64_t la, const uint8_t *b, int64_t lb) {
  const int64_t m = la < lb ? la : lb;
  for (int64_t i = 0; i < m; i++) {
    const uint8_t x = a[i], y = b[i];
    if (x != y) return x < y ? -1 : 1;
  }
  return la < lb ? -1 : la > lb ? 1 : 0;
}

MBX_SM_HD bool StrBytesEqual(const uint8_t *a, const uint8_t *b, int64_t n) {
  for (int64_t i = 0; i < n; i++)
    if (a[i] != b[i]) return false;
  return true;
}

MBX_SM_HD bool StrCompareOp(int op, int c) {
  switch (op) {
    case SM_EQ: case SM_NOT_DISTINCT: return c == 0;
    case SM_NE: case SM_DISTINCT: return c != 0;
    case SM_LT: return c < 0;
    case SM_LE: return c <= 0;
    case SM_GT: return c > 0;
    default: return c >= 0;
  }
}

// 'const OP column' as 'column OP const'
inline uint8_t StrFlipOp(uint8_t op) {
  return op == SM_LT ? SM_GT : op == SM_GT ? SM_LT : op == SM_LE ? SM_GE : op == SM_GE ? SM_LE : op;
}

inline StrPlanStatus PlanStrCompare(uint8_t op, const uint8_t *c, int64_t len, StrMatchPlan *out) {
  *out = StrMatchPlan();
  if (len > kStrMatchCap) return SP_TOO_LONG;
  out->op = op;
  out->form = SF_COMPARE;
  out->len = (int32_t)len;
  for (int64_t i = 0; i < len; i++) out->bytes[i] = c[i];
  return SP_OK;
}

// Classifies a LIKE pattern, unescaping as it goes.  general: keep SF_GENERAL
// whatever the shape (the forms are tested against it).
inline StrPlanStatus PlanLike(const uint8_t *pat, int64_t plen, bool has_escape, uint8_t escape, StrMatchPlan *out,
                              bool general = false) {
  *out = StrMatchPlan();
  out->op = SM_LIKE;
  out->has_escape = has_escape;
  out->escape = escape;
  int n = 0, lits = 0, ones = 0;
  for (int64_t i = 0; i < plen; i++) {
    uint8_t b = pat[i], k = ST_LIT;
    if (has_escape && b == escape) {
      if (i + 1 >= plen) return SP_TRAILING_ESCAPE;
      b = pat[++i];
    } else if (b == '%') {
      k = ST_ANY;
    } else if (b == '_') {
      k = ST_ONE;
    }
    if (k == ST_ANY && n > 0 && out->kind[n - 1] == ST_ANY) continue;
    if (n >= kStrMatchCap) return SP_TOO_LONG;
    out->bytes[n] = k == ST_LIT ? b : 0;
    out->kind[n++] = k;
    lits += k == ST_LIT;
    ones += k == ST_ONE;
  }
  out->len = n;
  out->form = SF_GENERAL;
  if (general) return SP_OK;
  const bool any_first = n > 0 && out->kind[0] == ST_ANY, any_last = n > 0 && out->kind[n - 1] == ST_ANY;
  const int anys = n - lits - ones;
  int form = SF_GENERAL, from = 0;
  if (ones == 0 && anys == 0) form = SF_EXACT;
  else if (ones == 0 && lits == 0) form = SF_ALL;  // n == 1: one collapsed '%'
  else if (ones == 0 && anys == 1 && any_last) form = SF_PREFIX;
  else if (ones == 0 && anys == 1 && any_first) form = SF_SUFFIX, from = 1;
  else if (ones == 0 && anys == 2 && any_first && any_last) form = SF_CONTAINS, from = 1;
  if (form == SF_GENERAL) return SP_OK;
  for (int i = 0; i < lits; i++) out->bytes[i] = out->bytes[from + i];
  for (int i = 0; i < n; i++) out->kind[i] = ST_LIT;
  out->form = (uint8_t)form;
  out->len = lits;
  return SP_OK;
}

// The GENERAL form: iterative two-pointer wildcard match.  It remembers the last
// '%' and the string position to retry from, so it neither recurses nor
// allocates and its work is bounded by len x pattern length.
MBX_SM_HD bool LikeMatch(const uint8_t *pb, const uint8_t *pk, int plen, const uint8_t *s, int64_t len) {
  int64_t si = 0, retry_s = 0;
  int pi = 0, star = -1;
  while (si < len) {
    if (pi < plen) {
      const uint8_t k = pk[pi];
      if (k == ST_ANY) {
        star = pi++;
        retry_s = si;
        continue;
      }
      if (k == ST_ONE) {
        si++;
        while (si < len && (s[si] & 0xC0) == 0x80) si++;
        pi++;
        continue;
      }
      if (pb[pi] == s[si]) {
        si++;
        pi++;
        continue;
      }
    }
    if (star < 0) return false;
    pi = star + 1;
    si = ++retry_s;
  }
  while (pi < plen && pk[pi] == ST_ANY) pi++;
  return pi == plen;
}

// One row of a plan of form FORM and (SF_COMPARE) operator OP; pb / pk: the
// plan's bytes / kind (the kernels keep a copy in LDS).
template <int FORM, int OP>
MBX_SM_HD bool StrMatchRowT(const uint8_t *pb, const uint8_t *pk, int plen, const uint8_t *s, int64_t len) {
  if constexpr (FORM == SF_COMPARE) {
    if constexpr (OP == SM_EQ || OP == SM_NE || OP == SM_DISTINCT || OP == SM_NOT_DISTINCT) {
      const bool eq = len == plen && StrBytesEqual(s, pb, len);  // lengths before any byte
      return (OP == SM_EQ || OP == SM_NOT_DISTINCT) ? eq : !eq;
    } else {
      return StrCompareOp(OP, StrCompare(s, len, pb, plen));
    }
  } else if constexpr (FORM == SF_EXACT) {
    return len == plen && StrBytesEqual(s, pb, len);
  } else if constexpr (FORM == SF_PREFIX) {
    return len >= plen && StrBytesEqual(s, pb, plen);
  } else if constexpr (FORM == SF_SUFFIX) {
    return len >= plen && StrBytesEqual(s + (len - plen), pb, plen);
  } else if constexpr (FORM == SF_CONTAINS) {
    for (int64_t i = 0; i + plen <= len; i++)
      if (StrBytesEqual(s + i, pb, plen)) return true;
    return false;
  } else if constexpr (FORM == SF_ALL) {
    return true;
  } else {
    return LikeMatch(pb, pk, plen, s, len);
  }
}

// The same with the form and operator read from the plan (host use).
inline bool StrMatchRow(const StrMatchPlan &p, const uint8_t *s, int64_t len) {
  switch (p.form) {
    case SF_COMPARE: return StrCompareOp(p.op, StrCompare(s, len, p.bytes, p.len));
    case SF_EXACT: return StrMatchRowT<SF_EXACT, SM_LIKE>(p.bytes, p.kind, p.len, s, len);
    case SF_PREFIX: return StrMatchRowT<SF_PREFIX, SM_LIKE>(p.bytes, p.kind, p.len, s, len);
    case SF_SUFFIX: return StrMatchRowT<SF_SUFFIX, SM_LIKE>(p.bytes, p.kind, p.len, s, len);
    case SF_CONTAINS: return StrMatchRowT<SF_CONTAINS, SM_LIKE>(p.bytes, p.kind, p.len, s, len);
    case SF_ALL: return true;
    default: return LikeMatch(p.bytes, p.kind, p.len, s, len);
  }
}

}  // namespace mbx
