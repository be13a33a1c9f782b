// Host check of duckdb.mbt_amd/csrc/str_match.h (tests/test_str_match_host.py
// builds this with the host compiler under ASan + UBSan and runs it).
//
// LikeMatch and the plan's forms against a recursive definition of LIKE written
// here: every pattern of length <= 5 over {a, b, %, _, \} with '\' as the
// escape against every string of length <= 6 over {a, b}, then a hand list
// (UTF-8, bytes >= 0x80, the backtracking case, the length cap).
#include <stdint.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>

#include <string>
#include <vector>

#include "str_match.h"

using namespace mbx;

static int g_fail = 0;
#define CHECK(c, ...)                          \
  do {                                         \
    if (!(c)) {                                \
      printf("FAIL %s:%d: ", __FILE__, __LINE__); \
      printf(__VA_ARGS__);                     \
      printf("\n");                            \
      if (++g_fail > 20) exit(1);              \
    }                                          \
  } while (0)

typedef std::string S;
static const uint8_t *U(const S &s) { return (const uint8_t *)s.data(); }

// the definition: '%' any run of bytes, '_' one byte and the continuation bytes
// after it, the escape makes the next byte literal
static bool RefLike(const uint8_t *p, size_t pn, const uint8_t *s, size_t sn, bool he, uint8_t esc) {
  if (pn == 0) return sn == 0;
  if (he && p[0] == esc) return sn > 0 && s[0] == p[1] && RefLike(p + 2, pn - 2, s + 1, sn - 1, he, esc);
  if (p[0] == '%') {
    for (size_t k = 0; k <= sn; k++)
      if (RefLike(p + 1, pn - 1, s + k, sn - k, he, esc)) return true;
    return false;
  }
  if (sn == 0) return false;
  if (p[0] == '_') {
    size_t k = 1;
    while (k < sn && (s[k] & 0xC0) == 0x80) k++;
    return RefLike(p + 1, pn - 1, s + k, sn - k, he, esc);
  }
  return s[0] == p[0] && RefLike(p + 1, pn - 1, s + 1, sn - 1, he, esc);
}
static bool RefRaises(const S &p, bool he, uint8_t esc) {
  for (size_t i = 0; i < p.size(); i++)
    if (he && (uint8_t)p[i] == esc) {
      if (i + 1 >= p.size()) return true;
      i++;
    }
  return false;
}

// plan (chosen form and forced GENERAL) == definition; returns the chosen form
static int CheckOne(const S &pat, const S &str, bool he, uint8_t esc) {
  StrMatchPlan pl, pg;
  StrPlanStatus a = PlanLike(U(pat), (int64_t)pat.size(), he, esc, &pl);
  StrPlanStatus b = PlanLike(U(pat), (int64_t)pat.size(), he, esc, &pg, true);
  const bool raises = RefRaises(pat, he, esc);
  CHECK((a == SP_TRAILING_ESCAPE) == raises && (b == SP_TRAILING_ESCAPE) == raises, "raise '%s'", pat.c_str());
  if (raises || a != SP_OK || b != SP_OK) return -1;
  const bool want = RefLike(U(pat), pat.size(), U(str), str.size(), he, esc);
  const bool got_form = StrMatchRow(pl, U(str), (int64_t)str.size());
  const bool got_gen = StrMatchRow(pg, U(str), (int64_t)str.size());
  const bool got_like = LikeMatch(pg.bytes, pg.kind, pg.len, U(str), (int64_t)str.size());
  CHECK(pg.form == SF_GENERAL, "forced general '%s'", pat.c_str());
  CHECK(got_gen == want && got_like == want, "GENERAL '%s' on '%s': got %d want %d", pat.c_str(), str.c_str(), got_gen, want);
  CHECK(got_form == want, "form %d '%s' on '%s': got %d want %d", pl.form, pat.c_str(), str.c_str(), got_form, want);
  return pl.form;
}

static void Enumerate(const char *alpha, int maxlen, std::vector<S> &out) {
  const int na = (int)strlen(alpha);
  out.push_back("");
  size_t from = 0;
  for (int l = 1; l <= maxlen; l++) {
    const size_t to = out.size();
    for (size_t i = from; i < to; i++)
      for (int a = 0; a < na; a++) out.push_back(out[i] + alpha[a]);
    from = to;
  }
}

static int FormOf(const S &pat, bool he = true) {
  StrMatchPlan p;
  if (PlanLike(U(pat), (int64_t)pat.size(), he, '\\', &p) != SP_OK) return -1;
  return p.form;
}

static bool Like(const S &pat, const S &s, bool he = false, uint8_t esc = 0) {
  const int f = CheckOne(pat, s, he, esc);
  CHECK(f >= 0, "plan '%s'", pat.c_str());
  StrMatchPlan p;
  PlanLike(U(pat), (int64_t)pat.size(), he, esc, &p);
  return StrMatchRow(p, U(s), (int64_t)s.size());
}

static int Cmp(const S &a, const S &b) { return StrCompare(U(a), (int64_t)a.size(), U(b), (int64_t)b.size()); }

int main() {
  std::vector<S> pats, strs;
  Enumerate("ab%_\\", 5, pats);
  Enumerate("ab", 6, strs);
  CHECK(pats.size() == 3906 && strs.size() == 127, "enumeration sizes");
  long forms[SF_FORMS] = {0}, raised = 0;
  for (const S &p : pats) {
    int f = -1;
    for (const S &s : strs) f = CheckOne(p, s, true, '\\');
    if (f < 0) raised++;
    else forms[f]++;
  }
  CHECK(raised > 0, "no pattern raised");
  for (int f = SF_EXACT; f <= SF_GENERAL; f++) CHECK(forms[f] > 0, "form %d never chosen", f);
  // without an escape, '\' is an ordinary byte and nothing raises
  for (const S &p : pats)
    if (p.size() <= 3)
      for (const S &s : strs) CHECK(CheckOne(p, s, false, 0) >= 0, "no-escape plan '%s'", p.c_str());

  // the classification itself
  CHECK(FormOf("abc") == SF_EXACT && FormOf("") == SF_EXACT && FormOf("a\\%") == SF_EXACT, "EXACT");
  CHECK(FormOf("ab%") == SF_PREFIX && FormOf("ab%%") == SF_PREFIX && FormOf("\\_%") == SF_PREFIX, "PREFIX");
  CHECK(FormOf("%bc") == SF_SUFFIX && FormOf("%%b") == SF_SUFFIX, "SUFFIX");
  CHECK(FormOf("%b%") == SF_CONTAINS && FormOf("%\\%%") == SF_CONTAINS, "CONTAINS");
  CHECK(FormOf("%") == SF_ALL && FormOf("%%") == SF_ALL && FormOf("%%%") == SF_ALL, "ALL");
  CHECK(FormOf("_") == SF_GENERAL && FormOf("a%b") == SF_GENERAL && FormOf("a_c") == SF_GENERAL &&
            FormOf("%a%b%") == SF_GENERAL && FormOf("a%_") == SF_GENERAL,
        "GENERAL");
  CHECK(FormOf("ab\\") == -1 && FormOf("\\") == -1 && FormOf("ab\\", false) == SF_EXACT, "trailing escape");

  // hand list
  CHECK(Like("", "") && !Like("", "a") && Like("%", "") && Like("%%", "") && Like("%%", "abc"), "empty and doubled wildcard");
  CHECK(!Like("_", "") && Like("_", "a") && !Like("_", "ab"), "_ ascii");
  const S e2 = "\xC3\xA9", e3 = "\xE2\x82\xAC", e4 = "\xF0\x9F\x98\x80";  // 2-, 3- and 4-byte characters
  CHECK(Like("_", e2) && Like("_", e3) && Like("_", e4), "_ one code point");
  CHECK(!Like("__", e2) && !Like("__", e4) && Like("__", e2 + e3) && Like("a_c", "a" + e4 + "c"), "_ code points");
  CHECK(Like("_%", e3 + "x") && Like("%_", "x" + e3) && Like("_b", e2 + "b") && !Like("_b", e2 + e2), "_ with a wildcard");
  CHECK(Like("_", "\x80") && Like("_", "\x80\x80") && Like("a_", "a\x80") && Like("__", "a\x80" "b"),
        "lone continuation byte");
  CHECK(Like("%\\%%", "50%", true, '\\') && !Like("%\\%%", "50", true, '\\') && Like("a\\_c", "a_c", true, '\\') &&
            !Like("a\\_c", "abc", true, '\\') && Like("a#%", "a%", true, '#') && Like("##", "#", true, '#'),
        "escape");
  CHECK(Like("\xFF%", "\xFF\x01") && !Like("\xFF", "\x7F"), "high bytes in LIKE");
  CHECK(Cmp("a", "b") == -1 && Cmp("b", "a") == 1 && Cmp("ab", "ab") == 0 && Cmp("", "") == 0, "StrCompare basics");
  CHECK(Cmp("a", "ab") == -1 && Cmp("ab", "a") == 1 && Cmp("", "a") == -1, "StrCompare prefix");
  CHECK(Cmp("\x7F", "\x80") == -1 && Cmp("\xFF", "a") == 1 && Cmp("a\xC3\xA9", "az") == 1, "StrCompare is unsigned");
  for (int op = SM_EQ; op <= SM_NOT_DISTINCT; op++) {
    StrMatchPlan p;
    CHECK(PlanStrCompare((uint8_t)op, U(S("m")), 1, &p) == SP_OK, "compare plan");
    const bool lt = StrMatchRow(p, U(S("a")), 1), eq = StrMatchRow(p, U(S("m")), 1), gt = StrMatchRow(p, U(S("z")), 1);
    const bool wl = op == SM_NE || op == SM_LT || op == SM_LE || op == SM_DISTINCT;
    const bool we = op == SM_EQ || op == SM_LE || op == SM_GE || op == SM_NOT_DISTINCT;
    const bool wg = op == SM_NE || op == SM_GT || op == SM_GE || op == SM_DISTINCT;
    CHECK(lt == wl && eq == we && gt == wg, "compare op %d", op);
  }
  CHECK(StrFlipOp(SM_LT) == SM_GT && StrFlipOp(SM_GE) == SM_LE && StrFlipOp(SM_EQ) == SM_EQ, "flip");
  // backtracking: quadratic at worst, so 200 a's finish at once
  CHECK(!Like("a%a%a%b", S(200, 'a')) && Like("a%a%a%b", S(200, 'a') + "b") && Like("%a%a%a%a%a%a%a%a%", S(200, 'a')),
        "backtracking");
  // the length cap: 255 pattern bytes plan, 256 do not; collapsed '%'s and
  // escapes do not count
  {
    StrMatchPlan p;
    const S cap(kStrMatchCap, 'x'), over(kStrMatchCap + 1, 'x');
    CHECK(PlanLike(U(cap), (int64_t)cap.size(), false, 0, &p) == SP_OK && p.form == SF_EXACT && p.len == kStrMatchCap,
          "cap");
    CHECK(StrMatchRow(p, U(cap), (int64_t)cap.size()) && !StrMatchRow(p, U(over), (int64_t)over.size()), "cap match");
    CHECK(PlanLike(U(over), (int64_t)over.size(), false, 0, &p) == SP_TOO_LONG, "over the cap");
    const S gen = S(kStrMatchCap - 2, 'x') + "_%" + S(40, '%');
    CHECK(PlanLike(U(gen), (int64_t)gen.size(), false, 0, &p) == SP_OK && p.form == SF_GENERAL && p.len == kStrMatchCap,
          "cap, general");
    CHECK(StrMatchRow(p, U(cap), (int64_t)cap.size()) && !StrMatchRow(p, U(cap), kStrMatchCap - 2), "cap, general match");
    CHECK(PlanStrCompare(SM_EQ, U(cap), kStrMatchCap, &p) == SP_OK && PlanStrCompare(SM_EQ, U(over), 256, &p) == SP_TOO_LONG,
          "compare cap");
  }
  if (g_fail) {
    printf("str match: %d failures\n", g_fail);
    return 1;
  }
  printf("str match: ok (%zu patterns x %zu strings, %ld raised)\n", pats.size(), strs.size(), raised);
  return 0;
}
