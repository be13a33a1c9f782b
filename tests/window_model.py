"""The reference model of the window functions: plain Python, no engine code.

window(n, partition, order, calls) returns one list per call with the value of
every source row, in source order.

  partition  keys as (values, valid, kind): sort_model's key without a direction
  order      sort_model keys (values, valid, kind, desc, nulls_first)
  calls      Call(func, arg, kind, frame, offset, scale)

The rows are sorted stably by (partition keys, order keys) with sort_model's
ranking (NULL placement, direction, floats: every NaN one value, -0.0 = +0.0),
so ties keep source order.  Two rows are in one partition, or are peers, when
every key has the same NULL flag and the same rank; a NULL partition key is a
partition of its own.  Then the partitions are walked.

func   row_number, rank, dense_rank, count_star, count, sum, min, max, avg, lag, lead
arg    one value per source row, None for NULL (not for the ranks and count_star)
kind   "int": exact integers (DECIMAL unscaled); "f64": doubles
frame  "rows"  the running value row by row
       "range" up to the current row's last peer (the default with ORDER BY)
       "part"  the whole partition (the default without ORDER BY)
Results: ints for the ranks and counts; for kind "int" SUM / MIN / MAX exact
ints and AVG a Ratio (sum over count * 10^scale, exact); for "f64" SUM as (correctly
rounded sum, sum of |x|) so that a caller can scale a tolerance, AVG likewise
(avg, sum of |x| / count), MIN / MAX as agg_model's set of acceptable bit
patterns.  None is NULL."""
from fractions import Fraction

import numpy as np

import agg_model as A
import sort_model as M
import vm_reference as R


class Ratio:
    """an exact quotient of two ints (AVG of integers), kept unreduced: float() is its correctly rounded double"""
    __slots__ = ("num", "den")

    def __init__(self, num, den):
        self.num, self.den = num, den

    def __float__(self):
        return self.num / self.den  # int / int is correctly rounded

    def fraction(self):
        return Fraction(self.num, self.den)

    def __eq__(self, other):
        return self.fraction() == (other.fraction() if isinstance(other, Ratio) else other)

    def __repr__(self):
        return f"Ratio({self.num}, {self.den})"


class Call:
    def __init__(self, func, arg=None, kind="int", frame="rows", offset=1, scale=0):
        self.func, self.arg, self.kind, self.frame, self.offset, self.scale = func, arg, kind, frame, offset, scale


def _same(keys, n):
    """same[i]: a tuple equal exactly where row i's keys are equal (NULL flag and rank of every key)"""
    cols = []
    for values, valid, kind in keys:
        r = M.rank(values, valid, kind)
        ok = np.ones(n, dtype=bool) if valid is None else np.asarray(valid, dtype=bool)
        cols.append(np.where(ok, r, -1).tolist())  # ranks are >= 0: -1 is NULL
    return list(zip(*cols)) if cols else [()] * n


def _running(call, rows):
    """the running state after each row of one partition (sorted order)"""
    out = []
    vals = [call.arg[r] for r in rows] if call.arg is not None else None
    if call.func == "count":
        c = 0
        for v in vals:
            c += v is not None
            out.append(c)
        return out
    if call.func in ("sum", "avg") and call.kind == "int":
        c, s = 0, 0
        for v in vals:
            if v is not None:
                c, s = c + 1, s + v
            out.append(None if not c else s if call.func == "sum" else Ratio(s, c * 10 ** call.scale))
        return out
    if call.func in ("sum", "avg"):
        c, s, a = 0, Fraction(0), Fraction(0)
        special = []
        for v in vals:
            if v is not None:
                c += 1
                if call.kind == "f64" and (v != v or v in (float("inf"), float("-inf"))):
                    special.append(v)
                else:
                    s += Fraction(v)
                    a += abs(Fraction(v))
            if not c:
                out.append(None)
            else:
                tot = A.fsum_special(special + [float(s)]) if special else float(s)
                out.append((tot, float(a)) if call.func == "sum" else (tot / c, float(a) / c))
        return out
    assert call.func in ("min", "max"), call.func
    sign = -1 if call.func == "min" else 1
    best, ties = None, None
    for v in vals:
        if v is not None:
            if call.kind == "int":
                best = v if best is None else (min(best, v) if sign < 0 else max(best, v))
            else:
                c = 1 if best is None else sign * R.cmp3(v, best)
                if c > 0:
                    best, ties = v, {A.NAN} if v != v else {R.bits(v)}
                elif c == 0 and v == v:
                    ties = ties | {R.bits(v)}
        out.append(None if best is None else best if call.kind == "int" else set(ties))
    return out


def window(n, partition, order, calls):
    keys = [(v, ok, kind, False, None) for v, ok, kind in partition] + list(order)
    perm = M.order_np(n, keys) if keys else list(range(n))
    psame = _same(partition, n)
    osame = _same([(v, ok, kind) for v, ok, kind, _, _ in order], n)
    results = [[None] * n for _ in calls]
    at = 0
    while at < n:
        end = at + 1
        while end < n and psame[perm[end]] == psame[perm[at]]:
            end += 1
        rows = perm[at:end]
        m = len(rows)
        # peer groups: first / last position of every row's group, and the dense rank
        first, last, dense = [0] * m, [0] * m, [0] * m
        g0, d = 0, 0
        for p in range(m + 1):
            if p == m or (p > 0 and osame[rows[p]] != osame[rows[p - 1]]):
                d += 1
                for x in range(g0, p):
                    first[x], last[x], dense[x] = g0, p - 1, d
                g0 = p
        running = {}  # one partition's running states, shared by the frames that read them
        for ci, call in enumerate(calls):
            res = results[ci]
            tgt = range(m) if call.frame == "rows" else last if call.frame == "range" else [m - 1] * m
            if call.func == "row_number":
                for p, r in enumerate(rows):
                    res[r] = p + 1
            elif call.func == "rank":
                for p, r in enumerate(rows):
                    res[r] = first[p] + 1
            elif call.func == "dense_rank":
                for p, r in enumerate(rows):
                    res[r] = dense[p]
            elif call.func == "count_star":
                for p, r in enumerate(rows):
                    res[r] = tgt[p] + 1
            elif call.func in ("lag", "lead"):
                for p, r in enumerate(rows):
                    j = p - call.offset if call.func == "lag" else p + call.offset
                    res[r] = call.arg[rows[j]] if 0 <= j < m else None
            else:
                key = (call.func, id(call.arg), call.kind, call.scale)
                if key not in running:
                    running[key] = _running(call, rows)
                st = running[key]
                for p, r in enumerate(rows):
                    res[r] = st[tgt[p]]
        at = end
    return results
