"""The ORDER BY model of the sort tests: plain Python and numpy, no engine code.

order(rows, keys) returns the row indices (0..rows-1, or the given ones) in
sorted order.  Each key is
(values, valid, kind, desc, nulls_first):

  values       one Python value per row (whatever stands under a NULL is ignored)
  valid        one flag per row, or None for a column without NULLs
  kind         'int'  integers of any width and sign, DECIMAL (unscaled), DATE,
                      TIMESTAMP: by value
               'bool' false < true
               'f64' / 'f32'  vm_reference.cmp3: NaN is greatest, all NaNs are
                      equal, -0.0 equals +0.0
               'str'  the UTF-8 bytes, unsigned, so a prefix sorts first
  desc         descending
  nulls_first  True / False / None; None is the binder's default, NULLS LAST,
               for ASC and DESC alike

Keys compare left to right.  The caller passes a unique last key (the row id),
so the order is total and the model says nothing about true ties.

order() is a comparison sort over a three-way comparator (the definition);
order_np() gets the same order from np.lexsort over per-key rank arrays, for
the sizes where the comparator is too slow.  test_sort_model.py holds them
against each other and against hand-written expectations."""
import functools

import numpy as np

import vm_reference as R


def _b(s):
    return s if isinstance(s, bytes) else s.encode("utf-8")


def cmp_values(kind, a, b):
    """three-way comparison of two non-NULL values"""
    if kind in ("f64", "f32"):
        return R.cmp3(a, b)
    if kind == "str":
        a, b = _b(a), _b(b)
    elif kind == "bool":
        a, b = bool(a), bool(b)
    return int(a > b) - int(a < b)


def cmp_rows(keys, i, j):
    for values, valid, kind, desc, nulls_first in keys:
        ni, nj = valid is not None and not valid[i], valid is not None and not valid[j]
        if ni or nj:
            if ni and nj:
                continue
            return (-1 if ni else 1) * (1 if nulls_first else -1)  # direction does not move the NULLs
        c = cmp_values(kind, values[i], values[j])
        if c:
            return -c if desc else c
    return 0


def order(rows, keys):
    """rows: a row count, or the row indices to sort"""
    idx = range(rows) if isinstance(rows, int) else list(rows)
    return sorted(idx, key=functools.cmp_to_key(lambda i, j: cmp_rows(keys, i, j)))


def rank(values, valid, kind):
    """int64 ranks: rank[i] < rank[j] iff row i's value sorts before row j's (NULL rows: 0)"""
    n = len(values)
    ok = np.ones(n, dtype=bool) if valid is None else np.asarray(valid, dtype=bool)
    out = np.zeros(n, dtype=np.int64)
    if not ok.any():
        return out
    if kind in ("f64", "f32"):
        v = np.asarray(values, dtype=np.float64)[ok]
        nan = np.isnan(v)
        w = np.where(nan, np.inf, v + 0.0)  # -0.0 + 0.0 = +0.0
        _, inv = np.unique(w, return_inverse=True)
        out[ok] = inv.reshape(-1) + nan  # every NaN one step above +inf
        return out
    if isinstance(values, np.ndarray) and values.dtype.kind in "iub":
        v = values[ok]
    else:
        pick = [values[i] for i in np.flatnonzero(ok)]
        if kind == "str":
            pick = [_b(s) for s in pick]
        elif kind == "bool":
            pick = [bool(x) for x in pick]
        v = np.empty(len(pick), dtype=object)  # Python ints of any size, bytes
        v[:] = pick
    _, inv = np.unique(v, return_inverse=True)
    out[ok] = inv.reshape(-1)
    return out


def order_np(rows, keys):
    idx = np.arange(rows) if isinstance(rows, int) else np.asarray(list(rows), dtype=np.int64)
    cols = []  # np.lexsort: the last array is the primary key
    for values, valid, kind, desc, nulls_first in reversed(keys):
        r = rank(values, valid, kind)
        cols.append((-r if desc else r)[idx])
        if valid is not None:
            isnull = ~np.asarray(valid, dtype=bool)
            cols.append((np.where(isnull, -1, 0) if nulls_first else np.where(isnull, 1, 0))[idx])
    return [int(i) for i in idx[np.lexsort(cols)]] if cols else [int(i) for i in idx]


def key_of(col, desc=False, nulls_first=None):
    """the key of a vm_cases.Col"""
    kind = "str" if col.sqltype == "VARCHAR" else "int" if col.kind == "dec" else col.kind
    return col.values, None if all(col.valid) else col.valid, kind, desc, nulls_first
