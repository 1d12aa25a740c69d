"""Plain reference of GROUPBY_MULTI with SQL null semantics
(pg_plan_groupby.sql_nulls = 1) and, with sql_nulls=False, of the legacy
behaviour in which keys and aggregate inputs read the stored values.

Integer aggregates are computed in Python ints, SUM_F64 with math.fsum (the
correctly rounded exact sum) over products formed in float64 one operation
at a time, as the kernel forms them.  No GPU, no library."""
import math

import numpy as np

INT64_MAX = (1 << 63) - 1
INT64_MIN = -(1 << 63)

# aggregate functions
COUNT, SUM_I64, SUM_DEC, SUM_F64, MIN, MAX = (
    "count", "sum_i64", "sum_dec", "sum_f64", "min", "max")
# projections: (kind, a[, b]) over value-column indexes
IDENT, MUL, DISC_PRICE = "ident", "mul", "disc_price"
# per-aggregate FILTER: None, (NOT_NULL, col), (IS_NULL, col) or
# (GT, col, literal) — a comparison with a null operand rejects the row
NOT_NULL, IS_NULL, GT = "not_null", "is_null", "gt"

_READS = {IDENT: 1, MUL: 2, DISC_PRICE: 2}


def _isnull(masks, col, n):
    m = None if masks is None else masks[col]
    return np.zeros(n, bool) if m is None else np.asarray(m) != 0


def _filter_pass(flt, cols, masks, n):
    if flt is None:
        return np.ones(n, bool)
    null = _isnull(masks, flt[1], n)
    if flt[0] == NOT_NULL:
        return ~null
    if flt[0] == IS_NULL:
        return null
    assert flt[0] == GT
    return ~null & (np.asarray(cols[flt[1]]) > flt[2])


def _proj_null(proj, masks, n):
    null = np.zeros(n, bool)
    for c in proj[1:1 + _READS[proj[0]]]:
        null |= _isnull(masks, c, n)
    return null


def _proj_values(func, proj, cols, rows):
    """The projection's values at `rows` as a Python list."""
    a = np.asarray(cols[proj[1]])[rows]
    if proj[0] == IDENT:
        return a.tolist()
    b = np.asarray(cols[proj[2]])[rows]
    if func == SUM_F64:
        assert a.dtype == np.float64 and b.dtype == np.float64
        if proj[0] == MUL:
            return (a * b).tolist()
        return (a * (1.0 - b)).tolist()        # two roundings, no fma
    assert proj[0] == MUL                       # raw integer product
    return [x * y for x, y in zip(a.tolist(), b.tolist())]


def _group_rows(keys, key_masks, n, sql_nulls):
    """{key tuple: ascending row indexes}; None stands for a null key."""
    planes, nulls = [], []
    for ch, k in enumerate(keys):
        m = key_masks[ch] if (sql_nulls and key_masks is not None) else None
        null = np.zeros(n, bool) if m is None else np.asarray(m) != 0
        planes.append(np.where(null, 0, np.asarray(k).astype(np.int64)))
        nulls.append(null)
    mat = np.stack(planes + [x.astype(np.int64) for x in nulls], axis=1)
    order = np.lexsort(mat.T[::-1])             # stable: rows stay ascending
    srt = mat[order]
    first = np.ones(n, bool)
    first[1:] = (srt[1:] != srt[:-1]).any(axis=1)
    bounds = np.append(np.flatnonzero(first), n)
    nk = len(keys)
    out = {}
    for g, row in enumerate(srt[first].tolist()):
        key = tuple(None if row[nk + ch] else row[ch] for ch in range(nk))
        out[key] = order[bounds[g]:bounds[g + 1]]
    return out


def _inputs(spec, cols, masks, n, sql_nulls):
    """(rows passing the FILTER, of those the rows with a non-null input)"""
    func, proj, flt = spec
    passing = _filter_pass(flt, cols, masks, n)
    if func == COUNT or not sql_nulls:
        return passing, passing
    return passing, passing & ~_proj_null(proj, masks, n)


def group_by(keys, key_masks, specs, cols, masks, sql_nulls=True):
    """keys: one integer array per key channel; key_masks: their uint8
    null masks (entries or the whole list may be None); specs: (func, proj,
    filter) per aggregate; cols / masks: the value columns and their masks.

    Returns {key tuple, None for null: ([aggregate value or None], rows)}.
    With sql_nulls=False key masks and the nullness of aggregate inputs are
    ignored (FILTER predicates still read the masks) and an aggregate
    without input reports its identity: 0, INT64_MAX for MIN, INT64_MIN for
    MAX."""
    n = len(keys[0])
    fed = [_inputs(s, cols, masks, n, sql_nulls) for s in specs]
    out = {}
    for key, rows in _group_rows(keys, key_masks, n, sql_nulls).items():
        vals = []
        for (func, proj, _), (passing, nonnull) in zip(specs, fed):
            if func == COUNT:
                vals.append(int(passing[rows].sum()))
                continue
            use = rows[nonnull[rows]]
            if len(use) == 0:
                if sql_nulls:
                    vals.append(None)
                else:
                    vals.append({MIN: INT64_MAX, MAX: INT64_MIN,
                                 SUM_F64: 0.0}.get(func, 0))
                continue
            x = _proj_values(func, proj, cols, use)
            if func == SUM_F64:
                vals.append(math.fsum(x))
            elif func == MIN:
                vals.append(min(x))
            elif func == MAX:
                vals.append(max(x))
            else:
                vals.append(sum(x))
        out[key] = (vals, len(rows))
    return out


def input_counts(keys, key_masks, specs, cols, masks):
    """{key tuple: [(null inputs, non-null inputs) per aggregate]} among
    the rows passing each aggregate's FILTER, under SQL semantics — what a
    test uses to show that its data holds all-null and mixed groups."""
    n = len(keys[0])
    fed = [_inputs(s, cols, masks, n, True) for s in specs]
    out = {}
    for key, rows in _group_rows(keys, key_masks, n, True).items():
        out[key] = [(int((p[rows] & ~nn[rows]).sum()), int(nn[rows].sum()))
                    for p, nn in fed]
    return out
