"""Plan constructors: the one place that fills the ctypes plan structs of
engine.py (the mirrors of include/presto_gpu.h).

Pure ctypes — no GPU, no .so, importing loads nothing.  Every constructor
takes sequences (preds=, payload=, emit=, proj=, aggs=), derives the n_*
counts from them and rejects a sequence longer than the struct's array
with a ValueError naming the field.  Any other struct field is a plain
keyword argument passed through (a sequence for an array field); an
unknown name is a TypeError.
"""
import ctypes as C

import numbers

from .engine import (
    Pred, Proj, Agg, PlanFilterProject, PlanHashAggSmall, PlanHashBuild,
    PlanLookupJoin, PlanGroupBy, PlanTopN, PlanPartition, PlanOrderBy,
    PlanWindow, WinSpec, PlanMarkDistinct, DISTINCT_MARK, DISTINCT_ONLY,
    WIN_ROW_NUMBER, WIN_RANK, WIN_DENSE_RANK, WIN_COUNT, WIN_SUM, WIN_MIN,
    WIN_MAX, WIN_LAG, WIN_LEAD,
    FRAME_RANGE_RUNNING, FRAME_ROWS_RUNNING, FRAME_PARTITION,
    SORT_ASC_NULLS_FIRST, SORT_ASC_NULLS_LAST, SORT_DESC_NULLS_FIRST,
    SORT_DESC_NULLS_LAST,
    CMP_CONTAINS2, CMP_NOT_CONTAINS2, CMP_IS_NULL, CMP_IS_NOT_NULL,
    JOIN_PROBE_OUTER, JOIN_LOOKUP_OUTER, JOIN_FULL_OUTER,
    PROJ_IDENT, PROJ_DISC_PRICE, PROJ_CHARGE, PROJ_MUL, PROJ_DIV,
    PROJ_KEYSHL, PROJ_SUBDIV, PROJ_KEYSHL_DIV,
    AGG_COUNT, AGG_SUM_F64, AGG_SUM_DEC, AGG_SUM_I64, AGG_MIN, AGG_MAX,
)


# ---- predicates ----
def pred(col, op, val):
    """col <op> literal: an int compares as ival, a float as dval."""
    if isinstance(val, float):
        return Pred(col, op, 0, val)
    return Pred(col, op, int(val), 0.0)


def pred_cols(col, op, rhs, plus=0):
    """col <op> channel rhs (+ integer constant `plus`); rhs_col is stored
    biased by one so that 0 keeps meaning "literal compare"."""
    p = Pred(col, op, plus, 0.0)
    p.rhs_col = rhs + 1
    return p


def pred_varbin(col, op, needle, needle2=None):
    """VARBIN CONTAINS / PREFIX of `needle`; the ordered two-needle
    CONTAINS2 / NOT_CONTAINS2 stores both concatenated in sval, slen = the
    length of the FIRST and ival = the length of the second."""
    if (needle2 is not None) != (op in (CMP_CONTAINS2, CMP_NOT_CONTAINS2)):
        raise ValueError("needle2 goes with CONTAINS2 / NOT_CONTAINS2 only")
    sval = needle + (needle2 or b"")
    if len(sval) > Pred.sval.size:
        raise ValueError(f"sval: {len(sval)} bytes exceed {Pred.sval.size}")
    p = Pred(col, op, len(needle2 or b""), 0.0)
    # not `p.sval = sval`: the c_char array setter stops at the first NUL,
    # and a needle is bytes, not a C string
    C.memmove(C.addressof(p) + Pred.sval.offset, sval, len(sval))
    p.slen = len(needle)
    return p


def pred_is_null(col):
    """col IS NULL: reads the column's null mask only (any column type;
    a column without a mask is never null)."""
    return Pred(col, CMP_IS_NULL, 0, 0.0)


def pred_not_null(col):
    """col IS NOT NULL; as a per-aggregate filter it makes count()
    count(col)."""
    return Pred(col, CMP_IS_NOT_NULL, 0, 0.0)


# ---- projections ----
def ident(ch):
    return Proj(PROJ_IDENT, ch, 0, 0)


def disc_price(ep, dc):
    return Proj(PROJ_DISC_PRICE, ep, dc, 0)


def charge(ep, dc, tx):
    return Proj(PROJ_CHARGE, ep, dc, tx)


def mul(a, b):
    return Proj(PROJ_MUL, a, b, 0)


def div(a, b):
    return Proj(PROJ_DIV, a, b, 0)


def keyshl(a, b, shift):
    return Proj(PROJ_KEYSHL, a, b, shift)


def subdiv(a, b, c):
    return Proj(PROJ_SUBDIV, a, b, c)


def keyshl_div(a, b, shift, divisor):
    return Proj(PROJ_KEYSHL_DIV, a, b, (shift << 16) | divisor)


# ---- aggregates ----
def count():
    return Agg(AGG_COUNT, ident(0), 0)


def sum_dec(proj, scale):
    return Agg(AGG_SUM_DEC, proj, scale)


def sum_f64(proj, scale=0):
    return Agg(AGG_SUM_F64, proj, scale)


def sum_i64(proj):
    return Agg(AGG_SUM_I64, proj, 0)


def agg_min(proj, scale=0):
    """MIN over integer ticks (scale 0: the integer column itself)."""
    return Agg(AGG_MIN, proj, scale)


def agg_max(proj, scale=0):
    return Agg(AGG_MAX, proj, scale)


# ---- struct filling ----
def _fill(arr, field, seq):
    """Copy seq into the ctypes array of struct field `field`; returns
    the count for the field's n_* companion."""
    seq = list(seq)
    if len(seq) > len(arr):
        raise ValueError(f"{field}: {len(seq)} entries exceed the struct's "
                         f"{len(arr)}")
    for i, v in enumerate(seq):
        arr[i] = v
    return len(seq)


_ARRAY_FIELDS = {
    cls: {name: issubclass(tp, C.Array) for name, tp in cls._fields_}
    for cls in (PlanFilterProject, PlanHashAggSmall, PlanHashBuild,
                PlanLookupJoin)}


def _set(plan, fields):
    """The pass-through keyword arguments; the n_* counts are derived."""
    is_array = _ARRAY_FIELDS[type(plan)]
    for name, value in fields.items():
        if name not in is_array or name.startswith("n_"):
            raise TypeError(f"{type(plan).__name__} has no settable field "
                            f"{name!r}")
        if is_array[name]:
            _fill(getattr(plan, name), name, value)
        else:
            setattr(plan, name, value)
    return plan


def _aggs(plan, preds, filters, aggs):
    """preds + filters share preds[]: only preds[0..n_preds) filter rows,
    the rest are per-aggregate FILTER predicates.  An aggregate is an Agg
    (unfiltered) or (Agg, i) gated by filters[i]."""
    preds, filters = list(preds), list(filters)
    _fill(plan.preds, "preds", preds + filters)
    plan.n_preds = len(preds)
    pairs = [a if isinstance(a, tuple) else (a, None) for a in aggs]
    if any(f is not None and not 0 <= f < len(filters) for _, f in pairs):
        raise ValueError("agg_filter: index outside filters=")
    plan.n_aggs = _fill(plan.aggs, "aggs", [a for a, _ in pairs])
    _fill(plan.agg_filter, "agg_filter",
          [-1 if f is None else len(preds) + f for _, f in pairs])


def _join_keys(plan, key_col):
    """key_col of a build or a join: an int is the single bigint key
    (n_keys = 0, the path every plan took before multi-key joins); a
    sequence of 1..4 channels, most significant first, is a multi-key
    join key (n_keys = len, key_cols)."""
    if isinstance(key_col, numbers.Integral):
        plan.key_col = int(key_col)
        return
    keys = list(key_col)
    if not keys:
        raise ValueError("key_cols: a multi-key join needs at least one "
                         "key (pass an int for the single-key path)")
    plan.n_keys = _fill(plan.key_cols, "key_cols", keys)


# ---- one constructor per operator kind ----
def hash_build(key_col=0, *, preds=(), payload=(), semijoin_table=-1,
               **fields):
    """key_col: an int, or a sequence of 1..4 channels for a multi-key
    chained build (see _join_keys)."""
    p = PlanHashBuild()
    p.n_preds = _fill(p.preds, "preds", preds)
    _join_keys(p, key_col)
    p.n_payload = _fill(p.payload_col, "payload_col", payload)
    p.semijoin_table = semijoin_table
    return _set(p, fields)


def flag_set(key_col, capacity_hint, preds=()):
    """Dense key flag set: 1-byte membership flags over keys 1..hint."""
    return hash_build(key_col, preds=preds, capacity_hint=capacity_hint,
                      key_set_only=1, dense_array=1)


def range_group(capacity_hint):
    """Range-group table: the group domain is the key range 1..hint
    itself (no build input, no hash)."""
    return hash_build(capacity_hint=capacity_hint, range_group=1)


def lookup_join(table, key_col, mode, *, preds=(), filters=(), emit=(),
                aggs=(), group_vals=(), **fields):
    """mode 0 emits `emit` probe channels + the payloads (modes 4-6 are
    its outer variants: left_join / right_join / full_join); mode 1 is the
    fused grouped aggregate (single proj=/dec_scale=, or aggs= with
    optional filters= and acc_pack fields); modes 2/3 take table2= etc.
    key_col: an int, or a sequence of 1..4 channels to probe a multi-key
    table (emit modes only)."""
    p = PlanLookupJoin()
    p.table = table
    _join_keys(p, key_col)
    p.mode = mode
    _aggs(p, preds, filters, aggs)
    p.n_emit = _fill(p.emit_probe_cols, "emit_probe_cols", emit)
    p.n_group_vals = _fill(p.group_vals, "group_vals", group_vals)
    return _set(p, fields)


def emit_join(table, key_col, emit, preds=()):
    return lookup_join(table, key_col, 0, preds=preds, emit=emit)


def left_join(table, key_col, emit, preds=()):
    """LEFT: emit_join plus one null-padded row per unmatched probe row;
    the payload columns of the output carry a null mask."""
    return lookup_join(table, key_col, JOIN_PROBE_OUTER, preds=preds,
                       emit=emit)


def right_join(table, key_col, emit, preds=()):
    """RIGHT: emit_join plus, after finish(), one drain page of the build
    rows this operator never matched (chained tables only)."""
    return lookup_join(table, key_col, JOIN_LOOKUP_OUTER, preds=preds,
                       emit=emit)


def full_join(table, key_col, emit, preds=()):
    """FULL: left_join and right_join together."""
    return lookup_join(table, key_col, JOIN_FULL_OUTER, preds=preds,
                       emit=emit)


def agg_join(table, key_col, proj, dec_scale=0, preds=(), **fields):
    """Single fused grouped SUM of `proj` per matched key (mode 1)."""
    return lookup_join(table, key_col, 1, preds=preds, proj=proj,
                       dec_scale=dec_scale, **fields)


def small_agg(aggs, *, preds=(), keys=(), **fields):
    """keys: up to two (channel, listed key values) pairs."""
    p = PlanHashAggSmall()
    p.n_preds = _fill(p.preds, "preds", preds)
    p.n_aggs = _fill(p.aggs, "aggs", aggs)
    keys = list(keys)
    p.n_keys = _fill(p.key_col, "key_col", [c for c, _ in keys])
    for i, (_, vals) in enumerate(keys):
        p.n_vals[i] = _fill(p.key_vals[i], "key_vals", vals)
    return _set(p, fields)


def filter_project(proj, *, preds=(), **fields):
    p = PlanFilterProject()
    p.n_preds = _fill(p.preds, "preds", preds)
    p.n_proj = _fill(p.proj, "proj", proj)
    return _set(p, fields)


def group_by(keys, aggs, capacity_hint, *, preds=(), filters=(),
             sql_nulls=False):
    """sql_nulls=True: null group keys form groups of their own, SUM / MIN
    / MAX skip null inputs and emit null for a group without any, and the
    output carries null masks (pg_plan_groupby in the header).  count()
    stays count(*); count(x) is (count(), i) with filters[i] =
    pred_not_null(x)."""
    p = PlanGroupBy()
    p.n_keys = _fill(p.key_col, "key_col", keys)
    p.capacity_hint = capacity_hint
    _aggs(p, preds, filters, aggs)
    p.sql_nulls = int(sql_nulls)
    return p


def top_n(limit, val_col, date_col, key_col):
    return PlanTopN(limit, val_col, date_col, key_col)


def asc(col, nulls_last=True):
    """ORDER BY key: col ASC NULLS LAST (or FIRST)."""
    return (col, SORT_ASC_NULLS_LAST if nulls_last else SORT_ASC_NULLS_FIRST)


def desc(col, nulls_last=True):
    """ORDER BY key: col DESC NULLS LAST (or FIRST)."""
    return (col,
            SORT_DESC_NULLS_LAST if nulls_last else SORT_DESC_NULLS_FIRST)


def order_by(keys, emit, limit=0):
    """Stable multi-key sort: keys is a sequence of (col, order) pairs,
    most significant first (see asc / desc); emit lists the output
    channels; limit > 0 keeps the first `limit` rows."""
    keys = list(keys)
    p = PlanOrderBy()
    p.n_keys = _fill(p.key_col, "key_col", [c for c, _ in keys])
    _fill(p.order, "order", [o for _, o in keys])
    p.n_emit = _fill(p.emit_cols, "emit_cols", emit)
    if p.n_keys == 0:
        raise ValueError("key_col: ORDER BY needs at least one key")
    if p.n_emit == 0:
        raise ValueError("emit_cols: ORDER BY needs at least one column")
    p.limit = limit
    return p


# ---- window functions (pg_win_spec) ----
def row_number():
    return WinSpec(WIN_ROW_NUMBER, -1, 0, 0, 0)


def rank():
    return WinSpec(WIN_RANK, -1, 0, 0, 0)


def dense_rank():
    return WinSpec(WIN_DENSE_RANK, -1, 0, 0, 0)


def win_count(col=None, frame=FRAME_RANGE_RUNNING):
    """count(*) over the frame, or count(col): its non-null rows."""
    return WinSpec(WIN_COUNT, -1 if col is None else col, frame, 0, 0)


def win_sum(col, frame=FRAME_RANGE_RUNNING):
    return WinSpec(WIN_SUM, col, frame, 0, 0)


def win_min(col, frame=FRAME_RANGE_RUNNING):
    return WinSpec(WIN_MIN, col, frame, 0, 0)


def win_max(col, frame=FRAME_RANGE_RUNNING):
    return WinSpec(WIN_MAX, col, frame, 0, 0)


def lag(col, offset=1):
    """col of the row `offset` rows back in its partition, else null."""
    return WinSpec(WIN_LAG, col, 0, 0, offset)


def lead(col, offset=1):
    return WinSpec(WIN_LEAD, col, 0, 0, offset)


def window(partition_by, order_by, emit, funcs):
    """Window functions over PARTITION BY partition_by ORDER BY order_by:
    both are sequences of (col, order) pairs (see asc / desc), either may
    be empty; emit lists the input channels to pass through, funcs the
    WinSpec entries (row_number(), win_sum(...), lag(...) ...) whose
    columns follow them in the output."""
    partition_by, order_by = list(partition_by), list(order_by)
    keys = partition_by + order_by
    p = PlanWindow()
    p.n_keys = _fill(p.key_col, "key_col", [c for c, _ in keys])
    _fill(p.order, "order", [o for _, o in keys])
    p.n_partition_keys = len(partition_by)
    p.n_emit = _fill(p.emit_cols, "emit_cols", emit)
    p.n_funcs = _fill(p.funcs, "funcs", funcs)
    if p.n_emit == 0:
        raise ValueError("emit_cols: WINDOW needs at least one column")
    if p.n_funcs == 0:
        raise ValueError("funcs: WINDOW needs at least one function")
    return p


def _mark_distinct(mode, keys, emit, capacity, limit):
    p = PlanMarkDistinct()
    p.n_keys = _fill(p.key_col, "key_col", keys)
    p.n_emit = _fill(p.emit_cols, "emit_cols", emit)
    if p.n_keys == 0:
        raise ValueError("key_col: MARK_DISTINCT needs at least one key")
    if p.n_emit == 0:
        raise ValueError("emit_cols: MARK_DISTINCT needs at least one "
                         "column")
    p.mode = mode
    p.capacity_hint = capacity
    p.limit = limit
    return p


def mark_distinct(keys, emit, capacity):
    """First-occurrence marker over the key channels: every input page
    comes back as its `emit` channels plus a trailing U8 column, 1 on the
    first row ever seen with its key combination (null is a value).
    capacity is the expected number of distinct combinations.
    count(DISTINCT x) GROUP BY g is mark_distinct([g, x], ...) feeding
    group_by([g], [(count(), 0)], filters=[pred(marker, CMP_EQ, 1)])."""
    return _mark_distinct(DISTINCT_MARK, keys, emit, capacity, 0)


def distinct(keys, emit, capacity, limit=0):
    """SELECT DISTINCT: only the first row of every key combination, in
    input order, as the `emit` channels; limit > 0 stops after that many
    rows (DistinctLimit), after which the operator takes no more input."""
    return _mark_distinct(DISTINCT_ONLY, keys, emit, capacity, limit)


def partition(n_partitions, key_col, emit):
    p = PlanPartition()
    p.n_partitions = n_partitions
    p.key_col = key_col
    p.n_emit = _fill(p.emit_cols, "emit_cols", emit)
    return p
