"""Plain reference for PG_OP_ORDER_BY: a stable comparator sort over row
indices.  Shares no code with the product — no key transform, no radix
passes; it restates the contract of include/presto_gpu.h directly:

  - U8 compares unsigned, I32/I64 signed, F64 as Double.compare
    (-inf < ... < -0.0 < +0.0 < ... < +inf < NaN, all NaNs equal);
  - a null key goes first or last as the order says, whatever ASC/DESC
    says; nulls are equal to each other and the value under a null is
    never looked at;
  - equal rows keep their input order (Python's sorted is stable);
  - limit > 0 keeps the first min(limit, n) rows;
  - emit columns and masks are gathered by the sorted row indices.
"""
import functools
import struct

import numpy as np

ASC_NULLS_FIRST, ASC_NULLS_LAST, DESC_NULLS_FIRST, DESC_NULLS_LAST = range(4)
ORDERS = (ASC_NULLS_FIRST, ASC_NULLS_LAST, DESC_NULLS_FIRST, DESC_NULLS_LAST)


def _sign(a, b):
    return (a > b) - (a < b)


def f64_bits(x):
    """The IEEE-754 bit pattern of a Python float as an unsigned int."""
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def f64_from_bits(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def double_compare_bits(a, b):
    """Double.compare on two bit patterns (unsigned ints): numeric order
    where < or > decides; otherwise -0.0 < +0.0 and NaN above everything,
    every NaN equal to every other (doubleToLongBits collapses NaNs)."""
    exp_mask, frac_mask = 0x7ff0000000000000, 0x000fffffffffffff

    def is_nan(u):
        return (u & exp_mask) == exp_mask and (u & frac_mask) != 0

    na, nb = is_nan(a), is_nan(b)
    if na or nb:
        return int(na) - int(nb)
    x, y = f64_from_bits(a), f64_from_bits(b)
    if x < y:
        return -1
    if x > y:
        return 1
    # equal numerically: only the zeros can still differ, by sign
    return _sign(b >> 63, a >> 63)


def compare_values(dtype, a, b):
    """Ascending compare of two non-null values of a key column."""
    dtype = np.dtype(dtype)
    if dtype == np.float64:
        return double_compare_bits(int(a), int(b))  # bit patterns
    return _sign(int(a), int(b))  # uint8 / int32 / int64 as Python ints


def _key_view(col):
    """Python values to compare: ints, or bit patterns for F64."""
    col = np.asarray(col)
    if col.dtype == np.float64:
        return [int(v) for v in col.view(np.uint64)]
    return [int(v) for v in col]


def sort_indices(keys, limit=0):
    """keys: [(values array, order, mask or None)], most significant
    first.  Returns the sorted row indices (a Python list), truncated to
    `limit` when it is > 0."""
    n = len(keys[0][0])
    views = [(_key_view(v), np.asarray(v).dtype, order,
              None if m is None else [int(x) for x in m])
             for v, order, m in keys]

    def cmp(i, j):
        for vals, dtype, order, mask in views:
            ni = bool(mask[i]) if mask is not None else False
            nj = bool(mask[j]) if mask is not None else False
            if ni or nj:
                if ni and nj:
                    continue
                nulls_last = order in (ASC_NULLS_LAST, DESC_NULLS_LAST)
                first = -1 if ni else 1       # as if NULLS FIRST
                return -first if nulls_last else first
            c = compare_values(dtype, vals[i], vals[j])
            if c:
                return -c if order in (DESC_NULLS_FIRST,
                                       DESC_NULLS_LAST) else c
        return 0

    idx = sorted(range(n), key=functools.cmp_to_key(cmp))
    if limit > 0:
        idx = idx[:limit]
    return idx


def order_by(cols, masks, keys, emit, limit=0):
    """cols: list of numpy columns (an I128 column is an (n, 2) uint64
    array); masks: {column index: uint8 mask}; keys: [(column index,
    order)]; emit: column indices.  Returns (emitted columns, {emit
    position: gathered mask})."""
    idx = sort_indices([(cols[c], o, masks.get(c)) for c, o in keys], limit)
    take = np.asarray(idx, np.int64)
    out = [np.asarray(cols[c])[take] for c in emit]
    out_masks = {o: np.asarray(masks[c], np.uint8)[take]
                 for o, c in enumerate(emit) if c in masks}
    return out, out_masks


def concat_pages(pages):
    """pages: [(cols, masks)] -> one (cols, masks); a page without a mask
    for a column that has one elsewhere contributes zeros."""
    n_cols = len(pages[0][0])
    cols = [np.concatenate([np.asarray(p[0][c]) for p in pages])
            for c in range(n_cols)]
    masked = sorted({c for _, m in pages for c in m})
    masks = {c: np.concatenate(
        [np.asarray(m[c], np.uint8) if c in m
         else np.zeros(len(p[0]), np.uint8) for p, m in pages])
        for c in masked}
    return cols, masks
