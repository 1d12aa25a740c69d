"""Plain numpy references for the outer LOOKUP_JOIN modes and the null
predicates (include/presto_gpu.h: PG_JOIN_*, PG_CMP_IS_NULL).  No GPU, no
library: the tests compare the operators against these, and
test_outer_join_refs.py checks these against values typed out by hand."""
import numpy as np

INNER, PROBE_OUTER, LOOKUP_OUTER, FULL_OUTER = 0, 4, 5, 6


def is_null(mask, n):
    """Row-wise nullness of a column: its mask as bools, all False for a
    column without a mask."""
    if mask is None:
        return np.zeros(n, bool)
    mask = np.asarray(mask)
    assert len(mask) == n
    return mask != 0


def outer_join(build_keys, build_payloads, probe_cols, probe_key, key_nulls,
               pred_keep, mode):
    """One LOOKUP_JOIN emit join over a single probe page.

    build_keys / build_payloads: the build rows in build-row order.
    probe_cols: the emitted probe columns; probe_key: the probe keys;
    key_nulls: null mask of the probe key (or None); pred_keep: which probe
    rows pass the predicates (or None for all); mode: 0, 4, 5 or 6.

    Returns (probe_pages_rows, masks, drain_rows):
    probe_pages_rows: the output columns — probe columns, then payloads —
      rows in probe-row order and, within one probe row, in build-row
      order (the operator may order one probe row's matches differently);
      a payload under a null is 0;
    masks: uint8 per output row, 1 = the payloads are null (all 0 in the
      modes that never pad);
    drain_rows: payload columns of the build rows no kept probe row
      matched, in build-row order (None in modes 0 and 4).
    Mode 0 does not read key_nulls, like the operator."""
    assert mode in (INNER, PROBE_OUTER, LOOKUP_OUTER, FULL_OUTER)
    bk = np.asarray(build_keys, np.int64)
    pk = np.asarray(probe_key, np.int64)
    n, nb = len(pk), len(bk)
    keep = np.ones(n, bool) if pred_keep is None \
        else np.asarray(pred_keep).astype(bool)
    if mode != INNER:
        keep_key = ~is_null(key_nulls, n)
    else:
        keep_key = np.ones(n, bool)
    order = np.argsort(bk, kind="stable")
    sk = bk[order]
    lo = np.searchsorted(sk, pk, "left")
    hi = np.searchsorted(sk, pk, "right")
    cnt = np.where(keep & keep_key, hi - lo, 0)
    if mode in (PROBE_OUTER, FULL_OUTER):
        pad = keep & (cnt == 0)
    else:
        pad = np.zeros(n, bool)
    out_cnt = cnt + pad
    total = int(out_cnt.sum())
    src = np.repeat(np.arange(n), out_cnt)
    starts = np.cumsum(out_cnt) - out_cnt
    within = np.arange(total) - np.repeat(starts, out_cnt)
    is_pad = np.repeat(pad, out_cnt)
    if nb:
        at = np.minimum(np.repeat(lo, out_cnt) + within, nb - 1)
        brow = np.where(is_pad, 0, order[at])
    else:
        brow = np.zeros(total, np.int64)
    cols = [np.asarray(c)[src] for c in probe_cols]
    for p in build_payloads:
        p = np.asarray(p)
        vals = p[brow] if nb else np.zeros(total, p.dtype)
        cols.append(np.where(is_pad, np.zeros(1, p.dtype), vals))
    masks = is_pad.astype(np.uint8)
    drain = None
    if mode in (LOOKUP_OUTER, FULL_OUTER):
        matched = np.zeros(nb, bool)
        matched[brow[~is_pad]] = True
        drain = [np.asarray(p)[~matched] for p in build_payloads]
    return cols, masks, drain


def anti_join(build_keys, probe_key, key_nulls=None, pred_keep=None):
    """Indexes of the probe rows a LEFT join pads: kept by the predicates
    and without a match (a null key never matches) — the rows of
    `... LEFT JOIN b ... WHERE b.x IS NULL`."""
    pk = np.asarray(probe_key, np.int64)
    n = len(pk)
    keep = np.ones(n, bool) if pred_keep is None \
        else np.asarray(pred_keep).astype(bool)
    hit = np.isin(pk, np.asarray(build_keys, np.int64)) & \
        ~is_null(key_nulls, n)
    return np.flatnonzero(keep & ~hit)


def canonical(cols, masks=None):
    """The rows of `cols` (+ the mask as a last column) as one sorted list
    of tuples — the multiset the comparisons use, since the order of one
    probe row's matches is not pinned."""
    cols = [np.asarray(c) for c in cols]
    if masks is not None:
        cols = cols + [np.asarray(masks)]
    return sorted(zip(*(c.tolist() for c in cols)))
