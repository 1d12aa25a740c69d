"""Plain reference for PG_OP_WINDOW.  It sorts with the comparator sort of
order_by_refs.py, then walks the sorted rows one at a time, partition by
partition, and computes every function the obvious way with Python ints
(so a SUM outside int64 is detected exactly).  Shares no code with the
product; it restates the contract of include/presto_gpu.h:

  - rows are stably sorted by the partition keys, then the order keys;
    with no keys the input order is kept and everything is one partition;
  - adjacent sorted rows are in one partition when they compare equal on
    the partition keys under the sort's comparator, peers when equal on
    all keys: null == null, NaN == NaN, -0.0 != +0.0;
  - ROW_NUMBER / RANK / DENSE_RANK / COUNT give int64 without a mask;
  - SUM (int64), MIN / MAX (the column's type) skip nulls, are null (value
    0) over a frame without a non-null row, and always carry a mask;
  - the frames: RANGE_RUNNING ends at the row's last peer, ROWS_RUNNING at
    the row, PARTITION at the partition's last row;
  - an emitted SUM outside int64 raises SumOverflow(function index);
  - LAG / LEAD copy the value and null flag of the row `offset` rows back /
    ahead inside the partition, else null with value 0; always a mask.
"""
import numpy as np

import order_by_refs as R

(ROW_NUMBER, RANK, DENSE_RANK, COUNT, SUM, MIN, MAX, LAG, LEAD) = range(9)
RANGE_RUNNING, ROWS_RUNNING, PARTITION = range(3)


class SumOverflow(Exception):
    def __init__(self, func_index):
        super().__init__(f"SUM of function {func_index} does not fit int64")
        self.func_index = func_index


def _bits(col):
    """Values to compare or copy: F64 as bit patterns, the rest as is."""
    col = np.asarray(col)
    return col.view(np.uint64) if col.dtype == np.float64 else col


def _equal_on(cols, masks, keys, i, j):
    for c, _ in keys:
        m = masks.get(c)
        ni = bool(m[i]) if m is not None else False
        nj = bool(m[j]) if m is not None else False
        if ni or nj:
            if ni != nj:
                return False
            continue
        col = np.asarray(cols[c])
        b = _bits(col)
        if R.compare_values(col.dtype, b[i], b[j]) != 0:
            return False
    return True


def _groups(idx, same):
    """Split the sorted row list into runs of adjacent rows for which
    same(previous, row) holds."""
    out = []
    for r in idx:
        if out and same(out[-1][-1], r):
            out[-1].append(r)
        else:
            out.append([r])
    return out


def window(cols, masks, partition_by, order_by, emit, funcs):
    """cols: numpy columns (I128 = (n, 2) uint64); masks: {column: uint8};
    partition_by / order_by: [(column, order)]; emit: columns; funcs:
    [(func, col, frame, offset)] with col None or < 0 for count(*).
    Returns (columns, {output position: mask}): the emit columns, then
    one column per function."""
    n = len(cols[0])
    keys = list(partition_by) + list(order_by)
    if keys:
        idx = R.sort_indices([(cols[c], o, masks.get(c)) for c, o in keys])
    else:
        idx = list(range(n))
    take = np.asarray(idx, np.int64)
    out = [np.asarray(cols[c])[take] for c in emit]
    out_masks = {o: np.asarray(masks[c], np.uint8)[take]
                 for o, c in enumerate(emit) if c in masks}

    parts = _groups(idx, lambda a, b: _equal_on(cols, masks, partition_by,
                                                a, b))
    # per partition and per row of it: the peer group's number and its
    # first and last position inside the partition
    layout = []
    for part in parts:
        grp, first, last = [], [], []
        k = 0
        for g, pg in enumerate(_groups(
                part, lambda a, b: _equal_on(cols, masks, keys, a, b))):
            for _ in pg:
                grp.append(g)
                first.append(k)
                last.append(k + len(pg) - 1)
            k += len(pg)
        layout.append((part, grp, first, last))
    for f, (func, col, frame, offset) in enumerate(funcs):
        pos = len(emit) + f
        src = None if col is None or col < 0 else np.asarray(cols[col])
        smask = None if src is None else masks.get(col)
        if func in (MIN, MAX, LAG, LEAD):
            vals = np.zeros((n,) + src.shape[1:], _bits(src).dtype)
        else:
            vals = np.zeros(n, np.int64)
        nulls = np.zeros(n, np.uint8)
        at = 0          # output position of the partition's first row
        for part, grp, first, last in layout:
            # running state after each row, in sorted order
            run = []
            cnt, tot, lo, hi = 0, 0, None, None
            for r in part:
                null = smask is not None and bool(smask[r])
                if src is None:
                    cnt += 1
                elif not null:
                    cnt += 1
                    if func in (SUM, MIN, MAX):
                        v = int(src[r])
                        tot += v
                        lo = v if lo is None else min(lo, v)
                        hi = v if hi is None else max(hi, v)
                run.append((cnt, tot, lo, hi))
            for k, r in enumerate(part):
                o = at + k
                if func == ROW_NUMBER:
                    vals[o] = k + 1
                elif func == RANK:
                    vals[o] = first[k] + 1
                elif func == DENSE_RANK:
                    vals[o] = grp[k] + 1
                elif func in (LAG, LEAD):
                    t = k - offset if func == LAG else k + offset
                    if 0 <= t < len(part):
                        vals[o] = _bits(src)[part[t]]
                        nulls[o] = 0 if smask is None else smask[part[t]]
                    else:
                        nulls[o] = 1
                else:
                    end = {ROWS_RUNNING: k, RANGE_RUNNING: last[k],
                           PARTITION: len(part) - 1}[frame]
                    cnt, tot, lo, hi = run[end]
                    if func == COUNT:
                        vals[o] = cnt
                    elif cnt == 0:
                        nulls[o] = 1
                    elif func == SUM:
                        if not -2**63 <= tot < 2**63:
                            raise SumOverflow(f)
                        vals[o] = tot
                    else:
                        vals[o] = lo if func == MIN else hi
            at += len(part)
        if src is not None and src.dtype == np.float64 \
                and func in (LAG, LEAD):
            vals = vals.view(np.float64)
        out.append(vals)
        if func in (SUM, MIN, MAX, LAG, LEAD):
            out_masks[pos] = nulls
    return out, out_masks
