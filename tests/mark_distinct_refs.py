"""Row-at-a-time reference of PG_OP_MARK_DISTINCT (include/presto_gpu.h,
pg_plan_mark_distinct): a dict of key tuples, None for a null.  No GPU, no
numpy tricks — this is the checker, never the product.

keys: one sequence per key channel; key_masks: per channel a sequence of
0 / 1 (1 = null) or None for a channel without a mask.  The rows are those
of all pages, in page order then row order; `seen` carries the key tuples
of earlier pages when the pages are fed one at a time.
"""


def key_tuples(keys, key_masks):
    """One tuple per row; a null key is None whatever is stored under it."""
    out = []
    for i in range(len(keys[0])):
        out.append(tuple(
            None if (m is not None and m[i]) else int(k[i])
            for k, m in zip(keys, key_masks)))
    return out


def markers(keys, key_masks, seen=None):
    """[1 if row i is the first row with its key tuple else 0]."""
    seen = set() if seen is None else seen
    out = []
    for t in key_tuples(keys, key_masks):
        out.append(0 if t in seen else 1)
        seen.add(t)
    return out


def first_rows(keys, key_masks, seen=None):
    """Only mode: the indexes of the first rows, ascending."""
    return [i for i, m in enumerate(markers(keys, key_masks, seen)) if m]


def distinct_pages(keys, key_masks, splits, limit=0):
    """Only mode over the pages [splits[p], splits[p+1]): per page fed, the
    list of GLOBAL row indexes it emits.  With limit > 0 the page that
    reaches the limit is cut to fit and is the last one fed: the operator
    takes no more input, so the list is shorter than the page list."""
    tuples = key_tuples(keys, key_masks)
    seen, emitted, pages = set(), 0, []
    for lo, hi in zip(splits, splits[1:]):
        rows = []
        for i in range(lo, hi):
            if tuples[i] not in seen:
                seen.add(tuples[i])
                rows.append(i)
        if limit > 0 and emitted + len(rows) >= limit:
            pages.append(rows[:limit - emitted])
            return pages
        emitted += len(rows)
        pages.append(rows)
    return pages
