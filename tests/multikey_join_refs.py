"""Plain reference for the multi-key LOOKUP_JOIN emit joins
(include/presto_gpu.h: pg_plan_hash_build.n_keys / pg_plan_lookup_join
.n_keys).  No GPU, no library, no hashing tricks: row at a time over Python
tuples, a dict from key tuple to the list of build rows.  The tests compare
the operators against it, and test_multikey_join_refs.py checks it against
rows typed out by hand and against outer_join_refs.outer_join."""
import numpy as np

INNER, PROBE_OUTER, LOOKUP_OUTER, FULL_OUTER = 0, 4, 5, 6


def _key_rows(keys, nulls, n):
    """Per row: the key tuple of Python ints, or None when any channel is
    null.  keys: one array per channel; nulls: None, or per channel a mask
    (nonzero = null) or None."""
    chans = [np.asarray(k).tolist() for k in keys]
    for c in chans:
        assert len(c) == n
    nulls = [None] * len(chans) if nulls is None else list(nulls)
    assert len(nulls) == len(chans)
    masks = [None if m is None else np.asarray(m).tolist() for m in nulls]
    rows = []
    for i in range(n):
        if any(m is not None and m[i] != 0 for m in masks):
            rows.append(None)           # the value under a null is ignored
        else:
            rows.append(tuple(int(c[i]) for c in chans))
    return rows


def multikey_join(build_keys, build_key_nulls, build_payloads, probe_cols,
                  probe_keys, probe_key_nulls, pred_keep, mode):
    """One multi-key emit join over a single probe page.

    build_keys: one array per key channel, the build rows in build-row
    order (integers of any width: they compare as Python ints);
    build_key_nulls: None, or per channel a null mask or None;
    build_payloads: the payload columns; probe_cols: the emitted probe
    columns; probe_keys / probe_key_nulls: like the build's; pred_keep:
    which probe rows pass the predicates (None = all); mode: 0, 4, 5, 6.

    A row whose key is null in any channel matches nothing, on either side
    and in every mode (mode 0 included, unlike the single-key mode 0).

    Returns (cols, masks, drain) shaped like outer_join_refs.outer_join:
    cols: probe columns then payloads, rows in probe-row order and, within
      one probe row, in build-row order; a payload under a null is 0;
    masks: uint8 per output row, 1 = the payloads are null;
    drain: payload columns of the build rows no kept probe row matched, in
      build-row order, null-key build rows included (None in modes 0, 4)."""
    assert mode in (INNER, PROBE_OUTER, LOOKUP_OUTER, FULL_OUTER)
    assert len(build_keys) == len(probe_keys) and 1 <= len(build_keys) <= 4
    nb = len(build_keys[0])
    n = len(probe_keys[0])
    brows = _key_rows(build_keys, build_key_nulls, nb)
    prows = _key_rows(probe_keys, probe_key_nulls, n)
    keep = [True] * n if pred_keep is None \
        else [bool(x) for x in np.asarray(pred_keep).tolist()]
    table = {}
    for b, key in enumerate(brows):
        if key is not None:             # a null-key build row is not inserted
            table.setdefault(key, []).append(b)
    padding = mode in (PROBE_OUTER, FULL_OUTER)
    src, brow, is_pad = [], [], []
    matched = [False] * nb
    for i in range(n):
        if not keep[i]:
            continue
        hits = table.get(prows[i], []) if prows[i] is not None else []
        for b in hits:
            src.append(i)
            brow.append(b)
            is_pad.append(False)
            matched[b] = True
        if not hits and padding:
            src.append(i)
            brow.append(0)
            is_pad.append(True)
    src = np.asarray(src, np.int64)
    brow = np.asarray(brow, np.int64)
    pad = np.asarray(is_pad, bool)
    cols = [np.asarray(c)[src] for c in probe_cols]
    for p in build_payloads:
        p = np.asarray(p)
        vals = p[brow] if nb else np.zeros(len(src), p.dtype)
        cols.append(np.where(pad, np.zeros(1, p.dtype), vals))
    masks = pad.astype(np.uint8)
    drain = None
    if mode in (LOOKUP_OUTER, FULL_OUTER):
        unmatched = ~np.asarray(matched, bool)
        drain = [np.asarray(p)[unmatched] for p in build_payloads]
    return cols, masks, drain


def canonical(cols, masks=None):
    """The rows of `cols` (+ the mask as a last column) as one sorted list
    of tuples: the order of one probe row's matches is not pinned."""
    cols = [np.asarray(c) for c in cols]
    if masks is not None:
        cols = cols + [np.asarray(masks)]
    return sorted(zip(*(c.tolist() for c in cols)))
