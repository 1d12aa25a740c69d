"""Outer LOOKUP_JOIN modes (PG_JOIN_PROBE_OUTER / LOOKUP_OUTER /
FULL_OUTER), the null masks they put on output pages, and the
IS NULL / IS NOT NULL predicates — against the numpy references of
outer_join_refs.py.  All comparisons are exact.

Within one probe row the matches are compared as a sorted multiset (chain
order among duplicate build keys follows the order of parallel inserts);
probe-row order itself is checked through an emitted row-id column."""
import numpy as np
import pytest

import outer_join_refs as R

pytestmark = pytest.mark.gpu

OUTER = (R.PROBE_OUTER, R.LOOKUP_OUTER, R.FULL_OUTER)
PADDING = (R.PROBE_OUTER, R.FULL_OUTER)
DRAINING = (R.LOOKUP_OUTER, R.FULL_OUTER)


@pytest.fixture(scope="module")
def P():
    import presto_amd
    return presto_amd


@pytest.fixture(scope="module")
def pl():
    from presto_amd import plans
    return plans


# ---------------- plumbing ----------------

def _probe(P, pl, s, table, pages, mode, key_col, emit, preds=()):
    """One join operator over the probe pages: ([(cols, nulls) per page],
    drain (cols, nulls) or None).  Columns come back as c0, c1, ..."""
    j = s.op(P.OP_LOOKUP_JOIN,
             pl.lookup_join(table, key_col, mode, preds=preds, emit=emit))
    outs = []
    for pg in pages:
        j.add_input(pg)
        outs.append(j.get_output_nulls())
        assert j.get_output() is None
    j.finish()
    drain = j.get_output_nulls()
    assert j.get_output() is None and j.is_finished()
    s.release(j)
    return outs, drain


def _check_probe_page(got, ref_cols, ref_masks, mode, n_emit,
                      probe_masks=None):
    """One probe output page against the reference columns.  c0 must be
    the emitted row id.  probe_masks: {emit index: expected mask}."""
    cols, nulls = got
    names = [f"c{i}" for i in range(len(ref_cols))]
    assert list(cols) == names
    for nm, ref in zip(names, ref_cols):
        assert cols[nm].dtype == ref.dtype and len(cols[nm]) == len(ref), nm
    rowid = cols["c0"]
    assert np.all(rowid[1:] >= rowid[:-1])      # probe rows ascending
    pay = names[n_emit:]
    if mode in PADDING:
        mask = nulls[pay[0]]
        assert mask.dtype == np.uint8 and len(mask) == len(rowid)
        for nm in pay:                           # one mask for all payloads
            assert np.array_equal(nulls[nm], mask), nm
            assert not cols[nm][mask == 1].any(), nm   # 0 under a null
    else:
        assert not any(nm in nulls for nm in pay)
        mask = np.zeros(len(rowid), np.uint8)
    probe_masks = probe_masks or {}
    extra, ref_extra = [], []
    for o in range(n_emit):
        if o in probe_masks:
            extra.append(nulls[f"c{o}"])
            ref_extra.append(probe_masks[o])
        else:
            assert f"c{o}" not in nulls
    got_cols = [cols[nm] for nm in names] + extra
    exp_cols = list(ref_cols) + ref_extra
    if len(rowid) > 20000:      # unique build keys: the order is pinned
        for g, e in zip(got_cols + [mask], exp_cols + [ref_masks]):
            assert np.array_equal(g, e)
    else:
        assert R.canonical(got_cols, mask) == R.canonical(exp_cols, ref_masks)


def _check_drain(got, ref_drain, mode, n_emit, probe_dtypes):
    if mode not in DRAINING:
        assert got is None
        return
    cols, nulls = got
    n = len(ref_drain[0]) if ref_drain else 0
    for o in range(n_emit):                      # probe side: all null
        c = cols[f"c{o}"]
        assert c.dtype == probe_dtypes[o] and len(c) == n
        assert not c.any()
        assert np.array_equal(nulls[f"c{o}"], np.ones(n, np.uint8))
    for o, ref in enumerate(ref_drain):          # build-row order, exact
        nm = f"c{n_emit + o}"
        assert cols[nm].dtype == ref.dtype
        assert np.array_equal(cols[nm], ref), nm
        assert nm not in nulls


def _build(P, pl, s, keys, payloads, **kw):
    cols = {"k": np.asarray(keys, np.int64)}
    for i, p in enumerate(payloads):
        cols[f"p{i}"] = p
    b = s.build(pl.hash_build(0, payload=range(1, 1 + len(payloads)), **kw),
                P.Page(cols))
    return b.table()


def _join_all_modes(P, pl, bkeys, payloads, rowid, pkeys, modes=OUTER):
    """Chained build + one probe page [rowid, key] per mode, each checked
    against the reference."""
    with P.Scope() as s:
        table = _build(P, pl, s, bkeys, payloads)
        page = P.Page({"rowid": rowid, "k": pkeys})
        for mode in modes:
            outs, drain = _probe(P, pl, s, table, [page], mode, 1, [0])
            ref_cols, ref_masks, ref_drain = R.outer_join(
                bkeys, payloads, [rowid], pkeys, None, None, mode)
            _check_probe_page(outs[0], ref_cols, ref_masks, mode, 1)
            _check_drain(drain, ref_drain, mode, 1, [np.int64])


# ---------------- the hand case ----------------

BK = np.array([10, 20, 20, 30], np.int64)
P0 = np.array([100, 200, 201, 300], np.int64)
P1 = np.array([1, 2, 3, 4], np.int32)
PK = np.array([20, 5, 10, 20, 40], np.int64)
INNER_ROWS = [(0, 200, 2), (0, 201, 3), (2, 100, 1), (3, 200, 2),
              (3, 201, 3)]
LEFT_ROWS = [(0, 200, 2, 0), (0, 201, 3, 0), (1, 0, 0, 1), (2, 100, 1, 0),
             (3, 200, 2, 0), (3, 201, 3, 0), (4, 0, 0, 1)]


@pytest.mark.parametrize("mode", OUTER)
def test_hand_case(P, pl, mode):
    rowid = np.arange(5, dtype=np.int64)
    with P.Scope() as s:
        table = _build(P, pl, s, BK, [P0, P1])
        page = P.Page({"rowid": rowid, "k": PK})
        (inner,), none = _probe(P, pl, s, table, [page], 0, 1, [0])
        assert none is None and inner[1] == {}
        assert R.canonical(inner[0].values()) == INNER_ROWS
        ((cols, nulls),), drain = _probe(P, pl, s, table, [page], mode, 1,
                                         [0])
    assert [c.dtype for c in cols.values()] == [np.int64, np.int64, np.int32]
    assert "c0" not in nulls
    if mode in PADDING:
        assert sorted(nulls) == ["c1", "c2"]
        assert np.array_equal(nulls["c1"], nulls["c2"])
        mask = nulls["c1"]
        assert R.canonical(cols.values(), mask) == LEFT_ROWS
        assert cols["c0"].tolist() == [0, 0, 1, 2, 3, 3, 4]
        assert mask.tolist() == [0, 0, 1, 0, 0, 0, 1]
    else:
        assert nulls == {}
        mask = np.zeros(len(cols["c0"]), np.uint8)
    # the rows that are not null-padded are mode 0's output
    assert R.canonical([c[mask == 0] for c in cols.values()]) == INNER_ROWS
    if mode in DRAINING:
        dcols, dnulls = drain
        assert {k: v.tolist() for k, v in dcols.items()} == \
            {"c0": [0], "c1": [300], "c2": [4]}
        assert {k: v.tolist() for k, v in dnulls.items()} == {"c0": [1]}
    else:
        assert drain is None


# ---------------- tile and chunk boundaries ----------------

PATTERNS = ("all", "none", "alternating", "first_unmatched",
            "last_unmatched")


def _matched(pattern, n):
    m = np.ones(n, bool)
    if pattern == "none":
        m[:] = False
    elif pattern == "alternating":
        m[1::2] = False
    elif pattern == "first_unmatched":
        m[0] = False
    elif pattern == "last_unmatched":
        m[-1] = False
    return m


# 262145 is the first row count at which a block owns two 256-row tiles
# (the `running` carry between tiles); the rest straddle wave and tile edges
@pytest.mark.parametrize("n", [1, 63, 64, 65, 255, 256, 257, 513, 262145])
def test_boundaries(P, pl, n):
    rng = np.random.default_rng(n)
    rowid = np.arange(n, dtype=np.int64)
    pkeys = rowid + 1
    for pattern in PATTERNS:
        # three build rows no probe row ever matches keep the drain busy
        bkeys = np.concatenate([pkeys[_matched(pattern, n)],
                                np.array([n + 1, n + 2, n + 3])])
        bkeys = rng.permutation(bkeys).astype(np.int64)
        payloads = [bkeys * 10, (bkeys % 1000).astype(np.int32)]
        _join_all_modes(P, pl, bkeys, payloads, rowid, pkeys)


@pytest.mark.parametrize("n", [65, 257])
def test_boundaries_with_chains(P, pl, n):
    """Build chains of 1..5 rows per key and every third probe row
    unmatched: the output count differs from the input count on both sides
    of the wave / tile edge."""
    rng = np.random.default_rng(n)
    rowid = np.arange(n, dtype=np.int64)
    pkeys = rowid + 1
    hit = pkeys[rowid % 3 != 1]
    bkeys = np.repeat(hit, hit % 5 + 1)
    bkeys = rng.permutation(np.concatenate([bkeys, [n + 7]])).astype(np.int64)
    payloads = [np.arange(len(bkeys), dtype=np.int64),
                (bkeys % 100).astype(np.int32)]
    _join_all_modes(P, pl, bkeys, payloads, rowid, pkeys)


# ---------------- fuzz ----------------

@pytest.mark.parametrize("mode", OUTER)
@pytest.mark.parametrize("seed", [1, 2, 3])
def test_fuzz(P, pl, seed, mode):
    """Half the probe keys miss, duplicates on both sides, a predicate
    that drops a third of the probe rows, 5% null probe keys (over keys
    that would match), one emitted probe column with its own mask."""
    rng = np.random.default_rng(seed)
    n, nb, dom = 5000 - seed, 1500 + seed, 700
    bkeys = rng.integers(0, dom, nb).astype(np.int64)
    payloads = [rng.integers(-2**62, 2**62, nb).astype(np.int64),
                rng.integers(-2**31, 2**31, nb).astype(np.int32),
                rng.integers(0, 256, nb).astype(np.uint8)]
    pkeys = rng.integers(0, 2 * dom, n).astype(np.int64)
    key_nulls = (rng.random(n) < 0.05).astype(np.uint8)
    pkeys[key_nulls == 1] = bkeys[0]
    sel = rng.integers(0, 3, n).astype(np.int32)
    val = rng.integers(-1000, 1000, n).astype(np.int32)
    val_nulls = (rng.random(n) < 0.1).astype(np.uint8)
    rowid = np.arange(n, dtype=np.int64)
    page = P.Page({"rowid": rowid, "k": pkeys, "sel": sel, "val": val},
                  nulls={"k": key_nulls, "val": val_nulls})
    keep = sel != 0
    with P.Scope() as s:
        table = _build(P, pl, s, bkeys, payloads)
        outs, drain = _probe(P, pl, s, table, [page], mode, 1, [0, 3],
                             preds=[pl.pred(2, P.CMP_NE, 0)])
    ref_cols, ref_masks, ref_drain = R.outer_join(
        bkeys, payloads, [rowid, val], pkeys, key_nulls, keep, mode)
    _check_probe_page(outs[0], ref_cols, ref_masks, mode, 2,
                      probe_masks={1: val_nulls[ref_cols[0]]})
    _check_drain(drain, ref_drain, mode, 2, [np.int64, np.int32])
    assert 0 < ref_masks.sum() or mode == R.LOOKUP_OUTER
    assert ref_drain is None or 0 < len(ref_drain[0]) < nb


# ---------------- several pages on both sides ----------------

@pytest.mark.parametrize("mode", DRAINING)
def test_multi_page(P, pl, mode):
    """The drain reflects the marks of every probe page and keeps
    build-row order across build pages."""
    b1 = np.array([5, 1, 9, 1], np.int64)
    b2 = np.array([7, 5, 3], np.int64)
    bkeys = np.concatenate([b1, b2])
    pay = np.arange(100, 107, dtype=np.int64)
    p1 = np.array([1, 2], np.int64)          # marks build rows 1, 3
    p2 = np.array([3, 8, 1], np.int64)       # marks build row 6 (1 again)
    with P.Scope() as s:
        b = s.build(pl.hash_build(0, payload=[1]),
                    P.Page({"k": b1, "p": pay[:4]}),
                    P.Page({"k": b2, "p": pay[4:]}))
        pages = [P.Page({"rowid": np.arange(2, dtype=np.int64), "k": p1}),
                 P.Page({"rowid": np.arange(2, 5, dtype=np.int64), "k": p2})]
        outs, drain = _probe(P, pl, s, b.table(), pages, mode, 1, [0])
        # a second operator over the same table has marks of its own
        _, drain_none = _probe(P, pl, s, b.table(), [], mode, 1, [0, 1])
        empty = P.Page({"rowid": np.empty(0, np.int32),
                        "k": np.empty(0, np.int64)})
        outs0, drain_empty = _probe(P, pl, s, b.table(), [empty], mode, 1,
                                    [0])
    assert drain[0]["c1"].tolist() == [100, 102, 104, 105]   # keys 5 9 7 5
    assert drain[0]["c0"].tolist() == [0, 0, 0, 0]
    assert drain[1]["c0"].tolist() == [1, 1, 1, 1]
    if mode == R.FULL_OUTER:
        exp = [[(0, 101, 0), (0, 103, 0), (1, 0, 1)],
               [(2, 106, 0), (3, 0, 1), (4, 101, 0), (4, 103, 0)]]
    else:
        exp = [[(0, 101, 0), (0, 103, 0)],
               [(2, 106, 0), (4, 101, 0), (4, 103, 0)]]
    for (cols, nulls), e in zip(outs, exp):
        mask = nulls.get("c1", np.zeros(len(cols["c0"]), np.uint8))
        assert R.canonical(cols.values(), mask) == e
    # no page fed: every build row drains, probe columns default to I64
    cols, nulls = drain_none
    assert cols["c2"].tolist() == pay.tolist()
    assert cols["c0"].dtype == np.int64 and cols["c1"].dtype == np.int64
    assert sorted(nulls) == ["c0", "c1"]
    # a 0-row page fed: a 0-row output with the same columns, same drain,
    # probe columns typed as in that page
    (cols, nulls), = outs0
    assert [(k, v.dtype, len(v)) for k, v in cols.items()] == \
        [("c0", np.int32, 0), ("c1", np.int64, 0)]
    cols, nulls = drain_empty
    assert cols["c1"].tolist() == pay.tolist()
    assert cols["c0"].dtype == np.int32 and cols["c0"].tolist() == [0] * 7
    assert nulls["c0"].tolist() == [1] * 7 and "c1" not in nulls


# ---------------- table shapes ----------------

SHAPES = {
    "agg_table": dict(agg_table=1, capacity_hint=64),
    "packed_agg_table": dict(agg_table=1, capacity_hint=64, pack_bits=8),
    "dense_array": dict(dense_array=1, capacity_hint=40),
}


@pytest.mark.parametrize("shape", SHAPES)
def test_left_join_over_other_table_shapes(P, pl, shape):
    """Mode 4 takes every table mode 0 takes; modes 5 and 6 need the
    build-row arrays only chained tables keep."""
    bkeys = np.array([3, 17, 8, 40, 21], np.int64)     # unique, in 1..40
    pay = (bkeys + 100).astype(np.uint8)
    n = 300
    rowid = np.arange(n, dtype=np.int64)
    pkeys = (rowid * 7) % 45
    page = P.Page({"rowid": rowid, "k": pkeys})
    with P.Scope() as s:
        table = _build(P, pl, s, bkeys, [pay], **SHAPES[shape])
        outs, drain = _probe(P, pl, s, table, [page], R.PROBE_OUTER, 1, [0])
        assert drain is None
        ref_cols, ref_masks, _ = R.outer_join(bkeys, [pay], [rowid], pkeys,
                                              None, None, R.PROBE_OUTER)
        _check_probe_page(outs[0], ref_cols, ref_masks, R.PROBE_OUTER, 1)
        for mode in DRAINING:
            with pytest.raises(RuntimeError, match=f"mode {mode}"):
                P.Operator(P.OP_LOOKUP_JOIN,
                           pl.lookup_join(table, 1, mode, emit=[0]))


# ---------------- IS NULL / IS NOT NULL ----------------

def _filter(P, plan, page, names=None):
    op = P.Operator(P.OP_FILTER_PROJECT, plan)
    try:
        op.feed(page)
        return op.get_output(names)
    finally:
        op.destroy()


def test_null_predicates_in_filter_project(P, pl):
    n = 1000
    rng = np.random.default_rng(7)
    rowid = np.arange(n, dtype=np.int64)
    masked = rng.integers(0, 9, n).astype(np.int64)
    mask = (rng.random(n) < 0.3).astype(np.uint8)
    plain = rng.random(n)
    words = [b"", b"special", b"requests and more", b"x"]
    text = P.Varbin([words[i % 4] for i in range(n)])
    tmask = (rng.random(n) < 0.5).astype(np.uint8)
    coded = P.DictVarbin(words, rng.integers(0, 4, n))
    cmask = (rng.random(n) < 0.2).astype(np.uint8)
    page = P.Page({"rowid": rowid, "masked": masked, "plain": plain,
                   "text": text, "coded": coded},
                  nulls={"masked": mask, "text": tmask, "coded": cmask})
    cases = [(1, mask), (2, np.zeros(n, np.uint8)), (3, tmask), (4, cmask)]
    for col, m in cases:
        got = _filter(P, pl.filter_project([pl.ident(0)],
                                           preds=[pl.pred_is_null(col)]),
                      page)["c0"]
        assert np.array_equal(got, rowid[m == 1]), col
        got = _filter(P, pl.filter_project([pl.ident(0)],
                                           preds=[pl.pred_not_null(col)]),
                      page)["c0"]
        assert np.array_equal(got, rowid[m == 0]), col
    # next to a comparison on the same column: nulls stay excluded
    got = _filter(P, pl.filter_project(
        [pl.ident(0)], preds=[pl.pred_not_null(1),
                              pl.pred(1, P.CMP_GE, 4)]), page)["c0"]
    assert np.array_equal(got, rowid[(mask == 0) & (masked >= 4)])
    got = _filter(P, pl.filter_project(
        [pl.ident(0)], preds=[pl.pred_is_null(1),
                              pl.pred(1, P.CMP_GE, 0)]), page)["c0"]
    assert len(got) == 0


@pytest.mark.parametrize("shape", ["agg_table", "dense_array"])
def test_single_scan_builds_reject_null_tests(P, pl, shape):
    """The single-scan build kernels evaluate comparisons only; a null
    test there is refused at create, never misread.  A chained build
    takes it."""
    for pred in (pl.pred_is_null(1), pl.pred_not_null(1)):
        with pytest.raises(RuntimeError, match="IS NULL"):
            P.Operator(P.OP_HASH_BUILD, pl.hash_build(
                0, payload=[1], preds=[pred], **SHAPES[shape]))
    keys = np.arange(1, 9, dtype=np.int64)
    mask = (keys % 2).astype(np.uint8)
    with P.Scope() as s:
        b = s.build(pl.hash_build(0, payload=[1],
                                  preds=[pl.pred_not_null(1)]),
                    P.Page({"k": keys, "p": keys * 3}, nulls={"p": mask}))
        outs, _ = _probe(P, pl, s, b.table(),
                         [P.Page({"rowid": keys, "k": keys})], 0, 1, [0])
    assert outs[0][0]["c0"].tolist() == [2, 4, 6, 8]
    assert outs[0][0]["c1"].tolist() == [6, 12, 18, 24]


def _left_join_data():
    rng = np.random.default_rng(11)
    n, nb = 3000, 400
    bkeys = rng.integers(0, 500, nb).astype(np.int64)
    pay = rng.integers(1, 10**6, nb).astype(np.int64)
    pkeys = rng.integers(0, 1000, n).astype(np.int64)
    key_nulls = (rng.random(n) < 0.05).astype(np.uint8)
    return bkeys, pay, pkeys, key_nulls


def test_raw_left_join_page_feeds_is_null_filter(P, pl):
    """LEFT JOIN ... WHERE payload IS NULL over the raw device page: the
    masks in the snapshot are honoured downstream (the anti join)."""
    bkeys, pay, pkeys, key_nulls = _left_join_data()
    rowid = np.arange(len(pkeys), dtype=np.int64)
    with P.Scope() as s:
        table = _build(P, pl, s, bkeys, [pay])
        j, raw = s.pipe(P.OP_LOOKUP_JOIN, pl.left_join(table, 1, [0]),
                        P.Page({"rowid": rowid, "k": pkeys},
                               nulls={"k": key_nulls}))
        assert raw.cols[1].null_mask and not raw.cols[0].null_mask
        got = _filter(P, pl.filter_project([pl.ident(0)],
                                           preds=[pl.pred_is_null(1)]), raw)
        hits = _filter(P, pl.filter_project([pl.ident(0)],
                                            preds=[pl.pred_not_null(1)]), raw)
    anti = R.anti_join(bkeys, pkeys, key_nulls)
    assert np.array_equal(got["c0"], rowid[anti])
    assert 0 < len(anti) < len(pkeys)
    assert set(hits["c0"].tolist()) == set(rowid.tolist()) - set(anti.tolist())


def test_count_of_column_in_groupby_multi(P, pl):
    """count(payload) per probe row = COUNT FILTER (payload IS NOT NULL)
    over the raw LEFT join page; the plain row count still counts the
    null-padded row."""
    bkeys, pay, pkeys, key_nulls = _left_join_data()
    rowid = np.arange(len(pkeys), dtype=np.int64)
    with P.Scope() as s:
        table = _build(P, pl, s, bkeys, [pay])
        j, raw = s.pipe(P.OP_LOOKUP_JOIN, pl.left_join(table, 1, [0]),
                        P.Page({"rowid": rowid, "k": pkeys},
                               nulls={"k": key_nulls}))
        g = s.run(P.OP_GROUPBY_MULTI, pl.group_by(
            [0], [(pl.count(), 0)], len(rowid) + 16,
            filters=[pl.pred_not_null(1)]), raw)
        out = g.get_output(["rowid", "count_pay", "rows"])
    ref_cols, ref_masks, _ = R.outer_join(bkeys, [pay], [rowid], pkeys,
                                          key_nulls, None, R.PROBE_OUTER)
    exp_rows = np.bincount(ref_cols[0], minlength=len(rowid))
    exp_cnt = np.bincount(ref_cols[0][ref_masks == 0], minlength=len(rowid))
    order = np.argsort(out["rowid"])
    assert np.array_equal(out["rowid"][order], rowid)
    assert np.array_equal(out["count_pay"][order], exp_cnt)
    assert np.array_equal(out["rows"][order], exp_rows)
    assert (exp_cnt == 0).any() and (exp_cnt > 1).any()


Q1_COLS = ("quantity", "extendedprice", "discount", "tax", "shipdate",
           "returnflag", "linestatus")
QTY, EP, DC, TX, SD, RF, LS = range(7)


def _q1_plan(P, pl, preds):
    aggs = [P.Agg(P.AGG_SUM_DEC, proj, scale) for proj, scale in (
        (pl.ident(QTY), 0), (pl.ident(EP), 2), (pl.disc_price(EP, DC), 4),
        (pl.charge(EP, DC, TX), 6), (pl.ident(DC), 2))]
    return pl.small_agg(aggs + [pl.count()], preds=preds,
                        keys=[(RF, b"ANR"), (LS, b"FO")])


def _fast_launches(P):
    import ctypes as C
    f = P.lib().c.pg_q1_fast_launches
    f.restype = C.c_int64
    return f()


def _agg(P, plan, page):
    op = P.Operator(P.OP_HASH_AGG_SMALL, plan)
    try:
        op.feed(page)
        op.finish()
        return op.get_output()
    finally:
        op.destroy()


def test_q1_shape_with_not_null_takes_the_generic_kernel(P, pl, oracle_lib):
    """The Q1 plan with `shipdate IS NOT NULL` in place of its date
    comparison has the fast path's shape in every other respect; the
    specialised kernel would read the predicate as a comparison."""
    li = oracle_lib.gen_lineitem(0.01)
    n = 4097
    cols = {k: np.ascontiguousarray(li[k][:n]) for k in Q1_COLS}
    i32max = 2**31 - 1
    before = _fast_launches(P)
    fast = _agg(P, _q1_plan(P, pl, [pl.pred(SD, P.CMP_LE, i32max)]),
                P.Page(cols))
    assert _fast_launches(P) == before + 1      # the shape is the fast one
    got = _agg(P, _q1_plan(P, pl, [pl.pred_not_null(SD)]), P.Page(cols))
    assert _fast_launches(P) == before + 1
    assert list(got) == list(fast)
    for k in fast:                  # every row kept: same exact sums
        assert np.array_equal(got[k], fast[k]), k
    # with a mask, the null rows leave — generic kernel on both sides
    mask = (np.arange(n) % 5 == 3).astype(np.uint8)
    got = _agg(P, _q1_plan(P, pl, [pl.pred_not_null(SD)]),
               P.Page(cols, nulls={"shipdate": mask}))
    exp = _agg(P, _q1_plan(P, pl, [pl.pred(SD, P.CMP_LE, i32max)]),
               P.Page(cols, nulls={"shipdate": mask}))
    assert _fast_launches(P) == before + 1
    for k in exp:
        assert np.array_equal(got[k], exp[k]), k
    last = list(got)[-1]                         # the group row count
    assert int(got[last].sum()) == int((mask == 0).sum())


# ---------------- q13 through the general operators ----------------

def test_q13_through_left_join(P, pl, oracle_lib):
    """customer LEFT JOIN orders (comment NOT LIKE '%special%requests%'),
    count(o_orderkey) per customer, then customers per count — SF 0.01."""
    sf = 0.01
    orders = oracle_lib.gen_orders(sf)
    data, offs = oracle_lib.gen_orders_comment_varbin(sf)
    comment = P.Varbin.from_arrays(data, offs)
    cust = oracle_lib.gen_customer(sf)
    n_cust = len(cust["custkey"])
    assert (n_cust, len(orders["orderkey"])) == (1500, 15000)
    with P.Scope() as s:
        b = s.build(
            pl.hash_build(0, payload=[1], preds=[pl.pred_varbin(
                2, P.CMP_NOT_CONTAINS2, b"special", b"requests")]),
            P.Page({"custkey": orders["custkey"],
                    "orderkey": orders["orderkey"], "comment": comment}))
        j, joined = s.pipe(P.OP_LOOKUP_JOIN,
                           pl.left_join(b.table(), 0, [0]),
                           P.Page({"custkey": cust["custkey"]}))
        # [c_custkey, o_orderkey (nullable)]
        per_cust = s.run(P.OP_GROUPBY_MULTI, pl.group_by(
            [0], [(pl.count(), 0)], n_cust + 16,
            filters=[pl.pred_not_null(1)]), joined)
        counts = per_cust.get_output_raw()     # [custkey, c_count, rows]
        assert counts.n_rows == n_cust
        dist = s.run(P.OP_GROUPBY_MULTI,
                     pl.group_by([1], [pl.count()], 1024), counts)
        out = dist.get_output(["c_count", "custdist", "rows"])
    got = sorted(zip(out["c_count"].tolist(), out["custdist"].tolist()),
                 key=lambda r: (-r[1], -r[0]))
    assert got == oracle_lib.q13(sf, orders)
    assert any(c == 0 for c, _ in got)      # the LEFT join's zero bucket
