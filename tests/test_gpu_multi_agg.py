"""The multi-aggregate probe (LOOKUP_JOIN mode 1 with n_aggs > 0) against
the row-at-a-time reference of multi_agg_refs: k_probe_agg_multi,
k_groups_emit_multi and the packed branch of k_groups_count.

Every comparison is of exact integers, keyed by group key; the order of the
output rows is not part of the contract, that the keys are unique and as
many as the reference's is.  The datasets live in multi_agg_refs, where
tests/test_multi_agg_refs.py shows on the CPU that each one can see the
bugs it is meant to see and that none is ambiguous about overflow.

Geometry, read from the kernels:
  - k_probe_agg_multi: C = 4 consecutive rows per thread (an aligned quad),
    256 threads per block, 4096 blocks: BLOCK_ROWS = 1024 rows a block,
    PASS = 4 194 304 rows a grid pass.  A run is consecutive equal keys
    inside one thread's quad; one flush per run.
  - k_groups_count / k_groups_emit_multi: FLT_NB = 1024 blocks of 256
    threads over chunks of ceil(cap / 1024) slots rounded up to a multiple
    of 256.
"""
import numpy as np
import pytest

import multi_agg_refs as R

pytestmark = pytest.mark.gpu

QUAD, THREADS, BLOCKS = 4, 256, 4096
BLOCK_ROWS = QUAD * THREADS
PASS = BLOCK_ROWS * BLOCKS
assert (QUAD, BLOCK_ROWS, PASS) == (R.QUAD, 1024, 4_194_304)

SHAPES = ("hash", "range")


@pytest.fixture(scope="module")
def P():
    import presto_amd
    return presto_amd


@pytest.fixture(scope="module")
def pl(P):
    return P.plans


# --------------------------------------------------------------------- #
# from reference terms to plans                                          #
# --------------------------------------------------------------------- #
def _free(P, *ops):
    for op in ops:
        P.lib().c.pg_table_destroy(op.table())
        op.destroy()


def _build(P, tbl):
    """The device table of an R.Table, finished."""
    pl = P.plans
    if tbl.kind == "range":
        b = P.Operator(P.OP_HASH_BUILD, pl.range_group(tbl.K))
        pages = []
    else:
        cols = {"k": np.array(tbl.keys, np.int64)}
        for o, p in enumerate(tbl.payloads):
            cols[f"p{o}"] = np.ascontiguousarray(p)
        b = P.Operator(P.OP_HASH_BUILD, pl.hash_build(
            0, payload=list(range(1, len(cols))), agg_table=1,
            capacity_hint=len(tbl.keys), pack_bits=tbl.pack_bits,
            fill_x10=tbl.fill_x10, bitmap_max_key=tbl.bitmap_max_key))
        pages = [P.Page(cols)]
    try:
        for pg in pages:
            b.add_input(pg)
        b.finish()
    except BaseException:
        b.destroy()
        raise
    return b


def _pred(P, page, p):
    pl = P.plans
    ch = page.channel(p.col)
    if p.op == "is_null":
        return pl.pred_is_null(ch)
    if p.op == "not_null":
        return pl.pred_not_null(ch)
    op = {"lt": P.CMP_LT, "le": P.CMP_LE, "gt": P.CMP_GT, "ge": P.CMP_GE,
          "eq": P.CMP_EQ, "ne": P.CMP_NE}[p.op]
    return pl.pred(ch, op, p.rhs)


def _plan(P, table, page, spec):
    """The pg_plan_lookup_join of a Spec over the channels of `page`."""
    pl = P.plans
    aggs = []
    for ag in spec.aggs:
        if ag.kind == "count":
            aggs.append(pl.count())
        elif ag.kind == "sum_i64":
            aggs.append(pl.sum_i64(pl.ident(page.channel(ag.col))))
        else:
            aggs.append(pl.sum_dec(pl.ident(page.channel(ag.col)),
                                   ag.scale))
    fields = {}
    if spec.pack is not None:
        fields = dict(acc_pack=1, acc_pack_shift=list(spec.pack.shift),
                      acc_pack_width=list(spec.pack.width),
                      acc_pack_cnt_shift=spec.pack.cnt_shift,
                      acc_pack_cnt_width=spec.pack.cnt_width)
    plan = pl.lookup_join(
        table, page.channel(spec.key), 1,
        preds=[_pred(P, page, p) for p in spec.preds],
        filters=[_pred(P, page, p) for p in spec.filters], aggs=aggs,
        **fields)
    # agg_filter indexes preds[] as a whole, so that it can also name a
    # row predicate
    for a, ag in enumerate(spec.aggs):
        plan.agg_filter[a] = -1 if ag.filt is None else ag.filt
    return plan


def _dev_page(P, page):
    return P.Page({k: np.ascontiguousarray(v) for k, v in page.cols.items()},
                  nulls={k: np.ascontiguousarray(v)
                         for k, v in page.nulls.items()})


def _names(tbl, spec):
    return ["key"] + [f"p{o}" for o in range(len(tbl.payloads))] + \
        [f"a{a}" for a in range(len(spec.aggs))] + ["cnt"]


def _probe(P, build, tbl, pages, spec):
    """One operator over the pages; its groups page as the reference's
    dict.  A 0-row page still carries every column."""
    j = P.Operator(P.OP_LOOKUP_JOIN, _plan(P, build.table(), pages[0], spec))
    names = _names(tbl, spec)
    try:
        for pg in pages:
            j.add_input(_dev_page(P, pg))
        j.finish()
        out = j.get_output(names)
    finally:
        j.destroy()
    assert out is not None and list(out) == names
    for o, p in enumerate(tbl.payloads):
        assert out[f"p{o}"].dtype == p.dtype
    rows = list(zip(*(out[nm].tolist() for nm in names)))
    got = {r[0]: tuple(r[1:]) for r in rows}
    assert len(got) == len(rows), "a group key came out twice"
    return got


def _run(P, case):
    b = _build(P, case.table)
    try:
        return _probe(P, b, case.table, case.pages, case.spec)
    finally:
        _free(P, b)


def _check(P, case):
    """Clean cases equal the reference; must-raise cases raise at finish.
    Which one a case is was decided on the CPU (R.classify; also asserted
    for every dataset by tests/test_multi_agg_refs.py)."""
    assert R.classify(case.table, case.pages, case.spec) == case.expect
    if case.expect == "overflow":
        with pytest.raises(RuntimeError, match="overflow"):
            _run(P, case)
        return None
    ref = R.multi_agg_ref(case.table, case.pages, case.spec)
    got = _run(P, case)
    assert len(got) == len(ref)
    assert got == ref
    return ref


# --------------------------------------------------------------------- #
# a. row counts                                                          #
# --------------------------------------------------------------------- #
@pytest.mark.parametrize("n", R.SWEEP_NS)
def test_row_count_sweep(P, n):
    """Around the quad (3, 4, 5) and the block (1023, 1024, 1025); every
    row hits and carries a distinct value.  n = 0 gives a 0-row page with
    the full column list (_probe asserts the columns)."""
    ref = _check(P, R.sweep_case(n))
    assert sum(r[-1] for r in ref.values()) == n


def test_one_grid_pass_and_five_rows(P):
    """PASS + 5 rows, sorted keys: one run straddles the pass boundary,
    so the rows a thread takes on its second trip meet accumulators its
    neighbours filled on their first.  Checked with the numpy twin (the
    CPU tests hold it equal to the row model); clean because every |value|
    is < 1000 over 4.2 M rows."""
    n = PASS + 5
    c = R.pass_case(n)
    pg = c.pages[0]
    k = pg.cols["k"]
    assert k[PASS - 1] == k[PASS] and int(k[PASS]) in c.table.domain()
    assert int(np.abs(pg.cols["w"].astype(np.int64)).sum()) < 1 << 62
    ref = R.multi_agg_ref_np(c.table, c.pages, c.spec)
    assert len(ref) == len(c.table.keys)
    got = _run(P, c)
    assert len(got) == len(ref)
    assert got == ref


# --------------------------------------------------------------------- #
# b. run patterns                                                        #
# --------------------------------------------------------------------- #
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("pattern", list(R.RUN_PATTERNS))
def test_run_patterns(P, pattern, shape):
    """1025 rows: runs that straddle quads, waves and blocks; no run at
    all; a miss or a row failing the row predicate between two rows of one
    key; quads that start with key 0, the kernel's initial cur_key, which
    must be a miss and not a hit on slot 0."""
    ref = _check(P, R.run_case(pattern, shape))
    assert 0 not in ref and ref


# --------------------------------------------------------------------- #
# c. FILTER masks                                                        #
# --------------------------------------------------------------------- #
@pytest.mark.parametrize("name", ["six_filtered", "one_unfiltered",
                                  "counts"])
def test_filters(P, name):
    """six_filtered: I64, I32 and F64 left-hand sides, a null-masked
    column, IS_NULL, and agg_filter[5] = 0, a row predicate.  Group 5 has
    every row rejected by the first filter and keeps its row with sum 0
    and the full count."""
    ref = _check(P, R.filter_cases()[name])
    if name == "six_filtered":
        assert ref[5][0] == 0 and ref[5][-1] > 10


# --------------------------------------------------------------------- #
# d. table shapes                                                        #
# --------------------------------------------------------------------- #
@pytest.mark.parametrize("shape", list(R.shape_tables()))
def test_table_shapes(P, shape):
    """One table of the shape, a fresh operator per page with the
    accumulators zeroed in between.  The payload columns are compared with
    the sums.  all_miss gives a 0-row groups page."""
    tbl = R.shape_tables()[shape]
    b = _build(P, tbl)
    try:
        for name in R.shape_pages(shape):
            c = R.shape_case(shape, name)
            assert R.classify(c.table, c.pages, c.spec) == "clean"
            ref = R.multi_agg_ref(c.table, c.pages, c.spec)
            got = _probe(P, b, tbl, c.pages, c.spec)
            assert len(got) == len(ref), name
            assert got == ref, name
            assert (name == "all_miss") == (not got)
            assert P.lib().c.pg_table_reset_acc(b.table()) == 0
    finally:
        _free(P, b)


# --------------------------------------------------------------------- #
# e. packed layouts                                                      #
# --------------------------------------------------------------------- #
@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("layout", list(R.pack_layouts()))
def test_packed_layouts(P, layout, shape):
    """Group 20 fills every bit field to 2^w - 1 and the count to 7 next
    to groups whose fields stay 0; own words carry mixed signs.  The packed
    plan equals the reference and the same plan unpacked."""
    packed = R.pack_case(layout, shape, packed=True)
    ref = _check(P, packed)
    unpacked = R.pack_case(layout, shape, packed=False)
    assert _check(P, unpacked) == ref


@pytest.mark.parametrize("shape", SHAPES)
@pytest.mark.parametrize("name", R.PACK_RAISE)
def test_packed_contribution_raises(P, name, shape):
    """2^w in a w-bit field, an isolated negative row in a bit field, an
    own word of positive addends past int64."""
    c = R.pack_raise_case(name, shape)
    assert c.expect == "overflow"
    _check(P, c)


@pytest.mark.parametrize("shape", SHAPES)
def test_packed_contribution_that_fits(P, shape):
    """The companion of exactly_2_pow_w: 2^w - 1 passes."""
    c = R.pack_raise_case("2_pow_w_minus_1", shape)
    ref = _check(P, c)
    assert ref[9][1] == (1 << 7) - 1


# --------------------------------------------------------------------- #
# f. unpacked overflow                                                   #
# --------------------------------------------------------------------- #
@pytest.mark.parametrize("name", ["one_quad", "blocks_apart", "two_pages"])
def test_unpacked_overflow_raises(P, name):
    c = R.overflow_case(name)
    assert c.expect == "overflow"
    _check(P, c)


def test_unpacked_extremes_that_fit(P):
    ref = _check(P, R.overflow_clean_case())
    assert ref[4][0] == R.I64_MAX and ref[6][0] == R.I64_MIN + 1


# --------------------------------------------------------------------- #
# g. pages and operators                                                 #
# --------------------------------------------------------------------- #
@pytest.mark.parametrize("packed", [True, False], ids=["packed", "unpacked"])
@pytest.mark.parametrize("shape", SHAPES)
def test_pages_and_operators_accumulate(P, shape, packed):
    """Two pages into one operator; then the same two pages through two
    operators of one layout on one table, where the second groups page
    holds both operators' totals; then, after pg_table_reset_acc, a third
    operator whose page holds its own rows only."""
    c = R.accumulate_case(shape, packed)
    both = _check(P, c)
    first = R.multi_agg_ref(c.table, c.pages[:1], c.spec)
    second = R.multi_agg_ref(c.table, c.pages[1:], c.spec)
    assert first != both != second and set(second) - set(first)
    b = _build(P, c.table)
    try:
        assert _probe(P, b, c.table, c.pages[:1], c.spec) == first
        assert _probe(P, b, c.table, c.pages[1:], c.spec) == both
        assert P.lib().c.pg_table_reset_acc(b.table()) == 0
        assert _probe(P, b, c.table, c.pages[1:], c.spec) == second
    finally:
        _free(P, b)


# --------------------------------------------------------------------- #
# h. plan validation: every case fails pg_op_create                      #
# --------------------------------------------------------------------- #
@pytest.fixture(scope="module")
def small(P):
    b = _build(P, R.small_tables()["hash"])
    yield b
    _free(P, b)


def _packed_plan(P, table, shift, width, cnt_shift, cnt_width, aggs=None):
    pl = P.plans
    return pl.lookup_join(
        table, 0, 1, aggs=aggs or [pl.sum_i64(pl.ident(1))] * len(shift),
        acc_pack=1, acc_pack_shift=shift, acc_pack_width=width,
        acc_pack_cnt_shift=cnt_shift, acc_pack_cnt_width=cnt_width)


@pytest.mark.parametrize("func", ["AGG_MIN", "AGG_MAX", "AGG_SUM_F64"])
def test_only_count_and_tick_sums(P, pl, small, func):
    plan = pl.lookup_join(small.table(), 0, 1, aggs=[
        pl.count(), P.Agg(getattr(P, func), pl.ident(1), 0)])
    with pytest.raises(RuntimeError,
                       match=r"LOOKUP_JOIN: aggs\[1\]\.func = \d \(" +
                             func[4:] + r"\)"):
        P.Operator(P.OP_LOOKUP_JOIN, plan)


BAD_FIELDS = {
    # name: (shift, width, cnt_shift, cnt_width, message)
    "width_64_at_shift_0": ([0], [64], 0, 3, r"acc_pack_width\[0\]"),
    "cnt_width_64": ([0], [5], 0, 64, "acc_pack_cnt_width"),
    "negative_cnt_shift": ([0], [5], -1, 3, "acc_pack_cnt_shift"),
    "cnt_width_0": ([0], [5], 8, 0, "acc_pack_cnt_width"),
    "width_0": ([0, 8], [5, 0], 20, 3, r"acc_pack_width\[1\]"),
    "shift_plus_width_65": ([0, 60], [5, 5], 20, 3, r"acc_pack_shift\[1\]"),
    "cnt_shift_plus_width_65": ([0], [5], 62, 3, "acc_pack_cnt_shift"),
    "shift_minus_2": ([-2], [5], 20, 3, r"acc_pack_shift\[0\]"),
    "two_fields_overlap": ([0, 4], [5, 5], 20, 3,
                           r"acc_pack_shift\[1\].*overlaps"),
    "field_overlaps_count": ([0, 22], [5, 5], 20, 3,
                             r"acc_pack_shift\[1\].*overlaps"),
}


@pytest.mark.parametrize("name", list(BAD_FIELDS))
def test_bad_fields_fail_create(P, small, name):
    shift, width, cs, cw, msg = BAD_FIELDS[name]
    with pytest.raises(RuntimeError, match=msg):
        P.Operator(P.OP_LOOKUP_JOIN,
                   _packed_plan(P, small.table(), shift, width, cs, cw))


def test_n_aggs_7_and_chained_table(P, pl, small):
    plan = pl.lookup_join(small.table(), 0, 1, aggs=[pl.count()] * 6)
    plan.n_aggs = 7
    with pytest.raises(RuntimeError, match="n_aggs must be 1..6"):
        P.Operator(P.OP_LOOKUP_JOIN, plan)
    keys = np.arange(1, 9, dtype=np.int64)
    chained = P.Operator(P.OP_HASH_BUILD,
                         pl.hash_build(0, payload=[1], capacity_hint=8))
    try:
        chained.add_input(P.Page({"k": keys, "v": keys + 100}))
        chained.finish()
        with pytest.raises(RuntimeError,
                           match="multi-agg probes need an agg_table build"):
            P.Operator(P.OP_LOOKUP_JOIN, pl.lookup_join(
                chained.table(), 0, 1, aggs=[pl.count()]))
    finally:
        _free(P, chained)


def test_second_operator_must_repeat_the_layout(P, pl):
    """Same n_aggs and same stride (3 words) in all three plans: unpacked
    has the count in word 2, all-own-word packed in word 0, and the third
    moves a field.  Only the repeat of the first layout attaches, also
    after pg_table_reset_acc."""
    b = _build(P, R.small_tables()["hash"])
    t = b.table()
    two = [pl.sum_i64(pl.ident(1))] * 2
    unpacked = pl.lookup_join(t, 0, 1, aggs=two)
    all_own = _packed_plan(P, t, [-1, -1], [0, 0], 0, 3)
    ops = []
    try:
        ops.append(P.Operator(P.OP_LOOKUP_JOIN, unpacked))
        ops.append(P.Operator(P.OP_LOOKUP_JOIN, unpacked))
        for reset in (False, True):
            if reset:
                assert P.lib().c.pg_table_reset_acc(t) == 0
            with pytest.raises(RuntimeError,
                               match="different multi-agg layout"):
                P.Operator(P.OP_LOOKUP_JOIN, all_own)
            with pytest.raises(RuntimeError,
                               match="different multi-agg layout"):
                P.Operator(P.OP_LOOKUP_JOIN,
                           pl.lookup_join(t, 0, 1, aggs=two[:1]))
    finally:
        for op in ops:
            op.destroy()
        _free(P, b)
    # packed first: other shifts, other widths, another count field
    b = _build(P, R.small_tables()["range"])
    t = b.table()
    try:
        first = P.Operator(P.OP_LOOKUP_JOIN,
                           _packed_plan(P, t, [0, -1], [5, 0], 8, 3))
        ops = [first]
        # the width of an own word is not read, so this is the same layout
        ops.append(P.Operator(P.OP_LOOKUP_JOIN,
                              _packed_plan(P, t, [0, -1], [5, 9], 8, 3)))
        for shift, width, cs, cw in (([1, -1], [5, 0], 8, 3),
                                     ([0, -1], [6, 0], 8, 3),
                                     ([0, -1], [5, 0], 9, 3),
                                     ([0, -1], [5, 0], 8, 4),
                                     ([-1, 0], [0, 5], 8, 3)):
            with pytest.raises(RuntimeError,
                               match="different multi-agg layout"):
                P.Operator(P.OP_LOOKUP_JOIN,
                           _packed_plan(P, t, shift, width, cs, cw))
        with pytest.raises(RuntimeError, match="different multi-agg layout"):
            P.Operator(P.OP_LOOKUP_JOIN, pl.lookup_join(
                t, 0, 1, aggs=[pl.sum_i64(pl.ident(1))]))
    finally:
        for op in ops:
            op.destroy()
        _free(P, b)
