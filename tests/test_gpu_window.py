"""PG_OP_WINDOW on the GPU against the row-at-a-time reference of
window_refs.py.  Every comparison is exact (floats through their bit
patterns), every case emits a row-id column so that the order of ties is
visible in the result.

Sizes follow the kernel's geometry (kernels.hip): a wave is 64 lanes, a
block scans SORT_WINDOW = 256 rows per step and owns a chunk of at least
SORT_MIN_WINDOWS = 4 windows, at most SORT_NB = 1024 blocks run — so below
2^20 rows the chunk IS 1024 rows, and 3 * CHUNK + 1 rows are four blocks
with a one-row last chunk."""
import ctypes as C

import numpy as np
import pytest

import order_by_refs as R
import window_refs as W

pytestmark = pytest.mark.gpu

WAVE = 64
WINDOW = 256          # SORT_WINDOW
CHUNK = 4 * WINDOW    # SORT_MIN_WINDOWS * SORT_WINDOW

T_U8, T_I32, T_I64, T_F64, T_I128 = 0, 1, 2, 3, 5
_NP_OF_TAG = {T_U8: np.uint8, T_I32: np.int32, T_I64: np.int64,
              T_F64: np.float64}
ASC, DESC = R.ASC_NULLS_LAST, R.DESC_NULLS_LAST
RANGE, ROWS, PART = W.RANGE_RUNNING, W.ROWS_RUNNING, W.PARTITION


@pytest.fixture(scope="module")
def P():
    import presto_amd
    return presto_amd


@pytest.fixture(scope="module")
def pl():
    from presto_amd import plans
    return plans


# ---------------- plumbing ----------------

def _make_page(P, cols, masks, device):
    """cols: numpy columns ((n, 2) uint64 = I128); masks: {index: uint8}.
    Returns (keepalive, raw PgPage)."""
    import torch
    n = len(cols[0])
    named, nulls = {}, {}
    for i, a in enumerate(cols):
        a = np.ascontiguousarray(a)
        flat = a.view(np.int64).reshape(-1) if a.ndim == 2 else a
        named[f"c{i}"] = torch.from_numpy(flat).cuda() if device else flat
        if i in masks:
            m = np.ascontiguousarray(masks[i], np.uint8)
            nulls[f"c{i}"] = torch.from_numpy(m).cuda() if device else m
    page = P.Page(named, n_rows=n, nulls=nulls)
    raw = page.to_c()
    for i, a in enumerate(cols):
        if np.asarray(a).ndim == 2:
            raw.cols[i].tag = T_I128
    if device:
        torch.cuda.synchronize()
    return page, raw


def _d2h(P, ptr, nbytes):
    buf = np.empty(nbytes, np.uint8)
    if nbytes:
        L = P.lib()
        L.check(L.c.pg_memcpy_d2h(buf.ctypes.data, ptr, nbytes), "d2h")
    return buf


def _read_raw(P, raw):
    """A raw device output page -> (columns, {position: mask})."""
    n = raw.n_rows
    cols, masks = [], {}
    for i in range(raw.n_cols):
        c = raw.cols[i]
        assert c.on_device == 1
        if c.tag == T_I128:
            cols.append(_d2h(P, c.data, n * 16).view(np.uint64)
                        .reshape(n, 2))
        else:
            dt = np.dtype(_NP_OF_TAG[c.tag])
            cols.append(_d2h(P, c.data, n * dt.itemsize).view(dt))
        if c.null_mask:
            masks[i] = _d2h(P, c.null_mask, n)
    return cols, masks


def _specs(P, funcs):
    return [P.WinSpec(f, -1 if c is None else c, fr, 0, off)
            for f, c, fr, off in funcs]


def _plan(P, pl, part, order, emit, funcs):
    return pl.window(part, order, emit, _specs(P, funcs))


def _window(P, pl, pages, part, order, emit, funcs, device=None):
    """pages: [(cols, masks)].  device: per-page flags (default: page i is
    device-resident when i is odd).  Runs the whole lifecycle and returns
    (columns, masks) of the one output page."""
    with P.Scope() as s:
        op = s.op(P.OP_WINDOW, _plan(P, pl, part, order, emit, funcs))
        for i, (cols, masks) in enumerate(pages):
            dev = (i % 2 == 1) if device is None else device[i]
            keep, raw = _make_page(P, cols, masks, dev)
            assert op.needs_input()
            op.add_input_raw(raw)
            del keep
        assert op.get_output_raw() is None
        op.finish()
        raw = op.get_output_raw()
        assert raw is not None
        got = _read_raw(P, raw)
        assert op.get_output_raw() is None and op.is_finished()
    return got


def _bits(a):
    a = np.asarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _assert_same(got, ref, names=None):
    gcols, gmasks = got
    rcols, rmasks = ref
    assert len(gcols) == len(rcols)
    for o, (g, r) in enumerate(zip(gcols, rcols)):
        what = (o, names[o]) if names else o
        r = np.asarray(r)
        assert g.dtype == r.dtype and g.shape == r.shape, what
        if not np.array_equal(_bits(g), _bits(r)):
            bad = np.flatnonzero((_bits(g) != _bits(r)).reshape(len(g), -1)
                                 .any(axis=1))
            assert False, (what, bad[:5], _bits(g)[bad[:5]],
                           _bits(r)[bad[:5]])
    assert sorted(gmasks) == sorted(rmasks)
    for o in rmasks:
        assert np.array_equal(gmasks[o], rmasks[o]), \
            (o, names[o]) if names else o


def _check(P, pl, pages, part, order, funcs, emit=(0,), device=None):
    """The reference once over all functions; the operator in plans of at
    most eight functions each."""
    emit = list(emit)
    cols, masks = R.concat_pages(pages)
    rcols, rmasks = W.window(cols, masks, part, order, emit, funcs)
    ne = len(emit)
    for at in range(0, len(funcs), 8):
        group = funcs[at:at + 8]
        pos = list(range(ne)) + [ne + at + k for k in range(len(group))]
        ref = ([rcols[p] for p in pos],
               {o: rmasks[p] for o, p in enumerate(pos) if p in rmasks})
        got = _window(P, pl, pages, part, order, emit, group, device)
        _assert_same(got, ref, ["emit"] * ne + group)
    return rcols, rmasks


def _rowid(n):
    return np.arange(n, dtype=np.int64)


# ---------------- data ----------------
# columns of every table: 0 rowid, 1 partition key (i64), 2 order key
# (i32), 3 i64 value (masked), 4 i32 value (masked), 5 u8 value, 6 f64
# (masked), 7 i128, 8 full-range i64 (MIN / MAX only: its SUM overflows)

def _table(rng, pkey, okey, null_parts=()):
    n = len(pkey)
    f = rng.integers(-2**63, 2**63 - 1, n).view(np.float64)
    cols = [_rowid(n), np.asarray(pkey, np.int64), np.asarray(okey, np.int32),
            rng.integers(-2**40, 2**40, n),
            rng.integers(-2**31, 2**31, n).astype(np.int32),
            rng.integers(0, 256, n).astype(np.uint8),
            f,
            rng.integers(0, 2**63, (n, 2)).astype(np.uint64),
            rng.integers(-2**63, 2**63 - 1, n, endpoint=True)]
    m3 = (rng.random(n) < 0.3).astype(np.uint8)
    for p in null_parts:            # a partition whose every value is null
        m3[cols[1] == p] = 1
    masks = {3: m3, 4: (rng.random(n) < 0.5).astype(np.uint8),
             6: (rng.random(n) < 0.2).astype(np.uint8)}
    # what sits under a null is never looked at
    cols[3] = np.where(m3 == 1, rng.integers(-2**63, 2**63 - 1, n), cols[3])
    return cols, masks


def _frames(func, col):
    return [(func, col, fr, 0) for fr in (RANGE, ROWS, PART)]


RANKS = [(W.ROW_NUMBER, None, 0, 0), (W.RANK, None, 0, 0),
         (W.DENSE_RANK, None, 0, 0)] + _frames(W.COUNT, None) + \
        [(W.COUNT, 3, RANGE, 0), (W.COUNT, 6, ROWS, 0)]
SUMS = _frames(W.SUM, 3) + [(W.SUM, 4, ROWS, 0), (W.SUM, 5, RANGE, 0),
                            (W.MIN, 8, ROWS, 0), (W.MAX, 8, RANGE, 0),
                            (W.MIN, 5, PART, 0)]
MINMAX = _frames(W.MIN, 3) + _frames(W.MAX, 3) + \
    [(W.MIN, 4, ROWS, 0), (W.MAX, 5, RANGE, 0)]
SHIFTS = [(W.LAG, 3, 0, 1), (W.LEAD, 3, 0, 1), (W.LAG, 6, 0, 2),
          (W.LEAD, 7, 0, 3), (W.LAG, 5, 0, 0), (W.LEAD, 4, 0, 300),
          (W.LAG, 7, 0, 1), (W.LEAD, 6, 0, 2**40)]
EVERYTHING = RANKS + SUMS + MINMAX + SHIFTS
# one of each kind, for the shapes that vary something else
MIXED = [(W.ROW_NUMBER, None, 0, 0), (W.RANK, None, 0, 0),
         (W.DENSE_RANK, None, 0, 0), (W.SUM, 3, RANGE, 0),
         (W.MIN, 4, ROWS, 0), (W.MAX, 5, PART, 0), (W.LAG, 3, 0, 1),
         (W.LEAD, 6, 0, 2)]
BY_PKEY, BY_OKEY = [(1, ASC)], [(2, ASC)]


# ---------------- sizes ----------------

@pytest.mark.parametrize("n", [
    0, 1, 2, WAVE - 1, WAVE, WAVE + 1, WINDOW - 1, WINDOW, WINDOW + 1,
    CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 1])
def test_sizes(P, pl, n):
    rng = np.random.default_rng(n)
    pkey = rng.integers(0, max(1, n // 40), n)
    okey = rng.integers(0, 6, n)
    _check(P, pl, [_table(rng, pkey, okey)], BY_PKEY, BY_OKEY, MIXED,
           device=[True])


# ---------------- partition shapes ----------------

def test_one_partition_over_four_chunks(P, pl):
    """The carry crosses blocks, and the middle chunks contain no
    partition head."""
    n = 3 * CHUNK + 1
    rng = np.random.default_rng(101)
    okey = rng.integers(0, n // 5, n)
    _check(P, pl, [_table(rng, np.zeros(n), okey)], [], BY_OKEY, EVERYTHING)


def test_one_partition_of_peers(P, pl):
    """No keys at all: the input order, one peer group over every chunk."""
    n = 2 * CHUNK + 7
    rng = np.random.default_rng(103)
    ref, _ = _check(P, pl, [_table(rng, np.zeros(n), np.zeros(n))], [], [],
                    RANKS + SUMS + SHIFTS)
    assert np.array_equal(ref[0], _rowid(n))


def test_all_singleton_partitions(P, pl):
    n = 2 * CHUNK + 1
    rng = np.random.default_rng(107)
    _check(P, pl, [_table(rng, rng.permutation(n), np.zeros(n))], BY_PKEY,
           BY_OKEY, MIXED + SHIFTS)


def test_partition_heads_at_the_first_and_last_row_of_a_chunk(P, pl):
    sizes = [CHUNK - 1, 1, CHUNK - 1, 1, CHUNK + 1]
    heads = np.cumsum([0] + sizes[:-1])
    assert heads.tolist() == [0, CHUNK - 1, CHUNK, 2 * CHUNK - 1, 2 * CHUNK]
    rng = np.random.default_rng(109)
    pkey = np.repeat(np.arange(len(sizes)), sizes)      # already sorted
    n = len(pkey)
    ref, _ = _check(P, pl, [_table(rng, pkey, np.zeros(n))], BY_PKEY, [],
                    EVERYTHING, device=[True])
    assert np.array_equal(ref[0], _rowid(n))
    rn = ref[1]
    assert rn[heads].tolist() == [1] * 5 and rn[CHUNK - 2] == CHUNK - 1


def test_peer_groups_straddle_the_chunk_boundaries(P, pl):
    """Peer groups of 37 rows: RANGE and PARTITION frames read across the
    boundary and LEAD reaches into the next chunk."""
    n = 3 * CHUNK + 1
    rng = np.random.default_rng(113)
    pkey = np.repeat([0, 1], [CHUNK - 100, n - (CHUNK - 100)])
    okey = _rowid(n) // 37
    assert (CHUNK - 1) // 37 == CHUNK // 37      # one group holds both rows
    funcs = RANKS + SUMS + [(W.LEAD, 3, 0, 15), (W.LAG, 3, 0, 15),
                            (W.LEAD, 7, 0, CHUNK), (W.LAG, 6, 0, CHUNK + 3)]
    _check(P, pl, [_table(rng, pkey, okey)], BY_PKEY, BY_OKEY, funcs)


def _skewed(rng, n):
    """Partition sizes from one row to about a third of the table."""
    return np.minimum(rng.zipf(1.4, n), 60)


def test_skewed_partitions_over_mixed_pages(P, pl):
    """Random order, four pages — host, device, device, host — of which
    only two carry masks, and one partition whose every value is null."""
    n = 3 * CHUNK - 50
    rng = np.random.default_rng(127)
    pkey = _skewed(rng, n)
    cols, masks = _table(rng, pkey, rng.integers(0, 9, n), null_parts=[2])
    # the rows masked on one page are plain values on a page without masks
    cols[3] = rng.integers(-2**40, 2**40, n)
    cuts = [0, 900, 900, 2000, n]       # 900 rows, an empty page, ...
    pages = []
    for i, (a, b) in enumerate(zip(cuts[:-1], cuts[1:])):
        m = {c: v[a:b] for c, v in masks.items()} if i in (0, 3) else {}
        pages.append(([c[a:b] for c in cols], m))
    ref, rmasks = _check(P, pl, pages, BY_PKEY, BY_OKEY, EVERYTHING,
                         emit=[0, 3], device=[False, True, True, False])
    assert 1 in rmasks      # the emitted value column carries its mask


# ---------------- keys ----------------

def test_null_nan_and_signed_zero_partition_keys(P, pl):
    n = CHUNK + 300
    rng = np.random.default_rng(131)
    pool = np.array([0x7ff8000000000000, 0xfff00000deadbeef,
                     0x8000000000000000, 0, 0x3ff8000000000000,
                     0xfff0000000000000], np.uint64).view(np.float64)
    cols, masks = _table(rng, np.zeros(n), rng.integers(0, 4, n))
    cols[6] = pool[rng.integers(0, len(pool), n)]
    null = (rng.random(n) < 0.2).astype(np.uint8)
    cols[6] = np.where(null == 1,
                       rng.integers(-2**63, 2**63 - 1, n).view(np.float64),
                       cols[6])
    masks[6] = null
    ref, _ = _check(P, pl, [(cols, masks)], [(6, ASC)], BY_OKEY,
                    MIXED + RANKS, emit=[0, 6])
    # -inf | -0.0 | +0.0 | 1.5 | the NaNs together | the nulls together
    assert int((ref[2] == 1).sum()) == 6


@pytest.mark.parametrize("p_order", R.ORDERS)
@pytest.mark.parametrize("o_order", [R.DESC_NULLS_FIRST, R.ASC_NULLS_LAST])
def test_desc_and_nulls_first_keys(P, pl, p_order, o_order):
    n = CHUNK + 130
    rng = np.random.default_rng(137)
    cols, masks = _table(rng, rng.integers(-3, 3, n), rng.integers(0, 5, n))
    masks[1] = (rng.random(n) < 0.15).astype(np.uint8)
    masks[2] = (rng.random(n) < 0.15).astype(np.uint8)
    _check(P, pl, [(cols, masks)], [(1, p_order)], [(2, o_order)], MIXED)


KEYS = [(5, R.DESC_NULLS_LAST), (2, R.ASC_NULLS_FIRST), (6, R.ASC_NULLS_LAST),
        (1, R.DESC_NULLS_FIRST)]     # u8, i32, f64, i64


@pytest.mark.parametrize("n_keys,n_part", [
    (k, p) for k in range(5) for p in range(k + 1)])
def test_zero_to_four_keys_with_zero_to_all_partition_keys(P, pl, n_keys,
                                                           n_part):
    n = CHUNK + 77
    rng = np.random.default_rng(139)
    cols, masks = _table(rng, rng.integers(0, 3, n), rng.integers(0, 3, n))
    cols[5] = rng.integers(0, 3, n).astype(np.uint8)
    cols[6] = rng.integers(0, 3, n).astype(np.float64) - 1.0
    keys = KEYS[:n_keys]
    funcs = [(W.ROW_NUMBER, None, 0, 0), (W.RANK, None, 0, 0),
             (W.DENSE_RANK, None, 0, 0), (W.SUM, 3, RANGE, 0),
             (W.COUNT, None, PART, 0), (W.LAG, 3, 0, 1)]
    _check(P, pl, [(cols, masks)], keys[:n_part], keys[n_part:], funcs)


# ---------------- SUM at the edge of int64 ----------------

def _sum_table(vals):
    vals = np.asarray(vals, np.int64)
    return [_rowid(len(vals)), vals], {}


def test_sum_near_the_ends_of_int64_that_fits(P, pl):
    """Running sums 2^63-1, -1, 2^63-2, -2, ... over two blocks."""
    n = CHUNK + 10
    vals = np.where(_rowid(n) % 2 == 0, 2**63 - 1, -2**63)
    ref, _ = _check(P, pl, [_sum_table(vals)], [], [(0, ASC)],
                    _frames(W.SUM, 1))
    assert ref[2][0] == 2**63 - 1 and ref[2][1] == -1
    low = np.where(_rowid(n) % 2 == 0, -(2**63 - 1), 2**63 - 1)
    low[0] = -2**63                 # then -1, -2^63, -1, ...
    ref, _ = _check(P, pl, [_sum_table(low)], [], [(0, ASC)],
                    [(W.SUM, 1, ROWS, 0)])
    assert ref[1][0] == -2**63


def test_sub_range_sums_beyond_64_bits_with_every_prefix_inside(P, pl):
    """-X, +X, +X, -X repeated (X = 2^63-1): the prefixes are -X, 0, X, 0
    while rows 1..2 alone sum to 2X — what a lane pair or a wave total
    holds inside the scan."""
    X = 2**63 - 1
    n = CHUNK + 10
    vals = np.array([-X, X, X, -X] * (n // 4 + 1), np.int64)[:n]
    ref, _ = _check(P, pl, [_sum_table(vals)], [], [(0, ASC)],
                    [(W.SUM, 1, ROWS, 0), (W.SUM, 1, RANGE, 0)])
    assert ref[1][:4].tolist() == [-X, 0, X, 0]


@pytest.mark.parametrize("frame,vals", [
    (ROWS, [2**63 - 1, 1, -1]),           # a prefix leaves, the total fits
    (RANGE, [-2**63, -1]),
    (PART, [2**62] * 3)])
def test_sum_overflow_fails_finish_naming_the_function(P, pl, frame, vals):
    page = _sum_table(vals)
    funcs = [(W.COUNT, None, 0, 0), (W.SUM, 1, frame, 0)]
    with pytest.raises(W.SumOverflow) as e:
        W.window(page[0], {}, [], [(0, ASC)], [0], funcs)
    assert e.value.func_index == 1
    with P.Scope() as s:
        op = s.op(P.OP_WINDOW, _plan(P, pl, [], [(0, ASC)], [0], funcs))
        keep, raw = _make_page(P, page[0], {}, False)
        op.add_input_raw(raw)
        with pytest.raises(RuntimeError,
                           match=r"WINDOW: funcs\[1\].*SUM.*int64"):
            op.finish()
        # no page comes out, and the operator stays failed
        assert op.get_output_raw() is None
        with pytest.raises(RuntimeError, match=r"funcs\[1\].*SUM"):
            op.finish()
        with pytest.raises(RuntimeError, match=r"funcs\[1\].*SUM"):
            op.add_input_raw(raw)


def test_partition_total_that_fits_over_an_overflowing_prefix(P, pl):
    """More lenient than the reference: only emitted values count."""
    _check(P, pl, [_sum_table([2**63 - 1, 1, -1])], [], [(0, ASC)],
           [(W.SUM, 1, PART, 0)])


# ---------------- composition ----------------

def test_top_three_per_partition_through_a_filter(P, pl):
    n = CHUNK + 200
    rng = np.random.default_rng(149)
    cols, masks = _table(rng, _skewed(rng, n), rng.integers(0, 50, n))
    funcs = [(W.ROW_NUMBER, None, 0, 0)]
    rcols, _ = W.window(cols, {}, BY_PKEY, [(2, DESC)], [0, 1, 2], funcs)
    keep = rcols[3] <= 3
    with P.Scope() as s:
        page, raw = _make_page(P, cols[:3], {}, True)
        w = s.run(P.OP_WINDOW,
                  _plan(P, pl, BY_PKEY, [(2, DESC)], [0, 1, 2], funcs), raw)
        f, out = s.pipe(P.OP_FILTER_PROJECT, pl.filter_project(
            [pl.ident(0), pl.ident(1), pl.ident(2), pl.ident(3)],
            preds=[pl.pred(3, P.CMP_LE, 3)]), w.get_output_raw())
        got = _read_raw(P, out)
    _assert_same(got, ([c[keep] for c in rcols], {}))
    assert 0 < keep.sum() < n


# ---------------- lifecycle ----------------

def test_lifecycle(P, pl):
    with P.Scope() as s:
        op = s.op(P.OP_WINDOW, pl.window([], [pl.asc(0)], [0],
                                         [pl.row_number(), pl.win_sum(0)]))
        assert op.needs_input() and not op.is_finished()
        assert op.get_output() is None
        op.add_input(P.Page({"k": np.array([3, 1, 2], np.int64)}))
        assert op.get_output() is None and op.needs_input()
        op.finish()
        assert not op.needs_input() and not op.is_finished()
        op.finish()                          # harmless
        out, nulls = op.get_output_nulls(["k", "rn", "sum"])
        assert out["k"].tolist() == [1, 2, 3]
        assert out["rn"].tolist() == [1, 2, 3]
        assert out["sum"].tolist() == [1, 3, 6]
        assert nulls["sum"].tolist() == [0, 0, 0] and sorted(nulls) == ["sum"]
        assert op.is_finished() and op.get_output() is None


def test_finish_without_rows_gives_a_typed_empty_page(P, pl):
    plan = pl.window([pl.asc(0)], [pl.desc(1)], [1, 0],
                     [pl.rank(), pl.win_count(), pl.win_sum(0),
                      pl.win_min(2), pl.lag(1), pl.lead(2)])
    empty = P.Page({"a": np.empty(0, np.int32), "b": np.empty(0, np.float64),
                    "c": np.empty(0, np.uint8)})
    with P.Scope() as s:
        op = s.run(P.OP_WINDOW, plan, empty)
        raw = op.get_output_raw()
        assert raw.n_rows == 0 and raw.n_cols == 8
        assert [raw.cols[i].tag for i in range(8)] == [
            T_F64, T_I32, T_I64, T_I64, T_I64, T_U8, T_F64, T_U8]
        # SUM, MIN, LAG and LEAD carry a mask even here
        assert [bool(raw.cols[i].null_mask) for i in range(8)] == [
            False, False, False, False, True, True, True, True]
        assert op.get_output_raw() is None and op.is_finished()
        # no page at all: nothing names the types, the columns are I64
        op = s.run(P.OP_WINDOW, plan)
        raw = op.get_output_raw()
        assert raw.n_rows == 0 and raw.n_cols == 8
        assert [raw.cols[i].tag for i in range(8)] == [T_I64] * 8


# ---------------- errors ----------------

def _raw_plan(P, n_keys=1, n_part=1, key_col=(0,), order=(1,), n_emit=1,
              emit=(0,), n_funcs=1, funcs=((0, -1, 0, 0),)):
    p = P.PlanWindow()
    p.n_keys, p.n_partition_keys = n_keys, n_part
    p.n_emit, p.n_funcs = n_emit, n_funcs
    for i, v in enumerate(key_col):
        p.key_col[i] = v
    for i, v in enumerate(order):
        p.order[i] = v
    for i, v in enumerate(emit):
        p.emit_cols[i] = v
    for i, (f, c, fr, off) in enumerate(funcs):
        p.funcs[i] = P.WinSpec(f, c, fr, 0, off)
    return p


@pytest.mark.parametrize("kw,field", [
    (dict(n_keys=-1, n_part=0), "n_keys"), (dict(n_keys=5), "n_keys"),
    (dict(n_part=2), "n_partition_keys"),
    (dict(n_part=-1), "n_partition_keys"),
    (dict(n_emit=0), "n_emit"), (dict(n_emit=17), "n_emit"),
    (dict(n_funcs=0), "n_funcs"), (dict(n_funcs=9), "n_funcs"),
    (dict(order=(4,)), r"order\[0\]"), (dict(order=(-1,)), r"order\[0\]"),
    (dict(n_keys=2, key_col=(0, 0), order=(1, 7)), r"order\[1\]"),
    (dict(key_col=(-1,)), r"key_col\[0\]"),
    (dict(n_emit=2, emit=(0, -3)), r"emit_cols\[1\]"),
    (dict(funcs=((9, 0, 0, 0),)), r"funcs\[0\]\.func"),
    (dict(funcs=((-1, 0, 0, 0),)), r"funcs\[0\]\.func"),
    (dict(n_funcs=2, funcs=((0, -1, 0, 0), (W.SUM, 0, 3, 0))),
     r"funcs\[1\]\.frame"),
    (dict(funcs=((W.COUNT, -1, -1, 0),)), r"funcs\[0\]\.frame"),
    (dict(funcs=((W.LAG, 0, 0, -1),)), r"funcs\[0\]\.offset"),
    (dict(funcs=((W.LEAD, 0, 0, -2**40),)), r"funcs\[0\]\.offset"),
    (dict(funcs=((W.SUM, -1, 0, 0),)), r"funcs\[0\]\.col"),
    (dict(funcs=((W.MIN, -1, 0, 0),)), r"funcs\[0\]\.col"),
    (dict(funcs=((W.MAX, -2, 0, 0),)), r"funcs\[0\]\.col"),
    (dict(n_funcs=2, funcs=((0, -1, 0, 0), (W.LAG, -1, 0, 1))),
     r"funcs\[1\]\.col"),
    (dict(funcs=((W.LEAD, -1, 0, 1),)), r"funcs\[0\]\.col"),
])
def test_create_rejects(P, kw, field):
    with pytest.raises(RuntimeError, match="WINDOW: " + field):
        P.Operator(P.OP_WINDOW, _raw_plan(P, **kw))


def test_create_ignores_what_a_function_does_not_read(P):
    """Ranks ignore col, frame and offset; LAG / LEAD ignore frame;
    COUNT takes any negative col as count(*)."""
    for f in [(W.RANK, -7, 99, -5), (W.LAG, 0, 99, 1), (W.COUNT, -9, 2, -1)]:
        P.Operator(P.OP_WINDOW, _raw_plan(P, funcs=(f,))).destroy()


def test_create_rejects_a_wrong_plan_size(P):
    L = P.lib()
    plan = _raw_plan(P)
    h = C.c_int64()
    assert L.c.pg_op_create(P.OP_WINDOW, C.byref(plan),
                            C.sizeof(plan) - 4, C.byref(h)) != 0
    assert "plan size" in L.err()


def test_add_input_rejects_and_leaves_the_operator_usable(P, pl):
    i64 = np.arange(4, dtype=np.int64)
    i32 = np.arange(4, dtype=np.int32)
    f64 = np.arange(4, dtype=np.float64)
    words = P.Varbin([b"a", b"b", b"c", b"d"])
    dct = P.DictVarbin([b"x", b"y"], [0, 1, 1, 0])
    wide = np.arange(8, dtype=np.uint64).reshape(4, 2)

    def rejects(plan, page, field, first=None):
        with P.Scope() as s:
            op = s.op(P.OP_WINDOW, plan)
            if first is not None:
                op.add_input(first)
            with pytest.raises(RuntimeError, match="WINDOW: " + field):
                op.feed(page)
            # the operator is as it was: it still works on what it has
            op.finish()
            assert op.get_output_raw().n_rows == \
                (0 if first is None else 4)

    def plan(part=(0,), order=(), emit=(0,), funcs=(pl.row_number(),)):
        return pl.window([pl.asc(c) for c in part],
                         [pl.asc(c) for c in order], list(emit), list(funcs))

    two = P.Page({"a": i64, "b": i32})
    # an index past the page's columns: key, emit column, argument
    rejects(plan(part=(2,)), two, r"key_col\[0\]")
    rejects(plan(order=(1, 3)), two, r"key_col\[2\]")
    rejects(plan(emit=(1, 5)), two, r"emit_cols\[1\]")
    rejects(plan(funcs=(pl.rank(), pl.win_sum(4))), two,
            r"funcs\[1\]\.col = 4")
    rejects(plan(funcs=(pl.lag(2),)), two, r"funcs\[0\]\.col = 2")
    rejects(plan(funcs=(pl.win_count(9),)), two, r"funcs\[0\]\.col = 9")
    # VARBIN and dictionary columns anywhere
    vb = P.Page({"a": i64, "w": words})
    dc = P.Page({"a": i64, "d": dct})
    rejects(plan(part=(0, 1)), vb, r"key_col\[1\]")
    rejects(plan(order=(1,)), dc, r"key_col\[1\]")
    rejects(plan(emit=(1,)), vb, r"emit_cols\[0\]")
    rejects(plan(emit=(0, 1)), dc, r"emit_cols\[1\]")
    rejects(plan(funcs=(pl.lead(1),)), vb, r"funcs\[0\]\.col.*VARBIN")
    rejects(plan(funcs=(pl.win_count(1),)), dc, r"funcs\[0\]\.col.*VARBIN")
    rejects(plan(funcs=(pl.win_min(1),)), vb, r"funcs\[0\]\.col.*VARBIN")
    # I128 keys; I128 and F64 under SUM / MIN / MAX
    _, raw = keep = _make_page(P, [i64, wide, f64], {}, False)
    rejects(plan(part=(1,)), raw, r"key_col\[0\].*I128")
    rejects(plan(funcs=(pl.win_sum(1),)), raw,
            r"funcs\[0\]\.col = 1.*I128.*SUM")
    rejects(plan(funcs=(pl.rank(), pl.win_min(2))), raw,
            r"funcs\[1\]\.col = 2.*F64.*MIN")
    rejects(plan(funcs=(pl.win_max(2, frame=pl.FRAME_PARTITION),)), raw,
            r"funcs\[0\]\.col = 2.*F64.*MAX")
    del keep
    # a type that differs from the first page's
    rejects(plan(emit=(1,)), P.Page({"a": i64, "b": i64}),
            r"emit_cols\[0\]", first=two)
    rejects(plan(), P.Page({"a": i32, "b": i32}), r"key_col\[0\]",
            first=two)
    rejects(plan(funcs=(pl.lag(1),)), P.Page({"a": i64, "b": f64}),
            r"funcs\[0\]\.col.*differs", first=two)


def test_add_input_rejects_more_rows_than_row_ids(P, pl):
    small = np.arange(4, dtype=np.int64)
    with P.Scope() as s:
        op = s.op(P.OP_WINDOW, pl.window([], [pl.asc(0)], [0],
                                         [pl.row_number()]))
        op.add_input(P.Page({"a": small}))
        page = P.Page({"a": small})
        raw = page.to_c()
        raw.n_rows = 2**31 - 4
        with pytest.raises(RuntimeError, match="WINDOW.*2\\^31-1"):
            op.add_input_raw(raw)
        op.finish()
        assert op.get_output(["a", "rn"])["rn"].tolist() == [1, 2, 3, 4]
