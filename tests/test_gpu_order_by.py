"""PG_OP_ORDER_BY on the GPU against the comparator sort of
order_by_refs.py.  Every comparison is exact (floats through their bit
patterns), every case emits a row-id column so that the order of ties —
the stability the header promises — is visible in the result.

Sizes follow the kernel's geometry (kernels.hip): a scatter block ranks
SORT_WINDOW = 256 rows per step, owns a chunk of at least
SORT_MIN_WINDOWS = 4 windows (1024 rows), and a pass launches at most
SORT_NB = 1024 blocks — so below 2^20 rows the chunk IS 1024 rows and
n / 1024 blocks run."""
import ctypes as C

import numpy as np
import pytest

import order_by_refs as R

pytestmark = pytest.mark.gpu

WINDOW = 256          # SORT_WINDOW
CHUNK = 4 * WINDOW    # SORT_MIN_WINDOWS * SORT_WINDOW

T_U8, T_I32, T_I64, T_F64, T_I128 = 0, 1, 2, 3, 5
_NP_OF_TAG = {T_U8: np.uint8, T_I32: np.int32, T_I64: np.int64,
              T_F64: np.float64}


@pytest.fixture(scope="module")
def P():
    import presto_amd
    return presto_amd


@pytest.fixture(scope="module")
def pl():
    from presto_amd import plans
    return plans


# ---------------- plumbing ----------------

def _is_i128(a):
    return a.ndim == 2


def _make_page(P, cols, masks, device):
    """cols: numpy columns ((n, 2) uint64 = I128); masks: {index: uint8}.
    Returns (keepalive, raw PgPage)."""
    import torch
    n = len(cols[0])
    named, nulls = {}, {}
    for i, a in enumerate(cols):
        a = np.ascontiguousarray(a)
        flat = a.view(np.int64).reshape(-1) if _is_i128(a) else a
        named[f"c{i}"] = torch.from_numpy(flat).cuda() if device else flat
        if i in masks:
            m = np.ascontiguousarray(masks[i], np.uint8)
            nulls[f"c{i}"] = torch.from_numpy(m).cuda() if device else m
    page = P.Page(named, n_rows=n, nulls=nulls)
    raw = page.to_c()
    for i, a in enumerate(cols):
        if _is_i128(np.asarray(a)):
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


def _sort(P, pl, pages, keys, emit, limit=0, device=None):
    """pages: [(cols, masks)].  device: per-page flags (default: page i is
    device-resident when i is odd).  Runs the whole lifecycle and returns
    (columns, masks) of the one output page."""
    with P.Scope() as s:
        op = s.op(P.OP_ORDER_BY, pl.order_by(keys, emit, limit))
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


def _assert_same(got, ref):
    gcols, gmasks = got
    rcols, rmasks = ref
    assert len(gcols) == len(rcols)
    for o, (g, r) in enumerate(zip(gcols, rcols)):
        r = np.asarray(r)
        assert g.dtype == r.dtype and g.shape == r.shape, o
        assert np.array_equal(_bits(g), _bits(r)), o
    assert sorted(gmasks) == sorted(rmasks)
    for o in rmasks:
        assert np.array_equal(gmasks[o], rmasks[o]), o


def _check(P, pl, pages, keys, emit, limit=0, device=None):
    cols, masks = R.concat_pages(pages)
    ref = R.order_by(cols, masks, keys, emit, limit)
    got = _sort(P, pl, pages, keys, emit, limit, device)
    _assert_same(got, ref)
    return got


def _rowid(n):
    return np.arange(n, dtype=np.int64)


# ---------------- data ----------------

def _f(bits):
    return np.array(bits, np.uint64).view(np.float64)


EDGES = {
    np.int64: np.array([-2**63, -1, 0, 1, 2**63 - 1], np.int64),
    np.int32: np.array([-2**31, -1, 0, 1, 2**31 - 1], np.int32),
    np.uint8: np.array([0, 127, 128, 255], np.uint8),
    np.float64: np.concatenate([
        np.array([np.inf, -np.inf, 0.0, -0.0, 5e-324, -5e-324, 1.5, -1.5,
                  1.7976931348623157e308, -1.7976931348623157e308]),
        _f([0x7ff8000000000000, 0xfff8000000000000, 0x7ff0000000000001,
            0xfff00000deadbeef, 0x7fffffffffffffff])]),
}
TYPES = [np.uint8, np.int32, np.int64, np.float64]
TYPE_IDS = ["u8", "i32", "i64", "f64"]


def _dups(rng, dtype, n):
    """Random values with heavy duplicates: ~n/8 distinct, spread over
    the type's whole range (negatives, both halves of every byte)."""
    k = max(2, n // 8)
    if dtype == np.uint8:
        pool = rng.integers(0, 256, k).astype(np.uint8)
    elif dtype == np.float64:
        pool = rng.integers(-2**63, 2**63 - 1, k).view(np.float64)
        pool = np.where(np.isnan(pool), 0.25, pool)
    else:
        info = np.iinfo(dtype)
        pool = rng.integers(info.min, info.max, k, endpoint=True) \
            .astype(dtype)
    return pool[rng.integers(0, k, n)] if n else pool[:0]


def _garbage(rng, dtype, n):
    """Arbitrary bit patterns: what sits under a null."""
    w = np.dtype(dtype).itemsize
    return rng.integers(0, 256, n * w).astype(np.uint8).view(dtype)


# ---------------- sizes ----------------

@pytest.mark.parametrize("n", [
    0, 1, 2, 63, 64, 65, 255, 256, 257,
    CHUNK - 1, CHUNK, CHUNK + 1,          # a whole chunk of windows -+ 1
    2 * CHUNK - 1, 2 * CHUNK + 1,
    70001])                               # 69 blocks, ragged last chunk
def test_sizes(P, pl, n):
    rng = np.random.default_rng(n)
    key = _dups(rng, np.int64, n)
    _check(P, pl, [([_rowid(n), key], {})],
           [(1, R.DESC_NULLS_LAST)], [0, 1], device=[True])


# ---------------- single key ----------------

@pytest.mark.parametrize("order", R.ORDERS)
@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
def test_single_key_duplicates_and_edges(P, pl, dtype, order):
    n = CHUNK + 300     # two blocks, the second one ragged
    rng = np.random.default_rng(7)
    key = np.concatenate([_dups(rng, dtype, n), EDGES[dtype],
                          EDGES[dtype][::-1]])
    key = key[rng.permutation(len(key))]
    _check(P, pl, [([_rowid(len(key)), key], {})], [(1, order)], [0, 1],
           device=[False])


@pytest.mark.parametrize("order", R.ORDERS)
@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
def test_all_rows_equal_is_the_identity(P, pl, dtype, order):
    """Every digit pass is skipped; the output is the input."""
    n = CHUNK + 77
    key = np.full(n, EDGES[dtype][1], dtype)
    got = _check(P, pl, [([_rowid(n), key], {})], [(1, order)], [0, 1])
    assert np.array_equal(got[0][0], _rowid(n))


@pytest.mark.parametrize("order", R.ORDERS)
@pytest.mark.parametrize("which", ["top", "bottom"])
@pytest.mark.parametrize("dtype", [np.int32, np.int64, np.float64],
                         ids=["i32", "i64", "f64"])
def test_keys_differing_in_one_byte(P, pl, dtype, which, order):
    """Only the top, or only the bottom, byte varies: pass skipping from
    both ends."""
    n = CHUNK + 130
    rng = np.random.default_rng(11)
    b = rng.integers(0, 256, n).astype(np.uint64)
    w = np.dtype(dtype).itemsize
    shift = 8 * (w - 1) if which == "top" else 0
    if dtype == np.float64:
        # top byte = sign + the exponent's high bits; the exponent's low
        # nibble stays 0 there, so no pattern is a NaN (which would be
        # canonicalised and change the other bytes)
        base = 0x0000edcba9876543 if which == "top" else 0x4035edcba9876543
    else:
        base = 0x00345678 if w == 4 else 0x0034567812345678
    bits = np.uint64(base & ~(0xff << shift)) | (b << np.uint64(shift))
    key = bits.astype(np.uint32).view(np.int32) if w == 4 \
        else bits.view(dtype)
    assert len(np.unique(key)) > 200
    _check(P, pl, [([_rowid(n), key], {})], [(1, order)], [0, 1])


# ---------------- nulls ----------------

@pytest.mark.parametrize("order", R.ORDERS)
@pytest.mark.parametrize("dtype", TYPES, ids=TYPE_IDS)
def test_nulls_with_garbage_underneath(P, pl, dtype, order):
    n = CHUNK + 211
    rng = np.random.default_rng(13)
    key = _dups(rng, dtype, n)
    mask = (rng.random(n) < 0.3).astype(np.uint8)
    key = np.where(mask == 1, _garbage(rng, dtype, n), key)
    got = _check(P, pl, [([_rowid(n), key], {1: mask})], [(1, order)],
                 [0, 1])
    # the nulls sit together at the end the order names, in input order
    k = int(mask.sum())
    nulls = got[1][1]
    block = nulls[-k:] if order in (R.ASC_NULLS_LAST,
                                    R.DESC_NULLS_LAST) else nulls[:k]
    assert block.all() and int(nulls.sum()) == k


@pytest.mark.parametrize("order", R.ORDERS)
def test_all_null_key_is_the_identity(P, pl, order):
    n = CHUNK + 5
    rng = np.random.default_rng(17)
    key = _garbage(rng, np.float64, n)
    got = _check(P, pl, [([_rowid(n), key], {1: np.ones(n, np.uint8)})],
                 [(1, order)], [0, 1])
    assert np.array_equal(got[0][0], _rowid(n))


@pytest.mark.parametrize("order", R.ORDERS)
def test_mask_on_one_of_three_pages(P, pl, order):
    rng = np.random.default_rng(19)
    sizes = [300, 500, 400]
    pages, base = [], 0
    for i, n in enumerate(sizes):
        key = _dups(rng, np.int32, n)
        masks = {}
        if i == 1:
            masks[1] = (rng.random(n) < 0.3).astype(np.uint8)
            key = np.where(masks[1] == 1, _garbage(rng, np.int32, n), key)
        pages.append(([_rowid(n) + base, key], masks))
        base += n
    got = _check(P, pl, pages, [(1, order)], [0, 1])
    assert 1 in got[1]      # the emitted key carries the gathered mask


# ---------------- several keys ----------------

def _mixed_cols(rng, n):
    """[rowid, u8 with 3 values, i32 dups, f64 dups, i64 dups]"""
    return [_rowid(n),
            rng.integers(0, 3, n).astype(np.uint8),
            _dups(rng, np.int32, n)[rng.integers(0, n, n)] % 7,
            _dups(rng, np.float64, n),
            rng.integers(-3, 3, n).astype(np.int64)]


@pytest.mark.parametrize("keys", [
    [(1, R.ASC_NULLS_LAST), (3, R.DESC_NULLS_LAST)],
    [(1, R.DESC_NULLS_FIRST), (2, R.ASC_NULLS_LAST), (4, R.DESC_NULLS_LAST)],
    [(4, R.ASC_NULLS_FIRST), (1, R.DESC_NULLS_LAST), (2, R.DESC_NULLS_FIRST),
     (3, R.ASC_NULLS_LAST)],
], ids=["2keys", "3keys", "4keys"])
def test_multi_key_mixed_types_and_directions(P, pl, keys):
    n = 2 * CHUNK + 45
    rng = np.random.default_rng(23)
    cols = _mixed_cols(rng, n)
    cols[2] = cols[2].astype(np.int32)
    _check(P, pl, [(cols, {})], keys, [0, 1, 2, 3, 4])


@pytest.mark.parametrize("masked", [1, 2, 3])
def test_multi_key_with_one_masked_key(P, pl, masked):
    n = CHUNK + 190
    rng = np.random.default_rng(29)
    cols = _mixed_cols(rng, n)
    cols[2] = cols[2].astype(np.int32)
    mask = (rng.random(n) < 0.3).astype(np.uint8)
    cols[masked] = np.where(mask == 1,
                            _garbage(rng, cols[masked].dtype, n),
                            cols[masked])
    keys = [(1, R.DESC_NULLS_FIRST), (2, R.ASC_NULLS_LAST),
            (3, R.DESC_NULLS_LAST)]
    _check(P, pl, [(cols, {masked: mask})], keys, [0, 1, 2, 3])


# ---------------- pages ----------------

@pytest.mark.parametrize("device", [[False, True, True, False],
                                    [True, False, False, True]],
                         ids=["hddh", "dhhd"])
def test_uneven_pages_equal_the_one_page_result(P, pl, device):
    rng = np.random.default_rng(31)
    n = CHUNK + 333
    key = _dups(rng, np.int64, n)
    pay = _dups(rng, np.float64, n)
    mask = (rng.random(n) < 0.2).astype(np.uint8)
    cuts = [0, 700, 700, 701, n]      # 700 rows, an empty page, 1 row, rest
    pages = [([_rowid(n)[a:b], key[a:b], pay[a:b]], {2: mask[a:b]})
             for a, b in zip(cuts[:-1], cuts[1:])]
    keys = [(1, R.DESC_NULLS_LAST)]
    many = _check(P, pl, pages, keys, [0, 1, 2], device=device)
    one = _sort(P, pl, [([_rowid(n), key, pay], {2: mask})], keys,
                [0, 1, 2], device=[True])
    _assert_same(many, one)


# ---------------- limit ----------------

@pytest.mark.parametrize("delta", ["one", "n-1", "n", "n+5", "cut"])
def test_limit_with_a_duplicate_key_at_the_cut(P, pl, delta):
    n = CHUNK + 60
    rng = np.random.default_rng(37)
    key = rng.integers(0, 5, n).astype(np.int32)   # ~n/5 rows per value
    limit = {"one": 1, "n-1": n - 1, "n": n, "n+5": n + 5,
             "cut": int((key == 0).sum()) + 3}[delta]
    got = _check(P, pl, [([_rowid(n), key], {})],
                 [(1, R.ASC_NULLS_LAST)], [0, 1], limit=limit)
    assert len(got[0][0]) == min(limit, n)
    if delta == "cut":      # stability decides which key-1 rows survive
        assert np.array_equal(got[0][0][-3:], np.flatnonzero(key == 1)[:3])


# ---------------- emit ----------------

def test_emit_i128_u8_twice_and_unemitted_key(P, pl):
    n = CHUNK + 99
    rng = np.random.default_rng(41)
    cols = [_rowid(n),
            _dups(rng, np.float64, n),                              # key
            rng.integers(0, 2**63, (n, 2)).astype(np.uint64),       # I128
            rng.integers(0, 256, n).astype(np.uint8),
            _dups(rng, np.int32, n)]                                # masked
    mask = (rng.random(n) < 0.4).astype(np.uint8)
    got = _check(P, pl, [(cols, {4: mask})], [(1, R.DESC_NULLS_LAST)],
                 [0, 2, 3, 4, 2, 3])      # the key itself is not emitted
    assert sorted(got[1]) == [3]          # only the masked column's mask
    assert np.array_equal(got[0][1], got[0][4])


def test_no_mask_anywhere_gives_null_masks(P, pl):
    n = 300
    rng = np.random.default_rng(43)
    cols = [_rowid(n), _dups(rng, np.int64, n), _dups(rng, np.uint8, n)]
    got = _check(P, pl, [(cols, {})], [(2, R.ASC_NULLS_FIRST),
                                       (1, R.DESC_NULLS_LAST)], [0, 1, 2])
    assert got[1] == {}


# ---------------- chaining ----------------

def test_output_feeds_a_filter_with_is_not_null(P, pl):
    n = CHUNK + 17
    rng = np.random.default_rng(47)
    cols = [_rowid(n), _dups(rng, np.int64, n), _dups(rng, np.int32, n)]
    mask = (rng.random(n) < 0.3).astype(np.uint8)
    keys = [(1, R.DESC_NULLS_LAST)]
    ref_cols, ref_masks = R.order_by(cols, {2: mask}, keys, [0, 1, 2])
    keep = ref_masks[2] == 0
    with P.Scope() as s:
        page, raw = _make_page(P, cols, {2: mask}, True)
        ob = s.run(P.OP_ORDER_BY, pl.order_by(keys, [0, 1, 2]), raw)
        sorted_raw = ob.get_output_raw()
        f, out = s.pipe(P.OP_FILTER_PROJECT, pl.filter_project(
            [pl.ident(0), pl.ident(1), pl.ident(2)],
            preds=[pl.pred_not_null(2)]), sorted_raw)
        got = _read_raw(P, out)
    _assert_same(got, ([c[keep] for c in ref_cols], {}))


# ---------------- lifecycle ----------------

def test_lifecycle(P, pl):
    with P.Scope() as s:
        op = s.op(P.OP_ORDER_BY, pl.order_by([pl.asc(0)], [0]))
        assert op.needs_input() and not op.is_finished()
        assert op.get_output() is None
        op.add_input(P.Page({"k": np.array([3, 1, 2], np.int64)}))
        assert op.get_output() is None and op.needs_input()
        op.finish()
        assert not op.needs_input()
        assert not op.is_finished()          # the page is still queued
        op.finish()                          # harmless
        out = op.get_output(["k"])
        assert out["k"].tolist() == [1, 2, 3]
        assert op.is_finished()
        assert op.get_output() is None
        op.finish()
        assert op.get_output() is None and op.is_finished()


def test_finish_without_rows_gives_a_typed_empty_page(P, pl):
    plan = pl.order_by([pl.desc(1)], [1, 0, 2])
    empty = P.Page({"a": np.empty(0, np.int32), "b": np.empty(0, np.float64),
                    "c": np.empty(0, np.uint8)})
    with P.Scope() as s:
        op = s.run(P.OP_ORDER_BY, plan, empty)
        raw = op.get_output_raw()
        assert raw.n_rows == 0 and raw.n_cols == 3
        assert [raw.cols[i].tag for i in range(3)] == [T_F64, T_I32, T_U8]
        assert op.get_output_raw() is None and op.is_finished()
        # no page at all: nothing names the types, the columns are I64
        op = s.run(P.OP_ORDER_BY, plan)
        raw = op.get_output_raw()
        assert raw.n_rows == 0 and raw.n_cols == 3
        assert [raw.cols[i].tag for i in range(3)] == [T_I64] * 3
        assert op.get_output_raw() is None and op.is_finished()


# ---------------- errors ----------------

def _plan(P, n_keys=1, key_col=(0,), order=(1,), n_emit=1, emit=(0,),
          limit=0):
    p = P.PlanOrderBy()
    p.n_keys, p.n_emit, p.limit = n_keys, n_emit, limit
    for i, v in enumerate(key_col):
        p.key_col[i] = v
    for i, v in enumerate(order):
        p.order[i] = v
    for i, v in enumerate(emit):
        p.emit_cols[i] = v
    return p


@pytest.mark.parametrize("kw,field", [
    (dict(n_keys=0), "n_keys"), (dict(n_keys=5), "n_keys"),
    (dict(n_emit=0), "n_emit"), (dict(n_emit=17), "n_emit"),
    (dict(order=(4,)), r"order\[0\]"), (dict(order=(-1,)), r"order\[0\]"),
    (dict(n_keys=2, key_col=(0, 0), order=(1, 7)), r"order\[1\]"),
    (dict(limit=-1), "limit"),
    (dict(key_col=(-1,)), r"key_col\[0\]"),
    (dict(n_emit=2, emit=(0, -3)), r"emit_cols\[1\]"),
])
def test_create_rejects(P, kw, field):
    with pytest.raises(RuntimeError, match=field):
        P.Operator(P.OP_ORDER_BY, _plan(P, **kw))


def test_create_rejects_a_wrong_plan_size(P):
    L = P.lib()
    plan = _plan(P)
    h = C.c_int64()
    assert L.c.pg_op_create(P.OP_ORDER_BY, C.byref(plan),
                            C.sizeof(plan) - 4, C.byref(h)) != 0
    assert "plan size" in L.err()


def test_add_input_rejects(P, pl):
    i64 = np.arange(4, dtype=np.int64)
    i32 = np.arange(4, dtype=np.int32)
    words = P.Varbin([b"a", b"b", b"c", b"d"])
    dct = P.DictVarbin([b"x", b"y"], [0, 1, 1, 0])
    wide = np.arange(8, dtype=np.uint64).reshape(4, 2)

    def rejects(plan, page, field, first=None):
        with P.Scope() as s:
            op = s.op(P.OP_ORDER_BY, plan)
            if first is not None:
                op.add_input(first)
            with pytest.raises(RuntimeError, match=field):
                op.feed(page)
            # the operator is as it was: it still sorts what it has
            op.finish()
            assert op.get_output_raw().n_rows == \
                (0 if first is None else 4)

    two = P.Page({"a": i64, "b": i32})
    rejects(pl.order_by([pl.asc(2)], [0]), two, r"key_col\[0\]")
    rejects(pl.order_by([pl.asc(0)], [1, 5]), two, r"emit_cols\[1\]")
    rejects(pl.order_by([pl.asc(0), pl.asc(1)], [0]),
            P.Page({"a": i64, "w": words}), r"key_col\[1\]")
    rejects(pl.order_by([pl.asc(0)], [1]),
            P.Page({"a": i64, "w": words}), r"emit_cols\[0\]")
    rejects(pl.order_by([pl.asc(1)], [0]),
            P.Page({"a": i64, "d": dct}), r"key_col\[0\]")
    rejects(pl.order_by([pl.asc(0)], [0, 1]),
            P.Page({"a": i64, "d": dct}), r"emit_cols\[1\]")
    _, raw = keep = _make_page(P, [i64, wide], {}, False)
    rejects(pl.order_by([pl.asc(1)], [0]), raw, r"key_col\[0\].*I128")
    del keep
    # a type that differs from the first page's
    rejects(pl.order_by([pl.asc(0)], [1]),
            P.Page({"a": i64, "b": i64}), r"emit_cols\[0\]", first=two)
    rejects(pl.order_by([pl.asc(0)], [1]),
            P.Page({"a": i32, "b": i32}), r"key_col\[0\]", first=two)


def test_add_input_rejects_more_rows_than_row_ids(P, pl):
    """Row ids are 32-bit.  The count is checked before anything is
    copied, so the page only has to CLAIM its rows."""
    small = np.arange(4, dtype=np.int64)
    with P.Scope() as s:
        op = s.op(P.OP_ORDER_BY, pl.order_by([pl.asc(0)], [0]))
        op.add_input(P.Page({"a": small}))
        page = P.Page({"a": small})
        raw = page.to_c()
        raw.n_rows = 2**31 - 4
        with pytest.raises(RuntimeError, match="2\\^31-1"):
            op.add_input_raw(raw)
        op.finish()
        assert op.get_output(["a"])["a"].tolist() == [0, 1, 2, 3]
