"""PG_OP_MARK_DISTINCT on the GPU against mark_distinct_refs.py.  Every
comparison is exact.

Sizes follow the new kernels' geometry (kernels.hip): the insert and mark
kernels run min(ceil(n / 256), 4096) blocks of 256 threads with a grid
stride, so 2^20 + 1 rows is the smallest page whose last row is the second
row of a thread (row 0's), and at 2^21 rows every thread takes two; the
only-mode compaction ballots 64-row waves inside 256-row windows.  Pages
alternate between host- and device-resident, page 0 on the host.

Every case is built on the CPU first, and a CPU-side assertion checks that
it contains what it is meant to contain before anything runs.  At 2^20
rows and more the reference is numpy's first-occurrence index
(np.unique(..., return_index=True)); on the small cases that shortcut is
itself checked against the row-at-a-time reference."""
import ctypes as C
import functools

import numpy as np
import pytest

import mark_distinct_refs as M

pytestmark = pytest.mark.gpu

T_U8, T_I32, T_I64, T_F64, T_VARBIN, T_I128 = 0, 1, 2, 3, 4, 5
_NP_OF_TAG = {T_U8: np.uint8, T_I32: np.int32, T_I64: np.int64,
              T_F64: np.float64}
I64_MIN, I64_MAX = np.iinfo(np.int64).min, np.iinfo(np.int64).max
DICT = [b"key-%02d" % i for i in range(40)]     # distinct entries

GRID, BLOCK, WAVE = 4096, 256, 64               # the insert kernel's
TWO_PASS = GRID * BLOCK                         # row 0's thread: 2nd row
SPLITS = (0, 1000, 2049, 3000)      # three pages, none a multiple of 256


@pytest.fixture(scope="module")
def P():
    import presto_amd
    return presto_amd


@pytest.fixture(scope="module")
def pl():
    from presto_amd import plans
    return plans


# ---------------- references ----------------

def np_markers(keys, key_masks):
    """First-occurrence markers through np.unique: a null key is its mask
    bit over a zeroed value."""
    cols = []
    for k, m in zip(keys, key_masks):
        k = np.asarray(k).astype(np.int64)
        if m is not None:
            k = np.where(m != 0, 0, k)
            cols.append(m.astype(np.int64))
        cols.append(k)
    if len(cols) == 1:
        _, idx = np.unique(cols[0], return_index=True)
    else:
        _, idx = np.unique(np.stack(cols, 1), axis=0, return_index=True)
    out = np.zeros(len(keys[0]), np.uint8)
    out[idx] = 1
    return out


class Case:
    """keys: one array per key channel (int32 dictionary ids where kinds
    says "dict"); key_masks: a uint8 array or None per channel;
    mask_pages: {channel: pages that pass the mask} (default: all);
    extras: the non-key columns as (array, mask or None), an (n, 2) uint64
    array being I128.  Page columns: the keys, then the extras."""

    def __init__(self, kinds, keys, key_masks, extras=(), splits=SPLITS,
                 mask_pages=None, capacity=None):
        self.kinds, self.keys, self.key_masks = kinds, keys, key_masks
        self.extras, self.splits = list(extras), splits
        self.mask_pages = mask_pages or {}
        self.n = len(keys[0])
        assert splits[0] == 0 and splits[-1] == self.n
        self._capacity = capacity

    @functools.cached_property
    def expected(self):
        got = np_markers(self.keys, self.key_masks)
        if self.n <= 10000:     # the shortcut against the plain reference
            assert got.tolist() == M.markers(self.keys, self.key_masks)
        return got

    @property
    def capacity(self):
        return self._capacity or int(self.expected.sum())

    def columns(self):
        """[(array, mask or None, is_dict)] in page order."""
        out = [(k, m, kind == "dict") for k, m, kind in
               zip(self.keys, self.key_masks, self.kinds)]
        return out + [(a, m, False) for a, m in self.extras]


def _is_i128(a):
    return a.ndim == 2


def _page(P, case, p, device):
    """Page p of the case -> (keepalive, raw PgPage)."""
    import torch
    lo, hi = case.splits[p], case.splits[p + 1]
    named, nulls, wide = {}, {}, []
    for i, (a, m, is_dict) in enumerate(case.columns()):
        a = np.ascontiguousarray(a[lo:hi])
        if is_dict:
            a = P.DictVarbin(DICT, a)
            named[f"c{i}"] = P.DeviceVarbin.from_host(a) if device else a
        else:
            if _is_i128(a):
                wide.append(i)
                a = a.view(np.int64).reshape(-1)
            named[f"c{i}"] = torch.from_numpy(a).cuda() if device else a
        if m is not None and p in case.mask_pages.get(
                i, range(len(case.splits))):
            m = np.ascontiguousarray(m[lo:hi], np.uint8)
            nulls[f"c{i}"] = torch.from_numpy(m).cuda() if device else m
        elif m is not None:
            assert not m[lo:hi].any()   # a page without the mask: no nulls
    page = P.Page(named, n_rows=hi - lo, nulls=nulls)
    raw = page.to_c()
    for i in wide:
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


def _bits(a):
    a = np.asarray(a)
    return a.view(np.uint64) if a.dtype == np.float64 else a


def _expect_emit(case, emit, rows):
    """The emit columns of the global rows `rows`, and their masks."""
    table = case.columns()
    cols, masks = [], {}
    for o, c in enumerate(emit):
        a, m, _ = table[c]
        cols.append(a[rows])
        if m is not None:
            masks[o] = m[rows]
    return cols, masks


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


def _has_mask(case, c, p):
    m = case.columns()[c][1]
    return m is not None and p in case.mask_pages.get(
        c, range(len(case.splits)))


def run_mark(P, pl, case, emit, capacity=None, splits=None):
    """Mark mode over the case's pages: every page's emit columns are
    checked bit for bit; returns the concatenated marker column."""
    if splits is not None:
        case = Case(case.kinds, case.keys, case.key_masks, case.extras,
                    splits, case.mask_pages)
    nk = len(case.keys)
    plan = pl.mark_distinct(range(nk), emit, capacity or case.capacity)
    marks = []
    with P.Scope() as s:
        op = s.op(P.OP_MARK_DISTINCT, plan)
        assert op.get_output_raw() is None
        for p in range(len(case.splits) - 1):
            keep, raw = _page(P, case, p, p % 2 == 1)
            assert op.needs_input()
            op.add_input_raw(raw)
            del keep
            out = op.get_output_raw()
            assert out is not None and op.get_output_raw() is None
            lo, hi = case.splits[p], case.splits[p + 1]
            assert out.n_rows == hi - lo and out.n_cols == len(emit) + 1
            cols, masks = _read_raw(P, out)
            mk = out.cols[len(emit)]
            assert mk.tag == T_U8 and not mk.null_mask
            marks.append(cols.pop())
            rows = np.arange(lo, hi)
            rcols, rmasks = _expect_emit(case, emit, rows)
            rmasks = {o: m for o, m in rmasks.items()
                      if _has_mask(case, emit[o], p)}
            _assert_same((cols, masks), (rcols, rmasks))
        op.finish()
        assert op.get_output_raw() is None and op.is_finished()
    got = np.concatenate(marks)
    assert set(np.unique(got).tolist()) <= {0, 1}
    return got


def run_only(P, pl, case, emit, limit=0, capacity=None):
    """Only mode: every page fed is checked against the reference rows, in
    order; with a limit the feed stops where the operator stops taking
    input.  Returns the global row ids emitted."""
    nk = len(case.keys)
    plan = pl.distinct(range(nk), emit, capacity or case.capacity, limit)
    exp_pages = M.distinct_pages(case.keys, case.key_masks, case.splits,
                                 limit)
    # the reference stops feeding at the page that reaches the limit
    stops = limit > 0 and sum(map(len, exp_pages)) == limit
    assert stops or len(exp_pages) == len(case.splits) - 1
    emitted = []
    with P.Scope() as s:
        op = s.op(P.OP_MARK_DISTINCT, plan)
        for p, rows in enumerate(exp_pages):
            keep, raw = _page(P, case, p, p % 2 == 1)
            assert op.needs_input()
            op.add_input_raw(raw)
            out = op.get_output_raw()
            assert out is not None and op.get_output_raw() is None
            assert out.n_cols == len(emit)
            rows = np.asarray(rows, np.int64)
            assert out.n_rows == len(rows)
            rcols, rmasks = _expect_emit(case, emit, rows)
            rmasks = {o: m for o, m in rmasks.items()
                      if _has_mask(case, emit[o], p)}
            _assert_same(_read_raw(P, out), (rcols, rmasks))
            emitted += rows.tolist()
            if stops and p == len(exp_pages) - 1:
                # the limit is reached: the operator has finished itself
                assert not op.needs_input()
                with pytest.raises(RuntimeError, match="after finish"):
                    op.add_input_raw(raw)
            del keep
        assert op.needs_input() != stops
        op.finish()
        assert op.get_output_raw() is None and op.is_finished()
    return emitted


# ---------------- cases (CPU only) ----------------

_GARBAGE = {"u8": (0, 256), "i32": (-2**31, 2**31), "i64": (-2**62, 2**62),
            "dict": (0, len(DICT))}
_DTYPE = {"u8": np.uint8, "i32": np.int32, "i64": np.int64, "dict": np.int32}


def _rowid(n):
    return np.arange(n, dtype=np.int64)


def _key_channel(rng, n, kind, domain, frac=0.1):
    """Values 0..domain-1 (the real key 0 included), ~frac nulls, and under
    the nulls garbage that differs from row to row."""
    k = rng.integers(0, domain, n)
    m = (rng.random(n) < frac).astype(np.uint8)
    lo, hi = _GARBAGE[kind]
    k = np.where(m == 1, rng.integers(lo, hi, n), k).astype(_DTYPE[kind])
    assert (k[m == 0] == 0).any() and len(np.unique(k[m == 1])) > 1
    return k, m


N_SETS = 300


@functools.lru_cache(maxsize=None)
def dup_case():
    """2^21 rows of unique keys, then duplicate sets planted at every
    distance the insert kernel knows.  `sets` lists (first row, later
    rows)."""
    n = 2 * TWO_PASS
    key = np.arange(n, dtype=np.int64) * 2 + 1
    sets = [(0, [TWO_PASS])]        # row 0 and its thread's second row
    for s in range(N_SETS):
        w = 8 * s * BLOCK           # windows 8s+1 .. 8s+4 hold first rows
        a = w + 1 * BLOCK + 3       # one wave
        sets.append((a, [a + 17, a + 40]))
        a = w + 2 * BLOCK + 5       # two and three waves of one block
        sets.append((a, [a + WAVE, a + 3 * WAVE]))
        a = w + 3 * BLOCK + 7       # other blocks
        sets.append((a, [a + BLOCK, a + 50 * BLOCK]))
        a = w + 4 * BLOCK + 9       # the same thread's second row
        sets.append((a, [a + TWO_PASS]))
    for s in range(N_SETS + 100):
        # INVERTED in time: the later row is a SECOND row of a block that
        # is resident from the start, the first row belongs to a block
        # that can only start once a thousand others have retired
        first = (3072 + 2 * s) * BLOCK + 13
        later = TWO_PASS + 2 * s * WAVE + 11
        sets.append((first, [later]))
    for first, later in sets:
        key[later] = key[first]
    return Case(("i64",), [key], [None], [(_rowid(n), None)], (0, n)), sets


def _covered_dups(case, sets):
    rows = [r for first, later in sets for r in [first] + later]
    assert len(set(rows)) == len(rows)          # no set touches another
    exp = case.expected
    kinds = dict(wave=0, block=0, grid=0, thread=0, inverted=0)
    for first, later in sets:
        assert exp[first] == 1 and not exp[later].any()
        assert all(r > first for r in later)
        for r in later:
            if r // WAVE == first // WAVE:
                kinds["wave"] += 1
            elif r // BLOCK == first // BLOCK:
                kinds["block"] += 1
            elif r - first == TWO_PASS:
                kinds["thread"] += 1
            elif r >= TWO_PASS and (r - TWO_PASS) // BLOCK < 1024 and \
                    first // BLOCK >= 3072:
                kinds["inverted"] += 1
            elif r < TWO_PASS:
                kinds["grid"] += 1
    assert all(v >= N_SETS for v in kinds.values()), kinds
    assert exp[0] == 1 and exp[TWO_PASS] == 0
    # the sets sit in different waves
    assert len({first // WAVE for first, _ in sets}) == len(sets)
    assert int(exp.sum()) == case.n - sum(len(x) for _, x in sets)


@functools.lru_cache(maxsize=None)
def pages_case():
    """Page 0 holds most keys; they recur in pages 1 and 2, which also
    bring new ones."""
    rng = np.random.default_rng(3)
    n = SPLITS[-1]
    key = rng.integers(-200, 200, n).astype(np.int64)
    return Case(("i64",), [key], [None], [(_rowid(n), None)])


KEY_KINDS = [("u8",), ("i32",), ("i64",), ("dict",), ("u8", "i64"),
             ("i32", "dict"), ("i64", "i32", "u8"),
             ("dict", "i64", "u8", "i32")]


@functools.lru_cache(maxsize=None)
def key_case(kinds):
    rng = np.random.default_rng(len(kinds) * 100 + sum(map(ord, kinds[0])))
    n = SPLITS[-1]
    chans = [_key_channel(rng, n, kind, 3) for kind in kinds]
    return Case(kinds, [k for k, _ in chans], [m for _, m in chans],
                [(_rowid(n), None)])


@functools.lru_cache(maxsize=None)
def extreme_case():
    rng = np.random.default_rng(7)
    n = SPLITS[-1]
    vals = np.array([I64_MIN, I64_MIN + 1, -1, 0, 1, I64_MAX - 1, I64_MAX,
                     -2**32, 2**32, 2**31, -2**31], np.int64)
    key = vals[rng.integers(0, len(vals), n)]
    m = (rng.random(n) < 0.1).astype(np.uint8)
    key[m == 1] = rng.integers(-2**62, 2**62, int(m.sum()))
    return Case(("i64",), [key], [m], [(_rowid(n), None)]), vals


@functools.lru_cache(maxsize=None)
def one_page_mask_case():
    """Nulls in page 1 only, and only page 1 passes a mask."""
    rng = np.random.default_rng(13)
    n = SPLITS[-1]
    key = rng.integers(0, 6, n).astype(np.int64)
    m = np.zeros(n, np.uint8)
    lo, hi = SPLITS[1], SPLITS[2]
    m[lo:hi] = rng.random(hi - lo) < 0.2
    key[m == 1] = rng.integers(-2**62, 2**62, int(m.sum()))
    return Case(("i64",), [key], [m], [(_rowid(n), None)],
                mask_pages={0: (1,)})


@functools.lru_cache(maxsize=None)
def four_combinations_case():
    """(null,1) (0,1) (null,null) (0,null) and nothing else, over garbage."""
    rng = np.random.default_rng(19)
    n = SPLITS[-1]
    am = rng.integers(0, 2, n).astype(np.uint8)
    bm = rng.integers(0, 2, n).astype(np.uint8)
    a = np.where(am == 1, rng.integers(-2**62, 2**62, n), 0).astype(np.int64)
    b = np.where(bm == 1, rng.integers(-2**31, 2**31, n), 1).astype(np.int32)
    return Case(("i64", "i32"), [a, b], [am, bm], [(_rowid(n), None)])


@functools.lru_cache(maxsize=None)
def all_null_case():
    rng = np.random.default_rng(23)
    n = SPLITS[-1]
    key = rng.integers(-2**62, 2**62, n).astype(np.int64)
    assert len(np.unique(key)) == n
    return Case(("i64",), [key], [np.ones(n, np.uint8)],
                [(_rowid(n), None)])


EDGE_ROWS = (255, 256, 999, 1000, 1500, 1501, 1777, 2048, 2049)


@functools.lru_cache(maxsize=None)
def only_case():
    """Few keys, plus a new key at the rows on both sides of a 256-row
    window edge (255 | 256) and of the page edges (999 | 1000 and
    2048 | 2049), and at three rows inside page 1 for a limit to cut
    between."""
    rng = np.random.default_rng(29)
    n = SPLITS[-1]
    key, m = _key_channel(rng, n, "i64", 40, 0.05)
    for r in EDGE_ROWS:
        key[r], m[r] = 1000 + r, 0
    v = rng.integers(-1000, 1000, n).astype(np.int32)
    vm = (rng.random(n) < 0.3).astype(np.uint8)
    return Case(("i64",), [key], [m], [(_rowid(n), None), (v, vm)])


@functools.lru_cache(maxsize=None)
def emit_case(with_masks):
    rng = np.random.default_rng(31)
    n = SPLITS[-1]
    key, km = _key_channel(rng, n, "i32", 300, 0.05)
    wide = rng.integers(0, 2**63, (n, 2)).astype(np.uint64)
    small = rng.integers(0, 256, n).astype(np.uint8)
    f = rng.standard_normal(n)
    f[::7] = np.nan
    f[1::7] = -0.0
    masks = [(rng.random(n) < 0.3).astype(np.uint8) for _ in range(3)]
    if not with_masks:
        km, masks = None, [None] * 3
    return Case(("i32",), [key], [km],
                [(_rowid(n), None), (wide, masks[0]), (small, masks[1]),
                 (f, masks[2])], capacity=400)


EMIT = [2, 3, 3, 1, 4]      # I128, U8 twice, row id, F64; the key is not


@functools.lru_cache(maxsize=None)
def count_distinct_case():
    rng = np.random.default_rng(37)
    n = SPLITS[-1]
    g = rng.integers(0, 12, n).astype(np.int32)
    x, xm = _key_channel(rng, n, "i64", 30, 0.1)
    y = rng.integers(-10**6, 10**6, n).astype(np.int64)
    return Case(("i32", "i64"), [g, x], [None, xm], [(y, None)])


# ---------------- the tests ----------------

def test_duplicates_at_every_distance(P, pl):
    """The same key twice in one wave, in two waves of a block, in two
    blocks, in the two rows of one thread (row 0 and row 2^20 among them),
    and INVERTED: the later row is the second row of a block that starts
    at once, the first row belongs to a block that starts late.  The
    emitted row ids tell WHICH row was marked.  An implementation that
    marks whoever wins the slot's claim marks the later row of the
    inverted sets, four hundred of them, each in a wave of its own (a
    build that did so failed here on 729 of the 1601 sets, sets inside one
    block among them)."""
    case, sets = dup_case()
    _covered_dups(case, sets)
    got = run_mark(P, pl, case, [1])
    exp = case.expected
    wrong = np.flatnonzero(got != exp)
    assert len(wrong) == 0, (len(wrong), wrong[:10].tolist())
    for first, later in sets:
        assert got[first] == 1 and not got[later].any()


@functools.lru_cache(maxsize=None)
def equal_case():
    n = TWO_PASS + 1
    return Case(("i64",), [np.full(n, -5, np.int64)], [None],
                [(_rowid(n), None)], (0, n))


@functools.lru_cache(maxsize=None)
def distinct_case():
    n = TWO_PASS + 1
    rng = np.random.default_rng(43)
    key = rng.permutation(n).astype(np.int64) - n // 2
    return Case(("i64",), [key], [None], [(_rowid(n), None)], (0, n))


def test_all_rows_equal(P, pl):
    """2^20 + 1 equal rows: every thread lowers one word; one marker, on
    row 0."""
    case = equal_case()
    assert case.expected.sum() == 1 and case.expected[0] == 1
    got = run_mark(P, pl, case, [1])
    assert np.flatnonzero(got).tolist() == [0]


def test_all_rows_distinct_at_exact_capacity(P, pl):
    case = distinct_case()
    assert case.expected.all() and case.capacity == case.n
    got = run_mark(P, pl, case, [1], capacity=case.n)
    assert got.all()


def test_across_pages(P, pl):
    case = pages_case()
    key, exp = case.keys[0], case.expected
    p0 = set(key[:SPLITS[1]].tolist())
    for lo, hi in zip(SPLITS[1:], SPLITS[2:]):
        page = key[lo:hi]
        recur = np.isin(page, list(p0))
        assert recur.sum() > 100 and not exp[lo:hi][recur].any()
        assert exp[lo:hi].sum() > 0         # and the page brings new keys
    got = run_mark(P, pl, case, [1, 0])
    assert np.array_equal(got, exp)
    one = run_mark(P, pl, case, [1, 0], splits=(0, case.n))
    assert np.array_equal(one, got)


@pytest.mark.parametrize("kinds", KEY_KINDS, ids="-".join)
def test_key_types_and_nulls(P, pl, kinds):
    """1..4 keys of mixed type; each channel has nulls over garbage that
    differs from row to row, and the real key 0 next to them."""
    case = key_case(kinds)
    tuples = set(M.key_tuples(case.keys, case.key_masks))
    nk = len(kinds)
    for ch in range(nk):
        assert any(t[ch] is None for t in tuples)
        assert any(t[ch] == 0 for t in tuples)
    assert len(tuples) == case.expected.sum()
    if nk <= 2:                 # every combination of {null, 0, 1, 2}
        assert len(tuples) == 4 ** nk
        assert nk == 1 or {(None, None), (None, 0), (0, None), (0, 0)} \
            <= tuples
    got = run_mark(P, pl, case, [nk])
    assert np.array_equal(got, case.expected)


def test_extreme_i64_keys(P, pl):
    case, vals = extreme_case()
    tuples = set(M.key_tuples(case.keys, case.key_masks))
    assert tuples == {(int(v),) for v in vals} | {(None,)}
    got = run_mark(P, pl, case, [1])
    assert np.array_equal(got, case.expected)
    assert got.sum() == len(vals) + 1


def test_mask_on_one_page_only(P, pl):
    case = one_page_mask_case()
    exp = case.expected
    nulls = np.flatnonzero(case.key_masks[0])
    assert len(nulls) > 50 and exp[nulls[0]] == 1 and exp[nulls].sum() == 1
    assert exp.sum() == 7
    got = run_mark(P, pl, case, [1])
    assert np.array_equal(got, exp)


def test_four_null_combinations(P, pl):
    case = four_combinations_case()
    assert set(M.key_tuples(case.keys, case.key_masks)) == {
        (None, 1), (0, 1), (None, None), (0, None)}
    got = run_mark(P, pl, case, [2])
    assert np.array_equal(got, case.expected) and got.sum() == 4


def test_all_null_key_column(P, pl):
    case = all_null_case()
    got = run_mark(P, pl, case, [1])
    assert np.flatnonzero(got).tolist() == [0]


def _only_limits():
    case = only_case()
    pages = M.distinct_pages(case.keys, case.key_masks, case.splits)
    d = sum(map(len, pages))
    assert len(pages[1]) > 3
    return [0, 1, d, d - 1, d + 5, len(pages[0]) + 2]


@pytest.mark.parametrize("which", range(6), ids=[
    "unlimited", "1", "distinct", "distinct-1", "more", "inside-page-1"])
def test_only_mode(P, pl, which):
    """Output rows = the reference's first rows, in order, per page; the
    limit cuts the page that reaches it and ends the feed."""
    case = only_case()
    limit = _only_limits()[which]
    firsts = M.first_rows(case.keys, case.key_masks)
    assert set(EDGE_ROWS) <= set(firsts)
    assert case.key_masks[0].any() and (case.keys[0] == 0).any()
    emitted = run_only(P, pl, case, [1, 0, 2], limit)
    assert emitted == (firsts[:limit] if limit else firsts)


@pytest.mark.parametrize("with_masks", [True, False],
                         ids=["masks", "no-masks"])
def test_emit_columns(P, pl, with_masks):
    """I128 and U8 columns, one column twice, the key not emitted, NaN and
    -0.0 bit for bit; masks are carried in both modes (run_mark and
    run_only compare them), and without input masks every output
    null_mask is NULL (_assert_same compares the sets of masked
    columns)."""
    case = emit_case(with_masks)
    assert 0 not in EMIT
    assert 50 < case.expected.sum() < case.n
    got = run_mark(P, pl, case, EMIT)
    assert np.array_equal(got, case.expected)
    emitted = run_only(P, pl, case, EMIT)
    assert emitted == np.flatnonzero(case.expected).tolist()


def test_count_distinct_next_to_a_sum(P, pl):
    """count(DISTINCT x), sum(y) GROUP BY g: mark mode over (g, x), its raw
    pages fed into GROUPBY_MULTI(keys=[g], COUNT FILTER (marker = 1),
    SUM_I64(y)).  Nulls in x count as ONE distinct value per group, as the
    reference's MarkDistinct mask does (null is a key value there) — NOT
    SQL's count(DISTINCT x), which would skip them."""
    case = count_distinct_case()
    g, x = case.keys
    xm = case.key_masks[1]
    y = case.extras[0][0]
    exp = {}
    for gi, xi, mi, yi in zip(g.tolist(), x.tolist(), xm.tolist(),
                              y.tolist()):
        seen, total = exp.setdefault(gi, (set(), [0]))
        seen.add(None if mi else xi)
        total[0] += yi
    assert all(None in seen for seen, _ in exp.values())    # a null per group
    exp = {k: (len(s), t[0]) for k, (s, t) in exp.items()}
    with P.Scope() as s:
        md = s.op(P.OP_MARK_DISTINCT,
                  pl.mark_distinct([0, 1], [0, 1, 2], case.capacity))
        gb = s.op(P.OP_GROUPBY_MULTI, pl.group_by(
            [0], [(pl.count(), 0), pl.sum_i64(pl.ident(2))], 64,
            filters=[pl.pred(3, P.CMP_EQ, 1)]))
        for p in range(len(case.splits) - 1):
            keep, raw = _page(P, case, p, p % 2 == 1)
            md.add_input_raw(raw)
            del keep
            gb.add_input_raw(md.get_output_raw())
        md.finish()
        gb.finish()
        out = gb.get_output()
    got = {int(k): (int(c), int(t))
           for k, c, t in zip(out["c0"], out["c1"], out["c2"])}
    assert got == exp
    assert np.array_equal(np.sort(out["c3"]),
                          np.sort(np.bincount(g)[np.bincount(g) > 0]))


def test_table_full(P, pl):
    """200 distinct keys, capacity_hint 8: add_input fails naming the
    field, and so does everything after it."""
    page = P.Page({"k": np.arange(200, dtype=np.int64)})
    with P.Scope() as s:
        op = s.op(P.OP_MARK_DISTINCT, pl.mark_distinct([0], [0], 8))
        with pytest.raises(RuntimeError, match="capacity_hint"):
            op.add_input(page)
        assert op.get_output_raw() is None
        with pytest.raises(RuntimeError, match="capacity_hint"):
            op.add_input(P.Page({"k": np.zeros(1, np.int64)}))
        with pytest.raises(RuntimeError, match="capacity_hint"):
            op.finish()


# ---------------- lifecycle and errors ----------------

@pytest.mark.parametrize("only", [False, True], ids=["mark", "only"])
def test_zero_row_page_and_lifecycle(P, pl, only):
    empty = P.Page({"a": np.empty(0, np.int32), "b": np.empty(0, np.float64),
                    "c": np.empty(0, np.uint8)})
    some = P.Page({"a": np.array([4, 4, 5], np.int32),
                   "b": np.array([1.5, 2.5, 3.5]),
                   "c": np.array([7, 8, 9], np.uint8)})
    make = pl.distinct if only else pl.mark_distinct
    with P.Scope() as s:
        op = s.op(P.OP_MARK_DISTINCT, make([0], [1, 0, 2], 16))
        assert op.needs_input() and not op.is_finished()
        assert op.get_output_raw() is None
        for _ in range(2):
            op.add_input(empty)
            raw = op.get_output_raw()
            assert raw.n_rows == 0
            assert [raw.cols[i].tag for i in range(raw.n_cols)] == \
                [T_F64, T_I32, T_U8] + ([] if only else [T_U8])
            assert op.get_output_raw() is None
        op.add_input(some)
        out = op.get_output()
        if only:
            assert out["c1"].tolist() == [4, 5]
            assert out["c0"].tolist() == [1.5, 3.5]
        else:
            assert out["c3"].tolist() == [1, 0, 1]
            assert out["c2"].tolist() == [7, 8, 9]
        op.add_input(empty)
        assert op.get_output_raw().n_rows == 0
        assert op.needs_input()
        op.finish()
        op.finish()                                     # idempotent
        assert op.get_output_raw() is None              # queues nothing
        assert op.is_finished() and not op.needs_input()
        with pytest.raises(RuntimeError, match="after finish"):
            op.add_input(some)


def _plan(P, n_keys=1, key_col=(0,), mode=0, n_emit=1, emit=(0,),
          capacity=16, limit=0):
    p = P.PlanMarkDistinct()
    p.n_keys, p.mode, p.n_emit = n_keys, mode, n_emit
    p.capacity_hint, p.limit = capacity, limit
    for i, v in enumerate(key_col):
        p.key_col[i] = v
    for i, v in enumerate(emit):
        p.emit_cols[i] = v
    return p


@pytest.mark.parametrize("kw,field", [
    (dict(n_keys=0), "n_keys"), (dict(n_keys=5), "n_keys"),
    (dict(n_emit=0), "n_emit"), (dict(n_emit=17), "n_emit"),
    (dict(mode=2), "mode"), (dict(mode=-1), "mode"),
    (dict(mode=1, limit=-1), "limit"), (dict(mode=0, limit=3), "limit"),
    (dict(capacity=0), "capacity_hint"), (dict(capacity=-4), "capacity_hint"),
    (dict(key_col=(-1,)), r"key_col\[0\]"),
    (dict(n_keys=2, key_col=(0, -2)), r"key_col\[1\]"),
    (dict(n_emit=2, emit=(0, -3)), r"emit_cols\[1\]"),
])
def test_create_rejects(P, kw, field):
    with pytest.raises(RuntimeError, match="MARK_DISTINCT.*" + field):
        P.Operator(P.OP_MARK_DISTINCT, _plan(P, **kw))


def test_create_rejects_a_wrong_plan_size(P):
    L = P.lib()
    plan = _plan(P)
    h = C.c_int64()
    assert L.c.pg_op_create(P.OP_MARK_DISTINCT, C.byref(plan),
                            C.sizeof(plan) - 4, C.byref(h)) != 0
    assert "plan size" in L.err()


def test_add_input_rejects(P, pl):
    i64 = np.array([3, 3, 4, 5], np.int64)
    i32 = np.arange(4, dtype=np.int32)
    f64 = np.arange(4, dtype=np.float64)
    words = P.Varbin([b"a", b"b", b"c", b"d"])
    dct = P.DictVarbin([b"x", b"y"], [0, 1, 1, 0])
    wide = np.arange(8, dtype=np.uint64).reshape(4, 2)
    two = P.Page({"a": i64, "b": i32})
    three = P.Page({"a": i64, "b": i32, "c": i64})

    def raw_of(cols):
        case = Case(("i64",) * len(cols), cols, [None] * len(cols),
                    splits=(0, 4))
        return _page(P, case, 0, False)

    def rejects(plan, page, field, ok, marker, first=None):
        """`page` is rejected naming `field`; the operator is as it was:
        the page `ok` then gives `marker`, so the rejected page's rows
        were never seen."""
        with P.Scope() as s:
            op = s.op(P.OP_MARK_DISTINCT, plan)
            if first is not None:
                op.add_input(first)
                assert op.get_output_raw().n_rows == 4
            with pytest.raises(RuntimeError, match=field):
                op.feed(page)
            assert op.get_output_raw() is None and op.needs_input()
            op.add_input(ok)
            assert list(op.get_output().values())[-1].tolist() == marker

    md = pl.mark_distinct
    rejects(md([2], [0], 16), two, r"key_col\[0\]", three, [1, 0, 1, 1])
    rejects(md([0], [0, 2], 16), two, r"emit_cols\[1\]", three,
            [1, 0, 1, 1])
    rejects(md([0, 1], [0], 16), P.Page({"a": i64, "f": f64}),
            r"key_col\[1\].*F64", two, [1, 1, 1, 1])
    rejects(md([0, 1], [0], 16), P.Page({"a": i64, "w": words}),
            r"key_col\[1\].*VARBIN", two, [1, 1, 1, 1])
    rejects(md([0], [1], 16), P.Page({"a": i64, "w": words}),
            r"emit_cols\[0\]", two, [1, 0, 1, 1])
    rejects(md([0], [0, 1], 16), P.Page({"a": i64, "d": dct}),
            r"emit_cols\[1\]", two, [1, 0, 1, 1])
    keep, raw = raw_of([i64, wide])
    rejects(md([1], [0], 16), raw, r"key_col\[0\].*I128", two, [1, 1, 1, 1])
    del keep
    # a type that differs from the first page's; the keys 6 and 7 of the
    # rejected page stay unseen
    rejects(md([0], [1], 16), P.Page({"a": i64 + 3, "b": i64}),
            r"emit_cols\[0\]", P.Page({"a": i64 + 2, "b": i32}),
            [0, 0, 1, 1], first=two)
    rejects(md([0], [1], 16), P.Page({"a": i32 + 6, "b": i32}),
            r"key_col\[0\]", P.Page({"a": i64 + 2, "b": i32}),
            [0, 0, 1, 1], first=two)
    # a dictionary key is fine
    with P.Scope() as s:
        op = s.op(P.OP_MARK_DISTINCT, md([1], [0], 16))
        op.add_input(P.Page({"a": i64, "d": dct}))
        assert op.get_output()["c1"].tolist() == [1, 1, 0, 0]


def test_add_input_rejects_more_rows_than_row_ids(P, pl):
    """Row ids are 32-bit.  The count is checked before anything is
    copied, so the page only has to CLAIM its rows."""
    small = np.arange(4, dtype=np.int64)
    with P.Scope() as s:
        op = s.op(P.OP_MARK_DISTINCT, pl.distinct([0], [0], 16))
        page = P.Page({"a": small})
        raw = page.to_c()
        raw.n_rows = 2**31
        with pytest.raises(RuntimeError, match="2\\^31-1"):
            op.add_input_raw(raw)
        op.add_input(page)
        assert op.get_output_raw().n_rows == 4
