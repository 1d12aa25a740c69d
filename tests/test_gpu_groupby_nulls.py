"""PG_OP_GROUPBY_MULTI with pg_plan_groupby.sql_nulls = 1 on the GPU against
the reference of groupby_null_refs.py.  Every comparison is exact, after the
groups are keyed by their key tuple (None for a null key).

Sizes follow the kernels' geometry (kernels.hip): the insert kernel is a
4096 x 256 grid with a grid stride, so 2^20 + 1 rows is the smallest input
whose last row is taken in a second pass; the emit kernel compacts 256
slots per step over 64-lane waves, and the tables here span several steps.
Pages alternate between host- and device-resident, page 0 on the host.

Every case is built on the CPU first and must contain a null-key group, a
group in which some aggregate receives no non-null input and a group in
which some aggregate receives both null and non-null input (_covered)."""
import functools

import numpy as np
import pytest

import groupby_null_refs as G
import outer_join_refs as R

pytestmark = pytest.mark.gpu

T_U8, T_I32, T_I64, T_F64 = 0, 1, 2, 3
_NP_OF_TAG = {T_U8: np.uint8, T_I32: np.int32, T_I64: np.int64,
              T_F64: np.float64}
I64_MAX = np.iinfo(np.int64).max
DICT = [b"key-%02d" % i for i in range(40)]     # distinct entries


@pytest.fixture(scope="module")
def P():
    import presto_amd
    return presto_amd


@pytest.fixture(scope="module")
def pl():
    from presto_amd import plans
    return plans


# ---------------- cases (CPU only) ----------------

class Case:
    """keys / key_masks / cols / masks as the reference takes them;
    dict_key: the key channels that are dictionary VARBIN (their key array
    holds the ids); splits: the page boundaries."""

    def __init__(self, keys, key_masks, specs, cols, masks, splits,
                 dict_key=(), capacity=None):
        # the legacy run groups by the garbage under the nulls: up to n
        # groups
        self.capacity = capacity or len(keys[0]) + 16
        self.keys, self.key_masks, self.specs = keys, key_masks, specs
        self.cols, self.masks, self.splits = cols, masks, splits
        self.dict_key = tuple(dict_key)
        self.n = len(keys[0])

    @functools.cached_property
    def expected(self):
        return G.group_by(self.keys, self.key_masks, self.specs, self.cols,
                          self.masks)

    @functools.cached_property
    def legacy(self):
        return G.group_by(self.keys, self.key_masks, self.specs, self.cols,
                          self.masks, sql_nulls=False)

    @functools.cached_property
    def counts(self):
        return G.input_counts(self.keys, self.key_masks, self.specs,
                              self.cols, self.masks)


def _covered(case):
    """A null-key group, an all-null (group, aggregate) and a mixed one."""
    fed = [(key, a, nulls, vals) for key, per in case.counts.items()
           for a, (nulls, vals) in enumerate(per)
           if case.specs[a][0] != G.COUNT]
    assert any(None in key for key in case.expected)
    assert any(vals == 0 for _, _, _, vals in fed)
    assert any(nulls > 0 and vals > 0 for _, _, nulls, vals in fed)
    for key, a, _, vals in fed:
        assert (case.expected[key][0][a] is None) == (vals == 0)


_GARBAGE = {"u8": (0, 256), "i32": (-2**31, 2**31), "i64": (-2**62, 2**62),
            "dict": (0, len(DICT))}
_DTYPE = {"u8": np.uint8, "i32": np.int32, "i64": np.int64, "dict": np.int32}


def _key_channel(rng, n, kind, domain, frac=0.1):
    """Values 0..domain-1 (the real key 0 included), ~frac nulls, and under
    the nulls garbage that differs from row to row."""
    k = rng.integers(0, domain, n)
    m = (rng.random(n) < frac).astype(np.uint8)
    lo, hi = _GARBAGE[kind]
    k = np.where(m == 1, rng.integers(lo, hi, n), k).astype(_DTYPE[kind])
    assert (k[m == 0] == 0).any() and len(np.unique(k[m == 1])) > 1
    return k, m


def _force(key, key_mask, value, cols, masks, null):
    """Rows of the non-null key `value`: all value columns null, or all
    non-null zeros."""
    rows = (key == value) & (key_mask == 0)
    assert rows.sum() > 1
    for c, m in zip(cols, masks):
        m[rows] = 1 if null else 0
        if not null:
            c[rows] = 0


SPLITS = (0, 1000, 2049, 3000)      # three pages, none a multiple of 256


@functools.lru_cache(maxsize=None)
def key_case(kinds):
    rng = np.random.default_rng(len(kinds) * 100 + sum(map(ord, kinds[0])))
    n = SPLITS[-1]
    chans = [_key_channel(rng, n, kind, 5) for kind in kinds]
    keys, key_masks = [k for k, _ in chans], [m for _, m in chans]
    v = rng.integers(-1000, 1000, n).astype(np.int64)
    vm = (rng.random(n) < 0.3).astype(np.uint8)
    _force(keys[0], key_masks[0], 1, [v], [vm], null=True)
    specs = [(G.SUM_I64, (G.IDENT, 0), None), (G.MIN, (G.IDENT, 0), None),
             (G.COUNT, (G.IDENT, 0), None)]
    return Case(keys, key_masks, specs, [v], [vm], SPLITS,
                [i for i, kind in enumerate(kinds) if kind == "dict"])


KEY_KINDS = [("u8",), ("i32",), ("i64",), ("dict",), ("u8", "i64"),
             ("i32", "u8"), ("i64", "i32"), ("dict", "i64")]


@functools.lru_cache(maxsize=None)
def one_group_case():
    rng = np.random.default_rng(5)
    n = 2**20 + 1
    key = rng.integers(-2**62, 2**62, n).astype(np.int64)
    a = rng.integers(-1000, 1000, n).astype(np.int64)
    am = (rng.random(n) < 0.3).astype(np.uint8)
    am[-1] = 0
    a[-1] = 5000            # the second-pass row holds the maximum
    b = rng.integers(-2**62, 2**62, n).astype(np.int64)
    specs = [(G.SUM_I64, (G.IDENT, 0), None), (G.MIN, (G.IDENT, 1), None),
             (G.MAX, (G.IDENT, 0), None), (G.COUNT, (G.IDENT, 0), None)]
    return Case([key], [np.ones(n, np.uint8)], specs, [a, b],
                [am, np.ones(n, np.uint8)], (0, n), capacity=64)


@functools.lru_cache(maxsize=None)
def agg_case():
    """Group 1 all null, group 2 zeros only, the rest (the null-key group
    included) mixed.  What sits under the nulls is small and in domain, so
    the same pages also run with sql_nulls = 0."""
    rng = np.random.default_rng(17)
    n = SPLITS[-1]
    key, km = _key_channel(rng, n, "i64", 8)
    key[km == 1] = rng.integers(100, 2000, int(km.sum()))
    v0, v1, v2 = (rng.integers(-1000, 1000, n).astype(np.int64)
                  for _ in range(3))
    v3 = rng.integers(-2**40, 2**40, n).astype(np.int64)
    f0 = rng.integers(0, 4000, n).astype(np.float64) * 0.25
    f1 = rng.integers(0, 2, n).astype(np.float64) * 0.5
    cols = [v0, v1, v2, v3, f0, f1]
    masks = [(rng.random(n) < p).astype(np.uint8)
             for p in (0.3, 0.3, 0.3, 0.3, 0.3, 0.2)]
    _force(key, km, 1, cols, masks, null=True)
    _force(key, km, 2, cols, masks, null=False)
    specs = [(G.SUM_I64, (G.IDENT, 0), None), (G.SUM_DEC, (G.IDENT, 0), None),
             (G.SUM_I64, (G.MUL, 1, 2), None), (G.MIN, (G.IDENT, 3), None),
             (G.MAX, (G.IDENT, 3), None),
             (G.SUM_F64, (G.DISC_PRICE, 4, 5), None)]
    return Case([key], [km], specs, cols, masks, SPLITS)


@functools.lru_cache(maxsize=None)
def poison_case():
    rng = np.random.default_rng(23)
    n = SPLITS[-1]
    key, km = _key_channel(rng, n, "i64", 6)
    v = rng.integers(1, 100, n).astype(np.int64)
    f = rng.integers(0, 4000, n).astype(np.float64) * 0.25
    vm = (rng.random(n) < 0.2).astype(np.uint8)
    fm = (rng.random(n) < 0.2).astype(np.uint8)
    _force(key, km, 1, [v, f], [vm, fm], null=True)
    v[vm == 1] = I64_MAX
    f[fm == 1] = np.where(np.arange(int(fm.sum())) % 2, np.nan, -1.0)
    specs = [(G.SUM_I64, (G.IDENT, 0), None), (G.SUM_F64, (G.IDENT, 1), None)]
    return Case([key], [km], specs, [v, f], [vm, fm], SPLITS)


FILTER_EMPTY = (1, 2)       # the groups whose every row the FILTER rejects


@functools.lru_cache(maxsize=None)
def filter_case():
    rng = np.random.default_rng(29)
    n = SPLITS[-1]
    key, km = _key_channel(rng, n, "i64", 8)
    key[km == 1] = rng.integers(100, 2000, int(km.sum()))
    v = rng.integers(-1000, 1000, n).astype(np.int64)
    vm = (rng.random(n) < 0.2).astype(np.uint8)
    f = rng.integers(0, 300, n).astype(np.int64)
    fm = (rng.random(n) < 0.05).astype(np.uint8)
    low = np.isin(key, FILTER_EMPTY) & (km == 0)
    f[low] = rng.integers(0, 101, int(low.sum()))
    flt = (G.GT, 1, 100)
    specs = [(G.MIN, (G.IDENT, 0), flt), (G.MAX, (G.IDENT, 0), flt),
             (G.SUM_I64, (G.IDENT, 0), flt), (G.COUNT, (G.IDENT, 0), flt),
             (G.SUM_I64, (G.IDENT, 0), None)]
    return Case([key], [km], specs, [v, f], [vm, fm], SPLITS)


# ---------------- plumbing ----------------

def _plan(P, pl, case, sql_nulls, specs=None):
    nk = len(case.keys)
    filters, aggs = [], []
    for func, proj, flt in (case.specs if specs is None else specs):
        ch = [nk + c for c in proj[1:]]
        pr = {G.IDENT: pl.ident, G.MUL: pl.mul,
              G.DISC_PRICE: pl.disc_price}[proj[0]](*ch)
        agg = {G.COUNT: lambda: pl.count(),
               G.SUM_I64: lambda: pl.sum_i64(pr),
               G.SUM_DEC: lambda: pl.sum_dec(pr, 0),
               G.SUM_F64: lambda: pl.sum_f64(pr),
               G.MIN: lambda: pl.agg_min(pr),
               G.MAX: lambda: pl.agg_max(pr)}[func]()
        if flt is None:
            aggs.append(agg)
            continue
        col = nk + flt[1]
        pred = {G.NOT_NULL: lambda: pl.pred_not_null(col),
                G.IS_NULL: lambda: pl.pred_is_null(col),
                G.GT: lambda: pl.pred(col, P.CMP_GT, flt[2])}[flt[0]]()
        aggs.append((agg, len(filters)))
        filters.append(pred)
    return pl.group_by(range(nk), aggs, case.capacity,
                       filters=filters, sql_nulls=sql_nulls)


def _page(P, case, lo, hi, device):
    import torch
    named, nulls = {}, {}
    chans = [(k, m, ch in case.dict_key) for ch, (k, m) in
             enumerate(zip(case.keys, case.key_masks))]
    chans += [(c, m, False) for c, m in zip(case.cols, case.masks)]
    for i, (a, m, is_dict) in enumerate(chans):
        a = np.ascontiguousarray(a[lo:hi])
        if is_dict:
            a = P.DictVarbin(DICT, a)
            named[f"c{i}"] = P.DeviceVarbin.from_host(a) if device else a
        else:
            named[f"c{i}"] = torch.from_numpy(a).cuda() if device else a
        if m is not None:
            m = np.ascontiguousarray(m[lo:hi], np.uint8)
            nulls[f"c{i}"] = torch.from_numpy(m).cuda() if device else m
    page = P.Page(named, n_rows=hi - lo, nulls=nulls)
    raw = page.to_c()
    if device:
        torch.cuda.synchronize()
    return page, raw


def _d2h(P, ptr, nbytes):
    buf = np.empty(nbytes, np.uint8)
    if nbytes:
        L = P.lib()
        L.check(L.c.pg_memcpy_d2h(buf.ctypes.data, ptr, nbytes), "d2h")
    return buf


def _read_groups(P, raw, nk, funcs, sql_nulls):
    """The raw output page as {key tuple: ([values], rows)}, after checking
    which columns carry a mask and that values under nulls are 0."""
    n = raw.n_rows
    assert raw.n_cols == nk + len(funcs) + 1
    want_mask = [True] * nk + [f != G.COUNT for f in funcs] + [False]
    cols = []
    for i in range(raw.n_cols):
        c = raw.cols[i]
        assert c.on_device == 1
        dt = np.dtype(_NP_OF_TAG[c.tag])
        vals = _d2h(P, c.data, n * dt.itemsize).view(dt)
        assert bool(c.null_mask) == (sql_nulls and want_mask[i]), i
        if c.null_mask:
            m = _d2h(P, c.null_mask, n)
            assert set(np.unique(m).tolist()) <= {0, 1}, i
            assert not vals[m == 1].view(np.uint8).any(), i   # 0 under null
            vals = [None if isnull else v
                    for v, isnull in zip(vals.tolist(), m.tolist())]
        else:
            vals = vals.tolist()
        cols.append(vals)
    out = {}
    for row in zip(*cols):
        out[tuple(row[:nk])] = (list(row[nk:-1]), row[-1])
    assert len(out) == n        # exact grouping: no key tuple twice
    return out


def _tags(P, raw):
    return [raw.cols[i].tag for i in range(raw.n_cols)]


def _run(P, pl, case, sql_nulls, specs=None):
    specs = case.specs if specs is None else specs
    with P.Scope() as s:
        op = s.op(P.OP_GROUPBY_MULTI, _plan(P, pl, case, sql_nulls, specs))
        for i, (lo, hi) in enumerate(zip(case.splits, case.splits[1:])):
            keep, raw = _page(P, case, lo, hi, i % 2 == 1)
            assert op.needs_input()
            op.add_input_raw(raw)
            del keep
        op.finish()
        raw = op.get_output_raw()
        assert raw is not None
        got = _read_groups(P, raw, len(case.keys), [f for f, _, _ in specs],
                           sql_nulls)
        tags = _tags(P, raw)
        assert op.get_output_raw() is None and op.is_finished()
    return got, tags


def _same(got, exp):
    assert sorted(got, key=repr) == sorted(exp, key=repr)
    for key in exp:
        assert got[key] == exp[key], key


_KEY_TAG = {np.dtype(np.uint8): T_U8, np.dtype(np.int32): T_I32,
            np.dtype(np.int64): T_I64}


# ---------------- the tests ----------------

@pytest.mark.parametrize("kinds", KEY_KINDS, ids="-".join)
def test_key_nulls(P, pl, kinds):
    case = key_case(kinds)
    _covered(case)
    exp = case.expected
    nk = len(kinds)
    # null is a group of its own next to the real key 0, per channel
    for ch in range(nk):
        assert any(k[ch] is None for k in exp)
        assert any(k[ch] == 0 for k in exp)
    if nk == 2:
        assert {(None, None), (None, 0), (0, None), (0, 0)} <= set(exp)
    assert len(exp) == 6 ** nk
    got, tags = _run(P, pl, case, True)
    _same(got, exp)
    assert tags[:nk] == [_KEY_TAG[k.dtype] for k in case.keys]


def test_one_group_of_null_keys(P, pl):
    """2^20 + 1 rows, every key null over differing garbage: one slot takes
    every atomic, and the last row comes in the second grid pass."""
    case = one_group_case()
    _covered(case)
    exp = case.expected
    assert list(exp) == [(None,)] and exp[(None,)][1] == 2**20 + 1
    assert exp[(None,)][0][1] is None and exp[(None,)][0][2] == 5000
    got, _ = _run(P, pl, case, True)
    _same(got, exp)


def test_aggregate_nulls(P, pl):
    case = agg_case()
    _covered(case)
    exp = case.expected
    assert exp[(1,)][0] == [None] * 6 and exp[(1,)][1] > 1      # all null
    assert exp[(2,)][0] == [0, 0, 0, 0, 0, 0.0]                 # zeros only
    for key in ((None,), (0,), (3,)):                           # mixed
        assert None not in exp[key][0]
        assert all(n > 0 and v > 0 for n, v in case.counts[key])
    got, tags = _run(P, pl, case, True)
    _same(got, exp)
    assert tags == [T_I64] * 6 + [T_F64, T_I64]


def test_poison_under_nulls(P, pl):
    """INT64_MAX, NaN and -1.0 under the nulls reach no accumulator and no
    overflow or domain counter — and they are live: the same pages fail
    finish when the masks are not honored."""
    case = poison_case()
    _covered(case)
    assert all((case.cols[0][(case.keys[0] == k) & (case.key_masks[0] == 0)]
                == I64_MAX).sum() >= 2 for k in range(6))
    assert np.isnan(case.cols[1]).any() and (case.cols[1] == -1.0).any()
    got, _ = _run(P, pl, case, True)
    _same(got, case.expected)
    with pytest.raises(RuntimeError, match="SUM overflow"):
        _run(P, pl, case, False, case.specs[:1])
    with pytest.raises(RuntimeError, match="SUM_F64"):
        _run(P, pl, case, False, case.specs[1:])


def test_filter_that_empties_groups(P, pl):
    case = filter_case()
    _covered(case)
    exp = case.expected
    for k in FILTER_EMPTY:
        vals, rows = exp[(k,)]
        assert vals[:4] == [None, None, None, 0] and rows > 0
        assert vals[4] is not None
    got, _ = _run(P, pl, case, True)
    _same(got, exp)


def test_masks_on_output(P, pl):
    """Key and SUM / MIN / MAX columns carry a device mask of n_rows bytes,
    COUNT and the row count none; a value under a null is 0 (checked for
    every run in _read_groups, here on the descriptor itself)."""
    case = filter_case()
    with P.Scope() as s:
        op = s.op(P.OP_GROUPBY_MULTI, _plan(P, pl, case, True))
        op.add_input_raw(_page(P, case, 0, case.n, False)[1])
        op.finish()
        raw = op.get_output_raw()
        assert raw.n_rows == len(case.expected)
        present = [bool(raw.cols[i].null_mask) for i in range(raw.n_cols)]
        assert present == [True, True, True, True, False, True, False]
        ptrs = [raw.cols[i].null_mask for i in range(raw.n_cols)
                if raw.cols[i].null_mask]
        assert len(set(ptrs)) == len(ptrs)
        key_mask = _d2h(P, raw.cols[0].null_mask, raw.n_rows)
        key = _d2h(P, raw.cols[0].data, raw.n_rows * 8).view(np.int64)
        assert key_mask.sum() == 1 and key[key_mask == 1].tolist() == [0]
        mn_mask = _d2h(P, raw.cols[1].null_mask, raw.n_rows)
        mn = _d2h(P, raw.cols[1].data, raw.n_rows * 8).view(np.int64)
        assert mn_mask.sum() == len(FILTER_EMPTY)
        assert mn[mn_mask == 1].tolist() == [0] * len(FILTER_EMPTY)


# data helpers in the shapes of test_gpu_outer_join.py

def _build(P, pl, s, keys, payloads, **kw):
    cols = {"k": np.asarray(keys, np.int64)}
    for i, p in enumerate(payloads):
        cols[f"p{i}"] = p
    b = s.build(pl.hash_build(0, payload=range(1, 1 + len(payloads)), **kw),
                P.Page(cols))
    return b.table()


ALL_UNMATCHED = (3, 7)      # groups whose probe keys match no build row


@functools.lru_cache(maxsize=None)
def _left_join_data():
    rng = np.random.default_rng(11)
    n, nb = 3000, 400
    bkeys = rng.integers(0, 500, nb).astype(np.int64)
    pay = rng.integers(-10**6, 10**6, nb).astype(np.int64)
    pkeys = rng.integers(0, 1000, n).astype(np.int64)
    key_nulls = (rng.random(n) < 0.05).astype(np.uint8)
    grp, grp_nulls = _key_channel(rng, n, "i64", 40, 0.05)
    pkeys[np.isin(grp, ALL_UNMATCHED) & (grp_nulls == 0)] += 5000
    return bkeys, pay, pkeys, key_nulls, grp, grp_nulls


@functools.lru_cache(maxsize=None)
def join_case():
    """The LEFT join's output page [group, payload] as a group-by case."""
    bkeys, pay, pkeys, key_nulls, grp, grp_nulls = _left_join_data()
    cols, masks, _ = R.outer_join(bkeys, [pay], [grp, grp_nulls], pkeys,
                                  key_nulls, None, R.PROBE_OUTER)
    specs = [(G.MIN, (G.IDENT, 0), None), (G.SUM_I64, (G.IDENT, 0), None),
             (G.COUNT, (G.IDENT, 0), (G.NOT_NULL, 0))]
    return Case([cols[0]], [cols[1]], specs, [cols[2]], [masks],
                (0, len(masks)))


def test_left_join_then_group_by(P, pl):
    """LEFT JOIN -> GROUP BY through raw device pages: unmatched probe rows
    give null min / sum and count 0."""
    case = join_case()
    _covered(case)
    exp = case.expected
    for g in ALL_UNMATCHED:
        assert exp[(g,)][0] == [None, None, 0] and exp[(g,)][1] > 0
    bkeys, pay, pkeys, key_nulls, grp, grp_nulls = _left_join_data()
    with P.Scope() as s:
        table = _build(P, pl, s, bkeys, [pay])
        j, raw = s.pipe(P.OP_LOOKUP_JOIN, pl.left_join(table, 1, [0]),
                        P.Page({"g": grp, "k": pkeys},
                               nulls={"g": grp_nulls, "k": key_nulls}))
        assert raw.n_rows == case.n
        assert raw.cols[0].null_mask and raw.cols[1].null_mask
        g = s.run(P.OP_GROUPBY_MULTI, pl.group_by(
            [0], [pl.agg_min(pl.ident(1)), pl.sum_i64(pl.ident(1)),
                  (pl.count(), 0)], case.n + 16,
            filters=[pl.pred_not_null(1)], sql_nulls=True), raw)
        got = _read_groups(P, g.get_output_raw(), 1,
                           [G.MIN, G.SUM_I64, G.COUNT], True)
    _same(got, exp)


@pytest.mark.parametrize("name", ["agg", "filter", "keys-i64-i32",
                                  "keys-dict"])
def test_default_is_unchanged(P, pl, name):
    """sql_nulls = 0 on the same pages: keys and inputs are the stored
    values, an aggregate without input shows its identity, no masks."""
    case = {"agg": agg_case, "filter": filter_case,
            "keys-i64-i32": lambda: key_case(("i64", "i32")),
            "keys-dict": lambda: key_case(("dict",))}[name]()
    exp = case.legacy
    assert not any(None in k for k in exp)
    assert sorted(exp, key=repr) != sorted(case.expected, key=repr)
    got, _ = _run(P, pl, case, False)       # asserts that no mask is set
    _same(got, exp)
    if name == "filter":
        assert exp[(1,)][0][:4] == [G.INT64_MAX, G.INT64_MIN, 0, 0]


def test_bad_plan_value(P, pl):
    case = filter_case()
    with pytest.raises(RuntimeError, match="sql_nulls"):
        with P.Scope() as s:
            s.op(P.OP_GROUPBY_MULTI, _plan(P, pl, case, 2))
