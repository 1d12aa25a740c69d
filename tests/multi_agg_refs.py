"""Row-at-a-time reference of the multi-aggregate probe (LOOKUP_JOIN mode 1
with n_aggs > 0; include/presto_gpu.h, pg_plan_lookup_join.n_aggs and
acc_pack), the named wrong models it must be told apart from, and the
datasets of tests/test_gpu_multi_agg.py.  numpy arrays for storage, Python
ints for the arithmetic.  No GPU, no ctypes — this is the checker, never
the product.

The contract, as the header states it:
  - a row that fails the row predicates is skipped;
  - a row whose key is in the table's domain counts, and adds its ticks to
    every aggregate whose FILTER (if any) passes;
  - a null under a mask makes a comparison false, IS_NULL / IS_NOT_NULL
    test the mask;
  - output {key: (payloads..., agg_0 .. agg_{n-1}, count)} for count >= 1.

Loud errors are modelled without the kernel's flush granularity: classify()
sorts an input into "clean" or "overflow" (finish must raise) and refuses
the rest as ambiguous, because which wrapped partial sum the kernel sees
depends on the order of its adds.
"""
import operator
from typing import NamedTuple, Optional

import numpy as np

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1

_CMP = {"lt": operator.lt, "le": operator.le, "gt": operator.gt,
        "ge": operator.ge, "eq": operator.eq, "ne": operator.ne}


# --------------------------------------------------------------------- #
# the plan, in reference terms                                           #
# --------------------------------------------------------------------- #
class Pred(NamedTuple):
    col: str
    op: str            # lt le gt ge eq ne is_null not_null
    rhs: object = 0    # an int for integer columns, a float for f64 ones


class Agg(NamedTuple):
    kind: str                    # count | sum_i64 | sum_dec
    col: Optional[str] = None    # count: ignored
    filt: Optional[int] = None   # index into preds + filters, as agg_filter
    scale: int = 0               # sum_dec: ticks = round(x * 10^scale)


class Pack(NamedTuple):
    shift: tuple       # per aggregate: bit offset in word 0, -1 = own word
    width: tuple       # per aggregate (unread for an own word)
    cnt_shift: int
    cnt_width: int


class Spec(NamedTuple):
    key: str
    aggs: tuple
    preds: tuple = ()      # row predicates (a conjunction)
    filters: tuple = ()    # per-aggregate FILTER predicates
    pack: Optional[Pack] = None


class Page:
    """cols: name -> array, in channel order.  nulls: name -> 0/1 mask.
    ticks: name -> list of Python ints, the exact ticks of an f64 column
    as edge_refs.ticks_exact returned them (what SUM_DEC must add)."""

    def __init__(self, cols, nulls=None, ticks=None):
        self.cols = {k: np.asarray(v) for k, v in cols.items()}
        self.nulls = {k: np.asarray(v, np.uint8)
                      for k, v in (nulls or {}).items()}
        self.ticks = dict(ticks or {})
        self.n = len(next(iter(self.cols.values())))
        assert all(len(v) == self.n for v in self.cols.values())
        assert all(len(v) == self.n for v in self.nulls.values())
        assert all(len(v) == self.n for v in self.ticks.values())

    def channel(self, name):
        return list(self.cols).index(name)

    def rows(self, lo, hi):
        return Page({k: v[lo:hi] for k, v in self.cols.items()},
                    {k: v[lo:hi] for k, v in self.nulls.items()},
                    {k: v[lo:hi] for k, v in self.ticks.items()})


class Table(NamedTuple):
    """The group domain: build keys with their payload columns (kind
    "hash", an agg_table), or the range [1, K] (kind "range").  pack_bits,
    fill_x10 and bitmap_max_key shape the device table and leave the
    domain alone."""
    kind: str
    keys: tuple = ()
    payloads: tuple = ()     # arrays, one per payload column
    K: int = 0
    pack_bits: int = 0
    fill_x10: int = 0
    bitmap_max_key: int = 0

    def domain(self):
        if self.kind == "range":
            return None
        return {int(k): tuple(int(p[i]) for p in self.payloads)
                for i, k in enumerate(self.keys)}


def hash_table(keys, payloads=(), **shape):
    keys = tuple(int(k) for k in keys)
    assert len(set(keys)) == len(keys)
    return Table("hash", keys, tuple(np.asarray(p) for p in payloads),
                 **shape)


def range_table(K):
    return Table("range", K=K)


class Case(NamedTuple):
    """One input of the GPU tests.  sees: the wrong models (letters of
    WRONG_MODELS) whose output on this input must differ from the
    reference's.  expect: what classify() must say."""
    table: Table
    pages: tuple
    spec: Spec
    sees: str = ""
    expect: str = "clean"


# --------------------------------------------------------------------- #
# the reference                                                          #
# --------------------------------------------------------------------- #
def _is_null(page, col, i):
    m = page.nulls.get(col)
    return m is not None and bool(m[i])


def _value(page, col, i):
    a = page.cols[col]
    return float(a[i]) if a.dtype.kind == "f" else int(a[i])


def pred_ok(page, p, i):
    null = _is_null(page, p.col, i)
    if p.op == "is_null":
        return null
    if p.op == "not_null":
        return not null
    if null:
        return False
    v = _value(page, p.col, i)
    assert isinstance(p.rhs, float) == isinstance(v, float), \
        "a literal compares in its column's domain"
    return _CMP[p.op](v, p.rhs)


def _ticks(page, ag, i):
    if ag.kind == "count":
        return 1
    if ag.kind == "sum_i64":
        assert page.cols[ag.col].dtype.kind in "iu"
        return int(page.cols[ag.col][i])
    assert ag.kind == "sum_dec"
    return int(page.ticks[ag.col][i])


class Row(NamedTuple):
    page: int
    i: int
    key: int
    passed: bool              # the row predicates
    payload: Optional[tuple]  # None: the key is not in the domain
    contrib: tuple            # per aggregate: ticks, or None = filtered out


def _lookup(table, dom, key):
    if dom is None:
        return () if 1 <= key <= table.K else None
    return dom.get(key)


def rows(table, pages, spec, with_failed=False):
    """Every probe row that passes the row predicates (with_failed: every
    row), in page order."""
    dom = table.domain()
    allp = tuple(spec.preds) + tuple(spec.filters)
    for pno, pg in enumerate(pages):
        for i in range(pg.n):
            passed = all(pred_ok(pg, p, i) for p in spec.preds)
            if not passed and not with_failed:
                continue
            key = int(pg.cols[spec.key][i])
            contrib = tuple(
                None if ag.filt is not None and
                not pred_ok(pg, allp[ag.filt], i) else _ticks(pg, ag, i)
                for ag in spec.aggs)
            yield Row(pno, i, key, passed, _lookup(table, dom, key), contrib)


def _emit(table, acc):
    dom = table.domain()
    return {k: (dom[k] if dom is not None else ()) + tuple(st)
            for k, st in acc.items() if st[-1] >= 1}


def _add(acc, n, key, contrib, count=1):
    st = acc.setdefault(key, [0] * (n + 1))
    for a, c in enumerate(contrib):
        if c is not None:
            st[a] += c
    st[n] += count


def multi_agg_ref(table, pages, spec):
    """{key: (payloads..., agg_0 .. agg_{n-1}, count)} in Python ints."""
    n = len(spec.aggs)
    acc = {}
    for r in rows(table, pages, spec):
        if r.payload is not None:
            _add(acc, n, r.key, r.contrib)
    return _emit(table, acc)


def _is_field(spec, a):
    return spec.pack is not None and spec.pack.shift[a] >= 0


def classify(table, pages, spec):
    """"clean": finish must not raise and the output is multi_agg_ref's.
    "overflow": finish must raise.  Anything else is an input on which the
    kernel's answer depends on the order of its adds: ValueError."""
    n = len(spec.aggs)
    hit = [r for r in rows(table, pages, spec)]
    addends = {}                       # key -> per aggregate list of ticks
    for r in hit:
        if r.payload is None:
            continue
        per = addends.setdefault(r.key, [[] for _ in range(n)] + [0])
        for a, c in enumerate(r.contrib):
            if c is not None:
                per[a].append(c)
        per[n] += 1
    clean, must = True, False
    for key, per in addends.items():
        if spec.pack is not None and per[n] >= 1 << spec.pack.cnt_width:
            clean = False
        for a in range(n):
            v = per[a]
            if _is_field(spec, a):
                w = spec.pack.width[a]
                if any(c < 0 for c in v) or sum(v) >= 1 << w:
                    clean = False
                if all(c >= 0 for c in v) and any(c >= 1 << w for c in v):
                    must = True
            else:
                if sum(abs(c) for c in v) >= 1 << 63:
                    clean = False
                one_sign = all(c >= 0 for c in v) or all(c <= 0 for c in v)
                if one_sign and not I64_MIN <= sum(v) <= I64_MAX:
                    must = True
    # a negative contribution to a bit field that no run can cancel: both
    # neighbours among the rows that pass the row predicates (a failing row
    # breaks no run) hold other keys, or there is none in the page
    for j, r in enumerate(hit):
        if r.payload is None:
            continue
        neg = [a for a in range(n) if _is_field(spec, a) and
               r.contrib[a] is not None and r.contrib[a] < 0]
        if not neg:
            continue
        alone = all(not (0 <= q < len(hit)) or hit[q].page != r.page or
                    hit[q].key != r.key for q in (j - 1, j + 1))
        if alone:
            must = True
    if clean and must:
        raise AssertionError("classification rules contradict each other")
    if clean:
        return "clean"
    if must:
        return "overflow"
    raise ValueError("ambiguous input")


# --------------------------------------------------------------------- #
# the numpy twin, for the one multi-million-row case                     #
# --------------------------------------------------------------------- #
def _pred_mask(pg, p):
    null = pg.nulls.get(p.col)
    null = np.zeros(pg.n, bool) if null is None else null != 0
    if p.op == "is_null":
        return null
    if p.op == "not_null":
        return ~null
    a = pg.cols[p.col]
    a = a.astype(np.float64) if a.dtype.kind == "f" else a.astype(np.int64)
    return getattr(np, {"lt": "less", "le": "less_equal", "gt": "greater",
                        "ge": "greater_equal", "eq": "equal",
                        "ne": "not_equal"}[p.op])(a, p.rhs) & ~null


def multi_agg_ref_np(table, pages, spec):
    """multi_agg_ref on int64 with np.add.at: exact while every group total
    stays inside int64, which the caller's small values guarantee (and the
    CPU tests check against the row model)."""
    n = len(spec.aggs)
    dom = table.domain()
    allp = tuple(spec.preds) + tuple(spec.filters)
    acc = {}
    for pg in pages:
        key = pg.cols[spec.key].astype(np.int64)
        ok = np.ones(pg.n, bool)
        for p in spec.preds:
            ok &= _pred_mask(pg, p)
        if dom is None:
            ok &= (key >= 1) & (key <= table.K)
        else:
            ok &= np.isin(key, np.fromiter(dom, np.int64, len(dom)))
        uk, inv = np.unique(key[ok], return_inverse=True)
        sums = np.zeros((n + 1, len(uk)), np.int64)
        for a, ag in enumerate(spec.aggs):
            if ag.kind == "count":
                t = np.ones(pg.n, np.int64)
            elif ag.kind == "sum_i64":
                t = pg.cols[ag.col].astype(np.int64)
            else:
                t = np.array(pg.ticks[ag.col], np.int64)
            if ag.filt is not None:
                t = np.where(_pred_mask(pg, allp[ag.filt]), t, 0)
            np.add.at(sums[a], inv, t[ok])
        np.add.at(sums[n], inv, 1)
        for g, k in enumerate(uk.tolist()):
            st = acc.setdefault(k, [0] * (n + 1))
            for a in range(n + 1):
                st[a] += int(sums[a, g])
    return _emit(table, acc)


# --------------------------------------------------------------------- #
# wrong models: what a subtly broken kernel would return                 #
# --------------------------------------------------------------------- #
WRONG_MODELS = {
    "a": "a FILTER also gates the count",
    "b": "a FILTER gates the next aggregate too",
    "c": "the last run of every aligned 4-row quad is dropped",
    "d": "a miss keeps accumulating into the previous hit's slot",
    "e": "a row failing the row predicates breaks the run and is counted",
    "f": "own-word aggregates are read back one word off",
    "g": "a field's value is read with a width one bit short",
    "h": "range keys are indexed by key instead of key - 1",
    "i": "a pack_bits key is emitted unshifted",
    "j": "the second page overwrites the first instead of adding to it",
}
QUAD = 4


def _quads(table, pages, spec):
    """The rows that pass the row predicates, grouped by (page, aligned
    quad), as one thread of the kernel sees them."""
    out = {}
    for r in rows(table, pages, spec):
        out.setdefault((r.page, r.i // QUAD), []).append(r)
    return out.values()


def _u64(x):
    return x & ((1 << 64) - 1)


def _s64(x):
    x = _u64(x)
    return x - (1 << 64) if x >> 63 else x


def _reread(table, spec, true, f_off=0, g_short=0):
    """Pack the true totals into slot words and unpack them with a broken
    reader: own words read f_off words early, bit fields and the count read
    g_short bits short."""
    pk = spec.pack
    n = len(spec.aggs)
    npay = len(table.payloads)
    out = {}
    for k, row in true.items():
        vals = row[npay:]
        words = [_u64(vals[n] << pk.cnt_shift)]
        for a in range(n):
            if pk.shift[a] >= 0:
                words[0] = _u64(words[0] + (vals[a] << pk.shift[a]))
            else:
                words.append(_u64(vals[a]))
        got, w = [], 1
        for a in range(n):
            if pk.shift[a] >= 0:
                m = (1 << (pk.width[a] - g_short)) - 1
                got.append((words[0] >> pk.shift[a]) & m)
            else:
                got.append(_s64(words[w - f_off]))
                w += 1
        cnt = (words[0] >> pk.cnt_shift) & \
            ((1 << (pk.cnt_width - g_short)) - 1)
        if cnt:
            out[k] = row[:npay] + tuple(got) + (cnt,)
    return out


def wrong_model(bug, table, pages, spec):
    """The output of the kernel if it had the named bug.  A bug that does
    not apply to the input (no FILTER, no own word, ...) returns the
    reference's output."""
    assert bug in WRONG_MODELS
    n = len(spec.aggs)
    true = multi_agg_ref(table, pages, spec)
    acc = {}
    if bug == "a":
        for r in rows(table, pages, spec):
            if r.payload is not None:
                _add(acc, n, r.key, r.contrib,
                     count=int(all(c is not None for c in r.contrib)))
        return _emit(table, acc)
    if bug == "b":
        for r in rows(table, pages, spec):
            if r.payload is None:
                continue
            c = [None if a and r.contrib[a - 1] is None else r.contrib[a]
                 for a in range(n)]
            _add(acc, n, r.key, c)
        return _emit(table, acc)
    if bug == "c":
        for quad in _quads(table, pages, spec):
            last = len(quad) - 1
            while last > 0 and quad[last - 1].key == quad[last].key:
                last -= 1
            for r in quad[:last]:
                if r.payload is not None:
                    _add(acc, n, r.key, r.contrib)
        return _emit(table, acc)
    if bug == "d":
        for quad in _quads(table, pages, spec):
            prev = None
            for r in quad:
                if r.payload is not None:
                    prev = r.key
                if prev is not None:
                    _add(acc, n, prev, r.contrib)
        return _emit(table, acc)
    if bug == "e":
        for r in rows(table, pages, spec, with_failed=True):
            if r.payload is not None:
                _add(acc, n, r.key, r.contrib if r.passed else [None] * n)
        return _emit(table, acc)
    if bug == "f":
        if spec.pack is None or all(s >= 0 for s in spec.pack.shift[:n]):
            return true
        return _reread(table, spec, true, f_off=1)
    if bug == "g":
        return true if spec.pack is None else \
            _reread(table, spec, true, g_short=1)
    if bug == "h":
        if table.kind != "range":
            return true
        for r in rows(table, pages, spec):
            if 0 <= r.key <= table.K - 1:
                _add(acc, n, r.key + 1, r.contrib)
        return _emit(table, acc)
    if bug == "i":
        if not table.pack_bits:
            return true
        return {(k << table.pack_bits) | row[0]: row
                for k, row in true.items()}
    assert bug == "j"
    for pno in range(len(pages)):
        acc.update(multi_agg_ref(table, pages[pno:pno + 1], spec))
    return acc


# --------------------------------------------------------------------- #
# datasets of tests/test_gpu_multi_agg.py                                #
# --------------------------------------------------------------------- #
N_RUN = 1025          # one row past a block of the probe (256 x 4 rows)
N_DOM = 50            # group domain 1..N_DOM of the small cases


def small_tables():
    """The two shapes of the same domain 1..N_DOM: an agg_table built from
    the keys in a scrambled order, and range_group(N_DOM)."""
    keys = np.random.RandomState(7).permutation(N_DOM) + 1
    return {"hash": hash_table(keys), "range": range_table(N_DOM)}


def _values(n, seed):
    """v: distinct positive values, so losing or doubling any one row
    changes a sum; f: the 0/1 column of the FILTER; p: the 0/1 column of
    the row predicate (all 1 unless a pattern clears it)."""
    rng = np.random.RandomState(seed)
    return {"v": (1000 + 3 * np.arange(n)).astype(np.int64),
            "w": rng.randint(-99, 100, n).astype(np.int32),
            "f": rng.randint(0, 2, n).astype(np.uint8),
            "p": np.ones(n, np.uint8)}


RUN_SPEC = Spec("k",
                aggs=(Agg("sum_i64", "v"), Agg("sum_i64", "w", filt=1),
                      Agg("count")),
                preds=(Pred("p", "eq", 1),), filters=(Pred("f", "eq", 1),))


def _cycle_keys(n, lo=1, hi=N_DOM):
    """Sorted keys with run lengths cycling 1..9."""
    out, k, length = [], lo, 1
    while len(out) < n:
        out += [k] * length
        k = lo if k == hi else k + 1
        length = length % 9 + 1
    return np.array(out[:n], np.int64)


def run_pattern(name, n=N_RUN):
    """Key column and row-predicate column of one run pattern; N_DOM + 1,
    N_DOM + 2 and 0 are misses on both table shapes."""
    i = np.arange(n)
    p = np.ones(n, np.uint8)
    if name == "one_key":
        k = np.full(n, 17)
    elif name == "cycle_1_9":
        k = _cycle_keys(n)
    elif name == "abab":
        k = np.where(i % 2 == 0, 3, 4) + 2 * (i // 6 % 5)
    elif name == "a_miss_a":
        # A M A  B M B ...: three rows a group, so the miss takes every
        # position of the quad in turn
        k = np.where(i % 3 == 1, N_DOM + 1 + i % 2, 1 + i // 3 % N_DOM)
    elif name == "a_failed_a":
        # A, a row of another (present) key that fails the row predicate, A
        k = np.where(i % 3 == 1, 1 + (i // 3 + 7) % N_DOM,
                     1 + i // 3 % N_DOM)
        p = (i % 3 != 1).astype(np.uint8)
    elif name == "zero_first":
        # every quad starts with key 0 (the kernel's initial cur_key): a
        # miss, then a run of 1s or 2s
        k = np.where(i % 4 == 0, 0, 1 + i // 4 % 2)
    elif name == "long_run_one_miss":
        k = np.full(n, 9)
        k[501] = N_DOM + 1
    else:
        raise KeyError(name)
    return k.astype(np.int64), p


RUN_PATTERNS = {
    # name -> the wrong models the pattern must see
    "one_key": "abch",
    "cycle_1_9": "abch",
    "abab": "abch",
    "a_miss_a": "abcdh",
    "a_failed_a": "abceh",
    "zero_first": "abch",
    "long_run_one_miss": "abcdh",
}


def run_case(name, shape, n=N_RUN):
    k, p = run_pattern(name, n)
    cols = {"k": k, **_values(n, 11)}
    cols["p"] = p
    sees = RUN_PATTERNS[name]
    if shape != "range":
        sees = sees.replace("h", "")
    return Case(small_tables()[shape], (Page(cols),), RUN_SPEC, sees)


SWEEP_NS = (0, 1, 3, 4, 5, 1023, 1024, 1025)


def sweep_case(n):
    """The first n rows of the 1..9 cycle on the hashed table: every row
    hits, so a lost tail row is a wrong sum."""
    c = run_case("cycle_1_9", "hash")
    return c._replace(pages=(c.pages[0].rows(0, n),),
                      sees=c.sees if n == N_RUN else "")


def pass_case(n):
    """The one long page (the test passes one grid pass + 5 rows): sorted
    I64 keys in runs of about n / 1000 rows, every seventh key absent from
    the table, a U8 and an I32 value column."""
    keys = np.arange(n, dtype=np.int64) * 1000 // n + 1
    present = [k for k in range(1, 1001) if k % 7]
    rng = np.random.RandomState(3)
    cols = {"k": keys, "b": rng.randint(0, 256, n).astype(np.uint8),
            "w": rng.randint(-1000, 1000, n).astype(np.int32)}
    spec = Spec("k", aggs=(Agg("sum_i64", "b"),
                           Agg("sum_i64", "w", filt=0), Agg("count")),
                filters=(Pred("b", "lt", 100),))
    return Case(hash_table(present), (Page(cols),), spec, "abc")


def _filter_page(n=300):
    from edge_refs import ticks_exact
    rng = np.random.RandomState(23)
    i = np.arange(n)
    x, tx = ticks_exact(rng.randint(-50000, 50000, n), 2)
    m_null = (rng.rand(n) < 0.3).astype(np.uint8)
    a = rng.randint(0, 40, n).astype(np.int64)
    k = _cycle_keys(n, 1, 12)
    a[k == 5] = 3      # group 5: the filter a > 10 rejects every row
    return Page({"k": k, "a": a,
                 "b": rng.randint(-5, 6, n).astype(np.int32),
                 "x": x, "m": rng.randint(0, 10, n).astype(np.int64),
                 "p": (i % 5 != 2).astype(np.uint8),
                 "y": rng.rand(n)},
                nulls={"m": m_null}, ticks={"x": tx})


def filter_cases():
    """name -> Case.  six_filtered: n_aggs = 6, every aggregate behind a
    FILTER of its own; agg_filter[5] = 0 names the row predicate."""
    tbl = hash_table(range(1, 11))        # keys 11, 12 of the page miss
    pg = _filter_page()
    six = Spec("k", preds=(Pred("p", "eq", 1),),
               filters=(Pred("a", "gt", 10), Pred("b", "le", 3),
                        Pred("y", "lt", 0.5), Pred("m", "ge", 5),
                        Pred("m", "is_null")),
               aggs=(Agg("sum_i64", "a", filt=1),
                     Agg("sum_i64", "b", filt=2),
                     Agg("sum_dec", "x", filt=3, scale=2),
                     Agg("count", filt=4),
                     Agg("sum_i64", "m", filt=5),
                     Agg("sum_dec", "x", filt=0, scale=2)))
    return {
        "six_filtered": Case(tbl, (pg,), six, "abce"),
        "one_unfiltered": Case(tbl, (pg,), Spec(
            "k", aggs=(Agg("sum_dec", "x", scale=2),)), "c"),
        "counts": Case(tbl, (pg,), Spec(
            "k", aggs=(Agg("count"), Agg("count", filt=0),
                       Agg("count", filt=1)),
            filters=(Pred("m", "not_null"), Pred("a", "gt", 10))), "abc"),
    }


# ---- table shapes ----------------------------------------------------- #
K_SHAPE = 1000


def shape_tables():
    """Five device shapes.  The hashed ones share 300 build keys of
    1..K_SHAPE, 1 and K_SHAPE among them; the range table's domain is all
    of 1..K_SHAPE."""
    rng = np.random.RandomState(31)
    keys = np.r_[1, K_SHAPE, rng.permutation(K_SHAPE - 2)[:298] + 2]
    keys = keys[rng.permutation(len(keys))]
    p32 = (keys * 3 - 1500).astype(np.int32)
    p64 = keys.astype(np.int64) * (1 << 40) - 7
    p8 = (keys % 256).astype(np.uint8)
    p8[keys == K_SHAPE] = 255
    p8[keys == 1] = 0
    return {
        "payload_i32_i64": hash_table(keys, (p32, p64)),
        "pack_bits_8": hash_table(keys, (p8,), pack_bits=8),
        "fill_x10_13": hash_table(keys, fill_x10=13),
        "bitmap": hash_table(keys, bitmap_max_key=K_SHAPE),
        "range": range_table(K_SHAPE),
    }


SHAPE_SPEC = Spec("k", aggs=(Agg("sum_i64", "v"), Agg("count", filt=0),
                             Agg("sum_i64", "w")),
                  filters=(Pred("f", "eq", 1),))


def _shape_page(keys):
    keys = np.asarray(keys, np.int64)
    return Page({"k": keys, **_values(len(keys), 37)})


def shape_pages(shape):
    """name -> probe page, the same for every shape but for INT64_MIN,
    which only the range probe takes (the hashed tables reserve it)."""
    rng = np.random.RandomState(41)
    edge = [1, K_SHAPE, K_SHAPE + 1, 0, -1, I64_MAX, K_SHAPE, 1, 2,
            K_SHAPE - 1]
    if shape == "range":
        edge.append(I64_MIN)
    body = np.sort(rng.randint(-3, K_SHAPE + 40, 600))
    return {
        "mixed": _shape_page(np.r_[edge, body, edge[::-1]]),
        "only_key_1": _shape_page([0, 1, K_SHAPE + 1, -1, 1, 0, 1]),
        "only_key_K": _shape_page([K_SHAPE + 1, K_SHAPE, 0, K_SHAPE,
                                   K_SHAPE + 2]),
        "all_K": _shape_page(np.r_[np.arange(1, K_SHAPE + 1),
                                   np.arange(K_SHAPE, 0, -3)]),
        "all_miss": _shape_page([0, -1, K_SHAPE + 1, I64_MAX, 0, 0,
                                 K_SHAPE + 7, -K_SHAPE]),
    }


def shape_case(shape, page):
    sees = {"mixed": "abc", "only_key_1": "c", "only_key_K": "c",
            "all_K": "abc", "all_miss": ""}[page]
    if shape == "range" and page != "all_miss":
        sees += "h"
    if shape == "pack_bits_8" and page != "all_miss":
        sees += "i"
    return Case(shape_tables()[shape], (shape_pages(shape)[page],),
                SHAPE_SPEC, sees)


# ---- packed layouts --------------------------------------------------- #
def _pack_page(rows):
    """rows: (key, u0, u1, u2, u3, s0, s1, s2, s3).  u*: the non-negative
    columns bit fields sum, s*: the signed ones own words sum."""
    a = np.array(rows, dtype=object).reshape(-1, 9)
    cols = {"k": a[:, 0].astype(np.int64)}
    for j in range(4):
        cols[f"u{j}"] = a[:, 1 + j].astype(np.int64)
    for j in range(4):
        cols[f"s{j}"] = a[:, 5 + j].astype(np.int64)
    return Page(cols)


def _split(total, parts):
    """`parts` non-negative ints that sum to total, no two alike where
    that is possible."""
    out = [total * (j + 1) // (parts * (parts + 1) // 2) for j in range(parts)]
    out[-1] += total - sum(out)
    assert sum(out) == total and min(out) >= 0
    return out


def pack_layouts():
    """name -> (Pack, n_aggs).  Aggregate a sums column u<a> when it is a
    bit field and s<a> when it is an own word."""
    return {
        # the "<= 7 lineitems per order" shape: adjacent from bit 0
        "w5_w7_w13_cnt3": (Pack((0, 5, 12), (5, 7, 13), 25, 3), 3),
        "top_field_ends_at_64": (Pack((0, 44, 10), (6, 20, 9), 19, 3), 3),
        "cnt_at_bit_0": (Pack((3, 20, 40), (5, 7, 13), 0, 3), 3),
        "own_first": (Pack((-1, 0, 5, 12), (0, 5, 7, 13), 25, 3), 4),
        "own_middle": (Pack((0, 5, -1, 12), (5, 7, 0, 13), 25, 3), 4),
        "own_last": (Pack((0, 5, 12, -1), (5, 7, 13, 0), 25, 3), 4),
        "own_two": (Pack((-1, 0, -1, 5), (0, 5, 0, 7), 12, 3), 4),
        "all_own": (Pack((-1, -1, -1), (0, 0, 0), 0, 3), 3),
    }


def pack_spec(layout, packed=True):
    pk, n = pack_layouts()[layout]
    aggs = tuple(Agg("sum_i64", f"u{a}" if pk.shift[a] >= 0 else f"s{a}")
                 for a in range(n))
    return Spec("k", aggs=aggs, pack=pk if packed else None)


def pack_case(layout, shape, packed=True):
    """Group 20 has 7 rows (the count field's capacity) that drive every
    bit field to exactly 2^w - 1; its neighbours 19 and 21 have the same
    7 rows of zeros in the bit-field columns; own-word columns carry mixed
    signs, one group of them around +-2^61.  Keys 18..23 sit in adjacent
    slots of the range table."""
    pk, n = pack_layouts()[layout]
    spec = pack_spec(layout, packed)
    full = [_split((1 << pk.width[a]) - 1, 7) if pk.shift[a] >= 0
            else [0] * 7 for a in range(n)] + [[0] * 7] * (4 - n)
    big = 1 << 60

    def round_(r):
        s = [(-1) ** r * (big + r), -5 + r, 3 - 2 * r, (r - 3) * 10 ** 9 + 1]
        return [(19, 0, 0, 0, 0, *[-v for v in s]),
                (20, *[full[a][r] for a in range(4)], *s),
                (21, 0, 0, 0, 0, *s[::-1]),
                (51 + r, 1, 1, 1, 1, 9, 9, 9, 9)]           # a miss

    # rounds 0..3 sorted by key (runs of four), rounds 4..6 interleaved
    rows = sorted((row for r in range(4) for row in round_(r)),
                  key=lambda row: row[0])
    rows += [(18, 1, 2, 3, 4, -1, -2, -3, -4)]
    for r in range(4, 7):
        rows += round_(r)
    rows += [(23, 31, 0, 1, 0, 7, 7, 7, 7), (22, 0, 0, 0, 0, 0, 0, 0, 0)]
    has_own = any(s < 0 for s in pk.shift[:n])
    sees = "c" + ("g" if packed else "") + \
        ("f" if packed and has_own else "")
    if shape == "range":
        sees += "h"
    return Case(small_tables()[shape], (_pack_page(rows),), spec, sees)


def pack_raise_case(name, shape):
    """The packed must-raise inputs and the clean companion."""
    w = 7
    pk = Pack((0, 5, -1), (5, w, 0), 12, 3)
    spec = Spec("k", aggs=(Agg("sum_i64", "u0"), Agg("sum_i64", "u1"),
                           Agg("sum_i64", "s2")), pack=pk)
    u1, s2, expect = [3, 4, 5, 6], [1, -2, 3, -4], "overflow"
    if name == "exactly_2_pow_w":
        u1[2] = 1 << w
    elif name == "2_pow_w_minus_1":
        u1[2], expect = (1 << w) - 1, "clean"
    elif name == "isolated_negative":
        u1[2] = -1
    elif name == "own_word_past_int64":
        s2 = [1 << 62, (1 << 62) - 1, 1, 5]
    else:
        raise KeyError(name)
    # rows 0, 1: group 7; row 2: group 9 alone between other keys; row 3
    # adds to group 7 again
    cols = {"k": np.array([7, 7, 9, 7], np.int64),
            "u0": np.array([1, 2, 3, 4], np.int64),
            "u1": np.array(u1, np.int64), "s2": np.array(s2, np.int64)}
    if name == "own_word_past_int64":
        cols["k"][:] = 7
    return Case(small_tables()[shape], (Page(cols),), spec, "",
                expect)


PACK_RAISE = ("exactly_2_pow_w", "isolated_negative", "own_word_past_int64")


# ---- unpacked overflow ------------------------------------------------ #
OVF_SPEC = Spec("k", aggs=(Agg("sum_i64", "v"), Agg("count")))
BIG = (1 << 62) + 1


def overflow_case(name):
    """Two rows of 2^62 + 1 on key 5 among rows of 1: in one quad (the
    in-run check), 1024 rows apart (two blocks: the atomic's check), in
    two pages."""
    n = 1100
    k = _cycle_keys(n, 1, 9)
    v = np.ones(n, np.int64)
    at = {"one_quad": (4, 5), "blocks_apart": (4, 1028),
          "two_pages": (4, 1028)}[name]
    k[list(at)] = 5
    k[[6, 7]] = 5          # rows 4..7: one aligned quad of key 5
    v[list(at)] = BIG
    pg = Page({"k": k, "v": v})
    pages = (pg.rows(0, 600), pg.rows(600, n)) if name == "two_pages" \
        else (pg,)
    return Case(small_tables()["hash"], pages, OVF_SPEC, "", "overflow")


def overflow_clean_case():
    """+2^62 and -2^62 patterns whose sum of |addends| stays under 2^63:
    group 1 = 2^62, group 2 = -2^62, group 3 = 2^62 - (2^62 - 1) = 1,
    group 4 = 2^62 + (2^62 - 1) = INT64_MAX, group 5 the same 1024 rows
    apart, group 6 = -(2^62) - (2^62 - 1) = INT64_MIN + 1."""
    h = 1 << 62
    n = 1100
    k = np.full(n, N_DOM + 1, np.int64)      # misses
    v = np.full(n, 7, np.int64)
    put = [(0, 1, h), (1, 2, -h), (4, 3, h), (5, 3, -(h - 1)),
           (8, 4, h), (9, 4, h - 1), (12, 5, h), (1036, 5, h - 1),
           (16, 6, -h), (18, 6, -(h - 1))]
    for i, kk, vv in put:
        k[i], v[i] = kk, vv
    return Case(small_tables()["hash"], (Page({"k": k, "v": v}),),
                OVF_SPEC, "d")


# ---- pages and operators ---------------------------------------------- #
def accumulate_case(shape, packed):
    """Two pages that share most of their groups; page 2 also brings a new
    one.  Packed: the fields of group 20 are full only after both pages."""
    c = pack_case("own_middle", shape, packed)
    pg = c.pages[0]
    h = pg.n // 2 + 1
    return c._replace(pages=(pg.rows(0, h), pg.rows(h, pg.n)),
                      sees=c.sees + "j")


# ---- the registry the CPU tests walk ---------------------------------- #
def all_cases():
    """name -> Case, every dataset generator of the GPU tests at the
    parameters they use (the long page at a reduced length)."""
    out = {}
    for n in SWEEP_NS:
        out[f"sweep[{n}]"] = sweep_case(n)
    out["pass[4099]"] = pass_case(4099)
    for shape in ("hash", "range"):
        for name in RUN_PATTERNS:
            out[f"run[{name}-{shape}]"] = run_case(name, shape)
        for layout in pack_layouts():
            for packed in (True, False):
                out[f"pack[{layout}-{shape}-{packed}]"] = \
                    pack_case(layout, shape, packed)
        for name in PACK_RAISE + ("2_pow_w_minus_1",):
            out[f"pack_raise[{name}-{shape}]"] = pack_raise_case(name, shape)
        for packed in (True, False):
            out[f"accumulate[{shape}-{packed}]"] = \
                accumulate_case(shape, packed)
    for name, c in filter_cases().items():
        out[f"filter[{name}]"] = c
    for shape in shape_tables():
        for page in shape_pages(shape):
            out[f"shape[{shape}-{page}]"] = shape_case(shape, page)
    for name in ("one_quad", "blocks_apart", "two_pages"):
        out[f"overflow[{name}]"] = overflow_case(name)
    out["overflow[clean]"] = overflow_clean_case()
    return out
