"""The staged multi-row insert kernel of the direct agg_table build
(k_tbl_insert_staged) against a numpy reference and against the generic
k_tbl_insert_direct as a second witness.

Table content is read back through a mode-1 dec_only probe that asks for
every build key once (plus keys that were never built), so the number of
groups that come back IS the inserted count.  pg_build_staged_launches()
pins which kernel a page went to, so no parity here is vacuous.

Tile edges: a thread owns R = 4 consecutive rows, a block 256 threads =
1024 rows, the grid at most 4096 blocks.
"""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

R = 4
BLOCK = 256
GRID = 4096
Q3_DATE = 9204
OPS = {
    "LT": np.less, "LE": np.less_equal, "GT": np.greater,
    "GE": np.greater_equal, "EQ": np.equal, "NE": np.not_equal,
}


@pytest.fixture(scope="module")
def P():
    import presto_amd
    return presto_amd


def _launches(P):
    f = P.lib().c.pg_build_staged_launches
    f.restype = C.c_int64
    return f()


@contextlib.contextmanager
def _generic_only():
    os.environ["PG_BUILD_STAGED"] = "0"
    try:
        yield
    finally:
        del os.environ["PG_BUILD_STAGED"]


def _cmp(P, name):
    return getattr(P, "CMP_" + name)


def _dense_flags(P, n_keys, member):
    """Flag set over keys 1..n_keys; member[i] says whether key i+1 is in."""
    page = P.Page({"ck": np.arange(1, n_keys + 1, dtype=np.int64),
                   "m": member.astype(np.int32)})
    b = P.Operator(P.OP_HASH_BUILD, P.plans.flag_set(
        0, n_keys, preds=[P.plans.pred(1, P.CMP_EQ, 1)]))
    b.add_input(page)
    b.finish()
    return b


def _dense_u8(P, n_keys, values):
    page = P.Page({"ck": np.arange(1, n_keys + 1, dtype=np.int64),
                   "v": values.astype(np.uint8)})
    b = P.Operator(P.OP_HASH_BUILD, P.plans.hash_build(
        0, payload=[1], capacity_hint=n_keys, dense_array=1))
    b.add_input(page)
    b.finish()
    return b


def _free(P, *ops):
    for op in ops:
        P.lib().c.pg_table_destroy(op.table())
        op.destroy()


def _build_and_probe(P, pages, probe, **plan):
    """Feed the pages to one agg_table build, then read the table through
    a grouped probe.  Returns (sorted groups, staged launches)."""
    before = _launches(P)
    b = P.Operator(P.OP_HASH_BUILD,
                   P.plans.hash_build(0, agg_table=1, **plan))
    try:
        for pg in pages:
            b.add_input(pg)
        staged = _launches(P) - before
        b.finish()
    except BaseException:
        b.destroy()
        raise
    pk, pv = probe
    j = P.Operator(P.OP_LOOKUP_JOIN, P.plans.agg_join(
        b.table(), 0, P.plans.ident(1), 0, dec_only=1))
    j.add_input(P.Page({"k": pk, "v": pv}))
    j.finish()
    out = j.get_output(["key", "pay", "sum", "f64", "cnt"])
    j.destroy()
    _free(P, b)
    if out is None:
        out = {nm: np.zeros(0, np.int64) for nm in ("key", "pay", "sum",
                                                     "cnt")}
    order = np.argsort(out["key"], kind="stable")
    return ({nm: np.asarray(out[nm])[order].astype(np.int64)
             for nm in ("key", "pay", "sum", "cnt")}, staged)


def _expected(keys, pays, keep, probe):
    """Reference table {key: payload} of the kept rows and the grouped
    sums of the probe over it, as sorted arrays."""
    k, p = keys[keep], pays[keep].astype(np.int64)
    uk, first = np.unique(k, return_index=True)
    up = p[first]
    # duplicates must be exact (same key, same payload)
    assert np.array_equal(up[np.searchsorted(uk, k)], p)
    pk, pv = probe
    hit = np.isin(pk, uk)
    idx = np.searchsorted(uk, pk[hit])
    # probe values are below 1000: the float64 weights stay exact
    sums = np.bincount(idx, weights=pv[hit],
                       minlength=len(uk)).astype(np.int64)
    cnts = np.bincount(idx, minlength=len(uk)).astype(np.int64)
    got = cnts > 0
    return {"key": uk[got], "pay": up[got], "sum": sums[got],
            "cnt": cnts[got]}


def _probe_for(rng, keys, extra_misses):
    """Every build key once, in random order, plus keys never built."""
    pk = np.concatenate([np.unique(keys), extra_misses]).astype(np.int64)
    pk = pk[rng.permutation(len(pk))]
    pv = rng.randint(1, 1000, len(pk)).astype(np.int64)
    return pk, pv


def _same(a, b):
    for nm in ("key", "pay", "sum", "cnt"):
        assert np.array_equal(a[nm], b[nm]), nm


def _both_paths(P, pages, probe, exp, staged_pages, **plan):
    """Default path (must send staged_pages pages to the staged kernel),
    the generic kernel alone, and the reference agree."""
    got, staged = _build_and_probe(P, pages, probe, **plan)
    assert staged == staged_pages
    with _generic_only():
        gen, staged0 = _build_and_probe(P, pages, probe, **plan)
    assert staged0 == 0
    _same(got, exp)
    _same(gen, exp)
    return got


# --------------------------------------------------------------------- #
# the Q3 shape at every tile edge                                        #
# --------------------------------------------------------------------- #
def _q3_rows(rng, n, n_cust):
    keys = (rng.permutation(4 * n + 8)[:n] + 1).astype(np.int64)
    dates = rng.randint(Q3_DATE - 1000, Q3_DATE + 1000, n).astype(np.int32)
    cust = rng.randint(1, n_cust + 1, n).astype(np.int64)
    return keys, dates, cust


@pytest.mark.parametrize("n", [0, 1, 3, 4, 5, 255, 256, 257, 1023, 1024,
                               1025, GRID * BLOCK * R + 5])
def test_q3_shape_row_counts(P, n):
    """Date filter + dense flag semijoin + payload = the predicate column,
    pack_bits 16 and a key bitmap, at the per-thread (R) and per-block
    (256 x R) tile edges and just over one full grid stride, where the
    second loop iteration and its scalar tail both run."""
    rng = np.random.RandomState(1000 + n % 997)
    n_cust = 97
    member = rng.randint(0, 5, n_cust) == 0
    member[:2] = True
    keys, dates, cust = _q3_rows(rng, n, n_cust)
    keep = (dates < Q3_DATE) & member[cust - 1]
    probe = _probe_for(rng, keys, np.array([4 * n + 100, 4 * n + 101]))
    exp = _expected(keys, dates, keep, probe)
    flags = _dense_flags(P, n_cust, member)
    try:
        _both_paths(
            P, [P.Page({"k": keys, "d": dates, "c": cust})], probe, exp, 1,
            preds=[P.plans.pred(1, P.CMP_LT, Q3_DATE)], payload=[1],
            semijoin_table=flags.table(), semijoin_col=2,
            capacity_hint=max(n // 4, 16), pack_bits=16,
            bitmap_max_key=4 * n + 16)
    finally:
        _free(P, flags)


# --------------------------------------------------------------------- #
# predicates                                                             #
# --------------------------------------------------------------------- #
N_PRED = 2 * BLOCK * R + 3  # two block tiles and a scalar tail
PRED_CASES = {
    "LT": [("LT", 50)], "LE": [("LE", 50)], "GT": [("GT", 50)],
    "GE": [("GE", 50)], "EQ": [("EQ", 50)], "NE": [("NE", 50)],
    "window": [("GE", 30), ("LT", 70)],   # the Q5 shape
    "none": [],
    "all_pass": [("GE", -20)],
    "none_pass": [("GT", 1000)],
}


@pytest.mark.parametrize("case", list(PRED_CASES))
@pytest.mark.parametrize("pay_dtype", [np.int32, np.uint8, np.int64])
def test_predicates_and_payload_types(P, case, pay_dtype):
    """Each comparison operator on an I32 column, a two-sided window, no
    predicate, all rows and no row passing; the payload is a column of
    its own of each admitted type; no semijoin."""
    rng = np.random.RandomState(7)
    n = N_PRED
    keys = (rng.permutation(3 * n)[:n] + 1).astype(np.int64)
    # negative values too: the comparison is signed
    d = rng.randint(-20, 101, n).astype(np.int32)
    d[:8] = 50
    pay = rng.randint(0, 256, n).astype(pay_dtype)
    keep = np.ones(n, bool)
    for op, val in PRED_CASES[case]:
        keep &= OPS[op](d.astype(np.int64), val)
    probe = _probe_for(rng, keys, np.array([3 * n + 7]))
    exp = _expected(keys, pay, keep, probe)
    if case == "none_pass":
        assert len(exp["key"]) == 0
    if case in ("none", "all_pass"):
        assert len(exp["key"]) == n
    _both_paths(
        P, [P.Page({"k": keys, "d": d, "p": pay})], probe, exp, 1,
        preds=[P.plans.pred(1, _cmp(P, op), val)
               for op, val in PRED_CASES[case]],
        payload=[2], capacity_hint=n, pack_bits=8, bitmap_max_key=3 * n)


# --------------------------------------------------------------------- #
# dense semijoin / lookup keys at and past the ends of the dense range   #
# --------------------------------------------------------------------- #
def _edge_cust(rng, n, n_cust):
    cust = rng.randint(1, n_cust + 1, n).astype(np.int64)
    # out-of-range keys in the vector body, at a block edge and in the tail
    for at in (0, 5, BLOCK * R - 1, BLOCK * R, n - 1):
        cust[at] = 0
        cust[at + 1 if at + 1 < n else at - 1] = -1
    cust[10:14] = [n_cust, n_cust + 1, -(1 << 40), 1 << 40]
    cust[n - 3] = n_cust + 1
    cust[n - 2] = n_cust
    return cust


def test_semijoin_edge_keys_are_dropped(P):
    """Semijoin keys 0, -1, n and n + 1 against a dense flag set over
    1..n: n is looked up, the others are dropped without a read."""
    rng = np.random.RandomState(11)
    n, n_cust = BLOCK * R + 7, 64
    member = rng.randint(0, 2, n_cust) == 0
    member[n_cust - 1] = True
    keys = (rng.permutation(2 * n)[:n] + 1).astype(np.int64)
    d = rng.randint(0, 100, n).astype(np.int32)
    cust = _edge_cust(rng, n, n_cust)
    inr = (cust >= 1) & (cust <= n_cust)
    keep = inr.copy()
    keep[inr] = member[cust[inr] - 1]
    assert keep[12 - 2] and not keep[11] and keep[n - 2]
    probe = _probe_for(rng, keys, np.array([2 * n + 9]))
    exp = _expected(keys, d, keep, probe)
    flags = _dense_flags(P, n_cust, member)
    try:
        _both_paths(
            P, [P.Page({"k": keys, "d": d, "c": cust})], probe, exp, 1,
            payload=[1], semijoin_table=flags.table(), semijoin_col=2,
            capacity_hint=n, pack_bits=8, bitmap_max_key=2 * n)
    finally:
        _free(P, flags)


def test_lookup_edge_keys_are_dropped(P):
    """The same edge keys for the fused dense u8 payload lookup (the Q5
    shape, with its date window): misses drop the row."""
    rng = np.random.RandomState(12)
    n, n_cust = BLOCK * R + 7, 64
    nation = rng.randint(0, 25, n_cust)
    keys = (rng.permutation(2 * n)[:n] + 1).astype(np.int64)
    d = rng.randint(0, 100, n).astype(np.int32)
    cust = _edge_cust(rng, n, n_cust)
    inr = (cust >= 1) & (cust <= n_cust)
    keep = inr & (d >= 20) & (d < 80)
    pay = np.zeros(n, np.int64)
    pay[inr] = nation[cust[inr] - 1]
    probe = _probe_for(rng, keys, np.array([2 * n + 9]))
    exp = _expected(keys, pay, keep, probe)
    lut = _dense_u8(P, n_cust, nation)
    try:
        _both_paths(
            P, [P.Page({"k": keys, "d": d, "c": cust})], probe, exp, 1,
            preds=[P.plans.pred(1, P.CMP_GE, 20),
                   P.plans.pred(1, P.CMP_LT, 80)],
            payload=[0], payload_lookup_table=lut.table(),
            payload_lookup_key_col=2, capacity_hint=n, pack_bits=8,
            bitmap_max_key=2 * n)
    finally:
        _free(P, lut)


# --------------------------------------------------------------------- #
# packing and bitmap ranges, capacity                                    #
# --------------------------------------------------------------------- #
PBITS = 6
BMAX = 5000


def _limits_page(P, key_at=None, pay_at=None):
    n = BLOCK * R + 2
    keys = np.arange(2, n + 2, dtype=np.int64)
    pay = (np.arange(n) % (1 << PBITS)).astype(np.int64)
    keys[0], keys[n - 1] = 1, BMAX                  # both ends accepted
    pay[3], pay[n - 2] = (1 << PBITS) - 1, (1 << PBITS) - 1
    for at, v in (key_at or {}).items():
        keys[at] = v
    for at, v in (pay_at or {}).items():
        pay[at] = v
    return keys, pay, P.Page({"k": keys, "p": pay})


def test_range_limits_accepted(P):
    """Key 1, key = bitmap_max_key and payload 2^pack_bits - 1 go in; an
    exact duplicate row (same key and payload) is idempotent."""
    rng = np.random.RandomState(13)
    keys, pay, _ = _limits_page(P)
    keys = np.concatenate([keys, keys[:9]])
    pay = np.concatenate([pay, pay[:9]])
    probe = _probe_for(rng, keys, np.array([BMAX + 1, 0, -1]))
    exp = _expected(keys, pay, np.ones(len(keys), bool), probe)
    assert exp["key"][0] == 1 and exp["key"][-1] == BMAX
    assert len(exp["key"]) == len(keys) - 9
    _both_paths(P, [P.Page({"k": keys, "p": pay})], probe, exp, 1,
                payload=[1], capacity_hint=len(keys), pack_bits=PBITS,
                bitmap_max_key=BMAX)


@pytest.mark.parametrize("what,at,value,err", [
    ("key", 6, 0, "bitmap_max_key violated"),
    ("key", BLOCK * R + 1, BMAX + 1, "bitmap_max_key violated"),
    # a negative key fails the pack range (0 <= key < 2^(63-pack_bits))
    # before the bitmap range is looked at, in the generic kernel as here
    ("key", 6, -7, "pack_bits violated"),
    ("pay", 6, 1 << PBITS, "pack_bits violated"),
    ("pay", BLOCK * R + 1, -1, "pack_bits violated"),
])
def test_range_violations_raise(P, what, at, value, err):
    """One offending row, in the vector body or in the scalar tail, raises
    the build's existing error at finish on both kernels."""
    _, _, page = _limits_page(P, **{what + "_at": {at: value}})

    def build():
        before = _launches(P)
        b = P.Operator(P.OP_HASH_BUILD, P.plans.hash_build(
            0, payload=[1], capacity_hint=2 * BLOCK * R, agg_table=1,
            pack_bits=PBITS, bitmap_max_key=BMAX))
        try:
            b.add_input(page)
            staged = _launches(P) - before
            with pytest.raises(RuntimeError, match=err):
                b.finish()
        finally:
            b.destroy()
        return staged

    assert build() == 1
    with _generic_only():
        assert build() == 0


def test_capacity_too_small_raises(P):
    """A capacity_hint far below the row count ends in the existing
    overflow / fill error: the probe loop gives up after mask + 1 tries."""
    n = 2 * BLOCK * R
    page = P.Page({"k": np.arange(1, n + 1, dtype=np.int64),
                   "p": np.zeros(n, np.int64)})

    def build():
        before = _launches(P)
        b = P.Operator(P.OP_HASH_BUILD, P.plans.hash_build(
            0, payload=[1], capacity_hint=16, agg_table=1, pack_bits=PBITS))
        try:
            b.add_input(page)
            staged = _launches(P) - before
            with pytest.raises(RuntimeError,
                               match="agg table overflow|fill exceeded"):
                b.finish()
        finally:
            b.destroy()
        return staged

    assert build() == 1
    with _generic_only():
        assert build() == 0


# --------------------------------------------------------------------- #
# pages                                                                  #
# --------------------------------------------------------------------- #
def test_two_pages_accumulate(P):
    """Two pages fed to one build accumulate; the second page goes through
    the same semijoin flag set as the first."""
    rng = np.random.RandomState(14)
    n, n_cust = BLOCK * R + 5, 45
    member = rng.randint(0, 2, n_cust) == 0
    keys = (rng.permutation(4 * n)[:2 * n] + 1).astype(np.int64)
    d = rng.randint(0, 100, 2 * n).astype(np.int32)
    cust = rng.randint(1, n_cust + 1, 2 * n).astype(np.int64)
    keep = (d < 60) & member[cust - 1]
    probe = _probe_for(rng, keys, np.array([4 * n + 3]))
    exp = _expected(keys, d, keep, probe)
    pages = [P.Page({"k": keys[:n], "d": d[:n], "c": cust[:n]}),
             P.Page({"k": keys[n:], "d": d[n:], "c": cust[n:]})]
    flags = _dense_flags(P, n_cust, member)
    try:
        _both_paths(P, pages, probe, exp, 2,
                    preds=[P.plans.pred(1, P.CMP_LT, 60)], payload=[1],
                    semijoin_table=flags.table(), semijoin_col=2,
                    capacity_hint=2 * n, pack_bits=8, bitmap_max_key=4 * n)
    finally:
        _free(P, flags)


def test_misaligned_key_view_gives_same_table(P):
    """A device key column that starts one element into its buffer is
    8-byte but not 16-byte aligned: the page goes to the generic kernel
    and the table is the same."""
    import torch
    rng = np.random.RandomState(15)
    n = BLOCK * R + 5
    keys = (rng.permutation(2 * n)[:n] + 1).astype(np.int64)
    d = rng.randint(0, 100, n).astype(np.int32)
    keep = d >= 40
    probe = _probe_for(rng, keys, np.array([2 * n + 3]))
    exp = _expected(keys, d, keep, probe)
    buf = torch.zeros(n + 1, dtype=torch.int64, device="cuda")
    buf[1:] = torch.from_numpy(keys).cuda()
    kview = buf[1:]
    assert kview.data_ptr() % 16 == 8
    dd = torch.from_numpy(d).cuda()
    plan = dict(preds=[P.plans.pred(1, P.CMP_GE, 40)], payload=[1],
                capacity_hint=n, pack_bits=8, bitmap_max_key=2 * n)
    got, staged = _build_and_probe(P, [P.Page({"k": kview, "d": dd})],
                                   probe, **plan)
    assert staged == 0
    _same(got, exp)
    # the same page from an aligned buffer takes the staged kernel
    kal = torch.from_numpy(keys).cuda()
    assert kal.data_ptr() % 16 == 0
    got, staged = _build_and_probe(P, [P.Page({"k": kal, "d": dd})],
                                   probe, **plan)
    assert staged == 1
    _same(got, exp)


def test_shapes_outside_the_gate_stay_generic(P):
    """A predicate column with a null mask (null rows are excluded), an
    unpacked table, an I64 predicate column, a column-to-column predicate
    and three predicates all keep the generic kernel."""
    rng = np.random.RandomState(16)
    n = BLOCK * R + 5
    keys = (rng.permutation(2 * n)[:n] + 1).astype(np.int64)
    d = rng.randint(0, 100, n).astype(np.int32)
    d2 = rng.randint(0, 100, n).astype(np.int32)
    nulls = (rng.randint(0, 4, n) == 0).astype(np.uint8)
    probe = _probe_for(rng, keys, np.array([2 * n + 3]))
    pl = P.plans
    base = dict(payload=[1], capacity_hint=n, pack_bits=8,
                bitmap_max_key=2 * n)
    lt60 = pl.pred(1, P.CMP_LT, 60)
    cases = [
        (P.Page({"k": keys, "d": d}, nulls={"d": nulls}),
         dict(base, preds=[lt60]), (d < 60) & (nulls == 0)),
        (P.Page({"k": keys, "d": d}),
         dict(base, preds=[lt60], pack_bits=0), d < 60),
        (P.Page({"k": keys, "d": d.astype(np.int64)}),
         dict(base, preds=[lt60]), d < 60),
        (P.Page({"k": keys, "d": d, "e": d2}),
         dict(base, preds=[pl.pred_cols(1, P.CMP_LT, 2)]), d < d2),
        (P.Page({"k": keys, "d": d}),
         dict(base, preds=[lt60, pl.pred(1, P.CMP_GE, 5),
                           pl.pred(1, P.CMP_NE, 33)]),
         (d < 60) & (d >= 5) & (d != 33)),
    ]
    for page, plan, keep in cases:
        got, staged = _build_and_probe(P, [page], probe, **plan)
        assert staged == 0
        _same(got, _expected(keys, d, keep, probe))


# --------------------------------------------------------------------- #
# plan level                                                             #
# --------------------------------------------------------------------- #
def test_q3_q5_pipelines_match_generic_and_oracle(P, oracle_lib):
    """pipelines.q3 and pipelines.q5 on generated TPC-H data: their orders
    builds take the staged kernel, and the results equal those of the
    generic kernel and of the CPU oracle."""
    sf = 0.05
    orders = oracle_lib.gen_orders(sf)
    ord_page = P.Page({k: orders[k] for k in
                       ("orderkey", "custkey", "orderdate")})
    # Q3
    li = oracle_lib.gen_lineitem(sf)
    cust = oracle_lib.gen_customer(sf)
    q3_pages = (
        P.Page({"custkey": cust["custkey"], "mktseg": cust["mktseg"]}),
        ord_page,
        P.Page({k: li[k] for k in
                ("quantity", "extendedprice", "discount", "tax", "shipdate",
                 "returnflag", "linestatus", "orderkey")}))
    before = _launches(P)
    got3 = P.pipelines.q3(*q3_pages, mode="dec")
    assert _launches(P) - before == 1
    with _generic_only():
        gen3 = P.pipelines.q3(*q3_pages, mode="dec")
    assert _launches(P) - before == 1
    assert sorted(got3) == sorted(gen3)
    for nm in got3:
        assert np.array_equal(got3[nm], gen3[nm]), nm
    exp3 = oracle_lib.q3(cust, orders, li)
    assert len(got3["orderkey"]) == len(exp3) == 10
    for i, r in enumerate(exp3):
        assert got3["orderkey"][i] == r.orderkey
        assert got3["revenue_1e4"][i] == r.revenue_1e4
        assert got3["orderdate"][i] == r.orderdate
    # Q5
    li2 = oracle_lib.gen_lineitem2(sf)
    cust2 = oracle_lib.gen_customer2(sf)
    supp = oracle_lib.gen_supplier(sf)
    q5_pages = (
        P.Page({"custkey": cust2["custkey"],
                "nationkey": cust2["nationkey"]}),
        ord_page,
        P.Page({"suppkey": supp["suppkey"], "nationkey": supp["nationkey"]}),
        P.Page({k: li2[k] for k in ("orderkey", "suppkey", "extendedprice",
                                    "discount")}))
    before = _launches(P)
    got5 = P.pipelines.q5(*q5_pages)
    assert _launches(P) - before == 1
    with _generic_only():
        gen5 = P.pipelines.q5(*q5_pages)
    assert _launches(P) - before == 1
    assert sorted(got5) == sorted(gen5)
    for nm in got5:
        assert np.array_equal(got5[nm], gen5[nm]), nm
    exp5 = {int(r.nationkey): int(r.revenue_1e4)
            for r in oracle_lib.q5(cust2, orders, li2, supp)}
    assert {int(got5["nationkey"][i]): int(got5["rev_lo"][i])
            for i in range(len(got5["nationkey"]))} == exp5
    assert len(exp5) == 5
