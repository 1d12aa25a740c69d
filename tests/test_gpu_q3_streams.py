"""The load scheduling of the Q3 orders build (k_tbl_insert_staged) and of
the Q3 probe (k_probe_agg_q3): every load of a stage is issued for all rows
of a thread, a dropped row's gather from a clamped index, and nothing is
read at or beyond row n of a column.  Also which tables carry byte tags.

Every column of a page under test is the first n rows of a longer device
buffer whose remaining rows are poison: they pass every filter and carry
keys of their own, so a use of data past n shows as extra groups (build) or
as extra counts and sums (probe).  PG_STAGED_GRID / PG_PROBE_GRID cap the
grids, so that a block walks several tiles or passes at a few thousand rows.

Geometry: the build gives a thread R = 4 rows and a block a tile of 1024;
the probe gives a thread Q = 2 rows per pass, a pass of the grid is
grid x 256 x Q rows.  Neither kernel prefetches across tiles or passes, so
the edges are 1, 2 and 3 tiles (passes), each exact, minus 1 and plus 1.

A numpy reference is the first witness, the generic path (PG_BUILD_STAGED=0,
PG_GROUPS_LIST=0) the second.

Not built: the issue asks for the clamped-gather test to put poison of the
opposite truth value right behind the flag / lookup bytes.  Those arrays are
allocated by the library at exactly the declared capacity and no plan takes
a caller's buffer for them, so the bytes behind them cannot be set from a
test.  The test below instead gives byte 0, the byte a dropped row's clamped
gather reads, the truth value that would keep the row.
"""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

R = 4
BLOCK = 256
TILE = BLOCK * R
Q = 2
PAD = 2 * TILE  # poison rows behind every column
Q3_DATE = 9204
EDGES = [t * TILE + d for t in (1, 2, 3) for d in (-1, 0, 1)]


@pytest.fixture(scope="module")
def P():
    import presto_amd
    return presto_amd


@contextlib.contextmanager
def _env(**kv):
    old = {k: os.environ.get(k) for k in kv}
    os.environ.update({k: str(v) for k, v in kv.items()})
    try:
        yield
    finally:
        for k, v in old.items():
            if v is None:
                del os.environ[k]
            else:
                os.environ[k] = v


def _counter(P, name):
    f = getattr(P.lib().c, name)
    f.restype = C.c_int64
    return f()


def _free(P, *ops):
    for op in ops:
        P.lib().c.pg_table_destroy(op.table())
        op.destroy()


def _views(cols, n):
    """Device buffers of the whole columns; the page sees the first n rows."""
    import torch
    bufs = {nm: torch.from_numpy(np.ascontiguousarray(v)).cuda()
            for nm, v in cols.items()}
    for b in bufs.values():
        assert b.data_ptr() % 16 == 0
    return bufs, {nm: b[:n] for nm, b in bufs.items()}


def _dense_flags(P, n_keys, member):
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


# --------------------------------------------------------------------- #
# build                                                                  #
# --------------------------------------------------------------------- #
def _read_table(P, page, probe, **plan):
    """One agg_table build of the page, read back through a dec_only
    grouped probe.  Returns (groups sorted by key, staged launches)."""
    before = _counter(P, "pg_build_staged_launches")
    b = P.Operator(P.OP_HASH_BUILD,
                   P.plans.hash_build(0, agg_table=1, **plan))
    try:
        b.add_input(page)
        staged = _counter(P, "pg_build_staged_launches") - before
        b.finish()
    except BaseException:
        b.destroy()
        raise
    pk, pv = probe
    j = P.Operator(P.OP_LOOKUP_JOIN, P.plans.agg_join(
        b.table(), 0, P.plans.ident(1), 0, dec_only=1))
    try:
        j.add_input(P.Page({"k": pk, "v": pv}))
        j.finish()
        out = j.get_output(["key", "pay", "sum", "f64", "cnt"])
    finally:
        j.destroy()
        _free(P, b)
    names = ("key", "pay", "sum", "cnt")
    if out is None:
        out = {nm: np.zeros(0, np.int64) for nm in names}
    order = np.argsort(out["key"], kind="stable")
    return ({nm: np.asarray(out[nm])[order].astype(np.int64)
             for nm in names}, staged)


def _table_ref(keys, pays, keep, probe):
    """{key: payload} of the kept rows and the grouped sums of the probe
    over it, as sorted arrays."""
    k, p = keys[keep], pays[keep].astype(np.int64)
    uk, first = np.unique(k, return_index=True)
    up = p[first]
    pk, pv = probe
    hit = np.isin(pk, uk)
    idx = np.searchsorted(uk, pk[hit])
    sums = np.bincount(idx, weights=pv[hit],
                       minlength=len(uk)).astype(np.int64)
    cnts = np.bincount(idx, minlength=len(uk)).astype(np.int64)
    got = cnts > 0
    return {"key": uk[got], "pay": up[got], "sum": sums[got],
            "cnt": cnts[got]}


def _same_table(a, b):
    for nm in ("key", "pay", "sum", "cnt"):
        assert np.array_equal(a[nm], b[nm]), nm


def _probe_all(rng, keys, misses):
    """Every key of the buffer once, poison rows' keys included, and keys
    that were never there."""
    pk = np.concatenate([np.unique(keys), misses]).astype(np.int64)
    pk = pk[rng.permutation(len(pk))]
    return pk, rng.randint(1, 1000, len(pk)).astype(np.int64)


def _staged_and_generic(P, page, probe, exp, grid, **plan):
    with _env(PG_STAGED_GRID=grid):
        got, staged = _read_table(P, page, probe, **plan)
    assert staged == 1
    with _env(PG_BUILD_STAGED=0):
        gen, staged0 = _read_table(P, page, probe, **plan)
    assert staged0 == 0
    _same_table(got, exp)
    _same_table(gen, exp)


@pytest.mark.parametrize("n", EDGES)
@pytest.mark.parametrize("grid", [1, 2])
def test_build_q3_shape_tail_poison(P, grid, n):
    """Date filter, dense flag semijoin, payload = the predicate column,
    pack_bits 16 and a bitmap; the rows past n would all be inserted."""
    rng = np.random.RandomState(100 + n)
    n_cust, tot = 97, n + PAD
    member = rng.randint(0, 3, n_cust) == 0
    member[0] = True
    keys = (rng.permutation(4 * tot)[:tot] + 1).astype(np.int64)
    dates = rng.randint(Q3_DATE - 1000, Q3_DATE + 1000, tot).astype(np.int32)
    cust = rng.randint(1, n_cust + 1, tot).astype(np.int64)
    dates[n:] = Q3_DATE - 500
    cust[n:] = 1
    keep = (dates < Q3_DATE) & member[cust - 1]
    assert keep[n:].all()
    keep[n:] = False
    probe = _probe_all(rng, keys, np.array([4 * tot + 5, 4 * tot + 6]))
    exp = _table_ref(keys, dates, keep, probe)
    assert 0 < len(exp["key"]) < n
    bufs, view = _views({"k": keys, "d": dates, "c": cust}, n)
    flags = _dense_flags(P, n_cust, member)
    try:
        _staged_and_generic(
            P, P.Page(view), probe, exp, grid,
            preds=[P.plans.pred(1, P.CMP_LT, Q3_DATE)], payload=[1],
            semijoin_table=flags.table(), semijoin_col=2,
            capacity_hint=tot, pack_bits=16, bitmap_max_key=4 * tot + 16)
    finally:
        _free(P, flags)


@pytest.mark.parametrize("n", EDGES)
@pytest.mark.parametrize("grid", [1, 2])
def test_build_q5_shape_tail_poison(P, grid, n):
    """Two-sided date window and the dense u8 payload lookup."""
    rng = np.random.RandomState(200 + n)
    n_cust, tot = 64, n + PAD
    nation = rng.randint(0, 25, n_cust)
    keys = (rng.permutation(4 * tot)[:tot] + 1).astype(np.int64)
    d = rng.randint(0, 100, tot).astype(np.int32)
    cust = rng.randint(1, n_cust + 1, tot).astype(np.int64)
    d[n:] = 50
    keep = (d >= 20) & (d < 80)
    assert keep[n:].all()
    keep[n:] = False
    probe = _probe_all(rng, keys, np.array([4 * tot + 5]))
    exp = _table_ref(keys, nation[cust - 1], keep, probe)
    assert 0 < len(exp["key"]) < n
    bufs, view = _views({"k": keys, "d": d, "c": cust}, n)
    lut = _dense_u8(P, n_cust, nation)
    try:
        _staged_and_generic(
            P, P.Page(view), probe, exp, grid,
            preds=[P.plans.pred(1, P.CMP_GE, 20),
                   P.plans.pred(1, P.CMP_LT, 80)],
            payload=[0], payload_lookup_table=lut.table(),
            payload_lookup_key_col=2, capacity_hint=tot, pack_bits=8,
            bitmap_max_key=4 * tot + 16)
    finally:
        _free(P, lut)


def _edge_keys(n_cust):
    return [0, -1, n_cust, n_cust + 1, -(1 << 40), 1 << 40]


def _edge_cust(rng, n, n_cust):
    """Each edge key in each lane position j = 0..3 of full-tile threads;
    everything else in range."""
    cust = rng.randint(1, n_cust + 1, n).astype(np.int64)
    at = 40
    for ek in _edge_keys(n_cust):
        for j in range(R):
            cust[at + j] = ek     # this thread: position j alone
            at += R
        cust[at:at + R] = ek      # and all four positions at once
        at += R
    assert at < TILE
    return cust


def test_build_semijoin_keys_outside_the_flags_are_dropped(P):
    """Semijoin keys 0, -1, n_cust + 1 and +-2^40 are dropped, n_cust is
    looked up.  Flag byte 0, which a dropped row's gather reads, is set:
    using it would keep the row."""
    rng = np.random.RandomState(21)
    n, n_cust = 2 * TILE, 64
    member = rng.randint(0, 2, n_cust) == 0
    member[0] = True
    member[n_cust - 1] = True
    keys = (rng.permutation(2 * n)[:n] + 1).astype(np.int64)
    d = rng.randint(0, 100, n).astype(np.int32)
    cust = _edge_cust(rng, n, n_cust)
    inr = (cust >= 1) & (cust <= n_cust)
    assert (~inr).sum() == 5 * 2 * R
    keep = inr.copy()
    keep[inr] = member[cust[inr] - 1]
    assert keep[cust == n_cust].all()
    probe = _probe_all(rng, keys, np.array([2 * n + 9]))
    exp = _table_ref(keys, d, keep, probe)
    flags = _dense_flags(P, n_cust, member)
    try:
        for grid in (1, 4096):
            _staged_and_generic(
                P, P.Page({"k": keys, "d": d, "c": cust}), probe, exp, grid,
                payload=[1], semijoin_table=flags.table(), semijoin_col=2,
                capacity_hint=n, pack_bits=8, bitmap_max_key=2 * n)
    finally:
        _free(P, flags)


def test_build_lookup_keys_outside_the_range_are_dropped(P):
    """The same keys for the dense u8 payload lookup, under the Q5 date
    window; rows the window drops gather from byte 0 as well."""
    rng = np.random.RandomState(22)
    n, n_cust = 2 * TILE, 64
    nation = rng.randint(1, 25, n_cust)
    keys = (rng.permutation(2 * n)[:n] + 1).astype(np.int64)
    d = rng.randint(0, 100, n).astype(np.int32)
    cust = _edge_cust(rng, n, n_cust)
    d[:TILE] = 50  # the edge rows pass the window
    inr = (cust >= 1) & (cust <= n_cust)
    keep = inr & (d >= 20) & (d < 80)
    pay = np.zeros(n, np.int64)
    pay[inr] = nation[cust[inr] - 1]
    probe = _probe_all(rng, keys, np.array([2 * n + 9]))
    exp = _table_ref(keys, pay, keep, probe)
    lut = _dense_u8(P, n_cust, nation)
    try:
        for grid in (1, 4096):
            _staged_and_generic(
                P, P.Page({"k": keys, "d": d, "c": cust}), probe, exp, grid,
                preds=[P.plans.pred(1, P.CMP_GE, 20),
                       P.plans.pred(1, P.CMP_LT, 80)],
                payload=[0], payload_lookup_table=lut.table(),
                payload_lookup_key_col=2, capacity_hint=n, pack_bits=8,
                bitmap_max_key=2 * n)
    finally:
        _free(P, lut)


# --------------------------------------------------------------------- #
# probe                                                                  #
# --------------------------------------------------------------------- #
OUT5 = ["key", "pay", "dec", "f64", "cnt"]


def _groups(P, table, plan, page):
    j = P.Operator(P.OP_LOOKUP_JOIN, plan)
    try:
        j.add_input(page)
        j.finish()
        out = j.get_output(OUT5)
    finally:
        j.destroy()
    out = out or {}
    out = {nm: np.asarray(out.get(nm, np.zeros(0, np.int64))) for nm in OUT5}
    order = np.argsort(out["key"], kind="stable")
    return {nm: out[nm][order] for nm in OUT5}


def _same_groups(got, exp):
    for nm in OUT5:
        a, b = np.asarray(got[nm]), np.asarray(exp[nm])
        assert a.shape == b.shape, (nm, a.shape, b.shape)
        if b.dtype == np.float64:
            assert np.array_equal(a.astype(np.float64).view(np.int64),
                                  b.view(np.int64)), nm
        else:
            assert np.array_equal(a.astype(np.int64), b.astype(np.int64)), nm


def _groups_ref(bkeys, bpay, pk, keep, ticks, f64, dec_only):
    order = np.argsort(bkeys)
    sk = bkeys[order]
    hit = keep & np.isin(pk, sk)
    uk, inv = np.unique(pk[hit], return_inverse=True)
    cnt = np.bincount(inv, minlength=len(uk)).astype(np.int64)
    dec = np.zeros(len(uk), np.int64)
    np.add.at(dec, inv, ticks[hit])
    fs = np.zeros(len(uk), np.float64)
    if not dec_only:
        np.add.at(fs, inv, f64[hit])
    return {"key": uk, "pay": bpay[order][np.searchsorted(sk, uk)],
            "dec": dec, "f64": fs, "cnt": cnt}


def _orders_table(P, bkeys, bpay, bmax, **plan):
    b = P.Operator(P.OP_HASH_BUILD, P.plans.hash_build(
        0, payload=[1], agg_table=1, pack_bits=16, bitmap_max_key=bmax,
        **plan))
    b.add_input(P.Page({"k": bkeys, "p": bpay}))
    b.finish()
    return b


def _q3_plan(P, table, op, dec_only):
    preds = [] if op is None else [P.plans.pred(1, op, Q3_DATE)]
    return P.plans.agg_join(table, 0, P.plans.disc_price(2, 3), dec_scale=4,
                            preds=preds, dec_only=dec_only)


@pytest.mark.parametrize("dec_only", [1, 0], ids=["dec_only", "fx128"])
@pytest.mark.parametrize("op", ["GT", "LT", None])
@pytest.mark.parametrize("grid", [1, 2])
def test_probe_tail_poison_and_keys_outside_the_bitmap(P, grid, op, dec_only):
    """n around 1, 2 and 3 passes of the capped grid.  The rows past n hit
    build keys and pass the predicate; keys 0, -7 and bmax + 1 sit in both
    row positions of a thread, in the vector body and in the last rows."""
    rng = np.random.RandomState(300 + 10 * grid + dec_only)
    nb = 600
    bmax = 4 * nb
    bkeys = (rng.permutation(bmax)[:nb] + 1).astype(np.int64)
    bkeys[:2] = [1, bmax]  # both ends of the bitmap range are keys
    bkeys = np.unique(bkeys)
    bpay = rng.randint(0, 1 << 16, len(bkeys)).astype(np.int64)
    passing = Q3_DATE + 9 if op in ("GT", None) else Q3_DATE - 9
    cmp_ = {"GT": np.greater, "LT": np.less}
    pass_rows = grid * BLOCK * Q
    for n in [p * pass_rows + d for p in (1, 2, 3) for d in (-1, 0, 1)]:
        tot = n + PAD
        # keys 1..bmax, about a quarter of them built
        pk = rng.randint(1, bmax + 1, tot).astype(np.int64)
        sd = rng.randint(Q3_DATE - 50, Q3_DATE + 50, tot).astype(np.int32)
        ep = rng.randint(1, 4000, tot) * 0.25
        dc = rng.randint(0, 3, tot) * 0.25
        at = 6
        for bad in (0, -7, bmax + 1):
            for j in range(Q):
                pk[at + j] = bad           # position j alone
                pk[n - 1 - at - j] = bad   # and among the last rows
                at += Q
            pk[at:at + Q] = bad            # both positions at once
            at += Q
        sd[:at] = passing
        sd[n - at:n] = passing
        pk[n:] = bkeys[rng.randint(0, len(bkeys), PAD)]
        sd[n:] = passing
        keep = np.ones(tot, bool) if op is None else cmp_[op](sd, Q3_DATE)
        assert keep[n:].all() and np.isin(pk[n:], bkeys).all()
        keep[n:] = False
        cents = np.rint(ep * 100.0).astype(np.int64)
        di = np.rint(dc * 100.0).astype(np.int64)
        exp = _groups_ref(bkeys, bpay, pk, keep, cents * (100 - di),
                          ep * (1.0 - dc), dec_only)
        assert len(exp["key"]) > 0
        bufs, view = _views({"k": pk, "sd": sd, "ep": ep, "dc": dc}, n)
        for env in ({}, {"PG_GROUPS_LIST": 0}):
            with _env(**env):
                b = _orders_table(P, bkeys, bpay, bmax,
                                  capacity_hint=16 * nb)
            try:
                plan = _q3_plan(P, b.table(),
                                None if op is None else getattr(
                                    P, "CMP_" + op), dec_only)
                before = _counter(P, "pg_groups_list_extractions")
                with _env(PG_PROBE_GRID=grid):
                    got = _groups(P, b.table(), plan, P.Page(view))
                lists = _counter(P, "pg_groups_list_extractions") - before
            finally:
                _free(P, b)
            assert lists == (0 if env else 1), (n, env)
            _same_groups(got, exp)


# --------------------------------------------------------------------- #
# tags                                                                   #
# --------------------------------------------------------------------- #
def _tag_bytes(P, table):
    return _counter_arg(P, "pg_table_tag_bytes", table)


def _counter_arg(P, name, arg):
    f = getattr(P.lib().c, name)
    f.restype = C.c_int64
    f.argtypes = [C.c_int64]
    return f(arg)


@pytest.fixture(scope="module")
def tag_case():
    """A few thousand build rows; a Q3-shape probe that hits every key
    once and carries as many misses."""
    rng = np.random.RandomState(41)
    nb = 3000
    bmax = 8 * nb
    ids = rng.permutation(bmax)[:2 * nb] + 1
    bkeys = np.sort(ids[:nb]).astype(np.int64)
    bpay = rng.randint(0, 1 << 16, nb).astype(np.int64)
    pk = ids[rng.permutation(2 * nb)].astype(np.int64)
    n = len(pk)
    sd = np.full(n, Q3_DATE + 3, np.int32)
    ep = rng.randint(1, 4000, n) * 0.25
    dc = rng.randint(0, 3, n) * 0.25
    cents = np.rint(ep * 100.0).astype(np.int64)
    di = np.rint(dc * 100.0).astype(np.int64)
    exp = _groups_ref(bkeys, bpay, pk, np.ones(n, bool), cents * (100 - di),
                      ep * (1.0 - dc), 0)
    assert np.array_equal(exp["key"], bkeys) and (exp["cnt"] == 1).all()
    return bkeys, bpay, bmax, {"k": pk, "sd": sd, "ep": ep, "dc": dc}, exp


@pytest.mark.parametrize("hint,bitmap,tag_bytes", [
    (20_000_000, True, 0),        # 2^26 slots: the bitmap replaces the tags
    (20_000_000, False, 1 << 26),
    (16 * 3000, True, 0),         # small tables never had them
    (16 * 3000, False, 0),
])
def test_tags_only_without_an_exact_bitmap(P, tag_case, hint, bitmap,
                                           tag_bytes):
    bkeys, bpay, bmax, cols, exp = tag_case
    b = _orders_table(P, bkeys, bpay, bmax if bitmap else 0,
                      capacity_hint=hint)
    try:
        assert _tag_bytes(P, b.table()) == tag_bytes
        got = _groups(P, b.table(), _q3_plan(P, b.table(), P.CMP_GT, 0),
                      P.Page(cols))
    finally:
        _free(P, b)
    _same_groups(got, exp)
