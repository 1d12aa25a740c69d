"""Group extraction from the probe-built hit list (k_groups_emit_list)
against a numpy reference and against the accumulator scan (k_groups_emit,
forced with PG_GROUPS_LIST=0 at build creation) as a second witness.

pg_groups_list_extractions() pins which path a finish() took, so no parity
here is vacuous.

Probe geometry: k_probe_agg_q3 gives a thread 2 consecutive rows, the
generic k_probe_agg 4; a wave is 64 threads, a block 4 waves, the grid 4096
blocks.  A wave stages its first touches in 64 entries and flushes a full
buffer inside the loop, the rest when it leaves.
"""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

WAVE = 64
BLOCK = 256
GRID = 4096
OUT4 = ["key", "dec", "f64", "cnt"]
OUT5 = ["key", "pay", "dec", "f64", "cnt"]


@pytest.fixture(scope="module")
def P():
    import presto_amd
    return presto_amd


def _extractions(P):
    f = P.lib().c.pg_groups_list_extractions
    f.restype = C.c_int64
    return f()


@contextlib.contextmanager
def _scan_only():
    os.environ["PG_GROUPS_LIST"] = "0"
    try:
        yield
    finally:
        del os.environ["PG_GROUPS_LIST"]


def _build(P, keys, pay=None, *, hint=None, agg_table=1, **plan):
    """A finished build over unique i64 keys (payload optional).  The
    default hint gives an agg table at least 16 slots per key, so that at
    16 accumulator bytes per slot or more the byte rule (groups x 128 B <
    slots x accumulator bytes) picks the list for any probe."""
    cols = {"k": np.asarray(keys, np.int64)}
    if pay is not None:
        cols["p"] = pay
        plan["payload"] = [1]
    if agg_table:
        plan["agg_table"] = 1
    b = P.Operator(P.OP_HASH_BUILD, P.plans.hash_build(
        0, capacity_hint=hint if hint is not None else 8 * len(keys) + 16,
        **plan))
    b.add_input(P.Page(cols))
    b.finish()
    return b


def _free(P, *builds):
    for b in builds:
        P.lib().c.pg_table_destroy(b.table())
        b.destroy()


def _sorted(out, names):
    if out is None:
        out = {}
    out = {nm: np.asarray(out.get(nm, np.zeros(0, np.int64))) for nm in names}
    order = np.argsort(out["key"], kind="stable")
    return {nm: out[nm][order] for nm in names}


def _probe(P, table, plan, pages, names):
    """One grouped probe: (groups sorted by key, list extractions)."""
    before = _extractions(P)
    j = P.Operator(P.OP_LOOKUP_JOIN, plan)
    try:
        for pg in pages:
            j.add_input(pg)
        j.finish()
        out = j.get_output(names)
    finally:
        j.destroy()
    return _sorted(out, names), _extractions(P) - before


def _same(got, exp, names):
    for nm in names:
        a, b = np.asarray(got[nm]), np.asarray(exp[nm])
        assert a.shape == b.shape, (nm, a.shape, b.shape)
        if b.dtype == np.float64:
            assert a.dtype == np.float64, nm
            assert np.array_equal(a.view(np.int64), b.view(np.int64)), nm
        else:
            assert np.array_equal(a.astype(np.int64), b.astype(np.int64)), nm


def _reference(bkeys, bpay, pk, keep, ticks, f64, *, dec_only, dec_min=False):
    """Groups of the probe rows that pass `keep` and match a build key.
    ticks are int64, f64 exact binary fractions whose sums are exact."""
    bkeys = np.asarray(bkeys, np.int64)
    order = np.argsort(bkeys)
    sk = bkeys[order]
    hit = keep & np.isin(pk, sk)
    uk, inv = np.unique(pk[hit], return_inverse=True)
    cnt = np.bincount(inv, minlength=len(uk)).astype(np.int64)
    if dec_min:
        dec = np.full(len(uk), np.iinfo(np.int64).max, np.int64)
        np.minimum.at(dec, inv, ticks[hit])
    else:
        dec = np.zeros(len(uk), np.int64)
        np.add.at(dec, inv, ticks[hit])
    fs = np.zeros(len(uk), np.float64)
    if not (dec_only or dec_min):
        np.add.at(fs, inv, f64[hit])
    out = {"key": uk, "dec": dec, "f64": fs, "cnt": cnt}
    if bpay is not None:
        out["pay"] = np.asarray(bpay)[order][np.searchsorted(sk, uk)]
    return out


# --------------------------------------------------------------------- #
# the two probe shapes                                                   #
# --------------------------------------------------------------------- #
Q3_DATE = 9204


def _q3_probe(rng, pk):
    """Q3-shape probe columns: orderkey, shipdate (i32), two f64 money
    columns whose DISC_PRICE products and sums are exact in binary."""
    n = len(pk)
    sd = rng.randint(Q3_DATE - 50, Q3_DATE + 50, n).astype(np.int32)
    ep = rng.randint(1, 4000, n) * 0.25
    dc = rng.randint(0, 3, n) * 0.25
    keep = sd > Q3_DATE
    cents = np.rint(ep * 100.0).astype(np.int64)
    di = np.rint(dc * 100.0).astype(np.int64)
    return ({"k": pk, "sd": sd, "ep": ep, "dc": dc}, keep,
            cents * (100 - di), ep * (1.0 - dc))


def _q3_plan(P, table, dec_only):
    return P.plans.agg_join(table, 0, P.plans.disc_price(2, 3), dec_scale=4,
                            preds=[P.plans.pred(1, P.CMP_GT, Q3_DATE)],
                            dec_only=dec_only)


def _ident_probe(rng, pk):
    n = len(pk)
    v = rng.randint(-1000, 1000, n).astype(np.int64)
    return {"k": pk, "v": v}, np.ones(n, bool), v, np.abs(v).astype(np.float64)


def _run_shape(P, shape, bkeys, bpay, pages_pk, *, dec_only=1, dec_min=0,
               seed=1, expect_list=1, build=None):
    """Build, probe the pages through one operator, and compare with the
    reference; then the same under PG_GROUPS_LIST=0.  Returns the groups."""
    rng = np.random.RandomState(seed)
    names = OUT5 if bpay is not None else OUT4
    build = dict(build or {})
    pages, keeps, tks, fvs = [], [], [], []
    for pk in pages_pk:
        pk = np.asarray(pk, np.int64)
        if shape == "q3":
            cols, keep, tk, fv = _q3_probe(rng, pk)
        else:
            cols, keep, tk, fv = _ident_probe(rng, pk)
            if not (dec_only or dec_min):
                cols["v"] = np.abs(cols["v"])  # SUM_F64 takes x >= 0
                tk = cols["v"]
        pages.append(P.Page(cols))
        keeps.append(keep), tks.append(tk), fvs.append(fv)
    allpk = np.concatenate([np.asarray(p, np.int64) for p in pages_pk]) \
        if pages_pk else np.zeros(0, np.int64)
    cat = (lambda xs, dt: np.concatenate(xs) if xs else np.zeros(0, dt))
    exp = _reference(bkeys, bpay, allpk, cat(keeps, bool),
                     cat(tks, np.int64), cat(fvs, np.float64),
                     dec_only=dec_only, dec_min=dec_min)

    def once():
        b = _build(P, bkeys, bpay, **build)
        try:
            if shape == "q3":
                plan = _q3_plan(P, b.table(), dec_only)
            else:
                plan = P.plans.agg_join(b.table(), 0, P.plans.ident(1),
                                        dec_only=dec_only, dec_min=dec_min)
            return _probe(P, b.table(), plan, pages, names)
        finally:
            _free(P, b)

    got, by_list = once()
    assert by_list == expect_list
    with _scan_only():
        scan, by_list0 = once()
    assert by_list0 == 0
    _same(got, exp, names)
    _same(scan, exp, names)
    # every group exactly once
    assert len(np.unique(got["key"])) == len(got["key"])
    return got


def _table_keys(rng, n):
    return (rng.permutation(4 * n)[:n] + 1).astype(np.int64)


@pytest.mark.parametrize("shape,dec_only,dec_min", [
    ("q3", 1, 0), ("q3", 0, 0), ("ident", 1, 0), ("ident", 0, 0),
    ("ident", 0, 1)])
def test_both_kernels_and_accumulator_layouts(P, shape, dec_only, dec_min):
    """The Q3 shape (k_probe_agg_q3) and a generic shape (k_probe_agg, with
    a dec_min run), on 2-word and 4-word accumulators; pack_bits=16 with an
    i32 payload, hits and misses mixed."""
    rng = np.random.RandomState(5)
    bkeys = _table_keys(rng, 3000)
    bpay = rng.randint(0, 1 << 16, len(bkeys)).astype(np.int32)
    pk = rng.choice(np.concatenate([bkeys[:1500], bkeys[:200] + 4 * 3000 + 5]),
                    5 * BLOCK + 3)
    got = _run_shape(P, shape, bkeys, bpay, [pk], dec_only=dec_only,
                     dec_min=dec_min, build=dict(pack_bits=16))
    assert 0 < len(got["key"]) <= 1500
    if not dec_only and not dec_min:
        assert np.any(got["f64"] != 0.0)


# --------------------------------------------------------------------- #
# first-touch exactness                                                  #
# --------------------------------------------------------------------- #
@pytest.mark.parametrize("shape,rows", [("q3", 2), ("ident", 4)])
def test_first_touch_patterns(P, shape, rows):
    """Per wave pass (64 threads x `rows` rows): every lane first-touches a
    key of its own with the same key in its adjacent rows (all 64); one key
    in every lane of a wave (exactly 1 first touch); misses only (0); the
    same key again in other blocks; a block whose rows are all keys of its
    own (every wave fills its 64-entry buffer more than once and flushes
    inside the pass); a wave with 50 then 50 first touches (the second
    batch straddles a flush).  Every group comes out once."""
    rng = np.random.RandomState(6)
    bkeys = np.arange(1, 3001, dtype=np.int64) * 3
    wave_rows = WAVE * rows
    block_rows = BLOCK * rows
    w_all = np.repeat(bkeys[:WAVE], rows)            # adjacent rows share
    w_one = np.full(wave_rows, bkeys[100])           # many lanes, one key
    w_none = np.full(wave_rows, 7, np.int64)         # not a build key
    lanes = bkeys[200:200 + WAVE].copy()
    lanes[::2] = 8                                   # every other lane misses
    w_mixed = np.repeat(lanes, rows)
    blk0 = np.concatenate([w_all, w_one, w_none, w_mixed])
    assert len(blk0) == block_rows
    # other blocks: the same keys again, and a single new one
    blk1 = np.concatenate([w_one, w_all, w_none, w_none])
    blk2 = np.full(block_rows, 7, np.int64)
    blk2[block_rows // 2 + 1] = bkeys[2900]          # exactly one lane
    blk3 = rng.choice(bkeys[:WAVE], block_rows)
    blk4 = bkeys[1000:1000 + block_rows]             # all rows, own keys
    two = bkeys[2100:2200].reshape(50, 2)            # 50 lanes, 2 keys each
    w_cross = np.concatenate([np.repeat(two, rows // 2, axis=1).ravel(),
                              np.full((WAVE - 50) * rows, 7, np.int64)])
    assert len(w_cross) == wave_rows
    blk5 = np.concatenate([w_cross, w_none, w_none, w_none])
    pk = np.concatenate([blk0, blk1, blk2, blk3, blk4, blk5,
                         w_one[:rows + 1]])
    if shape == "q3":   # the predicate must not thin the pattern out
        got = _first_touch_q3(P, bkeys, pk)
    else:
        got = _run_shape(P, "ident", bkeys, None, [pk])
    exp_keys = np.unique(np.concatenate(
        [bkeys[:WAVE], bkeys[100:101], lanes[1::2], bkeys[2900:2901], blk4,
         bkeys[2100:2200]]))
    assert len(exp_keys) == WAVE + 1 + WAVE // 2 + 1 + block_rows + 100
    assert np.array_equal(got["key"], exp_keys)


def _first_touch_q3(P, bkeys, pk):
    """The Q3 kernel without a predicate: every pattern row is selected."""
    n = len(pk)
    rng = np.random.RandomState(8)
    ep = rng.randint(1, 4000, n) * 0.25
    dc = rng.randint(0, 3, n) * 0.25
    cents = np.rint(ep * 100.0).astype(np.int64)
    di = np.rint(dc * 100.0).astype(np.int64)
    exp = _reference(bkeys, None, pk, np.ones(n, bool), cents * (100 - di),
                     ep * (1.0 - dc), dec_only=0)
    page = P.Page({"k": pk, "ep": ep, "dc": dc})

    def once():
        b = _build(P, bkeys)
        try:
            plan = P.plans.agg_join(b.table(), 0, P.plans.disc_price(1, 2),
                                    dec_scale=4)
            return _probe(P, b.table(), plan, [page], OUT4)
        finally:
            _free(P, b)

    got, by_list = once()
    assert by_list == 1
    with _scan_only():
        scan, by_list0 = once()
    assert by_list0 == 0
    _same(got, exp, OUT4)
    _same(scan, exp, OUT4)
    return got


# --------------------------------------------------------------------- #
# edges                                                                  #
# --------------------------------------------------------------------- #
@pytest.mark.parametrize("shape", ["q3", "ident"])
@pytest.mark.parametrize("n", [0, 1, 3, 5, 4 * BLOCK + 1, 4 * BLOCK + 3])
def test_row_counts(P, shape, n):
    """0 rows, 1 row, and counts that are no multiple of 2 or 4."""
    rng = np.random.RandomState(20 + n)
    bkeys = _table_keys(rng, 1000)
    pk = rng.choice(bkeys, n) if n else np.zeros(0, np.int64)
    _run_shape(P, shape, bkeys, None, [pk], seed=n)


@pytest.mark.parametrize("shape", ["q3", "ident"])
def test_no_hits_gives_empty_output(P, shape):
    rng = np.random.RandomState(30)
    bkeys = _table_keys(rng, 1000)
    pk = bkeys[rng.randint(0, 1000, 2 * BLOCK + 1)] + 4 * 1000 + 1
    got = _run_shape(P, shape, bkeys, None, [pk])
    assert len(got["key"]) == 0


def test_all_keys_hit_list_full(P):
    """Every build key is hit, so the group count equals the list's
    capacity (the inserted rows); at a quarter fill the byte rule
    (groups x 128 B < slots x accumulator bytes) still picks the list."""
    rng = np.random.RandomState(31)
    n = 1000
    bkeys = _table_keys(rng, n)
    pk = np.concatenate([bkeys, bkeys[:77]])[rng.permutation(n + 77)]
    # hint 4000 -> 8192 slots x 32 B = 262144 B > 1000 x 128 B
    got = _run_shape(P, "ident", bkeys, None, [pk], dec_only=0,
                     build=dict(hint=4000))
    assert len(got["key"]) == n


def test_all_keys_hit_falls_back_to_scan(P):
    """The same probe of a half-full 2-word table: one sweep of the
    accumulators is cheaper than the gather, the scan runs and the counter
    does not move."""
    rng = np.random.RandomState(32)
    n = 1000
    bkeys = _table_keys(rng, n)
    pk = np.concatenate([bkeys, bkeys[:77]])[rng.permutation(n + 77)]
    # hint 1000 -> 2048 slots x 16 B = 32768 B < 1000 x 128 B
    got = _run_shape(P, "ident", bkeys, None, [pk], dec_only=1,
                     build=dict(hint=1000), expect_list=0)
    assert len(got["key"]) == n


def test_page_longer_than_a_grid_pass(P):
    """One full grid pass of the Q3 kernel plus 3 rows: the stride loop
    runs a second pass whose only rows belong to the first two threads,
    and every wave flushes what it staged when it leaves the loop."""
    rng = np.random.RandomState(33)
    n = GRID * BLOCK * 2 + 3
    bkeys = _table_keys(rng, 4000)
    pk = rng.choice(np.concatenate([bkeys[:3990], bkeys + 16001]), n)
    pk[-3:] = bkeys[-3:]          # keys that only the second pass touches
    got = _run_shape(P, "q3", bkeys, None, [pk], dec_only=1)
    assert len(got["key"]) > 3900


# --------------------------------------------------------------------- #
# accumulation across calls                                              #
# --------------------------------------------------------------------- #
@pytest.mark.parametrize("shape", ["q3", "ident"])
def test_two_pages_overlapping_keys(P, shape):
    """Two add_input pages whose key sets overlap: no group twice, sums
    add."""
    rng = np.random.RandomState(40)
    bkeys = _table_keys(rng, 2000)
    p1 = rng.choice(bkeys[:1200], 3 * BLOCK + 1)
    p2 = rng.choice(bkeys[800:], 3 * BLOCK + 2)
    p2[:40] = p1[:40]       # keys that both pages touch, whatever the draw
    got = _run_shape(P, shape, bkeys, None, [p1, p2], dec_only=0)
    assert 0 < len(got["key"]) <= len(np.union1d(p1, p2))


def test_reset_acc_starts_the_list_over(P):
    """After pg_table_reset_acc a second probe of the same table returns
    the second probe's groups only, again through the list."""
    rng = np.random.RandomState(41)
    bkeys = _table_keys(rng, 2000)
    b = _build(P, bkeys)
    try:
        for part in (bkeys[:700], bkeys[600:900]):
            pk = rng.choice(part, 2 * BLOCK + 5)
            cols, keep, tk, fv = _ident_probe(rng, pk)
            plan = P.plans.agg_join(b.table(), 0, P.plans.ident(1),
                                    dec_only=1)
            got, by_list = _probe(P, b.table(), plan, [P.Page(cols)], OUT4)
            assert by_list == 1
            _same(got, _reference(bkeys, None, pk, keep, tk, fv, dec_only=1),
                  OUT4)
            assert P.lib().c.pg_table_reset_acc(b.table()) == 0
    finally:
        _free(P, b)


# --------------------------------------------------------------------- #
# tables whose list is not trusted                                       #
# --------------------------------------------------------------------- #
def test_range_group_table_keeps_the_scan(P):
    rng = np.random.RandomState(50)
    K = 3000
    r = P.Operator(P.OP_HASH_BUILD, P.plans.range_group(K))
    r.finish()
    try:
        pk = rng.randint(-5, K + 50, 4 * BLOCK + 3).astype(np.int64)
        cols, keep, tk, fv = _ident_probe(rng, pk)
        plan = P.plans.agg_join(r.table(), 0, P.plans.ident(1), dec_only=1)
        got, by_list = _probe(P, r.table(), plan, [P.Page(cols)], OUT4)
        assert by_list == 0
        exp = _reference(np.arange(1, K + 1), None, pk, keep, tk, fv,
                         dec_only=1)
        _same(got, exp, OUT4)
    finally:
        _free(P, r)


def test_mode3_accumulation_distrusts_the_list(P):
    """A groups table that a mode-3 probe (k_probe_agg_pay, which does not
    append) accumulates into is extracted by the scan: by the mode-3
    operator itself, and by a later mode-1 operator on the same table,
    whose page sees the sums of all three probes."""
    rng = np.random.RandomState(51)
    pl = P.plans
    gkeys = np.arange(1, 401, dtype=np.int64) * 5
    n_o = 3000
    okey = np.arange(1, n_o + 1, dtype=np.int64) * 3
    ogrp = rng.choice(gkeys[100:], n_o)
    g = _build(P, gkeys)
    o = _build(P, okey, ogrp, agg_table=0, hint=n_o)
    try:
        # 1. mode 1 on the groups table: the list is born and used
        pk1 = rng.choice(gkeys[:150], 2 * BLOCK + 1)
        v1 = rng.randint(1, 1000, len(pk1)).astype(np.int64)
        plan1 = pl.agg_join(g.table(), 0, pl.ident(1))
        got, by_list = _probe(P, g.table(), plan1,
                              [P.Page({"k": pk1, "v": v1})], OUT4)
        assert by_list == 1
        exp1 = _reference(gkeys, None, pk1, np.ones(len(pk1), bool), v1,
                          v1.astype(np.float64), dec_only=0)
        _same(got, exp1, OUT4)
        # 2. mode 3 into the same table, accumulators not reset
        pk3 = rng.choice(okey, 2 * BLOCK + 3)
        v3 = rng.randint(1, 1000, len(pk3)).astype(np.int64)
        plan3 = pl.lookup_join(o.table(), 0, 3, table2=g.table(),
                               proj=pl.ident(1))
        got, by_list = _probe(P, g.table(), plan3,
                              [P.Page({"k": pk3, "v": v3})], OUT4)
        assert by_list == 0
        grp3 = ogrp[np.searchsorted(okey, pk3)]
        both_k = np.concatenate([pk1, grp3])
        both_v = np.concatenate([v1, v3])
        exp = _reference(gkeys, None, both_k, np.ones(len(both_k), bool),
                         both_v, both_v.astype(np.float64), dec_only=0)
        _same(got, exp, OUT4)
        # 3. mode 1 again: appends nothing it could trust, scans
        got, by_list = _probe(P, g.table(), plan1,
                              [P.Page({"k": pk1, "v": v1})], OUT4)
        assert by_list == 0
        all_k = np.concatenate([both_k, pk1])
        all_v = np.concatenate([both_v, v1])
        exp = _reference(gkeys, None, all_k, np.ones(len(all_k), bool),
                         all_v, all_v.astype(np.float64), dec_only=0)
        _same(got, exp, OUT4)
    finally:
        _free(P, o, g)


# --------------------------------------------------------------------- #
# packing and payload placement                                          #
# --------------------------------------------------------------------- #
@pytest.mark.parametrize("case", ["packed_i32", "packed_u8", "slot_i64",
                                  "slot_f64", "slot_u8", "chained_i64"])
def test_payload_placement(P, case):
    """Payload packed into the key word (pack_bits), kept per slot without
    packing (each payload type), and reached through head[] on a chained
    build."""
    rng = np.random.RandomState(60)
    bkeys = _table_keys(rng, 1500)
    n = len(bkeys)
    build = {}
    if case == "packed_i32":
        bpay, build = rng.randint(0, 1 << 12, n).astype(np.int32), \
            dict(pack_bits=12)
    elif case == "packed_u8":
        bpay, build = rng.randint(0, 256, n).astype(np.uint8), \
            dict(pack_bits=8)
    elif case == "slot_i64":
        bpay = rng.randint(-2**40, 2**40, n).astype(np.int64)
    elif case == "slot_f64":
        bpay = rng.randint(-1000, 1000, n) * 0.125
    elif case == "slot_u8":
        bpay = rng.randint(0, 256, n).astype(np.uint8)
    else:
        bpay = rng.randint(-2**40, 2**40, n).astype(np.int64)
        build = dict(agg_table=0)
    # a chained build sizes itself at 2 slots per row (4096 x 16 B here):
    # 300 groups x 128 B keep the list on the cheaper side there too
    pk = rng.choice(np.concatenate([bkeys[:300], bkeys[:50] + 6001]),
                    3 * BLOCK + 2)
    got = _run_shape(P, "q3", bkeys, bpay, [pk], dec_only=1, build=build)
    assert got["pay"].dtype == bpay.dtype
