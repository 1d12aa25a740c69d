"""Multi-channel join keys (pg_plan_hash_build.n_keys /
pg_plan_lookup_join.n_keys = 1..4): multi-key chained builds and the four
emit joins over them, against the row-at-a-time reference of
multikey_join_refs.py.  All comparisons are exact.

The plumbing follows test_gpu_outer_join.py: an emitted row-id column pins
the probe-row order, and the rows of one probe row's matches compare as a
multiset (the chain order among duplicate build keys follows the order of
parallel inserts)."""
import functools

import numpy as np
import pytest

import groupby_null_refs as G
import multikey_join_refs as M

pytestmark = pytest.mark.gpu

MODES = (M.INNER, M.PROBE_OUTER, M.LOOKUP_OUTER, M.FULL_OUTER)
PADDING = (M.PROBE_OUTER, M.FULL_OUTER)
DRAINING = (M.LOOKUP_OUTER, M.FULL_OUTER)
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


@pytest.fixture(scope="module")
def P():
    import presto_amd
    return presto_amd


@pytest.fixture(scope="module")
def pl():
    from presto_amd import plans
    return plans


# ---------------- plumbing ----------------

def _page(P, prefix, keys, nulls, extra=(), extra_nulls=None, device=False):
    """Page [extra columns..., k0, k1, ...] (host, or device tensors)."""
    cols, masks = {}, {}
    for name, a in extra:
        cols[name] = a
        if extra_nulls and name in extra_nulls:
            masks[name] = extra_nulls[name]
    for ch, k in enumerate(keys):
        cols[f"{prefix}{ch}"] = k
        if nulls is not None and nulls[ch] is not None:
            masks[f"{prefix}{ch}"] = np.asarray(nulls[ch], np.uint8)
    if device:
        import torch
        cols = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda()
                for k, v in cols.items()}
        masks = {k: torch.from_numpy(v).cuda() for k, v in masks.items()}
    return P.Page(cols, nulls=masks)


def _build(P, pl, s, keys, nulls, payloads, **kw):
    """Multi-key build of one host page [k0.., p0..]; returns the table."""
    nk = len(keys)
    extra = [(f"p{i}", p) for i, p in enumerate(payloads)]
    pg = _page(P, "k", keys, nulls)
    cols = dict(pg.cols)
    cols.update(extra)
    pg = P.Page(cols, nulls=pg.nulls)
    b = s.build(pl.hash_build(range(nk), payload=range(nk, nk + len(extra)),
                              **kw), pg)
    return b.table()


def _probe(P, pl, s, table, pages, mode, key_cols, emit, preds=()):
    """One join operator over the probe pages: ([(cols, nulls) per page],
    drain (cols, nulls) or None).  Columns come back as c0, c1, ..."""
    j = s.op(P.OP_LOOKUP_JOIN,
             pl.lookup_join(table, key_cols, mode, preds=preds, emit=emit))
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


def _sorted_rows(cols):
    """The rows as one int64/uint64-safe matrix sorted row-wise: equal
    multisets give equal matrices.  Floats compare by their bits."""
    mat = [np.asarray(c) for c in cols]
    mat = [c.view(np.int64) if c.dtype == np.float64 else c.astype(np.int64)
           for c in mat]
    order = np.lexsort(mat[::-1]) if len(mat[0]) else np.zeros(0, np.int64)
    return [c[order] for c in mat]


def _check_probe_page(got, ref_cols, ref_masks, mode, n_emit,
                      probe_masks=None, exact_order=False):
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
    # the page of an empty probe page carries no masks, as on the single-key
    # path (it has the columns and nothing to mask)
    if mode in PADDING and len(rowid):
        mask = nulls[pay[0]]
        assert mask.dtype == np.uint8 and len(mask) == len(rowid)
        for nm in pay:                           # one mask for all payloads
            assert np.array_equal(nulls[nm], mask), nm
            assert not cols[nm][mask == 1].view(np.uint8).any(), nm
    else:
        assert mode in PADDING or not any(nm in nulls for nm in pay)
        mask = np.zeros(len(rowid), np.uint8)
    probe_masks = probe_masks or {}
    extra, ref_extra = [], []
    for o in range(n_emit):
        if o in probe_masks:
            extra.append(nulls[f"c{o}"])
            ref_extra.append(probe_masks[o])
        else:
            assert f"c{o}" not in nulls
    got_cols = [cols[nm] for nm in names] + extra + [mask]
    exp_cols = list(ref_cols) + ref_extra + [np.asarray(ref_masks)]
    if exact_order:
        for g, e in zip(got_cols, exp_cols):
            assert np.array_equal(g, e)
    else:
        for g, e in zip(_sorted_rows(got_cols), _sorted_rows(exp_cols)):
            assert np.array_equal(g, e)


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


def _join_all_modes(P, pl, bkeys, bnulls, payloads, pkeys, pnulls,
                    modes=MODES, exact_order=False):
    """Build + one probe page [rowid, k0..] per mode against the reference;
    returns the reference outputs per mode."""
    n = len(pkeys[0])
    nk = len(bkeys)
    rowid = np.arange(n, dtype=np.int64)
    refs = {}
    with P.Scope() as s:
        table = _build(P, pl, s, bkeys, bnulls, payloads)
        page = _page(P, "k", pkeys, pnulls, [("rowid", rowid)])
        for mode in modes:
            outs, drain = _probe(P, pl, s, table, [page], mode,
                                 range(1, 1 + nk), [0])
            ref = M.multikey_join(bkeys, bnulls, payloads, [rowid], pkeys,
                                  pnulls, None, mode)
            _check_probe_page(outs[0], ref[0], ref[1], mode, 1,
                              exact_order=exact_order)
            _check_drain(drain, ref[2], mode, 1, [np.int64])
            refs[mode] = ref
    return refs


def _i64(*v):
    return np.array(v, np.int64)


# ---------------- 1. the hand case ----------------

BK = [_i64(1, 1, 2, 2, 1), _i64(10, 20, 10, 10, 10)]
PAY = _i64(100, 101, 102, 103, 104)
PK = [_i64(1, 2, 2, 10, 1), _i64(10, 20, 10, 1, 20)]
INNER_ROWS = [(0, 100), (0, 104), (2, 102), (2, 103), (4, 101)]
LEFT_ROWS = [(0, 100, 0), (0, 104, 0), (1, 0, 1), (2, 102, 0), (2, 103, 0),
             (3, 0, 1), (4, 101, 0)]


@pytest.mark.parametrize("mode", MODES)
def test_hand_case(P, pl, mode):
    rowid = np.arange(5, dtype=np.int64)
    with P.Scope() as s:
        table = _build(P, pl, s, BK, None, [PAY])
        page = _page(P, "k", PK, None, [("rowid", rowid)])
        ((cols, nulls),), drain = _probe(P, pl, s, table, [page], mode,
                                         [1, 2], [0])
    assert [c.dtype for c in cols.values()] == [np.int64, np.int64]
    assert "c0" not in nulls
    if mode in PADDING:
        assert sorted(nulls) == ["c1"]
        assert M.canonical(cols.values(), nulls["c1"]) == LEFT_ROWS
        assert cols["c0"].tolist() == [0, 0, 1, 2, 2, 3, 4]
        assert nulls["c1"].tolist() == [0, 0, 1, 0, 0, 1, 0]
    else:
        assert nulls == {}
        assert M.canonical(cols.values()) == INNER_ROWS
        assert cols["c0"].tolist() == [0, 0, 2, 2, 4]
    if mode in DRAINING:                 # every build row was matched
        dcols, dnulls = drain
        assert {k: v.tolist() for k, v in dcols.items()} == \
            {"c0": [], "c1": []}
        assert dcols["c0"].dtype == np.int64
    else:
        assert drain is None


def test_hand_case_drain(P, pl):
    """Without probe rows 0 and 2 their build rows drain, in row order."""
    rowid = np.arange(5, dtype=np.int64)
    keep = np.array([0, 1, 0, 1, 1], np.uint8)
    with P.Scope() as s:
        table = _build(P, pl, s, BK, None, [PAY])
        page = _page(P, "k", PK, None, [("rowid", rowid), ("keep", keep)])
        ((cols, nulls),), (dcols, dnulls) = _probe(
            P, pl, s, table, [page], M.FULL_OUTER, [2, 3], [0],
            preds=[pl.pred(1, P.CMP_EQ, 1)])
    assert M.canonical(cols.values(), nulls["c1"]) == \
        [(1, 0, 1), (3, 0, 1), (4, 101, 0)]
    assert dcols["c1"].tolist() == [100, 102, 103, 104]
    assert dnulls["c0"].tolist() == [1, 1, 1, 1] and "c1" not in dnulls


# ---------------- 2. position and bits ----------------

def test_position_and_bits(P, pl):
    B = 1 << 32
    rows = [
        (1, 2, 0, 0), (2, 1, 0, 0),              # (a, b) vs (b, a)
        (7, 5, 5, 5), (8, 5, 5, 5),              # differ in the first only
        (5, 5, 5, 7), (5, 5, 5, 8),              # differ in the last only
        (1, 9, 9, 9), (1 + B, 9, 9, 9),          # differ above bit 32
        (9, 9, 9, 1), (9, 9, 9, 1 + B),
        (-1, -2, -3, -4), (-1, -2, -3, 4),
        (I64_MIN, 0, 0, 0), (0, 0, 0, I64_MIN), (I64_MIN,) * 4,
        (I64_MAX, I64_MIN, I64_MAX, I64_MIN),
        (0, 0, 0, 0),
    ]
    bkeys = [np.array([r[ch] for r in rows], np.int64) for ch in range(4)]
    pay = np.arange(len(rows), dtype=np.int64)
    probes = rows + [
        (2, 1, 0, 1), (0, 0, 1, 2), (5, 5, 5, 5), (1 + 2 * B, 9, 9, 9),
        (9, 9, 9, 1 - B), (1, 2, 3, 4), (-1, -2, -3, -5),
        (I64_MIN, 0, 0, 1), (I64_MAX,) * 4, (0, 0, 0, 1), (B, 0, 0, 0)]
    pkeys = [np.array([r[ch] for r in probes], np.int64) for ch in range(4)]
    refs = _join_all_modes(P, pl, bkeys, None, [pay], pkeys, None)
    # every build combination is distinct: each of the first len(rows)
    # probe rows finds exactly its own build row, the rest find nothing
    cols, masks, _ = refs[M.INNER]
    assert cols[0].tolist() == list(range(len(rows)))
    assert cols[1].tolist() == list(range(len(rows)))
    assert refs[M.PROBE_OUTER][1].sum() == len(probes) - len(rows)


@pytest.mark.parametrize("nk", [1, 2, 3])
def test_zero_and_prefix_keys(P, pl, nk):
    """0 in every channel, and vectors that agree on a prefix, at the
    smaller key counts."""
    rng = np.random.default_rng(nk)
    bkeys = [rng.integers(-1, 2, 200).astype(np.int64) for _ in range(nk)]
    pkeys = [rng.integers(-1, 3, 300).astype(np.int64) for _ in range(nk)]
    for ch in range(nk):
        bkeys[ch][0] = 0
        pkeys[ch][0] = 0
    pay = np.arange(200, dtype=np.int32)
    refs = _join_all_modes(P, pl, bkeys, None, [pay], pkeys, None)
    assert (refs[M.INNER][0][0] == 0).any()     # the all-zero key matched


# ---------------- 3. mixed widths ----------------

def test_mixed_widths(P, pl):
    """Build typed (I64, I32, U8), probe typed (I32, I64, I64): channels
    compare as their widened signed values."""
    bk = [np.array([-1, 255, 7, -1, 300, 1 << 40], np.int64),
          np.array([-1, -1, 2, 255, -7, 0], np.int32),
          np.array([255, 255, 0, 255, 1, 9], np.uint8)]
    pay = np.arange(6, dtype=np.int64)
    pk = [np.array([-1, 255, 7, -1, -1, 300, 0, -1], np.int32),
          np.array([-1, -1, 2, 255, -1, -7, 0, (1 << 32) - 1], np.int64),
          np.array([255, 255, 0, 255, -1, 1, 9, 255], np.int64)]
    refs = _join_all_modes(P, pl, bk, None, [pay], pk, None)
    cols, _, drain = refs[M.FULL_OUTER]
    # I32 -1 == I64 -1; U8 255 == I64 255 and != I64 -1; 2^32-1 != I32 -1;
    # 2^40 is not reachable from an I32 probe channel
    inner = refs[M.INNER][0]
    assert list(zip(inner[0].tolist(), inner[1].tolist())) == \
        [(0, 0), (1, 1), (2, 2), (3, 3), (5, 4)]
    assert drain[0].tolist() == [5]


def test_u8_key_against_i32(P, pl):
    bk = [np.array([255, 0, 128], np.uint8)]
    pk = [np.array([-1, 255, 0, 128, -128], np.int32)]
    refs = _join_all_modes(P, pl, bk, None, [np.arange(3, dtype=np.uint8)],
                           pk, None)
    inner = refs[M.INNER][0]
    assert list(zip(inner[0].tolist(), inner[1].tolist())) == \
        [(1, 0), (2, 1), (3, 2)]


# ---------------- 4. nulls ----------------

def test_probe_nulls(P, pl):
    """Probe nulls in channel 0 only, channel 1 only and both, each over a
    value that equals a real build key."""
    bk = [_i64(1, 2, 3, 3), _i64(10, 20, 30, 30)]
    pay = np.array([1.5, 2.5, 3.5, 4.5])
    pk = [_i64(1, 2, 3, 3, 1, 2), _i64(10, 20, 30, 30, 10, 21)]
    pn = [np.array([0, 1, 0, 1, 0, 0], np.uint8),
          np.array([0, 0, 1, 1, 0, 0], np.uint8)]
    refs = _join_all_modes(P, pl, bk, None, [pay], pk, pn)
    # mode 0 on the multi-key path drops null-key probe rows as well
    assert refs[M.INNER][0][0].tolist() == [0, 4]
    assert refs[M.PROBE_OUTER][1].tolist() == [0, 1, 1, 1, 0, 1]
    assert refs[M.LOOKUP_OUTER][2][0].tolist() == [2.5, 3.5, 4.5]


def test_build_nulls(P, pl):
    """The same on the build side: null-key build rows match nothing and
    drain at their build-row positions."""
    bk = [_i64(1, 2, 3, 4, 1, 5), _i64(10, 20, 30, 40, 10, 50)]
    bn = [np.array([0, 1, 0, 1, 0, 0], np.uint8),
          np.array([0, 0, 1, 1, 0, 0], np.uint8)]
    pay = np.array([100, 101, 102, 103, 104, 105], np.int32)
    pk = [_i64(1, 2, 3, 4, 6), _i64(10, 20, 30, 40, 60)]
    refs = _join_all_modes(P, pl, bk, bn, [pay], pk, None)
    inner = refs[M.INNER][0]
    assert list(zip(inner[0].tolist(), inner[1].tolist())) == \
        [(0, 100), (0, 104)]
    for mode in DRAINING:
        assert refs[mode][2][0].tolist() == [101, 102, 103, 105]
    # null never equals null: both sides null over equal stored values
    pn = [np.array([0, 1, 0, 1, 0], np.uint8),
          np.array([0, 0, 1, 1, 0], np.uint8)]
    refs = _join_all_modes(P, pl, bk, bn, [pay], pk, pn)
    assert refs[M.FULL_OUTER][1].tolist() == [0, 0, 1, 1, 1, 1]


def test_value_under_null_is_ignored(P, pl):
    bn = [np.array([0, 1, 0], np.uint8), None]
    pay = np.arange(3, dtype=np.int64)
    pk = [_i64(1, 2, 3, -5), _i64(1, 2, 3, 2)]
    a = _join_all_modes(P, pl, [_i64(1, 2, 3), _i64(1, 2, 3)], bn, [pay],
                        pk, None)
    b = _join_all_modes(P, pl, [_i64(1, -5, 3), _i64(1, 2, 3)], bn, [pay],
                        pk, None)
    for mode in MODES:
        for x, y in zip(a[mode][0], b[mode][0]):
            assert np.array_equal(x, y)
    assert a[M.INNER][0][0].tolist() == [0, 2]


# ---------------- 5. chains ----------------

def test_long_chain(P, pl):
    """One combination on 5,000 build rows among 3,000 distinct others:
    every probe row that hits it emits all 5,000 row ids exactly once."""
    rng = np.random.default_rng(5)
    nb = 8000
    k0 = np.empty(nb, np.int64)
    k1 = np.empty(nb, np.int64)
    hot = rng.permutation(nb)[:5000]
    cold = np.setdiff1d(np.arange(nb), hot)
    k0[hot], k1[hot] = 77, -77
    k0[cold] = np.arange(3000)
    k1[cold] = np.arange(3000) * 3
    ids = np.arange(nb, dtype=np.int64)
    n = 120
    p0 = rng.integers(0, 3000, n).astype(np.int64)
    p1 = p0 * 3
    hits = rng.permutation(n)[:50]
    p0[hits], p1[hits] = 77, -77
    rowid = np.arange(n, dtype=np.int64)
    with P.Scope() as s:
        table = _build(P, pl, s, [k0, k1], None, [ids])
        page = _page(P, "k", [p0, p1], None, [("rowid", rowid)])
        ((cols, nulls),), drain = _probe(P, pl, s, table, [page],
                                         M.FULL_OUTER, [1, 2], [0])
    assert not nulls["c1"].any()
    want = np.sort(ids[hot])
    for r in hits:
        got = np.sort(cols["c1"][cols["c0"] == r])
        assert np.array_equal(got, want)
    assert len(cols["c0"]) == 50 * 5000 + (n - 50)
    ref = M.multikey_join([k0, k1], None, [ids], [rowid], [p0, p1], None,
                          None, M.FULL_OUTER)
    _check_probe_page((cols, nulls), ref[0], ref[1], M.FULL_OUTER, 1)
    _check_drain(drain, ref[2], M.FULL_OUTER, 1, [np.int64])


def test_all_rows_identical(P, pl):
    n = 4096
    keys = [np.full(n, 3, np.int64), np.full(n, -9, np.int32),
            np.full(n, 200, np.uint8)]
    ids = np.arange(n, dtype=np.int32)
    refs = _join_all_modes(P, pl, keys, None, [ids],
                           [_i64(3), _i64(-9), _i64(200)], None)
    assert len(refs[M.INNER][0][0]) == n
    assert np.array_equal(np.sort(refs[M.INNER][0][1]), ids)
    assert len(refs[M.FULL_OUTER][2][0]) == 0


# ---------------- 6. fuzz ----------------

@functools.lru_cache(maxsize=None)
def _fuzz_data(nk):
    rng = np.random.default_rng(100 + nk)
    nb, n = 3000, 5000
    dts = (np.int64, np.int32, np.uint8, np.int64)
    bk = [rng.integers(0, 8, nb).astype(dts[ch]) for ch in range(nk)]
    bn = [(rng.random(nb) < 0.05).astype(np.uint8) for _ in range(nk)]
    pays = [np.arange(nb, dtype=np.int64),
            rng.integers(0, 250, nb).astype(np.uint8),
            rng.standard_normal(nb)]
    pk = [rng.integers(0, 9, n).astype(dts[::-1][ch]) for ch in range(nk)]
    pn = [(rng.random(n) < 0.05).astype(np.uint8) for _ in range(nk)]
    flag = rng.integers(0, 4, n).astype(np.int32)   # the predicate: != 0
    extra = rng.integers(-99, 99, n).astype(np.int32)
    extra_null = (rng.random(n) < 0.3).astype(np.uint8)
    return bk, bn, pays, pk, pn, flag, extra, extra_null


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("nk", [1, 2, 3, 4])
def test_fuzz(P, pl, nk, mode):
    bk, bn, pays, pk, pn, flag, extra, extra_null = _fuzz_data(nk)
    n = len(flag)
    rowid = np.arange(n, dtype=np.int64)
    with P.Scope() as s:
        table = _build(P, pl, s, bk, bn, pays)
        page = _page(P, "k", pk, pn,
                     [("rowid", rowid), ("flag", flag), ("extra", extra)],
                     {"extra": extra_null})
        outs, drain = _probe(P, pl, s, table, [page], mode,
                             range(3, 3 + nk), [0, 2],
                             preds=[pl.pred(1, P.CMP_NE, 0)])
    ref = M.multikey_join(bk, bn, pays, [rowid, extra], pk, pn, flag != 0,
                          mode)
    assert len(ref[0][0]) > 0
    pm = {1: extra_null[ref[0][0]]} if mode != M.INNER else None
    _check_probe_page(outs[0], ref[0], ref[1], mode, 2, probe_masks=pm)
    _check_drain(drain, ref[2], mode, 2, [np.int64, np.int32])


# ---------------- 7. sizes ----------------

@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 255, 256, 257])
def test_probe_page_sizes(P, pl, n):
    rng = np.random.default_rng(n)
    bk = [rng.integers(0, 6, 40).astype(np.int64),
          rng.integers(0, 3, 40).astype(np.int32)]
    pay = np.arange(40, dtype=np.int32)
    pk = [rng.integers(0, 7, n).astype(np.int64),
          rng.integers(0, 3, n).astype(np.int64)]
    _join_all_modes(P, pl, bk, None, [pay], pk, None)


def test_empty_probe_page_columns(P, pl):
    with P.Scope() as s:
        table = _build(P, pl, s, BK, None, [PAY.astype(np.int32)])
        page = _page(P, "k", [np.zeros(0, np.int64), np.zeros(0, np.int32)],
                     None, [("rowid", np.zeros(0, np.int32))])
        for mode in MODES:
            ((cols, nulls),), drain = _probe(P, pl, s, table, [page], mode,
                                             [1, 2], [0])
            assert [(c.dtype, len(c)) for c in cols.values()] == \
                [(np.int32, 0), (np.int32, 0)]
            if mode in DRAINING:
                assert drain[0]["c1"].tolist() == PAY.tolist()


def test_large_probe_page_exact_order(P, pl):
    """300,001 probe rows over unique build keys: beyond 262,144 rows every
    block walks two 256-row windows and carries its running offset, and
    with unique keys the whole output order is pinned."""
    rng = np.random.default_rng(7)
    nb, n = 50000, 300001
    perm = rng.permutation(nb).astype(np.int64)
    bk = [perm // 200, (perm % 200).astype(np.int32)]
    pay = np.arange(nb, dtype=np.int64)
    x = rng.integers(0, nb + nb // 3, n).astype(np.int64)
    pk = [x // 200, x % 200]
    refs = _join_all_modes(P, pl, bk, None, [pay], pk, None,
                           modes=(M.INNER, M.FULL_OUTER), exact_order=True)
    assert 0 < refs[M.FULL_OUTER][1].sum() < n


@pytest.mark.parametrize("nb", [0, 1])
def test_tiny_builds(P, pl, nb):
    bk = [np.full(nb, 4, np.int64), np.full(nb, 5, np.int64)]
    pay = np.full(nb, 9, np.int32)
    pk = [_i64(4, 4, 1), _i64(5, 6, 5)]
    refs = _join_all_modes(P, pl, bk, None, [pay], pk, None)
    if nb == 0:
        assert len(refs[M.INNER][0][0]) == 0
        assert len(refs[M.LOOKUP_OUTER][0][0]) == 0
        assert refs[M.PROBE_OUTER][1].tolist() == [1, 1, 1]
        assert refs[M.FULL_OUTER][1].tolist() == [1, 1, 1]
        assert len(refs[M.FULL_OUTER][2][0]) == 0
    else:
        assert refs[M.FULL_OUTER][1].tolist() == [0, 1, 1]


def test_build_without_pages(P, pl):
    with P.Scope() as s:
        b = s.build(pl.hash_build([0, 1], payload=[2]))
        page = _page(P, "k", [_i64(1), _i64(2)], None,
                     [("rowid", _i64(0))])
        for mode in MODES:
            ((cols, nulls),), drain = _probe(P, pl, s, b.table(), [page],
                                             mode, [1, 2], [0])
            assert len(cols["c0"]) == (1 if mode in PADDING else 0)
            if mode in DRAINING:
                assert len(drain[0]["c1"]) == 0


# ---------------- 8. pages ----------------

def test_build_and_probe_pages(P, pl):
    """A build from three pages (1,000 / 1 / 2,500 rows, host and device,
    masks on the middle page only) that outgrows its capacity_hint, three
    probe pages through one operator, one drain over all of it."""
    rng = np.random.default_rng(8)
    sizes = (1000, 1, 2500)
    nb = sum(sizes)
    bk = [rng.integers(0, 40, nb).astype(np.int64),
          rng.integers(0, 40, nb).astype(np.int32)]
    bn = [np.zeros(nb, np.uint8), np.zeros(nb, np.uint8)]
    bn[1][1000] = 1                          # the middle page's only row
    ids = np.arange(nb, dtype=np.int64)
    f64 = rng.standard_normal(nb)
    psizes = (700, 0, 900)
    n = sum(psizes)
    pk = [rng.integers(0, 45, n).astype(np.int32),
          rng.integers(0, 30, n).astype(np.int64)]
    pn = [(rng.random(n) < 0.1).astype(np.uint8), None]
    rowid = np.arange(n, dtype=np.int64)
    with P.Scope() as s:
        bpages, lo = [], 0
        for i, sz in enumerate(sizes):
            bpages.append(_bpage(P, bk, bn, ids, f64, slice(lo, lo + sz),
                                 masked=(i == 1), device=(i == 2)))
            lo += sz
        table = s.build(pl.hash_build([0, 1], payload=[2, 3],
                                      capacity_hint=16), *bpages).table()
        for mode in MODES:
            pages, lo = [], 0
            for sz in psizes:
                sl = slice(lo, lo + sz)
                pages.append(_page(P, "k", [k[sl] for k in pk],
                                   [pn[0][sl], None],
                                   [("rowid", rowid[sl])],
                                   device=(sz == 900)))
                lo += sz
            outs, drain = _probe(P, pl, s, table, pages, mode, [1, 2], [0])
            unmatched = np.ones(nb, bool)
            lo = 0
            for got, sz in zip(outs, psizes):
                sl = slice(lo, lo + sz)
                ref = M.multikey_join(bk, bn, [ids, f64], [rowid[sl]],
                                      [k[sl] for k in pk], [pn[0][sl], None],
                                      None, mode)
                _check_probe_page(got, ref[0], ref[1], mode, 1)
                if ref[2] is not None:
                    unmatched &= np.isin(ids, ref[2][0])
                lo += sz
            ref_drain = [ids[unmatched], f64[unmatched]]
            _check_drain(drain, ref_drain, mode, 1, [np.int64])
            if mode in DRAINING:
                assert 1000 in drain[0]["c1"].tolist()   # the null-key row


def _bpage(P, bk, bn, ids, f64, sl, masked, device):
    cols = {"k0": bk[0][sl], "k1": bk[1][sl], "id": ids[sl], "x": f64[sl]}
    masks = {"k0": bn[0][sl].copy(), "k1": bn[1][sl].copy()} if masked \
        else {}
    if device:
        import torch
        cols = {k: torch.from_numpy(np.ascontiguousarray(v)).cuda()
                for k, v in cols.items()}
        masks = {k: torch.from_numpy(v).cuda() for k, v in masks.items()}
    return P.Page(cols, nulls=masks)


# ---------------- 9. build filter ----------------

def test_build_filter(P, pl):
    """Rows failing the build preds or the build semijoin are neither
    matched nor drained."""
    rng = np.random.default_rng(9)
    nb = 600
    bk = [rng.integers(0, 10, nb).astype(np.int64),
          rng.integers(0, 10, nb).astype(np.int64)]
    ids = np.arange(nb, dtype=np.int64)
    flag = rng.integers(0, 3, nb).astype(np.int32)
    member = rng.integers(1, 9, nb).astype(np.int64)
    in_set = [2, 3, 5, 8]
    kept = (flag != 0) & np.isin(member, in_set)
    assert 0 < kept.sum() < nb
    pk = [rng.integers(0, 11, 500).astype(np.int64),
          rng.integers(0, 11, 500).astype(np.int64)]
    rowid = np.arange(500, dtype=np.int64)
    with P.Scope() as s:
        kset = s.build(pl.hash_build(0, capacity_hint=32, key_set_only=1),
                       P.Page({"key": np.asarray(in_set, np.int64)}))
        b = s.build(pl.hash_build(
            [0, 1], payload=[2], preds=[pl.pred(3, P.CMP_NE, 0)],
            semijoin_table=kset.table(), semijoin_col=4),
            P.Page({"k0": bk[0], "k1": bk[1], "id": ids, "flag": flag,
                    "member": member}))
        page = _page(P, "k", pk, None, [("rowid", rowid)])
        for mode in MODES:
            outs, drain = _probe(P, pl, s, b.table(), [page], mode, [1, 2],
                                 [0])
            ref = M.multikey_join([k[kept] for k in bk], None, [ids[kept]],
                                  [rowid], pk, None, None, mode)
            _check_probe_page(outs[0], ref[0], ref[1], mode, 1)
            _check_drain(drain, ref[2], mode, 1, [np.int64])


# ---------------- 10. errors ----------------

def _create_fails(P, s, kind, plan, *words):
    with pytest.raises(RuntimeError) as e:
        s.op(kind, plan)
    for w in words:
        assert w in str(e.value), (w, str(e.value))


@pytest.mark.parametrize("field,value", [
    ("agg_table", 1), ("dense_array", 1), ("range_group", 1),
    ("key_set_only", 1), ("pack_bits", 8), ("fill_x10", 13),
    ("bitmap_max_key", 100), ("payload_lookup_table", 1)])
def test_build_rejects_other_shapes(P, pl, field, value):
    with P.Scope() as s:
        _create_fails(P, s, P.OP_HASH_BUILD,
                      pl.hash_build([0, 1], payload=[2], capacity_hint=64,
                                    **{field: value}),
                      "HASH_BUILD", "n_keys", field)


def test_create_rejections(P, pl):
    with P.Scope() as s:
        for bad in (-1, 5):
            plan = pl.hash_build([0, 1])
            plan.n_keys = bad
            _create_fails(P, s, P.OP_HASH_BUILD, plan, "HASH_BUILD",
                          "n_keys", str(bad))
        plan = pl.hash_build([0, 1])
        plan.key_cols[1] = -1
        _create_fails(P, s, P.OP_HASH_BUILD, plan, "HASH_BUILD", "n_keys",
                      "key_cols[1]")
        mk = _build(P, pl, s, BK, None, [PAY])
        legacy = s.build(pl.hash_build(0, payload=[1]),
                         P.Page({"k": BK[0], "p": PAY})).table()
        three = _build(P, pl, s, BK + [BK[0]], None, [PAY])
        # the counts must agree, legacy (0) included, in both directions
        _create_fails(P, s, P.OP_LOOKUP_JOIN, pl.emit_join(mk, 0, [0]),
                      "n_keys = 0", "n_keys = 2")
        _create_fails(P, s, P.OP_LOOKUP_JOIN,
                      pl.emit_join(legacy, [0, 1], [0]),
                      "n_keys = 2", "n_keys = 0")
        _create_fails(P, s, P.OP_LOOKUP_JOIN,
                      pl.left_join(three, [0, 1], [0]),
                      "n_keys = 2", "n_keys = 3")
        for mode in (1, 2, 3):
            _create_fails(P, s, P.OP_LOOKUP_JOIN,
                          pl.lookup_join(mk, [0, 1], mode,
                                         proj=pl.ident(0)),
                          f"mode {mode}", "multi-key")
        plan = pl.emit_join(mk, [0, 1], [0])
        plan.key_cols[0] = -3
        _create_fails(P, s, P.OP_LOOKUP_JOIN, plan, "LOOKUP_JOIN", "n_keys",
                      "key_cols[0]")
        plan = pl.emit_join(mk, [0, 1], [0])
        plan.n_keys = 7
        _create_fails(P, s, P.OP_LOOKUP_JOIN, plan, "LOOKUP_JOIN", "n_keys",
                      "7")
        # a multi-key table is no key set
        _create_or_feed_fails(P, pl, s, mk)


def _create_or_feed_fails(P, pl, s, mk):
    f = s.op(P.OP_FILTER_PROJECT, pl.filter_project(
        [pl.ident(0)], semijoin_table=mk, semijoin_col=0))
    with pytest.raises(RuntimeError, match="multi-key"):
        f.add_input(P.Page({"k": BK[0]}))


def _bad_key_pages(P):
    k = _i64(1, 2)
    return [
        ("F64", P.Page({"a": k, "b": np.array([1.0, 2.0])})),
        ("VARBIN", P.Page({"a": k, "b": P.Varbin([b"x", b"y"])})),
        ("dictionary", P.Page({"a": k,
                               "b": P.DictVarbin([b"x", b"y"], [0, 1])})),
    ]


def test_build_add_input_rejections(P, pl):
    good = P.Page({"a": _i64(1, 2), "b": _i64(3, 4), "p": _i64(5, 6)})
    with P.Scope() as s:
        b = s.op(P.OP_HASH_BUILD, pl.hash_build([0, 1], payload=[2]))
        for word, page in _bad_key_pages(P):
            pg = P.Page(dict(page.cols, p=_i64(5, 6)))
            with pytest.raises(RuntimeError) as e:
                b.add_input(pg)
            assert all(w in str(e.value) for w in
                       ("HASH_BUILD", "key_cols[1]", "column 1", word))
        i128_page = P.Page({"a": _i64(1), "b": _i64(2), "p": _i64(3)})
        i128 = i128_page.to_c()
        i128.cols[1].tag = P.engine.T_I128
        with pytest.raises(RuntimeError, match=r"key_cols\[1\].*I128"):
            b.add_input_raw(i128)
        with pytest.raises(RuntimeError, match=r"key_cols\[1\].*outside"):
            b.add_input(P.Page({"a": _i64(1, 2)}))
        b.add_input(good)
        with pytest.raises(RuntimeError) as e:      # types stay the same
            b.add_input(P.Page({"a": _i64(1), "b": np.array([3], np.int32),
                                "p": _i64(5)}))
        assert "key_cols[1]" in str(e.value) and \
            "differs from the first page's" in str(e.value)
        with pytest.raises(RuntimeError, match=r"payload_col\[0\]"):
            b.add_input(P.Page({"a": _i64(1), "b": _i64(3),
                                "p": np.array([5], np.int32)}))
        # after the rejected pages the build still works
        b.add_input(good)
        b.finish()
        page = P.Page({"rowid": _i64(0, 1), "a": _i64(2, 1), "b": _i64(4, 9)})
        ((cols, _),), drain = _probe(P, pl, s, b.table(), [page],
                                     M.LOOKUP_OUTER, [1, 2], [0])
        assert M.canonical(cols.values()) == [(0, 6), (0, 6)]
        assert drain[0]["c1"].tolist() == [5, 5]
        s._free_table(b.table())


def test_probe_add_input_rejections(P, pl):
    with P.Scope() as s:
        table = _build(P, pl, s, BK, None, [PAY])
        j = s.op(P.OP_LOOKUP_JOIN, pl.full_join(table, [0, 1], [0]))
        for word, page in _bad_key_pages(P):
            with pytest.raises(RuntimeError) as e:
                j.add_input(page)
            assert all(w in str(e.value) for w in
                       ("LOOKUP_JOIN", "key_cols[1]", "column 1", word))
        i128_page = P.Page({"a": _i64(1), "b": _i64(2)})
        i128 = i128_page.to_c()
        i128.cols[1].tag = P.engine.T_I128
        with pytest.raises(RuntimeError, match=r"key_cols\[1\].*I128"):
            j.add_input_raw(i128)
        j.add_input(P.Page({"a": _i64(1, 7), "b": _i64(10, 7)}))
        first = j.get_output_nulls()
        with pytest.raises(RuntimeError, match="differs from the first"):
            j.add_input(P.Page({"a": np.array([1], np.int32),
                                "b": _i64(10)}))
        # after the rejected pages the operator still works
        j.add_input(P.Page({"a": _i64(2), "b": _i64(10)}))
        second = j.get_output_nulls()
        j.finish()
        drain = j.get_output_nulls()
    assert M.canonical(first[0].values(), first[1]["c1"]) == \
        [(1, 100, 0), (1, 104, 0), (7, 0, 1)]
    assert M.canonical(second[0].values(), second[1]["c1"]) == \
        [(2, 102, 0), (2, 103, 0)]
    assert drain[0]["c1"].tolist() == [101]


# ---------------- 11. path pinning ----------------

def test_counter_pins_the_path(P, pl):
    f = P.engine.lib().c.pg_multikey_probe_pages
    rowid = np.arange(5, dtype=np.int64)
    with P.Scope() as s:
        table = _build(P, pl, s, BK, None, [PAY])
        page = _page(P, "k", PK, None, [("rowid", rowid)])
        before = f()
        _probe(P, pl, s, table, [page, page, page], M.INNER, [1, 2], [0])
        assert f() == before + 3
        _probe(P, pl, s, table, [page], M.FULL_OUTER, [1, 2], [0])
        assert f() == before + 4
        legacy = s.build(pl.hash_build(0, payload=[1]),
                         P.Page({"k": BK[0], "p": PAY})).table()
        for mode in MODES:
            _probe(P, pl, s, legacy, [page], mode, 1, [0])
        assert f() == before + 4


# ---------------- 12. composition ----------------

def test_left_join_then_group_by(P, pl):
    """A LEFT two-key join's raw device page into GROUP BY with SQL nulls:
    the null-padded payloads form the null group."""
    rng = np.random.default_rng(12)
    nb, n = 300, 2000
    bk = [rng.integers(0, 12, nb).astype(np.int64),
          rng.integers(0, 12, nb).astype(np.int32)]
    grp_pay = rng.integers(0, 6, nb).astype(np.int64)   # the group key
    pk = [rng.integers(0, 14, n).astype(np.int64),
          rng.integers(0, 14, n).astype(np.int64)]
    pn = [(rng.random(n) < 0.05).astype(np.uint8), None]
    val = rng.integers(-1000, 1000, n).astype(np.int64)
    cols, masks, _ = M.multikey_join(bk, None, [grp_pay], [val], pk, pn,
                                     None, M.PROBE_OUTER)
    exp = G.group_by([cols[1]], [masks],
                     [(G.SUM_I64, (G.IDENT, 0), None)], [cols[0]], [None])
    assert (None,) in exp and len(exp) >= 3
    with P.Scope() as s:
        table = _build(P, pl, s, bk, None, [grp_pay])
        j, raw = s.pipe(P.OP_LOOKUP_JOIN,
                        pl.left_join(table, [1, 2], [0]),
                        _page(P, "k", pk, pn, [("val", val)]))
        assert raw.n_rows == len(masks) and raw.cols[1].null_mask
        g = s.run(P.OP_GROUPBY_MULTI, pl.group_by(
            [1], [pl.sum_i64(pl.ident(0))], 64, sql_nulls=True), raw)
        out, nulls = g.get_output_nulls(["key", "sum", "cnt"])
    got = {}
    for i in range(len(out["key"])):
        key = None if nulls["key"][i] else int(out["key"][i])
        assert "sum" not in nulls or not nulls["sum"][i]
        got[(key,)] = ([int(out["sum"][i])], int(out["cnt"][i]))
    assert got == exp


# ---------------- 13. q9 ----------------

def test_q9_multikey_exact(P, oracle_lib):
    sf = 0.1
    li = oracle_lib.gen_lineitem2(sf)
    lpk = oracle_lib.gen_lineitem_partkey(sf)
    orders = oracle_lib.gen_orders(sf)
    supp = oracle_lib.gen_supplier(sf)
    ps = oracle_lib.gen_partsupp(sf)
    words = oracle_lib.gen_part_name_words(sf)
    names = [oracle_lib.color_name(i) for i in range(92)]
    strings = [" ".join(names[w] for w in row).encode() for row in words]
    n = len(strings)
    pages = (
        P.Page({"partkey": np.arange(1, n + 1, dtype=np.int64),
                "name": P.Varbin(strings)}),
        P.Page({"suppkey": supp["suppkey"], "nationkey": supp["nationkey"]}),
        P.Page({"orderkey": orders["orderkey"],
                "orderdate": orders["orderdate"]}),
        P.Page({"partkey": ps["partkey"], "suppkey": ps["suppkey"],
                "supplycost": ps["supplycost_cents"] / 100.0}),
        P.Page({"partkey": lpk, "suppkey": li["suppkey"],
                "orderkey": li["orderkey"], "quantity": li["quantity"],
                "extendedprice": li["extendedprice"],
                "discount": li["discount"]}))
    f = P.engine.lib().c.pg_multikey_probe_pages
    before = f()
    got = P.pipelines.q9_multikey(*pages)
    assert f() == before + 1
    gid = oracle_lib.color_id("green")
    p_match = (words == gid).any(axis=1).astype(np.uint8)
    exp = oracle_lib.q9(li, lpk, orders, supp, ps, p_match)
    got_a = np.array(got, dtype=np.int64)
    assert np.array_equal(got_a, exp)
    assert np.abs(got_a).sum() > 0
    assert got == P.pipelines.q9(*pages)
