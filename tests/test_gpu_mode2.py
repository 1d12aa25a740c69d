"""LOOKUP_JOIN mode 2 (the single-pass Q5 probe) and the dense-array fills
it reads, against the row-at-a-time references of mode2_refs.

Mode 2 has two kernels behind one contract: k_probe_agg_q5<8> for the Q5
shape and the generic k_probe_agg_fused2<8>.  JoinOp::add_input picks per
page: packed table, no preds, DISC_PRICE, I64 key and suppkey, F64 price
and discount, dec_scale 4, both key columns 16-byte aligned, no null mask
on any of the four columns.  pg_mode2_q5_launches() counts the pages that
went to the specialised kernel, and every probe here asserts the count it
expects, so no parity is vacuous: every variant below changes exactly one
term of the gate, named in VARIANTS.

The tables are built the way pipelines.Q5PipelineFused builds them: a dense
customer dimension, an agg_table orders build with payload_lookup_table, a
dense supplier table; the probe is mode 2 with disc_price and dec_scale 4.
Ticks and counts are compared as ints, sum_f64 bitwise: the contract is the
correctly rounded exact sum.  Money is non-negative exact hundredths
(edge_refs.ticks_exact), inside the two documented mode-2 exceptions.

Tile edges: k_probe_agg_q5 owns two rows per thread, 256 threads a block,
4096 blocks; k_probe_agg_fused2 one row per thread on the same grid; the
dense fills run 2048 blocks of 256 threads, one row per thread.
"""
import ctypes as C

import numpy as np
import pytest

import mode2_refs as M
from edge_refs import ticks_exact

pytestmark = pytest.mark.gpu

I64_MAX = (1 << 63) - 1
GRID, BLOCK = 4096, 256
FILL_GRID = 2048
N_CUST, N_SUPP, N_NAT = 50, 64, 12
BMAX = 1300                      # bitmap_max_key of the orders build
GV = (3, 11, 5, 7, 9)            # group_vals, deliberately not sorted
N_BASE = 4099

# name -> the one term of the gate the variant changes (None: it takes the
# specialised kernel)
VARIANTS = {
    "q5": None,
    "q5_bitmap": None,                    # kbits non-null, same gate
    "unpacked": "t->pack_bits > 0",
    "true_pred": "plan.n_preds == 0",
    "skey_i32": "table2_key_col tag == I64",
    "dc_null_mask": "no null_mask on proj.b",
    "misaligned_key": "key column 16-byte aligned",
}
SPEC, GENERIC = "q5_bitmap", "true_pred"
BOTH = [SPEC, GENERIC]


@pytest.fixture(scope="module")
def P():
    import presto_amd
    return presto_amd


@pytest.fixture(scope="module")
def pl(P):
    return P.plans


def _free(P, *ops):
    for op in ops:
        P.lib().c.pg_table_destroy(op.table())
        op.destroy()


def _build(P, plan, *pages):
    b = P.Operator(P.OP_HASH_BUILD, plan)
    try:
        for pg in pages:
            b.add_input(pg)
        b.finish()
    except BaseException:
        b.destroy()
        raise
    return b


# --------------------------------------------------------------------- #
# data                                                                   #
# --------------------------------------------------------------------- #
class Data:
    """The three build inputs, their reference tables, and probe columns."""

    def __init__(self, cust_nat, okeys, ocust, supp_keys, supp_nat, probe):
        self.cust_nat = np.asarray(cust_nat, np.uint8)
        self.okeys = np.asarray(okeys, np.int64)
        self.ocust = np.asarray(ocust, np.int64)
        self.supp_keys = np.asarray(supp_keys, np.int64)
        self.supp_nat = np.asarray(supp_nat, np.uint8)
        self.n_supp = N_SUPP
        # reference tables: the customer dimension is dense over 1..n, an
        # orders row whose custkey is outside it is dropped by the build
        self.table = {int(k): int(self.cust_nat[c - 1])
                      for k, c in zip(self.okeys, self.ocust)
                      if 1 <= c <= len(self.cust_nat)}
        self.dense2 = M.dense_fill_ref(self.supp_keys, self.supp_nat,
                                       self.n_supp, 0, None, np.uint8)
        self.set_probe(*probe)

    def set_probe(self, okey, skey, cents, dcents):
        self.okey = np.asarray(okey, np.int64)
        self.skey = np.asarray(skey, np.int64)
        self.cents = np.asarray(cents, np.int64)
        self.dcents = np.asarray(dcents, np.int64)
        self.ep, _ = ticks_exact(self.cents, 2)
        self.dc, _ = ticks_exact(self.dcents, 2)
        return self

    def cols(self, lo=0, hi=None):
        return {"ok": self.okey[lo:hi], "sk": self.skey[lo:hi],
                "ep": self.ep[lo:hi], "dc": self.dc[lo:hi]}

    def group_index(self, group_vals=GV, sel=None):
        return M.mode2_group_index(self.table, self.dense2, self.okey,
                                   self.skey, sel, group_vals)

    def ref(self, group_vals=GV, sel=None, gi=None):
        if gi is None:
            gi = self.group_index(group_vals, sel)
        return M.mode2_aggregate(gi, self.cents, self.dcents, self.ep,
                                 self.dc, group_vals)


def _base_data():
    """About 300 order keys of which about 40 % are in the table, probe
    keys clustered in runs as lineitem is, 64 suppliers, nations 1..12.
    Half of the rows of a present order take a supplier of the customer's
    nation, so that the local-supplier equality keeps a fair share."""
    rng = np.random.RandomState(20240521)
    cust_nat = rng.randint(1, N_NAT + 1, N_CUST)
    cand = np.sort(rng.permutation(BMAX - 2)[:300] + 1)
    present = cand[rng.rand(300) < 0.4]
    ocust = rng.randint(1, N_CUST + 1, len(present))
    ocust[:3] = [0, N_CUST + 1, -7]          # dropped by the build's lookup
    supp_nat = rng.randint(1, N_NAT + 1, N_SUPP)
    d = Data(cust_nat, present, ocust, np.arange(1, N_SUPP + 1), supp_nat,
             ([], [], [], []))
    by_nat = {n: np.flatnonzero(supp_nat == n) + 1
              for n in range(1, N_NAT + 1)}
    okey, skey = [], []
    while len(okey) < N_BASE:
        k = int(cand[rng.randint(300)])
        for _ in range(rng.randint(1, 8)):
            nat = d.table.get(k)
            if nat is not None and len(by_nat[nat]) and rng.rand() < 0.5:
                s = int(rng.choice(by_nat[nat]))
            else:
                s = int(rng.randint(1, N_SUPP + 1))
            okey.append(k)
            skey.append(s)
    okey, skey = okey[:N_BASE], skey[:N_BASE]
    # money from 1.00 to 99999.99, discounts 0.00 to 0.10
    cents = rng.randint(100, 10_000_000, N_BASE)
    dcents = rng.randint(0, 11, N_BASE)
    return d.set_probe(okey, skey, cents, dcents)


@pytest.fixture(scope="module")
def base():
    d = _base_data()
    d.gi = d.group_index()
    d.rows, ovf = d.ref(gi=d.gi)
    assert not ovf
    # the data exercises what it is meant to
    hit = np.array([int(k) in d.table for k in d.okey])
    assert 0.25 < hit.mean() < 0.6
    assert [r[0] for r in d.rows] == list(GV)
    assert all(r[3] >= 20 for r in d.rows)
    assert len(d.table) == len(d.okeys) - 3
    return d


@pytest.fixture(scope="module")
def hits(base):
    """Rows that all accumulate, with distinct amounts: losing any one row
    (a dropped pair tail, a block edge) changes a tick sum."""
    idx = np.resize(np.flatnonzero(base.gi >= 0), 513)
    cents = base.cents[idx] + np.arange(513) * 1000
    d = Data(base.cust_nat, base.okeys, base.ocust, base.supp_keys,
             base.supp_nat, (base.okey[idx], base.skey[idx], cents,
                             base.dcents[idx]))
    assert (d.group_index() >= 0).all()
    return d


# --------------------------------------------------------------------- #
# tables and probe                                                       #
# --------------------------------------------------------------------- #
class Tables:
    """Customer dimension, orders agg_table and supplier table of one
    Data, built once per orders shape and freed on exit."""

    def __init__(self, P, d, pack_bits=8, bitmap_max_key=0):
        pl = P.plans
        self.P = P
        self.ops = []
        try:
            b1 = self._add(pl.hash_build(
                0, payload=[1], capacity_hint=len(d.cust_nat),
                dense_array=1),
                P.Page({"ck": np.arange(1, len(d.cust_nat) + 1,
                                        dtype=np.int64),
                        "nat": d.cust_nat}))
            self.orders = self._add(pl.hash_build(
                0, payload=[0], payload_lookup_table=b1.table(),
                payload_lookup_key_col=1,
                capacity_hint=max(len(d.okeys), 64), agg_table=1,
                pack_bits=pack_bits, bitmap_max_key=bitmap_max_key),
                P.Page({"ok": d.okeys, "ck": d.ocust}))
            self.supp = self._add(pl.hash_build(
                0, payload=[1], capacity_hint=d.n_supp, dense_array=1,
                semijoin_table=0),
                P.Page({"sk": d.supp_keys, "nat": d.supp_nat}))
        except BaseException:
            self.close()
            raise

    def _add(self, plan, page):
        b = _build(self.P, plan, page)
        self.ops.append(b)
        return b

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    def close(self):
        while self.ops:
            _free(self.P, self.ops.pop())


def _tables(P, d, variant):
    return Tables(P, d, pack_bits=0 if variant == "unpacked" else 8,
                  bitmap_max_key=0 if variant == "q5" else BMAX)


def _page(P, cols, variant):
    """The probe page of a variant: channels ok, sk, ep, dc."""
    import torch
    ok, sk, ep, dc = (cols[c] for c in ("ok", "sk", "ep", "dc"))
    if variant == "skey_i32":
        return P.Page({"ok": ok, "sk": sk.astype(np.int32), "ep": ep,
                       "dc": dc})
    if variant == "dc_null_mask":
        return P.Page(dict(cols), nulls={"dc": np.zeros(len(ok), np.uint8)})
    if variant == "misaligned_key":
        # a device key column that starts one element into its buffer:
        # 8-byte but not 16-byte aligned
        buf = torch.zeros(len(ok) + 1, dtype=torch.int64, device="cuda")
        buf[1:] = torch.from_numpy(np.ascontiguousarray(ok)).cuda()
        kview = buf[1:]
        assert kview.data_ptr() % 16 == 8
        dev = {c: torch.from_numpy(np.ascontiguousarray(a)).cuda()
               for c, a in (("sk", sk), ("ep", ep), ("dc", dc))}
        assert dev["sk"].data_ptr() % 16 == 0
        return P.Page({"ok": kview, **dev})
    return P.Page(dict(cols))


def _preds(P, variant):
    # suppkey >= -2^40: true for every row of every test here
    return [P.plans.pred(1, P.CMP_GE, -(1 << 40))] \
        if variant == "true_pred" else []


def _q5_launches(P):
    f = P.lib().c.pg_mode2_q5_launches
    f.restype = C.c_int64
    return f()


def _spec_pages(variant, n_pages):
    """How many of a variant's pages pass the gate."""
    return n_pages if VARIANTS[variant] is None else 0


def _probe(P, t, pages, group_vals=GV, preds=(), *, spec_pages):
    """Mode 2 over the pages; the output page as a list of
    (group, ticks, f64 bits, count).  spec_pages of the pages must have
    gone to k_probe_agg_q5 and the rest to k_probe_agg_fused2; that is
    checked before finish, so also when finish raises."""
    pl = P.plans
    before = _q5_launches(P)
    j = P.Operator(P.OP_LOOKUP_JOIN, pl.lookup_join(
        t.orders.table(), 0, 2, preds=preds, proj=pl.disc_price(2, 3),
        dec_scale=4, table2=t.supp.table(), table2_key_col=1,
        group_vals=group_vals))
    try:
        for pg in pages:
            j.add_input(pg)
        assert _q5_launches(P) - before == spec_pages
        j.finish()
        out = j.get_output(["g", "ticks", "f64", "cnt"])
    finally:
        j.destroy()
    assert out is not None and sorted(out) == ["cnt", "f64", "g", "ticks"]
    assert out["g"].dtype == np.uint8 and out["f64"].dtype == np.float64
    return [(int(g), int(t_), int(f.view(np.int64)), int(c))
            for g, t_, f, c in zip(out["g"], out["ticks"], out["f64"],
                                   out["cnt"])]


def _bits(rows):
    return [(g, t, int(np.float64(f).view(np.int64)), c)
            for g, t, f, c in rows]


def _run(P, d, variant, group_vals=GV, splits=None):
    splits = splits or [0, len(d.okey)]
    with _tables(P, d, variant) as t:
        pages = [_page(P, d.cols(lo, hi), variant)
                 for lo, hi in zip(splits, splits[1:])]
        return _probe(P, t, pages, group_vals, _preds(P, variant),
                      spec_pages=_spec_pages(variant, len(pages)))


# --------------------------------------------------------------------- #
# a. both kernels, one answer                                            #
# --------------------------------------------------------------------- #
@pytest.mark.parametrize("variant", list(VARIANTS))
def test_variants_equal_reference(P, base, variant):
    """The base data through each shape: the two that pass the gate take
    k_probe_agg_q5, each of the others fails the one term VARIANTS names
    and takes k_probe_agg_fused2 (_probe asserts the launch count).  All
    equal mode2_ref, so they equal each other."""
    assert _run(P, base, variant) == _bits(base.rows)


def test_pred_that_drops_rows(P, base):
    """sel is the conjunction of preds: suppkey > 20 on the generic
    kernel."""
    sel = base.skey > 20
    rows, _ = base.ref(sel=sel)
    assert rows != base.rows
    with _tables(P, base, GENERIC) as t:
        got = _probe(P, t, [P.Page(base.cols())],
                     preds=[P.plans.pred(1, P.CMP_GT, 20)], spec_pages=0)
    assert got == _bits(rows)


# --------------------------------------------------------------------- #
# b. row edges                                                           #
# --------------------------------------------------------------------- #
def _edge_data():
    """Nation per customer = the custkey (customer 0's nation is 0, stored
    as custkey 13 -> 0); supplier s has nation s for s <= 12 except the
    unfilled slot 4; supplier cap = 64 has nation 3."""
    cust_nat = list(range(1, 13)) + [0]
    okeys = [1, 5, 6, 8, BMAX, 20, 21, 22, 23]
    ocust = [3, 3, 5, 7, 9, 13, 4, 2, 3]     # -> nations 3 3 5 7 9 0 4 2 3
    supp_keys = [s for s in range(1, N_SUPP + 1) if s != 4]
    supp_nat = [s if s <= 12 else 1 for s in supp_keys]
    supp_nat[-1] = 3
    rows = [
        # probe key edges; the supplier is a listed nation so that a false
        # hit could not hide
        (0, 3), (-1, 3), (I64_MAX, 3), (BMAX + 1, 3),
        (7, 3), (4, 3), (2, 3),      # 6 and 8, 5, 1 are neighbours in the table
        (BMAX, 9),                   # the bitmap's last key is a hit
        # suppkey edges on order 1 (nation 3): 64 = cap lands, 3 lands
        (1, 0), (1, -5), (1, 1), (1, N_SUPP), (1, N_SUPP + 1), (1, 3),
        (1, I64_MAX), (1, -I64_MAX - 1),
        (20, 4),                     # g1 = 0 = the unfilled slot; 0 unlisted
        (21, 4),                     # g1 = 4, unfilled slot reads 0
        (6, 7), (8, 5),              # supplier nation differs
        (22, 2),                     # equal nations, 2 is not in group_vals
        (5, 3), (6, 5), (8, 7), (23, N_SUPP),
    ]
    okey, skey = zip(*rows)
    cents = 100 + 17 * np.arange(len(rows))
    d = Data(cust_nat, okeys, ocust, supp_keys, supp_nat,
             (okey, skey, cents, np.arange(len(rows)) % 11))
    return d


@pytest.mark.parametrize("variant", BOTH)
def test_row_edges(P, variant):
    d = _edge_data()
    gi = d.group_index()
    gv = list(GV)
    want = [-1] * 7 + [gv.index(9)] + [-1, -1, -1, 0, -1, 0, -1, -1] + \
        [-1] * 5 + [0, gv.index(5), gv.index(7), 0]
    assert list(gi) == want          # the reference, by hand
    rows, _ = d.ref(gi=gi)
    assert _run(P, d, variant) == _bits(rows)
    # the same rows twice over, so that the edge rows also sit in the
    # second slot of a thread's pair
    d2 = Data(d.cust_nat, d.okeys, d.ocust, d.supp_keys, d.supp_nat,
              (np.r_[d.okey[:1], d.okey], np.r_[d.skey[:1], d.skey],
               np.r_[d.cents[:1], d.cents], np.r_[d.dcents[:1], d.dcents]))
    rows2, _ = d2.ref()
    assert rows2 == rows             # the added row is a miss
    assert _run(P, d2, variant) == _bits(rows)


# --------------------------------------------------------------------- #
# c. n_group_vals                                                        #
# --------------------------------------------------------------------- #
@pytest.mark.parametrize("variant", BOTH)
def test_one_and_eight_group_vals(P, base, variant):
    """13 is no nation: its group is absent and the others keep the order
    of group_vals."""
    one = (7,)
    rows1, _ = base.ref(group_vals=one)
    assert len(rows1) == 1
    eight = (11, 2, 13, 7, 5, 1, 9, 4)
    rows8, _ = base.ref(group_vals=eight)
    assert [r[0] for r in rows8] == [11, 2, 7, 5, 1, 9, 4]
    with _tables(P, base, variant) as t:
        page = _page(P, base.cols(), variant)
        pr = _preds(P, variant)
        sp = _spec_pages(variant, 1)
        assert _probe(P, t, [page], one, pr, spec_pages=sp) == _bits(rows1)
        assert _probe(P, t, [page], eight, pr, spec_pages=sp) == \
            _bits(rows8)


@pytest.mark.parametrize("n", [0, 9])
def test_n_group_vals_out_of_range(P, base, n):
    pl = P.plans
    with _tables(P, base, SPEC) as t:
        plan = pl.lookup_join(
            t.orders.table(), 0, 2, proj=pl.disc_price(2, 3), dec_scale=4,
            table2=t.supp.table(), table2_key_col=1, group_vals=GV)
        plan.n_group_vals = n
        with pytest.raises(RuntimeError, match=r"n_group_vals must be 1\.\.8"):
            P.Operator(P.OP_LOOKUP_JOIN, plan)


# --------------------------------------------------------------------- #
# d. row counts                                                          #
# --------------------------------------------------------------------- #
@pytest.mark.parametrize("variant", BOTH)
@pytest.mark.parametrize("n", [0, 1, 2, 3, 511, 512, 513])
def test_row_counts(P, hits, variant, n):
    """Every row accumulates, so a lost pair tail (odd n) or block edge
    (2 x 256 rows are one block of the specialised kernel, 256 one of the
    generic) is a wrong sum."""
    d = Data(hits.cust_nat, hits.okeys, hits.ocust, hits.supp_keys,
             hits.supp_nat, (hits.okey[:n], hits.skey[:n], hits.cents[:n],
                             hits.dcents[:n]))
    rows, _ = d.ref()
    assert sum(r[3] for r in rows) == n
    assert _run(P, d, variant) == _bits(rows)


@pytest.mark.parametrize("variant", BOTH)
def test_page_longer_than_one_grid_pass(P, base, hits, variant):
    """2 x 4096 x 256 + 3 rows: one full pass of the specialised kernel's
    grid (two of the generic one's) and three rows more, which are hits.
    The columns are the base data tiled; so is the reference's group
    index."""
    n = 2 * GRID * BLOCK + 3

    def tile(a, h):
        out = np.resize(a, n)
        out[-3:] = h[:3]
        return out

    d = Data(base.cust_nat, base.okeys, base.ocust, base.supp_keys,
             base.supp_nat,
             (tile(base.okey, hits.okey), tile(base.skey, hits.skey),
              tile(base.cents, hits.cents), tile(base.dcents, hits.dcents)))
    gi = tile(base.gi, hits.group_index())
    assert (gi[-3:] >= 0).all()
    rows, ovf = d.ref(gi=gi)
    assert not ovf and sum(r[3] for r in rows) == int((gi >= 0).sum())
    assert _run(P, d, variant) == _bits(rows)


# --------------------------------------------------------------------- #
# e. pages                                                               #
# --------------------------------------------------------------------- #
@pytest.mark.parametrize("variant", BOTH)
def test_two_pages_accumulate(P, base, variant):
    assert _run(P, base, variant, splits=[0, 2049, N_BASE]) == \
        _bits(base.rows)


def test_one_operator_both_kernels(P, base):
    """The first page passes the gate, the second (misaligned key view)
    does not: one operator, both kernels, one set of accumulators."""
    with _tables(P, base, SPEC) as t:
        pages = [_page(P, base.cols(0, 2049), SPEC),
                 _page(P, base.cols(2049, None), "misaligned_key")]
        assert _probe(P, t, pages, spec_pages=1) == _bits(base.rows)


@pytest.mark.parametrize("variant", BOTH)
@pytest.mark.parametrize("empty_page", [False, True])
def test_no_rows_gives_empty_four_column_page(P, base, variant, empty_page):
    with _tables(P, base, variant) as t:
        pages = [_page(P, base.cols(0, 0), variant)] if empty_page else []
        assert _probe(P, t, pages, GV, _preds(P, variant),
                      spec_pages=_spec_pages(variant, len(pages))) == []


# --------------------------------------------------------------------- #
# f. table-shape errors                                                  #
# --------------------------------------------------------------------- #
def _mode2_plan(pl, table, table2):
    return pl.lookup_join(table, 0, 2, proj=pl.disc_price(2, 3),
                          dec_scale=4, table2=table2, table2_key_col=1,
                          group_vals=GV)


def test_table_shape_errors(P, pl, base):
    keys = np.arange(1, 9, dtype=np.int64)
    chained = _build(P, pl.hash_build(0, payload=[1], capacity_hint=8),
                     P.Page({"k": keys, "v": keys + 100}))
    i32pay = _build(P, pl.hash_build(0, payload=[1], capacity_hint=8,
                                     agg_table=1),
                    P.Page({"k": keys, "v": keys.astype(np.int32)}))
    try:
        with _tables(P, base, SPEC) as t:
            for tbl in (chained, i32pay):
                with pytest.raises(
                        RuntimeError,
                        match="mode 2 probes an agg_table with one u8 "
                              "payload"):
                    P.Operator(P.OP_LOOKUP_JOIN, _mode2_plan(
                        pl, tbl.table(), t.supp.table()))
            with pytest.raises(RuntimeError,
                               match="mode 2 needs a dense_array table2"):
                P.Operator(P.OP_LOOKUP_JOIN, _mode2_plan(
                    pl, t.orders.table(), chained.table()))
    finally:
        _free(P, chained, i32pay)


# --------------------------------------------------------------------- #
# g. tick overflow                                                       #
# --------------------------------------------------------------------- #
def _big_rows(n, hit=None):
    """Rows of 9.0e13 at no discount on one supplier and group: in the f64
    domain (ep * 100 < 2^53), 9e17 ticks each.  hit[i] says whether row i
    probes order 1, which is in the table, or order 2, which is not; the
    default is n hits."""
    hit = np.ones(n, bool) if hit is None else np.asarray(hit, bool)
    n = len(hit)
    d = Data([3], [1], [1], [1], [3],
             (np.where(hit, 1, 2), [1] * n, [9 * 10 ** 15] * n, [0] * n))
    assert d.ep[0] == 9.0e13 and d.ep[0] * 100.0 < 2.0 ** 53
    assert int((d.group_index((3,)) >= 0).sum()) == int(hit.sum())
    return d


@pytest.mark.parametrize("variant", BOTH)
def test_tick_sum_that_fits(P, variant):
    d = _big_rows(10)
    rows, ovf = d.ref(group_vals=(3,))
    assert not ovf and rows == [(3, 9 * 10 ** 18, 9.0e14, 10)]
    assert _run(P, d, variant, group_vals=(3,)) == _bits(rows)


_I = np.arange(64)
# where the 9e17-tick rows sit in the first wave.  The generic kernel gives
# row i to lane i, the specialised one rows 2t and 2t + 1 to lane t.  In
# the xor butterfly a lane performs six of the tree's 63 adds, so with the
# hits in the odd lanes only, the add that leaves int64 happens in a lane
# other than the one that publishes the total: lane 0 then adds a
# non-negative value and an already wrapped negative one, which does not
# overflow.
OVERFLOW_LAYOUTS = {
    "first_16_rows": np.ones(16, bool),          # lanes 0..15 / 0..7
    "odd_rows_of_32": _I[:32] % 2 == 1,          # generic: 16 odd lanes
    "odd_rows_of_64": _I % 2 == 1,               # generic: 32 odd lanes
    "odd_pairs_of_64": (_I // 2) % 2 == 1,       # specialised: 16 odd lanes
    "first_row_of_odd_pairs": _I % 4 == 2,       # one row in each of them
    "odd_pairs_of_128": (np.arange(128) // 2) % 2 == 1,  # all 32 odd lanes
}


@pytest.mark.parametrize("variant", BOTH)
@pytest.mark.parametrize("layout", list(OVERFLOW_LAYOUTS))
def test_tick_overflow_raises(P, variant, layout):
    """Sixteen or more rows of 9e17 ticks in one wave and one group: the
    exact sum of at least 1.44e19 leaves int64, so finish must raise
    (Math.addExact semantics) and not hand back a wrapped wave total,
    whichever lane's add it was that wrapped."""
    d = _big_rows(0, OVERFLOW_LAYOUTS[layout])
    rows, ovf = d.ref(group_vals=(3,))
    assert ovf and rows[0][3] >= 16 and rows[0][1] > I64_MAX
    with pytest.raises(RuntimeError, match="decimal SUM overflow"):
        _run(P, d, variant, group_vals=(3,))


# --------------------------------------------------------------------- #
# h. dense fills, read back through a mode-0 emit join (a key set, which #
#    the emit joins refuse, through a semijoin)                          #
# --------------------------------------------------------------------- #
def _dense_read(P, build, cap):
    """{key: value} as an emit join on the dense table sees it: every key
    of -1 .. cap + 2 is probed once."""
    pk = np.arange(-1, cap + 3, dtype=np.int64)
    j = P.Operator(P.OP_LOOKUP_JOIN,
                   P.plans.emit_join(build.table(), 0, [0]))
    try:
        j.add_input(P.Page({"k": pk}))
        out = j.get_output(["k", "v"])
    finally:
        j.destroy()
    assert len(set(out["k"].tolist())) == len(out["k"])
    return {int(k): int(v) for k, v in zip(out["k"], out["v"])}, \
        out["v"].dtype


def _key_set_read(P, build, cap):
    """The members of a dense key set.  The emit joins refuse a key-set-only
    table, so the keys -1 .. cap + 2 go through a FILTER_PROJECT semijoin on
    it and the survivors are the set."""
    pl = P.plans
    pk = np.arange(-1, cap + 3, dtype=np.int64)
    f = P.Operator(P.OP_FILTER_PROJECT, pl.filter_project(
        [pl.ident(0)], semijoin_table=build.table(), semijoin_col=0))
    try:
        f.add_input(P.Page({"k": pk}))
        out = f.get_output(["k"])
    finally:
        f.destroy()
    return sorted(int(k) for k in out["k"])


def _fill_and_read(P, plan, pages, cap, read=_dense_read):
    b = _build(P, plan, *pages)
    try:
        return read(P, b, cap)
    finally:
        _free(P, b)


EDGE_KEYS = [0, -1, 9, 10, 3, 7, 1]      # cap = 9: of the first four only
EDGE_VALS = [9, 9, 21, 9, 0, 255, 254]   # cap lands


@pytest.mark.parametrize("bias", [0, 1])
def test_dense_fill_u8(P, pl, bias):
    """k_dense_fill: keys 0, -1, cap, cap + 1; a payload of 0 and the u8
    wrap of 255 + 1.  Presence is "nonzero": with bias 0 the key that
    stores 0 is absent from the join, with bias 1 it is present as 1 (what
    dense_payload_bias is for) and 255 wraps to absent."""
    cap = 9
    keys = np.array(EDGE_KEYS, np.int64)
    vals = np.array(EDGE_VALS, np.uint8)
    ref = M.dense_present(M.dense_fill_ref(keys, vals, cap, bias, None,
                                           np.uint8))
    assert ref == ({9: 21, 7: 255, 1: 254} if bias == 0 else
                   {9: 22, 3: 1, 1: 255})
    got, dt = _fill_and_read(P, pl.hash_build(
        0, payload=[1], capacity_hint=cap, dense_array=1,
        dense_payload_bias=bias), [P.Page({"k": keys, "v": vals})], cap)
    assert got == ref and dt == np.uint8


def test_dense_fill_i32_bias_and_negative_values(P, pl):
    """k_dense_fill32 with bias 1: negative payloads stay negative, -1 + 1
    is 0 and so absent, values past a byte are kept whole."""
    cap = 9
    keys = np.array(EDGE_KEYS + [2, 4], np.int64)
    vals = np.array([9, 9, -40000, 9, 0, 70000, -1, -2, 255], np.int32)
    ref = M.dense_present(M.dense_fill_ref(keys, vals, cap, 1, None,
                                           np.int32))
    assert ref == {9: -39999, 3: 1, 7: 70001, 2: -1, 4: 256}
    got, dt = _fill_and_read(P, pl.hash_build(
        0, payload=[1], capacity_hint=cap, dense_array=1,
        dense_payload_bias=1), [P.Page({"k": keys, "v": vals})], cap)
    assert got == ref and dt == np.int32


def test_dense_key_set_pred_and_two_pages(P, pl):
    """key_set_only stores flag 1 whatever the bias (the reference shows
    it; the device set is read by membership); a build pred drops rows;
    two pages fill one array."""
    cap = 300
    rng = np.random.RandomState(5)
    keys = (rng.permutation(cap + 20) - 9).astype(np.int64)  # -9 .. cap+10
    d = rng.randint(0, 100, len(keys)).astype(np.int32)
    sel = d < 50
    ref = M.dense_present(M.dense_fill_ref(keys, None, cap, 3, sel,
                                           np.uint8))
    assert 100 < len(ref) < 200 and set(ref.values()) == {1}
    h = len(keys) // 2 + 1
    pages = [P.Page({"k": keys[:h], "d": d[:h]}),
             P.Page({"k": keys[h:], "d": d[h:]})]
    got = _fill_and_read(P, pl.hash_build(
        0, preds=[pl.pred(1, P.CMP_LT, 50)], capacity_hint=cap,
        key_set_only=1, dense_array=1, dense_payload_bias=3), pages, cap,
        read=_key_set_read)
    assert got == sorted(ref)
    # the same two pages with a u8 payload and the pred
    vals = rng.randint(1, 256, len(keys)).astype(np.uint8)
    ref = M.dense_present(M.dense_fill_ref(keys, vals, cap, 0, sel,
                                           np.uint8))
    pages = [P.Page({"k": keys[:h], "d": d[:h], "v": vals[:h]}),
             P.Page({"k": keys[h:], "d": d[h:], "v": vals[h:]})]
    got, _ = _fill_and_read(P, pl.hash_build(
        0, preds=[pl.pred(1, P.CMP_LT, 50)], payload=[2],
        capacity_hint=cap, dense_array=1), pages, cap)
    assert got == ref


def test_dense_payload_tag_change_raises(P, pl):
    keys = np.arange(1, 5, dtype=np.int64)
    b = P.Operator(P.OP_HASH_BUILD, pl.hash_build(
        0, payload=[1], capacity_hint=8, dense_array=1))
    try:
        b.add_input(P.Page({"k": keys, "v": keys.astype(np.uint8)}))
        with pytest.raises(RuntimeError,
                           match="dense_array payload tag changed across "
                                 "pages"):
            b.add_input(P.Page({"k": keys + 4, "v": keys.astype(np.int32)}))
    finally:
        b.destroy()


def test_dense_semijoin_raises(P, pl):
    keys = np.arange(1, 5, dtype=np.int64)
    flags = _build(P, pl.flag_set(0, 8), P.Page({"k": keys}))
    b = P.Operator(P.OP_HASH_BUILD, pl.hash_build(
        0, payload=[1], capacity_hint=8, dense_array=1,
        semijoin_table=flags.table(), semijoin_col=0))
    try:
        with pytest.raises(RuntimeError,
                           match="dense_array builds do not evaluate "
                                 "semijoins"):
            b.add_input(P.Page({"k": keys, "v": keys.astype(np.uint8)}))
    finally:
        b.destroy()
        _free(P, flags)


def _lookup(P, pl, lu_vals):
    n = len(lu_vals)
    return _build(P, pl.hash_build(0, payload=[1], capacity_hint=n,
                                   dense_array=1),
                  P.Page({"k": np.arange(1, n + 1, dtype=np.int64),
                          "v": np.asarray(lu_vals, np.uint8)}))


@pytest.mark.parametrize("bias", [0, 1])
def test_dense_fill_through_lookup(P, pl, bias):
    """k_dense_fill_lu: k2 = 0 and lu_cap + 1 miss and leave the key absent
    from the join, 1 and lu_cap are looked up; a looked-up 0 is a hit that
    only the bias makes visible; keys 0, -1, cap + 1 never land."""
    lu_vals = [6, 0, 255, 17]              # lu_cap = 4
    cap = 9
    keys = np.array([1, 2, 3, 4, 5, 6, 0, -1, 9, 10], np.int64)
    k2 = np.array([0, 1, 4, 5, 2, 3, 1, 1, 4, 1], np.int64)
    ref = M.dense_present(M.dense_fill_lu_ref(
        keys, k2, np.array(lu_vals, np.uint8), cap, bias, None))
    assert ref == ({2: 6, 3: 17, 6: 255, 9: 17} if bias == 0 else
                   {2: 7, 3: 18, 5: 1, 9: 18})
    lu = _lookup(P, pl, lu_vals)
    try:
        got, dt = _fill_and_read(P, pl.hash_build(
            0, payload=[0], payload_lookup_table=lu.table(),
            payload_lookup_key_col=1, capacity_hint=cap, dense_array=1,
            dense_payload_bias=bias), [P.Page({"k": keys, "c": k2})], cap)
    finally:
        _free(P, lu)
    assert got == ref and dt == np.uint8


@pytest.mark.parametrize("kernel", ["u8", "i32", "lookup"])
@pytest.mark.parametrize("n", [0, 1, 257, FILL_GRID * BLOCK + 1])
def test_dense_fill_row_counts(P, pl, kernel, n):
    """Each fill at 0 rows, 1 row, one row past a block and one row past a
    full pass of its grid; every key of 1..n once, in random order, with
    bias 1 so that every row is visible."""
    rng = np.random.RandomState(100 + n % 1000)
    cap = max(n, 1)
    keys = (rng.permutation(n) + 1).astype(np.int64)
    plan = dict(capacity_hint=cap, dense_array=1, dense_payload_bias=1)
    lu = None
    if kernel == "lookup":
        lu_vals = rng.randint(0, 255, 37)
        k2 = rng.randint(1, 38, n).astype(np.int64)
        ref = M.dense_fill_lu_ref(keys, k2, lu_vals.astype(np.uint8), cap,
                                  1, None)
        lu = _lookup(P, pl, lu_vals)
        plan.update(payload=[0], payload_lookup_table=lu.table(),
                    payload_lookup_key_col=1)
        page = P.Page({"k": keys, "c": k2})
    else:
        dt = np.uint8 if kernel == "u8" else np.int32
        vals = (rng.randint(0, 255, n) if kernel == "u8" else
                rng.randint(-(1 << 30), 1 << 30, n)).astype(dt)
        if kernel == "i32":
            vals[vals == -1] = 5           # -1 + 1 would be absent
        ref = M.dense_fill_ref(keys, vals, cap, 1, None, dt)
        plan.update(payload=[1])
        page = P.Page({"k": keys, "v": vals})
    assert np.count_nonzero(ref) == n
    try:
        got, _ = _fill_and_read(P, pl.hash_build(0, **plan), [page], cap)
    finally:
        if lu is not None:
            _free(P, lu)
    assert got == M.dense_present(ref)
