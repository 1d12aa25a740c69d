"""Query pipelines assembled from the C-ABI operators — the host analog of
LocalExecutionPlanner wiring OperatorFactories into a Driver
(presto-main-base/.../sql/planner/LocalExecutionPlanner.java:1663,2552,3648
for the ScanFilterAndProject / HashBuilder / HashAggregation factories) and
of the hand-wired pipelines in
presto-benchmark/.../HandTpchQuery1.java:30-110.

Plans come from the constructors in plans.py; every operator and hash
table lives in an engine.Scope, which frees whatever is still alive when
the query ends or fails.  Intermediates are still released EARLY where
noted: their buffers go back to the size-bucketed pool for the next
operator, which decides peak HBM and timing.  The pool hands out
same-size buffers in the order they came back, so the multi-table queries
also end with one explicit release in a fixed order (probes newest first,
then tables oldest first) instead of leaving it to the scope: which
physical buffer an operator gets next run is measurable (TPC-DS Q72:
2-3%).  The scope stays the backstop for errors.

Date constants: epoch-day literals from the benchmark SQL
(presto-benchto-benchmarks/.../tpch/q01.sql, q03.sql):
  Q1: shipdate <= DATE '1998-12-01' - 90 days = 1998-09-02 = 10471
  Q3: DATE '1995-03-15' = 9204
"""
import numpy as np

from . import plans as pl
from .engine import (
    Page, Scope,
    OP_FILTER_PROJECT, OP_GROUPBY_MULTI, OP_HASH_AGG_SMALL, OP_LOOKUP_JOIN,
    OP_ORDER_BY, OP_TOPN,
    CMP_LE, CMP_LT, CMP_GT, CMP_GE, CMP_EQ, CMP_NE, CMP_CONTAINS,
    CMP_PREFIX, CMP_CONTAINS2, CMP_NOT_CONTAINS2,
)

Q1_SHIP_MAX = 10471
Q3_DATE = 9204


def _ticks(r, i=0):
    """Row i of an exact SUM_DEC (hi, lo) output pair as a Python int."""
    return (int(r["hi"][i]) << 64) | int(np.uint64(r["lo"][i]))


def _agg_once(s, plan, page, names):
    """One small-key aggregation over a page, released as soon as read."""
    a = s.run(OP_HASH_AGG_SMALL, plan, page)
    r = a.get_output(names)
    s.release(a)
    return r


def q1_plan(page: Page, mode="f64"):
    qty = page.channel("quantity")
    ep = page.channel("extendedprice")
    dc = page.channel("discount")
    tx = page.channel("tax")
    sums = [(pl.ident(qty), 0), (pl.ident(ep), 2),
            (pl.disc_price(ep, dc), 4), (pl.charge(ep, dc, tx), 6),
            (pl.ident(dc), 2)]
    agg = pl.sum_dec if mode == "dec" else pl.sum_f64
    return pl.small_agg(
        [agg(proj, scale) for proj, scale in sums] + [pl.count()],
        preds=[pl.pred(page.channel("shipdate"), CMP_LE, Q1_SHIP_MAX)],
        keys=[(page.channel("returnflag"), b"ANR"),
              (page.channel("linestatus"), b"FO")])


Q1_F64_NAMES = ["returnflag", "linestatus", "sum_qty", "sum_base",
                "sum_disc_price", "sum_charge", "sum_disc", "count"]
Q1_DEC_NAMES = ["returnflag", "linestatus",
                "sum_qty_hi", "sum_qty_lo", "sum_base_hi", "sum_base_lo",
                "sum_disc_price_hi", "sum_disc_price_lo",
                "sum_charge_hi", "sum_charge_lo",
                "sum_disc_hi", "sum_disc_lo", "count"]


def q1(page: Page, mode="f64"):
    """Full Q1 over one lineitem page. Returns dict of numpy group columns
    (groups in (returnflag, linestatus) order)."""
    with Scope() as s:
        op = s.run(OP_HASH_AGG_SMALL, q1_plan(page, mode), page)
        return op.get_output(Q1_F64_NAMES if mode == "f64" else Q1_DEC_NAMES)


def okey_max(n_orders):
    """Largest o_orderkey for an n_orders-row orders table: dbgen's
    mk_sparse keeps the low 3 index bits and shifts the rest up by 2
    (oracle/tpchgen.c:141-145), which is monotone in the row index."""
    return ((n_orders >> 3) << 5) | (n_orders & 7)


class Q3Pipeline:
    """Q3 operator graph, reusable across inputs (tables freed on close).

    customer(BUILDING) -> key set          [HashBuilderOperator analog]
    orders(date<9204) semijoin set -> tbl  [HashBuilder w/ fused filter]
    lineitem(date>9204) probe tbl          [LookupJoin + fused grouped SUM]
    groups -> TopN 10 (rev desc, odate asc, okey asc)
    """

    def __init__(self, cust: Page, orders: Page, mode="dec", limit=10):
        self.mode = mode
        self.limit = limit
        self.scope = Scope()
        with self.scope.on_error() as s:
            # 1-byte membership flags, L2/L3-resident (custkeys dense 1..n)
            b1 = s.build(pl.flag_set(
                cust.channel("custkey"), cust.n_rows,
                preds=[pl.pred(cust.channel("mktseg"), CMP_EQ, 1)]), cust)
            b2 = s.build(pl.hash_build(
                orders.channel("orderkey"),
                preds=[pl.pred(orders.channel("orderdate"), CMP_LT,
                               Q3_DATE)],
                semijoin_table=b1.table(),
                semijoin_col=orders.channel("custkey"),
                payload=[orders.channel("orderdate")],
                capacity_hint=max(orders.n_rows // 8, 16),  # ~48.6%*20% pass
                # direct single-scan insert (fused-agg probe only)
                agg_table=1,
                # slot = orderkey<<16 | orderdate: one CAS carries key AND
                # payload (date < 2^16)
                pack_bits=16,
                # dynamic-filter bitmap: ~91% of probes miss; one (mostly
                # L3-resident at SF100: 75 MB) bit load rejects them before
                # the hash+tag chain
                bitmap_max_key=okey_max(orders.n_rows)), orders)
            self.tbl = b2.table()

    def run(self, lineitem: Page):
        dec = self.mode == "dec"
        with Scope() as s:
            # dec mode consumes only the exact tick sums: skip the fx128
            # legs (halves the per-hit atomic traffic); f64 mode keeps them
            j = s.run(OP_LOOKUP_JOIN, pl.agg_join(
                self.tbl, lineitem.channel("orderkey"),
                pl.disc_price(lineitem.channel("extendedprice"),
                              lineitem.channel("discount")), 4,
                preds=[pl.pred(lineitem.channel("shipdate"), CMP_GT,
                               Q3_DATE)],
                dec_only=1 if dec else 0), lineitem)
            # groups page cols: [orderkey, orderdate, sum_dec, sum_f64, cnt]
            t = s.run(OP_TOPN, pl.top_n(self.limit, 2 if dec else 3, 1, 0),
                      j.get_output_raw())
            return t.get_output(["orderkey",
                                 "revenue_1e4" if dec else "revenue",
                                 "orderdate"])

    def close(self):
        self.scope.close()


def q3(cust: Page, orders: Page, lineitem: Page, mode="dec", limit=10):
    p = Q3Pipeline(cust, orders, mode=mode, limit=limit)
    try:
        return p.run(lineitem)
    finally:
        p.close()


class Q5Pipeline:
    """Q5 operator graph (q05.sql): region 'ASIA', orderdate in
    [1994-01-01, 1995-01-01), local-supplier join c_nationkey=s_nationkey,
    revenue grouped per nation.

    customer -> custkey->nationkey table
    orders(date) probe it (emit orderkey + cust nation) -> orderkey table
    supplier -> suppkey->nationkey table
    lineitem probe orders-table (emit suppkey, price, disc + cust nation)
             probe supplier-table (emit ... + supplier nation)
    small-key agg: key = supplier nation restricted to ASIA nations
    (drop_unlisted = the region membership), pred cnat == snat (col-col).
    """
    Q5_LO, Q5_HI = 8766, 9131
    ASIA = (8, 9, 12, 18, 21)

    def __init__(self, cust: Page, orders: Page, supp: Page):
        self.scope = Scope()
        with self.scope.on_error() as s:
            self.b1 = s.build(pl.hash_build(
                cust.channel("custkey"),
                payload=[cust.channel("nationkey")],
                capacity_hint=cust.n_rows), cust)
            odate = orders.channel("orderdate")
            j, opage = s.pipe(OP_LOOKUP_JOIN, pl.emit_join(
                self.b1.table(), orders.channel("custkey"),
                [orders.channel("orderkey")],
                preds=[pl.pred(odate, CMP_GE, self.Q5_LO),
                       pl.pred(odate, CMP_LT, self.Q5_HI)]), orders)
            # opage: [orderkey, cust_nationkey]
            self.b2 = s.build(pl.hash_build(
                0, payload=[1], capacity_hint=max(opage.n_rows, 16)), opage)
            s.release(j)
            self.b3 = s.build(pl.hash_build(
                supp.channel("suppkey"),
                payload=[supp.channel("nationkey")],
                capacity_hint=supp.n_rows), supp)

    def run(self, li: Page):
        with Scope() as s:
            ja, pa = s.pipe(OP_LOOKUP_JOIN, pl.emit_join(
                self.b2.table(), li.channel("orderkey"),
                [li.channel("suppkey"), li.channel("extendedprice"),
                 li.channel("discount")]), li)
            # pa: [suppkey, ep, dc, cnat]
            jb, pb = s.pipe(OP_LOOKUP_JOIN, pl.emit_join(
                self.b3.table(), 0, [1, 2, 3]), pa)
            # pb: [ep, dc, cnat, snat]
            s.release(ja)
            return _agg_once(s, pl.small_agg(
                [pl.sum_dec(pl.disc_price(0, 1), 4), pl.count()],
                # compare channel 2 (cnat) == channel 3 (snat)
                preds=[pl.pred_cols(2, CMP_EQ, 3)],
                keys=[(3, self.ASIA)], drop_unlisted_keys=1),
                pb, ["nationkey", "rev_hi", "rev_lo", "count"])

    def close(self):
        self.scope.close()


def q5_composed(cust: Page, orders: Page, supp: Page, li: Page):
    p = Q5Pipeline(cust, orders, supp)
    try:
        return p.run(li)
    finally:
        p.close()


class Q5PipelineFused:
    """Q5 with the single-pass fused probe (LOOKUP_JOIN mode 2): lineitem
    is scanned ONCE — probe the orderkey->cust-nation agg table, dense
    suppkey->supplier-nation lookup, local-supplier equality, per-nation
    register accumulation.  The codegen-analog specialization of the
    composed graph above (same results, no materialized intermediates)."""

    def __init__(self, cust: Page, orders: Page, supp: Page):
        self.scope = Scope()
        with self.scope.on_error() as s:
            # customer dimension as a dense array (payload = nationkey;
            # custkeys dense 1..n)
            b1 = s.build(pl.hash_build(
                cust.channel("custkey"),
                payload=[cust.channel("nationkey")],
                capacity_hint=cust.n_rows, dense_array=1), cust)
            # orders build fused with the customer dimension join: one scan
            # of orders, payload = cust_table[o_custkey].nationkey
            odate = orders.channel("orderdate")
            self.b2 = s.build(pl.hash_build(
                orders.channel("orderkey"),
                preds=[pl.pred(odate, CMP_GE, Q5Pipeline.Q5_LO),
                       pl.pred(odate, CMP_LT, Q5Pipeline.Q5_HI)],
                payload=[0],  # sourced through the lookup instead
                payload_lookup_table=b1.table(),
                payload_lookup_key_col=orders.channel("custkey"),
                # the date window passes ~15.2% of orders; //4 keeps fill
                # ~0.18.  Measured: smaller tables (fill 0.36 / 0.71) cost
                # 1-17 ms of the 600M-row probe — linear-probe cluster
                # length beats any L3 residency gain, so size for SHORT
                # clusters.
                capacity_hint=max(orders.n_rows // 4, 64),
                agg_table=1,
                pack_bits=8,  # slot = orderkey<<8 | cust_nation (u8)
                bitmap_max_key=okey_max(orders.n_rows)), orders)
            self.b3 = s.build(pl.hash_build(
                supp.channel("suppkey"),
                payload=[supp.channel("nationkey")],
                capacity_hint=supp.n_rows, dense_array=1,
                # a dense build reads 0 like -1: no semijoin
                semijoin_table=0), supp)

    def run(self, li: Page):
        with Scope() as s:
            j = s.run(OP_LOOKUP_JOIN, pl.lookup_join(
                self.b2.table(), li.channel("orderkey"), 2,
                proj=pl.disc_price(li.channel("extendedprice"),
                                   li.channel("discount")),
                dec_scale=4, table2=self.b3.table(),
                table2_key_col=li.channel("suppkey"),
                group_vals=Q5Pipeline.ASIA), li)
            return j.get_output(["nationkey", "rev_lo", "rev_f64", "count"])

    def close(self):
        self.scope.close()


def q5(cust: Page, orders: Page, supp: Page, li: Page):
    p = Q5PipelineFused(cust, orders, supp)
    try:
        return p.run(li)
    finally:
        p.close()


def q6(li: Page):
    """Q6 scalar aggregate (q06.sql): keyless HASH_AGG_SMALL with the
    BETWEEN predicates fused; exact decimal ticks (scale 4) + count."""
    sd, dc = li.channel("shipdate"), li.channel("discount")
    plan = pl.small_agg(
        [pl.sum_dec(pl.mul(li.channel("extendedprice"), dc), 4), pl.count()],
        preds=[pl.pred(sd, CMP_GE, 8766), pl.pred(sd, CMP_LT, 9131),
               pl.pred(dc, CMP_GE, 0.05), pl.pred(dc, CMP_LE, 0.07),
               pl.pred(li.channel("quantity"), CMP_LT, 24.0)])
    with Scope() as s:
        return _agg_once(s, plan, li, ["rev_hi", "rev_lo", "count"])


def q7(cust: Page, orders: Page, supp: Page, li: Page):
    """Q7 volume shipping (q07.sql): FRANCE(6)<->GERMANY(7) pairs, shipdate
    in [1995-01-01, 1996-12-31], volume grouped by (supp_nation,
    cust_nation, year).  Composed: dense customer dimension, orders
    agg-table with fused dimension lookup (no date filter), supplier hash
    table, two emit joins, then four keyless aggregations (the OR over
    nation pairs and the year split decompose into conjunctive plans).
    Returns list of (supp_nation, cust_nation, year, revenue_1e4)."""
    with Scope() as s:
        o1 = s.build(pl.hash_build(
            cust.channel("custkey"), payload=[cust.channel("nationkey")],
            capacity_hint=cust.n_rows, dense_array=1), cust)
        # orderkey -> customer nation as a dense u8 array over the orderkey
        # range (one scan + one byte per possible key; nation is fetched
        # through the dense customer dimension during the fill).  Presence
        # = nonzero, so the stored value is nation+1 — downstream
        # predicates are biased accordingly.
        o2 = s.build(pl.hash_build(
            orders.channel("orderkey"), payload=[0],
            payload_lookup_table=o1.table(),
            payload_lookup_key_col=orders.channel("custkey"),
            capacity_hint=okey_max(orders.n_rows), dense_array=1,
            dense_payload_bias=1), orders)
        o3 = s.build(pl.hash_build(
            supp.channel("suppkey"), payload=[supp.channel("nationkey")],
            capacity_hint=supp.n_rows), supp)

        sd = li.channel("shipdate")
        ja, pa = s.pipe(OP_LOOKUP_JOIN, pl.emit_join(
            o2.table(), li.channel("orderkey"),
            [li.channel("suppkey"), li.channel("extendedprice"),
             li.channel("discount"), sd],  # shipdate is needed downstream
            preds=[pl.pred(sd, CMP_GE, 9131), pl.pred(sd, CMP_LE, 9861)]),
            li)
        # pa: [suppkey, ep, dc, sdate, cnat]
        jb, pb = s.pipe(OP_LOOKUP_JOIN,
                        pl.emit_join(o3.table(), 0, [1, 2, 3, 4]), pa)
        # pb: [ep, dc, sdate, cnat, snat]
        s.release(ja)

        out = []
        for sn, cn in ((6, 7), (7, 6)):
            for ylo, yhi, yr in ((9131, 9495, 1995), (9496, 9861, 1996)):
                res = _agg_once(s, pl.small_agg(
                    [pl.sum_dec(pl.disc_price(0, 1), 4), pl.count()],
                    preds=[pl.pred(4, CMP_EQ, sn),
                           pl.pred(3, CMP_EQ, cn + 1),  # dense bias
                           pl.pred(2, CMP_GE, ylo),
                           pl.pred(2, CMP_LE, yhi)]),
                    pb, ["hi", "lo", "cnt"])
                if len(res["lo"]) and res["cnt"][0] > 0:
                    out.append((sn, cn, yr, int(res["lo"][0])))
        s.release(jb, o1, o2, o3)
        return out


AMERICA_NATIONS = (1, 2, 3, 17, 24)  # tpch_nation_region(k) == 1 (AMERICA)
BRAZIL = 2


def _key_set(s, keys):
    """A tiny (non-dense) key set from a handful of host keys."""
    page = Page({"key": np.asarray(keys, dtype=np.int64)})
    return s.build(pl.hash_build(0, capacity_hint=32, key_set_only=1), page)


def q8(cust: Page, orders: Page, supp: Page, part: Page, li: Page):
    """Q8 national market share (q08.sql): revenue of 'ECONOMY ANODIZED
    STEEL' (type id 103) parts sold to AMERICA-region customers with
    orderdate in 1995..1996, split into BRAZIL(2)-supplier vs total per
    order year.  Composed from the §8 operators only:

      nation keys -> key set; customer semijoin filter -> custkey flag set
      orders chained build (date range + customer semijoin, payload
        orderdate)                      [HashBuilderOperator analog]
      part(type==103) -> partkey flag set; supplier(BRAZIL) -> flag set
      lineitem semijoin(part) filter -> emit join (payload orderdate)
        -> brazil semijoin filter + 4 keyless year aggregations
    Returns (brazil_1e4[2], total_1e4[2]) exact ticks for (1995, 1996);
    share = brazil/total (golden q08_sf1.result: 0.0344 / 0.0415)."""
    with Scope() as s:
        # American nation keys as a tiny key set
        on = _key_set(s, AMERICA_NATIONS)

        # AMERICA customers -> dense custkey flag set (custkeys dense 1..n)
        f1, cpage = s.pipe(OP_FILTER_PROJECT, pl.filter_project(
            [pl.ident(cust.channel("custkey"))], semijoin_table=on.table(),
            semijoin_col=cust.channel("nationkey")), cust)
        oc = s.build(pl.flag_set(0, cust.n_rows), cpage)

        # qualifying orders: chained table keyed by orderkey, payload
        # orderdate
        odate = orders.channel("orderdate")
        oo = s.build(pl.hash_build(
            orders.channel("orderkey"),
            preds=[pl.pred(odate, CMP_GE, 9131),
                   pl.pred(odate, CMP_LE, 9861)],
            semijoin_table=oc.table(),
            semijoin_col=orders.channel("custkey"), payload=[odate],
            capacity_hint=max(orders.n_rows // 8, 16),
            bitmap_max_key=okey_max(orders.n_rows)), orders)

        # part type 103 -> dense partkey flag set
        opart = s.build(pl.flag_set(
            part.channel("partkey"), part.n_rows,
            preds=[pl.pred(part.channel("type_id"), CMP_EQ, 103)]), part)

        # BRAZIL suppliers -> dense suppkey flag set
        ob = s.build(pl.flag_set(
            supp.channel("suppkey"), supp.n_rows,
            preds=[pl.pred(supp.channel("nationkey"), CMP_EQ, BRAZIL)]),
            supp)

        # lineitem: keep type-103 parts, project the join/agg columns
        f2, lpage = s.pipe(OP_FILTER_PROJECT, pl.filter_project(
            [pl.ident(li.channel(n)) for n in
             ("orderkey", "suppkey", "extendedprice", "discount")],
            semijoin_table=opart.table(),
            semijoin_col=li.channel("partkey")), li)
        # lpage: [orderkey, suppkey, ep, dc]

        # emit join against qualifying orders; payload appends orderdate
        jo, jpage = s.pipe(OP_LOOKUP_JOIN,
                           pl.emit_join(oo.table(), 0, [1, 2, 3]), lpage)
        # jpage: [suppkey, ep, dc, orderdate]

        # brazil-supplier subset
        f3, bpage = s.pipe(OP_FILTER_PROJECT, pl.filter_project(
            [pl.ident(1), pl.ident(2), pl.ident(3)],
            semijoin_table=ob.table(), semijoin_col=0), jpage)
        # bpage: [ep, dc, orderdate]

        def rev(page, odcol, epcol, dccol, lo, hi):
            r = _agg_once(s, pl.small_agg(
                [pl.sum_dec(pl.disc_price(epcol, dccol), 4)],
                preds=[pl.pred(odcol, CMP_GE, lo),
                       pl.pred(odcol, CMP_LE, hi)]), page, ["hi", "lo"])
            return _ticks(r) if len(r["lo"]) else 0

        YEARS = ((9131, 9495), (9496, 9861))  # 1995, 1996 epoch-day ranges
        total = [rev(jpage, 3, 1, 2, lo, hi) for lo, hi in YEARS]
        brazil = [rev(bpage, 2, 0, 1, lo, hi) for lo, hi in YEARS]
        s.release(f3, jo, f2, f1, on, oc, oo, opart, ob)
        return brazil, total


def q14(part: Page, li: Page):
    """Q14 promo revenue (q14.sql): shipdate in [1995-09-01, 1995-10-01) =
    [9374, 9404); promo parts = type ids 125..149 ('PROMO*') as a dense
    partkey flag set.  Returns (promo_1e4, total_1e4) exact ticks; the
    result is 100.00*promo/total at scale 6 HALF_UP."""
    epc, dcc = li.channel("extendedprice"), li.channel("discount")
    sdc, pkc = li.channel("shipdate"), li.channel("partkey")
    window = [pl.pred(sdc, CMP_GE, 9374), pl.pred(sdc, CMP_LT, 9404)]
    with Scope() as s:
        ob = s.build(pl.flag_set(
            part.channel("partkey"), part.n_rows,
            preds=[pl.pred(part.channel("type_id"), CMP_GE, 125)]), part)

        def rev(page, ep, dc, preds=()):
            r = _agg_once(s, pl.small_agg(
                [pl.sum_dec(pl.disc_price(ep, dc), 4)], preds=preds),
                page, ["hi", "lo"])
            return _ticks(r) if len(r["lo"]) else 0

        total = rev(li, epc, dcc, window)
        f, fpage = s.pipe(OP_FILTER_PROJECT, pl.filter_project(
            [pl.ident(epc), pl.ident(dcc)], preds=window,
            semijoin_table=ob.table(), semijoin_col=pkc), li)
        promo = rev(fpage, 0, 1)
        return promo, total


def q12(orders: Page, li: Page):
    """Q12 shipmode priority (q12.sql): late-commit lineitems received in
    1994 joined to orders; counts per (shipmode in {MAIL=4, SHIP=6},
    priority class).  Returns {mode_id: (high, low)}."""
    with Scope() as s:
        # orderkey -> priority as a dense u8 array over the orderkey range
        # (presence = nonzero, so priority+1 is stored; the class-split
        # predicates below are biased accordingly)
        oo = s.build(pl.hash_build(
            orders.channel("orderkey"), payload=[orders.channel("priority")],
            capacity_hint=okey_max(orders.n_rows), dense_array=1,
            dense_payload_bias=1), orders)

        cdc, rdc = li.channel("commitdate"), li.channel("receiptdate")
        sdc = li.channel("shipdate")
        f, fpage = s.pipe(OP_FILTER_PROJECT, pl.filter_project(
            [pl.ident(li.channel("orderkey")),
             pl.ident(li.channel("shipmode"))],
            preds=[pl.pred_cols(cdc, CMP_LT, rdc),
                   pl.pred_cols(sdc, CMP_LT, cdc),
                   pl.pred(rdc, CMP_GE, 8766), pl.pred(rdc, CMP_LT, 9131)]),
            li)
        # fpage: [orderkey, shipmode]
        jo, jpage = s.pipe(OP_LOOKUP_JOIN,
                           pl.emit_join(oo.table(), 0, [1]), fpage)
        # jpage: [shipmode, priority]

        res = {4: [0, 0], 6: [0, 0]}
        for cls, (op_, val) in enumerate(((CMP_LE, 2), (CMP_GE, 3))):
            # priority stored +1 (dense bias): URGENT/HIGH {0,1} -> {1,2}
            out = _agg_once(s, pl.small_agg(
                [pl.count()],
                preds=[pl.pred(1, op_, val)],  # priority class split
                keys=[(0, (4, 6))],            # MAIL, SHIP
                drop_unlisted_keys=1), jpage, ["shipmode", "count"])
            for i in range(len(out["shipmode"])):
                res[int(out["shipmode"][i])][cls] += int(out["count"][i])
        return {m: tuple(v) for m, v in res.items()}


def q17(part: Page, li: Page):
    """Q17 small-quantity-order revenue (q17.sql): Brand#23 'MED BOX'
    (container id 17) parts; rows with quantity < 0.2*avg(part quantity).
    The correlated avg is a fused-agg probe (sum_qty + count per target
    part); the tiny per-part cutoffs (0.2*avg <= 10) come back to the
    host (coordinator-side scalar-subquery plan constants, ~200 rows) and
    drive per-cutoff-class flag-set semijoins.  Returns the exact cents
    sum of extendedprice (result = cents/7.0 at scale 2 HALF_UP)."""
    pkc = part.channel("partkey")
    target = [pl.pred(part.channel("brand"), CMP_EQ, 23),
              pl.pred(part.channel("container"), CMP_EQ, 17)]
    with Scope() as s:
        ot = s.build(pl.hash_build(
            pkc, preds=target, capacity_hint=max(part.n_rows // 16, 4096),
            agg_table=1,
            bitmap_max_key=part.n_rows),  # ~0.1% of 600M probes hit
            part)
        os_ = s.build(pl.flag_set(pkc, part.n_rows, preds=target), part)

        # per-target-part sum(quantity) + count over ALL lineitems
        jo = s.run(OP_LOOKUP_JOIN, pl.agg_join(
            ot.table(), li.channel("partkey"),
            pl.ident(li.channel("quantity")), dec_only=1), li)
        g = jo.get_output(["partkey", "sum_qty", "sum_f64", "cnt"])
        s.release(jo)

        # cutoff class per part: qty < sum/(5*cnt)  =>  qty <= c_p
        classes = {}
        for i in range(len(g["partkey"])):
            sq, c = int(g["sum_qty"][i]), int(g["cnt"][i])
            cp = (sq + 5 * c - 1) // (5 * c) - 1  # max qty with 5*qty*c < s
            if cp >= 1:
                classes.setdefault(cp, []).append(int(g["partkey"][i]))

        # li restricted to target parts (small page)
        f, fpage = s.pipe(OP_FILTER_PROJECT, pl.filter_project(
            [pl.ident(li.channel(n)) for n in
             ("partkey", "quantity", "extendedprice")],
            semijoin_table=os_.table(),
            semijoin_col=li.channel("partkey")), li)
        # fpage: [partkey, qty, ep]

        total = 0
        for cp, pks in sorted(classes.items()):
            cpage = Page({"partkey": np.asarray(pks, dtype=np.int64)})
            oc = s.build(pl.flag_set(0, part.n_rows), cpage)
            ff, cpage2 = s.pipe(OP_FILTER_PROJECT, pl.filter_project(
                [pl.ident(2)], preds=[pl.pred(1, CMP_LE, float(cp))],
                semijoin_table=oc.table(), semijoin_col=0), fpage)
            r = _agg_once(s, pl.small_agg([pl.sum_dec(pl.ident(0), 2)]),
                          cpage2, ["hi", "lo"])
            if len(r["lo"]):
                total += _ticks(r)
            s.release(ff, oc)
        s.release(f, ot, os_)
        return total


def q11(supp: Page, ps: Page, n_part: int):
    """Q11 important stock (q11.sql): GERMANY(7) partsupp grouped by
    partkey, value = sum(supplycost*availqty); HAVING value >
    0.0001*total; ORDER BY value DESC (partkey ASC tiebreak).  The MUL
    decimal projection yields 1e-4 ticks (cents x hundredth-encoded
    qty); the strict HAVING threshold total/10000 becomes a plan
    constant.  The final ORDER BY is an ORDER_BY operator over the HAVING
    filter's device page.  Returns (partkeys, value_cents) host arrays."""
    with Scope() as s:
        og = s.build(pl.flag_set(
            supp.channel("suppkey"), supp.n_rows,
            preds=[pl.pred(supp.channel("nationkey"), CMP_EQ, 7)]), supp)
        f, gpage = s.pipe(OP_FILTER_PROJECT, pl.filter_project(
            [pl.ident(ps.channel(n)) for n in
             ("partkey", "supplycost", "availqty")],
            semijoin_table=og.table(),
            semijoin_col=ps.channel("suppkey")), ps)
        # gpage: [partkey, cost, qty]
        total_1e4 = _ticks(_agg_once(
            s, pl.small_agg([pl.sum_dec(pl.mul(1, 2), 4)]), gpage,
            ["hi", "lo"]))

        keys = Page({"partkey": np.arange(1, n_part + 1, dtype=np.int64)})
        ok = s.build(pl.hash_build(0, capacity_hint=n_part, agg_table=1),
                     keys)
        jo = s.run(OP_LOOKUP_JOIN, pl.agg_join(
            ok.table(), 0, pl.mul(1, 2), 4, dec_only=1), gpage)
        groups = jo.get_output_raw()  # [partkey, sum_1e4, f64, cnt]
        fo = s.op(OP_FILTER_PROJECT, pl.filter_project(
            [pl.ident(0), pl.ident(1)],
            preds=[pl.pred(1, CMP_GT, total_1e4 // 10000)]))
        fo.add_input_raw(groups)
        ob = s.run(OP_ORDER_BY, pl.order_by([pl.desc(1), pl.asc(0)], [0, 1]),
                   fo.get_output_raw())
        out = ob.get_output(["partkey", "value_1e4"])
        s.release(ob, fo, jo, f, og, ok)
    # ticks are cents*100, so the order of the ticks is the order of the
    # cents and the division is exact
    assert not (out["value_1e4"] % 100).any()
    return out["partkey"], out["value_1e4"] // 100


def q18(orders: Page, li: Page, limit=100):
    """Q18 large-volume customers (q18.sql): per-order quantity sums via
    a fused-agg probe over the full orders key table; HAVING sum > 300
    as a plan-constant filter; the ~1e-5-selectivity survivors join back
    to the orders columns (emit join) and the bounded final ORDER BY
    runs host-side.  Returns [(custkey, orderkey, orderdate,
    totalprice_cents, sum_qty)] sorted (totalprice desc, orderdate asc,
    orderkey asc) LIMIT limit."""
    with Scope() as s:
        # per-order qty sums take NOTHING from orders: range-group domain
        # over the orderkey range replaces the 150M-row build, and the
        # orderkey-clustered lineitem makes the accumulator atomics
        # near-sequential (see q21)
        oo = s.build(pl.range_group(okey_max(orders.n_rows)))
        jo = s.run(OP_LOOKUP_JOIN, pl.agg_join(
            oo.table(), li.channel("orderkey"),
            pl.ident(li.channel("quantity")), dec_only=1), li)
        # groups: [orderkey, sum_qty, f64, cnt]
        fo, big = s.pipe(OP_FILTER_PROJECT, pl.filter_project(
            [pl.ident(0), pl.ident(1)], preds=[pl.pred(1, CMP_GT, 300)]),
            jo.get_output_raw())
        # big: [orderkey, sum_qty]
        ob = s.build(pl.hash_build(
            0, payload=[1], capacity_hint=max(big.n_rows, 16),
            # ~6K hits of 150M probes
            bitmap_max_key=okey_max(orders.n_rows)), big)
        js = s.op(OP_LOOKUP_JOIN, pl.emit_join(
            ob.table(), orders.channel("orderkey"),
            [orders.channel(n) for n in
             ("orderkey", "custkey", "orderdate", "totalprice")]))
        js.add_input(orders)
        out = js.get_output(["orderkey", "custkey", "orderdate",
                             "totalprice", "sum_qty"])
        s.release(js, fo, jo, oo, ob)
    rows = [(int(out["custkey"][i]), int(out["orderkey"][i]),
             int(out["orderdate"][i]), int(out["totalprice"][i]),
             int(out["sum_qty"][i])) for i in range(len(out["orderkey"]))]
    rows.sort(key=lambda r: (-r[3], r[2], r[1]))
    return rows[:limit]


def q19(part: Page, li: Page):
    """Q19 discounted revenue (q19.sql): part attributes join (chained
    table, 3 u8 payloads) fused with the shipmode/shipinstruct/quantity
    pre-filter, then the three brand/container/size/qty disjuncts as
    twelve conjunctive keyless aggregations over the joined page (the
    OR decomposes per container id).  Exact 1e-4 ticks."""
    with Scope() as s:
        ob = s.build(pl.hash_build(
            part.channel("partkey"),
            payload=[part.channel(n) for n in ("brand", "container", "size")],
            capacity_hint=part.n_rows), part)
        jo, jpage = s.pipe(OP_LOOKUP_JOIN, pl.emit_join(
            ob.table(), li.channel("partkey"),
            [li.channel("quantity"), li.channel("extendedprice"),
             li.channel("discount")],
            preds=[pl.pred(li.channel("shipmode"), CMP_EQ, 1),   # AIR
                   pl.pred(li.channel("shipinstruct"), CMP_EQ, 0),
                   pl.pred(li.channel("quantity"), CMP_LE, 30.0)]), li)
        # jpage: [qty, ep, dc, brand, container, size]

        DISJ = ((12, (0, 1, 5, 4), 1, 11, 5),
                (23, (18, 17, 21, 20), 10, 20, 10),
                (34, (8, 9, 13, 12), 20, 30, 15))
        total = 0
        for bnum, cset, qlo, qhi, szhi in DISJ:
            for c in cset:
                r = _agg_once(s, pl.small_agg(
                    [pl.sum_dec(pl.disc_price(1, 2), 4)],
                    preds=[pl.pred(3, CMP_EQ, bnum), pl.pred(4, CMP_EQ, c),
                           pl.pred(5, CMP_GE, 1), pl.pred(5, CMP_LE, szhi),
                           pl.pred(0, CMP_GE, float(qlo)),
                           pl.pred(0, CMP_LE, float(qhi))]),
                    jpage, ["hi", "lo"])
                if len(r["lo"]):
                    total += _ticks(r)
        return total


def q21(supp: Page, orders: Page, li: Page, limit=100):
    """Q21 suppliers who kept orders waiting (q21.sql).  The correlated
    EXISTS / NOT-EXISTS pair decomposes into per-order aggregates; all of
    them come out of ONE multi-accumulator fused-agg probe over lineitem
    (LOOKUP_JOIN mode 1, n_aggs=5 with per-aggregate FILTER predicates —
    the InMemoryHashAggregationBuilder + AggregationNode-mask analog):
      a0 = sum(suppkey)            over all lines of the order
      a1 = count                   where linestatus = 'F'
      a2 = sum(suppkey)            where receiptdate > commitdate (late)
      a3 = count                   where late
      a4 = sum(suppkey*suppkey)    where late  (raw integer product)
      cnt = count of all lines
    An order qualifies when every line is 'F' (a1 == cnt), it has a late
    line (a3 > 0), all late lines share one supplier (zero variance:
    a3*a4 == a2*a2, exact in f64 — both sides < 2^53), and some line has
    a different supplier (a2*cnt != a0*a3); s* = a2/a3 is that supplier.
    numwait(s) = sum of a3 over qualifying orders with s* = s (counting
    the l1 late lines, per q21.sql's count(*)), SAUDI ARABIA semijoin.
    Returns [(suppkey, numwait)] sorted (numwait desc, suppkey asc)
    LIMIT limit."""
    with Scope() as s:
        # The probe takes NOTHING from orders (no payload — the table is
        # only the group-by domain, and every lineitem orderkey exists in
        # orders by FK): a RANGE-GROUP table over the orderkey domain
        # replaces the whole 150M-row build, and the orderkey-clustered
        # lineitem makes the accumulator atomics near-sequential instead
        # of hash-scattered.
        otbl = s.build(pl.range_group(okey_max(orders.n_rows)))

        # accumulator packing: the probe is atomic-op-rate bound, and every
        # per-order total is bounded by integrity facts — at most 7
        # lineitems per order (TPC-H PK) and suppkey < supplier count — so
        # a0/a2 (sums of suppkeys) and the three counts share ONE u64 word;
        # only a4 (sum of squared suppkeys) needs its own.  One flush = 1-2
        # atomics on 1-2 adjacent words instead of up to 6.
        wsum = (7 * supp.n_rows).bit_length()
        pack = {}
        if 2 * wsum + 12 <= 64:
            pack = dict(
                acc_pack=1,
                acc_pack_shift=[0,               # a0: sum(suppkey) all
                                2 * wsum,        # a1: cnt F
                                wsum,            # a2: sum(suppkey) late
                                2 * wsum + 4,    # a3: cnt late
                                -1],      # a4: sum(sk^2) -> own word
                acc_pack_width=[wsum, 4, wsum, 4],
                acc_pack_cnt_shift=2 * wsum + 8, acc_pack_cnt_width=4)
        sk = li.channel("suppkey")
        F, LATE = 0, 1  # indices into filters=
        jo = s.run(OP_LOOKUP_JOIN, pl.lookup_join(
            otbl.table(), li.channel("orderkey"), 1,
            # no row-level predicate: both are per-aggregate FILTERs
            filters=[pl.pred(li.channel("linestatus"), CMP_EQ, ord("F")),
                     pl.pred_cols(li.channel("receiptdate"), CMP_GT,
                                  li.channel("commitdate"))],
            aggs=[pl.sum_i64(pl.ident(sk)), (pl.count(), F),
                  (pl.sum_i64(pl.ident(sk)), LATE), (pl.count(), LATE),
                  (pl.sum_i64(pl.mul(sk, sk)), LATE)],
            **pack), li)
        # pg: [ok(0), sum_all(1), cnt_F(2), sum_l(3), cnt_l(4), sq_l(5),
        #      cnt_all(6)]
        f1, pe = s.pipe(OP_FILTER_PROJECT, pl.filter_project(
            [pl.div(3, 4),    # s* = sum_l / cnt_l
             pl.ident(4),     # cnt_l
             pl.mul(4, 5),    # m1 = cnt_l * sq_l  (<2^53)
             pl.mul(3, 3),    # m2 = sum_l^2       (<2^53)
             pl.mul(3, 6),    # m3 = sum_l * cnt_all
             pl.mul(1, 4)],   # m4 = sum_all * cnt_l
            preds=[pl.pred_cols(2, CMP_EQ, 6),  # every line 'F':
                                                # cnt_F == cnt_all
                   pl.pred(4, CMP_GT, 0)]),     # EXISTS late line
            jo.get_output_raw())
        # pe: [s*, cnt_l, m1, m2, m3, m4]

        saudi = [pl.pred(supp.channel("nationkey"), CMP_EQ, 20)]
        osa = s.build(pl.flag_set(supp.channel("suppkey"), supp.n_rows,
                                  preds=saudi), supp)
        f2, pf2 = s.pipe(OP_FILTER_PROJECT, pl.filter_project(
            [pl.ident(0), pl.ident(1)],
            preds=[pl.pred_cols(2, CMP_EQ, 3),   # zero variance: m1 == m2
                   pl.pred_cols(4, CMP_NE, 5)],  # some different supplier:
                                                 # m3 != m4
            semijoin_table=osa.table(), semijoin_col=0), pe)
        # pf2: [s*, cnt_l] qualifying orders

        ow = s.build(pl.hash_build(
            supp.channel("suppkey"), preds=saudi,
            capacity_hint=supp.n_rows + 64, agg_table=1), supp)
        jn = s.run(OP_LOOKUP_JOIN,
                   pl.agg_join(ow.table(), 0, pl.ident(1), dec_only=1), pf2)
        out = jn.get_output(["suppkey", "numwait", "f64", "cnt"])
        s.release(jn, f2, f1, jo, otbl, osa, ow)
    rows = sorted(
        ((int(out["suppkey"][i]), int(out["numwait"][i]))
         for i in range(len(out["suppkey"]))),
        key=lambda r: (-r[1], r[0]))
    return rows[:limit]


Q9_YEAR_BOUNDS = (8035, 8401, 8766, 9131, 9496, 9862, 10227, 10592)


def q9(part: Page, supp: Page, orders: Page, ps: Page, li: Page):
    """Q9 product-type profit (q09.sql): LIKE '%green%' as a VARBIN
    CONTAINS predicate building a dense part flag set; the partsupp
    composite-key (partkey, suppkey) lookup is an emit join on partkey
    followed by the suppkey equality (4 candidate suppliers per part);
    supplier-nation and order-year attach by payload emit joins; the
    (nation, year) grouping runs as per-group conjunctive aggregations
    of the two exact sums (revenue - supplycost*qty).  Returns a 25x7
    list of exact 1e-4 tick profits ([nation][year-1992])."""
    with Scope() as s:
        og = s.build(pl.flag_set(
            part.channel("partkey"), part.n_rows,
            preds=[pl.pred_varbin(part.channel("name"), CMP_CONTAINS,
                                  b"green")]), part)
        f, gli = s.pipe(OP_FILTER_PROJECT, pl.filter_project(
            [pl.ident(li.channel(n)) for n in
             ("partkey", "suppkey", "orderkey", "quantity", "extendedprice",
              "discount")],
            semijoin_table=og.table(),
            semijoin_col=li.channel("partkey")), li)
        # gli: [pk, sk, ok, qty, ep, dc]

        ops_ = s.build(pl.hash_build(
            ps.channel("partkey"),
            payload=[ps.channel("suppkey"), ps.channel("supplycost")],
            capacity_hint=ps.n_rows), ps)
        ja, pa = s.pipe(OP_LOOKUP_JOIN,
                        pl.emit_join(ops_.table(), 0, range(6)), gli)
        # pa: [pk, sk, ok, qty, ep, dc, ps_sk, cost]
        f2, pb = s.pipe(OP_FILTER_PROJECT, pl.filter_project(
            [pl.ident(c) for c in (1, 2, 3, 4, 5, 7)],
            preds=[pl.pred_cols(1, CMP_EQ, 6)]), pa)
        # pb: [sk, ok, qty, ep, dc, cost]

        os_ = s.build(pl.hash_build(
            supp.channel("suppkey"), payload=[supp.channel("nationkey")],
            capacity_hint=supp.n_rows), supp)
        jb, pc = s.pipe(OP_LOOKUP_JOIN,
                        pl.emit_join(os_.table(), 0, [1, 2, 3, 4, 5]), pb)
        # pc: [ok, qty, ep, dc, cost, nat]

        # orderkey -> orderdate as a dense i32 array over the orderkey
        # range (2.4 GB at SF100): one scan + direct stores replace the
        # 150M-row chained insert, and each probe is one i32 load (presence
        # = nonzero payload; epoch-day dates are always nonzero)
        oo = s.build(pl.hash_build(
            orders.channel("orderkey"),
            payload=[orders.channel("orderdate")],
            capacity_hint=okey_max(orders.n_rows), dense_array=1), orders)
        jc, pd = s.pipe(OP_LOOKUP_JOIN,
                        pl.emit_join(oo.table(), 0, [1, 2, 3, 4, 5]), pc)
        # pd: [qty, ep, dc, cost, nat, odate]

        # ONE general multi-channel group-by over (nation, orderdate) — the
        # MultiChannelGroupByHash analog replaces the former 25 nation-split
        # scans x 7 year aggregations (175 launches); the date groups fold
        # into years on the host (exact integer ticks end to end)
        gop = s.run(OP_GROUPBY_MULTI, pl.group_by(
            [4, 5],  # nat, odate
            [pl.sum_dec(pl.disc_price(1, 2), 4),
             pl.sum_dec(pl.mul(3, 0), 4)],
            25 * 2500 + 1024), pd)
        gout = gop.get_output(["nat", "odate", "rev", "cost", "cnt"])
        s.release(gop)
        profit = [[0] * 7 for _ in range(25)]
        years = np.searchsorted(np.asarray(Q9_YEAR_BOUNDS[1:]),
                                np.asarray(gout["odate"]), side="right")
        for i in range(len(gout["nat"])):
            y = int(years[i])
            if y < 7:
                profit[int(gout["nat"][i])][y] += \
                    int(gout["rev"][i]) - int(gout["cost"][i])
        s.release(jc, jb, f2, ja, f, og, ops_, os_, oo)
        return profit


def q9_multikey(part: Page, supp: Page, orders: Page, ps: Page, li: Page):
    """q9 with the partsupp lookup as ONE two-key emit join on (partkey,
    suppkey): a multi-key chained build of partsupp and a probe that emits
    the one matching row, instead of q9's four candidates per lineitem and
    the suppkey equality FILTER_PROJECT behind them.  Everything else, and
    the return value, is q9's."""
    with Scope() as s:
        og = s.build(pl.flag_set(
            part.channel("partkey"), part.n_rows,
            preds=[pl.pred_varbin(part.channel("name"), CMP_CONTAINS,
                                  b"green")]), part)
        f, gli = s.pipe(OP_FILTER_PROJECT, pl.filter_project(
            [pl.ident(li.channel(n)) for n in
             ("partkey", "suppkey", "orderkey", "quantity", "extendedprice",
              "discount")],
            semijoin_table=og.table(),
            semijoin_col=li.channel("partkey")), li)
        # gli: [pk, sk, ok, qty, ep, dc]

        ops_ = s.build(pl.hash_build(
            [ps.channel("partkey"), ps.channel("suppkey")],
            payload=[ps.channel("supplycost")],
            capacity_hint=ps.n_rows), ps)
        ja, pb = s.pipe(OP_LOOKUP_JOIN,
                        pl.emit_join(ops_.table(), [0, 1], [1, 2, 3, 4, 5]),
                        gli)
        # pb: [sk, ok, qty, ep, dc, cost]

        os_ = s.build(pl.hash_build(
            supp.channel("suppkey"), payload=[supp.channel("nationkey")],
            capacity_hint=supp.n_rows), supp)
        jb, pc = s.pipe(OP_LOOKUP_JOIN,
                        pl.emit_join(os_.table(), 0, [1, 2, 3, 4, 5]), pb)
        # pc: [ok, qty, ep, dc, cost, nat]

        oo = s.build(pl.hash_build(
            orders.channel("orderkey"),
            payload=[orders.channel("orderdate")],
            capacity_hint=okey_max(orders.n_rows), dense_array=1), orders)
        jc, pd = s.pipe(OP_LOOKUP_JOIN,
                        pl.emit_join(oo.table(), 0, [1, 2, 3, 4, 5]), pc)
        # pd: [qty, ep, dc, cost, nat, odate]

        gop = s.run(OP_GROUPBY_MULTI, pl.group_by(
            [4, 5],  # nat, odate
            [pl.sum_dec(pl.disc_price(1, 2), 4),
             pl.sum_dec(pl.mul(3, 0), 4)],
            25 * 2500 + 1024), pd)
        gout = gop.get_output(["nat", "odate", "rev", "cost", "cnt"])
        s.release(gop)
        profit = [[0] * 7 for _ in range(25)]
        years = np.searchsorted(np.asarray(Q9_YEAR_BOUNDS[1:]),
                                np.asarray(gout["odate"]), side="right")
        for i in range(len(gout["nat"])):
            y = int(years[i])
            if y < 7:
                profit[int(gout["nat"][i])][y] += \
                    int(gout["rev"][i]) - int(gout["cost"][i])
        s.release(jc, jb, ja, f, og, ops_, os_, oo)
        return profit


def q13(n_cust: int, orders, max_count=64):
    """Q13 customer distribution (q13.sql): the NOT LIKE
    '%special%requests%' comment filter runs as the ordered
    two-substring VARBIN predicate (CONTAINS2 negated); per-customer
    order counts come from a fused-agg probe over the full customer key
    table; the count histogram is a second fused-agg probe keyed by the
    count value.  The LEFT OUTER zero bucket is n_cust minus the
    customers with qualifying orders.  Returns [(c_count, custdist)]
    sorted (custdist desc, c_count desc).

    orders: one Page or an iterable of Pages — the o_comment
    VariableWidthBlock has int32 offsets (the reference's Slice cap), so
    beyond ~SF20 the orders table arrives as MULTIPLE pages, exactly as
    Presto's Driver would feed them; every operator here accumulates
    across addInput calls."""
    order_pages = [orders] if isinstance(orders, Page) else list(orders)

    def count_join(table, key_col, width):
        """Count-only probe whose count + row count share one u64."""
        return pl.lookup_join(
            table, key_col, 1, aggs=[pl.count()], acc_pack=1,
            acc_pack_shift=[0], acc_pack_width=[width],
            acc_pack_cnt_shift=width, acc_pack_cnt_width=width)

    with Scope() as s:
        # the "table" is the keys 1..n_cust themselves: a range-group
        # domain (no build, no hash; acc index = custkey-1)
        oc = s.build(pl.range_group(n_cust))
        # count-only probe with a packed 1-word accumulator: per-customer
        # order counts are bounded far below 2^16, so count+cnt share one
        # u64 (one atomic per row into a ~120 MB L3-resident array)
        jo = s.op(OP_LOOKUP_JOIN, count_join(oc.table(), 0, 16))
        f = s.op(OP_FILTER_PROJECT, pl.filter_project(
            [pl.ident(order_pages[0].channel("custkey"))],
            preds=[pl.pred_varbin(order_pages[0].channel("comment"),
                                  CMP_NOT_CONTAINS2, b"special",
                                  b"requests")]))
        for opg in order_pages:
            f.add_input(opg)
            jo.add_input_raw(f.get_output_raw())  # [custkey] qualifying
        jo.finish()
        groups = jo.get_output_raw()  # [custkey, n_orders, cnt]
        n_with_orders = groups.n_rows

        # counts beyond max_count: range miss
        oh = s.build(pl.range_group(max_count))
        jo2 = s.run(OP_LOOKUP_JOIN,
                    count_join(oh.table(), 1, 32),  # key: the count
                    groups)
        hist = jo2.get_output(["c_count", "n_cust", "custdist"])
        s.release(jo2, jo, f, oc, oh)
    rows = [(int(hist["c_count"][i]), int(hist["custdist"][i]))
            for i in range(len(hist["c_count"]))]
    rows.append((0, n_cust - n_with_orders))
    rows.sort(key=lambda r: (-r[1], -r[0]))
    return rows


def _fill_flag_set(s, part, pred_sets):
    """A disjunction over `part` as ONE dense partkey flag set: one
    conjunctive filter pass per predicate set, whose partkey outputs all
    feed the same build (flags OR across add_input)."""
    fops, pages = [], []
    for preds in pred_sets:
        f, page = s.pipe(OP_FILTER_PROJECT, pl.filter_project(
            [pl.ident(part.channel("partkey"))], preds=preds), part)
        fops.append(f)
        pages.append(page)
    built = s.build(pl.flag_set(0, part.n_rows), *pages)
    s.release(*fops)
    return built


def q16(part: Page, ps: Page, supp: Page, type_name):
    """Q16 parts/supplier relationship (q16.sql).  The disjunctive part
    qualifiers (size IN 8 values, type NOT LIKE 'MEDIUM POLISHED%')
    build one dense flag set through repeated conjunctive fill passes;
    complaint suppliers come from the CONTAINS2 'Customer..Complaints'
    comment predicate (anti-semijoin); count(DISTINCT suppkey) per
    (brand, type, size) runs as composite-key (KEYSHL) fused-agg
    dedup + a second grouping probe.  type_name maps a type id to its
    display string for the final ORDER BY.  Returns
    [(brand, type_id, size, supplier_cnt)] in golden order."""
    SIZES = (49, 14, 23, 45, 19, 3, 36, 9)
    brandc = part.channel("brand")
    typec = part.channel("type_id")
    sizec = part.channel("size")
    with Scope() as s:
        # qualifying-part flag set: the disjunction (8 sizes x NOT a type
        # range) decomposes into 16 conjunctive filter passes
        oqual = _fill_flag_set(s, part, [
            [pl.pred(sizec, CMP_EQ, v), pl.pred(brandc, CMP_NE, 45),
             pl.pred(typec, op_, bound)]
            for v in SIZES for op_, bound in ((CMP_LE, 64), (CMP_GE, 70))])

        # complaint suppliers: CONTAINS2('Customer','Complaints') flag set
        ocompl = s.build(pl.flag_set(
            supp.channel("suppkey"), supp.n_rows,
            preds=[pl.pred_varbin(supp.channel("comment"), CMP_CONTAINS2,
                                  b"Customer", b"Complaints")]), supp)

        # part attributes keyed by partkey (qualifying parts only)
        oattr = s.build(pl.hash_build(
            part.channel("partkey"), semijoin_table=oqual.table(),
            semijoin_col=part.channel("partkey"),
            bitmap_max_key=part.n_rows, payload=[brandc, typec, sizec],
            capacity_hint=part.n_rows), part)

        # ps -> attributes emit join, then composite keys
        ja, pa = s.pipe(OP_LOOKUP_JOIN, pl.emit_join(
            oattr.table(), ps.channel("partkey"), [ps.channel("suppkey")]),
            ps)
        # pa: [sk, brand, type, size]
        f1, pb = s.pipe(OP_FILTER_PROJECT, pl.filter_project(
            [pl.ident(1), pl.ident(2), pl.ident(3), pl.ident(0)],
            semijoin_table=ocompl.table(), semijoin_col=0, semijoin_anti=1),
            pa)
        # pb: [brand, type, size, sk]

        # count(DISTINCT suppkey) per (brand, type, size) as two general
        # multi-channel group-bys (MultiChannelGroupByHash analog):
        # distinct (brand,type,size,sk) rows, then supplier count per group
        g1 = s.run(OP_GROUPBY_MULTI, pl.group_by(
            range(4), [pl.count()], max(pb.n_rows, 1024)), pb)
        pdist = g1.get_output_raw()  # [brand, type, size, sk, cnt, cnt]
        g2 = s.run(OP_GROUPBY_MULTI, pl.group_by(
            range(3), [pl.count()], max(pdist.n_rows, 1024)), pdist)
        out = g2.get_output(["brand", "type", "size", "scnt", "cnt"])
        s.release(g2, g1, f1, ja, oqual, ocompl, oattr)
    rows = [(int(out["brand"][i]), int(out["type"][i]), int(out["size"][i]),
             int(out["scnt"][i])) for i in range(len(out["brand"]))]
    rows.sort(key=lambda r: (-r[3], r[0], type_name(r[1]), r[2]))
    return rows


def q10(cust_n: int, orders: Page, li: Page, limit=20):
    """Q10 returned items (q10.sql): orders date filter fused into a
    chained build (payload custkey); returned lineitems emit-join to
    their customer; per-customer revenue by fused-agg probe; the group
    page goes raw through rev > 0 into ORDER_BY (revenue desc, custkey
    asc, limit).  Returns [(custkey, revenue_1e4)]."""
    with Scope() as s:
        odate = orders.channel("orderdate")
        oo = s.build(pl.hash_build(
            orders.channel("orderkey"),
            preds=[pl.pred(odate, CMP_GE, 8674),
                   pl.pred(odate, CMP_LT, 8766)],
            payload=[orders.channel("custkey")],
            capacity_hint=max(orders.n_rows // 8, 16),
            bitmap_max_key=okey_max(orders.n_rows)), orders)
        # the customer group domain is the keys 1..cust_n themselves
        oc = s.build(pl.range_group(cust_n))
        # one fused pass: probe orders by orderkey, group the revenue by
        # the matched o_custkey payload into the customer table (mode 3)
        j2 = s.run(OP_LOOKUP_JOIN, pl.lookup_join(
            oo.table(), li.channel("orderkey"), 3, table2=oc.table(),
            preds=[pl.pred(li.channel("returnflag"), CMP_EQ, ord("R"))],
            proj=pl.disc_price(li.channel("extendedprice"),
                               li.channel("discount")),
            dec_scale=4, dec_only=1), li)
        # [custkey, rev, f64, cnt] stays on the device: customers with
        # revenue, sorted there, and only `limit` rows cross to the host
        f, pos = s.pipe(OP_FILTER_PROJECT, pl.filter_project(
            [pl.ident(0), pl.ident(1)], preds=[pl.pred(1, CMP_GT, 0)]),
            j2.get_output_raw())
        ob = s.run(OP_ORDER_BY, pl.order_by(
            [pl.desc(1), pl.asc(0)], [0, 1], limit), pos)
        top = ob.get_output(["custkey", "rev"])
        s.release(ob, f, j2, oo, oc)
    return [(int(c), int(r)) for c, r in zip(top["custkey"], top["rev"])]


def q15(supp: Page, li: Page):
    """Q15 top supplier (q15.sql): per-supplier revenue over the 1996-Q1
    window by fused-agg probe; the scalar max subquery resolves on the
    group page (output stage).  Returns [(suppkey, revenue_1e4)] of the
    max-revenue supplier(s), suppkey ascending."""
    with Scope() as s:
        os_ = s.build(pl.hash_build(
            supp.channel("suppkey"), capacity_hint=supp.n_rows + 64,
            agg_table=1), supp)
        sd = li.channel("shipdate")
        jo = s.run(OP_LOOKUP_JOIN, pl.agg_join(
            os_.table(), li.channel("suppkey"),
            pl.disc_price(li.channel("extendedprice"),
                          li.channel("discount")), 4,
            preds=[pl.pred(sd, CMP_GE, 9496), pl.pred(sd, CMP_LT, 9587)],
            dec_only=1), li)
        g = jo.get_output(["suppkey", "rev", "f64", "cnt"])
    rev = np.asarray(g["rev"])
    rows = []
    if len(rev):
        mx = int(rev.max())
        if mx > 0:
            sel = np.nonzero(rev == mx)[0]
            sk = np.asarray(g["suppkey"])[sel]
            order = np.argsort(sk)
            rows = [(int(sk[i]), mx) for i in order]
    return rows


def q20(part: Page, ps: Page, supp: Page, li: Page):
    """Q20 potential part promotion (q20.sql): 'forest%' as a VARBIN
    PREFIX flag set; per-(part,supplier) 1994 quantities via a
    composite-key (KEYSHL) fused-agg probe; the correlated
    availqty > 0.5*sum compare runs as 2*availqty > sum using a KEYSHL
    doubling against the group page's zero column (missing sums drop at
    the inner join — SQL's NULL comparison); CANADA(3) semijoin;
    distinct suppliers via a final fused-agg probe.  Returns qualifying
    suppkeys ascending."""
    with Scope() as s:
        of = s.build(pl.flag_set(
            part.channel("partkey"), part.n_rows,
            preds=[pl.pred_varbin(part.channel("name"), CMP_PREFIX,
                                  b"forest")]), part)

        # forest 1994 lineitems -> composite (pk<<32|sk, qty)
        sd = li.channel("shipdate")
        f1, lq = s.pipe(OP_FILTER_PROJECT, pl.filter_project(
            [pl.keyshl(li.channel("partkey"), li.channel("suppkey"), 32),
             pl.ident(li.channel("quantity"))],
            preds=[pl.pred(sd, CMP_GE, 8766), pl.pred(sd, CMP_LT, 9131)],
            semijoin_table=of.table(),
            semijoin_col=li.channel("partkey")), li)
        # lq: [key, qty]
        ok_ = s.build(pl.hash_build(0, capacity_hint=max(lq.n_rows, 1024)),
                      lq)
        jo = s.run(OP_LOOKUP_JOIN,
                   pl.agg_join(ok_.table(), 0, pl.ident(1), dec_only=1), lq)
        sums = jo.get_output_raw()  # [key, sum_qty, f64(zeros), cnt]

        # forest partsupp rows -> [key, availqty, suppkey]
        f2, psq = s.pipe(OP_FILTER_PROJECT, pl.filter_project(
            [pl.keyshl(ps.channel("partkey"), ps.channel("suppkey"), 32),
             pl.ident(ps.channel("availqty")),
             pl.ident(ps.channel("suppkey"))],
            semijoin_table=of.table(),
            semijoin_col=ps.channel("partkey")), ps)
        osum = s.build(pl.hash_build(
            0, payload=[1,   # sum_qty
                        2],  # the zero column (for the KEYSHL doubling)
            capacity_hint=max(sums.n_rows, 1024)), sums)
        j3, pj = s.pipe(OP_LOOKUP_JOIN, pl.emit_join(
            osum.table(), 0, [1, 2]), psq)  # emit availqty, suppkey
        # pj: [aq, sk, sum, zeros]

        ocan = s.build(pl.flag_set(
            supp.channel("suppkey"), supp.n_rows,
            preds=[pl.pred(supp.channel("nationkey"), CMP_EQ, 3)]), supp)
        f3, pk2 = s.pipe(OP_FILTER_PROJECT, pl.filter_project(
            [pl.keyshl(0, 3, 1),  # 2*availqty (zeros low bit)
             pl.ident(1),         # suppkey
             pl.ident(2)],        # sum
            semijoin_table=ocan.table(), semijoin_col=1), pj)
        # pk2: [2aq, sk, sum]
        f4, excess = s.pipe(OP_FILTER_PROJECT, pl.filter_project(
            [pl.ident(1)], preds=[pl.pred_cols(0, CMP_GT, 2)]), pk2)
        # excess: [sk] with dupes

        oq = s.build(pl.hash_build(
            supp.channel("suppkey"), capacity_hint=supp.n_rows + 64,
            agg_table=1), supp)
        j5 = s.run(OP_LOOKUP_JOIN,
                   pl.agg_join(oq.table(), 0, pl.ident(0), dec_only=1),
                   excess)
        out = j5.get_output(["suppkey", "s", "f", "c"])
        s.release(j5, f4, f3, j3, f2, jo, f1, of, ok_, osum, ocan, oq)
        return sorted(int(v) for v in out["suppkey"])


def q2(part: Page, ps: Page, supp: Page, s_abal, s_nat, limit=100):
    """Q2 minimum-cost supplier (q02.sql): size-15 '%BRASS' parts (the
    type%5 disjunction as 30 conjunctive flag-set fills), EUROPE
    suppliers, per-part MIN supplycost via a dec_min fused-agg probe,
    then an equality join back to emit the (supplier, part) pairs.  The
    final ORDER BY (acctbal desc, nation name, supplier, part) resolves
    on the host output stage from the pinned streams.  Returns
    [(suppkey, partkey)] in golden order."""
    with Scope() as s:
        # qualifying parts: size == 15 AND type % 5 == 2 ('%BRASS')
        oq = _fill_flag_set(s, part, [
            [pl.pred(part.channel("size"), CMP_EQ, 15),
             pl.pred(part.channel("type_id"), CMP_EQ, t)]
            for t in range(2, 150, 5)])

        # EUROPE supplier flag set: nation-key set semijoin (region 3
        # nations: FRANCE, GERMANY, ROMANIA, RUSSIA, UNITED KINGDOM)
        on = _key_set(s, (6, 7, 19, 22, 23))
        fe, eup = s.pipe(OP_FILTER_PROJECT, pl.filter_project(
            [pl.ident(supp.channel("suppkey"))], semijoin_table=on.table(),
            semijoin_col=supp.channel("nationkey")), supp)
        oeu = s.build(pl.flag_set(0, supp.n_rows), eup)
        s.release(fe)

        # partsupp restricted to qualifying parts AND european suppliers
        f1, pa = s.pipe(OP_FILTER_PROJECT, pl.filter_project(
            [pl.ident(ps.channel(n)) for n in
             ("partkey", "suppkey", "supplycost")],
            semijoin_table=oq.table(),
            semijoin_col=ps.channel("partkey")), ps)
        f2, pb = s.pipe(OP_FILTER_PROJECT, pl.filter_project(
            [pl.ident(i) for i in range(3)], semijoin_table=oeu.table(),
            semijoin_col=1), pa)
        # pb: [pk, sk, cost_cents]

        # per-part MIN supplycost
        om = s.build(pl.hash_build(
            part.channel("partkey"), semijoin_table=oq.table(),
            semijoin_col=part.channel("partkey"),
            capacity_hint=max(part.n_rows // 64, 4096), agg_table=1,
            bitmap_max_key=part.n_rows), part)
        j1 = s.run(OP_LOOKUP_JOIN,
                   pl.agg_join(om.table(), 0, pl.ident(2), dec_min=1), pb)
        mins = j1.get_output_raw()  # [pk, min_cost, f64, cnt]
        omm = s.build(pl.hash_build(
            0, payload=[1], capacity_hint=max(mins.n_rows, 16)), mins)
        j2, pc = s.pipe(OP_LOOKUP_JOIN,
                        pl.emit_join(omm.table(), 0, range(3)), pb)
        # pc: [pk, sk, cost, min]
        f3 = s.op(OP_FILTER_PROJECT, pl.filter_project(
            [pl.ident(1), pl.ident(0)], preds=[pl.pred_cols(2, CMP_EQ, 3)]))
        f3.add_input_raw(pc)
        out = f3.get_output(["suppkey", "partkey"])
        s.release(f3, j2, j1, f2, f1, oq, on, oeu, om, omm)
    rows = sorted(
        ((int(out["suppkey"][i]), int(out["partkey"][i]))
         for i in range(len(out["suppkey"]))),
        key=lambda r: (-int(s_abal[r[0] - 1]),
                       NATION_NAMES[int(s_nat[r[0] - 1])], r[0], r[1]))
    return rows[:limit]


NATION_NAMES = [
    "ALGERIA", "ARGENTINA", "BRAZIL", "CANADA", "EGYPT", "ETHIOPIA",
    "FRANCE", "GERMANY", "INDIA", "INDONESIA", "IRAN", "IRAQ", "JAPAN",
    "JORDAN", "KENYA", "MOROCCO", "MOZAMBIQUE", "PERU", "CHINA", "ROMANIA",
    "SAUDI ARABIA", "VIETNAM", "RUSSIA", "UNITED KINGDOM", "UNITED STATES"]


Q22_CODE_NATIONS = (3, 7, 8, 13, 19, 20, 21)  # codes '13'..'31' ascending


def q22(cust: Page, orders: Page):
    """Q22 global sales opportunity (q22.sql): customers of the 7 phone
    country codes (code = nationkey+10) with above-average positive
    balance and no orders (anti-semijoin NOT-EXISTS pushdown).  The
    population average becomes a strict plan constant
    floor(sum/cnt).  Returns (counts[7], sums_cents[7]) in code order."""
    abc = cust.channel("acctbal")
    natc = cust.channel("nationkey")
    with Scope() as s:
        on = _key_set(s, Q22_CODE_NATIONS)

        # positive-balance population aggregate (sum, count)
        f0, ppage = s.pipe(OP_FILTER_PROJECT, pl.filter_project(
            [pl.ident(abc)], preds=[pl.pred(abc, CMP_GT, 0)],
            semijoin_table=on.table(), semijoin_col=natc), cust)
        r = _agg_once(s, pl.small_agg(
            [pl.sum_dec(pl.ident(0), 0), pl.count()]), ppage,
            ["hi", "lo", "cnt"])
        sum_pos, cnt_pos = _ticks(r), int(r["cnt"][0])
        s.release(f0)

        oo = s.build(pl.hash_build(
            orders.channel("custkey"), capacity_hint=orders.n_rows,
            key_set_only=1), orders)
        f1, page1 = s.pipe(OP_FILTER_PROJECT, pl.filter_project(
            [pl.ident(cust.channel("custkey")), pl.ident(natc),
             pl.ident(abc)],
            preds=[pl.pred(abc, CMP_GT, sum_pos // cnt_pos)],
            semijoin_table=on.table(), semijoin_col=natc), cust)
        f2, page2 = s.pipe(OP_FILTER_PROJECT, pl.filter_project(
            [pl.ident(1), pl.ident(2)], semijoin_table=oo.table(),
            semijoin_col=0, semijoin_anti=1), page1)
        # page2: [nationkey, acctbal]
        out = _agg_once(s, pl.small_agg(
            [pl.sum_dec(pl.ident(1), 0), pl.count()],
            keys=[(0, Q22_CODE_NATIONS)]), page2,
            ["nationkey", "hi", "lo", "cnt"])
        s.release(f2, f1, on, oo)
    cnts = [0] * len(Q22_CODE_NATIONS)
    sums = [0] * len(Q22_CODE_NATIONS)
    for i in range(len(out["nationkey"])):
        j = Q22_CODE_NATIONS.index(int(out["nationkey"][i]))
        cnts[j] = int(out["cnt"][i])
        sums[j] = _ticks(out, i)
    return cnts, sums


def q4(orders: Page, li_dates: Page):
    """Q4 order-priority checking (q04.sql): EXISTS(lineitem with
    commitdate < receiptdate) as a key-set build with a col-vs-col
    predicate, then orders filter (date range + semijoin) and a 5-value
    priority COUNT aggregation.  Returns counts per priority 0..4."""
    with Scope() as s:
        # dense flag set over the orderkey range (one byte per possible
        # key, ~600 MB at SF100): one predicated scan + flag stores
        # replaces the 380M-key chained set insert, and the semijoin probe
        # is one byte load (all lineitem orderkeys are in range by FK)
        b = s.build(pl.flag_set(
            li_dates.channel("orderkey"), okey_max(orders.n_rows),
            preds=[pl.pred_cols(li_dates.channel("commitdate"), CMP_LT,
                                li_dates.channel("receiptdate"))]), li_dates)
        odate = orders.channel("orderdate")
        f, fpage = s.pipe(OP_FILTER_PROJECT, pl.filter_project(
            [pl.ident(orders.channel("priority"))],
            preds=[pl.pred(odate, CMP_GE, 8582),
                   pl.pred(odate, CMP_LT, 8674)],
            semijoin_table=b.table(),
            semijoin_col=orders.channel("orderkey")), orders)
        out = _agg_once(s, pl.small_agg(
            [pl.count()], keys=[(0, range(5))]), fpage,
            ["priority", "count"])
    counts = [0] * 5
    for i in range(len(out["priority"])):
        counts[int(out["priority"][i])] = int(out["count"][i])
    return counts
