"""TPC-DS config-5 pipelines (BASELINE.json configs[4]): Q17 and Q72 —
decimal arithmetic + deep multi-join — composed from the same GPU
operator set as TPC-H (filter/semijoin, chained + agg hash builds,
emit-mode joins, the general multi-channel GroupBy).

Data comes from oracle/tpcds.c's dsdgen restatement; parity is pinned
with the oracle as the single data source (see oracle/tpcds.h: the
reference vendors neither the Teradata generator source nor any TPC-DS
golden vectors, so raw dsdgen parity is unpinned in-repo — stated
openly, as SURVEY.md §8c prescribes).  The oracle restates the
query17.tpl / query72.tpl semantics; GPU results must match it
integer-exactly.

Reference anchors for the operator shapes: HashBuilderOperator.java:55,
LookupJoinOperator.java:481-604, MultiChannelGroupByHash.java:300-380,
PageProcessor.java:299-343 (semijoin pushdown = dynamic-filter analog).
"""
import ctypes as C

import numpy as np

from . import plans as pl
from .engine import (
    Scope, OP_FILTER_PROJECT, OP_LOOKUP_JOIN, OP_GROUPBY_MULTI,
    CMP_LT, CMP_GT, CMP_GE, CMP_LE, CMP_EQ, CMP_NE,
)

DATE_COUNT = 73049


class DsGen:
    """ctypes view of the tpcds.c generator + oracle."""

    def __init__(self, lib_path):
        L = C.CDLL(str(lib_path))
        for f in ("dsgen_store_sales_count", "dsgen_store_returns_count",
                  "dsgen_catalog_sales_count", "dsgen_catalog_returns_count",
                  "dsgen_inventory_count", "dsgen_item_count",
                  "dsgen_store_count", "dsgen_warehouse_count",
                  "dsgen_customer_count", "dsgen_promotion_count"):
            getattr(L, f).restype = C.c_int64
            getattr(L, f).argtypes = [C.c_double]
        L.oracle_ds_q17.restype = C.c_int64
        L.oracle_ds_q72.restype = C.c_int64
        self.L = L

    def _p(self, a):
        return C.c_void_p(0 if a is None else a.ctypes.data)

    def date_dim(self):
        year = np.zeros(DATE_COUNT, np.int32)
        qname = np.zeros(DATE_COUNT, np.int32)
        week = np.zeros(DATE_COUNT, np.int32)
        self.L.dsgen_date_dim(self._p(year), self._p(qname), self._p(week))
        return year, qname, week

    def store_sales(self, sf):
        n = self.L.dsgen_store_sales_count(C.c_double(sf))
        d = np.zeros(n, np.int32)
        it = np.zeros(n, np.int64)
        cu = np.zeros(n, np.int64)
        st = np.zeros(n, np.int64)
        tk = np.zeros(n, np.int64)
        q = np.zeros(n, np.int32)
        self.L.dsgen_store_sales(C.c_double(sf), C.c_int64(0), C.c_int64(n),
                                 self._p(d), self._p(it), self._p(cu),
                                 self._p(st), self._p(tk), self._p(q))
        return dict(date=d, item=it, cust=cu, store=st, ticket=tk, qty=q)

    def store_returns(self, sf):
        n = self.L.dsgen_store_returns_count(C.c_double(sf))
        d = np.zeros(n, np.int32)
        it = np.zeros(n, np.int64)
        cu = np.zeros(n, np.int64)
        tk = np.zeros(n, np.int64)
        q = np.zeros(n, np.int32)
        self.L.dsgen_store_returns(C.c_double(sf), C.c_int64(0),
                                   C.c_int64(n), self._p(d), self._p(it),
                                   self._p(cu), self._p(tk), self._p(q))
        return dict(date=d, item=it, cust=cu, ticket=tk, qty=q)

    def catalog_sales(self, sf, want_all=False):
        n = self.L.dsgen_catalog_sales_count(C.c_double(sf))
        sold = np.zeros(n, np.int32)
        it = np.zeros(n, np.int64)
        cu = np.zeros(n, np.int64)
        q = np.zeros(n, np.int32)
        ship = np.zeros(n, np.int32) if want_all else None
        on = np.zeros(n, np.int64) if want_all else None
        cd = np.zeros(n, np.int64) if want_all else None
        hd = np.zeros(n, np.int64) if want_all else None
        pr = np.zeros(n, np.int64) if want_all else None
        self.L.dsgen_catalog_sales(
            C.c_double(sf), C.c_int64(0), C.c_int64(n), self._p(sold),
            self._p(ship), self._p(it), self._p(cu), self._p(on),
            self._p(q), self._p(cd), self._p(hd), self._p(pr))
        out = dict(sold=sold, item=it, cust=cu, qty=q)
        if want_all:
            out.update(ship=ship, order=on, cdemo=cd, hdemo=hd, promo=pr)
        return out

    def catalog_returns(self, sf):
        n = self.L.dsgen_catalog_returns_count(C.c_double(sf))
        it = np.zeros(n, np.int64)
        on = np.zeros(n, np.int64)
        self.L.dsgen_catalog_returns(C.c_double(sf), C.c_int64(0),
                                     C.c_int64(n), self._p(it), self._p(on))
        return dict(item=it, order=on)

    def inventory(self, sf):
        n = self.L.dsgen_inventory_count(C.c_double(sf))
        d = np.zeros(n, np.int32)
        it = np.zeros(n, np.int64)
        wh = np.zeros(n, np.int64)
        q = np.zeros(n, np.int32)
        self.L.dsgen_inventory(C.c_double(sf), C.c_int64(0), C.c_int64(n),
                               self._p(d), self._p(it), self._p(wh),
                               self._p(q))
        return dict(date=d, item=it, wh=wh, qoh=q)

    def cdemo_marital(self):
        n = 1920800
        m = np.zeros(n, np.uint8)
        self.L.dsgen_cdemo(self._p(m))
        return m

    def hdemo_buypot(self):
        n = 7200
        b = np.zeros(n, np.uint8)
        self.L.dsgen_hdemo(self._p(b))
        return b

    def store_state(self, sf):
        n = self.L.dsgen_store_count(C.c_double(sf))
        s = np.zeros(n, np.uint8)
        self.L.dsgen_store(C.c_double(sf), self._p(s))
        return s

    def q17(self, sf, q0):
        N = 1 << 20
        gi = np.zeros(N, np.int64)
        gs = np.zeros(N, np.int32)
        a = [np.zeros(N, np.int64) for _ in range(9)]
        n = self.L.oracle_ds_q17(
            C.c_double(sf), C.c_int32(q0), C.c_int64(N), self._p(gi),
            self._p(gs), *(self._p(x) for x in a))
        return [(int(gi[i]), int(gs[i])) + tuple(int(x[i]) for x in a)
                for i in range(n)]

    def q72(self, sf, year, marital, buypot):
        N = 1 << 23
        gi = np.zeros(N, np.int64)
        gw = np.zeros(N, np.int64)
        gk = np.zeros(N, np.int32)
        b = [np.zeros(N, np.int64) for _ in range(3)]
        n = self.L.oracle_ds_q72(
            C.c_double(sf), C.c_int32(year), C.c_int32(marital),
            C.c_int32(buypot), C.c_int64(N), self._p(gi), self._p(gw),
            self._p(gk), *(self._p(x) for x in b))
        return [(int(gi[i]), int(gw[i]), int(gk[i])) +
                tuple(int(x[i]) for x in b) for i in range(n)]


def _filter(s, page, preds=(), projs=(), semi=0, semi_col=0):
    """Filter/project (+ optional semijoin) over a Page or raw page:
    returns (operator, raw output page)."""
    return s.pipe(OP_FILTER_PROJECT, pl.filter_project(
        projs, preds=preds, semijoin_table=semi, semijoin_col=semi_col),
        page)


def _dense_set(s, page, preds, cap):
    """Dense key set of the column-0 sks passing preds — the
    dynamic-filter analog of a dimension join."""
    f, out = _filter(s, page, preds=preds, projs=[pl.ident(0)])
    b = s.build(pl.flag_set(0, cap + 1), out)
    s.release(f)
    return b


def _date_set(s, date_page, lo, hi):
    """date_sks whose qname/year column c1 is in [lo, hi]."""
    return _dense_set(s, date_page, [pl.pred(1, CMP_GE, lo),
                                     pl.pred(1, CMP_LE, hi)], DATE_COUNT)


def _chain_build(s, page_raw, key_col, payload_cols, hint):
    return s.build(pl.hash_build(key_col, payload=payload_cols,
                                 capacity_hint=max(hint, 16)), page_raw)


def _emit_join(s, page_raw, table, key_col, emit_cols):
    return s.pipe(OP_LOOKUP_JOIN, pl.emit_join(table, key_col, emit_cols),
                  page_raw)


def ds_q17(gen, sf, ss_page, sr_page, cs_page, date_page, q0):
    """TPC-DS Q17 (query17.tpl): store sale in quarter q0, its return in
    q0..q0+2 (joined on customer, item, ticket), a catalog re-purchase
    in q0..q0+2 (joined on customer, item); grouped by (item, store):
    count/sum/sum-of-squares of the three quantities, integer-exact.
    Returns host rows [(item_id, state, c,s,q x3)] sorted, after the
    display-side item_id/state fold."""
    with Scope() as s:
        set_q0 = _date_set(s, date_page, q0, q0)
        set_q02 = _date_set(s, date_page, q0, q0 + 2)

        # store_sales in q0 -> chained table keyed by ticket
        f_ss, p_ss = _filter(s, ss_page,
                             projs=(pl.ident(4),   # ticket
                                    pl.ident(2),   # cust
                                    pl.ident(1),   # item
                                    pl.ident(5),   # qty
                                    pl.ident(3)),  # store
                             semi=set_q0.table())
        b1 = _chain_build(s, p_ss, 0, (1, 2, 3, 4), p_ss.n_rows)

        # store_returns in q0..q0+2 probe on ticket, then (cust,item)
        # equality
        f_sr, p_sr = _filter(s, sr_page,
                             projs=(pl.ident(3),   # ticket
                                    pl.ident(2),   # cust
                                    pl.ident(1),   # item
                                    pl.ident(4)),  # rqty
                             semi=set_q02.table())
        j1, p1 = _emit_join(s, p_sr, b1.table(), 0, (1, 2, 3))
        # p1: [r_cust, r_item, rqty, s_cust, s_item, s_qty, s_store]
        f_eq, p_eq = _filter(s, p1,
                             preds=(pl.pred_cols(0, CMP_EQ, 3),
                                    pl.pred_cols(1, CMP_EQ, 4)),
                             projs=(pl.keyshl(0, 1, 20),  # (cust<<20)|item
                                    pl.ident(5),          # ssqty
                                    pl.ident(2),          # rqty
                                    pl.ident(6),          # store
                                    pl.ident(1)))         # item
        b2 = _chain_build(s, p_eq, 0, (1, 2, 3, 4), p_eq.n_rows)

        # catalog re-purchases in q0..q0+2 probe on (cust, item)
        f_cs, p_cs = _filter(s, cs_page,
                             projs=(pl.keyshl(2, 1, 20),
                                    pl.ident(3)),   # csqty
                             semi=set_q02.table())
        j2, p2 = _emit_join(s, p_cs, b2.table(), 0, (1,))
        # p2: [csqty, ssqty, rqty, store, item]

        # per quantity channel: its sum, then its sum of squares
        gop = s.run(OP_GROUPBY_MULTI, pl.group_by(
            [4, 3],  # item, store
            [pl.sum_i64(pl.mul(ch, ch) if sq else pl.ident(ch))
             for ch in (1, 2, 0) for sq in (False, True)],
            max(p2.n_rows * 2, 4096)), p2)
        out = gop.get_output(["item", "store", "s_ss", "q_ss", "s_sr",
                              "q_sr", "s_cs", "q_cs", "cnt"])
        # fixed end-of-query order (see pipelines.py): streams, then tables
        s.release(gop, f_ss, f_sr, j1, f_eq, f_cs, j2,
                  set_q0, set_q02, b1, b2)

    # display-side fold: item_sk -> i_item_id (pairs share an id),
    # store_sk -> s_state; equal (id, state) groups merge
    state = gen.store_state(sf)
    agg = {}
    for i in range(len(out["item"])):
        key = ((int(out["item"][i]) + 1) // 2,
               int(state[int(out["store"][i]) - 1]))
        cur = agg.setdefault(key, [0] * 9)
        cnt = int(out["cnt"][i])
        vals = (cnt, int(out["s_ss"][i]), int(out["q_ss"][i]),
                cnt, int(out["s_sr"][i]), int(out["q_sr"][i]),
                cnt, int(out["s_cs"][i]), int(out["q_cs"][i]))
        for j in range(9):
            cur[j] += vals[j]
    return [k + tuple(v) for k, v in sorted(agg.items())]


def ds_q72(gen, sf, cs_page, inv_pages, cr_page, date_page, cdemo_page,
           hdemo_page, year, marital, buypot):
    """TPC-DS Q72 (query72.tpl): promotional-item inventory shortfalls —
    catalog sales in `year` with the demographics filters and
    ship > sold + 5, joined to the weekly inventory snapshot
    (same item, sold week, any warehouse) where on-hand < ordered;
    LEFT JOINs to promotion (promo/no_promo split) and catalog_returns
    (row multiplicity).  Grouped by (item, warehouse, week_seq).
    Returns host rows [(item_id, wh, week, no_promo, promo, total)]."""
    # the promo / no_promo split as per-aggregate FILTERs on channel 3
    promo_split = [pl.pred(3, CMP_EQ, 0), pl.pred(3, CMP_NE, 0)]
    with Scope() as s:
        set_year = _date_set(s, date_page, year, year)
        # demographics dynamic-filter sets (dense sks)
        cdset = _dense_set(s, cdemo_page, [pl.pred(1, CMP_EQ, marital)],
                           1920800)
        hdset = _dense_set(s, hdemo_page, [pl.pred(1, CMP_EQ, buypot)],
                           7200)

        # cs: year + ship > sold + 5 + demographics, then (item, week) key
        # cs_page cols: [sold, ship, item, order, qty, cdemo, hdemo, promo]
        f1, p = _filter(s, cs_page,
                        preds=[pl.pred_cols(1, CMP_GT, 0, plus=5)],
                        projs=[pl.ident(c) for c in (0, 2, 3, 4, 5, 6, 7)],
                        semi=set_year.table())
        # [sold, item, order, qty, cdemo, hdemo, promo]
        f2, p = _filter(s, p,
                        projs=[pl.ident(c) for c in (0, 1, 2, 3, 5, 6)],
                        semi=cdset.table(), semi_col=4)
        # [sold, item, order, qty, hdemo, promo]
        f3, p = _filter(s, p, projs=(pl.subdiv(0, 0, 7),  # week
                                     pl.ident(1), pl.ident(2), pl.ident(3),
                                     pl.ident(5)),
                        semi=hdset.table(), semi_col=4)
        # [week, item, order, qty, promo]
        f4, p = _filter(s, p, projs=(pl.keyshl(1, 0, 14),   # item<<14|wk
                                     pl.ident(3),           # qty
                                     pl.ident(4),           # promo
                                     pl.keyshl(1, 2, 25)))  # crkey
        b3 = _chain_build(s, p, 0, (1, 2, 3), p.n_rows)

        # inventory probes the (item, week) table; on-hand < ordered.
        # ONE pass: the (item<<14 | date/7) key and the week channel are
        # both derived in the same projection set (KEYSHL_DIV / SUBDIV)
        joined, fqs = [], []
        for inv in inv_pages:
            fi, pi = _filter(s, inv, projs=(pl.keyshl_div(1, 0, 14, 7),
                                            pl.ident(1),
                                            pl.subdiv(0, 0, 7),
                                            pl.ident(2), pl.ident(3)))
            jj, pj = _emit_join(s, pi, b3.table(), 0, (1, 2, 3, 4))
            s.release(fi)
            # pj: [item, wk, wh, qoh, qty, promo, crkey]
            fq, pq = _filter(s, pj, preds=[pl.pred_cols(3, CMP_LT, 4)],
                             projs=[pl.ident(c) for c in (0, 1, 2, 5, 6)])
            s.release(jj)
            fqs.append(fq)
            joined.append(pq)  # [item, wk, wh, promo, crkey]

        # base counts per (item, wk, wh) with the promo split
        gop1 = s.run(OP_GROUPBY_MULTI, pl.group_by(
            range(3), [(pl.count(), 0), (pl.count(), 1)],
            max(sum(pq.n_rows for pq in joined) * 2, 4096),
            filters=promo_split), *joined)
        base = gop1.get_output(["item", "wk", "wh", "no_promo", "promo",
                                "cnt"])
        s.release(gop1)

        # catalog_returns multiplicity: LEFT JOIN row expansion =
        # base + (matches - 1) for matched rows
        f_cr, p_cr = _filter(s, cr_page, projs=(pl.keyshl(0, 1, 25),))
        gopc = s.run(OP_GROUPBY_MULTI, pl.group_by(
            [0], [pl.count()], max(p_cr.n_rows, 1024)), p_cr)
        crg = gopc.get_output_raw()  # [crkey, cnt, cnt]
        ocr = s.build(pl.hash_build(0, payload=[1],
                                    capacity_hint=max(crg.n_rows, 16),
                                    agg_table=1), crg)
        s.release(gopc)

        extra_rows = pl.sum_i64(pl.subdiv(4, 1, 1))  # cr_cnt - 1
        gop2 = s.op(OP_GROUPBY_MULTI, pl.group_by(
            range(3), [(extra_rows, 0), (extra_rows, 1), extra_rows],
            max(len(base["item"]) * 2, 4096), filters=promo_split))
        any_extra = False
        for pq in joined:
            jm, pm = _emit_join(s, pq, ocr.table(), 4, (0, 1, 2, 3))
            # pm: [item, wk, wh, promo, cr_cnt]
            if pm.n_rows:
                gop2.add_input_raw(pm)
                any_extra = True
            s.release(jm)
        gop2.finish()
        extra = gop2.get_output(["item", "wk", "wh", "e_np", "e_p", "e_t",
                                 "cnt"]) if any_extra else None
        # fixed end-of-query order (see pipelines.py): streams, then tables
        s.release(gop2, *fqs, f1, f2, f3, f4, f_cr,
                  set_year, cdset, hdset, b3, ocr)

    # host fold (display side), vectorized: item_sk -> item_id, merge
    # base + extra group rows, sort by (item_id, wh, week)
    def cols(d, names):
        return [np.asarray(d[n]) for n in names]

    b_item, b_wh, b_wk, b_np_, b_p, b_c = cols(
        base, ("item", "wh", "wk", "no_promo", "promo", "cnt"))
    parts = [((b_item + 1) // 2, b_wh, b_wk, b_np_, b_p, b_c)]
    if extra is not None:
        e_item, e_wh, e_wk, e_np_, e_p, e_t = cols(
            extra, ("item", "wh", "wk", "e_np", "e_p", "e_t"))
        parts.append(((e_item + 1) // 2, e_wh, e_wk, e_np_, e_p, e_t))
    item = np.concatenate([p[0] for p in parts])
    wh = np.concatenate([p[1] for p in parts])
    wk = np.concatenate([p[2] for p in parts]).astype(np.int64)
    vnp = np.concatenate([p[3] for p in parts])
    vp = np.concatenate([p[4] for p in parts])
    vt = np.concatenate([p[5] for p in parts])
    key = (item << 32) | (wh << 16) | wk
    ukey, inv_ = np.unique(key, return_inverse=True)
    s_np = np.bincount(inv_, vnp, minlength=len(ukey)).astype(np.int64)
    s_p = np.bincount(inv_, vp, minlength=len(ukey)).astype(np.int64)
    s_t = np.bincount(inv_, vt, minlength=len(ukey)).astype(np.int64)
    return list(zip((ukey >> 32).tolist(),
                    ((ukey >> 16) & 0xffff).tolist(),
                    (ukey & 0xffff).tolist(),
                    s_np.tolist(), s_p.tolist(), s_t.tolist()))
