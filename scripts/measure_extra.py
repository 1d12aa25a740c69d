#!/usr/bin/env python3
"""Measurement harness for the fifteen beyond-contract query pipelines
(everything outside bench.py's q1/q3/q5) at a given scale factor.

TEST/BENCH INFRASTRUCTURE: generates inputs with the oracle's dbgen
restatement (like bench.py), stages the hot columns into HBM as torch
tensors, times the GPU pipeline (best of reps, wall clock around the
operator graph), and verifies the result against the CPU oracle run on
the host cores.  Writes one JSON line per query to stdout and
gpurun_out/extra_q.json.

Usage: python scripts/measure_extra.py [--sf 30] [--reps 3]
       [--queries q9,q12,...]
"""
import argparse
import json
import os
import pathlib
import sys
import time

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))

import numpy as np  # noqa: E402
import torch  # noqa: E402

from tests.oracle_binding import OracleLib  # noqa: E402
import presto_amd as P  # noqa: E402
from presto_amd.pipelines import Q22_CODE_NATIONS  # noqa: E402

REPO = pathlib.Path(__file__).resolve().parent.parent


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def page(cols):
    """Stage every column into HBM — including variable-width ones (the
    boundary of SURVEY.md §8d: data starts device-resident; re-uploading
    VARBIN bytes per step would put PCIe inside the timed region)."""
    def up(v):
        if isinstance(v, (P.Varbin, P.DictVarbin)):
            return P.DeviceVarbin.from_host(v)
        return dev(v)
    return P.Page({k: up(v) for k, v in cols.items()})


def run(name, fn, reps):
    best = None
    out = None
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        out = fn()
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return out, best


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sf", type=float, default=30.0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--queries",
                    default="q2,q4,q6,q7,q8,q9,q9_multikey,q10,q11,q12,q13,"
                            "q14,q15,"
                            "q16,q17,q18,q19,q20,q21,q22")
    args = ap.parse_args()
    sf = args.sf
    orc = OracleLib(str(REPO / "oracle" / "liboracle.so"))
    want = set(args.queries.split(","))

    print(f"generating SF{sf} inputs on host ...", file=sys.stderr)
    li = orc.gen_lineitem2(sf)
    lpk = orc.gen_lineitem_partkey(sf)
    orders = orc.gen_orders(sf)
    cust = orc.gen_customer2(sf)
    supp = orc.gen_supplier(sf)
    n_li = len(li["orderkey"])
    results = []

    def record(q, secs, ok, extra=None):
        r = {"query": q, "sf": sf, "ms": round(secs * 1e3, 3),
             "grows_per_s": round(n_li / secs / 1e9, 3), "exact": bool(ok),
             "n_lineitem": n_li}
        if extra:
            r.update(extra)
        results.append(r)
        print(json.dumps(r), flush=True)

    if "q6" in want:
        pages = (page({k: li[k] for k in
                       ("quantity", "extendedprice", "discount",
                        "shipdate")}),)
        got, secs = run("q6", lambda: P.pipelines.q6(*pages), args.reps)
        rev, cnt = orc.q6(li)
        ok = (len(got["rev_lo"]) == 1 and int(got["rev_lo"][0]) == rev
              and int(got["count"][0]) == cnt)
        record("q6", secs, ok)

    if "q4" in want:
        pri = orc.gen_orders_priority(sf)
        lid = orc.gen_lineitem_dates(sf)
        pages = (page({"orderkey": orders["orderkey"],
                       "orderdate": orders["orderdate"],
                       "priority": pri}),
                 page({k: lid[k] for k in ("orderkey", "commitdate",
                                           "receiptdate")}))
        got, secs = run("q4", lambda: P.pipelines.q4(*pages), args.reps)
        exp = orc.q4(orders, pri, lid)
        record("q4", secs, got == exp)
        del pages, lid

    if "q7" in want:
        pages = (page({"custkey": cust["custkey"],
                       "nationkey": cust["nationkey"]}),
                 page({k: orders[k] for k in ("orderkey", "custkey")}),
                 page({"suppkey": supp["suppkey"],
                       "nationkey": supp["nationkey"]}),
                 page({k: li[k] for k in
                       ("orderkey", "suppkey", "extendedprice",
                        "discount", "shipdate")}))
        got, secs = run("q7", lambda: P.pipelines.q7(*pages), args.reps)
        exp = orc.q7(cust, orders, li, supp)
        exp_t = [(r.supp_nation, r.cust_nation, r.year, r.revenue_1e4)
                 for r in exp]
        record("q7", secs, sorted(got) == sorted(exp_t))
        del pages

    if "q11" in want:
        ps11 = orc.gen_partsupp(sf)
        n_part = int(200000 * sf)
        pages = (page({"suppkey": supp["suppkey"],
                       "nationkey": supp["nationkey"]}),
                 page({"partkey": ps11["partkey"],
                       "suppkey": ps11["suppkey"],
                       "supplycost": ps11["supplycost_cents"] / 100.0,
                       "availqty":
                           ps11["availqty"].astype(np.float64)}),)
        got_pk, got_val = None, None

        def _q11():
            return P.pipelines.q11(pages[0], pages[1], n_part)
        got, secs = run("q11", _q11, args.reps)
        got_pk, got_val = got
        exp_pk, exp_val = orc.q11(ps11, supp, n_part)
        ok = (list(got_pk) == list(exp_pk) and
              got_val.tolist() == list(exp_val))
        record("q11", secs, ok)
        del pages, ps11

    if "q2" in want:
        part3 = orc.gen_part3(sf)
        ptype = orc.gen_part_type(sf)
        ps = orc.gen_partsupp(sf)
        abal = orc.gen_supplier_acctbal(sf)
        n_part = len(ptype)
        pages = (page({"partkey": np.arange(1, n_part + 1, dtype=np.int64),
                       "type_id": ptype, "size": part3["size"]}),
                 page({"partkey": ps["partkey"], "suppkey": ps["suppkey"],
                       "supplycost": ps["supplycost_cents"]}),
                 page({"suppkey": supp["suppkey"],
                       "nationkey": supp["nationkey"]}),
                 abal, supp["nationkey"])
        got, secs = run("q2", lambda: P.pipelines.q2(*pages), args.reps)
        exp = orc.q2(part3, ptype, ps, supp, abal)
        record("q2", secs, got == exp)
        del pages, ps

    if "q10" in want:
        n_cust = len(cust["custkey"])
        pages = (page({k: orders[k] for k in ("orderkey", "custkey",
                                              "orderdate")}),
                 page({"orderkey": li["orderkey"],
                       "returnflag": li["returnflag"],
                       "extendedprice": li["extendedprice"],
                       "discount": li["discount"]}))
        got, secs = run("q10", lambda: P.pipelines.q10(n_cust, *pages),
                        args.reps)
        exp = orc.q10(orders, li, n_cust)
        record("q10", secs, got == exp)
        del pages

    if "q13" in want:
        # the o_comment VariableWidthBlock has int32 offsets (the
        # reference Slice cap), so at full SF the orders table arrives
        # as MULTIPLE pages of <= 30M orders — Driver-style paging, no
        # scale cap
        from presto_amd.engine import Varbin
        n_ord = len(orders["custkey"])
        chunk = 30_000_000
        off_all, ln_all = orc.gen_orders_comment(sf)
        pool = np.frombuffer(orc.text_pool(), np.uint8)
        opages = []
        for a in range(0, n_ord, chunk):
            b = min(a + chunk, n_ord)
            ln = ln_all[a:b]
            offs = np.zeros(b - a + 1, np.int32)
            np.cumsum(ln, out=offs[1:])
            starts = np.repeat(off_all[a:b] -
                               offs[:-1].astype(np.int64), ln)
            data = pool[starts + np.arange(int(offs[-1]))]
            cm = Varbin.__new__(Varbin)
            cm.data, cm.offsets, cm.n = data, offs, b - a
            opages.append(P.Page({"custkey": dev(orders["custkey"][a:b]),
                                  "comment":
                                      P.DeviceVarbin.from_host(cm)}))
        n_cust = int(150000 * sf)
        got, secs = run("q13", lambda: P.pipelines.q13(n_cust, opages),
                        args.reps)
        exp = orc.q13(sf, orders)
        record("q13", secs, got == exp, {"sf": sf})
        del opages

    if "q15" in want:
        pages = (page({"suppkey": supp["suppkey"],
                       "nationkey": supp["nationkey"]}),
                 page({"suppkey": li["suppkey"], "shipdate": li["shipdate"],
                       "extendedprice": li["extendedprice"],
                       "discount": li["discount"]}))
        got, secs = run("q15", lambda: P.pipelines.q15(*pages), args.reps)
        exp = orc.q15(li, len(supp["suppkey"]))
        record("q15", secs, got == exp)
        del pages

    if "q16" in want:
        part3 = orc.gen_part3(sf)
        ptype = orc.gen_part_type(sf)
        ps = orc.gen_partsupp(sf)
        bbb = orc.gen_supplier_bbb(sf)
        pool = orc.text_pool()
        soff = np.empty(len(bbb), np.int64)
        sln = np.empty(len(bbb), np.int32)
        import ctypes as CT
        orc.lib.tpch_gen_supplier_comment(
            CT.c_double(sf), CT.c_int64(0), CT.c_int64(len(bbb)),
            soff.ctypes.data_as(CT.c_void_p),
            sln.ctypes.data_as(CT.c_void_p))
        strings = []
        for i in range(len(bbb)):
            t = pool[soff[i]:soff[i] + sln[i]]
            if bbb[i] == 1:
                t = t[:5] + b"Customer criticizes Complaints" + t[5:]
            elif bbb[i] == 2:
                t = t[:5] + b"Customer Recommends" + t[5:]
            strings.append(t)
        n_part = len(ptype)
        pages = (page({"partkey": np.arange(1, n_part + 1, dtype=np.int64),
                       "brand": part3["brand"], "type_id": ptype,
                       "size": part3["size"]}),
                 page({"partkey": ps["partkey"], "suppkey": ps["suppkey"]}),
                 P.Page({"suppkey": dev(supp["suppkey"]),
                         "comment": P.Varbin(strings)}),
                 orc.part_type_name)
        got, secs = run("q16", lambda: P.pipelines.q16(*pages), args.reps)
        exp = orc.q16(part3, ptype, ps, bbb)
        record("q16", secs, got == exp)
        del pages, ps, strings

    if "q20" in want:
        words = orc.gen_part_name_words(sf)
        names = [orc.color_name(i) for i in range(92)]
        strings = [" ".join(names[w] for w in row).encode() for row in words]
        ps = orc.gen_partsupp(sf)
        pages = (P.Page({"partkey": dev(np.arange(1, len(strings) + 1,
                                                  dtype=np.int64)),
                         "name": P.Varbin(strings)}),
                 page({"partkey": ps["partkey"], "suppkey": ps["suppkey"],
                       "availqty": ps["availqty"]}),
                 page({"suppkey": supp["suppkey"],
                       "nationkey": supp["nationkey"]}),
                 page({"partkey": lpk, "suppkey": li["suppkey"],
                       "quantity": li["quantity"],
                       "shipdate": li["shipdate"]}))
        got, secs = run("q20", lambda: P.pipelines.q20(*pages), args.reps)
        exp = orc.q20(words, ps, li, lpk, supp)
        record("q20", secs, got == exp)
        del pages, ps, strings, words

    if "q8" in want:
        ptype = orc.gen_part_type(sf)
        pages = (page({"custkey": cust["custkey"],
                       "nationkey": cust["nationkey"]}),
                 page({k: orders[k] for k in ("orderkey", "custkey",
                                              "orderdate")}),
                 page({"suppkey": supp["suppkey"],
                       "nationkey": supp["nationkey"]}),
                 page({"partkey": np.arange(1, len(ptype) + 1,
                                            dtype=np.int64),
                       "type_id": ptype}),
                 page({"orderkey": li["orderkey"], "suppkey": li["suppkey"],
                       "partkey": lpk, "extendedprice": li["extendedprice"],
                       "discount": li["discount"]}))
        got, secs = run("q8", lambda: P.pipelines.q8(*pages), args.reps)
        exp = orc.q8(cust, orders, li, lpk, supp, ptype)
        record("q8", secs, tuple(got[0]) == tuple(exp[0]) and
               tuple(got[1]) == tuple(exp[1]))
        del pages, ptype

    if "q9" in want or "q9_multikey" in want:
        ps = orc.gen_partsupp(sf)
        words = orc.gen_part_name_words(sf)
        names = [orc.color_name(i) for i in range(92)]
        strings = [" ".join(names[w] for w in row).encode() for row in words]
        n_part = len(strings)
        pages = (P.Page({"partkey": dev(np.arange(1, n_part + 1,
                                                  dtype=np.int64)),
                         "name": P.Varbin(strings)}),
                 page({"suppkey": supp["suppkey"],
                       "nationkey": supp["nationkey"]}),
                 page({"orderkey": orders["orderkey"],
                       "orderdate": orders["orderdate"]}),
                 page({"partkey": ps["partkey"], "suppkey": ps["suppkey"],
                       "supplycost": ps["supplycost_cents"] / 100.0}),
                 page({"partkey": lpk, "suppkey": li["suppkey"],
                       "orderkey": li["orderkey"],
                       "quantity": li["quantity"],
                       "extendedprice": li["extendedprice"],
                       "discount": li["discount"]}))
        gid = orc.color_id("green")
        p_match = (words == gid).any(axis=1).astype(np.uint8)
        exp = orc.q9(li, lpk, orders, supp, ps, p_match)
        # q9_multikey: the partsupp lookup as one two-key emit join
        for q in ("q9", "q9_multikey"):
            if q in want:
                fn = getattr(P.pipelines, q)
                got, secs = run(q, lambda: fn(*pages), args.reps)
                record(q, secs,
                       np.array_equal(np.array(got, np.int64), exp))
        del pages, ps, words, strings

    if "q12" in want:
        pri = orc.gen_orders_priority(sf)
        lid = orc.gen_lineitem_dates(sf)
        smode = orc.gen_lineitem_shipmode(sf)
        pages = (page({"orderkey": orders["orderkey"], "priority": pri}),
                 page({"orderkey": li["orderkey"], "shipmode": smode,
                       "shipdate": li["shipdate"],
                       "commitdate": lid["commitdate"],
                       "receiptdate": lid["receiptdate"]}))
        got, secs = run("q12", lambda: P.pipelines.q12(*pages), args.reps)
        hi, lo = orc.q12(orders, pri, li, lid, smode)
        record("q12", secs,
               got == {4: (hi[4], lo[4]), 6: (hi[6], lo[6])})
        del pages

    if "q14" in want:
        ptype = orc.gen_part_type(sf)
        pages = (page({"partkey": np.arange(1, len(ptype) + 1,
                                            dtype=np.int64),
                       "type_id": ptype}),
                 page({"partkey": lpk, "extendedprice": li["extendedprice"],
                       "discount": li["discount"],
                       "shipdate": li["shipdate"]}))
        got, secs = run("q14", lambda: P.pipelines.q14(*pages), args.reps)
        exp = orc.q14(li, lpk, ptype)
        record("q14", secs, tuple(got) == tuple(exp))
        del pages, ptype

    if "q17" in want:
        part2 = orc.gen_part2(sf)
        n_part = len(part2["brand"])
        pages = (page({"partkey": np.arange(1, n_part + 1, dtype=np.int64),
                       "brand": part2["brand"],
                       "container": part2["container"]}),
                 page({"partkey": lpk, "quantity": li["quantity"],
                       "extendedprice": li["extendedprice"]}))
        got, secs = run("q17", lambda: P.pipelines.q17(*pages), args.reps)
        exp = orc.q17(li, lpk, part2)
        record("q17", secs, got == exp)
        del pages, part2

    if "q18" in want:
        tp = orc.gen_orders_totalprice(sf)
        li1 = orc.gen_lineitem(sf)
        pages = (page({"orderkey": orders["orderkey"],
                       "custkey": orders["custkey"],
                       "orderdate": orders["orderdate"],
                       "totalprice": tp}),
                 page({"orderkey": li1["orderkey"],
                       "quantity": li1["quantity"]}))
        got, secs = run("q18", lambda: P.pipelines.q18(*pages), args.reps)
        exp = orc.q18(orders, tp, li1)
        record("q18", secs, got == exp)
        del pages, tp, li1

    if "q19" in want:
        part3 = orc.gen_part3(sf)
        smode = orc.gen_lineitem_shipmode(sf)
        sinst = orc.gen_lineitem_shipinstruct(sf)
        n_part = len(part3["brand"])
        pages = (page({"partkey": np.arange(1, n_part + 1, dtype=np.int64),
                       "brand": part3["brand"],
                       "container": part3["container"],
                       "size": part3["size"]}),
                 page({"partkey": lpk, "quantity": li["quantity"],
                       "extendedprice": li["extendedprice"],
                       "discount": li["discount"], "shipmode": smode,
                       "shipinstruct": sinst}))
        got, secs = run("q19", lambda: P.pipelines.q19(*pages), args.reps)
        exp = orc.q19(li, lpk, smode, sinst, part3)
        record("q19", secs, got == exp)
        del pages, part3

    if "q21" in want:
        lid = orc.gen_lineitem_dates(sf)
        pages = (page({"suppkey": supp["suppkey"],
                       "nationkey": supp["nationkey"]}),
                 page({"orderkey": orders["orderkey"]}),
                 page({"orderkey": li["orderkey"], "suppkey": li["suppkey"],
                       "linestatus": li["linestatus"],
                       "commitdate": lid["commitdate"],
                       "receiptdate": lid["receiptdate"]}))
        got, secs = run("q21", lambda: P.pipelines.q21(*pages), args.reps)
        exp = orc.q21(supp, li, lid)
        record("q21", secs, got == exp)
        del pages

    if "q22" in want:
        abal = orc.gen_customer_acctbal(sf)
        pages = (page({"custkey": cust["custkey"],
                       "nationkey": cust["nationkey"], "acctbal": abal}),
                 page({"custkey": orders["custkey"]}))
        got, secs = run("q22", lambda: P.pipelines.q22(*pages), args.reps)
        exp = orc.q22(cust, abal, orders)
        record("q22", secs, list(got[0]) == exp[0] and
               list(got[1]) == exp[1])
        del pages

    os.makedirs("gpurun_out", exist_ok=True)
    with open("gpurun_out/extra_q.json", "w") as f:
        for r in results:
            f.write(json.dumps(r) + "\n")
    bad = [r["query"] for r in results if not r["exact"]]
    print(f"done: {len(results)} queries, inexact: {bad or 'none'}",
          file=sys.stderr)
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
