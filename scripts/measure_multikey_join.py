#!/usr/bin/env python3
"""What a two-key join costs against the spelling it replaces.

Synthetic partsupp-shaped data, generated from a seed on the device: the
build holds P parts x 4 suppliers (partkey, suppkey, cost), every probe row
names one (part, supplier) pair of the build (as q9's lineitem rows do).
Per shape (--parts log2 P x --rows log2 probe rows), two forms:

  a  the single-key spelling (pipelines.q9): a chained build on partkey
     with payloads (suppkey, cost); emit_join on partkey (four candidate
     rows per probe row) and the pred_cols equality FILTER_PROJECT
     suppkey = ps_suppkey behind it
  b  one two-key build on (partkey, suppkey) with payload cost, and one
     two-key emit_join

Build (create, add_input, finish) and probe (create, add_input(s), the
output page left on the device) are timed separately, each with a device
synchronise on both sides.  The forms alternate in one process after a
warm-up; each figure is the mean over a window of at least --window
seconds, and --windows such windows per form give the spread.  Before
timing, both forms' output pages [row id, cost] are copied back at the
timed size and compared: one match per probe row and a pinned probe-row
order make the two pages equal element for element, which is the multiset
equality and more.

Prints one JSON line per shape and writes them all to --out."""
import argparse
import json
import pathlib
import sys
import time

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import presto_amd as P  # noqa: E402
from presto_amd import plans as pl  # noqa: E402

STEP = 2503     # supplier j of part p: (p + j * STEP) % n_supp + 1


def build_a(s, ps):
    return s.build(pl.hash_build(0, payload=[1, 2],
                                 capacity_hint=ps.n_rows), ps)


def build_b(s, ps):
    return s.build(pl.hash_build([0, 1], payload=[2],
                                 capacity_hint=ps.n_rows), ps)


def probe_a(s, table, li):
    # li: [rowid, partkey, suppkey] -> [rowid, sk, ps_sk, cost] -> filter
    j, pa = s.pipe(P.OP_LOOKUP_JOIN, pl.emit_join(table, 1, [0, 2]), li)
    f = s.op(P.OP_FILTER_PROJECT, pl.filter_project(
        [pl.ident(0), pl.ident(3)], preds=[pl.pred_cols(1, P.CMP_EQ, 2)]))
    f.feed(pa)
    return f


def probe_b(s, table, li):
    j = s.op(P.OP_LOOKUP_JOIN, pl.emit_join(table, [1, 2], [0]))
    j.feed(li)
    return j


def window(fn, seconds):
    """Mean ms of fn() over a window of at least `seconds`."""
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    n = 0
    while True:
        fn()
        n += 1
        torch.cuda.synchronize()
        dt = time.perf_counter() - t0
        if dt >= seconds:
            return dt * 1e3 / n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--parts", default="20,22", help="log2 part counts")
    ap.add_argument("--rows", default="24,26", help="log2 probe rows")
    ap.add_argument("--window", type=float, default=1.0)
    ap.add_argument("--windows", type=int, default=3)
    ap.add_argument("--out", default="profiles/multikey_join.json")
    args = ap.parse_args()
    out = pathlib.Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    res = []
    for lgp in (int(x) for x in args.parts.split(",")):
        n_part = 1 << lgp
        n_supp = n_part // 20 + 1
        part = torch.arange(1, n_part + 1, dtype=torch.int64, device="cuda")
        j4 = torch.arange(4, dtype=torch.int64, device="cuda")
        ps_pk = part.repeat_interleave(4)
        ps_sk = (ps_pk + j4.repeat(n_part) * STEP) % n_supp + 1
        gen = torch.Generator(device="cuda").manual_seed(lgp)
        cost = torch.randint(100, 100000, (4 * n_part,), dtype=torch.int64,
                             device="cuda", generator=gen)
        ps = P.Page({"partkey": ps_pk, "suppkey": ps_sk, "cost": cost})
        for lg in (int(x) for x in args.rows.split(",")):
            n = 1 << lg
            gen = torch.Generator(device="cuda").manual_seed(lgp * 131 + lg)
            pk = torch.randint(1, n_part + 1, (n,), dtype=torch.int64,
                               device="cuda", generator=gen)
            jj = torch.randint(0, 4, (n,), dtype=torch.int64, device="cuda",
                               generator=gen)
            sk = (pk + jj * STEP) % n_supp + 1
            rowid = torch.arange(n, dtype=torch.int64, device="cuda")
            li = P.Page({"rowid": rowid, "partkey": pk, "suppkey": sk})
            del jj
            with P.Scope() as s:
                ta, tb = build_a(s, ps), build_b(s, ps)
                # the outputs agree (and warm both forms up)
                oa = probe_a(s, ta.table(), li).get_output(["rowid", "cost"])
                ob = probe_b(s, tb.table(), li).get_output(["rowid", "cost"])
                same = bool(len(oa["rowid"]) == n
                            and np.array_equal(oa["rowid"], ob["rowid"])
                            and np.array_equal(oa["cost"], ob["cost"]))
                del oa, ob
            t = {"build_a": [], "build_b": [], "probe_a": [], "probe_b": []}

            def timed_build(build):
                def go():
                    with P.Scope() as s:
                        build(s, ps)
                return go

            with P.Scope() as s:
                ta, tb = build_a(s, ps), build_b(s, ps)

                def timed_probe(probe, table):
                    def go():
                        with P.Scope() as s2:
                            probe(s2, table, li)
                    return go

                for _ in range(args.windows):
                    t["build_a"].append(window(timed_build(build_a),
                                               args.window))
                    t["build_b"].append(window(timed_build(build_b),
                                               args.window))
                    t["probe_a"].append(window(
                        timed_probe(probe_a, ta.table()), args.window))
                    t["probe_b"].append(window(
                        timed_probe(probe_b, tb.table()), args.window))
            r = {"parts": n_part, "build_rows": 4 * n_part, "probe_rows": n,
                 "same_rows": same, "window_s": args.window}
            for k, v in t.items():
                r[k + "_ms"] = [round(x, 3) for x in v]
                r[k + "_mean_ms"] = round(sum(v) / len(v), 3)
                r[k + "_spread_ms"] = round(max(v) - min(v), 3)
            r["ratio_build_b_over_a"] = round(
                r["build_b_mean_ms"] / r["build_a_mean_ms"], 3)
            r["ratio_probe_b_over_a"] = round(
                r["probe_b_mean_ms"] / r["probe_a_mean_ms"], 3)
            res.append(r)
            print(json.dumps(r), flush=True)
            with open(out, "w") as f:
                json.dump(res, f, indent=1)
            del li, pk, sk, rowid
            torch.cuda.empty_cache()
        del ps, ps_pk, ps_sk, cost
        torch.cuda.empty_cache()
    return 0 if all(r["same_rows"] for r in res) else 1


if __name__ == "__main__":
    sys.exit(main())
