#!/usr/bin/env python3
"""What PG_OP_MARK_DISTINCT costs, against the two things it replaces.

Per shape (--rows log2 row counts x --distinct log2 distinct combinations):
two I64 key columns (g, x), device-resident; g takes 64 values, x the rest
of the combination.  Timed, each with a device synchronise on both sides,
in interleaved rounds after a warm-up round:

  mark          MARK_DISTINCT mark mode add_input over keys (g, x),
                emitting both (insert launch, mark launch, the copies of
                the emit columns); create stays outside the clock
  groupby       yardstick 1: GROUPBY_MULTI add_input with one COUNT over
                the same two keys on the same page — the same table work
                without the ordinal and the mark pass.  k_groupby_multi is
                not touched by MARK_DISTINCT, so this IS the parent
                commit's kernel
  e2e_mark      count(DISTINCT x) GROUP BY g, create to output page:
                MARK_DISTINCT -> GROUPBY_MULTI(g; COUNT FILTER marker = 1)
  e2e_two_stage yardstick 2: q16's spelling of the same query, two
                GROUPBY_MULTI stages (distinct (g, x) rows, then a count
                per g)

Both end-to-end results are verified against torch.unique on the device.
Reports the medians and the ratios mark / groupby and e2e_mark /
e2e_two_stage.  Prints one JSON line per shape and writes them all to
--out."""
import argparse
import json
import pathlib
import statistics
import sys
import time

sys.path.insert(0, str(pathlib.Path(__file__).resolve().parent.parent))
import numpy as np  # noqa: E402
import torch  # noqa: E402
import presto_amd as P  # noqa: E402
from presto_amd import plans as pl  # noqa: E402

G = 64      # values of g


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    out = fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, out


def run_mark(page, distinct):
    with P.Scope() as s:
        op = s.op(P.OP_MARK_DISTINCT,
                  pl.mark_distinct([0, 1], [0, 1], distinct + 16))
        ms, _ = timed(lambda: op.add_input(page))
    return ms


def run_groupby(page, distinct):
    with P.Scope() as s:
        op = s.op(P.OP_GROUPBY_MULTI,
                  pl.group_by([0, 1], [pl.count()], distinct + 16))
        ms, _ = timed(lambda: op.add_input(page))
    return ms


def e2e_mark(page, distinct):
    def go():
        with P.Scope() as s:
            md, marked = s.pipe(
                P.OP_MARK_DISTINCT,
                pl.mark_distinct([0, 1], [0], distinct + 16), page)
            gb = s.run(P.OP_GROUPBY_MULTI, pl.group_by(
                [0], [(pl.count(), 0)], G + 16,
                filters=[pl.pred(1, P.CMP_EQ, 1)]), marked)
            return gb.get_output(["g", "dcnt", "rows"])
    return timed(go)


def e2e_two_stage(page, distinct):
    def go():
        with P.Scope() as s:
            g1 = s.run(P.OP_GROUPBY_MULTI, pl.group_by(
                [0, 1], [pl.count()], distinct + 16), page)
            g2 = s.run(P.OP_GROUPBY_MULTI, pl.group_by(
                [0], [pl.count()], G + 16), g1.get_output_raw())
            return g2.get_output(["g", "dcnt", "rows"])
    return timed(go)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", default="24,26", help="log2 row counts")
    ap.add_argument("--distinct", default="10,22",
                    help="log2 distinct (g, x) combinations")
    ap.add_argument("--out", default="profiles/mark_distinct.json")
    args = ap.parse_args()
    out = pathlib.Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    res = []
    for lg in (int(x) for x in args.rows.split(",")):
        for lgd in (int(x) for x in args.distinct.split(",")):
            n, distinct = 1 << lg, 1 << lgd
            gen = torch.Generator(device="cuda").manual_seed(lg * 131 + lgd)
            combo = torch.randint(0, distinct, (n,), dtype=torch.int64,
                                  device="cuda", generator=gen)
            g, x = combo % G, combo // G
            exp = torch.bincount(torch.unique(combo) % G, minlength=G) \
                .cpu().numpy()
            del combo
            torch.cuda.synchronize()
            page = P.Page({"g": g, "x": x})

            def exact(cols):
                o = np.argsort(cols["g"])
                return bool(np.array_equal(cols["g"][o], np.arange(G))
                            and np.array_equal(cols["dcnt"][o], exp))

            ok = exact(e2e_mark(page, distinct)[1]) and \
                exact(e2e_two_stage(page, distinct)[1])
            cfgs = [("mark", run_mark), ("groupby", run_groupby),
                    ("e2e_mark", lambda p, d: e2e_mark(p, d)[0]),
                    ("e2e_two_stage", lambda p, d: e2e_two_stage(p, d)[0])]
            times = {name: [] for name, _ in cfgs}
            for _ in range(args.reps + 1):       # the first is a warm-up
                for name, fn in cfgs:
                    times[name].append(fn(page, distinct))
            med = {k: statistics.median(v[1:]) for k, v in times.items()}
            r = {"rows": n, "distinct": distinct, "groups": G, "exact": ok}
            for k, v in times.items():
                r[k + "_ms"] = [round(t, 3) for t in v[1:]]
                r[k + "_median_ms"] = round(med[k], 3)
            r["ratio_mark_over_groupby"] = round(
                med["mark"] / med["groupby"], 3)
            r["ratio_e2e_mark_over_two_stage"] = round(
                med["e2e_mark"] / med["e2e_two_stage"], 3)
            res.append(r)
            print(json.dumps(r), flush=True)
            with open(out, "w") as f:
                json.dump(res, f, indent=1)
            del page, g, x
            torch.cuda.empty_cache()
    return 0 if all(r["exact"] for r in res) else 1


if __name__ == "__main__":
    sys.exit(main())
