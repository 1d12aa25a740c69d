#!/usr/bin/env python3
"""What pg_plan_groupby.sql_nulls = 1 costs GROUPBY_MULTI's add_input.

Per shape (--rows log2 row counts x --groups log2 distinct keys): one I64
key, one I64 value, the aggregates SUM_I64 + MIN + COUNT, all columns
device-resident.  Four configurations on the same keys and values:

  legacy        sql_nulls = 0, no masks
  sql_clean     sql_nulls = 1, no masks on the page
  sql_nulls5    sql_nulls = 1, 5 % nulls on the key and on the value
  legacy_skew5  sql_nulls = 0, no masks, the keys of sql_nulls5's null rows
                replaced by one extra key value: the same groups, so the
                same 5 % of all rows landing on one slot, without any null
                handling

Each is verified first (against torch on the device: the null group, the
per-group sums, minima and counts), then add_input is timed with a device
synchronise around it in interleaved rounds after a warm-up round; create
and finish stay outside the clock.  Reports the medians and the ratios
sql_clean / legacy, sql_nulls5 / legacy and sql_nulls5 / legacy_skew5 (which
takes the one hot group out of the comparison).  Prints one JSON line per
shape and writes them all to --out."""
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


def plan(groups, sql_nulls):
    return pl.group_by([0], [pl.sum_i64(pl.ident(1)),
                             pl.agg_min(pl.ident(1)), pl.count()],
                       groups + 16, sql_nulls=sql_nulls)


def d2h(ptr, n, dt):
    a = np.empty(n, dt)
    if n and ptr:
        L = P.lib()
        L.check(L.c.pg_memcpy_d2h(a.ctypes.data, ptr, a.nbytes), "d2h")
    return a


def run(groups, sql_nulls, page, read=None):
    """add_input inside the clock; returns ms."""
    with P.Scope() as s:
        op = s.op(P.OP_GROUPBY_MULTI, plan(groups, sql_nulls))
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        op.add_input(page)
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        if read is not None:
            op.finish()
            read(op.get_output_raw())
    return ms


def read_groups(raw):
    n = raw.n_rows
    cols = [d2h(raw.cols[i].data, n, np.int64) for i in range(5)]
    masks = [d2h(raw.cols[i].null_mask, n, np.uint8)
             if raw.cols[i].null_mask else None for i in range(5)]
    return cols, masks


def expected(key, val, kmask, vmask, groups):
    """Per key 0..groups-1, plus the null group at index `groups`: sum,
    min (INT64_MAX where no input), count(*), and inputs received."""
    n = key.numel()
    gid = key if kmask is None else torch.where(kmask.bool(),
                                                torch.full_like(key, groups),
                                                key)
    live = torch.ones(n, dtype=torch.bool, device=key.device) \
        if vmask is None else ~vmask.bool()
    zero = torch.zeros(groups + 1, dtype=torch.int64, device=key.device)
    s = zero.clone().scatter_add_(0, gid, torch.where(live, val, 0))
    big = torch.iinfo(torch.int64).max
    mn = torch.full_like(zero, big).scatter_reduce_(
        0, gid, torch.where(live, val, big), "amin")
    cnt = zero.clone().scatter_add_(0, gid, torch.ones_like(gid))
    fed = zero.clone().scatter_add_(0, gid, live.to(torch.int64))
    return [t.cpu().numpy() for t in (s, mn, cnt, fed)]


def verify(groups, sql_nulls, page, key, val, kmask, vmask):
    """key holds values 0..groups (the last one only in legacy_skew5)."""
    got = {}
    run(groups, sql_nulls, page, lambda raw: got.update(r=read_groups(raw)))
    (k, s, mn, cnt, rows), masks = got["r"]
    es, emn, ecnt, efed = expected(key, val, kmask, vmask, groups)
    if not sql_nulls:
        if any(m is not None for m in masks):
            return False
        o = np.argsort(k)
        live = ecnt > 0
        return bool(np.array_equal(k[o], np.flatnonzero(live))
                    and np.array_equal(s[o], es[live])
                    and np.array_equal(mn[o], emn[live])
                    and np.array_equal(cnt[o], ecnt[live])
                    and np.array_equal(rows[o], ecnt[live]))
    if [m is not None for m in masks] != [True, True, True, False, False]:
        return False
    gid = np.where(masks[0] == 1, groups, k)
    o = np.argsort(gid)
    live = ecnt > 0
    null = (efed[live] == 0).astype(np.uint8)
    return bool(np.array_equal(gid[o], np.flatnonzero(live))
                and not k[masks[0] == 1].any()
                and np.array_equal(masks[1][o], null)
                and np.array_equal(masks[2][o], null)
                and np.array_equal(s[o], np.where(null, 0, es[live]))
                and np.array_equal(mn[o], np.where(null, 0, emn[live]))
                and np.array_equal(cnt[o], ecnt[live])
                and np.array_equal(rows[o], ecnt[live]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", default="24,26", help="log2 row counts")
    ap.add_argument("--groups", default="10,22", help="log2 distinct keys")
    ap.add_argument("--out", default="profiles/groupby_nulls.json")
    args = ap.parse_args()
    out = pathlib.Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    res = []
    for lg in (int(x) for x in args.rows.split(",")):
        for lgg in (int(x) for x in args.groups.split(",")):
            n, groups = 1 << lg, 1 << lgg
            g = torch.Generator(device="cuda").manual_seed(lg * 131 + lgg)
            key = torch.randint(0, groups, (n,), dtype=torch.int64,
                                device="cuda", generator=g)
            val = torch.randint(-1000, 1000, (n,), dtype=torch.int64,
                                device="cuda", generator=g)
            kmask = (torch.rand(n, device="cuda", generator=g) < 0.05) \
                .to(torch.uint8)
            vmask = (torch.rand(n, device="cuda", generator=g) < 0.05) \
                .to(torch.uint8)
            torch.cuda.synchronize()
            clean = P.Page({"k": key, "v": val})
            nulls = P.Page({"k": key, "v": val},
                           nulls={"k": kmask, "v": vmask})
            skey = torch.where(kmask.bool(), torch.full_like(key, groups),
                               key)
            skew = P.Page({"k": skey, "v": val})
            cfgs = [("legacy", 0, clean, key, None, None),
                    ("sql_clean", 1, clean, key, None, None),
                    ("sql_nulls5", 1, nulls, key, kmask, vmask),
                    ("legacy_skew5", 0, skew, skey, None, None)]
            exact = all(verify(groups, sq, pg, k, val, km, vm)
                        for _, sq, pg, k, km, vm in cfgs)
            times = {name: [] for name, *_ in cfgs}
            for _ in range(args.reps + 1):       # the first is a warm-up
                for name, sq, pg, *_ in cfgs:
                    times[name].append(run(groups, sq, pg))
            med = {k: statistics.median(v[1:]) for k, v in times.items()}
            r = {"rows": n, "groups": groups, "exact": exact,
                 "aggs": "sum_i64+min+count"}
            for k, v in times.items():
                r[k + "_add_input_ms"] = [round(t, 3) for t in v[1:]]
                r[k + "_median_ms"] = round(med[k], 3)
            r["ratio_sql_clean_over_legacy"] = round(
                med["sql_clean"] / med["legacy"], 3)
            r["ratio_sql_nulls5_over_legacy"] = round(
                med["sql_nulls5"] / med["legacy"], 3)
            r["ratio_sql_nulls5_over_legacy_skew5"] = round(
                med["sql_nulls5"] / med["legacy_skew5"], 3)
            res.append(r)
            print(json.dumps(r), flush=True)
            with open(out, "w") as f:
                json.dump(res, f, indent=1)
            del clean, nulls, skew, key, skey, val, kmask, vmask
            torch.cuda.empty_cache()
    return 0 if all(r["exact"] for r in res) else 1


if __name__ == "__main__":
    sys.exit(main())
