#!/usr/bin/env python3
"""ORDER_BY over one device page vs torch.sort(stable=True) + gather.
Medians of --reps runs after a warm-up, device synchronise around each.
Prints one JSON line per case and writes them all to --out (default
bench_out/sort.json)."""
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


def d2h(ptr, n, dt):
    a = np.empty(n, dt)
    L = P.lib()
    L.check(L.c.pg_memcpy_d2h(a.ctypes.data, ptr, a.nbytes), "d2h")
    return a


def run_order_by(page, check=False):
    with P.Scope() as s:
        ob = s.run(P.OP_ORDER_BY, pl.order_by([pl.asc(0)], [0, 1]), page)
        raw = ob.get_output_raw()
        if check:
            n = raw.n_rows
            kdt = {1: np.int32, 2: np.int64}[raw.cols[0].tag]
            return d2h(raw.cols[0].data, n, kdt), \
                d2h(raw.cols[1].data, n, np.int64)


def run_torch(key, pay):
    vals, idx = torch.sort(key, stable=True)
    out = pay[idx]
    return vals, out


def timed(fn, reps):
    fn()  # warm-up
    ts = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--cases", default="i64_24,i64_27,date_27")
    ap.add_argument("--out", default="bench_out/sort.json")
    args = ap.parse_args()
    out = pathlib.Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    res = []
    for case in args.cases.split(","):
        kind, lg = case.split("_")
        n = 1 << int(lg)
        g = torch.Generator(device="cuda").manual_seed(1)
        if kind == "i64":
            key = torch.randint(-2**63, 2**63 - 1, (n,), dtype=torch.int64,
                                device="cuda", generator=g)
            passes, kw = 8, 8
        else:  # l_shipdate's range, 1992-01-02 .. 1998-12-01 in epoch days
            key = torch.randint(8036, 10562, (n,), dtype=torch.int32,
                                device="cuda", generator=g)
            passes, kw = 2, 4
        pay = torch.arange(n, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        page = P.Page({"k": key, "p": pay})
        # exactness at the timed size, against the yardstick's own output
        gk, gp = run_order_by(page, check=True)
        tv, tp = run_torch(key, pay)
        torch.cuda.synchronize()
        same = bool(np.array_equal(gk, tv.cpu().numpy()) and
                    np.array_equal(gp, tp.cpu().numpy()))
        del gk, gp, tv, tp
        t_ob = timed(lambda: run_order_by(page), args.reps)
        t_th = timed(lambda: run_torch(key, pay), args.reps)
        # traffic from the code, bytes per row: input copies (2 x key +
        # payload), encode (key in, 8 key + 4 id out), digits (8 in),
        # per pass count (8 in) + scatter (12 in, 12 out), gather (4 id
        # in, key + payload in and out)
        per_row = 2 * (kw + 8) + (kw + 12) + 8 + passes * 32 \
            + 4 + 2 * (kw + 8)
        m_ob, m_th = statistics.median(t_ob), statistics.median(t_th)
        r = {"case": case, "rows": n, "passes": passes, "exact": same,
             "order_by_ms": [round(t, 3) for t in t_ob],
             "torch_ms": [round(t, 3) for t in t_th],
             "order_by_median_ms": round(m_ob, 3),
             "torch_median_ms": round(m_th, 3),
             "ratio_order_by_over_torch": round(m_ob / m_th, 3),
             "bytes_per_row": per_row,
             "effective_GBps": round(per_row * n / m_ob / 1e6, 1)}
        res.append(r)
        print(json.dumps(r), flush=True)
        with open(out, "w") as f:
            json.dump(res, f, indent=1)
        del page, key, pay
        torch.cuda.empty_cache()
    return 0 if all(r["exact"] for r in res) else 1


if __name__ == "__main__":
    sys.exit(main())
