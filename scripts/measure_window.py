#!/usr/bin/env python3
"""WINDOW's finish vs ORDER_BY's finish on the same keys and emit columns
(the sort the window operator starts with) vs a plain torch composition:
two stable torch.sort, boundary compares, cummax / cummin / cumsum with
segment reset.

Per shape: one I64 partition key with about --parts distinct values, one
I32 order key, the functions row_number, rank, a RANGE running sum and
lag.  The three are verified equal first, then timed in interleaved
rounds after a warm-up round, a device synchronise around each.  Reports
(WINDOW - ORDER_BY) / ORDER_BY — the post-sort phases as a share of the
sort — and WINDOW / torch.  Prints one JSON line per case and writes them
all to --out."""
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

# columns of the page: 0 partition key (i64), 1 order key (i32), 2 value
# (i64), 3 row id (i64)
KEYS = [pl.asc(0), pl.asc(1)]
EMIT = [3]

# bytes per row of the post-sort phases, counted from the kernels (unique
# bytes; a row's predecessor keys come from the cache):
#   flags   4 id + 12 keys gathered + 1 flag out                    = 17
#   bounds  2 flag reads (forward, backward) + 5 x 4 out            = 22
#   sum     reduce 1 flag + 4 id + 8 value; rescan the same + 20 out = 46
#   emit    row_number 4 + 8; rank 8 + 8; sum 4 + 20 gathered + 9;
#           lag 4 + 4 id + 8 value gathered + 9                     = 86
POST_SORT_BYTES_PER_ROW = 17 + 22 + 46 + 86


def window_plan():
    return pl.window(KEYS[:1], KEYS[1:], EMIT,
                     [pl.row_number(), pl.rank(), pl.win_sum(2), pl.lag(2)])


def d2h(ptr, n, dt):
    a = np.empty(n, dt)
    if n:
        L = P.lib()
        L.check(L.c.pg_memcpy_d2h(a.ctypes.data, ptr, a.nbytes), "d2h")
    return a


def finish_ms(kind, plan, page, read=None):
    """add_input outside the clock, finish inside it."""
    with P.Scope() as s:
        op = s.op(kind, plan)
        op.add_input(page)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        op.finish()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3
        if read is not None:
            read(op.get_output_raw())
    return ms


def run_torch(pkey, okey, val):
    n = pkey.numel()
    i1 = torch.sort(okey, stable=True).indices
    i2 = torch.sort(pkey[i1], stable=True).indices
    idx = i1[i2]
    p, o, v = pkey[idx], okey[idx], val[idx]
    pos = torch.arange(n, device=p.device)
    first = torch.ones(1, dtype=torch.bool, device=p.device)
    part_head = torch.cat([first, p[1:] != p[:-1]])
    peer_head = part_head | torch.cat([first, o[1:] != o[:-1]])
    zero = torch.zeros_like(pos)
    part_start = torch.cummax(torch.where(part_head, pos, zero), 0).values
    peer_start = torch.cummax(torch.where(peer_head, pos, zero), 0).values
    # the next peer head after each row, by a reversed cummin
    nxt = torch.where(peer_head, pos, torch.full_like(pos, n))
    nxt = torch.cat([nxt[1:], torch.full_like(pos[:1], n)])
    peer_end = torch.flip(torch.cummin(torch.flip(nxt, [0]), 0).values,
                          [0]) - 1
    cs = torch.cumsum(v, 0)
    rows_sum = cs - (cs[part_start] - v[part_start])
    lag = torch.where(part_head, zero, torch.cat([zero[:1], v[:-1]]))
    return (idx, pos - part_start + 1, peer_start - part_start + 1,
            rows_sum[peer_end], lag, part_head.to(torch.uint8))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--rows", default="24,26", help="log2 row counts")
    ap.add_argument("--parts", default="100,1000000")
    ap.add_argument("--out", default="profiles/window.json")
    args = ap.parse_args()
    out = pathlib.Path(args.out)
    out.parent.mkdir(parents=True, exist_ok=True)
    res = []
    for lg in (int(x) for x in args.rows.split(",")):
        for parts in (int(x) for x in args.parts.split(",")):
            n = 1 << lg
            g = torch.Generator(device="cuda").manual_seed(lg * 131 + parts)
            pkey = torch.randint(-parts // 2, parts - parts // 2, (n,),
                                 dtype=torch.int64, device="cuda",
                                 generator=g)
            okey = torch.randint(0, 2557, (n,), dtype=torch.int32,
                                 device="cuda", generator=g)   # 7 years
            val = torch.randint(0, 1000, (n,), dtype=torch.int64,
                                device="cuda", generator=g)
            rowid = torch.arange(n, dtype=torch.int64, device="cuda")
            torch.cuda.synchronize()
            page = P.Page({"p": pkey, "o": okey, "v": val, "r": rowid})
            wplan, oplan = window_plan(), pl.order_by(KEYS, EMIT)

            # ---- equality at the timed size ----
            got = {}

            def read_window(raw):
                got["w"] = [d2h(raw.cols[i].data, n, np.int64)
                            for i in range(5)]
                got["w_masks"] = [bool(raw.cols[i].null_mask)
                                  for i in range(5)]
                got["sum_null"] = d2h(raw.cols[3].null_mask, n, np.uint8)
                got["lag_null"] = d2h(raw.cols[4].null_mask, n, np.uint8)

            def read_order_by(raw):
                got["o"] = d2h(raw.cols[0].data, n, np.int64)

            finish_ms(P.OP_WINDOW, wplan, page, read_window)
            finish_ms(P.OP_ORDER_BY, oplan, page, read_order_by)
            ref = [t.cpu().numpy() for t in run_torch(pkey, okey, val)]
            torch.cuda.synchronize()
            same = bool(
                all(np.array_equal(a, b) for a, b in zip(got["w"], ref[:5]))
                and np.array_equal(got["o"], ref[0])
                and got["w_masks"] == [False, False, False, True, True]
                and not got["sum_null"].any()
                and np.array_equal(got["lag_null"], ref[5]))
            n_parts = int(ref[5].sum())
            got.clear()
            del ref

            # ---- interleaved rounds, the first one a warm-up ----
            t_w, t_o, t_t = [], [], []
            for _ in range(args.reps + 1):
                t_w.append(finish_ms(P.OP_WINDOW, wplan, page))
                t_o.append(finish_ms(P.OP_ORDER_BY, oplan, page))
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                r = run_torch(pkey, okey, val)
                torch.cuda.synchronize()
                t_t.append((time.perf_counter() - t0) * 1e3)
                del r
            t_w, t_o, t_t = t_w[1:], t_o[1:], t_t[1:]
            m_w, m_o, m_t = (statistics.median(t) for t in (t_w, t_o, t_t))
            post = m_w - m_o
            r = {"rows": n, "partitions": n_parts, "exact": same,
                 "window_finish_ms": [round(t, 3) for t in t_w],
                 "order_by_finish_ms": [round(t, 3) for t in t_o],
                 "torch_ms": [round(t, 3) for t in t_t],
                 "window_median_ms": round(m_w, 3),
                 "order_by_median_ms": round(m_o, 3),
                 "torch_median_ms": round(m_t, 3),
                 "post_sort_ms": round(post, 3),
                 "post_sort_share_of_order_by": round(post / m_o, 3),
                 "ratio_window_over_torch": round(m_w / m_t, 3),
                 "post_sort_bytes_per_row_computed": POST_SORT_BYTES_PER_ROW,
                 "post_sort_effective_GBps": round(
                     POST_SORT_BYTES_PER_ROW * n / post / 1e6, 1)
                 if post > 0 else None}
            res.append(r)
            print(json.dumps(r), flush=True)
            with open(out, "w") as f:
                json.dump(res, f, indent=1)
            del page, pkey, okey, val, rowid
            torch.cuda.empty_cache()
    return 0 if all(r["exact"] for r in res) else 1


if __name__ == "__main__":
    sys.exit(main())
