#!/usr/bin/env python3
"""bench.py — driver-contract benchmark for the MI355X-native Presto
hot-path library.

A "step" is one pass of the hot path over one batch of synthetic input:
  q1: the full TPC-H Q1 pipeline (fused scan+filter+group-by+aggregate +
      final reduce) over the SF100 lineitem columns resident in HBM —
      BASELINE.json configs[1].
  q3: the full Q3 pipeline (customer set build, orders build with fused
      filter+semijoin, lineitem probe with fused grouped sum, TopN 10) —
      BASELINE.json configs[2].
  q5: the 6-way join (customer/orders/lineitem/supplier/nation/region,
      local-supplier condition, per-nation revenue).

The default invocation (--query all) does only what the headline figure
needs: it measures q1 and q3 and prints ONE JSON line, the combined line for
the BASELINE metric, which names "TPC-H SF100 Q1 & Q3": the combined value is
lineitem rows/s over one Q1 pass + one Q3 pass per step.

--full adds everything else: the q5 leg, the CPU-oracle baselines, one JSON
line per query ahead of the combined line, and (with --verify) the full-size
comparison against the CPU oracle.

--dump-outputs DIR writes what the last timed step of each query returned,
one DIR/<query>.<column>.npy per output column (float32/float64), so that two
builds can be compared output for output: inputs depend on the arguments only.

Inputs are synthetic TPC-H columns from the dbgen restatement in
oracle/tpchgen.c (golden-pinned; generation is test/bench input
infrastructure and happens OUTSIDE the timed region).  Data is resident in
HBM when the timed region starts.

Multi-GPU (--gpus N via torch.distributed.run): weak scaling — each rank
holds its own SF-sized shard; Q1 ends with an all_gather of the tiny group
partials combined in rank order (the partial->final Step split of
HashAggregationOperator.java:72); Q3/Q5 exchange by orderkey hash over
RCCL all_to_all (presto_amd/dist.py) before local build/probe.

cpu_baseline (--full only): the CPU oracle (oracle/liboracle.so, kind "port")
timed on the host cores over a bounded sample — reported baseline only, never
the measured value.
"""
import argparse
import ctypes as C
import json
import os
import pathlib
import sys
import time

import numpy as np

REPO = pathlib.Path(__file__).resolve().parent
sys.path.insert(0, str(REPO))

Q1_WORKLOAD = ("TPC-H SF{sf} Q1 on {n}xMI355X - scan/filter/hash-aggregate "
               "kernels, lineitem columns resident in HBM")
Q3_WORKLOAD = ("TPC-H SF{sf} Q3 on {n}xMI355X - 3-way hash join "
               "(HashBuilder+LookupJoin) + order-by/limit")
Q5_WORKLOAD = ("TPC-H SF{sf} Q5 on {n}xMI355X - 6-way join "
               "(customer/orders/lineitem/supplier/nation/region), "
               "local-supplier condition, per-nation revenue")
Q13_WORKLOAD = ("TPC-H SF{sf} Q13 on {n}xMI355X - varchar NOT LIKE scan + "
                "outer-join count distribution")

# Q1 algorithmic bytes/row: 4 f64 money cols +
# dict-u8 returnflag/linestatus + date32 = 38 B
Q1_BYTES_PER_ROW = 38
# Q3 probe kernel: lineitem orderkey 8 + eprice 8 + discount 8 +
# shipdate 4 = 28 B/row algorithmic scan
Q3_BYTES_PER_ROW = 28
# Q5 probe1 emit sequence: orderkey 8 + suppkey 8 + eprice 8 + discount 8
Q5_BYTES_PER_ROW = 32
HBM_PEAK = 8.0e12  # B/s, MI355X_MICROARCH.md chip parameters (spec)


def log(msg):
    print(msg, file=sys.stderr, flush=True)


def load_oracle():
    import subprocess
    so = REPO / "oracle" / "liboracle.so"
    if not so.exists():
        subprocess.run(["make", "-C", str(REPO / "oracle"), "liboracle.so"],
                       check=True)
    from tests.oracle_binding import OracleLib
    return OracleLib(str(so))


def gen_lineitem_device(orc, sf, device, want_orderkey=False,
                        want_suppkey=False,
                        chunk_orders=4_000_000, ord_start=0, ord_count=None):
    """Generate lineitem columns for orders [ord_start, ord_start+ord_count)
    of logical scale sf, chunkwise on host, uploaded to device tensors.
    Returns dict of torch tensors."""
    import torch
    n_all = orc.lib.tpch_orders_count(C.c_double(sf))
    if ord_count is None:
        ord_count = n_all - ord_start
    n = (orc.lib.tpch_lineitem_offset(C.c_double(sf),
                                      C.c_int64(ord_start + ord_count)) -
         orc.lib.tpch_lineitem_offset(C.c_double(sf), C.c_int64(ord_start)))
    cols = {
        "quantity": torch.empty(n, dtype=torch.float64, device=device),
        "extendedprice": torch.empty(n, dtype=torch.float64, device=device),
        "discount": torch.empty(n, dtype=torch.float64, device=device),
        "tax": torch.empty(n, dtype=torch.float64, device=device),
        "shipdate": torch.empty(n, dtype=torch.int32, device=device),
        "returnflag": torch.empty(n, dtype=torch.uint8, device=device),
        "linestatus": torch.empty(n, dtype=torch.uint8, device=device),
    }
    if want_orderkey:
        cols["orderkey"] = torch.empty(n, dtype=torch.int64, device=device)
    if want_suppkey:
        cols["suppkey"] = torch.empty(n, dtype=torch.int64, device=device)
    maxrows = chunk_orders * 7
    # pinned host staging: the generator writes straight into pinned
    # memory, then one async h2d copy per column per chunk
    buf = {k: torch.empty(maxrows, dtype=v.dtype, pin_memory=True)
           for k, v in cols.items()}
    ptr = {k: C.c_void_p(t.data_ptr()) for k, t in buf.items()}
    off = 0
    o = ord_start
    end = ord_start + ord_count
    t0 = time.time()
    while o < end:
        cnt = min(chunk_orders, end - o)
        if want_suppkey:
            w = orc.lib.tpch_gen_lineitem2(
                C.c_double(sf), C.c_int64(o), C.c_int64(cnt),
                ptr["orderkey"], ptr["quantity"], ptr["extendedprice"],
                ptr["discount"], ptr["tax"], ptr["shipdate"],
                ptr["returnflag"], ptr["linestatus"], ptr["suppkey"])
        else:
            w = orc.lib.tpch_gen_lineitem(
                C.c_double(sf), C.c_int64(o), C.c_int64(cnt),
                ptr["orderkey"] if want_orderkey else None,
                ptr["quantity"], ptr["extendedprice"],
                ptr["discount"], ptr["tax"],
                ptr["shipdate"], ptr["returnflag"], ptr["linestatus"])
        for k, t in cols.items():
            t[off:off + w].copy_(buf[k][:w], non_blocking=True)
        torch.cuda.synchronize()
        off += w
        o += cnt
    assert off == n
    log(f"generated+uploaded lineitem sf={sf}: {n} rows in "
        f"{time.time() - t0:.1f}s")
    return cols, n


def gen_orders_customer_device(orc, sf, device, rank=0, world=1):
    """Rank shard of orders + customer at logical scale sf."""
    import torch
    n_all = orc.lib.tpch_orders_count(C.c_double(sf))
    o0, o1 = n_all * rank // world, n_all * (rank + 1) // world
    n_ord = o1 - o0
    nc_all = orc.lib.tpch_customer_count(C.c_double(sf))
    c0, c1 = nc_all * rank // world, nc_all * (rank + 1) // world
    n_cust = c1 - c0
    ok = np.empty(n_ord, np.int64)
    ck = np.empty(n_ord, np.int64)
    od = np.empty(n_ord, np.int32)
    orc.lib.tpch_gen_orders(C.c_double(sf), C.c_int64(o0), C.c_int64(n_ord),
                            C.c_void_p(ok.ctypes.data),
                            C.c_void_p(ck.ctypes.data),
                            C.c_void_p(od.ctypes.data), None)
    cck = np.empty(n_cust, np.int64)
    seg = np.empty(n_cust, np.uint8)
    orc.lib.tpch_gen_customer(C.c_double(sf), C.c_int64(c0),
                              C.c_int64(n_cust),
                              C.c_void_p(cck.ctypes.data),
                              C.c_void_p(seg.ctypes.data))
    t = lambda a: __import__("torch").from_numpy(a).to(device)
    return (dict(orderkey=t(ok), custkey=t(ck), orderdate=t(od)),
            dict(custkey=t(cck), mktseg=t(seg)))


def cpu_baseline_q1(orc, target_secs=10.0):
    """Time the oracle's Q1 (OpenMP over all host cores) on a bounded
    sample; returns (rows_per_sec, n_rows_sample)."""
    sf_sample = 4.0
    li = orc.gen_lineitem(sf_sample)
    n = len(li["quantity"])
    reps = 1
    t0 = time.time()
    orc.q1(li)
    dt = time.time() - t0
    while dt * reps < target_secs / 2 and reps < 64:
        reps *= 2
    t0 = time.time()
    for _ in range(reps):
        orc.q1(li)
    dt = (time.time() - t0) / reps
    return n / dt, n


def cpu_baseline_q5(orc, target_secs=10.0):
    sf_sample = 2.0
    li = orc.gen_lineitem2(sf_sample)
    orders = orc.gen_orders(sf_sample)
    cust = orc.gen_customer2(sf_sample)
    supp = orc.gen_supplier(sf_sample)
    n = len(li["quantity"])
    t0 = time.time()
    orc.q5(cust, orders, li, supp)
    dt = time.time() - t0
    reps = min(max(1, int(target_secs / 2 / max(dt, 0.05))), 16)
    t0 = time.time()
    for _ in range(reps):
        orc.q5(cust, orders, li, supp)
    dt = (time.time() - t0) / reps
    return n / dt, n


def cpu_baseline_q3(orc, target_secs=10.0):
    sf_sample = 2.0
    li = orc.gen_lineitem(sf_sample)
    orders = orc.gen_orders(sf_sample)
    cust = orc.gen_customer(sf_sample)
    n = len(li["quantity"])
    t0 = time.time()
    orc.q3(cust, orders, li)
    dt = time.time() - t0
    reps = max(1, int(target_secs / 2 / max(dt, 0.05)))
    reps = min(reps, 16)
    t0 = time.time()
    for _ in range(reps):
        orc.q3(cust, orders, li)
    dt = (time.time() - t0) / reps
    return n / dt, n


class Bench:
    """Shared state for the per-query benchmark legs."""

    def __init__(self, args):
        self.args = args
        world = int(os.environ.get("WORLD_SIZE", "1"))
        if world > 1 and "OMP_NUM_THREADS" not in os.environ:
            os.environ["OMP_NUM_THREADS"] = str(
                max(1, (os.cpu_count() or 8) // world))
        import torch
        self.torch = torch
        self.world = world
        self.rank = int(os.environ.get("RANK", "0"))
        self.local_rank = int(os.environ.get("LOCAL_RANK", "0"))
        self.n_gpus = max(world, args.gpus if world == 1 else world)
        if world > 1:
            import torch.distributed as dist
            torch.cuda.set_device(self.local_rank)
            dist.init_process_group("nccl")
        self.device = torch.device("cuda", self.local_rank)
        import presto_amd
        self.P = presto_amd
        self.orc = load_oracle()
        self.lib = presto_amd.engine.lib()
        self.lib.c.pg_last_hot_kernel_ms.restype = C.c_double
        self.lib.c.pg_hot_max_ms.restype = C.c_double
        # weak scaling: per-rank work fixed at args.sf
        self.sf_total = args.sf * world
        n_ord_all = self.orc.lib.tpch_orders_count(C.c_double(self.sf_total))
        self.o0 = n_ord_all * self.rank // world
        self.o1 = n_ord_all * (self.rank + 1) // world
        self.li_cols = None
        self.li_n = 0
        self.ocols = self.ccols = None

    def barrier_sync(self):
        self.torch.cuda.synchronize()
        if self.world > 1:
            import torch.distributed as dist
            dist.barrier()
            self.torch.cuda.synchronize()

    def lineitem(self, queries):
        """Generate the lineitem shard once, as the column superset the
        requested queries need."""
        if self.li_cols is None:
            want_ok = any(q in queries for q in ("q3", "q5"))
            want_sk = "q5" in queries
            self.li_cols, self.li_n = gen_lineitem_device(
                self.orc, self.sf_total, self.device,
                want_orderkey=want_ok, want_suppkey=want_sk,
                ord_start=self.o0, ord_count=self.o1 - self.o0)
        return self.li_cols, self.li_n

    def orders_customer(self):
        if self.ocols is None:
            self.ocols, self.ccols = gen_orders_customer_device(
                self.orc, self.sf_total, self.device, self.rank, self.world)
        return self.ocols, self.ccols

    def time_steps(self, step):
        a = self.args
        for _ in range(a.warmup):
            step()
        self.lib.c.pg_hot_reset()
        if self.world > 1:
            from presto_amd import dist as pdist
            pdist.exchange_bytes_reset()
        self.barrier_sync()
        out = None
        t0 = time.time()
        for _ in range(a.steps):
            out = step()
        self.barrier_sync()
        elapsed = time.time() - t0
        if self.world > 1:
            from presto_amd import dist as pdist
            log(f"rank {self.rank}: RCCL all_to_all xGMI-crossing volume "
                f"{pdist.EXCHANGE_BYTES / a.steps / 1e9:.3f} GB/step "
                f"(SURVEY.md §8d config-4 scale estimate: ~10.8 GB total "
                f"at SF300 Q3 across 8 ranks)")
        if self.world > 1:
            import torch.distributed as dist
            e = self.torch.tensor([elapsed], device=self.device)
            dist.all_reduce(e, op=dist.ReduceOp.MAX)
            elapsed = float(e.item())
        hot_ms = float(self.lib.c.pg_hot_max_ms())
        return elapsed, hot_ms, out

    def total_rows(self, n_local):
        if self.world > 1:
            import torch.distributed as dist
            tr = self.torch.tensor([n_local], dtype=self.torch.int64,
                                   device=self.device)
            dist.all_reduce(tr)
            return int(tr.item())
        return n_local * self.n_gpus


def setup_q1(B):
    cols, n_rows = B.lineitem(B.args.queries)
    P, pipelines = B.P, B.P.pipelines
    page = P.Page(cols, n_rows=n_rows)
    plan = pipelines.q1_plan(page, B.args.mode)
    names = (pipelines.Q1_F64_NAMES if B.args.mode == "f64"
             else pipelines.Q1_DEC_NAMES)

    def step():
        op = P.Operator(P.OP_HASH_AGG_SMALL, plan)
        op.add_input(page)
        op.finish()
        out = op.get_output(names)
        op.destroy()
        if B.world > 1:
            # partial->final: gather the tiny per-rank group partials
            # (fixed 6x8 f64-bits buffer, zero-padded) and combine on
            # every rank in rank order — the partial/final Step split
            # of HashAggregationOperator.java:72
            import torch.distributed as dist
            buf = B.torch.zeros(6 * 8, dtype=B.torch.float64,
                                device=B.device)
            vals = [k for k in out
                    if k not in ("returnflag", "linestatus")][:8]
            ng = len(out["returnflag"])
            for c, k in enumerate(vals):
                buf[c * 6:c * 6 + ng] = B.torch.from_numpy(
                    np.ascontiguousarray(out[k]).view(np.float64)
                ).to(B.device)
            allp = [B.torch.empty_like(buf) for _ in range(B.world)]
            dist.all_gather(allp, buf)
        return out

    return dict(step=step, n_rows=n_rows,
                workload=Q1_WORKLOAD, bytes_per_row=Q1_BYTES_PER_ROW,
                baseline=cpu_baseline_q1)


def setup_q3(B):
    cols, n_rows = B.lineitem(B.args.queries)
    P, pipelines = B.P, B.P.pipelines
    li_page = P.Page(cols, n_rows=n_rows)
    ocols, ccols = B.orders_customer()
    ord_page = P.Page(ocols)
    cust_page = P.Page(ccols)
    okb = pipelines.okey_max(
        B.orc.lib.tpch_orders_count(C.c_double(B.sf_total)))

    def step():
        if B.world > 1:
            from presto_amd.dist import q3_distributed
            return q3_distributed(cust_page, ord_page, li_page, B.world,
                                  B.rank, B.device, mode="dec",
                                  okey_bound=okb)
        return pipelines.q3(cust_page, ord_page, li_page, mode="dec")

    return dict(step=step, n_rows=n_rows,
                workload=Q3_WORKLOAD, bytes_per_row=Q3_BYTES_PER_ROW,
                baseline=cpu_baseline_q3,
                verify_pages=(cols, ocols, ccols))


def setup_q5(B):
    import torch
    cols, n_rows = B.lineitem(B.args.queries)
    P, pipelines = B.P, B.P.pipelines
    orc, sf_total, rank, world = B.orc, B.sf_total, B.rank, B.world
    n_cust_all = orc.lib.tpch_customer_count(C.c_double(sf_total))
    c0 = n_cust_all * rank // world
    c1 = n_cust_all * (rank + 1) // world
    cck = np.empty(c1 - c0, np.int64)
    cnat = np.empty(c1 - c0, np.uint8)
    orc.lib.tpch_gen_customer2(C.c_double(sf_total), C.c_int64(c0),
                               C.c_int64(c1 - c0),
                               C.c_void_p(cck.ctypes.data), None,
                               C.c_void_p(cnat.ctypes.data))
    n_supp_all = orc.lib.tpch_supplier_count(C.c_double(sf_total))
    s0 = n_supp_all * rank // world
    s1 = n_supp_all * (rank + 1) // world
    ssk = np.empty(s1 - s0, np.int64)
    snat = np.empty(s1 - s0, np.uint8)
    orc.lib.tpch_gen_supplier(C.c_double(sf_total), C.c_int64(s0),
                              C.c_int64(s1 - s0),
                              C.c_void_p(ssk.ctypes.data),
                              C.c_void_p(snat.ctypes.data))
    ook = np.empty(B.o1 - B.o0, np.int64)
    ock = np.empty(B.o1 - B.o0, np.int64)
    ood = np.empty(B.o1 - B.o0, np.int32)
    orc.lib.tpch_gen_orders(C.c_double(sf_total), C.c_int64(B.o0),
                            C.c_int64(B.o1 - B.o0),
                            C.c_void_p(ook.ctypes.data),
                            C.c_void_p(ock.ctypes.data),
                            C.c_void_p(ood.ctypes.data), None)
    t = lambda a: torch.from_numpy(a).to(B.device)
    cust_page = P.Page({"custkey": t(cck), "nationkey": t(cnat)})
    cust_page.n_total = n_cust_all
    ord_page = P.Page({"orderkey": t(ook), "custkey": t(ock),
                       "orderdate": t(ood)})
    supp_page = P.Page({"suppkey": t(ssk), "nationkey": t(snat)})
    supp_page.n_total = n_supp_all
    li5 = P.Page({k: cols[k] for k in ("orderkey", "suppkey",
                                      "extendedprice", "discount")})

    def step():
        if B.world > 1:
            from presto_amd.dist import q5_distributed
            return q5_distributed(cust_page, ord_page, supp_page, li5,
                                  B.world, B.rank, B.device,
                                  okey_bound=pipelines.okey_max(
                                      B.orc.lib.tpch_orders_count(
                                          C.c_double(B.sf_total))))
        return pipelines.q5(cust_page, ord_page, supp_page, li5)

    return dict(step=step, n_rows=n_rows,
                workload=Q5_WORKLOAD, bytes_per_row=Q5_BYTES_PER_ROW,
                baseline=cpu_baseline_q5,
                verify_data=(cck, cnat, ook, ock, ood, ssk, snat, cols))


SETUPS = {"q1": setup_q1, "q3": setup_q3, "q5": setup_q5}
WORKLOADS = {"q1": Q1_WORKLOAD, "q3": Q3_WORKLOAD, "q5": Q5_WORKLOAD}


def traffic_for(query, mode, sf):
    """Measured per-launch HBM traffic from committed rocprofv3 PMC passes
    (profiles/pmc_traffic.json; see profiles/*_pmc.txt)."""
    try:
        tr = json.loads((REPO / "profiles" / "pmc_traffic.json").read_text())
        return tr.get(f"{query}:{mode}:sf{int(sf)}")
    except Exception:
        return None


DUMP_BUDGET = 64 << 20  # bytes over all files of one --dump-outputs run


def dump_outputs(outdir, outs):
    """Write the last timed step's return value of every measured query as
    outdir/<query>.<column>.npy, float32 for columns of up to 2 bytes per
    value, float64 for the rest.  An 8-byte integer column that float64
    cannot hold exactly (the low word of a 128-bit decimal sum) is also
    written as its exact 32-bit halves, <column>.hi32 (signed) and
    <column>.lo32.  A column over its share of DUMP_BUDGET is cut to a
    fixed, seeded sample of its rows."""
    outdir = pathlib.Path(outdir)
    outdir.mkdir(parents=True, exist_ok=True)
    arrays = {}
    for q, out in outs.items():
        if not isinstance(out, dict) or not out:
            raise RuntimeError(f"--dump-outputs: {q} step returned no "
                               f"columns ({type(out).__name__})")
        for name, v in out.items():
            a = np.atleast_1d(np.asarray(v))
            if a.dtype.kind not in "iufb":
                raise RuntimeError(f"--dump-outputs: {q}.{name} has "
                                   f"non-numeric dtype {a.dtype}")
            key = f"{q}.{name}"
            if a.dtype.kind in "iu" and a.dtype.itemsize == 8:
                f = a.astype(np.float64)
                exact = bool(np.all(np.abs(f) < 2.0 ** 63)) and bool(
                    np.all(f.astype(a.dtype) == a))
                if not exact:
                    bits = np.ascontiguousarray(a).view(np.int64)
                    arrays[key + ".hi32"] = (bits >> 32).astype(np.float64)
                    arrays[key + ".lo32"] = (
                        bits & 0xFFFFFFFF).astype(np.float64)
                arrays[key] = f
            elif a.dtype.itemsize <= 2:
                arrays[key] = a.astype(np.float32)
            else:
                arrays[key] = a.astype(np.float64)
    share = DUMP_BUDGET // max(len(arrays), 1) - 128  # .npy header
    for key, a in arrays.items():
        cap = share // a.dtype.itemsize
        if a.size > cap:
            idx = np.sort(np.random.default_rng(0).choice(
                a.size, size=cap, replace=False))
            a = a.reshape(-1)[idx]
        np.save(outdir / f"{key}.npy", np.ascontiguousarray(a))
    log(f"dumped {len(arrays)} output arrays to {outdir}")


def bench_query(B, q):
    args = B.args
    su = SETUPS[q](B)
    elapsed, hot_ms, last_out = B.time_steps(su["step"])
    n_rows = su["n_rows"]
    total_rows = B.total_rows(n_rows)
    ms_per_step = elapsed / args.steps * 1000.0
    value = total_rows * args.steps / elapsed
    rec = None
    if B.rank == 0:
        alg_bytes = su["bytes_per_row"] * n_rows
        achieved = (alg_bytes / (hot_ms / 1000.0) / 1e9
                    if hot_ms > 0 else None)
        mode = args.mode if q == "q1" else "dec"
        roofline = {
            "bound": "hbm",
            "achieved": achieved,
            "peak": HBM_PEAK / 1e9,
            "unit": "GB/s",
            "frac": achieved / (HBM_PEAK / 1e9) if achieved else None,
            "traffic": traffic_for(q, mode, args.sf),
        }
        cpu = None
        if args.full and not args.skip_cpu_baseline and B.n_gpus == 1:
            rps, nsamp = su["baseline"](B.orc)
            cpu = {
                "value": rps,
                "unit": "rows/s",
                "cores": os.cpu_count(),
                "kind": "port",
                "sample": (f"oracle (OpenMP, all host cores) on a "
                           f"{nsamp}-row TPC-H sample of the same workload"),
            }
        rec = {
            "metric": "tpch_lineitem_rows_per_sec",
            "value": value,
            "unit": "rows/s",
            "n_gpus": B.n_gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": ms_per_step,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "f64" if (q == "q1" and args.mode == "f64") else "i64",
            "data": ("synthetic (spec-conformant TPC-H dbgen restatement, "
                     f"SF{int(args.sf)}, golden-pinned)"),
            "config": {
                "workload": WORKLOADS[q].format(sf=int(B.sf_total),
                                                n=B.n_gpus),
                "query": q,
                "sf": args.sf,
                "rows_per_gpu": n_rows,
                "mode": mode,
            },
            "roofline": roofline,
            "cpu_baseline": cpu,
        }
    return su, rec, dict(elapsed=elapsed, hot_ms=hot_ms, n_rows=n_rows,
                         total_rows=total_rows, last_out=last_out)


def verify(B, q, su):
    """After timing, check full-size results against the CPU oracle
    (exact decimal + bitwise f64)."""
    if B.rank != 0 or B.world != 1:
        return
    orc, pipelines, P = B.orc, B.P.pipelines, B.P
    if q == "q1":
        cols, n_rows = B.li_cols, B.li_n
        li_host = {k: v.cpu().numpy() for k, v in cols.items()}
        exp = orc.q1(li_host)
        page = P.Page(cols, n_rows=n_rows)
        got_d = pipelines.q1(page, mode="dec")
        got_f = pipelines.q1(page, mode="f64")
        for i, g in enumerate(exp):
            assert got_d["count"][i] == g.count_order
            assert got_d["sum_qty_lo"][i] == g.sum_qty_units
            assert got_d["sum_base_lo"][i] == g.sum_base_cents
            assert got_d["sum_disc_price_lo"][i] == g.sum_disc_1e4
            assert got_d["sum_charge_hi"][i] == g.sum_charge_1e6_hi
            assert np.uint64(got_d["sum_charge_lo"][i].astype(
                np.uint64)) == np.uint64(g.sum_charge_1e6_lo)
            assert got_f["sum_charge"][i].view(np.int64) == np.float64(
                g.f64_sum_charge).view(np.int64)
        log(f"verify q1 sf={B.args.sf}: exact decimal + bitwise f64 OK "
            f"({len(exp)} groups, {n_rows} rows)")
    elif q == "q3":
        cols, ocols, ccols = su["verify_pages"]
        li_host = {k: v.cpu().numpy() for k, v in cols.items()}
        oc = {k: v.cpu().numpy() for k, v in ocols.items()}
        cc = {k: v.cpu().numpy() for k, v in ccols.items()}
        exp3 = orc.q3(cc, oc, li_host)
        got3 = su["step"]()
        for i, r in enumerate(exp3):
            assert got3["orderkey"][i] == r.orderkey
            assert got3["revenue_1e4"][i] == r.revenue_1e4
            assert got3["orderdate"][i] == r.orderdate
        log(f"verify q3 sf={B.args.sf}: top-10 exact OK")
    elif q == "q5":
        (cck, cnat, ook, ock, ood, ssk, snat, cols) = su["verify_data"]
        li_host = {k: v.cpu().numpy() for k, v in cols.items()}
        exp5 = orc.q5({"custkey": cck, "nationkey": cnat},
                      {"orderkey": ook, "custkey": ock,
                       "orderdate": ood}, li_host,
                      {"suppkey": ssk, "nationkey": snat})
        got5 = su["step"]()
        got_rows = sorted(
            ((int(got5["nationkey"][i]), int(got5["rev_lo"][i]))
             for i in range(len(got5["nationkey"]))),
            key=lambda r: (-r[1], r[0]))
        exp_rows = [(r.nationkey, r.revenue_1e4) for r in exp5]
        assert got_rows == exp_rows, (got_rows, exp_rows)
        log(f"verify q5 sf={B.args.sf}: per-nation revenue exact OK")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=8)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--query", choices=["all", "q1", "q3", "q5"],
                    default="all")
    ap.add_argument("--sf", type=float, default=100.0)
    ap.add_argument("--mode", choices=["f64", "dec"], default="f64")
    ap.add_argument("--full", action="store_true",
                    help="also measure q5 (with --query all) and the "
                         "CPU-oracle baselines, print one line per query "
                         "ahead of the combined line, and allow --verify")
    ap.add_argument("--skip-cpu-baseline", action="store_true",
                    help="with --full: leave the CPU-oracle baselines out")
    ap.add_argument("--verify", action="store_true",
                    help="with --full: after timing, check full-size results "
                         "against the CPU oracle (exact decimal + bitwise "
                         "f64)")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="write what the last timed step of each query "
                         "returned as DIR/<query>.<column>.npy")
    args = ap.parse_args()
    if args.verify and not args.full:
        ap.error("--verify is part of the full run: add --full")
    if args.steps < 1:
        ap.error("--steps must be at least 1")
    if args.query != "all":
        args.queries = [args.query]
    else:
        # the headline names Q1 & Q3; q5 is an extra leg of the full run
        args.queries = ["q1", "q3", "q5"] if args.full else ["q1", "q3"]
    # a plain --query all run prints the combined line alone
    per_query_lines = args.full or args.query != "all"

    B = Bench(args)
    per_q = {}
    for q in args.queries:
        su, rec, stats = bench_query(B, q)
        per_q[q] = (rec, stats)
        if args.verify:
            verify(B, q, su)
        if rec is not None and per_query_lines:
            print(json.dumps(rec), flush=True)

    if args.dump_outputs and B.rank == 0:
        dump_outputs(args.dump_outputs,
                     {q: per_q[q][1]["last_out"] for q in per_q})

    # combined headline: the BASELINE metric names "TPC-H SF100 Q1 & Q3" —
    # one combined step = one Q1 pass + one Q3 pass over the HBM-resident
    # SF columns; value = lineitem rows processed per second across both
    if B.rank == 0 and "q1" in per_q and "q3" in per_q:
        r1, s1 = per_q["q1"]
        r3, s3 = per_q["q3"]
        elapsed = s1["elapsed"] + s3["elapsed"]
        total_rows = s1["total_rows"] + s3["total_rows"]
        # dominant kernel of the combined step (larger hot launch)
        dom = "q1" if s1["hot_ms"] >= s3["hot_ms"] else "q3"
        comb = {
            "metric": "tpch_lineitem_rows_per_sec",
            "value": total_rows * args.steps / elapsed,
            "unit": "rows/s",
            "n_gpus": B.n_gpus,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": elapsed / args.steps * 1000.0,
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": r1["dtype"],
            "data": r1["data"],
            "config": {
                "workload": (f"TPC-H SF{int(B.sf_total)} Q1 & Q3 on "
                             f"{B.n_gpus}xMI355X - one step = one Q1 pass "
                             "+ one Q3 pass, columns resident in HBM"),
                "query": "q1+q3",
                "sf": args.sf,
                "rows_per_gpu": s1["n_rows"] + s3["n_rows"],
                "mode": args.mode,
            },
            "roofline": per_q[dom][0]["roofline"],
            "queries": {q: {k: per_q[q][0][k] for k in
                            ("value", "ms_per_step", "roofline",
                             "cpu_baseline")}
                        for q in per_q},
        }
        # combined CPU baseline: same Q1+Q3 composition over the oracle legs
        b1 = r1.get("cpu_baseline")
        b3 = r3.get("cpu_baseline")
        if b1 and b3:
            # rows/s of one q1 pass + one q3 pass on the host cores
            t_unit = 1.0 / b1["value"] + 1.0 / b3["value"]
            comb["cpu_baseline"] = {
                "value": 2.0 / t_unit,
                "unit": "rows/s",
                "cores": b1["cores"],
                "kind": "port",
                "sample": ("oracle (OpenMP, all host cores): one Q1 pass + "
                           "one Q3 pass over bounded TPC-H samples"),
            }
        else:
            comb["cpu_baseline"] = None
        print(json.dumps(comb), flush=True)


if __name__ == "__main__":
    main()
