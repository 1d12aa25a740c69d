"""HBM-overflow (grace) partitioned join — the MI355X-native analog of the
reference's spill-to-disk hash build (HashBuilderOperator spilling states,
presto-main-base/.../operator/HashBuilderOperator.java:120-162, and
GenericSpiller).  Instead of serializing to disk, oversized build/probe
sides are hash-PARTITIONED on the GPU (PG_OP_PARTITION — the same
murmur3/`(u32(h)*P)>>32` math as PartitionedOutputOperator) and the
partitions staged out to host memory; each partition then joins entirely
in HBM.  Partitions are disjoint by key, so per-partition results
concatenate exactly.

Partition count: ceil(total_bytes / budget_bytes) rounded up — with 288 GB
of HBM3E per GPU a single partition covers every TPC-H size this repo
benches, so the tests force small budgets to exercise the path.
"""
from . import plans as pl
from .engine import (
    Page, Scope, OP_LOOKUP_JOIN, OP_TOPN, OP_PARTITION,
    CMP_LT, CMP_GT, CMP_EQ,
)


def spill_partition(page: Page, key: str, n_parts: int):
    """Split a page into n_parts host-resident pages by bigint key hash
    (PartitionedOutputOperator.partitionPage math).  The d2h copy is the
    'spill'; partitions return as host Pages ready to re-stage."""
    with Scope() as s:
        op = s.op(OP_PARTITION, pl.partition(
            n_parts, page.channel(key), range(len(page.names))))
        op.add_input(page)
        # d2h: the spill
        return [Page(op.get_output(list(page.names)))
                for _ in range(n_parts)]


def q3_grace(cust: Page, orders: Page, li: Page, n_parts: int, mode="dec",
             limit=10):
    """Q3 with the orders build side treated as HBM-overflowing: orders
    and lineitem are hash-partitioned by orderkey and spilled to host;
    each partition runs the resident Q3 graph (flag-set semijoin build +
    fused-agg probe + TopN); the global TopN is the bounded merge of the
    per-partition TopNs (partitions are disjoint by orderkey).  Results
    are identical to the resident pipeline bit for bit."""
    from .pipelines import Q3_DATE

    rows = []
    with Scope() as s:
        b1 = s.build(pl.flag_set(
            cust.channel("custkey"), cust.n_rows,
            preds=[pl.pred(cust.channel("mktseg"), CMP_EQ, 1)]), cust)

        o_parts = spill_partition(orders, "orderkey", n_parts)
        l_parts = spill_partition(li, "orderkey", n_parts)

        for op_page, lp_page in zip(o_parts, l_parts):
            b2 = s.build(pl.hash_build(
                op_page.channel("orderkey"),
                preds=[pl.pred(op_page.channel("orderdate"), CMP_LT,
                               Q3_DATE)],
                semijoin_table=b1.table(),
                semijoin_col=op_page.channel("custkey"),
                payload=[op_page.channel("orderdate")],
                capacity_hint=max(op_page.n_rows // 4, 16), agg_table=1),
                op_page)
            j = s.run(OP_LOOKUP_JOIN, pl.agg_join(
                b2.table(), lp_page.channel("orderkey"),
                pl.disc_price(lp_page.channel("extendedprice"),
                              lp_page.channel("discount")), 4,
                preds=[pl.pred(lp_page.channel("shipdate"), CMP_GT,
                               Q3_DATE)]), lp_page)
            t = s.run(OP_TOPN,
                      pl.top_n(limit, 2 if mode == "dec" else 3, 1, 0),
                      j.get_output_raw())
            out = t.get_output(["orderkey", "revenue", "orderdate"])
            for i in range(len(out["orderkey"])):
                rows.append((int(out["orderkey"][i]), int(out["revenue"][i])
                             if mode == "dec" else float(out["revenue"][i]),
                             int(out["orderdate"][i])))
            s.release(t, j, b2)
    rows.sort(key=lambda r: (-r[1], r[2], r[0]))
    return rows[:limit]
