"""presto_amd — MI355X-native implementation of Presto's per-Page operator
hot path (ScanFilterAndProject / HashAggregation / HashBuilder+LookupJoin /
TopN / PartitionedOutput) as hand-written CDNA4 HIP kernels behind the C-ABI
of include/presto_gpu.h.

This package is the host-side mirror of the reference's Operator surface
(presto-main-base/.../operator/Operator.java:20-102): the Operator class
exposes needs_input/add_input/get_output/finish/is_finished with the same
meaning, and the pipelines in presto_amd.pipelines drive them exactly like
Driver.processInternal (operator/Driver.java:402-475).

There is NO CPU fallback: importing works anywhere (so symbol tests run
without a GPU) but creating any operator requires an AMD gfx950 GPU and
fails loudly otherwise.
"""
from .engine import (  # noqa: F401
    lib, Operator, Scope, Page, Varbin, DictVarbin, DeviceVarbin,
    PlanFilterProject,
    PlanHashAggSmall,
    PlanHashBuild, PlanLookupJoin, PlanTopN, PlanPartition, PlanGroupBy,
    Pred, Proj, Agg,
    CMP_LT, CMP_LE, CMP_GT, CMP_GE, CMP_EQ, CMP_NE, CMP_CONTAINS,
    CMP_PREFIX, CMP_CONTAINS2, CMP_NOT_CONTAINS2, CMP_IS_NULL,
    CMP_IS_NOT_NULL,
    JOIN_INNER, JOIN_PROBE_OUTER, JOIN_LOOKUP_OUTER, JOIN_FULL_OUTER,
    PROJ_IDENT, PROJ_DISC_PRICE, PROJ_CHARGE, PROJ_MUL, PROJ_DIV,
    PROJ_KEYSHL, PROJ_SHR, PROJ_SUBDIV, PROJ_KEYSHL_DIV,
    AGG_COUNT, AGG_SUM_F64, AGG_SUM_DEC, AGG_SUM_I64, AGG_MIN, AGG_MAX,
    OP_FILTER_PROJECT, OP_HASH_AGG_SMALL, OP_HASH_BUILD, OP_LOOKUP_JOIN,
    OP_TOPN, OP_PARTITION, OP_GROUPBY_MULTI, OP_ORDER_BY,
    PlanOrderBy, SORT_ASC_NULLS_FIRST, SORT_ASC_NULLS_LAST,
    SORT_DESC_NULLS_FIRST, SORT_DESC_NULLS_LAST,
    OP_WINDOW, PlanWindow, WinSpec,
    WIN_ROW_NUMBER, WIN_RANK, WIN_DENSE_RANK, WIN_COUNT, WIN_SUM, WIN_MIN,
    WIN_MAX, WIN_LAG, WIN_LEAD,
    FRAME_RANGE_RUNNING, FRAME_ROWS_RUNNING, FRAME_PARTITION,
    OP_MARK_DISTINCT, PlanMarkDistinct, DISTINCT_MARK, DISTINCT_ONLY,
)
from . import pipelines, plans  # noqa: F401
