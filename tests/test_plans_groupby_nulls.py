"""plans.group_by and the sql_nulls field of the PlanGroupBy mirror
(CPU-only, no library)."""
import ctypes as C

from presto_amd import engine as E
from presto_amd import plans as pl


def _bytes(p):
    return bytes(memoryview(p).cast("B"))


def _args():
    return ([4, 5], [pl.sum_i64(pl.ident(1)), (pl.count(), 0)], 1000)


def test_sql_nulls_sets_only_that_field():
    off = pl.group_by(*_args(), filters=[pl.pred_not_null(1)],
                      sql_nulls=False)
    on = pl.group_by(*_args(), filters=[pl.pred_not_null(1)],
                     sql_nulls=True)
    assert off.sql_nulls == 0 and on.sql_nulls == 1
    on.sql_nulls = 0
    assert _bytes(on) == _bytes(off)


def test_default_is_legacy_and_equals_a_default_mirror():
    exp = E.PlanGroupBy()
    exp.n_keys = 1
    exp.key_col[0] = 3
    exp.capacity_hint = 64
    exp.n_aggs = 1
    exp.aggs[0] = E.Agg(E.AGG_SUM_I64, E.Proj(E.PROJ_IDENT, 2, 0, 0), 0)
    exp.agg_filter[0] = -1
    got = pl.group_by([3], [pl.sum_i64(pl.ident(2))], 64)
    assert got.sql_nulls == 0
    assert _bytes(got) == _bytes(exp)


def test_field_is_last_and_follows_agg_filter():
    f = E.PlanGroupBy
    assert f._fields_[-1][0] == "sql_nulls"
    assert f.sql_nulls.offset == f.agg_filter.offset + f.agg_filter.size
    assert f.sql_nulls.size == 4
    assert C.sizeof(f) % 8 == 0            # capacity_hint aligns the struct
    assert C.sizeof(f) >= f.sql_nulls.offset + 4


def test_other_values_pass_through_for_the_library_to_reject():
    assert pl.group_by(*_args(), filters=[pl.pred_not_null(1)],
                       sql_nulls=2).sql_nulls == 2


def test_min_max_constructors():
    a = pl.agg_min(pl.ident(3))
    b = pl.agg_max(pl.mul(1, 2))
    assert (a.func, a.proj.kind, a.proj.a, a.dec_scale) == \
        (E.AGG_MIN, E.PROJ_IDENT, 3, 0)
    assert (b.func, b.proj.kind, b.proj.a, b.proj.b) == \
        (E.AGG_MAX, E.PROJ_MUL, 1, 2)
