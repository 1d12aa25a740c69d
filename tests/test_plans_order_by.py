"""plans.order_by and its asc / desc helpers (CPU-only: pure ctypes)."""
import pytest

from presto_amd import plans as pl
from presto_amd import engine as E


def test_asc_desc_map_to_the_four_sort_orders():
    assert pl.asc(3) == (3, E.SORT_ASC_NULLS_LAST)
    assert pl.asc(3, nulls_last=False) == (3, E.SORT_ASC_NULLS_FIRST)
    assert pl.desc(5) == (5, E.SORT_DESC_NULLS_LAST)
    assert pl.desc(5, nulls_last=False) == (5, E.SORT_DESC_NULLS_FIRST)
    assert (E.SORT_ASC_NULLS_FIRST, E.SORT_ASC_NULLS_LAST,
            E.SORT_DESC_NULLS_FIRST, E.SORT_DESC_NULLS_LAST) == (0, 1, 2, 3)
    assert E.OP_ORDER_BY == 8


def test_constructor_derives_the_counts():
    p = pl.order_by([pl.desc(2), pl.asc(0, nulls_last=False)], [0, 1, 2, 1],
                    limit=20)
    assert isinstance(p, E.PlanOrderBy)
    assert p.n_keys == 2 and p.n_emit == 4 and p.limit == 20
    assert list(p.key_col)[:2] == [2, 0]
    assert list(p.order)[:2] == [E.SORT_DESC_NULLS_LAST,
                                 E.SORT_ASC_NULLS_FIRST]
    assert list(p.emit_cols)[:4] == [0, 1, 2, 1]
    assert pl.order_by([pl.asc(0)], [0]).limit == 0


def test_reexported_from_the_package():
    import presto_amd as P
    assert P.OP_ORDER_BY == 8 and P.PlanOrderBy is E.PlanOrderBy
    assert P.SORT_DESC_NULLS_FIRST == 2


@pytest.mark.parametrize("n_keys", [0, 5])
def test_rejects_key_counts_naming_the_field(n_keys):
    with pytest.raises(ValueError, match="key_col"):
        pl.order_by([pl.asc(i) for i in range(n_keys)], [0])


@pytest.mark.parametrize("n_emit", [0, 17])
def test_rejects_emit_counts_naming_the_field(n_emit):
    with pytest.raises(ValueError, match="emit_cols"):
        pl.order_by([pl.asc(0)], list(range(n_emit)))


def test_accepts_the_full_widths():
    p = pl.order_by([pl.asc(i) for i in range(4)], list(range(16)))
    assert p.n_keys == 4 and p.n_emit == 16
