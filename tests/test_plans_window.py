"""plans.window and the window-function helpers (CPU-only: pure ctypes)."""
import pytest

from presto_amd import plans as pl
from presto_amd import engine as E


def _spec(s):
    return (s.func, s.col, s.frame, s.pad, s.offset)


def test_enums_match_the_header():
    assert E.OP_WINDOW == 10
    assert (E.WIN_ROW_NUMBER, E.WIN_RANK, E.WIN_DENSE_RANK, E.WIN_COUNT,
            E.WIN_SUM, E.WIN_MIN, E.WIN_MAX, E.WIN_LAG, E.WIN_LEAD) == \
        tuple(range(9))
    assert (E.FRAME_RANGE_RUNNING, E.FRAME_ROWS_RUNNING,
            E.FRAME_PARTITION) == (0, 1, 2)
    assert (pl.FRAME_RANGE_RUNNING, pl.FRAME_ROWS_RUNNING,
            pl.FRAME_PARTITION) == (0, 1, 2)


def test_reexported_from_the_package():
    import presto_amd as P
    assert P.OP_WINDOW == 10 and P.PlanWindow is E.PlanWindow
    assert P.WinSpec is E.WinSpec and P.FRAME_PARTITION == 2
    assert P.WIN_LEAD == 8


def test_function_helpers():
    assert _spec(pl.row_number()) == (E.WIN_ROW_NUMBER, -1, 0, 0, 0)
    assert _spec(pl.rank()) == (E.WIN_RANK, -1, 0, 0, 0)
    assert _spec(pl.dense_rank()) == (E.WIN_DENSE_RANK, -1, 0, 0, 0)
    assert _spec(pl.win_count()) == (E.WIN_COUNT, -1, 0, 0, 0)
    assert _spec(pl.win_count(3, frame=pl.FRAME_PARTITION)) == \
        (E.WIN_COUNT, 3, 2, 0, 0)
    assert _spec(pl.win_sum(2)) == (E.WIN_SUM, 2, 0, 0, 0)
    assert _spec(pl.win_sum(2, frame=pl.FRAME_ROWS_RUNNING)) == \
        (E.WIN_SUM, 2, 1, 0, 0)
    assert _spec(pl.win_min(4, frame=pl.FRAME_PARTITION)) == \
        (E.WIN_MIN, 4, 2, 0, 0)
    assert _spec(pl.win_max(5)) == (E.WIN_MAX, 5, 0, 0, 0)
    assert _spec(pl.lag(1)) == (E.WIN_LAG, 1, 0, 0, 1)
    assert _spec(pl.lag(1, 0)) == (E.WIN_LAG, 1, 0, 0, 0)
    assert _spec(pl.lead(6, offset=2**40)) == (E.WIN_LEAD, 6, 0, 0, 2**40)


def test_constructor_derives_the_counts():
    p = pl.window([pl.asc(3), pl.desc(1, nulls_last=False)], [pl.desc(0)],
                  [0, 2, 2], [pl.rank(), pl.win_sum(2), pl.lead(4, 3)])
    assert isinstance(p, E.PlanWindow)
    assert p.n_keys == 3 and p.n_partition_keys == 2
    assert list(p.key_col)[:3] == [3, 1, 0]
    assert list(p.order)[:3] == [E.SORT_ASC_NULLS_LAST,
                                 E.SORT_DESC_NULLS_FIRST,
                                 E.SORT_DESC_NULLS_LAST]
    assert p.n_emit == 3 and list(p.emit_cols)[:3] == [0, 2, 2]
    assert p.n_funcs == 3
    assert [_spec(p.funcs[i]) for i in range(3)] == [
        (E.WIN_RANK, -1, 0, 0, 0), (E.WIN_SUM, 2, 0, 0, 0),
        (E.WIN_LEAD, 4, 0, 0, 3)]


def test_either_key_list_may_be_empty():
    p = pl.window([], [], [0], [pl.row_number()])
    assert p.n_keys == 0 and p.n_partition_keys == 0
    p = pl.window([], [pl.asc(1)], [0], [pl.row_number()])
    assert p.n_keys == 1 and p.n_partition_keys == 0
    p = pl.window([pl.asc(1)], [], [0], [pl.row_number()])
    assert p.n_keys == 1 and p.n_partition_keys == 1


def test_accepts_the_full_widths():
    p = pl.window([pl.asc(0), pl.asc(1)], [pl.asc(2), pl.asc(3)],
                  list(range(16)), [pl.rank()] * 8)
    assert p.n_keys == 4 and p.n_partition_keys == 2
    assert p.n_emit == 16 and p.n_funcs == 8


@pytest.mark.parametrize("n_part,n_order", [(5, 0), (0, 5), (3, 2)])
def test_rejects_more_than_four_keys_naming_the_field(n_part, n_order):
    with pytest.raises(ValueError, match="key_col"):
        pl.window([pl.asc(i) for i in range(n_part)],
                  [pl.asc(i) for i in range(n_order)], [0], [pl.rank()])


@pytest.mark.parametrize("n_emit", [0, 17])
def test_rejects_emit_counts_naming_the_field(n_emit):
    with pytest.raises(ValueError, match="emit_cols"):
        pl.window([pl.asc(0)], [], list(range(n_emit)), [pl.rank()])


@pytest.mark.parametrize("n_funcs", [0, 9])
def test_rejects_function_counts_naming_the_field(n_funcs):
    with pytest.raises(ValueError, match="funcs"):
        pl.window([pl.asc(0)], [], [0], [pl.rank()] * n_funcs)
