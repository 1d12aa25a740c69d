"""plans.mark_distinct / plans.distinct (CPU-only: pure ctypes)."""
import pytest

from presto_amd import plans as pl
from presto_amd import engine as E


def test_enums():
    assert E.OP_MARK_DISTINCT == 12
    assert (E.DISTINCT_MARK, E.DISTINCT_ONLY) == (0, 1)


def test_reexported_from_the_package():
    import presto_amd as P
    assert P.OP_MARK_DISTINCT == 12
    assert P.PlanMarkDistinct is E.PlanMarkDistinct
    assert (P.DISTINCT_MARK, P.DISTINCT_ONLY) == (0, 1)
    assert P.plans.mark_distinct is pl.mark_distinct
    assert P.plans.distinct is pl.distinct


def test_mark_distinct_derives_the_counts():
    p = pl.mark_distinct([3, 1], [0, 2, 2], 1000)
    assert isinstance(p, E.PlanMarkDistinct)
    assert p.mode == E.DISTINCT_MARK and p.limit == 0
    assert p.n_keys == 2 and list(p.key_col)[:2] == [3, 1]
    assert p.n_emit == 3 and list(p.emit_cols)[:3] == [0, 2, 2]
    assert p.capacity_hint == 1000


def test_distinct_derives_the_counts():
    p = pl.distinct([4], [4, 0], 7)
    assert p.mode == E.DISTINCT_ONLY and p.limit == 0
    assert p.n_keys == 1 and p.key_col[0] == 4
    assert p.n_emit == 2 and list(p.emit_cols)[:2] == [4, 0]
    assert p.capacity_hint == 7
    assert pl.distinct([0], [0], 7, limit=2**40).limit == 2**40
    assert pl.distinct([0], [0], 7, 5).limit == 5


def test_accepts_the_full_widths():
    for make in (pl.mark_distinct, pl.distinct):
        p = make(range(4), range(16), 1)
        assert p.n_keys == 4 and p.n_emit == 16
        assert list(p.key_col) == [0, 1, 2, 3]
        assert list(p.emit_cols) == list(range(16))


@pytest.mark.parametrize("make", [pl.mark_distinct, pl.distinct])
@pytest.mark.parametrize("n_keys", [0, 5])
def test_rejects_key_counts_naming_the_field(make, n_keys):
    with pytest.raises(ValueError, match="key_col"):
        make(range(n_keys), [0], 10)


@pytest.mark.parametrize("make", [pl.mark_distinct, pl.distinct])
@pytest.mark.parametrize("n_emit", [0, 17])
def test_rejects_emit_counts_naming_the_field(make, n_emit):
    with pytest.raises(ValueError, match="emit_cols"):
        make([0], range(n_emit), 10)


def test_mark_distinct_takes_no_limit():
    with pytest.raises(TypeError):
        pl.mark_distinct([0], [0], 10, limit=3)
