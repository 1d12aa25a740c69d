"""The group-by null reference against hand-written expectations (CPU)."""
import numpy as np

import groupby_null_refs as G


def _u8(*v):
    return np.array(v, np.uint8)


def _i64(*v):
    return np.array(v, np.int64)


def test_four_groups_of_two_nullable_channels():
    """(null,1), (0,1), (null,null) and (0,null) are four groups, whatever
    sits under the masks."""
    k0 = _i64(7, 0, 9, 0, 0, 5, 0, 3)
    m0 = _u8(1, 0, 1, 0, 0, 1, 0, 1)
    k1 = _i64(1, 1, 4, 8, 1, 1, 2, 6)
    m1 = _u8(0, 0, 1, 1, 0, 0, 1, 1)
    v = _i64(1, 2, 4, 8, 16, 32, 64, 128)
    got = G.group_by([k0, k1], [m0, m1], [(G.SUM_I64, (G.IDENT, 0), None)],
                     [v], [None])
    assert got == {(None, 1): ([1 + 32], 2), (0, 1): ([2 + 16], 2),
                   (None, None): ([4 + 128], 2), (0, None): ([8 + 64], 2)}
    legacy = G.group_by([k0, k1], [m0, m1],
                        [(G.SUM_I64, (G.IDENT, 0), None)], [v], [None],
                        sql_nulls=False)
    assert legacy[(0, 1)] == ([18], 2) and (7, 1) in legacy
    assert len(legacy) == 7


def test_all_null_aggregate_and_zero_only_group():
    k = _i64(1, 1, 2, 2, 3, 3)
    v = _i64(50, -60, 0, 0, 5, -9)
    m = _u8(1, 1, 0, 0, 0, 1)
    specs = [(G.SUM_I64, (G.IDENT, 0), None), (G.MIN, (G.IDENT, 0), None),
             (G.MAX, (G.IDENT, 0), None), (G.COUNT, (G.IDENT, 0), None)]
    got = G.group_by([k], None, specs, [v], [m])
    assert got == {(1,): ([None, None, None, 2], 2),     # all null
                   (2,): ([0, 0, 0, 2], 2),              # zeros are input
                   (3,): ([5, 5, 5, 2], 2)}              # mixed
    assert G.input_counts([k], None, specs, [v], [m]) == {
        (1,): [(2, 0)] * 3 + [(0, 2)], (2,): [(0, 2)] * 4,
        (3,): [(1, 1)] * 3 + [(0, 2)]}
    legacy = G.group_by([k], None, specs, [v], [m], sql_nulls=False)
    assert legacy[(1,)] == ([-10, -60, 50, 2], 2)
    assert legacy[(3,)] == ([-4, -9, 5, 2], 2)


def test_filter_that_empties_a_group():
    k = _i64(1, 1, 2, 2)
    v = _i64(3, 4, 5, 6)
    f = _i64(10, 200, 10, 20)
    fm = _u8(0, 0, 0, 0)
    flt = (G.GT, 1, 100)
    specs = [(G.MIN, (G.IDENT, 0), flt), (G.SUM_I64, (G.IDENT, 0), flt),
             (G.COUNT, (G.IDENT, 0), flt)]
    got = G.group_by([k], None, specs, [v, f], [None, fm])
    assert got == {(1,): ([4, 4, 1], 2), (2,): ([None, None, 0], 2)}
    legacy = G.group_by([k], None, specs, [v, f], [None, fm],
                        sql_nulls=False)
    assert legacy[(2,)] == ([G.INT64_MAX, 0, 0], 2)
    # a null operand of the comparison rejects the row
    got = G.group_by([k], None, specs, [v, f], [None, _u8(0, 1, 0, 0)])
    assert got[(1,)] == ([None, None, 0], 2)


def test_projection_nullness_and_not_null_filter():
    k = _i64(0, 0, 0, 0)
    a = _i64(2, 3, 5, 7)
    b = _i64(10, 10, 10, 10)
    ma, mb = _u8(0, 1, 0, 0), _u8(0, 0, 1, 0)
    specs = [(G.SUM_I64, (G.MUL, 0, 1), None),
             (G.COUNT, (G.IDENT, 0), (G.NOT_NULL, 0)),
             (G.COUNT, (G.IDENT, 0), (G.IS_NULL, 1))]
    got = G.group_by([k], None, specs, [a, b], [ma, mb])
    assert got == {(0,): ([20 + 70, 3, 1], 4)}


def test_sum_f64_is_the_correctly_rounded_sum_of_rounded_products():
    k = _i64(0, 0, 0)
    ep = np.array([2.0 ** 52 + 1.0, 0.25, 0.25])
    dc = np.array([0.0, 0.5, 0.0])
    specs = [(G.SUM_F64, (G.DISC_PRICE, 0, 1), None)]
    got = G.group_by([k], None, specs, [ep, dc], [None, _u8(0, 0, 1)])
    # 2^52 + 1 + 0.125: the third row is null, the tail rounds away
    assert got == {(0,): ([2.0 ** 52 + 1.0], 3)}
    got = G.group_by([k], None, specs, [ep, dc], None)
    assert got == {(0,): ([2.0 ** 52 + 1.0], 3)}        # + 0.375 rounds down
    ep[2] = 0.5
    got = G.group_by([k], None, specs, [ep, dc], None)
    assert got == {(0,): ([2.0 ** 52 + 2.0], 3)}        # + 0.625 rounds up
