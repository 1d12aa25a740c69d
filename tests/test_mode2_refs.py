"""mode2_refs on hand-computed cases of a few rows each (CPU-only)."""
import numpy as np
import pytest

import mode2_refs as M
from edge_refs import ticks_exact

TABLE = {10: 3, 11: 5, 12: 7}          # orderkey -> customer nation
DENSE2 = np.array([3, 5, 0, 7], np.uint8)  # suppkey 1..4 -> nation; 3 unfilled


def _money(cents, dcents):
    ep, _ = ticks_exact(cents, 2)
    dc, _ = ticks_exact(dcents, 2)
    return ep, dc


def _run(okey, skey, cents, dcents, sel=None, group_vals=(3, 5, 7),
         table=TABLE, dense2=DENSE2):
    ep, dc = _money(cents, dcents)
    return M.mode2_ref(table, dense2, np.array(okey), np.array(skey),
                       cents, dcents, ep, dc, sel, group_vals)


def test_one_match_by_hand():
    """12.34 at 5 % off: 1234 * 95 = 117230 ticks, 12.34 * 0.95 in f64."""
    rows, ovf = _run([10], [1], [1234], [5])
    assert rows == [(3, 117230, 12.34 * (1.0 - 0.05), 1)] and not ovf


def test_missing_key_and_sel():
    rows, _ = _run([10, 13, 10, 10], [1, 1, 1, 1], [100, 100, 200, 400],
                   [0, 0, 0, 0], sel=[1, 1, 0, 1])
    # row 1: key 13 is not in the table; row 2 fails sel
    assert rows == [(3, 50000, 5.0, 2)]


def test_skey_at_the_ends_of_the_dense_range():
    """skey 0 and cap + 1 are dropped unread; 1 and cap are looked up."""
    assert list(M.mode2_group_index(
        {10: 3, 12: 7}, DENSE2, [10, 10, 12, 12, 10], [0, 1, 4, 5, -5],
        None, (3, 7))) == [-1, 0, 1, -1, -1]


def test_unfilled_slot_mismatch_and_unlisted_value():
    tbl = {10: 3, 11: 5, 12: 7, 13: 0}
    gi = M.mode2_group_index(
        tbl, DENSE2,
        [13,   # g1 = 0 = the unfilled slot 3, but 0 is not a group value
         10,   # unfilled slot: g1 = 3 != g2 = 0
         10,   # g1 = 3 != g2 = 5
         11,   # g1 = g2 = 5, which group_vals does not list
         12],  # g1 = g2 = 7
        [3, 3, 2, 2, 4], None, (3, 7))
    assert list(gi) == [-1, -1, -1, -1, 1]
    # with 0 listed the unfilled slot is a group like any other
    assert M.mode2_group_index(tbl, DENSE2, [13], [3], None, (0,))[0] == 0


def test_empty_group_dropped_and_order_follows_group_vals():
    rows, _ = _run([12, 10, 12], [4, 1, 4], [100, 300, 50], [10, 0, 0],
                   group_vals=(7, 5, 3))
    assert rows == [(7, 100 * 90 + 50 * 100, 1.0 * (1.0 - 0.1) + 0.5, 2),
                    (3, 30000, 3.0, 1)]
    assert [r[0] for r in rows] == [7, 3]  # 5 got no row


def test_first_of_duplicate_group_vals_wins():
    rows, _ = _run([10], [1], [100], [0], group_vals=(3, 3))
    assert rows == [(3, 10000, 1.0, 1)]


def test_sum_f64_is_the_correctly_rounded_exact_sum():
    """0.1 ten times: the left-to-right f64 sum is 0.9999999999999999, the
    exact sum of the ten equal addends rounds to 1.0."""
    rows, _ = _run([10] * 10, [1] * 10, [10] * 10, [0] * 10)
    assert sum([0.1] * 10) != 1.0
    assert rows == [(3, 10 * 1000, 1.0, 10)]


def test_domain_assert_fires():
    with pytest.raises(AssertionError, match="64.64"):
        M.check_f64_domain([1.0, 2.0 ** -13])
    with pytest.raises(AssertionError, match="64.64"):
        M.check_f64_domain([2.0 ** 53])
    with pytest.raises(AssertionError, match="64.64"):
        M.check_f64_domain([-0.5])
    with pytest.raises(AssertionError, match="64.64"):
        M.check_f64_domain([float("nan")])
    M.check_f64_domain([0.0, 2.0 ** -12, 2.0 ** 53 - 1.0])
    # and through mode2_ref, on a row that is not even selected
    with pytest.raises(AssertionError, match="64.64"):
        M.mode2_ref(TABLE, DENSE2, [13], [1], [0], [0], [1e-9], [0.0],
                    None, (3,))


def test_overflow_flag():
    """9e17 ticks a row: ten rows fit int64, sixteen do not."""
    cents = [9 * 10 ** 15]
    ep, dc = _money(cents, [0])
    assert ep[0] == 9.0e13 and int(ep[0] * 100.0 + 0.5) == cents[0]
    for n, want in ((10, False), (11, True), (16, True)):
        rows, ovf = _run([10] * n, [1] * n, cents * n, [0] * n)
        assert ovf is want
        assert rows == [(3, n * 9 * 10 ** 17, n * 9.0e13, n)]
    assert 10 * 9 * 10 ** 17 <= M.I64_MAX < 11 * 9 * 10 ** 17


# ------------------------------------------------------------------ fills
def test_dense_fill_range_and_sel():
    out = M.dense_fill_ref([0, -1, 4, 5, 2, 3], [9, 9, 7, 9, 6, 8], 4, 0,
                           [1, 1, 1, 1, 1, 0], np.uint8)
    assert out.tolist() == [0, 6, 0, 7]  # only cap lands of 0, -1, cap, cap+1


def test_dense_fill_u8_bias_wraps():
    out = M.dense_fill_ref([1, 2, 3], [0, 254, 255], 3, 1, None, np.uint8)
    assert out.tolist() == [1, 255, 0]
    assert M.dense_present(out) == {1: 1, 2: 255}  # the wrapped 0 is absent


def test_dense_fill_i32_negative_and_key_set():
    out = M.dense_fill_ref([2, 1, 3], [-5, -1, 70000], 3, 1, None, np.int32)
    assert out.dtype == np.int32 and out.tolist() == [0, -4, 70001]
    flags = M.dense_fill_ref([3, 1], None, 3, 7, None, np.uint8)
    assert flags.tolist() == [1, 0, 1]  # flag 1, the bias does not apply


def test_dense_fill_duplicate_key_is_a_test_error():
    with pytest.raises(AssertionError, match="duplicate"):
        M.dense_fill_ref([2, 2], [1, 1], 3, 0, None, np.uint8)
    # an unselected duplicate is no duplicate
    M.dense_fill_ref([2, 2], [1, 1], 3, 0, [1, 0], np.uint8)
    with pytest.raises(AssertionError, match="duplicate"):
        M.dense_fill_lu_ref([2, 2], [1, 1], [5], 3, 0, None)


def test_dense_fill_lu_miss_leaves_slot_untouched():
    lu = np.array([4, 0, 255], np.uint8)
    out = M.dense_fill_lu_ref([1, 2, 3, 4, 5], [0, 1, 3, 4, 2], lu, 5, 1,
                              None)
    # k2 = 0 and k2 = lu_cap + 1 miss; lu[1] = 0 is a hit and stores 0 + 1;
    # 255 + 1 wraps to 0
    assert out.tolist() == [0, 5, 0, 0, 1]
    assert M.dense_present(out) == {2: 5, 5: 1}
