"""Pins the ORDER BY reference of order_by_refs.py itself on hand-written
cases of a few rows each, the expected outputs written out literally (the
GPU tests trust this reference, so it is checked against nothing but the
contract)."""
import numpy as np

import order_by_refs as R

NAN_A = 0x7ff8000000000000   # the canonical quiet NaN
NAN_B = 0xfff0000000000001   # negative sign, signalling payload
NAN_C = 0x7ff00000deadbeef   # another payload


def test_order_constants_are_the_abi_values():
    """The reference spells pg_sort_order on its own; the numbers must be
    the binding's."""
    from presto_amd import engine as E
    assert (R.ASC_NULLS_FIRST, R.ASC_NULLS_LAST, R.DESC_NULLS_FIRST,
            R.DESC_NULLS_LAST) == (
        E.SORT_ASC_NULLS_FIRST, E.SORT_ASC_NULLS_LAST,
        E.SORT_DESC_NULLS_FIRST, E.SORT_DESC_NULLS_LAST)


def _f64(bits):
    return np.array(bits, np.uint64).view(np.float64)


def test_f64_ladder_ascending():
    # rows:   0     1      2     3     4     5      6      7      8      9
    bits = [NAN_B, R.f64_bits(1.5), R.f64_bits(-0.0), R.f64_bits(float("inf")),
            NAN_A, R.f64_bits(0.0), R.f64_bits(-1.5),
            R.f64_bits(float("-inf")), NAN_C, R.f64_bits(5e-324)]
    idx = R.sort_indices([(_f64(bits), R.ASC_NULLS_LAST, None)])
    # -inf, -1.5, -0.0, +0.0, denormal, 1.5, +inf, then the NaNs in input
    # order (all equal)
    assert idx == [7, 6, 2, 5, 9, 1, 3, 0, 4, 8]


def test_f64_ladder_descending_keeps_nan_ties_in_input_order():
    bits = [NAN_B, R.f64_bits(1.5), R.f64_bits(-0.0), R.f64_bits(float("inf")),
            NAN_A, R.f64_bits(0.0), R.f64_bits(-1.5),
            R.f64_bits(float("-inf")), NAN_C, R.f64_bits(5e-324)]
    idx = R.sort_indices([(_f64(bits), R.DESC_NULLS_LAST, None)])
    assert idx == [0, 4, 8, 3, 1, 9, 5, 2, 6, 7]


def test_double_compare_signs():
    z, nz = R.f64_bits(0.0), R.f64_bits(-0.0)
    assert R.double_compare_bits(nz, z) == -1
    assert R.double_compare_bits(z, nz) == 1
    assert R.double_compare_bits(z, z) == 0
    assert R.double_compare_bits(NAN_A, NAN_B) == 0
    assert R.double_compare_bits(NAN_C, R.f64_bits(float("inf"))) == 1
    assert R.double_compare_bits(R.f64_bits(float("-inf")), NAN_B) == -1


def test_signed_and_unsigned_integers():
    i32 = np.array([0, -1, 2147483647, -2147483648, 1], np.int32)
    assert R.sort_indices([(i32, R.ASC_NULLS_LAST, None)]) == [3, 1, 0, 4, 2]
    u8 = np.array([128, 0, 255, 127], np.uint8)
    assert R.sort_indices([(u8, R.ASC_NULLS_LAST, None)]) == [1, 3, 0, 2]
    assert R.sort_indices([(u8, R.DESC_NULLS_LAST, None)]) == [2, 0, 3, 1]


def test_nulls_first_last_by_asc_desc():
    #                 0   1   2   3   4
    vals = np.array([30, 99, 10, -7, 20], np.int64)   # 99, -7 sit under nulls
    mask = np.array([0, 1, 0, 1, 0], np.uint8)
    got = {o: R.sort_indices([(vals, o, mask)]) for o in R.ORDERS}
    assert got[R.ASC_NULLS_FIRST] == [1, 3, 2, 4, 0]
    assert got[R.ASC_NULLS_LAST] == [2, 4, 0, 1, 3]
    assert got[R.DESC_NULLS_FIRST] == [1, 3, 0, 4, 2]
    assert got[R.DESC_NULLS_LAST] == [0, 4, 2, 1, 3]


def test_values_under_nulls_are_ignored():
    mask = np.array([1, 0, 1, 0], np.uint8)
    a = np.array([5, 2, -5, 1], np.int64)
    b = np.array([-9, 2, 77, 1], np.int64)
    for o in R.ORDERS:
        assert R.sort_indices([(a, o, mask)]) == \
            R.sort_indices([(b, o, mask)])


def test_ties_keep_input_order_under_desc():
    vals = np.array([1, 2, 1, 2, 1], np.int32)
    assert R.sort_indices([(vals, R.DESC_NULLS_LAST, None)]) == \
        [1, 3, 0, 2, 4]
    assert R.sort_indices([(vals, R.ASC_NULLS_FIRST, None)]) == \
        [0, 2, 4, 1, 3]


def test_two_keys_mixed_direction_and_limit():
    #                0  1  2  3  4  5
    k0 = np.array([1, 0, 1, 0, 1, 0], np.uint8)
    k1 = np.array([5.0, 7.0, 9.0, 7.0, 5.0, -1.0])
    keys = [(k0, R.ASC_NULLS_LAST, None), (k1, R.DESC_NULLS_LAST, None)]
    assert R.sort_indices(keys) == [1, 3, 5, 2, 0, 4]
    assert R.sort_indices(keys, limit=2) == [1, 3]
    assert R.sort_indices(keys, limit=99) == [1, 3, 5, 2, 0, 4]


def test_order_by_gathers_columns_and_masks():
    cols = [np.array([3, 1, 2], np.int64),
            np.array([30, 10, 20], np.int32),
            np.array([[1, 2], [3, 4], [5, 6]], np.uint64)]   # I128
    masks = {1: np.array([0, 1, 0], np.uint8)}
    out, om = R.order_by(cols, masks, [(0, R.ASC_NULLS_LAST)], [1, 2, 1],
                         limit=2)
    assert out[0].tolist() == [10, 20] and out[2].tolist() == [10, 20]
    assert out[1].tolist() == [[3, 4], [5, 6]]
    assert sorted(om) == [0, 2]
    assert om[0].tolist() == [1, 0] and om[2].tolist() == [1, 0]


def test_concat_pages_pads_missing_masks_with_zeros():
    p0 = ([np.array([1, 2], np.int64)], {})
    p1 = ([np.array([], np.int64)], {})
    p2 = ([np.array([3], np.int64)], {0: np.array([1], np.uint8)})
    cols, masks = R.concat_pages([p0, p1, p2])
    assert cols[0].tolist() == [1, 2, 3]
    assert masks[0].tolist() == [0, 0, 1]
