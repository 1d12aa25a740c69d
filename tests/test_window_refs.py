"""The plain reference of window_refs.py against results worked out by
hand on small tables (CPU-only)."""
import numpy as np
import pytest

import order_by_refs as R
import window_refs as W

ASC, DESC = R.ASC_NULLS_LAST, R.DESC_NULLS_LAST

# rowid, partition key, order key, value (row 3's value is null, 99 under it)
ROWID = np.arange(5, dtype=np.int64)
PKEY = np.array([2, 1, 1, 2, 1], np.int64)
OKEY = np.array([5, 20, 10, 5, 20], np.int32)
VAL = np.array([7, 3, 4, 99, 5], np.int64)
VNULL = np.array([0, 0, 0, 1, 0], np.uint8)
COLS = [ROWID, PKEY, OKEY, VAL]
MASKS = {3: VNULL}
# sorted by (pkey, okey), ties in input order:
#   partition 1: row 2 (o 10, v 4) | rows 1, 4 (o 20, v 3, 5: peers)
#   partition 2: rows 0, 3 (o 5, v 7, null: peers)
SORTED = [2, 1, 4, 0, 3]


def _run(funcs, cols=COLS, masks=MASKS, part=((1, ASC),), order=((2, ASC),)):
    out, m = W.window(cols, masks, list(part), list(order), [0], funcs)
    return out, m


def _one(func, col=None, frame=0, offset=0, **kw):
    out, m = _run([(func, col, frame, offset)], **kw)
    return out[1].tolist(), (m[1].tolist() if 1 in m else None)


def test_rows_come_out_sorted_and_stable():
    out, m = _run([(W.ROW_NUMBER, None, 0, 0)])
    assert out[0].tolist() == SORTED
    assert m == {}


def test_ranking_functions():
    assert _one(W.ROW_NUMBER) == ([1, 2, 3, 1, 2], None)
    assert _one(W.RANK) == ([1, 2, 2, 1, 1], None)
    assert _one(W.DENSE_RANK) == ([1, 2, 2, 1, 1], None)


def test_rank_and_dense_rank_part_ways_after_a_tie():
    # one partition, order keys 1 1 2 3 3 3 4
    o = np.array([1, 1, 2, 3, 3, 3, 4], np.int32)
    cols = [np.arange(7, dtype=np.int64), o]
    kw = dict(cols=cols, masks={}, part=(), order=((1, ASC),))
    assert _one(W.RANK, **kw)[0] == [1, 1, 3, 4, 4, 4, 7]
    assert _one(W.DENSE_RANK, **kw)[0] == [1, 1, 2, 3, 3, 3, 4]
    assert _one(W.ROW_NUMBER, **kw)[0] == [1, 2, 3, 4, 5, 6, 7]


@pytest.mark.parametrize("frame,star,nonnull", [
    (W.RANGE_RUNNING, [1, 3, 3, 2, 2], [1, 3, 3, 1, 1]),
    (W.ROWS_RUNNING, [1, 2, 3, 1, 2], [1, 2, 3, 1, 1]),
    (W.PARTITION, [3, 3, 3, 2, 2], [3, 3, 3, 1, 1]),
])
def test_count_star_and_count_col(frame, star, nonnull):
    assert _one(W.COUNT, None, frame) == (star, None)
    assert _one(W.COUNT, -1, frame) == (star, None)
    assert _one(W.COUNT, 3, frame) == (nonnull, None)


@pytest.mark.parametrize("frame,want", [
    (W.RANGE_RUNNING, [4, 12, 12, 7, 7]),     # peers 1, 4 both see 4+3+5
    (W.ROWS_RUNNING, [4, 7, 12, 7, 7]),
    (W.PARTITION, [12, 12, 12, 7, 7]),
])
def test_sum_per_frame(frame, want):
    assert _one(W.SUM, 3, frame) == (want, [0] * 5)


@pytest.mark.parametrize("func,frame,want", [
    (W.MIN, W.ROWS_RUNNING, [4, 3, 3, 7, 7]),
    (W.MIN, W.RANGE_RUNNING, [4, 3, 3, 7, 7]),
    (W.MIN, W.PARTITION, [3, 3, 3, 7, 7]),
    (W.MAX, W.ROWS_RUNNING, [4, 4, 5, 7, 7]),
    (W.MAX, W.RANGE_RUNNING, [4, 5, 5, 7, 7]),
    (W.MAX, W.PARTITION, [5, 5, 5, 7, 7]),
])
def test_min_max_per_frame(func, frame, want):
    assert _one(func, 3, frame) == (want, [0] * 5)


def test_min_max_keep_the_column_type_and_u8_is_unsigned():
    v = np.array([200, 100, 250, 3, 90], np.uint8)
    out, m = W.window([ROWID, PKEY, OKEY, v], {}, [(1, ASC)], [(2, ASC)],
                      [0], [(W.MAX, 3, W.PARTITION, 0),
                            (W.MIN, 3, W.ROWS_RUNNING, 0)])
    # sorted values: 250 | 100, 90 || 200, 3
    assert out[1].dtype == np.uint8 and out[2].dtype == np.uint8
    assert out[1].tolist() == [250, 250, 250, 200, 200]
    assert out[2].tolist() == [250, 100, 90, 200, 3]


def test_an_all_null_frame_is_null_with_value_zero():
    # partition 2 reversed by a DESC rowid order key: the null row first
    out, m = W.window(COLS, MASKS, [(1, ASC)], [(0, DESC)], [0],
                      [(W.SUM, 3, W.ROWS_RUNNING, 0),
                       (W.MIN, 3, W.ROWS_RUNNING, 0),
                       (W.MAX, 3, W.PARTITION, 0),
                       (W.COUNT, 3, W.ROWS_RUNNING, 0)])
    assert out[0].tolist() == [4, 2, 1, 3, 0]
    assert out[1].tolist() == [5, 9, 12, 0, 7]
    assert m[1].tolist() == [0, 0, 0, 1, 0]
    assert out[2].tolist() == [5, 4, 3, 0, 7]
    assert m[2].tolist() == [0, 0, 0, 1, 0]
    assert out[3].tolist() == [5, 5, 5, 7, 7] and m[3].tolist() == [0] * 5
    assert out[4].tolist() == [1, 2, 3, 0, 1] and 4 not in m


def test_lag_lead_at_the_partition_edges():
    # sorted values 4 | 3, 5 || 7, null(99)
    assert _one(W.LAG, 3, 0, 1) == ([0, 4, 3, 0, 7], [1, 0, 0, 1, 0])
    assert _one(W.LEAD, 3, 0, 1) == ([3, 5, 0, 99, 0], [0, 0, 1, 1, 1])
    assert _one(W.LAG, 3, 0, 2) == ([0, 0, 4, 0, 0], [1, 1, 0, 1, 1])
    assert _one(W.LEAD, 3, 0, 2) == ([5, 0, 0, 0, 0], [0, 1, 1, 1, 1])
    assert _one(W.LEAD, 3, 0, 2**62) == ([0] * 5, [1] * 5)


def test_lag_lead_offset_zero_is_the_row_itself():
    want = ([4, 3, 5, 7, 99], [0, 0, 0, 0, 1])
    assert _one(W.LAG, 3, 0, 0) == want
    assert _one(W.LEAD, 3, 0, 0) == want


def test_lag_copies_f64_bits_and_i128_pairs():
    nan = np.array([0xfff00000deadbeef], np.uint64).view(np.float64)[0]
    f = np.array([nan, -0.0, 1.5], np.float64)
    wide = np.array([[1, 2], [3, 4], [5, 6]], np.uint64)
    cols = [np.arange(3, dtype=np.int64), f, wide]
    out, m = W.window(cols, {}, [], [], [0],
                      [(W.LAG, 1, 0, 1), (W.LEAD, 2, 0, 1)])
    assert out[1].dtype == np.float64
    assert out[1].view(np.uint64).tolist() == [0, 0xfff00000deadbeef,
                                               0x8000000000000000]
    assert m[1].tolist() == [1, 0, 0]
    assert out[2].tolist() == [[3, 4], [5, 6], [0, 0]]
    assert m[2].tolist() == [0, 0, 1]


def test_no_keys_is_one_partition_of_peers_in_input_order():
    kw = dict(part=(), order=())
    assert _run([(W.ROW_NUMBER, None, 0, 0)], **kw)[0][0].tolist() == \
        [0, 1, 2, 3, 4]
    assert _one(W.ROW_NUMBER, **kw)[0] == [1, 2, 3, 4, 5]
    assert _one(W.RANK, **kw)[0] == [1] * 5
    assert _one(W.DENSE_RANK, **kw)[0] == [1] * 5
    assert _one(W.SUM, 3, W.RANGE_RUNNING, **kw)[0] == [19] * 5
    assert _one(W.SUM, 3, W.ROWS_RUNNING, **kw)[0] == [7, 10, 14, 14, 19]


def test_partition_keys_without_order_keys_make_whole_partitions_peers():
    kw = dict(order=())
    # partition 1: rows 1, 2, 4 (values 3, 4, 5); partition 2: rows 0, 3
    assert _run([(W.RANK, None, 0, 0)], **kw)[0][0].tolist() == \
        [1, 2, 4, 0, 3]
    assert _one(W.RANK, **kw)[0] == [1, 1, 1, 1, 1]
    assert _one(W.SUM, 3, W.RANGE_RUNNING, **kw)[0] == [12, 12, 12, 7, 7]
    assert _one(W.SUM, 3, W.ROWS_RUNNING, **kw)[0] == [3, 7, 12, 7, 7]


def test_null_nan_and_signed_zero_partition_keys():
    bits = [0x7ff8000000000000,     # NaN
            0x8000000000000000,     # -0.0
            0x0000000000000000,     # +0.0
            0xfff00000deadbeef,     # another NaN: the same partition
            0x3ff0000000000000,     # under a null
            0x4000000000000000,     # under a null
            0x0000000000000000]     # +0.0
    key = np.array(bits, np.uint64).view(np.float64)
    null = np.array([0, 0, 0, 0, 1, 1, 0], np.uint8)
    cols = [np.arange(7, dtype=np.int64), key]
    out, _ = W.window(cols, {1: null}, [(1, ASC)], [], [0],
                      [(W.ROW_NUMBER, None, 0, 0),
                       (W.COUNT, None, W.PARTITION, 0)])
    # -0.0 | +0.0 +0.0 | NaN NaN | null null
    assert out[0].tolist() == [1, 2, 6, 0, 3, 4, 5]
    assert out[1].tolist() == [1, 1, 2, 1, 2, 1, 2]
    assert out[2].tolist() == [1, 2, 2, 2, 2, 2, 2]


def test_desc_and_nulls_first_partition_keys():
    null = np.array([0, 1, 0, 0, 0], np.uint8)
    out, _ = W.window(COLS, {1: null}, [(1, R.DESC_NULLS_FIRST)],
                      [(2, DESC)], [0], [(W.RANK, None, 0, 0)])
    # null partition: row 1; partition 2: rows 0, 3 (o 5, 5);
    # partition 1: rows 4 (o 20), 2 (o 10)
    assert out[0].tolist() == [1, 0, 3, 4, 2]
    assert out[1].tolist() == [1, 1, 1, 1, 2]


def test_sum_overflow_is_raised_naming_the_function():
    big = np.array([2**63 - 1, 1, -1], np.int64)
    cols = [np.arange(3, dtype=np.int64), big]
    with pytest.raises(W.SumOverflow) as e:
        W.window(cols, {}, [], [(0, ASC)], [0],
                 [(W.COUNT, None, 0, 0), (W.SUM, 1, W.ROWS_RUNNING, 0)])
    assert e.value.func_index == 1
    # the whole partition's total fits: PARTITION is fine
    out, m = W.window(cols, {}, [], [(0, ASC)], [0],
                      [(W.SUM, 1, W.PARTITION, 0)])
    assert out[1].tolist() == [2**63 - 1] * 3
    # and so is a running sum that never leaves int64
    out, m = W.window(cols, {}, [], [(0, DESC)], [0],
                      [(W.SUM, 1, W.ROWS_RUNNING, 0)])
    assert out[1].tolist() == [-1, 0, 2**63 - 1]
    low = np.array([-2**63, -1], np.int64)
    with pytest.raises(W.SumOverflow):
        W.window([np.arange(2, dtype=np.int64), low], {}, [], [], [0],
                 [(W.SUM, 1, W.RANGE_RUNNING, 0)])


def test_zero_rows():
    cols = [np.empty(0, np.int64), np.empty(0, np.int32)]
    out, m = W.window(cols, {}, [(0, ASC)], [(1, ASC)], [0, 1],
                      [(W.ROW_NUMBER, None, 0, 0), (W.MIN, 1, 0, 0),
                       (W.SUM, 1, 0, 0)])
    assert [len(c) for c in out] == [0, 0, 0, 0, 0]
    assert out[3].dtype == np.int32 and out[4].dtype == np.int64
    assert sorted(m) == [3, 4]
