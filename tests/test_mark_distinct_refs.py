"""mark_distinct_refs on hand-written cases (CPU-only)."""
import mark_distinct_refs as M


def test_first_occurrence_one_channel():
    keys = [[5, 7, 5, 5, 9, 7]]
    assert M.markers(keys, [None]) == [1, 1, 0, 0, 1, 0]
    assert M.first_rows(keys, [None]) == [0, 1, 4]


def test_four_null_combinations_on_two_channels():
    """(null,1) (0,1) (null,null) (0,null): four combinations, whatever is
    stored under the nulls; each repeats once with other garbage."""
    a = [77, 0, 88, 0, 99, 0, 11, 0]
    am = [1, 0, 1, 0, 1, 0, 1, 0]
    b = [1, 1, 55, 66, 1, 1, 44, 33]
    bm = [0, 0, 1, 1, 0, 0, 1, 1]
    assert M.key_tuples([a, b], [am, bm])[:4] == [
        (None, 1), (0, 1), (None, None), (0, None)]
    assert M.markers([a, b], [am, bm]) == [1, 1, 1, 1, 0, 0, 0, 0]


def test_null_differs_from_zero_and_equals_null():
    keys = [[0, 0, 3, 0]]
    masks = [[0, 1, 1, 0]]
    assert M.markers(keys, masks) == [1, 1, 0, 0]


def test_all_null_column_is_one_marker():
    assert M.markers([[4, 5, 6]], [[1, 1, 1]]) == [1, 0, 0]


def test_channel_without_mask_has_no_nulls():
    assert M.markers([[1, 1], [2, 3]], [None, [0, 0]]) == [1, 1]


def test_seen_carries_across_pages():
    keys = [[1, 2, 1, 3, 2, 4]]
    whole = M.markers(keys, [None])
    seen = set()
    paged = M.markers([keys[0][:2]], [None], seen) + \
        M.markers([keys[0][2:5]], [None], seen) + \
        M.markers([keys[0][5:]], [None], seen)
    assert whole == paged == [1, 1, 0, 1, 0, 1]


def test_distinct_pages_unlimited():
    keys = [[1, 2, 1, 3, 2, 4, 4]]
    assert M.distinct_pages(keys, [None], (0, 3, 5, 7)) == [
        [0, 1], [3], [5]]
    assert M.distinct_pages(keys, [None], (0, 0, 7)) == [[], [0, 1, 3, 5]]


def test_distinct_pages_limit_cut():
    keys = [[1, 2, 1, 3, 2, 4, 4]]
    splits = (0, 3, 5, 7)
    assert M.distinct_pages(keys, [None], splits, 1) == [[0]]
    assert M.distinct_pages(keys, [None], splits, 2) == [[0, 1]]
    assert M.distinct_pages(keys, [None], splits, 3) == [[0, 1], [3]]
    # exactly the distinct count: the last page reaches it and ends the feed
    assert M.distinct_pages(keys, [None], splits, 4) == [[0, 1], [3], [5]]
    # more than there is: never reached
    assert M.distinct_pages(keys, [None], splits, 5) == [[0, 1], [3], [5]]
    # a cut inside the second page
    keys = [[1, 1, 2, 3, 4, 5]]
    assert M.distinct_pages(keys, [None], (0, 2, 6), 3) == [[0], [2, 3]]
