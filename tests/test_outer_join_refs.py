"""The numpy outer-join reference against hand-written cases: every
expected value below is typed out, none is computed."""
import numpy as np
import pytest

import outer_join_refs as R

BK = [10, 20, 20, 30]
P0 = np.array([100, 200, 201, 300], np.int64)
P1 = np.array([1, 2, 3, 4], np.int32)
PK = [20, 5, 10, 20, 40]
ROWID = np.arange(5, dtype=np.int64)


def _rows(cols, masks):
    return list(zip(*(c.tolist() for c in cols), masks.tolist()))


def _drain(drain):
    return None if drain is None else list(zip(*(c.tolist() for c in drain)))


def _join(mode, key_nulls=None, pred_keep=None):
    cols, masks, drain = R.outer_join(BK, [P0, P1], [ROWID], PK, key_nulls,
                                      pred_keep, mode)
    assert cols[0].dtype == np.int64 and cols[1].dtype == np.int64
    assert cols[2].dtype == np.int32 and masks.dtype == np.uint8
    return _rows(cols, masks), _drain(drain)


INNER_ROWS = [(0, 200, 2, 0), (0, 201, 3, 0), (2, 100, 1, 0),
              (3, 200, 2, 0), (3, 201, 3, 0)]
LEFT_ROWS = [(0, 200, 2, 0), (0, 201, 3, 0), (1, 0, 0, 1), (2, 100, 1, 0),
             (3, 200, 2, 0), (3, 201, 3, 0), (4, 0, 0, 1)]


def test_inner():
    assert _join(R.INNER) == (INNER_ROWS, None)


def test_left():
    assert _join(R.PROBE_OUTER) == (LEFT_ROWS, None)


def test_right():
    assert _join(R.LOOKUP_OUTER) == (INNER_ROWS, [(300, 4)])


def test_full():
    assert _join(R.FULL_OUTER) == (LEFT_ROWS, [(300, 4)])


NULL_KEY = np.array([0, 0, 1, 0, 0], np.uint8)   # probe row 2 (key 10)


def test_null_key_never_matches():
    left = [(0, 200, 2, 0), (0, 201, 3, 0), (1, 0, 0, 1), (2, 0, 0, 1),
            (3, 200, 2, 0), (3, 201, 3, 0), (4, 0, 0, 1)]
    right = [(0, 200, 2, 0), (0, 201, 3, 0), (3, 200, 2, 0), (3, 201, 3, 0)]
    assert _join(R.PROBE_OUTER, NULL_KEY) == (left, None)
    assert _join(R.LOOKUP_OUTER, NULL_KEY) == (right, [(100, 1), (300, 4)])
    assert _join(R.FULL_OUTER, NULL_KEY) == (left, [(100, 1), (300, 4)])
    # mode 0 does not read the key mask
    assert _join(R.INNER, NULL_KEY) == (INNER_ROWS, None)


def test_failed_predicate_emits_nothing_and_marks_nothing():
    keep = [False, True, True, False, True]   # both key-20 probes dropped
    rows = [(1, 0, 0, 1), (2, 100, 1, 0), (4, 0, 0, 1)]
    assert _join(R.FULL_OUTER, None, keep) == \
        (rows, [(200, 2), (201, 3), (300, 4)])
    assert _join(R.INNER, None, keep) == ([(2, 100, 1, 0)], None)


@pytest.mark.parametrize("mode", [R.PROBE_OUTER, R.LOOKUP_OUTER,
                                  R.FULL_OUTER])
def test_empty_sides(mode):
    e64 = np.empty(0, np.int64)
    cols, masks, drain = R.outer_join([], [e64], [ROWID], PK, None, None,
                                      mode)
    if mode == R.LOOKUP_OUTER:
        assert _rows(cols, masks) == []
    else:
        assert _rows(cols, masks) == [(i, 0, 1) for i in range(5)]
    assert drain is None or _drain(drain) == []
    cols, masks, drain = R.outer_join(BK, [P0], [e64], [], None, None, mode)
    assert _rows(cols, masks) == []
    if mode != R.PROBE_OUTER:
        assert _drain(drain) == [(100,), (200,), (201,), (300,)]


def test_is_null():
    assert R.is_null(None, 3).tolist() == [False, False, False]
    assert R.is_null(np.array([0, 1, 0], np.uint8), 3).tolist() == \
        [False, True, False]


def test_anti_join():
    assert R.anti_join(BK, PK).tolist() == [1, 4]
    assert R.anti_join(BK, PK, NULL_KEY).tolist() == [1, 2, 4]
    assert R.anti_join(BK, PK, None,
                       [True, False, True, True, True]).tolist() == [4]


def test_canonical_sorts_within_the_multiset():
    cols = [np.array([1, 0, 0]), np.array([5, 9, 7])]
    assert R.canonical(cols, np.array([0, 1, 0], np.uint8)) == \
        [(0, 7, 0), (0, 9, 1), (1, 5, 0)]
