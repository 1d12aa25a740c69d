"""multikey_join_refs.multikey_join against rows typed out by hand, against
outer_join_refs.outer_join where the two overlap (one key, no nulls), and
the null rules of the multi-key join contract."""
import numpy as np
import pytest

import multikey_join_refs as M
import outer_join_refs as R

MODES = (M.INNER, M.PROBE_OUTER, M.LOOKUP_OUTER, M.FULL_OUTER)

# the hand case of the contract: build (k0, k1, pay), probe (k0, k1)
BK0 = np.array([1, 1, 2, 2, 1], np.int64)
BK1 = np.array([10, 20, 10, 10, 10], np.int64)
PAY = np.array([100, 101, 102, 103, 104], np.int64)
PK0 = np.array([1, 2, 2, 10, 1], np.int64)
PK1 = np.array([10, 20, 10, 1, 20], np.int64)
ROWID = np.arange(5, dtype=np.int64)
# (rowid, pay, payload-is-null), probe-row order then build-row order
INNER_ROWS = [(0, 100, 0), (0, 104, 0), (2, 102, 0), (2, 103, 0), (4, 101, 0)]
LEFT_ROWS = [(0, 100, 0), (0, 104, 0), (1, 0, 1), (2, 102, 0), (2, 103, 0),
             (3, 0, 1), (4, 101, 0)]


@pytest.mark.parametrize("mode", MODES)
def test_hand_case(mode):
    cols, masks, drain = M.multikey_join(
        [BK0, BK1], None, [PAY], [ROWID], [PK0, PK1], None, None, mode)
    rows = list(zip(cols[0].tolist(), cols[1].tolist(), masks.tolist()))
    padding = mode in (M.PROBE_OUTER, M.FULL_OUTER)
    assert rows == (LEFT_ROWS if padding else INNER_ROWS)
    assert cols[0].dtype == np.int64 and cols[1].dtype == np.int64
    assert masks.dtype == np.uint8
    if mode in (M.LOOKUP_OUTER, M.FULL_OUTER):
        # every build row is matched by some probe row
        assert len(drain) == 1 and drain[0].tolist() == []
    else:
        assert drain is None


def test_hand_case_drain_and_predicate():
    # without probe rows 0 and 2 the build rows 100/104 and 102/103 drain
    keep = np.array([0, 1, 0, 1, 1], np.uint8)
    cols, masks, drain = M.multikey_join(
        [BK0, BK1], None, [PAY], [ROWID], [PK0, PK1], None, keep,
        M.FULL_OUTER)
    assert list(zip(cols[0].tolist(), cols[1].tolist(), masks.tolist())) == \
        [(1, 0, 1), (3, 0, 1), (4, 101, 0)]
    assert drain[0].tolist() == [100, 102, 103, 104]


def test_positional():
    # (1, 2) does not match (2, 1)
    cols, _, _ = M.multikey_join(
        [[1], [2]], None, [np.array([7], np.int32)], [np.arange(2)],
        [[2, 1], [1, 2]], None, None, M.INNER)
    assert cols[0].tolist() == [1] and cols[1].tolist() == [7]
    assert cols[1].dtype == np.int32


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("seed", [0, 1, 2])
def test_single_key_equals_outer_join(mode, seed):
    rng = np.random.default_rng(seed)
    nb, n = int(rng.integers(0, 60)), int(rng.integers(0, 80))
    bk = rng.integers(0, 12, nb).astype(np.int64)
    pays = [rng.integers(-5, 5, nb).astype(np.int64),
            rng.integers(0, 200, nb).astype(np.uint8)]
    pk = rng.integers(0, 16, n).astype(np.int64)
    rowid = np.arange(n, dtype=np.int64)
    keep = rng.integers(0, 4, n) > 0
    got = M.multikey_join([bk], None, pays, [rowid], [pk], None, keep, mode)
    ref = R.outer_join(bk, pays, [rowid], pk, None, keep, mode)
    for g, e in zip(got[0], ref[0]):
        assert g.dtype == e.dtype and np.array_equal(g, e)
    assert np.array_equal(got[1], ref[1])
    if ref[2] is None:
        assert got[2] is None
    else:
        for g, e in zip(got[2], ref[2]):
            assert g.dtype == e.dtype and np.array_equal(g, e)


@pytest.mark.parametrize("mode", MODES)
def test_null_never_matches_null(mode):
    # both sides null in channel 1 over equal stored values: no match
    bnull = [None, np.array([1, 0], np.uint8)]
    pnull = [None, np.array([1, 0, 0], np.uint8)]
    cols, masks, drain = M.multikey_join(
        [[5, 5], [9, 8]], bnull, [np.array([70, 71], np.int64)],
        [np.arange(3)], [[5, 5, 5], [9, 8, 9]], pnull, None, mode)
    rows = list(zip(cols[0].tolist(), cols[1].tolist(), masks.tolist()))
    if mode in (M.PROBE_OUTER, M.FULL_OUTER):
        assert rows == [(0, 0, 1), (1, 71, 0), (2, 0, 1)]
    else:                               # mode 0 drops null-key probe rows too
        assert rows == [(1, 71, 0)]
    if mode in (M.LOOKUP_OUTER, M.FULL_OUTER):
        assert drain[0].tolist() == [70]   # the null-key build row drains
    else:
        assert drain is None


def test_value_under_null_is_ignored():
    a = M.multikey_join([[1, 2], [3, 4]], [np.array([0, 1], np.uint8), None],
                        [np.array([10, 11])], [np.arange(2)],
                        [[1, 2], [3, 4]], None, None, M.FULL_OUTER)
    b = M.multikey_join([[1, -99], [3, 4]], [np.array([0, 1], np.uint8), None],
                        [np.array([10, 11])], [np.arange(2)],
                        [[1, 2], [3, 4]], None, None, M.FULL_OUTER)
    for x, y in zip(a[0] + [a[1]] + a[2], b[0] + [b[1]] + b[2]):
        assert np.array_equal(x, y)
    assert a[0][1].tolist() == [10, 0] and a[1].tolist() == [0, 1]
    assert a[2][0].tolist() == [11]


def test_empty_build():
    for mode in MODES:
        cols, masks, drain = M.multikey_join(
            [np.zeros(0, np.int64)] * 2, None, [np.zeros(0, np.int32)],
            [np.arange(3)], [[1, 2, 3], [1, 2, 3]], None, None, mode)
        if mode in (M.PROBE_OUTER, M.FULL_OUTER):
            assert cols[0].tolist() == [0, 1, 2] and masks.tolist() == [1] * 3
            assert cols[1].dtype == np.int32 and not cols[1].any()
        else:
            assert len(cols[0]) == 0 and len(masks) == 0
        if mode in (M.LOOKUP_OUTER, M.FULL_OUTER):
            assert len(drain[0]) == 0


def test_canonical_sorts_rows():
    assert M.canonical([[2, 1], [5, 6]], [0, 1]) == [(1, 6, 1), (2, 5, 0)]
