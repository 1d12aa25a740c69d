"""Multi-key join plan constructors: key_col as an int (the single-key
path, n_keys = 0) or as a sequence of 1..4 channels — no GPU and no library
needed."""
import numpy as np
import pytest

import presto_amd as P
from presto_amd import plans as pl

JOINS = (pl.emit_join, pl.left_join, pl.right_join, pl.full_join)
MODES = (P.JOIN_INNER, P.JOIN_PROBE_OUTER, P.JOIN_LOOKUP_OUTER,
         P.JOIN_FULL_OUTER)


def test_hash_build_int_key_is_the_single_key_path():
    for key in (0, 3, np.int64(3), np.int32(2)):
        p = pl.hash_build(key, payload=[1, 2])
        assert p.n_keys == 0 and list(p.key_cols) == [0, 0, 0, 0]
        assert p.key_col == int(key) and p.n_payload == 2
    assert pl.hash_build().n_keys == 0
    assert pl.flag_set(1, 100).n_keys == 0
    assert pl.range_group(100).n_keys == 0


@pytest.mark.parametrize("keys", [[2], [0, 1], (3, 1, 2), [4, 5, 6, 7],
                                  range(1, 3)])
def test_hash_build_sequence_is_multi_key(keys):
    p = pl.hash_build(keys, payload=[8], preds=[pl.pred(0, P.CMP_GT, 1)],
                      semijoin_table=5, semijoin_col=2, capacity_hint=99)
    keys = list(keys)
    assert p.n_keys == len(keys)
    assert list(p.key_cols)[:len(keys)] == keys
    assert list(p.key_cols)[len(keys):] == [0] * (4 - len(keys))
    assert p.key_col == 0
    assert (p.n_payload, p.n_preds, p.semijoin_table, p.semijoin_col,
            p.capacity_hint) == (1, 1, 5, 2, 99)


def test_lookup_join_int_key_is_the_single_key_path():
    for ctor, mode in zip(JOINS, MODES):
        p = ctor(7, 2, [0, 1])
        assert (p.table, p.key_col, p.mode, p.n_emit) == (7, 2, mode, 2)
        assert p.n_keys == 0 and list(p.key_cols) == [0, 0, 0, 0]
    assert pl.agg_join(7, 1, pl.ident(2)).n_keys == 0
    assert pl.lookup_join(7, np.int64(4), 0).key_col == 4


@pytest.mark.parametrize("keys", [[1], [2, 0], (0, 1, 2), [3, 2, 1, 0]])
def test_joins_take_sequences(keys):
    for ctor, mode in zip(JOINS, MODES):
        p = ctor(7, keys, [0], preds=[pl.pred(1, P.CMP_LT, 5)])
        assert p.n_keys == len(keys)
        assert list(p.key_cols)[:len(keys)] == list(keys)
        assert (p.table, p.mode, p.n_emit, p.n_preds, p.key_col) == \
            (7, mode, 1, 1, 0)
    assert pl.lookup_join(7, keys, 0, emit=[1]).n_keys == len(keys)


@pytest.mark.parametrize("keys", [[], (), [0, 1, 2, 3, 4], range(5)])
def test_empty_and_overlong_sequences_raise(keys):
    with pytest.raises(ValueError, match="key_cols"):
        pl.hash_build(keys)
    for ctor in JOINS:
        with pytest.raises(ValueError, match="key_cols"):
            ctor(7, keys, [0])
    with pytest.raises(ValueError, match="key_cols"):
        pl.lookup_join(7, keys, 0)


def test_n_keys_is_derived_not_settable():
    with pytest.raises(TypeError, match="n_keys"):
        pl.hash_build([0, 1], n_keys=1)
    with pytest.raises(TypeError, match="n_keys"):
        pl.lookup_join(7, [0, 1], 0, n_keys=1)
