"""CPU tests of tests/multi_agg_refs.py: the row model on hand-computed
miniatures, the numpy twin against it, and, for every dataset of
tests/test_gpu_multi_agg.py, that the data can see the bugs it is meant to
see (the named wrong models differ from the reference) and that its error
behaviour is decided (clean or must-raise, never ambiguous).
"""
import numpy as np
import pytest

import multi_agg_refs as R
from multi_agg_refs import Agg, Pack, Page, Pred, Spec

H = 1 << 62


# --------------------------------------------------------------------- #
# miniatures, by hand                                                    #
# --------------------------------------------------------------------- #
def _mini():
    """12 rows on the table {3: (30,), 5: (50,)}."""
    pg = Page({"k": np.array([3, 3, 9, 5, 5, 3, 0, 5, 3, 9, 5, 5], np.int64),
               "v": np.array([1, 2, 4, 8, 16, 32, 64, 128, 256, 512, 1024,
                              2048], np.int64),
               "f": np.array([1, 0, 1, 1, 0, 0, 1, 1, 1, 1, 0, 1], np.uint8),
               "p": np.array([1, 1, 1, 1, 1, 0, 1, 1, 1, 1, 1, 0], np.uint8)})
    return R.hash_table([5, 3], ([50, 30],)), pg


def test_hit_miss_and_payload():
    tbl, pg = _mini()
    spec = Spec("k", aggs=(Agg("sum_i64", "v"),))
    assert R.multi_agg_ref(tbl, (pg,), spec) == {
        3: (30, 1 + 2 + 32 + 256, 4),
        5: (50, 8 + 16 + 128 + 1024 + 2048, 5)}


def test_row_predicate_skips_the_row():
    tbl, pg = _mini()
    spec = Spec("k", aggs=(Agg("sum_i64", "v"),), preds=(Pred("p", "eq", 1),))
    assert R.multi_agg_ref(tbl, (pg,), spec) == {
        3: (30, 1 + 2 + 256, 3), 5: (50, 8 + 16 + 128 + 1024, 4)}


def test_filter_gates_its_aggregate_alone():
    tbl, pg = _mini()
    spec = Spec("k", filters=(Pred("f", "eq", 1),),
                aggs=(Agg("sum_i64", "v", filt=0), Agg("sum_i64", "v"),
                      Agg("count", filt=0), Agg("count")))
    assert R.multi_agg_ref(tbl, (pg,), spec) == {
        3: (30, 1 + 256, 291, 2, 4, 4),
        5: (50, 8 + 128 + 2048, 3224, 3, 5, 5)}


def test_filter_that_rejects_every_row_keeps_the_group():
    tbl, pg = _mini()
    spec = Spec("k", filters=(Pred("v", "gt", 5000),),
                aggs=(Agg("sum_i64", "v", filt=0),))
    assert R.multi_agg_ref(tbl, (pg,), spec) == {3: (30, 0, 4),
                                                 5: (50, 0, 5)}


def test_agg_filter_may_name_a_row_predicate():
    tbl, pg = _mini()
    spec = Spec("k", preds=(Pred("p", "eq", 1),),
                aggs=(Agg("sum_i64", "v", filt=0),))
    assert R.multi_agg_ref(tbl, (pg,), spec) == {
        3: (30, 1 + 2 + 256, 3), 5: (50, 8 + 16 + 128 + 1024, 4)}


def test_range_domain_and_no_payload():
    _, pg = _mini()
    spec = Spec("k", aggs=(Agg("count"),))
    assert R.multi_agg_ref(R.range_table(5), (pg,), spec) == {
        3: (4, 4), 5: (5, 5)}
    assert R.multi_agg_ref(R.range_table(9), (pg,), spec) == {
        3: (4, 4), 5: (5, 5), 9: (2, 2)}
    assert R.multi_agg_ref(R.range_table(2), (pg,), spec) == {}


def test_nulls_and_null_tests():
    """A null under the mask fails a comparison whatever the value under
    it; IS_NULL / IS_NOT_NULL read the mask alone."""
    pg = Page({"k": np.ones(6, np.int64),
               "m": np.array([7, 7, 1, 7, 1, 7], np.int64),
               "x": np.array([.25, .75, .25, .25, .75, .25])},
              nulls={"m": [0, 1, 0, 1, 0, 0]})
    spec = Spec("k", filters=(Pred("m", "ge", 5), Pred("m", "is_null"),
                              Pred("m", "not_null"), Pred("x", "lt", 0.5)),
                aggs=(Agg("count", filt=0), Agg("count", filt=1),
                      Agg("count", filt=2), Agg("sum_i64", "m", filt=3)))
    assert R.multi_agg_ref(R.range_table(1), (pg,), spec) == {
        1: (2, 2, 4, 7 + 1 + 7 + 7, 6)}
    # as a row predicate
    spec = Spec("k", preds=(Pred("m", "ne", 1),), aggs=(Agg("count"),))
    assert R.multi_agg_ref(R.range_table(1), (pg,), spec) == {1: (2, 2)}


def test_column_types_and_decimal_ticks():
    from edge_refs import ticks_exact
    x, tx = ticks_exact([-123, 250, 5], 2)
    pg = Page({"k": np.array([2, 2, 2], np.int64),
               "b": np.array([255, 1, 0], np.uint8),
               "w": np.array([-(1 << 31), 5, 6], np.int32),
               "v": np.array([R.I64_MAX, -R.I64_MAX, 1], np.int64),
               "x": x}, ticks={"x": tx})
    assert list(x) == [-1.23, 2.5, 0.05]
    spec = Spec("k", aggs=(Agg("sum_i64", "b"), Agg("sum_i64", "w"),
                           Agg("sum_i64", "v"), Agg("sum_dec", "x", scale=2),
                           Agg("count", "x")))
    assert R.multi_agg_ref(R.range_table(2), (pg,), spec) == {
        2: (256, -(1 << 31) + 11, 1, 132, 3, 3)}


def test_pages_add_up():
    tbl, pg = _mini()
    spec = Spec("k", aggs=(Agg("sum_i64", "v"),))
    whole = R.multi_agg_ref(tbl, (pg,), spec)
    assert R.multi_agg_ref(tbl, (pg.rows(0, 5), pg.rows(5, 12)),
                           spec) == whole
    assert R.multi_agg_ref(tbl, (pg.rows(0, 0),), spec) == {}


# --------------------------------------------------------------------- #
# classification                                                         #
# --------------------------------------------------------------------- #
def _cls(keys, v, pack=None):
    pg = Page({"k": np.array(keys, np.int64), "v": np.array(v, np.int64)})
    return R.classify(R.range_table(9), (pg,),
                      Spec("k", aggs=(Agg("sum_i64", "v"),), pack=pack))


def test_classify_unpacked():
    assert _cls([1, 1], [H, H - 1]) == "clean"          # INT64_MAX
    assert _cls([1, 1], [H, H]) == "overflow"            # 2^63, one sign
    assert _cls([1, 2], [H, H]) == "clean"               # two groups
    assert _cls([1, 1], [-H, -H - 1]) == "overflow"
    with pytest.raises(ValueError, match="ambiguous"):
        _cls([1, 1], [-H, -H])       # INT64_MIN: fits, sum of |x| = 2^63
    with pytest.raises(ValueError, match="ambiguous"):
        _cls([1, 1, 1], [H, H, -5])  # mixed signs, wraps on the way or not
    assert _cls([0, 0], [H, H]) == "clean"               # misses add nothing


def test_classify_packed_field():
    pk = Pack((0,), (4,), 4, 2)
    assert _cls([1, 1, 1], [7, 8, 0], pk) == "clean"              # 15
    with pytest.raises(ValueError, match="ambiguous"):
        _cls([1, 1, 1], [8, 8, 0], pk)       # total 16, no row >= 16
    assert _cls([1, 2, 1], [1, 16, 1], pk) == "overflow"
    assert _cls([1, 2, 1], [1, -1, 1], pk) == "overflow"   # isolated
    assert _cls([2], [-1], pk) == "overflow"               # page edges
    with pytest.raises(ValueError, match="ambiguous"):
        _cls([1, 2, 2], [1, -1, 1], pk)      # a run that may cancel it
    with pytest.raises(ValueError, match="ambiguous"):
        _cls([3, 3, 3, 3], [1, 1, 1, 1], pk)  # 4 rows, 2-bit count
    # an own word is a signed int64 sum
    own = Pack((-1,), (0,), 0, 2)
    assert _cls([1, 2, 1], [1, -1, 1], own) == "clean"
    assert _cls([1, 1], [H, H], own) == "overflow"


def test_classify_failed_rows_break_no_run():
    """The neighbours of a negative row are looked for among the rows that
    pass the row predicates."""
    pg = Page({"k": np.array([2, 3, 2, 3, 4], np.int64),
               "v": np.array([1, 5, -1, 5, 1], np.int64),
               "p": np.array([1, 0, 1, 0, 1], np.uint8)})
    pk = Pack((0,), (4,), 4, 2)
    spec = Spec("k", aggs=(Agg("sum_i64", "v"),), pack=pk,
                preds=(Pred("p", "eq", 1),))
    with pytest.raises(ValueError, match="ambiguous"):
        R.classify(R.range_table(9), (pg,), spec)
    assert R.classify(R.range_table(9), (pg,),
                      spec._replace(preds=())) == "overflow"


# --------------------------------------------------------------------- #
# the wrong models do what their names say                               #
# --------------------------------------------------------------------- #
def test_wrong_models_by_hand():
    tbl, pg = _mini()
    spec = Spec("k", preds=(Pred("p", "eq", 1),),
                filters=(Pred("f", "eq", 1),),
                aggs=(Agg("sum_i64", "v", filt=1), Agg("sum_i64", "v")))
    true = {3: (30, 1 + 256, 1 + 2 + 256, 3),
            5: (50, 8 + 128, 8 + 16 + 128 + 1024, 4)}
    assert R.multi_agg_ref(tbl, (pg,), spec) == true

    def w(bug, pages=(pg,), table=tbl, sp=spec):
        return R.wrong_model(bug, table, pages, sp)

    assert w("a") == {3: (30, 257, 259, 2), 5: (50, 136, 1176, 2)}
    assert w("b") == {3: (30, 257, 257, 3), 5: (50, 136, 136, 4)}
    # quads [3 3 9 5] [5 . 0 5] [3 9 5 .]: the last runs are 5, 5, 5
    assert w("c") == {3: (30, 257, 259, 3), 5: (50, 0, 16, 1)}
    # the misses 9 (row 2), 0 (row 6) and 9 (row 9) follow hits 3, 5, 3
    assert w("d") == {3: (30, 257 + 4 + 512, 259 + 4 + 512, 5),
                      5: (50, 136 + 64, 1176 + 64, 5)}
    assert w("e") == {3: (30, 257, 259, 4), 5: (50, 136, 1176, 5)}
    assert w("j", (pg.rows(0, 4), pg.rows(4, 12))) == {
        3: (30, 256, 256, 1), 5: (50, 128, 16 + 128 + 1024, 3)}
    # range [1, 5]: key k lands in slot k, emitted as k + 1; 5 falls out
    cnt = Spec("k", aggs=(Agg("count"),))
    assert w("h", table=R.range_table(5), sp=cnt) == {4: (4, 4), 1: (1, 1)}
    p8 = R.hash_table([5, 3], ([50, 30],), pack_bits=8)
    assert set(w("i", table=p8)) == {(3 << 8) | 30, (5 << 8) | 50}
    # packed readers: word 0 = a0 | cnt << 12, own word = a1
    pk = spec._replace(pack=Pack((0, -1), (9, 0), 12, 3))
    assert w("f", sp=pk)[3] == (30, 257, 257 | (3 << 12), 3)
    assert w("g", sp=pk) == {3: (30, 1, 259, 3)}     # 257 & 255; 4 & 3 = 0
    for bug in "fghi":                # not applicable: the reference
        assert w(bug) == true


# --------------------------------------------------------------------- #
# the datasets of the GPU tests                                          #
# --------------------------------------------------------------------- #
CASES = R.all_cases()


@pytest.fixture(scope="module")
def refs():
    return {}


def _ref(refs, name):
    if name not in refs:
        c = CASES[name]
        refs[name] = R.multi_agg_ref(c.table, c.pages, c.spec)
    return refs[name]


@pytest.mark.parametrize("name", list(CASES))
def test_dataset_is_decided(name):
    c = CASES[name]
    assert R.classify(c.table, c.pages, c.spec) == c.expect


@pytest.mark.parametrize(
    "name", [n for n, c in CASES.items() if c.expect == "clean"])
def test_numpy_twin_equals_row_model(refs, name):
    """The twin is int64, so the clean inputs only."""
    c = CASES[name]
    assert R.multi_agg_ref_np(c.table, c.pages, c.spec) == _ref(refs, name)


@pytest.mark.parametrize("name", [n for n, c in CASES.items() if c.sees])
def test_dataset_sees_its_wrong_models(refs, name):
    c = CASES[name]
    true = _ref(refs, name)
    for bug in c.sees:
        assert R.wrong_model(bug, c.table, c.pages, c.spec) != true, \
            (bug, R.WRONG_MODELS[bug])


def test_every_wrong_model_is_seen_and_every_generator_sees_some():
    seen = set("".join(c.sees for c in CASES.values()))
    assert seen == set(R.WRONG_MODELS)
    # the cases that claim nothing are the raise cases, the short row
    # counts of the sweep and the all-miss pages
    for name, c in CASES.items():
        if not c.sees:
            assert (c.expect == "overflow" or name.startswith("sweep[") or
                    name.endswith("all_miss]") or
                    name.startswith("pack_raise[")), name
    # of the sweep, the full length does
    assert CASES["sweep[1025]"].sees


def test_dataset_properties():
    """What the GPU tests say about their data."""
    six = CASES["filter[six_filtered]"]
    ref = R.multi_agg_ref(six.table, six.pages, six.spec)
    assert sorted(ref) == list(range(1, 11))       # 11 and 12 miss
    assert ref[5][0] == 0 and ref[5][-1] > 10      # all rows rejected
    assert all(ref[k][0] > 0 for k in ref if k != 5)
    assert all(any(row[a] != row[-1] for row in ref.values())
               for a in range(6))
    # the full fields: group 20 drives every bit field to 2^w - 1, the
    # count to 7, and its neighbours' fields stay 0
    for layout, (pk, n) in R.pack_layouts().items():
        c = R.pack_case(layout, "range")
        ref = R.multi_agg_ref(c.table, c.pages, c.spec)
        assert ref[20][n] == 7 == ref[19][n] == ref[21][n]
        for a in range(n):
            if pk.shift[a] >= 0:
                assert ref[20][a] == (1 << pk.width[a]) - 1
                assert ref[19][a] == ref[21][a] == 0
            else:
                assert ref[20][a] != 0
        own = [ref[k][a] for k in ref for a in range(n) if pk.shift[a] < 0]
        assert not own or (min(own) < 0 < max(own))
    assert R.pack_layouts()["top_field_ends_at_64"][0].shift[1] + \
        R.pack_layouts()["top_field_ends_at_64"][0].width[1] == 64
    # the shapes: payload 255 on the largest key, keys 1 and K present
    t = R.shape_tables()["pack_bits_8"].domain()
    assert t[R.K_SHAPE] == (255,) and t[1] == (0,) and max(t) == R.K_SHAPE
    for shape in R.shape_tables():
        pages = R.shape_pages(shape)
        tbl = R.shape_tables()[shape]
        n_dom = R.K_SHAPE if shape == "range" else 300

        def keys(page):
            return sorted(R.multi_agg_ref(tbl, (pages[page],),
                                          R.SHAPE_SPEC))
        assert keys("only_key_1") == [1]
        assert keys("only_key_K") == [R.K_SHAPE]
        assert len(keys("all_K")) == n_dom
        assert keys("all_miss") == []
        assert {1, R.K_SHAPE} <= set(keys("mixed"))
    # overflow companions
    ref = _ref({}, "overflow[clean]")
    assert {k: v[0] for k, v in ref.items()} == {
        1: H, 2: -H, 3: 1, 4: R.I64_MAX, 5: R.I64_MAX, 6: R.I64_MIN + 1}
    # the long page: a run of one present key straddles any row index
    # that is not a multiple of the run length
    c = R.pass_case(4099)
    k = c.pages[0].cols["k"]
    assert (np.diff(k) >= 0).all() and k[0] == 1 and k[-1] == 1000
