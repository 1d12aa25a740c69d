"""Plan constructors (presto_amd.plans) and operator scopes
(presto_amd.engine.Scope) — no GPU and no library needed.

Every constructor is pinned byte-for-byte against the struct filled in
field by field, the way the pipelines wrote their plans before the
constructors existed: the C-ABI sees bytes, not Python.
"""
import numpy as np
import pytest

import presto_amd as P
from presto_amd import plans as pl
from presto_amd.engine import Scope


def same(a, b):
    return type(a) is type(b) and bytes(a) == bytes(b)


def test_q3_orders_build_bytes():
    exp = P.PlanHashBuild()
    exp.n_preds = 1
    exp.preds[0] = P.Pred(2, P.CMP_LT, 9204, 0.0)
    exp.key_col = 0
    exp.semijoin_table = 7
    exp.semijoin_col = 1
    exp.n_payload = 1
    exp.payload_col[0] = 2
    exp.capacity_hint = 18750
    exp.key_set_only = 0
    exp.agg_table = 1
    exp.pack_bits = 16
    exp.bitmap_max_key = 600000
    got = pl.hash_build(0, preds=[pl.pred(2, P.CMP_LT, 9204)],
                        semijoin_table=7, semijoin_col=1, payload=[2],
                        capacity_hint=18750, agg_table=1, pack_bits=16,
                        bitmap_max_key=600000)
    assert same(got, exp)


def test_flag_set_and_range_group_bytes():
    exp = P.PlanHashBuild()
    exp.n_preds = 1
    exp.preds[0] = P.Pred(1, P.CMP_EQ, 1, 0.0)
    exp.key_col = 0
    exp.semijoin_table = -1
    exp.n_payload = 0
    exp.capacity_hint = 1500
    exp.key_set_only = 1
    exp.dense_array = 1
    assert same(pl.flag_set(0, 1500, preds=[pl.pred(1, P.CMP_EQ, 1)]), exp)

    exp = P.PlanHashBuild()
    exp.semijoin_table = -1
    exp.capacity_hint = 6000
    exp.range_group = 1
    assert same(pl.range_group(6000), exp)


def test_q21_multi_agg_probe_bytes():
    sk, wsum = 3, 17
    exp = P.PlanLookupJoin()
    exp.table = 11
    exp.key_col = 0
    exp.mode = 1
    exp.n_preds = 0  # preds[] holds the per-aggregate FILTER predicates
    exp.preds[0] = P.Pred(5, P.CMP_EQ, ord("F"), 0.0)
    late = P.Pred(7, P.CMP_GT, 0, 0.0)
    late.rhs_col = 6 + 1
    exp.preds[1] = late
    exp.n_aggs = 5
    exp.aggs[0] = P.Agg(P.AGG_SUM_I64, P.Proj(P.PROJ_IDENT, sk, 0, 0), 0)
    exp.aggs[1] = P.Agg(P.AGG_COUNT, P.Proj(P.PROJ_IDENT, 0, 0, 0), 0)
    exp.aggs[2] = P.Agg(P.AGG_SUM_I64, P.Proj(P.PROJ_IDENT, sk, 0, 0), 0)
    exp.aggs[3] = P.Agg(P.AGG_COUNT, P.Proj(P.PROJ_IDENT, 0, 0, 0), 0)
    exp.aggs[4] = P.Agg(P.AGG_SUM_I64, P.Proj(P.PROJ_MUL, sk, sk, 0), 0)
    for i, f in enumerate((-1, 0, 1, 1, 1)):
        exp.agg_filter[i] = f
    exp.acc_pack = 1
    exp.acc_pack_shift[0] = 0
    exp.acc_pack_width[0] = wsum
    exp.acc_pack_shift[2] = wsum
    exp.acc_pack_width[2] = wsum
    exp.acc_pack_shift[1] = 2 * wsum
    exp.acc_pack_width[1] = 4
    exp.acc_pack_shift[3] = 2 * wsum + 4
    exp.acc_pack_width[3] = 4
    exp.acc_pack_shift[4] = -1
    exp.acc_pack_cnt_shift = 2 * wsum + 8
    exp.acc_pack_cnt_width = 4
    got = pl.lookup_join(
        11, 0, 1,
        filters=[pl.pred(5, P.CMP_EQ, ord("F")),
                 pl.pred_cols(7, P.CMP_GT, 6)],
        aggs=[pl.sum_i64(pl.ident(sk)), (pl.count(), 0),
              (pl.sum_i64(pl.ident(sk)), 1), (pl.count(), 1),
              (pl.sum_i64(pl.mul(sk, sk)), 1)],
        acc_pack=1, acc_pack_shift=[0, 2 * wsum, wsum, 2 * wsum + 4, -1],
        acc_pack_width=[wsum, 4, wsum, 4],
        acc_pack_cnt_shift=2 * wsum + 8, acc_pack_cnt_width=4)
    assert same(got, exp)


def test_filters_index_past_row_predicates():
    """With row-level predicates present, the FILTER predicates follow
    them in preds[] and agg_filter is shifted accordingly."""
    got = pl.group_by([0], [(pl.count(), 1), pl.count()], 64,
                      preds=[pl.pred(2, P.CMP_GT, 0)],
                      filters=[pl.pred(3, P.CMP_EQ, 0),
                               pl.pred(3, P.CMP_NE, 0)])
    assert got.n_preds == 1
    assert bytes(got.preds[2]) == bytes(P.Pred(3, P.CMP_NE, 0, 0.0))
    assert list(got.agg_filter)[:2] == [2, -1]
    with pytest.raises(ValueError, match="agg_filter"):
        pl.group_by([0], [(pl.count(), 2)], 64,
                    filters=[pl.pred(3, P.CMP_EQ, 0)])


def test_emit_and_fused_join_bytes():
    exp = P.PlanLookupJoin()
    exp.table = 4
    exp.n_preds = 2
    exp.preds[0] = P.Pred(2, P.CMP_GE, 8766, 0.0)
    exp.preds[1] = P.Pred(2, P.CMP_LT, 9131, 0.0)
    exp.key_col = 1
    exp.mode = 0
    exp.n_emit = 1
    exp.emit_probe_cols[0] = 0
    got = pl.emit_join(4, 1, [0], preds=[pl.pred(2, P.CMP_GE, 8766),
                                         pl.pred(2, P.CMP_LT, 9131)])
    assert same(got, exp)

    exp = P.PlanLookupJoin()  # Q3's single fused aggregate
    exp.table = 4
    exp.n_preds = 1
    exp.preds[0] = P.Pred(4, P.CMP_GT, 9204, 0.0)
    exp.key_col = 7
    exp.mode = 1
    exp.proj = P.Proj(P.PROJ_DISC_PRICE, 1, 2, 0)
    exp.dec_scale = 4
    exp.dec_only = 1
    got = pl.agg_join(4, 7, pl.disc_price(1, 2), 4,
                      preds=[pl.pred(4, P.CMP_GT, 9204)], dec_only=1)
    assert same(got, exp)

    exp = P.PlanLookupJoin()  # Q5's mode 2
    exp.table = 9
    exp.key_col = 7
    exp.mode = 2
    exp.proj = P.Proj(P.PROJ_DISC_PRICE, 1, 2, 0)
    exp.dec_scale = 4
    exp.table2 = 10
    exp.table2_key_col = 3
    exp.n_group_vals = 5
    for i, v in enumerate((8, 9, 12, 18, 21)):
        exp.group_vals[i] = v
    got = pl.lookup_join(9, 7, 2, proj=pl.disc_price(1, 2), dec_scale=4,
                         table2=10, table2_key_col=3,
                         group_vals=(8, 9, 12, 18, 21))
    assert same(got, exp)

    exp = P.PlanLookupJoin()  # Q10's mode 3
    exp.table = 9
    exp.table2 = 10
    exp.n_preds = 1
    exp.preds[0] = P.Pred(5, P.CMP_EQ, ord("R"), 0.0)
    exp.key_col = 7
    exp.mode = 3
    exp.proj = P.Proj(P.PROJ_DISC_PRICE, 1, 2, 0)
    exp.dec_scale = 4
    exp.dec_only = 1
    got = pl.lookup_join(9, 7, 3, table2=10,
                         preds=[pl.pred(5, P.CMP_EQ, ord("R"))],
                         proj=pl.disc_price(1, 2), dec_scale=4, dec_only=1)
    assert same(got, exp)


def test_q5_column_predicate_bytes():
    exp = P.Pred(2, P.CMP_EQ, 0, 0.0)
    exp.rhs_col = 3 + 1  # compare channel 2 == channel 3
    assert same(pl.pred_cols(2, P.CMP_EQ, 3), exp)
    exp = P.Pred(1, P.CMP_GT, 5, 0.0)  # ship > sold + 5
    exp.rhs_col = 0 + 1
    assert same(pl.pred_cols(1, P.CMP_GT, 0, plus=5), exp)


def test_literal_predicates_bytes():
    assert same(pl.pred(4, P.CMP_GE, 8766), P.Pred(4, P.CMP_GE, 8766, 0.0))
    assert same(pl.pred(2, P.CMP_LE, 0.07), P.Pred(2, P.CMP_LE, 0, 0.07))
    assert same(pl.pred(1, P.CMP_GT, np.int64(300)),
                P.Pred(1, P.CMP_GT, 300, 0.0))


def test_q13_two_needle_predicate_bytes():
    exp = P.Pred(3, P.CMP_NOT_CONTAINS2, 8, 0.0)
    exp.sval = b"special" + b"requests"
    exp.slen = 7
    assert same(pl.pred_varbin(3, P.CMP_NOT_CONTAINS2, b"special",
                               b"requests"), exp)
    exp = P.Pred(1, P.CMP_PREFIX, 0, 0.0)
    exp.sval = b"forest"
    exp.slen = 6
    assert same(pl.pred_varbin(1, P.CMP_PREFIX, b"forest"), exp)
    with pytest.raises(ValueError, match="needle2"):
        pl.pred_varbin(1, P.CMP_CONTAINS, b"a", b"b")
    with pytest.raises(ValueError, match="sval"):
        pl.pred_varbin(1, P.CMP_CONTAINS, b"x" * 41)


def test_varbin_needle_keeps_nul_bytes():
    """A needle is bytes, not a C string: what follows a NUL must reach
    sval (the c_char array setter would stop there)."""
    import ctypes as C
    p = pl.pred_varbin(0, P.CMP_CONTAINS, b"\x00\xffab\x00c")
    assert C.string_at(C.addressof(p) + P.Pred.sval.offset, 40) == \
        b"\x00\xffab\x00c".ljust(40, b"\0")
    assert p.slen == 6
    p = pl.pred_varbin(0, P.CMP_CONTAINS2, b"a\x00", b"\x00b")
    assert C.string_at(C.addressof(p) + P.Pred.sval.offset, 5) == \
        b"a\x00\x00b\x00"
    assert (p.slen, p.ival) == (2, 2)


def test_q1_small_agg_bytes():
    qty, ep, dc, tx, sd, rf, ls = range(7)
    exp = P.PlanHashAggSmall()
    exp.n_preds = 1
    exp.preds[0] = P.Pred(sd, P.CMP_LE, 10471, 0.0)
    exp.n_keys = 2
    exp.key_col[0] = rf
    exp.key_col[1] = ls
    exp.n_vals[0] = 3
    exp.n_vals[1] = 2
    for j, v in enumerate(b"ANR"):
        exp.key_vals[0][j] = v
    for j, v in enumerate(b"FO"):
        exp.key_vals[1][j] = v
    sums = [(P.Proj(P.PROJ_IDENT, qty, 0, 0), 0),
            (P.Proj(P.PROJ_IDENT, ep, 0, 0), 2),
            (P.Proj(P.PROJ_DISC_PRICE, ep, dc, 0), 4),
            (P.Proj(P.PROJ_CHARGE, ep, dc, tx), 6),
            (P.Proj(P.PROJ_IDENT, dc, 0, 0), 2)]
    exp.n_aggs = 6
    for i, (proj, scale) in enumerate(sums):
        exp.aggs[i] = P.Agg(P.AGG_SUM_DEC, proj, scale)
    exp.aggs[5] = P.Agg(P.AGG_COUNT, P.Proj(P.PROJ_IDENT, 0, 0, 0), 0)
    page = P.Page({n: np.zeros(1) for n in
                   ("quantity", "extendedprice", "discount", "tax",
                    "shipdate", "returnflag", "linestatus")})
    assert same(P.pipelines.q1_plan(page, "dec"), exp)
    for i in range(5):
        exp.aggs[i].func = P.AGG_SUM_F64
    assert same(P.pipelines.q1_plan(page, "f64"), exp)

    exp = P.PlanHashAggSmall()  # Q5's listed-key aggregate
    exp.n_preds = 1
    exp.preds[0] = pl.pred_cols(2, P.CMP_EQ, 3)
    exp.n_keys = 1
    exp.key_col[0] = 3
    exp.n_vals[0] = 5
    for i, v in enumerate((8, 9, 12, 18, 21)):
        exp.key_vals[0][i] = v
    exp.n_aggs = 2
    exp.aggs[0] = P.Agg(P.AGG_SUM_DEC, P.Proj(P.PROJ_DISC_PRICE, 0, 1, 0), 4)
    exp.aggs[1] = P.Agg(P.AGG_COUNT, P.Proj(P.PROJ_IDENT, 0, 0, 0), 0)
    exp.drop_unlisted_keys = 1
    got = pl.small_agg([pl.sum_dec(pl.disc_price(0, 1), 4), pl.count()],
                       preds=[pl.pred_cols(2, P.CMP_EQ, 3)],
                       keys=[(3, (8, 9, 12, 18, 21))], drop_unlisted_keys=1)
    assert same(got, exp)


def test_filter_project_bytes():
    exp = P.PlanFilterProject()
    exp.n_preds = 2
    exp.preds[0] = P.Pred(4, P.CMP_GE, 8766, 0.0)
    exp.preds[1] = P.Pred(4, P.CMP_LT, 9131, 0.0)
    exp.n_proj = 2
    exp.proj[0] = P.Proj(P.PROJ_KEYSHL, 0, 1, 32)
    exp.proj[1] = P.Proj(P.PROJ_IDENT, 2, 0, 0)
    exp.semijoin_table = 5
    exp.semijoin_col = 0
    exp.semijoin_anti = 1
    got = pl.filter_project(
        [pl.keyshl(0, 1, 32), pl.ident(2)],
        preds=[pl.pred(4, P.CMP_GE, 8766), pl.pred(4, P.CMP_LT, 9131)],
        semijoin_table=5, semijoin_col=0, semijoin_anti=1)
    assert same(got, exp)
    exp = P.PlanFilterProject()  # no semijoin: the field stays 0
    exp.n_proj = 1
    exp.proj[0] = P.Proj(P.PROJ_KEYSHL_DIV, 1, 0, (14 << 16) | 7)
    assert same(pl.filter_project([pl.keyshl_div(1, 0, 14, 7)]), exp)


def test_group_by_bytes():
    exp = P.PlanGroupBy()
    exp.n_keys = 2
    exp.key_col[0] = 4
    exp.key_col[1] = 5
    exp.capacity_hint = 25 * 2500 + 1024
    exp.n_aggs = 2
    exp.aggs[0] = P.Agg(P.AGG_SUM_DEC, P.Proj(P.PROJ_DISC_PRICE, 1, 2, 0), 4)
    exp.aggs[1] = P.Agg(P.AGG_SUM_DEC, P.Proj(P.PROJ_MUL, 3, 0, 0), 4)
    exp.agg_filter[0] = -1
    exp.agg_filter[1] = -1
    got = pl.group_by([4, 5], [pl.sum_dec(pl.disc_price(1, 2), 4),
                               pl.sum_dec(pl.mul(3, 0), 4)],
                      25 * 2500 + 1024)
    assert same(got, exp)

    exp = P.PlanGroupBy()  # TPC-DS Q72: FILTER split, no row predicate
    exp.n_keys = 3
    for i in range(3):
        exp.key_col[i] = i
    exp.capacity_hint = 4096
    exp.n_preds = 0
    exp.preds[0] = P.Pred(3, P.CMP_EQ, 0, 0.0)
    exp.preds[1] = P.Pred(3, P.CMP_NE, 0, 0.0)
    exp.n_aggs = 3
    for i in range(3):
        exp.aggs[i] = P.Agg(P.AGG_SUM_I64, P.Proj(P.PROJ_SUBDIV, 4, 1, 1), 0)
    exp.agg_filter[0] = 0
    exp.agg_filter[1] = 1
    exp.agg_filter[2] = -1
    extra = pl.sum_i64(pl.subdiv(4, 1, 1))
    got = pl.group_by(range(3), [(extra, 0), (extra, 1), extra], 4096,
                      filters=[pl.pred(3, P.CMP_EQ, 0),
                               pl.pred(3, P.CMP_NE, 0)])
    assert same(got, exp)


def test_top_n_and_partition_bytes():
    exp = P.PlanTopN()
    exp.limit = 10
    exp.val_col = 2
    exp.date_col = 1
    exp.key_col = 0
    assert same(pl.top_n(10, 2, 1, 0), exp)

    exp = P.PlanPartition()
    exp.n_partitions = 8
    exp.key_col = 2
    exp.n_emit = 3
    for i in range(3):
        exp.emit_cols[i] = i
    assert same(pl.partition(8, 2, range(3)), exp)


@pytest.mark.parametrize("field, make", [
    ("preds", lambda: pl.hash_build(0, preds=[pl.pred(0, 0, 0)] * 9)),
    ("preds", lambda: pl.lookup_join(1, 0, 1, preds=[pl.pred(0, 0, 0)] * 7,
                                     filters=[pl.pred(0, 0, 0)] * 2)),
    ("payload_col", lambda: pl.hash_build(0, payload=range(5))),
    ("emit_probe_cols", lambda: pl.emit_join(1, 0, range(9))),
    ("aggs", lambda: pl.lookup_join(1, 0, 1, aggs=[pl.count()] * 7)),
    ("aggs", lambda: pl.group_by([0], [pl.count()] * 7, 16)),
    ("aggs", lambda: pl.small_agg([pl.count()] * 9)),
    ("proj", lambda: pl.filter_project([pl.ident(0)] * 17)),
    ("key_col", lambda: pl.group_by(range(5), [pl.count()], 16)),
    ("key_vals", lambda: pl.small_agg([pl.count()], keys=[(0, range(9))])),
    ("emit_cols", lambda: pl.partition(2, 0, range(9))),
    ("acc_pack_shift", lambda: pl.lookup_join(1, 0, 1,
                                              acc_pack_shift=[0] * 7)),
])
def test_over_long_sequence_names_the_field(field, make):
    with pytest.raises(ValueError, match=field):
        make()


def test_unknown_field_is_rejected():
    with pytest.raises(TypeError, match="dense_aray"):
        pl.hash_build(0, dense_aray=1)


# ---- Scope, driven by stand-in operators that record calls ----
class _FakeOp:
    def __init__(self, log, name, fail_on_feed=False):
        self.log, self.name, self.fail = log, name, fail_on_feed
        self.h = name

    def feed(self, page):
        if self.fail:
            raise RuntimeError("add_input failed")

    def finish(self):
        self.log.append(("finish", self.name))

    def table(self):
        return "T-" + self.name

    def destroy(self):
        self.log.append(("op", self.name))


class _FakeScope(Scope):
    """Scope over stand-ins: only operator creation and the table free
    are replaced; recording, release and unwinding are the real code."""

    def __init__(self, log):
        super().__init__()
        self.log = log
        self.fail_next_feed = False

    def op(self, kind, plan):
        op = _FakeOp(self.log, plan, self.fail_next_feed)
        self._live.append([op, None])
        return op

    def _free_table(self, handle):
        self.log.append(("table", handle))


def _frees(log):
    return [e for e in log if e[0] != "finish"]


def test_scope_unwinds_in_reverse_on_error():
    log = []
    with pytest.raises(KeyError):
        with _FakeScope(log) as s:
            s.build("b1", None)
            s.op(0, "probe1")
            s.build("b2", None)
            s.op(0, "probe2")
            raise KeyError("mid-query")
    assert _frees(log) == [("op", "probe2"),
                           ("table", "T-b2"), ("op", "b2"),
                           ("op", "probe1"),
                           ("table", "T-b1"), ("op", "b1")]
    # each table goes after every probe created after it
    assert log.index(("table", "T-b1")) > log.index(("op", "probe1"))
    assert log.index(("table", "T-b2")) > log.index(("op", "probe2"))


def test_scope_early_release_frees_once():
    log = []
    with _FakeScope(log) as s:
        b = s.build("b", None)
        j = s.op(0, "j")
        s.release(j)
        s.release(j)          # harmless
        k = s.op(0, "k")
        s.release(k, b)
        assert _frees(log) == [("op", "j"), ("op", "k"), ("table", "T-b"),
                               ("op", "b")]
        s.op(0, "last")
    s.close()                 # harmless after exit
    assert _frees(log)[4:] == [("op", "last")]


def test_scope_unfinished_build_has_no_table():
    log = []
    with pytest.raises(RuntimeError, match="add_input failed"):
        with _FakeScope(log) as s:
            s.build("ok", None)
            s.fail_next_feed = True
            s.build("broken", "page")
    assert log == [("finish", "ok"), ("op", "broken"), ("table", "T-ok"),
                   ("op", "ok")]


def test_scope_on_error_keeps_on_success_frees_on_failure():
    log = []
    owner = _FakeScope(log)
    with owner.on_error() as s:
        s.build("kept", None)
    assert _frees(log) == []
    with pytest.raises(ZeroDivisionError):
        with owner.on_error() as s:
            s.op(0, "half")
            1 / 0
    assert _frees(log) == [("op", "half"), ("table", "T-kept"),
                           ("op", "kept")]
