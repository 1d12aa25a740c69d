"""Outer-join and null-predicate plan constructors, the constants behind
them and Page null masks — no GPU and no library needed."""
import pathlib
import re

import numpy as np
import pytest

import presto_amd as P
from presto_amd import plans as pl

HDR = pathlib.Path(__file__).resolve().parent.parent / "include" / \
    "presto_gpu.h"


def _header_defines():
    return {m.group(1): int(m.group(2)) for m in re.finditer(
        r"^#define\s+(PG_\w+)\s+(-?\d+)\b", HDR.read_text(), re.M)}


def _header_enum(last_member, typedef):
    """name -> value of a `typedef enum { ... } typedef;` of the header,
    comments stripped, explicit `= n` honoured."""
    text = re.sub(r"/\*.*?\*/", "", HDR.read_text(), flags=re.S)
    body = re.search(r"typedef enum \{([^}]*" + last_member + r"[^}]*)\}\s*"
                     + typedef + ";", text).group(1)
    out, nxt = {}, 0
    for item in filter(None, (s.strip() for s in body.split(","))):
        name, _, val = (s.strip() for s in item.partition("="))
        nxt = int(val) if val else nxt
        out[name] = nxt
        nxt += 1
    return out


def test_join_mode_constants_match_header():
    d = _header_defines()
    assert (P.JOIN_INNER, P.JOIN_PROBE_OUTER, P.JOIN_LOOKUP_OUTER,
            P.JOIN_FULL_OUTER) == (0, 4, 5, 6)
    assert d["PG_JOIN_INNER"] == P.JOIN_INNER
    assert d["PG_JOIN_PROBE_OUTER"] == P.JOIN_PROBE_OUTER
    assert d["PG_JOIN_LOOKUP_OUTER"] == P.JOIN_LOOKUP_OUTER
    assert d["PG_JOIN_FULL_OUTER"] == P.JOIN_FULL_OUTER


def test_cmp_constants_match_header():
    e = _header_enum("PG_CMP_IS_NOT_NULL", "pg_cmp")
    # appended: every earlier comparison keeps its number
    assert [e[k] for k in ("PG_CMP_LT", "PG_CMP_NE", "PG_CMP_CONTAINS",
                           "PG_CMP_NOT_CONTAINS2")] == [0, 5, 6, 9]
    assert (P.CMP_IS_NULL, P.CMP_IS_NOT_NULL) == (10, 11)
    assert e["PG_CMP_IS_NULL"] == P.CMP_IS_NULL
    assert e["PG_CMP_IS_NOT_NULL"] == P.CMP_IS_NOT_NULL
    for name, val in e.items():
        assert getattr(P, name[3:]) == val, name


@pytest.mark.parametrize("ctor, mode", [
    (pl.left_join, 4), (pl.right_join, 5), (pl.full_join, 6)])
def test_outer_join_constructors(ctor, mode):
    keep = pl.pred(2, P.CMP_GT, 7)
    got = ctor(11, 1, [0, 3], preds=[keep])
    assert isinstance(got, P.PlanLookupJoin)
    assert got.mode == mode
    exp = pl.emit_join(11, 1, [0, 3], preds=[keep])
    exp.mode = mode     # the inner emit join in every other field
    assert bytes(got) == bytes(exp)
    assert (got.table, got.key_col, got.n_emit, got.n_preds) == (11, 1, 2, 1)
    assert list(got.emit_probe_cols)[:2] == [0, 3]
    assert ctor(11, 1, []).n_preds == 0


@pytest.mark.parametrize("ctor", [pl.left_join, pl.right_join, pl.full_join])
def test_outer_join_rejects_long_emit(ctor):
    ctor(1, 0, range(8))
    with pytest.raises(ValueError, match="emit_probe_cols"):
        ctor(1, 0, range(9))


def test_null_predicates():
    p = pl.pred_is_null(3)
    assert (p.col, p.op, p.rhs_col) == (3, P.CMP_IS_NULL, 0)
    q = pl.pred_not_null(5)
    assert (q.col, q.op, q.rhs_col) == (5, P.CMP_IS_NOT_NULL, 0)
    # count(col) = COUNT FILTER (col IS NOT NULL)
    g = pl.group_by([0], [(pl.count(), 0)], 16, filters=[q])
    assert g.n_preds == 0 and g.agg_filter[0] == 0
    assert g.preds[0].op == P.CMP_IS_NOT_NULL


def test_page_attaches_host_masks():
    a = np.arange(4, dtype=np.int64)
    m = np.array([0, 1, 0, 1], np.uint8)
    page = P.Page({"a": a, "b": a.copy()}, nulls={"b": m})
    c = page.to_c()
    assert not c.cols[0].null_mask
    assert c.cols[1].null_mask == m.ctypes.data
    assert page.nulls["b"] is m     # kept alive by the page
    assert not P.Page({"a": a}).to_c().cols[0].null_mask
    v = P.Varbin([b"x", b"", b"yz"])
    vm = np.array([0, 1, 0], np.uint8)
    c = P.Page({"s": v}, nulls={"s": vm}).to_c()
    assert c.cols[0].null_mask == vm.ctypes.data


def test_page_rejects_bad_masks():
    a = np.arange(4, dtype=np.int64)
    with pytest.raises(ValueError, match="3 entries for 4 rows"):
        P.Page({"a": a}, nulls={"a": np.zeros(3, np.uint8)})
    with pytest.raises(ValueError, match="5 entries for 2 rows"):
        P.Page({"a": a}, n_rows=2, nulls={"a": np.zeros(5, np.uint8)})
    with pytest.raises(ValueError, match="uint8"):
        P.Page({"a": a}, nulls={"a": np.zeros(4, np.int32)})
    with pytest.raises(ValueError, match="no column"):
        P.Page({"a": a}, nulls={"z": np.zeros(4, np.uint8)})
