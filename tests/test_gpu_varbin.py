"""GPU tests of the variable-width column paths — LIKE pushdowns (d_find),
XxHash64 partitioning and the two-pass VARBIN emit — operator by operator
through the C-ABI, over the four layouts a PG_T_VARBIN column can take:
host raw (Varbin), host dictionary (DictVarbin) and DeviceVarbin of each.

References are the plain Python ones of tests/varbin_refs.py (self-checked on
the CPU by tests/test_varbin_refs.py).  Every assertion is exact.  Each
mandatory case (a match at the last byte, every window offset, a gather of 64
bytes and more, every XXH64 length class) is guarded by an assertion on the
reference, so a change of test data cannot drop it unnoticed.
"""
import ctypes as C
import itertools
import random

import numpy as np
import pytest

import varbin_refs as R  # tests/ is on sys.path (pytest's rootdir import mode)

pytestmark = pytest.mark.gpu

LAYOUTS = ("raw", "dict", "dev_raw", "dev_dict")
FOUR = ("CONTAINS", "PREFIX", "EQ", "NE")
TWO = ("CONTAINS2", "NOT_CONTAINS2")


@pytest.fixture(scope="module")
def P():
    import presto_amd
    return presto_amd


@pytest.fixture(scope="module")
def pl():
    from presto_amd import plans
    return plans


# ---------------- plumbing ----------------

def _words(alphabet, max_len):
    """Every string over `alphabet` (a list of 1-byte strings) of length
    0..max_len, shortest first."""
    return [b"".join(t) for n in range(max_len + 1)
            for t in itertools.product(alphabet, repeat=n)]


def _dictionary(strings, seed):
    """(entries, ids): the distinct strings in shuffled order, with entries
    no row references put between them (copies of real entries with b"ab"
    appended, so a read through a wrong id shows)."""
    uniq = sorted(set(strings))
    random.Random(seed).shuffle(uniq)
    entries, where = [], {}
    for j, u in enumerate(uniq):
        if j % 4 == 0:
            entries.append(u + b"ab")
        where[u] = len(entries)
        entries.append(u)
    entries.append(b"never referenced")
    ids = np.array([where[s] for s in strings], np.int32)
    assert len(set(ids.tolist())) < len(entries)
    return entries, ids


def _column(P, layout, strings, seed=1):
    if layout.endswith("dict"):
        v = P.DictVarbin(*_dictionary(strings, seed))
    else:
        v = P.Varbin(strings)
    return P.DeviceVarbin.from_host(v) if layout.startswith("dev") else v


def _vpage(P, layout, strings, cols, nulls=None, vnull=None):
    """Page {"s": the strings in `layout`, **cols}; cols are host numpy
    columns, nulls their masks, vnull the mask of s (per position)."""
    nl = dict(nulls or {})
    if vnull is not None:
        if layout.startswith("dev"):
            import torch
            nl["s"] = torch.from_numpy(vnull).cuda()
        else:
            nl["s"] = vnull
    return P.Page({"s": _column(P, layout, strings), **cols}, nulls=nl)


def _sval(pred):
    """The 40 bytes of sval as the library will see them."""
    return C.string_at(C.addressof(pred) + type(pred).sval.offset, 40)


def _vpred(P, col, op, a, b=b""):
    """pg_pred of a string op.  sval is written with memmove: needles may
    hold NUL bytes, which the c_char array setter would stop at."""
    raw = a + (b if op in TWO else b"")
    assert len(raw) <= 40
    p = P.Pred(col, R.CMP[op], len(b) if op in TWO else 0, 0.0)
    C.memmove(C.addressof(p) + P.Pred.sval.offset, raw, len(raw))
    p.slen = len(a)
    assert _sval(p) == raw.ljust(40, b"\0")
    return p


def _filter(P, plan, page, names=None):
    op = P.Operator(P.OP_FILTER_PROJECT, plan)
    try:
        op.feed(page)
        return op.get_output(names)
    finally:
        op.destroy()


def _run(P, kind, plan, pages, names=None):
    op = P.Operator(kind, plan)
    try:
        for pg in pages:
            op.feed(pg)
        op.finish()
        return op.get_output(names)
    finally:
        op.destroy()


def _rows(P, pl, page, preds, rid_col=1):
    """Row ids FILTER_PROJECT keeps under the conjunction `preds`."""
    out = _filter(P, pl.filter_project([pl.ident(rid_col)], preds=preds),
                  page)
    return out["c0"].tolist()


def _fails(P, kind, plan, *needles):
    """pg_op_create must fail with a message holding every needle."""
    with pytest.raises(RuntimeError) as e:
        P.Operator(kind, plan).destroy()
    for nd in needles:
        assert nd in str(e.value), (nd, str(e.value))
    return str(e.value)


def _feed_fails(op, page, *needles):
    with pytest.raises(RuntimeError) as e:
        op.feed(page)
    for nd in needles:
        assert nd in str(e.value), (nd, str(e.value))
    return str(e.value)


_REF = {}


def _ref(key, strings, op, a, b=b""):
    """pred_rows without nulls, computed once per (data set, op, needles)
    and shared by the layouts."""
    k = (key, op, a, b)
    if k not in _REF:
        _REF[k] = R.pred_rows(op, strings, a, b)
    return _REF[k]


def _every_third(seq, layout):
    """The full matrix on host raw; the other layouts take every third
    case, chosen by index."""
    return list(seq) if layout == "raw" else list(seq)[::3]


# ---------------- data sets ----------------

STR_A = _words([b"a", b"b"], 10)
PATS_A = _words([b"a", b"b"], 4)[1:]
BYTES_B = [b"\x00", b"\x01", b"\xfe", b"\xff"]
STR_B = _words(BYTES_B, 5)
PATS_B = _words(BYTES_B, 2)[1:]
NEEDLES_C = [b"", b"a", b"b", b"aa", b"ab", b"ba", b"bb"]
N_A = len(STR_A)
RID_A = np.arange(N_A, dtype=np.int64)


def test_data_set_sizes():
    assert (N_A, len(PATS_A), len(STR_B), len(PATS_B)) == (2047, 30, 1365, 20)


@pytest.fixture(scope="module")
def pages_a(P):
    return {lay: _vpage(P, lay, STR_A, {"rid": RID_A}) for lay in LAYOUTS}


# ---------------- a. LIKE matrix over {a, b} ----------------

@pytest.mark.parametrize("layout", LAYOUTS)
def test_like_matrix_ab(P, pl, pages_a, layout):
    """All 2047 strings over {a, b} of length 0..10 against the 30 patterns
    of length 1..4: CONTAINS, PREFIX, EQ, NE through FILTER_PROJECT."""
    pats = _every_third(PATS_A, layout)
    last_only, residues = False, set()
    for a in pats:
        for op in FOUR:
            exp = _ref("A", STR_A, op, a)
            assert _rows(P, pl, pages_a[layout], [_vpred(P, 0, op, a)]) == \
                exp, (op, a)
        for i in _ref("A", STR_A, "CONTAINS", a):
            offs = R.match_offsets(STR_A[i], a)
            last_only |= offs == [len(STR_A[i]) - len(a)] and offs[0] > 0
            residues.add(offs[0] % 4)
    # the reference selected a row matching only at its last position, and
    # a leftmost match at every offset of the 4-byte search window
    assert last_only and residues == {0, 1, 2, 3}


# ---------------- b. LIKE matrix over {00, 01, FE, FF} ----------------

@pytest.mark.parametrize("layout", LAYOUTS)
def test_like_matrix_high_bytes(P, pl, layout):
    """All 1365 strings over {0x00, 0x01, 0xFE, 0xFF} of length 0..5 against
    the 20 patterns of length 1..2: NUL and high-bit bytes, and the
    zero-byte trick's false positive (a byte equal to c0 ^ 0x01 next to a
    real c0)."""
    rid = np.arange(len(STR_B), dtype=np.int64)
    page = _vpage(P, layout, STR_B, {"rid": rid})
    false_pos = False
    for a in _every_third(PATS_B, layout):
        for op in FOUR:
            pred = _vpred(P, 0, op, a)
            plan = pl.filter_project([pl.ident(1)], preds=[pred])
            # every byte of the needle arrived in the plan, NULs included
            assert _sval(plan.preds[0])[:len(a)] == a
            assert plan.preds[0].slen == len(a)
            exp = _ref("B", STR_B, op, a)
            assert _filter(P, plan, page)["c0"].tolist() == exp, (op, a)
        near = bytes([a[0] ^ 1]) + a
        false_pos |= any(near in STR_B[i]
                         for i in _ref("B", STR_B, "CONTAINS", a))
    assert false_pos
    # the plan helper carries NUL bytes too
    for op in ("CONTAINS", "EQ"):
        pred = pl.pred_varbin(0, R.CMP[op], b"\x00\xff")
        assert _sval(pred)[:2] == b"\x00\xff"
        assert _rows(P, pl, page, [pred]) == _ref("B", STR_B, op,
                                                  b"\x00\xff")


def test_one_entry_dictionary(P, pl):
    """A dictionary of one entry that every row references."""
    n = 300
    rid = np.arange(n, dtype=np.int64)
    strings = [b"abab"] * n
    for dev in (False, True):
        v = P.DictVarbin([b"abab"], np.zeros(n, np.int32))
        page = P.Page({"s": P.DeviceVarbin.from_host(v) if dev else v,
                       "rid": rid})
        for op, a in (("EQ", b"abab"), ("NE", b"abab"), ("CONTAINS", b"bab"),
                      ("CONTAINS", b"bb"), ("PREFIX", b"ab")):
            assert _rows(P, pl, page, [_vpred(P, 0, op, a)]) == \
                R.pred_rows(op, strings, a), (dev, op, a)


# ---------------- c. CONTAINS2 / NOT_CONTAINS2 ----------------

@pytest.mark.parametrize("layout", LAYOUTS)
def test_contains2_matrix_ab(P, pl, pages_a, layout):
    """All 49 ordered needle pairs from {"", a, b, aa, ab, ba, bb}: b
    overlapping the tail of a, b directly after a, a == b, empty a or b."""
    pairs = list(itertools.product(NEEDLES_C, NEEDLES_C))
    assert len(pairs) == 49
    for a, b in _every_third(pairs, layout):
        for op in TWO:
            exp = _ref("A", STR_A, op, a, b)
            assert _rows(P, pl, pages_a[layout], [_vpred(P, 0, op, a, b)]) \
                == exp, (op, a, b)
    # the reference met a row in which b only overlaps the tail of a, and
    # one in which b follows a directly
    assert STR_A.index(b"aba") not in _ref("A", STR_A, "CONTAINS2", b"ab",
                                           b"ba")
    assert STR_A.index(b"abba") in _ref("A", STR_A, "CONTAINS2", b"ab", b"ba")


A20 = b"xy yx xxy yyx x y xy"
B20 = b"y xyy  yx xyx yy x x"   # starts with the last 4 bytes of A20


@pytest.fixture(scope="module")
def str_c():
    """About 500 random strings of length 0..300 over {x, y, ' '}; every
    fifth has the 20-byte needles planted: A then B, B then A, A alone, A
    with B overlapping its tail, A directly followed by B."""
    assert len(A20) == len(B20) == 20 and A20[-4:] == B20[:4]
    rng = np.random.default_rng(303)
    alpha = np.frombuffer(b"xy ", np.uint8)
    out = []
    for i in range(500):
        s = alpha[rng.integers(0, 3, rng.integers(0, 301))].tobytes()
        if i % 5 == 0:
            cut = len(s) // 2
            plant = [A20 + s[:7] + B20, B20 + s[:7] + A20, A20,
                     A20 + B20[4:], A20 + B20][i // 5 % 5]
            s = s[:cut] + plant + s[cut:]
        out.append(s)
    return out


@pytest.mark.parametrize("layout", LAYOUTS)
def test_contains2_long_strings(P, pl, str_c, layout):
    rid = np.arange(len(str_c), dtype=np.int64)
    page = _vpage(P, layout, str_c, {"rid": rid})
    for a, b in ((b"xy", b"yx"), (b"x", b"x"), (A20, B20)):
        for op in TWO:
            pred = _vpred(P, 0, op, a, b)
            exp = _ref("C", str_c, op, a, b)
            assert _rows(P, pl, page, [pred]) == exp, (op, a, b)
    pred = _vpred(P, 0, "CONTAINS2", A20, B20)
    assert pred.slen + pred.ival == 40 == len(_sval(pred).rstrip(b"\0"))
    hit = _ref("C", str_c, "CONTAINS2", A20, B20)
    planted = [i for i, s in enumerate(str_c) if A20 in s]
    assert 0 < len(hit) < len(planted)      # some planted rows must fail
    assert max(len(s) for s in str_c) > 256


# ---------------- d. null masks ----------------

VNULL_A = (RID_A % 3 == 0).astype(np.uint8)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_null_masks(P, pl, layout):
    """A mask on every third row (per position for the dictionary layouts,
    whose ids under nulls stay valid): a null passes neither an op nor its
    negation; IS_NULL / IS_NOT_NULL read the mask alone."""
    v = (RID_A % 7).astype(np.int64)
    vmask = (RID_A % 5 == 0).astype(np.uint8)
    page = _vpage(P, layout, STR_A, {"rid": RID_A, "v": v},
                  nulls={"v": vmask}, vnull=VNULL_A)
    for op, a, b in (("EQ", b"ab", b""), ("NE", b"ab", b""),
                     ("CONTAINS", b"ab", b""), ("PREFIX", b"ab", b""),
                     ("CONTAINS2", b"ab", b"ba"),
                     ("NOT_CONTAINS2", b"ab", b"ba"), ("NE", b"", b""),
                     ("EQ", b"aa", b""), ("CONTAINS", b"b", b"")):
        exp = R.pred_rows(op, STR_A, a, b, VNULL_A)
        plain = _ref("A", STR_A, op, a, b)
        # the mask removed rows (the one row equal to b"ab" is not null)
        assert set(exp) < set(plain) or \
            (op == "EQ" and exp == plain == [STR_A.index(b"ab")])
        assert _rows(P, pl, page, [_vpred(P, 0, op, a, b)]) == exp, (op, a)
    null_rows = np.flatnonzero(VNULL_A).tolist()
    assert _rows(P, pl, page, [pl.pred_is_null(0)]) == null_rows
    assert _rows(P, pl, page, [pl.pred_not_null(0)]) == \
        np.flatnonzero(VNULL_A == 0).tolist()
    # NE and NOT_CONTAINS2 are not plain negation: with the mask, an op and
    # its negation together miss exactly the null rows
    both = R.pred_rows("EQ", STR_A, b"ab", nulls=VNULL_A) + \
        R.pred_rows("NE", STR_A, b"ab", nulls=VNULL_A)
    assert sorted(both + null_rows) == RID_A.tolist()
    # a conjunction with an integer predicate whose mask differs
    assert (VNULL_A != vmask).any()
    s_ok = set(R.pred_rows("CONTAINS", STR_A, b"ba", nulls=VNULL_A))
    exp = [i for i in range(N_A) if i in s_ok and not vmask[i] and v[i] >= 3]
    got = _rows(P, pl, page, [_vpred(P, 0, "CONTAINS", b"ba"),
                              pl.pred(2, P.CMP_GE, 3)])
    assert got == exp and 0 < len(exp) < len(s_ok)
    got = _rows(P, pl, page, [pl.pred(2, P.CMP_GE, 3),
                              _vpred(P, 0, "NOT_CONTAINS2", b"a", b"b")])
    s_ok = set(R.pred_rows("NOT_CONTAINS2", STR_A, b"a", b"b", VNULL_A))
    assert got == [i for i in range(N_A)
                   if i in s_ok and not vmask[i] and v[i] >= 3]


# ---------------- e. the same predicates inside the other kernels --------

KERNEL_PREDS = (("EQ", b"abab", b""), ("NE", b"abab", b""),
                ("CONTAINS", b"bab", b""), ("PREFIX", b"ba", b""),
                ("CONTAINS2", b"ab", b"ba"), ("NOT_CONTAINS2", b"ab", b"ba"))
G_A = (RID_A % 3 + 1).astype(np.uint8)


def _q1_fast_launches(P):
    f = P.lib().c.pg_q1_fast_launches
    f.restype = C.c_int64
    return f()


@pytest.mark.parametrize("layout", LAYOUTS)
def test_string_predicates_in_agg_kernels(P, pl, layout):
    """As the HASH_AGG_SMALL pre-filter (one u8 key: the generic kernel) and
    as a GROUPBY_MULTI per-aggregate FILTER, with a null mask on the
    strings: COUNT per group equals the reference."""
    vnull = (RID_A % 5 == 1).astype(np.uint8)    # cuts across the groups
    page = _vpage(P, layout, STR_A, {"rid": RID_A, "g": G_A}, vnull=vnull)
    before = _q1_fast_launches(P)
    for op, a, b in KERNEL_PREDS:
        sel = np.zeros(N_A, bool)
        sel[R.pred_rows(op, STR_A, a, b, vnull)] = True
        want = {k: int((sel & (G_A == k)).sum()) for k in (1, 2, 3)}
        assert sel.any() and sel.sum() < (vnull == 0).sum()
        pred = _vpred(P, 0, op, a, b)
        out = _run(P, P.OP_HASH_AGG_SMALL,
                   pl.small_agg([pl.count()], preds=[pred],
                                keys=[(2, [1, 2, 3])]), [page], ["g", "cnt"])
        assert dict(zip(out["g"].tolist(), out["cnt"].tolist())) == \
            {k: v for k, v in want.items() if v}, op
        out = _run(P, P.OP_GROUPBY_MULTI,
                   pl.group_by([2], [(pl.count(), 0)], 16, filters=[pred]),
                   [page], ["g", "cnt_flt", "cnt"])
        got = {k: (f, c) for k, f, c in zip(out["g"].tolist(),
                                            out["cnt_flt"].tolist(),
                                            out["cnt"].tolist())}
        assert got == {k: (want[k], int((G_A == k).sum()))
                       for k in (1, 2, 3)}, op
    assert _q1_fast_launches(P) == before      # never the Q1 kernel


def test_single_scan_builds_refuse_null_tests(P, pl):
    """agg_table and dense_array builds refuse what they refused before:
    IS NULL / IS NOT NULL pre-filters, at create."""
    for fields in (dict(agg_table=1), dict(dense_array=1, payload=[1])):
        for pred in (pl.pred_is_null(0), pl.pred_not_null(0)):
            _fails(P, P.OP_HASH_BUILD,
                   pl.hash_build(0, preds=[pred], capacity_hint=64, **fields),
                   "IS NULL / IS NOT NULL")


BUILD_ROWS = list(range(20, 20 + 97 * 21, 21))    # b"abab" among them


@pytest.mark.parametrize("layout", LAYOUTS)
def test_string_predicates_in_build_and_probe(P, pl, layout):
    """As the pre-filter of a chained HASH_BUILD over 97 unique keys and as
    the probe predicate of the mode-0 LOOKUP_JOIN on it: the emitted rows
    equal a Python join of the reference-selected rows."""
    assert len(BUILD_ROWS) == 97 and BUILD_ROWS[-1] < N_A
    assert STR_A[BUILD_ROWS[0]] == b"abab"
    n_joined = 0
    b_str = [STR_A[i] for i in BUILD_ROWS]
    b_key = np.arange(1, 98, dtype=np.int64)
    b_pay = b_key * 10
    b_page = _vpage(P, layout, b_str, {"k": b_key, "p": b_pay})
    p_key = (RID_A % 97 + 1).astype(np.int64)
    p_page = _vpage(P, layout, STR_A, {"rid": RID_A, "k": p_key})
    for (bop, ba, bb), (pop, pa, pb) in zip(KERNEL_PREDS,
                                            KERNEL_PREDS[1:] +
                                            KERNEL_PREDS[:1]):
        built = {int(b_key[j]): int(b_pay[j])
                 for j in R.pred_rows(bop, b_str, ba, bb)}
        exp = [(i, built[int(p_key[i])])
               for i in R.pred_rows(pop, STR_A, pa, pb)
               if int(p_key[i]) in built]
        assert 0 < len(built) < 97
        n_joined += len(exp)
        b = P.Operator(P.OP_HASH_BUILD,
                       pl.hash_build(1, preds=[_vpred(P, 0, bop, ba, bb)],
                                     payload=[2], capacity_hint=97))
        try:
            b.feed(b_page)
            b.finish()
            tbl = b.table()
            try:
                out = _run(P, P.OP_LOOKUP_JOIN,
                           pl.emit_join(tbl, 2, [1],
                                        preds=[_vpred(P, 0, pop, pa, pb)]),
                           [p_page], ["rid", "p"])
            finally:
                P.lib().c.pg_table_destroy(tbl)
        finally:
            b.destroy()
        assert list(zip(out["rid"].tolist(), out["p"].tolist())) == exp, \
            (bop, pop)
    assert n_joined > 500


# ---------------- f. VARBIN emit ----------------

EMIT_LENS = (0, 1, 63, 64, 65, 127, 128, 129, 1000)
N_EMIT = 2049


@pytest.fixture(scope="module")
def str_f():
    """Lengths cycle through EMIT_LENS; byte b of row r is (7r + b) % 251."""
    base = np.arange(1000, dtype=np.int64)
    return [((7 * r + base[:EMIT_LENS[r % 9]]) % 251).astype(np.uint8)
            .tobytes() for r in range(N_EMIT)]


@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 2049])
def test_varbin_emit(P, pl, str_f, n):
    """k_varbin_len / k_varbin_gather: output offsets and bytes equal the
    Python gather, for every layout and selection; the strings of 64 bytes
    and more take further trips of the per-wave copy loop."""
    strings = str_f[:n]
    rid = np.arange(n, dtype=np.int64)
    sels = {"all": list(range(n)), "none": [], "odd": list(range(1, n, 2)),
            "last": [n - 1],
            "empty": [i for i in range(n) if not strings[i]]}
    assert sels["empty"] and all(i % 9 == 0 for i in sels["empty"])
    if n >= 63:
        for name in ("all", "odd"):
            lens = {len(strings[i]) for i in sels[name]}
            assert lens >= {63, 64, 65, 127, 128, 129, 1000}
    flags = {}
    for name, rows in sels.items():
        flags[name] = np.zeros(n, np.uint8)
        flags[name][rows] = 1
    for layout in LAYOUTS:
        page = _vpage(P, layout, strings, {"rid": rid, **flags})
        for name, rows in sels.items():
            pred = _vpred(P, 0, "EQ", b"") if name == "empty" \
                else pl.pred(page.channel(name), P.CMP_EQ, 1)
            out = _filter(P, pl.filter_project([pl.ident(0), pl.ident(1)],
                                               preds=[pred]), page)
            offs, data = R.gather(strings, rows)
            assert out["c1"].tolist() == rows, (layout, name)
            assert out["c0"].offsets.tolist() == offs, (layout, name)
            assert out["c0"].data.tobytes() == data, (layout, name)


@pytest.mark.parametrize("layout", LAYOUTS)
def test_varbin_emit_same_column_twice(P, pl, str_f, layout):
    n = 257
    strings = str_f[:n]
    rid = np.arange(n, dtype=np.int64)
    page = _vpage(P, layout, strings, {"rid": rid, "m": rid % 3})
    rows = [i for i in range(n) if i % 3 != 1]
    assert {len(strings[i]) for i in rows} >= {0, 64, 1000}
    out = _filter(P, pl.filter_project(
        [pl.ident(0), pl.ident(1), pl.ident(0)],
        preds=[pl.pred(2, P.CMP_NE, 1)]), page)
    offs, data = R.gather(strings, rows)
    assert out["c1"].tolist() == rows
    for c in ("c0", "c2"):
        assert out[c].offsets.tolist() == offs
        assert out[c].data.tobytes() == data


# ---------------- g. XxHash64 partitioning on the device ----------------

HASH_CLASSES = (0, 3, 4, 7, 8, 31, 32, 33, 39, 40, 63, 64, 65, 100)


@pytest.fixture(scope="module")
def str_g():
    """505 rows: five strings of every length 0..100, bytes 0..255, in a
    shuffled order (so that a prefix mixes the lengths)."""
    rng = np.random.default_rng(404)
    out = [bytes(rng.integers(0, 256, ln, dtype=np.uint8))
           for ln in range(101) for _ in range(5)]
    random.Random(404).shuffle(out)
    lens = {len(s) for s in out}
    assert len(out) == 505 and lens >= set(HASH_CLASSES)
    # the stripe loop, the 8-byte loop, the 4-byte step and the byte tail
    # in every combination, and the empty string
    assert len({tuple(sorted(R.xxh64_paths(n).items())) for n in lens}) == 16
    return out


@pytest.fixture(scope="module")
def hash_g(str_g):
    return [R.xxh64(s) for s in str_g]


def _partition_case(P, pl, layout, strings, hashes, n_part):
    n = len(strings)
    rid = np.arange(n, dtype=np.int64)
    page = _vpage(P, layout, strings, {"rid": rid})
    op = P.Operator(P.OP_PARTITION, pl.partition(n_part, 0, [1]))
    try:
        op.feed(page)
        counts = op.partition_counts(n_part)
        pages = [op.get_output(["rid"]) for _ in range(n_part)]
        assert op.get_output() is None
    finally:
        op.destroy()
    pid = [R.partition(h, n_part) for h in hashes]
    for p in range(n_part):
        exp = [i for i in range(n) if pid[i] == p]
        assert pages[p]["rid"].tolist() == exp, (layout, n_part, p)
        assert counts[p] == len(exp), (layout, n_part, p)
    return pid


@pytest.mark.parametrize("n_part", [1, 2, 7, 256])
@pytest.mark.parametrize("layout", LAYOUTS)
def test_xxh64_partitioning(P, pl, str_g, hash_g, layout, n_part):
    """pg_xxh64 on the device over every length class: each output page's
    row ids and pg_op_partition_counts equal partition(xxh64(s), n) of the
    Python restatement."""
    pid = _partition_case(P, pl, layout, str_g, hash_g, n_part)
    if n_part > 1:
        assert len(set(pid)) > n_part // 2      # the hash spreads the rows


@pytest.mark.parametrize("layout", LAYOUTS)
def test_xxh64_partitioning_row_counts(P, pl, str_g, hash_g, layout):
    """The wave and window tails of k_part_count / k_part_emit."""
    for n in (0, 1, 63, 64, 65, 255, 256, 257):
        _partition_case(P, pl, layout, str_g[:n], hash_g[:n], 7)


# ---------------- h. what the C ABI rejects ----------------

def _with_pred(P, pl, kind, pred, as_filter=False):
    """A plan of `kind` carrying `pred` as its only predicate."""
    if kind == P.OP_FILTER_PROJECT:
        return pl.filter_project([pl.ident(1)], preds=[pred])
    if kind == P.OP_HASH_AGG_SMALL:
        return pl.small_agg([pl.count()], preds=[pred], keys=[(2, [1, 2, 3])])
    if kind == P.OP_HASH_BUILD:
        return pl.hash_build(1, preds=[pred], capacity_hint=64)
    if kind == P.OP_LOOKUP_JOIN:
        return pl.emit_join(0, 1, [1], preds=[pred])
    if as_filter:
        return pl.group_by([2], [(pl.count(), 0)], 16, filters=[pred])
    return pl.group_by([2], [pl.count()], 16, preds=[pred])


def _op_kinds(P):
    return {"FILTER_PROJECT": P.OP_FILTER_PROJECT,
            "HASH_AGG_SMALL": P.OP_HASH_AGG_SMALL,
            "HASH_BUILD": P.OP_HASH_BUILD, "LOOKUP_JOIN": P.OP_LOOKUP_JOIN,
            "GROUPBY_MULTI": P.OP_GROUPBY_MULTI}


@pytest.mark.parametrize("name", ["FILTER_PROJECT", "HASH_AGG_SMALL",
                                  "HASH_BUILD", "LOOKUP_JOIN",
                                  "GROUPBY_MULTI"])
def test_needle_lengths_checked_at_create(P, pl, name):
    """slen and, for the two-needle ops, ival are validated by
    pg_op_create: the error names the operator, the predicate and the
    field."""
    kind = _op_kinds(P)[name]

    def bad(op, slen, ival):
        p = _vpred(P, 0, op, b"ab", b"ba")
        p.slen, p.ival = slen, ival
        return p

    for op, slen, ival, field in (("EQ", 41, 0, "slen"),
                                  ("CONTAINS", -1, 0, "slen"),
                                  ("CONTAINS2", 21, 20, "ival"),
                                  ("NOT_CONTAINS2", 20, 21, "ival"),
                                  ("CONTAINS2", 2, -1, "ival"),
                                  ("CONTAINS2", 41, 0, "slen")):
        msg = _fails(P, kind, _with_pred(P, pl, kind, bad(op, slen, ival)),
                     name, "preds[0]", field)
        other = "ival" if field == "slen" else "slen"
        assert other not in msg
    if name == "GROUPBY_MULTI":     # a per-aggregate FILTER is checked too
        _fails(P, kind, _with_pred(P, pl, kind, bad("EQ", 41, 0), True),
               name, "preds[0]", "slen")
    if name != "LOOKUP_JOIN":       # (table 0 does not exist)
        for op, slen, ival in (("EQ", 40, 0), ("CONTAINS2", 20, 20),
                               ("CONTAINS2", 0, 40), ("EQ", 0, 0)):
            P.Operator(kind, _with_pred(P, pl, kind,
                                        bad(op, slen, ival))).destroy()


def test_needles_of_full_length(P, pl):
    """slen = 40 works, and so does CONTAINS2 with slen + ival = 40."""
    full = bytes(range(1, 41))
    strings = [full, full[:39], full + b"\x29", full[:39] + b"\x00", b"",
               b"x" + full, A20 + B20, A20 + b"-" + B20, B20 + A20, A20]
    rid = np.arange(len(strings), dtype=np.int64)
    for layout in LAYOUTS:
        page = _vpage(P, layout, strings, {"rid": rid})
        for op, a, b in (("EQ", full, b""), ("NE", full, b""),
                         ("CONTAINS", full, b""), ("PREFIX", full, b""),
                         ("CONTAINS2", A20, B20),
                         ("NOT_CONTAINS2", A20, B20)):
            pred = _vpred(P, 0, op, a, b)
            assert pred.slen + (pred.ival if op in TWO else 0) == 40
            exp = R.pred_rows(op, strings, a, b)
            assert 0 < len(exp) < len(strings)
            assert _rows(P, pl, page, [pred]) == exp, (layout, op)


@pytest.fixture(scope="module")
def chained_table(P, pl):
    """A chained build over keys 1..97 with payload 10 * key."""
    k = np.arange(1, 98, dtype=np.int64)
    b = P.Operator(P.OP_HASH_BUILD,
                   pl.hash_build(0, payload=[1], capacity_hint=97))
    b.feed(P.Page({"k": k, "p": k * 10}))
    b.finish()
    tbl = b.table()
    yield tbl
    P.lib().c.pg_table_destroy(tbl)
    b.destroy()


@pytest.mark.parametrize("layout", ["raw", "dict"])
def test_varbin_emit_rejected_outside_filter_project(P, pl, chained_table,
                                                     layout):
    """PARTITION and the mode-0 LOOKUP_JOIN copy fixed-width values: a
    VARBIN emit column fails add_input, naming the entry, and the operator
    stays usable."""
    n = 200
    rid = np.arange(n, dtype=np.int64)
    key = rid % 120 + 1
    bad = _vpage(P, layout, STR_A[:n], {"rid": rid, "k": key})
    good = P.Page({"x": rid * 3, "rid": rid, "k": key})
    op = P.Operator(P.OP_PARTITION, pl.partition(5, 1, [1, 0]))
    try:
        _feed_fails(op, bad, "PARTITION", "emit_cols[1]", "VARBIN")
        assert op.get_output() is None
        op.feed(good)
        pages = [op.get_output(["rid", "x"]) for _ in range(5)]
        assert sum(op.partition_counts(5)) == n
    finally:
        op.destroy()
    got = sorted(r for pg in pages for r in pg["rid"].tolist())
    assert got == rid.tolist()
    assert all((pg["x"] == pg["rid"] * 3).all() for pg in pages)
    op = P.Operator(P.OP_LOOKUP_JOIN, pl.emit_join(chained_table, 2, [1, 0]))
    try:
        _feed_fails(op, bad, "LOOKUP_JOIN", "emit_probe_cols[1]", "VARBIN")
        assert op.get_output() is None
        op.feed(good)
        out = op.get_output(["rid", "x", "p"])
    finally:
        op.destroy()
    hit = key <= 97
    assert out["rid"].tolist() == rid[hit].tolist()
    assert out["x"].tolist() == (rid[hit] * 3).tolist()
    assert out["p"].tolist() == (key[hit] * 10).tolist()


def test_op_and_column_type_must_agree(P, pl, chained_table):
    """An ordering op on a VARBIN column, and a string op on a fixed-width
    one, fail add_input naming the predicate; the operator stays usable."""
    n = 100
    rid = np.arange(n, dtype=np.int64)
    g = (rid % 3 + 1).astype(np.uint8)
    strings = STR_A[:n]
    fixed = {"u8": g, "i32": rid.astype(np.int32), "i64": rid,
             "f64": rid.astype(np.float64)}
    # FILTER_PROJECT, every combination; the same plan then takes a page
    # whose column 0 has the type the op is defined for
    for layout in LAYOUTS:
        vb = _vpage(P, layout, strings, {"rid": rid, "g": g})
        for cmp_ in (P.CMP_LT, P.CMP_LE, P.CMP_GT, P.CMP_GE):
            op = P.Operator(P.OP_FILTER_PROJECT, pl.filter_project(
                [pl.ident(1)], preds=[pl.pred(0, cmp_, 50)]))
            try:
                _feed_fails(op, vb, "FILTER_PROJECT", "preds[0]", "VARBIN")
                op.feed(P.Page({"v": rid, "rid": rid}))
                exp = {P.CMP_LT: rid < 50, P.CMP_LE: rid <= 50,
                       P.CMP_GT: rid > 50, P.CMP_GE: rid >= 50}[cmp_]
                assert op.get_output()["c0"].tolist() == rid[exp].tolist()
            finally:
                op.destroy()
    vb = _vpage(P, "raw", strings, {"rid": rid, "g": g})
    for sop in ("CONTAINS", "PREFIX") + TWO:
        for tname, col in fixed.items():
            op = P.Operator(P.OP_FILTER_PROJECT, pl.filter_project(
                [pl.ident(1)], preds=[pl.pred(1, P.CMP_GE, 0),
                                      _vpred(P, 0, sop, b"ab", b"b")]))
            try:
                _feed_fails(op, P.Page({"v": col, "rid": rid}),
                            "FILTER_PROJECT", "preds[1]", "fixed-width")
                op.feed(vb)
                assert op.get_output()["c0"].tolist() == \
                    R.pred_rows(sop, strings, b"ab", b"b"), (sop, tname)
            finally:
                op.destroy()
    # the other operators that carry preds[]: one case of each kind
    num = P.Page({"v": rid, "rid": rid, "g": g})
    for name, kind in _op_kinds(P).items():
        if name == "FILTER_PROJECT":
            continue
        for pred, page, what in ((pl.pred(0, P.CMP_LT, 5), vb, "VARBIN"),
                                 (_vpred(P, 0, "CONTAINS", b"a"), num,
                                  "fixed-width")):
            plan = _with_pred(P, pl, kind, pred)
            if kind == P.OP_LOOKUP_JOIN:
                plan.table = chained_table
            op = P.Operator(kind, plan)
            try:
                _feed_fails(op, page, name, "preds[0]", what)
            finally:
                op.destroy()
    # GROUPBY_MULTI checks its per-aggregate FILTERs too
    op = P.Operator(P.OP_GROUPBY_MULTI,
                    _with_pred(P, pl, P.OP_GROUPBY_MULTI,
                               pl.pred(0, P.CMP_GT, 5), as_filter=True))
    try:
        _feed_fails(op, vb, "GROUPBY_MULTI", "preds[0]", "VARBIN")
        op.feed(num)
        op.finish()
        out = op.get_output(["g", "cnt_flt", "cnt"])
    finally:
        op.destroy()
    assert {k: (f, c) for k, f, c in zip(out["g"].tolist(),
                                         out["cnt_flt"].tolist(),
                                         out["cnt"].tolist())} == \
        {k: (int(((g == k) & (rid > 5)).sum()), int((g == k).sum()))
         for k in (1, 2, 3)}


def test_all_empty_column_with_null_byte_buffer(P, pl):
    """A host VARBIN column whose strings are all empty may come with
    data = NULL: its offsets are staged all the same."""
    from presto_amd.engine import PgPage, T_VARBIN, T_I64
    n = 300
    rid = np.arange(n, dtype=np.int64)
    offs = np.zeros(n + 1, np.int32)
    cp = PgPage()
    cp.n_rows, cp.n_cols = n, 2
    cp.cols[0].tag = T_VARBIN
    cp.cols[0].data = None
    cp.cols[0].offsets = offs.ctypes.data
    cp.cols[1].tag = T_I64
    cp.cols[1].data = rid.ctypes.data
    assert not cp.cols[0].data and not cp.cols[0].on_device
    assert _rows(P, pl, cp, [_vpred(P, 0, "EQ", b"")]) == rid.tolist()
    assert _rows(P, pl, cp, [_vpred(P, 0, "CONTAINS", b"a")]) == []
    assert _rows(P, pl, cp, [_vpred(P, 0, "NE", b"")]) == []
    out = _filter(P, pl.filter_project([pl.ident(0), pl.ident(1)]), cp)
    assert out["c0"].offsets.tolist() == [0] * (n + 1)
    assert len(out["c0"].data) == 0
    assert out["c1"].tolist() == rid.tolist()
