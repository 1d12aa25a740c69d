"""GPU edge tests — signed values, NaN/inf, null masks and tile / grid-pass
boundaries of the expression kernels, operator by operator through the
C-ABI.  References are the plain numpy/Python ones of tests/edge_refs.py
(self-checked on the CPU by tests/test_edge_refs.py).

Every assertion is exact: integer equality or equality of float bit
patterns.  Shapes are the smallest at which the kernel can still go wrong.
"""
import itertools

import numpy as np
import pytest

import edge_refs as R  # tests/ is on sys.path (pytest's rootdir import mode)

pytestmark = pytest.mark.gpu

VL = R.VL
I32_MIN, I32_MAX = -2**31, 2**31 - 1
I64_MIN1, I64_MAX = -2**63 + 1, 2**63 - 1
SUBNORMAL = 5e-324


@pytest.fixture(scope="module")
def P():
    import presto_amd
    return presto_amd


@pytest.fixture(scope="module")
def pl():
    from presto_amd import plans
    return plans


@pytest.fixture(scope="module")
def li01(oracle_lib):
    return oracle_lib.gen_lineitem(0.1)


# ---------------- plumbing ----------------

def _cpage(P, cols, nulls=None):
    """(Page, raw PgPage with the null masks attached).  The caller keeps
    both alive for the call — input pages are borrowed."""
    page = P.Page(cols)
    cp = page.to_c()
    for name, mask in (nulls or {}).items():
        assert mask.dtype == np.uint8 and len(mask) == page.n_rows
        cp.cols[page.channel(name)].null_mask = mask.ctypes.data
    return page, cp


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


def _agg_table(P, pl, keys):
    """A finished agg_table build over unique i64 keys: (op, table)."""
    b = P.Operator(P.OP_HASH_BUILD,
                   pl.hash_build(0, capacity_hint=len(keys) + 16,
                                 agg_table=1))
    b.add_input(P.Page({"k": keys}))
    b.finish()
    return b, b.table()


def _drop_table(P, b, table):
    P.lib().c.pg_table_destroy(table)
    b.destroy()


def _pred(P, col, op, ival=0, dval=0.0, rhs=None):
    p = P.Pred(col, op, int(ival), float(dval))
    if rhs is not None:
        p.rhs_col = rhs + 1
    return p


def _same_bytes(a, b):
    return a.dtype == b.dtype and a.shape == b.shape and \
        a.tobytes() == b.tobytes()


# ---------------- a. predicate matrix ----------------

N_PRED = 1000


@pytest.fixture(scope="module")
def pred_data():
    """One 1000-row page: a row id, an lhs and an rhs column per type (the
    rhs twins equal their lhs on a third of the rows so EQ/NE/LE/GE meet
    ties), edge values in every column, and a null mask on ~1/7 of the
    rows of each (different rows per column)."""
    rng = np.random.default_rng(101)
    n = N_PRED

    def with_edges(base, edges, stride):
        out = base.copy()
        e = np.array(edges, base.dtype)
        pos = (np.arange(len(e) * 6) * stride + 1) % n
        out[pos] = np.tile(e, 6)
        return out

    u8 = with_edges(rng.integers(0, 256, n).astype(np.uint8), [0, 1, 255], 7)
    i32 = with_edges(rng.integers(-1000, 1000, n).astype(np.int32),
                     [0, 1, -1, 255, I32_MIN, I32_MAX], 11)
    i64 = with_edges(rng.integers(-10**12, 10**12, n),
                     [0, 1, -1, 255, I32_MIN, I32_MAX, I64_MIN1, I64_MAX],
                     13)
    f64 = with_edges(rng.standard_normal(n) * 100,
                     [0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan,
                      SUBNORMAL, 255.0, float(I32_MAX)], 17)
    # rhs twins: no int64 extremes, so rhs + const never overflows
    u8b = with_edges(rng.integers(0, 256, n).astype(np.uint8), [0, 1, 255], 5)
    i32b = with_edges(rng.integers(-1000, 1000, n).astype(np.int32),
                      [0, 1, -1, 255, I32_MIN, I32_MAX], 19)
    i64b = with_edges(rng.integers(-10**12, 10**12, n),
                      [0, 1, -1, 255, I32_MIN, I32_MAX], 23)
    f64b = with_edges(rng.standard_normal(n) * 100,
                      [0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan,
                       SUBNORMAL, 255.0], 29)
    tie = np.arange(n) % 3 == 0
    u8b[tie] = u8[tie]
    i32b[tie] = i32[tie]
    t64 = tie & (np.abs(i64) <= 10**12)
    i64b[t64] = i64[t64]
    f64b[tie] = f64[tie]
    cols = {"rid": np.arange(n, dtype=np.int64), "u8": u8, "i32": i32,
            "i64": i64, "f64": f64, "u8b": u8b, "i32b": i32b, "i64b": i64b,
            "f64b": f64b,
            "g": (np.arange(n) % 3 + 1).astype(np.uint8)}
    nulls = {name: ((np.arange(n) + 3 * j) % 7 == 0).astype(np.uint8)
             for j, name in enumerate(("u8", "i32", "i64", "f64", "u8b",
                                       "i32b", "i64b", "f64b"))}
    return cols, nulls


CONSTS = {
    "u8": [0, 1, -1, 255, 256],
    "i32": [0, 1, -1, 255, I32_MIN, I32_MAX],
    "i64": [0, 1, -1, 255, I32_MIN, I32_MAX, I64_MIN1, I64_MAX],
    "f64": [0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, SUBNORMAL],
}
# (lhs, rhs column, constant): same type with 0, then another type with a
# non-zero constant (|const| <= 10^6)
RHS_CASES = [
    ("u8", "u8b", 0), ("u8", "i32b", 3), ("u8", "i64b", -200),
    ("i32", "i32b", 0), ("i32", "i64b", -7), ("i32", "u8b", -128),
    ("i64", "i64b", 0), ("i64", "i32b", -10**6), ("i64", "u8b", 10**6),
    ("f64", "f64b", 0.0), ("f64", "i32b", 2.5), ("f64", "i64b", -0.5),
    ("f64", "u8b", 0.0),
]


def _pred_case(P, cols, nulls, names, lhs, rhs, const, op):
    """(pg_pred, expected row mask) of `lhs op const` or
    `lhs op rhs + const`."""
    is_f = lhs == "f64"
    kw = {"dval": const} if is_f else {"ival": const}
    if rhs is None:
        x = np.float64(const) if is_f else np.int64(const)
        return (_pred(P, names.index(lhs), op, **kw),
                R.pred_ref(op, cols[lhs], x, nulls.get(lhs)))
    if is_f:
        x = cols[rhs].astype(np.float64) + np.float64(const)
    else:
        x = cols[rhs].astype(np.int64) + np.int64(const)
    return (_pred(P, names.index(lhs), op, rhs=names.index(rhs), **kw),
            R.pred_ref(op, cols[lhs], x, nulls.get(lhs), nulls.get(rhs)))


def _all_pred_cases(lhs_types):
    for lhs in lhs_types:
        for c in CONSTS[lhs]:
            yield lhs, None, c
    for lhs, rhs, c in RHS_CASES:
        if lhs in lhs_types:
            yield lhs, rhs, c


@pytest.mark.parametrize("lhs", ["u8", "i32", "i64", "f64"])
def test_predicate_matrix_filter(P, pl, pred_data, lhs):
    """FILTER_PROJECT emitting the row id: every op x (edge constants,
    same-type rhs column, other-type rhs column + constant), null masks on
    both sides."""
    cols, nulls = pred_data
    names = list(cols)
    page, cp = _cpage(P, cols, nulls)
    n_sel = 0
    for (l, rhs, const), op in itertools.product(_all_pred_cases([lhs]),
                                                 range(6)):
        pred, exp = _pred_case(P, cols, nulls, names, l, rhs, const, op)
        out = _filter(P, pl.filter_project([pl.ident(0)], preds=[pred]), cp)
        assert np.array_equal(out["c0"], cols["rid"][exp]), \
            (l, rhs, const, R.OPS[op])
        n_sel += int(exp.sum())
    assert n_sel > 0


def test_predicate_conjunction_null_masks_differ(P, pl, pred_data):
    cols, nulls = pred_data
    names = list(cols)
    page, cp = _cpage(P, cols, nulls)
    p0, m0 = _pred_case(P, cols, nulls, names, "i32", None, -5, P.CMP_GE)
    p1, m1 = _pred_case(P, cols, nulls, names, "f64", "i64b", -0.5,
                        P.CMP_NE)
    assert (nulls["i32"] != nulls["f64"]).any()
    out = _filter(P, pl.filter_project([pl.ident(0)], preds=[p0, p1]), cp)
    assert np.array_equal(out["c0"], cols["rid"][m0 & m1])
    assert 0 < (m0 & m1).sum() < min(m0.sum(), m1.sum())


@pytest.mark.parametrize("lhs", ["i64", "f64"])
def test_predicate_matrix_in_agg_kernels(P, pl, pred_data, lhs):
    """The same predicates as the HASH_AGG_SMALL pre-filter (one u8 key:
    not the Q1 shape) and as a GROUPBY_MULTI per-aggregate FILTER: COUNT
    per group must equal pred_ref — null exclusion inside those kernels."""
    cols, nulls = pred_data
    names = list(cols)
    g = cols["g"]
    gch = names.index("g")
    page, cp = _cpage(P, cols, nulls)
    for (l, rhs, const), op in itertools.product(_all_pred_cases([lhs]),
                                                 range(6)):
        pred, exp = _pred_case(P, cols, nulls, names, l, rhs, const, op)
        want = {k: int((exp & (g == k)).sum()) for k in (1, 2, 3)}
        tag = (l, rhs, const, R.OPS[op])
        out = _run(P, P.OP_HASH_AGG_SMALL,
                   pl.small_agg([pl.count()], preds=[pred],
                                keys=[(gch, [1, 2, 3])]), [cp],
                   ["g", "cnt"])
        got = dict(zip(out["g"].tolist(), out["cnt"].tolist()))
        assert got == {k: v for k, v in want.items() if v}, tag
        out = _run(P, P.OP_GROUPBY_MULTI,
                   pl.group_by([gch], [(pl.count(), 0)], 16,
                               filters=[pred]), [cp],
                   ["g", "cnt_flt", "cnt"])
        got = {k: (f, c) for k, f, c in zip(out["g"].tolist(),
                                            out["cnt_flt"].tolist(),
                                            out["cnt"].tolist())}
        assert got == {k: (want[k], int((g == k).sum()))
                       for k in (1, 2, 3)}, tag


# ---------------- b. projection matrix ----------------

N_PROJ = 513  # two 256-row windows + 1


@pytest.fixture(scope="module")
def proj_data():
    rng = np.random.default_rng(202)
    n = N_PROJ
    f_edges = [0.0, -0.0, 1.0, -1.0, np.inf, -np.inf, np.nan, SUBNORMAL,
               0.07, 1e300, -1e300]

    def f64col(seed):
        v = np.random.default_rng(seed).standard_normal(n) * 1000
        v[np.arange(len(f_edges)) * 5 + seed % 5] = f_edges
        return v

    cols = {
        "u8": rng.integers(0, 256, n).astype(np.uint8),
        "i32": rng.integers(-10**6, 10**6, n).astype(np.int32),
        "i64": rng.integers(-10**12, 10**12, n),
        "f64": f64col(1),
        "u8b": rng.integers(0, 11, n).astype(np.uint8),
        "i32b": rng.integers(-3, 4, n).astype(np.int32),      # zeros: x/0
        "i64b": rng.integers(-10**6, 10**6, n),
        "f64b": f64col(2),
        "u8c": rng.integers(0, 9, n).astype(np.uint8),
        "i64c": rng.integers(-10**9, 10**9, n),
        "i32c": rng.integers(-50, 50, n).astype(np.int32),
        "f64c": rng.integers(0, 9, n) / 100.0,
        # small non-negative key parts: (a << 40) | b stays inside int64
        "ku8": rng.integers(0, 256, n).astype(np.uint8),
        "ki32": rng.integers(0, 2**20, n).astype(np.int32),
        "ki64": rng.integers(0, 2**22, n),
    }
    cols["u8"][:3] = [0, 1, 255]
    cols["i32"][:4] = [0, -1, I32_MIN, I32_MAX]
    cols["i64"][:4] = [0, -1, -10**12, 10**12]
    cols["i64b"][:3] = [0, -1, 1]
    return cols


def _run_projs(P, pl, cols, cases):
    """cases: (label, Proj, expected array).  Runs them 16 per operator and
    checks output tag (dtype) and values."""
    page = P.Page(cols)
    for lo in range(0, len(cases), 16):
        part = cases[lo:lo + 16]
        out = _filter(P, pl.filter_project([c[1] for c in part]), page)
        for j, (label, _, exp) in enumerate(part):
            got = out[f"c{j}"]
            assert got.dtype == exp.dtype and len(got) == N_PROJ, label
            if exp.dtype == np.float64:
                assert R.same_f64(got, exp), label
            else:
                assert np.array_equal(got, exp), label


def test_projection_matrix(P, pl, proj_data):
    """All nine projection kinds over the input-type combinations they
    accept: IDENT and the four float kinds take any numeric type per
    operand; the integer key kinds take integer channels."""
    cols = proj_data
    names = list(cols)
    ch = names.index
    num_a = ["u8", "i32", "i64", "f64"]
    num_b = ["u8b", "i32b", "i64b", "f64b"]
    ints_a = ["u8", "i32", "i64"]
    keys = ["ku8", "ki32", "ki64"]
    cases = []
    for a in num_a + ["f64b"]:
        cases.append((("IDENT", a), pl.ident(ch(a)),
                      R.proj_ref(R.IDENT, cols[a])))
    for a, b in itertools.product(num_a, num_b):
        for kind, name in ((R.MUL, "MUL"), (R.DIV, "DIV"),
                           (R.DISC_PRICE, "DISC_PRICE")):
            cases.append(((name, a, b), P.Proj(kind, ch(a), ch(b), 0),
                          R.proj_ref(kind, cols[a], cols[b])))
    # DIV by +-0.0 / 0 is in there: make sure the reference met it
    with np.errstate(all="ignore"):
        q = cols["f64"] / cols["f64b"]
        assert np.isinf(cols["i64"] / cols["i32b"].astype(np.float64)).any()
    assert np.isnan(q).any() and np.isinf(q).any()
    for a, b, c in itertools.product(num_a, num_b,
                                     ["u8c", "i32c", "i64c", "f64c"]):
        cases.append((("CHARGE", a, b, c), pl.charge(ch(a), ch(b), ch(c)),
                      R.proj_ref(R.CHARGE, cols[a], cols[b], cols[c])))
    for a, b in itertools.product(keys, keys):
        for shift in (0, 40):
            cases.append((("KEYSHL", a, b, shift),
                          pl.keyshl(ch(a), ch(b), shift),
                          R.proj_ref(R.KEYSHL, cols[a], cols[b], shift)))
        for shift, dv in ((14, 7), (8, 0), (0, 1)):
            cases.append((("KEYSHL_DIV", a, b, shift, dv),
                          pl.keyshl_div(ch(a), ch(b), shift, dv),
                          R.proj_ref(R.KEYSHL_DIV, cols[a], cols[b],
                                     (shift << 16) | dv)))
    # a derived dimension with negative values divides toward zero
    for b in ("i32", "i64b"):
        cases.append((("KEYSHL_DIV", "ki32", b, 14, 7),
                      pl.keyshl_div(ch("ki32"), ch(b), 14, 7),
                      R.proj_ref(R.KEYSHL_DIV, cols["ki32"], cols[b],
                                 (14 << 16) | 7)))
    for a in ints_a:
        for shift in (0, 3, 40):
            cases.append((("SHR", a, shift),
                          P.Proj(P.PROJ_SHR, ch(a), 0, shift),
                          R.proj_ref(R.SHR, cols[a], c=shift)))
        for b, c in ((100, 7), (-5, 7), (10**6, 0), (3, 1), (300, 2)):
            cases.append((("SUBDIV", a, b, c), pl.subdiv(ch(a), b, c),
                          R.proj_ref(R.SUBDIV, cols[a], b, c)))
    assert (cols["i64"] >> 3 < 0).any() and (cols["i32"] - 100 < 0).any()
    assert {c[1].kind for c in cases} == set(range(9))
    _run_projs(P, pl, cols, cases)


# ---------------- c. selection / compaction row-count sweep ----------------

SWEEP_N = [0, 1, 63, 64, 65, 191, 192, 193, 255, 256, 257, 1023, 1025,
           262143, 262144, 262145, 262401]


def _varbin(P, n):
    """Vectorized host VARBIN column: row i holds 1 + i % 5 bytes."""
    lens = (1 + np.arange(n) % 5).astype(np.int32)
    offs = np.zeros(n + 1, np.int32)
    np.cumsum(lens, out=offs[1:])
    row = np.repeat(np.arange(n), lens)
    data = ((row * 7 + np.arange(len(row))) % 251).astype(np.uint8)
    return P.Varbin.from_arrays(data, offs), lens, row


@pytest.mark.parametrize("n", SWEEP_N)
def test_selection_row_count_sweep(P, pl, n):
    """count + scan + emit at the 64-row wave and 256-row window edges and
    across the chunk 256 -> 512 switch (n > 1024 * 256): row-ascending
    order and exact contents of an I64, a U8 and a VARBIN column."""
    i = np.arange(n)
    a = (i * 1_000_003 - 5 * 10**11).astype(np.int64)
    u = (i % 251).astype(np.uint8)
    vb, lens, byte_row = _varbin(P, n)
    patterns = {
        "all": np.ones(n, bool), "none": np.zeros(n, bool),
        "odd": i % 2 == 1, "last": i == n - 1,
        "lanes0_63": (i % 64 == 0) | (i % 64 == 63)}
    plan = pl.filter_project([pl.ident(0), pl.ident(1), pl.ident(2)],
                             preds=[pl.pred(3, P.CMP_EQ, 1)])
    for name, sel in patterns.items():
        page = P.Page({"a": a, "u": u, "v": vb,
                       "s": sel.astype(np.uint8)}, n_rows=n)
        out = _filter(P, plan, page, ["a", "u", "v"])
        assert np.array_equal(out["a"], a[sel]), name
        assert np.array_equal(out["u"], u[sel]), name
        exp_offs = np.zeros(int(sel.sum()) + 1, np.int32)
        np.cumsum(lens[sel], out=exp_offs[1:])
        assert np.array_equal(out["v"].offsets, exp_offs), name
        assert np.array_equal(out["v"].data, vb.data[sel[byte_row]]), name


# ---------------- d. signed decimal ticks ----------------

N_DEC = 4099
DEC_GROUPS = 97


@pytest.fixture(scope="module")
def dec_data():
    rng = np.random.default_rng(303)
    n = N_DEC
    k = rng.integers(-10**6, 10**6 + 1, n)
    k[:5] = [-1, -50, -99999, 10**6, -10**6]
    yk = rng.integers(-1000, 1001, n)       # signed second MUL operand
    dk = rng.integers(0, 11, n)
    tk = rng.integers(0, 11, n)
    x, cents = R.ticks_exact(k, 2)
    y, ycents = R.ticks_exact(yk, 2)
    d, dd = R.ticks_exact(dk, 2)
    t, tt = R.ticks_exact(tk, 2)
    assert (k < 0).sum() > n // 3 and (k > 0).sum() > n // 3
    gk = rng.integers(1, DEC_GROUPS + 1, n)
    gk[:DEC_GROUPS] = np.arange(1, DEC_GROUPS + 1)
    ticks = {"ident": cents, "disc": R.disc_price_ticks(cents, dd),
             "charge": R.charge_ticks(cents, dd, tt),
             "mul": R.mul_ticks(cents, ycents)}
    cols = {"gk": gk, "g8": (gk % 3 + 1).astype(np.uint8), "x": x, "d": d,
            "t": t, "y": y}
    return cols, ticks


def _dec_aggs(P, pl):
    """[(name, Agg, ticks key, reduce)] over channels x=2, d=3, t=4, y=5."""
    return [
        ("ident", pl.sum_dec(pl.ident(2), 2), "ident", sum),
        ("disc", pl.sum_dec(pl.disc_price(2, 3), 4), "disc", sum),
        ("charge", pl.sum_dec(pl.charge(2, 3, 4), 6), "charge", sum),
        ("mul", pl.sum_dec(pl.mul(2, 5), 4), "mul", sum),
        ("min", P.Agg(P.AGG_MIN, pl.ident(2), 2), "ident", min),
        ("max", P.Agg(P.AGG_MAX, pl.ident(2), 2), "ident", max),
    ]


def test_signed_ticks_small_agg(P, pl, dec_data):
    """HASH_AGG_SMALL decimal mode (one u8 key: generic kernel), hi/lo."""
    cols, ticks = dec_data
    aggs = _dec_aggs(P, pl)
    names = ["g"]
    for nm, *_ in aggs:
        names += [nm + "_hi", nm + "_lo"]
    out = _run(P, P.OP_HASH_AGG_SMALL,
               pl.small_agg([a[1] for a in aggs] + [pl.count()],
                            keys=[(1, [1, 2, 3])]),
               [P.Page(cols)], names + ["cnt"])
    assert out["g"].tolist() == [1, 2, 3]
    for nm, _, tk, red in aggs:
        exp = R.group_int(cols["g8"], ticks[tk], reduce=red)
        got = {g: R.i128(h, l) for g, h, l in
               zip(out["g"].tolist(), out[nm + "_hi"], out[nm + "_lo"])}
        assert got == exp, nm


def test_signed_ticks_groupby_multi(P, pl, dec_data):
    cols, ticks = dec_data
    aggs = _dec_aggs(P, pl)
    out = _run(P, P.OP_GROUPBY_MULTI,
               pl.group_by([0], [a[1] for a in aggs], DEC_GROUPS),
               [P.Page(cols)], ["gk"] + [a[0] for a in aggs] + ["cnt"])
    assert sorted(out["gk"].tolist()) == list(range(1, DEC_GROUPS + 1))
    for nm, _, tk, red in aggs:
        exp = R.group_int(cols["gk"], ticks[tk], reduce=red)
        assert dict(zip(out["gk"].tolist(), out[nm].tolist())) == exp, nm


def test_signed_ticks_lookup_join(P, pl, dec_data):
    """LOOKUP_JOIN mode 1 on a 97-key agg_table: the single-projection form
    (dec_scale 4, sum and dec_min) and the multi-aggregate form."""
    cols, ticks = dec_data
    page = P.Page(cols)
    keys = np.arange(1, DEC_GROUPS + 1, dtype=np.int64)
    # DISC_PRICE over f64 columns with dec_scale 4 is the shape the
    # specialized Q3 probe kernel takes for sums; MUL takes the generic one
    for tk, proj in (("disc", pl.disc_price(2, 3)), ("mul", pl.mul(2, 5))):
        for nm, fields, red in (("sum", dict(dec_only=1), sum),
                                ("min", dict(dec_min=1), min)):
            b, tbl = _agg_table(P, pl, keys)
            try:
                out = _run(P, P.OP_LOOKUP_JOIN,
                           pl.agg_join(tbl, 0, proj, dec_scale=4, **fields),
                           [page])
            finally:
                _drop_table(P, b, tbl)
            exp = R.group_int(cols["gk"], ticks[tk], reduce=red)
            assert dict(zip(out["c0"].tolist(), out["c1"].tolist())) == exp, \
                (tk, nm)
    b, tbl = _agg_table(P, pl, keys)
    try:
        out = _run(P, P.OP_LOOKUP_JOIN,
                   pl.lookup_join(tbl, 0, 1, aggs=[
                       pl.sum_dec(pl.ident(2), 2),
                       pl.sum_dec(pl.disc_price(2, 3), 4),
                       pl.sum_dec(pl.charge(2, 3, 4), 6),
                       pl.sum_dec(pl.mul(2, 5), 4)]), [page],
                   ["k", "ident", "disc", "charge", "mul", "cnt"])
    finally:
        _drop_table(P, b, tbl)
    for nm in ("ident", "disc", "charge", "mul"):
        exp = R.group_int(cols["gk"], ticks[nm])
        assert dict(zip(out["k"].tolist(), out[nm].tolist())) == exp, nm
    assert dict(zip(out["k"].tolist(), out["cnt"].tolist())) == \
        R.group_int(cols["gk"], [1] * N_DEC)


# ---------------- e. SUM_F64 domain ----------------

@pytest.fixture(scope="module")
def f64_data():
    rng = np.random.default_rng(404)
    ng, per = 300, 30
    keys = np.repeat(np.arange(1, ng + 1), per)
    vals = rng.integers(1, 10**9 + 1, ng * per) / 100.0
    keys = np.concatenate([keys, np.full(64, ng + 1), np.full(41, ng + 2)])
    vals = np.concatenate([vals, np.full(64, 2.0**52 + 0.5),
                           2.0**-12 * (1 + np.arange(41) / 1024)])
    perm = rng.permutation(len(keys))
    return keys[perm].astype(np.int64), vals[perm]


def _sum_f64_groupby(P, pl, keys, vals):
    out = _run(P, P.OP_GROUPBY_MULTI,
               pl.group_by([0], [pl.sum_f64(pl.ident(1))], len(keys)),
               [P.Page({"k": keys, "v": vals})], ["k", "s", "cnt"])
    return dict(zip(out["k"].tolist(), R.bits(out["s"]).tolist()))


def _sum_f64_join(P, pl, keys, vals):
    b, tbl = _agg_table(P, pl, np.unique(keys))
    try:
        out = _run(P, P.OP_LOOKUP_JOIN,
                   pl.agg_join(tbl, 0, pl.ident(1), dec_scale=0),
                   [P.Page({"k": keys, "v": vals})],
                   ["k", "dec", "s", "cnt"])
    finally:
        _drop_table(P, b, tbl)
    return dict(zip(out["k"].tolist(), R.bits(out["s"]).tolist()))


@pytest.mark.parametrize("via", ["groupby", "join"])
def test_sum_f64_in_domain_is_fsum(P, pl, f64_data, via):
    """Inside the documented domain the result is the exact sum rounded
    once, bit for bit — including 64 x (2^52 + 0.5) and addends at the
    2^-12 resolution limit."""
    keys, vals = f64_data
    run = _sum_f64_groupby if via == "groupby" else _sum_f64_join
    got = run(P, pl, keys, vals)
    exp = {k: int(R.bits(v)) for k, v in R.fsum_groups(keys, vals).items()}
    assert len(exp) == 302
    assert got == exp


@pytest.mark.parametrize("via", ["groupby", "join"])
@pytest.mark.parametrize("bad", [-0.01, np.nan, 2.0**53, 2.0**-70],
                         ids=["negative", "nan", "2p53", "2m70"])
def test_sum_f64_out_of_domain_raises(P, pl, via, bad):
    """One addend outside the 64.64 domain in an otherwise valid page is
    an operator error naming SUM_F64, not a silently dropped row."""
    keys = (np.arange(100) % 5 + 1).astype(np.int64)
    vals = np.arange(1, 101) / 4.0
    run = _sum_f64_groupby if via == "groupby" else _sum_f64_join
    exp = {k: int(R.bits(v)) for k, v in R.fsum_groups(keys, vals).items()}
    assert run(P, pl, keys, vals) == exp        # the page itself is valid
    vals = vals.copy()
    vals[37] = bad
    with pytest.raises(RuntimeError, match="SUM_F64"):
        run(P, pl, keys, vals)


def test_sum_f64_domain_in_q3_shape_probe(P, pl):
    """Mode 1 DISC_PRICE over f64 columns with dec_scale 4 takes the
    specialized Q3 probe kernel; it keeps the same SUM_F64 contract."""
    rng = np.random.default_rng(707)
    n = 3001
    keys = rng.integers(1, 50, n)
    price = rng.integers(100, 10**7, n) / 100.0
    disc = rng.integers(0, 11, n) / 100.0

    def run(price):
        b, tbl = _agg_table(P, pl, np.unique(keys))
        try:
            out = _run(P, P.OP_LOOKUP_JOIN,
                       pl.agg_join(tbl, 0, pl.disc_price(1, 2), dec_scale=4),
                       [P.Page({"k": keys, "p": price, "d": disc})],
                       ["k", "dec", "s", "cnt"])
        finally:
            _drop_table(P, b, tbl)
        return dict(zip(out["k"].tolist(), R.bits(out["s"]).tolist()))

    exp = R.fsum_groups(keys, price * (1.0 - disc))
    assert run(price) == {k: int(R.bits(v)) for k, v in exp.items()}
    bad = price.copy()
    bad[n // 2] = -19.99
    with pytest.raises(RuntimeError, match="SUM_F64"):
        run(bad)


def _mode3(P, pl, okey, grp, probe_cols, **fields):
    """LOOKUP_JOIN mode 3: probe a chained build (orderkey -> i64 group
    payload) and accumulate into a second, agg-table keyed by the payload.
    Returns the groups page [key, sum_dec, sum_f64, cnt]."""
    b1 = P.Operator(P.OP_HASH_BUILD,
                    pl.hash_build(0, payload=[1], capacity_hint=len(okey)))
    b1.add_input(P.Page({"k": okey, "g": grp}))
    b1.finish()
    t1 = b1.table()
    b2, t2 = _agg_table(P, pl, np.unique(grp))
    try:
        return _run(P, P.OP_LOOKUP_JOIN,
                    pl.lookup_join(t1, 0, 3, table2=t2, **fields),
                    [P.Page(dict(k=okey, **probe_cols))],
                    ["g", "dec", "s", "cnt"])
    finally:
        _drop_table(P, b2, t2)
        _drop_table(P, b1, t1)


def test_mode3_signed_ticks_and_sum_f64_domain(P, pl, dec_data):
    """The star-join probe (k_probe_agg_pay) shares both fixes: signed
    CHARGE ticks per payload group, fsum-exact f64 sums inside the domain,
    and an error naming SUM_F64 for one negative addend."""
    cols, ticks = dec_data
    grp = cols["gk"]
    okey = np.arange(1, N_DEC + 1, dtype=np.int64) * 3
    out = _mode3(P, pl, okey, grp,
                 {k: cols[k] for k in ("x", "d", "t")},
                 proj=pl.charge(1, 2, 3), dec_scale=6, dec_only=1)
    assert dict(zip(out["g"].tolist(), out["dec"].tolist())) == \
        R.group_int(grp, ticks["charge"])
    assert dict(zip(out["g"].tolist(), out["cnt"].tolist())) == \
        R.group_int(grp, [1] * N_DEC)
    vals = np.abs(cols["x"])
    out = _mode3(P, pl, okey, grp, {"v": vals}, proj=pl.ident(1),
                 dec_scale=0)
    exp = {k: int(R.bits(v)) for k, v in R.fsum_groups(grp, vals).items()}
    assert dict(zip(out["g"].tolist(), R.bits(out["s"]).tolist())) == exp
    vals = vals.copy()
    vals[1234] = -0.01
    with pytest.raises(RuntimeError, match="SUM_F64"):
        _mode3(P, pl, okey, grp, {"v": vals}, proj=pl.ident(1), dec_scale=0)


# ---------------- f. small-key aggregation across grid passes ----------------

PASS_N = [1, 2, 3, 2 * VL - 1, 2 * VL, 2 * VL + 1, 2 * VL + 3]


@pytest.fixture(scope="module")
def pass_data(li01):
    """2*VL + 3 rows, generated once: a generic page (u8 key, cents value,
    int32 filter column) and SF0.1 lineitem tiled with np.resize (a prefix
    of the tiling is the tiling of the prefix)."""
    rng = np.random.default_rng(505)
    n = 2 * VL + 3
    kx = rng.integers(-10**6, 10**6 + 1, n)
    x, _ = R.ticks_exact(kx, 2)
    gen = {"k": rng.choice(np.array([5, 9], np.uint8), n), "x": x,
           "sd": rng.integers(0, 100, n).astype(np.int32)}
    gen["sd"][:3] = 0   # the 1..3-row pages select their rows
    names = ("quantity", "extendedprice", "discount", "tax", "shipdate",
             "returnflag", "linestatus")
    li = {k: np.resize(li01[k], n) for k in names}
    return gen, kx, li


@pytest.mark.parametrize("n", PASS_N)
def test_small_agg_generic_grid_passes(P, pl, pass_data, n):
    """Generic kernel, 1..3 rows and the rows around the second grid pass
    (thread v owns rows 2v, 2v+1, then 2v + 2*VL, ...): decimal mode exact
    against integer ticks, f64 mode bit-equal to the schedule replay."""
    gen, kx, _ = pass_data
    cols = {k: v[:n] for k, v in gen.items()}
    kx = kx[:n]
    page = P.Page(cols)
    sel = cols["sd"] < 60
    pred = pl.pred(2, P.CMP_LT, 60)
    keys = [(0, [5, 9])]
    dec = _run(P, P.OP_HASH_AGG_SMALL, pl.small_agg(
        [pl.sum_dec(pl.ident(1), 2), P.Agg(P.AGG_MIN, pl.ident(1), 2),
         P.Agg(P.AGG_MAX, pl.ident(1), 2), pl.count()],
        preds=[pred], keys=keys), [page],
        ["k", "s_hi", "s_lo", "mn_hi", "mn_lo", "mx_hi", "mx_lo", "cnt"])
    f64 = _run(P, P.OP_HASH_AGG_SMALL, pl.small_agg(
        [pl.sum_f64(pl.ident(1)), P.Agg(P.AGG_MIN, pl.ident(1), 0),
         P.Agg(P.AGG_MAX, pl.ident(1), 0), pl.count()],
        preds=[pred], keys=keys), [page], ["k", "s", "mn", "mx", "cnt"])
    present = [kv for kv in (5, 9) if (sel & (cols["k"] == kv)).any()]
    assert dec["k"].tolist() == present and f64["k"].tolist() == present
    for row, kv in enumerate(present):
        m = sel & (cols["k"] == kv)
        assert dec["cnt"][row] == f64["cnt"][row] == int(m.sum())
        assert R.i128(dec["s_hi"][row], dec["s_lo"][row]) == int(kx[m].sum())
        assert R.i128(dec["mn_hi"][row], dec["mn_lo"][row]) == kx[m].min()
        assert R.i128(dec["mx_hi"][row], dec["mx_lo"][row]) == kx[m].max()
        exp = R.butterfly_sum(np.where(m, cols["x"], 0.0))
        assert R.bits(f64["s"][row]) == R.bits(exp), (kv, f64["s"][row], exp)
        assert R.bits(f64["mn"][row]) == R.bits(cols["x"][m].min())
        assert R.bits(f64["mx"][row]) == R.bits(cols["x"][m].max())


Q1_F64_FIELDS = (("sum_qty", "f64_sum_qty"), ("sum_base", "f64_sum_base"),
                 ("sum_disc_price", "f64_sum_disc_price"),
                 ("sum_charge", "f64_sum_charge"),
                 ("sum_disc", "f64_sum_disc"))


def _assert_q1_equals_oracle(dec, f64, exp):
    assert len(dec["returnflag"]) == len(f64["returnflag"]) == len(exp)
    for i, g in enumerate(exp):
        for out in (dec, f64):
            assert out["returnflag"][i] == g.returnflag
            assert out["linestatus"][i] == g.linestatus
            assert out["count"][i] == g.count_order
        assert R.i128(dec["sum_qty_hi"][i], dec["sum_qty_lo"][i]) == \
            g.sum_qty_units
        assert R.i128(dec["sum_base_hi"][i], dec["sum_base_lo"][i]) == \
            g.sum_base_cents
        assert R.i128(dec["sum_disc_price_hi"][i],
                      dec["sum_disc_price_lo"][i]) == g.sum_disc_1e4
        assert R.i128(dec["sum_charge_hi"][i], dec["sum_charge_lo"][i]) == \
            R.i128(g.sum_charge_1e6_hi, g.sum_charge_1e6_lo)
        assert R.i128(dec["sum_disc_hi"][i], dec["sum_disc_lo"][i]) == \
            g.sum_disc_cents
        for name, field in Q1_F64_FIELDS:
            assert R.bits(f64[name][i]) == R.bits(getattr(g, field)), name


@pytest.mark.parametrize("n", PASS_N)
def test_q1_shape_grid_passes(P, oracle_lib, pass_data, n):
    """The Q1 fast path over the same row counts, against the oracle on
    the same tiled columns: decimal digits and f64 bits."""
    _, _, li = pass_data
    cols = {k: v[:n] for k, v in li.items()}
    page = P.Page(cols)
    before = _fast_launches(P)
    _assert_q1_equals_oracle(P.pipelines.q1(page, mode="dec"),
                             P.pipelines.q1(page, mode="f64"),
                             oracle_lib.q1(cols))
    assert _fast_launches(P) - before == 2   # both took the Q1 kernel


# ---------------- g. Q1 fast path against the generic kernel ----------------

Q1_COLS = ("quantity", "extendedprice", "discount", "tax", "shipdate",
           "returnflag", "linestatus")
QTY, EP, DC, TX, SD, RF, LS = range(7)


def _q1_like_plan(P, pl, mode, funcs, ship_max, extra_pred=None, drop=0):
    """The Q1 plan with the aggregate function of each of the five value
    slots chosen by `funcs` ('sum' | 'min' | 'max')."""
    sums = [(pl.ident(QTY), 0), (pl.ident(EP), 2),
            (pl.disc_price(EP, DC), 4), (pl.charge(EP, DC, TX), 6),
            (pl.ident(DC), 2)]
    sum_fn = P.AGG_SUM_DEC if mode == "dec" else P.AGG_SUM_F64
    fn = {"sum": sum_fn, "min": P.AGG_MIN, "max": P.AGG_MAX}
    aggs = [P.Agg(fn[f], proj, scale if mode == "dec" else 0)
            for f, (proj, scale) in zip(funcs, sums)]
    preds = [pl.pred(SD, P.CMP_LE, ship_max)]
    if extra_pred is not None:
        preds.append(extra_pred)
    return pl.small_agg(aggs + [pl.count()], preds=preds,
                        keys=[(RF, b"ANR"), (LS, b"FO")],
                        drop_unlisted_keys=drop)


def _q1_like_ref(cols, rows, mode, funcs):
    """numpy reference of _q1_like_plan over the row mask `rows`: rows of
    (returnflag, linestatus, five values, count) for non-empty groups.
    Decimal values are Python ints from the cents the TPC-H columns hold;
    f64 sums replay the schedule, f64 MIN/MAX are numpy's."""
    q, e, d, t = (cols[k] for k in Q1_COLS[:4])
    out = []
    if mode == "dec":
        qi, ci, di, ti = (np.rint(v * s).astype(np.int64)
                          for v, s in ((q, 1), (e, 100), (d, 100),
                                       (t, 100)))
        series = [qi, ci, ci * (100 - di), ci * (100 - di) * (100 + ti), di]
    else:
        dp = e * (1.0 - d)
        series = [q, e, dp, dp * (1.0 + t), d]
    for rf in b"ANR":
        for ls in b"FO":
            m = rows & (cols["returnflag"] == rf) & (cols["linestatus"] == ls)
            if not m.any():
                continue
            vals = []
            for f, v in zip(funcs, series):
                if f == "min":
                    vals.append(v[m].min())
                elif f == "max":
                    vals.append(v[m].max())
                elif mode == "dec":
                    vals.append(sum(int(x) for x in v[m]))
                else:
                    vals.append(R.butterfly_sum(np.where(m, v, 0.0)))
            if mode == "dec":
                vals = [int(x) for x in vals]
            else:
                vals = [int(R.bits(x)) for x in vals]
            out.append((rf, ls, vals, int(m.sum())))
    return out


def _q1_like_rows(out, mode):
    """An output page of _q1_like_plan in the form of _q1_like_ref."""
    rows = []
    for i in range(len(out["c0"])):
        if mode == "dec":
            vals = [R.i128(out[f"c{2 + 2 * a}"][i], out[f"c{3 + 2 * a}"][i])
                    for a in range(5)]
            cnt = out["c12"][i]
        else:
            vals = [int(R.bits(out[f"c{2 + a}"][i])) for a in range(5)]
            cnt = out["c7"][i]
        rows.append((int(out["c0"][i]), int(out["c1"][i]), vals, int(cnt)))
    return rows


def _fast_launches(P):
    """Pages sent to the specialized Q1 kernel so far (process-wide)."""
    import ctypes as C
    f = P.lib().c.pg_q1_fast_launches
    f.restype = C.c_int64
    return f()


def _q1_both_paths(P, pl, cols, nulls, mode, funcs, ship_max, drop=0, *,
                   fast):
    """Run the plan as written and with an always-true second predicate on
    shipdate (never the Q1 shape: generic k_agg_small<7,6>).  `fast` says
    whether the plan as written must take the specialized Q1 kernel — the
    launch counter pins it either way, so neither a plan the kernel does
    not implement nor plain Q1 can change paths unnoticed."""
    page, cp = _cpage(P, cols, nulls)
    always = pl.pred(SD, P.CMP_GE, I32_MIN)
    res = []
    for extra, want in ((None, int(fast)), (always, 0)):
        before = _fast_launches(P)
        out = _run(P, P.OP_HASH_AGG_SMALL,
                   _q1_like_plan(P, pl, mode, funcs, ship_max, extra, drop),
                   [cp])
        assert _fast_launches(P) - before == want
        res.append(_q1_like_rows(out, mode))
    return res


@pytest.fixture(scope="module")
def q1_cols(li01):
    return {k: np.ascontiguousarray(li01[k][:4097]) for k in Q1_COLS}


SUMS = ("sum",) * 5


@pytest.mark.parametrize("mode", ["dec", "f64"])
@pytest.mark.parametrize("n", [1, 4097])
@pytest.mark.parametrize("ship_max", [10471, I32_MAX],
                         ids=["q1date", "int32max"])
def test_q1_paths_odd_row_tail(P, pl, oracle_lib, q1_cols, n, ship_max,
                               mode):
    """Odd n leaves the last thread half a row pair; with a predicate
    constant of INT32_MAX nothing but the row count keeps the missing
    second row out."""
    cols = {k: v[:n] for k, v in q1_cols.items()}
    rows = cols["shipdate"] <= ship_max
    exp = _q1_like_ref(cols, rows, mode, SUMS)
    fast, generic = _q1_both_paths(P, pl, cols, None, mode, SUMS, ship_max,
                                   fast=True)
    assert fast == exp
    assert generic == exp
    if ship_max == 10471:   # the numpy reference itself, against the oracle
        o = oracle_lib.q1(cols)
        assert [(r[0], r[1], r[3]) for r in exp] == \
            [(g.returnflag, g.linestatus, g.count_order) for g in o]
        if mode == "dec":
            assert [r[2][3] for r in exp] == \
                [R.i128(g.sum_charge_1e6_hi, g.sum_charge_1e6_lo) for g in o]
        else:
            assert [r[2][3] for r in exp] == \
                [int(R.bits(g.f64_sum_charge)) for g in o]


@pytest.mark.parametrize("mode", ["dec", "f64"])
def test_q1_paths_null_mask_on_shipdate(P, pl, q1_cols, mode):
    """A null in the predicate column excludes the row on both paths."""
    n = 4097
    nulls = {"shipdate": (np.arange(n) % 7 == 2).astype(np.uint8)}
    rows = (q1_cols["shipdate"] <= 10471) & (nulls["shipdate"] == 0)
    exp = _q1_like_ref(q1_cols, rows, mode, SUMS)
    fast, generic = _q1_both_paths(P, pl, q1_cols, nulls, mode, SUMS, 10471,
                                   fast=False)
    assert fast == exp
    assert generic == exp


@pytest.mark.parametrize("mode", ["dec", "f64"])
def test_q1_paths_null_mask_on_money_channel(P, pl, q1_cols, mode):
    """Null masks are a predicate concept (presto_gpu.h, pg_col): an
    aggregate input with a mask is read as is on both paths, and a
    predicate on that channel — even an always-true one — drops its null
    rows."""
    n = 4097
    nulls = {"extendedprice": (np.arange(n) % 5 == 1).astype(np.uint8)}
    rows = q1_cols["shipdate"] <= 10471
    exp = _q1_like_ref(q1_cols, rows, mode, SUMS)
    fast, generic = _q1_both_paths(P, pl, q1_cols, nulls, mode, SUMS, 10471,
                                   fast=False)
    assert fast == exp
    assert generic == exp
    page, cp = _cpage(P, q1_cols, nulls)
    out = _run(P, P.OP_HASH_AGG_SMALL,
               _q1_like_plan(P, pl, mode, SUMS, 10471,
                             _pred(P, EP, P.CMP_GE, dval=0.0)), [cp])
    assert _q1_like_rows(out, mode) == _q1_like_ref(
        q1_cols, rows & (nulls["extendedprice"] == 0), mode, SUMS)


@pytest.mark.parametrize("mode", ["dec", "f64"])
def test_q1_paths_min_max_slots(P, pl, q1_cols, mode):
    """MIN in slot 0 and MAX in slot 1 of an otherwise Q1-shaped plan are
    MIN and MAX, not sums."""
    funcs = ("min", "max", "sum", "sum", "sum")
    rows = q1_cols["shipdate"] <= 10471
    exp = _q1_like_ref(q1_cols, rows, mode, funcs)
    fast, generic = _q1_both_paths(P, pl, q1_cols, None, mode, funcs, 10471,
                                   fast=False)
    assert fast == exp
    assert generic == exp


@pytest.mark.parametrize("mode", ["dec", "f64"])
def test_q1_paths_drop_unlisted_keys(P, pl, q1_cols, mode):
    """drop_unlisted_keys = 1 drops a row whose returnflag is not listed
    and raises nothing; drop_unlisted_keys = 0 raises on the same page."""
    cols = dict(q1_cols)
    cols["returnflag"] = cols["returnflag"].copy()
    row = int(np.nonzero(cols["shipdate"] <= 10471)[0][5])
    cols["returnflag"][row] = ord("X")
    rows = (cols["shipdate"] <= 10471)
    exp = _q1_like_ref(cols, rows, mode, SUMS)   # 'X' is in no group
    assert sum(r[3] for r in exp) == int(rows.sum()) - 1
    fast, generic = _q1_both_paths(P, pl, cols, None, mode, SUMS, 10471,
                                   drop=1, fast=False)
    assert fast == exp
    assert generic == exp
    for extra in (None, pl.pred(SD, P.CMP_GE, I32_MIN)):
        with pytest.raises(RuntimeError, match="outside plan enumeration"):
            _run(P, P.OP_HASH_AGG_SMALL,
                 _q1_like_plan(P, pl, mode, SUMS, 10471, extra, drop=0),
                 [P.Page(cols)])


# ---------------- h. TopN edges ----------------

N_TOPN = 5000


def _topn(P, pl, limit, pages):
    return _run(P, P.OP_TOPN, pl.top_n(limit, 0, 1, 2), pages,
                ["k", "v", "d"])


def _assert_topn(out, val, date, key, limit):
    order = R.topn_ref(val, date, key, limit)
    assert np.array_equal(out["k"], key[order])
    assert _same_bytes(out["v"], val[order])
    assert np.array_equal(out["d"], date[order])


@pytest.fixture(scope="module")
def topn_data():
    rng = np.random.default_rng(606)
    n = N_TOPN
    date = rng.integers(8000, 8100, n).astype(np.int32)
    key = rng.permutation(n).astype(np.int64) - n // 2
    vi = rng.integers(-10**12, 10**12, n)
    vi[7] = I64_MIN1
    vi[11] = I64_MAX
    vf = rng.standard_normal(n) * 1e6
    vz = np.where(rng.random(n) < 0.3, -0.0, rng.random(n) * 10 + 0.001)
    tie_v = rng.choice(np.array([-7, -1, 0, 3, 10**12]), n)
    tie_f = tie_v.astype(np.float64) / 8
    tie_d = rng.choice(np.array([8000, 8001, 8002], np.int32), n)
    return dict(date=date, key=key, vi=vi, vf=vf, vz=vz, tie_v=tie_v,
                tie_f=tie_f, tie_d=tie_d)


@pytest.mark.parametrize("limit", [1, 16, 17, 100])
def test_topn_edges(P, pl, topn_data, limit):
    """Both limit tiers (per-thread lists up to 16, histogram preselect
    above): negative i64/f64 values, -0.0, heavy ties decided by date and
    key, and the same rows split over two pages."""
    t = topn_data
    n = N_TOPN
    for name, val, date in (("i64", t["vi"], t["date"]),
                            ("f64", t["vf"], t["date"]),
                            ("negzero", t["vz"], t["date"]),
                            ("ties_i64", t["tie_v"], t["tie_d"]),
                            ("ties_f64", t["tie_f"], t["tie_d"])):
        key = t["key"]
        out = _topn(P, pl, limit, [P.Page({"v": val, "d": date, "k": key})])
        _assert_topn(out, val, date, key, limit)
        cut = 1777
        out = _topn(P, pl, limit, [
            P.Page({"v": val[:cut], "d": date[:cut], "k": key[:cut]}),
            P.Page({"v": val[cut:], "d": date[cut:], "k": key[cut:]})])
        _assert_topn(out, val, date, key, limit)
    assert len(out["k"]) == min(limit, n)


@pytest.mark.parametrize("n,limit", [(0, 16), (0, 100), (3, 16), (3, 100)])
def test_topn_fewer_rows_than_limit(P, pl, n, limit):
    for val in (np.array([5, -9, 5], np.int64)[:n],
                np.array([-2.5, 1e-300, -2.5])[:n]):
        date = np.array([3, 2, 1], np.int32)[:n]
        key = np.array([10, 11, 12], np.int64)[:n]
        out = _topn(P, pl, limit, [P.Page({"v": val, "d": date, "k": key},
                                          n_rows=n)])
        assert len(out["k"]) == n
        _assert_topn(out, val, date, key, limit)
