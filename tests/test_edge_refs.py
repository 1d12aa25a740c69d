"""CPU self-checks of tests/edge_refs.py — the references the GPU edge tests
trust are themselves pinned against independent restatements (Decimal,
Fraction, the CPU oracle, hand-written tables).  No GPU needed."""
import math
from decimal import Decimal, ROUND_HALF_UP
from fractions import Fraction

import numpy as np
import pytest

import edge_refs as R  # tests/ is on sys.path (pytest's rootdir import mode)


def test_ticks_exact_is_half_up_rounding():
    """x = k/100 rounds back to k under Decimal ROUND_HALF_UP (half away
    from zero) for every cent in [-10^5, 10^5], negatives included."""
    k = np.arange(-10**5, 10**5 + 1)
    x, ticks = R.ticks_exact(k, 2)
    cent = Decimal("0.01")
    for xv, t in zip(x.tolist(), ticks):
        q = Decimal(xv).quantize(cent, rounding=ROUND_HALF_UP)
        assert int(q * 100) == t
    assert ticks[0] == -10**5 and ticks[-1] == 10**5
    # products in Python ints
    assert R.disc_price_ticks([-123], [7]) == [-123 * 93]
    assert R.charge_ticks([-123], [7], [8]) == [-123 * 93 * 108]
    assert R.mul_ticks([-123], [-5]) == [615]
    assert R.i128(-1, -5) == -5 and R.i128(0, -5) == 2**64 - 5
    assert R.i128(1, 2) == 2**64 + 2


def _old_model_sum(sel_vals, n):
    """The single-pass model test_generic_f64_agg_butterfly_model carries
    (n < 2*VL: one row pair per lane), kept verbatim as the yardstick."""
    VL = 4096 * 256
    w = np.zeros(2 * VL)
    w[:n] = sel_vals
    lane = w[0::2] + w[1::2]
    a = lane.reshape(-1, 64)
    idx = np.arange(64)
    for s in (32, 16, 8, 4, 2, 1):
        a = a + a[:, idx ^ s]
    wsum = a[:, 0].reshape(-1, 4)
    for s in (2, 1):
        wsum = wsum + wsum[:, np.arange(4) ^ s]
    bp = wsum[:, 0]
    g = np.zeros(64)
    for l in range(64):
        acc = 0.0
        for m in range(64):
            acc += bp[l + 64 * m]
        g[l] = acc
    g2 = g.copy()
    for s in (32, 16, 8, 4, 2, 1):
        g2 = g2 + g2[np.arange(64) ^ s]
    return g2[0]


@pytest.mark.parametrize("n", [1, 2, 3, 1000, 150_001])
def test_butterfly_sum_matches_single_pass_model(n):
    rng = np.random.default_rng(n)
    x = np.where(rng.random(n) < 0.6, rng.random(n) * 1000, 0.0)
    assert R.bits(R.butterfly_sum(x)) == R.bits(_old_model_sum(x, n))


def test_butterfly_sum_matches_oracle_q1(oracle_lib):
    """The replay equals the oracle's f64 Q1 sums on SF0.1 lineitem, and
    still does when the rows are tiled past one grid pass (2*VL + 3)."""
    li = oracle_lib.gen_lineitem(0.1)
    for n in (len(li["quantity"]), 2 * R.VL + 3):
        cols = {k: np.resize(v, n) for k, v in li.items()}
        exp = oracle_lib.q1(cols)
        sel = cols["shipdate"] <= 10471
        e, d, t = cols["extendedprice"], cols["discount"], cols["tax"]
        dp = e * (1.0 - d)
        series = (("f64_sum_qty", cols["quantity"]), ("f64_sum_base", e),
                  ("f64_sum_disc_price", dp),
                  ("f64_sum_charge", dp * (1.0 + t)), ("f64_sum_disc", d))
        assert len(exp) == 4
        for g in exp:
            m = sel & (cols["returnflag"] == g.returnflag) & \
                (cols["linestatus"] == g.linestatus)
            assert int(m.sum()) == g.count_order
            for name, v in series:
                got = R.butterfly_sum(np.where(m, v, 0.0))
                assert R.bits(got) == R.bits(getattr(g, name)), (n, name)


def test_fsum_groups_is_exact_sum_rounded_once():
    rng = np.random.default_rng(5)
    keys = rng.integers(0, 7, 4000)
    vals = rng.integers(1, 10**9, 4000) / 100.0
    vals[:64] = 2.0**52 + 0.5
    keys[:64] = 7
    vals[64:96] = 2.0**-12 * (1 + np.arange(32) / 1024)
    keys[64:96] = 8
    got = R.fsum_groups(keys, vals)
    for k in range(9):
        exact = sum((Fraction(float(v)) for v in vals[keys == k]),
                    Fraction(0))
        assert got[k] == float(exact)  # Fraction -> float rounds once
    assert got[7] == 64 * 2.0**52 + 32.0
    m = keys != 7
    assert 7 not in R.fsum_groups(keys, vals, m)
    assert R.group_int([1, 2, 1], [5, -7, 6]) == {1: 11, 2: -7}
    assert R.group_int([1, 2, 1], [5, -7, 6], reduce=min) == {1: 5, 2: -7}


def test_pred_ref_table():
    nan, inf = math.nan, math.inf
    lhs = np.array([1.0, nan, -0.0, inf, 5e-324, 2.0])
    rhs = np.array([1.0, 1.0, 0.0, nan, 0.0, 1.0])
    exp = {"lt": [0, 0, 0, 0, 0, 0], "le": [1, 0, 1, 0, 0, 0],
           "gt": [0, 0, 0, 0, 1, 1], "ge": [1, 0, 1, 0, 1, 1],
           "eq": [1, 0, 1, 0, 0, 0], "ne": [0, 1, 0, 1, 1, 1]}
    for i, name in enumerate(R.OPS):
        assert R.pred_ref(i, lhs, rhs).tolist() == [bool(v) for v in
                                                    exp[name]], name
        assert R.pred_ref(name, lhs, rhs).tolist() == \
            R.pred_ref(i, lhs, rhs).tolist()
    # integers compare as int64, exactly, at the extremes
    big = np.array([2**63 - 1, -2**63 + 1, 2**53 + 1], np.int64)
    assert R.pred_ref("gt", big, np.int64(2**53)).tolist() == \
        [True, False, True]
    assert R.pred_ref("eq", big, big - 1).tolist() == [False] * 3
    u8 = np.array([0, 255], np.uint8)
    assert R.pred_ref("gt", u8, -1).tolist() == [True, True]
    assert R.pred_ref("lt", u8, np.array([1, -1], np.int32)).tolist() == \
        [True, False]
    # nulls on either side exclude the row, NE included
    ln = np.array([1, 0, 0], np.uint8)
    rn = np.array([0, 0, 1], np.uint8)
    a = np.array([1, 2, 3], np.int64)
    assert R.pred_ref("ne", a, 0, ln, rn).tolist() == [False, True, False]
    # f64 lhs against an integer column + dval
    f = np.array([2.5, 3.5, nan])
    i32 = np.array([0, 1, 2], np.int32)
    assert R.pred_ref("eq", f, i32.astype(np.float64) + 2.5).tolist() == \
        [True, True, False]


def test_proj_ref_table():
    nan, inf = math.nan, math.inf
    a = np.array([-9, -1, 0, 7, 10**12], np.int64)
    assert R.proj_ref(R.SHR, a, c=1).tolist() == \
        [-5, -1, 0, 3, 5 * 10**11]          # arithmetic shift
    assert R.proj_ref(R.SHR, a, c=0).tolist() == a.tolist()
    assert R.proj_ref(R.SUBDIV, a, 3, 7).tolist() == \
        [-1, 0, 0, 0, (10**12 - 3) // 7]    # truncation toward zero
    assert R.proj_ref(R.SUBDIV, a, 3, 0).tolist() == (a - 3).tolist()
    k = np.array([1, 2, 3], np.int64)
    b = np.array([-15, 0, 22], np.int64)
    assert R.proj_ref(R.KEYSHL, k, np.array([5, 6, 7]), 40).tolist() == \
        [(1 << 40) | 5, (2 << 40) | 6, (3 << 40) | 7]
    assert R.proj_ref(R.KEYSHL, k, b, 0).tolist() == \
        [1 | -15, 2, 3 | 22]
    assert R.proj_ref(R.KEYSHL_DIV, k, b, (14 << 16) | 7).tolist() == \
        [(1 << 14) | -2, 2 << 14, (3 << 14) | 3]
    assert R.proj_ref(R.KEYSHL_DIV, k, b, (8 << 16) | 0).tolist() == \
        [(1 << 8) | -15, 2 << 8, (3 << 8) | 22]
    x = np.array([1.0, -1.0, 0.0, inf, nan])
    y = np.array([0.0, 0.0, 0.0, 2.0, 1.0])
    assert R.same_f64(R.proj_ref(R.DIV, x, y), [inf, -inf, nan, inf, nan])
    assert R.same_f64(R.proj_ref(R.DIV, x, -y),
                      [-inf, inf, nan, -inf, nan])
    assert not R.same_f64([0.0], [-0.0])
    e = np.array([100.0, 19.99])
    d = np.array([0.1, 0.05])
    t = np.array([2, 3], np.int32)
    assert R.same_f64(R.proj_ref(R.DISC_PRICE, e, d),
                      [100.0 * (1.0 - 0.1), 19.99 * (1.0 - 0.05)])
    assert R.same_f64(R.proj_ref(R.CHARGE, e, d, t),
                      [100.0 * (1.0 - 0.1) * 3.0, 19.99 * (1.0 - 0.05) * 4.0])
    assert R.same_f64(R.proj_ref(R.MUL, e, t), [200.0, 19.99 * 3.0])
    i32 = np.array([-3, 4], np.int32)
    assert R.proj_ref(R.IDENT, i32).dtype == np.int32


def test_topn_ref_order():
    val = np.array([5.0, -0.0, 5.0, 7.5, -3.0, 5.0])
    date = np.array([2, 1, 1, 9, 1, 1], np.int32)
    key = np.array([10, 11, 13, 12, 14, 12], np.int64)
    assert R.topn_ref(val, date, key, 4).tolist() == [3, 5, 2, 0]
    assert R.topn_ref(val, date, key, 100).tolist() == [3, 5, 2, 0, 1, 4]
    iv = np.array([-2**63 + 1, 0, 10**12], np.int64)
    assert R.topn_ref(iv, date[:3], key[:3], 3).tolist() == [2, 1, 0]
