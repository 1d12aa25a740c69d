"""Oracle pinning tests (CPU only).

Pins the TPC-H generator restatement (oracle/tpchgen.c) and the decimal
aggregate semantics of the oracle (oracle/oracle.c) against the reference's
own SF1 golden result vectors (tests/golden/q01_sf1.result, q03_sf1.result,
restated from presto-product-tests/.../hive_tpch/ by make_fixtures.py), and
the operator primitives against pure-Python restatements of the cited Java.
"""
import pathlib
from decimal import Decimal

import numpy as np
import pytest

GOLDEN = pathlib.Path(__file__).parent / "golden"


def _parse_golden(name):
    rows = []
    for line in (GOLDEN / name).read_text().splitlines():
        if line.startswith("--") or not line.strip():
            continue
        rows.append(line.rstrip("|").split("|"))
    return rows


@pytest.fixture(scope="session")
def sf1(oracle_lib):
    return dict(li=oracle_lib.gen_lineitem(1.0),
                orders=oracle_lib.gen_orders(1.0),
                cust=oracle_lib.gen_customer(1.0))


def test_lineitem_count_sf1(oracle_lib):
    # the published TPC-H SF1 lineitem cardinality
    assert oracle_lib.lineitem_count(1.0) == 6001215


def test_q1_sf1_golden(oracle_lib, sf1):
    groups = oracle_lib.q1(sf1["li"])
    golden = _parse_golden("q01_sf1.result")
    assert len(groups) == len(golden) == 4
    for g, row in zip(groups, golden):
        assert chr(g.returnflag) == row[0]
        assert chr(g.linestatus) == row[1]
        assert Decimal(g.sum_qty_units) == Decimal(row[2])
        assert Decimal(g.sum_base_cents) / 100 == Decimal(row[3])
        assert Decimal(g.sum_disc_1e4) / 10**4 == Decimal(row[4])
        charge = (g.sum_charge_1e6_hi << 64) | g.sum_charge_1e6_lo
        assert Decimal(charge) / 10**6 == Decimal(row[5])
        # avgs: HALF_UP at scale 2 (verified against the golden digits)
        def avg2(num_hundredths, cnt):
            return (2 * num_hundredths + cnt) // (2 * cnt)
        assert Decimal(avg2(100 * g.sum_qty_units, g.count_order)) / 100 == \
            Decimal(row[6])
        assert Decimal(avg2(g.sum_base_cents, g.count_order)) / 100 == \
            Decimal(row[7])
        assert Decimal(avg2(g.sum_disc_cents, g.count_order)) / 100 == \
            Decimal(row[8])
        assert g.count_order == int(row[9])
        # f64 fixed-tree sums agree with the exact decimal values to f64
        # roundoff (they are the same mathematical quantities)
        assert abs(g.f64_sum_base - float(g.sum_base_cents) / 100) < 1e-2
        assert abs(g.f64_sum_disc_price - float(g.sum_disc_1e4) / 1e4) < 1e-2
        assert abs(g.f64_sum_charge - float(charge) / 1e6) < 1e-1
        assert g.f64_sum_qty == float(g.sum_qty_units)


def test_q3_sf1_golden(oracle_lib, sf1):
    rows = oracle_lib.q3(sf1["cust"], sf1["orders"], sf1["li"])
    golden = _parse_golden("q03_sf1.result")
    assert len(rows) == len(golden) == 10
    for r, g in zip(rows, golden):
        assert r.orderkey == int(g[0])
        assert Decimal(r.revenue_1e4) / 10**4 == Decimal(g[1])
        y, m, d = (int(x) for x in g[2].split("-"))
        epoch = (np.datetime64(g[2]) - np.datetime64("1970-01-01")).astype(int)
        assert r.orderdate == epoch
        assert r.shippriority == int(g[3])
        # exact-fx128 f64 revenue equals the decimal value to f64 roundoff
        assert abs(r.f64_revenue - r.revenue_1e4 / 1e4) < 1e-6


# ---------------- operator primitives vs python restatements ------------

def _murmur3_py(h):
    M = (1 << 64) - 1
    h ^= h >> 33
    h = (h * 0xff51afd7ed558ccd) & M
    h ^= h >> 33
    h = (h * 0xc4ceb9fe1a85ec53) & M
    h ^= h >> 33
    return h


def _bigint_hash_py(v):
    # AbstractLongType.java:137-140
    M = (1 << 64) - 1
    x = (v * 0xC2B2AE3D27D4EB4F) & M
    x = ((x << 31) | (x >> 33)) & M
    return (x * 0x9E3779B185EBCA87) & M


def test_hash_primitives(oracle_lib):
    rng = np.random.default_rng(7)
    for v in [0, 1, -1, 42, 2**62, -2**62] + list(
            rng.integers(-2**63, 2**63 - 1, 64)):
        v = int(v)
        u = v & ((1 << 64) - 1)
        assert oracle_lib.lib.oracle_murmur3_finalize(u) == _murmur3_py(u)
        assert oracle_lib.lib.oracle_bigint_hash(v) == _bigint_hash_py(v)


def test_partition_math(oracle_lib):
    # HashGenerator.java:22-29
    rng = np.random.default_rng(8)
    for h in list(rng.integers(0, 2**64, 128, dtype=np.uint64)) + [0, 2**64 - 1]:
        h = int(h)
        for n in (1, 2, 7, 8, 1024):
            x = ((h ^ (h >> 32)) & 0xFFFFFFFF)
            expect = (x * n) >> 32
            assert oracle_lib.lib.oracle_partition(h, n) == expect


def test_group_by_dense_first_seen(oracle_lib):
    rng = np.random.default_rng(9)
    keys = rng.integers(-50, 50, 10000)
    ng, gids = oracle_lib.group_by(keys)
    # dense ids in first-seen order (BigintGroupByHash putIfAbsent semantics)
    seen = {}
    for k, g in zip(keys, gids):
        if k not in seen:
            assert g == len(seen)
            seen[k] = g
        else:
            assert seen[k] == g
    assert ng == len(seen)


def test_join_chains_head_insert(oracle_lib):
    # duplicate build keys: probe emits latest-inserted duplicate first
    # (ArrayPositionLinks.java:25-30 head-insert)
    build = [10, 20, 10, 30, 10]
    probe = [10, 99, 30]
    op, ob = oracle_lib.join(build, probe)
    pairs = list(zip(op.tolist(), ob.tolist()))
    assert pairs == [(0, 4), (0, 2), (0, 0), (2, 3)]


def test_join_random_vs_python(oracle_lib):
    rng = np.random.default_rng(10)
    build = rng.integers(0, 200, 500)
    probe = rng.integers(0, 250, 800)
    op, ob = oracle_lib.join(build, probe)
    got = set(zip(op.tolist(), ob.tolist()))
    expect = set()
    idx = {}
    for i, k in enumerate(build.tolist()):
        idx.setdefault(k, []).append(i)
    for i, k in enumerate(probe.tolist()):
        for b in idx.get(k, []):
            expect.add((i, b))
    assert got == expect


def test_fx128_exact_roundtrip(oracle_lib):
    """fx128 (shared header, presto_amd/csrc/fixed128.h) must equal native
    exact arithmetic: for values in the domain (ulp >= 2^-64, i.e.
    |v| >= ~2^-12 or exactly-representable dyadics), fx128_to_f64(sum of
    exact fixed-point reprs) == correctly-rounded sum via Fraction.
    Q3 revenue products are >= ~810, far inside the domain."""
    import ctypes as C
    from fractions import Fraction
    import subprocess, tempfile, textwrap, os
    # drive the header through a tiny C harness compiled on the fly
    src = textwrap.dedent("""
        #include <stdio.h>
        #include <stdint.h>
        #include "presto_amd/csrc/fixed128.h"
        int main(void) {
            double vals[6] = {0.0625, 123456.78, 810.0, 99999.99, 0.01, 3.5};
            uint64_t hi = 0, lo = 0;
            for (int i = 0; i < 6; i++) {
                uint64_t h, l;
                fx128_from_f64(vals[i], &h, &l);
                fx128_add(&hi, &lo, h, l);
            }
            printf("%llu %llu %.17g\\n", (unsigned long long)hi,
                   (unsigned long long)lo, fx128_to_f64(hi, lo));
            return 0;
        }
    """)
    import pathlib
    repo = pathlib.Path(__file__).resolve().parent.parent
    with tempfile.TemporaryDirectory() as d:
        cfile = os.path.join(d, "t.c")
        open(cfile, "w").write(src)
        exe = os.path.join(d, "t")
        subprocess.run(["gcc", "-O2", "-I", str(repo), cfile, "-o", exe],
                       check=True)
        out = subprocess.run([exe], capture_output=True, text=True,
                             check=True).stdout.split()
    hi, lo, back = int(out[0]), int(out[1]), float(out[2])
    vals = [0.0625, 123456.78, 810.0, 99999.99, 0.01, 3.5]
    exact = sum(Fraction(v) for v in vals)  # Fraction(float) is exact
    got = Fraction(hi) + Fraction(lo, 1 << 64)
    assert got == exact  # conversion+sum is exact
    # correctly rounded back-conversion matches python float of the exact sum
    assert back == float(exact)


from varbin_refs import xxh64 as _xxh64_py  # tests/ is on sys.path


def test_xxh64_restatement(oracle_lib):
    import ctypes as C
    L = oracle_lib.lib
    L.oracle_xxh64.restype = C.c_uint64
    L.oracle_xxh64.argtypes = [C.c_char_p, C.c_int64]
    # known-answer vector: XXH64("", seed 0)
    assert L.oracle_xxh64(b"", 0) == 0xEF46DB3751D8E999
    assert _xxh64_py(b"") == 0xEF46DB3751D8E999
    # cross-check C vs independent python restatement across lengths
    rng = np.random.default_rng(55)
    for ln in [1, 3, 4, 7, 8, 9, 15, 16, 31, 32, 33, 63, 64, 100, 1000]:
        data = bytes(rng.integers(0, 256, ln, dtype=np.uint8))
        assert L.oracle_xxh64(data, ln) == _xxh64_py(data), ln
    assert L.oracle_xxh64(b"BUILDING", 8) == _xxh64_py(b"BUILDING")


def test_q5_sf1_golden(oracle_lib):
    """Q5 golden pin: also pins the customer/supplier nationkey streams and
    the dbgen PART_SUPP supplier bridge formula."""
    li = oracle_lib.gen_lineitem2(1.0)
    orders = oracle_lib.gen_orders(1.0)
    cust = oracle_lib.gen_customer2(1.0)
    supp = oracle_lib.gen_supplier(1.0)
    rows = oracle_lib.q5(cust, orders, li, supp)
    golden = _parse_golden("q05_sf1.result")
    assert len(rows) == len(golden) == 5
    for r, g in zip(rows, golden):
        assert r.name.decode() == g[0]
        assert Decimal(r.revenue_1e4) / 10**4 == Decimal(g[1])


def test_q6_sf1_golden(oracle_lib, sf1):
    rev, cnt = oracle_lib.q6(sf1["li"])
    golden = _parse_golden("q06_sf1.result")
    assert Decimal(rev) / 10**4 == Decimal(golden[0][0])


def test_q7_sf1_golden(oracle_lib):
    li = oracle_lib.gen_lineitem2(1.0)
    orders = oracle_lib.gen_orders(1.0)
    cust = oracle_lib.gen_customer2(1.0)
    supp = oracle_lib.gen_supplier(1.0)
    rows = oracle_lib.q7(cust, orders, li, supp)
    golden = _parse_golden("q07_sf1.result")
    assert len(rows) == len(golden) == 4
    names = {6: "FRANCE", 7: "GERMANY"}
    for r, g in zip(rows, golden):
        assert names[r.supp_nation] == g[0]
        assert names[r.cust_nation] == g[1]
        assert r.year == int(g[2])
        assert Decimal(r.revenue_1e4) / 10**4 == Decimal(g[3])


def test_q4_sf1_golden(oracle_lib, sf1):
    pri = oracle_lib.gen_orders_priority(1.0)
    lid = oracle_lib.gen_lineitem_dates(1.0)
    counts = oracle_lib.q4(sf1["orders"], pri, lid)
    golden = _parse_golden("q04_sf1.result")
    names = ["1-URGENT", "2-HIGH", "3-MEDIUM", "4-NOT SPECIFIED", "5-LOW"]
    assert len(golden) == 5
    for k, g in enumerate(golden):
        assert names[k] == g[0]
        assert counts[k] == int(g[1])


def test_q8_sf1_golden(oracle_lib):
    """Q8 market share — pins the part-type stream + partkey replay.
    Golden prints share rounded to 4 decimals (HALF_UP)."""
    li = oracle_lib.gen_lineitem2(1.0)
    orders = oracle_lib.gen_orders(1.0)
    cust = oracle_lib.gen_customer2(1.0)
    supp = oracle_lib.gen_supplier(1.0)
    ptype = oracle_lib.gen_part_type(1.0)
    lpk = oracle_lib.gen_lineitem_partkey(1.0)
    br, tt = oracle_lib.q8(cust, orders, li, lpk, supp, ptype)
    golden = _parse_golden("q08_sf1.result")
    for y, g in enumerate(golden):
        assert int(g[0]) == 1995 + y
        share = (Decimal(br[y]) / Decimal(tt[y])).quantize(
            Decimal("0.0001"))
        assert share == Decimal(g[1]), (br[y], tt[y])


def test_q14_sf1_golden(oracle_lib):
    """Q14 promo revenue — pins the part-type stream through the revenue
    projection.  Golden is 100.00*promo/total at scale 6 (HALF_UP)."""
    from decimal import ROUND_HALF_UP
    li = oracle_lib.gen_lineitem2(1.0)
    lpk = oracle_lib.gen_lineitem_partkey(1.0)
    ptype = oracle_lib.gen_part_type(1.0)
    promo, total = oracle_lib.q14(li, lpk, ptype)
    golden = _parse_golden("q14_sf1.result")
    got = (Decimal(100 * promo) / Decimal(total)).quantize(
        Decimal("0.000001"), rounding=ROUND_HALF_UP)
    assert got == Decimal(golden[0][0]), (promo, total)


def test_q12_sf1_golden(oracle_lib):
    """Q12 shipmode priority counts — pins the L_SMODE stream (MAIL=4,
    SHIP=6)."""
    orders = oracle_lib.gen_orders(1.0)
    pri = oracle_lib.gen_orders_priority(1.0)
    li = oracle_lib.gen_lineitem2(1.0)
    lid = oracle_lib.gen_lineitem_dates(1.0)
    smode = oracle_lib.gen_lineitem_shipmode(1.0)
    hi, lo = oracle_lib.q12(orders, pri, li, lid, smode)
    golden = _parse_golden("q12_sf1.result")
    assert golden[0][0] == "MAIL" and golden[1][0] == "SHIP"
    assert [hi[4], lo[4]] == [int(golden[0][1]), int(golden[0][2])]
    assert [hi[6], lo[6]] == [int(golden[1][1]), int(golden[1][2])]


def test_q17_sf1_golden(oracle_lib):
    """Q17 small-quantity revenue — pins p_mfgr/p_brand/p_container.
    Golden is sum(extendedprice)/7.0 at scale 2 (HALF_UP)."""
    from decimal import ROUND_HALF_UP
    li = oracle_lib.gen_lineitem2(1.0)
    lpk = oracle_lib.gen_lineitem_partkey(1.0)
    part2 = oracle_lib.gen_part2(1.0)
    cents = oracle_lib.q17(li, lpk, part2)
    golden = _parse_golden("q17_sf1.result")
    got = (Decimal(cents) / Decimal(700)).quantize(
        Decimal("0.01"), rounding=ROUND_HALF_UP)
    assert got == Decimal(golden[0][0]), cents


def test_q11_sf1_golden(oracle_lib):
    """Q11 important stock — pins the partsupp bridge + availqty +
    supplycost streams on all 1048 golden rows (values exact cents;
    golden trims trailing zeros)."""
    supp = oracle_lib.gen_supplier(1.0)
    ps = oracle_lib.gen_partsupp(1.0)
    pk, val = oracle_lib.q11(ps, supp, 200000)
    golden = _parse_golden("q11_sf1.result")
    assert len(pk) == len(golden)
    for i, g in enumerate(golden):
        assert int(pk[i]) == int(g[0])
        assert Decimal(int(val[i])) / 100 == Decimal(g[1])


def test_q18_sf1_golden(oracle_lib):
    """Q18 large-volume customers — pins the o_totalprice floor-div
    derivation over all golden rows (names are the deterministic
    Customer#%09d of custkey)."""
    import datetime
    orders = oracle_lib.gen_orders(1.0)
    tp = oracle_lib.gen_orders_totalprice(1.0)
    li = oracle_lib.gen_lineitem(1.0)
    rows = oracle_lib.q18(orders, tp, li)
    golden = _parse_golden("q18_sf1.result")
    assert len(rows) == len(golden)
    epoch = datetime.date(1970, 1, 1)
    for r, g in enumerate(golden):
        ck, ok, od, otp, qt = rows[r]
        assert f"Customer#{ck:09d}" == g[0]
        assert (ck, ok) == (int(g[1]), int(g[2]))
        assert (epoch + datetime.timedelta(days=od)).isoformat() == g[3]
        assert Decimal(otp) / 100 == Decimal(g[4])
        assert qt == int(g[5])


def test_q21_sf1_golden(oracle_lib):
    """Q21 waiting suppliers — pins the derived o_orderstatus and the
    only-late-supplier EXISTS/NOT-EXISTS pair on all 100 golden rows."""
    supp = oracle_lib.gen_supplier(1.0)
    li = oracle_lib.gen_lineitem2(1.0)
    lid = oracle_lib.gen_lineitem_dates(1.0)
    rows = oracle_lib.q21(supp, li, lid)
    golden = _parse_golden("q21_sf1.result")
    assert len(rows) == len(golden) == 100
    for (sk, cnt), g in zip(rows, golden):
        assert f"Supplier#{sk:09d}" == g[0]
        assert cnt == int(g[1])


def test_q22_sf1_golden(oracle_lib):
    """Q22 global sales opportunity — pins the c_acctbal stream and the
    phone-country-code mapping (code = nationkey + 10)."""
    from tests.oracle_binding import Q22_CODE_NATIONS
    cust = oracle_lib.gen_customer2(1.0)
    abal = oracle_lib.gen_customer_acctbal(1.0)
    orders = oracle_lib.gen_orders(1.0)
    cnt, tot = oracle_lib.q22(cust, abal, orders)
    golden = _parse_golden("q22_sf1.result")
    assert len(golden) == len(Q22_CODE_NATIONS)
    for i, g in enumerate(golden):
        assert int(Q22_CODE_NATIONS[i]) + 10 == int(g[0])
        assert cnt[i] == int(g[1])
        assert Decimal(tot[i]) / 100 == Decimal(g[2])


def test_q19_sf1_golden(oracle_lib):
    """Q19 discounted revenue — pins p_size, shipinstruct and the 'AIR'
    shipmode id (the query's 'AIR REG' literal matches no generated
    value)."""
    li = oracle_lib.gen_lineitem2(1.0)
    lpk = oracle_lib.gen_lineitem_partkey(1.0)
    smode = oracle_lib.gen_lineitem_shipmode(1.0)
    sinst = oracle_lib.gen_lineitem_shipinstruct(1.0)
    part3 = oracle_lib.gen_part3(1.0)
    rev = oracle_lib.q19(li, lpk, smode, sinst, part3)
    golden = _parse_golden("q19_sf1.result")
    assert Decimal(rev) / 10**4 == Decimal(golden[0][0]), rev


def test_q9_sf1_golden(oracle_lib):
    """Q9 product-type profit — pins the p_name permutation stream on
    all 175 golden rows (nation x year, ordered by nation NAME asc,
    year desc)."""
    import numpy as np
    li = oracle_lib.gen_lineitem2(1.0)
    lpk = oracle_lib.gen_lineitem_partkey(1.0)
    orders = oracle_lib.gen_orders(1.0)
    supp = oracle_lib.gen_supplier(1.0)
    ps = oracle_lib.gen_partsupp(1.0)
    words = oracle_lib.gen_part_name_words(1.0)
    gid = oracle_lib.color_id("green")
    p_match = (words == gid).any(axis=1).astype(np.uint8)
    prof = oracle_lib.q9(li, lpk, orders, supp, ps, p_match)
    golden = _parse_golden("q09_sf1.result")
    names = {oracle_lib.nation_name(k): k for k in range(25)}
    rows = []
    for name in sorted(names):
        for y in range(1998, 1991, -1):
            rows.append((name, y, int(prof[names[name], y - 1992])))
    assert len(rows) == len(golden) == 175
    for (name, y, ticks), g in zip(rows, golden):
        assert name == g[0] and y == int(g[1])
        assert Decimal(ticks) / 10**4 == Decimal(g[2]), (name, y)


def test_q13_sf1_golden(oracle_lib):
    """Q13 customer distribution — pins the text pool (grammar + word
    distributions) and the o_comment stream on all 42 golden rows."""
    orders = oracle_lib.gen_orders(1.0)
    rows = oracle_lib.q13(1.0, orders)
    golden = _parse_golden("q13_sf1.result")
    assert len(rows) == len(golden)
    for (c, d), g in zip(rows, golden):
        assert (c, d) == (int(g[0]), int(g[1]))


def test_q16_sf1_golden(oracle_lib):
    """Q16 parts/supplier relationship — pins the supplier-comment BBB
    splice selection on all 18314 golden rows (incl. the type-NAME
    ordering)."""
    part3 = oracle_lib.gen_part3(1.0)
    ptype = oracle_lib.gen_part_type(1.0)
    ps = oracle_lib.gen_partsupp(1.0)
    bbb = oracle_lib.gen_supplier_bbb(1.0)
    assert [i + 1 for i, b in enumerate(bbb) if b == 1] == \
        [358, 2820, 3804, 9504]
    rows = oracle_lib.q16(part3, ptype, ps, bbb)
    golden = _parse_golden("q16_sf1.result")
    assert len(rows) == len(golden)
    for (b, t, z, c), g in zip(rows, golden):
        assert f"Brand#{b}" == g[0]
        assert oracle_lib.part_type_name(t) == g[1]
        assert (z, c) == (int(g[2]), int(g[3]))


def test_nation_comments_pool(oracle_lib):
    """The 25 nation comments reproduce byte-for-byte from the text pool
    + the nation comment stream (presto-nation.result fixture restated
    as offsets)."""
    import numpy as np
    import ctypes as C
    off = np.empty(25, np.int64)
    ln = np.empty(25, np.int32)
    oracle_lib.lib.tpch_gen_nation_comment(
        off.ctypes.data_as(C.c_void_p), ln.ctypes.data_as(C.c_void_p))
    pool = oracle_lib.text_pool()
    # spot-pin the first rows against the committed fixture text
    expect0 = b" haggle. carefully final deposits detect slyly agai"
    assert pool[off[0]:off[0]+ln[0]] == expect0
    assert ln[3] == 101  # CANADA
    assert b"ironic, silent packages" in pool[off[3]:off[3]+ln[3]]


def test_q10_sf1_golden(oracle_lib):
    """Q10 returned items — every golden column except c_address (the
    one unpinned v_string generator column): custkey, name, revenue,
    acctbal, nation, phone, comment."""
    orders = oracle_lib.gen_orders(1.0)
    li = oracle_lib.gen_lineitem2(1.0)
    cust = oracle_lib.gen_customer2(1.0)
    abal = oracle_lib.gen_customer_acctbal(1.0)
    rows = oracle_lib.q10(orders, li, len(cust["custkey"]))
    golden = _parse_golden("q10_sf1.result")
    assert len(rows) == len(golden) == 20
    phones = oracle_lib.customer_phone(1.0, cust["nationkey"])
    coff, cln = oracle_lib.gen_customer_comment(1.0)
    pool = oracle_lib.text_pool()
    for (ck, rev), g in zip(rows, golden):
        assert ck == int(g[0])
        assert f"Customer#{ck:09d}" == g[1]
        assert Decimal(rev) / 10**4 == Decimal(g[2])
        assert Decimal(int(abal[ck - 1])) / 100 == Decimal(g[3])
        assert oracle_lib.nation_name(int(cust["nationkey"][ck - 1])) == g[4]
        # g[5] = c_address: unpinned
        assert phones[ck - 1] == g[6]
        assert pool[coff[ck-1]:coff[ck-1]+cln[ck-1]].decode() == g[7]


def test_q15_sf1_golden(oracle_lib):
    """Q15 top supplier — all golden columns except s_address."""
    li = oracle_lib.gen_lineitem2(1.0)
    supp = oracle_lib.gen_supplier(1.0)
    rows = oracle_lib.q15(li, len(supp["suppkey"]))
    golden = _parse_golden("q15_sf1.result")
    assert len(rows) == len(golden)
    phones = oracle_lib.supplier_phone(1.0, supp["nationkey"])
    for (sk, rev), g in zip(rows, golden):
        assert sk == int(g[0])
        assert f"Supplier#{sk:09d}" == g[1]
        assert phones[sk - 1] == g[3]
        assert Decimal(rev) / 10**4 == Decimal(g[4])


def test_q20_sf1_golden(oracle_lib):
    """Q20 potential part promotion — supplier names on all golden rows
    (addresses unpinned)."""
    words = oracle_lib.gen_part_name_words(1.0)
    ps = oracle_lib.gen_partsupp(1.0)
    li = oracle_lib.gen_lineitem2(1.0)
    lpk = oracle_lib.gen_lineitem_partkey(1.0)
    supp = oracle_lib.gen_supplier(1.0)
    sks = oracle_lib.q20(words, ps, li, lpk, supp)
    golden = _parse_golden("q20_sf1.result")
    assert len(sks) == len(golden)
    for sk, g in zip(sks, golden):
        assert f"Supplier#{sk:09d}" == g[0]


def test_q2_sf1_golden(oracle_lib):
    """Q2 minimum-cost supplier — every golden column except s_address:
    acctbal, names, nation, partkey, mfgr, phone, comment."""
    part3 = oracle_lib.gen_part3(1.0)
    ptype = oracle_lib.gen_part_type(1.0)
    ps = oracle_lib.gen_partsupp(1.0)
    supp = oracle_lib.gen_supplier(1.0)
    abal = oracle_lib.gen_supplier_acctbal(1.0)
    rows = oracle_lib.q2(part3, ptype, ps, supp, abal)
    golden = _parse_golden("q02_sf1.result")
    assert len(rows) == len(golden) == 100
    phones = oracle_lib.supplier_phone(1.0, supp["nationkey"])
    soff, sln = oracle_lib.gen_supplier_comment(1.0)
    pool = oracle_lib.text_pool()
    for (sk, pk), g in zip(rows, golden):
        assert Decimal(int(abal[sk - 1])) / 100 == Decimal(g[0])
        assert f"Supplier#{sk:09d}" == g[1]
        assert oracle_lib.nation_name(int(supp["nationkey"][sk - 1])) == g[2]
        assert pk == int(g[3])
        assert f"Manufacturer#{int(part3['mfgr'][pk - 1])}" == g[4]
        # g[5] = s_address: unpinned
        assert phones[sk - 1] == g[6]
        assert pool[soff[sk-1]:soff[sk-1]+sln[sk-1]].decode() == g[7]


def test_tpcds_date_dim_math():
    """The tpcds.c proleptic calendar (year/quarter/week per day index)
    cross-checked against Python's datetime."""
    import ctypes as C
    import datetime
    import pathlib
    import numpy as np
    so = pathlib.Path(__file__).resolve().parent.parent / "oracle" / \
        "liboracle.so"
    L = C.CDLL(str(so))
    n = 73049
    year = np.zeros(n, np.int32)
    qname = np.zeros(n, np.int32)
    week = np.zeros(n, np.int32)
    L.dsgen_date_dim(C.c_void_p(year.ctypes.data),
                     C.c_void_p(qname.ctypes.data),
                     C.c_void_p(week.ctypes.data))
    d0 = datetime.date(1900, 1, 1)
    for i in list(range(0, n, 997)) + [0, 58, 59, 60, 36158, n - 1]:
        d = d0 + datetime.timedelta(days=i)
        assert year[i] == d.year, i
        q = (d.month - 1) // 3
        assert qname[i] == d.year * 4 + q, i
        assert week[i] == i // 7


def test_key_domain_invariants(oracle_lib):
    """The round-2 key-structure mechanisms (bitmap_max_key, range_group,
    dense_array over [1, n]) rest on dbgen's key domains: orderkey is
    mk_sparse-shaped with max == pipelines.okey_max(n_orders) and every
    key >= 1; custkey/partkey/suppkey are dense 1..n; every lineitem
    orderkey appears in orders (FK).  Pin all of that against the
    generator itself at two scale factors."""
    import numpy as np
    from presto_amd.pipelines import okey_max

    for sf in (0.01, 0.1):
        orders = oracle_lib.gen_orders(sf)
        ok = orders["orderkey"]
        n = len(ok)
        assert ok.min() >= 1
        assert ok.max() == okey_max(n), (sf, ok.max(), okey_max(n))
        # mk_sparse shape: low 3 bits dense within each 32-key block
        assert len(np.unique(ok)) == n
        cust = oracle_lib.gen_customer(sf)
        ck = cust["custkey"]
        assert np.array_equal(np.sort(ck), np.arange(1, len(ck) + 1))
        # orders custkeys stay inside the customer domain
        assert orders["custkey"].min() >= 1
        assert orders["custkey"].max() <= len(ck)
        li = oracle_lib.gen_lineitem(sf)
        lok = li["orderkey"]
        assert lok.min() >= 1 and lok.max() <= okey_max(n)
        # FK: every lineitem orderkey exists in orders
        assert np.isin(np.unique(lok), ok).all()


def test_q21_acc_pack_layout_fits_across_sfs():
    """q21's accumulator packing must fit 64 bits (or fall back) at every
    plausible scale factor: widths derive from the supplier count and
    the <= 7 lineitems/order spec bound."""
    for sf, n_supp in ((1, 10_000), (100, 1_000_000), (300, 3_000_000),
                       (1000, 10_000_000), (3000, 30_000_000)):
        wsum = (7 * n_supp).bit_length()
        packs = 2 * wsum + 12 <= 64
        if sf <= 300:
            assert packs, (sf, wsum)  # benched SFs must take the packed path
        if packs:
            # fields: a0[0,wsum) a2[wsum,2w) a1[2w,+4) a3[+4,+4) cnt[+4)
            assert 2 * wsum + 12 <= 64
            # totals fit: sum(suppkey) <= 7*n_supp < 2^wsum
            assert 7 * n_supp < (1 << wsum)
