"""CPU self-checks of tests/varbin_refs.py — the references the GPU
variable-width tests trust, pinned against hand-written tables, the XXH64
known answer, the CPU oracle and (where installed) the xxhash module.
No GPU needed."""
import ctypes as C

import numpy as np
import pytest

import varbin_refs as R  # tests/ is on sys.path (pytest's rootdir import mode)

T, F = True, False

# (op, s, a, b, expected): the edges a substring search gets wrong
LIKE_TABLE = [
    # a match at each of the four offsets of a 4-byte window
    ("CONTAINS", b"xy......", b"xy", b"", T),
    ("CONTAINS", b".xy.....", b"xy", b"", T),
    ("CONTAINS", b"..xy....", b"xy", b"", T),
    ("CONTAINS", b"...xy...", b"xy", b"", T),
    # a match ending exactly at the last byte; one byte short of it
    ("CONTAINS", b"......xy", b"xy", b"", T),
    ("CONTAINS", b".......x", b"xy", b"", F),
    # pattern as long as the string, and longer
    ("CONTAINS", b"abc", b"abc", b"", T),
    ("CONTAINS", b"abc", b"abcd", b"", F),
    ("CONTAINS", b"", b"a", b"", F),
    # 1-byte pattern, first / last / absent
    ("CONTAINS", b"abc", b"a", b"", T),
    ("CONTAINS", b"abc", b"c", b"", T),
    ("CONTAINS", b"abc", b"d", b"", F),
    # overlapping candidates
    ("CONTAINS", b"aaab", b"aab", b"", T),
    ("CONTAINS", b"aaaa", b"aab", b"", F),
    ("CONTAINS", b"ababac", b"abac", b"", T),
    # bytes >= 0x80 and NUL
    ("CONTAINS", b"\x00\xff\xfe", b"\xff\xfe", b"", T),
    ("CONTAINS", b"\x00\xff\xfe", b"\xfe\xff", b"", F),
    ("CONTAINS", b"a\x00b", b"\x00", b"", T),
    # the haszero false positive: c0 ^ 0x01 next to a real c0
    ("CONTAINS", b"\x00\x01", b"\x00", b"", T),
    ("CONTAINS", b"\x01\x01\x01\x01", b"\x00", b"", F),
    ("CONTAINS", b"\x01\x00\x01\x01", b"\x01\x01", b"", T),
    ("CONTAINS", b"\xfe\xff\xfe\xfe", b"\xff\xff", b"", F),
    # the empty needle matches everywhere
    ("CONTAINS", b"", b"", b"", T),
    ("CONTAINS", b"abc", b"", b"", T),
    ("PREFIX", b"abc", b"", b"", T),
    ("PREFIX", b"abc", b"ab", b"", T),
    ("PREFIX", b"abc", b"abc", b"", T),
    ("PREFIX", b"abc", b"abcd", b"", F),
    ("PREFIX", b"abc", b"bc", b"", F),
    ("PREFIX", b"", b"a", b"", F),
    ("EQ", b"abc", b"abc", b"", T),
    ("EQ", b"abc", b"ab", b"", F),
    ("EQ", b"ab", b"abc", b"", F),
    ("EQ", b"", b"", b"", T),
    ("EQ", b"a\x00", b"a", b"", F),
    ("NE", b"abc", b"abc", b"", F),
    ("NE", b"abc", b"abd", b"", T),
    ("NE", b"", b"", b"", F),
    # CONTAINS2: b must start at or after the end of some a
    ("CONTAINS2", b"ab", b"a", b"b", T),          # b directly after a
    ("CONTAINS2", b"ba", b"a", b"b", F),          # b only before a
    ("CONTAINS2", b"aba", b"ab", b"ba", F),       # b overlaps a's tail
    ("CONTAINS2", b"abba", b"ab", b"ba", T),
    ("CONTAINS2", b"a", b"a", b"a", F),           # a == b needs two
    ("CONTAINS2", b"aa", b"a", b"a", T),
    ("CONTAINS2", b"aaa", b"aa", b"aa", F),
    ("CONTAINS2", b"aaaa", b"aa", b"aa", T),
    ("CONTAINS2", b"xa.b", b"a", b"b", T),        # gap between the two
    ("CONTAINS2", b"a\nb", b"a", b"b", T),        # the gap may hold \n
    ("CONTAINS2", b"abc", b"", b"c", T),          # empty a
    ("CONTAINS2", b"abc", b"c", b"", T),          # empty b
    ("CONTAINS2", b"abc", b"d", b"", F),
    ("CONTAINS2", b"", b"", b"", T),
    ("CONTAINS2", b"a.b", b"a.", b"b", T),        # needles are literals
    ("CONTAINS2", b"axb", b"a.", b"b", F),
    ("NOT_CONTAINS2", b"ab", b"a", b"b", F),
    ("NOT_CONTAINS2", b"ba", b"a", b"b", T),
    ("NOT_CONTAINS2", b"", b"a", b"", T),
]


@pytest.mark.parametrize("op,s,a,b,exp", LIKE_TABLE)
def test_like_ref_table(op, s, a, b, exp):
    assert R.like_ref(op, s, a, b) is exp


def test_like_ref_contains2_is_the_two_find_rule():
    """The regular expression agrees with "some occurrence of a, then b at
    or after its end" spelled with find, over every short string."""
    import itertools
    alpha = (b"a", b"b")
    strings = [b"".join(t) for n in range(7)
               for t in itertools.product(alpha, repeat=n)]
    needles = [b"", b"a", b"b", b"aa", b"ab", b"ba", b"bb"]
    for a in needles:
        for b in needles:
            for s in strings:
                exp = any(s.find(b, i + len(a)) >= 0
                          for i in R.match_offsets(s, a))
                assert R.like_ref("CONTAINS2", s, a, b) is exp, (s, a, b)
                assert R.like_ref("NOT_CONTAINS2", s, a, b) is (not exp)


def test_pred_rows_nulls_exclude_for_every_op():
    strings = [b"ab", b"ab", b"ba", b"ba", b"", b""]
    nulls = [0, 1, 0, 1, 0, 1]
    assert R.pred_rows("EQ", strings, b"ab", nulls=nulls) == [0]
    assert R.pred_rows("NE", strings, b"ab", nulls=nulls) == [2, 4]
    assert R.pred_rows("CONTAINS", strings, b"a", nulls=nulls) == [0, 2]
    assert R.pred_rows("PREFIX", strings, b"b", nulls=nulls) == [2]
    assert R.pred_rows("CONTAINS2", strings, b"a", b"b", nulls) == [0]
    assert R.pred_rows("NOT_CONTAINS2", strings, b"a", b"b", nulls) == [2, 4]
    # without nulls an op and its negation split the rows
    assert R.pred_rows("NE", strings, b"ab") == [2, 3, 4, 5]
    assert R.match_offsets(b"aaab", b"aa") == [0, 1]
    assert R.match_offsets(b"ab", b"abc") == []


def test_xxh64_known_answer():
    assert R.xxh64(b"") == 0xEF46DB3751D8E999


def _strings_0_100():
    rng = np.random.default_rng(77)
    return [bytes(rng.integers(0, 256, ln, dtype=np.uint8))
            for ln in range(101)]


def test_xxh64_vs_oracle_every_length(oracle_lib):
    L = oracle_lib.lib
    L.oracle_xxh64.restype = C.c_uint64
    L.oracle_xxh64.argtypes = [C.c_char_p, C.c_int64]
    for data in _strings_0_100():
        assert L.oracle_xxh64(data, len(data)) == R.xxh64(data), len(data)
    # every length class of the algorithm was among them
    seen = {tuple(sorted(R.xxh64_paths(n).items())) for n in range(101)}
    assert len(seen) == 16


def test_xxh64_vs_xxhash_module():
    xxhash = pytest.importorskip("xxhash")
    for data in _strings_0_100():
        assert xxhash.xxh64(data).intdigest() == R.xxh64(data), len(data)


def test_xxh64_paths():
    assert R.xxh64_paths(0) == dict(stripe=F, u64=F, u32=F, bytes=F)
    assert R.xxh64_paths(3) == dict(stripe=F, u64=F, u32=F, bytes=T)
    assert R.xxh64_paths(4) == dict(stripe=F, u64=F, u32=T, bytes=F)
    assert R.xxh64_paths(31) == dict(stripe=F, u64=T, u32=T, bytes=T)
    assert R.xxh64_paths(32) == dict(stripe=T, u64=F, u32=F, bytes=F)
    assert R.xxh64_paths(40) == dict(stripe=T, u64=T, u32=F, bytes=F)
    assert R.xxh64_paths(100) == dict(stripe=T, u64=F, u32=T, bytes=F)


def test_partition_vs_oracle(oracle_lib):
    rng = np.random.default_rng(78)
    hs = [int(h) for h in rng.integers(0, 2**64, 256, dtype=np.uint64)]
    for h in hs + [0, 1, 2**32 - 1, 2**32, 2**63, 2**64 - 1]:
        for n in (1, 2, 7, 8, 256, 1024):
            assert R.partition(h, n) == oracle_lib.lib.oracle_partition(h, n)
            assert 0 <= R.partition(h, n) < n


def test_gather():
    strings = [b"ab", b"", b"cde"]
    assert R.gather(strings, [2, 0, 1, 2]) == ([0, 3, 5, 5, 8], b"cdeabcde")
    assert R.gather(strings, []) == ([0], b"")
    assert R.gather(strings, [1, 1]) == ([0, 0, 0], b"")
