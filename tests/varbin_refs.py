"""Plain Python references for the variable-width column tests
(tests/test_gpu_varbin.py).

Everything here works on `bytes` with the language's own operators (==, in,
startswith, re) and Python integers; nothing restates the kernels' search
loops and nothing is shared with csrc/.  tests/test_varbin_refs.py checks
the references themselves on a CPU-only box.
"""
import re

OPS = ("EQ", "NE", "CONTAINS", "PREFIX", "CONTAINS2", "NOT_CONTAINS2")
# pg_cmp values of the six string-capable ops (presto_gpu.h)
CMP = {"EQ": 4, "NE": 5, "CONTAINS": 6, "PREFIX": 7, "CONTAINS2": 8,
       "NOT_CONTAINS2": 9}

M64 = (1 << 64) - 1


# ---- LIKE pushdowns ----
def like_ref(op, s, a, b=b""):
    """Does the string s pass `op` with needle a (and second needle b)?
    CONTAINS2 is LIKE '%a%b%': some occurrence of a followed, without
    overlap, by an occurrence of b — stated as a regular expression, not
    through the leftmost-a argument the kernel relies on."""
    if op == "EQ":
        return s == a
    if op == "NE":
        return s != a
    if op == "CONTAINS":
        return a in s
    if op == "PREFIX":
        return s.startswith(a)
    if op in ("CONTAINS2", "NOT_CONTAINS2"):
        m = re.search(re.escape(a) + b".*" + re.escape(b), s, re.S)
        return (m is not None) == (op == "CONTAINS2")
    raise ValueError(op)


def pred_rows(op, strings, a, b=b"", nulls=None):
    """Row indexes that pass: like_ref with "a null excludes the row"
    applied to every op, NE and NOT_CONTAINS2 included (a null row passes
    neither an op nor its negation)."""
    return [i for i, s in enumerate(strings)
            if not (nulls is not None and nulls[i]) and like_ref(op, s, a, b)]


def match_offsets(s, a):
    """Every offset at which a occurs in s (overlapping ones too)."""
    return [i for i in range(len(s) - len(a) + 1) if s[i:i + len(a)] == a]


# ---- XXH64 (the reference's varchar hash, io.airlift.slice.XxHash64) ----
def xxh64(data, seed=0):
    """Independent pure-Python restatement of XXH64."""
    M = M64
    P1, P2, P3 = 0x9E3779B185EBCA87, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9
    P4, P5 = 0x85EBCA77C2B2AE63, 0x27D4EB2F165667C5

    def rotl(x, r):
        return ((x << r) | (x >> (64 - r))) & M

    def rnd(acc, x):
        return (rotl((acc + x * P2) & M, 31) * P1) & M

    n = len(data)
    i = 0
    if n >= 32:
        v = [(seed + P1 + P2) & M, (seed + P2) & M, seed,
             (seed - P1) & M]
        while i + 32 <= n:
            for j in range(4):
                lane = int.from_bytes(data[i:i + 8], "little")
                v[j] = rnd(v[j], lane)
                i += 8
        h = (rotl(v[0], 1) + rotl(v[1], 7) + rotl(v[2], 12) +
             rotl(v[3], 18)) & M
        for j in range(4):
            h = ((h ^ rnd(0, v[j])) * P1 + P4) & M
    else:
        h = (seed + P5) & M
    h = (h + n) & M
    while i + 8 <= n:
        h = ((rotl((h ^ rnd(0, int.from_bytes(data[i:i + 8], "little"))) & M,
                   27) * P1) + P4) & M
        i += 8
    if i + 4 <= n:
        h = ((rotl(h ^ (int.from_bytes(data[i:i + 4], "little") * P1) & M,
                   23) * P2) + P3) & M
        i += 4
    while i < n:
        h = (rotl(h ^ (data[i] * P5) & M, 11) * P1) & M
        i += 1
    h ^= h >> 33
    h = (h * P2) & M
    h ^= h >> 29
    h = (h * P3) & M
    h ^= h >> 32
    return h


def xxh64_paths(n):
    """Which parts of XXH64 a string of n bytes runs: the four-lane stripe
    loop, the 8-byte loop, the 4-byte step, the byte tail."""
    r = n % 32 if n >= 32 else n
    return {"stripe": n >= 32, "u64": r >= 8, "u32": r % 8 >= 4,
            "bytes": r % 4 > 0}


# ---- partition id (HashGenerator.java:22-29) ----
def partition(raw_hash, n):
    """The 32-bit fold of the raw hash scaled into [0, n):
    ((h ^ (h >>> 32)) & 0xffffffff) * n >> 32, as the HashGenerator comment
    states it."""
    h = raw_hash & M64
    return (((h ^ (h >> 32)) & 0xFFFFFFFF) * n) >> 32


# ---- VARBIN emit ----
def gather(strings, rows):
    """(offsets, bytes) of the VariableWidthBlock holding strings[rows]."""
    offs = [0]
    for r in rows:
        offs.append(offs[-1] + len(strings[r]))
    return offs, b"".join(strings[r] for r in rows)
