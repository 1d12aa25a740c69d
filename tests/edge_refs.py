"""Plain numpy/Python references for the edge tests (tests/test_gpu_edges.py).

None of these restates the kernels' arithmetic shortcuts: decimal ticks come
from the integers the inputs were generated from, f64 sums from math.fsum
(the correctly rounded exact sum fixed128.h promises) or from a replay of the
documented deterministic schedule, predicates and
projections from numpy's IEEE / int64 operators.  tests/test_edge_refs.py
checks the references themselves on a CPU-only box.
"""
import math

import numpy as np

FT_NBLOCKS = 4096
FT_NTHREADS = 256
VL = FT_NBLOCKS * FT_NTHREADS  # threads of the fixed aggregation grid

OPS = ("lt", "le", "gt", "ge", "eq", "ne")  # pg_cmp order 0..5


# ---- decimal ticks ----
def ticks_exact(k, scale):
    """Inputs for a decimal test, generated FROM integer ticks: returns
    (x, ticks) with x = k / 10**scale as float64 (correctly rounded quotient)
    and ticks = the Python ints k themselves — the expected
    round(x * 10**scale) by construction, whatever the sign."""
    k = np.asarray(k, np.int64)
    x = k / float(10 ** scale)
    return x, [int(v) for v in k]


def disc_price_ticks(cents, d):
    """a * (1 - b) in 1e-4 ticks from integer cents / hundredths."""
    return [int(c) * (100 - int(dd)) for c, dd in zip(cents, d)]


def charge_ticks(cents, d, t):
    """a * (1 - b) * (1 + c) in 1e-6 ticks."""
    return [int(c) * (100 - int(dd)) * (100 + int(tt))
            for c, dd, tt in zip(cents, d, t)]


def mul_ticks(cents, d):
    """a * b in 1e-4 ticks."""
    return [int(c) * int(dd) for c, dd in zip(cents, d)]


def i128(hi, lo):
    """A (hi, lo) int64 output pair as a signed Python int."""
    return (int(hi) << 64) | (int(lo) & 0xFFFFFFFFFFFFFFFF)


def group_int(keys, ticks, mask=None, reduce=sum):
    """{key: reduce(ticks of the key's unmasked rows)} in Python ints."""
    out = {}
    for i, (k, t) in enumerate(zip(keys, ticks)):
        if mask is not None and not mask[i]:
            continue
        out.setdefault(int(k), []).append(t)
    return {k: reduce(v) for k, v in out.items()}


# ---- exact f64 sums ----
def fsum_groups(keys, vals, mask=None):
    """{key: math.fsum(values of the key's rows)} — the exact real sum of
    the f64 addends, rounded once."""
    buckets = {}
    for i, (k, v) in enumerate(zip(keys, vals)):
        if mask is not None and not mask[i]:
            continue
        buckets.setdefault(int(k), []).append(float(v))
    return {k: math.fsum(v) for k, v in buckets.items()}


def bits(x):
    """int64 bit pattern(s) of float64 value(s)."""
    return np.asarray(x, np.float64).view(np.int64)


# ---- predicates ----
def pred_ref(op, lhs, rhs, lhs_null=None, rhs_null=None):
    """Row mask of `lhs <op> rhs` (op = pg_cmp 0..5 or its name) with
    IEEE/numpy comparison semantics: a NaN on either side is false for every
    op but NE.  Integer operands compare as int64, anything with a float
    side as float64.  Rows null on lhs or rhs are excluded."""
    name = OPS[op] if isinstance(op, (int, np.integer)) else op
    lhs = np.asarray(lhs)
    rhs = np.asarray(rhs)
    if lhs.dtype.kind == "f" or rhs.dtype.kind == "f":
        lhs, rhs = lhs.astype(np.float64), rhs.astype(np.float64)
    else:
        lhs, rhs = lhs.astype(np.int64), rhs.astype(np.int64)
    with np.errstate(invalid="ignore"):
        m = {"lt": np.less, "le": np.less_equal, "gt": np.greater,
             "ge": np.greater_equal, "eq": np.equal,
             "ne": np.not_equal}[name](lhs, rhs)
    m = np.broadcast_to(m, np.broadcast(lhs, rhs).shape).copy()
    for nm in (lhs_null, rhs_null):
        if nm is not None:
            m &= np.asarray(nm) == 0
    return m


# ---- projections ----
IDENT, DISC_PRICE, CHARGE, MUL, DIV, KEYSHL, SHR, SUBDIV, KEYSHL_DIV = range(9)


def _trunc_div(x, d):
    """C's truncating int64 division, d != 0."""
    x = np.asarray(x, np.int64)
    q = np.abs(x) // abs(int(d))
    return np.where((x < 0) != (d < 0), -q, q).astype(np.int64)


def proj_ref(kind, a, b=None, c=None):
    """Expected output column of pg_proj_kind `kind`.
    IDENT keeps a's type.  KEYSHL (a << c | b), SHR (arithmetic a >> c),
    SUBDIV ((a - b) / c, b and c constants, C truncation, c == 0 divides by
    1) and KEYSHL_DIV (c = shift << 16 | div, div == 0 divides by 1) give
    int64.  MUL, DIV, DISC_PRICE, CHARGE give float64 computed operation by
    operation in IEEE double (division by zero, inf and NaN included)."""
    if kind == IDENT:
        return np.asarray(a).copy()
    if kind == KEYSHL:
        return (np.asarray(a, np.int64) << np.int64(c)) | \
            np.asarray(b, np.int64)
    if kind == SHR:
        return np.asarray(a, np.int64) >> np.int64(c)
    if kind == SUBDIV:
        return _trunc_div(np.asarray(a, np.int64) - np.int64(b),
                          c if c else 1)
    if kind == KEYSHL_DIV:
        shift, dv = c >> 16, c & 0xFFFF
        return (np.asarray(a, np.int64) << np.int64(shift)) | \
            _trunc_div(b, dv if dv else 1)
    fa = np.asarray(a).astype(np.float64)
    fb = np.asarray(b).astype(np.float64)
    with np.errstate(all="ignore"):
        if kind == MUL:
            return fa * fb
        if kind == DIV:
            return fa / fb
        v = fa * (1.0 - fb)
        if kind == DISC_PRICE:
            return v
        if kind == CHARGE:
            return v * (1.0 + np.asarray(c).astype(np.float64))
    raise ValueError(kind)


def same_f64(got, exp):
    """Bit-equal where exp is a number, NaN where exp is NaN."""
    got = np.asarray(got, np.float64)
    exp = np.asarray(exp, np.float64)
    nan = np.isnan(exp)
    return bool(np.array_equal(np.isnan(got), nan) and
                np.array_equal(bits(got)[~nan], bits(exp)[~nan]))


# ---- the deterministic small-key aggregation schedule ----
def _bfly(a):
    """xor-butterfly over the last axis (x_i += x_{i^s}, s = n/2 .. 1);
    every lane ends with the same tree sum — lane 0 is returned."""
    n = a.shape[-1]
    idx = np.arange(n)
    s = n // 2
    while s >= 1:
        a = a + a[..., idx ^ s]
        s //= 2
    return a[..., 0]


def butterfly_sum(vals, n=None):
    """f64 sum of one page of n rows in the fixed schedule of the small-key
    aggregation kernels: thread v of the 4096 x 256 grid accumulates its
    rows sequentially across grid passes (acc = 0; acc += x[2v];
    acc += x[2v+1]; acc += x[2v + 2*VL]; ...), then a 64-lane butterfly per
    wave, a 4-wave butterfly per block, and the grid reduce (lane l sums
    blocks l, l+64, ... ascending, then a 64-lane butterfly).  `vals` holds
    0.0 at rows that are filtered out or belong to another group."""
    vals = np.asarray(vals, np.float64)
    if n is None:
        n = len(vals)
    passes = max(1, -(-n // (2 * VL)))
    # blocks past the data only ever add 0.0 + 0.0: their partial is 0.0,
    # so small pages replay just the blocks that own rows
    nb = FT_NBLOCKS if passes > 1 else max(1, -(-n // (2 * FT_NTHREADS)))
    nl = nb * FT_NTHREADS
    lane = np.zeros(nl)
    for p in range(passes):
        w = np.zeros(2 * nl)
        chunk = vals[p * 2 * VL:min(n, p * 2 * VL + 2 * nl)]
        w[:len(chunk)] = chunk
        lane = lane + w[0::2]
        lane = lane + w[1::2]
    wave = _bfly(lane.reshape(-1, 64))              # 4 wave sums per block
    block = np.zeros(FT_NBLOCKS)
    block[:nb] = 0.0 + _bfly(wave.reshape(nb, 4))   # partials start at 0.0
    by_lane = block.reshape(FT_NBLOCKS // 64, 64)   # [m, l] = block l + 64m
    g = np.zeros(64)
    for m in range(FT_NBLOCKS // 64):
        g = g + by_lane[m]
    return float(_bfly(g))


# ---- TopN ----
def topn_ref(val, date, key, limit):
    """Row indexes of ORDER BY val DESC, date ASC, key ASC LIMIT limit in
    plain IEEE ordering (inputs hold no NaN and never both zeros)."""
    val = np.asarray(val)
    return np.lexsort((key, date, -val))[:limit]
