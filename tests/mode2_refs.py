"""Row-at-a-time references of LOOKUP_JOIN mode 2 (the single-pass Q5 probe,
include/presto_gpu.h, pg_plan_lookup_join) and of the dense-array fills
behind it (pg_plan_hash_build.dense_array).  numpy arrays for storage,
Python ints and math.fsum for the arithmetic.  No GPU — this is the
checker, never the product.
"""
import math

import numpy as np

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
# the 64.64 accumulator domain of fixed128.h: 0, or 2^-12 <= x < 2^53
FX_LO, FX_HI = 2.0 ** -12, 2.0 ** 53


def _selected(n, sel):
    return range(n) if sel is None else [i for i in range(n) if sel[i]]


def dense_fill_ref(keys, vals, cap, bias, sel, dtype):
    """The dense array a build leaves: cap zeros, out[k-1] = vals + bias for
    the selected rows with 1 <= k <= cap.  vals None is a key set (flag 1,
    no bias).  uint8 stores wrap mod 256.  Duplicate keys race on the
    device, so a key seen twice among the selected rows is an error of the
    test."""
    out = np.zeros(cap, dtype)
    seen = set()
    for i in _selected(len(keys), sel):
        k = int(keys[i])
        assert k not in seen, f"duplicate dense key {k}"
        seen.add(k)
        if not 1 <= k <= cap:
            continue
        v = 1 if vals is None else int(vals[i]) + bias
        out[k - 1] = v % 256 if np.dtype(dtype) == np.uint8 else v
    return out


def dense_fill_lu_ref(keys, k2, lu, cap, bias, sel):
    """The same fill with the u8 payload fetched through the dense u8
    lookup `lu` (keys 1..len(lu)): out[k-1] = lu[k2-1] + bias.  A row whose
    k2 is outside 1..len(lu) leaves its slot untouched."""
    out = np.zeros(cap, np.uint8)
    seen = set()
    for i in _selected(len(keys), sel):
        k, kk = int(keys[i]), int(k2[i])
        assert k not in seen, f"duplicate dense key {k}"
        seen.add(k)
        if not 1 <= k <= cap or not 1 <= kk <= len(lu):
            continue
        out[k - 1] = (int(lu[kk - 1]) + bias) % 256
    return out


def dense_present(arr):
    """What a probe of a dense table sees: {key: value} of the NONZERO
    slots (presence = nonzero)."""
    return {int(i) + 1: int(arr[i]) for i in np.flatnonzero(arr)}


def mode2_group_index(table, dense2, okey, skey, sel, group_vals):
    """Per probe row the index into group_vals it accumulates into, or -1.
    The header's wording, literally: the row passes sel; the key is found;
    1 <= skey <= len(dense2); g1 == dense2[skey-1]; the FIRST index of
    group_vals equal to it."""
    gv = [int(g) for g in group_vals]
    gi = np.full(len(okey), -1, np.int64)
    for i in _selected(len(okey), sel):
        g1 = table.get(int(okey[i]))
        if g1 is None:
            continue
        s = int(skey[i])
        if not 1 <= s <= len(dense2):
            continue
        g2 = int(dense2[s - 1])
        if g1 != g2 or g2 not in gv:
            continue
        gi[i] = gv.index(g2)
    return gi


def check_f64_domain(prod):
    """Every product must sit in the 64.64 domain, or the device sum is not
    the exact one and a test could pass or fail by accident."""
    prod = np.asarray(prod, np.float64)
    ok = (prod == 0.0) | ((prod >= FX_LO) & (prod < FX_HI))
    assert ok.all(), ("SUM_F64 addend outside the 64.64 domain: "
                      f"{prod[~ok][:4]}")


def mode2_aggregate(gi, ep_cents, dc_cents, ep, dc, group_vals):
    """Sums per group from the per-row group index.  Returns (rows,
    overflow): rows = [(group, sum_ticks, sum_f64, count)] in group_vals
    order without the empty groups; ticks = cents * (100 - dcents) as
    Python ints; sum_f64 = the correctly rounded exact sum (math.fsum) of
    the f64 products ep * (1.0 - dc), one subtract and one multiply each,
    as the device rounds them.  overflow: the exact tick sum of some group
    is outside int64."""
    prod = np.asarray(ep, np.float64) * (1.0 - np.asarray(dc, np.float64))
    check_f64_domain(prod)
    n_g = len(group_vals)
    ticks, parts, cnt = [0] * n_g, [[] for _ in range(n_g)], [0] * n_g
    for i in np.flatnonzero(np.asarray(gi) >= 0):
        g = int(gi[i])
        ticks[g] += int(ep_cents[i]) * (100 - int(dc_cents[i]))
        parts[g].append(float(prod[i]))
        cnt[g] += 1
    rows = [(int(group_vals[g]), ticks[g], math.fsum(parts[g]), cnt[g])
            for g in range(n_g) if cnt[g]]
    overflow = any(not I64_MIN <= t <= I64_MAX for t in ticks)
    return rows, overflow


def mode2_ref(table, dense2, okey, skey, ep_cents, dc_cents, ep, dc, sel,
              group_vals):
    """table: dict orderkey -> u8 payload; dense2: the dense u8 array of
    table2.  Returns (rows, overflow), see mode2_aggregate."""
    gi = mode2_group_index(table, dense2, okey, skey, sel, group_vals)
    return mode2_aggregate(gi, ep_cents, dc_cents, ep, dc, group_vals)
