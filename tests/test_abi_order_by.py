"""C-ABI surface of PG_OP_ORDER_BY (CPU-only): the plan-size guard, loud
failure without a GPU, and the sortable-key transform of csrc/sortkey.h —
the code k_sort_encode runs — checked through the host hook
pg_sortkey_u64 against the comparator of order_by_refs.py."""
import ctypes as C
import itertools
import pathlib
import struct

import numpy as np
import pytest

import order_by_refs as R

REPO = pathlib.Path(__file__).resolve().parent.parent
SO = REPO / "presto_amd" / "libpresto_gpu.so"

T_U8, T_I32, T_I64, T_F64 = 0, 1, 2, 3


@pytest.fixture(scope="module")
def solib():
    if not SO.exists():
        import subprocess
        subprocess.run(["hipcc", "--offload-arch=gfx950", "-O3",
                        "-std=c++17", "-fPIC", "-ffp-contract=off", "-shared",
                        str(REPO / "presto_amd/csrc/kernels.hip"),
                        "-o", str(SO)], check=True)
    lib = C.CDLL(str(SO))
    lib.pg_abi_plan_size.argtypes = [C.c_int32]
    lib.pg_abi_plan_size.restype = C.c_int32
    lib.pg_sortkey_u64.argtypes = [C.c_int32, C.c_int32, C.c_uint64]
    lib.pg_sortkey_u64.restype = C.c_uint64
    lib.pg_last_error.restype = C.c_char_p
    return lib


def test_plan_size_of_every_kind(solib):
    from presto_amd import engine as E
    mirrors = {E.OP_FILTER_PROJECT: E.PlanFilterProject,
               E.OP_HASH_AGG_SMALL: E.PlanHashAggSmall,
               E.OP_HASH_BUILD: E.PlanHashBuild,
               E.OP_LOOKUP_JOIN: E.PlanLookupJoin,
               E.OP_TOPN: E.PlanTopN,
               E.OP_PARTITION: E.PlanPartition,
               E.OP_GROUPBY_MULTI: E.PlanGroupBy,
               E.OP_ORDER_BY: E.PlanOrderBy}
    assert sorted(mirrors) == list(range(1, 9))
    for kind, m in mirrors.items():
        assert solib.pg_abi_plan_size(kind) == C.sizeof(m), m.__name__
    assert solib.pg_abi_plan_size(8) == C.sizeof(E.PlanOrderBy)


@pytest.mark.parametrize("kind", [0, 9, -1, 1000])
def test_plan_size_of_unknown_kind(solib, kind):
    assert solib.pg_abi_plan_size(kind) == -1


def test_struct_size_list_keeps_its_twelve(solib):
    solib.pg_abi_struct_sizes.restype = C.c_int32
    assert solib.pg_abi_struct_sizes(None, 0) == 12


def test_create_fails_loudly_without_gpu(solib):
    n = C.c_int32()
    solib.pg_device_count(C.byref(n))
    from presto_amd import plans as pl
    plan = pl.order_by([pl.asc(0)], [0])
    h = C.c_int64()
    st = solib.pg_op_create(8, C.byref(plan), C.sizeof(plan), C.byref(h))
    if n.value == 0:
        assert st != 0
        assert "no AMD GPU" in (solib.pg_last_error() or b"").decode()
    else:
        # with a GPU the same call must work, and a wrong size must not
        assert st == 0, solib.pg_last_error()
        solib.pg_op_destroy.argtypes = [C.c_int64]
        solib.pg_op_destroy(h.value)
        st = solib.pg_op_create(8, C.byref(plan), C.sizeof(plan) - 8,
                                C.byref(h))
        assert st != 0
        assert "plan size" in (solib.pg_last_error() or b"").decode()


# ---- the transform: every pair, all four orders ----
def _f(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


I64_EDGES = [-2**63, -1, 0, 1, 2**63 - 1]
I32_EDGES = [-2**31, -1, 0, 1, 2**31 - 1]
U8_EDGES = [0, 127, 128, 255]
F64_EDGE_BITS = [
    _f(float("inf")), _f(float("-inf")), _f(0.0), _f(-0.0),
    _f(5e-324), _f(-5e-324), _f(1.5), _f(-1.5),
    _f(1.7976931348623157e308), _f(-1.7976931348623157e308),
    0x7ff8000000000000,   # canonical quiet NaN
    0xfff8000000000000,   # negative quiet NaN
    0x7ff0000000000001,   # signalling, smallest payload
    0xfff00000deadbeef,   # negative, another payload
    0x7fffffffffffffff,   # all payload bits
]

CASES = [(T_I64, np.int64, I64_EDGES), (T_I32, np.int32, I32_EDGES),
         (T_U8, np.uint8, U8_EDGES), (T_F64, np.float64, F64_EDGE_BITS)]


def _bits(tag, v):
    """What the kernel loads for a value: its bit pattern, zero-extended."""
    if tag == T_I64:
        return v & 0xffffffffffffffff
    if tag == T_I32:
        return v & 0xffffffff
    return v   # U8 values and F64 bit patterns are already unsigned


@pytest.mark.parametrize("tag,dtype,edges", CASES,
                         ids=["i64", "i32", "u8", "f64"])
@pytest.mark.parametrize("order", R.ORDERS)
def test_sortkey_orders_every_pair_like_the_reference(solib, tag, dtype,
                                                      edges, order):
    desc = order in (R.DESC_NULLS_FIRST, R.DESC_NULLS_LAST)
    enc = [solib.pg_sortkey_u64(tag, order, _bits(tag, v)) for v in edges]
    for (a, ea), (b, eb) in itertools.product(zip(edges, enc), repeat=2):
        want = R.compare_values(dtype, a, b)
        if desc:
            want = -want
        got = (ea > eb) - (ea < eb)
        assert got == want, (tag, order, hex(_bits(tag, a)),
                             hex(_bits(tag, b)), hex(ea), hex(eb))


def test_sortkey_null_placement_is_not_in_the_key(solib):
    """NULLS FIRST / LAST are a pass of their own: the two ASC orders
    encode alike, and so do the two DESC orders."""
    for tag, _, edges in CASES:
        for v in edges:
            b = _bits(tag, v)
            assert solib.pg_sortkey_u64(tag, 0, b) == \
                solib.pg_sortkey_u64(tag, 1, b)
            assert solib.pg_sortkey_u64(tag, 2, b) == \
                solib.pg_sortkey_u64(tag, 3, b)


def test_sortkey_i32_stays_in_the_low_half(solib):
    """I32 keys leave the high 32 bits equal across rows, so their four
    high radix passes are always skipped."""
    for order in R.ORDERS:
        for v in I32_EDGES:
            assert solib.pg_sortkey_u64(T_I32, order, _bits(T_I32, v)) >> 32 \
                == 0
