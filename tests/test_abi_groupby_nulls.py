"""C-ABI surface of pg_plan_groupby.sql_nulls (CPU-only): the plan size
of kind 7 follows the new last field, and create fails loudly without a
GPU."""
import ctypes as C
import pathlib

import pytest

REPO = pathlib.Path(__file__).resolve().parent.parent
SO = REPO / "presto_amd" / "libpresto_gpu.so"


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
    lib.pg_last_error.restype = C.c_char_p
    return lib


def test_plan_size_of_kind_7(solib):
    from presto_amd import engine as E
    assert E.OP_GROUPBY_MULTI == 7
    assert hasattr(E.PlanGroupBy, "sql_nulls")
    assert solib.pg_abi_plan_size(7) == C.sizeof(E.PlanGroupBy)


def test_field_offset_follows_agg_filter():
    from presto_amd import engine as E
    f = E.PlanGroupBy
    assert f.sql_nulls.offset == f.agg_filter.offset + 6 * 4
    assert C.sizeof(f) == (f.sql_nulls.offset + 4 + 7) // 8 * 8


def test_create_fails_loudly_without_gpu(solib):
    n = C.c_int32()
    solib.pg_device_count(C.byref(n))
    from presto_amd import plans as pl
    plan = pl.group_by([0], [pl.sum_i64(pl.ident(1))], 64, sql_nulls=True)
    h = C.c_int64()
    st = solib.pg_op_create(7, C.byref(plan), C.sizeof(plan), C.byref(h))
    if n.value == 0:
        assert st != 0
        assert "no AMD GPU" in (solib.pg_last_error() or b"").decode()
    else:
        # with a GPU the same call must work; a value other than 0 / 1 and
        # a plan of the size before the field must not
        assert st == 0, solib.pg_last_error()
        solib.pg_op_destroy.argtypes = [C.c_int64]
        solib.pg_op_destroy(h.value)
        plan.sql_nulls = 2
        st = solib.pg_op_create(7, C.byref(plan), C.sizeof(plan),
                                C.byref(h))
        assert st != 0
        assert "sql_nulls" in (solib.pg_last_error() or b"").decode()
        plan.sql_nulls = 1
        st = solib.pg_op_create(7, C.byref(plan), C.sizeof(plan) - 8,
                                C.byref(h))
        assert st != 0
        assert "plan size" in (solib.pg_last_error() or b"").decode()
