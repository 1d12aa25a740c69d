"""C-ABI surface of PG_OP_WINDOW (CPU-only): the plan-size guard of kind
10, the unassigned kind 9, the ctypes mirror's layout, and loud failure
without a GPU."""
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


def test_plan_size_of_kind_10(solib):
    from presto_amd import engine as E
    assert E.OP_WINDOW == 10
    assert solib.pg_abi_plan_size(E.OP_WINDOW) == C.sizeof(E.PlanWindow)
    assert solib.pg_abi_plan_size(9) == -1      # left unassigned
    assert solib.pg_abi_plan_size(11) == -1


def test_mirror_layout():
    """pg_win_spec is four int32 and an int64; the function array starts
    on an 8-byte boundary after 28 int32."""
    from presto_amd import engine as E
    assert C.sizeof(E.WinSpec) == 24
    assert E.WinSpec.offset.offset == 16
    assert E.PlanWindow.n_partition_keys.offset == 4
    assert E.PlanWindow.key_col.offset == 8
    assert E.PlanWindow.order.offset == 24
    assert E.PlanWindow.n_emit.offset == 40
    assert E.PlanWindow.emit_cols.offset == 44
    assert E.PlanWindow.n_funcs.offset == 108
    assert E.PlanWindow.funcs.offset == 112
    assert C.sizeof(E.PlanWindow) == 112 + 8 * 24


def test_struct_size_list_keeps_its_twelve(solib):
    solib.pg_abi_struct_sizes.restype = C.c_int32
    assert solib.pg_abi_struct_sizes(None, 0) == 12


def test_create_fails_loudly_without_gpu(solib):
    n = C.c_int32()
    solib.pg_device_count(C.byref(n))
    from presto_amd import plans as pl
    plan = pl.window([pl.asc(0)], [pl.asc(1)], [0], [pl.row_number()])
    h = C.c_int64()
    st = solib.pg_op_create(10, C.byref(plan), C.sizeof(plan), C.byref(h))
    if n.value == 0:
        assert st != 0
        assert "no AMD GPU" in (solib.pg_last_error() or b"").decode()
    else:
        # with a GPU the same call must work, and a wrong size must not
        assert st == 0, solib.pg_last_error()
        solib.pg_op_destroy.argtypes = [C.c_int64]
        solib.pg_op_destroy(h.value)
        st = solib.pg_op_create(10, C.byref(plan), C.sizeof(plan) - 8,
                                C.byref(h))
        assert st != 0
        assert "plan size" in (solib.pg_last_error() or b"").decode()
