"""C-ABI surface of PG_OP_MARK_DISTINCT (CPU-only): the plan-size guard of
kind 12, the ctypes mirror's layout against the header's struct, the enums
against the header, and loud failure without a GPU."""
import ctypes as C
import pathlib
import re

import pytest

REPO = pathlib.Path(__file__).resolve().parent.parent
SO = REPO / "presto_amd" / "libpresto_gpu.so"
HDR = REPO / "include" / "presto_gpu.h"


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


def test_plan_size_of_kind_12(solib):
    from presto_amd import engine as E
    assert E.OP_MARK_DISTINCT == 12
    assert solib.pg_abi_plan_size(12) == C.sizeof(E.PlanMarkDistinct)
    assert solib.pg_abi_plan_size(11) == -1     # left unassigned
    assert solib.pg_abi_plan_size(13) == -1


def test_struct_size_list_keeps_its_twelve(solib):
    solib.pg_abi_struct_sizes.restype = C.c_int32
    assert solib.pg_abi_struct_sizes(None, 0) == 12


_C_TYPES = {"int32_t": C.c_int32, "int64_t": C.c_int64}


def _header_struct():
    """pg_plan_mark_distinct as the header declares it, rebuilt field by
    field under the C layout rules ctypes applies to a fresh Structure."""
    text = HDR.read_text()
    body = re.search(r"typedef struct \{((?:(?!typedef struct).)*?)\}\s*"
                     r"pg_plan_mark_distinct;", text, re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    fields = []
    for ctype, name, dim in re.findall(
            r"(int32_t|int64_t)\s+(\w+)\s*(?:\[(\d+)\])?\s*;", body):
        t = _C_TYPES[ctype]
        fields.append((name, t * int(dim) if dim else t))
    return type("HdrPlan", (C.Structure,), {"_fields_": fields})


def test_mirror_matches_the_header_struct():
    from presto_amd import engine as E
    H = _header_struct()
    names = [n for n, _ in H._fields_]
    assert sorted(names) == sorted(
        ["n_keys", "key_col", "mode", "n_emit", "emit_cols",
         "capacity_hint", "limit"])
    assert [n for n, _ in E.PlanMarkDistinct._fields_] == names
    for n in names:
        assert getattr(E.PlanMarkDistinct, n).offset == \
            getattr(H, n).offset, n
        assert getattr(E.PlanMarkDistinct, n).size == getattr(H, n).size, n
    assert C.sizeof(E.PlanMarkDistinct) == C.sizeof(H)


def test_mirror_layout():
    """Two int64 first, then 23 int32: no hole inside, four bytes of tail
    padding."""
    from presto_amd import engine as E
    P = E.PlanMarkDistinct
    assert (P.capacity_hint.offset, P.limit.offset) == (0, 8)
    assert (P.n_keys.offset, P.key_col.offset) == (16, 20)
    assert (P.mode.offset, P.n_emit.offset, P.emit_cols.offset) == \
        (36, 40, 44)
    assert C.sizeof(P) == 112


def test_enums_match_the_header():
    from presto_amd import engine as E
    text = HDR.read_text()
    assert re.search(r"PG_OP_MARK_DISTINCT\s*=\s*12\b", text)
    assert int(re.search(r"#define PG_DISTINCT_MARK (\d+)", text).group(1)) \
        == E.DISTINCT_MARK == 0
    assert int(re.search(r"#define PG_DISTINCT_ONLY (\d+)", text).group(1)) \
        == E.DISTINCT_ONLY == 1


def test_create_fails_loudly_without_gpu(solib):
    n = C.c_int32()
    solib.pg_device_count(C.byref(n))
    from presto_amd import plans as pl
    plan = pl.mark_distinct([0], [0], 16)
    h = C.c_int64()
    st = solib.pg_op_create(12, C.byref(plan), C.sizeof(plan), C.byref(h))
    if n.value == 0:
        assert st != 0
        assert "no AMD GPU" in (solib.pg_last_error() or b"").decode()
    else:
        # with a GPU the same call must work, and a wrong size must not
        assert st == 0, solib.pg_last_error()
        solib.pg_op_destroy.argtypes = [C.c_int64]
        solib.pg_op_destroy(h.value)
        st = solib.pg_op_create(12, C.byref(plan), C.sizeof(plan) - 8,
                                C.byref(h))
        assert st != 0
        assert "plan size" in (solib.pg_last_error() or b"").decode()
