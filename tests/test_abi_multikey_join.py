"""C-ABI surface of the multi-key join fields (CPU-only):
pg_plan_hash_build and pg_plan_lookup_join end in n_keys / key_cols[4], the
library reports the grown sizes, a zeroed plan is the single-key path, and
engine.lib() checks the sizes when it loads the library."""
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
    lib.pg_abi_struct_sizes.restype = C.c_int32
    lib.pg_last_error.restype = C.c_char_p
    return lib


def test_plan_sizes_of_kinds_3_and_4(solib):
    from presto_amd import engine as E
    assert (E.OP_HASH_BUILD, E.OP_LOOKUP_JOIN) == (3, 4)
    assert solib.pg_abi_plan_size(3) == C.sizeof(E.PlanHashBuild)
    assert solib.pg_abi_plan_size(4) == C.sizeof(E.PlanLookupJoin)
    n = solib.pg_abi_struct_sizes(None, 0)
    sizes = (C.c_int32 * n)()
    solib.pg_abi_struct_sizes(sizes, n)
    assert sizes[7] == C.sizeof(E.PlanHashBuild)
    assert sizes[8] == C.sizeof(E.PlanLookupJoin)


@pytest.mark.parametrize("name", ["PlanHashBuild", "PlanLookupJoin"])
def test_new_fields_are_the_last_fields(name):
    from presto_amd import engine as E
    cls = getattr(E, name)
    assert [f[0] for f in cls._fields_[-2:]] == ["n_keys", "key_cols"]
    assert cls.key_cols.offset == cls.n_keys.offset + 4
    assert cls.key_cols.size == 16
    prev = getattr(cls, cls._fields_[-3][0])
    assert cls.n_keys.offset == prev.offset + prev.size
    # nothing but tail padding behind them
    assert C.sizeof(cls) == (cls.key_cols.offset + 16 + 7) // 8 * 8


@pytest.mark.parametrize("struct", ["pg_plan_hash_build",
                                    "pg_plan_lookup_join"])
def test_header_declares_them_last(struct):
    text = re.sub(r"/\*.*?\*/", "", HDR.read_text(), flags=re.S)
    body = text[:text.index("} " + struct + ";")]
    decls = [d.strip() for d in body.split(";") if d.strip()]
    assert decls[-2:] == ["int32_t n_keys", "int32_t key_cols[4]"]


@pytest.mark.parametrize("name", ["PlanHashBuild", "PlanLookupJoin"])
def test_zeroed_plan_is_the_single_key_path(name):
    from presto_amd import engine as E
    plan = getattr(E, name)()
    C.memset(C.byref(plan), 0xff, C.sizeof(plan))
    C.memset(C.byref(plan), 0, C.sizeof(plan))
    assert plan.n_keys == 0 and list(plan.key_cols) == [0, 0, 0, 0]


def test_counter_is_exported(solib):
    solib.pg_multikey_probe_pages.restype = C.c_int64
    assert solib.pg_multikey_probe_pages() >= 0


def test_engine_checks_sizes_at_load(monkeypatch):
    from presto_amd import engine as E
    L = E._Lib()                  # the real mirrors match the library
    assert L.c.pg_multikey_probe_pages() >= 0

    class Drifted(C.Structure):   # a mirror that lost its new fields
        _fields_ = E.PlanLookupJoin._fields_[:-2]

    structs = tuple(Drifted if s is E.PlanLookupJoin else s
                    for s in E._ABI_STRUCTS)
    monkeypatch.setattr(E, "_ABI_STRUCTS", structs)
    with pytest.raises(RuntimeError, match="Drifted"):
        E._Lib()


def test_create_fails_loudly_without_gpu(solib):
    n = C.c_int32()
    solib.pg_device_count(C.byref(n))
    if n.value:
        return  # with a GPU, test_gpu_multikey_join covers create
    from presto_amd import plans as pl
    plan = pl.hash_build([0, 1], payload=[2])
    h = C.c_int64()
    st = solib.pg_op_create(3, C.byref(plan), C.sizeof(plan), C.byref(h))
    assert st != 0
    assert "no AMD GPU" in (solib.pg_last_error() or b"").decode()
