"""ctypes binding of libpresto_gpu.so (the product C-ABI).

Mirrors include/presto_gpu.h exactly; see that header for the contract and
the reference citations.
"""
import contextlib
import ctypes as C
import pathlib

import numpy as np

_HERE = pathlib.Path(__file__).resolve().parent
_SO = _HERE / "libpresto_gpu.so"

# ---- enums (presto_gpu.h) ----
T_U8, T_I32, T_I64, T_F64, T_VARBIN, T_I128 = 0, 1, 2, 3, 4, 5
(CMP_LT, CMP_LE, CMP_GT, CMP_GE, CMP_EQ, CMP_NE, CMP_CONTAINS,
 CMP_PREFIX, CMP_CONTAINS2, CMP_NOT_CONTAINS2, CMP_IS_NULL,
 CMP_IS_NOT_NULL) = range(12)
# pg_plan_lookup_join.mode of the emit joins (PG_JOIN_*; 1-3 are the fused
# aggregating probes)
JOIN_INNER, JOIN_PROBE_OUTER, JOIN_LOOKUP_OUTER, JOIN_FULL_OUTER = 0, 4, 5, 6
(PROJ_IDENT, PROJ_DISC_PRICE, PROJ_CHARGE, PROJ_MUL, PROJ_DIV,
 PROJ_KEYSHL, PROJ_SHR, PROJ_SUBDIV, PROJ_KEYSHL_DIV) = range(9)
(AGG_COUNT, AGG_SUM_F64, AGG_SUM_DEC, AGG_SUM_I64,
 AGG_MIN, AGG_MAX) = range(6)
(OP_FILTER_PROJECT, OP_HASH_AGG_SMALL, OP_HASH_BUILD, OP_LOOKUP_JOIN,
 OP_TOPN, OP_PARTITION, OP_GROUPBY_MULTI, OP_ORDER_BY) = range(1, 9)
OP_WINDOW = 10  # 9 is left unassigned
OP_MARK_DISTINCT = 12  # 11 is left unassigned
# pg_plan_mark_distinct.mode (PG_DISTINCT_*)
DISTINCT_MARK, DISTINCT_ONLY = 0, 1
# pg_sort_order (SortOrder.java)
(SORT_ASC_NULLS_FIRST, SORT_ASC_NULLS_LAST, SORT_DESC_NULLS_FIRST,
 SORT_DESC_NULLS_LAST) = range(4)
# pg_win_func, pg_win_frame
(WIN_ROW_NUMBER, WIN_RANK, WIN_DENSE_RANK, WIN_COUNT, WIN_SUM, WIN_MIN,
 WIN_MAX, WIN_LAG, WIN_LEAD) = range(9)
FRAME_RANGE_RUNNING, FRAME_ROWS_RUNNING, FRAME_PARTITION = range(3)

_NP_TAG = {np.dtype(np.uint8): T_U8, np.dtype(np.int32): T_I32,
           np.dtype(np.int64): T_I64, np.dtype(np.float64): T_F64}
_TAG_NP = {v: k for k, v in _NP_TAG.items()}


class PgCol(C.Structure):
    _fields_ = [("tag", C.c_int32), ("on_device", C.c_int32),
                ("data", C.c_void_p), ("null_mask", C.c_void_p),
                ("offsets", C.c_void_p), ("dict_ids", C.c_void_p),
                ("dict_n", C.c_int32)]


class PgPage(C.Structure):
    _fields_ = [("n_rows", C.c_int64), ("n_cols", C.c_int32),
                ("cols", PgCol * 32)]


class Pred(C.Structure):
    _fields_ = [("col", C.c_int32), ("op", C.c_int32), ("ival", C.c_int64),
                ("dval", C.c_double), ("sval", C.c_char * 40),
                ("slen", C.c_int32), ("rhs_col", C.c_int32)]


class Proj(C.Structure):
    _fields_ = [("kind", C.c_int32), ("a", C.c_int32), ("b", C.c_int32),
                ("c", C.c_int32)]


class Agg(C.Structure):
    _fields_ = [("func", C.c_int32), ("proj", Proj), ("dec_scale", C.c_int32)]


class PlanFilterProject(C.Structure):
    _fields_ = [("n_preds", C.c_int32), ("preds", Pred * 8),
                ("n_proj", C.c_int32), ("proj", Proj * 16),
                ("semijoin_table", C.c_int64), ("semijoin_col", C.c_int32),
                ("semijoin_anti", C.c_int32)]


class PlanHashAggSmall(C.Structure):
    _fields_ = [("n_preds", C.c_int32), ("preds", Pred * 8),
                ("n_keys", C.c_int32), ("key_col", C.c_int32 * 2),
                ("n_vals", C.c_int32 * 2), ("key_vals", (C.c_uint8 * 8) * 2),
                ("n_aggs", C.c_int32), ("aggs", Agg * 8),
                ("drop_unlisted_keys", C.c_int32)]


class PlanHashBuild(C.Structure):
    _fields_ = [("n_preds", C.c_int32), ("preds", Pred * 8),
                ("key_col", C.c_int32), ("semijoin_table", C.c_int64),
                ("semijoin_col", C.c_int32), ("n_payload", C.c_int32),
                ("payload_col", C.c_int32 * 4), ("capacity_hint", C.c_int64),
                ("key_set_only", C.c_int32), ("dense_array", C.c_int32),
                ("payload_lookup_table", C.c_int64),
                ("payload_lookup_key_col", C.c_int32),
                ("agg_table", C.c_int32), ("pack_bits", C.c_int32),
                ("fill_x10", C.c_int32), ("bitmap_max_key", C.c_int64),
                ("range_group", C.c_int32),
                ("dense_payload_bias", C.c_int32),
                ("n_keys", C.c_int32), ("key_cols", C.c_int32 * 4)]


class PlanLookupJoin(C.Structure):
    _fields_ = [("table", C.c_int64), ("n_preds", C.c_int32),
                ("preds", Pred * 8), ("key_col", C.c_int32),
                ("mode", C.c_int32), ("n_emit", C.c_int32),
                ("emit_probe_cols", C.c_int32 * 8), ("proj", Proj),
                ("dec_scale", C.c_int32), ("table2", C.c_int64),
                ("table2_key_col", C.c_int32),
                ("n_group_vals", C.c_int32),
                ("group_vals", C.c_uint8 * 8), ("dec_only", C.c_int32),
                ("dec_min", C.c_int32), ("n_aggs", C.c_int32),
                ("aggs", Agg * 6), ("agg_filter", C.c_int32 * 6),
                ("acc_pack", C.c_int32), ("acc_pack_shift", C.c_int32 * 6),
                ("acc_pack_width", C.c_int32 * 6),
                ("acc_pack_cnt_shift", C.c_int32),
                ("acc_pack_cnt_width", C.c_int32),
                ("n_keys", C.c_int32), ("key_cols", C.c_int32 * 4)]


class PlanGroupBy(C.Structure):
    _fields_ = [("n_preds", C.c_int32), ("preds", Pred * 8),
                ("n_keys", C.c_int32), ("key_col", C.c_int32 * 4),
                ("capacity_hint", C.c_int64), ("n_aggs", C.c_int32),
                ("aggs", Agg * 6), ("agg_filter", C.c_int32 * 6),
                ("sql_nulls", C.c_int32)]


class PlanTopN(C.Structure):
    _fields_ = [("limit", C.c_int32), ("val_col", C.c_int32),
                ("date_col", C.c_int32), ("key_col", C.c_int32)]


class PlanPartition(C.Structure):
    _fields_ = [("n_partitions", C.c_int32), ("key_col", C.c_int32),
                ("n_emit", C.c_int32), ("emit_cols", C.c_int32 * 8)]


class PlanOrderBy(C.Structure):
    _fields_ = [("n_keys", C.c_int32), ("key_col", C.c_int32 * 4),
                ("order", C.c_int32 * 4), ("n_emit", C.c_int32),
                ("emit_cols", C.c_int32 * 16), ("limit", C.c_int64)]


class WinSpec(C.Structure):
    _fields_ = [("func", C.c_int32), ("col", C.c_int32),
                ("frame", C.c_int32), ("pad", C.c_int32),
                ("offset", C.c_int64)]


class PlanWindow(C.Structure):
    _fields_ = [("n_keys", C.c_int32), ("n_partition_keys", C.c_int32),
                ("key_col", C.c_int32 * 4), ("order", C.c_int32 * 4),
                ("n_emit", C.c_int32), ("emit_cols", C.c_int32 * 16),
                ("n_funcs", C.c_int32), ("funcs", WinSpec * 8)]


class PlanMarkDistinct(C.Structure):
    _fields_ = [("capacity_hint", C.c_int64), ("limit", C.c_int64),
                ("n_keys", C.c_int32), ("key_col", C.c_int32 * 4),
                ("mode", C.c_int32), ("n_emit", C.c_int32),
                ("emit_cols", C.c_int32 * 16)]


# pg_abi_struct_sizes order, and the plans pg_abi_plan_size alone reports
_ABI_STRUCTS = (PgCol, PgPage, Pred, Proj, Agg, PlanFilterProject,
                PlanHashAggSmall, PlanHashBuild, PlanLookupJoin, PlanGroupBy,
                PlanTopN, PlanPartition)
_ABI_PLANS = ((PlanOrderBy, OP_ORDER_BY), (PlanWindow, OP_WINDOW),
              (PlanMarkDistinct, OP_MARK_DISTINCT))


class _Lib:
    def __init__(self):
        if not _SO.exists():
            raise RuntimeError(
                f"{_SO} not built — run __graft_entry__.build() first "
                "(the product HIP library is required; no CPU fallback)")
        self.c = C.CDLL(str(_SO))
        self.c.pg_last_error.restype = C.c_char_p
        self.c.pg_op_create.argtypes = [C.c_int32, C.c_void_p, C.c_int64,
                                        C.POINTER(C.c_int64)]
        self.c.pg_op_add_input.argtypes = [C.c_int64, C.POINTER(PgPage)]
        self.c.pg_op_get_output.argtypes = [C.c_int64,
                                            C.POINTER(C.POINTER(PgPage))]
        for f in ("pg_op_finish", "pg_op_destroy", "pg_op_needs_input",
                  "pg_op_is_finished"):
            getattr(self.c, f).argtypes = [C.c_int64]
        self.c.pg_op_table.argtypes = [C.c_int64, C.POINTER(C.c_int64)]
        self.c.pg_op_partition_counts.argtypes = [C.c_int64,
                                                  C.POINTER(C.c_int64),
                                                  C.c_int32]
        self.c.pg_table_destroy.argtypes = [C.c_int64]
        self.c.pg_table_reset_acc.argtypes = [C.c_int64]
        self.c.pg_table_tag_bytes.argtypes = [C.c_int64]
        self.c.pg_table_tag_bytes.restype = C.c_int64
        self.c.pg_memcpy_d2h.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        self.c.pg_memcpy_d2d.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        self.c.pg_memcpy_h2d.argtypes = [C.c_void_p, C.c_void_p, C.c_int64]
        self.c.pg_device_sync.argtypes = []
        self.c.pg_abi_plan_size.argtypes = [C.c_int32]
        self.c.pg_abi_plan_size.restype = C.c_int32
        self.c.pg_sortkey_u64.argtypes = [C.c_int32, C.c_int32, C.c_uint64]
        self.c.pg_sortkey_u64.restype = C.c_uint64
        self.c.pg_multikey_probe_pages.argtypes = []
        self.c.pg_multikey_probe_pages.restype = C.c_int64
        self.c.pg_abi_struct_sizes.argtypes = [C.POINTER(C.c_int32),
                                               C.c_int32]
        self.c.pg_abi_struct_sizes.restype = C.c_int32
        self._check_struct_sizes()

    def _check_struct_sizes(self):
        """The load-time guard the header promises: every mirrored struct
        must be as large as the library compiled it."""
        n = self.c.pg_abi_struct_sizes(None, 0)
        sizes = (C.c_int32 * n)()
        self.c.pg_abi_struct_sizes(sizes, n)
        bad = [f"{cls.__name__}: ctypes {C.sizeof(cls)}, library {sz}"
               for cls, sz in zip(_ABI_STRUCTS, sizes)
               if C.sizeof(cls) != sz]
        for cls, kind in _ABI_PLANS:
            sz = self.c.pg_abi_plan_size(kind)
            if C.sizeof(cls) != sz:
                bad.append(f"{cls.__name__}: ctypes {C.sizeof(cls)}, "
                           f"library {sz}")
        if n < len(_ABI_STRUCTS):
            bad.append(f"pg_abi_struct_sizes reports {n} structs, the "
                       f"binding mirrors {len(_ABI_STRUCTS)}")
        if bad:
            raise RuntimeError(
                f"{_SO} does not match the ctypes mirrors of "
                "include/presto_gpu.h (rebuild the library): "
                + "; ".join(bad))

    def err(self):
        return (self.c.pg_last_error() or b"").decode()

    def check(self, st, what):
        if st != 0:
            raise RuntimeError(f"{what}: {self.err()}")


_lib = None


def lib():
    global _lib
    if _lib is None:
        _lib = _Lib()
    return _lib


class Varbin:
    """A host VariableWidthBlock column (VariableWidthBlock.java:48-61):
    concatenated bytes + n+1 int32 offsets."""

    def __init__(self, strings):
        self.offsets = np.zeros(len(strings) + 1, np.int32)
        for i, b in enumerate(strings):
            self.offsets[i + 1] = self.offsets[i] + len(b)
        joined = b"".join(strings)
        self.data = np.frombuffer(joined, np.uint8).copy() if joined \
            else np.empty(0, np.uint8)
        self.n = len(strings)

    @classmethod
    def from_arrays(cls, data, offsets):
        """Wrap an existing layout: uint8 bytes + int32 offsets (n+1)."""
        v = cls.__new__(cls)
        v.data = np.ascontiguousarray(data, np.uint8)
        v.offsets = np.ascontiguousarray(offsets, np.int32)
        v.n = len(v.offsets) - 1
        return v

    def __len__(self):
        return self.n

    def tolist(self):
        return [self.data[self.offsets[i]:self.offsets[i + 1]].tobytes()
                for i in range(self.n)]


class DictVarbin:
    """A host DictionaryBlock over a Varbin dictionary
    (DictionaryBlock.java:60-86): per-position int32 ids into the
    dictionary entries."""

    def __init__(self, dictionary_strings, ids):
        self.dictionary = Varbin(dictionary_strings)
        self.ids = np.ascontiguousarray(ids, np.int32)

    def __len__(self):
        return len(self.ids)


class DeviceVarbin:
    """A VariableWidthBlock resident in HBM: torch-cuda uint8 bytes +
    int32 offsets (+ optional int32 dictionary ids for DictionaryBlock
    columns).  The boundary form of Varbin/DictVarbin once a page has
    been staged."""

    def __init__(self, data, offsets, dict_ids=None, dict_n=0):
        self.data = data          # torch.uint8 cuda tensor
        self.offsets = offsets    # torch.int32 cuda tensor (n+1)
        self.dict_ids = dict_ids  # torch.int32 cuda tensor or None
        self.dict_n = dict_n

    @classmethod
    def from_host(cls, v):
        import torch
        if isinstance(v, DictVarbin):
            return cls(torch.from_numpy(v.dictionary.data).cuda(),
                       torch.from_numpy(v.dictionary.offsets).cuda(),
                       torch.from_numpy(v.ids).cuda(), v.dictionary.n)
        return cls(torch.from_numpy(v.data).cuda(),
                   torch.from_numpy(v.offsets).cuda())

    def __len__(self):
        n = len(self.dict_ids) if self.dict_ids is not None             else len(self.offsets) - 1
        return n


class Page:
    """A Presto Page: named columns backed by numpy (host) or torch-cuda
    (device) arrays (Varbin / DeviceVarbin for variable-width columns).
    Column order is the channel order.  nulls maps a column name to its
    null mask, one uint8 per row with 1 = null: a numpy array for a host
    column, a CUDA tensor for a device column.  The page keeps the masks
    alive, like the columns."""

    def __init__(self, cols, n_rows=None, nulls=None):
        self.names = list(cols.keys())
        self.cols = cols
        first = next(iter(cols.values()))
        self.n_rows = n_rows if n_rows is not None else len(first)
        self.nulls = {}
        for name, m in (nulls or {}).items():
            if name not in cols:
                raise ValueError(f"nulls: no column {name!r}")
            on_device = not isinstance(
                cols[name], (np.ndarray, Varbin, DictVarbin))
            if isinstance(m, np.ndarray) == on_device:
                raise ValueError(
                    f"nulls[{name!r}]: a host column takes a numpy mask, "
                    "a device column a CUDA tensor")
            if on_device:
                import torch
                ok = (isinstance(m, torch.Tensor) and m.is_cuda
                      and m.dtype == torch.uint8 and m.dim() == 1
                      and m.is_contiguous())
            else:
                ok = m.dtype == np.uint8 and m.ndim == 1 \
                    and m.flags.c_contiguous
            if not ok:
                raise ValueError(f"nulls[{name!r}]: mask must be a "
                                 "contiguous 1-d uint8 array")
            if len(m) != self.n_rows:
                raise ValueError(f"nulls[{name!r}]: {len(m)} entries for "
                                 f"{self.n_rows} rows")
            self.nulls[name] = m

    def channel(self, name):
        return self.names.index(name)

    def to_c(self):
        pg = PgPage()
        pg.n_rows = self.n_rows
        pg.n_cols = len(self.names)
        for i, name in enumerate(self.names):
            a = self.cols[name]
            col = PgCol()
            if isinstance(a, DeviceVarbin):
                col.tag = T_VARBIN
                col.on_device = 1
                col.data = a.data.data_ptr()
                col.offsets = a.offsets.data_ptr()
                if a.dict_ids is not None:
                    col.dict_ids = a.dict_ids.data_ptr()
                    col.dict_n = a.dict_n
            elif isinstance(a, Varbin):
                col.tag = T_VARBIN
                col.on_device = 0
                col.data = a.data.ctypes.data
                col.offsets = a.offsets.ctypes.data
            elif isinstance(a, DictVarbin):
                col.tag = T_VARBIN
                col.on_device = 0
                col.data = a.dictionary.data.ctypes.data
                col.offsets = a.dictionary.offsets.ctypes.data
                col.dict_ids = a.ids.ctypes.data
                col.dict_n = a.dictionary.n
            elif isinstance(a, np.ndarray):
                col.tag = _NP_TAG[a.dtype]
                col.on_device = 0
                col.data = a.ctypes.data
            else:  # torch tensor on cuda
                import torch
                assert isinstance(a, torch.Tensor) and a.is_cuda
                tagmap = {torch.uint8: T_U8, torch.int32: T_I32,
                          torch.int64: T_I64, torch.float64: T_F64}
                col.tag = tagmap[a.dtype]
                col.on_device = 1
                col.data = a.data_ptr()
            m = self.nulls.get(name)
            if m is None:
                col.null_mask = None
            elif isinstance(m, np.ndarray):
                col.null_mask = m.ctypes.data
            else:
                col.null_mask = m.data_ptr()
            pg.cols[i] = col
        return pg


def _read_output_page(cpage, names=None, nulls=None):
    """Copy an output pg_page (host or device cols) into numpy arrays.
    With a dict passed as nulls, the null masks the page carries are
    copied into it under the column names."""
    L = lib()
    n = cpage.n_rows
    out = {}
    for i in range(cpage.n_cols):
        col = cpage.cols[i]
        if nulls is not None and col.null_mask:
            m = np.empty(n, np.uint8)
            if n:
                if col.on_device:
                    L.check(L.c.pg_memcpy_d2h(m.ctypes.data, col.null_mask,
                                              n), "d2h")
                else:
                    C.memmove(m.ctypes.data, col.null_mask, n)
            nulls[names[i] if names else f"c{i}"] = m
        if col.tag == T_VARBIN:
            offs = np.empty(n + 1, np.int32)
            if col.on_device:
                L.check(L.c.pg_memcpy_d2h(offs.ctypes.data, col.offsets,
                                          (n + 1) * 4), "d2h")
            else:
                C.memmove(offs.ctypes.data, col.offsets, (n + 1) * 4)
            nb = int(offs[n])
            data = np.empty(nb, np.uint8)
            if nb:
                if col.on_device:
                    L.check(L.c.pg_memcpy_d2h(data.ctypes.data, col.data,
                                              nb), "d2h")
                else:
                    C.memmove(data.ctypes.data, col.data, nb)
            out[names[i] if names else f"c{i}"] = Varbin.from_arrays(data,
                                                                     offs)
            continue
        dt = _TAG_NP[col.tag]
        a = np.empty(n, dt)
        nbytes = n * dt.itemsize
        if nbytes:
            if col.on_device:
                L.check(L.c.pg_memcpy_d2h(a.ctypes.data, col.data, nbytes),
                        "d2h")
            else:
                C.memmove(a.ctypes.data, col.data, nbytes)
        out[names[i] if names else f"c{i}"] = a
    return out


class Operator:
    """Host mirror of operator/Operator.java:20-102 over the C-ABI."""

    def __init__(self, kind, plan):
        L = lib()
        h = C.c_int64()
        L.check(L.c.pg_op_create(kind, C.byref(plan), C.sizeof(plan),
                                 C.byref(h)), "op_create")
        self.h = h.value
        self.kind = kind

    def needs_input(self):
        return bool(lib().c.pg_op_needs_input(self.h))

    def add_input(self, page: Page):
        L = lib()
        cp = page.to_c()
        L.check(L.c.pg_op_add_input(self.h, C.byref(cp)), "add_input")

    def add_input_raw(self, cpage: PgPage):
        """Feed another operator's raw output page (device pointers pass
        through without copies — pages are borrowed for the call)."""
        L = lib()
        L.check(L.c.pg_op_add_input(self.h, C.byref(cpage)), "add_input")

    def feed(self, page):
        """add_input of a Page, or of another operator's raw PgPage."""
        if isinstance(page, PgPage):
            self.add_input_raw(page)
        else:
            self.add_input(page)

    def get_output(self, names=None):
        """Returns dict of numpy arrays, or None. (Materializes device
        outputs to host for harness use; device-to-device chaining uses
        get_output_raw.)"""
        L = lib()
        pp = C.POINTER(PgPage)()
        L.check(L.c.pg_op_get_output(self.h, C.byref(pp)), "get_output")
        if not pp:
            return None
        return _read_output_page(pp.contents, names)

    def get_output_nulls(self, names=None):
        """get_output plus the null masks: (cols, nulls) or None, nulls
        holding a uint8 array (1 = null) for exactly the columns whose
        output carries a mask."""
        L = lib()
        pp = C.POINTER(PgPage)()
        L.check(L.c.pg_op_get_output(self.h, C.byref(pp)), "get_output")
        if not pp:
            return None
        nulls = {}
        return _read_output_page(pp.contents, names, nulls), nulls

    def get_output_raw(self):
        """Returns a snapshot of the raw PgPage descriptor (device pointers
        stay on device) or None.  The column BUFFERS it points at are owned
        by the library: valid until the next get_output on this operator
        (PARTITION: until destroy — its pages alias op-owned buffers)."""
        L = lib()
        pp = C.POINTER(PgPage)()
        L.check(L.c.pg_op_get_output(self.h, C.byref(pp)), "get_output")
        if not pp:
            return None
        snap = PgPage()
        C.memmove(C.byref(snap), pp, C.sizeof(PgPage))
        return snap

    def finish(self):
        lib().check(lib().c.pg_op_finish(self.h), "finish")

    def is_finished(self):
        return bool(lib().c.pg_op_is_finished(self.h))

    def table(self):
        t = C.c_int64()
        lib().check(lib().c.pg_op_table(self.h, C.byref(t)), "table")
        return t.value

    def partition_counts(self, n):
        arr = (C.c_int64 * n)()
        lib().check(lib().c.pg_op_partition_counts(self.h, arr, n),
                    "partition_counts")
        return list(arr)

    def destroy(self):
        h, self.h = self.h, None
        if h is not None:
            lib().c.pg_op_destroy(h)

    def __del__(self):
        # guard on self.h so a stale finalizer can never destroy a live
        # operator if handle reuse is ever introduced
        try:
            if _lib is not None and self.h is not None:
                _lib.c.pg_op_destroy(self.h)
                self.h = None
        except Exception:
            pass


class Scope:
    """Owns the operators and hash tables of one query (or one long-lived
    pipeline object).  Leaving the scope — normally or by exception —
    destroys whatever is still alive in reverse order of creation, so a
    probe always goes before the table it points at.  release() frees
    intermediates early (their buffers go back to the size-bucketed pool
    for the next operator); releasing or closing twice is harmless."""

    def __init__(self):
        self._live = []  # [operator, table handle or None], creation order

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()

    @contextlib.contextmanager
    def on_error(self):
        """For an owner that outlives the block (a pipeline's __init__):
        close only if the block raises."""
        try:
            yield self
        except BaseException:
            self.close()
            raise

    def op(self, kind, plan):
        op = Operator(kind, plan)
        self._live.append([op, None])
        return op

    def pipe(self, kind, plan, page):
        """Streaming operator over one page (Page, or another operator's
        raw PgPage): returns (operator, its raw output page)."""
        op = self.op(kind, plan)
        op.feed(page)
        return op, op.get_output_raw()

    def run(self, kind, plan, *pages):
        """Accumulating operator: feed the pages and finish."""
        op = self.op(kind, plan)
        for pg in pages:
            op.feed(pg)
        op.finish()
        return op

    def build(self, plan, *pages):
        """HASH_BUILD over the pages; its table is recorded (and owned)
        once the build has finished."""
        b = self.run(OP_HASH_BUILD, plan, *pages)
        self._live[-1][1] = b.table()
        return b

    def _free_table(self, handle):
        lib().c.pg_table_destroy(handle)

    def release(self, *ops):
        for op in ops:
            for i, (o, tbl) in enumerate(self._live):
                if o is op:
                    del self._live[i]
                    if tbl is not None:
                        self._free_table(tbl)
                    op.destroy()
                    break

    def close(self):
        while self._live:
            self.release(self._live[-1][0])
