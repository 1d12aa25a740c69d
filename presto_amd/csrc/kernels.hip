/* kernels.hip — MI355X-native (gfx950/CDNA4) implementation of Presto's
 * per-Page operator hot path behind the C-ABI of include/presto_gpu.h.
 *
 * Built from scratch for CDNA4: wave64 ballots for selection compaction,
 * per-thread register accumulators + deterministic xor-butterfly reductions
 * for aggregation, HBM-resident open-address tables with atomicCAS inserts
 * for join build/probe, exact 64.64 fixed-point f64 summation (fixed128.h)
 * so grouped double sums are order-independent and bit-deterministic.
 *
 * Reference semantics restated per operator (file:line cites in the plan
 * structs of presto_gpu.h and per kernel below).  This library has NO CPU
 * fallback: every op fails loudly without a GPU.
 */
#include <hip/hip_runtime.h>
#include <stdio.h>
#include <stdlib.h>
#include <string.h>
#include <map>
#include <vector>
#include <algorithm>
#include <type_traits>
#include <stdexcept>
#include <string>

#include "../../include/presto_gpu.h"
#include "fixed128.h"
#include "sortkey.h"

/* ------------------------------------------------------------------ */
/* error handling                                                     */
/* ------------------------------------------------------------------ */
static __thread char g_err[512];
extern "C" const char* pg_last_error(void) { return g_err; }
static pg_status seterr(const char* msg)
{
    snprintf(g_err, sizeof(g_err), "%s", msg);
    return PG_ERR;
}
#define CHK(x)                                                          \
    do {                                                                \
        hipError_t e_ = (x);                                            \
        if (e_ != hipSuccess) {                                         \
            snprintf(g_err, sizeof(g_err), "%s:%d %s", __FILE__,        \
                     __LINE__, hipGetErrorString(e_));                  \
            return PG_ERR;                                              \
        }                                                               \
    } while (0)
#define CHKV(x)                                                         \
    do {                                                                \
        hipError_t e_ = (x);                                            \
        if (e_ != hipSuccess) {                                         \
            snprintf(g_err, sizeof(g_err), "%s:%d %s", __FILE__,        \
                     __LINE__, hipGetErrorString(e_));                  \
            throw std::runtime_error(g_err);                            \
        }                                                               \
    } while (0)

static hipStream_t g_stream = nullptr;
static bool g_have_gpu = false;
static pg_status ensure_gpu()
{
    static int state = 0; /* 0 unknown, 1 ok, -1 none */
    if (state == 0) {
        int n = 0;
        hipError_t e = hipGetDeviceCount(&n);
        if (e != hipSuccess || n == 0) {
            state = -1;
        } else {
            if (hipStreamCreateWithFlags(&g_stream, hipStreamNonBlocking) !=
                hipSuccess)
                state = -1;
            else
                state = 1;
        }
    }
    g_have_gpu = state == 1;
    if (state != 1)
        return seterr("presto_gpu: no AMD GPU available — this library has "
                      "no CPU fallback");
    return PG_OK;
}

/* ------------------------------------------------------------------ */
/* exported device helpers                                            */
/* ------------------------------------------------------------------ */
extern "C" pg_status pg_device_count(int32_t* out)
{
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) n = 0;
    *out = n;
    return PG_OK;
}
extern "C" pg_status pg_device_sync(void)
{
    if (ensure_gpu()) return PG_ERR;
    CHK(hipDeviceSynchronize());
    return PG_OK;
}
extern "C" pg_status pg_device_malloc(int64_t bytes, void** out)
{
    if (ensure_gpu()) return PG_ERR;
    CHK(hipMalloc(out, (size_t)bytes));
    return PG_OK;
}
extern "C" pg_status pg_device_free(void* p)
{
    if (ensure_gpu()) return PG_ERR;
    CHK(hipFree(p));
    return PG_OK;
}
extern "C" pg_status pg_memcpy_h2d(void* d, const void* s, int64_t n)
{
    if (ensure_gpu()) return PG_ERR;
    CHK(hipMemcpy(d, s, (size_t)n, hipMemcpyHostToDevice));
    return PG_OK;
}
extern "C" pg_status pg_memcpy_d2h(void* d, const void* s, int64_t n)
{
    if (ensure_gpu()) return PG_ERR;
    CHK(hipMemcpy(d, s, (size_t)n, hipMemcpyDeviceToHost));
    return PG_OK;
}
extern "C" pg_status pg_memcpy_d2d(void* d, const void* s, int64_t n)
{
    if (ensure_gpu()) return PG_ERR;
    CHK(hipMemcpy(d, s, (size_t)n, hipMemcpyDeviceToDevice));
    return PG_OK;
}

/* HIP-event elapsed time of the most recent hot-path kernel launch
 * (the fused agg or probe-agg kernel), for bench.py's roofline leg.
 * Events are recorded on g_stream, the stream the kernel launches on. */
static double g_last_hot_ms = 0.0;
static double g_hot_max_ms = 0.0; /* max hot region since pg_hot_reset */
static hipEvent_t g_ev0, g_ev1;
static bool g_ev_init = false;
static void hot_begin()
{
    hipError_t e;
    if (!g_ev_init) {
        e = hipEventCreate(&g_ev0);
        e = hipEventCreate(&g_ev1);
        g_ev_init = true;
    }
    e = hipEventRecord(g_ev0, g_stream);
    (void)e;
}
static void hot_end()
{
    hipError_t e;
    e = hipEventRecord(g_ev1, g_stream);
    e = hipEventSynchronize(g_ev1);
    float ms = 0;
    e = hipEventElapsedTime(&ms, g_ev0, g_ev1);
    (void)e;
    g_last_hot_ms = ms;
    if (ms > g_hot_max_ms) g_hot_max_ms = ms;
}
extern "C" double pg_last_hot_kernel_ms(void) { return g_last_hot_ms; }
extern "C" double pg_hot_max_ms(void) { return g_hot_max_ms; }
extern "C" void pg_hot_reset(void) { g_hot_max_ms = 0.0; }
static int64_t g_q1_fast_launches = 0;
extern "C" int64_t pg_q1_fast_launches(void) { return g_q1_fast_launches; }
static int64_t g_build_staged_launches = 0;
extern "C" int64_t pg_build_staged_launches(void)
{
    return g_build_staged_launches;
}
static int64_t g_mode2_q5_launches = 0;
extern "C" int64_t pg_mode2_q5_launches(void) { return g_mode2_q5_launches; }
static int64_t g_groups_list_extractions = 0;
extern "C" int64_t pg_groups_list_extractions(void)
{
    return g_groups_list_extractions;
}
static int64_t g_multikey_probe_pages = 0;
extern "C" int64_t pg_multikey_probe_pages(void)
{
    return g_multikey_probe_pages;
}

/* ------------------------------------------------------------------ */
/* device helpers                                                     */
/* ------------------------------------------------------------------ */
#define WAVE 64
#define FT_NBLOCKS 4096
#define FT_NTHREADS 256
#define FT_VL ((int64_t)FT_NBLOCKS * FT_NTHREADS)
static const int64_t TBL_EMPTY = INT64_MIN; /* reserved key (documented) */

/* one-byte tag per slot (the PagesHash.java:110 byte-tag idea, adapted):
 * tag = high byte of the bucket hash, forced nonzero; 0 = empty slot.
 * The tag array is 1/8 the key array and stays L3-resident, so the ~90%
 * probe misses of Q3 are rejected without touching the HBM key lines. */
__device__ __host__ inline uint8_t d_tbl_tag(uint64_t h)
{
    return (uint8_t)((h >> 56) | 1);
}

__device__ inline double d_load_f64(const pg_col& c, int64_t i)
{
    switch (c.tag) {
        case PG_T_F64: return ((const double*)c.data)[i];
        case PG_T_I64: return (double)((const int64_t*)c.data)[i];
        case PG_T_I32: return (double)((const int32_t*)c.data)[i];
        default: return (double)((const uint8_t*)c.data)[i];
    }
}
__device__ inline int64_t d_load_i64(const pg_col& c, int64_t i)
{
    switch (c.tag) {
        case PG_T_I64: return ((const int64_t*)c.data)[i];
        case PG_T_I32: return (int64_t)((const int32_t*)c.data)[i];
        case PG_T_U8: return (int64_t)((const uint8_t*)c.data)[i];
        default: return (int64_t)((const double*)c.data)[i];
    }
}

/* substring search with a SWAR first-byte skip: one unaligned u32 load
 * covers four candidate offsets in the common no-match case (the
 * LikeFunctions.likeVarchar positional scan, vectorized).  Returns the
 * leftmost match offset >= from, or -1. */
__device__ inline int32_t d_find(const uint8_t* d, int32_t n,
                                 const char* pat, int32_t len,
                                 int32_t from)
{
    if (len <= 0) return from <= n ? from : -1;
    const uint8_t c0 = (uint8_t)pat[0];
    const uint32_t c4 = 0x01010101u * c0;
    int32_t last = n - len;
    int32_t s = from;
    for (; s + 3 <= last; ) {
        uint32_t w;
        memcpy(&w, d + s, 4);
        uint32_t x = w ^ c4;
        uint32_t t = (x - 0x01010101u) & ~x & 0x80808080u;
        if (!t) {
            s += 4;
            continue;
        }
        /* some byte equals c0: test the 4 offsets the window covers */
        for (int k = 0; k < 4; k++, s++) {
            if (((w >> (8 * k)) & 0xff) != c0) continue;
            bool e = true;
            for (int j = 1; j < len; j++)
                e = e && d[s + j] == (uint8_t)pat[j];
            if (e) return s;
        }
    }
    for (; s <= last; s++) {
        if (d[s] != c0) continue;
        bool e = true;
        for (int j = 1; j < len; j++)
            e = e && d[s + j] == (uint8_t)pat[j];
        if (e) return s;
    }
    return -1;
}

/* predicate conjunction — PageFilter semantics (PageProcessor.java:299-343:
 * null comparison result excludes the row; our round-1 columns are
 * non-null, null_mask honored as exclusion).  Every specialised kernel
 * that bypasses this function is gated on one exact comparison op
 * (Q1: LE, Q3 probe: GT/LT) or on n_preds == 0 (mode-2 Q5 probe), so the
 * null tests always land here.
 * NULL_TESTS = false compiles the null tests out: the single-scan build
 * kernels (dense_array fills, agg_table direct insert and partition
 * scatter — the build scan of the Q3 headline) keep exactly the code they
 * had, and HASH_BUILD rejects a null test on those builds at create. */
template <bool NULL_TESTS = true>
__device__ inline bool d_eval_preds(const pg_page& pg, const pg_pred* preds,
                                    int n_preds, int64_t i)
{
    for (int p = 0; p < n_preds; p++) {
        const pg_pred& pr = preds[p];
        const pg_col& c = pg.cols[pr.col];
        if constexpr (NULL_TESTS) {
            /* IS [NOT] NULL reads the mask alone (any column type, no mask
             * = never null) and is decided before the exclusion rule */
            if (pr.op >= PG_CMP_IS_NULL) {
                const bool is_null = c.null_mask && c.null_mask[i];
                if (is_null != (pr.op == PG_CMP_IS_NULL)) return false;
                continue;
            }
        }
        if (c.null_mask && c.null_mask[i]) return false;
        bool ok;
        if (c.tag == PG_T_VARBIN) {
            /* EQ/NE/CONTAINS/PREFIX against a constant
             * (VariableWidthBlock bytesEqual,
             * AbstractVariableWidthBlock.java:95-99; LikeFunctions.java
             * likeVarchar for wildcard-free %w% / w% patterns).
             * Dictionary blocks read through the ids. */
            int64_t e = c.dict_ids ? (int64_t)c.dict_ids[i] : i;
            int32_t b0 = c.offsets[e], b1 = c.offsets[e + 1];
            const uint8_t* d = (const uint8_t*)c.data + b0;
            int32_t n = b1 - b0;
            if (pr.op == PG_CMP_CONTAINS) {
                ok = d_find(d, n, pr.sval, pr.slen, 0) >= 0;
            } else if (pr.op == PG_CMP_PREFIX) {
                bool e = pr.slen <= n;
                for (int j = 0; e && j < pr.slen; j++)
                    e = d[j] == (uint8_t)pr.sval[j];
                ok = e;
            } else if (pr.op == PG_CMP_CONTAINS2 ||
                       pr.op == PG_CMP_NOT_CONTAINS2) {
                /* ordered '%a%b%': find a, then b after it (leftmost-a
                 * suffices: any later a leaves less room for b) */
                int32_t la = pr.slen, lb = (int32_t)pr.ival;
                int32_t a = d_find(d, n, pr.sval, la, 0);
                bool m = a >= 0 &&
                         d_find(d, n, pr.sval + la, lb, a + la) >= 0;
                ok = (pr.op == PG_CMP_CONTAINS2) ? m : !m;
            } else {
                bool eq = n == pr.slen;
                for (int j = 0; eq && j < pr.slen; j++)
                    eq = d[j] == (uint8_t)pr.sval[j];
                ok = pr.op == PG_CMP_EQ ? eq : !eq;
            }
        } else if (c.tag == PG_T_F64) {
            double v = ((const double*)c.data)[i];
            double x;
            if (pr.rhs_col > 0) {
                const pg_col& rc = pg.cols[pr.rhs_col - 1];
                if (rc.null_mask && rc.null_mask[i]) return false;
                x = d_load_f64(rc, i) + pr.dval;
            } else {
                x = pr.dval;
            }
            switch (pr.op) {
                case PG_CMP_LT: ok = v < x; break;
                case PG_CMP_LE: ok = v <= x; break;
                case PG_CMP_GT: ok = v > x; break;
                case PG_CMP_GE: ok = v >= x; break;
                case PG_CMP_EQ: ok = v == x; break;
                default: ok = v != x; break;
            }
        } else {
            int64_t v = d_load_i64(c, i);
            int64_t x;
            if (pr.rhs_col > 0) {
                const pg_col& rc = pg.cols[pr.rhs_col - 1];
                if (rc.null_mask && rc.null_mask[i]) return false;
                x = d_load_i64(rc, i) + pr.ival; /* col OP col + const */
            } else {
                x = pr.ival;
            }
            switch (pr.op) {
                case PG_CMP_LT: ok = v < x; break;
                case PG_CMP_LE: ok = v <= x; break;
                case PG_CMP_GT: ok = v > x; break;
                case PG_CMP_GE: ok = v >= x; break;
                case PG_CMP_EQ: ok = v == x; break;
                default: ok = v != x; break;
            }
        }
        if (!ok) return false;
    }
    return true;
}

__device__ inline double d_eval_proj_f64(const pg_page& pg, const pg_proj& p,
                                         int64_t i)
{
    double a = d_load_f64(pg.cols[p.a], i);
    if (p.kind == PG_PROJ_IDENT) return a;
    double b = d_load_f64(pg.cols[p.b], i);
    if (p.kind == PG_PROJ_MUL) return a * b;
    if (p.kind == PG_PROJ_DIV) return a / b;
    double v = a * (1.0 - b);
    if (p.kind == PG_PROJ_DISC_PRICE) return v;
    double c = d_load_f64(pg.cols[p.c], i);
    return v * (1.0 + c);
}

/* scaled value -> integer ticks, rounding half away from zero (the
 * header's ticks = round(value * 10^dec_scale)).  Non-negative x takes
 * the (i64)(x + 0.5) of the oracle unchanged; a plain +0.5 would truncate
 * negative values toward zero (-1.23 -> -122). */
__device__ inline int64_t d_round_ticks(double x)
{
    return (int64_t)(x + (x < 0 ? -0.5 : 0.5));
}

/* checked entry to the 64.64 accumulators: fx128_from_f64 is exact only for
 * 0 <= p < 2^53 whose fraction fits 64 bits (fixed128.h).  Anything else
 * (negative, NaN, >= 2^53, fraction bits below 2^-64) contributes nothing
 * and bumps *bad, which the host raises as a SUM_F64 domain error. */
__device__ inline void d_fx128_from_f64_ck(double p, uint64_t* hi,
                                           uint64_t* lo,
                                           unsigned long long* bad)
{
    bool ok = p >= 0.0 && p < 9007199254740992.0; /* false for NaN */
    if (ok) {
        fx128_from_f64(p, hi, lo);
        double frac = p - (double)*hi;
        ok = (double)*lo == frac * 18446744073709551616.0;
    }
    if (!ok) {
        *hi = 0;
        *lo = 0;
        atomicAdd(bad, 1ull);
    }
}

/* exact decimal ticks; operand-wise decomposition identical to the oracle
 * (oracle.c) on its non-negative domain: cents = (i64)(x*100+0.5) etc. */
__device__ inline int64_t d_eval_proj_dec(const pg_page& pg, const pg_agg& ag,
                                          int64_t i)
{
    const pg_proj& p = ag.proj;
    if (p.kind == PG_PROJ_IDENT) {
        const pg_col& c = pg.cols[p.a];
        if (c.tag != PG_T_F64 && ag.dec_scale == 0)
            return d_load_i64(c, i); /* integer column: exact, no f64 trip
                                        (LongSumAggregation semantics) */
        double a = d_load_f64(c, i);
        double s = 1.0;
        for (int k = 0; k < ag.dec_scale; k++) s *= 10.0;
        return d_round_ticks(a * s);
    }
    if (p.kind == PG_PROJ_SUBDIV)
        return (d_load_i64(pg.cols[p.a], i) - (int64_t)p.b) /
               (p.c ? (int64_t)p.c : 1);
    if (p.kind == PG_PROJ_MUL && ag.dec_scale == 0 &&
        pg.cols[p.a].tag != PG_T_F64 && pg.cols[p.b].tag != PG_T_F64)
        /* raw integer product (e.g. Q21's exact sum of squared
         * suppkeys) — scale-4 money products keep the cents path */
        return d_load_i64(pg.cols[p.a], i) * d_load_i64(pg.cols[p.b], i);
    int64_t cents = d_round_ticks(d_load_f64(pg.cols[p.a], i) * 100.0);
    int64_t d = d_round_ticks(d_load_f64(pg.cols[p.b], i) * 100.0);
    if (p.kind == PG_PROJ_MUL) return cents * d; /* scale 4 ticks */
    int64_t v = cents * (100 - d);
    if (p.kind == PG_PROJ_DISC_PRICE) return v;
    int64_t t = d_round_ticks(d_load_f64(pg.cols[p.c], i) * 100.0);
    return v * (100 + t);
}

/* SQL nullness of a projection's input at row i: null when any COLUMN the
 * kind reads is null there.  The one place that knows which of a, b, c are
 * channels: IDENT, SHR and SUBDIV read a (their b, c are constants);
 * DISC_PRICE, MUL, DIV, KEYSHL and KEYSHL_DIV read a and b; CHARGE reads
 * all three. */
__device__ inline bool d_col_is_null(const pg_page& pg, int32_t col,
                                     int64_t i)
{
    const uint8_t* m = pg.cols[col].null_mask;
    return m && m[i];
}
__device__ inline bool d_proj_is_null(const pg_page& pg, const pg_proj& p,
                                      int64_t i)
{
    bool n = d_col_is_null(pg, p.a, i);
    switch (p.kind) {
        case PG_PROJ_IDENT:
        case PG_PROJ_SHR:
        case PG_PROJ_SUBDIV:
            return n;
        case PG_PROJ_CHARGE:
            n = d_col_is_null(pg, p.c, i) || n;
            [[fallthrough]];
        default:
            return d_col_is_null(pg, p.b, i) || n;
    }
}

/* deterministic wave butterfly sum (order fixed: x_i += x_{i^s}) */
__device__ inline double d_bfly_f64(double v)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v = v + __shfl_xor(v, s, WAVE);
    return v;
}
__device__ inline int64_t d_bfly_i64(int64_t v)
{
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1) v = v + __shfl_xor(v, s, WAVE);
    return v;
}
/* the same butterfly for exact tick sums (Math.addExact semantics).  A lane
 * performs only six of the tree's 63 adds; the other partial sums form in
 * partner lanes and would arrive already wrapped, so every lane checks its
 * own adds and the wave votes: the result is true in all 64 lanes when any
 * add anywhere in the tree left int64.  All lanes of the wave must call. */
__device__ inline int64_t d_bfly_i64_ck(int64_t v, bool* wrapped)
{
    bool w = false;
#pragma unroll
    for (int s = 32; s >= 1; s >>= 1)
        w |= __builtin_add_overflow(v, __shfl_xor(v, s, WAVE), &v);
    *wrapped = __any(w);
    return v;
}

/* ------------------------------------------------------------------ */
/* HASH_AGG_SMALL: fused scan+filter+group-by+aggregate               */
/* (the Q1 pipeline: ScanFilterAndProjectOperator +                   */
/*  HashAggregationOperator.addInput:413 +                            */
/*  InMemoryHashAggregationBuilder.processPage:204)                   */
/* Deterministic schedule: fixed 4096x256    */
/* grid; thread v owns rows {2v,2v+1} + k*2*VL sequentially; wave     */
/* xor-butterfly; 4 wave sums butterfly(s=2,1); block partial += tree */
/* result per page; finish: 64-lane kernel, lane l sums blocks        */
/* l+64k ascending then butterfly.                                    */
/* ------------------------------------------------------------------ */
template <int NA, int MAXG, bool DEC>
__global__ __launch_bounds__(FT_NTHREADS) void k_agg_small(
    pg_page pg, pg_plan_hash_agg_small plan, double* partials /* f64 mode */,
    int64_t* partials_i /* dec mode */, unsigned long long* bad_keys)
{
    using T = typename std::conditional<DEC, int64_t, double>::type;
    T acc[NA][MAXG];
#pragma unroll
    for (int a = 0; a < NA; a++) {
        T id = (T)0;
        if (a < plan.n_aggs) {
            if (plan.aggs[a].func == PG_AGG_MIN)
                id = DEC ? (T)INT64_MAX : (T)INFINITY;
            else if (plan.aggs[a].func == PG_AGG_MAX)
                id = DEC ? (T)INT64_MIN : (T)-INFINITY;
        }
#pragma unroll
        for (int g = 0; g < MAXG; g++) acc[a][g] = id;
    }

    const int64_t n = pg.n_rows;
    const int64_t v = (int64_t)blockIdx.x * FT_NTHREADS + threadIdx.x;
    unsigned long long local_bad = 0, local_ovf = 0;

    for (int64_t base = 2 * v; base < n; base += 2 * FT_VL) {
        int64_t lim = base + 2 < n ? base + 2 : n;
        for (int64_t i = base; i < lim; i++) {
            if (!d_eval_preds(pg, plan.preds, plan.n_preds, i)) continue;
            /* group id: enumerated u8 key values (n_keys==0: one group) */
            int idx0 = -1, idx1 = 0, n1 = 1;
            uint8_t k0 = plan.n_keys
                             ? ((const uint8_t*)
                                    pg.cols[plan.key_col[0]].data)[i]
                             : 0;
            if (plan.n_keys == 0) idx0 = 0;
#pragma unroll
            for (int j = 0; j < PG_MAX_KEYVALS; j++)
                if (j < plan.n_vals[0] && k0 == plan.key_vals[0][j] &&
                    idx0 < 0)
                    idx0 = j;
            if (plan.n_keys == 2) {
                n1 = plan.n_vals[1];
                uint8_t k1 =
                    ((const uint8_t*)pg.cols[plan.key_col[1]].data)[i];
                idx1 = -1;
#pragma unroll
                for (int j = 0; j < PG_MAX_KEYVALS; j++)
                    if (j < plan.n_vals[1] && k1 == plan.key_vals[1][j] &&
                        idx1 < 0)
                        idx1 = j;
            }
            if (idx0 < 0 || idx1 < 0) {
                if (!plan.drop_unlisted_keys) local_bad++;
                continue;
            }
            int g = idx0 * n1 + idx1;
#pragma unroll
            for (int a = 0; a < NA; a++) {
                if (a >= plan.n_aggs) continue;
                T val;
                if (DEC) {
                    int64_t t;
                    if (plan.aggs[a].func == PG_AGG_COUNT)
                        t = 1;
                    else
                        t = d_eval_proj_dec(pg, plan.aggs[a], i);
                    val = (T)t;
                } else {
                    double t;
                    if (plan.aggs[a].func == PG_AGG_COUNT)
                        t = 1.0; /* exact as f64 below 2^53 */
                    else
                        t = d_eval_proj_f64(pg, plan.aggs[a].proj, i);
                    val = (T)t;
                }
                int32_t fn = plan.aggs[a].func;
#pragma unroll
                for (int gg = 0; gg < MAXG; gg++) {
                    bool m = gg == g;
                    if (fn == PG_AGG_MIN)
                        acc[a][gg] =
                            m && val < acc[a][gg] ? val : acc[a][gg];
                    else if (fn == PG_AGG_MAX)
                        acc[a][gg] =
                            m && val > acc[a][gg] ? val : acc[a][gg];
                    else if constexpr (DEC) {
                        /* overflow-checked add: LongSumAggregation.java:33-37
                         * raises via Math.addExact — wraps are surfaced as
                         * an operator error, never silent */
                        int64_t cur = (int64_t)acc[a][gg], nv;
                        if (__builtin_add_overflow(
                                cur, (int64_t)(m ? val : (T)0), &nv))
                            local_ovf++;
                        acc[a][gg] = (T)nv;
                    } else {
                        acc[a][gg] += m ? val : (T)0;
                    }
                }
            }
        }
    }

    /* wave butterfly, then 4-wave combine in LDS, then block partial
     * merge (sum, or min/max per the aggregate) */
    __shared__ T lds[4][NA][MAXG];
    const int lane = threadIdx.x & (WAVE - 1);
    const int wid = threadIdx.x >> 6;
#pragma unroll
    for (int a = 0; a < NA; a++) {
        int32_t fn = a < plan.n_aggs ? plan.aggs[a].func : PG_AGG_COUNT;
#pragma unroll
        for (int g = 0; g < MAXG; g++) {
            T s = acc[a][g];
#pragma unroll
            for (int w = 32; w >= 1; w >>= 1) {
                T o;
                if (DEC)
                    o = (T)__shfl_xor((int64_t)s, w, WAVE);
                else
                    o = (T)__shfl_xor((double)s, w, WAVE);
                if (fn == PG_AGG_MIN)
                    s = o < s ? o : s;
                else if (fn == PG_AGG_MAX)
                    s = o > s ? o : s;
                else if constexpr (DEC) {
                    int64_t nv;
                    if (__builtin_add_overflow((int64_t)s, (int64_t)o, &nv))
                        local_ovf++;
                    s = (T)nv;
                } else {
                    s = s + o;
                }
            }
            if (lane == 0) lds[wid][a][g] = s;
        }
    }
    __syncthreads();
    if (wid == 0 && lane < 4) {
#pragma unroll
        for (int a = 0; a < NA; a++) {
            int32_t fn = a < plan.n_aggs ? plan.aggs[a].func : PG_AGG_COUNT;
#pragma unroll
            for (int g = 0; g < MAXG; g++) {
                T x = lds[lane][a][g];
#pragma unroll
                for (int w = 2; w >= 1; w >>= 1) {
                    T o;
                    if (DEC)
                        o = (T)__shfl_xor((int64_t)x, w, WAVE);
                    else
                        o = (T)__shfl_xor((double)x, w, WAVE);
                    if (fn == PG_AGG_MIN)
                        x = o < x ? o : x;
                    else if (fn == PG_AGG_MAX)
                        x = o > x ? o : x;
                    else if constexpr (DEC) {
                        int64_t nv;
                        if (__builtin_add_overflow((int64_t)x, (int64_t)o,
                                                   &nv))
                            local_ovf++;
                        x = (T)nv;
                    } else {
                        x = x + o;
                    }
                }
                if (lane == 0) {
                    size_t off =
                        ((size_t)blockIdx.x * NA + a) * MAXG + g;
                    if (DEC) {
                        int64_t* d = &partials_i[off];
                        if (fn == PG_AGG_MIN)
                            *d = (int64_t)x < *d ? (int64_t)x : *d;
                        else if (fn == PG_AGG_MAX)
                            *d = (int64_t)x > *d ? (int64_t)x : *d;
                        else if (__builtin_add_overflow(*d, (int64_t)x, d))
                            local_ovf++;
                    } else {
                        double* d = &partials[off];
                        if (fn == PG_AGG_MIN)
                            *d = (double)x < *d ? (double)x : *d;
                        else if (fn == PG_AGG_MAX)
                            *d = (double)x > *d ? (double)x : *d;
                        else
                            *d += (double)x;
                    }
                }
            }
        }
    }
    if (local_bad) atomicAdd(bad_keys, local_bad);
    if (local_ovf) atomicAdd(bad_keys + 1, local_ovf);
}


/* Specialized fused Q1 kernel — the AOT analog of the reference's
 * per-query codegen (PageFunctionCompiler/AccumulatorCompiler specialize
 * the scan+filter+aggregate loop per expression; this kernel is that
 * specialization for the Q1 shape: one int32 <= filter, two enumerated u8
 * keys (3x2), aggregates [sum(a), sum(e), sum(e*(1-d)), sum(e*(1-d)*(1+t)),
 * sum(d), count]).  Same deterministic schedule and partials layout as the
 * generic k_agg_small<7,6,DEC>, so the finish kernel and host code are
 * shared.  Each column is loaded ONCE per row pair with 16-byte vector
 * loads; predicate and group selection are branchless. */
template <bool DEC, int VAR = 0>
__global__ __launch_bounds__(FT_NTHREADS) void k_agg_q1(
    const double* qty, const double* ep, const double* dc, const double* tx,
    const int32_t* sd, const uint8_t* rf, const uint8_t* ls, int64_t n,
    int32_t ship_max, uint8_t k00, uint8_t k01, uint8_t k02, uint8_t k10,
    uint8_t k11, double* partials, int64_t* partials_i,
    unsigned long long* bad_keys)
{
    using T = typename std::conditional<DEC, int64_t, double>::type;
    T acc[5][6];
    int32_t cnt[6];
#pragma unroll
    for (int a = 0; a < 5; a++)
#pragma unroll
        for (int g = 0; g < 6; g++) acc[a][g] = (T)0;
#pragma unroll
    for (int g = 0; g < 6; g++) cnt[g] = 0;

    const int64_t v = (int64_t)blockIdx.x * FT_NTHREADS + threadIdx.x;
    unsigned long long local_bad = 0;

    for (int64_t base = 2 * v; base < n; base += 2 * FT_VL) {
        const bool pair = base + 1 < n;
        /* one vector load per column per pair */
        double2 q2, e2, d2, t2;
        int2 s2;
        uint8_t r0, r1, l0, l1;
        if (pair) {
            if (VAR >= 1) {
                /* nontemporal: streamed once, no L2 retention needed */
                typedef double vd2 __attribute__((ext_vector_type(2)));
                typedef int vi2 __attribute__((ext_vector_type(2)));
                vd2 q_ = __builtin_nontemporal_load((const vd2*)(qty + base));
                vd2 e_ = __builtin_nontemporal_load((const vd2*)(ep + base));
                vd2 d_ = __builtin_nontemporal_load((const vd2*)(dc + base));
                vd2 t_ = __builtin_nontemporal_load((const vd2*)(tx + base));
                vi2 s_ = __builtin_nontemporal_load((const vi2*)(sd + base));
                q2.x = q_[0]; q2.y = q_[1];
                e2.x = e_[0]; e2.y = e_[1];
                d2.x = d_[0]; d2.y = d_[1];
                t2.x = t_[0]; t2.y = t_[1];
                s2.x = s_[0]; s2.y = s_[1];
                uint16_t rw = __builtin_nontemporal_load(
                    (const uint16_t*)(rf + base));
                uint16_t lw = __builtin_nontemporal_load(
                    (const uint16_t*)(ls + base));
                r0 = (uint8_t)rw; r1 = (uint8_t)(rw >> 8);
                l0 = (uint8_t)lw; l1 = (uint8_t)(lw >> 8);
            } else {
            q2 = *(const double2*)(qty + base);
            e2 = *(const double2*)(ep + base);
            d2 = *(const double2*)(dc + base);
            t2 = *(const double2*)(tx + base);
            s2 = *(const int2*)(sd + base);
            uchar2 rr = *(const uchar2*)(rf + base);
            uchar2 ll = *(const uchar2*)(ls + base);
            r0 = rr.x; r1 = rr.y; l0 = ll.x; l1 = ll.y;
            }
        } else {
            q2.x = qty[base]; e2.x = ep[base]; d2.x = dc[base];
            t2.x = tx[base]; s2.x = sd[base];
            r0 = rf[base]; l0 = ls[base];
            /* no second row: sel is false for it below (!pair), whatever
             * the predicate constant; the zeros only keep the registers
             * defined */
            q2.y = 0; e2.y = 0; d2.y = 0; t2.y = 0; s2.y = 0;
            r1 = 0; l1 = 0;
        }
#pragma unroll
        for (int r = 0; r < 2; r++) {
            double q = r ? q2.y : q2.x, e = r ? e2.y : e2.x;
            double d = r ? d2.y : d2.x, t = r ? t2.y : t2.x;
            int32_t sdv = r ? s2.y : s2.x;
            uint8_t rv = r ? r1 : r0, lv = r ? l1 : l0;
            bool sel = sdv <= ship_max && (r == 0 || pair);
            int i0 = rv == k00 ? 0 : (rv == k01 ? 1 : (rv == k02 ? 2 : -1));
            int i1 = lv == k10 ? 0 : (lv == k11 ? 1 : -1);
            if (i0 < 0 || i1 < 0) {
                local_bad += sel ? 1 : 0;
                continue;
            }
            int g = i0 * 2 + i1;
            T vq, ve, vdp, vch, vd;
            if (DEC) {
                int64_t qq = (int64_t)(q + 0.5);
                int64_t cents = (int64_t)(e * 100.0 + 0.5);
                int64_t dd = (int64_t)(d * 100.0 + 0.5);
                int64_t tt = (int64_t)(t * 100.0 + 0.5);
                int64_t dp = cents * (100 - dd);
                vq = (T)qq; ve = (T)cents; vdp = (T)dp;
                vch = (T)(dp * (100 + tt)); vd = (T)dd;
            } else {
                double dp = e * (1.0 - d);
                vq = (T)q; ve = (T)e; vdp = (T)dp;
                vch = (T)(dp * (1.0 + t)); vd = (T)d;
            }
#pragma unroll
            for (int gg = 0; gg < 6; gg++) {
                bool m = sel && gg == g;
                acc[0][gg] += m ? vq : (T)0;
                acc[1][gg] += m ? ve : (T)0;
                acc[2][gg] += m ? vdp : (T)0;
                acc[3][gg] += m ? vch : (T)0;
                acc[4][gg] += m ? vd : (T)0;
                cnt[gg] += m ? 1 : 0;
            }
        }
    }

    /* identical reduction to k_agg_small (NA=7, MAXG=6 layout: rows 5 and
     * 6 both carry the count — user count agg + internal presence) */
    __shared__ T lds[4][7][6];
    const int lane = threadIdx.x & (WAVE - 1);
    const int wid = threadIdx.x >> 6;
#pragma unroll
    for (int a = 0; a < 7; a++)
#pragma unroll
        for (int g = 0; g < 6; g++) {
            T x = a < 5 ? acc[a][g] : (T)cnt[g];
            T s;
            if (DEC)
                s = (T)d_bfly_i64((int64_t)x);
            else
                s = (T)d_bfly_f64((double)x);
            if (lane == 0) lds[wid][a][g] = s;
        }
    __syncthreads();
    if (wid == 0 && lane < 4) {
#pragma unroll
        for (int a = 0; a < 7; a++)
#pragma unroll
            for (int g = 0; g < 6; g++) {
                T x = lds[lane][a][g];
                if (DEC) {
                    int64_t y = (int64_t)x;
                    y += __shfl_xor(y, 2, WAVE);
                    y += __shfl_xor(y, 1, WAVE);
                    x = (T)y;
                } else {
                    double y = (double)x;
                    y += __shfl_xor(y, 2, WAVE);
                    y += __shfl_xor(y, 1, WAVE);
                    x = (T)y;
                }
                if (lane == 0) {
                    size_t off = ((size_t)blockIdx.x * 7 + a) * 6 + g;
                    if (DEC)
                        partials_i[off] += (int64_t)x;
                    else
                        partials[off] += (double)x;
                }
            }
    }
    if (local_bad) atomicAdd(bad_keys, local_bad);
}

struct agg_funcs {
    int32_t f[12];
    int32_t maxg;
};

/* initialize block partials to each aggregate's identity (0 for sums and
 * counts; +/-extremes for MIN/MAX) */
template <bool DEC>
__global__ __launch_bounds__(256) void k_agg_partials_init(
    double* partials, int64_t* partials_i, agg_funcs fns, int64_t n_total,
    int na)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n_total; i += stride) {
        int a = (int)((i / fns.maxg) % na);
        int32_t fn = fns.f[a];
        if (DEC) {
            int64_t id = fn == PG_AGG_MIN
                             ? INT64_MAX
                             : (fn == PG_AGG_MAX ? INT64_MIN : 0);
            partials_i[i] = id;
        } else {
            double id = fn == PG_AGG_MIN
                            ? INFINITY
                            : (fn == PG_AGG_MAX ? -INFINITY : 0.0);
            partials[i] = id;
        }
    }
}

/* finish: 64-lane deterministic reduce of block partials.
 * DEC: output int128 (hi,lo) pairs (plain i64 for MIN/MAX); F64: doubles. */
template <bool DEC>
__global__ __launch_bounds__(WAVE) void k_agg_small_finish(
    const double* partials, const int64_t* partials_i, int na_x_maxg,
    double* out_f, int64_t* out_hi, uint64_t* out_lo, agg_funcs fns)
{
    int lane = threadIdx.x;
    {
        int j = blockIdx.x; /* one block (one wave) per output field; the
                               per-field reduction tree is unchanged */
        int32_t fn = fns.f[j / fns.maxg];
        if (DEC && (fn == PG_AGG_MIN || fn == PG_AGG_MAX)) {
            int64_t v = fn == PG_AGG_MIN ? INT64_MAX : INT64_MIN;
            for (int k = 0; k < FT_NBLOCKS / WAVE; k++) {
                int64_t x = partials_i[(size_t)(lane + k * WAVE) *
                                           na_x_maxg + j];
                v = fn == PG_AGG_MIN ? (x < v ? x : v) : (x > v ? x : v);
            }
#pragma unroll
            for (int w = 32; w >= 1; w >>= 1) {
                int64_t o = __shfl_xor(v, w, WAVE);
                v = fn == PG_AGG_MIN ? (o < v ? o : v) : (o > v ? o : v);
            }
            if (lane == 0) {
                out_hi[j] = v < 0 ? -1 : 0;
                out_lo[j] = (uint64_t)v;
            }
        } else if (DEC) {
            /* lane l: sequential over blocks l, l+64, ... (i64 safe:
             * 64 block partials each bounded by per-block row counts) */
            int64_t hi = 0;
            uint64_t lo = 0;
            for (int k = 0; k < FT_NBLOCKS / WAVE; k++) {
                int64_t x = partials_i[(size_t)(lane + k * WAVE) *
                                           na_x_maxg + j];
                /* sign-extend into 128-bit accumulator */
                uint64_t xlo = (uint64_t)x;
                int64_t xhi = x < 0 ? -1 : 0;
                uint64_t nlo = lo + xlo;
                hi += xhi + (nlo < xlo ? 1 : 0);
                lo = nlo;
            }
#pragma unroll
            for (int s = 32; s >= 1; s >>= 1) {
                int64_t ohi = __shfl_xor(hi, s, WAVE);
                uint64_t olo =
                    (uint64_t)__shfl_xor((int64_t)lo, s, WAVE);
                uint64_t nlo = lo + olo;
                hi += ohi + (nlo < olo ? 1 : 0);
                lo = nlo;
            }
            if (lane == 0) {
                out_hi[j] = hi;
                out_lo[j] = lo;
            }
        } else {
            double v = fn == PG_AGG_MIN
                           ? INFINITY
                           : (fn == PG_AGG_MAX ? -INFINITY : 0.0);
            for (int k = 0; k < FT_NBLOCKS / WAVE; k++) {
                double x =
                    partials[(size_t)(lane + k * WAVE) * na_x_maxg + j];
                if (fn == PG_AGG_MIN)
                    v = x < v ? x : v;
                else if (fn == PG_AGG_MAX)
                    v = x > v ? x : v;
                else
                    v += x;
            }
#pragma unroll
            for (int w = 32; w >= 1; w >>= 1) {
                double o = __shfl_xor(v, w, WAVE);
                if (fn == PG_AGG_MIN)
                    v = o < v ? o : v;
                else if (fn == PG_AGG_MAX)
                    v = o > v ? o : v;
                else
                    v += o;
            }
            if (lane == 0) out_f[j] = v;
        }
    }
}

/* ------------------------------------------------------------------ */
/* selection + stable compaction (PageProcessor/SelectedPositions)    */
/* Geometry: NB blocks x 256 threads; block b owns the contiguous     */
/* row chunk [b*chunk, (b+1)*chunk); within a 256-row window, wave w  */
/* covers rows [base+64w, base+64w+64) — wave64 ballot + popcount     */
/* gives a stable (row-ascending) output position.                    */
/* ------------------------------------------------------------------ */
#define FLT_NB 1024

__device__ inline uint64_t d_ballot(bool p)
{
    return __ballot(p);
}

/* key-set membership test (dense flags when set_mask < 0, else hash set);
 * anti inverts it (NOT-EXISTS pushdown) */
__device__ inline bool d_semi_ok(const pg_page& pg, int32_t set_col,
                                 int64_t i, const int64_t* set_keys,
                                 int64_t set_mask, int32_t anti)
{
    int64_t key = d_load_i64(pg.cols[set_col], i);
    bool in;
    if (set_mask < 0) { /* dense flags: |mask| = capacity */
        in = key >= 1 && key <= -set_mask &&
             ((const uint8_t*)set_keys)[key - 1];
    } else {
        in = false;
        uint64_t h = pg_murmur3_finalize(pg_bigint_hash(key));
        int64_t s = (int64_t)(h & (uint64_t)set_mask);
        for (;;) {
            int64_t k = set_keys[s];
            if (k == key) { in = true; break; }
            if (k == TBL_EMPTY) break;
            s = (s + 1) & set_mask;
        }
    }
    return in != (bool)anti;
}

__global__ __launch_bounds__(256) void k_sel_count(pg_page pg,
                                                   pg_plan_filter_project plan,
                                                   int64_t chunk,
                                                   int64_t* block_counts,
                                                   const int64_t* set_keys,
                                                   int64_t set_mask,
                                                   int32_t set_col,
                                                   unsigned long long*
                                                       selbits)
{
    /* the per-window ballot masks are saved so the emit pass never
     * re-evaluates the predicates — for expensive VARBIN scans (q13's
     * NOT LIKE) that halves the whole filter cost; the mask array is
     * n/8 bytes.  Chunks are 256-aligned, so each wave owns one
     * 64-aligned mask word. */
    const int64_t n = pg.n_rows;
    const int64_t lo = (int64_t)blockIdx.x * chunk;
    const int64_t hi = min(lo + chunk, n);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int64_t cnt = 0;
    for (int64_t base = lo + 64 * wid; base < hi; base += 256) {
        int64_t i = base + lane;
        bool sel = i < hi && d_eval_preds(pg, plan.preds, plan.n_preds, i);
        if (sel && set_keys)
            sel = d_semi_ok(pg, set_col, i, set_keys, set_mask,
                            plan.semijoin_anti);
        uint64_t m = d_ballot(sel);
        if (lane == 0) {
            cnt += __popcll(m);
            if (selbits) selbits[base >> 6] = m;
        }
    }
    __shared__ int64_t lds[4];
    if (lane == 0) lds[wid] = cnt;
    __syncthreads();
    if (threadIdx.x == 0)
        block_counts[blockIdx.x] = lds[0] + lds[1] + lds[2] + lds[3];
}

#define PG_PROJ_ROWID 100 /* internal: emit the source row index (used by
                             the VARBIN two-pass emit) */

/* emit one output column value for a selected row */
__device__ inline void d_emit_val(const pg_page& pg, const pg_proj& p,
                                  int64_t i, void* out, int out_tag,
                                  int64_t pos)
{
    if (p.kind == PG_PROJ_ROWID) {
        ((int64_t*)out)[pos] = i;
        return;
    }
    if (p.kind == PG_PROJ_KEYSHL) {
        int64_t va = d_load_i64(pg.cols[p.a], i);
        int64_t vb = d_load_i64(pg.cols[p.b], i);
        ((int64_t*)out)[pos] = (va << p.c) | vb;
        return;
    }
    if (p.kind == PG_PROJ_SHR) {
        ((int64_t*)out)[pos] = d_load_i64(pg.cols[p.a], i) >> p.c;
        return;
    }
    if (p.kind == PG_PROJ_SUBDIV) {
        ((int64_t*)out)[pos] =
            (d_load_i64(pg.cols[p.a], i) - (int64_t)p.b) /
            (p.c ? (int64_t)p.c : 1);
        return;
    }
    if (p.kind == PG_PROJ_KEYSHL_DIV) {
        int32_t shift = p.c >> 16, dv = p.c & 0xffff;
        ((int64_t*)out)[pos] =
            (d_load_i64(pg.cols[p.a], i) << shift) |
            (d_load_i64(pg.cols[p.b], i) / (dv ? dv : 1));
        return;
    }
    if (p.kind == PG_PROJ_IDENT) {
        const pg_col& c = pg.cols[p.a];
        switch (c.tag) {
            case PG_T_U8:
                ((uint8_t*)out)[pos] = ((const uint8_t*)c.data)[i];
                return;
            case PG_T_I32:
                ((int32_t*)out)[pos] = ((const int32_t*)c.data)[i];
                return;
            case PG_T_I64:
                ((int64_t*)out)[pos] = ((const int64_t*)c.data)[i];
                return;
            case PG_T_I128: {
                const int64_t* s = (const int64_t*)c.data + 2 * i;
                int64_t* d = (int64_t*)out + 2 * pos;
                d[0] = s[0];
                d[1] = s[1];
                return;
            }
            default:
                ((double*)out)[pos] = ((const double*)c.data)[i];
                return;
        }
    }
    ((double*)out)[pos] = d_eval_proj_f64(pg, p, i);
    (void)out_tag;
}

#define MAX_OUT 16
struct emit_outs {
    void* ptr[MAX_OUT];
    int32_t tag[MAX_OUT];
    int32_t n;
};

__global__ __launch_bounds__(256) void k_sel_emit(pg_page pg,
                                                  pg_plan_filter_project plan,
                                                  int64_t chunk,
                                                  const int64_t* block_offs,
                                                  emit_outs outs,
                                                  const int64_t* set_keys,
                                                  int64_t set_mask,
                                                  int32_t set_col,
                                                  const unsigned long long*
                                                      selbits)
{
    const int64_t n = pg.n_rows;
    const int64_t lo = (int64_t)blockIdx.x * chunk;
    const int64_t hi = min(lo + chunk, n);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    __shared__ int64_t wcnt[4];
    __shared__ int64_t running;
    if (threadIdx.x == 0) running = block_offs[blockIdx.x];
    __syncthreads();
    for (int64_t base = lo; base < hi; base += 256) {
        int64_t i = base + 64 * wid + lane;
        uint64_t m;
        bool sel;
        if (selbits) { /* verdicts cached by the count pass */
            m = selbits[(base + 64 * wid) >> 6];
            sel = i < hi && ((m >> lane) & 1);
        } else {
            sel = i < hi &&
                  d_eval_preds(pg, plan.preds, plan.n_preds, i);
            if (sel && set_keys)
                sel = d_semi_ok(pg, set_col, i, set_keys, set_mask,
                                plan.semijoin_anti);
            m = d_ballot(sel);
        }
        int wsum = __popcll(m);
        if (lane == 0) wcnt[wid] = wsum;
        __syncthreads();
        int64_t woff = running;
        for (int w = 0; w < wid; w++) woff += wcnt[w];
        if (sel) {
            int64_t pos =
                woff + __popcll(m & ((lane == 63) ? ~0ull >> 1
                                                  : ((1ull << lane) - 1)));
            /* note: (1<<63)-1 overflow guard above keeps lane 63 correct */
            for (int o = 0; o < outs.n; o++)
                d_emit_val(pg, plan.proj[o], i, outs.ptr[o], outs.tag[o],
                           pos);
        }
        __syncthreads();
        if (threadIdx.x == 0)
            running += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        __syncthreads();
    }
}

/* VARBIN emit pass 2: gather lengths then bytes through the selected
 * source row indexes (two-pass VariableWidthBlockBuilder analog) */
__global__ __launch_bounds__(256) void k_varbin_len(const int64_t* rowid,
                                                    int64_t n,
                                                    const int32_t* src_offs,
                                                    const int32_t* dict_ids,
                                                    int32_t* out_len)
{
    int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; j < n; j += stride) {
        int64_t i = rowid[j];
        int64_t e = dict_ids ? (int64_t)dict_ids[i] : i;
        out_len[j] = src_offs[e + 1] - src_offs[e];
    }
}

__global__ __launch_bounds__(256) void k_varbin_gather(
    const int64_t* rowid, int64_t n, const uint8_t* src_bytes,
    const int32_t* src_offs, const int32_t* dict_ids,
    const int32_t* dst_offs, uint8_t* dst_bytes)
{
    /* one 64-lane wave per row: coalesced byte copies for short strings */
    int64_t w = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6;
    int lane = threadIdx.x & 63;
    int64_t stride = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (; w < n; w += stride) {
        int64_t i = rowid[w];
        int64_t e = dict_ids ? (int64_t)dict_ids[i] : i;
        int32_t s0 = src_offs[e], len = src_offs[e + 1] - s0;
        int32_t d0 = dst_offs[w];
        for (int32_t b = lane; b < len; b += 64)
            dst_bytes[d0 + b] = src_bytes[s0 + b];
    }
}

/* ------------------------------------------------------------------ */
/* hash set / join-group table                                        */
/* build: PagesHash.java:81-125 (open-address, bucket =               */
/* murmur3_finalize(bigint_hash(key)), linear probe) with duplicate   */
/* chains per ArrayPositionLinks.java:25-30 (head-insert; parallel    */
/* insert order is non-deterministic across duplicates — result SET   */
/* semantics).                                         */
/* ------------------------------------------------------------------ */
/* dense-array build: payload[key-1] = u8 value (or membership flag 1 for
 * key sets); rows failing the plan predicates are skipped */
__global__ __launch_bounds__(256) void k_dense_fill(
    pg_page pg, pg_plan_hash_build plan, const uint8_t* vals, uint8_t* out,
    int64_t cap)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < pg.n_rows; i += stride) {
        if (!d_eval_preds<false>(pg, plan.preds, plan.n_preds, i)) continue;
        int64_t k = d_load_i64(pg.cols[plan.key_col], i);
        if (k >= 1 && k <= cap)
            out[k - 1] =
                vals ? (uint8_t)(vals[i] + plan.dense_payload_bias) : 1;
    }
}

/* dense fill with the payload fetched THROUGH a dense u8 dimension
 * (q7's orderkey -> customer nation: out[ok-1] = cust_nat[ck-1]+bias) */
__global__ __launch_bounds__(256) void k_dense_fill_lu(
    pg_page pg, pg_plan_hash_build plan, const uint8_t* lu, int64_t lu_cap,
    uint8_t* out, int64_t cap)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < pg.n_rows; i += stride) {
        if (!d_eval_preds<false>(pg, plan.preds, plan.n_preds, i)) continue;
        int64_t k = d_load_i64(pg.cols[plan.key_col], i);
        int64_t k2 = d_load_i64(pg.cols[plan.payload_lookup_key_col], i);
        if (k >= 1 && k <= cap && k2 >= 1 && k2 <= lu_cap)
            out[k - 1] =
                (uint8_t)(lu[k2 - 1] + plan.dense_payload_bias);
    }
}

__global__ __launch_bounds__(256) void k_dense_fill32(
    pg_page pg, pg_plan_hash_build plan, const int32_t* vals, int32_t* out,
    int64_t cap)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < pg.n_rows; i += stride) {
        if (!d_eval_preds<false>(pg, plan.preds, plan.n_preds, i)) continue;
        int64_t k = d_load_i64(pg.cols[plan.key_col], i);
        if (k >= 1 && k <= cap)
            out[k - 1] = vals[i] + plan.dense_payload_bias;
    }
}

__global__ __launch_bounds__(256) void k_tbl_init(int64_t* keys, int32_t* head,
                                                  int64_t cap)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < cap; i += stride) {
        keys[i] = TBL_EMPTY;
        if (head) head[i] = -1;
    }
}

__global__ __launch_bounds__(256) void k_set_insert(const int64_t* in_keys,
                                                    int64_t n, int64_t* keys,
                                                    int64_t mask)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        int64_t key = in_keys[i];
        uint64_t h = pg_murmur3_finalize(pg_bigint_hash(key));
        int64_t s = (int64_t)(h & (uint64_t)mask);
        for (;;) {
            int64_t old = atomicCAS((unsigned long long*)&keys[s],
                                    (unsigned long long)TBL_EMPTY,
                                    (unsigned long long)key);
            if (old == TBL_EMPTY || old == key) break;
            s = (s + 1) & mask;
        }
    }
}

/* insert build rows (already filtered/compacted) with chains */
/* key-presence bitmap over [1, bmax] (pg_plan_hash_build.bitmap_max_key):
 * the bigint dynamic-filter analog.  Tested BEFORE the bucket hash on
 * probes; a clear bit is a definitive miss. */
__device__ inline void d_kbit_set(unsigned long long* kb, int64_t key)
{
    atomicOr(&kb[(uint64_t)key >> 6], 1ull << (key & 63));
}
__device__ inline bool d_kbit_test(const unsigned long long* kb,
                                   int64_t bmax, int64_t key)
{
    if ((uint64_t)(key - 1) >= (uint64_t)bmax) return false;
    return (kb[(uint64_t)key >> 6] >> (key & 63)) & 1;
}

__global__ __launch_bounds__(256) void k_tbl_insert(const int64_t* in_keys,
                                                    int64_t n, int64_t* keys,
                                                    uint8_t* tags,
                                                    int32_t* head,
                                                    int32_t* next,
                                                    int64_t mask,
                                                    unsigned long long* kbits,
                                                    int64_t bmax,
                                                    unsigned long long* bm_err)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        int64_t key = in_keys[i];
        if (kbits) {
            if ((uint64_t)(key - 1) >= (uint64_t)bmax) {
                atomicAdd(bm_err, 1ull);
                continue;
            }
            d_kbit_set(kbits, key);
        }
        uint64_t h = pg_murmur3_finalize(pg_bigint_hash(key));
        int64_t s = (int64_t)(h & (uint64_t)mask);
        for (;;) {
            int64_t old = atomicCAS((unsigned long long*)&keys[s],
                                    (unsigned long long)TBL_EMPTY,
                                    (unsigned long long)key);
            if (old == TBL_EMPTY || old == key) {
                if (tags) tags[s] = d_tbl_tag(h); /* probes run post-sync */
                int32_t prev = atomicExch(&head[s], (int32_t)i);
                next[i] = prev;
                break;
            }
            s = (s + 1) & mask;
        }
    }
}

/* linear-probe step with partition-local wraparound: partitioned tables
 * (radix-partitioned agg builds) wrap within their cap_p-slot
 * region; unpartitioned tables pass lmask == mask (identical behavior) */
__device__ inline int64_t d_probe_next(int64_t s, int64_t lmask)
{
    return (s & ~lmask) | ((s + 1) & lmask);
}

__device__ inline int64_t d_tbl_find_tagged(const int64_t* keys,
                                            const uint8_t* tags,
                                            int64_t mask, int64_t lmask,
                                            int32_t pbits, int64_t key);

/* direct insert for agg tables: filter+semijoin+insert in ONE scan of the
 * build input; payloads stored per SLOT (keys unique).  count tracks
 * inserted rows; full table -> give-up flag (bounded probe loop). */
struct direct_payloads {
    void* ptr[4];
    int32_t tag[4];
    int32_t src[4];
    int32_t n;
};
__global__ __launch_bounds__(256) void k_tbl_insert_direct(
    pg_page pg, pg_plan_hash_build plan, const int64_t* set_keys,
    int64_t set_mask, const int64_t* lu_keys, const uint8_t* lu_tags,
    int64_t lu_mask, int64_t lu_lmask, const uint8_t* lu_payload,
    int64_t* keys, uint8_t* tags, direct_payloads dp, int64_t mask,
    unsigned long long* inserted, unsigned long long* overflow,
    unsigned long long* pack_err, unsigned long long* kbits, int64_t bmax,
    unsigned long long* bm_err)
{
    const int32_t pbits = plan.pack_bits;
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    int64_t my_inserted = 0, my_overflow = 0, my_packerr = 0;
    for (; i < pg.n_rows; i += stride) {
        if (!d_eval_preds<false>(pg, plan.preds, plan.n_preds, i)) continue;
        uint8_t plv = 0;
        if (lu_payload) {
            /* fused dimension join: fetch u8 payload through the lookup
             * table (hash or dense); rows that miss are dropped
             * (inner-join semantics) */
            int64_t k2 =
                d_load_i64(pg.cols[plan.payload_lookup_key_col], i);
            int64_t sl2;
            if (lu_keys) {
                sl2 = d_tbl_find_tagged(lu_keys, lu_tags, lu_mask,
                                        lu_lmask, 0, k2);
            } else { /* dense: payload[key-1], lu_mask = capacity */
                sl2 = (k2 >= 1 && k2 <= lu_mask) ? k2 - 1 : -1;
            }
            if (sl2 < 0) continue;
            plv = lu_payload[sl2];
        }
        if (set_keys) {
            int64_t sk = d_load_i64(pg.cols[plan.semijoin_col], i);
            bool found;
            if (set_mask < 0) { /* dense flags */
                found = sk >= 1 && sk <= -set_mask &&
                        ((const uint8_t*)set_keys)[sk - 1];
            } else {
                found = false;
                uint64_t h = pg_murmur3_finalize(pg_bigint_hash(sk));
                int64_t s = (int64_t)(h & (uint64_t)set_mask);
                for (;;) {
                    int64_t k = set_keys[s];
                    if (k == sk) { found = true; break; }
                    if (k == TBL_EMPTY) break;
                    s = (s + 1) & set_mask;
                }
            }
            if (!found) continue;
        }
        int64_t key = d_load_i64(pg.cols[plan.key_col], i);
        int64_t word = key;
        if (pbits) {
            /* packed slot: key<<pbits | payload0 (single payload) */
            int64_t pay0 = lu_payload
                               ? (int64_t)plv
                               : d_load_i64(pg.cols[dp.src[0]], i);
            if (key < 0 || key >= (1ll << (63 - pbits)) || pay0 < 0 ||
                pay0 >= (1ll << pbits)) {
                my_packerr++;
                continue;
            }
            word = (key << pbits) | pay0;
        }
        if (kbits) {
            if ((uint64_t)(key - 1) >= (uint64_t)bmax) {
                atomicAdd(bm_err, 1ull);
                continue;
            }
            d_kbit_set(kbits, key);
        }
        uint64_t h = pg_murmur3_finalize(pg_bigint_hash(key));
        int64_t s = (int64_t)(h & (uint64_t)mask);
        int64_t tries = 0;
        for (;;) {
            int64_t old = atomicCAS((unsigned long long*)&keys[s],
                                    (unsigned long long)TBL_EMPTY,
                                    (unsigned long long)word);
            if (old == TBL_EMPTY || old == word) {
                if (old == TBL_EMPTY) {
                    my_inserted++;
                    if (tags) tags[s] = d_tbl_tag(h);
                }
                if (pbits) break; /* payload lives in the slot word */
                if (lu_payload && dp.n >= 1)
                    ((uint8_t*)dp.ptr[0])[s] = plv;
                for (int o = lu_payload ? 1 : 0; o < dp.n; o++) {
                    const pg_col& c = pg.cols[dp.src[o]];
                    switch (dp.tag[o]) {
                        case PG_T_U8:
                            ((uint8_t*)dp.ptr[o])[s] =
                                (uint8_t)d_load_i64(c, i);
                            break;
                        case PG_T_I32:
                            ((int32_t*)dp.ptr[o])[s] =
                                (int32_t)d_load_i64(c, i);
                            break;
                        case PG_T_I64:
                            ((int64_t*)dp.ptr[o])[s] = d_load_i64(c, i);
                            break;
                        default:
                            ((double*)dp.ptr[o])[s] = d_load_f64(c, i);
                    }
                }
                break;
            }
            if (++tries > mask) { /* table full: bounded give-up */
                my_overflow++;
                break;
            }
            s = (s + 1) & mask;
        }
    }
    /* one atomic per wave, not per insert (a single-address atomicAdd per
     * row serializes the whole grid) */
    my_inserted = d_bfly_i64(my_inserted);
    my_overflow = d_bfly_i64(my_overflow);
    my_packerr = d_bfly_i64(my_packerr);
    if ((threadIdx.x & 63) == 0) {
        if (my_inserted) atomicAdd(inserted, (unsigned long long)my_inserted);
        if (my_overflow) atomicAdd(overflow, (unsigned long long)my_overflow);
        if (my_packerr) atomicAdd(pack_err, (unsigned long long)my_packerr);
    }
}

/* Staged direct insert: the Q3/Q5 orders-build shape of
 * k_tbl_insert_direct (packed slot word, 0-2 literal int32 predicates,
 * optional dense flag semijoin, optional dense u8 payload lookup; BuildOp
 * gates it per page).  The generic kernel walks one row per thread
 * through a chain of dependent misses (predicate column -> semijoin key
 * -> flag gather -> build key -> CAS); here a thread owns BS_R
 * consecutive rows of a 1024-row block tile and every load of a stage is
 * issued for all of them before any result is consumed:
 *   A  nontemporal vector loads of the predicate / semijoin / lookup /
 *      build-key columns and the loads of a payload column of its own,
 *      unconditionally;
 *   B  predicates, then the dense flag and lookup gathers of all rows,
 *      from an index clamped to 0 for the rows that did not pass, and the
 *      select afterwards;
 *   C  pack and bitmap range checks, bitmap set, bounded CAS probe, tag
 *      store — per row exactly what the generic kernel does; the first
 *      CAS of every surviving row goes out before any result is read.
 * A load that sits behind a branch of its own is waited for before the
 * next one is issued, even where the condition is the same for the whole
 * launch, so the shape of the page (number of predicates, semijoin,
 * lookup, payload source) is a template parameter and the host picks the
 * instance (bs_pick); only the last, partial tile of a page takes the
 * scalar path with its per-row bounds tests.
 * Measured on the SF100 Q3 build (profiles/build_staged.json): 2.80 ms ->
 * 2.04 ms.  Deferring the build-key load to the ~10% of rows that pass
 * (2.08 ms) and compacting a tile's survivors through LDS so that the CAS
 * chains run in full waves (2.13 ms) both measured slower and are not
 * kept.  Issuing each stage's loads together took 78 VGPRs to 53 and the
 * occupancy from 6 to 8 waves per SIMD, but only 2.04 -> 2.00 ms
 * (profiles/q3_streams.json): the kernel is not bound by those round
 * trips.  Loading the next tile's stage A between the gathers and their
 * first use (74 VGPRs, occupancy 6; 1.74 against 1.76 ms) and grids of
 * 2048 and 8192 blocks (1.77, 1.72 ms) are inside the run-to-run spread
 * and are not kept.  What did pay is leaving the tag array out under an
 * exact bitmap (BuildOp::init): 2.00 -> 1.76 ms.
 * No block waits on another; every loop is bounded. */
#define BS_R 4
#define BS_TILE (256 * BS_R)
#define BS_GRID 4096 /* blocks at most; a block walks tiles BS_GRID apart */
/* payload source of a staged page */
enum {
    BS_PAY_PRED = 0, /* the predicate column #pay_pred */
    BS_PAY_LOOKUP,   /* the dense u8 lookup */
    BS_PAY_I32,      /* a column of its own, by type */
    BS_PAY_U8,
    BS_PAY_I64
};
struct staged_args {
    const int32_t* pc[2]; /* predicate columns (I32) */
    int64_t pval[2];
    int32_t pop[2];
    int32_t n_preds;
    const int64_t* sk;    /* semijoin key column, or null */
    const uint8_t* flags; /* dense flag set over keys 1..nflags */
    int64_t nflags;
    const int64_t* lk;    /* payload lookup key column, or null */
    const uint8_t* lu;    /* dense u8 lookup over keys 1..lucap */
    int64_t lucap;
    const int64_t* key;   /* build key column */
    const void* pay;      /* payload column (no lookup, pay_pred < 0) */
    int32_t pay_tag;
    int32_t pay_pred;     /* >= 0: the payload is predicate column #n */
    int64_t n;
};
__device__ inline bool d_cmp_i64(int32_t op, int64_t v, int64_t x)
{
    switch (op) {
        case PG_CMP_LT: return v < x;
        case PG_CMP_LE: return v <= x;
        case PG_CMP_GT: return v > x;
        case PG_CMP_GE: return v >= x;
        case PG_CMP_EQ: return v == x;
        default: return v != x;
    }
}
/* BS_R rows of a full tile: 16-byte nontemporal loads */
__device__ inline void d_bs_vload_i32(const int32_t* p, int32_t* out)
{
    typedef int vi4 __attribute__((ext_vector_type(4)));
    vi4 v = __builtin_nontemporal_load((const vi4*)p);
#pragma unroll
    for (int j = 0; j < BS_R; j++) out[j] = v[j];
}
__device__ inline void d_bs_vload_i64(const int64_t* p, int64_t* out)
{
    typedef long vl2 __attribute__((ext_vector_type(2)));
#pragma unroll
    for (int j = 0; j < BS_R; j += 2) {
        vl2 v = __builtin_nontemporal_load((const vl2*)(p + j));
        out[j] = v[0];
        out[j + 1] = v[1];
    }
}
/* row i of a payload column of its own (the gate asks no alignment of
 * it, so it is read by element) */
template <int PAY>
__device__ inline int64_t d_bs_pay(const void* p, int64_t i)
{
    if constexpr (PAY == BS_PAY_I32) return ((const int32_t*)p)[i];
    else if constexpr (PAY == BS_PAY_U8) return ((const uint8_t*)p)[i];
    else return ((const int64_t*)p)[i];
}
/* the probe loop of k_tbl_insert_direct for a packed word, entered with
 * the result of the first CAS already in hand */
__device__ inline void d_bs_probe(int64_t* keys, uint8_t* tags,
                                  int64_t mask, uint64_t h, int64_t s,
                                  int64_t word, int64_t old,
                                  int64_t& my_inserted, int64_t& my_overflow)
{
    int64_t tries = 0;
    for (;;) {
        if (old == TBL_EMPTY || old == word) {
            if (old == TBL_EMPTY) {
                my_inserted++;
                if (tags) tags[s] = d_tbl_tag(h);
            }
            return;
        }
        if (++tries > mask) { /* table full: bounded give-up */
            my_overflow++;
            return;
        }
        s = (s + 1) & mask;
        old = atomicCAS((unsigned long long*)&keys[s],
                        (unsigned long long)TBL_EMPTY,
                        (unsigned long long)word);
    }
}
template <int NP, bool SK, bool LK, int PAY>
__global__ __launch_bounds__(256) void k_tbl_insert_staged(
    staged_args a, int32_t pbits, int64_t* keys, uint8_t* tags,
    int64_t mask, unsigned long long* inserted,
    unsigned long long* overflow, unsigned long long* pack_err,
    unsigned long long* kbits, int64_t bmax, unsigned long long* bm_err)
{
    constexpr bool OWN_PAY = PAY >= BS_PAY_I32;
    const int64_t n = a.n;
    const int64_t n_tiles = (n + BS_TILE - 1) / BS_TILE;
    int64_t my_inserted = 0, my_overflow = 0, my_packerr = 0;
    for (int64_t tile = blockIdx.x; tile < n_tiles; tile += gridDim.x) {
        const int64_t base = tile * BS_TILE + (int64_t)threadIdx.x * BS_R;
        /* ---- stage A ---- */
        int32_t pv[2][BS_R] = {};
        int64_t skv[BS_R] = {}, lkv[BS_R] = {}, kv[BS_R], pay[BS_R] = {};
        if (base + BS_R <= n) {
            if constexpr (NP > 0) d_bs_vload_i32(a.pc[0] + base, pv[0]);
            if constexpr (NP > 1) d_bs_vload_i32(a.pc[1] + base, pv[1]);
            if constexpr (SK) d_bs_vload_i64(a.sk + base, skv);
            if constexpr (LK) d_bs_vload_i64(a.lk + base, lkv);
            d_bs_vload_i64(a.key + base, kv);
            if constexpr (OWN_PAY) {
#pragma unroll
                for (int j = 0; j < BS_R; j++)
                    pay[j] = d_bs_pay<PAY>(a.pay, base + j);
            }
        } else { /* scalar tail: the last, partial tile of the page */
#pragma unroll
            for (int j = 0; j < BS_R; j++) {
                const bool in = base + j < n;
                if constexpr (NP > 0) pv[0][j] = in ? a.pc[0][base + j] : 0;
                if constexpr (NP > 1) pv[1][j] = in ? a.pc[1][base + j] : 0;
                if constexpr (SK) skv[j] = in ? a.sk[base + j] : 0;
                if constexpr (LK) lkv[j] = in ? a.lk[base + j] : 0;
                kv[j] = in ? a.key[base + j] : 0;
                if constexpr (OWN_PAY)
                    pay[j] = in ? d_bs_pay<PAY>(a.pay, base + j) : 0;
            }
        }
        /* ---- stage B ---- */
        bool ok[BS_R];
#pragma unroll
        for (int j = 0; j < BS_R; j++) {
            ok[j] = base + j < n;
            if constexpr (NP > 0)
                ok[j] = ok[j] && d_cmp_i64(a.pop[0], pv[0][j], a.pval[0]);
            if constexpr (NP > 1)
                ok[j] = ok[j] && d_cmp_i64(a.pop[1], pv[1][j], a.pval[1]);
            /* keys outside the dense ranges are dropped before the gather */
            if constexpr (LK)
                ok[j] = ok[j] && lkv[j] >= 1 && lkv[j] <= a.lucap;
            if constexpr (SK)
                ok[j] = ok[j] && skv[j] >= 1 && skv[j] <= a.nflags;
        }
        /* every gather goes out, a dropped row's from index 0 (the host
         * sees to it that byte 0 exists), and is selected afterwards */
        uint8_t fl[BS_R], plv[BS_R];
#pragma unroll
        for (int j = 0; j < BS_R; j++) {
            if constexpr (SK) fl[j] = a.flags[ok[j] ? skv[j] - 1 : 0];
            if constexpr (LK) plv[j] = a.lu[ok[j] ? lkv[j] - 1 : 0];
        }
#pragma unroll
        for (int j = 0; j < BS_R; j++) {
            if constexpr (SK) ok[j] = ok[j] && fl[j] != 0;
            if constexpr (LK) pay[j] = plv[j];
            else if constexpr (PAY == BS_PAY_PRED)
                pay[j] = a.pay_pred ? pv[1][j] : pv[0][j];
        }
        /* ---- stage C ---- */
        int64_t word[BS_R];
#pragma unroll
        for (int j = 0; j < BS_R; j++) {
            word[j] = 0;
            if (!ok[j]) continue;
            const int64_t key = kv[j];
            if (key < 0 || key >= (1ll << (63 - pbits)) || pay[j] < 0 ||
                pay[j] >= (1ll << pbits)) {
                my_packerr++;
                ok[j] = false;
                continue;
            }
            if (kbits) {
                if ((uint64_t)(key - 1) >= (uint64_t)bmax) {
                    atomicAdd(bm_err, 1ull);
                    ok[j] = false;
                    continue;
                }
                d_kbit_set(kbits, key);
            }
            word[j] = (key << pbits) | pay[j];
        }
        uint64_t h[BS_R];
        int64_t old[BS_R];
#pragma unroll
        for (int j = 0; j < BS_R; j++) {
            h[j] = pg_murmur3_finalize(pg_bigint_hash(kv[j]));
            old[j] = 0;
            if (ok[j])
                old[j] = atomicCAS(
                    (unsigned long long*)&keys[h[j] & (uint64_t)mask],
                    (unsigned long long)TBL_EMPTY,
                    (unsigned long long)word[j]);
        }
#pragma unroll
        for (int j = 0; j < BS_R; j++)
            if (ok[j])
                d_bs_probe(keys, tags, mask, h[j],
                           (int64_t)(h[j] & (uint64_t)mask), word[j], old[j],
                           my_inserted, my_overflow);
    }
    /* one atomic per wave, as in k_tbl_insert_direct */
    my_inserted = d_bfly_i64(my_inserted);
    my_overflow = d_bfly_i64(my_overflow);
    my_packerr = d_bfly_i64(my_packerr);
    if ((threadIdx.x & 63) == 0) {
        if (my_inserted) atomicAdd(inserted, (unsigned long long)my_inserted);
        if (my_overflow) atomicAdd(overflow, (unsigned long long)my_overflow);
        if (my_packerr) atomicAdd(pack_err, (unsigned long long)my_packerr);
    }
}
/* the instance of k_tbl_insert_staged for a page's shape */
typedef void (*staged_fn)(staged_args, int32_t, int64_t*, uint8_t*, int64_t,
                          unsigned long long*, unsigned long long*,
                          unsigned long long*, unsigned long long*, int64_t,
                          unsigned long long*);
template <int NP, bool SK>
static staged_fn bs_pick_pay(const staged_args& a)
{
    if (a.lk) return k_tbl_insert_staged<NP, SK, true, BS_PAY_LOOKUP>;
    if (a.pay_pred >= 0)
        return k_tbl_insert_staged<NP, SK, false, BS_PAY_PRED>;
    switch (a.pay_tag) {
        case PG_T_I32:
            return k_tbl_insert_staged<NP, SK, false, BS_PAY_I32>;
        case PG_T_U8:
            return k_tbl_insert_staged<NP, SK, false, BS_PAY_U8>;
        default:
            return k_tbl_insert_staged<NP, SK, false, BS_PAY_I64>;
    }
}
static staged_fn bs_pick(const staged_args& a)
{
    switch (a.n_preds) {
        case 0:
            return a.sk ? bs_pick_pay<0, true>(a) : bs_pick_pay<0, false>(a);
        case 1:
            return a.sk ? bs_pick_pay<1, true>(a) : bs_pick_pay<1, false>(a);
        default:
            return a.sk ? bs_pick_pay<2, true>(a) : bs_pick_pay<2, false>(a);
    }
}

/* ------------------------------------------------------------------ */
/* Radix-partitioned agg-table build (round 2).                        */
/* The old direct insert (k_tbl_insert_direct) random-stores into the  */
/* whole table: at SF100 the Q3 orders build fetched ~12.5 GB against  */
/* ~3 GB of algorithmic input (profiles/r01_q3_sf100_pmc.txt) because  */
/* every insert pulls whole 64-B lines of an HBM-resident table.       */
/* Fix: (A) one fused filter+semijoin+lookup+hash pass scatters the    */
/* surviving {key, payload} records into per-partition staging runs    */
/* (partition = high bits of the masked slot index, so probes keep     */
/* bit-identical slot math); (B) a persistent kernel then initializes  */
/* and fills K partition regions at a time — each region sized to sit  */
/* in the 256 MiB Infinity Cache — separated by grid barriers, so the  */
/* random CAS/stores hit L3 instead of HBM and each table line is      */
/* written back exactly once.                                          */
/* ------------------------------------------------------------------ */
#define SCAT_TILE 8192
#define SCAT_MAXP 256

struct build_row {
    int64_t key;
    int64_t pay[4];
};

/* shared row evaluation for the partitioned build: predicates, fused
 * dimension lookup, semijoin, then key + payload words (f64 payloads are
 * bit-copied).  Returns 0 when the row is dropped. */
__device__ inline int d_build_eval(
    const pg_page& pg, const pg_plan_hash_build& plan,
    const int64_t* set_keys, int64_t set_mask, const int64_t* lu_keys,
    const uint8_t* lu_tags, int64_t lu_mask, int64_t lu_lmask,
    const uint8_t* lu_payload, const direct_payloads& dp, int64_t i,
    bool want_pay, build_row* out)
{
    if (!d_eval_preds<false>(pg, plan.preds, plan.n_preds, i)) return 0;
    uint8_t plv = 0;
    if (lu_payload) {
        int64_t k2 = d_load_i64(pg.cols[plan.payload_lookup_key_col], i);
        int64_t sl2;
        if (lu_keys)
            sl2 = d_tbl_find_tagged(lu_keys, lu_tags, lu_mask, lu_lmask,
                                    0, k2);
        else /* dense: payload[key-1], lu_mask = capacity */
            sl2 = (k2 >= 1 && k2 <= lu_mask) ? k2 - 1 : -1;
        if (sl2 < 0) return 0;
        plv = lu_payload[sl2];
        out->pay[0] = (int64_t)plv; /* cached even when !want_pay (the
                                       scatter pass-1 LDS row tag) */
    }
    if (set_keys) {
        int64_t sk = d_load_i64(pg.cols[plan.semijoin_col], i);
        bool found;
        if (set_mask < 0) {
            found = sk >= 1 && sk <= -set_mask &&
                    ((const uint8_t*)set_keys)[sk - 1];
        } else {
            found = false;
            uint64_t h = pg_murmur3_finalize(pg_bigint_hash(sk));
            int64_t s = (int64_t)(h & (uint64_t)set_mask);
            for (;;) {
                int64_t k = set_keys[s];
                if (k == sk) { found = true; break; }
                if (k == TBL_EMPTY) break;
                s = (s + 1) & set_mask;
            }
        }
        if (!found) return 0;
    }
    out->key = d_load_i64(pg.cols[plan.key_col], i);
    if (want_pay) {
        if (lu_payload && dp.n >= 1) out->pay[0] = (int64_t)plv;
        for (int o = lu_payload ? 1 : 0; o < dp.n; o++) {
            const pg_col& c = pg.cols[dp.src[o]];
            if (dp.tag[o] == PG_T_F64) {
                double v = d_load_f64(c, i);
                int64_t b;
                memcpy(&b, &v, 8);
                out->pay[o] = b;
            } else {
                out->pay[o] = d_load_i64(c, i);
            }
        }
    }
    return 1;
}

/* (A) fused filter + partition scatter: per-tile LDS counting sort —
 * pass 1 evaluates each row ONCE (predicates + semijoin + dimension
 * lookup), caching {partition+1, lookup payload} per row in a 32 KB LDS
 * tile; the cursor reservation costs ~P global atomics per 8192-row
 * tile; pass 2 re-reads only the SELECTED rows' key/payload columns and
 * places the records in dense per-partition runs. */
__global__ __launch_bounds__(256) void k_part_scatter(
    pg_page pg, pg_plan_hash_build plan, const int64_t* set_keys,
    int64_t set_mask, const int64_t* lu_keys, const uint8_t* lu_tags,
    int64_t lu_mask, int64_t lu_lmask, const uint8_t* lu_payload,
    direct_payloads dp, int64_t mask, int32_t capp_bits, int32_t P,
    int64_t* stage, unsigned long long* cursor, int64_t cap_stage_rows,
    int32_t r_words, unsigned long long* stage_ovf)
{
    __shared__ unsigned int cnt[SCAT_MAXP];
    __shared__ unsigned int c2[SCAT_MAXP];
    __shared__ unsigned long long gbase[SCAT_MAXP];
    /* per-row eval cache: low 16 bits = partition+1 (0 = dropped),
     * high 16 = the u8 lookup payload */
    __shared__ unsigned int rowp[SCAT_TILE];
    const int64_t n = pg.n_rows;
    for (int64_t t0 = (int64_t)blockIdx.x * SCAT_TILE; t0 < n;
         t0 += (int64_t)gridDim.x * SCAT_TILE) {
        const int64_t t1 = t0 + SCAT_TILE < n ? t0 + SCAT_TILE : n;
        for (int p = threadIdx.x; p < P; p += 256) {
            cnt[p] = 0;
            c2[p] = 0;
        }
        __syncthreads();
        for (int64_t i = t0 + threadIdx.x; i < t1; i += 256) {
            build_row r;
            r.pay[0] = 0;
            unsigned int tagw = 0;
            if (d_build_eval(pg, plan, set_keys, set_mask, lu_keys,
                             lu_tags, lu_mask, lu_lmask, lu_payload, dp,
                             i, false, &r)) {
                uint64_t h = pg_murmur3_finalize(pg_bigint_hash(r.key));
                int p = (int)((h & (uint64_t)mask) >> capp_bits);
                atomicAdd(&cnt[p], 1u);
                tagw = (unsigned int)(p + 1) |
                       ((unsigned int)(uint8_t)r.pay[0] << 16);
            }
            rowp[i - t0] = tagw;
        }
        __syncthreads();
        for (int p = threadIdx.x; p < P; p += 256) {
            if (cnt[p]) {
                unsigned long long b =
                    atomicAdd(&cursor[p], (unsigned long long)cnt[p]);
                gbase[p] = b;
                if (b + cnt[p] > (unsigned long long)cap_stage_rows)
                    atomicAdd(stage_ovf, 1ull);
            }
        }
        __syncthreads();
        for (int64_t i = t0 + threadIdx.x; i < t1; i += 256) {
            unsigned int tagw = rowp[i - t0];
            if (!tagw) continue;
            int p = (int)(tagw & 0xffffu) - 1;
            unsigned long long row = gbase[p] + atomicAdd(&c2[p], 1u);
            if (row >= (unsigned long long)cap_stage_rows) continue;
            int64_t* rec = stage +
                ((int64_t)p * cap_stage_rows + (int64_t)row) * r_words;
            rec[0] = d_load_i64(pg.cols[plan.key_col], i);
            const bool lu = lu_payload != nullptr;
            if (lu && dp.n >= 1) rec[1] = (int64_t)(tagw >> 16);
            for (int o = lu ? 1 : 0; o < dp.n; o++) {
                const pg_col& c = pg.cols[dp.src[o]];
                if (dp.tag[o] == PG_T_F64) {
                    double v = d_load_f64(c, i);
                    int64_t b;
                    memcpy(&b, &v, 8);
                    rec[1 + o] = b;
                } else {
                    rec[1 + o] = d_load_i64(c, i);
                }
            }
        }
        __syncthreads();
    }
}

/* grid barrier for the persistent insert kernel: monotonic counter,
 * agent-scope release before arrive / acquire after (per-XCD L2s are not
 * coherent — MI355X_MICROARCH.md §Workgroup dispatch; the inline
 * s_waitcnt guards the known ROCm 7.2 release-fence hazard).  Caller
 * guarantees every block is resident (grid <= 1 block per CU). */
__device__ inline void d_grid_barrier(unsigned long long* bar,
                                      unsigned long long target)
{
    __syncthreads();
    if (threadIdx.x == 0) {
        __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
        asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
        __hip_atomic_fetch_add(bar, 1ull, __ATOMIC_RELAXED,
                               __HIP_MEMORY_SCOPE_AGENT);
        while (__hip_atomic_load(bar, __ATOMIC_RELAXED,
                                 __HIP_MEMORY_SCOPE_AGENT) < target)
            __builtin_amdgcn_s_sleep(32);
        __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    }
    __syncthreads();
}

/* (B) persistent partitioned insert: waves of K L3-resident regions —
 * init the region slots, barrier, CAS-insert that wave's staged rows
 * (partition-local linear probe), barrier, next wave. */
__global__ __launch_bounds__(256) void k_part_insert(
    const int64_t* stage, const unsigned long long* cursor,
    int64_t cap_stage_rows, int32_t r_words, int64_t* keys, uint8_t* tags,
    direct_payloads dp, int64_t cap_p, int32_t P, int32_t K,
    int32_t use_barrier, int32_t pbits, unsigned long long* bar,
    unsigned long long* inserted, unsigned long long* overflow,
    unsigned long long* pack_err, unsigned long long* kbits, int64_t bmax,
    unsigned long long* bm_err)
{
    int64_t my_packerr = 0;
    /* use_barrier=1: init K L3-resident regions in-kernel between grid
     * barriers (strict cache blocking; grid must be all-resident).
     * use_barrier=0 (default): table pre-initialized by k_tbl_init; the
     * partition-ORDERED staging alone clusters each region's CAS/store
     * lines in time, so they are pulled into L3 once and written back
     * once — no barrier, any grid size. */
    const int64_t lmask = cap_p - 1;
    const int64_t stride = (int64_t)gridDim.x * 256;
    int64_t my_ins = 0, my_ovf = 0;
    unsigned long long target = 0;
    for (int32_t w0 = 0; w0 < P; w0 += K) {
        const int32_t kmax = w0 + K <= P ? K : P - w0;
        const int64_t tot = (int64_t)kmax * cap_p;
        const int64_t wave_base = (int64_t)w0 * cap_p;
        if (use_barrier) {
            for (int64_t idx = (int64_t)blockIdx.x * 256 + threadIdx.x;
                 idx < tot; idx += stride) {
                keys[wave_base + idx] = TBL_EMPTY;
                if (tags) tags[wave_base + idx] = 0;
            }
            target += gridDim.x;
            d_grid_barrier(bar, target);
        }
        for (int32_t k = 0; k < kmax; k++) {
            const int32_t p = w0 + k;
            int64_t n_p = (int64_t)cursor[p];
            if (n_p > cap_stage_rows) n_p = cap_stage_rows;
            const int64_t base_slot = (int64_t)p * cap_p;
            const int64_t* prows = stage + (int64_t)p * cap_stage_rows *
                                              r_words;
            for (int64_t r = (int64_t)blockIdx.x * 256 + threadIdx.x;
                 r < n_p; r += stride) {
                const int64_t* rec = prows + r * r_words;
                const int64_t key = rec[0];
                int64_t word = key;
                if (pbits) {
                    int64_t pay0 = rec[1];
                    if (key < 0 || key >= (1ll << (63 - pbits)) ||
                        pay0 < 0 || pay0 >= (1ll << pbits)) {
                        my_packerr++;
                        continue;
                    }
                    word = (key << pbits) | pay0;
                }
                if (kbits) {
                    if ((uint64_t)(key - 1) >= (uint64_t)bmax) {
                        atomicAdd(bm_err, 1ull);
                        continue;
                    }
                    d_kbit_set(kbits, key);
                }
                uint64_t h = pg_murmur3_finalize(pg_bigint_hash(key));
                int64_t off = (int64_t)(h & (uint64_t)lmask);
                int64_t tries = 0;
                for (;;) {
                    int64_t s = base_slot + off;
                    int64_t old =
                        atomicCAS((unsigned long long*)&keys[s],
                                  (unsigned long long)TBL_EMPTY,
                                  (unsigned long long)word);
                    if (old == TBL_EMPTY || old == word) {
                        if (old == TBL_EMPTY) {
                            my_ins++;
                            if (tags) tags[s] = d_tbl_tag(h);
                        }
                        if (pbits) break;
                        for (int o = 0; o < dp.n; o++) {
                            int64_t w = rec[1 + o];
                            switch (dp.tag[o]) {
                                case PG_T_U8:
                                    ((uint8_t*)dp.ptr[o])[s] = (uint8_t)w;
                                    break;
                                case PG_T_I32:
                                    ((int32_t*)dp.ptr[o])[s] = (int32_t)w;
                                    break;
                                default: /* I64 and F64 bits */
                                    ((int64_t*)dp.ptr[o])[s] = w;
                            }
                        }
                        break;
                    }
                    if (++tries > lmask) {
                        my_ovf++;
                        break;
                    }
                    off = (off + 1) & lmask;
                }
            }
        }
        if (use_barrier) {
            target += gridDim.x;
            d_grid_barrier(bar, target);
        }
    }
    my_ins = d_bfly_i64(my_ins);
    my_ovf = d_bfly_i64(my_ovf);
    my_packerr = d_bfly_i64(my_packerr);
    if ((threadIdx.x & 63) == 0) {
        if (my_ins) atomicAdd(inserted, (unsigned long long)my_ins);
        if (my_ovf) atomicAdd(overflow, (unsigned long long)my_ovf);
        if (my_packerr)
            atomicAdd(pack_err, (unsigned long long)my_packerr);
    }
}

__device__ inline int64_t d_tbl_find(const int64_t* keys, int64_t mask,
                                     int64_t lmask, int32_t pbits,
                                     int64_t key)
{
    /* pbits > 0: slot word = key << pbits | payload (pg_plan_hash_build
     * .pack_bits) — compare the key field only */
    uint64_t h = pg_murmur3_finalize(pg_bigint_hash(key));
    int64_t s = (int64_t)(h & (uint64_t)mask);
    for (;;) {
        int64_t k = keys[s];
        if (k == TBL_EMPTY) return -1;
        if ((k >> pbits) == key) return s;
        s = d_probe_next(s, lmask);
    }
}


__device__ inline int64_t d_tbl_find_tagged(const int64_t* keys,
                                            const uint8_t* tags,
                                            int64_t mask, int64_t lmask,
                                            int32_t pbits, int64_t key)
{
    if (!tags) return d_tbl_find(keys, mask, lmask, pbits, key);
    uint64_t h = pg_murmur3_finalize(pg_bigint_hash(key));
    int64_t s = (int64_t)(h & (uint64_t)mask);
    uint8_t tag = d_tbl_tag(h);
    for (;;) {
        uint8_t t = tags[s];
        if (t == 0) return -1;
        if (t == tag && (keys[s] >> pbits) == key) return s;
        s = d_probe_next(s, lmask);
    }
}

/* per-slot accumulators, interleaved so one probe hit touches ONE cache
 * line (32 B of one 64-B line) instead of four separate arrays */
/* per-slot accumulators: 4 words [dec ticks, fx128 lo, fx128 hi, cnt],
 * or the SLIM 2-word layout [dec ticks, cnt] when every probe of the
 * table is dec_only/dec_min (integer consumers — halves the zeroing and
 * extraction traffic).  Kernels take the word stride (aw); cnt is the
 * last word. */
struct slot_acc {
    unsigned long long dec;  /* exact decimal ticks */
    unsigned long long flo;  /* 64.64 fixed-point f64 sum, low word */
    unsigned long long fhi;  /* high word (carries) */
    unsigned long long cnt;
};

/* overflow-checked atomic tick add: a wrapped int64 tick sum is raised as
 * an operator error, never silent (Math.addExact semantics,
 * LongSumAggregation.java:33-37; exact-decimal sums depend on never
 * wrapping).  Detection is post-hoc from the returned old value. */
__device__ inline void d_atomic_add_dec_ck(unsigned long long* slot,
                                           int64_t ticks,
                                           unsigned long long* ovf)
{
    long long old = (long long)atomicAdd(slot, (unsigned long long)ticks);
    long long nv = old + ticks;
    if (((old ^ nv) & (ticks ^ nv)) < 0 && ovf) atomicAdd(ovf, 1ull);
}

/* Hit list of a table (Table::hits): the mode-1 probes append every slot
 * whose count they take from 0, so extraction gathers those slots.  The
 * add that returns 0 is unique per slot and accumulator lifetime, so each
 * group is appended exactly once.  First touches are rare (0.2 % of Q3's
 * probe rows) and the cursor is one address, so a wave stages them in 64
 * LDS entries of its own and flushes a full buffer with one cursor add
 * and one coalesced store.  The staging is wave-synchronous: every lane
 * of the wave calls in, so the probe loops bound their trip count by the
 * wave's first lane and predicate per lane. */
struct hit_list {
    void* ents; /* null: do not append */
    unsigned long long* cursor;
    int64_t cap; /* entries; a flush never stores beyond it */
    int32_t wide; /* int64 entries (cap > 2^32), else uint32 */
};

__device__ inline void d_hits_flush(const hit_list& hl,
                                    volatile int64_t* wbuf, int cnt)
{
    const int lane = threadIdx.x & 63;
    int64_t g = 0;
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "wavefront");
    __builtin_amdgcn_wave_barrier();
    if (lane == 0)
        g = (int64_t)atomicAdd(hl.cursor, (unsigned long long)cnt);
    g = __shfl(g, 0, WAVE);
    if (lane < cnt && g + lane < hl.cap) {
        int64_t s = wbuf[lane];
        if (hl.wide)
            ((int64_t*)hl.ents)[g + lane] = s;
        else
            ((uint32_t*)hl.ents)[g + lane] = (uint32_t)s;
    }
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "wavefront");
    __builtin_amdgcn_wave_barrier();
}

/* all 64 lanes call; lanes with ft stage their slot.  *cnt is the wave's
 * staged count, the same in every lane. */
__device__ inline void d_hits_stage(const hit_list& hl,
                                    volatile int64_t* wbuf, int* cnt,
                                    bool ft, int64_t slot)
{
    uint64_t m = d_ballot(ft);
    if (!m) return;
    const int lane = threadIdx.x & 63;
    int pos = *cnt + __popcll(m & ((1ull << lane) - 1));
    int total = *cnt + __popcll(m);
    if (ft && pos < WAVE) wbuf[pos] = slot;
    if (total >= WAVE) {
        d_hits_flush(hl, wbuf, WAVE);
        if (ft && pos >= WAVE) wbuf[pos - WAVE] = slot;
        total -= WAVE;
    }
    *cnt = total;
}

/* probe + fused grouped SUM into table accumulators (Q3's
 * LookupJoinOperator + HashAggregationOperator fused; revenue summed
 * exactly in decimal ticks AND in 64.64 fixed point — order-independent,
 * so atomics preserve bit-determinism) */
/* waves_per_eu(7): the occupancy this kernel had before the hit list */
__global__ __launch_bounds__(256)
__attribute__((amdgpu_waves_per_eu(7))) void k_probe_agg(
    pg_page pg, pg_plan_lookup_join plan, const int64_t* keys,
    const uint8_t* tags, int64_t mask, int64_t lmask, int32_t pbits,
    const unsigned long long* kbits, int64_t bmax,
    unsigned long long* acc, int32_t aw,
    unsigned long long* ovf /* [tick overflow, SUM_F64 domain] */,
    hit_list hl)
{
    /* 4 CONSECUTIVE rows per thread with run dedup: neighboring rows
     * often share the join key (lineitem is clustered by orderkey), so
     * a run of equal keys probes the table ONCE and flushes one set of
     * atomics — on all-hit per-order aggregations this cuts both the
     * random key-line pulls and the accumulator atomics ~4x.  Exact:
     * dedup is by key equality, never an assumption of sortedness. */
    const int C = 4;
    int64_t base =
        ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * C;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x * C;
    const int lane = threadIdx.x & 63;
    __shared__ int64_t hbuf[4][WAVE];
    volatile int64_t* wbuf = hbuf[threadIdx.x >> 6];
    int hcnt = 0;
    /* the wave's first lane bounds the loop (lanes past the end run an
     * empty row loop), so the hit-list staging sees whole waves */
    for (; base - C * lane < pg.n_rows; base += stride) {
        const int64_t lim = base + C < pg.n_rows ? base + C : pg.n_rows;
        int64_t cur_key = 0, cur_slot = -2; /* -2 = no open run */
        /* slots this thread first-touched in this pass: at most one per
         * row, kept newest-first in registers */
        int64_t fts[C] = {0, 0, 0, 0};
        int nft = 0;
        int64_t run_dec = 0;
        long long run_min = INT64_MAX;
        uint64_t run_flo = 0, run_fhi = 0;
        int run_cnt = 0;
        auto flush = [&]() {
            if (cur_slot < 0 || run_cnt == 0) return;
            unsigned long long* s = acc + (size_t)cur_slot * aw;
            if (plan.dec_min) {
                atomicMin((long long*)&s[0], run_min);
            } else if (run_dec) {
                d_atomic_add_dec_ck(&s[0], run_dec, ovf);
            }
            if (!plan.dec_only && !plan.dec_min && (run_flo | run_fhi)) {
                unsigned long long old = atomicAdd(&s[1], run_flo);
                atomicAdd(&s[2],
                          run_fhi + (old > ~run_flo ? 1ull : 0ull));
            }
            unsigned long long old =
                atomicAdd(&s[aw - 1], (unsigned long long)run_cnt);
            if (old == 0 && hl.ents) {
#pragma unroll
                for (int k = C - 1; k > 0; k--) fts[k] = fts[k - 1];
                fts[0] = cur_slot;
                nft++;
            }
        };
        for (int64_t i = base; i < lim; i++) {
            if (!d_eval_preds(pg, plan.preds, plan.n_preds, i)) continue;
            int64_t key = d_load_i64(pg.cols[plan.key_col], i);
            if (cur_slot == -2 || key != cur_key) {
                flush();
                cur_key = key;
                if (!keys) /* range-group: acc index = key-1 */
                    cur_slot = (uint64_t)(key - 1) <= (uint64_t)mask
                                   ? key - 1
                                   : -1;
                else
                    cur_slot = kbits && !d_kbit_test(kbits, bmax, key)
                                   ? -1
                                   : d_tbl_find_tagged(keys, tags, mask,
                                                       lmask, pbits, key);
                run_dec = 0;
                run_flo = run_fhi = 0;
                run_cnt = 0;
                run_min = INT64_MAX;
            }
            if (cur_slot < 0) continue;
            pg_agg ag;
            ag.proj = plan.proj;
            ag.dec_scale = plan.dec_scale;
            int64_t ticks = d_eval_proj_dec(pg, ag, i);
            if (plan.dec_min) {
                run_min = ticks < run_min ? ticks : run_min;
            } else if (__builtin_add_overflow(run_dec, ticks, &run_dec)) {
                if (ovf) atomicAdd(ovf, 1ull);
            }
            if (!plan.dec_only && !plan.dec_min) {
                double p = d_eval_proj_f64(pg, plan.proj, i);
                uint64_t phi, plo;
                d_fx128_from_f64_ck(p, &phi, &plo, ovf + 1);
                uint64_t nlo = run_flo + plo;
                run_fhi += phi + (nlo < plo ? 1u : 0u);
                run_flo = nlo;
            }
            run_cnt++;
        }
        flush();
        if (hl.ents) {
#pragma unroll
            for (int k = 0; k < C; k++)
                d_hits_stage(hl, wbuf, &hcnt, k < nft, fts[k]);
        }
    }
    if (hl.ents && hcnt) d_hits_flush(hl, wbuf, hcnt);
}

/* specialized fused probe+agg for the Q3 shape (the codegen-analog
 * specialization, like k_agg_q1): optional single int32 predicate, i64
 * key column, DISC_PRICE(a,b) projection over two f64 columns.
 * PQ3_Q rows per thread per pass: the key/predicate columns are read with
 * nontemporal vector loads.  ep/dc are loaded only for probe hits (~9%
 * of rows at SF100): skipping the 16 B money loads on the miss path
 * saves ~5 GB of the 600M-row pass. */
/* The dependent loads of a pass go out together, row by row of a stage and
 * not stage by stage of a row: the bitmap words of all rows, then the
 * first tag and the first key word of all rows.  A row that is not
 * selected, or whose key is outside [1, bmax], or that the bitmap
 * rejected, loads word / slot 0 instead and is deselected afterwards, so
 * no load sits behind a per-row branch (the compiler waits for such a
 * load before it issues the next).  Only chains longer than one slot,
 * which are rare at fill 0.5, run one after another.  Whether there is a
 * bitmap and whether there are tags is the same for the whole launch and
 * is a template parameter.
 * Measured (profiles/q3_streams.json): this ordering left the SF100 kernel
 * where it was (2.10 ms against 2.10 ms), so the kernel is not bound by
 * the round trips of its dependent loads; four rows per thread (2.13 ms)
 * and grids of 2048 and 8192 blocks (2.13, 2.09 ms) are inside the same
 * spread and are not kept.  An earlier 4-row lockstep state machine was
 * slower than two unrolled chains. */
/* waves_per_eu(8): 4096 blocks are exactly two rounds at 8 waves per SIMD.
 * The hit-list staging raised scalar-register use past that occupancy;
 * the attribute has the compiler park the cold ones in vector lanes. */
#define PQ3_Q 2       /* rows per thread and pass */
#define PQ3_GRID 4096 /* blocks */
template <bool KB, bool TAGS>
__global__ __launch_bounds__(256)
__attribute__((amdgpu_waves_per_eu(8))) void k_probe_agg_q3(
    const int32_t* sd /* nullable pred col */, int32_t pred_op,
    int32_t pred_val, const int64_t* okey, const double* ep,
    const double* dc, int64_t n, const int64_t* keys, const uint8_t* tags,
    int64_t mask, int64_t lmask, int32_t pbits,
    const unsigned long long* kbits, int64_t bmax, int32_t dec_only,
    unsigned long long* acc, int32_t aw, unsigned long long* ovf,
    hit_list hl)
{
    typedef int vi2 __attribute__((ext_vector_type(2)));
    typedef long vl2 __attribute__((ext_vector_type(2)));
    const int Q = PQ3_Q;
    int64_t base0 = Q * ((int64_t)blockIdx.x * blockDim.x + threadIdx.x);
    int64_t stride = Q * (int64_t)gridDim.x * blockDim.x;
    const int lane = threadIdx.x & 63;
    __shared__ int64_t hbuf[4][WAVE];
    volatile int64_t* wbuf = hbuf[threadIdx.x >> 6];
    int hcnt = 0;
    /* the count adds of the previous pass: slot (< 0: no hit) and the
     * count they found.  They are looked at one pass late, behind the
     * next pass's probe loads, so the probe never waits on an add's
     * return. */
    int64_t pslot[Q];
    unsigned long long pold[Q];
#pragma unroll
    for (int j = 0; j < Q; j++) {
        pslot[j] = -1;
        pold[j] = 1;
    }
    /* the wave's first lane bounds the loop (lanes past the end take the
     * tail path with nothing selected), so the hit-list staging sees
     * whole waves; one more pass than there are rows for drains the last
     * pass's adds through the same staging code */
    for (int64_t base = base0; base - Q * lane < n + stride;
         base += stride) {
        int64_t k[Q];
        int32_t s[Q] = {};
        bool sel[Q];
        if (base + Q <= n) {
#pragma unroll
            for (int j = 0; j < Q; j += 2) {
                vl2 ka = __builtin_nontemporal_load(
                    (const vl2*)(okey + base + j));
                k[j] = ka[0]; k[j + 1] = ka[1];
            }
            if (sd) {
#pragma unroll
                for (int j = 0; j < Q; j += 2) {
                    vi2 ss = __builtin_nontemporal_load(
                        (const vi2*)(sd + base + j));
                    s[j] = ss[0]; s[j + 1] = ss[1];
                }
            }
#pragma unroll
            for (int j = 0; j < Q; j++) sel[j] = true;
        } else {
#pragma unroll
            for (int j = 0; j < Q; j++) {
                sel[j] = base + j < n;
                k[j] = sel[j] ? okey[base + j] : 0;
                s[j] = sel[j] && sd ? sd[base + j] : 0;
            }
        }
        if (sd) {
#pragma unroll
            for (int j = 0; j < Q; j++)
                sel[j] = sel[j] && (pred_op == PG_CMP_GT ? s[j] > pred_val
                                                         : s[j] < pred_val);
        }
        /* dynamic-filter bitmap: one (usually L3-hot) load rejects ~91% of
         * rows before the hash + tag/key chain */
        if constexpr (KB) {
            unsigned long long w[Q];
#pragma unroll
            for (int j = 0; j < Q; j++) {
                sel[j] = sel[j] && (uint64_t)(k[j] - 1) < (uint64_t)bmax;
                w[j] = kbits[sel[j] ? (uint64_t)k[j] >> 6 : 0];
            }
#pragma unroll
            for (int j = 0; j < Q; j++)
                sel[j] = sel[j] && ((w[j] >> (k[j] & 63)) & 1);
        }
        /* with tags and no bitmap the tags are what rejects a miss: the
         * key word is then read behind a matching tag only */
        constexpr bool KEY_WITH_TAG = KB || !TAGS;
        int64_t p[Q], kw[Q];
        uint8_t tg[Q], t[Q];
#pragma unroll
        for (int j = 0; j < Q; j++) {
            uint64_t h = pg_murmur3_finalize(pg_bigint_hash(k[j]));
            p[j] = sel[j] ? (int64_t)(h & (uint64_t)mask) : 0;
            tg[j] = d_tbl_tag(h);
            t[j] = 0;
            kw[j] = 0;
            if constexpr (TAGS) t[j] = tags[p[j]];
            if constexpr (KEY_WITH_TAG) kw[j] = keys[p[j]];
        }
        int64_t slot[Q];
#pragma unroll
        for (int j = 0; j < Q; j++) {
            slot[j] = -1;
            if (!sel[j]) continue;
            for (;;) {
                if (TAGS ? t[j] == 0 : kw[j] == TBL_EMPTY) break;
                if (!TAGS || t[j] == tg[j]) {
                    if constexpr (!KEY_WITH_TAG) kw[j] = keys[p[j]];
                    if ((kw[j] >> pbits) == k[j]) {
                        slot[j] = p[j];
                        break;
                    }
                }
                p[j] = d_probe_next(p[j], lmask);
                if constexpr (TAGS) t[j] = tags[p[j]];
                if constexpr (KEY_WITH_TAG) kw[j] = keys[p[j]];
            }
        }
        if (hl.ents) {
#pragma unroll
            for (int j = 0; j < Q; j++)
                d_hits_stage(hl, wbuf, &hcnt,
                             pslot[j] >= 0 && pold[j] == 0, pslot[j]);
        }
#pragma unroll
        for (int j = 0; j < Q; j++) {
            int64_t sl = slot[j];
            pslot[j] = sl;
            if (sl < 0) continue;
            double e = ep[base + j], d = dc[base + j];
            int64_t cents = d_round_ticks(e * 100.0);
            int64_t di = d_round_ticks(d * 100.0);
            int64_t ticks = cents * (100 - di);
            /* no per-add overflow round trip here: this specialization is
             * gated on the DISC_PRICE money shape (dec_scale 4, f64 money
             * columns < 1e7), so |ticks| < 1e9 per row and an int64 slot
             * sum cannot wrap before ~9.2e9 matched rows on ONE key —
             * far beyond a page.  The generic k_probe_agg keeps the
             * checked add.  ovf[1] counts SUM_F64 domain errors. */
            unsigned long long* s = acc + (size_t)sl * aw;
            atomicAdd(&s[0], (unsigned long long)ticks);
            if (!dec_only) {
                double pr = e * (1.0 - d);
                uint64_t phi, plo;
                d_fx128_from_f64_ck(pr, &phi, &plo, ovf + 1);
                unsigned long long old = atomicAdd(&s[1], plo);
                atomicAdd(&s[2], phi + (old > ~plo ? 1ull : 0ull));
            }
            /* exactly one add per slot and accumulator lifetime finds 0 */
            pold[j] = atomicAdd(&s[aw - 1], 1ull);
        }
    }
    if (hl.ents && hcnt) d_hits_flush(hl, wbuf, hcnt);
}

/* mode 3: probe + grouped SUM keyed by the matched build row's first
 * i64 payload, accumulated into a SECOND (agg) table — the fused
 * star-join shape (probe li -> orders, group by o_custkey): one pass,
 * two random lookups per row, no materialized join output. */
__global__ __launch_bounds__(256) void k_probe_agg_pay(
    pg_page pg, pg_plan_lookup_join plan, const int64_t* keys1,
    const uint8_t* tags1, const int32_t* head1, int64_t mask1,
    int64_t lmask1, const unsigned long long* kbits1, int64_t bmax1,
    const int64_t* pay1, const int64_t* keys2,
    const uint8_t* tags2, int64_t mask2, int64_t lmask2,
    unsigned long long* acc2, int32_t aw, unsigned long long* ovf)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < pg.n_rows; i += stride) {
        if (!d_eval_preds(pg, plan.preds, plan.n_preds, i)) continue;
        int64_t key = d_load_i64(pg.cols[plan.key_col], i);
        if (kbits1 && !d_kbit_test(kbits1, bmax1, key)) continue;
        int64_t s1 = d_tbl_find_tagged(keys1, tags1, mask1, lmask1, 0,
                                       key);
        if (s1 < 0) continue;
        int64_t r = head1 ? (int64_t)head1[s1] : s1;
        if (r < 0) continue;
        int64_t g = pay1[r];
        int64_t s2 =
            keys2 ? d_tbl_find_tagged(keys2, tags2, mask2, lmask2, 0, g)
                  : ((uint64_t)(g - 1) <= (uint64_t)mask2 ? g - 1 : -1);
        if (s2 < 0) continue;
        pg_agg ag;
        ag.proj = plan.proj;
        ag.dec_scale = plan.dec_scale;
        int64_t ticks = d_eval_proj_dec(pg, ag, i);
        unsigned long long* s = acc2 + (size_t)s2 * aw;
        d_atomic_add_dec_ck(&s[0], ticks, ovf);
        if (!plan.dec_only) {
            double p = d_eval_proj_f64(pg, plan.proj, i);
            uint64_t phi, plo;
            d_fx128_from_f64_ck(p, &phi, &plo, ovf + 1);
            unsigned long long old = atomicAdd(&s[1], plo);
            atomicAdd(&s[2], phi + (old > ~plo ? 1ull : 0ull));
        }
        atomicAdd(&s[aw - 1], 1ull);
    }
}

/* MIN-accumulator identity init (dec = +inf sentinel, rest zero) */
__global__ __launch_bounds__(256) void k_acc_min_init(
    unsigned long long* acc, int32_t aw, int64_t cap)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < cap; i += stride) {
        unsigned long long* s = acc + (size_t)i * aw;
        s[0] = 0x7f7f7f7f7f7f7f7fULL;
        for (int w = 1; w < aw; w++) s[w] = 0;
    }
}

/* probe match counting (emit mode, pass 1): per-BLOCK totals over the
 * chunked stable geometry — no per-row counts array; the emit pass
 * recomputes per-row counts and places rows with in-window prefix sums */
/* dense-array probe: present iff the payload value is nonzero (u8 flag
 * sets store 1; i32 payloads carry values the caller guarantees nonzero,
 * e.g. epoch-day dates) */
__device__ inline int64_t d_dense_find(const uint8_t* dv8,
                                       const int32_t* dv32, int64_t dcap,
                                       int64_t key)
{
    if ((uint64_t)(key - 1) >= (uint64_t)dcap) return -1;
    if (dv32) return dv32[key - 1] ? key - 1 : -1;
    return dv8[key - 1] ? key - 1 : -1;
}

/* outer-join outputs of the emit pass (modes 4-6; unused and all NULL in
 * mode 0).  pay_null: the one mask the payload columns share (PROBE_OUTER).
 * marks: one byte per build row, set when a probe row matched it (MARK).
 * pmask_src/pmask_out: per emitted probe column, the input null mask and
 * where it is gathered to (both NULL for a column without a mask). */
struct outer_outs {
    uint8_t* pay_null;
    uint8_t* marks;
    const uint8_t* pmask_src[8];
    uint8_t* pmask_out[8];
};

/* PROBE_OUTER (modes 4, 6): a probe row that passes the predicates and
 * has no match — a null key never matches — counts and emits one
 * null-padded row.  MARK (modes 5, 6): matched build rows are marked for
 * the drain; null keys are skipped.  Mode 0 is <false, false>. */
template <bool PROBE_OUTER, bool MARK>
__global__ __launch_bounds__(256) void k_probe_count(
    pg_page pg, pg_plan_lookup_join plan, const int64_t* keys,
    const uint8_t* tags, const int32_t* head, const int32_t* next,
    int64_t mask, int64_t lmask, int32_t pbits,
    const unsigned long long* kbits, int64_t bmax,
    const uint8_t* dv8, const int32_t* dv32, int64_t dcap,
    int64_t chunk, int64_t* block_counts)
{
    const int64_t n = pg.n_rows;
    const int64_t lo = (int64_t)blockIdx.x * chunk;
    const int64_t hi = min(lo + chunk, n);
    int64_t total = 0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
        if (!d_eval_preds(pg, plan.preds, plan.n_preds, i)) continue;
        if constexpr (PROBE_OUTER || MARK) {
            const uint8_t* knull = pg.cols[plan.key_col].null_mask;
            if (knull && knull[i]) {
                if constexpr (PROBE_OUTER) total++;
                continue;
            }
        }
        int64_t key = d_load_i64(pg.cols[plan.key_col], i);
        int64_t sl;
        if (dv8 || dv32) {
            sl = d_dense_find(dv8, dv32, dcap, key);
        } else {
            if (kbits && !d_kbit_test(kbits, bmax, key)) {
                if constexpr (PROBE_OUTER) total++;
                continue;
            }
            sl = d_tbl_find_tagged(keys, tags, mask, lmask, pbits, key);
        }
        if (sl >= 0) {
            if (head)
                for (int32_t r = head[sl]; r >= 0; r = next[r]) total++;
            else
                total++; /* slot-payload table: unique keys */
        } else if constexpr (PROBE_OUTER) {
            total++;
        }
    }
    total = d_bfly_i64(total);
    __shared__ int64_t lds[4];
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = total;
    __syncthreads();
    if (threadIdx.x == 0)
        block_counts[blockIdx.x] = lds[0] + lds[1] + lds[2] + lds[3];
}

/* probe emit (pass 2): offsets = exclusive scan of counts */
struct build_payloads {
    const void* ptr[4];
    int32_t tag[4];
    int32_t n;
    int32_t by_slot; /* 1: payload arrays indexed by slot, not build row */
    int32_t pack_bits; /* >0: payload[0] = keys[slot] & (2^bits-1) and the
                          emitted key = keys[slot] >> bits */
};

/* the probe columns of output row pos, from probe row i; the outer modes
 * also gather the column's null mask */
template <bool OUTER>
__device__ inline void d_emit_probe_cols(const pg_page& pg,
                                         const pg_plan_lookup_join& plan,
                                         const emit_outs& probe_outs,
                                         const outer_outs& oo, int64_t i,
                                         int64_t pos)
{
    for (int o = 0; o < probe_outs.n; o++) {
        pg_proj pr;
        pr.kind = PG_PROJ_IDENT;
        pr.a = plan.emit_probe_cols[o];
        d_emit_val(pg, pr, i, probe_outs.ptr[o], probe_outs.tag[o], pos);
        if constexpr (OUTER)
            if (oo.pmask_out[o]) oo.pmask_out[o][pos] = oo.pmask_src[o][i];
    }
}

template <bool PROBE_OUTER, bool MARK>
__global__ __launch_bounds__(256) void k_probe_emit(
    pg_page pg, pg_plan_lookup_join plan, const int64_t* keys,
    const uint8_t* tags, const int32_t* head, const int32_t* next,
    int64_t mask, int64_t lmask, int32_t pbits,
    const unsigned long long* kbits, int64_t bmax,
    const uint8_t* dv8, const int32_t* dv32, int64_t dcap,
    int64_t chunk,
    const int64_t* block_offs, emit_outs probe_outs, build_payloads bp,
    emit_outs build_outs, outer_outs oo)
{
    constexpr bool OUTER = PROBE_OUTER || MARK;
    const int64_t n = pg.n_rows;
    const int64_t lo = (int64_t)blockIdx.x * chunk;
    const int64_t hi = min(lo + chunk, n);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    __shared__ int64_t wcnt[4];
    __shared__ int64_t running;
    if (threadIdx.x == 0) running = block_offs[blockIdx.x];
    __syncthreads();
    for (int64_t base = lo; base < hi; base += 256) {
        int64_t i = base + 64 * wid + lane;
        int64_t sl = -1;
        int32_t c = 0;
        if (i < hi && d_eval_preds(pg, plan.preds, plan.n_preds, i)) {
            bool key_ok = true;
            if constexpr (OUTER) {
                const uint8_t* knull = pg.cols[plan.key_col].null_mask;
                key_ok = !(knull && knull[i]);
            }
            if (key_ok) {
                int64_t key = d_load_i64(pg.cols[plan.key_col], i);
                if (dv8 || dv32)
                    sl = d_dense_find(dv8, dv32, dcap, key);
                else
                    sl = kbits && !d_kbit_test(kbits, bmax, key)
                             ? -1
                             : d_tbl_find_tagged(keys, tags, mask, lmask,
                                                 pbits, key);
            }
            if (sl >= 0) {
                if (head)
                    for (int32_t r = head[sl]; r >= 0; r = next[r]) c++;
                else
                    c = 1;
            } else if constexpr (PROBE_OUTER) {
                c = 1; /* the null-padded row */
            }
        }
        /* wave inclusive prefix of counts (stable row order) */
        int64_t pre = c;
        for (int d = 1; d < 64; d <<= 1) {
            int64_t t = __shfl_up((long long)pre, d, 64);
            if (lane >= d) pre += t;
        }
        int64_t wtotal = __shfl((long long)pre, 63, 64);
        int64_t excl = pre - c;
        if (lane == 0) wcnt[wid] = wtotal;
        __syncthreads();
        int64_t woff = running;
        for (int w = 0; w < wid; w++) woff += wcnt[w];
        int64_t pos = woff + excl;
        if (sl >= 0)
        for (int64_t r = head ? (int64_t)head[sl] : sl; r >= 0;
             r = head ? (int64_t)next[r] : -1) {
            d_emit_probe_cols<OUTER>(pg, plan, probe_outs, oo, i, pos);
            for (int o = 0; o < bp.n; o++) {
                int64_t pv = bp.pack_bits && o == 0
                                 ? (keys[r] &
                                    ((1ll << bp.pack_bits) - 1))
                                 : 0;
                switch (bp.tag[o]) {
                    case PG_T_I32:
                        ((int32_t*)build_outs.ptr[o])[pos] =
                            bp.pack_bits && o == 0
                                ? (int32_t)pv
                                : ((const int32_t*)bp.ptr[o])[r];
                        break;
                    case PG_T_I64:
                        ((int64_t*)build_outs.ptr[o])[pos] =
                            bp.pack_bits && o == 0
                                ? pv
                                : ((const int64_t*)bp.ptr[o])[r];
                        break;
                    case PG_T_F64:
                        ((double*)build_outs.ptr[o])[pos] =
                            ((const double*)bp.ptr[o])[r];
                        break;
                    default:
                        ((uint8_t*)build_outs.ptr[o])[pos] =
                            bp.pack_bits && o == 0
                                ? (uint8_t)pv
                                : ((const uint8_t*)bp.ptr[o])[r];
                }
            }
            if constexpr (PROBE_OUTER) oo.pay_null[pos] = 0;
            /* lanes that matched the same build row all store 1: benign */
            if constexpr (MARK) oo.marks[r] = 1;
            pos++;
        }
        if constexpr (PROBE_OUTER) {
            if (sl < 0 && c) { /* no match: payloads are null, values 0 */
                d_emit_probe_cols<OUTER>(pg, plan, probe_outs, oo, i, pos);
                for (int o = 0; o < bp.n; o++) {
                    switch (bp.tag[o]) {
                        case PG_T_I32:
                            ((int32_t*)build_outs.ptr[o])[pos] = 0;
                            break;
                        case PG_T_I64:
                        case PG_T_F64:
                            ((int64_t*)build_outs.ptr[o])[pos] = 0;
                            break;
                        default:
                            ((uint8_t*)build_outs.ptr[o])[pos] = 0;
                    }
                }
                oo.pay_null[pos] = 1;
            }
        }
        __syncthreads();
        if (threadIdx.x == 0)
            running += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        __syncthreads();
    }
}

/* ------------------------------------------------------------------ */
/* Multi-key joins (pg_plan_hash_build.n_keys >= 1): JoinHash /          */
/* PagesHash over 1..4 hash channels (PagesHash.java:81-181).            */
/* The build rows keep their widened key vector row-major in key_rows    */
/* (n_keys int64 per row, written by k_mk_gather in add_input, immutable */
/* afterwards) plus one "any channel null" byte.  The table is one u64   */
/* word per slot, (hash >> 32) << 32 | representative build row, all     */
/* ones = empty (a row id is < 2^31, so no word collides with it).  A    */
/* claim is ONE CAS that installs the word; whoever meets an occupied    */
/* slot with the same 32 hash bits compares its key vector against       */
/* key_rows[rep], which an earlier launch wrote — so no thread ever      */
/* waits for another (no claim/publish state as in GROUPBY_MULTI).       */
/* Duplicates hang off the representative: next[i] =                     */
/* atomicExch(&next[rep], i) on a next[] preset to -1; next[rep] is only */
/* ever exchanged and next[i] of a duplicate only ever stored by i.      */
/* A probe miss costs one random line; key_rows is touched only when the */
/* 32 hash bits agree.  Hash = the group-by's: murmur3 finaliser over    */
/* the CombineHashFunction fold of the per-channel bigint hashes.        */
/* ------------------------------------------------------------------ */
#define MK_EMPTY 0xffffffffffffffffull

struct mk_keys {
    int32_t n;
    int32_t col[4];
};

/* the key vector of row i and its hash; false when a channel is null */
__device__ inline bool d_mk_load(const pg_page& pg, const mk_keys& mk,
                                 int64_t i, int64_t* k, uint64_t* h)
{
    uint64_t f = 0;
#pragma unroll
    for (int ch = 0; ch < 4; ch++) {
        if (ch >= mk.n) break;
        if (d_col_is_null(pg, mk.col[ch], i)) return false;
        k[ch] = d_load_i64(pg.cols[mk.col[ch]], i);
        f = 31u * f + pg_bigint_hash(k[ch]);
    }
    *h = pg_murmur3_finalize(f);
    return true;
}

__device__ inline bool d_mk_equal(const int64_t* kr, const int64_t* k, int n)
{
    bool eq = true;
#pragma unroll
    for (int ch = 0; ch < 4; ch++) {
        if (ch >= n) break;
        eq = eq && kr[ch] == k[ch];
    }
    return eq;
}

/* build add_input: widen the key channels of the selected rows (rowid =
 * their source row indexes, in build-row order) into key_rows / knull */
__global__ __launch_bounds__(256) void k_mk_gather(
    pg_page pg, mk_keys mk, const int64_t* rowid, int64_t n,
    int64_t* key_rows, uint8_t* knull)
{
    int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; j < n; j += stride) {
        const int64_t i = rowid[j];
        bool isnull = false;
#pragma unroll
        for (int ch = 0; ch < 4; ch++) {
            if (ch >= mk.n) break;
            const bool nl = d_col_is_null(pg, mk.col[ch], i);
            isnull = isnull || nl;
            /* the value under a null never matters: store 0 */
            key_rows[j * mk.n + ch] =
                nl ? 0 : d_load_i64(pg.cols[mk.col[ch]], i);
        }
        knull[j] = isnull ? 1 : 0;
    }
}

/* build finish: slots preset to MK_EMPTY, next[] to -1.  The probe walk is
 * bounded by the fill rule (cap >= 2n + 16); err counts rows that found no
 * slot all the same, which finish() turns into an error. */
__global__ __launch_bounds__(256) void k_mk_insert(
    const int64_t* key_rows, const uint8_t* knull, int64_t n, int32_t nk,
    unsigned long long* slots, int32_t* next, int64_t mask,
    unsigned long long* err)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        if (knull[i]) continue; /* kept as a build row, never matched */
        int64_t k[4];
        uint64_t f = 0;
#pragma unroll
        for (int ch = 0; ch < 4; ch++) {
            if (ch >= nk) break;
            k[ch] = key_rows[i * nk + ch];
            f = 31u * f + pg_bigint_hash(k[ch]);
        }
        const uint64_t h = pg_murmur3_finalize(f);
        const unsigned long long tag = h & 0xffffffff00000000ull;
        const unsigned long long mine = tag | (unsigned long long)i;
        int64_t s = (int64_t)(h & (uint64_t)mask);
        int64_t tries = 0;
        for (;;) {
            unsigned long long cur = __hip_atomic_load(
                &slots[s], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (cur == MK_EMPTY) {
                cur = atomicCAS(&slots[s], MK_EMPTY, mine);
                if (cur == MK_EMPTY) break; /* i represents its key */
            }
            if ((cur & 0xffffffff00000000ull) == tag) {
                const int64_t rep = (int64_t)(cur & 0xffffffffull);
                if (d_mk_equal(key_rows + rep * nk, k, nk)) {
                    next[i] = atomicExch(&next[rep], (int32_t)i);
                    break;
                }
            }
            s = (s + 1) & mask;
            if (++tries > mask) {
                atomicAdd(err, 1ull);
                break;
            }
        }
    }
}

/* the representative build row of key vector k, or -1 */
__device__ inline int64_t d_mk_find(const unsigned long long* slots,
                                    int64_t mask, const int64_t* key_rows,
                                    int32_t nk, const int64_t* k, uint64_t h)
{
    const unsigned long long tag = h & 0xffffffff00000000ull;
    int64_t s = (int64_t)(h & (uint64_t)mask);
    for (int64_t tries = 0; tries <= mask; tries++) {
        const unsigned long long cur = slots[s];
        if (cur == MK_EMPTY) return -1;
        if ((cur & 0xffffffff00000000ull) == tag) {
            const int64_t rep = (int64_t)(cur & 0xffffffffull);
            if (d_mk_equal(key_rows + rep * nk, k, nk)) return rep;
        }
        s = (s + 1) & mask;
    }
    return -1;
}

/* the probe passes: k_probe_count / k_probe_emit's geometry (per-block
 * counts, host scan, wave prefix), so the row order is mode 0's.  A null
 * in any key channel matches nothing in every mode, mode 0 included. */
template <bool PROBE_OUTER, bool MARK>
__global__ __launch_bounds__(256) void k_mk_probe_count(
    pg_page pg, pg_plan_lookup_join plan, const unsigned long long* slots,
    const int32_t* next, int64_t mask, const int64_t* key_rows,
    int64_t chunk, int64_t* block_counts)
{
    const int64_t n = pg.n_rows;
    const int64_t lo = (int64_t)blockIdx.x * chunk;
    const int64_t hi = min(lo + chunk, n);
    mk_keys mk;
    mk.n = plan.n_keys;
    for (int ch = 0; ch < 4; ch++) mk.col[ch] = plan.key_cols[ch];
    int64_t total = 0;
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
        if (!d_eval_preds(pg, plan.preds, plan.n_preds, i)) continue;
        int64_t k[4];
        uint64_t h;
        int64_t rep = -1;
        if (d_mk_load(pg, mk, i, k, &h))
            rep = d_mk_find(slots, mask, key_rows, mk.n, k, h);
        if (rep >= 0) {
            for (int32_t r = (int32_t)rep; r >= 0; r = next[r]) total++;
        } else if constexpr (PROBE_OUTER) {
            total++;
        }
    }
    total = d_bfly_i64(total);
    __shared__ int64_t lds[4];
    if ((threadIdx.x & 63) == 0) lds[threadIdx.x >> 6] = total;
    __syncthreads();
    if (threadIdx.x == 0)
        block_counts[blockIdx.x] = lds[0] + lds[1] + lds[2] + lds[3];
}

/* payload columns of output row pos: build row r's, or zeros (r < 0) */
__device__ inline void d_mk_emit_payloads(const build_payloads& bp,
                                          const emit_outs& build_outs,
                                          int64_t r, int64_t pos)
{
    for (int o = 0; o < bp.n; o++) {
        switch (bp.tag[o]) {
            case PG_T_I32:
                ((int32_t*)build_outs.ptr[o])[pos] =
                    r < 0 ? 0 : ((const int32_t*)bp.ptr[o])[r];
                break;
            case PG_T_I64:
            case PG_T_F64: /* bit copy */
                ((int64_t*)build_outs.ptr[o])[pos] =
                    r < 0 ? 0 : ((const int64_t*)bp.ptr[o])[r];
                break;
            default:
                ((uint8_t*)build_outs.ptr[o])[pos] =
                    r < 0 ? 0 : ((const uint8_t*)bp.ptr[o])[r];
        }
    }
}

template <bool PROBE_OUTER, bool MARK>
__global__ __launch_bounds__(256) void k_mk_probe_emit(
    pg_page pg, pg_plan_lookup_join plan, const unsigned long long* slots,
    const int32_t* next, int64_t mask, const int64_t* key_rows,
    int64_t chunk, const int64_t* block_offs, emit_outs probe_outs,
    build_payloads bp, emit_outs build_outs, outer_outs oo)
{
    constexpr bool OUTER = PROBE_OUTER || MARK;
    const int64_t n = pg.n_rows;
    const int64_t lo = (int64_t)blockIdx.x * chunk;
    const int64_t hi = min(lo + chunk, n);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    mk_keys mk;
    mk.n = plan.n_keys;
    for (int ch = 0; ch < 4; ch++) mk.col[ch] = plan.key_cols[ch];
    __shared__ int64_t wcnt[4];
    __shared__ int64_t running;
    if (threadIdx.x == 0) running = block_offs[blockIdx.x];
    __syncthreads();
    for (int64_t base = lo; base < hi; base += 256) {
        int64_t i = base + 64 * wid + lane;
        int64_t rep = -1;
        int32_t c = 0;
        if (i < hi && d_eval_preds(pg, plan.preds, plan.n_preds, i)) {
            int64_t k[4];
            uint64_t h;
            if (d_mk_load(pg, mk, i, k, &h))
                rep = d_mk_find(slots, mask, key_rows, mk.n, k, h);
            if (rep >= 0) {
                for (int32_t r = (int32_t)rep; r >= 0; r = next[r]) c++;
            } else if constexpr (PROBE_OUTER) {
                c = 1; /* the null-padded row */
            }
        }
        /* wave inclusive prefix of counts (stable row order) */
        int64_t pre = c;
        for (int d = 1; d < 64; d <<= 1) {
            int64_t t = __shfl_up((long long)pre, d, 64);
            if (lane >= d) pre += t;
        }
        int64_t wtotal = __shfl((long long)pre, 63, 64);
        int64_t excl = pre - c;
        if (lane == 0) wcnt[wid] = wtotal;
        __syncthreads();
        int64_t woff = running;
        for (int w = 0; w < wid; w++) woff += wcnt[w];
        int64_t pos = woff + excl;
        for (int32_t r = (int32_t)rep; r >= 0; r = next[r]) {
            d_emit_probe_cols<OUTER>(pg, plan, probe_outs, oo, i, pos);
            d_mk_emit_payloads(bp, build_outs, r, pos);
            if constexpr (PROBE_OUTER) oo.pay_null[pos] = 0;
            /* lanes that matched the same build row all store 1: benign */
            if constexpr (MARK) oo.marks[r] = 1;
            pos++;
        }
        if constexpr (PROBE_OUTER) {
            if (rep < 0 && c) { /* no match: payloads are null, values 0 */
                d_emit_probe_cols<OUTER>(pg, plan, probe_outs, oo, i, pos);
                d_mk_emit_payloads(bp, build_outs, -1, pos);
                oo.pay_null[pos] = 1;
            }
        }
        __syncthreads();
        if (threadIdx.x == 0)
            running += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        __syncthreads();
    }
}

/* mode 2: fused probe + dense-dictionary lookup + equality + small-key
 * grouped SUM — the Q5 local-supplier specialization (see presto_gpu.h).
 * Deterministic: exact ticks (order-independent) + fx128 for f64; groups
 * accumulate in per-thread registers then wave butterfly + global atomics
 * on ticks (exact). */
template <int MAXG>
__global__ __launch_bounds__(256) void k_probe_agg_fused2(
    pg_page pg, pg_plan_lookup_join plan, const int64_t* keys,
    int64_t lmask_in, int32_t pbits,
    const uint8_t* tags, int64_t mask, const uint8_t* slot_payload_u8,
    const uint8_t* dense_vals, int64_t dense_n,
    unsigned long long* out_dec /* [MAXG] */,
    unsigned long long* out_flo, unsigned long long* out_fhi,
    unsigned long long* out_cnt)
{
    int64_t acc[MAXG];
    uint64_t fhi[MAXG], flo[MAXG];
    int32_t cnt[MAXG];
#pragma unroll
    for (int g = 0; g < MAXG; g++) {
        acc[g] = 0;
        fhi[g] = 0;
        flo[g] = 0;
        cnt[g] = 0;
    }
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < pg.n_rows; i += stride) {
        if (!d_eval_preds(pg, plan.preds, plan.n_preds, i)) continue;
        int64_t key = d_load_i64(pg.cols[plan.key_col], i);
        int64_t sl = d_tbl_find_tagged(keys, tags, mask, lmask_in, pbits,
                                       key);
        if (sl < 0) continue;
        uint8_t g1 = pbits ? (uint8_t)(keys[sl] & ((1ll << pbits) - 1))
                           : slot_payload_u8[sl];
        int64_t k2 = d_load_i64(pg.cols[plan.table2_key_col], i);
        if (k2 < 1 || k2 > dense_n) continue;
        uint8_t g2 = dense_vals[k2 - 1];
        if (g1 != g2) continue;
        int gi = -1;
#pragma unroll
        for (int g = 0; g < MAXG; g++)
            if (g < plan.n_group_vals && plan.group_vals[g] == g2 && gi < 0)
                gi = g;
        if (gi < 0) continue;
        pg_agg ag;
        ag.proj = plan.proj;
        ag.dec_scale = plan.dec_scale;
        int64_t ticks = d_eval_proj_dec(pg, ag, i);
        double p = d_eval_proj_f64(pg, plan.proj, i);
        uint64_t phi, plo;
        fx128_from_f64(p, &phi, &plo);
#pragma unroll
        for (int g = 0; g < MAXG; g++) {
            bool m = g == gi;
            if (__builtin_add_overflow(acc[g], m ? ticks : 0, &acc[g]))
                atomicAdd(out_cnt + MAXG, 1ull); /* ovf slot */
            cnt[g] += m ? 1 : 0;
            uint64_t nlo = flo[g] + (m ? plo : 0);
            fhi[g] += (m ? phi : 0) + (nlo < flo[g] ? 1u : 0u);
            flo[g] = nlo;
        }
    }
    /* wave reduce ticks/count (exact; a wave total that leaves int64 bumps
     * the overflow slot like the per-thread add and the atomic do), then
     * one atomic per wave; the fx128 halves go through carry-aware atomics
     * per lane (exact, order-independent) */
#pragma unroll
    for (int g = 0; g < MAXG; g++) {
        bool wrapped;
        int64_t a = d_bfly_i64_ck(acc[g], &wrapped);
        int64_t c = d_bfly_i64((int64_t)cnt[g]);
        if ((threadIdx.x & 63) == 0) {
            if (wrapped) atomicAdd(out_cnt + MAXG, 1ull); /* ovf slot */
            else if (a) d_atomic_add_dec_ck(&out_dec[g], a, out_cnt + MAXG);
            if (c) atomicAdd(&out_cnt[g], (unsigned long long)c);
        }
        if (flo[g] | fhi[g]) {
            unsigned long long old = atomicAdd(&out_flo[g], flo[g]);
            atomicAdd(&out_fhi[g],
                      fhi[g] + (old > ~flo[g] ? 1ull : 0ull));
        }
    }
}

/* specialized mode-2 probe for the Q5 local-supplier shape (the
 * codegen-analog of k_agg_q1/k_probe_agg_q3): PACKED orders table
 * (slot = orderkey << pbits | cust_nation), dense suppkey->nation
 * payload, no predicates, DISC_PRICE over two f64 columns.  Two rows
 * per thread with nontemporal vector key loads; ep/dc are loaded only
 * for local-supplier matches (~0.6% of rows at SF100); per-thread
 * register group accumulators, wave butterfly, one atomic per group per
 * wave (exact ticks + exact fx128 — deterministic). */
template <int MAXG>
__global__ __launch_bounds__(256) void k_probe_agg_q5(
    pg_plan_lookup_join plan, const int64_t* okey, const int64_t* skey,
    const double* ep, const double* dc, int64_t n, const int64_t* keys,
    const uint8_t* tags, int64_t mask, int64_t lmask, int32_t pbits,
    const unsigned long long* kbits, int64_t bmax,
    const uint8_t* dense_vals, int64_t dense_n,
    unsigned long long* out_dec, unsigned long long* out_flo,
    unsigned long long* out_fhi, unsigned long long* out_cnt)
{
    typedef long vl2 __attribute__((ext_vector_type(2)));
    const int64_t pmask = (1ll << pbits) - 1;
    int64_t acc[MAXG];
    uint64_t fhi[MAXG], flo[MAXG];
    int32_t cnt[MAXG];
#pragma unroll
    for (int g = 0; g < MAXG; g++) {
        acc[g] = 0;
        fhi[g] = 0;
        flo[g] = 0;
        cnt[g] = 0;
    }
    int64_t base0 = 2 * ((int64_t)blockIdx.x * blockDim.x + threadIdx.x);
    int64_t stride = 2 * (int64_t)gridDim.x * blockDim.x;
    for (int64_t base = base0; base < n; base += stride) {
        int64_t k[2], sk[2];
        bool sel[2];
        if (base + 2 <= n) {
            vl2 ka = __builtin_nontemporal_load((const vl2*)(okey + base));
            vl2 kb = __builtin_nontemporal_load((const vl2*)(skey + base));
            k[0] = ka[0]; k[1] = ka[1];
            sk[0] = kb[0]; sk[1] = kb[1];
            sel[0] = sel[1] = true;
        } else {
#pragma unroll
            for (int j = 0; j < 2; j++) {
                sel[j] = base + j < n;
                k[j] = sel[j] ? okey[base + j] : 0;
                sk[j] = sel[j] ? skey[base + j] : 0;
            }
        }
#pragma unroll
        for (int j = 0; j < 2; j++) {
            if (!sel[j]) continue;
            if (kbits && !d_kbit_test(kbits, bmax, k[j])) continue;
            int64_t slot = -1;
            uint64_t h = pg_murmur3_finalize(pg_bigint_hash(k[j]));
            int64_t p = (int64_t)(h & (uint64_t)mask);
            uint8_t tg = tags ? d_tbl_tag(h) : 0;
            for (;;) {
                if (tags) {
                    uint8_t t = tags[p];
                    if (t == 0) break;
                    if (t == tg && (keys[p] >> pbits) == k[j]) {
                        slot = p;
                        break;
                    }
                } else {
                    int64_t kw = keys[p];
                    if (kw == TBL_EMPTY) break;
                    if ((kw >> pbits) == k[j]) { slot = p; break; }
                }
                p = d_probe_next(p, lmask);
            }
            if (slot < 0) continue;
            uint8_t g1 = (uint8_t)(keys[slot] & pmask);
            if (sk[j] < 1 || sk[j] > dense_n) continue;
            uint8_t g2 = dense_vals[sk[j] - 1];
            if (g1 != g2) continue;
            int gi = -1;
#pragma unroll
            for (int g = 0; g < MAXG; g++)
                if (g < plan.n_group_vals && plan.group_vals[g] == g2 &&
                    gi < 0)
                    gi = g;
            if (gi < 0) continue;
            double e = ep[base + j], d = dc[base + j];
            int64_t cents = (int64_t)(e * 100.0 + 0.5);
            int64_t di = (int64_t)(d * 100.0 + 0.5);
            int64_t ticks = cents * (100 - di);
            double pr = e * (1.0 - d);
            uint64_t phi, plo;
            fx128_from_f64(pr, &phi, &plo);
#pragma unroll
            for (int g = 0; g < MAXG; g++) {
                bool m = g == gi;
                acc[g] += m ? ticks : 0;
                cnt[g] += m ? 1 : 0;
                uint64_t nlo = flo[g] + (m ? plo : 0);
                fhi[g] += (m ? phi : 0) + (nlo < flo[g] ? 1u : 0u);
                flo[g] = nlo;
            }
        }
    }
#pragma unroll
    for (int g = 0; g < MAXG; g++) {
        bool wrapped;
        int64_t a = d_bfly_i64_ck(acc[g], &wrapped);
        int64_t c = d_bfly_i64((int64_t)cnt[g]);
        if ((threadIdx.x & 63) == 0) {
            if (wrapped) atomicAdd(out_cnt + MAXG, 1ull); /* ovf slot */
            else if (a) d_atomic_add_dec_ck(&out_dec[g], a, out_cnt + MAXG);
            if (c) atomicAdd(&out_cnt[g], (unsigned long long)c);
        }
        if (flo[g] | fhi[g]) {
            unsigned long long old = atomicAdd(&out_flo[g], flo[g]);
            atomicAdd(&out_fhi[g],
                      fhi[g] + (old > ~flo[g] ? 1ull : 0ull));
        }
    }
}

/* MULTI-ACCUMULATOR fused-agg probe (mode 1 with n_aggs > 0): the full
 * InMemoryHashAggregationBuilder.processPage:204 analog — ONE getGroupIds
 * probe per row, then every aggregator accumulates, each optionally
 * gated by its own FILTER predicate (AggregationNode masks).  Per-slot
 * state: n_aggs overflow-checked int64 tick sums + the match count. */
__global__ __launch_bounds__(256) void k_probe_agg_multi(
    pg_page pg, pg_plan_lookup_join plan, const int64_t* keys,
    const uint8_t* tags, int64_t mask, int64_t lmask, int32_t pbits,
    const unsigned long long* kbits, int64_t bmax,
    unsigned long long* acc, unsigned long long* ovf)
{
    const int n_aggs = plan.n_aggs;
    /* packed layout: word 0 carries the bit-field aggs + count, own-word
     * aggs follow in agg order (plan.acc_pack; see presto_gpu.h) */
    int64_t stride_w = n_aggs + 1;
    if (plan.acc_pack) {
        stride_w = 1;
        for (int a = 0; a < n_aggs; a++)
            if (plan.acc_pack_shift[a] < 0) stride_w++;
    }
    /* consecutive-row run dedup, as in k_probe_agg: one probe and one
     * set of atomics per run of equal keys */
    const int C = 4;
    int64_t base =
        ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) * C;
    const int64_t stride = (int64_t)gridDim.x * blockDim.x * C;
    for (; base < pg.n_rows; base += stride) {
        const int64_t lim = base + C < pg.n_rows ? base + C : pg.n_rows;
        int64_t cur_key = 0, cur_slot = -2;
        int64_t run[6];
        int run_cnt = 0;
        auto flush = [&]() {
            if (cur_slot < 0 || run_cnt == 0) return;
            unsigned long long* slot = acc + (size_t)cur_slot * stride_w;
            if (plan.acc_pack) {
                unsigned long long w0 =
                    (unsigned long long)run_cnt
                    << plan.acc_pack_cnt_shift;
                unsigned long long bad =
                    (unsigned long long)run_cnt >>
                    plan.acc_pack_cnt_width;
                int w = 1;
#pragma unroll
                for (int a = 0; a < 6; a++) {
                    if (a >= n_aggs) break;
                    if (plan.acc_pack_shift[a] >= 0) {
                        /* negative contributions wrap the uint64 and
                         * trip the width check -> loud overflow */
                        bad |= (unsigned long long)run[a] >>
                               plan.acc_pack_width[a];
                        w0 += (unsigned long long)run[a]
                              << plan.acc_pack_shift[a];
                    } else {
                        if (run[a])
                            d_atomic_add_dec_ck(slot + w, run[a], ovf);
                        w++;
                    }
                }
                atomicAdd(&slot[0], w0);
                if (bad && ovf) atomicAdd(ovf, 1ull);
            } else {
#pragma unroll
                for (int a = 0; a < 6; a++) {
                    if (a >= n_aggs) break;
                    if (run[a]) d_atomic_add_dec_ck(slot + a, run[a], ovf);
                }
                atomicAdd(slot + n_aggs, (unsigned long long)run_cnt);
            }
        };
        for (int64_t i = base; i < lim; i++) {
            if (!d_eval_preds(pg, plan.preds, plan.n_preds, i)) continue;
            int64_t key = d_load_i64(pg.cols[plan.key_col], i);
            if (cur_slot == -2 || key != cur_key) {
                flush();
                cur_key = key;
                if (!keys) { /* range-group: acc index = key-1, taken
                                unsigned so that INT64_MIN is a miss and
                                not a signed overflow */
                    const uint64_t s = (uint64_t)key - 1;
                    cur_slot = s <= (uint64_t)mask ? (int64_t)s : -1;
                } else
                    cur_slot = kbits && !d_kbit_test(kbits, bmax, key)
                                   ? -1
                                   : d_tbl_find_tagged(keys, tags, mask,
                                                       lmask, pbits, key);
#pragma unroll
                for (int a = 0; a < 6; a++) run[a] = 0;
                run_cnt = 0;
            }
            if (cur_slot < 0) continue;
#pragma unroll
            for (int a = 0; a < 6; a++) {
                if (a >= n_aggs) break;
                int f = plan.agg_filter[a];
                if (f >= 0 && !d_eval_preds(pg, &plan.preds[f], 1, i))
                    continue;
                int64_t ticks = plan.aggs[a].func == PG_AGG_COUNT
                                    ? 1
                                    : d_eval_proj_dec(pg, plan.aggs[a],
                                                      i);
                if (__builtin_add_overflow(run[a], ticks, &run[a]))
                    if (ovf) atomicAdd(ovf, 1ull);
            }
            run_cnt++;
        }
        flush();
    }
}

/* group extraction for the multi-accumulator layout: key (+payloads),
 * then the n_aggs tick sums and the count, slot-ascending */
struct acc_pack_desc {
    int32_t on;        /* 0 = unpacked (cnt at word n_aggs) */
    int32_t shift[6];  /* bit offset in word0, or -1 = own word */
    int32_t width[6];
    int32_t cnt_shift, cnt_width;
};
__device__ inline int64_t d_acc_field(const unsigned long long* slot,
                                      const acc_pack_desc& pk, int a)
{
    if (pk.shift[a] >= 0)
        return (int64_t)((slot[0] >> pk.shift[a]) &
                         ((1ull << pk.width[a]) - 1));
    int w = 1;
    for (int b = 0; b < a; b++)
        if (pk.shift[b] < 0) w++;
    return (int64_t)slot[w];
}
__global__ __launch_bounds__(256) void k_groups_emit_multi(
    const int64_t* keys, const unsigned long long* acc, int64_t stride_w,
    int32_t n_aggs, build_payloads bp, int64_t cap, int64_t chunk,
    unsigned long long* cursor, int64_t* out_key, emit_outs payload_outs,
    emit_outs agg_outs, acc_pack_desc pk)
{
    auto slot_cnt = [&](int64_t i) -> unsigned long long {
        const unsigned long long* sl = acc + i * stride_w;
        return pk.on ? (sl[0] >> pk.cnt_shift) &
                           ((1ull << pk.cnt_width) - 1)
                     : sl[n_aggs];
    };
    const int64_t lo = (int64_t)blockIdx.x * chunk;
    const int64_t hi = min(lo + chunk, cap);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    __shared__ int64_t wcnt[4];
    __shared__ int64_t running;
    {
        int64_t mycnt = 0;
        for (int64_t i = lo + threadIdx.x; i < hi; i += 256)
            mycnt += slot_cnt(i) > 0;
        mycnt = d_bfly_i64(mycnt);
        if (lane == 0) wcnt[wid] = mycnt;
        __syncthreads();
        if (threadIdx.x == 0) {
            int64_t t = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
            running = t ? (int64_t)atomicAdd(cursor,
                                             (unsigned long long)t)
                        : 0;
        }
    }
    __syncthreads();
    for (int64_t base = lo; base < hi; base += 256) {
        int64_t i = base + 64 * wid + lane;
        bool sel = i < hi && slot_cnt(i) > 0;
        uint64_t m = d_ballot(sel);
        int wsum = __popcll(m);
        if (lane == 0) wcnt[wid] = wsum;
        __syncthreads();
        int64_t woff = running;
        for (int w = 0; w < wid; w++) woff += wcnt[w];
        if (sel) {
            int64_t pos = woff + __popcll(m & ((1ull << lane) - 1));
            /* range-group tables store no keys: the slot index IS key-1 */
            int64_t kw = keys ? keys[i] : i + 1;
            out_key[pos] = bp.pack_bits ? (kw >> bp.pack_bits) : kw;
            for (int o = 0; o < bp.n; o++) {
                int64_t pv = bp.pack_bits && o == 0
                                 ? (kw & ((1ll << bp.pack_bits) - 1))
                                 : 0;
                switch (bp.tag[o]) {
                    case PG_T_U8:
                        ((uint8_t*)payload_outs.ptr[o])[pos] =
                            bp.pack_bits && o == 0
                                ? (uint8_t)pv
                                : ((const uint8_t*)bp.ptr[o])[i];
                        break;
                    case PG_T_I32:
                        ((int32_t*)payload_outs.ptr[o])[pos] =
                            bp.pack_bits && o == 0
                                ? (int32_t)pv
                                : ((const int32_t*)bp.ptr[o])[i];
                        break;
                    case PG_T_I64:
                        ((int64_t*)payload_outs.ptr[o])[pos] =
                            bp.pack_bits && o == 0
                                ? pv
                                : ((const int64_t*)bp.ptr[o])[i];
                        break;
                    default:
                        ((double*)payload_outs.ptr[o])[pos] =
                            ((const double*)bp.ptr[o])[i];
                }
            }
            if (pk.on) {
                const unsigned long long* sl = acc + i * stride_w;
                for (int a = 0; a < n_aggs; a++)
                    ((int64_t*)agg_outs.ptr[a])[pos] =
                        d_acc_field(sl, pk, a);
                ((int64_t*)agg_outs.ptr[n_aggs])[pos] =
                    (int64_t)slot_cnt(i);
            } else {
                for (int a = 0; a <= n_aggs; a++)
                    ((int64_t*)agg_outs.ptr[a])[pos] =
                        (int64_t)acc[i * stride_w + a];
            }
        }
        __syncthreads();
        if (threadIdx.x == 0)
            running += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        __syncthreads();
    }
}

/* ------------------------------------------------------------------ */
/* GROUPBY_MULTI: general multi-channel grouped aggregation            */
/* (MultiChannelGroupByHash.java:300-380 + InMemoryHashAggregation-    */
/*  Builder.processPage:204).  Group hash = murmur3 finalizer over the */
/* CombineHashFunction fold (31*h + bigint_hash per channel,           */
/* CombineHashFunction.java:28-30); open-address linear probe.        */
/* Multi-word keys are EXACT: a per-slot state word is CAS-claimed     */
/* (0->1), the claimer publishes the key words with system-scope       */
/* stores + vmcnt drain + a state=2 flag (the MI355X_MICROARCH.md      */
/* "sc1 payload -> vmcnt(0) -> sc1 flag" handoff form, so readers      */
/* need no acquire fences), and losers compare the full key vector —  */
/* never a fingerprint approximation.                                  */
/* SQL_NULLS (pg_plan_groupby.sql_nulls = 1) instantiates the null-     */
/* aware variant: the key vector grows by one word of per-channel null  */
/* bits (kv plane n_keys, published and compared like the key words;    */
/* key words under a null are 0 and fold NULL_HASH_CODE = 0), and each  */
/* slot carries one word of "aggregate a received input" bits in front  */
/* of the row count.  SQL_NULLS = false compiles all of that out.       */
/* ------------------------------------------------------------------ */
struct gb_agg_off {
    int32_t off[6];
};

__device__ inline int64_t d_gb_key(const pg_page& pg, int32_t col,
                                   int64_t i)
{
    const pg_col& c = pg.cols[col];
    if (c.tag == PG_T_VARBIN)
        return (int64_t)c.dict_ids[i]; /* DictionaryBlock id identity */
    return d_load_i64(c, i);
}

template <bool SQL_NULLS>
__global__ __launch_bounds__(256) void k_groupby_multi(
    pg_page pg, pg_plan_groupby plan, unsigned int* state, int64_t* kv,
    int64_t cap, int64_t mask, unsigned long long* acc, int32_t acc_words,
    gb_agg_off offs,
    unsigned long long* counters /* [ovf, full, groups, SUM_F64 domain] */)
{
    const int n_keys = plan.n_keys;
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < pg.n_rows; i += stride) {
        if (!d_eval_preds(pg, plan.preds, plan.n_preds, i)) continue;
        int64_t k[4];
        int64_t knull = 0; /* SQL_NULLS: bit ch = channel ch is null */
        uint64_t h = 0;
#pragma unroll
        for (int ch = 0; ch < 4; ch++) {
            if (ch >= n_keys) break;
            if constexpr (SQL_NULLS) {
                if (d_col_is_null(pg, plan.key_col[ch], i)) {
                    k[ch] = 0; /* the stored value never groups */
                    knull |= (int64_t)1 << ch;
                    h = 31u * h; /* NULL_HASH_CODE = 0 */
                    continue;
                }
            }
            k[ch] = d_gb_key(pg, plan.key_col[ch], i);
            h = 31u * h + pg_bigint_hash(k[ch]);
        }
        int64_t pos = (int64_t)(pg_murmur3_finalize(h) & (uint64_t)mask);
        int64_t slot = -1, tries = 0;
        for (;;) {
            unsigned int st = __hip_atomic_load(
                &state[pos], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (st == 2u) {
                bool eq = true;
#pragma unroll
                for (int ch = 0; ch < 4; ch++) {
                    if (ch >= n_keys) break;
                    eq = eq && __hip_atomic_load(
                                   &kv[(size_t)ch * cap + pos],
                                   __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_SYSTEM) == k[ch];
                }
                if constexpr (SQL_NULLS)
                    eq = eq && __hip_atomic_load(
                                   &kv[(size_t)n_keys * cap + pos],
                                   __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_SYSTEM) == knull;
                if (eq) {
                    slot = pos;
                    break;
                }
                pos = (pos + 1) & mask;
                if (++tries > mask) {
                    atomicAdd(counters + 1, 1ull);
                    break;
                }
            } else if (st == 0u) {
                unsigned int prev = atomicCAS(&state[pos], 0u, 1u);
                if (prev == 0u) {
#pragma unroll
                    for (int ch = 0; ch < 4; ch++) {
                        if (ch >= n_keys) break;
                        __hip_atomic_store(&kv[(size_t)ch * cap + pos],
                                           k[ch], __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_SYSTEM);
                    }
                    if constexpr (SQL_NULLS)
                        __hip_atomic_store(&kv[(size_t)n_keys * cap + pos],
                                           knull, __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_SYSTEM);
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    __hip_atomic_store(&state[pos], 2u, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_SYSTEM);
                    atomicAdd(counters + 2, 1ull); /* distinct groups */
                    slot = pos;
                    break;
                }
                /* lost the claim: retry the same position */
            }
            /* st == 1: publisher in flight — retry (it completes within
             * its own branch, so intra-wave divergence cannot deadlock
             * this loop) */
        }
        if (slot < 0) continue;
        unsigned long long* s = acc + (size_t)slot * acc_words;
        unsigned long long got = 0; /* SQL_NULLS: aggregates fed by row i */
#pragma unroll
        for (int a = 0; a < 6; a++) {
            if (a >= plan.n_aggs) break;
            int f = plan.agg_filter[a];
            if (f >= 0 && !d_eval_preds(pg, &plan.preds[f], 1, i))
                continue;
            unsigned long long* w = s + offs.off[a];
            if constexpr (SQL_NULLS) {
                /* COUNT is count(*): its proj is never read.  A null
                 * input is skipped before it is evaluated. */
                if (plan.aggs[a].func != PG_AGG_COUNT) {
                    if (d_proj_is_null(pg, plan.aggs[a].proj, i)) continue;
                    got |= 1ull << a;
                }
            }
            switch (plan.aggs[a].func) {
                case PG_AGG_COUNT:
                    atomicAdd(w, 1ull);
                    break;
                case PG_AGG_SUM_F64: {
                    double v = d_eval_proj_f64(pg, plan.aggs[a].proj, i);
                    uint64_t phi, plo;
                    d_fx128_from_f64_ck(v, &phi, &plo, counters + 3);
                    unsigned long long old = atomicAdd(w, plo);
                    atomicAdd(w + 1, phi + (old > ~plo ? 1ull : 0ull));
                    break;
                }
                case PG_AGG_MIN:
                    atomicMin((long long*)w,
                              (long long)d_eval_proj_dec(pg, plan.aggs[a],
                                                         i));
                    break;
                case PG_AGG_MAX:
                    atomicMax((long long*)w,
                              (long long)d_eval_proj_dec(pg, plan.aggs[a],
                                                         i));
                    break;
                default: { /* SUM_DEC / SUM_I64: checked tick sums */
                    int64_t ticks = d_eval_proj_dec(pg, plan.aggs[a], i);
                    if (ticks) d_atomic_add_dec_ck(w, ticks, counters);
                }
            }
        }
        if constexpr (SQL_NULLS) {
            /* "received input" bits, word acc_words - 2.  They only go
             * 0 -> 1, so a relaxed load that already shows them set makes
             * the atomic redundant (the steady state of a group). */
            unsigned long long* gw = s + acc_words - 2;
            if (got &&
                (__hip_atomic_load(gw, __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_AGENT) & got) != got)
                atomicOr(gw, got);
        }
        atomicAdd(s + acc_words - 1, 1ull);
    }
}

/* MIN/MAX identity init for the groupby accumulator words */
__global__ __launch_bounds__(256) void k_gb_acc_init(
    unsigned long long* acc, int64_t cap, int32_t acc_words,
    gb_agg_off offs, pg_plan_groupby plan)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < cap; i += stride) {
        unsigned long long* s = acc + (size_t)i * acc_words;
#pragma unroll
        for (int a = 0; a < 6; a++) {
            if (a >= plan.n_aggs) break;
            if (plan.aggs[a].func == PG_AGG_MIN)
                s[offs.off[a]] = (unsigned long long)INT64_MAX;
            else if (plan.aggs[a].func == PG_AGG_MAX)
                s[offs.off[a]] = (unsigned long long)INT64_MIN;
        }
    }
}

/* groupby extraction: occupied slots (cnt>0) slot-ascending; keys
 * re-narrowed to their input tags, aggregate columns per layout.
 * SQL_NULLS also writes the masks: key_masks.ptr[ch] from the null-bits
 * plane, agg_masks.ptr[a] (SUM / MIN / MAX; NULL for COUNT) from the
 * "received input" bits, and 0 for every value under a null. */
template <bool SQL_NULLS>
__global__ __launch_bounds__(256) void k_groupby_emit(
    const int64_t* kv, int64_t cap, int32_t n_keys,
    const unsigned long long* acc, int32_t acc_words, gb_agg_off offs,
    pg_plan_groupby plan, int64_t chunk, unsigned long long* cursor,
    emit_outs key_outs, emit_outs agg_outs, emit_outs key_masks,
    emit_outs agg_masks)
{
    const int64_t lo = (int64_t)blockIdx.x * chunk;
    const int64_t hi = min(lo + chunk, cap);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    __shared__ int64_t wcnt[4];
    __shared__ int64_t running;
    {
        int64_t mycnt = 0;
        for (int64_t i = lo + threadIdx.x; i < hi; i += 256)
            mycnt += acc[i * acc_words + acc_words - 1] > 0;
        mycnt = d_bfly_i64(mycnt);
        if (lane == 0) wcnt[wid] = mycnt;
        __syncthreads();
        if (threadIdx.x == 0) {
            int64_t t = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
            running = t ? (int64_t)atomicAdd(cursor,
                                             (unsigned long long)t)
                        : 0;
        }
    }
    __syncthreads();
    for (int64_t base = lo; base < hi; base += 256) {
        int64_t i = base + 64 * wid + lane;
        bool sel = i < hi && acc[i * acc_words + acc_words - 1] > 0;
        uint64_t m = d_ballot(sel);
        int wsum = __popcll(m);
        if (lane == 0) wcnt[wid] = wsum;
        __syncthreads();
        int64_t woff = running;
        for (int w = 0; w < wid; w++) woff += wcnt[w];
        if (sel) {
            int64_t pos = woff + __popcll(m & ((1ull << lane) - 1));
            for (int ch = 0; ch < n_keys; ch++) {
                int64_t kvv = kv[(size_t)ch * cap + i];
                switch (key_outs.tag[ch]) {
                    case PG_T_U8:
                        ((uint8_t*)key_outs.ptr[ch])[pos] = (uint8_t)kvv;
                        break;
                    case PG_T_I32:
                        ((int32_t*)key_outs.ptr[ch])[pos] = (int32_t)kvv;
                        break;
                    default:
                        ((int64_t*)key_outs.ptr[ch])[pos] = kvv;
                }
            }
            const unsigned long long* s = acc + (size_t)i * acc_words;
            if constexpr (SQL_NULLS) {
                /* key words under a null were stored as 0 */
                const int64_t knull = kv[(size_t)n_keys * cap + i];
                for (int ch = 0; ch < n_keys; ch++)
                    ((uint8_t*)key_masks.ptr[ch])[pos] =
                        (uint8_t)((knull >> ch) & 1);
            }
            for (int a = 0; a < plan.n_aggs; a++) {
                if constexpr (SQL_NULLS) {
                    if (plan.aggs[a].func != PG_AGG_COUNT) {
                        const bool isnull =
                            !((s[acc_words - 2] >> a) & 1ull);
                        ((uint8_t*)agg_masks.ptr[a])[pos] = isnull;
                        if (isnull) { /* not the MIN/MAX identity */
                            ((int64_t*)agg_outs.ptr[a])[pos] = 0;
                            continue;
                        }
                    }
                }
                if (plan.aggs[a].func == PG_AGG_SUM_F64)
                    ((double*)agg_outs.ptr[a])[pos] =
                        fx128_to_f64(s[offs.off[a] + 1], s[offs.off[a]]);
                else
                    ((int64_t*)agg_outs.ptr[a])[pos] =
                        (int64_t)s[offs.off[a]];
            }
            ((int64_t*)agg_outs.ptr[plan.n_aggs])[pos] =
                (int64_t)s[acc_words - 1];
        }
        __syncthreads();
        if (threadIdx.x == 0)
            running += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        __syncthreads();
    }
}

/* extract group rows after fused probe-agg: slots with count>0, emitted
 * slot-ascending (stable compaction over the slot array) */
__global__ __launch_bounds__(256) void k_groups_count(
    const unsigned long long* acc, int64_t stride_w, int64_t cnt_off,
    int32_t cnt_shift, unsigned long long cnt_mask,
    int64_t cap, int64_t chunk, int64_t* block_counts)
{
    const int64_t lo = (int64_t)blockIdx.x * chunk;
    const int64_t hi = min(lo + chunk, cap);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int64_t cnt = 0;
    for (int64_t base = lo + 64 * wid; base < hi; base += 256) {
        int64_t i = base + lane;
        bool sel = i < hi &&
                   ((acc[i * stride_w + cnt_off] >> cnt_shift) &
                    cnt_mask) > 0;
        uint64_t m = d_ballot(sel);
        if (lane == 0) cnt += __popcll(m);
    }
    __shared__ int64_t lds[4];
    if (lane == 0) lds[wid] = cnt;
    __syncthreads();
    if (threadIdx.x == 0)
        block_counts[blockIdx.x] = lds[0] + lds[1] + lds[2] + lds[3];
}

/* one group row: key, payloads and accumulator words of slot i written to
 * output row pos (shared by the scan and the hit-list extraction) */
__device__ inline void d_group_row(
    const int64_t* keys, const int32_t* head,
    const unsigned long long* acc, int32_t aw, const build_payloads& bp,
    int64_t i, int64_t pos, int64_t* out_key, const emit_outs& payload_outs,
    int64_t* out_dec, double* out_f64, int64_t* out_cnt)
{
    /* range-group tables store no keys: the slot index IS key-1 */
    int64_t kw = keys ? keys[i] : i + 1;
    out_key[pos] = bp.pack_bits ? (kw >> bp.pack_bits) : kw;
    int64_t r = bp.by_slot ? i : (int64_t)head[i];
    for (int o = 0; o < bp.n; o++) {
        int64_t pv = bp.pack_bits && o == 0
                         ? (kw & ((1ll << bp.pack_bits) - 1))
                         : 0;
        switch (bp.tag[o]) {
            case PG_T_U8:
                ((uint8_t*)payload_outs.ptr[o])[pos] =
                    bp.pack_bits && o == 0
                        ? (uint8_t)pv
                        : ((const uint8_t*)bp.ptr[o])[r];
                break;
            case PG_T_I32:
                ((int32_t*)payload_outs.ptr[o])[pos] =
                    bp.pack_bits && o == 0
                        ? (int32_t)pv
                        : ((const int32_t*)bp.ptr[o])[r];
                break;
            case PG_T_I64:
                ((int64_t*)payload_outs.ptr[o])[pos] =
                    bp.pack_bits && o == 0
                        ? pv
                        : ((const int64_t*)bp.ptr[o])[r];
                break;
            default:
                ((double*)payload_outs.ptr[o])[pos] =
                    ((const double*)bp.ptr[o])[r];
        }
    }
    const unsigned long long* s = acc + (size_t)i * aw;
    out_dec[pos] = (int64_t)s[0];
    out_f64[pos] = aw == 4 ? fx128_to_f64(s[2], s[1]) : 0.0;
    out_cnt[pos] = (int64_t)s[aw - 1];
}

/* ONE pass per block: count the block's chunk (first sweep, lines land
 * in L2), reserve a contiguous span with one atomicAdd, then emit into
 * it (second sweep hits L2).  Group output order is block-interleaved —
 * result-set semantics, like the reference's parallel drivers; every
 * consumer (TopN, joins, host folds) is order-free. */
__global__ __launch_bounds__(256) void k_groups_emit(
    const int64_t* keys, const int32_t* head,
    const unsigned long long* acc, int32_t aw, build_payloads bp,
    int64_t cap, int64_t chunk, unsigned long long* cursor,
    int64_t* out_key, emit_outs payload_outs, int64_t* out_dec,
    double* out_f64, int64_t* out_cnt)
{
    const int64_t lo = (int64_t)blockIdx.x * chunk;
    const int64_t hi = min(lo + chunk, cap);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    __shared__ int64_t wcnt[4];
    __shared__ int64_t running;
    {
        int64_t mycnt = 0;
        for (int64_t i = lo + threadIdx.x; i < hi; i += 256)
            mycnt += acc[i * aw + aw - 1] > 0;
        mycnt = d_bfly_i64(mycnt);
        if (lane == 0) wcnt[wid] = mycnt;
        __syncthreads();
        if (threadIdx.x == 0)
            running = wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3]
                          ? (int64_t)atomicAdd(
                                cursor, (unsigned long long)(wcnt[0] +
                                                             wcnt[1] +
                                                             wcnt[2] +
                                                             wcnt[3]))
                          : 0;
    }
    __syncthreads();
    for (int64_t base = lo; base < hi; base += 256) {
        int64_t i = base + 64 * wid + lane;
        bool sel = i < hi && acc[i * aw + aw - 1] > 0;
        uint64_t m = d_ballot(sel);
        int wsum = __popcll(m);
        if (lane == 0) wcnt[wid] = wsum;
        __syncthreads();
        int64_t woff = running;
        for (int w = 0; w < wid; w++) woff += wcnt[w];
        if (sel) {
            int64_t pos = woff + __popcll(m & ((1ull << lane) - 1));
            d_group_row(keys, head, acc, aw, bp, i, pos, out_key,
                        payload_outs, out_dec, out_f64, out_cnt);
        }
        __syncthreads();
        if (threadIdx.x == 0)
            running += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        __syncthreads();
    }
}

/* the same rows from the table's hit list: entry i names the slot of
 * output row i, so there is no scan, no cursor and no second pass — one
 * key line and one accumulator line gathered per group.  Row order is the
 * probes' append order (unspecified, as above). */
__global__ __launch_bounds__(256) void k_groups_emit_list(
    const void* hits, int32_t wide, int64_t n_hits, const int64_t* keys,
    const int32_t* head, const unsigned long long* acc, int32_t aw,
    build_payloads bp, int64_t* out_key, emit_outs payload_outs,
    int64_t* out_dec, double* out_f64, int64_t* out_cnt)
{
    int64_t pos = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (pos >= n_hits) return;
    int64_t i = wide ? ((const int64_t*)hits)[pos]
                     : (int64_t)((const uint32_t*)hits)[pos];
    d_group_row(keys, head, acc, aw, bp, i, pos, out_key, payload_outs,
                out_dec, out_f64, out_cnt);
}

/* ------------------------------------------------------------------ */
/* TopN — TopNOperator.java:32,90-111 / InMemoryGroupedTopNBuilder:   */
/* ORDER BY val DESC, date ASC, key ASC LIMIT L.  Per-thread local    */
/* top-L, then a block tournament in LDS; block winners merged on the */
/* host (the candidate set of any block's top-L contains every global */
/* top-L member of that block's rows).                                */
/* ------------------------------------------------------------------ */
#define TOPN_NB 256
#define TOPN_MAXL 16

struct topn_cand {
    int64_t val_bits; /* i64 ticks, or f64 bits (non-negative) */
    int64_t key;
    int32_t date;
    int32_t valid;
};

__device__ inline bool d_topn_less(bool is_f64, int64_t av, int32_t ad,
                                   int64_t ak, int64_t bv, int32_t bd,
                                   int64_t bk)
{
    /* returns true if a ranks WORSE than b (b wins) */
    if (av != bv) {
        if (is_f64) {
            double x = __longlong_as_double(av), y = __longlong_as_double(bv);
            return x < y;
        }
        return av < bv;
    }
    if (ad != bd) return ad > bd;
    return ak > bk;
}

__global__ __launch_bounds__(256) void k_topn(const void* vals, int is_f64,
                                              const int32_t* dates,
                                              const int64_t* keys, int64_t n,
                                              int32_t L, topn_cand* block_out)
{
    /* per-thread local top-L (insertion array; rare-path scratch) */
    int64_t lv[TOPN_MAXL];
    int32_t ld[TOPN_MAXL];
    int64_t lk[TOPN_MAXL];
    int cnt = 0;
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        int64_t v = is_f64 ? __double_as_longlong(((const double*)vals)[i])
                           : ((const int64_t*)vals)[i];
        int32_t d = dates[i];
        int64_t k = keys[i];
        if (cnt == L &&
            d_topn_less(is_f64, v, d, k, lv[cnt - 1], ld[cnt - 1],
                        lk[cnt - 1]))
            continue;
        /* insert */
        int pos = cnt < L ? cnt : L - 1;
        while (pos > 0 &&
               d_topn_less(is_f64, lv[pos - 1], ld[pos - 1], lk[pos - 1], v,
                           d, k)) {
            lv[pos] = lv[pos - 1];
            ld[pos] = ld[pos - 1];
            lk[pos] = lk[pos - 1];
            pos--;
        }
        lv[pos] = v;
        ld[pos] = d;
        lk[pos] = k;
        if (cnt < L) cnt++;
    }
    /* block tournament: L rounds of argmax over 256 exposed heads */
    __shared__ int64_t sv[256];
    __shared__ int32_t sd[256];
    __shared__ int64_t sk[256];
    __shared__ int32_t sidx[256];
    int head = 0;
    for (int r = 0; r < L; r++) {
        bool have = head < cnt;
        sv[threadIdx.x] = have ? lv[head] : (int64_t)0x8000000000000000ll;
        sd[threadIdx.x] = have ? ld[head] : 0x7fffffff;
        sk[threadIdx.x] = have ? lk[head] : 0x7fffffffffffffffll;
        sidx[threadIdx.x] = have ? (int)threadIdx.x : -1;
        __syncthreads();
        for (int s = 128; s >= 1; s >>= 1) {
            if (threadIdx.x < s) {
                int a = threadIdx.x, b = threadIdx.x + s;
                bool bwins =
                    sidx[a] < 0 ||
                    (sidx[b] >= 0 &&
                     d_topn_less(is_f64, sv[a], sd[a], sk[a], sv[b], sd[b],
                                 sk[b]));
                if (bwins) {
                    sv[a] = sv[b];
                    sd[a] = sd[b];
                    sk[a] = sk[b];
                    sidx[a] = sidx[b];
                }
            }
            __syncthreads();
        }
        if (threadIdx.x == 0) {
            topn_cand c;
            c.val_bits = sv[0];
            c.date = sd[0];
            c.key = sk[0];
            c.valid = sidx[0] >= 0;
            block_out[(size_t)blockIdx.x * L + r] = c;
        }
        int win = sidx[0];
        __syncthreads();
        if (win == (int)threadIdx.x) head++;
    }
}

/* large-limit TopN (limit > TOPN_MAXL): histogram preselect.
 * Pass 1 histograms the 16 high bits of the order-preserving key
 * transform; the host scans from the top bin until >= limit rows are
 * covered; pass 2 collects every row at or above that bin's floor
 * (wave-aggregated append), and the host does the exact final sort of
 * the <= limit + bin-slop candidates — the same candidate-merge step
 * the block-tournament path ends with. */
__device__ inline uint64_t d_topn_sortable(int is_f64, int64_t bits)
{
    if (!is_f64) return (uint64_t)bits ^ 0x8000000000000000ull;
    uint64_t u = (uint64_t)bits;
    return (u & 0x8000000000000000ull) ? ~u : (u | 0x8000000000000000ull);
}

__global__ __launch_bounds__(256) void k_topn_hist(
    const void* vals, int is_f64, int64_t n,
    unsigned long long* hist /* [65536] */)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        int64_t b = is_f64
                        ? __double_as_longlong(((const double*)vals)[i])
                        : ((const int64_t*)vals)[i];
        uint64_t s = d_topn_sortable(is_f64, b);
        atomicAdd(&hist[(unsigned)(s >> 48)], 1ull);
    }
}

__global__ __launch_bounds__(256) void k_topn_collect(
    const void* vals, int is_f64, const int32_t* dates,
    const int64_t* keys, int64_t n, uint64_t floor_sortable,
    topn_cand* out, int64_t cap, unsigned long long* cursor)
{
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < n; i += stride) {
        int64_t b = is_f64
                        ? __double_as_longlong(((const double*)vals)[i])
                        : ((const int64_t*)vals)[i];
        uint64_t s = d_topn_sortable(is_f64, b);
        bool sel = s >= floor_sortable;
        uint64_t m = d_ballot(sel);
        int lane = threadIdx.x & 63;
        unsigned long long base = 0;
        if (lane == 0 && m)
            base = atomicAdd(cursor, (unsigned long long)__popcll(m));
        base = __shfl((long long)base, 0, 64);
        if (sel) {
            int64_t pos =
                (int64_t)base + __popcll(m & ((1ull << lane) - 1));
            if (pos < cap) {
                topn_cand c;
                c.val_bits = b;
                c.date = dates[i];
                c.key = keys[i];
                c.valid = 1;
                out[pos] = c;
            }
        }
    }
}

/* ------------------------------------------------------------------ */
/* partition split — PartitionedOutputOperator.partitionPage:394 /    */
/* OptimizedPartitionedOutputOperator.java:86 columnar split;         */
/* partition id per pg_plan_partition (math in fixed128.h, cites      */
/* HashGenerator.java:22-29 + AbstractLongType.java:137-140).         */
/* Stable within partition (row-ascending), like the reference's      */
/* per-partition position lists (PartitioningExchanger.java:73).      */
/* ------------------------------------------------------------------ */
#define PART_NB 1024
#define PART_MAXP 256

__device__ inline int d_part_id(const pg_page& pg, int key_col, int np,
                                int64_t i)
{
    /* rawHash: CombineHashFunction.java:28-30 fold from
     * INITIAL_HASH_VALUE=0: h = 31*0 + typeHash(key); bigint typeHash =
     * AbstractLongType.java:137-140, varchar typeHash = XxHash64 over the
     * bytes (AbstractVariableWidthBlock.java:102-105) */
    const pg_col& c = pg.cols[key_col];
    if (c.tag == PG_T_VARBIN) {
        int64_t e = c.dict_ids ? (int64_t)c.dict_ids[i] : i;
        int32_t b0 = c.offsets[e], b1 = c.offsets[e + 1];
        return pg_partition(
            pg_xxh64((const uint8_t*)c.data + b0, (uint64_t)(b1 - b0)), np);
    }
    int64_t key = d_load_i64(c, i);
    return pg_partition(pg_bigint_hash(key), np);
}

__global__ __launch_bounds__(256) void k_part_count(pg_page pg,
                                                    pg_plan_partition plan,
                                                    int64_t chunk,
                                                    int64_t* block_counts)
{
    const int64_t n = pg.n_rows;
    const int64_t lo = (int64_t)blockIdx.x * chunk;
    const int64_t hi = min(lo + chunk, n);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    __shared__ int64_t cnt[4][PART_MAXP];
    for (int p = threadIdx.x; p < 4 * PART_MAXP; p += 256)
        ((int64_t*)cnt)[p] = 0;
    __syncthreads();
    for (int64_t base = lo + 64 * wid; base < hi; base += 256) {
        int64_t i = base + lane;
        int pid = i < hi ? d_part_id(pg, plan.key_col, plan.n_partitions, i)
                         : -1;
        for (int p = 0; p < plan.n_partitions; p++) {
            uint64_t m = d_ballot(pid == p);
            if (lane == 0) cnt[wid][p] += __popcll(m);
        }
    }
    __syncthreads();
    if (threadIdx.x < (unsigned)plan.n_partitions) {
        int p = threadIdx.x;
        block_counts[(size_t)blockIdx.x * plan.n_partitions + p] =
            cnt[0][p] + cnt[1][p] + cnt[2][p] + cnt[3][p];
    }
}

__global__ __launch_bounds__(256) void k_part_emit(pg_page pg,
                                                   pg_plan_partition plan,
                                                   int64_t chunk,
                                                   const int64_t* block_offs,
                                                   emit_outs outs)
{
    const int64_t n = pg.n_rows;
    const int64_t lo = (int64_t)blockIdx.x * chunk;
    const int64_t hi = min(lo + chunk, n);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    __shared__ int64_t running[PART_MAXP];
    __shared__ int64_t wcnt[4][PART_MAXP];
    for (int p = threadIdx.x; p < plan.n_partitions; p += 256)
        running[p] =
            block_offs[(size_t)blockIdx.x * plan.n_partitions + p];
    __syncthreads();
    for (int64_t base = lo; base < hi; base += 256) {
        int64_t i = base + 64 * wid + lane;
        int pid = i < hi ? d_part_id(pg, plan.key_col, plan.n_partitions, i)
                         : -1;
        for (int p = 0; p < plan.n_partitions; p++) {
            uint64_t mm = d_ballot(pid == p);
            if (lane == 0) wcnt[wid][p] = __popcll(mm);
        }
        __syncthreads();
        /* second ballot pass: emit (uniform execution of ballot per p) */
        for (int p = 0; p < plan.n_partitions; p++) {
            uint64_t mm = d_ballot(pid == p);
            if (pid == p) {
                int64_t woff = running[p];
                for (int w = 0; w < wid; w++) woff += wcnt[w][p];
                int64_t pos = woff + __popcll(mm & ((1ull << lane) - 1));
                for (int o = 0; o < outs.n; o++) {
                    pg_proj pr;
                    pr.kind = PG_PROJ_IDENT;
                    pr.a = plan.emit_cols[o];
                    d_emit_val(pg, pr, i, outs.ptr[o], outs.tag[o], pos);
                }
            }
        }
        __syncthreads();
        if (threadIdx.x < (unsigned)plan.n_partitions) {
            int p = threadIdx.x;
            running[p] += wcnt[0][p] + wcnt[1][p] + wcnt[2][p] + wcnt[3][p];
        }
        __syncthreads();
    }
}

/* ------------------------------------------------------------------ */
/* ORDER BY — OrderByOperator.java over PagesIndex.sort /             */
/* PagesIndexOrdering, orders per SortOrder.java.  A least-significant */
/* -digit radix sort, 8-bit digits, over (u64 sortable key, u32 row   */
/* id) pairs in ping-pong buffers.  Keys are processed last to first; */
/* every pass is stable, which yields the multi-key order and keeps   */
/* ties in input order (stricter than the reference's sort).          */
/* ------------------------------------------------------------------ */
#define SORT_WINDOW 256      /* rows one block ranks per step */
#define SORT_MIN_WINDOWS 4   /* a block's chunk is at least this many */
#define SORT_NB 1024         /* most blocks a pass launches */

/* keys[i] = sortable key of column[rowid[i]] (sortkey.h).  rowid NULL is
 * the first key processed: the identity, which also seeds ids.  A row
 * that is null in the key's mask encodes as 0, so the value under a null
 * never reaches the sort.  mask_mode: the key is the gathered mask byte
 * itself, turned into the two bins of the NULLS FIRST/LAST pass. */
__global__ __launch_bounds__(256) void k_sort_encode(
    const void* col, int tag, int order, const uint8_t* mask, int mask_mode,
    const uint32_t* rowid, uint32_t* ids, uint64_t* keys, int64_t n)
{
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n;
         i += stride) {
        uint32_t r = rowid ? rowid[i] : (uint32_t)i;
        if (!rowid) ids[i] = r;
        bool null = mask && mask[r];
        uint64_t k;
        if (mask_mode) {
            /* order & 1: NULLS LAST */
            k = null == (bool)(order & 1) ? 1 : 0;
        } else if (null) {
            k = 0;
        } else {
            uint64_t bits;
            switch (tag) {
                case PG_T_U8: bits = ((const uint8_t*)col)[r]; break;
                case PG_T_I32: bits = ((const uint32_t*)col)[r]; break;
                default: bits = ((const uint64_t*)col)[r]; break;
            }
            k = pg_sortkey(tag, order, bits);
        }
        keys[i] = k;
    }
}

/* one read of the keys -> the 8 x 256 global digit histograms.  LDS
 * atomics per block, then one global add per non-empty bin.  A byte on
 * which a whole wave agrees (the common case for the high bytes) costs
 * one LDS add for the wave, not 64 colliding ones. */
__global__ __launch_bounds__(256) void k_sort_digits(const uint64_t* keys,
                                                     int64_t n,
                                                     uint32_t* hist)
{
    __shared__ uint32_t h[8 * 256];
    for (int p = threadIdx.x; p < 8 * 256; p += 256) h[p] = 0;
    __syncthreads();
    const int lane = threadIdx.x & 63;
    const int64_t stride = (int64_t)gridDim.x * 256;
    /* whole waves enter together so the ballots are uniform */
    for (int64_t base = (int64_t)blockIdx.x * 256 + (threadIdx.x & ~63);
         base < n; base += stride) {
        int64_t i = base + lane;
        bool valid = i < n;
        uint64_t k = valid ? keys[i] : 0;
        uint64_t act = d_ballot(valid);
        /* base < n, so lane 0 is always a valid row: compare with it */
        uint32_t f_lo = __shfl((uint32_t)k, 0);
        uint32_t f_hi = __shfl((uint32_t)(k >> 32), 0);
        uint64_t x = k ^ (((uint64_t)f_hi << 32) | f_lo);
        for (int b = 0; b < 8; b++) {
            int d = (int)(k >> (8 * b)) & 255;
            bool differs = valid && ((x >> (8 * b)) & 255) != 0;
            if (d_ballot(differs) == 0) {
                if (lane == 0)
                    atomicAdd(&h[b * 256 + d], (uint32_t)__popcll(act));
            } else if (valid) {
                atomicAdd(&h[b * 256 + d], 1u);
            }
        }
    }
    __syncthreads();
    for (int p = threadIdx.x; p < 8 * 256; p += 256)
        if (h[p]) atomicAdd(&hist[p], h[p]);
}

/* per pass: block b owns rows [b*chunk, (b+1)*chunk) and writes its 256
 * bin counts, digit-major (counts[d * nb + b]) — the order the scan
 * wants */
__global__ __launch_bounds__(256) void k_radix_count(const uint64_t* keys,
                                                     int64_t n, int shift,
                                                     int64_t chunk,
                                                     uint32_t* counts)
{
    __shared__ uint32_t h[256];
    h[threadIdx.x] = 0;
    __syncthreads();
    const int64_t lo = (int64_t)blockIdx.x * chunk;
    const int64_t hi = min(lo + chunk, n);
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256)
        atomicAdd(&h[(keys[i] >> shift) & 255], 1u);
    __syncthreads();
    counts[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = h[threadIdx.x];
}

/* exclusive scan of the counters in digit-major, block-minor order, in
 * place, one block per digit: afterwards counts[d * nb + b] is where
 * block b's first row of digit d goes.  Block d starts at the number of
 * rows with a smaller digit, which it reads off the pass's global
 * histogram (totals[256], from k_sort_digits over the same keys), and
 * scans its own row of nb <= SORT_NB block counts. */
__global__ __launch_bounds__(256) void k_radix_scan(uint32_t* counts, int nb,
                                                    const uint32_t* totals)
{
    __shared__ uint32_t part[256];
    __shared__ uint32_t below[256];
    const int d = blockIdx.x, t = threadIdx.x;
    uint32_t* row = counts + (size_t)d * nb;
    const int per = (nb + 255) / 256;
    const int lo = min(t * per, nb);
    const int hi = min(lo + per, nb);
    uint32_t s = 0;
    for (int i = lo; i < hi; i++) s += row[i];
    part[t] = s;
    below[t] = t < d ? totals[t] : 0;
    __syncthreads();
    /* Hillis-Steele inclusive scans of the per-thread sums and of the
     * smaller digits' totals */
    for (int off = 1; off < 256; off <<= 1) {
        uint32_t v = t >= off ? part[t - off] : 0;
        uint32_t b = t >= off ? below[t - off] : 0;
        __syncthreads();
        part[t] += v;
        below[t] += b;
        __syncthreads();
    }
    uint32_t run = below[255] + part[t] - s;
    for (int i = lo; i < hi; i++) {
        uint32_t c = row[i];
        row[i] = run;
        run += c;
    }
}

/* the stable scatter.  Geometry of k_part_emit: a block walks its chunk
 * in SORT_WINDOW-row windows with running[256] in LDS and per-wave bin
 * counts wcnt[4][256]; a row lands at running[d] + the counts of the
 * waves before its own + its rank among the same-digit lanes below it.
 * The same-digit peer mask comes from 8 ballots, one per digit bit (each
 * ANDed in as is or complemented, by the lane's own bit), not from one
 * ballot per bin.  Lanes past the end of the chunk are taken out by the
 * ballot of `valid`, so they match nobody. */
__global__ __launch_bounds__(256) void k_radix_scatter(
    const uint64_t* keys_in, const uint32_t* ids_in, uint64_t* keys_out,
    uint32_t* ids_out, int64_t n, int shift, int64_t chunk,
    const uint32_t* offs)
{
    __shared__ uint32_t running[256];
    __shared__ uint32_t wcnt[4][256];
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    const int64_t lo = (int64_t)blockIdx.x * chunk;
    const int64_t hi = min(lo + chunk, n);
    running[threadIdx.x] = offs[(size_t)threadIdx.x * gridDim.x + blockIdx.x];
    for (int w = 0; w < 4; w++) wcnt[w][threadIdx.x] = 0;
    __syncthreads();
    for (int64_t base = lo; base < hi; base += SORT_WINDOW) {
        int64_t i = base + threadIdx.x;
        bool valid = i < hi;
        uint64_t k = valid ? keys_in[i] : 0;
        uint32_t id = valid ? ids_in[i] : 0;
        int d = (int)(k >> shift) & 255;
        uint64_t peers = d_ballot(valid);
        for (int b = 0; b < 8; b++) {
            bool bit = (d >> b) & 1;
            uint64_t m = d_ballot(bit);
            peers &= bit ? m : ~m;
        }
        int rank = __popcll(peers & ((1ull << lane) - 1));
        if (valid && rank == 0) wcnt[wid][d] = (uint32_t)__popcll(peers);
        __syncthreads();
        if (valid) {
            uint32_t pos = running[d] + rank;
            for (int w = 0; w < wid; w++) pos += wcnt[w][d];
            keys_out[pos] = k;
            ids_out[pos] = id;
        }
        __syncthreads();
        /* thread t owns bin t: fold the window in and clear it */
        uint32_t add = 0;
        for (int w = 0; w < 4; w++) {
            add += wcnt[w][threadIdx.x];
            wcnt[w][threadIdx.x] = 0;
        }
        running[threadIdx.x] += add;
        __syncthreads();
    }
}

/* out[c][i] = in[c][rowid[i]] for i < n_out (the limit), per emit column
 * of width 1, 4, 8 or 16 bytes, and for the masks */
struct sort_gather_cols {
    int n;
    const void* src[PG_MAX_SORT_EMIT];
    void* dst[PG_MAX_SORT_EMIT];
    int width[PG_MAX_SORT_EMIT];
    const uint8_t* msrc[PG_MAX_SORT_EMIT]; /* NULL: column has no mask */
    uint8_t* mdst[PG_MAX_SORT_EMIT];
};

__global__ __launch_bounds__(256) void k_sort_gather(const uint32_t* rowid,
                                                     int64_t n_out,
                                                     sort_gather_cols g)
{
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n_out;
         i += stride) {
        uint32_t r = rowid[i];
        for (int c = 0; c < g.n; c++) {
            switch (g.width[c]) {
                case 1:
                    ((uint8_t*)g.dst[c])[i] = ((const uint8_t*)g.src[c])[r];
                    break;
                case 4:
                    ((uint32_t*)g.dst[c])[i] = ((const uint32_t*)g.src[c])[r];
                    break;
                case 8:
                    ((uint64_t*)g.dst[c])[i] = ((const uint64_t*)g.src[c])[r];
                    break;
                default:
                    ((ulonglong2*)g.dst[c])[i] =
                        ((const ulonglong2*)g.src[c])[r];
                    break;
            }
            if (g.msrc[c]) g.mdst[c][i] = g.msrc[c][r];
        }
    }
}

/* ids[i] = i: the "sorted" permutation of a plan without keys */
__global__ __launch_bounds__(256) void k_sort_iota(uint32_t* ids, int64_t n)
{
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n;
         i += stride)
        ids[i] = (uint32_t)i;
}

/* ------------------------------------------------------------------ */
/* MARK_DISTINCT — MarkDistinctOperator.java / MarkDistinctHash.java   */
/* and DistinctLimitOperator.java: is this row the first one with its  */
/* key combination?  The table is GROUPBY_MULTI's null-aware one: a    */
/* state word per slot, n_keys + 1 key planes (the last holds the      */
/* per-channel null bits), the same hash fold, finalizer and           */
/* CAS-claim / publish protocol.  Each slot carries one more u64,       */
/* `first`: the smallest global row ordinal (rows of all earlier pages  */
/* + row index) seen for the slot, all ones until one is.  Winning the  */
/* claim says nothing about being first — a later row of the page may   */
/* well claim the slot — so launch 1 only lowers `first` and launch 2,  */
/* strictly after it, marks the row whose ordinal `first` ended up as.  */
/* The slot each row found is kept per row (slot_of, 4 bytes) so that   */
/* launch 2 does not probe again.                                       */
/* ------------------------------------------------------------------ */
#define MD_NO_SLOT 0xffffffffu /* the table was full: the row has no slot */

__global__ __launch_bounds__(256) void k_mark_distinct_insert(
    pg_page pg, pg_plan_mark_distinct plan, unsigned int* state, int64_t* kv,
    int64_t cap, int64_t mask, unsigned long long* first, int64_t base,
    uint32_t* slot_of, unsigned long long* counters /* [claims, full] */)
{
    const int n_keys = plan.n_keys;
    int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (; i < pg.n_rows; i += stride) {
        int64_t k[4];
        int64_t knull = 0; /* bit ch = channel ch is null */
        uint64_t h = 0;
#pragma unroll
        for (int ch = 0; ch < 4; ch++) {
            if (ch >= n_keys) break;
            if (d_col_is_null(pg, plan.key_col[ch], i)) {
                k[ch] = 0; /* the stored value never matters */
                knull |= (int64_t)1 << ch;
                h = 31u * h; /* NULL_HASH_CODE = 0 */
                continue;
            }
            k[ch] = d_gb_key(pg, plan.key_col[ch], i);
            h = 31u * h + pg_bigint_hash(k[ch]);
        }
        int64_t pos = (int64_t)(pg_murmur3_finalize(h) & (uint64_t)mask);
        int64_t slot = -1, tries = 0;
        for (;;) {
            unsigned int st = __hip_atomic_load(
                &state[pos], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (st == 2u) {
                bool eq = true;
#pragma unroll
                for (int ch = 0; ch < 4; ch++) {
                    if (ch >= n_keys) break;
                    eq = eq && __hip_atomic_load(
                                   &kv[(size_t)ch * cap + pos],
                                   __ATOMIC_RELAXED,
                                   __HIP_MEMORY_SCOPE_SYSTEM) == k[ch];
                }
                eq = eq && __hip_atomic_load(&kv[(size_t)n_keys * cap + pos],
                                             __ATOMIC_RELAXED,
                                             __HIP_MEMORY_SCOPE_SYSTEM) ==
                               knull;
                if (eq) {
                    slot = pos;
                    break;
                }
                pos = (pos + 1) & mask;
                if (++tries > mask) {
                    atomicAdd(counters + 1, 1ull);
                    break;
                }
            } else if (st == 0u) {
                unsigned int prev = atomicCAS(&state[pos], 0u, 1u);
                if (prev == 0u) {
#pragma unroll
                    for (int ch = 0; ch < 4; ch++) {
                        if (ch >= n_keys) break;
                        __hip_atomic_store(&kv[(size_t)ch * cap + pos],
                                           k[ch], __ATOMIC_RELAXED,
                                           __HIP_MEMORY_SCOPE_SYSTEM);
                    }
                    __hip_atomic_store(&kv[(size_t)n_keys * cap + pos],
                                       knull, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_SYSTEM);
                    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                    __hip_atomic_store(&state[pos], 2u, __ATOMIC_RELAXED,
                                       __HIP_MEMORY_SCOPE_SYSTEM);
                    atomicAdd(counters, 1ull); /* distinct combinations */
                    slot = pos;
                    break;
                }
                /* lost the claim: retry the same position */
            }
            /* st == 1: publisher in flight — retry (as k_groupby_multi) */
        }
        slot_of[i] = slot < 0 ? MD_NO_SLOT : (uint32_t)slot;
        if (slot < 0) continue;
        /* `first` only falls, so a relaxed load that already shows a
         * smaller ordinal makes the atomic redundant — always, on every
         * page after the key's first one */
        const unsigned long long ord = (unsigned long long)(base + i);
        if (__hip_atomic_load(&first[slot], __ATOMIC_RELAXED,
                              __HIP_MEMORY_SCOPE_AGENT) > ord)
            atomicMin(&first[slot], ord);
    }
}

/* launch 2: first[slot] is final for the page */
__device__ inline bool d_md_is_first(const uint32_t* slot_of,
                                     const unsigned long long* first,
                                     int64_t base, int64_t i)
{
    const uint32_t s = slot_of[i];
    return s != MD_NO_SLOT && first[s] == (unsigned long long)(base + i);
}

/* mark mode: one marker byte per row */
__global__ __launch_bounds__(256) void k_mark_distinct_mark(
    const uint32_t* slot_of, const unsigned long long* first, int64_t base,
    int64_t n, uint8_t* marker)
{
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n;
         i += stride)
        marker[i] = d_md_is_first(slot_of, first, base, i);
}

/* only mode, the selection kernels' block-window scheme: block b owns the
 * 256-aligned row chunk [b*chunk, (b+1)*chunk), a wave one 64-aligned
 * ballot word of each 256-row window.  The count pass keeps the words and
 * the per-block totals; after the host's prefix sum over the blocks the
 * second pass turns the words into the ascending list of the first
 * n_out marked row ids, which k_sort_gather then reads. */
__global__ __launch_bounds__(256) void k_mark_distinct_count(
    const uint32_t* slot_of, const unsigned long long* first, int64_t base,
    int64_t n, int64_t chunk, int64_t* block_counts,
    unsigned long long* selbits)
{
    const int64_t lo = (int64_t)blockIdx.x * chunk;
    const int64_t hi = min(lo + chunk, n);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    int64_t cnt = 0;
    for (int64_t wbase = lo + 64 * wid; wbase < hi; wbase += 256) {
        const int64_t i = wbase + lane;
        const bool sel = i < hi && d_md_is_first(slot_of, first, base, i);
        const uint64_t m = d_ballot(sel);
        if (lane == 0) {
            cnt += __popcll(m);
            selbits[wbase >> 6] = m;
        }
    }
    __shared__ int64_t lds[4];
    if (lane == 0) lds[wid] = cnt;
    __syncthreads();
    if (threadIdx.x == 0)
        block_counts[blockIdx.x] = lds[0] + lds[1] + lds[2] + lds[3];
}

__global__ __launch_bounds__(256) void k_mark_distinct_rowids(
    const unsigned long long* selbits, int64_t n, int64_t chunk,
    const int64_t* block_offs, int64_t n_out, uint32_t* rowid)
{
    const int64_t lo = (int64_t)blockIdx.x * chunk;
    const int64_t hi = min(lo + chunk, n);
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
    __shared__ int64_t wcnt[4];
    __shared__ int64_t running;
    if (threadIdx.x == 0) running = block_offs[blockIdx.x];
    __syncthreads();
    for (int64_t base = lo; base < hi; base += 256) {
        const int64_t wbase = base + 64 * wid;
        /* a wave past the chunk's end has no word of its own */
        const uint64_t m = wbase < hi ? selbits[wbase >> 6] : 0;
        if (lane == 0) wcnt[wid] = __popcll(m);
        __syncthreads();
        int64_t woff = running;
        for (int w = 0; w < wid; w++) woff += wcnt[w];
        if ((m >> lane) & 1) {
            const int64_t pos = woff + __popcll(m & ((1ull << lane) - 1));
            if (pos < n_out) rowid[pos] = (uint32_t)(wbase + lane);
        }
        __syncthreads();
        if (threadIdx.x == 0)
            running += wcnt[0] + wcnt[1] + wcnt[2] + wcnt[3];
        __syncthreads();
    }
}

/* ------------------------------------------------------------------ */
/* WINDOW — WindowOperator.java over the sorted PagesIndex: what runs */
/* after the sort.  Boundary flags from the keys of adjacent sorted   */
/* rows, per-row partition / peer-group bounds from scans of the head */
/* indices, one segmented scan per aggregate, and a per-function emit */
/* that reads those at the row, at its peer group's end or at its     */
/* partition's end.                                                   */
/*                                                                    */
/* Every scan is three launches in the sort's chunk geometry: each    */
/* block folds its chunk into a carry, one block scans the <= SORT_NB */
/* carries, each block rescans its chunk from its carry-in.  No block */
/* ever waits on another.                                             */
/* ------------------------------------------------------------------ */
#define WIN_PART_HEAD 1 /* first row of a partition */
#define WIN_PEER_HEAD 2 /* first row of a peer group */
#define WIN_NONE 0xffffffffu /* no head: above every row index */

/* inclusive scan over the block's 256 threads of a type with
 * identity / combine / shfl_up: wave64 shuffles, then the four wave
 * totals through LDS.  excl is the scan without the thread's own value,
 * total the fold of all 256.  Every thread of the block must call it. */
template <class T>
__device__ inline T win_scan256(T v, T* wtot, T& excl, T& total)
{
    const int lane = threadIdx.x & 63, wid = threadIdx.x >> 6;
#pragma unroll
    for (int d = 1; d < 64; d <<= 1) {
        T o = T::shfl_up(v, d);
        if (lane >= d) v = T::combine(o, v);
    }
    T up = T::shfl_up(v, 1);
    if (lane == 0) up = T::identity();
    if (lane == 63) wtot[wid] = v;
    __syncthreads();
    T pre = T::identity(), tot = T::identity();
#pragma unroll
    for (int w = 0; w < 4; w++) {
        T t = wtot[w];
        if (w < wid) pre = T::combine(pre, t);
        tot = T::combine(tot, t);
    }
    __syncthreads(); /* wtot is free for the next call */
    total = tot;
    excl = T::combine(pre, up);
    return T::combine(pre, v);
}

/* exclusive scan, in place, of nb <= SORT_NB block carries by one block:
 * each thread folds its run of consecutive carries, the 256 partial folds
 * are scanned, and the thread rewrites its run.  REV scans from the last
 * carry down (for a commutative combine only). */
template <class T, bool REV>
__device__ inline void win_carry_scan(T* c, int nb, T* wtot)
{
    const int per = (nb + 255) / 256;
    const int lo = min((int)threadIdx.x * per, nb);
    const int hi = min(lo + per, nb);
    T s = T::identity();
    for (int k = lo; k < hi; k++)
        s = T::combine(s, c[REV ? nb - 1 - k : k]);
    T run, tot;
    win_scan256(s, wtot, run, tot);
    for (int k = lo; k < hi; k++) {
        const int j = REV ? nb - 1 - k : k;
        T cur = c[j];
        c[j] = run;
        run = T::combine(run, cur);
    }
}

/* forward: the last partition head and the last peer head at or before a
 * row (-1: none yet) and the number of peer heads up to it */
struct win_fwd {
    int32_t part, peer;
    uint32_t heads;
    static __device__ inline win_fwd identity() { return {-1, -1, 0}; }
    static __device__ inline win_fwd combine(win_fwd a, win_fwd b)
    {
        return {max(a.part, b.part), max(a.peer, b.peer), a.heads + b.heads};
    }
    static __device__ inline win_fwd shfl_up(win_fwd v, int d)
    {
        return {__shfl_up(v.part, d, 64), __shfl_up(v.peer, d, 64),
                __shfl_up(v.heads, d, 64)};
    }
};
/* backward: the first partition head and the first peer head after a row */
struct win_bwd {
    uint32_t part, peer;
    static __device__ inline win_bwd identity()
    {
        return {WIN_NONE, WIN_NONE};
    }
    static __device__ inline win_bwd combine(win_bwd a, win_bwd b)
    {
        return {min(a.part, b.part), min(a.peer, b.peer)};
    }
    static __device__ inline win_bwd shfl_up(win_bwd v, int d)
    {
        return {__shfl_up(v.part, d, 64), __shfl_up(v.peer, d, 64)};
    }
};

struct win_keys {
    int n_keys, n_part;
    const void* col[PG_MAX_SORT_KEYS];
    const uint8_t* mask[PG_MAX_SORT_KEYS]; /* NULL: the key has no nulls */
    int tag[PG_MAX_SORT_KEYS];
};

/* do input rows a and b differ on key j under ORDER_BY's comparator:
 * null equals null, and pg_sortkey maps every NaN to one key */
__device__ inline bool win_key_differs(const win_keys& k, int j, uint32_t a,
                                       uint32_t b)
{
    const bool na = k.mask[j] && k.mask[j][a];
    const bool nb = k.mask[j] && k.mask[j][b];
    if (na || nb) return na != nb;
    uint64_t x, y;
    switch (k.tag[j]) {
        case PG_T_U8:
            x = ((const uint8_t*)k.col[j])[a];
            y = ((const uint8_t*)k.col[j])[b];
            break;
        case PG_T_I32:
            x = ((const uint32_t*)k.col[j])[a];
            y = ((const uint32_t*)k.col[j])[b];
            break;
        default:
            x = ((const uint64_t*)k.col[j])[a];
            y = ((const uint64_t*)k.col[j])[b];
            break;
    }
    return pg_sortkey(k.tag[j], 0, x) != pg_sortkey(k.tag[j], 0, y);
}

/* launch 1 of the bounds scans, fused with the flags: sorted row i
 * against row i-1, key by key; a difference on a partition key heads a
 * partition (and a peer group), one on an order key a peer group.  The
 * block's carries: its last / first heads and its peer-head count. */
__global__ __launch_bounds__(256) void k_win_flags(
    win_keys k, const uint32_t* ids, int64_t n, int64_t chunk,
    uint8_t* flags, win_fwd* fwdc, win_bwd* bwdc)
{
    __shared__ win_fwd wf[4];
    __shared__ win_bwd wb[4];
    const int64_t lo = (int64_t)blockIdx.x * chunk;
    const int64_t hi = min(lo + chunk, n);
    win_fwd f = win_fwd::identity();
    win_bwd b = win_bwd::identity();
    for (int64_t i = lo + threadIdx.x; i < hi; i += 256) {
        uint8_t fl = 0;
        if (i == 0) {
            fl = WIN_PART_HEAD | WIN_PEER_HEAD;
        } else {
            const uint32_t r = ids[i], p = ids[i - 1];
            for (int j = 0; j < k.n_keys; j++)
                if (win_key_differs(k, j, r, p)) {
                    fl = j < k.n_part ? WIN_PART_HEAD | WIN_PEER_HEAD
                                      : WIN_PEER_HEAD;
                    break;
                }
        }
        flags[i] = fl;
        if (fl & WIN_PART_HEAD) {
            f.part = max(f.part, (int32_t)i);
            b.part = min(b.part, (uint32_t)i);
        }
        if (fl & WIN_PEER_HEAD) {
            f.peer = max(f.peer, (int32_t)i);
            b.peer = min(b.peer, (uint32_t)i);
            f.heads++;
        }
    }
    /* both combines commute, so the strided per-thread folds are fine */
    win_fwd xf, tf;
    win_bwd xb, tb;
    win_scan256(f, wf, xf, tf);
    win_scan256(b, wb, xb, tb);
    if (threadIdx.x == 0) {
        fwdc[blockIdx.x] = tf;
        bwdc[blockIdx.x] = tb;
    }
}

/* launch 2: block b's carry-in = the fold of the blocks before it
 * (forward) and after it (backward) */
__global__ __launch_bounds__(256) void k_win_bounds_carry(win_fwd* fwdc,
                                                          win_bwd* bwdc,
                                                          int nb)
{
    __shared__ win_fwd wf[4];
    __shared__ win_bwd wb[4];
    win_carry_scan<win_fwd, false>(fwdc, nb, wf);
    win_carry_scan<win_bwd, true>(bwdc, nb, wb);
}

/* launch 3: per row, the first row of its partition and of its peer
 * group and the running count of peer heads (a forward scan), then the
 * last row of its peer group and of its partition (a backward scan: the
 * element of row i is the head bit of row i+1) */
__global__ __launch_bounds__(256) void k_win_bounds(
    const uint8_t* flags, int64_t n, int64_t chunk, const win_fwd* fwdc,
    const win_bwd* bwdc, uint32_t* part_start, uint32_t* peer_start,
    uint32_t* heads, uint32_t* part_end, uint32_t* peer_end)
{
    __shared__ win_fwd wf[4];
    __shared__ win_bwd wb[4];
    const int64_t lo = (int64_t)blockIdx.x * chunk;
    const int64_t hi = min(lo + chunk, n);
    win_fwd frun = fwdc[blockIdx.x];
    for (int64_t base = lo; base < hi; base += SORT_WINDOW) {
        const int64_t i = base + threadIdx.x;
        const bool valid = i < hi;
        const uint8_t fl = valid ? flags[i] : 0;
        win_fwd e = {fl & WIN_PART_HEAD ? (int32_t)i : -1,
                     fl & WIN_PEER_HEAD ? (int32_t)i : -1,
                     fl & WIN_PEER_HEAD ? 1u : 0u};
        win_fwd ex, tot;
        e = win_fwd::combine(frun, win_scan256(e, wf, ex, tot));
        if (valid) {
            /* row 0 heads both, so neither index is -1 here */
            part_start[i] = (uint32_t)e.part;
            peer_start[i] = (uint32_t)e.peer;
            heads[i] = e.heads;
        }
        frun = win_fwd::combine(frun, tot);
    }
    win_bwd brun = bwdc[blockIdx.x];
    for (int64_t base = hi - 1; base >= lo; base -= SORT_WINDOW) {
        const int64_t i = base - threadIdx.x;
        const bool valid = i >= lo;
        /* heads at or past hi are in the carry-in */
        const uint8_t fl = valid && i + 1 < hi ? flags[i + 1] : 0;
        win_bwd e = {fl & WIN_PART_HEAD ? (uint32_t)(i + 1) : WIN_NONE,
                     fl & WIN_PEER_HEAD ? (uint32_t)(i + 1) : WIN_NONE};
        win_bwd ex, tot;
        e = win_bwd::combine(brun, win_scan256(e, wb, ex, tot));
        if (valid) {
            part_end[i] = (e.part == WIN_NONE ? (uint32_t)n : e.part) - 1;
            peer_end[i] = (e.peer == WIN_NONE ? (uint32_t)n : e.peer) - 1;
        }
        brun = win_bwd::combine(brun, tot);
    }
}

/* the scanned state of one aggregate: the non-null count, the 128-bit
 * sum (SUM: hi:lo, two's complement) or the extreme (MIN / MAX: lo as a
 * signed 64-bit value), and whether a partition head has been passed —
 * the segmented scan's reset bit.  K is the pg_win_func. */
template <int K>
struct win_acc {
    uint64_t lo;
    int64_t hi;
    uint32_t cnt;
    uint32_t head;
    static __device__ inline win_acc identity()
    {
        return {K == PG_WIN_MIN   ? (uint64_t)INT64_MAX
                : K == PG_WIN_MAX ? (uint64_t)INT64_MIN
                                  : 0,
                0, 0, 0};
    }
    /* a then b, b later in sorted order */
    static __device__ inline win_acc combine(win_acc a, win_acc b)
    {
        if (b.head) return b;
        win_acc r = b;
        r.head = a.head;
        r.cnt = a.cnt + b.cnt;
        if (K == PG_WIN_SUM) {
            uint64_t h = (uint64_t)b.hi;
            r.lo = b.lo;
            fx128_add(&h, &r.lo, (uint64_t)a.hi, a.lo);
            r.hi = (int64_t)h;
        } else if (K == PG_WIN_MIN) {
            r.lo = (uint64_t)min((int64_t)a.lo, (int64_t)b.lo);
        } else if (K == PG_WIN_MAX) {
            r.lo = (uint64_t)max((int64_t)a.lo, (int64_t)b.lo);
        }
        return r;
    }
    static __device__ inline win_acc shfl_up(win_acc v, int d)
    {
        win_acc r = v;
        if (K != PG_WIN_COUNT)
            r.lo = (uint64_t)__shfl_up((long long)v.lo, d, 64);
        if (K == PG_WIN_SUM) r.hi = __shfl_up((long long)v.hi, d, 64);
        r.cnt = __shfl_up(v.cnt, d, 64);
        r.head = __shfl_up(v.head, d, 64);
        return r;
    }
};

struct win_arg {
    const void* col;     /* NULL: count(*) */
    const uint8_t* mask; /* NULL: no nulls */
    int tag;
};

/* sorted row i as a scan element: the argument gathered through ids, a
 * null as the identity */
template <int K>
__device__ inline win_acc<K> win_load(const win_arg& a, const uint32_t* ids,
                                      const uint8_t* flags, int64_t i)
{
    win_acc<K> e = win_acc<K>::identity();
    e.head = flags[i] & WIN_PART_HEAD;
    if (K == PG_WIN_COUNT && !a.mask) {
        e.cnt = 1;
        return e;
    }
    const uint32_t r = ids[i];
    if (a.mask && a.mask[r]) return e;
    e.cnt = 1;
    if (K != PG_WIN_COUNT) {
        int64_t v;
        switch (a.tag) {
            case PG_T_U8: v = ((const uint8_t*)a.col)[r]; break;
            case PG_T_I32: v = ((const int32_t*)a.col)[r]; break;
            default: v = ((const int64_t*)a.col)[r]; break;
        }
        e.lo = (uint64_t)v;
        e.hi = v < 0 ? -1 : 0;
    }
    return e;
}

/* launch 1 of an aggregate's scan: the block's chunk folded in row order
 * (the segmented combine does not commute) */
template <int K>
__global__ __launch_bounds__(256) void k_win_agg_reduce(
    win_arg a, const uint32_t* ids, const uint8_t* flags, int64_t n,
    int64_t chunk, win_acc<K>* carry)
{
    __shared__ win_acc<K> wtot[4];
    const int64_t lo = (int64_t)blockIdx.x * chunk;
    const int64_t hi = min(lo + chunk, n);
    win_acc<K> run = win_acc<K>::identity();
    for (int64_t base = lo; base < hi; base += SORT_WINDOW) {
        const int64_t i = base + threadIdx.x;
        win_acc<K> e = i < hi ? win_load<K>(a, ids, flags, i)
                              : win_acc<K>::identity();
        win_acc<K> ex, tot;
        win_scan256(e, wtot, ex, tot);
        run = win_acc<K>::combine(run, tot);
    }
    if (threadIdx.x == 0) carry[blockIdx.x] = run;
}

/* launch 2 */
template <int K>
__global__ __launch_bounds__(256) void k_win_agg_carry(win_acc<K>* carry,
                                                       int nb)
{
    __shared__ win_acc<K> wtot[4];
    win_carry_scan<win_acc<K>, false>(carry, nb, wtot);
}

/* launch 3: the inclusive segmented scan, written per sorted row */
template <int K>
__global__ __launch_bounds__(256) void k_win_agg_scan(
    win_arg a, const uint32_t* ids, const uint8_t* flags, int64_t n,
    int64_t chunk, const win_acc<K>* carry, uint64_t* s_lo, int64_t* s_hi,
    uint32_t* s_cnt)
{
    __shared__ win_acc<K> wtot[4];
    const int64_t lo = (int64_t)blockIdx.x * chunk;
    const int64_t hi = min(lo + chunk, n);
    win_acc<K> run = carry[blockIdx.x];
    for (int64_t base = lo; base < hi; base += SORT_WINDOW) {
        const int64_t i = base + threadIdx.x;
        const bool valid = i < hi;
        win_acc<K> e = valid ? win_load<K>(a, ids, flags, i)
                             : win_acc<K>::identity();
        win_acc<K> ex, tot;
        e = win_acc<K>::combine(run, win_scan256(e, wtot, ex, tot));
        if (valid) {
            s_cnt[i] = e.cnt;
            if (K != PG_WIN_COUNT) s_lo[i] = e.lo;
            if (K == PG_WIN_SUM) s_hi[i] = e.hi;
        }
        run = win_acc<K>::combine(run, tot);
    }
}

/* one function's output column (and mask) from the bounds and, for the
 * aggregates, from the scan read at the frame's last row */
struct win_emit {
    int func, frame, width; /* width: bytes of an output value */
    int64_t offset;
    const uint32_t *ids, *part_start, *peer_start, *heads, *part_end,
        *peer_end;
    const uint64_t* s_lo;
    const int64_t* s_hi;
    const uint32_t* s_cnt;
    const void* col;      /* LAG / LEAD: the column and its mask */
    const uint8_t* cmask;
    void* out;
    uint8_t* omask; /* NULL for the columns that are never null */
    int32_t* err;   /* set to 1 by a SUM outside int64 */
};

__device__ inline void win_store(void* out, int width, int64_t i, int64_t v)
{
    switch (width) {
        case 1: ((uint8_t*)out)[i] = (uint8_t)v; break;
        case 4: ((int32_t*)out)[i] = (int32_t)v; break;
        default: ((int64_t*)out)[i] = v; break;
    }
}

__global__ __launch_bounds__(256) void k_win_emit(win_emit e, int64_t n)
{
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n;
         i += stride) {
        switch (e.func) {
            case PG_WIN_ROW_NUMBER:
                ((int64_t*)e.out)[i] = i - e.part_start[i] + 1;
                break;
            case PG_WIN_RANK:
                ((int64_t*)e.out)[i] =
                    (int64_t)e.peer_start[i] - e.part_start[i] + 1;
                break;
            case PG_WIN_DENSE_RANK:
                ((int64_t*)e.out)[i] =
                    (int64_t)e.heads[i] - e.heads[e.part_start[i]] + 1;
                break;
            case PG_WIN_LAG:
            case PG_WIN_LEAD: {
                int64_t t = -1;
                if (e.func == PG_WIN_LAG) {
                    if (e.offset <= i - (int64_t)e.part_start[i])
                        t = i - e.offset;
                } else if (e.offset <= (int64_t)e.part_end[i] - i) {
                    t = i + e.offset;
                }
                const uint32_t r = t < 0 ? 0 : e.ids[t];
                const bool null = t < 0 || (e.cmask && e.cmask[r]);
                if (e.width == 16) {
                    ulonglong2 v = {0, 0};
                    if (t >= 0) v = ((const ulonglong2*)e.col)[r];
                    ((ulonglong2*)e.out)[i] = v;
                } else {
                    int64_t v = 0;
                    if (t >= 0) switch (e.width) {
                        case 1: v = ((const uint8_t*)e.col)[r]; break;
                        case 4: v = ((const int32_t*)e.col)[r]; break;
                        default: v = ((const int64_t*)e.col)[r]; break;
                    }
                    win_store(e.out, e.width, i, v);
                }
                e.omask[i] = null;
                break;
            }
            default: {
                const int64_t at = e.frame == PG_FRAME_ROWS_RUNNING ? i
                                   : e.frame == PG_FRAME_RANGE_RUNNING
                                       ? (int64_t)e.peer_end[i]
                                       : (int64_t)e.part_end[i];
                const uint32_t cnt = e.s_cnt[at];
                if (e.func == PG_WIN_COUNT) {
                    ((int64_t*)e.out)[i] = cnt;
                    break;
                }
                int64_t v = 0;
                if (cnt) {
                    v = (int64_t)e.s_lo[at];
                    /* fits int64: the high word is the sign extension */
                    if (e.func == PG_WIN_SUM && e.s_hi[at] != (v >> 63)) {
                        *e.err = 1;
                        v = 0;
                    }
                }
                win_store(e.out, e.width, i, v);
                e.omask[i] = cnt == 0;
                break;
            }
        }
    }
}

/* ================================================================== */
/* host side: operator state machines + C-ABI                         */
/* ================================================================== */
#include <deque>
#include <memory>
#include <mutex>

namespace {

/* size-bucketed device buffer pool: operator lifecycles alloc/free the
 * same sizes every query, and hipMalloc/hipFree cost ~0.5-1 ms each —
 * pooling keeps the per-query overhead at kernel time.  Exact-size reuse;
 * bounded total. */
struct BufPool {
    std::mutex mu;
    std::multimap<size_t, void*> free_bufs;
    size_t pooled = 0;
    /* 288 GB HBM3E per GPU: cache aggressively — GB-scale hipMalloc
     * costs ~100 ms (page-table setup) and an 8 GB cap thrashed the
     * multi-probe pipelines (q21 at SF30: 109 ms of kernels inside a
     * 990 ms wall — see profiles/r01_q21_sf10_kernel_stats_before.txt) */
    static const size_t CAP = 96ull << 30;
    void* get(size_t n)
    {
        std::lock_guard<std::mutex> lk(mu);
        auto it = free_bufs.find(n);
        if (it == free_bufs.end()) return nullptr;
        void* p = it->second;
        free_bufs.erase(it);
        pooled -= n;
        return p;
    }
    bool put(size_t n, void* p)
    {
        std::lock_guard<std::mutex> lk(mu);
        if (pooled + n > CAP) return false;
        free_bufs.emplace(n, p);
        pooled += n;
        return true;
    }
};
static BufPool g_pool;

struct DevBuf {
    void* p = nullptr;
    size_t sz = 0;
    DevBuf() = default;
    DevBuf(const DevBuf&) = delete;
    DevBuf& operator=(const DevBuf&) = delete;
    DevBuf(DevBuf&& o) noexcept : p(o.p), sz(o.sz)
    {
        o.p = nullptr;
        o.sz = 0;
    }
    DevBuf& operator=(DevBuf&& o) noexcept
    {
        free();
        p = o.p;
        sz = o.sz;
        o.p = nullptr;
        o.sz = 0;
        return *this;
    }
    void alloc(size_t n)
    {
        free();
        size_t want = n ? n : 1;
        p = g_pool.get(want);
        if (!p) CHKV(hipMalloc(&p, want));
        sz = want;
    }
    void zero() { CHKV(hipMemsetAsync(p, 0, sz, g_stream)); }
    void free()
    {
        if (p && !g_pool.put(sz, p)) {
            hipError_t e = hipFree(p);
            (void)e;
        }
        p = nullptr;
        sz = 0;
    }
    ~DevBuf() { free(); }
};

static size_t type_size(int tag)
{
    switch (tag) {
        case PG_T_U8: return 1;
        case PG_T_I32: return 4;
        case PG_T_I128: return 16;
        default: return 8;
    }
}

/* ---- host checks of a plan's predicates ----
 * d_eval_preds trusts what it is given: it indexes sval by slen (and by
 * ival for the second needle) and picks its arm by the column's tag alone.
 * These two checks keep a foreign caller from reaching it with a plan the
 * kernels would answer silently wrong.  Both are plain loops over at most
 * PG_MAX_PRED predicates: no launch, no sync. */

/* the entries of preds[] a plan reads, one bit each: the row filter
 * preds[0..n_preds) plus any per-aggregate FILTER */
static uint32_t preds_used(int32_t n_preds,
                           const int32_t* agg_filter = nullptr,
                           int32_t n_aggs = 0)
{
    uint32_t used = 0;
    for (int p = 0; p < n_preds && p < PG_MAX_PRED; p++) used |= 1u << p;
    for (int a = 0; a < n_aggs && a < 6; a++)
        if (agg_filter[a] >= 0 && agg_filter[a] < PG_MAX_PRED)
            used |= 1u << agg_filter[a];
    return used;
}

/* at create: needle lengths inside sval */
static void check_pred_lens(const char* opname, const pg_pred* preds,
                            uint32_t used)
{
    const int64_t cap = (int64_t)sizeof(preds[0].sval);
    for (int p = 0; p < PG_MAX_PRED; p++) {
        if (!(used >> p & 1)) continue;
        const pg_pred& pr = preds[p];
        if (pr.op >= PG_CMP_IS_NULL) continue; /* reads the mask alone */
        if (pr.slen < 0 || pr.slen > cap)
            throw std::runtime_error(
                std::string(opname) + ": preds[" + std::to_string(p) +
                "].slen = " + std::to_string(pr.slen) + " is outside 0.." +
                std::to_string(cap) + " (the size of sval)");
        if ((pr.op == PG_CMP_CONTAINS2 || pr.op == PG_CMP_NOT_CONTAINS2) &&
            (pr.ival < 0 || pr.ival > cap - pr.slen))
            throw std::runtime_error(
                std::string(opname) + ": preds[" + std::to_string(p) +
                "].ival = " + std::to_string(pr.ival) +
                " (the second needle's length) must be >= 0 and fit sval "
                "after the first needle's " + std::to_string(pr.slen) +
                " of " + std::to_string(cap) + " bytes");
    }
}

/* at add_input, where the column types are known: ordering comparisons are
 * not defined for VARBIN, the string ops for nothing else */
static void check_pred_types(const char* opname, const pg_pred* preds,
                             uint32_t used, const pg_page* in)
{
    for (int p = 0; p < PG_MAX_PRED; p++) {
        if (!(used >> p & 1)) continue;
        const pg_pred& pr = preds[p];
        if (pr.op >= PG_CMP_IS_NULL) continue; /* any column type */
        if (pr.col < 0 || pr.col >= in->n_cols || pr.col >= 32) continue;
        const bool varbin = in->cols[pr.col].tag == PG_T_VARBIN;
        const bool ordering = pr.op >= PG_CMP_LT && pr.op <= PG_CMP_GE;
        const bool string_op =
            pr.op >= PG_CMP_CONTAINS && pr.op <= PG_CMP_NOT_CONTAINS2;
        if (varbin && ordering)
            throw std::runtime_error(
                std::string(opname) + ": preds[" + std::to_string(p) +
                "] is an ordering comparison (op " + std::to_string(pr.op) +
                ") on VARBIN column " + std::to_string(pr.col) +
                "; LT/LE/GT/GE are not defined for variable-width columns");
        if (!varbin && string_op)
            throw std::runtime_error(
                std::string(opname) + ": preds[" + std::to_string(p) +
                "] is a string op (" + std::to_string(pr.op) +
                ": CONTAINS/PREFIX/CONTAINS2/NOT_CONTAINS2) on fixed-width "
                "column " + std::to_string(pr.col) +
                "; it needs a VARBIN column");
    }
}

/* stage a (possibly host-resident) page onto the device; staged buffers
 * live for the duration of one call (input pages are borrowed) */
struct StagedPage {
    pg_page pg;
    std::vector<DevBuf> bufs;
    void stage(const pg_page* in)
    {
        pg = *in;
        for (int c = 0; c < in->n_cols; c++) {
            /* a host VARBIN column whose strings are all empty may come
             * with a NULL byte buffer: its offsets, ids and mask are staged
             * all the same */
            const bool host_varbin = in->cols[c].tag == PG_T_VARBIN &&
                                     !in->cols[c].on_device;
            if (!in->cols[c].data && !(host_varbin && in->cols[c].offsets))
                continue;
            if (host_varbin) {
                /* bytes buffer + offsets (n_rows+1, or dict_n+1 for
                 * dictionary blocks) + optional dict ids */
                const int32_t* ho = in->cols[c].offsets;
                int64_t n_elem = in->cols[c].dict_ids ? in->cols[c].dict_n
                                                      : in->n_rows;
                size_t nb = (size_t)ho[n_elem];
                if (nb && !in->cols[c].data)
                    throw std::runtime_error(
                        "VARBIN column " + std::to_string(c) +
                        ": data is NULL but its offsets span " +
                        std::to_string(nb) + " bytes");
                bufs.emplace_back();
                bufs.back().alloc(nb ? nb : 1);
                if (nb)
                    CHKV(hipMemcpyAsync(bufs.back().p, in->cols[c].data, nb,
                                        hipMemcpyHostToDevice, g_stream));
                pg.cols[c].data = bufs.back().p;
                bufs.emplace_back();
                bufs.back().alloc(((size_t)n_elem + 1) * 4);
                CHKV(hipMemcpyAsync(bufs.back().p, ho,
                                    ((size_t)n_elem + 1) * 4,
                                    hipMemcpyHostToDevice, g_stream));
                pg.cols[c].offsets = (const int32_t*)bufs.back().p;
                if (in->cols[c].dict_ids) {
                    bufs.emplace_back();
                    bufs.back().alloc((size_t)in->n_rows * 4);
                    CHKV(hipMemcpyAsync(bufs.back().p, in->cols[c].dict_ids,
                                        (size_t)in->n_rows * 4,
                                        hipMemcpyHostToDevice, g_stream));
                    pg.cols[c].dict_ids = (const int32_t*)bufs.back().p;
                }
                pg.cols[c].on_device = 1;
                if (in->cols[c].null_mask) {
                    bufs.emplace_back();
                    bufs.back().alloc(in->n_rows);
                    CHKV(hipMemcpyAsync(bufs.back().p, in->cols[c].null_mask,
                                        in->n_rows, hipMemcpyHostToDevice,
                                        g_stream));
                    pg.cols[c].null_mask = (const uint8_t*)bufs.back().p;
                }
                continue;
            }
            if (!in->cols[c].on_device) {
                size_t n = (size_t)in->n_rows * type_size(in->cols[c].tag);
                bufs.emplace_back();
                bufs.back().alloc(n);
                CHKV(hipMemcpyAsync(bufs.back().p, in->cols[c].data, n,
                                    hipMemcpyHostToDevice, g_stream));
                pg.cols[c].data = bufs.back().p;
                pg.cols[c].on_device = 1;
                if (in->cols[c].null_mask) {
                    bufs.emplace_back();
                    bufs.back().alloc(in->n_rows);
                    CHKV(hipMemcpyAsync(bufs.back().p, in->cols[c].null_mask,
                                        in->n_rows, hipMemcpyHostToDevice,
                                        g_stream));
                    pg.cols[c].null_mask = (const uint8_t*)bufs.back().p;
                }
            }
        }
    }
};

/* an output page owned by the library */
struct OutPage {
    pg_page pg{};
    std::vector<DevBuf> dev;
    std::vector<std::vector<uint8_t>> host;
};

struct Table {
    int64_t cap = 0, mask = 0, n_rows = 0;
    int64_t local_mask = 0; /* cap_p-1 for partitioned tables, else mask */
    int32_t pack_bits = 0;  /* slot word = key << pack_bits | payload0 */
    bool key_set_only = false;
    DevBuf keys, head, next, tags;
    DevBuf acc; /* per-slot accumulators, acc_words u64 each */
    int32_t acc_words = 0; /* 4 = [dec, flo, fhi, cnt]; 2 = [dec, cnt] */
    /* hit list: the slots whose count went 0 -> 1 since acc was last
     * zeroed, appended by the mode-1 probes (n_rows entries, u32 while
     * cap <= 2^32) so that finish() gathers the groups instead of
     * sweeping acc.  Trusted (list_ok) only while every kernel that added
     * into acc since then also appended. */
    DevBuf hits, hits_n;    /* entries; device cursor (one u64) */
    int64_t hits_cap = 0;   /* entries allocated */
    unsigned long long hits_n_host = 0; /* cursor as of the last probe */
    bool use_hits = true;   /* PG_GROUPS_LIST=0 at build creation: never */
    bool list_ok = false;
    DevBuf acc_multi; /* multi-agg probes: acc_stride u64 per slot
                         (n_acc+1 unpacked; fewer when acc_pack) */
    int32_t n_acc = 0;
    int32_t acc_stride = 0;
    /* the layout acc_multi was allocated for, as the first multi-agg
     * operator declared it (unused entries zero).  A later operator must
     * declare the same one; pg_table_reset_acc keeps it. */
    int32_t acc_packed = 0;
    int32_t acc_shift[6] = {0, 0, 0, 0, 0, 0};
    int32_t acc_width[6] = {0, 0, 0, 0, 0, 0};
    int32_t acc_cnt_shift = 0, acc_cnt_width = 0;
    DevBuf kbits;    /* key-presence bitmap (dynamic-filter analog) */
    int64_t bmax = 0; /* bitmap covers keys [1, bmax]; 0 = none */
    bool range_group = false; /* dense-range group domain [1, cap]:
                                 keys.p stays null, acc index = key-1 */
    bool dense_alloc_pending = false; /* dense payload tag set on first
                                         input page */
    bool slot_payloads = false; /* payloads indexed by slot (agg tables) */
    bool dense = false;          /* dense_array: payload[key-1], no hash */
    /* multi-key chained tables (n_keys >= 1): keys holds the slot words
     * (hash bits | representative row), next the duplicate chains (no
     * head), key_rows n_keys int64 per build row and knull one "any key
     * channel null" byte per build row */
    int32_t n_keys = 0;
    int32_t key_tag[4] = {-1, -1, -1, -1}; /* the first build page's */
    DevBuf knull;
    /* compacted build-row arrays: key + payloads */
    DevBuf key_rows;
    std::vector<DevBuf> payload;
    std::vector<int32_t> ptag;
};

/* acc has just been zeroed (queued on g_stream): the hit list starts over
 * and is trusted again */
static void hits_restart(Table* t)
{
    if (!t->hits.p) return;
    CHKV(hipMemsetAsync(t->hits_n.p, 0, 8, g_stream));
    t->hits_n_host = 0;
    t->list_ok = true;
}

static hit_list hits_arg(const Table* t)
{
    hit_list hl{};
    if (t->list_ok) {
        hl.ents = t->hits.p;
        hl.cursor = (unsigned long long*)t->hits_n.p;
        hl.cap = t->hits_cap;
        hl.wide = t->cap > (1ll << 32);
    }
    return hl;
}

static std::mutex g_mu;
static std::map<int64_t, std::unique_ptr<Table>> g_tables;
static int64_t g_next_table = 1;

struct Op {
    int32_t kind;
    bool finished = false;
    std::deque<OutPage> outq;
    OutPage current; /* last page handed out */
    virtual void add_input(const pg_page* p) = 0;
    virtual void finish() = 0;
    virtual ~Op() = default;
    virtual int64_t table_handle() { return -1; }
    virtual void partition_counts(int64_t*, int32_t)
    {
        throw std::runtime_error("not a partition op");
    }
    const pg_page* pop_output()
    {
        if (outq.empty()) return nullptr;
        current = std::move(outq.front());
        outq.pop_front();
        return &current.pg;
    }
};

static int64_t next_pow2(int64_t x)
{
    int64_t c = 2;
    while (c < x) c <<= 1;
    return c;
}

/* run the selection count+scan+emit pipeline; returns n_selected.
 * outs must be pre-sized by caller after count via the callback. */
struct SelResult {
    int64_t n = 0;
    std::vector<int64_t> block_offs; /* host */
    std::shared_ptr<DevBuf> selbits; /* per-window ballot masks */
};

/* semijoin set arguments: dense sets pass the flag array with a negative
 * mask (-capacity); hash sets pass keys + mask */
static const int64_t* set_ptr(const Table* semi)
{
    if (!semi) return nullptr;
    return semi->dense ? (const int64_t*)semi->payload[0].p
                       : (const int64_t*)semi->keys.p;
}
static int64_t set_mask_of(const Table* semi)
{
    if (!semi) return 0;
    return semi->dense ? -semi->cap : semi->mask;
}

static SelResult sel_count(const pg_page& pg,
                           const pg_plan_filter_project& plan,
                           const Table* semi, int32_t semi_col,
                           int64_t chunk)
{
    DevBuf d_counts;
    d_counts.alloc(FLT_NB * sizeof(int64_t));
    auto selbits = std::make_shared<DevBuf>();
    /* k_sel_emit reads the mask word of all four waves of every 256-row
     * window it enters, the last (partial) one included */
    selbits->alloc(((size_t)(pg.n_rows + 255) / 256 * 4 + 1) * 8);
    hipLaunchKernelGGL(k_sel_count, dim3(FLT_NB), dim3(256), 0, g_stream, pg,
                       plan, chunk, (int64_t*)d_counts.p, set_ptr(semi),
                       set_mask_of(semi), semi_col,
                       (unsigned long long*)selbits->p);
    std::vector<int64_t> h(FLT_NB);
    CHKV(hipMemcpyAsync(h.data(), d_counts.p, FLT_NB * 8,
                        hipMemcpyDeviceToHost, g_stream));
    CHKV(hipStreamSynchronize(g_stream));
    SelResult r;
    r.selbits = selbits;
    r.block_offs.resize(FLT_NB);
    for (int b = 0; b < FLT_NB; b++) {
        r.block_offs[b] = r.n;
        r.n += h[b];
    }
    return r;
}

static int64_t sel_chunk(int64_t n)
{
    int64_t chunk = (n + FLT_NB - 1) / FLT_NB;
    return (chunk + 255) / 256 * 256 > 256 ? (chunk + 255) / 256 * 256 : 256;
}

static void sel_emit(const pg_page& pg, const pg_plan_filter_project& plan,
                     const Table* semi, int32_t semi_col, int64_t chunk,
                     const SelResult& r, const emit_outs& outs)
{
    DevBuf d_offs;
    d_offs.alloc(FLT_NB * sizeof(int64_t));
    CHKV(hipMemcpyAsync(d_offs.p, r.block_offs.data(), FLT_NB * 8,
                        hipMemcpyHostToDevice, g_stream));
    hipLaunchKernelGGL(k_sel_emit, dim3(FLT_NB), dim3(256), 0, g_stream, pg,
                       plan, chunk, (const int64_t*)d_offs.p, outs,
                       set_ptr(semi), set_mask_of(semi), semi_col,
                       r.selbits ? (const unsigned long long*)r.selbits->p
                                 : nullptr);
    CHKV(hipStreamSynchronize(g_stream));
}

/* the key channels of a multi-key build or probe page: U8 / I32 / I64
 * columns, typed as on the operator's first page (first_tag[k] < 0 until
 * one was fed).  Throws before anything is staged or launched. */
static void check_multikey_cols(const char* opname, int n_keys,
                                const int32_t* key_cols, const pg_page* in,
                                const int32_t* first_tag)
{
    for (int k = 0; k < n_keys; k++) {
        const int32_t c = key_cols[k];
        const std::string name = std::string(opname) + ": key_cols[" +
                                 std::to_string(k) + "] (column " +
                                 std::to_string(c) + ")";
        if (c < 0 || c >= in->n_cols)
            throw std::runtime_error(
                name + " is outside the page's " +
                std::to_string(in->n_cols) + " columns");
        const pg_col& col = in->cols[c];
        const char* what = nullptr;
        if (col.tag == PG_T_VARBIN)
            what = col.dict_ids ? "a dictionary column (ids of two "
                                  "dictionaries are not comparable)"
                                : "a VARBIN column";
        else if (col.tag == PG_T_F64)
            what = "an F64 column";
        else if (col.tag == PG_T_I128)
            what = "an I128 column";
        else if (col.tag != PG_T_U8 && col.tag != PG_T_I32 &&
                 col.tag != PG_T_I64)
            what = "of an unknown column type";
        if (what)
            throw std::runtime_error(name + " is " + what +
                                     ": join keys are U8, I32 or I64");
        if (first_tag[k] >= 0 && first_tag[k] != col.tag)
            throw std::runtime_error(
                name + ": type " + std::to_string(col.tag) +
                " differs from the first page's " +
                std::to_string(first_tag[k]));
    }
}

/* a multi-key table keeps slot words where the others keep keys: it serves
 * multi-key LOOKUP_JOINs only */
static void reject_multikey(const Table* t, const char* role)
{
    if (t && t->n_keys)
        throw std::runtime_error(
            std::string("a multi-key (n_keys >= 1) table cannot serve as ") +
            role);
}

/* ---------------- FILTER_PROJECT ---------------- */
struct FilterOp : Op {
    pg_plan_filter_project plan;
    void init()
    {
        check_pred_lens("FILTER_PROJECT", plan.preds,
                        preds_used(plan.n_preds));
    }
    void add_input(const pg_page* in) override
    {
        check_pred_types("FILTER_PROJECT", plan.preds,
                         preds_used(plan.n_preds), in);
        StagedPage sp;
        sp.stage(in);
        const Table* semi = nullptr;
        if (plan.semijoin_table > 0) {
            std::lock_guard<std::mutex> lk(g_mu);
            auto it = g_tables.find(plan.semijoin_table);
            if (it == g_tables.end())
                throw std::runtime_error("semijoin table not found");
            semi = it->second.get();
            reject_multikey(semi, "a semijoin_table");
        }
        int64_t chunk = sel_chunk(sp.pg.n_rows);
        SelResult r = sel_count(sp.pg, plan, semi, plan.semijoin_col, chunk);
        OutPage op;
        op.pg.n_rows = r.n;
        op.pg.n_cols = plan.n_proj;
        emit_outs outs{};
        outs.n = plan.n_proj;
        pg_plan_filter_project ep = plan; /* VARBIN slots -> ROWID emit */
        std::vector<int> vb_cols;
        for (int o = 0; o < plan.n_proj; o++) {
            int tag = plan.proj[o].kind == PG_PROJ_IDENT
                          ? sp.pg.cols[plan.proj[o].a].tag
                      : (plan.proj[o].kind == PG_PROJ_KEYSHL ||
                         plan.proj[o].kind == PG_PROJ_SHR ||
                         plan.proj[o].kind == PG_PROJ_SUBDIV ||
                         plan.proj[o].kind == PG_PROJ_KEYSHL_DIV)
                          ? PG_T_I64
                          : PG_T_F64;
            if (tag == PG_T_VARBIN) {
                /* pass 1 emits the source row index; pass 2 gathers the
                 * variable-width bytes (see k_varbin_len/gather) */
                vb_cols.push_back(o);
                ep.proj[o].kind = PG_PROJ_ROWID;
                op.dev.emplace_back();
                op.dev.back().alloc((size_t)r.n * 8 + 8);
                outs.ptr[o] = op.dev.back().p;
                outs.tag[o] = PG_T_I64;
                op.pg.cols[o].tag = PG_T_VARBIN;
                continue;
            }
            op.dev.emplace_back();
            op.dev.back().alloc((size_t)r.n * type_size(tag));
            op.pg.cols[o].tag = tag;
            op.pg.cols[o].on_device = 1;
            op.pg.cols[o].data = op.dev.back().p;
            op.pg.cols[o].null_mask = nullptr;
            outs.ptr[o] = op.dev.back().p;
            outs.tag[o] = tag;
        }
        sel_emit(sp.pg, ep, semi, plan.semijoin_col, chunk, r, outs);
        for (int o : vb_cols) {
            const pg_col& src = sp.pg.cols[plan.proj[o].a];
            const int64_t* rowid = (const int64_t*)outs.ptr[o];
            DevBuf d_len;
            d_len.alloc((size_t)r.n * 4 + 4);
            hipLaunchKernelGGL(k_varbin_len, dim3(2048), dim3(256), 0,
                               g_stream, rowid, r.n, src.offsets,
                               src.dict_ids, (int32_t*)d_len.p);
            std::vector<int32_t> h_len(r.n);
            if (r.n)
                CHKV(hipMemcpyAsync(h_len.data(), d_len.p, (size_t)r.n * 4,
                                    hipMemcpyDeviceToHost, g_stream));
            CHKV(hipStreamSynchronize(g_stream));
            std::vector<int32_t> h_offs(r.n + 1);
            h_offs[0] = 0;
            int64_t total_bytes = 0; /* offsets are 32-bit: checked below */
            for (int64_t j = 0; j < r.n; j++) {
                total_bytes += h_len[j];
                if (total_bytes > INT32_MAX)
                    throw std::runtime_error(
                        "FILTER_PROJECT: VARBIN output column " +
                        std::to_string(o) + " exceeds 2^31-1 bytes (32-bit "
                        "offsets); feed smaller pages");
                h_offs[j + 1] = (int32_t)total_bytes;
            }
            op.dev.emplace_back(); /* offsets */
            op.dev.back().alloc(((size_t)r.n + 1) * 4);
            void* offs_p = op.dev.back().p;
            CHKV(hipMemcpyAsync(offs_p, h_offs.data(),
                                ((size_t)r.n + 1) * 4, hipMemcpyHostToDevice,
                                g_stream));
            op.dev.emplace_back(); /* bytes */
            op.dev.back().alloc((size_t)h_offs[r.n] + 1);
            void* bytes_p = op.dev.back().p;
            hipLaunchKernelGGL(k_varbin_gather, dim3(2048), dim3(256), 0,
                               g_stream, rowid, r.n,
                               (const uint8_t*)src.data, src.offsets,
                               src.dict_ids, (const int32_t*)offs_p,
                               (uint8_t*)bytes_p);
            CHKV(hipStreamSynchronize(g_stream));
            op.pg.cols[o].on_device = 1;
            op.pg.cols[o].data = bytes_p;
            op.pg.cols[o].offsets = (const int32_t*)offs_p;
            op.pg.cols[o].null_mask = nullptr;
        }
        outq.push_back(std::move(op));
    }
    void finish() override {}
};

/* ---------------- HASH_AGG_SMALL ---------------- */
struct AggSmallOp : Op {
    pg_plan_hash_agg_small plan; /* with internal count agg appended */
    int user_aggs = 0;
    bool dec = false;
    int n_groups = 0, na = 0, maxg = 0;
    DevBuf partials; /* + trailing bad-key flag, see bad_ptr() */
    void init()
    {
        if (plan.n_aggs < 1 || plan.n_aggs >= PG_MAX_AGG)
            throw std::runtime_error("n_aggs must be in [1, 7]");
        check_pred_lens("HASH_AGG_SMALL", plan.preds,
                        preds_used(plan.n_preds));
        user_aggs = plan.n_aggs;
        /* internal presence count */
        pg_agg cnt{};
        cnt.func = PG_AGG_COUNT;
        plan.aggs[plan.n_aggs++] = cnt;
        dec = false;
        for (int a = 0; a < user_aggs; a++) {
            if (plan.aggs[a].func == PG_AGG_SUM_DEC ||
                plan.aggs[a].func == PG_AGG_SUM_I64)
                dec = true;
        }
        for (int a = 0; a < user_aggs; a++) {
            int32_t fn = plan.aggs[a].func;
            bool both = fn == PG_AGG_COUNT || fn == PG_AGG_MIN ||
                        fn == PG_AGG_MAX;
            bool adec = both || fn == PG_AGG_SUM_DEC ||
                        fn == PG_AGG_SUM_I64;
            bool af64 = both || fn == PG_AGG_SUM_F64;
            if (dec ? !adec : !af64)
                throw std::runtime_error(
                    "mixed decimal/f64 aggregates in one op unsupported");
        }
        n_groups = plan.n_keys == 0
                       ? 1
                       : plan.n_vals[0] *
                             (plan.n_keys == 2 ? plan.n_vals[1] : 1);
        static const int NAS[] = {2, 4, 7, 9};
        static const int MGS[] = {2, 4, 6, 8};
        for (int x : NAS)
            if (plan.n_aggs <= x) {
                na = x;
                break;
            }
        for (int x : MGS)
            if (n_groups <= x) {
                maxg = x;
                break;
            }
        if (!na || !maxg)
            throw std::runtime_error("agg plan exceeds kernel limits");
        /* one allocation: [partials | bad flag] (fewer alloc/memset/launch
         * round trips per operator lifecycle) */
        partials.alloc((size_t)FT_NBLOCKS * na * maxg * 8 + 64);
        partials.zero(); /* zero covers sums/counts + the bad flag */
        bool has_mm = false;
        for (int a = 0; a < plan.n_aggs; a++)
            has_mm = has_mm || plan.aggs[a].func == PG_AGG_MIN ||
                     plan.aggs[a].func == PG_AGG_MAX;
        if (has_mm) {
            agg_funcs fns = funcs();
            if (dec)
                hipLaunchKernelGGL(k_agg_partials_init<true>, dim3(512),
                                   dim3(256), 0, g_stream, nullptr,
                                   (int64_t*)partials.p, fns,
                                   (int64_t)FT_NBLOCKS * na * maxg, na);
            else
                hipLaunchKernelGGL(k_agg_partials_init<false>, dim3(512),
                                   dim3(256), 0, g_stream,
                                   (double*)partials.p, nullptr, fns,
                                   (int64_t)FT_NBLOCKS * na * maxg, na);
        }
    }
    agg_funcs funcs() const
    {
        agg_funcs f{};
        f.maxg = maxg;
        for (int a = 0; a < 12; a++)
            f.f[a] = a < plan.n_aggs ? plan.aggs[a].func : PG_AGG_COUNT;
        return f;
    }
    void* bad_ptr() const
    {
        return (int8_t*)partials.p + (size_t)FT_NBLOCKS * na * maxg * 8;
    }
    bool q1_shape(const pg_page& pg) const
    {
        const pg_plan_hash_agg_small& p = plan;
        if (user_aggs != 6 || p.n_keys != 2 || p.n_vals[0] != 3 ||
            p.n_vals[1] != 2 || p.n_preds != 1)
            return false;
        if (na != 7 || maxg != 6) return false;
        if (pg.cols[p.preds[0].col].tag != PG_T_I32 ||
            p.preds[0].op != PG_CMP_LE || p.preds[0].rhs_col != 0)
            return false;
        const pg_agg* a = p.aggs;
        if (!(a[0].proj.kind == PG_PROJ_IDENT &&
              a[1].proj.kind == PG_PROJ_IDENT &&
              a[2].proj.kind == PG_PROJ_DISC_PRICE &&
              a[3].proj.kind == PG_PROJ_CHARGE &&
              a[4].proj.kind == PG_PROJ_IDENT && a[5].func == PG_AGG_COUNT))
            return false;
        /* the kernel computes five SUMs and a count: MIN/MAX (or a
         * count) in a sum slot takes the generic kernel */
        for (int i = 0; i < 5; i++) {
            int32_t fn = a[i].func;
            if (dec ? !(fn == PG_AGG_SUM_DEC || fn == PG_AGG_SUM_I64)
                    : fn != PG_AGG_SUM_F64)
                return false;
        }
        /* it always reports unlisted keys and never reads a null mask */
        if (p.drop_unlisted_keys) return false;
        if (a[2].proj.a != a[1].proj.a || a[3].proj.a != a[1].proj.a ||
            a[3].proj.b != a[2].proj.b || a[4].proj.a != a[2].proj.b)
            return false;
        if (dec && !(a[0].dec_scale == 0 && a[1].dec_scale == 2 &&
                     a[4].dec_scale == 2))
            return false;
        /* all four money channels must be f64 and 16-byte aligned */
        int chans[4] = {a[0].proj.a, a[1].proj.a, a[2].proj.b, a[3].proj.c};
        for (int i = 0; i < 4; i++) {
            const pg_col& c = pg.cols[chans[i]];
            if (c.tag != PG_T_F64 || ((uintptr_t)c.data & 15)) return false;
            if (c.null_mask) return false;
        }
        if (((uintptr_t)pg.cols[p.preds[0].col].data & 7)) return false;
        if (pg.cols[p.key_col[0]].tag != PG_T_U8 ||
            pg.cols[p.key_col[1]].tag != PG_T_U8)
            return false;
        if (pg.cols[p.preds[0].col].null_mask ||
            pg.cols[p.key_col[0]].null_mask ||
            pg.cols[p.key_col[1]].null_mask)
            return false;
        return true;
    }
    void launch_q1(const pg_page& pg)
    {
        static int var = -1;
        if (var < 0) {
            const char* e = getenv("PG_Q1_VARIANT");
            var = e ? atoi(e) : 1; /* nontemporal default: +17% measured */
        }
        const pg_plan_hash_agg_small& p = plan;
        g_q1_fast_launches++;
        const double* qty = (const double*)pg.cols[p.aggs[0].proj.a].data;
        const double* ep = (const double*)pg.cols[p.aggs[1].proj.a].data;
        const double* dc = (const double*)pg.cols[p.aggs[2].proj.b].data;
        const double* tx = (const double*)pg.cols[p.aggs[3].proj.c].data;
        const int32_t* sd = (const int32_t*)pg.cols[p.preds[0].col].data;
        const uint8_t* rf = (const uint8_t*)pg.cols[p.key_col[0]].data;
        const uint8_t* ls = (const uint8_t*)pg.cols[p.key_col[1]].data;
#define LAUNCH_Q1(D, V)                                                  \
    hipLaunchKernelGGL((k_agg_q1<D, V>), dim3(FT_NBLOCKS),               \
                       dim3(FT_NTHREADS), 0, g_stream, qty, ep, dc, tx,  \
                       sd, rf, ls, pg.n_rows, (int32_t)p.preds[0].ival,  \
                       p.key_vals[0][0], p.key_vals[0][1],               \
                       p.key_vals[0][2], p.key_vals[1][0],               \
                       p.key_vals[1][1],                                 \
                       D ? nullptr : (double*)partials.p,                \
                       D ? (int64_t*)partials.p : nullptr,               \
                       (unsigned long long*)bad_ptr())
        if (dec) {
            if (var == 1) LAUNCH_Q1(true, 1);
            else if (var == 2) LAUNCH_Q1(true, 2);
            else LAUNCH_Q1(true, 0);
        } else {
            if (var == 1) LAUNCH_Q1(false, 1);
            else if (var == 2) LAUNCH_Q1(false, 2);
            else LAUNCH_Q1(false, 0);
        }
#undef LAUNCH_Q1
    }
    template <int NA, int MAXG>
    void launch2(const pg_page& pg)
    {
        if (dec)
            hipLaunchKernelGGL((k_agg_small<NA, MAXG, true>),
                               dim3(FT_NBLOCKS), dim3(FT_NTHREADS), 0,
                               g_stream, pg, plan, nullptr,
                               (int64_t*)partials.p,
                               (unsigned long long*)bad_ptr());
        else
            hipLaunchKernelGGL((k_agg_small<NA, MAXG, false>),
                               dim3(FT_NBLOCKS), dim3(FT_NTHREADS), 0,
                               g_stream, pg, plan, (double*)partials.p,
                               nullptr, (unsigned long long*)bad_ptr());
    }
    void add_input(const pg_page* in) override
    {
        check_pred_types("HASH_AGG_SMALL", plan.preds,
                         preds_used(plan.n_preds), in);
        StagedPage sp;
        sp.stage(in);
        hot_begin();
        if (q1_shape(sp.pg)) {
            launch_q1(sp.pg);
            hot_end();
            CHKV(hipStreamSynchronize(g_stream));
            return;
        }
        switch (na * 16 + maxg) {
            case 2 * 16 + 2: launch2<2, 2>(sp.pg); break;
            case 2 * 16 + 4: launch2<2, 4>(sp.pg); break;
            case 2 * 16 + 6: launch2<2, 6>(sp.pg); break;
            case 2 * 16 + 8: launch2<2, 8>(sp.pg); break;
            case 4 * 16 + 2: launch2<4, 2>(sp.pg); break;
            case 4 * 16 + 4: launch2<4, 4>(sp.pg); break;
            case 4 * 16 + 6: launch2<4, 6>(sp.pg); break;
            case 4 * 16 + 8: launch2<4, 8>(sp.pg); break;
            case 7 * 16 + 2: launch2<7, 2>(sp.pg); break;
            case 7 * 16 + 4: launch2<7, 4>(sp.pg); break;
            case 7 * 16 + 6: launch2<7, 6>(sp.pg); break;
            case 7 * 16 + 8: launch2<7, 8>(sp.pg); break;
            case 9 * 16 + 2: launch2<9, 2>(sp.pg); break;
            case 9 * 16 + 4: launch2<9, 4>(sp.pg); break;
            case 9 * 16 + 6: launch2<9, 6>(sp.pg); break;
            default: launch2<9, 8>(sp.pg); break;
        }
        hot_end(); /* waits for the kernel via its trailing event */
        if (!sp.bufs.empty()) CHKV(hipStreamSynchronize(g_stream));
    }
    void finish() override
    {
        int nm = na * maxg;
        DevBuf out_f, out_hi, out_lo;
        out_f.alloc(nm * 8);
        out_hi.alloc(nm * 8);
        out_lo.alloc(nm * 8);
        if (dec)
            hipLaunchKernelGGL(k_agg_small_finish<true>, dim3(nm),
                               dim3(WAVE), 0, g_stream, nullptr,
                               (int64_t*)partials.p, nm, nullptr,
                               (int64_t*)out_hi.p, (uint64_t*)out_lo.p,
                               funcs());
        else
            hipLaunchKernelGGL(k_agg_small_finish<false>, dim3(nm),
                               dim3(WAVE), 0, g_stream,
                               (double*)partials.p, nullptr, nm,
                               (double*)out_f.p, nullptr, nullptr,
                               funcs());
        std::vector<double> hf(nm);
        std::vector<int64_t> hhi(nm);
        std::vector<uint64_t> hlo(nm);
        unsigned long long hbad[2] = {0, 0};
        CHKV(hipMemcpyAsync(hf.data(), out_f.p, nm * 8, hipMemcpyDeviceToHost,
                            g_stream));
        CHKV(hipMemcpyAsync(hhi.data(), out_hi.p, nm * 8,
                            hipMemcpyDeviceToHost, g_stream));
        CHKV(hipMemcpyAsync(hlo.data(), out_lo.p, nm * 8,
                            hipMemcpyDeviceToHost, g_stream));
        CHKV(hipMemcpyAsync(hbad, bad_ptr(), 16, hipMemcpyDeviceToHost,
                            g_stream));
        CHKV(hipStreamSynchronize(g_stream));
        if (hbad[0])
            throw std::runtime_error(
                "group key value outside plan enumeration");
        if (hbad[1])
            throw std::runtime_error(
                "bigint/decimal SUM overflow (Math.addExact semantics, "
                "LongSumAggregation.java:33-37)");
        /* a SUM(bigint)'s 128-bit total past int64 range is the same
         * overflow Presto raises on */
        for (int a = 0; a < user_aggs; a++)
            if (dec && plan.aggs[a].func == PG_AGG_SUM_I64)
                for (int g = 0; g < n_groups; g++) {
                    int64_t hi = hhi[a * maxg + g];
                    int64_t lo = (int64_t)hlo[a * maxg + g];
                    if (hi != (lo < 0 ? -1 : 0))
                        throw std::runtime_error(
                            "BIGINT sum overflow (Math.addExact semantics, "
                            "LongSumAggregation.java:33-37)");
                }
        /* presence from internal count agg (index user_aggs) */
        int ic = user_aggs;
        auto cnt_of = [&](int g) -> int64_t {
            return dec ? (int64_t)hlo[ic * maxg + g]
                       : (int64_t)hf[ic * maxg + g];
        };
        int n_out = 0;
        for (int g = 0; g < n_groups; g++)
            if (cnt_of(g) > 0) n_out++;
        /* host page: key cols then per-agg cols */
        OutPage op;
        op.pg.n_rows = n_out;
        int nc = 0;
        auto add_host_col = [&](int tag) {
            op.host.emplace_back((size_t)n_out * type_size(tag));
            op.pg.cols[nc].tag = tag;
            op.pg.cols[nc].on_device = 0;
            op.pg.cols[nc].data = op.host.back().data();
            op.pg.cols[nc].null_mask = nullptr;
            return nc++;
        };
        int c_k0 = plan.n_keys >= 1 ? add_host_col(PG_T_U8) : -1;
        int c_k1 = plan.n_keys == 2 ? add_host_col(PG_T_U8) : -1;
        std::vector<int> agg_col(user_aggs);
        std::vector<int> agg_col2(user_aggs, -1);
        for (int a = 0; a < user_aggs; a++) {
            if (dec && plan.aggs[a].func != PG_AGG_COUNT) {
                agg_col[a] = add_host_col(PG_T_I64); /* hi */
                agg_col2[a] = add_host_col(PG_T_I64); /* lo */
            } else if (plan.aggs[a].func == PG_AGG_COUNT) {
                agg_col[a] = add_host_col(PG_T_I64);
            } else {
                agg_col[a] = add_host_col(PG_T_F64);
            }
        }
        op.pg.n_cols = nc;
        int row = 0;
        for (int g = 0; g < n_groups; g++) {
            if (cnt_of(g) <= 0) continue;
            int i0 = plan.n_keys == 2 ? g / plan.n_vals[1] : g;
            int i1 = plan.n_keys == 2 ? g % plan.n_vals[1] : 0;
            if (c_k0 >= 0)
                ((uint8_t*)op.pg.cols[c_k0].data)[row] = plan.key_vals[0][i0];
            if (c_k1 >= 0)
                ((uint8_t*)op.pg.cols[c_k1].data)[row] =
                    plan.key_vals[1][i1];
            for (int a = 0; a < user_aggs; a++) {
                if (plan.aggs[a].func == PG_AGG_COUNT) {
                    ((int64_t*)op.pg.cols[agg_col[a]].data)[row] = cnt_of(g);
                } else if (dec) {
                    ((int64_t*)op.pg.cols[agg_col[a]].data)[row] =
                        hhi[a * maxg + g];
                    ((int64_t*)op.pg.cols[agg_col2[a]].data)[row] =
                        (int64_t)hlo[a * maxg + g];
                } else {
                    ((double*)op.pg.cols[agg_col[a]].data)[row] =
                        hf[a * maxg + g];
                }
            }
            row++;
        }
        outq.push_back(std::move(op));
    }
};

/* ---------------- HASH_BUILD ---------------- */
/* grid for persistent kernels: exactly one 256-thread block per CU so a
 * hand-rolled grid barrier can never strand a non-resident block */
static int persistent_grid()
{
    /* 4 blocks of 256 threads per CU: enough latency hiding for the CAS
     * chains, still guaranteed-resident for the grid barrier (8/CU is
     * the hardware cap at <=80 sgprs; 4 leaves margin) */
    static int nb = 0;
    if (!nb) {
        hipDeviceProp_t p{};
        int cus = 0;
        if (hipGetDeviceProperties(&p, 0) == hipSuccess)
            cus = p.multiProcessorCount;
        if (cus <= 0) cus = 64;
        if (cus > 256) cus = 256;
        nb = cus * 4;
        const char* e = getenv("PG_PART_NB");
        if (e && atoi(e) > 0) nb = atoi(e);
    }
    return nb;
}

struct BuildOp : Op {
    pg_plan_hash_build plan;
    int64_t tbl = -1;
    std::unique_ptr<Table> t;
    int64_t cap_rows = 0;
    DevBuf counters; /* direct mode: [inserted, overflow, stage_ovf] */
    /* radix-partitioned agg build (tables too big for cache-resident
     * random stores): staging + cursors + barrier counter */
    bool part = false;
    int32_t P = 1, Kact = 1, capp_bits = 0;
    DevBuf stage, cursorb, barb;
    bool staged = true; /* direct builds may use k_tbl_insert_staged */
    /* does this page of a direct agg_table build fit the staged insert
     * kernel?  Fills its arguments when it does; everything else stays on
     * k_tbl_insert_direct. */
    bool staged_fit(const pg_page& pg, const Table* semi, const Table* lu,
                    staged_args* sa) const
    {
        auto vec_i64 = [](const pg_col& c) {
            return c.tag == PG_T_I64 && !c.null_mask &&
                   ((uintptr_t)c.data & 15) == 0;
        };
        if (!staged || plan.pack_bits <= 0 || plan.n_payload != 1)
            return false;
        if (plan.n_preds < 0 || plan.n_preds > 2) return false;
        staged_args a{};
        a.n = pg.n_rows;
        a.n_preds = plan.n_preds;
        for (int p = 0; p < plan.n_preds; p++) {
            const pg_pred& pr = plan.preds[p];
            const pg_col& c = pg.cols[pr.col];
            if (pr.rhs_col != 0 || pr.op < PG_CMP_LT || pr.op > PG_CMP_NE ||
                c.tag != PG_T_I32 || c.null_mask ||
                ((uintptr_t)c.data & 15) != 0)
                return false;
            a.pc[p] = (const int32_t*)c.data;
            a.pval[p] = pr.ival;
            a.pop[p] = pr.op;
        }
        const pg_col& kc = pg.cols[plan.key_col];
        if (!vec_i64(kc)) return false;
        a.key = (const int64_t*)kc.data;
        if (semi) {
            const pg_col& sc = pg.cols[plan.semijoin_col];
            if (!semi->dense || semi->ptag.empty() ||
                semi->ptag[0] != PG_T_U8 || !vec_i64(sc))
                return false;
            a.sk = (const int64_t*)sc.data;
            a.flags = (const uint8_t*)semi->payload[0].p;
            a.nflags = semi->cap;
        }
        a.pay_pred = -1;
        if (lu) {
            const pg_col& lc = pg.cols[plan.payload_lookup_key_col];
            if (!lu->dense || !vec_i64(lc)) return false; /* u8: checked */
            a.lk = (const int64_t*)lc.data;
            a.lu = (const uint8_t*)lu->payload[0].p;
            a.lucap = lu->cap;
        } else {
            const pg_col& pc = pg.cols[plan.payload_col[0]];
            if (pc.tag != PG_T_I32 && pc.tag != PG_T_U8 &&
                pc.tag != PG_T_I64)
                return false;
            a.pay = pc.data;
            a.pay_tag = pc.tag;
            for (int p = 0; p < plan.n_preds; p++)
                if (plan.preds[p].col == plan.payload_col[0]) a.pay_pred = p;
        }
        *sa = a;
        return true;
    }
    void init()
    {
        check_pred_lens("HASH_BUILD", plan.preds, preds_used(plan.n_preds));
        if (plan.n_keys < 0 || plan.n_keys > 4)
            throw std::runtime_error(
                "HASH_BUILD: n_keys must be 0..4, got " +
                std::to_string(plan.n_keys));
        if (plan.n_keys >= 1) {
            /* a multi-key table is a chained one and nothing else */
            const char* bad =
                plan.agg_table              ? "agg_table"
                : plan.dense_array          ? "dense_array"
                : plan.range_group          ? "range_group"
                : plan.key_set_only         ? "key_set_only"
                : plan.pack_bits            ? "pack_bits"
                : plan.fill_x10             ? "fill_x10"
                : plan.bitmap_max_key       ? "bitmap_max_key"
                : plan.payload_lookup_table ? "payload_lookup_table"
                                            : nullptr;
            if (bad)
                throw std::runtime_error(
                    std::string("HASH_BUILD: n_keys >= 1 builds a multi-key "
                                "chained table and cannot be combined "
                                "with ") + bad);
            for (int k = 0; k < plan.n_keys; k++)
                if (plan.key_cols[k] < 0)
                    throw std::runtime_error(
                        "HASH_BUILD: n_keys = " +
                        std::to_string(plan.n_keys) + " but key_cols[" +
                        std::to_string(k) + "] is negative");
            if (plan.n_payload < 0 || plan.n_payload > 4)
                throw std::runtime_error(
                    "HASH_BUILD: n_keys >= 1 takes n_payload 0..4");
        }
        t.reset(new Table());
        t->key_set_only = plan.key_set_only != 0;
        /* PG_GROUPS_LIST=0 keeps group extraction on the accumulator scan */
        if (const char* eg = getenv("PG_GROUPS_LIST"))
            t->use_hits = atoi(eg) != 0;
        /* the single-scan builds evaluate comparisons only (see
         * d_eval_preds); chained builds filter through the selection
         * path, which knows the null tests */
        if (plan.dense_array || plan.agg_table)
            for (int p = 0; p < plan.n_preds && p < PG_MAX_PRED; p++)
                if (plan.preds[p].op >= PG_CMP_IS_NULL)
                    throw std::runtime_error(
                        "IS NULL / IS NOT NULL predicates are not "
                        "supported on dense_array and agg_table builds "
                        "(filter ahead of the build, or use a chained "
                        "build)");
        if (plan.range_group) {
            if (plan.capacity_hint <= 0)
                throw std::runtime_error(
                    "range_group needs capacity_hint = max key");
            t->range_group = true;
            t->slot_payloads = true; /* unique "rows" = the range */
            t->cap = plan.capacity_hint;
            t->mask = t->cap - 1;       /* bound, not a hash mask */
            t->local_mask = t->mask;
            return;
        }
        if (plan.dense_array) {
            if (plan.n_payload != 1 && !plan.key_set_only)
                throw std::runtime_error(
                    "dense_array needs one u8 payload (or key_set_only)");
            t->dense = true;
            t->cap = plan.capacity_hint;
            t->payload.emplace_back();
            /* payload tag resolved on first add_input (U8 or I32 —
             * an I32 dense payload doubles as the presence flag, so
             * its values must be nonzero; U8 flag sets stay as-is) */
            t->ptag.push_back(PG_T_U8);
            t->dense_alloc_pending = true;
            if (plan.key_set_only) {
                t->payload.back().alloc((size_t)t->cap);
                t->payload.back().zero();
                t->dense_alloc_pending = false;
            }
            return;
        }
        if (plan.agg_table) {
            /* direct mode: size the table now from the hint; payloads
             * live per slot */
            t->slot_payloads = true;
            if (plan.pack_bits) {
                if (plan.n_payload != 1 || plan.pack_bits < 1 ||
                    plan.pack_bits > 32)
                    throw std::runtime_error(
                        "pack_bits needs exactly one payload and "
                        "1..32 bits");
                t->pack_bits = plan.pack_bits;
            }
            /* fill <= ~0.5 by default: linear-probe cluster length is
             * what the 324M-probe miss path pays for (measured: x1.3
             * sizing cost ~0.7 ms of Q3 probe); override via PG_CAP_X10 */
            int64_t mult10 = plan.fill_x10 >= 11 ? plan.fill_x10 : 20;
            if (const char* em = getenv("PG_CAP_X10"))
                if (atoi(em) >= 11) mult10 = atoi(em);
            int64_t cap = next_pow2(plan.capacity_hint * mult10 / 10 + 16);
            t->cap = cap;
            t->mask = cap - 1;
            t->local_mask = cap - 1;
            t->keys.alloc((size_t)cap * 8);
            /* partitioned build once the random-store working set leaves
             * the 256 MiB L3 (see k_part_scatter/insert) */
            /* A/B-measured up to 150M inserts / 2 GB tables: the direct
             * random insert WINS OR TIES at every size this hardware can
             * hold (not a locality effect: the generic kernel was bound
             * by its per-row evaluation chain), so
             * the radix path engages only beyond measured scales; it
             * stays parity-tested and selectable via PG_PART_MIN_SLOTS */
            int64_t part_min = 512ll << 20;
            if (const char* ep = getenv("PG_PART_MIN_SLOTS"))
                if (atoll(ep) > 0) part_min = atoll(ep);
            part = cap >= part_min;
            /* PG_BUILD_STAGED=0 keeps every page on k_tbl_insert_direct */
            staged = true;
            if (const char* es = getenv("PG_BUILD_STAGED"))
                staged = atoi(es) != 0;
            /* byte tags reject probe misses from a cap-sized L3-resident
             * array (8x denser than the key lines).  For partitioned
             * builds the tag store lands in the L3-resident region wave
             * (nearly free), so enable them there unconditionally.
             * A tight fill_x10 declares always-hit probes (no misses to
             * reject): skip the tag array and its random stores.
             * A key bitmap is an exact membership test (a bit is set if
             * and only if the key went in; keys outside its range raise),
             * so a probe that passed it is a hit and the tags could
             * reject nothing: a non-partitioned build with a bitmap skips
             * them as well. */
            bool always_hit = plan.fill_x10 >= 11 && plan.fill_x10 < 20;
            bool exact_bitmap = !part && plan.bitmap_max_key > 0;
            if (!always_hit && !exact_bitmap &&
                (part || cap >= (64ll << 20))) {
                t->tags.alloc((size_t)cap);
                if (!part) t->tags.zero(); /* part: k_part_insert inits */
            }
            /* acc is allocated lazily by the first mode-1 probe (mode-2
             * and emit probes never touch it — at SF300 the slot_acc
             * array is 8 GB of alloc+memset otherwise) */
            counters.alloc(40); /* [+4] = bitmap-range errors */
            counters.zero();
            if (plan.bitmap_max_key > 0) {
                t->bmax = plan.bitmap_max_key;
                t->kbits.alloc((size_t)((t->bmax >> 6) + 1) * 8);
                t->kbits.zero();
            }
            if (part) {
                /* P=256 keeps the scatter's per-row LDS counter atomics
                 * nearly conflict-free (≈1 lane per counter per wave) */
                P = 256;
                while (cap / P < (64ll << 10)) P >>= 1;
                int64_t slot_bytes = 8 + (t->tags.p ? 1 : 0) +
                                     8ll * plan.n_payload;
                /* K regions in flight, bounded by ~half the L3 */
                int64_t region_bytes = cap / P * slot_bytes;
                Kact = (int32_t)((128ll << 20) / region_bytes);
                if (Kact < 1) Kact = 1;
                if (Kact > P) Kact = P;
                const char* ek = getenv("PG_PART_K"); /* tuning knob */
                if (ek && atoi(ek) > 0) {
                    Kact = atoi(ek);
                    if (Kact > P) Kact = P;
                }
                int64_t cap_p = cap / P;
                capp_bits = 0;
                while ((1ll << capp_bits) < cap_p) capp_bits++;
                t->local_mask = cap_p - 1;
                int32_t r_words = 1 + plan.n_payload;
                stage.alloc((size_t)cap * r_words * 8);
                cursorb.alloc((size_t)P * 8);
                cursorb.zero();
                barb.alloc(8);
                barb.zero();
            } else {
                hipLaunchKernelGGL(k_tbl_init, dim3(1024), dim3(256), 0,
                                   g_stream, (int64_t*)t->keys.p, nullptr,
                                   cap);
            }
            for (int i = 0; i < plan.n_payload; i++) {
                t->payload.emplace_back();
                t->ptag.push_back(-1);
                /* packed payloads live in the key word — the array is a
                 * placeholder so output plumbing keeps one column */
                t->payload.back().alloc(
                    plan.pack_bits ? 1 : (size_t)cap * 8);
            }
            return;
        }
        cap_rows = plan.capacity_hint > 16 ? plan.capacity_hint : 16;
        t->n_keys = plan.n_keys;
        t->key_rows.alloc((size_t)cap_rows * 8 * key_words());
        if (plan.n_keys) t->knull.alloc((size_t)cap_rows);
        for (int i = 0; i < plan.n_payload; i++) {
            t->payload.emplace_back();
            t->ptag.push_back(-1); /* resolved on first input */
            t->payload.back().alloc((size_t)cap_rows * 8);
        }
    }
    /* int64 words of key_rows per build row */
    size_t key_words() const { return plan.n_keys ? plan.n_keys : 1; }
    void grow(int64_t need)
    {
        if (need <= cap_rows) return;
        int64_t nc = cap_rows;
        while (nc < need) nc *= 2;
        DevBuf nk;
        nk.alloc((size_t)nc * 8 * key_words());
        CHKV(hipMemcpyAsync(nk.p, t->key_rows.p,
                            (size_t)t->n_rows * 8 * key_words(),
                            hipMemcpyDeviceToDevice, g_stream));
        t->key_rows = std::move(nk);
        if (plan.n_keys) {
            DevBuf nn;
            nn.alloc((size_t)nc);
            CHKV(hipMemcpyAsync(nn.p, t->knull.p, (size_t)t->n_rows,
                                hipMemcpyDeviceToDevice, g_stream));
            t->knull = std::move(nn);
        }
        for (size_t i = 0; i < t->payload.size(); i++) {
            DevBuf np;
            np.alloc((size_t)nc * 8);
            CHKV(hipMemcpyAsync(np.p, t->payload[i].p,
                                (size_t)t->n_rows *
                                    (t->ptag[i] >= 0
                                         ? type_size(t->ptag[i])
                                         : 8),
                                hipMemcpyDeviceToDevice, g_stream));
            t->payload[i] = std::move(np);
        }
        cap_rows = nc;
    }
    const Table* semi_table()
    {
        if (plan.semijoin_table < 0) return nullptr;
        std::lock_guard<std::mutex> lk(g_mu);
        auto it = g_tables.find(plan.semijoin_table);
        if (it == g_tables.end())
            throw std::runtime_error("semijoin table not found");
        reject_multikey(it->second.get(), "a semijoin_table");
        return it->second.get();
    }
    /* multi-key chained build: the surviving rows go through the selection
     * path (row ids + payloads), then k_mk_gather widens their key
     * channels into key_rows / knull.  Every check runs before anything
     * changes, so a rejected page leaves the build as it was. */
    void add_input_multikey(const pg_page* in)
    {
        check_multikey_cols("HASH_BUILD", plan.n_keys, plan.key_cols, in,
                            t->key_tag);
        for (int i = 0; i < plan.n_payload; i++) {
            const int32_t c = plan.payload_col[i];
            const std::string name = "HASH_BUILD: payload_col[" +
                                     std::to_string(i) + "] (column " +
                                     std::to_string(c) + ")";
            if (c < 0 || c >= in->n_cols)
                throw std::runtime_error(
                    name + " is outside the page's " +
                    std::to_string(in->n_cols) + " columns");
            const int tag = in->cols[c].tag;
            if (tag != PG_T_U8 && tag != PG_T_I32 && tag != PG_T_I64 &&
                tag != PG_T_F64)
                throw std::runtime_error(
                    name + ": payloads of a multi-key build are U8, I32, "
                           "I64 or F64 columns");
            if (t->ptag[i] >= 0 && t->ptag[i] != tag)
                throw std::runtime_error(
                    name + ": type " + std::to_string(tag) +
                    " differs from the first page's " +
                    std::to_string(t->ptag[i]));
        }
        const Table* semi = plan.semijoin_table > 0 ? semi_table() : nullptr;
        if (semi && plan.semijoin_col < 0)
            throw std::runtime_error("HASH_BUILD: semijoin_col is negative");
        StagedPage sp;
        sp.stage(in);
        pg_plan_filter_project fp{};
        fp.n_preds = plan.n_preds;
        memcpy(fp.preds, plan.preds, sizeof(fp.preds));
        fp.n_proj = 1 + plan.n_payload;
        fp.proj[0].kind = PG_PROJ_ROWID;
        for (int i = 0; i < plan.n_payload; i++) {
            fp.proj[1 + i].kind = PG_PROJ_IDENT;
            fp.proj[1 + i].a = plan.payload_col[i];
        }
        int64_t chunk = sel_chunk(sp.pg.n_rows);
        SelResult r = sel_count(sp.pg, fp, semi, plan.semijoin_col, chunk);
        if (t->n_rows + r.n > (int64_t)INT32_MAX)
            throw std::runtime_error(
                "HASH_BUILD: a multi-key build holds at most 2^31-1 rows "
                "(row ids are 32-bit)");
        for (int k = 0; k < plan.n_keys; k++)
            t->key_tag[k] = in->cols[plan.key_cols[k]].tag;
        for (int i = 0; i < plan.n_payload; i++)
            t->ptag[i] = in->cols[plan.payload_col[i]].tag;
        grow(t->n_rows + r.n);
        DevBuf rowid;
        rowid.alloc((size_t)(r.n ? r.n : 1) * 8);
        emit_outs outs{};
        outs.n = fp.n_proj;
        outs.ptr[0] = rowid.p;
        outs.tag[0] = PG_T_I64;
        for (int i = 0; i < plan.n_payload; i++) {
            outs.ptr[1 + i] = (int8_t*)t->payload[i].p +
                              t->n_rows * type_size(t->ptag[i]);
            outs.tag[1 + i] = t->ptag[i];
        }
        sel_emit(sp.pg, fp, semi, plan.semijoin_col, chunk, r, outs);
        if (r.n) {
            mk_keys mk{};
            mk.n = plan.n_keys;
            for (int k = 0; k < plan.n_keys; k++)
                mk.col[k] = plan.key_cols[k];
            int64_t nb = (r.n + 255) / 256;
            hipLaunchKernelGGL(
                k_mk_gather, dim3((unsigned)(nb < 2048 ? nb : 2048)),
                dim3(256), 0, g_stream, sp.pg, mk,
                (const int64_t*)rowid.p, r.n,
                (int64_t*)t->key_rows.p + t->n_rows * plan.n_keys,
                (uint8_t*)t->knull.p + t->n_rows);
            CHKV(hipStreamSynchronize(g_stream));
        }
        t->n_rows += r.n;
    }
    void add_input(const pg_page* in) override
    {
        if (plan.range_group)
            throw std::runtime_error(
                "range_group tables take no build input (the domain is "
                "the key range itself)");
        check_pred_types("HASH_BUILD", plan.preds, preds_used(plan.n_preds),
                         in);
        if (plan.n_keys) {
            add_input_multikey(in);
            return;
        }
        StagedPage sp;
        sp.stage(in);
        /* resolve payload tags on first page (payload 0 is u8 when it
         * is sourced through a fused dimension lookup) */
        for (int i = 0; i < plan.n_payload; i++)
            if (t->ptag[i] < 0)
                t->ptag[i] = (plan.agg_table &&
                              plan.payload_lookup_table > 0 && i == 0)
                                 ? PG_T_U8
                                 : sp.pg.cols[plan.payload_col[i]].tag;
        if (plan.dense_array) {
            if (plan.semijoin_table > 0) /* 0 / -1 both mean unused */
                throw std::runtime_error(
                    "dense_array builds do not evaluate semijoins — "
                    "pre-filter with a FILTER_PROJECT semijoin instead");
            if (sp.pg.cols[plan.key_col].tag != PG_T_I64 ||
                (!plan.key_set_only && !plan.payload_lookup_table &&
                 sp.pg.cols[plan.payload_col[0]].tag != PG_T_U8 &&
                 sp.pg.cols[plan.payload_col[0]].tag != PG_T_I32))
                throw std::runtime_error(
                    "dense_array expects I64 keys and a U8/I32 payload");
            int32_t ptag =
                plan.key_set_only || plan.payload_lookup_table
                    ? PG_T_U8
                    : sp.pg.cols[plan.payload_col[0]].tag;
            if (t->dense_alloc_pending) {
                t->ptag[0] = ptag;
                t->payload[0].alloc((size_t)t->cap *
                                    (ptag == PG_T_I32 ? 4 : 1));
                t->payload[0].zero();
                t->dense_alloc_pending = false;
            } else if (t->ptag[0] != ptag) {
                throw std::runtime_error(
                    "dense_array payload tag changed across pages");
            }
            if (plan.payload_lookup_table > 0) {
                const Table* lu;
                {
                    std::lock_guard<std::mutex> lk(g_mu);
                    auto it = g_tables.find(plan.payload_lookup_table);
                    if (it == g_tables.end() || !it->second->dense ||
                        it->second->ptag[0] != PG_T_U8)
                        throw std::runtime_error(
                            "dense fill lookup needs a dense u8 table");
                    lu = it->second.get();
                }
                hipLaunchKernelGGL(
                    k_dense_fill_lu, dim3(2048), dim3(256), 0, g_stream,
                    sp.pg, plan, (const uint8_t*)lu->payload[0].p,
                    lu->cap, (uint8_t*)t->payload[0].p, t->cap);
            } else if (ptag == PG_T_I32)
                hipLaunchKernelGGL(
                    k_dense_fill32, dim3(2048), dim3(256), 0, g_stream,
                    sp.pg, plan,
                    (const int32_t*)sp.pg.cols[plan.payload_col[0]].data,
                    (int32_t*)t->payload[0].p, t->cap);
            else
                hipLaunchKernelGGL(
                    k_dense_fill, dim3(2048), dim3(256), 0, g_stream,
                    sp.pg, plan,
                    plan.key_set_only
                        ? nullptr
                        : (const uint8_t*)
                              sp.pg.cols[plan.payload_col[0]].data,
                    (uint8_t*)t->payload[0].p, t->cap);
            CHKV(hipStreamSynchronize(g_stream));
            return;
        }
        if (plan.agg_table) {
            const Table* semi = semi_table();
            const Table* lu = nullptr;
            if (plan.payload_lookup_table > 0) {
                std::lock_guard<std::mutex> lk(g_mu);
                auto it = g_tables.find(plan.payload_lookup_table);
                if (it == g_tables.end() ||
                    !(it->second->slot_payloads || it->second->dense) ||
                    it->second->ptag.empty() ||
                    it->second->ptag[0] != PG_T_U8)
                    throw std::runtime_error(
                        "payload_lookup_table must be an agg_table or "
                        "dense_array with a u8 payload");
                lu = it->second.get();
            }
            direct_payloads dp{};
            dp.n = plan.n_payload;
            for (int o = 0; o < dp.n; o++) {
                dp.ptr[o] = t->payload[o].p;
                dp.tag[o] = lu && o == 0 ? PG_T_U8 : t->ptag[o];
                dp.src[o] = plan.payload_col[o];
            }
            if (part) {
                /* phase A: scatter surviving rows into partition runs;
                 * inserts happen at finish (k_part_insert) */
                hot_begin();
                hipLaunchKernelGGL(
                    k_part_scatter, dim3(2048), dim3(256), 0, g_stream,
                    sp.pg, plan, set_ptr(semi), set_mask_of(semi),
                    lu && !lu->dense ? (const int64_t*)lu->keys.p
                                     : nullptr,
                    lu && !lu->dense ? (const uint8_t*)lu->tags.p
                                     : nullptr,
                    lu ? (lu->dense ? lu->cap : lu->mask) : 0,
                    lu ? (lu->dense ? lu->cap : lu->local_mask) : 0,
                    lu ? (const uint8_t*)lu->payload[0].p : nullptr, dp,
                    t->mask, capp_bits, P, (int64_t*)stage.p,
                    (unsigned long long*)cursorb.p, t->cap / P,
                    1 + plan.n_payload,
                    (unsigned long long*)counters.p + 2);
                hot_end();
                CHKV(hipStreamSynchronize(g_stream));
                return;
            }
            staged_args sa;
            if (staged_fit(sp.pg, semi, lu, &sa)) {
                int64_t tiles = (sa.n + BS_TILE - 1) / BS_TILE;
                int64_t cap_grid = BS_GRID;
                /* PG_STAGED_GRID caps the grid (tests: several tiles per
                 * block at a few thousand rows) */
                if (const char* eg = getenv("PG_STAGED_GRID"))
                    if (atoi(eg) > 0) cap_grid = atoi(eg);
                int grid = (int)(tiles < cap_grid ? (tiles > 0 ? tiles : 1)
                                                  : cap_grid);
                /* the clamped gathers of dropped rows read byte 0: an
                 * empty dense range gets a byte that exists (every row is
                 * dropped, so its value is never looked at) */
                if (sa.sk && sa.nflags <= 0)
                    sa.flags = (const uint8_t*)counters.p;
                if (sa.lk && sa.lucap <= 0)
                    sa.lu = (const uint8_t*)counters.p;
                hot_begin();
                hipLaunchKernelGGL(
                    bs_pick(sa), dim3(grid), dim3(256), 0, g_stream,
                    sa, plan.pack_bits, (int64_t*)t->keys.p,
                    (uint8_t*)t->tags.p, t->mask,
                    (unsigned long long*)counters.p,
                    (unsigned long long*)counters.p + 1,
                    (unsigned long long*)counters.p + 3,
                    (unsigned long long*)t->kbits.p, t->bmax,
                    (unsigned long long*)counters.p + 4);
                hot_end();
                g_build_staged_launches++;
                CHKV(hipStreamSynchronize(g_stream));
                return;
            }
            hot_begin();
            hipLaunchKernelGGL(k_tbl_insert_direct, dim3(4096), dim3(256),
                               0, g_stream, sp.pg, plan, set_ptr(semi),
                               set_mask_of(semi),
                               lu && !lu->dense
                                   ? (const int64_t*)lu->keys.p
                                   : nullptr,
                               lu && !lu->dense
                                   ? (const uint8_t*)lu->tags.p
                                   : nullptr,
                               lu ? (lu->dense ? lu->cap : lu->mask) : 0,
                               lu ? (lu->dense ? lu->cap : lu->local_mask)
                                  : 0,
                               lu ? (const uint8_t*)lu->payload[0].p
                                  : nullptr,
                               (int64_t*)t->keys.p,
                               (uint8_t*)t->tags.p, dp, t->mask,
                               (unsigned long long*)counters.p,
                               (unsigned long long*)counters.p + 1,
                               (unsigned long long*)counters.p + 3,
                               (unsigned long long*)t->kbits.p, t->bmax,
                               (unsigned long long*)counters.p + 4);
            hot_end();
            CHKV(hipStreamSynchronize(g_stream));
            return;
        }
        pg_plan_filter_project fp{};
        fp.n_preds = plan.n_preds;
        memcpy(fp.preds, plan.preds, sizeof(fp.preds));
        fp.n_proj = 1 + plan.n_payload;
        fp.proj[0].kind = PG_PROJ_IDENT;
        fp.proj[0].a = plan.key_col;
        for (int i = 0; i < plan.n_payload; i++) {
            fp.proj[1 + i].kind = PG_PROJ_IDENT;
            fp.proj[1 + i].a = plan.payload_col[i];
        }
        const Table* semi = nullptr;
        if (plan.semijoin_table >= 0) {
            std::lock_guard<std::mutex> lk(g_mu);
            auto it = g_tables.find(plan.semijoin_table);
            if (it == g_tables.end())
                throw std::runtime_error("semijoin table not found");
            semi = it->second.get();
            reject_multikey(semi, "a semijoin_table");
        }
        int64_t chunk = sel_chunk(sp.pg.n_rows);
        SelResult r =
            sel_count(sp.pg, fp, semi, plan.semijoin_col, chunk);
        grow(t->n_rows + r.n);
        /* emit into build-row arrays at offset n_rows; payload element size
         * is the input tag size, so emit uses byte-offset pointers */
        emit_outs outs{};
        outs.n = fp.n_proj;
        outs.ptr[0] = (int8_t*)t->key_rows.p + t->n_rows * 8;
        outs.tag[0] = PG_T_I64;
        for (int i = 0; i < plan.n_payload; i++) {
            outs.ptr[1 + i] = (int8_t*)t->payload[i].p +
                              t->n_rows * type_size(t->ptag[i]);
            outs.tag[1 + i] = t->ptag[i];
        }
        /* key col may be i32 etc.: force i64 materialization via a
         * non-ident trick is unnecessary — keys must be I64 columns */
        if (sp.pg.cols[plan.key_col].tag != PG_T_I64)
            throw std::runtime_error("build key must be an I64 column");
        sel_emit(sp.pg, fp, semi, plan.semijoin_col, chunk, r, outs);
        t->n_rows += r.n;
    }
    void finish() override
    {
        if (plan.dense_array || plan.range_group) {
            std::lock_guard<std::mutex> lk(g_mu);
            tbl = g_next_table++;
            g_tables[tbl] = std::move(t);
            return;
        }
        if (plan.agg_table) {
            if (part) {
                direct_payloads dp{};
                dp.n = plan.n_payload;
                for (int o = 0; o < dp.n; o++) {
                    dp.ptr[o] = t->payload[o].p;
                    dp.tag[o] = (plan.payload_lookup_table > 0 && o == 0)
                                    ? PG_T_U8
                                    : t->ptag[o];
                }
                static int use_bar = -1;
                if (use_bar < 0) {
                    const char* eb = getenv("PG_PART_BARRIER");
                    use_bar = eb ? atoi(eb) : 0;
                }
                hot_begin();
                if (!use_bar) {
                    hipLaunchKernelGGL(k_tbl_init, dim3(1024), dim3(256),
                                       0, g_stream, (int64_t*)t->keys.p,
                                       nullptr, t->cap);
                    if (t->tags.p)
                        CHKV(hipMemsetAsync(t->tags.p, 0, t->tags.sz,
                                            g_stream));
                }
                hipLaunchKernelGGL(k_part_insert,
                                   dim3(use_bar ? persistent_grid()
                                                : 4096), dim3(256), 0,
                                   g_stream, (const int64_t*)stage.p,
                                   (const unsigned long long*)cursorb.p,
                                   t->cap / P, 1 + plan.n_payload,
                                   (int64_t*)t->keys.p,
                                   (uint8_t*)t->tags.p, dp, t->cap / P, P,
                                   Kact, use_bar, plan.pack_bits,
                                   (unsigned long long*)barb.p,
                                   (unsigned long long*)counters.p,
                                   (unsigned long long*)counters.p + 1,
                                   (unsigned long long*)counters.p + 3,
                                   (unsigned long long*)t->kbits.p,
                                   t->bmax,
                                   (unsigned long long*)counters.p + 4);
                hot_end();
                CHKV(hipStreamSynchronize(g_stream));
                stage.free();
                cursorb.free();
                barb.free();
            }
            unsigned long long c[5];
            CHKV(hipMemcpy(c, counters.p, 40, hipMemcpyDeviceToHost));
            if (c[4])
                throw std::runtime_error(
                    "bitmap_max_key violated: build key outside "
                    "[1, bitmap_max_key]");
            if (c[3])
                throw std::runtime_error(
                    "pack_bits violated: key or payload outside the "
                    "declared bit ranges");
            if (c[2])
                throw std::runtime_error(
                    "partition staging overflow (unexpected hash skew): "
                    "raise capacity_hint");
            if (c[1])
                throw std::runtime_error(
                    "agg table overflow: capacity_hint too small");
            if ((int64_t)c[0] * 100 > t->cap * 85)
                throw std::runtime_error(
                    "agg table fill exceeded 0.85: raise capacity_hint");
            t->n_rows = (int64_t)c[0];
            std::lock_guard<std::mutex> lk(g_mu);
            tbl = g_next_table++;
            g_tables[tbl] = std::move(t);
            return;
        }
        if (plan.n_keys) {
            if (t->n_rows > (int64_t)INT32_MAX)
                throw std::runtime_error(
                    "HASH_BUILD: a multi-key build holds at most 2^31-1 "
                    "rows (row ids are 32-bit)");
            int64_t cap = next_pow2(t->n_rows * 2 + 16); /* fill <= 0.5 */
            t->cap = cap;
            t->mask = cap - 1;
            t->local_mask = cap - 1;
            t->keys.alloc((size_t)cap * 8); /* the slot words */
            t->next.alloc((size_t)(t->n_rows ? t->n_rows : 1) * 4);
            CHKV(hipMemsetAsync(t->keys.p, 0xff, (size_t)cap * 8, g_stream));
            CHKV(hipMemsetAsync(t->next.p, 0xff,
                                (size_t)(t->n_rows ? t->n_rows : 1) * 4,
                                g_stream));
            DevBuf err;
            err.alloc(8);
            err.zero();
            if (t->n_rows) {
                int64_t nb = (t->n_rows + 255) / 256;
                hipLaunchKernelGGL(
                    k_mk_insert, dim3((unsigned)(nb < 2048 ? nb : 2048)),
                    dim3(256), 0, g_stream, (const int64_t*)t->key_rows.p,
                    (const uint8_t*)t->knull.p, t->n_rows, plan.n_keys,
                    (unsigned long long*)t->keys.p, (int32_t*)t->next.p,
                    t->mask, (unsigned long long*)err.p);
            }
            unsigned long long e = 0;
            CHKV(hipMemcpyAsync(&e, err.p, 8, hipMemcpyDeviceToHost,
                                g_stream));
            CHKV(hipStreamSynchronize(g_stream));
            if (e)
                throw std::runtime_error(
                    "HASH_BUILD: multi-key insert found no free slot");
            std::lock_guard<std::mutex> lk(g_mu);
            tbl = g_next_table++;
            g_tables[tbl] = std::move(t);
            return;
        }
        int64_t cap = next_pow2(t->n_rows * 2 + 16); /* fill <= 0.5 */
        t->cap = cap;
        t->mask = cap - 1;
        t->local_mask = cap - 1;
        t->keys.alloc((size_t)cap * 8);
        if (!t->key_set_only) {
            t->head.alloc((size_t)cap * 4);
            t->next.alloc((size_t)(t->n_rows ? t->n_rows : 1) * 4);
            /* byte tags pay off only when the key array is far beyond the
             * 256 MiB L3 (measured: at SF100's 256 MB keys the insert-side
             * extra random store costs more than the probe saves); enable
             * for tables past 64M slots. */
            if (cap >= (64ll << 20)) {
                t->tags.alloc((size_t)cap);
                t->tags.zero();
            }
        }
        hipLaunchKernelGGL(k_tbl_init, dim3(1024), dim3(256), 0, g_stream,
                           (int64_t*)t->keys.p,
                           t->key_set_only ? nullptr : (int32_t*)t->head.p,
                           cap);
        DevBuf bm_err;
        if (plan.bitmap_max_key > 0 && !t->key_set_only) {
            t->bmax = plan.bitmap_max_key;
            t->kbits.alloc((size_t)((t->bmax >> 6) + 1) * 8);
            t->kbits.zero();
            bm_err.alloc(8);
            bm_err.zero();
        }
        if (t->n_rows) {
            if (t->key_set_only)
                hipLaunchKernelGGL(k_set_insert, dim3(2048), dim3(256), 0,
                                   g_stream, (const int64_t*)t->key_rows.p,
                                   t->n_rows, (int64_t*)t->keys.p, t->mask);
            else
                hipLaunchKernelGGL(k_tbl_insert, dim3(2048), dim3(256), 0,
                                   g_stream, (const int64_t*)t->key_rows.p,
                                   t->n_rows, (int64_t*)t->keys.p,
                                   (uint8_t*)t->tags.p,
                                   (int32_t*)t->head.p, (int32_t*)t->next.p,
                                   t->mask,
                                   (unsigned long long*)t->kbits.p,
                                   t->bmax,
                                   (unsigned long long*)bm_err.p);
        }
        CHKV(hipStreamSynchronize(g_stream));
        if (bm_err.p) {
            unsigned long long e = 0;
            CHKV(hipMemcpy(&e, bm_err.p, 8, hipMemcpyDeviceToHost));
            if (e)
                throw std::runtime_error(
                    "bitmap_max_key violated: build key outside "
                    "[1, bitmap_max_key]");
        }
        std::lock_guard<std::mutex> lk(g_mu);
        tbl = g_next_table++;
        g_tables[tbl] = std::move(t);
    }
    int64_t table_handle() override { return tbl; }
};

/* ---------------- LOOKUP_JOIN ---------------- */
struct JoinOp : Op {
    pg_plan_lookup_join plan;
    Table* t = nullptr;
    Table* t2 = nullptr; /* mode 2 dense table */
    DevBuf m2_acc;       /* mode 2: [dec, flo, fhi, cnt] x 8 groups */
    DevBuf ovf;          /* modes 1/3: [tick-sum overflow, SUM_F64 addends
                            outside the 64.64 domain] */
    /* outer joins (modes 4-6).  The match marks are this operator's own:
     * one byte per build row, written by its probes and read once by the
     * drain in finish(). */
    DevBuf marks;
    std::vector<int32_t> probe_tags; /* emitted probe columns as typed in
                                        the first page fed (drain page) */
    int32_t key_tag[4] = {-1, -1, -1, -1}; /* multi-key: the key channels
                                              as typed in the first page */
    bool probe_outer() const
    {
        return plan.mode == PG_JOIN_PROBE_OUTER ||
               plan.mode == PG_JOIN_FULL_OUTER;
    }
    bool marking() const
    {
        return plan.mode == PG_JOIN_LOOKUP_OUTER ||
               plan.mode == PG_JOIN_FULL_OUTER;
    }
    bool outer() const { return probe_outer() || marking(); }
    bool emit_mode() const { return plan.mode == PG_JOIN_INNER || outer(); }
    /* a build that saw no input page never resolved its payload tags */
    static int32_t payload_tag(const Table* tb, int o)
    {
        return tb->ptag[o] >= 0 ? tb->ptag[o] : PG_T_I64;
    }
    /* the row filter, plus the per-aggregate FILTERs of a multi-agg probe */
    uint32_t used_preds() const
    {
        return plan.mode == 1 && plan.n_aggs > 0
                   ? preds_used(plan.n_preds, plan.agg_filter, plan.n_aggs)
                   : preds_used(plan.n_preds);
    }
    void init()
    {
        check_pred_lens("LOOKUP_JOIN", plan.preds, used_preds());
        std::lock_guard<std::mutex> lk(g_mu);
        auto it = g_tables.find(plan.table);
        if (it == g_tables.end())
            throw std::runtime_error("lookup table not found (build not "
                                     "finished?)");
        t = it->second.get();
        if (t->key_set_only)
            throw std::runtime_error(
                "cannot probe a key-set-only table");
        if (plan.mode < 0 || plan.mode > PG_JOIN_FULL_OUTER)
            throw std::runtime_error("unknown LOOKUP_JOIN mode");
        if (plan.n_keys < 0 || plan.n_keys > 4)
            throw std::runtime_error(
                "LOOKUP_JOIN: n_keys must be 0..4, got " +
                std::to_string(plan.n_keys));
        if (plan.n_keys != t->n_keys)
            throw std::runtime_error(
                "LOOKUP_JOIN: the plan has n_keys = " +
                std::to_string(plan.n_keys) + " but the table was built "
                "with n_keys = " + std::to_string(t->n_keys) +
                (plan.n_keys && t->n_keys
                     ? ""
                     : " (0 is the legacy single key_col)"));
        if (plan.n_keys) {
            if (!emit_mode())
                throw std::runtime_error(
                    "LOOKUP_JOIN mode " + std::to_string(plan.mode) +
                    " cannot probe a multi-key (n_keys >= 1) table: modes "
                    "0, 4, 5 and 6 only");
            for (int k = 0; k < plan.n_keys; k++)
                if (plan.key_cols[k] < 0)
                    throw std::runtime_error(
                        "LOOKUP_JOIN: n_keys = " +
                        std::to_string(plan.n_keys) + " but key_cols[" +
                        std::to_string(k) + "] is negative");
            if (plan.n_emit < 0 || plan.n_emit > 8)
                throw std::runtime_error("n_emit must be 0..8");
        }
        if (outer() && (plan.n_emit < 0 || plan.n_emit > 8))
            throw std::runtime_error("n_emit must be 0..8");
        if (outer() && t->range_group)
            throw std::runtime_error(
                "outer LOOKUP_JOIN modes cannot probe a range_group table");
        if (marking()) {
            /* the drain walks build-row arrays, which only chained tables
             * keep (slot-payload and dense tables have no row order) */
            if (t->slot_payloads || t->dense || (!t->head.p && !t->n_keys))
                throw std::runtime_error(
                    plan.mode == PG_JOIN_LOOKUP_OUTER
                        ? "LOOKUP_JOIN mode 5 (PG_JOIN_LOOKUP_OUTER) needs "
                          "a chained build table, not an agg_table or "
                          "dense_array"
                        : "LOOKUP_JOIN mode 6 (PG_JOIN_FULL_OUTER) needs a "
                          "chained build table, not an agg_table or "
                          "dense_array");
            marks.alloc((size_t)t->n_rows);
            marks.zero();
            CHKV(hipStreamSynchronize(g_stream));
        }
        if (t->dense && !emit_mode())
            throw std::runtime_error(
                "dense-array tables support emit-mode joins only");
        if (t->pack_bits &&
            !(plan.mode == 1 || plan.mode == 2 ||
              (emit_mode() && t->slot_payloads)))
            throw std::runtime_error(
                "packed tables support fused-agg probes and slot-payload "
                "emit joins only");
        /* mode 0 emit over a slot-payload table: unique keys, payloads
         * indexed by slot (no chains) */
        if (plan.mode == 1 || plan.mode == 3) {
            ovf.alloc(16);
            ovf.zero();
        }
        if (plan.mode == 1 && plan.n_aggs > 0) {
            if (plan.n_aggs > 6)
                throw std::runtime_error("n_aggs must be 1..6");
            if (!t->slot_payloads)
                throw std::runtime_error(
                    "multi-agg probes need an agg_table build");
            for (int a = 0; a < plan.n_aggs; a++)
                if (plan.agg_filter[a] >= plan.n_preds &&
                    plan.agg_filter[a] >= PG_MAX_PRED)
                    throw std::runtime_error("agg_filter out of range");
            /* the kernel knows COUNT and int64 tick sums; anything else
             * would come back as a sum of ticks */
            for (int a = 0; a < plan.n_aggs; a++) {
                const int32_t fn = plan.aggs[a].func;
                if (fn != PG_AGG_COUNT && fn != PG_AGG_SUM_DEC &&
                    fn != PG_AGG_SUM_I64)
                    throw std::runtime_error(
                        "LOOKUP_JOIN: aggs[" + std::to_string(a) +
                        "].func = " + std::to_string(fn) +
                        (fn == PG_AGG_SUM_F64 ? " (SUM_F64)"
                         : fn == PG_AGG_MIN   ? " (MIN)"
                         : fn == PG_AGG_MAX   ? " (MAX)"
                                              : "") +
                        " is not a multi-agg function: COUNT, SUM_DEC and "
                        "SUM_I64 only");
            }
            int32_t want_stride = plan.n_aggs + 1;
            int32_t lay_shift[6] = {0, 0, 0, 0, 0, 0};
            int32_t lay_width[6] = {0, 0, 0, 0, 0, 0};
            int32_t lay_cnt_shift = 0, lay_cnt_width = 0;
            if (plan.acc_pack) {
                want_stride = 1;
                /* widths and shifts are validated before any shift by
                 * them: a 64-bit shift is undefined on the host and on
                 * the device */
                lay_cnt_shift = plan.acc_pack_cnt_shift;
                lay_cnt_width = plan.acc_pack_cnt_width;
                if (lay_cnt_width < 1 || lay_cnt_width > 63)
                    throw std::runtime_error(
                        "acc_pack_cnt_width must be 1..63, got " +
                        std::to_string(lay_cnt_width));
                if (lay_cnt_shift < 0 || lay_cnt_shift + lay_cnt_width > 64)
                    throw std::runtime_error(
                        "acc_pack_cnt_shift must be >= 0 with shift + "
                        "width <= 64, got shift " +
                        std::to_string(lay_cnt_shift) + " width " +
                        std::to_string(lay_cnt_width));
                unsigned long long used =
                    ((1ull << lay_cnt_width) - 1) << lay_cnt_shift;
                for (int a = 0; a < plan.n_aggs; a++) {
                    const int32_t sh = plan.acc_pack_shift[a];
                    const int32_t wd = plan.acc_pack_width[a];
                    const std::string ix = "[" + std::to_string(a) + "]";
                    if (sh == -1) { /* own word: the width is not read */
                        lay_shift[a] = -1;
                        want_stride++;
                        continue;
                    }
                    if (wd < 1 || wd > 63)
                        throw std::runtime_error(
                            "acc_pack_width" + ix + " must be 1..63 (a "
                            "64-bit field is an own word, shift -1), got " +
                            std::to_string(wd));
                    if (sh < 0 || sh + wd > 64)
                        throw std::runtime_error(
                            "acc_pack_shift" + ix + " must be -1 (own "
                            "word) or >= 0 with shift + width <= 64, got "
                            "shift " + std::to_string(sh) + " width " +
                            std::to_string(wd));
                    unsigned long long fm = ((1ull << wd) - 1) << sh;
                    if (used & fm)
                        throw std::runtime_error(
                            "acc_pack_shift" + ix + ": the field overlaps "
                            "the count field or an earlier field");
                    used |= fm;
                    lay_shift[a] = sh;
                    lay_width[a] = wd;
                }
            }
            if (t->acc_multi.p) {
                bool same = t->n_acc == plan.n_aggs &&
                            t->acc_stride == want_stride &&
                            t->acc_packed == (plan.acc_pack ? 1 : 0) &&
                            t->acc_cnt_shift == lay_cnt_shift &&
                            t->acc_cnt_width == lay_cnt_width;
                for (int a = 0; a < 6; a++)
                    same = same && t->acc_shift[a] == lay_shift[a] &&
                           t->acc_width[a] == lay_width[a];
                if (!same)
                    throw std::runtime_error(
                        "table already carries a different multi-agg "
                        "layout (n_aggs, acc_pack, acc_pack_shift/width "
                        "and the count field must all match the first "
                        "multi-agg operator's)");
            }
            if (!t->acc_multi.p) {
                t->n_acc = plan.n_aggs;
                t->acc_stride = want_stride;
                t->acc_packed = plan.acc_pack ? 1 : 0;
                for (int a = 0; a < 6; a++) {
                    t->acc_shift[a] = lay_shift[a];
                    t->acc_width[a] = lay_width[a];
                }
                t->acc_cnt_shift = lay_cnt_shift;
                t->acc_cnt_width = lay_cnt_width;
                t->acc_multi.alloc((size_t)t->cap * want_stride * 8);
                t->acc_multi.zero();
                CHKV(hipStreamSynchronize(g_stream));
            }
            t->list_ok = false; /* k_probe_agg_multi does not append */
        } else if (plan.mode == 1) {
            /* slim 2-word accumulators when this consumer reads only the
             * tick sum + count (dec_only / dec_min) — halves the zeroing
             * and extraction traffic; a later fx128 consumer of the same
             * table errors out loudly */
            int32_t want_aw = (plan.dec_only || plan.dec_min) ? 2 : 4;
            if (!t->acc.p) {
                t->acc_words = want_aw;
                t->acc.alloc((size_t)t->cap * t->acc_words * 8);
                t->acc.zero();
                /* the hit list is born with the zeroed accumulators.
                 * Groups <= inserted build rows, so n_rows entries hold
                 * every first touch; no zeroing needed.  Range-group
                 * tables hit most of their range and keep the scan. */
                if (t->use_hits && !t->range_group) {
                    t->hits_cap = t->n_rows;
                    t->hits.alloc((size_t)t->hits_cap *
                                  (t->cap > (1ll << 32) ? 8 : 4));
                    t->hits_n.alloc(8);
                    t->hits_n.zero();
                    t->hits_n_host = 0;
                    t->list_ok = true;
                }
                CHKV(hipStreamSynchronize(g_stream));
            } else if (want_aw == 4 && t->acc_words == 2) {
                throw std::runtime_error(
                    "table accumulators were allocated dec-only; fx128 "
                    "probes need a fresh table");
            }
        }
        if (plan.mode == 1 && plan.dec_min) {
            /* MIN identity: dec = large positive sentinel; cnt
             * distinguishes matched groups */
            hipLaunchKernelGGL(k_acc_min_init, dim3(2048), dim3(256), 0,
                               g_stream, (unsigned long long*)t->acc.p,
                               t->acc_words, t->cap);
            hits_restart(t); /* every count is zero again */
            CHKV(hipStreamSynchronize(g_stream));
        }
        if (plan.mode == 2) {
            if (!t->slot_payloads || t->ptag.size() != 1 ||
                t->ptag[0] != PG_T_U8)
                throw std::runtime_error(
                    "mode 2 probes an agg_table with one u8 payload");
            auto it2 = g_tables.find(plan.table2);
            if (it2 == g_tables.end() || !it2->second->dense)
                throw std::runtime_error("mode 2 needs a dense_array "
                                         "table2");
            t2 = it2->second.get();
            if (plan.n_group_vals < 1 || plan.n_group_vals > 8)
                throw std::runtime_error("n_group_vals must be 1..8");
            m2_acc.alloc(4 * 8 * 8 + 8); /* + tick-overflow counter */
            m2_acc.zero();
        }
        if (plan.mode == 3) {
            if (t->slot_payloads || t->ptag.empty() ||
                t->ptag[0] != PG_T_I64)
                throw std::runtime_error(
                    "mode 3 needs a chained build whose first payload "
                    "is the i64 grouping key");
            auto it2 = g_tables.find(plan.table2);
            if (it2 == g_tables.end() || it2->second->dense ||
                it2->second->key_set_only)
                throw std::runtime_error(
                    "mode 3 needs an agg/keyed table2 for the groups");
            t2 = it2->second.get();
            reject_multikey(t2, "table2");
            if (t2->pack_bits)
                throw std::runtime_error(
                    "mode 3 groups table cannot be packed");
            if (!t2->acc.p) {
                t2->acc_words = 4;
                t2->acc.alloc((size_t)t2->cap * 4 * 8);
                t2->acc.zero();
                CHKV(hipStreamSynchronize(g_stream));
            }
            t2->list_ok = false; /* k_probe_agg_pay does not append */
        }
    }
    void add_input(const pg_page* in) override
    {
        check_pred_types("LOOKUP_JOIN", plan.preds, used_preds(), in);
        if (plan.n_keys) {
            check_multikey_cols("LOOKUP_JOIN", plan.n_keys, plan.key_cols,
                                in, key_tag);
            for (int o = 0; o < plan.n_emit; o++)
                if (plan.emit_probe_cols[o] < 0 ||
                    plan.emit_probe_cols[o] >= in->n_cols)
                    throw std::runtime_error(
                        "LOOKUP_JOIN: emit_probe_cols[" +
                        std::to_string(o) + "] is outside the page's " +
                        std::to_string(in->n_cols) + " columns");
        }
        /* the emit joins copy fixed-width probe columns only (VARBIN emit
         * is FILTER_PROJECT's two-pass gather): refuse before any launch */
        if (emit_mode())
            for (int o = 0; o < plan.n_emit && o < 8; o++) {
                const int32_t ec = plan.emit_probe_cols[o];
                if (ec >= 0 && ec < in->n_cols &&
                    in->cols[ec].tag == PG_T_VARBIN)
                    throw std::runtime_error(
                        std::string(outer() ? "outer " : "") +
                        "LOOKUP_JOIN emits fixed-width probe columns only: "
                        "emit_probe_cols[" + std::to_string(o) +
                        "] is VARBIN column " + std::to_string(ec));
            }
        for (int k = 0; k < plan.n_keys; k++)
            key_tag[k] = in->cols[plan.key_cols[k]].tag;
        StagedPage sp;
        sp.stage(in);
        if (plan.mode == 2) {
            unsigned long long* a = (unsigned long long*)m2_acc.p;
            /* specialized fast path: packed table + no predicates +
             * DISC_PRICE over aligned f64 columns (the Q5 shape) */
            bool spec = plan.n_preds == 0 && t->pack_bits > 0 &&
                        plan.proj.kind == PG_PROJ_DISC_PRICE &&
                        sp.pg.cols[plan.key_col].tag == PG_T_I64 &&
                        sp.pg.cols[plan.table2_key_col].tag == PG_T_I64 &&
                        sp.pg.cols[plan.proj.a].tag == PG_T_F64 &&
                        sp.pg.cols[plan.proj.b].tag == PG_T_F64 &&
                        plan.dec_scale == 4 &&
                        !((uintptr_t)sp.pg.cols[plan.key_col].data & 15) &&
                        !((uintptr_t)sp.pg.cols[plan.table2_key_col].data &
                          15) &&
                        !sp.pg.cols[plan.key_col].null_mask &&
                        !sp.pg.cols[plan.table2_key_col].null_mask &&
                        !sp.pg.cols[plan.proj.a].null_mask &&
                        !sp.pg.cols[plan.proj.b].null_mask;
            hot_begin();
            if (spec) {
                hipLaunchKernelGGL(
                    k_probe_agg_q5<8>, dim3(4096), dim3(256), 0, g_stream,
                    plan, (const int64_t*)sp.pg.cols[plan.key_col].data,
                    (const int64_t*)sp.pg.cols[plan.table2_key_col].data,
                    (const double*)sp.pg.cols[plan.proj.a].data,
                    (const double*)sp.pg.cols[plan.proj.b].data,
                    sp.pg.n_rows, (const int64_t*)t->keys.p,
                    (const uint8_t*)t->tags.p, t->mask, t->local_mask,
                    t->pack_bits, (const unsigned long long*)t->kbits.p, t->bmax,
                    (const uint8_t*)t2->payload[0].p,
                    t2->cap, a, a + 8, a + 16, a + 24);
                g_mode2_q5_launches++;
            } else {
                hipLaunchKernelGGL(k_probe_agg_fused2<8>, dim3(4096),
                                   dim3(256), 0, g_stream, sp.pg, plan,
                                   (const int64_t*)t->keys.p,
                                   t->local_mask, t->pack_bits,
                                   (const uint8_t*)t->tags.p, t->mask,
                                   (const uint8_t*)t->payload[0].p,
                                   (const uint8_t*)t2->payload[0].p,
                                   t2->cap, a, a + 8, a + 16, a + 24);
            }
            hot_end();
            CHKV(hipStreamSynchronize(g_stream));
            return;
        }
        if (plan.mode == 3) {
            t2->list_ok = false; /* also after a reset since construction */
            hot_begin();
            hipLaunchKernelGGL(k_probe_agg_pay, dim3(4096), dim3(256), 0,
                               g_stream, sp.pg, plan,
                               (const int64_t*)t->keys.p,
                               (const uint8_t*)t->tags.p,
                               (const int32_t*)t->head.p, t->mask,
                               t->local_mask,
                               (const unsigned long long*)t->kbits.p, t->bmax,
                               (const int64_t*)t->payload[0].p,
                               (const int64_t*)t2->keys.p,
                               (const uint8_t*)t2->tags.p, t2->mask,
                               t2->local_mask,
                               (unsigned long long*)t2->acc.p,
                               t2->acc_words,
                               (unsigned long long*)ovf.p);
            hot_end();
            CHKV(hipStreamSynchronize(g_stream));
            return;
        }
        if (plan.mode == 1 && plan.n_aggs > 0) {
            hot_begin();
            hipLaunchKernelGGL(k_probe_agg_multi, dim3(4096), dim3(256), 0,
                               g_stream, sp.pg, plan,
                               (const int64_t*)t->keys.p,
                               (const uint8_t*)t->tags.p, t->mask,
                               t->local_mask, t->pack_bits,
                               (const unsigned long long*)t->kbits.p, t->bmax,
                               (unsigned long long*)t->acc_multi.p,
                               (unsigned long long*)ovf.p);
            hot_end();
            CHKV(hipStreamSynchronize(g_stream));
            return;
        }
        if (plan.mode == 1) {
            /* specialized fast path for the Q3 shape (a SUM: dec_min
             * keeps the generic kernel) */
            bool spec = plan.proj.kind == PG_PROJ_DISC_PRICE &&
                        !plan.dec_min &&
                        sp.pg.cols[plan.key_col].tag == PG_T_I64 &&
                        sp.pg.cols[plan.proj.a].tag == PG_T_F64 &&
                        sp.pg.cols[plan.proj.b].tag == PG_T_F64 &&
                        plan.dec_scale == 4 && plan.n_preds <= 1 &&
                        !((uintptr_t)sp.pg.cols[plan.key_col].data & 15) &&
                        !((uintptr_t)sp.pg.cols[plan.proj.a].data & 15) &&
                        !((uintptr_t)sp.pg.cols[plan.proj.b].data & 15);
            if (plan.n_preds == 1) {
                const pg_pred& pr = plan.preds[0];
                spec = spec && pr.rhs_col == 0 &&
                       sp.pg.cols[pr.col].tag == PG_T_I32 &&
                       (pr.op == PG_CMP_GT || pr.op == PG_CMP_LT) &&
                       !((uintptr_t)sp.pg.cols[pr.col].data & 7) &&
                       !sp.pg.cols[pr.col].null_mask;
            }
            spec = spec && !sp.pg.cols[plan.key_col].null_mask &&
                   !sp.pg.cols[plan.proj.a].null_mask &&
                   !sp.pg.cols[plan.proj.b].null_mask;
            hot_begin();
            if (spec) {
                const pg_pred& pr = plan.preds[0];
                auto kern =
                    t->kbits.p
                        ? (t->tags.p ? k_probe_agg_q3<true, true>
                                     : k_probe_agg_q3<true, false>)
                        : (t->tags.p ? k_probe_agg_q3<false, true>
                                     : k_probe_agg_q3<false, false>);
                /* PG_PROBE_GRID caps the grid (tests: several passes per
                 * block at a few thousand rows) */
                int grid = PQ3_GRID;
                if (const char* eg = getenv("PG_PROBE_GRID"))
                    if (atoi(eg) > 0) grid = atoi(eg);
                hipLaunchKernelGGL(
                    kern, dim3(grid), dim3(256), 0, g_stream,
                    plan.n_preds
                        ? (const int32_t*)sp.pg.cols[pr.col].data
                        : nullptr,
                    plan.n_preds ? pr.op : 0,
                    plan.n_preds ? (int32_t)pr.ival : 0,
                    (const int64_t*)sp.pg.cols[plan.key_col].data,
                    (const double*)sp.pg.cols[plan.proj.a].data,
                    (const double*)sp.pg.cols[plan.proj.b].data,
                    sp.pg.n_rows, (const int64_t*)t->keys.p,
                    (const uint8_t*)t->tags.p, t->mask, t->local_mask,
                    t->pack_bits, (const unsigned long long*)t->kbits.p, t->bmax, plan.dec_only,
                    (unsigned long long*)t->acc.p, t->acc_words,
                    (unsigned long long*)ovf.p, hits_arg(t));
            } else {
                hipLaunchKernelGGL(k_probe_agg, dim3(4096), dim3(256), 0,
                                   g_stream, sp.pg, plan,
                                   (const int64_t*)t->keys.p,
                                   (const uint8_t*)t->tags.p, t->mask,
                                   t->local_mask, t->pack_bits,
                                   (const unsigned long long*)t->kbits.p, t->bmax,
                                   (unsigned long long*)t->acc.p,
                                   t->acc_words,
                                   (unsigned long long*)ovf.p, hits_arg(t));
            }
            hot_end();
            /* the list count rides on this page's synchronise, so that
             * finish() can size and launch the extraction without one */
            if (t->list_ok)
                CHKV(hipMemcpyAsync(&t->hits_n_host, t->hits_n.p, 8,
                                    hipMemcpyDeviceToHost, g_stream));
            CHKV(hipStreamSynchronize(g_stream));
            return;
        }
        /* emit mode: per-block count -> host scan -> prefix emit */
        int64_t n = sp.pg.n_rows;
        /* the multi-key path types its pages like the outer modes do */
        const bool typed_cols = outer() || plan.n_keys;
        if (typed_cols && probe_tags.empty())
            for (int o = 0; o < plan.n_emit; o++)
                probe_tags.push_back(
                    sp.pg.cols[plan.emit_probe_cols[o]].tag);
        if (n == 0) { /* empty probe page -> empty output page */
            OutPage op;
            op.pg.n_rows = 0;
            op.pg.n_cols = plan.n_emit + (int32_t)t->payload.size();
            for (int c = 0; c < op.pg.n_cols; c++) {
                op.pg.cols[c].tag = PG_T_I64;
                if (typed_cols) /* the columns a non-empty page would have */
                    op.pg.cols[c].tag =
                        c < plan.n_emit ? probe_tags[c]
                                        : payload_tag(t, c - plan.n_emit);
                op.pg.cols[c].on_device = 1;
                op.pg.cols[c].data = nullptr;
            }
            outq.push_back(std::move(op));
            return;
        }
        const uint8_t* dv8 = (const uint8_t*)(
            t->dense && t->ptag[0] == PG_T_U8 ? t->payload[0].p : nullptr);
        const int32_t* dv32 = (const int32_t*)(
            t->dense && t->ptag[0] == PG_T_I32 ? t->payload[0].p : nullptr);
        const int64_t dcap = t->dense ? t->cap : 0;
        hot_begin();
        int64_t chunk = sel_chunk(n);
        DevBuf d_counts;
        d_counts.alloc(FLT_NB * 8);
#define LAUNCH_PROBE_COUNT(PO, MK)                                       \
    hipLaunchKernelGGL((k_probe_count<PO, MK>), dim3(FLT_NB), dim3(256), \
                       0, g_stream, sp.pg, plan,                         \
                       (const int64_t*)t->keys.p,                        \
                       (const uint8_t*)t->tags.p,                        \
                       (const int32_t*)t->head.p,                        \
                       (const int32_t*)t->next.p, t->mask,               \
                       t->local_mask, t->pack_bits,                      \
                       (const unsigned long long*)t->kbits.p, t->bmax,   \
                       dv8, dv32, dcap, chunk, (int64_t*)d_counts.p)
#define LAUNCH_MK_COUNT(PO, MK)                                          \
    hipLaunchKernelGGL((k_mk_probe_count<PO, MK>), dim3(FLT_NB),         \
                       dim3(256), 0, g_stream, sp.pg, plan,              \
                       (const unsigned long long*)t->keys.p,             \
                       (const int32_t*)t->next.p, t->mask,               \
                       (const int64_t*)t->key_rows.p, chunk,             \
                       (int64_t*)d_counts.p)
        if (plan.n_keys) {
            g_multikey_probe_pages++;
            switch (plan.mode) {
                case PG_JOIN_PROBE_OUTER: LAUNCH_MK_COUNT(true, false); break;
                case PG_JOIN_LOOKUP_OUTER: LAUNCH_MK_COUNT(false, true); break;
                case PG_JOIN_FULL_OUTER: LAUNCH_MK_COUNT(true, true); break;
                default: LAUNCH_MK_COUNT(false, false);
            }
        } else
        switch (plan.mode) {
            case PG_JOIN_PROBE_OUTER: LAUNCH_PROBE_COUNT(true, false); break;
            case PG_JOIN_LOOKUP_OUTER: LAUNCH_PROBE_COUNT(false, true); break;
            case PG_JOIN_FULL_OUTER: LAUNCH_PROBE_COUNT(true, true); break;
            default: LAUNCH_PROBE_COUNT(false, false);
        }
#undef LAUNCH_MK_COUNT
#undef LAUNCH_PROBE_COUNT
        std::vector<int64_t> h(FLT_NB);
        CHKV(hipMemcpyAsync(h.data(), d_counts.p, FLT_NB * 8,
                            hipMemcpyDeviceToHost, g_stream));
        CHKV(hipStreamSynchronize(g_stream));
        int64_t total = 0;
        for (int b = 0; b < FLT_NB; b++) {
            int64_t v = h[b];
            h[b] = total;
            total += v;
        }
        DevBuf d_offs;
        d_offs.alloc(FLT_NB * 8);
        CHKV(hipMemcpyAsync(d_offs.p, h.data(), FLT_NB * 8,
                            hipMemcpyHostToDevice, g_stream));
        /* output page: probe cols then build payloads */
        OutPage op;
        op.pg.n_rows = total;
        emit_outs pouts{};
        pouts.n = plan.n_emit;
        outer_outs oo{};
        int nc = 0;
        for (int o = 0; o < plan.n_emit; o++) {
            const pg_col& src = sp.pg.cols[plan.emit_probe_cols[o]];
            int tag = src.tag;
            op.dev.emplace_back();
            op.dev.back().alloc((size_t)total * type_size(tag));
            op.pg.cols[nc].tag = tag;
            op.pg.cols[nc].on_device = 1;
            op.pg.cols[nc].data = op.dev.back().p;
            pouts.ptr[o] = op.dev.back().p;
            pouts.tag[o] = tag;
            if (outer() && src.null_mask) { /* mask travels with values */
                op.dev.emplace_back();
                op.dev.back().alloc((size_t)total);
                oo.pmask_src[o] = src.null_mask;
                oo.pmask_out[o] = (uint8_t*)op.dev.back().p;
                op.pg.cols[nc].null_mask = oo.pmask_out[o];
            }
            nc++;
        }
        if (probe_outer()) { /* one mask shared by the payload columns */
            op.dev.emplace_back();
            op.dev.back().alloc((size_t)total);
            oo.pay_null = (uint8_t*)op.dev.back().p;
        }
        oo.marks = (uint8_t*)marks.p;
        build_payloads bp{};
        bp.n = (int32_t)t->payload.size();
        bp.by_slot = (t->slot_payloads || t->dense) ? 1 : 0;
        bp.pack_bits = t->pack_bits;
        emit_outs bouts{};
        bouts.n = bp.n;
        for (int o = 0; o < bp.n; o++) {
            const int32_t ptag = typed_cols ? payload_tag(t, o) : t->ptag[o];
            bp.ptr[o] = t->payload[o].p;
            bp.tag[o] = ptag;
            op.dev.emplace_back();
            op.dev.back().alloc((size_t)total * type_size(ptag));
            op.pg.cols[nc].tag = ptag;
            op.pg.cols[nc].on_device = 1;
            op.pg.cols[nc].data = op.dev.back().p;
            op.pg.cols[nc].null_mask = oo.pay_null;
            bouts.ptr[o] = op.dev.back().p;
            bouts.tag[o] = ptag;
            nc++;
        }
        op.pg.n_cols = nc;
#define LAUNCH_PROBE_EMIT(PO, MK)                                        \
    hipLaunchKernelGGL((k_probe_emit<PO, MK>), dim3(FLT_NB), dim3(256),  \
                       0, g_stream, sp.pg, plan,                         \
                       (const int64_t*)t->keys.p,                        \
                       (const uint8_t*)t->tags.p,                        \
                       (const int32_t*)t->head.p,                        \
                       (const int32_t*)t->next.p, t->mask,               \
                       t->local_mask, t->pack_bits,                      \
                       (const unsigned long long*)t->kbits.p, t->bmax,   \
                       dv8, dv32, dcap, chunk, (const int64_t*)d_offs.p, \
                       pouts, bp, bouts, oo)
#define LAUNCH_MK_EMIT(PO, MK)                                           \
    hipLaunchKernelGGL((k_mk_probe_emit<PO, MK>), dim3(FLT_NB),          \
                       dim3(256), 0, g_stream, sp.pg, plan,              \
                       (const unsigned long long*)t->keys.p,             \
                       (const int32_t*)t->next.p, t->mask,               \
                       (const int64_t*)t->key_rows.p, chunk,             \
                       (const int64_t*)d_offs.p, pouts, bp, bouts, oo)
        if (plan.n_keys)
            switch (plan.mode) {
                case PG_JOIN_PROBE_OUTER: LAUNCH_MK_EMIT(true, false); break;
                case PG_JOIN_LOOKUP_OUTER: LAUNCH_MK_EMIT(false, true); break;
                case PG_JOIN_FULL_OUTER: LAUNCH_MK_EMIT(true, true); break;
                default: LAUNCH_MK_EMIT(false, false);
            }
        else
        switch (plan.mode) {
            case PG_JOIN_PROBE_OUTER: LAUNCH_PROBE_EMIT(true, false); break;
            case PG_JOIN_LOOKUP_OUTER: LAUNCH_PROBE_EMIT(false, true); break;
            case PG_JOIN_FULL_OUTER: LAUNCH_PROBE_EMIT(true, true); break;
            default: LAUNCH_PROBE_EMIT(false, false);
        }
#undef LAUNCH_MK_EMIT
#undef LAUNCH_PROBE_EMIT
        hot_end();
        CHKV(hipStreamSynchronize(g_stream));
        outq.push_back(std::move(op));
    }
    /* modes 5/6: the unmatched build rows, in build-row order, through the
     * stable selection path — the build-row arrays presented as a page
     * {marks u8, payloads...} filtered by marks == 0 */
    void drain()
    {
        const int np = (int)t->payload.size();
        pg_page bpg{};
        bpg.n_rows = t->n_rows;
        bpg.n_cols = 1 + np;
        bpg.cols[0].tag = PG_T_U8;
        bpg.cols[0].on_device = 1;
        bpg.cols[0].data = marks.p;
        pg_plan_filter_project fp{};
        fp.n_preds = 1;
        fp.preds[0].col = 0;
        fp.preds[0].op = PG_CMP_EQ;
        fp.preds[0].ival = 0;
        fp.n_proj = np;
        for (int o = 0; o < np; o++) {
            bpg.cols[1 + o].tag = payload_tag(t, o);
            bpg.cols[1 + o].on_device = 1;
            bpg.cols[1 + o].data = t->payload[o].p;
            fp.proj[o].kind = PG_PROJ_IDENT;
            fp.proj[o].a = 1 + o;
        }
        int64_t chunk = sel_chunk(bpg.n_rows);
        SelResult r = sel_count(bpg, fp, nullptr, 0, chunk);
        OutPage op;
        op.pg.n_rows = r.n;
        op.pg.n_cols = plan.n_emit + np;
        /* probe side: zeros under one shared all-ones mask */
        op.dev.emplace_back();
        op.dev.back().alloc((size_t)r.n);
        uint8_t* ones = (uint8_t*)op.dev.back().p;
        CHKV(hipMemsetAsync(ones, 1, op.dev.back().sz, g_stream));
        for (int o = 0; o < plan.n_emit; o++) {
            int tag = probe_tags.empty() ? PG_T_I64 : probe_tags[o];
            op.dev.emplace_back();
            op.dev.back().alloc((size_t)r.n * type_size(tag));
            op.dev.back().zero();
            op.pg.cols[o].tag = tag;
            op.pg.cols[o].on_device = 1;
            op.pg.cols[o].data = op.dev.back().p;
            op.pg.cols[o].null_mask = ones;
        }
        emit_outs outs{};
        outs.n = np;
        for (int o = 0; o < np; o++) {
            int tag = payload_tag(t, o);
            op.dev.emplace_back();
            op.dev.back().alloc((size_t)r.n * type_size(tag));
            pg_col& c = op.pg.cols[plan.n_emit + o];
            c.tag = tag;
            c.on_device = 1;
            c.data = op.dev.back().p;
            outs.ptr[o] = c.data;
            outs.tag[o] = tag;
        }
        sel_emit(bpg, fp, nullptr, 0, chunk, r, outs);
        outq.push_back(std::move(op));
    }
    /* the groups page of t from its hit list: columns as in the scan
     * path (key, payloads, dec, f64, cnt), sized at the list count;
     * queues k_groups_emit_list and does not synchronise */
    void extract_by_list(OutPage& op)
    {
        const int64_t total = (int64_t)t->hits_n_host;
        op.pg.n_rows = total;
        int nc = 0;
        auto add_dev_col = [&](int tag) {
            op.dev.emplace_back();
            op.dev.back().alloc((size_t)total * type_size(tag));
            op.pg.cols[nc].tag = tag;
            op.pg.cols[nc].on_device = 1;
            op.pg.cols[nc].data = op.dev.back().p;
            return nc++;
        };
        int c_key = add_dev_col(PG_T_I64);
        build_payloads bp{};
        bp.n = (int32_t)t->payload.size();
        bp.by_slot = t->slot_payloads ? 1 : 0;
        bp.pack_bits = t->pack_bits;
        emit_outs pl_outs{};
        pl_outs.n = bp.n;
        for (int o = 0; o < bp.n; o++) {
            bp.ptr[o] = t->payload[o].p;
            bp.tag[o] = t->ptag[o];
            int c = add_dev_col(t->ptag[o]);
            pl_outs.ptr[o] = op.pg.cols[c].data;
            pl_outs.tag[o] = t->ptag[o];
        }
        int c_dec = add_dev_col(PG_T_I64);
        int c_f64 = add_dev_col(PG_T_F64);
        int c_cnt = add_dev_col(PG_T_I64);
        op.pg.n_cols = nc;
        if (total == 0) return;
        hipLaunchKernelGGL(k_groups_emit_list,
                           dim3((unsigned)((total + 255) / 256)), dim3(256),
                           0, g_stream, (const void*)t->hits.p,
                           (int32_t)(t->cap > (1ll << 32)), total,
                           (const int64_t*)t->keys.p,
                           (const int32_t*)t->head.p,
                           (const unsigned long long*)t->acc.p,
                           t->acc_words, bp,
                           (int64_t*)op.pg.cols[c_key].data, pl_outs,
                           (int64_t*)op.pg.cols[c_dec].data,
                           (double*)op.pg.cols[c_f64].data,
                           (int64_t*)op.pg.cols[c_cnt].data);
    }
    void finish() override
    {
        if (marking()) {
            drain();
            return;
        }
        if (plan.mode == 2) {
            unsigned long long h[33];
            CHKV(hipMemcpy(h, m2_acc.p, sizeof(h), hipMemcpyDeviceToHost));
            if (h[32])
                throw std::runtime_error(
                    "decimal SUM overflow in fused probe "
                    "(Math.addExact semantics)");
            int n_out = 0;
            for (int g = 0; g < plan.n_group_vals; g++)
                if (h[24 + g]) n_out++;
            OutPage op;
            op.pg.n_rows = n_out;
            op.pg.n_cols = 4;
            op.host.emplace_back(n_out ? n_out : 1);
            op.host.emplace_back((size_t)(n_out ? n_out : 1) * 8);
            op.host.emplace_back((size_t)(n_out ? n_out : 1) * 8);
            op.host.emplace_back((size_t)(n_out ? n_out : 1) * 8);
            op.pg.cols[0].tag = PG_T_U8;
            op.pg.cols[1].tag = PG_T_I64;
            op.pg.cols[2].tag = PG_T_F64;
            op.pg.cols[3].tag = PG_T_I64;
            for (int c = 0; c < 4; c++) {
                op.pg.cols[c].on_device = 0;
                op.pg.cols[c].data = op.host[c].data();
            }
            int row = 0;
            for (int g = 0; g < plan.n_group_vals; g++) {
                if (!h[24 + g]) continue;
                ((uint8_t*)op.pg.cols[0].data)[row] = plan.group_vals[g];
                ((int64_t*)op.pg.cols[1].data)[row] = (int64_t)h[g];
                ((double*)op.pg.cols[2].data)[row] =
                    fx128_to_f64(h[16 + g], h[8 + g]);
                ((int64_t*)op.pg.cols[3].data)[row] = (int64_t)h[24 + g];
                row++;
            }
            outq.push_back(std::move(op));
            return;
        }
        if (plan.mode != 1 && plan.mode != 3) return;
        /* list extraction (mode 1, single aggregate): gather the slots
         * the probes first touched.  One key line and one accumulator
         * line per group against one sweep of the accumulator array: an
         * all-keys-hit probe of a well-filled table stays on the scan.
         * The kernel is queued ahead of the overflow read-back, whose
         * synchronise is then the only one of this finish(). */
        OutPage lop;
        const bool by_list =
            plan.mode == 1 && plan.n_aggs == 0 && t->list_ok &&
            !t->range_group && t->hits_n_host <= (uint64_t)t->hits_cap &&
            (double)t->hits_n_host * 128.0 <
                (double)t->cap * t->acc_words * 8.0;
        if (by_list) extract_by_list(lop);
        {
            unsigned long long h_ovf[2] = {0, 0};
            CHKV(hipMemcpyAsync(h_ovf, ovf.p, 16, hipMemcpyDeviceToHost,
                                g_stream));
            CHKV(hipStreamSynchronize(g_stream));
            if (h_ovf[0])
                throw std::runtime_error(
                    "bigint/decimal SUM overflow in grouped probe "
                    "(Math.addExact semantics, "
                    "LongSumAggregation.java:33-37)");
            if (h_ovf[1])
                throw std::runtime_error(
                    "SUM_F64 addend outside the exact fixed-point domain "
                    "in grouped probe (needs 0 <= x < 2^53 with no "
                    "fraction bits below 2^-64)");
        }
        if (by_list) {
            g_groups_list_extractions++;
            outq.push_back(std::move(lop));
            return;
        }
        /* extract groups: slots with count>0, slot-ascending (mode 3
         * groups live in table2) */
        Table* gt = plan.mode == 3 ? t2 : t;
        const bool multi = plan.mode == 1 && plan.n_aggs > 0;
        int64_t cap = gt->cap;
        int64_t chunk = (cap + FLT_NB - 1) / FLT_NB;
        chunk = (chunk + 255) / 256 * 256;
        if (chunk < 256) chunk = 256;
        /* single-pass extraction: groups <= inserted build rows, so the
         * output buffers are sized at that bound and the emit kernel
         * reserves per-block spans off one cursor (n_rows read back).
         * Range-group tables have no build rows — their bound is the
         * whole range, far beyond the real group count, so size them
         * with an exact count pass (one scan of the accumulators). */
        int64_t total = gt->n_rows;
        if (gt->range_group) {
            DevBuf d_counts;
            d_counts.alloc(FLT_NB * 8);
            const unsigned long long* cacc =
                multi ? (const unsigned long long*)gt->acc_multi.p
                      : (const unsigned long long*)gt->acc.p;
            int64_t stride_w =
                multi ? gt->acc_stride : gt->acc_words;
            int64_t cnt_off = stride_w - 1;
            int32_t cnt_shift = 0;
            unsigned long long cnt_mask = ~0ull;
            if (multi && plan.acc_pack) {
                cnt_off = 0;
                cnt_shift = plan.acc_pack_cnt_shift;
                cnt_mask = (1ull << plan.acc_pack_cnt_width) - 1;
            }
            hipLaunchKernelGGL(k_groups_count, dim3(FLT_NB), dim3(256),
                               0, g_stream, cacc, stride_w, cnt_off,
                               cnt_shift, cnt_mask,
                               cap, chunk, (int64_t*)d_counts.p);
            std::vector<int64_t> hc(FLT_NB);
            CHKV(hipMemcpyAsync(hc.data(), d_counts.p, FLT_NB * 8,
                                hipMemcpyDeviceToHost, g_stream));
            CHKV(hipStreamSynchronize(g_stream));
            total = 0;
            for (int b = 0; b < FLT_NB; b++) total += hc[b];
        }
        DevBuf d_cursor;
        d_cursor.alloc(8);
        d_cursor.zero();
        OutPage op;
        op.pg.n_rows = total;
        int nc = 0;
        auto add_dev_col = [&](int tag) {
            op.dev.emplace_back();
            op.dev.back().alloc((size_t)total * type_size(tag));
            op.pg.cols[nc].tag = tag;
            op.pg.cols[nc].on_device = 1;
            op.pg.cols[nc].data = op.dev.back().p;
            return nc++;
        };
        int c_key = add_dev_col(PG_T_I64);
        build_payloads bp{};
        bp.n = (int32_t)gt->payload.size();
        bp.by_slot = gt->slot_payloads ? 1 : 0;
        bp.pack_bits = gt->pack_bits;
        emit_outs pl_outs{};
        pl_outs.n = bp.n;
        for (int o = 0; o < bp.n; o++) {
            bp.ptr[o] = gt->payload[o].p;
            bp.tag[o] = gt->ptag[o];
            int c = add_dev_col(gt->ptag[o]);
            pl_outs.ptr[o] = op.pg.cols[c].data;
            pl_outs.tag[o] = gt->ptag[o];
        }
        if (multi) {
            emit_outs agg_outs{};
            agg_outs.n = plan.n_aggs + 1;
            for (int a = 0; a <= plan.n_aggs; a++) {
                int c = add_dev_col(PG_T_I64);
                agg_outs.ptr[a] = op.pg.cols[c].data;
                agg_outs.tag[a] = PG_T_I64;
            }
            op.pg.n_cols = nc;
            acc_pack_desc pk{};
            pk.on = plan.acc_pack;
            for (int a = 0; a < 6; a++) {
                pk.shift[a] = plan.acc_pack_shift[a];
                pk.width[a] = plan.acc_pack_width[a];
            }
            pk.cnt_shift = plan.acc_pack_cnt_shift;
            pk.cnt_width = plan.acc_pack_cnt_width;
            hipLaunchKernelGGL(
                k_groups_emit_multi, dim3(FLT_NB), dim3(256), 0, g_stream,
                (const int64_t*)gt->keys.p,
                (const unsigned long long*)gt->acc_multi.p,
                gt->acc_stride, plan.n_aggs, bp, cap, chunk,
                (unsigned long long*)d_cursor.p,
                (int64_t*)op.pg.cols[c_key].data, pl_outs, agg_outs, pk);
            unsigned long long n_out = 0;
            CHKV(hipMemcpyAsync(&n_out, d_cursor.p, 8,
                                hipMemcpyDeviceToHost, g_stream));
            CHKV(hipStreamSynchronize(g_stream));
            op.pg.n_rows = (int64_t)n_out;
            outq.push_back(std::move(op));
            return;
        }
        int c_dec = add_dev_col(PG_T_I64);
        int c_f64 = add_dev_col(PG_T_F64);
        int c_cnt = add_dev_col(PG_T_I64);
        op.pg.n_cols = nc;
        hipLaunchKernelGGL(k_groups_emit, dim3(FLT_NB), dim3(256), 0,
                           g_stream, (const int64_t*)gt->keys.p,
                           (const int32_t*)gt->head.p,
                           (const unsigned long long*)gt->acc.p,
                           gt->acc_words, bp, cap,
                           chunk, (unsigned long long*)d_cursor.p,
                           (int64_t*)op.pg.cols[c_key].data, pl_outs,
                           (int64_t*)op.pg.cols[c_dec].data,
                           (double*)op.pg.cols[c_f64].data,
                           (int64_t*)op.pg.cols[c_cnt].data);
        unsigned long long n_out = 0;
        CHKV(hipMemcpyAsync(&n_out, d_cursor.p, 8, hipMemcpyDeviceToHost,
                            g_stream));
        CHKV(hipStreamSynchronize(g_stream));
        op.pg.n_rows = (int64_t)n_out;
        outq.push_back(std::move(op));
    }
};

/* ---------------- GROUPBY_MULTI ---------------- */
struct GroupByOp : Op {
    pg_plan_groupby plan;
    DevBuf state, kv, acc, counters;
    int32_t acc_words = 0;
    gb_agg_off offs{};
    int64_t cap = 0, mask = 0;
    int32_t key_out_tag[4] = {0, 0, 0, 0};
    bool tags_known = false;
    bool sql = false; /* plan.sql_nulls == 1 */
    void init()
    {
        if (plan.n_keys < 1 || plan.n_keys > 4)
            throw std::runtime_error("groupby needs 1..4 key channels");
        if (plan.n_aggs < 1 || plan.n_aggs > 6)
            throw std::runtime_error("groupby needs 1..6 aggregates");
        for (int a = 0; a < plan.n_aggs; a++)
            if (plan.agg_filter[a] >= PG_MAX_PRED)
                throw std::runtime_error("agg_filter out of range");
        check_pred_lens("GROUPBY_MULTI", plan.preds,
                        preds_used(plan.n_preds, plan.agg_filter,
                                   plan.n_aggs));
        if (plan.capacity_hint < 1)
            throw std::runtime_error("capacity_hint required");
        if (plan.sql_nulls != 0 && plan.sql_nulls != 1)
            throw std::runtime_error("groupby sql_nulls must be 0 or 1");
        sql = plan.sql_nulls == 1;
        cap = next_pow2(plan.capacity_hint * 2 + 16);
        mask = cap - 1;
        int w = 0;
        for (int a = 0; a < plan.n_aggs; a++) {
            offs.off[a] = w;
            w += plan.aggs[a].func == PG_AGG_SUM_F64 ? 2 : 1;
        }
        /* + group row count, always the last word; sql_nulls puts the
         * "received input" bits in front of it */
        acc_words = w + (sql ? 2 : 1);
        state.alloc((size_t)cap * 4);
        state.zero();
        /* sql_nulls: one more plane, the per-channel null bits */
        kv.alloc((size_t)cap * 8 * (plan.n_keys + (sql ? 1 : 0)));
        acc.alloc((size_t)cap * acc_words * 8);
        acc.zero();
        counters.alloc(32); /* [tick ovf, table full, distinct groups,
                               SUM_F64 domain] */
        counters.zero();
        bool mm = false;
        for (int a = 0; a < plan.n_aggs; a++)
            mm = mm || plan.aggs[a].func == PG_AGG_MIN ||
                 plan.aggs[a].func == PG_AGG_MAX;
        if (mm)
            hipLaunchKernelGGL(k_gb_acc_init, dim3(1024), dim3(256), 0,
                               g_stream, (unsigned long long*)acc.p, cap,
                               acc_words, offs, plan);
    }
    void add_input(const pg_page* in) override
    {
        check_pred_types("GROUPBY_MULTI", plan.preds,
                         preds_used(plan.n_preds, plan.agg_filter,
                                    plan.n_aggs),
                         in);
        StagedPage sp;
        sp.stage(in);
        for (int ch = 0; ch < plan.n_keys; ch++) {
            const pg_col& c = sp.pg.cols[plan.key_col[ch]];
            if (c.tag == PG_T_F64)
                throw std::runtime_error("f64 group keys unsupported");
            if (c.tag == PG_T_VARBIN && !c.dict_ids)
                throw std::runtime_error(
                    "varbin group keys must be dictionary blocks "
                    "(group identity = dictionary id)");
            int tag = c.tag == PG_T_VARBIN ? PG_T_I32 : c.tag;
            if (!tags_known)
                key_out_tag[ch] = tag;
            else if (key_out_tag[ch] != tag)
                throw std::runtime_error("key column type changed");
        }
        tags_known = true;
        hot_begin();
        hipLaunchKernelGGL(sql ? k_groupby_multi<true>
                               : k_groupby_multi<false>,
                           dim3(4096), dim3(256), 0, g_stream, sp.pg, plan,
                           (unsigned int*)state.p, (int64_t*)kv.p, cap,
                           mask, (unsigned long long*)acc.p, acc_words,
                           offs, (unsigned long long*)counters.p);
        hot_end();
        CHKV(hipStreamSynchronize(g_stream));
    }
    void finish() override
    {
        unsigned long long c[4];
        CHKV(hipMemcpy(c, counters.p, 32, hipMemcpyDeviceToHost));
        if (c[1])
            throw std::runtime_error(
                "groupby table full: raise capacity_hint");
        if (c[0])
            throw std::runtime_error(
                "bigint/decimal SUM overflow in groupby "
                "(Math.addExact semantics)");
        if (c[3])
            throw std::runtime_error(
                "SUM_F64 addend outside the exact fixed-point domain in "
                "groupby (needs 0 <= x < 2^53 with no fraction bits below "
                "2^-64)");
        int64_t total = (int64_t)c[2]; /* distinct groups, counted at
                                          claim time */
        if (total * 100 > cap * 85)
            throw std::runtime_error(
                "groupby fill exceeded 0.85: raise capacity_hint");
        int64_t chunk = (cap + FLT_NB - 1) / FLT_NB;
        chunk = (chunk + 255) / 256 * 256;
        if (chunk < 256) chunk = 256;
        DevBuf d_cursor;
        d_cursor.alloc(8);
        d_cursor.zero();
        OutPage op;
        op.pg.n_rows = total;
        int nc = 0;
        auto add_dev_col = [&](int tag) {
            op.dev.emplace_back();
            op.dev.back().alloc((size_t)total * type_size(tag) + 1);
            op.pg.cols[nc].tag = tag;
            op.pg.cols[nc].on_device = 1;
            op.pg.cols[nc].data = op.dev.back().p;
            return nc++;
        };
        /* sql_nulls: one byte per group, owned by the page like the
         * values */
        auto add_mask = [&](int cx) {
            op.dev.emplace_back();
            op.dev.back().alloc((size_t)total + 1);
            op.pg.cols[cx].null_mask = (const uint8_t*)op.dev.back().p;
            return op.dev.back().p;
        };
        emit_outs key_outs{}, key_masks{};
        key_outs.n = key_masks.n = plan.n_keys;
        for (int ch = 0; ch < plan.n_keys; ch++) {
            int tag = tags_known ? key_out_tag[ch] : PG_T_I64;
            int cx = add_dev_col(tag);
            key_outs.ptr[ch] = op.pg.cols[cx].data;
            key_outs.tag[ch] = tag;
            if (sql) key_masks.ptr[ch] = add_mask(cx);
        }
        emit_outs agg_outs{}, agg_masks{};
        agg_outs.n = plan.n_aggs + 1;
        agg_masks.n = plan.n_aggs;
        for (int a = 0; a < plan.n_aggs; a++) {
            int tag = plan.aggs[a].func == PG_AGG_SUM_F64 ? PG_T_F64
                                                          : PG_T_I64;
            int cx = add_dev_col(tag);
            agg_outs.ptr[a] = op.pg.cols[cx].data;
            agg_outs.tag[a] = tag;
            if (sql && plan.aggs[a].func != PG_AGG_COUNT)
                agg_masks.ptr[a] = add_mask(cx);
        }
        {
            int cx = add_dev_col(PG_T_I64);
            agg_outs.ptr[plan.n_aggs] = op.pg.cols[cx].data;
            agg_outs.tag[plan.n_aggs] = PG_T_I64;
        }
        op.pg.n_cols = nc;
        hipLaunchKernelGGL(sql ? k_groupby_emit<true>
                               : k_groupby_emit<false>,
                           dim3(FLT_NB), dim3(256), 0,
                           g_stream, (const int64_t*)kv.p, cap,
                           plan.n_keys,
                           (const unsigned long long*)acc.p, acc_words,
                           offs, plan, chunk,
                           (unsigned long long*)d_cursor.p,
                           key_outs, agg_outs, key_masks, agg_masks);
        unsigned long long n_out = 0;
        CHKV(hipMemcpyAsync(&n_out, d_cursor.p, 8, hipMemcpyDeviceToHost,
                            g_stream));
        CHKV(hipStreamSynchronize(g_stream));
        op.pg.n_rows = (int64_t)n_out;
        outq.push_back(std::move(op));
    }
};

/* ---------------- TOPN ---------------- */
struct TopNOp : Op {
    pg_plan_topn plan;
    struct Cand {
        int64_t val_bits;
        int64_t key;
        int32_t date;
        bool is_f64;
    };
    std::vector<Cand> cands;
    bool is_f64 = false;
    bool less(const Cand& a, const Cand& b)
    {
        /* a ranks worse than b */
        if (a.val_bits != b.val_bits) {
            if (is_f64) {
                double x, y;
                memcpy(&x, &a.val_bits, 8);
                memcpy(&y, &b.val_bits, 8);
                return x < y;
            }
            return a.val_bits < b.val_bits;
        }
        if (a.date != b.date) return a.date > b.date;
        return a.key > b.key;
    }
    void add_input(const pg_page* in) override
    {
        StagedPage sp;
        sp.stage(in);
        is_f64 = sp.pg.cols[plan.val_col].tag == PG_T_F64;
        int L = plan.limit;
        if (L > (1 << 20))
            throw std::runtime_error("limit > 1M unsupported");
        if (L > TOPN_MAXL) {
            /* histogram preselect (see k_topn_hist) */
            DevBuf hist;
            hist.alloc(65536 * 8);
            hist.zero();
            hipLaunchKernelGGL(k_topn_hist, dim3(2048), dim3(256), 0,
                               g_stream, sp.pg.cols[plan.val_col].data,
                               is_f64 ? 1 : 0, sp.pg.n_rows,
                               (unsigned long long*)hist.p);
            std::vector<unsigned long long> h(65536);
            CHKV(hipMemcpyAsync(h.data(), hist.p, 65536 * 8,
                                hipMemcpyDeviceToHost, g_stream));
            CHKV(hipStreamSynchronize(g_stream));
            int64_t cum = 0;
            int bin = 65535;
            for (; bin >= 0; bin--) {
                cum += (int64_t)h[bin];
                if (cum >= L) break;
            }
            if (bin < 0) bin = 0;
            uint64_t floor_sortable = (uint64_t)bin << 48;
            DevBuf cand, cur;
            cand.alloc((size_t)(cum ? cum : 1) * sizeof(topn_cand));
            cur.alloc(8);
            cur.zero();
            hipLaunchKernelGGL(k_topn_collect, dim3(2048), dim3(256), 0,
                               g_stream, sp.pg.cols[plan.val_col].data,
                               is_f64 ? 1 : 0,
                               (const int32_t*)
                                   sp.pg.cols[plan.date_col].data,
                               (const int64_t*)
                                   sp.pg.cols[plan.key_col].data,
                               sp.pg.n_rows, floor_sortable,
                               (topn_cand*)cand.p, cum,
                               (unsigned long long*)cur.p);
            std::vector<topn_cand> hc(cum);
            if (cum)
                CHKV(hipMemcpyAsync(hc.data(), cand.p,
                                    (size_t)cum * sizeof(topn_cand),
                                    hipMemcpyDeviceToHost, g_stream));
            CHKV(hipStreamSynchronize(g_stream));
            for (auto& c : hc)
                if (c.valid)
                    cands.push_back({c.val_bits, c.key, c.date, is_f64});
            return;
        }
        DevBuf bout;
        bout.alloc((size_t)TOPN_NB * L * sizeof(topn_cand));
        hipLaunchKernelGGL(k_topn, dim3(TOPN_NB), dim3(256), 0, g_stream,
                           sp.pg.cols[plan.val_col].data, is_f64 ? 1 : 0,
                           (const int32_t*)sp.pg.cols[plan.date_col].data,
                           (const int64_t*)sp.pg.cols[plan.key_col].data,
                           sp.pg.n_rows, L, (topn_cand*)bout.p);
        std::vector<topn_cand> h((size_t)TOPN_NB * L);
        CHKV(hipMemcpyAsync(h.data(), bout.p, h.size() * sizeof(topn_cand),
                            hipMemcpyDeviceToHost, g_stream));
        CHKV(hipStreamSynchronize(g_stream));
        for (auto& c : h)
            if (c.valid)
                cands.push_back({c.val_bits, c.key, c.date, is_f64});
    }
    void finish() override
    {
        std::sort(cands.begin(), cands.end(),
                  [&](const Cand& a, const Cand& b) { return less(b, a); });
        int n = (int)std::min<size_t>(plan.limit, cands.size());
        OutPage op;
        op.pg.n_rows = n;
        op.pg.n_cols = 3;
        op.host.emplace_back((size_t)n * 8);
        op.host.emplace_back((size_t)n * (is_f64 ? 8 : 8));
        op.host.emplace_back((size_t)n * 4);
        op.pg.cols[0] = {PG_T_I64, 0, op.host[0].data(), nullptr};
        op.pg.cols[1] = {is_f64 ? PG_T_F64 : PG_T_I64, 0, op.host[1].data(),
                         nullptr};
        op.pg.cols[2] = {PG_T_I32, 0, op.host[2].data(), nullptr};
        for (int i = 0; i < n; i++) {
            ((int64_t*)op.pg.cols[0].data)[i] = cands[i].key;
            ((int64_t*)op.pg.cols[1].data)[i] = cands[i].val_bits;
            ((int32_t*)op.pg.cols[2].data)[i] = cands[i].date;
        }
        outq.push_back(std::move(op));
    }
};

/* ---------------- PARTITION ---------------- */
struct PartitionOp : Op {
    pg_plan_partition plan;
    std::vector<int64_t> pcounts;
    std::vector<DevBuf> owned; /* partition column buffers; pages alias */
    void add_input(const pg_page* in) override
    {
        /* the scatter copies fixed-width values (VARBIN emit is
         * FILTER_PROJECT's two-pass gather): refuse before any launch.  A
         * VARBIN key is fine: it is hashed, not emitted. */
        for (int o = 0; o < plan.n_emit && o < 8; o++) {
            const int32_t ec = plan.emit_cols[o];
            if (ec >= 0 && ec < in->n_cols &&
                in->cols[ec].tag == PG_T_VARBIN)
                throw std::runtime_error(
                    "PARTITION emits fixed-width columns only: emit_cols[" +
                    std::to_string(o) + "] is VARBIN column " +
                    std::to_string(ec));
        }
        StagedPage sp;
        sp.stage(in);
        int P = plan.n_partitions;
        if (P > PART_MAXP) throw std::runtime_error("too many partitions");
        int64_t n = sp.pg.n_rows;
        int64_t chunk = (n + PART_NB - 1) / PART_NB;
        chunk = (chunk + 255) / 256 * 256;
        if (chunk < 256) chunk = 256;
        DevBuf d_counts;
        d_counts.alloc((size_t)PART_NB * P * 8);
        hipLaunchKernelGGL(k_part_count, dim3(PART_NB), dim3(256), 0,
                           g_stream, sp.pg, plan, chunk,
                           (int64_t*)d_counts.p);
        std::vector<int64_t> h((size_t)PART_NB * P);
        CHKV(hipMemcpyAsync(h.data(), d_counts.p, h.size() * 8,
                            hipMemcpyDeviceToHost, g_stream));
        CHKV(hipStreamSynchronize(g_stream));
        pcounts.assign(P, 0);
        for (int b = 0; b < PART_NB; b++)
            for (int p = 0; p < P; p++) pcounts[p] += h[(size_t)b * P + p];
        /* block_offs[b][p] = part_base[p] + sum_{b'<b} counts[b'][p] */
        std::vector<int64_t> part_base(P + 1, 0);
        for (int p = 0; p < P; p++)
            part_base[p + 1] = part_base[p] + pcounts[p];
        std::vector<int64_t> offs((size_t)PART_NB * P);
        std::vector<int64_t> run(P, 0);
        for (int b = 0; b < PART_NB; b++)
            for (int p = 0; p < P; p++) {
                offs[(size_t)b * P + p] = part_base[p] + run[p];
                run[p] += h[(size_t)b * P + p];
            }
        DevBuf d_offs;
        d_offs.alloc(offs.size() * 8);
        CHKV(hipMemcpyAsync(d_offs.p, offs.data(), offs.size() * 8,
                            hipMemcpyHostToDevice, g_stream));
        /* output: one buffer per emit col spanning all partitions; P pages
         * pointing at slices */
        std::vector<DevBuf> colbufs;
        emit_outs outs{};
        outs.n = plan.n_emit;
        std::vector<int> tags(plan.n_emit);
        for (int o = 0; o < plan.n_emit; o++) {
            tags[o] = sp.pg.cols[plan.emit_cols[o]].tag;
            colbufs.emplace_back();
            colbufs.back().alloc((size_t)n * type_size(tags[o]));
            outs.ptr[o] = colbufs.back().p;
            outs.tag[o] = tags[o];
        }
        hipLaunchKernelGGL(k_part_emit, dim3(PART_NB), dim3(256), 0,
                           g_stream, sp.pg, plan, chunk,
                           (const int64_t*)d_offs.p, outs);
        CHKV(hipStreamSynchronize(g_stream));
        for (auto& b : colbufs) owned.push_back(std::move(b));
        for (int p = 0; p < P; p++) {
            OutPage op;
            op.pg.n_rows = pcounts[p];
            op.pg.n_cols = plan.n_emit;
            for (int o = 0; o < plan.n_emit; o++) {
                op.pg.cols[o].tag = tags[o];
                op.pg.cols[o].on_device = 1;
                op.pg.cols[o].data = (int8_t*)outs.ptr[o] +
                                     part_base[p] * type_size(tags[o]);
                op.pg.cols[o].null_mask = nullptr;
            }
            outq.push_back(std::move(op));
        }
    }
    void finish() override {}
    void partition_counts(int64_t* out, int32_t n) override
    {
        for (int32_t i = 0; i < n && i < (int32_t)pcounts.size(); i++)
            out[i] = pcounts[i];
    }
};

/* the sort's block geometry, shared by the scans of WINDOW: a block owns
 * a chunk of whole SORT_WINDOW-row windows, at most SORT_NB blocks */
static int sort_geometry(int64_t n, int64_t* chunk_out)
{
    int64_t chunk = (n + SORT_NB - 1) / SORT_NB;
    chunk = (chunk + SORT_WINDOW - 1) / SORT_WINDOW * SORT_WINDOW;
    chunk = std::max<int64_t>(chunk, SORT_MIN_WINDOWS * SORT_WINDOW);
    *chunk_out = chunk;
    return (int)((n + chunk - 1) / chunk);
}

/* ---------------- what ORDER_BY and WINDOW share ---------------- */
/* page accumulation into per-column slots, their concatenation, the
 * sorted row-id permutation and the gather of the emit columns.  The
 * operator sets opname, the key list and the emit list from its plan. */
struct SortedInputOp : Op {
    const char* opname = ""; /* "ORDER_BY" / "WINDOW": prefixes errors */
    int n_keys = 0, n_emit = 0;
    const int32_t *key_col = nullptr, *order = nullptr, *emit_cols = nullptr;
    /* one slot per distinct input column the plan names, as key, as emit
     * column, as function argument or several of these: the per-page
     * copies, then the concatenation */
    struct Slot {
        int col = 0;
        int tag = PG_T_I64; /* the first page's; I64 until one is fed */
        bool has_mask = false;
        std::vector<DevBuf> data, mask; /* per page; mask unallocated
                                           where the page had none */
        DevBuf all, all_mask;
    };
    std::vector<Slot> slots;
    int key_slot[PG_MAX_SORT_KEYS], emit_slot[PG_MAX_SORT_EMIT];
    std::vector<int64_t> page_rows;
    int64_t n_total = 0;
    bool typed = false;

    std::string err(const std::string& what) const
    {
        return std::string(opname) + ": " + what;
    }
    std::string fname(const char* field, int i) const
    {
        return err(field) + "[" + std::to_string(i) + "]";
    }
    int slot_of(int col)
    {
        for (size_t s = 0; s < slots.size(); s++)
            if (slots[s].col == col) return (int)s;
        slots.emplace_back();
        slots.back().col = col;
        return (int)slots.size() - 1;
    }
    /* after the operator has checked its counts: the per-entry checks of
     * the key and emit lists, and their slots */
    void init_keys_and_emit()
    {
        for (int i = 0; i < n_keys; i++) {
            if (order[i] < PG_SORT_ASC_NULLS_FIRST ||
                order[i] > PG_SORT_DESC_NULLS_LAST)
                throw std::runtime_error(fname("order", i) +
                                         " is not a pg_sort_order");
            if (key_col[i] < 0)
                throw std::runtime_error(fname("key_col", i) +
                                         " is negative");
        }
        for (int i = 0; i < n_emit; i++)
            if (emit_cols[i] < 0)
                throw std::runtime_error(fname("emit_cols", i) +
                                         " is negative");
        for (int i = 0; i < n_keys; i++) key_slot[i] = slot_of(key_col[i]);
        for (int i = 0; i < n_emit; i++)
            emit_slot[i] = slot_of(emit_cols[i]);
    }
    /* the operator's own per-page checks, beyond keys and emit columns */
    virtual void check_more(const pg_page*) {}
    void check_col(const pg_page* in, const std::string& name, int c,
                   bool is_key)
    {
        if (c >= in->n_cols)
            throw std::runtime_error(name + " = " + std::to_string(c) +
                                     " is not a column of the page (n_cols " +
                                     std::to_string(in->n_cols) + ")");
        const pg_col& col = in->cols[c];
        if (col.tag == PG_T_VARBIN || col.dict_ids)
            throw std::runtime_error(name + ": VARBIN and dictionary "
                                     "columns are unsupported");
        if (col.tag == PG_T_I128 && is_key)
            throw std::runtime_error(name + ": I128 keys are unsupported");
        if (col.tag != PG_T_U8 && col.tag != PG_T_I32 &&
            col.tag != PG_T_I64 && col.tag != PG_T_F64 &&
            col.tag != PG_T_I128)
            throw std::runtime_error(name + ": unknown column type " +
                                     std::to_string(col.tag));
        const Slot& s = slots[slot_of(c)];
        if (typed && s.tag != col.tag)
            throw std::runtime_error(
                name + ": type " + std::to_string(col.tag) +
                " differs from the first page's " + std::to_string(s.tag));
    }
    void add_input(const pg_page* in) override
    {
        /* every check before the first copy: a rejected page leaves the
         * operator as it was */
        if (in->n_rows < 0) throw std::runtime_error(err("n_rows < 0"));
        for (int i = 0; i < n_keys; i++)
            check_col(in, fname("key_col", i), key_col[i], true);
        for (int i = 0; i < n_emit; i++)
            check_col(in, fname("emit_cols", i), emit_cols[i], false);
        check_more(in);
        const int64_t n = in->n_rows;
        if (n_total + n > INT32_MAX)
            throw std::runtime_error(err("more than 2^31-1 accumulated "
                                         "rows (row ids are 32-bit)"));
        for (auto& s : slots) {
            const pg_col& col = in->cols[s.col];
            s.tag = col.tag;
            hipMemcpyKind kind = col.on_device ? hipMemcpyDeviceToDevice
                                               : hipMemcpyHostToDevice;
            s.data.emplace_back();
            s.mask.emplace_back();
            size_t nb = (size_t)n * type_size(col.tag);
            s.data.back().alloc(nb);
            if (nb)
                CHKV(hipMemcpyAsync(s.data.back().p, col.data, nb, kind,
                                    g_stream));
            if (col.null_mask) {
                s.has_mask = true;
                s.mask.back().alloc((size_t)n);
                if (n)
                    CHKV(hipMemcpyAsync(s.mask.back().p, col.null_mask,
                                        (size_t)n, kind, g_stream));
            }
        }
        /* the page is borrowed for the call only */
        CHKV(hipStreamSynchronize(g_stream));
        typed = true;
        page_rows.push_back(n);
        n_total += n;
    }
    /* per-page copies -> one column; a page without a mask contributes
     * zeros to a column that has one */
    void concat(Slot& s)
    {
        const size_t w = type_size(s.tag);
        if (s.data.size() == 1) {
            s.all = std::move(s.data[0]);
        } else {
            s.all.alloc((size_t)n_total * w);
            size_t off = 0;
            for (size_t p = 0; p < s.data.size(); p++) {
                size_t nb = (size_t)page_rows[p] * w;
                if (nb)
                    CHKV(hipMemcpyAsync((int8_t*)s.all.p + off, s.data[p].p,
                                        nb, hipMemcpyDeviceToDevice,
                                        g_stream));
                off += nb;
            }
        }
        if (s.has_mask) {
            s.all_mask.alloc((size_t)n_total);
            s.all_mask.zero();
            size_t off = 0;
            for (size_t p = 0; p < s.mask.size(); p++) {
                if (s.mask[p].p && page_rows[p])
                    CHKV(hipMemcpyAsync((int8_t*)s.all_mask.p + off,
                                        s.mask[p].p, (size_t)page_rows[p],
                                        hipMemcpyDeviceToDevice, g_stream));
                off += (size_t)page_rows[p];
            }
        }
        /* stream order: the chunks go back to the pool only after the
         * copies out of them are queued, and the pool's next user runs
         * on the same stream */
        s.data.clear();
        s.mask.clear();
    }
    /* the sorted permutation of [0, n): a fixed launch sequence on
     * g_stream with one host read (the digit histograms) per key.
     * Allocates the id buffers it needs and returns which of the two
     * holds the result: NULL for no rows, the identity for one row or no
     * keys. */
    const uint32_t* sort_ids(int64_t n, DevBuf& idA, DevBuf& idB)
    {
        if (n == 0) return nullptr;
        idA.alloc((size_t)n * 4);
        const int sgrid = (int)std::min<int64_t>((n + 255) / 256, 2048);
        if (n == 1 || n_keys == 0) {
            hipLaunchKernelGGL(k_sort_iota, dim3(sgrid), dim3(256), 0,
                               g_stream, (uint32_t*)idA.p, n);
            return (const uint32_t*)idA.p;
        }
        idB.alloc((size_t)n * 4);
        DevBuf kA, kB, hist, counts;
        kA.alloc((size_t)n * 8);
        kB.alloc((size_t)n * 8);
        hist.alloc(8 * 256 * 4);
        int64_t chunk;
        const int nb = sort_geometry(n, &chunk);
        counts.alloc((size_t)256 * nb * 4);
        uint64_t *kin = (uint64_t*)kA.p, *kout = (uint64_t*)kB.p;
        uint32_t *iin = (uint32_t*)idA.p, *iout = (uint32_t*)idB.p;
        /* one pass over digit `shift / 8`; hist holds the histograms of
         * the keys being sorted */
        auto pass = [&](int shift) {
            hipLaunchKernelGGL(k_radix_count, dim3(nb), dim3(256), 0,
                               g_stream, kin, n, shift, chunk,
                               (uint32_t*)counts.p);
            hipLaunchKernelGGL(k_radix_scan, dim3(256), dim3(256), 0,
                               g_stream, (uint32_t*)counts.p, nb,
                               (const uint32_t*)hist.p + shift / 8 * 256);
            hipLaunchKernelGGL(k_radix_scatter, dim3(nb), dim3(256), 0,
                               g_stream, kin, iin, kout, iout, n, shift,
                               chunk, (const uint32_t*)counts.p);
            std::swap(kin, kout);
            std::swap(iin, iout);
        };
        std::vector<uint32_t> h(8 * 256);
        for (int k = n_keys - 1; k >= 0; k--) {
            const Slot& s = slots[key_slot[k]];
            const uint8_t* mask =
                s.has_mask ? (const uint8_t*)s.all_mask.p : nullptr;
            const bool first = k == n_keys - 1;
            hipLaunchKernelGGL(k_sort_encode, dim3(sgrid), dim3(256), 0,
                               g_stream, (const void*)s.all.p, s.tag,
                               order[k], mask, 0,
                               first ? (const uint32_t*)nullptr : iin, iin,
                               kin, n);
            hist.zero();
            hipLaunchKernelGGL(k_sort_digits, dim3(sgrid), dim3(256), 0,
                               g_stream, kin, n, (uint32_t*)hist.p);
            CHKV(hipMemcpyAsync(h.data(), hist.p, 8 * 256 * 4,
                                hipMemcpyDeviceToHost, g_stream));
            CHKV(hipStreamSynchronize(g_stream));
            for (int p = 0; p < 8; p++) {
                /* a digit on which every row agrees moves nothing */
                bool one_bin = false;
                for (int d = 0; d < 256 && !one_bin; d++)
                    one_bin = h[p * 256 + d] == (uint32_t)n;
                if (!one_bin) pass(8 * p);
            }
            if (mask) {
                /* NULLS FIRST/LAST: the key's most significant pass, two
                 * bins over the gathered mask byte */
                hipLaunchKernelGGL(k_sort_encode, dim3(sgrid), dim3(256), 0,
                                   g_stream, (const void*)s.all.p, s.tag,
                                   order[k], mask, 1,
                                   (const uint32_t*)iin, iin, kin, n);
                hist.zero();
                hipLaunchKernelGGL(k_sort_digits, dim3(sgrid), dim3(256), 0,
                                   g_stream, kin, n, (uint32_t*)hist.p);
                pass(0);
            }
        }
        CHKV(hipStreamSynchronize(g_stream)); /* before kA/kB are pooled */
        return iin;
    }
    /* the emit columns of the first n_out sorted rows into columns
     * [0, n_emit) of the output page, each with its gathered mask if it
     * has one */
    void gather_emit(OutPage& op, const uint32_t* ids, int64_t n_out)
    {
        sort_gather_cols g{};
        g.n = n_emit;
        for (int o = 0; o < n_emit; o++) {
            const Slot& s = slots[emit_slot[o]];
            const size_t w = type_size(s.tag);
            op.dev.emplace_back();
            op.dev.back().alloc((size_t)n_out * w);
            g.src[o] = s.all.p;
            g.dst[o] = op.dev.back().p;
            g.width[o] = (int)w;
            op.pg.cols[o].tag = s.tag;
            op.pg.cols[o].on_device = 1;
            op.pg.cols[o].data = g.dst[o];
            op.pg.cols[o].null_mask = nullptr;
            if (s.has_mask) {
                op.dev.emplace_back();
                op.dev.back().alloc((size_t)n_out);
                g.msrc[o] = (const uint8_t*)s.all_mask.p;
                g.mdst[o] = (uint8_t*)op.dev.back().p;
                op.pg.cols[o].null_mask = g.mdst[o];
            }
        }
        if (n_out > 0) {
            const int grid =
                (int)std::min<int64_t>((n_out + 255) / 256, 2048);
            hipLaunchKernelGGL(k_sort_gather, dim3(grid), dim3(256), 0,
                               g_stream, ids, n_out, g);
        }
    }
    void free_slots()
    {
        for (auto& s : slots) {
            s.all.free();
            s.all_mask.free();
        }
    }
};

/* ---------------- ORDER_BY ---------------- */
struct OrderByOp : SortedInputOp {
    pg_plan_order_by plan;
    void init()
    {
        opname = "ORDER_BY";
        if (plan.n_keys < 1 || plan.n_keys > PG_MAX_SORT_KEYS)
            throw std::runtime_error("ORDER_BY: n_keys must be 1..4");
        if (plan.n_emit < 1 || plan.n_emit > PG_MAX_SORT_EMIT)
            throw std::runtime_error("ORDER_BY: n_emit must be 1..16");
        if (plan.limit < 0)
            throw std::runtime_error("ORDER_BY: limit must be >= 0");
        n_keys = plan.n_keys;
        key_col = plan.key_col;
        order = plan.order;
        n_emit = plan.n_emit;
        emit_cols = plan.emit_cols;
        init_keys_and_emit();
    }
    void finish() override
    {
        const int64_t n = n_total;
        for (auto& s : slots) concat(s);
        DevBuf idA, idB;
        const uint32_t* ids = sort_ids(n, idA, idB);
        const int64_t n_out = plan.limit > 0 ? std::min(plan.limit, n) : n;
        OutPage op;
        op.pg.n_rows = n_out;
        op.pg.n_cols = plan.n_emit;
        gather_emit(op, ids, n_out);
        CHKV(hipStreamSynchronize(g_stream));
        free_slots();
        outq.push_back(std::move(op));
    }
};

/* ---------------- WINDOW ---------------- */
struct WindowOp : SortedInputOp {
    pg_plan_window plan;
    int arg_slot[PG_MAX_WIN_FUNCS]; /* -1: the function reads no column */
    std::string failed; /* a finish that failed fails again, the same way */

    static const char* func_name(int f)
    {
        static const char* const names[] = {
            "ROW_NUMBER", "RANK", "DENSE_RANK", "COUNT", "SUM",
            "MIN",        "MAX",  "LAG",        "LEAD"};
        return names[f];
    }
    static bool is_agg(int f) { return f >= PG_WIN_COUNT && f <= PG_WIN_MAX; }
    static bool is_shift(int f) { return f == PG_WIN_LAG || f == PG_WIN_LEAD; }
    std::string fn(int i, const char* field) const
    {
        return fname("funcs", i) + "." + field;
    }
    void init()
    {
        opname = "WINDOW";
        if (plan.n_keys < 0 || plan.n_keys > PG_MAX_SORT_KEYS)
            throw std::runtime_error("WINDOW: n_keys must be 0..4");
        if (plan.n_partition_keys < 0 || plan.n_partition_keys > plan.n_keys)
            throw std::runtime_error(
                "WINDOW: n_partition_keys must be 0..n_keys");
        if (plan.n_emit < 1 || plan.n_emit > PG_MAX_SORT_EMIT)
            throw std::runtime_error("WINDOW: n_emit must be 1..16");
        if (plan.n_funcs < 1 || plan.n_funcs > PG_MAX_WIN_FUNCS)
            throw std::runtime_error("WINDOW: n_funcs must be 1..8");
        n_keys = plan.n_keys;
        key_col = plan.key_col;
        order = plan.order;
        n_emit = plan.n_emit;
        emit_cols = plan.emit_cols;
        init_keys_and_emit();
        for (int i = 0; i < plan.n_funcs; i++) {
            const pg_win_spec& f = plan.funcs[i];
            if (f.func < PG_WIN_ROW_NUMBER || f.func > PG_WIN_LEAD)
                throw std::runtime_error(fn(i, "func") +
                                         " is not a pg_win_func");
            if (is_agg(f.func) && (f.frame < PG_FRAME_RANGE_RUNNING ||
                                   f.frame > PG_FRAME_PARTITION))
                throw std::runtime_error(fn(i, "frame") +
                                         " is not a pg_win_frame");
            if (is_shift(f.func) && f.offset < 0)
                throw std::runtime_error(fn(i, "offset") + " is negative");
            const bool reads = is_shift(f.func) ||
                               (is_agg(f.func) && (f.func != PG_WIN_COUNT ||
                                                   f.col >= 0));
            if (reads && f.col < 0)
                throw std::runtime_error(fn(i, "col") + " is negative (" +
                                         func_name(f.func) +
                                         " needs a column)");
            arg_slot[i] = reads ? slot_of(f.col) : -1;
        }
    }
    void check_more(const pg_page* in) override
    {
        for (int i = 0; i < plan.n_funcs; i++) {
            if (arg_slot[i] < 0) continue;
            const pg_win_spec& f = plan.funcs[i];
            const std::string name = fn(i, "col");
            check_col(in, name, f.col, false);
            const int tag = in->cols[f.col].tag;
            if (f.func >= PG_WIN_SUM && f.func <= PG_WIN_MAX &&
                (tag == PG_T_I128 || tag == PG_T_F64))
                throw std::runtime_error(
                    name + " = " + std::to_string(f.col) +
                    ": I128 and F64 columns are unsupported under " +
                    func_name(f.func));
        }
    }
    void add_input(const pg_page* in) override
    {
        if (!failed.empty()) throw std::runtime_error(failed);
        SortedInputOp::add_input(in);
    }
    /* the three launches of one aggregate's segmented scan */
    template <int K>
    void scan_agg(const win_arg& a, const uint32_t* ids, const uint8_t* flags,
                  int64_t n, int64_t chunk, int nb, void* carry,
                  uint64_t* s_lo, int64_t* s_hi, uint32_t* s_cnt)
    {
        auto* c = (win_acc<K>*)carry;
        hipLaunchKernelGGL(k_win_agg_reduce<K>, dim3(nb), dim3(256), 0,
                           g_stream, a, ids, flags, n, chunk, c);
        hipLaunchKernelGGL(k_win_agg_carry<K>, dim3(1), dim3(256), 0,
                           g_stream, c, nb);
        hipLaunchKernelGGL(k_win_agg_scan<K>, dim3(nb), dim3(256), 0,
                           g_stream, a, ids, flags, n, chunk,
                           (const win_acc<K>*)c, s_lo, s_hi, s_cnt);
    }
    /* everything after the sort, for n >= 1: flags and bounds (three
     * launches), then per function its scan (three launches, aggregates
     * only) and its emit.  All on g_stream, one host read at the end. */
    void run_functions(int64_t n, const uint32_t* ids, OutPage& op)
    {
        int64_t chunk;
        const int nb = sort_geometry(n, &chunk);
        const int grid = (int)std::min<int64_t>((n + 255) / 256, 2048);
        DevBuf flags, fwdc, bwdc, bounds, errs, carry, s_lo, s_hi, s_cnt;
        flags.alloc((size_t)n);
        fwdc.alloc((size_t)nb * sizeof(win_fwd));
        bwdc.alloc((size_t)nb * sizeof(win_bwd));
        bounds.alloc((size_t)n * 4 * 5);
        uint32_t* part_start = (uint32_t*)bounds.p;
        uint32_t* peer_start = part_start + n;
        uint32_t* heads = peer_start + n;
        uint32_t* part_end = heads + n;
        uint32_t* peer_end = part_end + n;
        win_keys wk{};
        wk.n_keys = plan.n_keys;
        wk.n_part = plan.n_partition_keys;
        for (int k = 0; k < plan.n_keys; k++) {
            const Slot& s = slots[key_slot[k]];
            wk.col[k] = s.all.p;
            wk.mask[k] = s.has_mask ? (const uint8_t*)s.all_mask.p : nullptr;
            wk.tag[k] = s.tag;
        }
        hipLaunchKernelGGL(k_win_flags, dim3(nb), dim3(256), 0, g_stream, wk,
                           ids, n, chunk, (uint8_t*)flags.p,
                           (win_fwd*)fwdc.p, (win_bwd*)bwdc.p);
        hipLaunchKernelGGL(k_win_bounds_carry, dim3(1), dim3(256), 0,
                           g_stream, (win_fwd*)fwdc.p, (win_bwd*)bwdc.p, nb);
        hipLaunchKernelGGL(k_win_bounds, dim3(nb), dim3(256), 0, g_stream,
                           (const uint8_t*)flags.p, n, chunk,
                           (const win_fwd*)fwdc.p, (const win_bwd*)bwdc.p,
                           part_start, peer_start, heads, part_end, peer_end);
        bool any_agg = false, any_val = false, any_sum = false;
        for (int i = 0; i < plan.n_funcs; i++) {
            const int f = plan.funcs[i].func;
            any_agg |= is_agg(f);
            any_val |= f >= PG_WIN_SUM && f <= PG_WIN_MAX;
            any_sum |= f == PG_WIN_SUM;
        }
        if (any_agg) {
            carry.alloc((size_t)nb * sizeof(win_acc<PG_WIN_SUM>));
            s_cnt.alloc((size_t)n * 4);
        }
        if (any_val) s_lo.alloc((size_t)n * 8);
        if (any_sum) s_hi.alloc((size_t)n * 8);
        errs.alloc(PG_MAX_WIN_FUNCS * 4);
        errs.zero();
        for (int i = 0; i < plan.n_funcs; i++) {
            const pg_win_spec& f = plan.funcs[i];
            const Slot* s = arg_slot[i] >= 0 ? &slots[arg_slot[i]] : nullptr;
            const uint8_t* smask =
                s && s->has_mask ? (const uint8_t*)s->all_mask.p : nullptr;
            if (is_agg(f.func)) {
                win_arg a{};
                if (s) {
                    a.col = s->all.p;
                    a.mask = smask;
                    a.tag = s->tag;
                }
                const uint8_t* fl = (const uint8_t*)flags.p;
                uint64_t* lo = (uint64_t*)s_lo.p;
                int64_t* hi = (int64_t*)s_hi.p;
                uint32_t* cnt = (uint32_t*)s_cnt.p;
                switch (f.func) {
                    case PG_WIN_COUNT:
                        scan_agg<PG_WIN_COUNT>(a, ids, fl, n, chunk, nb,
                                               carry.p, lo, hi, cnt);
                        break;
                    case PG_WIN_SUM:
                        scan_agg<PG_WIN_SUM>(a, ids, fl, n, chunk, nb,
                                             carry.p, lo, hi, cnt);
                        break;
                    case PG_WIN_MIN:
                        scan_agg<PG_WIN_MIN>(a, ids, fl, n, chunk, nb,
                                             carry.p, lo, hi, cnt);
                        break;
                    default:
                        scan_agg<PG_WIN_MAX>(a, ids, fl, n, chunk, nb,
                                             carry.p, lo, hi, cnt);
                        break;
                }
            }
            const pg_col& out = op.pg.cols[plan.n_emit + i];
            win_emit e{};
            e.func = f.func;
            e.frame = f.frame;
            e.width = (int)type_size(out.tag);
            e.offset = f.offset;
            e.ids = ids;
            e.part_start = part_start;
            e.peer_start = peer_start;
            e.heads = heads;
            e.part_end = part_end;
            e.peer_end = peer_end;
            e.s_lo = (const uint64_t*)s_lo.p;
            e.s_hi = (const int64_t*)s_hi.p;
            e.s_cnt = (const uint32_t*)s_cnt.p;
            if (is_shift(f.func)) {
                e.col = s->all.p;
                e.cmask = smask;
            }
            e.out = out.data;
            e.omask = (uint8_t*)out.null_mask;
            e.err = (int32_t*)errs.p + i;
            hipLaunchKernelGGL(k_win_emit, dim3(grid), dim3(256), 0, g_stream,
                               e, n);
        }
        int32_t herr[PG_MAX_WIN_FUNCS];
        CHKV(hipMemcpyAsync(herr, errs.p, sizeof(herr), hipMemcpyDeviceToHost,
                            g_stream));
        CHKV(hipStreamSynchronize(g_stream));
        for (int i = 0; i < plan.n_funcs && failed.empty(); i++)
            if (herr[i])
                failed = fname("funcs", i) +
                         ": a SUM does not fit int64 (col " +
                         std::to_string(plan.funcs[i].col) + ")";
    }
    void finish() override
    {
        if (!failed.empty()) throw std::runtime_error(failed);
        const int64_t n = n_total;
        for (auto& s : slots) concat(s);
        DevBuf idA, idB;
        const uint32_t* ids = sort_ids(n, idA, idB);
        OutPage op;
        op.pg.n_rows = n;
        op.pg.n_cols = plan.n_emit + plan.n_funcs;
        gather_emit(op, ids, n);
        for (int i = 0; i < plan.n_funcs; i++) {
            const int f = plan.funcs[i].func;
            /* ranks, COUNT and SUM are I64; MIN, MAX, LAG and LEAD have
             * their column's type.  SUM, MIN, MAX, LAG and LEAD can be
             * null and always carry a mask. */
            const bool typed_by_col = f >= PG_WIN_MIN;
            const bool masked = f >= PG_WIN_SUM;
            pg_col& c = op.pg.cols[plan.n_emit + i];
            c.tag = typed_by_col ? slots[arg_slot[i]].tag : PG_T_I64;
            c.on_device = 1;
            op.dev.emplace_back();
            op.dev.back().alloc((size_t)n * type_size(c.tag));
            c.data = op.dev.back().p;
            c.null_mask = nullptr;
            if (masked) {
                op.dev.emplace_back();
                op.dev.back().alloc((size_t)n);
                c.null_mask = (const uint8_t*)op.dev.back().p;
            }
        }
        if (n > 0) run_functions(n, ids, op);
        CHKV(hipStreamSynchronize(g_stream));
        free_slots();
        if (!failed.empty()) throw std::runtime_error(failed);
        outq.push_back(std::move(op));
    }
};

/* ---------------- MARK_DISTINCT ---------------- */
struct MarkDistinctOp : Op {
    pg_plan_mark_distinct plan;
    DevBuf state, kv, first, counters;
    int64_t cap = 0, mask = 0;
    int64_t rows_seen = 0; /* global ordinal of the next page's row 0 */
    int64_t emitted = 0;   /* only mode: rows emitted so far */
    int key_tag[4], emit_tag[16]; /* the first page's */
    bool typed = false;
    std::string failed; /* a full table fails every later call the same */

    static std::string fname(const char* field, int i)
    {
        return std::string("MARK_DISTINCT: ") + field + "[" +
               std::to_string(i) + "]";
    }
    void init()
    {
        if (plan.n_keys < 1 || plan.n_keys > 4)
            throw std::runtime_error("MARK_DISTINCT: n_keys must be 1..4");
        if (plan.n_emit < 1 || plan.n_emit > 16)
            throw std::runtime_error("MARK_DISTINCT: n_emit must be 1..16");
        if (plan.mode != PG_DISTINCT_MARK && plan.mode != PG_DISTINCT_ONLY)
            throw std::runtime_error(
                "MARK_DISTINCT: mode must be PG_DISTINCT_MARK or "
                "PG_DISTINCT_ONLY");
        if (plan.limit < 0)
            throw std::runtime_error("MARK_DISTINCT: limit must be >= 0");
        if (plan.limit != 0 && plan.mode == PG_DISTINCT_MARK)
            throw std::runtime_error(
                "MARK_DISTINCT: limit must be 0 in PG_DISTINCT_MARK mode");
        if (plan.capacity_hint < 1)
            throw std::runtime_error(
                "MARK_DISTINCT: capacity_hint must be >= 1");
        if (plan.capacity_hint > (1ll << 30) - 8)
            throw std::runtime_error(
                "MARK_DISTINCT: capacity_hint needs more than 2^31 slots");
        for (int i = 0; i < plan.n_keys; i++)
            if (plan.key_col[i] < 0)
                throw std::runtime_error(fname("key_col", i) +
                                         " is negative");
        for (int i = 0; i < plan.n_emit; i++)
            if (plan.emit_cols[i] < 0)
                throw std::runtime_error(fname("emit_cols", i) +
                                         " is negative");
        cap = next_pow2(plan.capacity_hint * 2 + 16); /* as GROUPBY_MULTI */
        mask = cap - 1;
        state.alloc((size_t)cap * 4);
        state.zero();
        kv.alloc((size_t)cap * 8 * (plan.n_keys + 1));
        first.alloc((size_t)cap * 8);
        CHKV(hipMemsetAsync(first.p, 0xff, (size_t)cap * 8, g_stream));
        counters.alloc(16); /* [claims, table full] */
        counters.zero();
    }
    /* every check before the first copy: a rejected page leaves the
     * operator as it was */
    void check(const pg_page* in)
    {
        if (in->n_rows < 0)
            throw std::runtime_error("MARK_DISTINCT: n_rows < 0");
        if (in->n_rows > INT32_MAX)
            throw std::runtime_error("MARK_DISTINCT: more than 2^31-1 rows "
                                     "in one page (row ids are 32-bit)");
        auto col_of = [&](const std::string& name, int c) -> const pg_col& {
            if (c >= in->n_cols)
                throw std::runtime_error(
                    name + " = " + std::to_string(c) +
                    " is not a column of the page (n_cols " +
                    std::to_string(in->n_cols) + ")");
            return in->cols[c];
        };
        auto same = [&](const std::string& name, int tag, int first_tag) {
            if (typed && tag != first_tag)
                throw std::runtime_error(
                    name + ": type " + std::to_string(tag) +
                    " differs from the first page's " +
                    std::to_string(first_tag));
        };
        for (int i = 0; i < plan.n_keys; i++) {
            const std::string name = fname("key_col", i);
            const pg_col& c = col_of(name, plan.key_col[i]);
            if (c.tag == PG_T_F64 || c.tag == PG_T_I128)
                throw std::runtime_error(name + ": F64 and I128 keys are "
                                                "unsupported");
            if (c.tag == PG_T_VARBIN && !c.dict_ids)
                throw std::runtime_error(
                    name + ": VARBIN keys must be dictionary blocks (the "
                           "key is the dictionary id)");
            if (c.tag != PG_T_U8 && c.tag != PG_T_I32 &&
                c.tag != PG_T_I64 && c.tag != PG_T_VARBIN)
                throw std::runtime_error(name + ": unknown column type " +
                                         std::to_string(c.tag));
            same(name, c.tag, key_tag[i]);
        }
        for (int i = 0; i < plan.n_emit; i++) {
            const std::string name = fname("emit_cols", i);
            const pg_col& c = col_of(name, plan.emit_cols[i]);
            if (c.tag == PG_T_VARBIN || c.dict_ids)
                throw std::runtime_error(name + ": VARBIN and dictionary "
                                                "columns are unsupported");
            if (c.tag != PG_T_U8 && c.tag != PG_T_I32 &&
                c.tag != PG_T_I64 && c.tag != PG_T_F64 &&
                c.tag != PG_T_I128)
                throw std::runtime_error(name + ": unknown column type " +
                                         std::to_string(c.tag));
            same(name, c.tag, emit_tag[i]);
        }
        for (int i = 0; i < plan.n_keys; i++)
            key_tag[i] = in->cols[plan.key_col[i]].tag;
        for (int i = 0; i < plan.n_emit; i++)
            emit_tag[i] = in->cols[plan.emit_cols[i]].tag;
        typed = true;
    }
    /* after the page's kernels have run: did the table fill? */
    void check_fill(const unsigned long long* c)
    {
        if (c[1] || (int64_t)c[0] * 100 > cap * 85) {
            failed = c[1] ? "MARK_DISTINCT: table full: raise capacity_hint"
                          : "MARK_DISTINCT: fill exceeded 0.85: raise "
                            "capacity_hint";
            throw std::runtime_error(failed);
        }
    }
    void add_input(const pg_page* in) override
    {
        if (!failed.empty()) throw std::runtime_error(failed);
        check(in);
        const int64_t n = in->n_rows;
        const bool only = plan.mode == PG_DISTINCT_ONLY;
        /* the kernels' page: the key columns, in only mode the emit
         * columns too (the gather reads them on the device); every other
         * column stays where it is */
        pg_page need = *in;
        for (int c = 0; c < need.n_cols; c++) {
            bool used = false;
            for (int i = 0; i < plan.n_keys; i++)
                used = used || plan.key_col[i] == c;
            for (int i = 0; only && i < plan.n_emit; i++)
                used = used || plan.emit_cols[i] == c;
            if (!used) need.cols[c] = pg_col{};
        }
        StagedPage sp;
        sp.stage(&need);
        const int64_t base = rows_seen;
        DevBuf slot_of;
        slot_of.alloc((size_t)n * 4);
        const int grid = (int)std::min<int64_t>((n + 255) / 256, FT_NBLOCKS);
        if (n > 0) {
            hot_begin();
            hipLaunchKernelGGL(k_mark_distinct_insert, dim3(grid), dim3(256),
                               0, g_stream, sp.pg, plan,
                               (unsigned int*)state.p, (int64_t*)kv.p, cap,
                               mask, (unsigned long long*)first.p, base,
                               (uint32_t*)slot_of.p,
                               (unsigned long long*)counters.p);
            hot_end();
        }
        unsigned long long c[2] = {0, 0};
        OutPage op;
        op.pg.n_cols = plan.n_emit + (only ? 0 : 1);
        auto add_col = [&](int cx, int tag, int64_t rows, bool with_mask) {
            op.dev.emplace_back();
            op.dev.back().alloc((size_t)rows * type_size(tag));
            op.pg.cols[cx].tag = tag;
            op.pg.cols[cx].on_device = 1;
            op.pg.cols[cx].data = op.dev.back().p;
            op.pg.cols[cx].null_mask = nullptr;
            if (with_mask) {
                op.dev.emplace_back();
                op.dev.back().alloc((size_t)rows);
                op.pg.cols[cx].null_mask = (const uint8_t*)op.dev.back().p;
            }
        };
        if (!only) {
            /* the emit columns as they are, from wherever they are */
            for (int o = 0; o < plan.n_emit; o++) {
                const pg_col& src = in->cols[plan.emit_cols[o]];
                const hipMemcpyKind kind = src.on_device
                                               ? hipMemcpyDeviceToDevice
                                               : hipMemcpyHostToDevice;
                add_col(o, src.tag, n, src.null_mask != nullptr);
                if (n > 0) {
                    CHKV(hipMemcpyAsync(op.pg.cols[o].data, src.data,
                                        (size_t)n * type_size(src.tag), kind,
                                        g_stream));
                    if (src.null_mask)
                        CHKV(hipMemcpyAsync((void*)op.pg.cols[o].null_mask,
                                            src.null_mask, (size_t)n, kind,
                                            g_stream));
                }
            }
            add_col(plan.n_emit, PG_T_U8, n, false);
            if (n > 0)
                hipLaunchKernelGGL(k_mark_distinct_mark, dim3(grid),
                                   dim3(256), 0, g_stream,
                                   (const uint32_t*)slot_of.p,
                                   (const unsigned long long*)first.p, base,
                                   n, (uint8_t*)op.pg.cols[plan.n_emit].data);
            CHKV(hipMemcpyAsync(c, counters.p, 16, hipMemcpyDeviceToHost,
                                g_stream));
            CHKV(hipStreamSynchronize(g_stream));
            check_fill(c);
            op.pg.n_rows = n;
        } else {
            const int64_t chunk = sel_chunk(n);
            DevBuf d_counts, selbits, d_offs, rowid;
            std::vector<int64_t> h(FLT_NB, 0);
            if (n > 0) {
                d_counts.alloc(FLT_NB * sizeof(int64_t));
                selbits.alloc(((size_t)(n + 255) / 256 * 4 + 1) * 8);
                hipLaunchKernelGGL(k_mark_distinct_count, dim3(FLT_NB),
                                   dim3(256), 0, g_stream,
                                   (const uint32_t*)slot_of.p,
                                   (const unsigned long long*)first.p, base,
                                   n, chunk, (int64_t*)d_counts.p,
                                   (unsigned long long*)selbits.p);
                CHKV(hipMemcpyAsync(h.data(), d_counts.p, FLT_NB * 8,
                                    hipMemcpyDeviceToHost, g_stream));
            }
            CHKV(hipMemcpyAsync(c, counters.p, 16, hipMemcpyDeviceToHost,
                                g_stream));
            CHKV(hipStreamSynchronize(g_stream));
            check_fill(c);
            int64_t total = 0;
            for (int b = 0; b < FLT_NB; b++) {
                const int64_t cnt = h[b];
                h[b] = total; /* the block's offset */
                total += cnt;
            }
            int64_t n_out = total;
            if (plan.limit > 0 && emitted + total >= plan.limit) {
                /* DistinctLimit: cut to fit, and no more input */
                n_out = plan.limit - emitted;
                finished = true;
            }
            emitted += n_out;
            sort_gather_cols g{};
            g.n = plan.n_emit;
            for (int o = 0; o < plan.n_emit; o++) {
                const pg_col& src = sp.pg.cols[plan.emit_cols[o]];
                add_col(o, src.tag, n_out, src.null_mask != nullptr);
                g.src[o] = src.data;
                g.dst[o] = op.pg.cols[o].data;
                g.width[o] = (int)type_size(src.tag);
                g.msrc[o] = src.null_mask;
                g.mdst[o] = (uint8_t*)op.pg.cols[o].null_mask;
            }
            if (n_out > 0) {
                rowid.alloc((size_t)n_out * 4);
                d_offs.alloc(FLT_NB * sizeof(int64_t));
                CHKV(hipMemcpyAsync(d_offs.p, h.data(), FLT_NB * 8,
                                    hipMemcpyHostToDevice, g_stream));
                hipLaunchKernelGGL(k_mark_distinct_rowids, dim3(FLT_NB),
                                   dim3(256), 0, g_stream,
                                   (const unsigned long long*)selbits.p, n,
                                   chunk, (const int64_t*)d_offs.p, n_out,
                                   (uint32_t*)rowid.p);
                const int ggrid =
                    (int)std::min<int64_t>((n_out + 255) / 256, 2048);
                hipLaunchKernelGGL(k_sort_gather, dim3(ggrid), dim3(256), 0,
                                   g_stream, (const uint32_t*)rowid.p, n_out,
                                   g);
                CHKV(hipStreamSynchronize(g_stream));
            }
            op.pg.n_rows = n_out;
        }
        rows_seen += n;
        outq.push_back(std::move(op));
    }
    void finish() override
    {
        if (!failed.empty()) throw std::runtime_error(failed);
    }
};

/* shared_ptr so a concurrent pg_op_destroy cannot free an Op another
 * thread's call still holds (each C-ABI entry copies the ref; the
 * per-handle single-threaded contract of presto_gpu.h still applies to
 * calls on the SAME handle) */
static std::map<int64_t, std::shared_ptr<Op>> g_ops;
static int64_t g_next_op = 1;

} /* namespace */

/* ---------------- C-ABI glue ---------------- */
extern "C" pg_status pg_op_create(int32_t kind, const void* plan,
                                  int64_t plan_bytes, pg_op* out)
{
    if (ensure_gpu()) return PG_ERR;
    try {
        std::unique_ptr<Op> op;
        switch (kind) {
            case PG_OP_FILTER_PROJECT: {
                if (plan_bytes != sizeof(pg_plan_filter_project))
                    return seterr("bad plan size");
                auto* o = new FilterOp();
                op.reset(o);
                memcpy(&o->plan, plan, sizeof(o->plan));
                o->init();
                break;
            }
            case PG_OP_HASH_AGG_SMALL: {
                if (plan_bytes != sizeof(pg_plan_hash_agg_small))
                    return seterr("bad plan size");
                auto* o = new AggSmallOp();
                memcpy(&o->plan, plan, sizeof(o->plan));
                o->init();
                op.reset(o);
                break;
            }
            case PG_OP_HASH_BUILD: {
                if (plan_bytes != sizeof(pg_plan_hash_build))
                    return seterr("bad plan size");
                auto* o = new BuildOp();
                memcpy(&o->plan, plan, sizeof(o->plan));
                o->init();
                op.reset(o);
                break;
            }
            case PG_OP_LOOKUP_JOIN: {
                if (plan_bytes != sizeof(pg_plan_lookup_join))
                    return seterr("bad plan size");
                auto* o = new JoinOp();
                memcpy(&o->plan, plan, sizeof(o->plan));
                o->init();
                op.reset(o);
                break;
            }
            case PG_OP_TOPN: {
                if (plan_bytes != sizeof(pg_plan_topn))
                    return seterr("bad plan size");
                auto* o = new TopNOp();
                memcpy(&o->plan, plan, sizeof(o->plan));
                op.reset(o);
                break;
            }
            case PG_OP_PARTITION: {
                if (plan_bytes != sizeof(pg_plan_partition))
                    return seterr("bad plan size");
                auto* o = new PartitionOp();
                memcpy(&o->plan, plan, sizeof(o->plan));
                op.reset(o);
                break;
            }
            case PG_OP_GROUPBY_MULTI: {
                if (plan_bytes != sizeof(pg_plan_groupby))
                    return seterr("bad plan size");
                auto* o = new GroupByOp();
                memcpy(&o->plan, plan, sizeof(o->plan));
                o->init();
                op.reset(o);
                break;
            }
            case PG_OP_ORDER_BY: {
                if (plan_bytes != sizeof(pg_plan_order_by))
                    return seterr("bad plan size");
                auto* o = new OrderByOp();
                op.reset(o);
                memcpy(&o->plan, plan, sizeof(o->plan));
                o->init();
                break;
            }
            case PG_OP_WINDOW: {
                if (plan_bytes != sizeof(pg_plan_window))
                    return seterr("bad plan size");
                auto* o = new WindowOp();
                op.reset(o);
                memcpy(&o->plan, plan, sizeof(o->plan));
                o->init();
                break;
            }
            case PG_OP_MARK_DISTINCT: {
                if (plan_bytes != sizeof(pg_plan_mark_distinct))
                    return seterr("bad plan size");
                auto* o = new MarkDistinctOp();
                op.reset(o);
                memcpy(&o->plan, plan, sizeof(o->plan));
                o->init();
                break;
            }
            default: return seterr("unknown operator kind");
        }
        op->kind = kind;
        std::lock_guard<std::mutex> lk(g_mu);
        int64_t h = g_next_op++;
        g_ops[h] = std::move(op);
        *out = h;
        return PG_OK;
    } catch (std::exception& e) {
        return seterr(e.what());
    }
}

static std::shared_ptr<Op> find_op(pg_op h)
{
    std::lock_guard<std::mutex> lk(g_mu);
    auto it = g_ops.find(h);
    return it == g_ops.end() ? nullptr : it->second;
}

extern "C" int32_t pg_op_needs_input(pg_op h)
{
    auto op = find_op(h);
    return op && !op->finished ? 1 : 0;
}
extern "C" pg_status pg_op_add_input(pg_op h, const pg_page* page)
{
    auto op = find_op(h);
    if (!op) return seterr("bad op handle");
    if (op->finished) return seterr("addInput after finish");
    try {
        op->add_input(page);
        return PG_OK;
    } catch (std::exception& e) {
        return seterr(e.what());
    }
}
extern "C" pg_status pg_op_get_output(pg_op h, const pg_page** out)
{
    auto op = find_op(h);
    if (!op) return seterr("bad op handle");
    try {
        *out = op->pop_output();
        return PG_OK;
    } catch (std::exception& e) {
        return seterr(e.what());
    }
}
extern "C" pg_status pg_op_finish(pg_op h)
{
    auto op = find_op(h);
    if (!op) return seterr("bad op handle");
    if (op->finished) return PG_OK; /* idempotent */
    try {
        op->finish();
        op->finished = true;
        return PG_OK;
    } catch (std::exception& e) {
        return seterr(e.what());
    }
}
extern "C" int32_t pg_op_is_finished(pg_op h)
{
    auto op = find_op(h);
    return op && op->finished && op->outq.empty() ? 1 : 0;
}
extern "C" pg_status pg_op_destroy(pg_op h)
{
    std::lock_guard<std::mutex> lk(g_mu);
    g_ops.erase(h);
    return PG_OK;
}
extern "C" pg_status pg_op_table(pg_op h, int64_t* out)
{
    auto op = find_op(h);
    if (!op) return seterr("bad op handle");
    int64_t t = op->table_handle();
    if (t < 0) return seterr("op has no table (finish the build first)");
    *out = t;
    return PG_OK;
}
extern "C" pg_status pg_op_partition_counts(pg_op h, int64_t* counts,
                                            int32_t n)
{
    auto op = find_op(h);
    if (!op) return seterr("bad op handle");
    try {
        op->partition_counts(counts, n);
        return PG_OK;
    } catch (std::exception& e) {
        return seterr(e.what());
    }
}
extern "C" pg_status pg_table_destroy(int64_t t)
{
    std::lock_guard<std::mutex> lk(g_mu);
    g_tables.erase(t);
    return PG_OK;
}

/* bytes of the table's tag array; 0: no tags (or no such table) */
extern "C" int64_t pg_table_tag_bytes(int64_t t)
{
    std::lock_guard<std::mutex> lk(g_mu);
    auto it = g_tables.find(t);
    if (it == g_tables.end()) return 0;
    return it->second->tags.p ? (int64_t)it->second->tags.sz : 0;
}

extern "C" pg_status pg_table_reset_acc(int64_t t)
{
    try {
        Table* tbl;
        {
            std::lock_guard<std::mutex> lk(g_mu);
            auto it = g_tables.find(t);
            if (it == g_tables.end())
                return seterr("pg_table_reset_acc: table not found");
            tbl = it->second.get();
        }
        if (tbl->acc.p) {
            CHK(hipMemsetAsync(tbl->acc.p, 0, tbl->acc.sz, g_stream));
            hits_restart(tbl);
        }
        if (tbl->acc_multi.p)
            CHK(hipMemsetAsync(tbl->acc_multi.p, 0, tbl->acc_multi.sz,
                               g_stream));
        CHK(hipStreamSynchronize(g_stream));
        return PG_OK;
    } catch (const std::exception& e) {
        return seterr(e.what());
    }
}

/* ================================================================== */
/* SerializedPage wire interop — citations in presto_gpu.h            */
/* ================================================================== */
namespace {

/* standard CRC-32 (zlib polynomial), as java.util.zip.CRC32 */
static uint32_t crc32_tab_[256];
static bool crc32_init_ = false;
static uint32_t pg_crc32(uint32_t crc, const uint8_t* p, size_t n)
{
    if (!crc32_init_) {
        for (uint32_t i = 0; i < 256; i++) {
            uint32_t c = i;
            for (int k = 0; k < 8; k++)
                c = (c & 1) ? 0xEDB88320u ^ (c >> 1) : c >> 1;
            crc32_tab_[i] = c;
        }
        crc32_init_ = true;
    }
    crc = ~crc;
    for (size_t i = 0; i < n; i++)
        crc = crc32_tab_[(crc ^ p[i]) & 0xff] ^ (crc >> 8);
    return ~crc;
}

struct ByteWriter {
    uint8_t* p;
    int64_t cap, off = 0;
    bool ok = true;
    void bytes(const void* src, int64_t n)
    {
        if (off + n > cap) { ok = false; return; }
        memcpy(p + off, src, n);
        off += n;
    }
    void u8(uint8_t v) { bytes(&v, 1); }
    void i32(int32_t v) { bytes(&v, 4); } /* little-endian host */
    void i64(int64_t v) { bytes(&v, 8); }
};
struct ByteReader {
    const uint8_t* p;
    int64_t len, off = 0;
    bool ok = true;
    const void* bytes(int64_t n)
    {
        if (off + n > len) { ok = false; return nullptr; }
        const void* r = p + off;
        off += n;
        return r;
    }
    uint8_t u8() { auto* r = (const uint8_t*)bytes(1); return r ? *r : 0; }
    int32_t i32()
    {
        int32_t v = 0;
        auto* r = bytes(4);
        if (r) memcpy(&v, r, 4);
        return v;
    }
    int64_t i64()
    {
        int64_t v = 0;
        auto* r = bytes(8);
        if (r) memcpy(&v, r, 8);
        return v;
    }
};

static const char* enc_name(int tag)
{
    switch (tag) {
        case PG_T_U8: return "BYTE_ARRAY";
        case PG_T_I32: return "INT_ARRAY";
        case PG_T_VARBIN: return "VARIABLE_WIDTH";
        default: return "LONG_ARRAY"; /* I64 and F64 (bits) */
    }
}

/* ---- LZ4 block format codec (host side) ----
 * The reference compresses SerializedPage bodies with airlift
 * aircompressor's Lz4Compressor (PagesSerde.java:67-95); this is an
 * independent implementation of the same LZ4 block format (the wire
 * LAYOUT — marker bit, sizes, checksum — is byte-pinned against
 * PagesSerdeUtil; the compressed byte stream itself is codec output and
 * interoperable with any LZ4 block decoder, not byte-identical to
 * aircompressor's encoder choices). */
static int64_t lz4_compress(const uint8_t* src, int64_t n, uint8_t* dst,
                            int64_t cap)
{
    if (n == 0) return 0;
    const int64_t HASH_SIZE = 1 << 14;
    static thread_local std::vector<int32_t> table;
    table.assign(HASH_SIZE, -1);
    int64_t ip = 0, op = 0, anchor = 0;
    const int64_t mflimit = n - 12; /* last match must end 12 before n */
    auto hash4 = [&](int64_t p) {
        uint32_t v;
        memcpy(&v, src + p, 4);
        return (int64_t)((v * 2654435761u) >> 18);
    };
    auto emit = [&](int64_t lit_len, int64_t lit_at, int64_t mlen,
                    int64_t dist) -> bool {
        int64_t need = 1 + lit_len + lit_len / 255 + 1 + 2 + mlen / 255 + 1;
        if (op + need > cap) return false;
        uint8_t* tok = dst + op++;
        int64_t l = lit_len;
        *tok = (uint8_t)((l >= 15 ? 15 : l) << 4);
        if (l >= 15) {
            l -= 15;
            while (l >= 255) { dst[op++] = 255; l -= 255; }
            dst[op++] = (uint8_t)l;
        }
        memcpy(dst + op, src + lit_at, lit_len);
        op += lit_len;
        if (mlen > 0) {
            dst[op++] = (uint8_t)dist;
            dst[op++] = (uint8_t)(dist >> 8);
            int64_t m = mlen - 4;
            *tok |= (uint8_t)(m >= 15 ? 15 : m);
            if (m >= 15) {
                m -= 15;
                while (m >= 255) { dst[op++] = 255; m -= 255; }
                dst[op++] = (uint8_t)m;
            }
        }
        return true;
    };
    while (ip < mflimit) {
        int64_t h = hash4(ip);
        int64_t ref = table[h];
        table[h] = (int32_t)ip;
        uint32_t a, b;
        if (ref >= 0 && ip - ref < 65536) {
            memcpy(&a, src + ref, 4);
            memcpy(&b, src + ip, 4);
            if (a == b) {
                int64_t mlen = 4;
                while (ip + mlen < n - 5 &&
                       src[ref + mlen] == src[ip + mlen])
                    mlen++;
                if (!emit(ip - anchor, anchor, mlen, ip - ref)) return -1;
                ip += mlen;
                anchor = ip;
                continue;
            }
        }
        ip++;
    }
    /* final literals */
    if (!emit(n - anchor, anchor, 0, 0)) return -1;
    return op;
}

static bool lz4_decompress(const uint8_t* src, int64_t n, uint8_t* dst,
                           int64_t dn)
{
    int64_t ip = 0, op = 0;
    while (ip < n) {
        uint8_t tok = src[ip++];
        int64_t lit = tok >> 4;
        if (lit == 15) {
            uint8_t b;
            do {
                if (ip >= n) return false;
                b = src[ip++];
                lit += b;
            } while (b == 255);
        }
        if (ip + lit > n || op + lit > dn) return false;
        memcpy(dst + op, src + ip, lit);
        ip += lit;
        op += lit;
        if (ip >= n) break; /* last sequence has no match */
        if (ip + 2 > n) return false;
        int64_t dist = src[ip] | ((int64_t)src[ip + 1] << 8);
        ip += 2;
        if (dist == 0 || dist > op) return false;
        int64_t mlen = (tok & 15) + 4;
        if ((tok & 15) == 15) {
            uint8_t b;
            do {
                if (ip >= n) return false;
                b = src[ip++];
                mlen += b;
            } while (b == 255);
        }
        if (op + mlen > dn) return false;
        for (int64_t j = 0; j < mlen; j++, op++) dst[op] = dst[op - dist];
    }
    return op == dn;
}

/* encodeNullsAsBits — EncoderUtil.java:31-63 (MSB-first per byte) */
static void write_null_bits(ByteWriter& w, const uint8_t* mask, int64_t n)
{
    if (!mask) {
        w.u8(0);
        return;
    }
    bool any = false;
    for (int64_t i = 0; i < n; i++) any = any || mask[i];
    w.u8(any ? 1 : 0);
    if (!any) return;
    for (int64_t base = 0; base < n; base += 8) {
        uint8_t v = 0;
        for (int64_t j = base; j < base + 8 && j < n; j++)
            if (mask[j]) v |= (uint8_t)(0x80u >> (j - base));
        w.u8(v);
    }
}

} /* namespace */

namespace {

/* write one block (writeRawPage writes blockCount then per-block a
 * length-prefixed encoding name + body — BlockEncodingManager.java:96-99) */
static void write_block(ByteWriter& w, const pg_col& col, int64_t n)
{
    if (col.tag == PG_T_VARBIN && col.dict_ids) {
        /* DICTIONARY (DictionaryBlockEncoding.java:32-55): positionCount,
         * nested dictionary block, raw int ids, then the 3-long
         * DictionaryId (most/least significant bits + sequence id) */
        static const char* dn = "DICTIONARY";
        w.i32((int32_t)strlen(dn));
        w.bytes(dn, strlen(dn));
        w.i32((int32_t)n);
        pg_col dict = col;
        dict.dict_ids = nullptr;
        write_block(w, dict, col.dict_n);
        w.bytes(col.dict_ids, n * 4);
        w.i64(0x50472d414d442d31ll); /* fixed instance id: readers treat
                                        it as an opaque dedup token */
        w.i64(0x4449435400000000ll);
        w.i64(1);
        return;
    }
    if (col.tag == PG_T_I128) {
        /* INT128_ARRAY (Int128ArrayBlockEncoding.java:36-50): two longs
         * per non-null position after the null bits */
        static const char* in = "INT128_ARRAY";
        w.i32((int32_t)strlen(in));
        w.bytes(in, strlen(in));
        w.i32((int32_t)n);
        write_null_bits(w, col.null_mask, n);
        const uint8_t* d = (const uint8_t*)col.data;
        if (!col.null_mask) {
            w.bytes(d, n * 16);
        } else {
            for (int64_t i = 0; i < n; i++)
                if (!col.null_mask[i]) w.bytes(d + i * 16, 16);
        }
        return;
    }
    const char* name = enc_name(col.tag);
    int32_t nl = (int32_t)strlen(name);
    w.i32(nl);
    w.bytes(name, nl);
    w.i32((int32_t)n);
    if (col.tag == PG_T_VARBIN) {
        /* VariableWidthBlockEncoding.writeBlock:37-58 */
        for (int64_t i = 0; i < n; i++) w.i32(col.offsets[i + 1]);
        write_null_bits(w, col.null_mask, n);
        int32_t total = col.offsets[n];
        w.i32(total);
        w.bytes(col.data, total);
        return;
    }
    write_null_bits(w, col.null_mask, n);
    size_t esz = type_size(col.tag);
    if (!col.null_mask) {
        w.bytes(col.data, n * esz);
    } else {
        for (int64_t i = 0; i < n; i++)
            if (!col.null_mask[i])
                w.bytes((const uint8_t*)col.data + i * esz, esz);
    }
}

static bool read_null_bits(ByteReader& r, int64_t n, uint8_t** out_mask)
{
    uint8_t may = r.u8();
    *out_mask = nullptr;
    if (!may) return r.ok;
    uint8_t* mask = (uint8_t*)calloc(n ? n : 1, 1);
    for (int64_t base = 0; base < n; base += 8) {
        uint8_t v = r.u8();
        for (int64_t j = base; j < base + 8 && j < n; j++)
            mask[j] = (v >> (7 - (j - base))) & 1;
    }
    *out_mask = mask;
    return r.ok;
}

static pg_status read_block(ByteReader& r, pg_col* out, int64_t* out_n);

/* expand an RLE value block to n positions (materialized on read, the
 * way LazyBlock consumers see a flat block) */
static pg_status expand_rle(const pg_col& v, int64_t vn, int64_t n,
                            pg_col* out)
{
    (void)vn;
    memset(out, 0, sizeof(*out));
    out->tag = v.tag;
    bool isnull = v.null_mask && v.null_mask[0];
    if (v.tag == PG_T_VARBIN) {
        int32_t len = isnull ? 0 : v.offsets[1];
        int32_t* offs = (int32_t*)calloc((size_t)n + 1, 4);
        uint8_t* data = (uint8_t*)calloc((size_t)len * (n ? n : 1) + 1, 1);
        for (int64_t i = 0; i < n; i++) {
            offs[i + 1] = offs[i] + len;
            if (len) memcpy(data + offs[i], v.data, len);
        }
        out->offsets = offs;
        out->data = data;
    } else {
        size_t esz = type_size(v.tag);
        uint8_t* data = (uint8_t*)calloc(n ? n : 1, esz);
        if (!isnull)
            for (int64_t i = 0; i < n; i++)
                memcpy(data + i * esz, v.data, esz);
        out->data = data;
    }
    if (isnull) {
        uint8_t* mask = (uint8_t*)malloc(n ? n : 1);
        memset(mask, 1, n ? n : 1);
        out->null_mask = mask;
    }
    free((void*)v.data);
    free((void*)v.null_mask);
    free((void*)v.offsets);
    return PG_OK;
}

static pg_status read_block(ByteReader& r, pg_col* out, int64_t* out_n)
{
    memset(out, 0, sizeof(*out));
    int32_t nl = r.i32();
    if (!r.ok || nl < 0 || nl > 64)
        return seterr("deserialize: bad encoding name");
    char name[65] = {0};
    const void* np_ = r.bytes(nl);
    if (np_) memcpy(name, np_, nl);
    if (!strcmp(name, "RLE")) {
        /* RunLengthBlockEncoding.java:31-51: run length then the
         * single-position value block */
        int32_t n = r.i32();
        pg_col v;
        int64_t vn = 0;
        pg_status st = read_block(r, &v, &vn);
        if (st != PG_OK) return st;
        if (vn != 1) return seterr("deserialize: RLE value not 1 row");
        *out_n = n;
        return expand_rle(v, vn, n, out);
    }
    if (!strcmp(name, "DICTIONARY")) {
        int32_t n = r.i32();
        pg_col dict;
        int64_t dn = 0;
        pg_status st = read_block(r, &dict, &dn);
        if (st != PG_OK) return st;
        int32_t* ids = (int32_t*)calloc(n ? n : 1, 4);
        const void* idsrc = r.bytes((int64_t)n * 4);
        if (idsrc) memcpy(ids, idsrc, (size_t)n * 4);
        r.i64();
        r.i64();
        r.i64(); /* DictionaryId: opaque */
        if (!r.ok) {
            free(ids);
            return seterr("deserialize: truncated DICTIONARY block");
        }
        *out_n = n;
        if (dict.tag == PG_T_VARBIN) {
            /* preserved in dictionary form (DictionaryBlock semantics) */
            *out = dict;
            out->dict_ids = ids;
            out->dict_n = (int32_t)dn;
            return PG_OK;
        }
        /* fixed-width dictionaries are expanded on read */
        size_t esz = type_size(dict.tag);
        uint8_t* data = (uint8_t*)calloc(n ? n : 1, esz);
        uint8_t* mask = nullptr;
        for (int64_t i = 0; i < n; i++) {
            int32_t id = ids[i];
            if (id < 0 || id >= dn) {
                free(ids);
                free(data);
                free(mask);
                free((void*)dict.data);
                free((void*)dict.null_mask);
                return seterr("deserialize: dictionary id out of range");
            }
            memcpy(data + i * esz, (const uint8_t*)dict.data + id * esz,
                   esz);
            if (dict.null_mask && dict.null_mask[id]) {
                if (!mask) mask = (uint8_t*)calloc(n, 1);
                mask[i] = 1;
            }
        }
        free(ids);
        free((void*)dict.data);
        free((void*)dict.null_mask);
        free((void*)dict.offsets);
        out->tag = dict.tag;
        out->data = data;
        out->null_mask = mask;
        return PG_OK;
    }
    int tag;
    if (!strcmp(name, "LONG_ARRAY")) tag = PG_T_I64;
    else if (!strcmp(name, "INT_ARRAY")) tag = PG_T_I32;
    else if (!strcmp(name, "BYTE_ARRAY")) tag = PG_T_U8;
    else if (!strcmp(name, "INT128_ARRAY")) tag = PG_T_I128;
    else if (!strcmp(name, "VARIABLE_WIDTH")) tag = PG_T_VARBIN;
    else return seterr("deserialize: unsupported block encoding");
    int32_t n = r.i32();
    *out_n = n;
    if (tag == PG_T_VARBIN) {
        /* VariableWidthBlockEncoding.readBlock:62-76 */
        int32_t* offs = (int32_t*)calloc((size_t)n + 1, 4);
        for (int64_t i = 0; i < n; i++) offs[i + 1] = r.i32();
        uint8_t* vmask = nullptr;
        read_null_bits(r, n, &vmask);
        int32_t nb = r.i32();
        uint8_t* vb = (uint8_t*)calloc(nb ? nb : 1, 1);
        const void* vsrc = r.bytes(nb);
        if (vsrc) memcpy(vb, vsrc, (size_t)nb);
        if (!r.ok || nb != offs[n]) {
            free(offs);
            free(vmask);
            free(vb);
            return seterr("deserialize: bad VARIABLE_WIDTH block");
        }
        out->tag = PG_T_VARBIN;
        out->data = vb;
        out->offsets = offs;
        out->null_mask = vmask;
        return PG_OK;
    }
    uint8_t* mask = nullptr;
    read_null_bits(r, n, &mask);
    size_t esz = type_size(tag);
    uint8_t* vals = (uint8_t*)calloc(n ? n : 1, esz);
    if (!mask) {
        const void* vsrc = r.bytes((int64_t)n * esz);
        if (vsrc) memcpy(vals, vsrc, (size_t)n * esz);
    } else {
        for (int64_t i = 0; i < n; i++)
            if (!mask[i]) {
                const void* vsrc = r.bytes(esz);
                if (vsrc) memcpy(vals + i * esz, vsrc, esz);
            }
    }
    if (!r.ok) {
        free(mask);
        free(vals);
        return seterr("deserialize: truncated block");
    }
    out->tag = tag;
    out->data = vals;
    out->null_mask = mask;
    return PG_OK;
}

} /* namespace */

extern "C" int32_t pg_abi_struct_sizes(int32_t* out, int32_t n)
{
    const int32_t sz[] = {
        (int32_t)sizeof(pg_col),
        (int32_t)sizeof(pg_page),
        (int32_t)sizeof(pg_pred),
        (int32_t)sizeof(pg_proj),
        (int32_t)sizeof(pg_agg),
        (int32_t)sizeof(pg_plan_filter_project),
        (int32_t)sizeof(pg_plan_hash_agg_small),
        (int32_t)sizeof(pg_plan_hash_build),
        (int32_t)sizeof(pg_plan_lookup_join),
        (int32_t)sizeof(pg_plan_groupby),
        (int32_t)sizeof(pg_plan_topn),
        (int32_t)sizeof(pg_plan_partition),
    };
    const int32_t count = (int32_t)(sizeof(sz) / sizeof(sz[0]));
    for (int32_t i = 0; i < n && i < count; i++) out[i] = sz[i];
    return count;
}

extern "C" int32_t pg_abi_plan_size(int32_t kind)
{
    switch (kind) {
        case PG_OP_FILTER_PROJECT:
            return (int32_t)sizeof(pg_plan_filter_project);
        case PG_OP_HASH_AGG_SMALL:
            return (int32_t)sizeof(pg_plan_hash_agg_small);
        case PG_OP_HASH_BUILD: return (int32_t)sizeof(pg_plan_hash_build);
        case PG_OP_LOOKUP_JOIN: return (int32_t)sizeof(pg_plan_lookup_join);
        case PG_OP_TOPN: return (int32_t)sizeof(pg_plan_topn);
        case PG_OP_PARTITION: return (int32_t)sizeof(pg_plan_partition);
        case PG_OP_GROUPBY_MULTI: return (int32_t)sizeof(pg_plan_groupby);
        case PG_OP_ORDER_BY: return (int32_t)sizeof(pg_plan_order_by);
        case PG_OP_WINDOW: return (int32_t)sizeof(pg_plan_window);
        case PG_OP_MARK_DISTINCT:
            return (int32_t)sizeof(pg_plan_mark_distinct);
        default: return -1;
    }
}

extern "C" uint64_t pg_sortkey_u64(int32_t tag, int32_t order, uint64_t bits)
{
    return pg_sortkey(tag, order, bits);
}

extern "C" pg_status pg_page_serialize2(const pg_page* page,
                                        int32_t compress, void* out,
                                        int64_t cap, int64_t* out_len)
{
    for (int c = 0; c < page->n_cols; c++)
        if (page->cols[c].on_device)
            return seterr("pg_page_serialize: host columns required");
    /* body built aside so the whole page can go through the compressor
     * (PagesSerde.java:67-95) */
    std::vector<uint8_t> body(64 + (size_t)page->n_rows * 64);
    ByteWriter w{body.data(), (int64_t)body.size()};
    for (;;) {
        w = ByteWriter{body.data(), (int64_t)body.size()};
        w.i32(page->n_cols);
        for (int c = 0; c < page->n_cols; c++)
            write_block(w, page->cols[c], page->n_rows);
        if (w.ok) break;
        body.resize(body.size() * 2);
    }
    int64_t usize = w.off;
    uint8_t marker = 0;
    const uint8_t* stored = body.data();
    int64_t ssize = usize;
    std::vector<uint8_t> cbuf;
    if (compress) {
        cbuf.resize((size_t)usize + usize / 16 + 256);
        int64_t cs = lz4_compress(body.data(), usize, cbuf.data(),
                                  (int64_t)cbuf.size());
        /* MINIMUM_COMPRESSION_RATIO = 0.9 (PagesSerde.java:41) */
        if (cs > 0 && (double)cs / (double)usize <= 0.9) {
            marker = 1; /* PageCodecMarker.COMPRESSED */
            stored = cbuf.data();
            ssize = cs;
        }
    }
    ByteWriter m{(uint8_t*)out, cap};
    m.i32((int32_t)page->n_rows);
    m.u8(marker);
    m.i32((int32_t)usize);
    m.i32((int32_t)ssize);
    /* computeSerializedPageChecksum:109-120 */
    uint32_t crc = pg_crc32(0, stored, ssize);
    uint8_t tail[9];
    tail[0] = marker;
    int32_t pc = (int32_t)page->n_rows;
    int32_t us32 = (int32_t)usize;
    memcpy(tail + 1, &pc, 4);
    memcpy(tail + 5, &us32, 4);
    crc = pg_crc32(crc, tail, 9);
    m.i64((int64_t)(uint32_t)crc);
    m.bytes(stored, ssize);
    if (!m.ok) return seterr("pg_page_serialize: buffer too small");
    *out_len = m.off;
    return PG_OK;
}

extern "C" pg_status pg_page_serialize(const pg_page* page, void* out,
                                       int64_t cap, int64_t* out_len)
{
    return pg_page_serialize2(page, 0, out, cap, out_len);
}

extern "C" pg_status pg_page_deserialize(const void* buf, int64_t len,
                                         pg_page* out)
{
    ByteReader r{(const uint8_t*)buf, len};
    int32_t pos_count = r.i32();
    uint8_t marker = r.u8();
    int32_t usize = r.i32();
    int32_t size = r.i32();
    int64_t checksum = r.i64();
    if (!r.ok) return seterr("deserialize: truncated metadata");
    if (marker & ~1)
        return seterr("deserialize: encrypted/checksummed markers "
                      "unsupported");
    if (r.off + size > len) return seterr("deserialize: bad sizes");
    uint32_t crc = pg_crc32(0, r.p + r.off, size);
    uint8_t tail[9];
    tail[0] = marker;
    memcpy(tail + 1, &pos_count, 4);
    memcpy(tail + 5, &usize, 4);
    crc = pg_crc32(crc, tail, 9);
    if ((int64_t)(uint32_t)crc != checksum)
        return seterr("deserialize: checksum mismatch");
    std::vector<uint8_t> ubuf;
    ByteReader body{r.p + r.off, size};
    if (marker & 1) {
        ubuf.resize(usize ? usize : 1);
        if (!lz4_decompress(r.p + r.off, size, ubuf.data(), usize))
            return seterr("deserialize: LZ4 stream corrupt");
        body = ByteReader{ubuf.data(), usize};
    } else if (size != usize) {
        return seterr("deserialize: bad sizes");
    }
    int32_t n_blocks = body.i32();
    if (n_blocks < 0 || n_blocks > 32)
        return seterr("deserialize: unsupported block count");
    memset(out, 0, sizeof(*out));
    out->n_rows = pos_count;
    out->n_cols = n_blocks;
    for (int c = 0; c < n_blocks; c++) {
        int64_t bn = 0;
        pg_status st = read_block(body, &out->cols[c], &bn);
        if (st != PG_OK) {
            pg_page_free(out);
            return st;
        }
        if (bn != pos_count) {
            pg_page_free(out);
            return seterr("deserialize: block position count mismatch");
        }
    }
    return PG_OK;
}

extern "C" pg_status pg_page_free(pg_page* page)
{
    for (int c = 0; c < page->n_cols; c++) {
        free(page->cols[c].data);
        free((void*)page->cols[c].null_mask);
        free((void*)page->cols[c].offsets);
        free((void*)page->cols[c].dict_ids);
        page->cols[c].data = nullptr;
        page->cols[c].null_mask = nullptr;
        page->cols[c].offsets = nullptr;
        page->cols[c].dict_ids = nullptr;
    }
    return PG_OK;
}
