/* presto_gpu.h — public C-ABI of the MI355X-native Presto hot-path library.
 *
 * This is the drop-in boundary of SURVEY.md §8b: a handle-based operator
 * lifecycle mirroring the reference's Operator interface
 * (presto-main-base/.../operator/Operator.java:20-102, constructed via
 * OperatorFactory.createOperator and driven by Driver.processInternal:402),
 * with Page data crossing the seam as flat column descriptors matching the
 * reference's Block layouts (presto-common/.../block/LongArrayBlock.java:38-52,
 * IntArrayBlock, ByteArrayBlock, DictionaryBlock.java:53-64).
 *
 * In production the Java side binds this ABI through a thin JNI veneer
 * (see INTEGRATION.md for the binding a presto-main maintainer would add);
 * in this repo the same ABI is driven by the Python harness in presto_amd/
 * and by tests/ replicating OperatorAssertion.toPages
 * (presto-main-base/src/test/.../OperatorAssertion.java:62-176).
 *
 * Contract (verified by the reference's Driver, restated here):
 *  - one handle == one logical driver: all calls on a handle are
 *    single-threaded (Driver.processInternal holds an exclusive lock);
 *  - pg_op_add_input only when pg_op_needs_input returns 1
 *    (Driver.java:446-458); input pages are borrowed for the call;
 *  - pg_op_get_output may produce nothing (*out == NULL); output pages are
 *    owned by the library until the next pg_op_get_output/pg_op_destroy;
 *  - pg_op_finish is idempotent; cleanup via pg_op_destroy (close()).
 *  - build->probe bridging uses table handles (mirrors
 *    PartitionedLookupSourceFactory.java:149,181).
 *
 * Errors: negative return, message via pg_last_error().
 * All compute requires an AMD gfx950 GPU; calls fail loudly without one
 * (there is no CPU fallback in this library).
 */
#ifndef PRESTO_GPU_H
#define PRESTO_GPU_H
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define PG_ABI_VERSION 1

/* ---- status ---- */
typedef int32_t pg_status; /* 0 ok, <0 error */
#define PG_OK 0
#define PG_ERR (-1)
const char* pg_last_error(void);

/* ---- device helpers (memory plumbing for the harness; tensors may also be
 * allocated by the caller, e.g. torch, and passed as raw device pointers) */
pg_status pg_device_count(int32_t* out);
pg_status pg_device_sync(void);
pg_status pg_device_malloc(int64_t bytes, void** out);
pg_status pg_device_free(void* p);
pg_status pg_memcpy_h2d(void* dst, const void* src, int64_t bytes);
pg_status pg_memcpy_d2h(void* dst, const void* src, int64_t bytes);
pg_status pg_memcpy_d2d(void* dst, const void* src, int64_t bytes);
/* HIP-event elapsed ms of the most recent hot-path kernel launch (fused
 * scan+filter+aggregate, or probe+aggregate) — measurement plumbing for
 * bench.py's roofline leg */
double pg_last_hot_kernel_ms(void);
/* max hot-region ms since pg_hot_reset (for pipelines with several hot
 * launches per step: the max is the dominant one) */
double pg_hot_max_ms(void);
void pg_hot_reset(void);
/* how many HASH_AGG_SMALL pages this process has sent to the specialized
 * Q1-shape kernel rather than the generic one (tests pin which plans
 * take it) */
int64_t pg_q1_fast_launches(void);
/* how many agg_table build pages this process has sent to the staged
 * multi-row insert kernel rather than the generic direct insert (the
 * packed Q3/Q5 orders-build shape; PG_BUILD_STAGED=0 in the environment
 * at build creation forces the generic kernel) */
int64_t pg_build_staged_launches(void);
/* how many LOOKUP_JOIN mode-2 pages this process has sent to the Q5-shape
 * kernel (k_probe_agg_q5) rather than the generic k_probe_agg_fused2: the
 * gate is per page (packed table, no preds, DISC_PRICE over F64 columns,
 * I64 keys, dec_scale 4, 16-byte aligned key columns, no null masks) */
int64_t pg_mode2_q5_launches(void);
/* how many grouped (mode 1, single aggregate) LOOKUP_JOIN finishes this
 * process has extracted from the table's hit list (a gather of the slots
 * the probes first touched) rather than by scanning the accumulator array
 * (PG_GROUPS_LIST=0 in the environment at build creation forces the
 * scan) */
int64_t pg_groups_list_extractions(void);
/* how many LOOKUP_JOIN probe pages this process has sent through the
 * multi-key probe kernels (plans with n_keys >= 1) rather than the
 * single-key ones; an empty page launches nothing and is not counted */
int64_t pg_multikey_probe_pages(void);

/* ---- Page / Block descriptors (SURVEY.md §8b struct) ----
 * Concrete layouts follow the Java blocks: fixed-width values array +
 * optional byte-per-position null mask (LongArrayBlock.java:38-52). */
typedef enum {
    PG_T_U8 = 0,  /* ByteArrayBlock / dictionary codes */
    PG_T_I32 = 1, /* IntArrayBlock / DateType days */
    PG_T_I64 = 2, /* LongArrayBlock / BigintType */
    PG_T_F64 = 3, /* LongArrayBlock bits / DoubleType */
    PG_T_I128 = 5, /* Int128ArrayBlock (Int128ArrayBlock.java): 16-byte
                       little-endian (low, high) pairs — decimal(p>18,s)
                       unscaled values.  Carried through staging, IDENT
                       projection/emit and the INT128_ARRAY wire encoding;
                       decimal arithmetic accumulates through the exact
                       int128 totals of the aggregation paths
                       (fixed128.h, UnscaledDecimal128Arithmetic.java:770
                       add semantics). */
    PG_T_VARBIN = 4, /* VariableWidthBlock (VariableWidthBlock.java:48-61):
                        data = bytes, offsets = int32[n_rows+1] (element i
                        spans bytes [offsets[i], offsets[i+1])).  Supports
                        EQ/NE/CONTAINS/PREFIX predicates, hashing/
                        partitioning (XxHash64 per
                        AbstractVariableWidthBlock.java:102-105) and
                        IDENT projection/emit (two-pass gather).
                        Emit is implemented by FILTER_PROJECT only: every
                        other emitting operator (PARTITION, all LOOKUP_JOIN
                        emit modes, ORDER_BY, WINDOW, MARK_DISTINCT)
                        rejects a variable-width or dictionary emit column
                        at add_input, naming the entry.  One output column
                        holds at most 2^31-1 bytes (32-bit offsets);
                        FILTER_PROJECT fails with an error naming the
                        column beyond that.  A host column whose strings
                        are all empty may pass data = NULL. */
} pg_type;

typedef struct {
    int32_t tag;            /* pg_type */
    int32_t on_device;      /* 1: data is a device pointer */
    void* data;             /* values array (VARBIN: the byte buffer) */
    const uint8_t* null_mask; /* optional, 1 byte/pos, 1 = null; may be NULL.
                                 Within operators it is honored by
                                 predicates: a null on either side of a
                                 comparison excludes the row, and
                                 PG_CMP_IS_NULL / PG_CMP_IS_NOT_NULL test
                                 the mask itself; projections and
                                 aggregate inputs read the values array
                                 as is, except in GROUPBY_MULTI with
                                 sql_nulls = 1, whose group keys and
                                 SUM / MIN / MAX inputs honor the masks
                                 (see pg_plan_groupby).  Output pages
                                 carry masks only
                                 out of the outer LOOKUP_JOIN modes
                                 (PG_JOIN_PROBE_OUTER and up: null-padded
                                 payloads, gathered probe-column masks,
                                 the drain page), out of ORDER_BY
                                 (gathered masks of emitted columns, and
                                 its keys honor theirs), out of WINDOW
                                 (the same, plus the masks of its SUM,
                                 MIN, MAX, LAG and LEAD columns) and out
                                 of GROUPBY_MULTI with sql_nulls = 1 (its
                                 key and SUM / MIN / MAX columns) and out
                                 of MARK_DISTINCT (the masks of emitted
                                 columns, and its keys honor theirs); every
                                 other operator emits null_mask = NULL.
                                 A mask follows
                                 its column: host for host columns,
                                 device for device columns.
                                 pg_page_serialize / pg_page_deserialize
                                 carry masks through (nulls-as-bits on
                                 the wire). */
    const int32_t* offsets; /* VARBIN only: offsets (n_rows+1, or dict_n+1
                               for dictionary columns) */
    /* dictionary encoding (DictionaryBlock.java:60-86): when dict_ids is
     * non-NULL the column is a dictionary VARBIN block — data/offsets
     * describe the dict_n dictionary entries and dict_ids[n_rows] maps
     * each position to an entry.  Predicates, hashing/partitioning and
     * emit read through the ids. */
    const int32_t* dict_ids;
    int32_t dict_n;
} pg_col;

typedef struct {
    int64_t n_rows;
    int32_t n_cols;
    pg_col cols[32];
} pg_page;

/* ---- plan blobs ----
 * The reference JIT-compiles per-query filter/projection/accumulator classes
 * at runtime (sql/gen/PageFunctionCompiler.java:126, AccumulatorCompiler,
 * JoinCompiler).  The MI355X-native analog is a set of ahead-of-time
 * specialized HIP kernels selected by these plan descriptors. */

typedef enum { PG_CMP_LT = 0, PG_CMP_LE, PG_CMP_GT, PG_CMP_GE, PG_CMP_EQ,
               PG_CMP_NE,
               /* VARBIN only — the LIKE '%w%' / 'w%' pushdowns
                * (LikeFunctions.java:64-77 likeVarchar for patterns
                * without '_' reduce to substring/prefix search) */
               PG_CMP_CONTAINS, PG_CMP_PREFIX,
               /* ordered two-substring LIKE '%a%b%' (and its negation —
                * Q13's o_comment NOT LIKE '%special%requests%'):
                * sval holds a then b concatenated, slen = len(a),
                * ival = len(b) */
               PG_CMP_CONTAINS2, PG_CMP_NOT_CONTAINS2,
               /* null tests, any column type (VARBIN and dictionary
                * columns included): they read the column's null_mask
                * and nothing else — a column without a mask is never
                * null; ival, dval, sval and rhs_col are ignored.  They
                * are decided before the "a null excludes the row" rule,
                * so IS_NULL keeps exactly the rows that rule drops.
                * As a per-aggregate FILTER, IS_NOT_NULL turns COUNT
                * into count(col).  Accepted wherever predicates are,
                * except as build-side filters of dense_array and
                * agg_table HASH_BUILDs (single-scan kernels that
                * evaluate comparisons only): those fail pg_op_create. */
               PG_CMP_IS_NULL, PG_CMP_IS_NOT_NULL } pg_cmp;

typedef struct {
    int32_t col;   /* input channel */
    int32_t op;    /* pg_cmp */
    int64_t ival;  /* compare value for integer columns */
    double dval;   /* compare value for f64 columns */
    char sval[40]; /* VARBIN: compare bytes (EQ/NE/CONTAINS/PREFIX;
                      CONTAINS2 packs both patterns) */
    int32_t slen;  /* LENGTH RULES, checked at pg_op_create by every
                      operator that carries preds[] (the error names the
                      operator, the predicate index and the field):
                      0 <= slen <= sizeof sval; for CONTAINS2 and
                      NOT_CONTAINS2 also 0 <= ival and
                      slen + ival <= sizeof sval.  An empty needle matches
                      everywhere.  IS_NULL / IS_NOT_NULL ignore both.
                      TYPE RULES, checked at pg_op_add_input where the
                      column types are known (the error names the
                      predicate index): the ordering ops LT/LE/GT/GE are
                      not defined for VARBIN columns, and CONTAINS,
                      PREFIX, CONTAINS2 and NOT_CONTAINS2 are defined for
                      VARBIN columns only; a rejected page leaves the
                      operator as it was. */
    int32_t rhs_col; /* 0: compare against the constant; k>0: compare
                        against integer channel k-1 PLUS the constant
                        (col OP col + ival / dval — e.g. Q5's
                        c_nationkey = s_nationkey, TPC-DS Q72's
                        d3.d_date > d1.d_date + 5).  Zero-initialized
                        plans keep constant semantics. */
} pg_pred;

/* projection expressions (PageProjection analogs) */
typedef enum {
    PG_PROJ_IDENT = 0,        /* column a */
    PG_PROJ_DISC_PRICE = 1,   /* a * (1 - b)            (Q1/Q3 revenue) */
    PG_PROJ_CHARGE = 2,       /* a * (1 - b) * (1 + c)  (Q1 charge) */
    PG_PROJ_MUL = 3,          /* a * b                  (Q6 revenue) */
    PG_PROJ_DIV = 4,          /* a / b (f64 emit only — e.g. a grouped
                                 sum/count mean materialized for a
                                 downstream compare, Q21's only-late
                                 supplier) */
    PG_PROJ_KEYSHL = 5,       /* (a << c) | b — composite grouping keys
                                 (c = shift constant, i64 emit; the
                                 codegen analog of CombineHashFunction
                                 key packing for multi-channel group-bys,
                                 e.g. Q16's (brand,type,size,suppkey)) */
    PG_PROJ_SHR = 6,          /* a >> c — composite key extraction */
    PG_PROJ_SUBDIV = 7,       /* (a - b) / c with b, c CONSTANTS (i64
                                 emit; floor division of non-negative
                                 differences) — planner expressions like
                                 date -> week_seq ((date - day0) / 7) or
                                 multiplicity - 1 */
    PG_PROJ_KEYSHL_DIV = 8,   /* (a << shift) | (b / div) with
                                 c = (shift << 16) | div — composite keys
                                 over a derived dimension (e.g. TPC-DS
                                 Q72's (item, week) key in ONE pass:
                                 item << 14 | date/7) */
} pg_proj_kind;

typedef struct {
    int32_t kind; /* pg_proj_kind */
    int32_t a, b, c; /* input channels */
} pg_proj;

/* aggregate functions over a projection */
typedef enum {
    PG_AGG_COUNT = 0,    /* CountAggregation.java:34 */
    PG_AGG_SUM_F64 = 1,  /* DoubleSumAggregation (deterministic schedule,
                            DESIGN.md §determinism).  DOMAIN in
                            GROUPBY_MULTI and the fused-agg probes
                            (LOOKUP_JOIN modes 1/3), which sum in exact
                            64.64 fixed point: every addend must satisfy
                            0 <= x < 2^53 with no fraction bits below
                            2^-64 (x = 0 or x >= ~2^-12); the result is
                            then the correctly rounded exact sum.  A
                            negative, NaN, >= 2^53 or finer addend makes
                            finish fail with an error naming SUM_F64
                            (signed f64 sums are unsupported there).
                            NOT checked: LOOKUP_JOIN mode 2, whose
                            callers guarantee non-negative money (its
                            kernels are off the benchmark headline, so
                            the cost of a check there is unmeasured).
                            HASH_AGG_SMALL sums plain f64 in its fixed
                            schedule and has no such domain. */
    PG_AGG_SUM_DEC = 2,  /* exact decimal ticks; scale from dec_scale
                            (hive-decimal semantics of the golden vectors) */
    PG_AGG_SUM_I64 = 3,  /* LongSumAggregation.java:33-37 */
    PG_AGG_MIN = 4,      /* MinAggregationFunction: decimal-ticks/i64 min
                            in decimal mode, f64 min in f64 mode */
    PG_AGG_MAX = 5,
} pg_agg_func;

typedef struct {
    int32_t func;     /* pg_agg_func */
    pg_proj proj;     /* input expression */
    int32_t dec_scale; /* for SUM_DEC: ticks = round(value * 10^dec_scale).
                          Rounding is half away from zero, so negative
                          values mirror positive ones (-1.23 at scale 2
                          -> -123 ticks, -0.01 -> -1); the
                          operands of MUL/DISC_PRICE/CHARGE are each
                          rounded to hundredths the same way.
                          EXCEPTIONS, defined for non-negative money
                          only: the Q1-shape fast path of HASH_AGG_SMALL
                          (Q1 plan shape over f64 columns without null
                          masks) and the Q5-shape mode-2 probe
                          (DISC_PRICE over f64 columns on a packed
                          table, no predicates) round with a plain
                          +0.5. */
} pg_agg;

/* -------- operator kinds + plans -------- */
typedef enum {
    PG_OP_FILTER_PROJECT = 1, /* ScanFilterAndProjectOperator.java:67 +
                                 PageProcessor.java:112,299-343 */
    PG_OP_HASH_AGG_SMALL = 2, /* HashAggregationOperator.java:56 with
                                 low-cardinality dict-u8 keys (Q1 shape) */
    PG_OP_HASH_BUILD = 3,     /* HashBuilderOperator.java:55 */
    PG_OP_LOOKUP_JOIN = 4,    /* LookupJoinOperator.java:481-604 (optionally
                                 fused with grouped SUM into the table —
                                 Q3's join+partial-agg pipeline) */
    PG_OP_TOPN = 5,           /* TopNOperator.java:32,90-111 */
    PG_OP_PARTITION = 6,      /* PartitionedOutputOperator.partitionPage:394 /
                                 LocalExchange partition split */
    PG_OP_GROUPBY_MULTI = 7,  /* MultiChannelGroupByHash.java:300-380 +
                                 InMemoryHashAggregationBuilder: general
                                 grouped aggregation over 1..4 key
                                 channels of mixed type at arbitrary
                                 cardinality (see pg_plan_groupby) */
    PG_OP_ORDER_BY = 8,       /* OrderByOperator.java + PagesIndex.sort /
                                 PagesIndexOrdering + SortOrder.java; with
                                 a limit, the general TopNOperator (see
                                 pg_plan_order_by) */
    /* 9 is left unassigned */
    PG_OP_WINDOW = 10,        /* WindowOperator.java: ranking functions,
                                 running and whole-partition aggregates,
                                 LAG / LEAD over PARTITION BY ... ORDER BY
                                 ... (see pg_plan_window) */
    /* 11 is left unassigned */
    PG_OP_MARK_DISTINCT = 12, /* MarkDistinctOperator.java +
                                 MarkDistinctHash.java: a first-occurrence
                                 marker column over 1..4 key channels; in
                                 PG_DISTINCT_ONLY mode SELECT DISTINCT and
                                 DistinctLimitOperator.java (see
                                 pg_plan_mark_distinct) */
} pg_op_kind;

#define PG_MAX_PRED 8
#define PG_MAX_AGG 8
#define PG_MAX_KEYVALS 8

typedef struct {
    int32_t n_preds;
    pg_pred preds[PG_MAX_PRED]; /* conjunction */
    int32_t n_proj;
    pg_proj proj[16];
    int64_t semijoin_table; /* >0: keep only rows whose semijoin_col key is
                               in that key-set table (EXISTS pushdown, e.g.
                               Q4); 0 = unused */
    int32_t semijoin_col;
    int32_t semijoin_anti;  /* 1: keep rows whose key is NOT in the set
                               (NOT-EXISTS pushdown, e.g. Q22's customers
                               without orders — LookupJoinOperator's
                               probe-side anti join) */
} pg_plan_filter_project;

typedef struct {
    /* up to two u8 key channels with enumerated code values; group id =
     * idx(key0)*n_vals1 + idx(key1); results emitted in that order,
     * restricted to non-empty groups */
    int32_t n_preds;
    pg_pred preds[PG_MAX_PRED]; /* fused pre-filter (scan+filter+agg) */
    int32_t n_keys;             /* 0 (single global group), 1 or 2 */
    int32_t key_col[2];
    int32_t n_vals[2];
    uint8_t key_vals[2][PG_MAX_KEYVALS];
    int32_t n_aggs;
    pg_agg aggs[PG_MAX_AGG];
    int32_t drop_unlisted_keys; /* 1: rows whose key is outside key_vals are
                                   dropped (dictionary-filter pushdown, e.g.
                                   Q5's region membership); 0: error */
} pg_plan_hash_agg_small;

typedef struct {
    int32_t n_preds;
    pg_pred preds[PG_MAX_PRED]; /* fused pre-filter on build input */
    int32_t key_col;            /* bigint key channel */
    int64_t semijoin_table;     /* >=0: keep only rows whose column
                                   semijoin_col matches that table's key set
                                   (Q3: orders ⋉ building-customers) */
    int32_t semijoin_col;
    int32_t n_payload;
    int32_t payload_col[4];     /* i32/i64 payload channels stored per row */
    int64_t capacity_hint;      /* expected distinct build rows */
    int32_t key_set_only;       /* 1: build a key SET (no payload slots) */
    int32_t dense_array;        /* 1: keys are dense 1..capacity_hint —
                                   store the single u8 payload in a direct
                                   array indexed by key-1 (no hashing);
                                   e.g. suppkey -> s_nationkey */
    /* agg_table only: fetch the u8 payload THROUGH another agg table
     * (star-schema dimension join fused into the build: e.g. Q5's orders
     * build stores customer nation = cust_table[o_custkey].payload; rows
     * whose lookup key misses are dropped).  0 = unused. */
    int64_t payload_lookup_table;
    int32_t payload_lookup_key_col;
    int32_t agg_table;          /* 1: table feeds a fused-agg probe only
                                   (LOOKUP_JOIN mode 1).  Rows are inserted
                                   directly during addInput (single scan,
                                   payloads stored per slot, keys must be
                                   unique); join-emit probing (chains) is
                                   rejected.  capacity_hint must be >= the
                                   number of inserted rows (errors out
                                   otherwise). */
    /* agg_table only: store the single payload in the low pack_bits of
     * the key slot word (slot = key << pack_bits | payload) so one CAS
     * carries key AND payload — one random line per insert and per probe
     * hit instead of two.  Caller guarantees 0 <= key < 2^(63-pack_bits)
     * and 0 <= payload < 2^pack_bits (checked; insert errors out
     * otherwise).  The analog of the reference's SyntheticAddress
     * packing (SyntheticAddress.java:23-36), applied to slot payloads.
     * 0 = unpacked.  Requires n_payload == 1. */
    int32_t pack_bits;
    /* agg_table only: capacity multiplier x10 (0 = default 20, i.e.
     * cap = next_pow2(2 x capacity_hint), fill <= ~0.5 — sized for
     * short linear-probe clusters on miss-heavy probes).  Probes that
     * ALWAYS hit (e.g. lineitem -> its order) can size tighter: 13
     * gives fill <= ~0.77 and halves the table/accumulator footprint. */
    int32_t fill_x10;
    /* > 0: also build a key-presence BITMAP over [1, bitmap_max_key]
     * (one bit per possible key; the analog of the reference's bigint
     * dynamic-filter / bloom pre-filter in front of a join probe,
     * DynamicFilterSourceOperator.java:214-258 collecting and
     * LookupJoinOperator applying it).  Probes test the bit BEFORE
     * computing the bucket hash: on miss-heavy probes of primary-key
     * domains (orderkey spans 4 x orders rows, so the SF100 bitmap is
     * 75 MB — L3-resident) this replaces the hash + tag-line dependent
     * chain with one cached load for ~90% of rows.  Build keys outside
     * [1, bitmap_max_key] are an error (the bitmap cannot represent
     * them, so probes would wrongly reject).  0 = no bitmap. */
    int64_t bitmap_max_key;
    /* 1: a RANGE-GROUP table — the group-by domain is the dense key
     * range [1, capacity_hint] itself (the perfect-hash GroupByHash
     * analog for primary-key-shaped bigint group channels, cf.
     * BigintGroupByHash.java:66-117 whose probe is exactly a
     * value->bucket map).  No build input is scanned and no key slots
     * are stored: a mode-1 fused-agg probe indexes its accumulators by
     * key-1 directly (keys outside the range are misses, matching
     * inner-join-with-FK semantics), and group extraction reconstructs
     * the key from the slot index.  For probe inputs CLUSTERED by the
     * key (lineitem by orderkey) the accumulator atomics become
     * near-sequential instead of hash-scattered. */
    int32_t range_group;
    /* dense_array only: constant added to the payload value at fill
     * time (probe-side consumers see value+bias).  Lets 0-valued
     * payloads (nationkey 0, priority 0) coexist with "presence =
     * nonzero" dense probing; the pipeline accounts for the bias in
     * its downstream predicates. */
    int32_t dense_payload_bias;
    /* MULTI-CHANNEL JOIN KEYS — the JoinHash / PagesHash analog
     * (PagesHash.java:81-181, JoinCompiler: a join on any list of hash
     * channels).  n_keys = 0 (a zero-initialised plan): the single bigint
     * key_col above, every table shape above, unchanged.  n_keys = 1..4:
     * a MULTI-KEY CHAINED table over key_cols[0, n_keys), most
     * significant first; key_col is ignored.
     *   - Shape: takes preds, semijoin_table / semijoin_col and
     *     payload_col[] (U8 / I32 / I64 / F64) and nothing else —
     *     agg_table, dense_array, range_group, key_set_only, pack_bits,
     *     fill_x10, bitmap_max_key and payload_lookup_table each fail
     *     pg_op_create with an error naming HASH_BUILD, n_keys and the
     *     field.  n_keys outside 0..4, or a negative key_cols entry, fails
     *     create.
     *   - Key types: U8, I32 or I64 columns, checked at add_input (F64,
     *     I128, VARBIN and dictionary keys are errors naming the key index
     *     and the column: ids of two dictionaries are not comparable) and
     *     the same on every page of one operator.  Each channel compares
     *     as the signed 64-bit value of the column (U8 zero-extended, I32
     *     sign-extended), so build and probe channels may differ in width:
     *     I32 -1 equals I64 -1, U8 255 equals I64 255 and not I32 -1.
     *     Equality is exact on the whole key vector (never a fingerprint)
     *     and positional: (1, 2) does not match (2, 1).
     *   - Null keys (SQL join semantics): a row whose key is null in any
     *     channel (the column has a null_mask and null_mask[i] != 0)
     *     matches nothing — null does not equal null here, unlike
     *     MARK_DISTINCT — and the value under a null never matters.  A
     *     build row with a null key is kept in the build-row arrays (it
     *     counts in build-row order and the outer modes drain it) but is
     *     never inserted into the table.  Build payload masks stay out of
     *     scope.
     *   - Build rows are capped at 2^31-1 (row ids are 32-bit): finish
     *     fails beyond that.
     *   - The table is probed by LOOKUP_JOIN plans with the same n_keys in
     *     modes 0, 4, 5 and 6 (see pg_plan_lookup_join), and cannot serve
     *     as a semijoin_table, payload_lookup_table or table2. */
    int32_t n_keys;      /* 0: legacy, key_col is the one bigint key;
                            1..4: multi-key */
    int32_t key_cols[4]; /* most significant first; only [0, n_keys) are
                            read */
} pg_plan_hash_build;

/* pg_plan_lookup_join.mode values of the emit joins (modes 1-3 are the
 * fused aggregating probes described in the struct) */
#define PG_JOIN_INNER 0        /* INNER: matched rows only */
#define PG_JOIN_PROBE_OUTER 4  /* LEFT:  + null-padded unmatched probe rows */
#define PG_JOIN_LOOKUP_OUTER 5 /* RIGHT: + drain page of unmatched build rows */
#define PG_JOIN_FULL_OUTER 6   /* FULL:  both */

typedef struct {
    int64_t table;    /* handle from a finished PG_OP_HASH_BUILD */
    int32_t n_preds;
    pg_pred preds[PG_MAX_PRED]; /* fused pre-filter on probe input */
    int32_t key_col;
    /* mode 2: fully fused probe + dense lookup + equality + small-key
     *   grouped SUM (the specialization for Q5's local-supplier shape):
     *   for each probe row passing preds: g1 = table[key_col] payload
     *   (u8), g2 = dense table2[table2_key_col], keep when g1 == g2 and
     *   g2 is one of group_vals; acc[g2] += proj (exact ticks + fx128).
     *   get_output after finish: host page [group u8, sum_dec i64 ticks,
     *   sum_f64, count i64] in group_vals order (non-empty groups).
     * mode 0: emit matched rows — output page =
     *   probe columns emit_probe_cols[] + build payloads (join emit order:
     *   probe rows ascending; within a probe row, chain head first —
     *   LookupJoinPageBuilder.appendRow:75 + ArrayPositionLinks order)
     * mode 3: fused star-join grouped SUM — probe table (chained, first
     *   payload = an i64 grouping key, e.g. orders keyed by orderkey
     *   with o_custkey payload), accumulate proj into table2's slots
     *   keyed by that payload (Q10: revenue per customer in ONE pass
     *   over lineitem).  get_output emits table2's groups page.
     * mode 1: fused grouped SUM into the build table (group = join key):
     *   for each match, table.acc += proj(probe row) in exact decimal ticks
     *   AND exact-f64 fixed-point (fixed128.h); get_output after finish
     *   emits the groups page: key i64, payloads..., sum_dec i64,
     *   sum_f64 f64 (rows = groups with >=1 match)
     * modes 4/5/6 (PG_JOIN_PROBE_OUTER / LOOKUP_OUTER / FULL_OUTER): the
     *   outer emit joins — LookupJoinOperator with probeOnOuterSide and
     *   LookupOuterOperator.  Each is mode 0 plus:
     *   4 (LEFT): a probe row that passes preds and has no match emits
     *     one row whose payload columns are null;
     *   5 (RIGHT): finish() queues one drain page of the build rows no
     *     probe row of this operator matched;
     *   6 (FULL): both.
     *   - Predicates: probe rows failing preds emit nothing in every
     *     mode (preds are the filter below the join), and only a probe
     *     row that passed preds marks a build row as matched.
     *   - Null probe keys: in modes 4 and 6 a key that is null in its
     *     null_mask never matches; the row is emitted null-padded.  In
     *     mode 5 it emits nothing.  Modes 0-3 do not read the key mask.
     *     Build-key masks are out of scope in every mode (build keys
     *     are taken as non-null).
     *   - Row order of probe pages is mode 0's; an unmatched row sits
     *     at its probe-row position.  Columns are the emit_probe_cols
     *     (fixed width only) then the build payloads.
     *   - Payload mask: in modes 4 and 6 every payload column of a probe
     *     output page carries a device null_mask of n_rows bytes (the
     *     payload columns share one buffer); a payload value under a
     *     null is 0.  In mode 5 payload masks are NULL.
     *   - Probe-column masks: in modes 4-6 an emitted probe column whose
     *     input column has a null_mask carries it through, gathered
     *     with the values; otherwise its null_mask is NULL.  Mode 0
     *     drops masks.
     *   - Drain page (modes 5, 6): exactly one, possibly of 0 rows,
     *     queued by finish().  Rows: the unmatched build rows in
     *     ascending build-row order (insertion order across build
     *     pages).  Probe columns are typed as in the first page fed
     *     (I64 when none was), hold 0 and share one all-ones mask;
     *     payload columns hold the values, null_mask NULL.
     *   - Match marks belong to the operator: one byte per build row,
     *     zeroed at creation.  Several probe operators sharing one set
     *     of marks (a partitioned probe with a single drain) is out of
     *     scope — each operator drains what IT did not match.
     *   - Tables: mode 4 takes every shape mode 0 takes (chained,
     *     agg_table slot-payload incl. packed, dense_array); modes 5
     *     and 6 take chained tables only and fail pg_op_create
     *     otherwise.
     *   - An empty probe page gives a 0-row page with the same columns.
     *   - All masks are owned by the output page: valid until the next
     *     pg_op_get_output / pg_op_destroy. */
    int32_t mode;
    int32_t n_emit;
    int32_t emit_probe_cols[8];
    pg_proj proj;
    int32_t dec_scale;
    /* mode 2 only: */
    int64_t table2;          /* dense_array build */
    int32_t table2_key_col;
    int32_t n_group_vals;
    uint8_t group_vals[8];
    /* mode 1 only: skip the exact-f64 (fx128) accumulator legs when the
     * consumer reads only the decimal sum + count (integer aggregates
     * such as Q17/Q18/Q21 quantity sums — halves the atomic traffic of
     * all-match probes) */
    int32_t dec_only;
    /* mode 1 only: the decimal accumulator keeps the MIN of the
     * projected ticks instead of the sum (MinAggregationFunction over a
     * grouped probe — Q2's per-part minimum supplycost).  Implies
     * dec_only. */
    int32_t dec_min;
    /* mode 1 only: MULTI-ACCUMULATOR probe — the full
     * InMemoryHashAggregationBuilder.processPage:204 analog (one
     * getGroupIds probe, then EVERY aggregator's addInput), optionally
     * with per-aggregate FILTER clauses (AggregationNode's
     * aggregation masks).  n_aggs > 0 replaces the single proj/dec legs:
     * per-slot accumulators are n_aggs int64 tick sums plus the match
     * count; agg_filter[a] >= 0 indexes a predicate in preds[] that
     * gates aggregate a alone (row-level filtering still uses
     * preds[0..n_preds)).  Overflow-checked (Math.addExact).  Output
     * page after finish: key, payloads..., agg0..agg{n-1}, count, one row
     * per key with count >= 1, in no particular order.
     *   - Functions: PG_AGG_COUNT (its proj is ignored), PG_AGG_SUM_DEC
     *     and PG_AGG_SUM_I64 only — every accumulator is an int64 tick
     *     sum.  SUM_F64, MIN and MAX fail pg_op_create with an error that
     *     names the aggregate and the function.
     *   - The count is the number of rows that passed preds[0..n_preds)
     *     and found their key.  A FILTER gates its own aggregate and
     *     nothing else: a row it rejects adds nothing to that sum, still
     *     feeds every other aggregate and still counts, so a group whose
     *     rows a FILTER rejects all the same comes out with sum 0 and its
     *     full count.  agg_filter[a] may also name a row predicate (an
     *     index below n_preds).
     *   - A row that fails the row predicates is skipped before its key
     *     is read.
     *   - Overflow: a group whose exact total leaves int64 raises at
     *     finish when its addends share one sign.  With mixed signs
     *     detection follows the order of the partial sums: totals whose
     *     sum of |addends| stays below 2^63 never raise.
     *   - Several pages, and several operators one after the other on one
     *     table, accumulate into the same slots; the table keeps the
     *     layout of its first multi-agg operator (n_aggs and the acc_pack
     *     fields below) and a later operator that declares another one
     *     fails pg_op_create with "different multi-agg layout".
     *     pg_table_reset_acc zeroes the sums and keeps the layout. */
    int32_t n_aggs; /* 0 = legacy single proj; 1..6 multi */
    pg_agg aggs[6];
    int32_t agg_filter[6];
    /* Multi-agg accumulator PACKING (the slot-word analog of pack_bits,
     * applied to the accumulator state): aggregates whose per-GROUP
     * totals the caller can bound (integrity facts like "<= 7 lineitems
     * per order" and "suppkey < supplier count") share ONE u64 word as
     * bit fields, so a probe flush issues one atomicAdd on one line
     * instead of one per aggregate — the multi-agg probe is atomic-op-
     * rate bound, not bandwidth bound.  acc_pack = 1 enables it;
     * acc_pack_shift[a] is the field's bit offset in word 0 or -1 for a
     * full u64 word of its own (appended after word 0 in agg order);
     * acc_pack_width[a] the field width.  The count field lives at
     * acc_pack_cnt_shift/width in word 0.  CONTRACT: the caller
     * guarantees every per-group TOTAL fits its declared field; each
     * probe flush additionally checks its own contribution against the
     * width and raises the overflow error on violation (gross width
     * mistakes fail loudly; the bound itself is the caller's integrity
     * fact, as with pack_bits).  Output schema is unchanged — group
     * extraction unpacks the fields.
     *   - Field widths and the count width are 1..63, shifts are >= 0
     *     (-1 = own word, for an aggregate only) and shift + width <= 64;
     *     fields may not overlap each other or the count.  A 64-bit field
     *     is an own word.  Anything else fails pg_op_create with an error
     *     naming the field; the width of an own-word aggregate is not
     *     read.
     *   - A bit field is unsigned.  A non-negative contribution that the
     *     group's total fits never raises, up to a total of exactly
     *     2^width - 1 (and 2^cnt_width - 1 rows), without touching the
     *     neighbouring fields or slots.  A contribution of 2^width or
     *     more, and a negative contribution that its run of equal keys
     *     does not cancel, raise the overflow error at finish.
     *   - Own words are signed int64 sums with the unpacked overflow
     *     rules. */
    int32_t acc_pack;
    int32_t acc_pack_shift[6];
    int32_t acc_pack_width[6];
    int32_t acc_pack_cnt_shift;
    int32_t acc_pack_cnt_width;
    /* MULTI-CHANNEL JOIN KEYS (see pg_plan_hash_build.n_keys).  n_keys = 0:
     * key_col above, unchanged.  n_keys = 1..4: the probe key is the
     * vector key_cols[0, n_keys) of U8 / I32 / I64 columns (checked at
     * add_input like the build's; the same on every page) and key_col is
     * ignored.
     *   - n_keys must equal the table's: a multi-key plan on a legacy
     *     table, a legacy plan on a multi-key table, or two different
     *     counts fail pg_op_create with an error naming both counts.
     *   - Modes 0, 4, 5 and 6 only; modes 1-3 fail create, naming the
     *     mode.
     *   - Null probe keys: a probe row whose key is null in any channel
     *     matches nothing in EVERY mode of the multi-key path — mode 0
     *     included, which drops the row.  (The legacy mode 0 does not read
     *     the key mask; no existing plan changes, the path is new.)  Modes
     *     4 and 6 emit the row null-padded, mode 5 emits nothing.
     *   - Everything else is the emit contract above word for word: probe
     *     rows ascending, the order among one probe row's matches
     *     unpinned, emit_probe_cols then the payloads, the payload mask in
     *     modes 4 and 6, gathered probe-column masks in modes 4-6, one
     *     drain page in build-row order across build pages (build rows
     *     with a null key are never matched, so they drain), marks owned
     *     by the operator, a 0-row page for an empty probe page, preds
     *     applied below the join. */
    int32_t n_keys;      /* 0: legacy, key_col is the one bigint key;
                            1..4: multi-key */
    int32_t key_cols[4]; /* most significant first; only [0, n_keys) are
                            read */
} pg_plan_lookup_join;

typedef struct {
    /* General multi-channel grouped aggregation — the
     * MultiChannelGroupByHash.java:300-380 analog: arbitrary group
     * cardinality over 1..4 key channels of mixed I64/I32/U8 or
     * dictionary-VARBIN type (dictionary keys group by their dictionary
     * id — DictionaryBlock identity, emitted back as I32 ids into the
     * same dictionary; requires distinct dictionary entries, i.e. a
     * proper dictionary).  Open-address table, linear probe, group hash
     * = murmur3-finalized CombineHashFunction fold of the per-channel
     * bigint hashes (CombineHashFunction.java:28-30,
     * AbstractLongType.java:137-140); multi-word keys are claimed with
     * a per-slot state word (CAS-claim, release-publish), so concurrent
     * inserts are exact — never fingerprint-approximate.
     * Aggregates: SUM_DEC/SUM_I64 (overflow-checked ticks), COUNT,
     * SUM_F64 (exact 64.64 fixed point), MIN/MAX (integer ticks), each
     * optionally gated by a FILTER predicate (agg_filter indexes
     * preds[]; row-level filtering uses preds[0..n_preds)).
     * Output after finish: key channels (input types), then per
     * aggregate its value column (I64 ticks or F64), then the group
     * row count; groups emitted slot-ascending (order is not part of
     * the contract, as with the reference's parallel drivers).
     * capacity_hint must be >= the number of distinct groups (errors
     * out past fill 0.85, like agg tables).
     *
     * sql_nulls (the last field): 0 = the behaviour above, in which key
     * channels and aggregate inputs read the values array as is and the
     * output carries no masks; 1 = SQL null semantics, below; any other
     * value fails pg_op_create with an error naming sql_nulls.
     *   - Row predicates preds[0..n_preds) are unchanged: a null
     *     excludes the row, IS_NULL / IS_NOT_NULL test the mask.
     *   - Group keys: a key channel is null at row i when its column has
     *     a null_mask and null_mask[i] != 0 (for a dictionary VARBIN key
     *     that is the per-position mask).  Null groups with null in that
     *     channel (IS NOT DISTINCT FROM) and is distinct from every
     *     value; the value stored under a null never influences
     *     grouping.  Channels are independent: (null, 1), (0, 1),
     *     (null, null) and (0, null) are four groups.  Grouping stays
     *     exact: the per-channel null flags are one more word of the
     *     compared key vector, never part of a fingerprint.
     *   - COUNT stays count(*) over the rows that pass the row
     *     predicates and its own FILTER; its proj is ignored (a zeroed
     *     proj is NOT count(col 0)).  count(x) is spelled
     *     COUNT FILTER (x IS NOT NULL).
     *   - SUM_DEC, SUM_I64, SUM_F64, MIN, MAX: the input is null when
     *     any column the projection reads is null at that row (IDENT,
     *     SHR, SUBDIV read a; DISC_PRICE, MUL, DIV, KEYSHL, KEYSHL_DIV
     *     read a and b; CHARGE reads a, b and c; constants held in b or
     *     c are not columns).  A null input is skipped before it is
     *     evaluated, so the bits under a mask reach neither the overflow
     *     check, the SUM_F64 domain check nor the accumulator.  A group
     *     in which an aggregate received no non-null input (all inputs
     *     null, its FILTER rejected every row, or both) emits null for
     *     it.  A non-null input of value 0 is an input: a group of zeros
     *     sums to 0, not null.  Overflow and SUM_F64 domain errors apply
     *     to the non-null inputs as with sql_nulls = 0.
     *   - The trailing row count is unchanged: the rows of the group
     *     that passed the row predicates.
     *   - Output masks: every key column and every SUM / MIN / MAX
     *     column carries a device null_mask of n_rows bytes, owned by
     *     the output page (valid until the next pg_op_get_output /
     *     pg_op_destroy); the value under a null is 0.  COUNT columns
     *     and the row count have null_mask = NULL.
     *   - Out of scope: HASH_AGG_SMALL and the fused aggregating probes
     *     (LOOKUP_JOIN modes 1-3) keep reading values as is; F64 and
     *     I128 group keys and signed SUM_F64 stay unsupported. */
    int32_t n_preds;
    pg_pred preds[PG_MAX_PRED];
    int32_t n_keys;
    int32_t key_col[4];
    int64_t capacity_hint;
    int32_t n_aggs;
    pg_agg aggs[6];
    int32_t agg_filter[6];
    int32_t sql_nulls;
} pg_plan_groupby;

typedef struct {
    /* ORDER BY value DESC, date ASC, key ASC LIMIT n  (Q3 shape).
     * NaN values are unsupported (their order is unspecified). */
    int32_t limit;
    int32_t val_col;  /* i64 (decimal ticks) or f64 */
    int32_t date_col; /* i32 */
    int32_t key_col;  /* i64 */
} pg_plan_topn;

typedef struct {
    int32_t n_partitions;
    int32_t key_col; /* bigint; rawHash = CombineHashFunction fold from
                        INITIAL_HASH_VALUE=0 of AbstractLongType.hash
                        (PlannerUtils.java:113, AbstractLongType.java:137-140);
                        partition = HashGenerator.java:22-29.  A VARBIN
                        (raw or dictionary) key hashes its bytes with
                        XxHash64.  The key's null_mask is NOT read:
                        partitioning null keys is out of scope */
    int32_t n_emit;
    int32_t emit_cols[8]; /* fixed-width columns only (see PG_T_VARBIN) */
} pg_plan_partition;

#define PG_MAX_SORT_KEYS 4
#define PG_MAX_SORT_EMIT 16
typedef enum { /* SortOrder.java */
    PG_SORT_ASC_NULLS_FIRST = 0, PG_SORT_ASC_NULLS_LAST = 1,
    PG_SORT_DESC_NULLS_FIRST = 2, PG_SORT_DESC_NULLS_LAST = 3 } pg_sort_order;

typedef struct {
    /* PG_OP_ORDER_BY: a stable multi-key sort of the accumulated pages,
     * entirely on the GPU, with an optional LIMIT — OrderByOperator.java
     * over PagesIndex.sort / PagesIndexOrdering, orders per SortOrder.java.
     *   - Lifecycle: the operator accumulates; needs_input is 1 until
     *     finish and get_output before finish gives NULL.  finish is
     *     idempotent and queues exactly one page, possibly of 0 rows;
     *     is_finished turns true once that page has been taken.  Input
     *     pages are borrowed: the key and emit columns are copied into
     *     buffers the operator owns.  Pages may be host- or
     *     device-resident, also mixed.  The output page is
     *     device-resident, owned by the operator until the next
     *     pg_op_get_output / pg_op_destroy, and can be fed raw into
     *     another operator.
     *   - Keys: U8, I32, I64 or F64 columns, most significant first.
     *     Integers compare signed, U8 unsigned.  F64 orders as
     *     Double.compare: -inf < ... < -0.0 < +0.0 < ... < +inf < NaN;
     *     every NaN, whatever its sign or payload, equals every other NaN
     *     and is greater than +inf.
     *   - Nulls: a key's null_mask is honored.  Null keys go first or
     *     last as the order says, independently of ASC/DESC, and compare
     *     equal to each other; the value stored under a null never
     *     influences the order.  A page without a mask for the column
     *     contributes no nulls.
     *   - Stability: rows that compare equal on all keys keep their input
     *     order (page order, then row order), for ASC and DESC alike.
     *     This is STRICTER than the reference, whose PagesIndex.sort is
     *     not stable; it makes the output deterministic.
     *   - Output: the emit_cols columns, in that order, permuted by the
     *     sort.  Emit columns are fixed width (U8, I32, I64, F64, I128);
     *     a key need not be emitted and a column may be emitted twice.
     *     Values are copied bit for bit (NaN payloads, -0.0 and values
     *     under nulls survive).  An emitted column that had a null_mask
     *     on any input page carries a gathered device mask (pages
     *     without one contribute zeros); otherwise its null_mask is NULL.
     *     With no page fed at all, the 0-row page types its columns I64;
     *     otherwise the types are the first page's.
     *   - Limit: limit > 0 keeps the first min(limit, n) sorted rows;
     *     0 means no limit.
     *   - Errors at create, naming the field: n_keys outside 1..4, n_emit
     *     outside 1..16, an unknown order, a negative limit, a negative
     *     column index.  Errors at add_input, naming the column: an index
     *     >= n_cols, a VARBIN or dictionary key or emit column, an I128
     *     key, a type that differs from the first page's.  More than
     *     2^31-1 accumulated rows is an error (row ids are 32-bit).
     *   - Out of scope: variable-width keys or emit columns; I128 keys;
     *     expression keys (project them first through FILTER_PROJECT); a
     *     preselection fast path for small limits; spilling. */
    int32_t n_keys;                    /* 1..4, most significant first */
    int32_t key_col[PG_MAX_SORT_KEYS];
    int32_t order[PG_MAX_SORT_KEYS];   /* pg_sort_order */
    int32_t n_emit;                    /* 1..16 */
    int32_t emit_cols[PG_MAX_SORT_EMIT];
    int64_t limit;                     /* 0 = none; >0: first `limit` rows */
} pg_plan_order_by;

#define PG_MAX_WIN_FUNCS 8
typedef enum { PG_WIN_ROW_NUMBER = 0, PG_WIN_RANK, PG_WIN_DENSE_RANK,
               PG_WIN_COUNT, PG_WIN_SUM, PG_WIN_MIN, PG_WIN_MAX,
               PG_WIN_LAG, PG_WIN_LEAD } pg_win_func;
typedef enum { PG_FRAME_RANGE_RUNNING = 0, /* RANGE UNBOUNDED PRECEDING..CURRENT ROW (SQL default) */
               PG_FRAME_ROWS_RUNNING  = 1, /* ROWS  UNBOUNDED PRECEDING..CURRENT ROW */
               PG_FRAME_PARTITION     = 2  /* the whole partition */ } pg_win_frame;
typedef struct { int32_t func;   /* pg_win_func */
                 int32_t col;    /* argument channel (see per function) */
                 int32_t frame;  /* pg_win_frame; aggregates only */
                 int32_t pad;
                 int64_t offset; /* LAG / LEAD: rows back / ahead, >= 0 */
} pg_win_spec;

typedef struct {
    /* PG_OP_WINDOW: window functions over PARTITION BY ... ORDER BY ... of
     * the accumulated pages, entirely on the GPU — WindowOperator.java with
     * the functions of operator/window/ (RowNumberFunction, RankFunction,
     * DenseRankFunction, LagFunction, LeadFunction, AggregateWindowFunction
     * over count / sum / min / max).  The rows are sorted by ORDER_BY's
     * sort; partition and peer-group boundaries, one segmented scan per
     * aggregate and the per-function emit follow it.
     *   - Lifecycle, page residency, key types, null ordering,
     *     Double.compare order, emit columns and their gathered masks, the
     *     0-row page, column typing from the first page and the 2^31-1 row
     *     cap are exactly pg_plan_order_by's.  A finish that fails (SUM
     *     overflow) leaves an operator whose every later add_input and
     *     finish fail with the same error.
     *   - Keys: the n_partition_keys partition keys first, then the order
     *     keys; every key has a pg_sort_order, partition keys too.  Output
     *     rows are the input rows stably sorted by all n_keys keys: ties
     *     keep input order (page order, then row order).  This is STRICTER
     *     than the reference and makes ROWS frames and ROW_NUMBER
     *     deterministic.  With n_keys == 0 the input order is kept and
     *     everything is one partition.
     *   - Partitions and peers: two adjacent sorted rows are in the same
     *     partition when they compare equal on the first n_partition_keys
     *     keys under ORDER_BY's comparator, and are peers when they compare
     *     equal on all keys.  So null equals null, every NaN equals every
     *     NaN, and -0.0 DIFFERS from +0.0 — a deviation from the
     *     reference, whose partition and peer tests use the types'
     *     equalTo (under which the two zeros are equal).  With no order
     *     keys every row of a partition is a peer of every other.
     *   - Output: the n_emit emit columns first, then one column per
     *     function, in plan order.
     *   - ROW_NUMBER, RANK, DENSE_RANK: col, frame and offset are ignored.
     *     I64, no mask.
     *   - COUNT: col < 0 is count(*) over the frame; otherwise the
     *     non-null rows of col, which may be of any fixed-width type.  I64,
     *     no mask.
     *   - SUM: over a U8, I32 or I64 col, nulls skipped, I64 output.  It
     *     accumulates in 128 bits; finish fails with an error naming
     *     WINDOW, SUM and the function index if any EMITTED value does not
     *     fit int64.  For the two running frames that is exactly the
     *     reference's Math.addExact behaviour.  For PG_FRAME_PARTITION it
     *     is MORE LENIENT: the reference fails on an overflowing prefix
     *     even when the partition's total fits.
     *   - MIN / MAX: over a U8 (unsigned), I32 or I64 (signed) col, nulls
     *     skipped; the output has the input type.
     *   - Nulls of SUM, MIN, MAX: a frame with no non-null input gives
     *     null.  These columns always carry a device null_mask; the value
     *     under a null is 0.
     *   - LAG / LEAD: col may be of any fixed-width type, I128 included,
     *     and is copied bit for bit.  offset >= 0 counts rows in sorted
     *     order within the partition; offset 0 is the row itself; frame is
     *     ignored.  A target outside the partition gives null with value
     *     0; otherwise the result is the target's value and its null flag.
     *     These columns always carry a mask.
     *   - Frames (aggregates): RANGE_RUNNING ends at the row's last peer,
     *     ROWS_RUNNING at the row itself, PARTITION at the partition's
     *     last row; all start at the partition's first row.
     *   - Errors at create, naming the field: a count out of range,
     *     n_partition_keys > n_keys, an unknown func, frame (aggregates) or
     *     order, a negative offset (LAG / LEAD), a negative column where
     *     one is required (keys, emit columns, every function argument but
     *     COUNT's).  Errors at add_input, naming the function index and
     *     column (or the key / emit entry, as ORDER_BY): an index >= n_cols,
     *     a VARBIN or dictionary column anywhere, an I128 key, an I128 or
     *     F64 column under SUM / MIN / MAX, a type that differs from the
     *     first page's.  A rejected page leaves the operator as it was.
     *   - Out of scope: F64 SUM, MIN and MAX (a parallel scan cannot
     *     reproduce the reference's left-to-right rounding); bounded
     *     frames (k PRECEDING, FOLLOWING); ntile, percent_rank, cume_dist,
     *     first_value, last_value, nth_value; LAG / LEAD default values;
     *     variable-width columns; a per-partition limit (compose ROW_NUMBER
     *     with a downstream FILTER_PROJECT predicate instead); spilling. */
    int32_t n_keys;             /* 0..4: partition keys first, then order keys */
    int32_t n_partition_keys;   /* 0..n_keys */
    int32_t key_col[PG_MAX_SORT_KEYS];
    int32_t order[PG_MAX_SORT_KEYS];   /* pg_sort_order, for partition keys too */
    int32_t n_emit;             /* 1..16 */
    int32_t emit_cols[PG_MAX_SORT_EMIT];
    int32_t n_funcs;            /* 1..8 */
    pg_win_spec funcs[PG_MAX_WIN_FUNCS];
} pg_plan_window;

#define PG_DISTINCT_MARK 0 /* every row, plus a trailing marker column */
#define PG_DISTINCT_ONLY 1 /* the first rows only (DISTINCT / DistinctLimit) */

typedef struct {
    /* PG_OP_MARK_DISTINCT: for each row, whether it is the first row ever
     * fed to this operator with its combination of key values —
     * MarkDistinctOperator.java over MarkDistinctHash.java (a GroupByHash
     * on the distinct channels whose group id tells a new group from a
     * known one).  The marker leaves as a U8 column that downstream
     * aggregates use as their mask: count(DISTINCT x) ... GROUP BY g is
     * this operator over (g, x) followed by GROUPBY_MULTI over g with
     * COUNT FILTER (marker = 1), next to any other aggregate.  In
     * PG_DISTINCT_ONLY mode the operator emits the first rows themselves:
     * SELECT DISTINCT, and with a limit DistinctLimitOperator.java.
     *   - Keys: U8, I32, I64 or dictionary VARBIN channels; a dictionary
     *     key is its dictionary id, under GROUPBY_MULTI's rules (proper
     *     dictionary, the same one on every page).  Keys are always
     *     null-aware: a key is null at row i when its column has a
     *     null_mask and null_mask[i] != 0.  Null equals null per channel
     *     and differs from every value; channels are independent, so
     *     (null, 1), (0, 1), (null, null) and (0, null) are four
     *     combinations; the value stored under a null never matters.
     *     Equality is exact on the full key vector plus the per-channel
     *     null bits, never a fingerprint.
     *   - First occurrence: rows are totally ordered by page order, then
     *     row index (what ORDER_BY calls input order).  A row is first if
     *     and only if no earlier row of any page fed to this operator has
     *     the same combination — exactly, whatever order the GPU's threads
     *     reach the table in: of several equal rows in one page the lowest
     *     row index is first, and a combination first seen in one page is
     *     never first again in a later one.
     *   - PG_DISTINCT_MARK: every add_input queues exactly one page of the
     *     same n_rows: the emit_cols columns in that order, copied bit for
     *     bit, then one U8 marker column (1 = first, 0 = not) without a
     *     mask.  limit must be 0.
     *   - PG_DISTINCT_ONLY: the queued page holds only the first rows of
     *     the input page, in input order: the emit_cols columns, no
     *     marker.  limit > 0 is DistinctLimit: once `limit` rows have been
     *     emitted over all pages, the page that reaches the limit is cut
     *     to fit and the operator finishes itself — needs_input returns 0
     *     and a later add_input fails as after finish.  limit = 0 is
     *     unlimited.
     *   - Emit columns: fixed width (U8, I32, I64, F64, I128).  A key need
     *     not be emitted and a column may be emitted twice.  An emitted
     *     column whose input column has a null_mask carries it (copied in
     *     mark mode, compacted in only mode); otherwise its null_mask is
     *     NULL.  Output pages are device-resident, owned by the operator
     *     until the next pg_op_get_output / pg_op_destroy, and can be fed
     *     raw into another operator.  Input pages are borrowed and may be
     *     host- or device-resident, also mixed.  A 0-row input page gives
     *     a 0-row output page with the same columns.  finish queues
     *     nothing.
     *   - Capacity: capacity_hint >= 1 is the expected number of distinct
     *     combinations; the table is sized as GROUPBY_MULTI sizes its own
     *     (at most 2^31 slots).  When the table fills past the same 0.85
     *     rule, the add_input that notices fails with an error naming
     *     capacity_hint, and every later add_input and finish fails the
     *     same way; the page that failed has been partly inserted.
     *   - Errors at create, naming MARK_DISTINCT and the field: n_keys
     *     outside 1..4, n_emit outside 1..16, an unknown mode, a negative
     *     limit, a non-zero limit in mark mode, capacity_hint < 1, a
     *     negative column index.  Errors at add_input, naming the entry:
     *     an index >= n_cols; an F64, I128 or non-dictionary VARBIN key; a
     *     VARBIN or dictionary emit column; a key or emit type that
     *     differs from the first page's; more than 2^31-1 rows in one
     *     page.  A rejected page leaves the operator as it was.
     *   - Out of scope: F64, I128 and raw VARBIN keys; variable-width emit
     *     columns; spilling; one table shared between operators. */
    int64_t capacity_hint;             /* expected distinct combinations */
    int64_t limit;                     /* only mode: 0 = none */
    int32_t n_keys;                    /* 1..4 */
    int32_t key_col[4];
    int32_t mode;                      /* PG_DISTINCT_MARK / PG_DISTINCT_ONLY */
    int32_t n_emit;                    /* 1..16 */
    int32_t emit_cols[16];
} pg_plan_mark_distinct;

/* ---- operator lifecycle (Operator.java:20-102 analog) ---- */
typedef int64_t pg_op;

pg_status pg_op_create(int32_t kind, const void* plan, int64_t plan_bytes,
                       pg_op* out);
/* needsInput() */
int32_t pg_op_needs_input(pg_op op);
/* addInput(Page) — page borrowed for the call */
pg_status pg_op_add_input(pg_op op, const pg_page* page);
/* getOutput() — *out set to an internal page (device pointers) or NULL */
pg_status pg_op_get_output(pg_op op, const pg_page** out);
/* finish() */
pg_status pg_op_finish(pg_op op);
/* isFinished() */
int32_t pg_op_is_finished(pg_op op);
pg_status pg_op_destroy(pg_op op);

/* table handle of a finished HASH_BUILD op
 * (lendPartitionLookupSource analog, HashBuilderOperator.java:534) */
pg_status pg_op_table(pg_op op, int64_t* out_table);
/* per-partition row counts after a PARTITION op's get_output */
pg_status pg_op_partition_counts(pg_op op, int64_t* counts, int32_t n);

/* destroy a table explicitly (tables outlive their build op until freed) */
pg_status pg_table_destroy(int64_t table);
/* zero an agg table's accumulators so the table (keys + chains) can be
 * reused by another fused-agg probe — the analog of reusing a lookup
 * source across probe factories (HashBuilderOperator.java:534
 * lendPartitionLookupSource is multi-consumer).  The multi-agg accumulators
 * are zeroed too and keep their layout: the next multi-agg operator on the
 * table must still declare the layout of the first. */
pg_status pg_table_reset_acc(int64_t table);
/* bytes of the table's byte-tag array (one tag per slot), 0 when the table
 * carries none: hash tables below 2^26 slots, and non-partitioned
 * agg_table builds with a key bitmap, whose bitmap already is an exact
 * membership test (tests pin which tables carry tags) */
int64_t pg_table_tag_bytes(int64_t table);

/* ---- SerializedPage wire interop ----
 * Presto's exchange wire format, restated from
 * spi/page/PagesSerdeUtil.java:64-88 (metadata: positionCount i32, codec
 * marker u8, uncompressedSize i32, size i32, checksum i64, then the page
 * bytes; little-endian), checksum per computeSerializedPageChecksum:109-120
 * (CRC32 over data + marker + positionCount + uncompressedSize bytes);
 * raw page bytes per writeRawPage:45-51 (block count i32 then per block a
 * length-prefixed encoding name, BlockEncodingManager.java:96-99) with
 * encodings LONG_ARRAY / INT_ARRAY / BYTE_ARRAY
 * (common/block/LongArrayBlockEncoding.java:26-48 etc.; nulls-as-bits per
 * EncoderUtil.java:31-63; non-null values only).
 * v1 scope: uncompressed, unencrypted (codec marker 0); fixed-width
 * blocks (I64/F64 -> LONG_ARRAY, I32 -> INT_ARRAY, U8 -> BYTE_ARRAY).
 * Host-side (the node-boundary seam stays on the host). */
pg_status pg_page_serialize(const pg_page* page /* host cols */,
                            void* out, int64_t cap, int64_t* out_len);
/* round-2 wire scope: compress=1 runs the body through the LZ4 block
 * codec and sets PageCodecMarker.COMPRESSED when the ratio clears
 * PagesSerde.java:41's MINIMUM_COMPRESSION_RATIO (0.9); encodings now
 * cover LONG/INT/BYTE/INT128_ARRAY, VARIABLE_WIDTH, DICTIONARY
 * (varbin dictionaries travel as dictionaries, fixed-width ones expand
 * on read) and RLE (expanded on read). */
/* ABI drift guard: fills out[0..n) with sizeof each public struct in
 * the order {pg_col, pg_page, pg_pred, pg_proj, pg_agg,
 * pg_plan_filter_project, pg_plan_hash_agg_small, pg_plan_hash_build,
 * pg_plan_lookup_join, pg_plan_groupby, pg_plan_topn,
 * pg_plan_partition}; returns how many it would fill.  Bindings compare
 * against their own struct sizes at load time. */
int32_t pg_abi_struct_sizes(int32_t* out, int32_t n);
/* sizeof the plan struct of an operator kind (every pg_op_kind value,
 * pg_plan_order_by, pg_plan_window and pg_plan_mark_distinct included),
 * or -1 for an unknown kind (the unassigned 9 and 11 among them). */
int32_t pg_abi_plan_size(int32_t kind);
/* the order-preserving key transform of PG_OP_ORDER_BY (csrc/sortkey.h,
 * the code k_sort_encode runs on the device): the u64 whose unsigned
 * order is the pg_sort_order of a `tag` column value with bit pattern
 * `bits`.  Host-only, needs no GPU — test plumbing */
uint64_t pg_sortkey_u64(int32_t tag, int32_t order, uint64_t bits);

pg_status pg_page_serialize2(const pg_page* page, int32_t compress,
                             void* out, int64_t cap, int64_t* out_len);
/* parses and verifies; fills *out with malloc-backed host columns
 * (free with pg_page_free). F64 consumers reinterpret LONG_ARRAY bits. */
pg_status pg_page_deserialize(const void* buf, int64_t len, pg_page* out);
pg_status pg_page_free(pg_page* page);

#ifdef __cplusplus
}
#endif
#endif
