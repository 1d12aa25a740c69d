/* sortkey.h — the order-preserving key transform of PG_OP_ORDER_BY.
 *
 * One function maps a column value to a u64 whose UNSIGNED order is the
 * order the plan asks for, so the radix sort of kernels.hip never looks at
 * types again.  k_sort_encode runs it on the device and the test hook
 * pg_sortkey_u64 runs the very same code on the host.  Compiles as both
 * host C/C++ and HIP device code.
 *
 * Semantics restated from the reference (SortOrder.java, and the types'
 * compareTo: BigintType/IntegerType signed compare, DoubleType.compareTo =
 * Double.compare):
 *   U8   unsigned;
 *   I32  signed, encoded into the low 32 bits (the high 32 stay equal
 *        across rows, so their radix passes are skipped);
 *   I64  signed;
 *   F64  -inf < ... < -0.0 < +0.0 < ... < +inf < NaN, and every NaN — any
 *        sign, any payload — is the same key.
 * DESC complements the key within the type's width.  Null placement is
 * not encoded here: the sort gives it a pass of its own. */
#ifndef PRESTO_AMD_SORTKEY_H
#define PRESTO_AMD_SORTKEY_H
#include <stdint.h>

#ifdef __HIPCC__
#define PG_SK_HD __host__ __device__
#else
#define PG_SK_HD
#endif

/* tag: pg_type (U8=0, I32=1, I64=2, F64=3); order: pg_sort_order (2 and 3
 * are DESC); bits: the value's bit pattern in the low bytes.  Any other
 * tag maps to 0. */
static inline PG_SK_HD uint64_t pg_sortkey(int32_t tag, int32_t order,
                                           uint64_t bits)
{
    uint64_t k, width;
    switch (tag) {
        case 0: /* U8 */
            width = 0xffull;
            k = bits & width;
            break;
        case 1: /* I32: flip the sign bit */
            width = 0xffffffffull;
            k = (bits & width) ^ 0x80000000ull;
            break;
        case 2: /* I64 */
            width = ~0ull;
            k = bits ^ 0x8000000000000000ull;
            break;
        case 3: /* F64 */
            width = ~0ull;
            if ((bits & 0x7fffffffffffffffull) > 0x7ff0000000000000ull)
                bits = 0x7ff8000000000000ull; /* one NaN, above +inf */
            k = (bits >> 63) ? ~bits : bits ^ 0x8000000000000000ull;
            break;
        default: return 0;
    }
    return order >= 2 ? ~k & width : k;
}

#endif
