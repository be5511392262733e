// The decimal text of one fp32 value as "%.6f" prints it (include/emogest.h, "BVH text of whole takes"): one routine for the kernels of
// bvhtext.hip and for the host-only export eg_bvh_text_decimal, so that what a CPU test pins is the arithmetic the device runs.  Internal.
//   q = (double)|v| * 1e6 is exact (1e6 = 2^6 * 15625: at most 24 + 14 significant bits) and below 2^53 for |v| < 2^31;
//   N = rint(q), ties to even;  text = '-' iff signbit(v), the digits of N / 10^6, '.', the six digits of N % 10^6.
// Integer division by constants only; no printf, no library conversion.
#pragma once
#include <math.h>
#include <stdint.h>

#if defined(__HIPCC__)
#define EGI_HD __host__ __device__ __forceinline__
#else
#define EGI_HD inline
#endif

struct EgiDecimal {
    uint32_t ip, fp;            // N / 10^6 (< 2^31), N % 10^6
    int digits, width;          // decimal digits of ip (1..10); bytes of the text, sign included (8..18)
    bool neg, ok;               // ok: finite and |v| < 2^31; a value that is not is laid out as +0 ("0.000000")
};

EGI_HD int egi_digits10(uint32_t x) {
    return x < 10u ? 1 : x < 100u ? 2 : x < 1000u ? 3 : x < 10000u ? 4 : x < 100000u ? 5 : x < 1000000u ? 6 : x < 10000000u ? 7
         : x < 100000000u ? 8 : x < 1000000000u ? 9 : 10;
}

EGI_HD EgiDecimal egi_decimal6(float v) {
    EgiDecimal d;
    uint32_t bits;
    __builtin_memcpy(&bits, &v, 4);
    const float a = fabsf(v);
    d.ok = a < 2147483648.f;                                   // false for NaN and inf
    d.neg = d.ok && (bits >> 31) != 0;
    d.ip = d.fp = 0;
    if (d.ok) {
        const uint64_t n = (uint64_t)rint((double)a * 1e6);
        const uint64_t ip = n / 1000000ull;
        d.ip = (uint32_t)ip;
        d.fp = (uint32_t)(n - ip * 1000000ull);
    }
    d.digits = egi_digits10(d.ip);
    d.width = (d.neg ? 1 : 0) + d.digits + 7;
    return d;
}

// The d.width bytes of the text through put(i, byte), i = 0 .. width - 1.
template <class Put>
EGI_HD void egi_decimal6_put(const EgiDecimal& d, Put put) {
    int p = 0;
    if (d.neg) put(p++, (unsigned char)'-');
    uint32_t x = d.ip;
    for (int i = d.digits - 1; i >= 0; --i) {
        const uint32_t q = x / 10u;
        put(p + i, (unsigned char)('0' + (x - q * 10u)));
        x = q;
    }
    p += d.digits;
    put(p++, (unsigned char)'.');
    x = d.fp;
#pragma unroll
    for (int i = 5; i >= 0; --i) {
        const uint32_t q = x / 10u;
        put(p + i, (unsigned char)('0' + (x - q * 10u)));
        x = q;
    }
}
