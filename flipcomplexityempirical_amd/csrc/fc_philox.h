// Counter-based random stream shared by the host (initial-state wait) and the kernels.
//
// Draw d of chain c: Philox4x32-10(ctr = (lo32 d, hi32 d, c, purpose), key = seed).
// purpose 0: the proposal words; 1: the geometric wait of the state created by draw d;
// 2 (d = 0): the geometric wait of the initial state.  DESIGN.md "Random stream".
#pragma once
#include <stdint.h>

#include <cmath>

#include "fc_lds.h"  // FC_HD

namespace fc {

struct Words4 {
    uint32_t x0, x1, x2, x3;
};

FC_HD Words4 philox4x32_10(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, uint32_t k0, uint32_t k1) {
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        if (r) {
            k0 += 0x9E3779B9u;
            k1 += 0xBB67AE85u;
#if defined(__HIP_DEVICE_COMPILE__)
            // keep the key schedule two scalar adds per round: hoisted out of the kernels'
            // loops, its 20 round keys were held in SGPRs, spilled to VGPR lanes and reloaded
            // (v_readlane + hazard nop) in every round
            asm volatile("" : "+s"(k0), "+s"(k1));
#endif
        }
        // one v_mad_u64_u32 per product gives both halves
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
#if defined(__HIP_DEVICE_COMPILE__)
        const uint32_t n0 = __builtin_amdgcn_bitop3_b32((uint32_t)(p1 >> 32), c1, k0, 0x96);  // 3-way xor
        const uint32_t n2 = __builtin_amdgcn_bitop3_b32((uint32_t)(p0 >> 32), c3, k1, 0x96);
#else
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ k0, n2 = (uint32_t)(p0 >> 32) ^ c3 ^ k1;
#endif
        c0 = n0;
        c1 = (uint32_t)p1;
        c2 = n2;
        c3 = (uint32_t)p0;
    }
    return Words4{c0, c1, c2, c3};
}

// The k = 2 flip kernel's form: the ten rounds' key words (kPhiloxKeyWords: k0, k1 of round 0,
// of round 1, ...) come from memory, filled once per run by the host (philox_round_keys), and are
// read by scalar loads where the words are needed, instead of two scalar adds per round in every
// call.  The same function of (counter, seed) as philox4x32_10.
constexpr int kPhiloxKeyWords = 20;
inline void philox_round_keys(uint32_t k0, uint32_t k1, uint32_t *out) {
    for (int r = 0; r < 10; ++r) {
        out[2 * r] = k0 + (uint32_t)r * 0x9E3779B9u;
        out[2 * r + 1] = k1 + (uint32_t)r * 0xBB67AE85u;
    }
}
#if defined(__HIPCC__) || defined(__HIP__)
typedef const uint32_t __attribute__((address_space(4))) *PhiloxKeys;  // constant memory: scalar loads
#endif
// KP: PhiloxKeys in the kernel; a plain pointer on the host (tests/native/philox_keys_check.cpp)
template <typename KP>
FC_HD Words4 philox4x32_10_keys(uint32_t c0, uint32_t c1, uint32_t c2, uint32_t c3, KP kp) {
    uint32_t K[kPhiloxKeyWords];
#pragma unroll
    for (int i = 0; i < kPhiloxKeyWords; ++i) K[i] = kp[i];
#pragma unroll
    for (int r = 0; r < 10; ++r) {
        const uint64_t p0 = (uint64_t)0xD2511F53u * c0, p1 = (uint64_t)0xCD9E8D57u * c2;
#if defined(__HIP_DEVICE_COMPILE__)
        const uint32_t n0 = __builtin_amdgcn_bitop3_b32((uint32_t)(p1 >> 32), c1, K[2 * r], 0x96);  // 3-way xor
        const uint32_t n2 = __builtin_amdgcn_bitop3_b32((uint32_t)(p0 >> 32), c3, K[2 * r + 1], 0x96);
#else
        const uint32_t n0 = (uint32_t)(p1 >> 32) ^ c1 ^ K[2 * r], n2 = (uint32_t)(p0 >> 32) ^ c3 ^ K[2 * r + 1];
#endif
        c0 = n0;
        c1 = (uint32_t)p1;
        c2 = n2;
        c3 = (uint32_t)p0;
    }
    return Words4{c0, c1, c2, c3};
}

// 53-bit mantissa of CPython random() / numpy random_sample() from two words.
FC_HD uint64_t mant53(uint32_t a, uint32_t b) { return ((uint64_t)(a >> 5) << 26) | (uint64_t)(b >> 6); }

FC_HD double u53(uint32_t a, uint32_t b) { return (double)mant53(a, b) * (1.0 / 9007199254740992.0); }

// geom_wait (grid_chain_sec11.py:147-148) by numpy's legacy inversion, ceil(log(1-U)/log(1-p)) - 1,
// saturated at 2^62 where log(1-p) rounds to 0 (|B| / (N^k - 1) below 2^-53, e.g. k >= 5 on 10^4
// nodes) -- the reference's float pipeline has no defined value there.
constexpr double kWaitCap = 4611686018427387904.0;  // 2^62

// log(x), correctly rounded, for 0 < x <= 1 (x normal): the value a host libm's log returns in all
// but its own rare misroundings (glibc: error below 0.52 ulp).  x = m 2^e with m in [sqrt 1/2,
// sqrt 2); log m = 2 atanh s, s = (m - 1) / (m + 1), as 2 s (1 + w Q(w)), w = s^2 <= 0.0295,
// Q(w) = 1/3 + w/5 + ... + w^12/27; s, w, the first four terms and every sum in double-double
// (error-free sums and fma products), the rest of Q in double.  Truncation (w^14 / 29) and the
// double tail (w^5 2^-53) are below 2^-74 of the result, so the rounding is wrong only for a
// value within 2^-21 ulp of a tie.
FC_HD void dd_two_sum(double a, double b, double &s, double &e) {
    s = a + b;
    const double bb = s - a;
    e = (a - (s - bb)) + (b - bb);
}
// (ah + al) (bh + bl)
FC_HD void dd_mul(double ah, double al, double bh, double bl, double &ph, double &pl) {
    const double p = ah * bh;
    const double e = fma(ah, bh, -p) + (ah * bl + al * bh);
    dd_two_sum(p, e, ph, pl);
}
// (ah + al) + (bh + bl)
FC_HD void dd_add(double ah, double al, double bh, double bl, double &sh, double &sl) {
    double s, e;
    dd_two_sum(ah, bh, s, e);
    e += al + bl;
    dd_two_sum(s, e, sh, sl);
}
FC_HD double log_cr(double x) {
    int e;
    double m = frexp(x, &e);  // [1/2, 1)
    if (m < 0x1.6a09e667f3bcdp-1) {
        m *= 2.0;
        e -= 1;
    }
    // s = (m - 1) / (m + 1): m - 1 is exact, m + 1 as a sum with its error, one division step
    const double num = m - 1.0;
    double dh, dl, sh, sl, wh, wl, qh, ql;
    dd_two_sum(m, 1.0, dh, dl);
    sh = num / dh;
    {
        const double p = sh * dh;
        const double r = ((num - p) - fma(sh, dh, -p)) - sh * dl;  // num - sh (dh + dl)
        sl = r / dh;
    }
    dd_mul(sh, sl, sh, sl, wh, wl);
    // Q's tail 1/11 + w/13 + ... + w^8/27 in double, its head in double-double
    double t = 0x1.2f684bda12f68p-5;
    t = fma(t, wh, 0x1.47ae147ae147bp-5);
    t = fma(t, wh, 0x1.642c8590b2164p-5);
    t = fma(t, wh, 0x1.8618618618618p-5);
    t = fma(t, wh, 0x1.af286bca1af28p-5);
    t = fma(t, wh, 0x1.e1e1e1e1e1e1ep-5);
    t = fma(t, wh, 0x1.1111111111111p-4);
    t = fma(t, wh, 0x1.3b13b13b13b14p-4);
    t = fma(t, wh, 0x1.745d1745d1746p-4);
    dd_mul(wh, wl, t, 0.0, qh, ql);
    dd_add(qh, ql, 0x1.c71c71c71c71cp-4, 0x1.c71c71c71c71cp-58, qh, ql);   // + 1/9
    dd_mul(wh, wl, qh, ql, qh, ql);
    dd_add(qh, ql, 0x1.2492492492492p-3, 0x1.2492492492492p-57, qh, ql);   // + 1/7
    dd_mul(wh, wl, qh, ql, qh, ql);
    dd_add(qh, ql, 0x1.999999999999ap-3, -0x1.999999999999ap-57, qh, ql);  // + 1/5
    dd_mul(wh, wl, qh, ql, qh, ql);
    dd_add(qh, ql, 0x1.5555555555555p-2, 0x1.5555555555555p-56, qh, ql);   // + 1/3
    dd_mul(wh, wl, qh, ql, qh, ql);  // w Q
    dd_mul(sh, sl, qh, ql, qh, ql);  // s w Q
    dd_add(sh, sl, qh, ql, qh, ql);  // s (1 + w Q)
    // + e log 2 (the high part has 42 bits: e times it is exact)
    const double ed = (double)e;
    dd_add(ed * 0x1.62e42fefa38p-1, ed * 0x1.ef35793c7673p-45, 2.0 * qh, 2.0 * ql, qh, ql);
    return qh;
}

FC_HD int64_t geom_from(double U, double log1mp) {
    double q = log(1.0 - U) / log1mp;
    if (!(fabs(q) < kWaitCap)) return (int64_t)kWaitCap;
#if defined(__HIP_DEVICE_COMPILE__)
    // The device's log is within an ulp, and the quotient's ceiling must be the host's (the
    // oracle's, numpy's): where q lies within that error of an integer -- its distance below
    // 2^-50 |q|: about one wait in 10^4 at q = 10^12 (64 nodes, k = 8), practically none below
    // 10^8 -- the logarithm is taken again, correctly rounded.
    if (fabs(q - rint(q)) <= fabs(q) * 0x1p-50) q = log_cr(1.0 - U) / log1mp;
#endif
    return (int64_t)ceil(q) - 1;
}

}  // namespace fc
