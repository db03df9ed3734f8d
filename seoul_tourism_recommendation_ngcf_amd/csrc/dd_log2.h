// log2 of a positive double, correctly rounded in all but astronomically rare cases, in the double-double arithmetic of dd_math.h
// (IEEE add, multiply, fma and divide alone: host and device compile the same text and return the same bits).  The maths
// library's log2 is good to an ulp, and which ulp differs between libraries - the device's and glibc's disagree at 129 of the
// integers 2..100001, the first of them 3 -, so a sum of 1/log2(rank + 2) terms taken on the device can only be compared with a
// host oracle to the bit if neither side trusts its library's last bit.  Used by the metrics of rank_position.hip; a host program can
// include this file on its own.
#ifndef NGCF_DD_LOG2_H
#define NGCF_DD_LOG2_H

#include "dd_math.h"

namespace ddm {

NGCF_DD_HD dd div(dd a, dd b)                                 // two quotient digits and a third for the rounding
{
#pragma clang fp contract(off) reassociate(off)
    const double q1 = a.hi / b.hi;
    dd r = add(a, mul(b, dd{-q1, 0.0}));
    const double q2 = r.hi / b.hi;
    r = add(r, mul(b, dd{-q2, 0.0}));
    const double q3 = r.hi / b.hi;
    return add(quick_two_sum(q1, q2), q3);
}

// 1/(2k + 1): atanh(s) = s * sum_k s^(2k) / (2k + 1).  |s| <= (sqrt(2) - 1)/(sqrt(2) + 1) = 0.1716, s^2 <= 0.0295: the first term
// left out, s^46 / 47, is below 2^-122
#define NGCF_DD_ATANH_TERMS 23
NGCF_DD_HD dd atanh_coef(int i)
{
    constexpr dd c[NGCF_DD_ATANH_TERMS] = {
        {0x1.0000000000000p+0, 0.0}, {0x1.5555555555555p-2, 0x1.5555555555555p-56}, {0x1.999999999999ap-3, -0x1.999999999999ap-57},
        {0x1.2492492492492p-3, 0x1.2492492492492p-57}, {0x1.c71c71c71c71cp-4, 0x1.c71c71c71c71cp-58},
        {0x1.745d1745d1746p-4, -0x1.745d1745d1746p-59}, {0x1.3b13b13b13b14p-4, -0x1.3b13b13b13b14p-58},
        {0x1.1111111111111p-4, 0x1.1111111111111p-60}, {0x1.e1e1e1e1e1e1ep-5, 0x1.e1e1e1e1e1e1ep-61},
        {0x1.af286bca1af28p-5, 0x1.af286bca1af28p-59}, {0x1.8618618618618p-5, 0x1.8618618618618p-59},
        {0x1.642c8590b2164p-5, 0x1.642c8590b2164p-60}, {0x1.47ae147ae147bp-5, -0x1.eb851eb851eb8p-61},
        {0x1.2f684bda12f68p-5, 0x1.2f684bda12f68p-59}, {0x1.1a7b9611a7b96p-5, 0x1.1a7b9611a7b96p-61},
        {0x1.0842108421084p-5, 0x1.0842108421084p-60}, {0x1.f07c1f07c1f08p-6, -0x1.f07c1f07c1f08p-61},
        {0x1.d41d41d41d41dp-6, 0x1.0750750750750p-60}, {0x1.bacf914c1bad0p-6, -0x1.bacf914c1bad0p-60},
        {0x1.a41a41a41a41ap-6, 0x1.0690690690690p-60}, {0x1.8f9c18f9c18fap-6, -0x1.f3831f3831f38p-61},
        {0x1.7d05f417d05f4p-6, 0x1.7d05f417d05f4p-62}, {0x1.6c16c16c16c17p-6, -0x1.f49f49f49f49fp-61}};
    return c[i];
}

// x = m * 2^e with m in [1/sqrt(2), sqrt(2)); log2(x) = e + (2 / ln 2) * atanh((m - 1)/(m + 1)).  m - 1 is exact, an exact power of
// two gives s = 0 and the integer e.  Zero, a negative, an infinity, a NaN or a subnormal goes to the maths library as it is.
NGCF_DD_HD double log2_cr(double x)
{
#pragma clang fp contract(off) reassociate(off)
    if (!(x >= 0x1.0p-1022 && x <= 0x1.fffffffffffffp+1023)) return log2(x);
    int e;
    double m = frexp(x, &e);                                  // [0.5, 1)
    if (m < 0x1.6a09e667f3bcdp-1) {
        m *= 2.0;
        e -= 1;
    }
    const dd s = div(dd{m - 1.0, 0.0}, two_sum(m, 1.0));
    const dd s2 = mul(s, s);
    dd p = atanh_coef(NGCF_DD_ATANH_TERMS - 1);
#pragma unroll
    for (int i = NGCF_DD_ATANH_TERMS - 2; i >= 0; --i) p = add(mul(p, s2), atanh_coef(i));
    constexpr dd kTwoOverLn2 = {0x1.71547652b82fep+1, 0x1.777d0ffda0d24p-55};
    const dd l = mul(mul(s, p), kTwoOverLn2);
    return add(l, (double)e).hi;
}

}  // namespace ddm

#endif  // NGCF_DD_LOG2_H
