// sin, cos and asin of a double, correctly rounded in all but astronomically rare cases, out of IEEE add, multiply, fma, divide
// and sqrt alone: double-double arithmetic (a value as an unevaluated sum hi + lo, ~106 bits).  Host and device compile the same
// text and, those five operations being correctly rounded on both, return the same bits: the device need not trust its maths
// library's last bit to agree with a host library that rounds correctly.  Used by the haversine table of context.hip; a host
// program can include this file on its own.
#ifndef NGCF_DD_MATH_H
#define NGCF_DD_MATH_H

#include <cmath>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define NGCF_DD_HD __host__ __device__ inline
#else
#define NGCF_DD_HD inline
#endif

namespace ddm {

struct dd {
    double hi, lo;
};

// Error-free transforms.  Nothing in this file may be contracted or re-associated: the low words ARE the rounding errors.
NGCF_DD_HD dd two_sum(double a, double b)
{
#pragma clang fp contract(off) reassociate(off)
    const double s = a + b, bb = s - a;
    return {s, (a - (s - bb)) + (b - bb)};
}
NGCF_DD_HD dd quick_two_sum(double a, double b)             // |a| >= |b|
{
#pragma clang fp contract(off) reassociate(off)
    const double s = a + b;
    return {s, b - (s - a)};
}
NGCF_DD_HD dd two_prod(double a, double b)
{
#pragma clang fp contract(off) reassociate(off)
    const double p = a * b;
    return {p, fma(a, b, -p)};
}
NGCF_DD_HD dd add(dd a, dd b)
{
#pragma clang fp contract(off) reassociate(off)
    dd s = two_sum(a.hi, b.hi);
    const dd t = two_sum(a.lo, b.lo);
    s = quick_two_sum(s.hi, s.lo + t.hi);
    return quick_two_sum(s.hi, s.lo + t.lo);
}
NGCF_DD_HD dd add(dd a, double b)
{
#pragma clang fp contract(off) reassociate(off)
    const dd s = two_sum(a.hi, b);
    return quick_two_sum(s.hi, s.lo + a.lo);
}
NGCF_DD_HD dd mul(dd a, dd b)
{
#pragma clang fp contract(off) reassociate(off)
    const dd p = two_prod(a.hi, b.hi);
    return quick_two_sum(p.hi, p.lo + (a.hi * b.lo + a.lo * b.hi));
}

// 1/n! with alternating sign: the series of sin(r) / r - 1 = -r^2/3! + r^4/5! - ... and of cos(r) - 1 = -r^2/2! + r^4/4! - ...
// in powers of r^2, to r^27 and r^28: below 2^-100 of the result on |r| <= pi/4
#define NGCF_DD_SIN_TERMS 13
#define NGCF_DD_COS_TERMS 14
NGCF_DD_HD dd sin_coef(int i)
{
    constexpr dd c[NGCF_DD_SIN_TERMS] = {
        {-0x1.5555555555555p-3, -0x1.5555555555555p-57}, {0x1.1111111111111p-7, 0x1.1111111111111p-63},
        {-0x1.a01a01a01a01ap-13, -0x1.a01a01a01a01ap-73}, {0x1.71de3a556c734p-19, -0x1.c154f8ddc6c00p-73},
        {-0x1.ae64567f544e4p-26, 0x1.c062e06d1f209p-80}, {0x1.6124613a86d09p-33, 0x1.f28e0cc748ebep-87},
        {-0x1.ae7f3e733b81fp-41, -0x1.1d8656b0ee8cbp-97}, {0x1.952c77030ad4ap-49, 0x1.ac981465ddc6cp-103},
        {-0x1.2f49b46814157p-57, -0x1.2650f61dbdcb4p-112}, {0x1.71b8ef6dcf572p-66, -0x1.d043ae40c4647p-120},
        {-0x1.761b41316381ap-75, 0x1.3423c7d91404fp-130}, {0x1.3f3ccdd165fa9p-84, -0x1.58ddadf344487p-139},
        {-0x1.d1ab1c2dccea3p-94, -0x1.054d0c78aea14p-149}};
    return c[i];
}
NGCF_DD_HD dd cos_coef(int i)
{
    constexpr dd c[NGCF_DD_COS_TERMS] = {
        {-0x1.0000000000000p-1, 0.0}, {0x1.5555555555555p-5, 0x1.5555555555555p-59},
        {-0x1.6c16c16c16c17p-10, 0x1.f49f49f49f49fp-65}, {0x1.a01a01a01a01ap-16, 0x1.a01a01a01a01ap-76},
        {-0x1.27e4fb7789f5cp-22, -0x1.cbbc05b4fa99ap-76}, {0x1.1eed8eff8d898p-29, -0x1.2aec959e14c06p-83},
        {-0x1.93974a8c07c9dp-37, -0x1.05d6f8a2efd1fp-92}, {0x1.ae7f3e733b81fp-45, 0x1.1d8656b0ee8cbp-101},
        {-0x1.6827863b97d97p-53, -0x1.eec01221a8b0bp-107}, {0x1.e542ba4020225p-62, 0x1.ea72b4afe3c2fp-120},
        {-0x1.0ce396db7f853p-70, 0x1.aebcdbd20331cp-124}, {0x1.f2cf01972f578p-80, -0x1.9ada5fcc1ab14p-135},
        {-0x1.88e85fc6a4e5ap-89, 0x1.71c37ebd16540p-143}, {0x1.0a18a2635085dp-98, 0x1.b9e2e28e1aa54p-153}};
    return c[i];
}

// sin(r) and cos(r) of a double-double |r| <= pi/4 (a little more does no harm)
NGCF_DD_HD dd sin_kernel(dd r)
{
    const dd r2 = mul(r, r);
    dd p = sin_coef(NGCF_DD_SIN_TERMS - 1);
#pragma unroll
    for (int i = NGCF_DD_SIN_TERMS - 2; i >= 0; --i) p = add(mul(p, r2), sin_coef(i));
    return add(mul(mul(p, r2), r), r);                       // r + r * (r^2 * p)
}
NGCF_DD_HD dd cos_kernel(dd r)
{
    const dd r2 = mul(r, r);
    dd p = cos_coef(NGCF_DD_COS_TERMS - 1);
#pragma unroll
    for (int i = NGCF_DD_COS_TERMS - 2; i >= 0; --i) p = add(mul(p, r2), cos_coef(i));
    return add(mul(p, r2), 1.0);
}

constexpr double kReduceMax = 1.0e5;                          // |x| up to which k * kPio2A below is exact with room to spare

// x = k * pi/2 + r, |r| <= pi/4 (+ a rounding): pi/2 in three parts of 33 + 53 + 53 bits, so that k * A is exact and x - k * A is
// exact (Sterbenz); what is left of r when x lies as close to a multiple of pi/2 as a double can still has ~80 good bits
NGCF_DD_HD dd reduce(double x, int &quadrant)
{
#pragma clang fp contract(off) reassociate(off)
    constexpr double kTwoOverPi = 0x1.45f306dc9c883p-1;
    constexpr double kPio2A = 0x1.921fb54400000p+0, kPio2B = 0x1.0b4611a626331p-34, kPio2C = 0x1.1701b839a2520p-88;
    const double k = rint(x * kTwoOverPi);
    quadrant = (int)((long long)k & 3);
    const double t = fma(-k, kPio2A, x);
    const dd w = two_prod(k, kPio2B);
    dd r = two_sum(t, -w.hi);
    const dd tail = two_sum(r.lo, -w.lo);
    r = two_sum(r.hi, tail.hi);
    return two_sum(r.hi, r.lo + (tail.lo - k * kPio2C));
}

NGCF_DD_HD dd sin_dd(double x)                                // |x| <= kReduceMax
{
    int q;
    const dd r = reduce(x, q);
    const dd v = (q & 1) ? cos_kernel(r) : sin_kernel(r);
    return (q & 2) ? dd{-v.hi, -v.lo} : v;
}

// the three functions: a NaN, an infinity or an argument beyond the reduction's range goes to the maths library as it is
NGCF_DD_HD double sin_cr(double x)
{
    if (!(fabs(x) <= kReduceMax)) return sin(x);
    if (x == 0.0) return x;
    return sin_dd(x).hi;
}
NGCF_DD_HD double cos_cr(double x)
{
    if (!(fabs(x) <= kReduceMax)) return cos(x);
    int q;
    const dd r = reduce(x, q);
    const dd v = (q & 1) ? sin_kernel(r) : cos_kernel(r);
    return ((q + 1) & 2) ? -v.hi : v.hi;
}
// asin(z), 0 <= z <= 1 (the formula's sqrt(d)): one Newton step on the library's value y0, whose error e leaves e^2 tan(y0) / 2 -
// below 2^-80 even one ulp under z = 1: y = y0 + (z - sin(y0)) / cos(y0), the difference taken in double-double
NGCF_DD_HD double asin_cr(double z)
{
#pragma clang fp contract(off) reassociate(off)
    if (!(z > 0.0 && z <= 1.0)) return asin(z);              // 0, a NaN, out of range: the library's answer
    const double y0 = asin(z);
    const dd s = sin_dd(y0);
    const dd diff = add(dd{-s.hi, -s.lo}, z);
    return y0 + diff.hi / cos(y0);
}

}  // namespace ddm

#endif  // NGCF_DD_MATH_H
