// exp10_scaled.h -- 10^x 2^-k in f64 for any finite |x| < 2^40 and any integer k, the staging
// arithmetic of cv_posterior_emissions* (emis_prepare_lin_f64, emis.hip).
//
// One source for the host and the device build: only +, -, *, explicit fma, rint, integer
// and bit operations -- no pow / exp / exp2 / ldexp of a math library -- so both builds give the
// same bits (every fused operation is spelled fma; build with -ffp-contract=off) and the
// host build can be measured against multi-precision arithmetic (tests/
// test_posterior_emissions.py: that measurement is the proof of the bound below).
//
//   y  = x log2(10) as a double-double (yh, yl): yh = fl(x Lh), yl = fma(x, Ll, fma(x, Lh, -yh));
//        |y - yh - yl| <= 2^-104 |y| + ... < 2^-62 for |x| < 2^40
//   n  = rint(yh), rh = yh - n exactly (|rh| <= 1/2), (r, re) = TwoSum(rh, yl)
//   t  = r ln2 as a double-double (th, tl); w = tl + re ln2  (the first order of the parts of
//        the exponent that th does not hold: |tl|, |re ln2| < 2^-54, so the second order is
//        below 2^-108)
//   m  = e^t = 1 + th + (w + th^2 Q(th)),  Q = the Taylor tail 1/2 + t/6 + ... + t^12/14!
//        (|th| <= 0.3467: the remainder is below 2^-63), summed as Fast2Sum(1, th) + tail, so
//        the final addition is the only rounding of the order of the result
//   10^x 2^-k = m 2^(n-k), m in [0.7071, 1.4143]; the scaling is exact while the result is
//        normal and rounds once when it is subnormal.
//
// Error, relative to m in u = 2^-53: the final addition at most 1 (1/2 ulp(m) = 2^-53 for m in
// [1, 2), 2^-54 / 0.7071 below 1); the inner addition lo + tail (|.| <= 0.08) at most 2^-57 /
// 0.7071 < 0.1; the tail itself (th^2 q: three roundings of a value <= 0.07) at most 0.3; the
// double-double steps and the truncated series below 0.01.  Sum < 1.5.  Bound stated and tested:
//   |exp10_scaled(x, k) - 10^x 2^-k| <= kExp10ScaledC u |10^x 2^-k|,  u = 2^-53,
// for every normal result (a relative bound in u is at least as strong as the same count of
// ulp).  The largest error measured against 60-digit arithmetic is recorded in DESIGN.md.
#pragma once
#include <stdint.h>

#if defined(__HIPCC__) || defined(__CUDACC__)
#define CV_HD __host__ __device__
#else
#define CV_HD
#endif

namespace cvx {

constexpr double kExp10ScaledC = 2.0;  // the bound c, in u = 2^-53 relative

struct Exp10Parts {
  double m;   // in [0.7071, 1.4143]; 0 for x = -inf
  int64_t n;  // 10^x = m 2^n
};

CV_HD inline double bits_f64(uint64_t u) { return __builtin_bit_cast(double, u); }
// 2^e for -1022 <= e <= 1023
CV_HD inline double pow2_f64(int e) { return bits_f64((uint64_t)(e + 1023) << 52); }

// x finite with |x| < 2^40, or -inf (any sign of zero reads as zero)
CV_HD inline Exp10Parts exp10_parts(double x) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  constexpr double kNegInf = -__builtin_inf();
  if (x == kNegInf) return {0.0, 0};
  // log2(10) = Lh + Ll, ln 2 = Gh + Gl (the two leading doubles of each constant)
  constexpr double Lh = 0x1.a934f0979a371p+1, Ll = 0x1.7f2495fb7fa6dp-53;
  constexpr double Gh = 0x1.62e42fefa39efp-1, Gl = 0x1.abc9e3b39803fp-56;
  const double yh = x * Lh;
  const double yl = __builtin_fma(x, Ll, __builtin_fma(x, Lh, -yh));
  const double nf = __builtin_rint(yh);
  const double rh = yh - nf;  // exact
  const double r = rh + yl;   // TwoSum
  const double bb = r - rh;
  const double re = (rh - (r - bb)) + (yl - bb);
  const double th = r * Gh;
  const double tl = __builtin_fma(r, Gl, __builtin_fma(r, Gh, -th));
  const double w = __builtin_fma(re, Gh, tl);
  // Q(t) = sum_{i=2}^{14} t^(i-2) / i!
  double q = 0x1.93974a8c07c9dp-37;            // 1/14!
  q = __builtin_fma(q, th, 0x1.6124613a86d09p-33);  // 1/13!
  q = __builtin_fma(q, th, 0x1.1eed8eff8d898p-29);  // 1/12!
  q = __builtin_fma(q, th, 0x1.ae64567f544e4p-26);  // 1/11!
  q = __builtin_fma(q, th, 0x1.27e4fb7789f5cp-22);  // 1/10!
  q = __builtin_fma(q, th, 0x1.71de3a556c734p-19);  // 1/9!
  q = __builtin_fma(q, th, 0x1.a01a01a01a01ap-16);  // 1/8!
  q = __builtin_fma(q, th, 0x1.a01a01a01a01ap-13);  // 1/7!
  q = __builtin_fma(q, th, 0x1.6c16c16c16c17p-10);  // 1/6!
  q = __builtin_fma(q, th, 0x1.1111111111111p-7);   // 1/5!
  q = __builtin_fma(q, th, 0x1.5555555555555p-5);   // 1/4!
  q = __builtin_fma(q, th, 0x1.5555555555555p-3);   // 1/3!
  q = __builtin_fma(q, th, 0.5);
  const double tail = __builtin_fma(th * th, q, w);
  const double hi = 1.0 + th;  // Fast2Sum: 1 >= |th|
  const double lo = th - (hi - 1.0);
  return {hi + (lo + tail), (int64_t)nf};
}

// m 2^e: exact for a normal result, one rounding into the subnormal range, 0 below it
CV_HD inline double scale_pow2(double m, int64_t e) {
#ifdef __clang__
#pragma clang fp contract(off)
#endif
  if (e >= -1000) return m * pow2_f64(e > 1023 ? 1023 : (int)e);
  if (e < -1200) e = -1200;
  return (m * pow2_f64(-1000)) * pow2_f64((int)e + 1000);
}

// the scale of a row whose largest score is xmax: the k with 10^xmax 2^-k (as computed) in [1, 2)
// (0 for a row that is all -inf)
CV_HD inline int64_t exp10_row_shift(const Exp10Parts& pmax) {
  return pmax.m == 0.0 ? 0 : pmax.m < 1.0 ? pmax.n - 1 : pmax.n;
}

CV_HD inline double exp10_scaled(double x, int64_t k) {
  const Exp10Parts p = exp10_parts(x);
  return scale_pow2(p.m, p.n - k);
}

}  // namespace cvx
