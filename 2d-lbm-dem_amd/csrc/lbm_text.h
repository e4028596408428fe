// lbm_text.h -- decimal text on the host and on the device: the bytes of printf("%.4lf", v), for every finite |v| < 1e9.
//
// glibc prints the EXACT binary value rounded to nearest, ties to even. The same from double arithmetic alone:
//   a = |v|, t = a * 1e4 (rounded), e = fma(a, 1e4, -t): the exact error of that product, so a * 1e4 == t + e exactly;
//   n = rint(t), d = t - n: exact (t < 2^44, so t and n share a grid that holds their difference).
//   |d| != 0.5: t is at least one ulp of t away from the tie, which is more than |e|: n is the nearest integer of t + e too.
//   |d| == 0.5: e decides -- above the tie floor(t) + 1, below it floor(t), on it (e == 0) the even one of the two.
// The fma is written out; the library is compiled -ffp-contract=off and without fast-math, so neither it nor t - n is
// re-associated. The sign is the sign bit's: -0.0 and negatives that round to zero print "-0.0000", as printf does.
#pragma once

#include <hip/hip_runtime.h>
#include <math.h>

// what fixed4_len / fixed4_put accept (everything else is printed by the host's printf)
__host__ __device__ inline bool fixed4_ok(double v) { return fabs(v) < 1e9; }   // (false for NaN and the infinities)

// |v| * 1e4 correctly rounded to an integer: at most 10^13
__host__ __device__ inline unsigned long long fixed4_scaled(double v) {
  const double a = fabs(v);
  const double t = a * 1e4;
  const double e = fma(a, 1e4, -t);
  double n = rint(t);
  const double d = t - n;
  if (fabs(d) == 0.5) {
    const double lo = floor(t);
    if (e > 0) n = lo + 1;
    else if (e < 0) n = lo;
    else n = ((unsigned long long)lo & 1ull) ? lo + 1 : lo;
  }
  return (unsigned long long)n;
}

__host__ __device__ inline int fixed4_digits(unsigned ip) {   // decimal digits of the integer part (<= 10^9)
  int nd = 1;
  while (ip >= 10u) { ip /= 10u; ++nd; }
  return nd;
}

// bytes of "%.4lf" of v
__host__ __device__ inline int fixed4_len(double v) {
  const unsigned long long N = fixed4_scaled(v);
  return (signbit(v) ? 1 : 0) + fixed4_digits((unsigned)(N / 10000ull)) + 5;
}

// writes them at p (no terminator) and returns their number
__host__ __device__ inline int fixed4_put(double v, char* p) {
  const unsigned long long N = fixed4_scaled(v);
  unsigned ip = (unsigned)(N / 10000ull), fr = (unsigned)(N % 10000ull);
  int at = 0;
  if (signbit(v)) p[at++] = '-';
  const int nd = fixed4_digits(ip);
  for (int k = nd - 1; k >= 0; --k) { p[at + k] = (char)('0' + ip % 10u); ip /= 10u; }
  at += nd;
  p[at++] = '.';
  for (int k = 3; k >= 0; --k) { p[at + k] = (char)('0' + fr % 10u); fr /= 10u; }
  return at + 4;
}
