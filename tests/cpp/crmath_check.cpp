// Host check of crmath.h's correctly rounded powers x^1.5, x^-0.5, x^2.25, x^1.25 against
// __float128 powq, on the argument files tests/test_crmath.py writes (raw doubles).
//
//   crmath_check in  <op> <file>   arguments strictly inside the power's double-double range:
//       exact (cr_pow_*<true>) == (double)powq;  fast (cr_pow_*<false>) == the same, or tie raised.
//       Where powq itself lies within 2^-110 (relative) of a rounding midpoint its rounding proves
//       nothing: those arguments are printed as "hard <x> <exact> <fast> <tie>" (hex bit patterns)
//       and the caller decides them in exact rational arithmetic.
//   crmath_check out <op> <file>   arguments outside the range: the fast path raises tie, the exact
//       one is the library pow (within one ulp of powq).
// op: 0 x^1.5, 1 x^-0.5, 2 x^2.25, 3 x^1.25.  Prints "ok <n> ties <t> hard <h>" or the first failure.
#include <quadmath.h>

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

#include "../../mm-admm_amd/csrc/kernels/crmath.h"

static uint64_t bits(double d) {
  uint64_t b;
  std::memcpy(&b, &d, 8);
  return b;
}

static double run(int op, bool exact, double x, bool& tie) {
  switch (op) {
    case 0: return exact ? mmx::cr_pow_p15<true>(x, tie) : mmx::cr_pow_p15<false>(x, tie);
    case 1: return exact ? mmx::cr_pow_m05<true>(x, tie) : mmx::cr_pow_m05<false>(x, tie);
    case 2: return exact ? mmx::cr_pow_p225<true>(x, tie) : mmx::cr_pow_p225<false>(x, tie);
    default: return exact ? mmx::cr_pow_p125<true>(x, tie) : mmx::cr_pow_p125<false>(x, tie);
  }
}

int main(int argc, char** argv) {
  if (argc != 4) return 2;
  const bool inside = std::strcmp(argv[1], "in") == 0;
  const int op = std::atoi(argv[2]);
  static const double ys[4] = {1.5, -0.5, 2.25, 1.25};
  static const double lim[4][2] = {{1e-90, 1e90}, {1e-100, 1e100}, {1e-30, 1e30}, {1e-50, 1e50}};
  if (op < 0 || op > 3) return 2;
  std::vector<double> xs;
  {
    FILE* f = std::fopen(argv[3], "rb");
    if (!f) return 2;
    double v;
    while (std::fread(&v, 8, 1, f) == 1) xs.push_back(v);
    std::fclose(f);
  }
  long ties = 0, hard = 0;
  for (double x : xs) {
    const bool in = x > lim[op][0] && x < lim[op][1];
    if (in != inside) {
      std::printf("x=%a is %s the range of op %d\n", x, in ? "inside" : "outside", op);
      return 1;
    }
    const __float128 q = powq((__float128)x, (__float128)ys[op]);
    const double want = (double)q;
    bool tE = false, tF = false;
    const double ex = run(op, true, x, tE), fa = run(op, false, x, tF);
    if (tE) {
      std::printf("the exact path raised tie at x=%a\n", x);
      return 1;
    }
    if (!inside) {
      if (!tF) {
        std::printf("op %d: fast path did not defer out-of-range x=%a\n", op, x);
        return 1;
      }
      if (!(ex == want || ex == std::nextafter(want, 0.0) || ex == std::nextafter(want, INFINITY))) {
        std::printf("op %d: pow(%a) = %a is more than one ulp from powq %a\n", op, x, ex, want);
        return 1;
      }
      continue;
    }
    ties += tF;
    // the rounding midpoint nearest q, and q's relative distance from it
    const double nb = ((__float128)want < q) ? std::nextafter(want, INFINITY) : std::nextafter(want, 0.0);
    const __float128 mid = ((__float128)want + (__float128)nb) / 2;
    if ((__float128)want != q && fabsq(q - mid) <= q * (__float128)0x1p-110) {
      std::printf("hard %016llx %016llx %016llx %d\n", (unsigned long long)bits(x), (unsigned long long)bits(ex),
                  (unsigned long long)bits(fa), (int)tF);
      ++hard;
      continue;
    }
    if (bits(ex) != bits(want)) {
      std::printf("op %d: exact(%a) = %a, powq rounds to %a\n", op, x, ex, want);
      return 1;
    }
    if (!tF && bits(fa) != bits(want)) {
      std::printf("op %d: fast(%a) = %a without tie, powq rounds to %a\n", op, x, fa, want);
      return 1;
    }
  }
  std::printf("ok %zu ties %ld hard %ld\n", xs.size(), ties, hard);
  return 0;
}
