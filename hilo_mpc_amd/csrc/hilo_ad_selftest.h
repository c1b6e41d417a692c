// Developer aid: every operation of hilo_ad.h at one point in each scalar type (double, FastD, Dual<1>, Dual<12>, Jet2).
//
// The body is __host__ __device__ like the header it exercises: hilo_selftest.hip runs it in a kernel (hilo_ad_selftest), a
// stand-alone host program built with --cuda-host-only runs the same statements on the CPU (tests/test_ad_ops_host.py).
//
// One point: op (AD_*), operands a, b, tangents da, db and second Taylor coefficients dda, ddb.
//   Dual<1>   a.d[0] = da,             b.d[0] = db
//   Dual<12>  a.d[k] = ad_seed(k) da,  b.d[k] = ad_seed(k) db      (powers of two and 0: component k is ad_seed(k) times Dual<1>'s, exactly)
//   Jet2      (a, da, dda), (b, db, ddb)
// out[AD_OUT = 20]: [0] double, [1] FastD, [2..3] Dual<1> v d, [4..16] Dual<12> v d[12], [17..19] Jet2 v a b.
#pragma once
#include "hilo_ad.h"

namespace hilo {

enum AdOp : int {
  // unary, of a
  AD_NEG = 0, AD_SQ, AD_SIN, AD_COS, AD_EXP, AD_LOG, AD_SQRT, AD_LOG10, AD_FABS, AD_SIGN, AD_ASIN, AD_ACOS, AD_ATAN, AD_ASINH,
  AD_ACOSH, AD_ATANH, AD_TANH, AD_SECH2,
  // T op T
  AD_ADD = 18, AD_SUB, AD_MUL, AD_DIV, AD_ATAN2,
  // T op double (b plain)
  AD_ADD_TC = 23, AD_SUB_TC, AD_MUL_TC, AD_DIV_TC, AD_ATAN2_TC,
  // double op T (a plain)
  AD_ADD_CT = 28, AD_SUB_CT, AD_MUL_CT, AD_DIV_CT, AD_ATAN2_CT,
  // out[0] = rcp_fast(a), the rest 0
  AD_RCP = 33,
  // valof / value of each type holding a: out[0] valof(double) [1] valof(FastD) [2] valof(Dual<1>) [3] value(Dual<1>)
  // [4] valof(Dual<12>) [5] value(Dual<12>) [17] valof(Jet2) [18] value(Jet2) [19] value(double)
  AD_VALOF = 34,
  // unary, of a: sinh and cosh as hilo_mpc_amd/expr.py composes them, e = exp(a), 0.5 * e -+ 0.5 / e
  AD_SINH = 35, AD_COSH,
  AD_NOPS = 37
};
constexpr int AD_OUT = 20;

HD double ad_seed(int k) {
  constexpr double s[12] = {1.0, -1.0, 2.0, 0.0, 0.5, -4.0, 16.0, -0.25, 0.125, 0.0, -8.0, 32.0};
  return s[k];
}

// ca, cb: the plain-double operands of the mixed overloads
template <class T>
HD T ad_apply(int op, const T& a, const T& b, double ca, double cb) {
  switch (op) {
    case AD_NEG: return -a;
    case AD_SQ: return sq(a);
    case AD_SIN: return sin(a);
    case AD_COS: return cos(a);
    case AD_EXP: return exp(a);
    case AD_LOG: return log(a);
    case AD_SQRT: return sqrt(a);
    case AD_LOG10: return log10(a);
    case AD_FABS: return fabs(a);
    case AD_SIGN: return sign(a);
    case AD_ASIN: return asin(a);
    case AD_ACOS: return acos(a);
    case AD_ATAN: return atan(a);
    case AD_ASINH: return asinh(a);
    case AD_ACOSH: return acosh(a);
    case AD_ATANH: return atanh(a);
    case AD_TANH: return tanh(a);
    case AD_SECH2: return sech2(a);
    case AD_ADD: return a + b;
    case AD_SUB: return a - b;
    case AD_MUL: return a * b;
    case AD_DIV: return a / b;
    case AD_ATAN2: return atan2(a, b);
    case AD_ADD_TC: return a + cb;
    case AD_SUB_TC: return a - cb;
    case AD_MUL_TC: return a * cb;
    case AD_DIV_TC: return a / cb;
    case AD_ATAN2_TC: return atan2(a, cb);
    case AD_ADD_CT: return ca + b;
    case AD_SUB_CT: return ca - b;
    case AD_MUL_CT: return ca * b;
    case AD_DIV_CT: return ca / b;
    case AD_ATAN2_CT: return atan2(ca, b);
    case AD_SINH: { const T e = exp(a); return 0.5 * e - 0.5 / e; }
    case AD_COSH: { const T e = exp(a); return 0.5 * e + 0.5 / e; }
    default: return a;
  }
}

HD void ad_selftest_point(int op, double a, double b, double da, double db, double dda, double ddb, double* out) {
  for (int i = 0; i < AD_OUT; ++i) out[i] = 0.0;
  Dual<1> a1(a), b1(b);
  a1.d[0] = da;
  b1.d[0] = db;
  Dual<12> a12(a), b12(b);
  for (int k = 0; k < 12; ++k) {
    a12.d[k] = ad_seed(k) * da;
    b12.d[k] = ad_seed(k) * db;
  }
  const Jet2 aj(a, da, dda), bj(b, db, ddb);
  if (op == AD_RCP) {
    out[0] = rcp_fast(a);
    return;
  }
  if (op == AD_VALOF) {
    out[0] = valof(a);
    out[1] = valof(FastD(a));
    out[2] = valof(a1);
    out[3] = value(a1);
    out[4] = valof(a12);
    out[5] = value(a12);
    out[17] = valof(aj);
    out[18] = value(aj);
    out[19] = value(a);
    return;
  }
  out[0] = ad_apply<double>(op, a, b, a, b);
  out[1] = ad_apply<FastD>(op, FastD(a), FastD(b), a, b).v;
  const Dual<1> r1 = ad_apply<Dual<1>>(op, a1, b1, a, b);
  out[2] = r1.v;
  out[3] = r1.d[0];
  const Dual<12> r12 = ad_apply<Dual<12>>(op, a12, b12, a, b);
  out[4] = r12.v;
  for (int k = 0; k < 12; ++k) out[5 + k] = r12.d[k];
  const Jet2 rj = ad_apply<Jet2>(op, aj, bj, a, b);
  out[17] = rj.v;
  out[18] = rj.a;
  out[19] = rj.b;
}

}  // namespace hilo
