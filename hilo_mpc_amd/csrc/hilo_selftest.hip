// Developer aids that run the derivative arithmetic (hilo_ad.h) and the postfix interpreter (hilo_expr.h) on their own, outside
// any solver: tests/test_ad_ops_gpu.py compares what they write with a 50-digit reference.
#include "hilo_ad_selftest.h"
#include "hilo_common.h"
#include "hilo_expr.h"

namespace hilo {

// in[i][7] = op, a, b, da, db, dda, ddb; out[i][AD_OUT]
__global__ void __launch_bounds__(64) ad_selftest_kernel(int64_t n, const double* __restrict__ in, double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const double* q = in + i * 7;
  double r[AD_OUT];
  ad_selftest_point((int)q[0], q[1], q[2], q[3], q[4], q[5], q[6], r);
  for (int c = 0; c < AD_OUT; ++c) out[i * AD_OUT + c] = r[c];
}

constexpr int XS_NX = 4, XS_NU = 2, XS_NP = 3;
constexpr int XS_IN = 3 * (XS_NX + XS_NU), XS_OUT = 4;

// in[i][18] = x[4] dx[4] ddx[4] u[2] du[2] ddu[2]; out[i][4] = value in double, then v a b in Jet2
__global__ void __launch_bounds__(64) expr_selftest_kernel(const double* __restrict__ block, int which, int64_t n,
                                                           const double* __restrict__ in, const double* __restrict__ p,
                                                           double* __restrict__ out) {
  const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
  if (i >= n) return;
  const double* q = in + i * XS_IN;
  double x[XS_NX], u[XS_NU];
  Jet2 xj[XS_NX], uj[XS_NU];
  for (int c = 0; c < XS_NX; ++c) {
    x[c] = q[c];
    xj[c] = Jet2(q[c], q[XS_NX + c], q[2 * XS_NX + c]);
  }
  for (int c = 0; c < XS_NU; ++c) {
    u[c] = q[3 * XS_NX + c];
    uj[c] = Jet2(q[3 * XS_NX + c], q[3 * XS_NX + XS_NU + c], q[3 * XS_NX + 2 * XS_NU + c]);
  }
  const double* prog = expr_program(block, which);
  const double v = expr_eval<XS_NX, XS_NU, double>(prog, x, u, p);
  const Jet2 j = expr_eval<XS_NX, XS_NU, Jet2>(prog, xj, uj, p);
  out[i * XS_OUT + 0] = v;
  out[i * XS_OUT + 1] = j.v;
  out[i * XS_OUT + 2] = j.a;
  out[i * XS_OUT + 3] = j.b;
}

}  // namespace hilo

using namespace hilo;

extern "C" int hilo_ad_selftest(int64_t n, const double* in, double* out, void* stream) {
  HILO_REQUIRE(n >= 1 && n <= (1 << 20) && in && out, "hilo_ad_selftest: bad argument");
  hipLaunchKernelGGL(ad_selftest_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, (hipStream_t)stream, n, in, out);
  HILO_HIP_CHECK(hipGetLastError());
  return HILO_OK;
}

extern "C" int hilo_expr_selftest(const double* block, int block_len, int count, int which, int64_t n, const double* in,
                                  const double* p, double* out, void* stream) {
  HILO_REQUIRE(block && block_len >= 1 && count >= 1 && which >= 0 && which < count && n >= 1 && n <= (1 << 20) && in && p && out,
               "hilo_expr_selftest: bad argument");
  const char* why = "";
  if (expr_check(block, block_len, count, XS_NX, XS_NU, XS_NP, &why)) return fail(HILO_EINVAL, "hilo_expr_selftest: %s", why);
  hipStream_t s = (hipStream_t)stream;
  double* d_block = nullptr;
  HILO_HIP_CHECK(hipMalloc((void**)&d_block, sizeof(double) * block_len));
  hipError_t e = hipMemcpyAsync(d_block, block, sizeof(double) * block_len, hipMemcpyHostToDevice, s);
  if (e == hipSuccess) {
    hipLaunchKernelGGL(expr_selftest_kernel, dim3((unsigned)((n + 63) / 64)), dim3(64), 0, s, d_block, which, n, in, p, out);
    e = hipGetLastError();
  }
  if (e == hipSuccess) e = hipStreamSynchronize(s);     // the program block is freed below
  hipFree(d_block);
  HILO_HIP_CHECK(e);
  return HILO_OK;
}
