// Linear-quadratic regulator for batches: C ABI and launches (device code: csrc/hilo_lqr.h).
//
// Reference semantics: `LinearQuadraticRegulator.setup / call` (hilo_mpc/modules/controller/lqr.py:204-306) - the gain of a linear
// (or linearised) discrete model after `horizon` backward Riccati steps from P = Q and u = -K x - for a batch of instances with
// their own parameters and operating points, plus the stationary gain the reference leaves to "future releases".
#include "hilo_lqr.h"
#include "hilo_kf_handle.h"

namespace hilo {

__global__ __launch_bounds__(64) void lqr_gain_kernel(int n, int m, LqrParams o, int64_t batch, const double* __restrict__ A, int64_t a_stride,
                                                      const double* __restrict__ B, int64_t b_stride, const double* __restrict__ Q,
                                                      int64_t q_stride, const double* __restrict__ R, int64_t r_stride,
                                                      const double* __restrict__ N, int64_t n_stride, double* __restrict__ K,
                                                      double* __restrict__ P, int* __restrict__ stats) {
  extern __shared__ double lqr_lds[];
  lqr_gain_body((lds_double*)lqr_lds, n, m, o, batch, A, a_stride, B, b_stride, Q, q_stride, R, r_stride, N, n_stride, K, P, stats);
}

template <class M>
__global__ __launch_bounds__(64) void lqr_call_kernel(KfParams kp, LqrParams o, int64_t batch, const double* __restrict__ x,
                                                      const double* __restrict__ x_eq, const double* __restrict__ u_eq,
                                                      const double* __restrict__ p, int64_t p_stride, const double* __restrict__ Q,
                                                      const double* __restrict__ R, const double* __restrict__ N, double* __restrict__ K,
                                                      double* __restrict__ P, double* __restrict__ u, int* __restrict__ stats) {
  __shared__ double lqr_lds[LqrModelOk<M>::value ? lqr_work_doubles(M::NX, M::NU) * lqr_lanes(M::NX, M::NU) : 1];
  lqr_call_body<M>((lds_double*)lqr_lds, kp, o, batch, x, x_eq, u_eq, p, p_stride, Q, R, N, K, P, u, stats);
}

template <class M>
__global__ __launch_bounds__(64) void lqr_linearize_kernel(KfParams kp, int64_t batch, const double* __restrict__ x,
                                                           const double* __restrict__ up, int64_t up_stride, double* __restrict__ A,
                                                           double* __restrict__ B, double* __restrict__ C) {
  lqr_linearize_body<M>(kp, batch, x, up, up_stride, A, B, C);
}

__global__ __launch_bounds__(64) void lqr_apply_kernel(int n, int m, int64_t batch, const double* __restrict__ K, int64_t k_stride,
                                                       const double* __restrict__ x, const double* __restrict__ x_eq,
                                                       const double* __restrict__ u_eq, double* __restrict__ u) {
  const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= batch) return;
  lqr_feedback(n, m, K + b * k_stride, x + b * n, x_eq != nullptr ? x_eq + b * n : nullptr, u_eq != nullptr ? u_eq + b * m : nullptr,
               u + b * m);
}

template <class M>
static int lqr_call_launch(const KfParams& kp, const LqrParams& o, int64_t batch, const double* x, const double* x_eq, const double* u_eq,
                           const double* p, int64_t ps, const double* Q, const double* R, const double* N, double* K, double* P, double* u,
                           int* stats, hipStream_t s) {
  if constexpr (LqrModelOk<M>::value) {
    constexpr int lanes = lqr_lanes(M::NX, M::NU);
    hipLaunchKernelGGL((lqr_call_kernel<M>), dim3((unsigned)((batch + lanes - 1) / lanes)), dim3(lanes), 0, s, kp, o, batch, x, x_eq, u_eq, p,
                       ps, Q, R, N, K, P, u, stats);
    HILO_HIP_CHECK(hipGetLastError());
    return HILO_OK;
  }
  return fail(HILO_ENOTSUP, "hilo_lqr_call: not built for this model (no inputs, more than %d states or %d inputs, algebraic states or a learned term)", HILO_LQR_MAX_NX, HILO_LQR_MAX_NU);
}

template <class M>
static int lqr_linearize_launch(const KfParams& kp, int64_t batch, const double* x, const double* up, int64_t us, double* A, double* B,
                                double* C, hipStream_t s) {
  if constexpr (LqrModelOk<M>::value) {
    hipLaunchKernelGGL((lqr_linearize_kernel<M>), dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, s, kp, batch, x, up, us, A, B, C);
    HILO_HIP_CHECK(hipGetLastError());
    return HILO_OK;
  }
  return fail(HILO_ENOTSUP, "hilo_model_linearize: not built for this model (no inputs, more than %d states or %d inputs, algebraic states or a learned term)", HILO_LQR_MAX_NX, HILO_LQR_MAX_NU);
}

// what both handle-based entries check: a discrete-time map of an admitted size, and a loaded kernel without scratch memory
static int lqr_check_handle(const hilo_kf* kf, const char* who) {
  HILO_REQUIRE(kf, "%s: NULL handle", who);
  HILO_REFUSE_TIME_VARIANT(kf, who);
  if (!kf->discrete && kf->kp.continuous)
    return fail(HILO_ENOTSUP, "%s: the handle holds a continuous model that was not discretised; the Jacobians and gains here are those "
                              "of the discrete-time map (Model.discretize)", who);
  if (kf->nx > HILO_LQR_MAX_NX || kf->nu > HILO_LQR_MAX_NU || kf->nx < 1)
    return fail(HILO_ENOTSUP, "%s: built for up to %d states and %d inputs; the model has %d and %d", who, HILO_LQR_MAX_NX, HILO_LQR_MAX_NU,
                kf->nx, kf->nu);
  if (kf->nu < 1) return fail(HILO_ENOTSUP, "%s: the model has no inputs", who);
  if (kf->desc.model_id == 100 /* HILO_MODEL_USER */) {
    HILO_REQUIRE(kf->jit.lqr_call && kf->jit.lqr_linearize, "%s: the run-time compiled kernels are not loaded", who);
    if (!kf->jit.lqr_ok)
      return fail(HILO_ENOTSUP, "%s: not built for this model (algebraic states)", who);
    if (kf->jit.lqr_scratch > 0)
      return fail(HILO_ENOTSUP, "%s: the compiled kernels of this model need %d bytes of scratch memory per lane; they are built to keep "
                                "the derivative arithmetic in registers", who, kf->jit.lqr_scratch);
  }
  return HILO_OK;
}

static int lqr_params(const hilo_lqr_opts* opts, const char* who, LqrParams* o) {
  *o = LqrParams{0, 50, 1e-12};
  if (opts) {
    HILO_REQUIRE(opts->horizon >= 0, "%s: horizon %d (0: stationary)", who, opts->horizon);
    o->horizon = opts->horizon;
    if (opts->max_iter > 0) o->max_iter = opts->max_iter;
    if (opts->tol > 0.0) o->tol = opts->tol;
  }
  return HILO_OK;
}

}  // namespace hilo

using namespace hilo;

static_assert(HILO_LQR_MAX_NX == LQR_MAX_NX && HILO_LQR_MAX_NU == LQR_MAX_NU && HILO_LQR_STATUS_OK == LQR_OK &&
              HILO_LQR_STATUS_MAX_ITER == LQR_MAX_ITER && HILO_LQR_STATUS_FAILED == LQR_FAILED,
              "include/hilo_hip.h and csrc/hilo_lqr.h disagree");
static_assert(lqr_lanes(LQR_MAX_NX, LQR_MAX_NU) * lqr_work_doubles(LQR_MAX_NX, LQR_MAX_NU) * 8 <= LQR_LDS_BYTES,
              "the widest admitted instance does not fit the LDS");

extern "C" int hilo_model_linearize(hilo_kf* kf, int64_t batch, const double* x, const double* up, int64_t up_stride, double* A, double* B,
                                    double* C, void* stream) {
  int rc = lqr_check_handle(kf, "hilo_model_linearize");
  if (rc) return rc;
  HILO_REQUIRE(batch >= 0, "hilo_model_linearize: negative batch");
  if (batch == 0) return HILO_OK;
  HILO_REQUIRE(x && up && A && B, "hilo_model_linearize: NULL argument");
  HILO_REQUIRE(up_stride == 0 || up_stride >= kf->nu + kf->np, "hilo_model_linearize: up_stride %lld < nu+np", (long long)up_stride);
  HILO_HIP_CHECK(hipSetDevice(kf->device));
  hipStream_t s = (hipStream_t)stream;
  const KfParams& kp = kf->kp;
  if (kf->desc.model_id == 100 /* HILO_MODEL_USER */) {
    KfParams kpv = kp;
    void* args[] = {&kpv, &batch, &x, &up, &up_stride, &A, &B, &C};
    HILO_HIP_CHECK(hipModuleLaunchKernel(kf->jit.lqr_linearize, (unsigned)((batch + 63) / 64), 1, 1, 64, 1, 1, 0, s, args, nullptr));
    return HILO_OK;
  }
  switch (kf->desc.model_id) {
#define X_(ID, T) case ID: return lqr_linearize_launch<T>(kp, batch, x, up, up_stride, A, B, C, s);
    HILO_KF_MODELS(X_)
#undef X_
    case HILO_MODEL_LTI:
      if (kf->nx == 2 && kf->ny == 1) return lqr_linearize_launch<Lti<2, 1, 1>>(kp, batch, x, up, up_stride, A, B, C, s);
      if (kf->nx == 2 && kf->ny == 2) return lqr_linearize_launch<Lti<2, 1, 2>>(kp, batch, x, up, up_stride, A, B, C, s);
      return lqr_linearize_launch<Lti<4, 2, 2>>(kp, batch, x, up, up_stride, A, B, C, s);
  }
  return fail(HILO_EINVAL, "unknown model id %d", kf->desc.model_id);
}

extern "C" int hilo_lqr_gain(int nx, int nu, int64_t batch, const double* A, int64_t a_stride, const double* B, int64_t b_stride,
                             const double* Q, int64_t q_stride, const double* R, int64_t r_stride, const double* N, int64_t n_stride,
                             const hilo_lqr_opts* opts, double* K, double* P, int32_t* stats, void* stream) {
  if (nx < 1 || nu < 1 || nx > HILO_LQR_MAX_NX || nu > HILO_LQR_MAX_NU)
    return fail(HILO_ENOTSUP, "hilo_lqr_gain: built for 1..%d states and 1..%d inputs; got %d and %d", HILO_LQR_MAX_NX, HILO_LQR_MAX_NU, nx,
                nu);
  LqrParams o;
  int rc = lqr_params(opts, "hilo_lqr_gain", &o);
  if (rc) return rc;
  HILO_REQUIRE(batch >= 0, "hilo_lqr_gain: negative batch");
  if (batch == 0) return HILO_OK;
  HILO_REQUIRE(A && B && Q && R && K, "hilo_lqr_gain: NULL argument");
  HILO_REQUIRE((a_stride == 0 || a_stride >= nx * nx) && (b_stride == 0 || b_stride >= nx * nu) && (q_stride == 0 || q_stride >= nx * nx) &&
                   (r_stride == 0 || r_stride >= nu * nu) && (n_stride == 0 || n_stride >= nx * nu),
               "hilo_lqr_gain: a stride is shorter than its matrix");
  const int lanes = lqr_lanes(nx, nu);
  const size_t lds = sizeof(double) * lqr_work_doubles(nx, nu) * lanes;
  if (lds > 64 * 1024)   // (more than the default limit of dynamic LDS: the attribute is set per device, and setting it again is harmless)
    HILO_HIP_CHECK(hipFuncSetAttribute((const void*)lqr_gain_kernel, hipFuncAttributeMaxDynamicSharedMemorySize, LQR_LDS_BYTES));
  hipLaunchKernelGGL(lqr_gain_kernel, dim3((unsigned)((batch + lanes - 1) / lanes)), dim3(lanes), lds, (hipStream_t)stream, nx, nu, o, batch, A,
                     a_stride, B, b_stride, Q, q_stride, R, r_stride, N, n_stride, K, P, (int*)stats);
  HILO_HIP_CHECK(hipGetLastError());
  return HILO_OK;
}

extern "C" int hilo_lqr_call(hilo_kf* kf, const hilo_lqr_opts* opts, int64_t batch, const double* x, const double* x_eq, const double* u_eq,
                             const double* p, int64_t p_stride, const double* Q, const double* R, const double* N, double* K, double* P,
                             double* u, int32_t* stats, void* stream) {
  int rc = lqr_check_handle(kf, "hilo_lqr_call");
  if (rc) return rc;
  LqrParams o;
  rc = lqr_params(opts, "hilo_lqr_call", &o);
  if (rc) return rc;
  HILO_REQUIRE(batch >= 0, "hilo_lqr_call: negative batch");
  if (batch == 0) return HILO_OK;
  HILO_REQUIRE(Q && R && K, "hilo_lqr_call: NULL argument");
  HILO_REQUIRE((x == nullptr) == (u == nullptr), "hilo_lqr_call: x and u go together (both NULL: the gains alone)");
  HILO_REQUIRE(kf->np == 0 || p, "hilo_lqr_call: the model has %d parameters but `p` is NULL", kf->np);
  HILO_REQUIRE(p_stride == 0 || p_stride >= kf->np, "hilo_lqr_call: p_stride %lld < np", (long long)p_stride);
  HILO_HIP_CHECK(hipSetDevice(kf->device));
  hipStream_t s = (hipStream_t)stream;
  const KfParams& kp = kf->kp;
  static const double zero = 0.0;
  if (!p) p = &zero;   // never read (np == 0)
  int* st = (int*)stats;
  if (kf->desc.model_id == 100 /* HILO_MODEL_USER */) {
    KfParams kpv = kp;
    const int lanes = lqr_lanes(kf->nx, kf->nu);
    void* args[] = {&kpv, &o, &batch, &x, &x_eq, &u_eq, &p, &p_stride, &Q, &R, &N, &K, &P, &u, &st};
    HILO_HIP_CHECK(hipModuleLaunchKernel(kf->jit.lqr_call, (unsigned)((batch + lanes - 1) / lanes), 1, 1, lanes, 1, 1, 0, s, args, nullptr));
    return HILO_OK;
  }
  switch (kf->desc.model_id) {
#define X_(ID, T) case ID: return lqr_call_launch<T>(kp, o, batch, x, x_eq, u_eq, p, p_stride, Q, R, N, K, P, u, st, s);
    HILO_KF_MODELS(X_)
#undef X_
    case HILO_MODEL_LTI:
      if (kf->nx == 2 && kf->ny == 1) return lqr_call_launch<Lti<2, 1, 1>>(kp, o, batch, x, x_eq, u_eq, p, p_stride, Q, R, N, K, P, u, st, s);
      if (kf->nx == 2 && kf->ny == 2) return lqr_call_launch<Lti<2, 1, 2>>(kp, o, batch, x, x_eq, u_eq, p, p_stride, Q, R, N, K, P, u, st, s);
      return lqr_call_launch<Lti<4, 2, 2>>(kp, o, batch, x, x_eq, u_eq, p, p_stride, Q, R, N, K, P, u, st, s);
  }
  return fail(HILO_EINVAL, "unknown model id %d", kf->desc.model_id);
}

extern "C" int hilo_lqr_apply(int nx, int nu, int64_t batch, const double* K, int64_t k_stride, const double* x, const double* x_eq,
                              const double* u_eq, double* u, void* stream) {
  HILO_REQUIRE(nx >= 1 && nu >= 1, "hilo_lqr_apply: need nx >= 1 and nu >= 1");
  HILO_REQUIRE(batch >= 0, "hilo_lqr_apply: negative batch");
  if (batch == 0) return HILO_OK;
  HILO_REQUIRE(K && x && u, "hilo_lqr_apply: NULL argument");
  HILO_REQUIRE(k_stride == 0 || k_stride >= nx * nu, "hilo_lqr_apply: k_stride %lld < nu*nx", (long long)k_stride);
  hipLaunchKernelGGL(lqr_apply_kernel, dim3((unsigned)((batch + 63) / 64)), dim3(64), 0, (hipStream_t)stream, nx, nu, batch, K, k_stride, x, x_eq,
                     u_eq, u);
  HILO_HIP_CHECK(hipGetLastError());
  return HILO_OK;
}
