// Batched roll-out of a handle's model over many sampling intervals in one launch: C ABI and launches (device code:
// csrc/hilo_integrate.h).
//
// Reference semantics: `Model.simulate` (hilo_mpc/modules/dynamic_model/dynamic_model.py:3911-4000) - inputs held over a
// sampling interval, the state and the measurements recorded at every sampling instant - for a batch of instances.  A run-time
// compiled model may depend on time explicitly (hilo_integrate.h, the section on time): its kernels take the time of the first
// row as a trailing argument; the functors of the zoo are autonomous and their kernels are the ones they were.
#include "hilo_integrate.h"
#include "hilo_kf_handle.h"

namespace hilo {

template <class M, int METHOD>
__global__ __launch_bounds__(ROLLOUT_TPB) void rollout_kernel(KfParams kp, SimParams sp, int64_t batch, int steps,
                                                              const double* __restrict__ x0, const double* __restrict__ up,
                                                              int64_t up_stride, int64_t up_step, double* __restrict__ X,
                                                              double* __restrict__ Y, int* __restrict__ stats) {
  if constexpr (METHOD == SIM_BDF) {
    __shared__ double bdf_lds[bdf_entries(M::NX) * ROLLOUT_TPB];
    rollout_body<M, SIM_BDF>(kp, sp, batch, steps, x0, up, up_stride, up_step, X, Y, stats, (lds_double*)bdf_lds);
  } else {
    rollout_body<M, METHOD>(kp, sp, batch, steps, x0, up, up_stride, up_step, X, Y, stats);
  }
}

template <class M>
static int rollout_launch(const KfParams& kp, const SimParams& sp, int64_t batch, int steps, const double* x0, const double* up,
                          int64_t us, int64_t ustep, double* X, double* Y, int* stats, hipStream_t s) {
  const unsigned grid = (unsigned)((batch + ROLLOUT_TPB - 1) / ROLLOUT_TPB);
  if (sp.method == SIM_DOPRI5) {
    if constexpr (!M::DISCRETE)
      hipLaunchKernelGGL((rollout_kernel<M, SIM_DOPRI5>), dim3(grid), dim3(ROLLOUT_TPB), 0, s, kp, sp, batch, steps, x0, up, us, ustep, X,
                         Y, stats);
    else
      return fail(HILO_ENOTSUP, "hilo_model_rollout: HILO_SIM_DOPRI5 on a discrete model");
  } else if (sp.method == SIM_BDF) {
    if constexpr (!M::DISCRETE && M::NX <= BDF_MAX_NX)
      hipLaunchKernelGGL((rollout_kernel<M, SIM_BDF>), dim3(grid), dim3(ROLLOUT_TPB), 0, s, kp, sp, batch, steps, x0, up, us, ustep, X, Y,
                         stats);
    else
      return fail(HILO_ENOTSUP, "hilo_model_rollout: HILO_SIM_BDF on a discrete model");
  } else {
    hipLaunchKernelGGL((rollout_kernel<M, SIM_MAP>), dim3(grid), dim3(ROLLOUT_TPB), 0, s, kp, sp, batch, steps, x0, up, us, ustep, X, Y,
                       stats);
  }
  HILO_HIP_CHECK(hipGetLastError());
  return HILO_OK;
}

// the roll-out with forward sensitivities, one instance on a team of T lanes (hilo_integrate.h::rollout_sens_body)
template <class M>
__global__ __launch_bounds__(ROLLOUT_TPB) void rollout_sens_kernel(KfParams kp, SimParams sp, int64_t batch, int steps,
                                                                   const double* __restrict__ x0, const double* __restrict__ up,
                                                                   int64_t up_stride, int64_t up_step, int wrt, int T,
                                                                   double* __restrict__ X, double* __restrict__ Y,
                                                                   double* __restrict__ SX, double* __restrict__ SY,
                                                                   int* __restrict__ stats) {
  rollout_sens_body<M>(kp, sp, batch, steps, x0, up, up_stride, up_step, wrt, T, X, Y, SX, SY, stats, 0.0);
}

template <class M>
static int rollout_sens_launch(const KfParams& kp, const SimParams& sp, int64_t batch, int steps, const double* x0, const double* up,
                               int64_t us, int64_t ustep, int wrt, int T, unsigned grid, double* X, double* Y, double* SX, double* SY,
                               int* stats, hipStream_t s) {
  if constexpr (!M::DISCRETE && !model_has_ext<M>::value && M::NX <= SENS_MAX_NX) {
    hipLaunchKernelGGL((rollout_sens_kernel<M>), dim3(grid), dim3(ROLLOUT_TPB), 0, s, kp, sp, batch, steps, x0, up, us, ustep, wrt, T, X,
                       Y, SX, SY, stats);
    HILO_HIP_CHECK(hipGetLastError());
    return HILO_OK;
  } else {
    return fail(HILO_ENOTSUP, "hilo_model_rollout_sens: no sensitivity kernel is built for this model (discrete, a learned term, or more "
                              "than %d states)", SENS_MAX_NX);
  }
}

}  // namespace hilo

using namespace hilo;

static_assert(HILO_SIM_DOPRI5_MAX_NX == DOPRI5_MAX_NX && HILO_SIM_DOPRI5 == SIM_DOPRI5 && HILO_SIM_STATUS_MAX_STEPS == SIM_MAX_STEPS &&
              HILO_SIM_STATUS_STEP_TOO_SMALL == SIM_STEP_TOO_SMALL && HILO_SIM_BDF == SIM_BDF && HILO_SIM_BDF_MAX_NX == BDF_MAX_NX &&
              HILO_SIM_IDAS == SIM_IDAS && HILO_SIM_STATUS_IC_FAILED == SIM_IC_FAILED && HILO_SIM_SENS_MAX_NX == SENS_MAX_NX &&
              HILO_SENS_X0 == SENS_X0 && HILO_SENS_U == SENS_U && HILO_SENS_P == SENS_P,
              "include/hilo_hip.h and csrc/hilo_integrate.h disagree");

// What the three entry points below share; `who` is the entry point's name, so that every message reads as it did.
// SimParams and the time of row 0 of X (read by a time-variant model only) from the caller's options (NULL: the defaults)
static int sim_options(const char* who, const hilo_sim_opts* opts, SimParams* sp, double* t0) {
  *sp = {SIM_MAP, 10000, 1e-6, 1e-8, 0.0};
  *t0 = 0.0;
  if (!opts) return HILO_OK;
  sp->method = opts->method;
  if (opts->max_steps > 0) sp->max_steps = opts->max_steps;
  if (opts->rtol > 0.0) sp->rtol = opts->rtol;
  if (opts->atol > 0.0) sp->atol = opts->atol;
  if (opts->h0 > 0.0) sp->h0 = opts->h0;
  HILO_REQUIRE(opts->t0 == opts->t0 && ::fabs(opts->t0) < INFINITY, "%s: t0 must be finite", who);
  *t0 = opts->t0;
  return HILO_OK;
}

// the checks of a non-empty batch's arguments (`pointers`: the entry point's own required ones are there); a NULL `up` leaves
// pointing at a stand-in
static int sim_check_args(const char* who, const hilo_kf* kf, int64_t batch, bool pointers, const double** up, int64_t up_stride,
                          int64_t up_step) {
  HILO_REQUIRE(pointers, "%s: NULL argument", who);
  HILO_REQUIRE(kf->nu + kf->np == 0 || *up, "%s: the model has %d inputs/parameters but `up` is NULL", who, kf->nu + kf->np);
  HILO_REQUIRE(up_stride == 0 || up_stride >= kf->nu + kf->np, "%s: up_stride %lld < nu+np", who, (long long)up_stride);
  HILO_REQUIRE(up_step == 0 || up_step >= (up_stride ? batch * up_stride : kf->nu + kf->np),
               "%s: up_step %lld is shorter than one sampling interval's rows", who, (long long)up_step);
  static const double zero = 0.0;
  if (!*up) *up = &zero;   // never read (nu + np == 0); keeps the pointer arithmetic of the kernel defined
  return HILO_OK;
}

// hilo_model_rollout (h NULL) and hilo_model_rollout_resume
static int rollout_impl(hilo_kf* kf, const hilo_sim_opts* opts, int64_t batch, int steps, const double* x0, const double* up,
                        int64_t up_stride, int64_t up_step, double* X, double* Y, int32_t* stats, double* h, void* stream) {
  HILO_REQUIRE(kf, "hilo_model_rollout: NULL handle");
  HILO_REQUIRE(batch >= 0 && steps >= 1, "hilo_model_rollout: need batch >= 0 and steps >= 1");
  HILO_REQUIRE(!opts || opts->method == HILO_SIM_MAP || opts->method == HILO_SIM_DOPRI5 || opts->method == HILO_SIM_BDF,
               "hilo_model_rollout: unknown method %d", opts->method);
  SimParams sp;
  double t0;
  if (int rc = sim_options("hilo_model_rollout", opts, &sp, &t0)) return rc;
  if (sp.method == SIM_DOPRI5) {
    if (kf->discrete || !kf->kp.continuous)
      return fail(HILO_ENOTSUP, "hilo_model_rollout: HILO_SIM_DOPRI5 integrates a continuous model; this handle holds a discrete "
                                "(or discretised) one");
    if (kf->nx > HILO_SIM_DOPRI5_MAX_NX)
      return fail(HILO_ENOTSUP, "hilo_model_rollout: HILO_SIM_DOPRI5 keeps its slopes in registers and is built for up to %d states; "
                                "the model has %d", HILO_SIM_DOPRI5_MAX_NX, kf->nx);
    if (kf->desc.model_id == 100 /* HILO_MODEL_USER */ && kf->jit.rollout_scratch > 0)
      return fail(HILO_ENOTSUP, "hilo_model_rollout: the compiled right-hand side of this model leaves HILO_SIM_DOPRI5 %d bytes of scratch "
                                "memory per lane; the pair is built to keep its slopes in registers", kf->jit.rollout_scratch);
  }
  if (sp.method == SIM_BDF) {
    if (kf->discrete || !kf->kp.continuous)
      return fail(HILO_ENOTSUP, "hilo_model_rollout: HILO_SIM_BDF integrates a continuous model; this handle holds a discrete "
                                "(or discretised) one");
    if (kf->nx > HILO_SIM_BDF_MAX_NX)
      return fail(HILO_ENOTSUP, "hilo_model_rollout: HILO_SIM_BDF keeps its difference table, the Jacobian and its factors in the LDS of "
                                "one workgroup and is built for up to %d states; the model has %d", HILO_SIM_BDF_MAX_NX, kf->nx);
    if (kf->desc.model_id == 100 /* HILO_MODEL_USER */ && kf->jit.rollout_bdf_scratch > 0)
      return fail(HILO_ENOTSUP, "hilo_model_rollout: the compiled right-hand side of this model leaves HILO_SIM_BDF %d bytes of scratch "
                                "memory per lane; the method is built to keep its vectors in registers", kf->jit.rollout_bdf_scratch);
  }
  if (sp.method != SIM_DOPRI5) h = nullptr;   // the other methods have no proposal to hand on
  if (h && kf->desc.model_id != 100 /* HILO_MODEL_USER */)
    return fail(HILO_ENOTSUP, "hilo_model_rollout_resume: the step-size proposal is handed on by the kernels of a run-time compiled "
                              "model; this handle holds a model of the zoo (pass h = NULL)");
  if (batch == 0) return HILO_OK;
  if (int rc = sim_check_args("hilo_model_rollout", kf, batch, x0 && X, &up, up_stride, up_step)) return rc;
  HILO_HIP_CHECK(hipSetDevice(kf->device));
  hipStream_t s = (hipStream_t)stream;
  const KfParams& kp = kf->kp;
  int* st = (int*)stats;
  if (kf->desc.model_id == 100 /* HILO_MODEL_USER */) {
    hipFunction_t fn = sp.method == SIM_BDF ? kf->jit.rollout_bdf : kf->jit.rollout;
    HILO_REQUIRE(fn, "hilo_model_rollout: the run-time compiled roll-out kernel is not loaded");
    KfParams kpv = kp;
    void* args[] = {&kpv, &sp, &batch, &steps, &x0, &up, &up_stride, &up_step, &X, &Y, &st, &t0, &h};   // (h: hilo_user_rollout alone)
    const unsigned grid = (unsigned)((batch + ROLLOUT_TPB - 1) / ROLLOUT_TPB);
    HILO_HIP_CHECK(hipModuleLaunchKernel(fn, grid, 1, 1, ROLLOUT_TPB, 1, 1, 0, s, args, nullptr));
    return HILO_OK;
  }
  switch (kf->desc.model_id) {
#define X_(ID, T) case ID: return rollout_launch<T>(kp, sp, batch, steps, x0, up, up_stride, up_step, X, Y, st, s);
    HILO_KF_MODELS(X_)
#undef X_
    case HILO_MODEL_LTI:
      if (kf->nx == 2 && kf->ny == 1) return rollout_launch<Lti<2, 1, 1>>(kp, sp, batch, steps, x0, up, up_stride, up_step, X, Y, st, s);
      if (kf->nx == 2 && kf->ny == 2) return rollout_launch<Lti<2, 1, 2>>(kp, sp, batch, steps, x0, up, up_stride, up_step, X, Y, st, s);
      return rollout_launch<Lti<4, 2, 2>>(kp, sp, batch, steps, x0, up, up_stride, up_step, X, Y, st, s);
  }
  return fail(HILO_EINVAL, "unknown model id %d", kf->desc.model_id);
}

extern "C" int hilo_model_rollout(hilo_kf* kf, const hilo_sim_opts* opts, int64_t batch, int steps, const double* x0,
                                  const double* up, int64_t up_stride, int64_t up_step, double* X, double* Y, int32_t* stats,
                                  void* stream) {
  return rollout_impl(kf, opts, batch, steps, x0, up, up_stride, up_step, X, Y, stats, nullptr, stream);
}

// A model with algebraic states under HILO_SIM_IDAS (csrc/hilo_integrate.h::rollout_idas_body).  The zoo has no such model: the
// kernel lives in the run-time compiled unit alone.
extern "C" int hilo_model_rollout_dae(hilo_kf* kf, const hilo_sim_opts* opts, int64_t batch, int steps, const double* x0,
                                      const double* z0, const double* up, int64_t up_stride, int64_t up_step, double* X, double* Z,
                                      double* Y, int32_t* stats, void* stream) {
  HILO_REQUIRE(kf, "hilo_model_rollout_dae: NULL handle");
  HILO_REQUIRE(batch >= 0 && steps >= 1, "hilo_model_rollout_dae: need batch >= 0 and steps >= 1");
  SimParams sp;
  double t0;   // (no kernel of a DAE reads it)
  if (int rc = sim_options("hilo_model_rollout_dae", opts, &sp, &t0)) return rc;
  if (sp.method != SIM_IDAS)
    return fail(HILO_ENOTSUP, "hilo_model_rollout_dae: method %d; this entry integrates with HILO_SIM_IDAS alone (the other methods: "
                              "hilo_model_rollout)", sp.method);
  const int nz = kf->desc.model_id == 100 /* HILO_MODEL_USER */ ? kf->jit.nz : 0;
  if (nz <= 0)
    return fail(HILO_ENOTSUP, "hilo_model_rollout_dae: HILO_SIM_IDAS integrates a model with algebraic states; this handle's model has "
                              "none (HILO_SIM_BDF through hilo_model_rollout integrates it)");
  if (kf->discrete || !kf->kp.continuous)
    return fail(HILO_ENOTSUP, "hilo_model_rollout_dae: HILO_SIM_IDAS integrates a continuous model; this handle holds a discrete "
                              "(or discretised) one");
  if (kf->nx + nz > HILO_SIM_BDF_MAX_NX)
    return fail(HILO_ENOTSUP, "hilo_model_rollout_dae: HILO_SIM_IDAS keeps its difference table, the Jacobian and its factors in the LDS "
                              "of one workgroup and is built for up to %d differential and algebraic states together; the model has "
                              "%d + %d", HILO_SIM_BDF_MAX_NX, kf->nx, nz);
  if (kf->jit.rollout_idas_scratch > 0)
    return fail(HILO_ENOTSUP, "hilo_model_rollout_dae: the compiled equations of this model leave HILO_SIM_IDAS %d bytes of scratch "
                              "memory per lane; the method is built to keep its vectors in registers", kf->jit.rollout_idas_scratch);
  if (batch == 0) return HILO_OK;
  if (int rc = sim_check_args("hilo_model_rollout_dae", kf, batch, x0 && X, &up, up_stride, up_step)) return rc;
  HILO_HIP_CHECK(hipSetDevice(kf->device));
  hipFunction_t fn = kf->jit.rollout_idas;
  HILO_REQUIRE(fn, "hilo_model_rollout_dae: the run-time compiled roll-out kernel is not loaded");
  KfParams kpv = kf->kp;
  int* st = (int*)stats;
  void* args[] = {&kpv, &sp, &batch, &steps, &x0, &z0, &up, &up_stride, &up_step, &X, &Z, &Y, &st};
  const unsigned grid = (unsigned)((batch + ROLLOUT_TPB - 1) / ROLLOUT_TPB);
  HILO_HIP_CHECK(hipModuleLaunchKernel(fn, grid, 1, 1, ROLLOUT_TPB, 1, 1, 0, (hipStream_t)stream, args, nullptr));
  return HILO_OK;
}

extern "C" int hilo_model_rollout_resume(hilo_kf* kf, const hilo_sim_opts* opts, int64_t batch, int steps, const double* x0,
                                         const double* up, int64_t up_stride, int64_t up_step, double* X, double* Y,
                                         int32_t* stats, double* h, void* stream) {
  return rollout_impl(kf, opts, batch, steps, x0, up, up_stride, up_step, X, Y, stats, h, stream);
}

// Forward sensitivities of the HILO_SIM_DOPRI5 roll-out (csrc/hilo_integrate.h::rollout_sens_body): the augmented system on a team
// of lanes per instance.
extern "C" int hilo_model_rollout_sens(hilo_kf* kf, const hilo_sim_opts* opts, int64_t batch, int steps, const double* x0,
                                       const double* up, int64_t up_stride, int64_t up_step, int32_t wrt, double* X, double* Y,
                                       double* SX, double* SY, int32_t* stats, void* stream) {
  HILO_REQUIRE(kf, "hilo_model_rollout_sens: NULL handle");
  HILO_REQUIRE(batch >= 0 && steps >= 1, "hilo_model_rollout_sens: need batch >= 0 and steps >= 1");
  SimParams sp;
  double t0;
  if (int rc = sim_options("hilo_model_rollout_sens", opts, &sp, &t0)) return rc;
  const bool user = kf->desc.model_id == 100 /* HILO_MODEL_USER */;
  if (sp.method != SIM_DOPRI5)
    return fail(HILO_ENOTSUP, "hilo_model_rollout_sens: method %d; the sensitivities are integrated with HILO_SIM_DOPRI5 alone (the "
                              "fixed-step maps and the implicit methods carry none)", sp.method);
  if (kf->discrete || !kf->kp.continuous)
    return fail(HILO_ENOTSUP, "hilo_model_rollout_sens: HILO_SIM_DOPRI5 integrates a continuous model; this handle holds a discrete "
                              "(or discretised) one");
  if (user && kf->jit.nz > 0)
    return fail(HILO_ENOTSUP, "hilo_model_rollout_sens: the model has algebraic states; sensitivities are integrated for models "
                              "without them");
  if (kf->desc.model_id == HILO_MODEL_CHEMOSTAT4_GP || (user && kf->desc.n_user_gp > 0))
    return fail(HILO_ENOTSUP, "hilo_model_rollout_sens: the model carries a learned term; its sensitivities are not implemented");
  if (kf->nx > HILO_SIM_SENS_MAX_NX)
    return fail(HILO_ENOTSUP, "hilo_model_rollout_sens: a lane keeps the pair's vectors twice as wide as the plain roll-out and the "
                              "kernel is built for up to %d states; the model has %d", HILO_SIM_SENS_MAX_NX, kf->nx);
  HILO_REQUIRE(wrt > 0 && (wrt & ~(HILO_SENS_X0 | HILO_SENS_U | HILO_SENS_P)) == 0, "hilo_model_rollout_sens: wrt %d is not a "
               "combination of HILO_SENS_X0, HILO_SENS_U, HILO_SENS_P", wrt);
  const int ns = ((wrt & HILO_SENS_X0) ? kf->nx : 0) + ((wrt & HILO_SENS_U) ? kf->nu : 0) + ((wrt & HILO_SENS_P) ? kf->np : 0);
  HILO_REQUIRE(ns >= 1, "hilo_model_rollout_sens: the selected groups are empty for this model (nu %d, np %d)", kf->nu, kf->np);
  if (ns > ROLLOUT_TPB)
    return fail(HILO_ENOTSUP, "hilo_model_rollout_sens: %d columns; a team is at most the %d lanes of a wave", ns, ROLLOUT_TPB);
  if ((wrt & HILO_SENS_U) && kf->nu > 0 && up_step != 0)
    return fail(HILO_ENOTSUP, "hilo_model_rollout_sens: with an input sequence every interval's input is a parameter of its own; "
                              "HILO_SENS_U needs inputs held over the roll-out (up_step 0)");
  if (user && kf->jit.rollout_sens_scratch > 0)
    return fail(HILO_ENOTSUP, "hilo_model_rollout_sens: the compiled right-hand side of this model leaves the sensitivity kernel %d "
                              "bytes of scratch memory per lane; it is built to keep its vectors in registers", kf->jit.rollout_sens_scratch);
  if (batch == 0) return HILO_OK;
  if (int rc = sim_check_args("hilo_model_rollout_sens", kf, batch, x0 && X && SX, &up, up_stride, up_step)) return rc;
  int T = 1;
  while (T < ns) T <<= 1;   // the smallest power of two >= ns
  const int per_wave = ROLLOUT_TPB / T;
  const int64_t blocks = (batch + per_wave - 1) / per_wave;
  HILO_REQUIRE(blocks < ((int64_t)1 << 31), "hilo_model_rollout_sens: batch %lld with teams of %d lanes exceeds the grid", (long long)batch, T);
  const unsigned grid = (unsigned)blocks;
  HILO_HIP_CHECK(hipSetDevice(kf->device));
  hipStream_t s = (hipStream_t)stream;
  const KfParams& kp = kf->kp;
  int* st = (int*)stats;
  if (user) {
    hipFunction_t fn = kf->jit.rollout_sens;
    HILO_REQUIRE(fn, "hilo_model_rollout_sens: the run-time compiled sensitivity kernel is not loaded");
    KfParams kpv = kp;
    int wrt_ = wrt;
    void* args[] = {&kpv, &sp, &batch, &steps, &x0, &up, &up_stride, &up_step, &wrt_, &T, &X, &Y, &SX, &SY, &st, &t0};
    HILO_HIP_CHECK(hipModuleLaunchKernel(fn, grid, 1, 1, ROLLOUT_TPB, 1, 1, 0, s, args, nullptr));
    return HILO_OK;
  }
  switch (kf->desc.model_id) {
#define X_(ID, T_) case ID: return rollout_sens_launch<T_>(kp, sp, batch, steps, x0, up, up_stride, up_step, wrt, T, grid, X, Y, SX, SY, st, s);
    HILO_KF_MODELS(X_)
#undef X_
  }
  return fail(HILO_ENOTSUP, "hilo_model_rollout_sens: no sensitivity kernel is built for model id %d", kf->desc.model_id);
}
