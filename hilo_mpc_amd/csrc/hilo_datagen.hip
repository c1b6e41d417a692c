// Data generation - excitation signal, plant and data set in one launch: C ABI and launches (device code: csrc/hilo_datagen.h).
//
// Reference semantics: `DataGenerator.random_uniform / random_normal / chirp` followed by `run` (hilo_mpc/util/data.py:806-1167) for
// a batch of experiments, each with its own initial state, parameters and random stream.
#include <stddef.h>
#include <string.h>

#include "hilo_datagen.h"
#include "hilo_kf_handle.h"

namespace hilo {

template <class M, int METHOD>
__global__ __launch_bounds__(ROLLOUT_TPB) void datagen_kernel(KfParams kp, SimParams sp, DatagenParams dg,
                                                              const double* __restrict__ chirp, int64_t batch, int T,
                                                              const double* __restrict__ x0, const double* __restrict__ up,
                                                              int64_t up_stride, double* __restrict__ F, double* __restrict__ L,
                                                              double* __restrict__ X, double* __restrict__ U, int* __restrict__ stats,
                                                              double t0) {
  datagen_body<M, METHOD>(kp, sp, dg, chirp, batch, T, x0, up, up_stride, F, L, X, U, stats, t0);
}

template <class M>
static int datagen_launch(const KfParams& kp, const SimParams& sp, const DatagenParams& dg, const double* chirp, int64_t batch, int T,
                          const double* x0, const double* up, int64_t us, double* F, double* L, double* X, double* U, int* stats,
                          double t0, hipStream_t s) {
  if constexpr (M::NU > 0 && M::NU <= DG_MAX_NU && M::NX <= DG_MAX_NX) {
    const unsigned grid = (unsigned)((batch + ROLLOUT_TPB - 1) / ROLLOUT_TPB);
    if (sp.method == SIM_DOPRI5) {
      if constexpr (!M::DISCRETE)
        hipLaunchKernelGGL((datagen_kernel<M, SIM_DOPRI5>), dim3(grid), dim3(ROLLOUT_TPB), 0, s, kp, sp, dg, chirp, batch, T, x0, up, us, F,
                           L, X, U, stats, t0);
      else
        return fail(HILO_ENOTSUP, "hilo_datagen_run: HILO_SIM_DOPRI5 on a discrete model");
    } else {
      hipLaunchKernelGGL((datagen_kernel<M, SIM_MAP>), dim3(grid), dim3(ROLLOUT_TPB), 0, s, kp, sp, dg, chirp, batch, T, x0, up, us, F, L,
                         X, U, stats, t0);
    }
    HILO_HIP_CHECK(hipGetLastError());
    return HILO_OK;
  } else {
    return fail(HILO_ENOTSUP, "hilo_datagen_run: the model has no inputs to excite");
  }
}

}  // namespace hilo

using namespace hilo;
using Lti211 = Lti<2, 1, 1>;
using Lti212 = Lti<2, 1, 2>;
using Lti422 = Lti<4, 2, 2>;

static_assert(HILO_DATAGEN_MAX_NU == DG_MAX_NU && HILO_DATAGEN_MAX_NU == HILO_PID_MAX_LOOPS && HILO_DATAGEN_MAX_NX == DG_MAX_NX &&
              HILO_DATAGEN_MAX_NX == HILO_SIM_DOPRI5_MAX_NX && HILO_DATAGEN_MAX_SEG == DG_MAX_SEG && HILO_DATAGEN_UNIFORM == DG_UNIFORM &&
              HILO_DATAGEN_NORMAL == DG_NORMAL && HILO_DATAGEN_CHIRP == DG_CHIRP && sizeof(hilo_datagen_opts) == sizeof(DatagenParams) &&
              offsetof(hilo_datagen_opts, instance_offset) == offsetof(DatagenParams, instance_offset) &&
              offsetof(hilo_datagen_opts, kind) == offsetof(DatagenParams, kind) &&
              offsetof(hilo_datagen_opts, hold) == offsetof(DatagenParams, hold) &&
              offsetof(hilo_datagen_opts, shift) == offsetof(DatagenParams, shift) &&
              offsetof(hilo_datagen_opts, difference) == offsetof(DatagenParams, difference) &&
              offsetof(hilo_datagen_opts, skip_mask) == offsetof(DatagenParams, skip_mask) &&
              offsetof(hilo_datagen_opts, a) == offsetof(DatagenParams, a) && offsetof(hilo_datagen_opts, b) == offsetof(DatagenParams, b) &&
              offsetof(hilo_datagen_opts, noise_kind) == offsetof(DatagenParams, noise_kind) &&
              offsetof(hilo_datagen_opts, noise_seed) == offsetof(DatagenParams, noise_seed) &&
              offsetof(hilo_datagen_opts, na) == offsetof(DatagenParams, na) && offsetof(hilo_datagen_opts, nb) == offsetof(DatagenParams, nb),
              "include/hilo_hip.h and csrc/hilo_datagen.h disagree");

extern "C" int hilo_datagen_run(hilo_kf* kf, const hilo_sim_opts* sim, const hilo_datagen_opts* opts, const double* chirp_table,
                                int64_t batch, int total_steps, const double* x0, const double* up, int64_t up_stride, double* F,
                                double* L, double* X, double* U, int32_t* stats, void* stream) {
  HILO_REQUIRE(kf, "hilo_datagen_run: NULL handle");
  HILO_REQUIRE(opts, "hilo_datagen_run: NULL opts");
  HILO_REQUIRE(batch >= 0 && total_steps >= 1, "hilo_datagen_run: need batch >= 0 and total_steps >= 1");
  SimParams sp = {SIM_MAP, 10000, 1e-6, 1e-8, 0.0};
  double t0 = 0.0;   // the time of row 0 of X (read by a time-variant model only)
  if (sim) {
    if (sim->method == HILO_SIM_BDF || sim->method == HILO_SIM_IDAS)
      return fail(HILO_ENOTSUP, "hilo_datagen_run: method %d; data generation is built for HILO_SIM_MAP and HILO_SIM_DOPRI5 (with an "
                                "input that jumps at the sampling instants the implicit methods would restart every interval)", sim->method);
    HILO_REQUIRE(sim->method == HILO_SIM_MAP || sim->method == HILO_SIM_DOPRI5, "hilo_datagen_run: unknown method %d", sim->method);
    sp.method = sim->method;
    if (sim->max_steps > 0) sp.max_steps = sim->max_steps;
    if (sim->rtol > 0.0) sp.rtol = sim->rtol;
    if (sim->atol > 0.0) sp.atol = sim->atol;
    if (sim->h0 > 0.0) sp.h0 = sim->h0;
    HILO_REQUIRE(sim->t0 == sim->t0 && ::fabs(sim->t0) < INFINITY, "hilo_datagen_run: t0 must be finite");
    t0 = sim->t0;
  }
  const bool user = kf->desc.model_id == 100 /* HILO_MODEL_USER */;
  if (user && kf->jit.nz > 0)
    return fail(HILO_ENOTSUP, "hilo_datagen_run: the model has algebraic states; data generation is built for models without them");
  if (kf->nu < 1) return fail(HILO_ENOTSUP, "hilo_datagen_run: the model has no inputs to excite");
  if (kf->nu > HILO_DATAGEN_MAX_NU)
    return fail(HILO_ENOTSUP, "hilo_datagen_run: the signal parameters are held for up to %d inputs; the model has %d",
                HILO_DATAGEN_MAX_NU, kf->nu);
  if (kf->nx > HILO_DATAGEN_MAX_NX)
    return fail(HILO_ENOTSUP, "hilo_datagen_run: the noise parameters are held for up to %d states; the model has %d",
                HILO_DATAGEN_MAX_NX, kf->nx);
  DatagenParams dg;
  static_assert(sizeof(dg) == sizeof(*opts), "by-value copy");
  memcpy(&dg, opts, sizeof(dg));
  dg.reserved = 0;
  HILO_REQUIRE(dg.kind == DG_UNIFORM || dg.kind == DG_NORMAL || dg.kind == DG_CHIRP, "hilo_datagen_run: unknown signal kind %d", dg.kind);
  HILO_REQUIRE(dg.kind == DG_CHIRP || dg.hold >= 1, "hilo_datagen_run: a staircase holds every sample for at least 1 interval, got %d",
               dg.hold);
  HILO_REQUIRE(dg.kind != DG_CHIRP || chirp_table, "hilo_datagen_run: HILO_DATAGEN_CHIRP without a chirp table");
  HILO_REQUIRE(dg.shift >= 0 && dg.shift < total_steps, "hilo_datagen_run: shift %d leaves no row of %d sampling intervals", dg.shift,
               total_steps);
  HILO_REQUIRE(dg.instance_offset >= 0 && dg.instance_offset + batch <= ((int64_t)1 << 32),
               "hilo_datagen_run: instance numbers %lld .. %lld do not fit the counter's 32-bit word", (long long)dg.instance_offset,
               (long long)(dg.instance_offset + batch));
  const int all = (int)((1u << kf->nx) - 1u);
  HILO_REQUIRE((dg.skip_mask & ~all) == 0 && (dg.skip_mask & all) != all, "hilo_datagen_run: skip_mask 0x%x names states beyond the "
               "model's %d or leaves none", dg.skip_mask, kf->nx);
  for (int i = 0; i < kf->nu; ++i) {
    if (dg.kind == DG_NORMAL) HILO_REQUIRE(dg.b[i] >= 0.0, "hilo_datagen_run: the variance of input %d is negative (%g)", i, dg.b[i]);
  }
  for (int i = 0; i < HILO_DATAGEN_MAX_NX; ++i) {
    if (i >= kf->nx) dg.noise_kind[i] = DG_NOISE_NONE;
    HILO_REQUIRE(dg.noise_kind[i] >= DG_NOISE_NONE && dg.noise_kind[i] <= DG_NOISE_NORMAL, "hilo_datagen_run: unknown noise kind %d "
                 "for state %d", dg.noise_kind[i], i);
  }
  if (sp.method == SIM_DOPRI5) {
    if (kf->discrete || !kf->kp.continuous)
      return fail(HILO_ENOTSUP, "hilo_datagen_run: HILO_SIM_DOPRI5 integrates a continuous model; this handle holds a discrete "
                                "(or discretised) one");
    if (user && kf->jit.datagen_scratch > 0)
      return fail(HILO_ENOTSUP, "hilo_datagen_run: the compiled right-hand side of this model leaves HILO_SIM_DOPRI5 %d bytes of scratch "
                                "memory per lane; the pair is built to keep its slopes in registers", kf->jit.datagen_scratch);
  }
  HILO_REQUIRE(up_stride == 0 || up_stride >= kf->nu + kf->np, "hilo_datagen_run: up_stride %lld < nu+np", (long long)up_stride);
  if (batch == 0) return HILO_OK;
  HILO_REQUIRE(x0 && up && F && L, "hilo_datagen_run: NULL argument");
  const int64_t blocks = (batch + ROLLOUT_TPB - 1) / ROLLOUT_TPB;
  HILO_REQUIRE(blocks < ((int64_t)1 << 31), "hilo_datagen_run: batch %lld exceeds the grid", (long long)batch);
  HILO_HIP_CHECK(hipSetDevice(kf->device));
  hipStream_t s = (hipStream_t)stream;
  const KfParams& kp = kf->kp;
  int* st = (int*)stats;
  const int T = total_steps;
  if (user) {
    hipFunction_t fn = kf->jit.datagen;
    HILO_REQUIRE(fn, "hilo_datagen_run: the run-time compiled data-generation kernel is not loaded");
    KfParams kpv = kp;
    int Tv = T;
    void* args[] = {&kpv, &sp, &dg, &chirp_table, &batch, &Tv, &x0, &up, &up_stride, &F, &L, &X, &U, &st, &t0};
    HILO_HIP_CHECK(hipModuleLaunchKernel(fn, (unsigned)blocks, 1, 1, ROLLOUT_TPB, 1, 1, 0, s, args, nullptr));
    return HILO_OK;
  }
  switch (kf->desc.model_id) {
#define X_(ID, M) \
  case ID: return datagen_launch<M>(kp, sp, dg, chirp_table, batch, T, x0, up, up_stride, F, L, X, U, st, t0, s);
    HILO_KF_MODELS(X_)
#undef X_
    case HILO_MODEL_LTI:
#define L_(M) return datagen_launch<M>(kp, sp, dg, chirp_table, batch, T, x0, up, up_stride, F, L, X, U, st, t0, s)
      if (kf->nx == 2 && kf->ny == 1) L_(Lti211);
      if (kf->nx == 2 && kf->ny == 2) L_(Lti212);
      L_(Lti422);
#undef L_
  }
  return fail(HILO_EINVAL, "unknown model id %d", kf->desc.model_id);
}
