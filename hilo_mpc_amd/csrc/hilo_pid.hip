// PID: the batched law and the closed loop of controller and plant in one launch: C ABI and launches (device code:
// csrc/hilo_pid.h).
//
// Reference semantics: `PID.call` (hilo_mpc/modules/controller/pid.py:335-365) for a batch of controllers, and what
// `SimpleControlLoop.run` does with such a controller and a plant (control_loop.py:343-397) - process value, law, plant step,
// `steps` times - for a batch of loops without leaving the device.
#include <stddef.h>

#include "hilo_pid.h"
#include "hilo_kf_handle.h"

namespace hilo {

constexpr int PID_CALL_TPB = 256;

// one loop of one instance per lane
__global__ __launch_bounds__(PID_CALL_TPB) void pid_call_kernel(PidParams po, int64_t batch, double dt, const double* __restrict__ pv,
                                                                const double* __restrict__ sp, int64_t sp_stride,
                                                                const double* __restrict__ gains, int64_t gain_stride,
                                                                double* __restrict__ mem, double* __restrict__ u) {
  const int64_t e = (int64_t)blockIdx.x * PID_CALL_TPB + threadIdx.x;
  const int nsp = po.nsp;
  if (e >= batch * nsp) return;
  const int64_t b = e / nsp;
  const int j = (int)(e - b * nsp);
  double m[PID_MEM];
#pragma unroll
  for (int r = 0; r < PID_MEM; ++r) m[r] = mem[e * PID_MEM + r];
  const double* g = gains + b * gain_stride;
  double err, lo = 0.0, hi = 0.0;   // (selects: a kernel argument indexed at run time would be copied to scratch memory first)
#pragma unroll
  for (int i = 0; i < PID_MAX_LOOPS; ++i) {
    lo = j == i ? po.lo[i] : lo;
    hi = j == i ? po.hi[i] : hi;
  }
  u[e] = pid_update(m, pv != nullptr ? pv[e] : 0.0, sp[b * sp_stride + j], g[j], g[nsp + j], g[2 * nsp + j], dt, po.flags, lo, hi, &err);
#pragma unroll
  for (int r = 0; r < PID_MEM; ++r) mem[e * PID_MEM + r] = m[r];
}

template <class M, int METHOD>
__global__ __launch_bounds__(ROLLOUT_TPB) void pid_loop_kernel(KfParams kp, SimParams sp, PidParams po, int64_t batch, int steps,
                                                               const double* __restrict__ x0, const double* __restrict__ up,
                                                               int64_t up_stride, const double* __restrict__ spt, int64_t sp_stride,
                                                               int64_t sp_step, const double* __restrict__ gains,
                                                               int64_t gain_stride, double* __restrict__ mem, double* __restrict__ X,
                                                               double* __restrict__ U, double* __restrict__ Y, double* __restrict__ J,
                                                               double* __restrict__ x_final, int* __restrict__ stats) {
  pid_loop_body<M, METHOD>(kp, sp, po, batch, steps, x0, up, up_stride, spt, sp_stride, sp_step, gains, gain_stride, mem, X, U, Y, J,
                           x_final, stats);
}

template <class M>
static int pid_loop_launch(const KfParams& kp, const SimParams& sp, const PidParams& po, int64_t batch, int steps, const double* x0,
                           const double* up, int64_t us, const double* spt, int64_t ss, int64_t sstep, const double* gains, int64_t gs,
                           double* mem, double* X, double* U, double* Y, double* J, double* xf, int* stats, hipStream_t s) {
  if constexpr (M::NU > 0) {
    const unsigned grid = (unsigned)((batch + ROLLOUT_TPB - 1) / ROLLOUT_TPB);
    if (sp.method == SIM_DOPRI5) {
      if constexpr (!M::DISCRETE)
        hipLaunchKernelGGL((pid_loop_kernel<M, SIM_DOPRI5>), dim3(grid), dim3(ROLLOUT_TPB), 0, s, kp, sp, po, batch, steps, x0, up, us, spt,
                           ss, sstep, gains, gs, mem, X, U, Y, J, xf, stats);
      else
        return fail(HILO_ENOTSUP, "hilo_pid_loop: HILO_SIM_DOPRI5 on a discrete model");
    } else {
      hipLaunchKernelGGL((pid_loop_kernel<M, SIM_MAP>), dim3(grid), dim3(ROLLOUT_TPB), 0, s, kp, sp, po, batch, steps, x0, up, us, spt, ss,
                         sstep, gains, gs, mem, X, U, Y, J, xf, stats);
    }
    HILO_HIP_CHECK(hipGetLastError());
    return HILO_OK;
  } else {
    return fail(HILO_EINVAL, "hilo_pid_loop: the model has no inputs for a controller to drive");
  }
}

static int pid_params(const hilo_pid_opts* opts, const char* who, PidParams* po) {
  HILO_REQUIRE(opts, "%s: NULL opts", who);
  HILO_REQUIRE(opts->nsp >= 1 && opts->nsp <= HILO_PID_MAX_LOOPS, "%s: %d loops; a controller has 1 to %d", who, opts->nsp,
               HILO_PID_MAX_LOOPS);
  HILO_REQUIRE((opts->flags & ~(HILO_PID_P_ON_PV | HILO_PID_D_ON_PV | HILO_PID_LIMITS)) == 0, "%s: unknown flags %d", who, opts->flags);
  po->nsp = opts->nsp;
  po->flags = opts->flags;
  for (int j = 0; j < HILO_PID_MAX_LOOPS; ++j) {
    po->pv_index[j] = opts->pv_index[j];
    po->pv_is_state[j] = opts->pv_is_state[j];
    po->out_index[j] = opts->out_index[j];
    po->lo[j] = opts->lo[j];
    po->hi[j] = opts->hi[j];
    if (j < opts->nsp && (opts->flags & HILO_PID_LIMITS))
      HILO_REQUIRE(opts->lo[j] <= opts->hi[j], "%s: the limits of loop %d are not an interval (lo %g, hi %g)", who, j, opts->lo[j],
                   opts->hi[j]);
  }
  return HILO_OK;
}

}  // namespace hilo

using namespace hilo;
using Lti211 = Lti<2, 1, 1>;
using Lti212 = Lti<2, 1, 2>;
using Lti422 = Lti<4, 2, 2>;

static_assert(HILO_PID_MAX_LOOPS == PID_MAX_LOOPS && HILO_PID_MEM == PID_MEM && HILO_PID_P_ON_PV == PID_P_ON_PV &&
              HILO_PID_D_ON_PV == PID_D_ON_PV && HILO_PID_LIMITS == PID_LIMITS && HILO_PID_MAX_LOOPS == HILO_LQR_MAX_NU &&
              sizeof(hilo_pid_opts) == sizeof(PidParams) && offsetof(hilo_pid_opts, pv_index) == offsetof(PidParams, pv_index) &&
              offsetof(hilo_pid_opts, pv_is_state) == offsetof(PidParams, pv_is_state) &&
              offsetof(hilo_pid_opts, out_index) == offsetof(PidParams, out_index) && offsetof(hilo_pid_opts, lo) == offsetof(PidParams, lo) &&
              offsetof(hilo_pid_opts, hi) == offsetof(PidParams, hi),
              "include/hilo_hip.h and csrc/hilo_pid.h disagree");

extern "C" int hilo_pid_call(const hilo_pid_opts* opts, int64_t batch, double dt, const double* pv, const double* sp,
                             int64_t sp_stride, const double* gains, int64_t gain_stride, double* mem, double* u, void* stream) {
  PidParams po;
  if (int rc = pid_params(opts, "hilo_pid_call", &po)) return rc;
  HILO_REQUIRE(batch >= 0, "hilo_pid_call: need batch >= 0");
  HILO_REQUIRE(dt > 0.0 && dt < INFINITY, "hilo_pid_call: the sampling interval must be positive and finite");
  HILO_REQUIRE(sp_stride == 0 || sp_stride >= po.nsp, "hilo_pid_call: sp_stride %lld < nsp", (long long)sp_stride);
  HILO_REQUIRE(gain_stride == 0 || gain_stride >= 3 * po.nsp, "hilo_pid_call: gain_stride %lld < 3 nsp", (long long)gain_stride);
  if (batch == 0) return HILO_OK;
  HILO_REQUIRE(sp && gains && mem && u, "hilo_pid_call: NULL argument");
  const int64_t blocks = (batch * po.nsp + PID_CALL_TPB - 1) / PID_CALL_TPB;
  HILO_REQUIRE(blocks < ((int64_t)1 << 31), "hilo_pid_call: batch %lld exceeds the grid", (long long)batch);
  hipLaunchKernelGGL(pid_call_kernel, dim3((unsigned)blocks), dim3(PID_CALL_TPB), 0, (hipStream_t)stream, po, batch, dt, pv, sp, sp_stride,
                     gains, gain_stride, mem, u);
  HILO_HIP_CHECK(hipGetLastError());
  return HILO_OK;
}

extern "C" int hilo_pid_loop(hilo_kf* kf, const hilo_sim_opts* sim, const hilo_pid_opts* opts, int64_t batch, int steps,
                             const double* x0, const double* up, int64_t up_stride, const double* spt, int64_t sp_stride,
                             int64_t sp_step, const double* gains, int64_t gain_stride, double* mem, double* X, double* U, double* Y,
                             double* J, double* x_final, int32_t* stats, double* h, void* stream) {
  HILO_REQUIRE(kf, "hilo_pid_loop: NULL handle");
  HILO_REQUIRE(batch >= 0 && steps >= 1, "hilo_pid_loop: need batch >= 0 and steps >= 1");
  PidParams po;
  if (int rc = pid_params(opts, "hilo_pid_loop", &po)) return rc;
  SimParams sp = {SIM_MAP, 10000, 1e-6, 1e-8, 0.0};
  double t0 = 0.0;   // the time of row 0 of X (read by a time-variant model only)
  if (sim) {
    if (sim->method == HILO_SIM_BDF || sim->method == HILO_SIM_IDAS)
      return fail(HILO_ENOTSUP, "hilo_pid_loop: method %d; the closed loop is built for HILO_SIM_MAP and HILO_SIM_DOPRI5 (with an input "
                                "that jumps at every sampling instant the implicit methods would restart every interval)", sim->method);
    HILO_REQUIRE(sim->method == HILO_SIM_MAP || sim->method == HILO_SIM_DOPRI5, "hilo_pid_loop: unknown method %d", sim->method);
    sp.method = sim->method;
    if (sim->max_steps > 0) sp.max_steps = sim->max_steps;
    if (sim->rtol > 0.0) sp.rtol = sim->rtol;
    if (sim->atol > 0.0) sp.atol = sim->atol;
    if (sim->h0 > 0.0) sp.h0 = sim->h0;
    HILO_REQUIRE(sim->t0 == sim->t0 && ::fabs(sim->t0) < INFINITY, "hilo_pid_loop: t0 must be finite");
    t0 = sim->t0;
  }
  const bool user = kf->desc.model_id == 100 /* HILO_MODEL_USER */;
  if (user && kf->jit.nz > 0)
    return fail(HILO_ENOTSUP, "hilo_pid_loop: the model has algebraic states; the closed loop is built for models without them");
  HILO_REQUIRE(po.nsp <= kf->nu, "hilo_pid_loop: %d loops for a model of %d inputs; every loop drives an input of its own", po.nsp,
               kf->nu);
  for (int j = 0; j < po.nsp; ++j) {
    const int n = po.pv_is_state[j] ? kf->nx : kf->ny;
    HILO_REQUIRE(po.pv_index[j] >= 0 && po.pv_index[j] < n, "hilo_pid_loop: loop %d selects %s %d of %d", j,
                 po.pv_is_state[j] ? "state" : "measurement", po.pv_index[j], n);
    HILO_REQUIRE(po.out_index[j] >= 0 && po.out_index[j] < kf->nu, "hilo_pid_loop: loop %d drives input %d of %d", j, po.out_index[j],
                 kf->nu);
    for (int i = 0; i < j; ++i)
      HILO_REQUIRE(po.out_index[i] != po.out_index[j], "hilo_pid_loop: loops %d and %d both drive input %d", i, j, po.out_index[j]);
  }
  if (sp.method == SIM_DOPRI5) {
    if (kf->discrete || !kf->kp.continuous)
      return fail(HILO_ENOTSUP, "hilo_pid_loop: HILO_SIM_DOPRI5 integrates a continuous model; this handle holds a discrete "
                                "(or discretised) one");
    if (kf->nx > HILO_SIM_DOPRI5_MAX_NX)
      return fail(HILO_ENOTSUP, "hilo_pid_loop: HILO_SIM_DOPRI5 keeps its slopes in registers and is built for up to %d states; "
                                "the model has %d", HILO_SIM_DOPRI5_MAX_NX, kf->nx);
    if (user && kf->jit.pid_loop_scratch > 0)
      return fail(HILO_ENOTSUP, "hilo_pid_loop: the compiled right-hand side of this model leaves HILO_SIM_DOPRI5 %d bytes of scratch "
                                "memory per lane; the pair is built to keep its slopes in registers", kf->jit.pid_loop_scratch);
  } else {
    h = nullptr;   // the map has no proposal to hand on
  }
  if (h && !user)
    return fail(HILO_ENOTSUP, "hilo_pid_loop: the step-size proposal is handed on by the kernel of a run-time compiled model; this "
                              "handle holds a model of the zoo (pass h = NULL)");
  HILO_REQUIRE(up_stride == 0 || up_stride >= kf->nu + kf->np, "hilo_pid_loop: up_stride %lld < nu+np", (long long)up_stride);
  HILO_REQUIRE(sp_stride == 0 || sp_stride >= po.nsp, "hilo_pid_loop: sp_stride %lld < nsp", (long long)sp_stride);
  HILO_REQUIRE(sp_step == 0 || sp_step >= (sp_stride ? batch * sp_stride : po.nsp),
               "hilo_pid_loop: sp_step %lld is shorter than one sampling interval's set points", (long long)sp_step);
  HILO_REQUIRE(gain_stride == 0 || gain_stride >= 3 * po.nsp, "hilo_pid_loop: gain_stride %lld < 3 nsp", (long long)gain_stride);
  if (batch == 0) return HILO_OK;
  HILO_REQUIRE(x0 && up && spt && gains && mem && J && x_final, "hilo_pid_loop: NULL argument");
  HILO_HIP_CHECK(hipSetDevice(kf->device));
  hipStream_t s = (hipStream_t)stream;
  const KfParams& kp = kf->kp;
  int* st = (int*)stats;
  if (user) {
    hipFunction_t fn = kf->jit.pid_loop;
    HILO_REQUIRE(fn, "hilo_pid_loop: the run-time compiled closed-loop kernel is not loaded");
    KfParams kpv = kp;
    void* args[] = {&kpv, &sp, &po, &batch, &steps, &x0, &up, &up_stride, &spt, &sp_stride, &sp_step, &gains, &gain_stride, &mem,
                    &X, &U, &Y, &J, &x_final, &st, &t0, &h};
    const unsigned grid = (unsigned)((batch + ROLLOUT_TPB - 1) / ROLLOUT_TPB);
    HILO_HIP_CHECK(hipModuleLaunchKernel(fn, grid, 1, 1, ROLLOUT_TPB, 1, 1, 0, s, args, nullptr));
    return HILO_OK;
  }
  switch (kf->desc.model_id) {
#define X_(ID, T) \
  case ID: return pid_loop_launch<T>(kp, sp, po, batch, steps, x0, up, up_stride, spt, sp_stride, sp_step, gains, gain_stride, mem, X, U, Y, J, x_final, st, s);
    HILO_KF_MODELS(X_)
#undef X_
    case HILO_MODEL_LTI:
#define L_(T) return pid_loop_launch<T>(kp, sp, po, batch, steps, x0, up, up_stride, spt, sp_stride, sp_step, gains, gain_stride, mem, X, U, Y, J, x_final, st, s)
      if (kf->nx == 2 && kf->ny == 1) L_(Lti211);
      if (kf->nx == 2 && kf->ny == 2) L_(Lti212);
      L_(Lti422);
#undef L_
  }
  return fail(HILO_EINVAL, "unknown model id %d", kf->desc.model_id);
}
