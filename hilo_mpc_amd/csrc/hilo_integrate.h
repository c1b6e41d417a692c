// Error-controlled integration of a continuous model and the roll-out kernel body: one launch advances a batch of instances over
// many sampling intervals, one instance per lane.
//
// Where the reference simulates a continuous model with CVODES (dynamic_model.py `setup(solver=...)`, `simulate`), the fixed-step
// maps of hilo_models.h carry no error control.  `dopri5_interval` is the Dormand-Prince 5(4) pair with the step-size control of
// scipy's `RK45` (scipy/integrate/_ivp/rk.py, common.py::select_initial_step), so that its behaviour can be compared with a
// solver everybody has:
//   error norm   RMS of e_i / (atol + rtol max(|x_i|, |x_i+|))
//   controller   h <- h * clamp(0.9 err^(-1/5), 0.2, 10), at most 1 right after a rejection
//   first step   Hairer, Norsett, Wanner I, II.4 (the estimate scipy uses)
// The seventh slope of an accepted step is the first of the next (first same as last).  Inputs and parameters are held over a
// sampling interval; the model functors are autonomous (their `ode` takes no time), t only enters the smallest admissible step.
//
// Everything up to `rollout_body` is `HD` and templated on the functor like erk_step / rk4_classic, for doubles only: the same
// statements compile for the host (tests/test_integrate_host.py builds a driver around this header and runs it on the CPU).
#pragma once
#include "hilo_common.h"
#include "hilo_models.h"

namespace hilo {

constexpr int SIM_MAP = 0;      // hilo_sim_opts.method: the handle's own map (model_step)
constexpr int SIM_DOPRI5 = 1;   // HILO_SIM_DOPRI5
constexpr int SIM_OK = 0, SIM_MAX_STEPS = 1, SIM_STEP_TOO_SMALL = 2;   // HILO_SIM_STATUS_*
// Widest model the pair is built for: six slopes, the state and the trial point are alive at once (8 NX doubles = 16 NX
// registers) next to the model's own temporaries.  Measured with a dense synthetic right-hand side (a sine, an exponential and
// two products per state): 8 states 328 registers, 12 states 434, 16 states 507 of a lane's 512 - no scratch yet, no margin
// either.  A wider model is refused by the host (HILO_ENOTSUP) instead of being left to spill.
constexpr int DOPRI5_MAX_NX = 12;

struct SimParams {   // mirrors hilo_sim_opts (include/hilo_hip.h)
  int method, max_steps;
  double rtol, atol, h0;
};

// what one instance carries from one sampling interval to the next
template <int NX>
struct Dopri5Carry {
  double k1[NX];      // slope at the current state (valid when have_k1)
  double h;           // step-size proposal (0: not chosen yet)
  double t;           // time since the start of the roll-out (only for the smallest admissible step)
  int status, n_acc, n_rej, n_rhs;
  bool have_k1;
};

template <int NX>
HD void dopri5_init(Dopri5Carry<NX>& c, double h0) {
  c.h = h0 > 0.0 ? h0 : 0.0;
  c.t = 0.0;
  c.status = SIM_OK;
  c.n_acc = c.n_rej = c.n_rhs = 0;
  c.have_k1 = false;
}

template <int NX>
HD double dopri5_rms(const double* v, const double* scale) {
  double s = 0.0;
#pragma unroll
  for (int i = 0; i < NX; ++i) {
    const double q = v[i] / scale[i];
    s += q * q;
  }
  return ::sqrt(s / NX);
}

// Integrates dx/dt = f(x, u, p) over one sampling interval of length dt, in place.  Returns c.status; on a failure x holds the
// state at the time the integration stopped (the caller discards it).  `max_steps` bounds the attempted steps of this call (the
// meaning of CasADi's `max_num_steps`: per integrator call).
template <class M>
HD int dopri5_interval(Dopri5Carry<M::NX>& c, double* x, const double* u, const double* p, double dt, double rtol, double atol,
                       int max_steps) {
  constexpr int NX = M::NX;
  constexpr double EPS = 2.220446049250313e-16;
  // Dormand & Prince (1980), the coefficients of RK5(4)7M
  constexpr double A21 = 1.0 / 5;
  constexpr double A31 = 3.0 / 40, A32 = 9.0 / 40;
  constexpr double A41 = 44.0 / 45, A42 = -56.0 / 15, A43 = 32.0 / 9;
  constexpr double A51 = 19372.0 / 6561, A52 = -25360.0 / 2187, A53 = 64448.0 / 6561, A54 = -212.0 / 729;
  constexpr double A61 = 9017.0 / 3168, A62 = -355.0 / 33, A63 = 46732.0 / 5247, A64 = 49.0 / 176, A65 = -5103.0 / 18656;
  constexpr double B1 = 35.0 / 384, B3 = 500.0 / 1113, B4 = 125.0 / 192, B5 = -2187.0 / 6784, B6 = 11.0 / 84;
  constexpr double E1 = -71.0 / 57600, E3 = 71.0 / 16695, E4 = -71.0 / 1920, E5 = 17253.0 / 339200, E6 = -22.0 / 525, E7 = 1.0 / 40;
  auto f = [&](const double* at, double* k) {
    M::ode(at, u, p, dt, k);
    ++c.n_rhs;
  };
  if (c.status != SIM_OK) return c.status;
  if (!c.have_k1) {
    f(x, c.k1);
    c.have_k1 = true;
  }
  if (!(c.h > 0.0)) {   // the first step of the roll-out
    double scale[NX], x1[NX], f1[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) scale[i] = atol + ::fabs(x[i]) * rtol;
    const double d0 = dopri5_rms<NX>(x, scale), d1 = dopri5_rms<NX>(c.k1, scale);
    double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
    h0 = ::fmin(h0, dt);
#pragma unroll
    for (int i = 0; i < NX; ++i) x1[i] = x[i] + h0 * c.k1[i];
    f(x1, f1);
#pragma unroll
    for (int i = 0; i < NX; ++i) f1[i] -= c.k1[i];
    const double d2 = dopri5_rms<NX>(f1, scale) / h0;
    const double h1 = (d1 <= 1e-15 && d2 <= 1e-15) ? ::fmax(1e-6, h0 * 1e-3) : ::pow(0.01 / ::fmax(d1, d2), 0.2);
    c.h = ::fmin(::fmin(100.0 * h0, h1), dt);
    if (!(c.h > 0.0)) c.h = dt;   // a non-finite estimate: the controller below finds the step (or fails)
  }
  double tl = 0.0;          // time inside this interval
  bool rejected = false;    // the previous attempt of the CURRENT step was rejected
  int attempts = 0;
  while (tl < dt) {
    if (attempts >= max_steps) return c.status = SIM_MAX_STEPS;
    if (c.h < 16.0 * EPS * ::fabs(c.t + tl)) return c.status = SIM_STEP_TOO_SMALL;
    ++attempts;
    // clipped so that the sampling instant is hit exactly (a step that would leave a sliver of its own hundredth is stretched)
    const double rem = dt - tl;
    const bool last = 1.01 * c.h >= rem;
    const double h = last ? rem : c.h;
    double k2[NX], k3[NX], k4[NX], k5[NX], k6[NX], k7[NX], xi[NX], xn[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) xi[i] = x[i] + h * (A21 * c.k1[i]);
    f(xi, k2);
#pragma unroll
    for (int i = 0; i < NX; ++i) xi[i] = x[i] + h * (A31 * c.k1[i] + A32 * k2[i]);
    f(xi, k3);
#pragma unroll
    for (int i = 0; i < NX; ++i) xi[i] = x[i] + h * (A41 * c.k1[i] + A42 * k2[i] + A43 * k3[i]);
    f(xi, k4);
#pragma unroll
    for (int i = 0; i < NX; ++i) xi[i] = x[i] + h * (A51 * c.k1[i] + A52 * k2[i] + A53 * k3[i] + A54 * k4[i]);
    f(xi, k5);
#pragma unroll
    for (int i = 0; i < NX; ++i) xi[i] = x[i] + h * (A61 * c.k1[i] + A62 * k2[i] + A63 * k3[i] + A64 * k4[i] + A65 * k5[i]);
    f(xi, k6);
#pragma unroll
    for (int i = 0; i < NX; ++i) xn[i] = x[i] + h * (B1 * c.k1[i] + B3 * k3[i] + B4 * k4[i] + B5 * k5[i] + B6 * k6[i]);
    f(xn, k7);
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      const double e = h * (E1 * c.k1[i] + E3 * k3[i] + E4 * k4[i] + E5 * k5[i] + E6 * k6[i] + E7 * k7[i]);
      const double q = e / (atol + ::fmax(::fabs(x[i]), ::fabs(xn[i])) * rtol);
      s += q * q;
    }
    const double err = ::sqrt(s / NX);
    if (err < 1.0) {   // accepted (a non-finite estimate fails this comparison: a rejection)
      double fac = err == 0.0 ? 10.0 : ::fmin(10.0, 0.9 * ::pow(err, -0.2));
      if (rejected) fac = ::fmin(1.0, fac);
      // a clipped step says nothing against the proposal it was clipped from: keep the larger of the two
      c.h = last ? ::fmax(c.h, h * fac) : h * fac;
      tl = last ? dt : tl + h;
#pragma unroll
      for (int i = 0; i < NX; ++i) { x[i] = xn[i]; c.k1[i] = k7[i]; }
      ++c.n_acc;
      rejected = false;
    } else {
      c.h = h * ::fmax(0.2, 0.9 * ::pow(err, -0.2));   // (NaN or inf: fmax answers 0.2)
      ++c.n_rej;
      rejected = true;
    }
  }
  c.t += dt;
  return c.status;
}

constexpr int ROLLOUT_TPB = 64;   // one wave per workgroup: a slow instance holds back 63 others, not 255

// One instance per lane.  X [steps + 1][batch][NX] (row 0: x0), Y [steps][batch][NY] or null, stats [batch][4] (status, accepted,
// rejected, right-hand-side evaluations) or null; up: rows [u; p] of instance b at up + k up_step + b up_stride (up_step 0: held
// over the roll-out, up_stride 0: shared by the batch).  sp.method SIM_MAP: the map of the handle - the statements of pf_body
// (hilo_kf_kernel.h), what Model.step computes; SIM_DOPRI5: the pair above (continuous models up to DOPRI5_MAX_NX states - the host
// refuses the others).  The lanes of a wave run their own step sequences (a lane that rejects recomputes while its neighbours
// commit, a lane that has reached the sampling instant idles until the slowest has: the divergent loop runs while any lane is
// active); no value crosses lanes, so an instance's result does not depend on the instances it shares the wave with.  An
// instance that fails (SIM_MAX_STEPS, SIM_STEP_TOO_SMALL) gets NaN for the sampling instant it did not reach and every later one.
// METHOD: SIM_MAP / SIM_DOPRI5 builds that path alone (the library's kernels: each with the registers of its own path), -1 chooses
// by sp.method at run time (the one kernel of a run-time compiled model).
template <class M, int METHOD = -1, class KP>
__device__ __forceinline__ void rollout_body(const KP& kp, const SimParams& sp, int64_t batch, int steps,
                                             const double* __restrict__ x0, const double* __restrict__ up, int64_t up_stride,
                                             int64_t up_step, double* __restrict__ X, double* __restrict__ Y,
                                             int* __restrict__ stats) {
  constexpr int NX = M::NX, NU = M::NU, NP = M::NP, NY = M::NY;
  const int64_t b = (int64_t)blockIdx.x * ROLLOUT_TPB + threadIdx.x;
  if (b >= batch) return;
  double x[NX], upv[NU + NP > 0 ? NU + NP : 1];
#pragma unroll
  for (int i = 0; i < NX; ++i) {
    x[i] = x0[b * NX + i];
    X[b * NX + i] = x[i];
  }
  constexpr bool ADAPTIVE = !M::DISCRETE && NX <= DOPRI5_MAX_NX;
  Dopri5Carry<ADAPTIVE ? NX : 1> c;
  dopri5_init(c, sp.h0);
  const double nan = __builtin_nan("");
  for (int k = 0; k < steps; ++k) {
    if (k == 0 || up_step != 0) {
      const double* src = up + (int64_t)k * up_step + b * up_stride;
#pragma unroll
      for (int i = 0; i < NU + NP; ++i) upv[i] = src[i];
      c.have_k1 = false;   // the slope kept from the last step belongs to the previous interval's inputs
    }
    const double* u = upv;
    const double* p = upv + NU;
    bool ok = true;
    if (METHOD == SIM_DOPRI5 || (METHOD < 0 && sp.method == SIM_DOPRI5)) {
      if constexpr (ADAPTIVE && METHOD != SIM_MAP) ok = dopri5_interval<M>(c, x, u, p, kp.dt, sp.rtol, sp.atol, sp.max_steps) == SIM_OK;
    } else if constexpr (METHOD != SIM_DOPRI5) {
      double xo[NX];
      if (kp.continuous && !M::DISCRETE) model_step<M>(4, kp.n_sub, x, u, p, kp.dt, xo);
      else model_step<M>(kp.erk_order, kp.n_sub, x, u, p, kp.dt, xo);
#pragma unroll
      for (int i = 0; i < NX; ++i) x[i] = xo[i];
    }
    double* Xk = X + ((int64_t)(k + 1) * batch + b) * NX;
#pragma unroll
    for (int i = 0; i < NX; ++i) Xk[i] = ok ? x[i] : nan;
    if constexpr (NY > 0) {
      if (Y != nullptr) {
        double yy[NY];
        M::meas(x, u, p, kp.dt, yy);
        double* Yk = Y + ((int64_t)k * batch + b) * NY;
#pragma unroll
        for (int i = 0; i < NY; ++i) Yk[i] = ok ? yy[i] : nan;
      }
    }
  }
  if (stats != nullptr) {
    stats[b * 4 + 0] = c.status;
    stats[b * 4 + 1] = c.n_acc;
    stats[b * 4 + 2] = c.n_rej;
    stats[b * 4 + 3] = c.n_rhs;
  }
}
}  // namespace hilo
