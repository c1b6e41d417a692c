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
// sampling interval; time is not.
//
// Time.  A functor that declares TIME_VARIANT (hilo_models.h::model_time_variant) is handed the absolute time of every evaluation
// through `ode_t` / `meas_t`; every other functor is autonomous, and for it the statements below are the ones they were before
// time existed (the selection is `if constexpr` on the trait).  The carry structs hold the start time `t0` of what they integrate
// next to their own clock `t`, which starts at 0: the absolute time is t0 + t (+ the position inside the interval).  The roll-out
// forms the start of sampling interval k as t0 + k dt, never as a running sum.
//   map          stage i of a sub-step of length h that starts at s is evaluated at s + c_i h (hilo_models.h::erk_c); a discrete
//                model's map and measurement of interval k see t_k = t0 + k dt (the reference hands its discrete function ONE
//                time per call, modules/base.py:1785-1795, :1882-1895)
//   dopri5       stage times of scipy's RK45, C = (0, 1/5, 3/10, 4/5, 8/9, 1, 1); the first-step estimate evaluates f(t + h0, x + h0 f0);
//                the slope kept from an accepted step was taken at the time and state the next step starts from
//   bdf          fun(t_new, y) in the Newton iteration, f(t + h0, y1) in the first-step estimate, the Jacobian df/dx at the current
//                (t, x) (no df/dt term, as in scipy)
//   measurement  a continuous model's y[k] = h(t_k + dt, x_{k+1}, u_k, p) (modules/base.py:1729)
// The smallest admissible step is measured against the absolute time in either method.
//
// One implementation per method.  `dopri5_core` is the pair for a value type and a norm policy: `dopri5_interval` is it on doubles,
// `dopri5_sens_interval` on dual numbers over a team of lanes.  `ndf_interval` is the variable-order step loop for a system
// policy: `bdf_interval` is it on dx/dt = f (OdeSystem), `idas_interval` on [x; z] (DaeSystem).  `select_initial_step` is the
// first-step estimate of all four.  The roll-out bodies and the closed loop of hilo_pid.h share `rollout_load_up`,
// `plant_interval` and `rollout_write_stats`.
//
// Everything up to `rollout_body` is `HD` and templated on the functor like erk_step / rk4_classic: the same statements compile
// for the host (tests/test_integrate_host.py builds a driver around this header and runs it on the CPU).
#pragma once
#include "hilo_common.h"
#include "hilo_models.h"

namespace hilo {

constexpr int SIM_MAP = 0;      // hilo_sim_opts.method: the handle's own map (model_step)
constexpr int SIM_DOPRI5 = 1;   // HILO_SIM_DOPRI5
constexpr int SIM_OK = 0, SIM_MAX_STEPS = 1, SIM_STEP_TOO_SMALL = 2, SIM_IC_FAILED = 3;   // HILO_SIM_STATUS_* (3: SIM_IDAS alone)
// Widest model the pair is built for: six slopes, the state and the trial point are alive at once (8 NX doubles = 16 NX
// registers) next to the model's own temporaries.  Measured with a dense synthetic right-hand side (a sine, an exponential and
// two products per state): 8 states 328 registers, 12 states 434, 16 states 507 of a lane's 512 - no scratch yet, no margin
// either.  A wider model is refused by the host (HILO_ENOTSUP) instead of being left to spill.
constexpr int DOPRI5_MAX_NX = 12;

struct SimParams {   // mirrors hilo_sim_opts (include/hilo_hip.h) up to its start time, which is a kernel argument of its own
  int method, max_steps;
  double rtol, atol, h0;
};

// what one instance carries from one sampling interval to the next.  T: the value type of the slope - double, or Dual<NC> for the
// roll-out with sensitivities (SensCarry below)
template <int NX, class T = double>
struct Dopri5Carry {
  T k1[NX];           // slope at the current state (valid when have_k1)
  double h;           // step-size proposal (0: not chosen yet)
  double t;           // time since the start of the roll-out, at the start of the interval handed to dopri5_interval
  double t0;          // absolute time of the start of the roll-out (a time-variant functor is evaluated at t0 + t + ...)
  int status, n_acc, n_rej, n_rhs;
  bool have_k1;
};

template <int NX, class T>
HD void dopri5_init(Dopri5Carry<NX, T>& c, double h0) {
  c.h = h0 > 0.0 ? h0 : 0.0;
  c.t = c.t0 = 0.0;
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

// a vector whose entry i is formed where it is read (the error estimate of a step: kept as an array, the plain roll-out of a
// time-variant model took two registers more and lost a wave per SIMD)
template <class F>
struct Lazy {
  F f;
  HD auto operator[](int i) const { return f(i); }
};
template <class F>
HD Lazy<F> lazy(F f) { return {f}; }

// The norm of the pair and of the first-step estimate as a policy: `sumsq(v, a, b)` is the sum over the vector of
// (v / (atol + rtol max(|a|, |b|)))^2 - v an array or a Lazy - and `divisor()` the number of its components.  This one is the
// plain vector of NX doubles; the one of the sensitivities (SensNorm below) adds the columns' share over a team of lanes.
template <int NX>
struct PlainNorm {
  double rtol, atol;
  template <class V>
  HD double sumsq(const V& v, const double* a, const double* b) const {
    double s = 0.0;
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      const double q = v[i] / (atol + ::fmax(::fabs(a[i]), ::fabs(b[i])) * rtol);
      s += q * q;
    }
    return s;
  }
  HD double divisor() const { return NX; }
};

// scipy's select_initial_step (Hairer, Norsett, Wanner I, II.4) from the state x and the slope f0 there: the first step of a method
// whose local error behaves like h^(1 / expo) - 0.2 for the pair, 0.5 for order 1 - at most `bound`.  `slope_at(h, x1, f1)`
// evaluates the slope at the trial point x1 = x + h f0, h after the start, into f1 and answers whether it could (the trial point of
// a model with algebraic states needs a Newton solve of its own); where it could not, the first guess stands.  A non-finite
// estimate answers `bound`: the method's own step control then finds the step (or fails).
template <int NX, class T, class NORM, class F>
HD double select_initial_step(const NORM& norm, const T* x, const T* f0, double bound, double expo, F&& slope_at) {
  const double n = norm.divisor();
  const double d0 = ::sqrt(norm.sumsq(x, x, x) / n), d1 = ::sqrt(norm.sumsq(f0, x, x) / n);
  double h0 = (d0 < 1e-5 || d1 < 1e-5) ? 1e-6 : 0.01 * d0 / d1;
  h0 = ::fmin(h0, bound);
  T x1[NX], f1[NX];
#pragma unroll
  for (int i = 0; i < NX; ++i) x1[i] = x[i] + h0 * f0[i];
  double h = h0;
  if (slope_at(h0, x1, f1)) {
#pragma unroll
    for (int i = 0; i < NX; ++i) f1[i] = f1[i] - f0[i];
    const double d2 = ::sqrt(norm.sumsq(f1, x, x) / n) / h0;
    const double h1 = (d1 <= 1e-15 && d2 <= 1e-15) ? ::fmax(1e-6, h0 * 1e-3) : ::pow(0.01 / ::fmax(d1, d2), expo);
    h = ::fmin(::fmin(100.0 * h0, h1), bound);
  }
  return h > 0.0 ? h : bound;
}

// One sampling interval of length dt with the pair, in place in x, for the value type T (double, or Dual<NC>: the augmented system
// of the sensitivities) under the norm `norm` - the one implementation behind dopri5_interval and dopri5_sens_interval.  Every
// decision of a step (accept / reject, the factor, the loop exit, the two failures) reads `norm.sumsq` and values derived from it
// alone.  u, p: of type UP (doubles, or duals that carry their seeds).
template <class M, class T, class UP, class NORM>
HD int dopri5_core(Dopri5Carry<M::NX, T>& c, const NORM& norm, T* x, const UP* u, const UP* p, double dt, int max_steps) {
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
  constexpr bool TV = model_time_variant<M>::value;
  constexpr double C2 = 1.0 / 5, C3 = 3.0 / 10, C4 = 4.0 / 5, C5 = 8.0 / 9;
  const double n = norm.divisor();
  double ts = 0.0;   // absolute time at the start of this interval (time-variant functors only)
  if constexpr (TV) ts = c.t0 + c.t;
  auto f = [&](double at_t, const T* at, T* k) {
    model_ode_at<M>(at_t, at, u, p, dt, k);
    ++c.n_rhs;
  };
  if (c.status != SIM_OK) return c.status;
  if (!c.have_k1) {
    f(ts, x, c.k1);
    c.have_k1 = true;
  }
  if (!(c.h > 0.0))   // the first step of the roll-out
    c.h = select_initial_step<NX>(norm, x, c.k1, dt, 0.2, [&](double h0, const T* x1, T* f1) {
      f(ts + h0, x1, f1);
      return true;
    });
  double tl = 0.0;          // time inside this interval
  bool rejected = false;    // the previous attempt of the CURRENT step was rejected
  int attempts = 0;
  while (tl < dt) {
    if (attempts >= max_steps) return c.status = SIM_MAX_STEPS;
    if constexpr (TV) {
      if (c.h < 16.0 * EPS * ::fabs(ts + tl)) return c.status = SIM_STEP_TOO_SMALL;
    } else {
      if (c.h < 16.0 * EPS * ::fabs(c.t + tl)) return c.status = SIM_STEP_TOO_SMALL;
    }
    ++attempts;
    // clipped so that the sampling instant is hit exactly (a step that would leave a sliver of its own hundredth is stretched)
    const double rem = dt - tl;
    const bool last = 1.01 * c.h >= rem;
    const double h = last ? rem : c.h;
    T k2[NX], k3[NX], k4[NX], k5[NX], k6[NX], k7[NX], xi[NX], xn[NX];
    double tn = 0.0;   // absolute time at the start of this step
    if constexpr (TV) tn = ts + tl;
#pragma unroll
    for (int i = 0; i < NX; ++i) xi[i] = x[i] + h * (A21 * c.k1[i]);
    f(tn + C2 * h, xi, k2);
#pragma unroll
    for (int i = 0; i < NX; ++i) xi[i] = x[i] + h * (A31 * c.k1[i] + A32 * k2[i]);
    f(tn + C3 * h, xi, k3);
#pragma unroll
    for (int i = 0; i < NX; ++i) xi[i] = x[i] + h * (A41 * c.k1[i] + A42 * k2[i] + A43 * k3[i]);
    f(tn + C4 * h, xi, k4);
#pragma unroll
    for (int i = 0; i < NX; ++i) xi[i] = x[i] + h * (A51 * c.k1[i] + A52 * k2[i] + A53 * k3[i] + A54 * k4[i]);
    f(tn + C5 * h, xi, k5);
#pragma unroll
    for (int i = 0; i < NX; ++i) xi[i] = x[i] + h * (A61 * c.k1[i] + A62 * k2[i] + A63 * k3[i] + A64 * k4[i] + A65 * k5[i]);
    f(tn + h, xi, k6);
#pragma unroll
    for (int i = 0; i < NX; ++i) xn[i] = x[i] + h * (B1 * c.k1[i] + B3 * k3[i] + B4 * k4[i] + B5 * k5[i] + B6 * k6[i]);
    f(last ? ts + dt : tn + h, xn, k7);
    const auto e = lazy([&](int i) { return h * (E1 * c.k1[i] + E3 * k3[i] + E4 * k4[i] + E5 * k5[i] + E6 * k6[i] + E7 * k7[i]); });
    const double err = ::sqrt(norm.sumsq(e, x, xn) / n);   // the step's one value that may cross lanes
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

// Integrates dx/dt = f(x, u, p) - or f(c.t0 + c.t + tau, x, u, p), tau in [0, dt], for a time-variant functor - over one sampling
// interval of length dt, in place.  Returns c.status; on a failure x holds the state at the time the integration stopped (the
// caller discards it).  `max_steps` bounds the attempted steps of this call (the meaning of CasADi's `max_num_steps`: per
// integrator call).
template <class M>
HD int dopri5_interval(Dopri5Carry<M::NX>& c, double* x, const double* u, const double* p, double dt, double rtol, double atol,
                       int max_steps) {
  return dopri5_core<M>(c, PlainNorm<M::NX>{rtol, atol}, x, u, p, dt, max_steps);
}

// ---- variable-order implicit integration ----------------------------------------------------------------------------------
// `ndf_interval` - `bdf_interval` is it on dx/dt = f - is the variable-order (1..5) backward differentiation method of scipy's `BDF`
// (scipy/integrate/_ivp/bdf.py, common.py::select_initial_step), restated statement by statement - the NDF constants, the table of backward differences D with
// MAX_ORDER + 3 rows and its rescaling `change_D`, the simplified Newton iteration, the retry logic (a stale Jacobian is renewed
// before the step is halved; I - c J is factorised again whenever c = h / alpha[order] changes), the error estimate, the count of
// equal steps and the order selection - so that its step sequence can be compared with a solver everybody has.  What differs:
//   Jacobian     exact, from M::ode on Dual numbers (the tests hand scipy the analytic one)
//   linear algebra  LU with partial pivoting per lane; a vanishing or non-finite pivot and any non-finite Newton update count as
//                a Newton failure (scipy warns and goes on with inf / nan); every acceptance is written as a comparison that a
//                NaN fails
//   change_D     U^T (R^T D) row by row instead of (R U)^T D: the same product, another order of the additions
//   bounds       `max_steps` attempted steps per sampling instant; scipy has none
// What is indexed by the order or by a pivot row - D, the Jacobian, its factors, the permutation - lives in a store of
// `bdf_entries(NX)` doubles per instance that the caller provides: LDS on the device (entry e of lane l at [e * STRIDE + l]: one
// double per lane at consecutive addresses, a wave's 64-bit accesses fall into distinct banks whatever row each lane asks for),
// a plain array on the host.  Everything else is held in registers under compile-time indices.
constexpr int SIM_BDF = 2;   // HILO_SIM_BDF
constexpr int BDF_MAX_ORDER = 5, BDF_NEWTON_MAXITER = 4;
constexpr double BDF_MIN_FACTOR = 0.2, BDF_MAX_FACTOR = 10.0;
// Widest model the method is built for: (MAX_ORDER + 3) NX + 2 NX^2 + 2 NX doubles per lane in LDS, 64 lanes per workgroup - 104 KiB
// of the 160 KiB of a compute unit at 8 states, 150 KiB at 10.  With the dense synthetic right-hand side of DOPRI5_MAX_NX: 8
// states 425 registers and no scratch, 10 states all 512 and 132 bytes of scratch per lane.
constexpr int BDF_MAX_NX = 8;
constexpr int bdf_entries(int nx) { return (BDF_MAX_ORDER + 3) * nx + 2 * nx * nx + 2 * nx; }

constexpr double BDF_KAPPA[6] = {0.0, -0.1850, -1.0 / 9, -0.0823, -0.0415, 0.0};
constexpr double BDF_GAMMA[6] = {0.0, 1.0, 1.0 + 1.0 / 2, 1.0 + 1.0 / 2 + 1.0 / 3, 1.0 + 1.0 / 2 + 1.0 / 3 + 1.0 / 4,
                                 1.0 + 1.0 / 2 + 1.0 / 3 + 1.0 / 4 + 1.0 / 5};
// a table read under a run-time order: a sum of constants times 0 or 1 - exact, no table in memory and no branch (the chain of
// conditionals was compiled into nested divergent regions whose else-copies tools/check_exec_prologue.py reports)
#define HILO_BDF_PICK(k, EXPR)                                                                                                  \
  ((double)((k) <= 0) * EXPR(0) + (double)((k) == 1) * EXPR(1) + (double)((k) == 2) * EXPR(2) + (double)((k) == 3) * EXPR(3) + \
   (double)((k) == 4) * EXPR(4) + (double)((k) >= 5) * EXPR(5))
#define HILO_BDF_GAMMA_(k) BDF_GAMMA[k]
#define HILO_BDF_ALPHA_(k) ((1.0 - BDF_KAPPA[k]) * BDF_GAMMA[k])
#define HILO_BDF_ERRC_(k) (BDF_KAPPA[k] * BDF_GAMMA[k] + 1.0 / ((k) + 1))
HD double bdf_gamma(int k) { return HILO_BDF_PICK(k, HILO_BDF_GAMMA_); }
HD double bdf_alpha(int k) { return HILO_BDF_PICK(k, HILO_BDF_ALPHA_); }
HD double bdf_error_const(int k) { return HILO_BDF_PICK(k, HILO_BDF_ERRC_); }
#undef HILO_BDF_PICK
#undef HILO_BDF_GAMMA_
#undef HILO_BDF_ALPHA_
#undef HILO_BDF_ERRC_
// compute_R(order, 1)[k][j] = prod_{m = 1..k} (m - 1 - j) / m: upper triangular, the same entries for every order
constexpr double bdf_U(int k, int j) {
  double r = 1.0;
  for (int m = 1; m <= k; ++m) r *= (double)(m - 1 - j) / m;
  return r;
}

// the store of one instance: MP = lds_double* (device) or double* (host)
template <int NX, int STRIDE, class MP>
struct BdfMem {
  MP m;
  static constexpr int O_J = (BDF_MAX_ORDER + 3) * NX, O_LU = O_J + NX * NX, O_W = O_LU + NX * NX, O_PIV = O_W + NX;
  static_assert(O_PIV + NX == bdf_entries(NX), "bdf_entries and the layout of BdfMem disagree");
  HD decltype(auto) D(int r, int i) const { return m[(r * NX + i) * STRIDE]; }          // D [MAX_ORDER + 3][NX]
  HD decltype(auto) J(int i, int j) const { return m[(O_J + i * NX + j) * STRIDE]; }     // df/dx
  HD decltype(auto) LU(int i, int j) const { return m[(O_LU + i * NX + j) * STRIDE]; }   // factors of I - c J, rows permuted
  HD decltype(auto) W(int i) const { return m[(O_W + i) * STRIDE]; }                     // the right-hand side being permuted
  HD decltype(auto) PIV(int i) const { return m[(O_PIV + i) * STRIDE]; }                 // row exchanged with row i
};

// what one instance carries from one step (and, inputs held, from one sampling instant) to the next, next to its store
template <int NX>
struct BdfCarry {
  double t, t_bound;   // time since the start of the integration and its end (the roll-out's; with an input sequence the interval's)
  double t0;           // absolute time of the start of the integration (a time-variant functor is evaluated at t0 + t)
  double h;            // step size (scipy's h_abs)
  int order, n_equal;
  bool started;        // D, J and h belong to this integration
  bool have_lu;        // the factors in the store belong to the current c (scipy's LU is not None)
  int status, n_acc, n_rej, n_rhs, n_jac, n_lu;
};

template <int NX>
HD void bdf_init(BdfCarry<NX>& c, double t_bound) {
  c.t = c.t0 = 0.0;
  c.t_bound = t_bound;
  c.h = 0.0;
  c.order = 1;
  c.n_equal = 0;
  c.started = c.have_lu = false;
  c.status = SIM_OK;
  c.n_acc = c.n_rej = c.n_rhs = c.n_jac = c.n_lu = 0;
}
// a new integration from the state handed to the next bdf_interval (the inputs jumped: the difference history is void); the
// status and the counters go on, and so does t0: the caller moves it to the new start
template <int NX>
HD void bdf_restart(BdfCarry<NX>& c, double t_bound) {
  c.t = 0.0;
  c.t_bound = t_bound;
  c.started = c.have_lu = false;
}

// change_D: D[:order + 1] <- (R U)^T D[:order + 1] when the step size changes by `factor`
template <int NX, class MEM>
HD void bdf_change_D(const MEM& mem, int order, double factor) {
  constexpr int N = BDF_MAX_ORDER + 1;
#pragma unroll 1
  for (int ix = 0; ix < NX; ++ix) {
    double d[N], e[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
      const double v = mem.D(i, ix);
      d[i] = i <= order ? v : 0.0;
    }
    // e = R^T d with R = compute_R(order, factor), R[i][k] = prod_{m = 1..i} (m - 1 - factor k) / m: the leading block of the one
    // for MAX_ORDER, its columns built as they are used (a 6 x 6 table kept over the loop costs 72 registers)
#pragma unroll
    for (int k = 0; k < N; ++k) {
      double r = 1.0;
      e[k] = d[0];
#pragma unroll
      for (int i = 1; i < N; ++i) {
        r *= ((double)(i - 1) - factor * k) * (1.0 / i);
        e[k] += r * d[i];
      }
    }
#pragma unroll
    for (int j = 0; j < N; ++j) {
      double s = 0.0;
#pragma unroll
      for (int k = 0; k <= j; ++k) s += bdf_U(k, j) * e[k];
      if (j <= order) mem.D(j, ix) = s;
    }
  }
}

// df/dx at (t, x) into the store, CH columns per evaluation of M::ode on Dual<CH> (t: read by a time-variant functor only)
template <class M, class MEM>
HD void bdf_jacobian(const MEM& mem, const double* x, const double* u, const double* p, double dt, double t = 0.0) {
  constexpr int NX = M::NX, CH = NX < 4 ? NX : 4;
#pragma unroll
  for (int c0 = 0; c0 < NX; c0 += CH) {
    Dual<CH> xd[NX], fd[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      xd[i] = Dual<CH>(x[i]);
      if (i >= c0 && i < c0 + CH) xd[i].d[i - c0] = 1.0;
    }
    model_ode_at<M>(t, xd, u, p, dt, fd);
#pragma unroll
    for (int i = 0; i < NX; ++i)
#pragma unroll
      for (int q = 0; q < CH; ++q)
        if (c0 + q < NX) mem.J(i, c0 + q) = fd[i].d[q];
  }
}

// factors of I - c J with partial pivoting, in place in the store; false for a vanishing or non-finite pivot.  The loops over rows
// stay rolled: every operand is in the store under a run-time row anyway, and unrolled the compiler keeps the whole matrix in
// registers across the elimination (at 8 states 80 registers more, at 10 the difference between none and 132 bytes of scratch).
template <int NX, class MEM>
HD bool bdf_lu(const MEM& mem);
template <int NX, class MEM>
HD bool bdf_factor(const MEM& mem, double c) {
#pragma unroll 1
  for (int i = 0; i < NX; ++i)
    for (int j = 0; j < NX; ++j) mem.LU(i, j) = (i == j ? 1.0 : 0.0) - c * mem.J(i, j);
  return bdf_lu<NX>(mem);
}
// the elimination of bdf_factor on the matrix that stands in LU (shared with idas_factor below)
template <int NX, class MEM>
HD bool bdf_lu(const MEM& mem) {
#pragma unroll 1
  for (int k = 0; k < NX; ++k) {
    int piv = k;
    double best = ::fabs(mem.LU(k, k));
    for (int i = k + 1; i < NX; ++i) {
      const double a = ::fabs(mem.LU(i, k));
      if (a > best) { best = a; piv = i; }
    }
    if (!(best > 0.0 && best < INFINITY)) return false;
    mem.PIV(k) = (double)piv;
    if (piv != k)
      for (int j = 0; j < NX; ++j) {
        const double a = mem.LU(k, j), b = mem.LU(piv, j);
        mem.LU(k, j) = b;
        mem.LU(piv, j) = a;
      }
    const double inv = 1.0 / mem.LU(k, k);
    for (int i = k + 1; i < NX; ++i) {
      const double l = mem.LU(i, k) * inv;
      mem.LU(i, k) = l;
      for (int j = k + 1; j < NX; ++j) mem.LU(i, j) -= l * mem.LU(k, j);
    }
  }
  return true;
}

// b <- (I - c J)^-1 b with the factors of bdf_factor
template <int NX, class MEM>
HD void bdf_solve(const MEM& mem, double* b) {
#pragma unroll
  for (int i = 0; i < NX; ++i) mem.W(i) = b[i];
  for (int k = 0; k < NX; ++k) {
    const int piv = (int)mem.PIV(k);
    if (piv != k) {
      const double a = mem.W(k), q = mem.W(piv);
      mem.W(k) = q;
      mem.W(piv) = a;
    }
  }
#pragma unroll
  for (int i = 0; i < NX; ++i) b[i] = mem.W(i);
#pragma unroll
  for (int i = 1; i < NX; ++i)
#pragma unroll
    for (int j = 0; j < i; ++j) b[i] -= mem.LU(i, j) * b[j];
#pragma unroll
  for (int i = NX - 1; i >= 0; --i) {
#pragma unroll
    for (int j = i + 1; j < NX; ++j) b[i] -= mem.LU(i, j) * b[j];
    b[i] /= mem.LU(i, i);
  }
}

// the end of a start (bdf_start, idas_start): the difference table of order 1 from the state y and its slope yp, c.h chosen
template <int N, class MEM>
HD void ndf_begin(BdfCarry<N>& c, const MEM& mem, const double* y, const double* yp) {
  for (int r = 0; r < BDF_MAX_ORDER + 3; ++r)
#pragma unroll
    for (int i = 0; i < N; ++i) mem.D(r, i) = r == 0 ? y[i] : (r == 1 ? yp[i] * c.h : 0.0);
  c.t = 0.0;
  c.order = 1;
  c.n_equal = 0;
  c.have_lu = false;
  c.started = true;
}

// The variable-order step loop, once, for a system policy SYS - OdeSystem below, DaeSystem in the next section - that supplies
// what differs between dx/dt = f and the DAE in [x; z]:
//   N, ND        the length of the vector and the number of its differential rows (residual c f - psi - d; the others: -f)
//   TV, time     whether the equations name the time, and the absolute time of the integration's t handed to rhs and jacobian
//   rhs, jacobian, factor, change_D   the right-hand side F(t, y), dF/dy into the store, the factors of the Newton matrix for
//                c = h / alpha[order], the rescaling of the difference table
//   start        the set-up of an integration on the first call after bdf_init / bdf_restart
//   finish       from the interpolated vector at t_target to the value handed out; false: SIM_IC_FAILED
// Advances until the integration time reaches t_target (<= c.t_bound) and reads the vector at t_target off the interpolant of the
// difference table (scipy's BdfDenseOutput) into y.  A step may pass t_target - and later targets, which the next calls then only
// interpolate; the end of the integration alone clips a step.  Returns c.status; on a failure y is left as it was (the caller
// discards it).  `max_steps` bounds the attempted steps of this call, h0 > 0 is the first step.
template <class SYS, class MEM>
HD int ndf_interval(const SYS& sys, BdfCarry<SYS::N>& c, const MEM& mem, double* y_out, double t_target, double rtol, double atol,
                    double h0, int max_steps) {
  constexpr int N = SYS::N, ND = SYS::ND;
  constexpr double EPS = 2.220446049250313e-16;
  if (c.status != SIM_OK) return c.status;
  if (!c.started && sys.start(c, mem, y_out, rtol, atol, h0) != SIM_OK) return c.status;
  const double newton_tol = ::fmax(10.0 * EPS / rtol, ::fmin(0.03, ::sqrt(rtol)));
  int attempts = 0;
  while (c.t < t_target) {   // one pass: scipy's _step_impl
    double min_step;
    if constexpr (SYS::TV) {
      const double ta = sys.time(c, c.t);
      min_step = 10.0 * ::fabs(::nextafter(ta, INFINITY) - ta);
    } else {
      min_step = 10.0 * (::nextafter(c.t, INFINITY) - c.t);
    }
    double h = c.h;
    int order = c.order;
    if (h < min_step) {
      sys.change_D(mem, order, min_step / h);
      h = min_step;
      c.n_equal = 0;
    }
    bool current_jac = false, accepted = false;
    double t_new = c.t, safety = 0.0, error_norm = 0.0;
    double scale[N], d[N];
    while (!accepted) {
      if (attempts >= max_steps) return c.status = SIM_MAX_STEPS;
      if (!(h >= min_step)) return c.status = SIM_STEP_TOO_SMALL;
      ++attempts;
      t_new = c.t + h;
      if (t_new > c.t_bound) {
        t_new = c.t_bound;
        sys.change_D(mem, order, (t_new - c.t) / h);
        c.n_equal = 0;
        c.have_lu = false;
      }
      h = t_new - c.t;
      double y_predict[N], psi[N], y[N];
#pragma unroll
      for (int i = 0; i < N; ++i) {
        y_predict[i] = mem.D(0, i);
        psi[i] = 0.0;
      }
      for (int j = 1; j <= order; ++j) {
        const double g = bdf_gamma(j);
#pragma unroll
        for (int i = 0; i < N; ++i) {
          const double v = mem.D(j, i);
          y_predict[i] += v;
          psi[i] += v * g;
        }
      }
      const double alpha = bdf_alpha(order);
#pragma unroll
      for (int i = 0; i < N; ++i) {
        scale[i] = atol + rtol * ::fabs(y_predict[i]);
        psi[i] /= alpha;
      }
      const double cc = h / alpha;
      bool converged = false;
      int n_iter = 0;
      while (!converged) {
        if (!c.have_lu) {
          c.have_lu = sys.factor(mem, cc);
          ++c.n_lu;
        }
        if (c.have_lu) {   // solve_bdf_system
          double dy_norm_old = -1.0;   // (none yet)
#pragma unroll
          for (int i = 0; i < N; ++i) {
            d[i] = 0.0;
            y[i] = y_predict[i];
          }
#pragma unroll 1
          for (int k = 0; k < BDF_NEWTON_MAXITER; ++k) {
            n_iter = k + 1;
            double f[N];
            sys.rhs(sys.time(c, t_new), y, f);
            ++c.n_rhs;
            bool finite = true;
#pragma unroll
            for (int i = 0; i < N; ++i) finite = finite && ::fabs(f[i]) < INFINITY;
            if (!finite) break;
#pragma unroll
            for (int i = 0; i < N; ++i) f[i] = i < ND ? cc * f[i] - psi[i] - d[i] : -f[i];
            bdf_solve<N>(mem, f);   // f: dy
            const double dy_norm = dopri5_rms<N>(f, scale);
            if (!(dy_norm < INFINITY)) break;
            const bool have_rate = dy_norm_old >= 0.0;
            const double rate = dy_norm / dy_norm_old;
            if (have_rate && !(rate < 1.0 && ::pow(rate, (double)(BDF_NEWTON_MAXITER - k)) / (1.0 - rate) * dy_norm <= newton_tol)) break;
#pragma unroll
            for (int i = 0; i < N; ++i) {
              y[i] += f[i];
              d[i] += f[i];
            }
            if (dy_norm == 0.0 || (have_rate && rate / (1.0 - rate) * dy_norm < newton_tol)) {
              converged = true;
              break;
            }
            dy_norm_old = dy_norm;
          }
        }
        if (!converged) {
          if (current_jac) break;
          sys.jacobian(mem, sys.time(c, t_new), y_predict);
          ++c.n_jac;
          c.have_lu = false;
          current_jac = true;
        }
      }
      if (!converged) {
        h *= 0.5;
        sys.change_D(mem, order, 0.5);
        c.n_equal = 0;
        c.have_lu = false;
        ++c.n_rej;
        continue;
      }
      safety = 0.9 * (2 * BDF_NEWTON_MAXITER + 1) / (2 * BDF_NEWTON_MAXITER + n_iter);
      const double ec = bdf_error_const(order);
      double s = 0.0;
#pragma unroll
      for (int i = 0; i < N; ++i) {
        scale[i] = atol + rtol * ::fabs(y[i]);
        const double q = ec * d[i] / scale[i];
        s += q * q;
      }
      error_norm = ::sqrt(s / N);
      if (!(error_norm <= 1.0)) {   // (a non-finite estimate fails the comparison: a rejection)
        const double factor = ::fmax(BDF_MIN_FACTOR, safety * ::pow(error_norm, -1.0 / (order + 1)));
        h *= factor;
        sys.change_D(mem, order, factor);
        c.n_equal = 0;   // the factors stay: the iteration had no trouble converging
        ++c.n_rej;
      } else {
        accepted = true;
      }
    }
    ++c.n_equal;
    ++c.n_acc;
    c.t = t_new;
    c.h = h;
    // D^{j+1} y_n = D^j y_n - D^j y_{n-1}, d = D^{order+1} y_n
#pragma unroll
    for (int i = 0; i < N; ++i) {
      mem.D(order + 2, i) = d[i] - mem.D(order + 1, i);
      mem.D(order + 1, i) = d[i];
    }
    for (int j = order; j >= 0; --j)
#pragma unroll
      for (int i = 0; i < N; ++i) mem.D(j, i) += mem.D(j + 1, i);
    if (c.n_equal < order + 1) continue;
    double sm = 0.0, sp = 0.0;
    {
      const double em = bdf_error_const(order - 1), ep = bdf_error_const(order + 1);
#pragma unroll
      for (int i = 0; i < N; ++i) {
        const double qm = em * mem.D(order, i) / scale[i], qp = ep * mem.D(order + 2, i) / scale[i];
        sm += qm * qm;
        sp += qp * qp;
      }
    }
    const double error_m_norm = order > 1 ? ::sqrt(sm / N) : INFINITY;
    const double error_p_norm = order < BDF_MAX_ORDER ? ::sqrt(sp / N) : INFINITY;
    const double fm = ::pow(error_m_norm, -1.0 / order), f0 = ::pow(error_norm, -1.0 / (order + 1)),
                 fp = ::pow(error_p_norm, -1.0 / (order + 2));
    double fmax_ = fm;   // argmax: the first of equal ones
    int delta = -1;
    if (f0 > fmax_) { fmax_ = f0; delta = 0; }
    if (fp > fmax_) { fmax_ = fp; delta = 1; }
    if (order + delta < 1) delta = 0;   // (order 1: fm is 0 and can only win against two zeros)
    order += delta;
    c.order = order;
    const double factor = ::fmin(BDF_MAX_FACTOR, safety * fmax_);
    c.h *= factor;
    sys.change_D(mem, order, factor);
    c.n_equal = 0;
    c.have_lu = false;
  }
  // BdfDenseOutput at t_target
  double acc[N];
#pragma unroll
  for (int i = 0; i < N; ++i) acc[i] = 0.0;
  double prod = 1.0;
  for (int j = 0; j < c.order; ++j) {
    prod *= (t_target - (c.t - c.h * j)) / (c.h * (1 + j));
#pragma unroll
    for (int i = 0; i < N; ++i) acc[i] += mem.D(j + 1, i) * prod;
  }
#pragma unroll
  for (int i = 0; i < N; ++i) acc[i] += mem.D(0, i);
  if (!sys.finish(acc)) return c.status = SIM_IC_FAILED;
#pragma unroll
  for (int i = 0; i < N; ++i) y_out[i] = acc[i];
  return c.status;
}

// The start of an integration of dx/dt = f from x: the slope and the Jacobian there, the first step (h0 > 0, or
// select_initial_step with order = 1) and the difference table.  Called by bdf_interval on the first call after bdf_init /
// bdf_restart.  Returns c.status.
template <class M, class MEM>
HD int bdf_start(BdfCarry<M::NX>& c, const MEM& mem, const double* x, const double* u, const double* p, double dt, double rtol,
                 double atol, double h0) {
  constexpr int NX = M::NX;
  if (c.status != SIM_OK || c.started) return c.status;
  double f0[NX];
  model_ode_at<M>(c.t0, x, u, p, dt, f0);
  ++c.n_rhs;
  bdf_jacobian<M>(mem, x, u, p, dt, c.t0);
  ++c.n_jac;
  if (h0 > 0.0)
    c.h = ::fmin(h0, c.t_bound);
  else   // (a non-finite estimate answers t_bound: the Newton iteration of the step fails and finds the step, or gives up)
    c.h = select_initial_step<NX>(PlainNorm<NX>{rtol, atol}, x, f0, c.t_bound, 0.5, [&](double hh, const double* x1, double* f1) {
      model_ode_at<M>(c.t0 + hh, x1, u, p, dt, f1);
      ++c.n_rhs;
      return true;
    });
  ndf_begin(c, mem, x, f0);
  return c.status;
}

// dx/dt = f(x, u, p) - or f(c.t0 + t, x, u, p) for a time-variant functor - as a system of ndf_interval
template <class M>
struct OdeSystem {
  static constexpr int N = M::NX, ND = M::NX;   // every row is differential: the residual's selection folds at compile time
  static constexpr bool TV = model_time_variant<M>::value;
  const double *u, *p;
  double dt;
  HD double time(const BdfCarry<N>& c, double t) const { return c.t0 + t; }   // (read by a time-variant functor only)
  HD void rhs(double t, const double* y, double* f) const { model_ode_at<M>(t, y, u, p, dt, f); }
  template <class MEM>
  HD void jacobian(const MEM& mem, double t, const double* y) const { bdf_jacobian<M>(mem, y, u, p, dt, t); }
  template <class MEM>
  HD bool factor(const MEM& mem, double cc) const { return bdf_factor<N>(mem, cc); }
  // deliberately inlined at its five sites, where DaeSystem calls one function: the kernels of this path are the ones they were
  template <class MEM>
  HD void change_D(const MEM& mem, int order, double factor) const { bdf_change_D<N>(mem, order, factor); }
  template <class MEM>
  HD int start(BdfCarry<N>& c, const MEM& mem, const double* x, double rtol, double atol, double h0) const {
    return bdf_start<M>(c, mem, x, u, p, dt, rtol, atol, h0);
  }
  HD bool finish(double*) const { return true; }   // the interpolated state is the answer
};

// ndf_interval on dx/dt = f: on the first call after bdf_init / bdf_restart x is the initial state, afterwards the state at t_target.
template <class M, class MEM>
HD int bdf_interval(BdfCarry<M::NX>& c, const MEM& mem, double* x, const double* u, const double* p, double dt, double t_target,
                    double rtol, double atol, double h0, int max_steps) {
  return ndf_interval(OdeSystem<M>{u, p, dt}, c, mem, x, t_target, rtol, atol, h0, max_steps);
}

// ---- variable-order implicit integration of a model with algebraic states ---------------------------------------------------
// `idas_interval` is `ndf_interval` on the semi-explicit index-1 DAE  dx/dt = f(x, z, u, p),  0 = g(x, z, u, p)  IN THE COMBINED
// VECTOR w = [x; z] (N = NX + NZ entries), where the reference integrates such a model with IDAS: the NDF constants, the difference
// table, change_D, the retry logic, the order selection and the dense output are the one step loop above under DaeSystem, on
// the same store (BdfMem<N>, bdf_entries(N) doubles per instance).  With the mass matrix M = diag(I_NX, 0) and c = h / alpha[order]
// the corrector solves M (psi + d) = c F(w_predict + d), F = [f; g]; the algebraic rows are divided by c.  What differs:
//   Newton system   rows (I - c f_x, -c f_z) with residual c f - psi_x - d_x, rows (g_x, g_z) with residual -g: a small step leaves
//                no rows of size c for the pivot search (idas_factor; the elimination and bdf_solve are shared)
//   Jacobian     M::ode_z and M::alg on Dual<CH> seeded over the N columns of [x; z], ceil(N / 4) evaluations; neither dae_solve nor
//                alg_jz.  A right-hand side is one ode_z and one alg in doubles; n_rhs counts such pairs
//   tests        predictor, error test and Newton convergence test over all N components, scale = atol + rtol |w| (IDAS's default,
//                suppress_algebraic off)
//   consistent start   at the first step and at every restart z solves g(x, z, u, p) = 0 by Newton's method from the value it is
//                handed (idas_newton_z: at most IDAS_IC_MAXITER sweeps, the exit test of dae_solve), then x' = f and
//                z' = -g_z^-1 g_x f, so that D[1] = h w' holds for both parts; no convergence, a singular g_z or a non-finite
//                value end the instance with SIM_IC_FAILED.  The first step is select_initial_step on the differential states
//                through the reduced right-hand side: the trial point x + h0 f0 gets a Newton solve of its own for z
//   sampling instants   x and z are read off the interpolant; z is then corrected by Newton sweeps on g(x, z) = 0 from the
//                interpolated value until the residual is at round-off: what the caller receives is a consistent pair (the
//                integrator's own state is not touched by that)
// The sweeps of idas_newton_z evaluate `alg` on dual numbers seeded over z (value and g_z at once); they are not counted in n_rhs.
constexpr int SIM_IDAS = 3;   // HILO_SIM_IDAS
constexpr int IDAS_IC_MAXITER = 40;

// J r' = r for a matrix of NZ x NZ entries held in registers, by Gaussian elimination with partial pivoting under static indices
// (conditional swaps, as in dae_solve); false for a vanishing or non-finite pivot
template <int NZ>
HD bool idas_dense_solve(double* J, double* r) {
  bool ok = true;
#pragma unroll
  for (int c = 0; c < NZ; ++c) {
#pragma unroll
    for (int q = c + 1; q < NZ; ++q) {
      if (::fabs(J[q * NZ + c]) > ::fabs(J[c * NZ + c])) {
#pragma unroll
        for (int j = c; j < NZ; ++j) { const double t = J[c * NZ + j]; J[c * NZ + j] = J[q * NZ + j]; J[q * NZ + j] = t; }
        const double t = r[c]; r[c] = r[q]; r[q] = t;
      }
    }
    const double piv = ::fabs(J[c * NZ + c]);
    ok = ok && piv > 0.0 && piv < INFINITY;
    const double ip = 1.0 / J[c * NZ + c];
#pragma unroll
    for (int q = c + 1; q < NZ; ++q) {
      const double f = J[q * NZ + c] * ip;
#pragma unroll
      for (int j = c + 1; j < NZ; ++j) J[q * NZ + j] -= f * J[c * NZ + j];
      r[q] -= f * r[c];
    }
  }
#pragma unroll
  for (int c = NZ - 1; c >= 0; --c) {
    double acc = r[c];
#pragma unroll
    for (int j = c + 1; j < NZ; ++j) acc -= J[c * NZ + j] * r[j];
    r[c] = acc / J[c * NZ + c];
  }
  return ok;
}

// Newton's method on g(x, z, u, p) = 0 for z, in place, from the z it is handed: value and dg/dz of a sweep from `alg` on dual
// numbers seeded over z.  Ends like dae_solve - after the second sweep that found the residual at round-off, 1e-13 (1 + |z|) - and
// answers false when IDAS_IC_MAXITER sweeps did not get there, for a singular dg/dz and for a non-finite value.
template <class M>
HD bool idas_newton_z(const double* x, double* z, const double* u, const double* p) {
  constexpr int NX = M::NX, NZ = M::NZ, NU = M::NU, CH = NZ < 4 ? NZ : 4;
  int done = 0;
  bool ok = true;
#pragma unroll 1
  for (int it = 0; it < IDAS_IC_MAXITER; ++it) {
    // No lane leaves the loop on its own: on the device the exit is a vote of the wave, and a lane that is done -
    // converged or failed - no longer changes its z, so its result does not depend on how long its neighbours go on.
    const bool active = ok && done < 2;
#if defined(__HIP_DEVICE_COMPILE__)
    if (!__any((int)active)) break;
#else
    if (!active) break;
#endif
    double r[NZ], J[NZ * NZ];
#pragma unroll
    for (int c0 = 0; c0 < NZ; c0 += CH) {
      Dual<CH> xd[NX], zd[NZ], ud[NU > 0 ? NU : 1], gd[NZ];
#pragma unroll
      for (int i = 0; i < NX; ++i) xd[i] = Dual<CH>(x[i]);
#pragma unroll
      for (int i = 0; i < NU; ++i) ud[i] = Dual<CH>(u[i]);
#pragma unroll
      for (int i = 0; i < NZ; ++i) {
        zd[i] = Dual<CH>(z[i]);
        if (i >= c0 && i < c0 + CH) zd[i].d[i - c0] = 1.0;
      }
      M::alg(xd, zd, ud, p, gd);
#pragma unroll
      for (int i = 0; i < NZ; ++i) {
        r[i] = gd[i].v;
#pragma unroll
        for (int q = 0; q < CH; ++q)
          if (c0 + q < NZ) J[i * NZ + c0 + q] = gd[i].d[q];
      }
    }
    double rmax = 0.0, zmax = 0.0;
    bool good = true;
#pragma unroll
    for (int i = 0; i < NZ; ++i) {
      rmax = ::fmax(rmax, ::fabs(r[i]));
      zmax = ::fmax(zmax, ::fabs(z[i]));
      good = good && ::fabs(r[i]) < INFINITY;
    }
    good = idas_dense_solve<NZ>(J, r) && good;
#pragma unroll
    for (int i = 0; i < NZ; ++i) good = good && ::fabs(z[i] - r[i]) < INFINITY;
#pragma unroll
    for (int i = 0; i < NZ; ++i) z[i] = active && good ? z[i] - r[i] : z[i];
    ok = active ? good : ok;
    done += (int)(active && good && rmax <= 1e-13 * (1.0 + zmax));   // the values had converged before this sweep
  }
  return ok && done >= 2;
}

// [f; g] at w = [x; z] in doubles: one right-hand side
template <class M>
HD void idas_rhs(const double* w, const double* u, const double* p, double* F) {
  M::ode_z(w, w + M::NX, u, p, F);
  M::alg(w, w + M::NX, u, p, F + M::NX);
}

// d[f; g] / d[x; z] at w into the store, CH columns per evaluation of M::ode_z and M::alg on Dual<CH>
template <class M, class MEM>
HD void idas_jacobian(const MEM& mem, const double* w, const double* u, const double* p) {
  constexpr int NX = M::NX, NZ = M::NZ, NU = M::NU, N = NX + NZ, CH = N < 4 ? N : 4;
#pragma unroll
  for (int c0 = 0; c0 < N; c0 += CH) {
    Dual<CH> wd[N], ud[NU > 0 ? NU : 1], Fd[N];
#pragma unroll
    for (int i = 0; i < N; ++i) {
      wd[i] = Dual<CH>(w[i]);
      if (i >= c0 && i < c0 + CH) wd[i].d[i - c0] = 1.0;
    }
#pragma unroll
    for (int i = 0; i < NU; ++i) ud[i] = Dual<CH>(u[i]);
    M::ode_z(wd, wd + NX, ud, p, Fd);
    M::alg(wd, wd + NX, ud, p, Fd + NX);
#pragma unroll
    for (int i = 0; i < N; ++i)
#pragma unroll
      for (int q = 0; q < CH; ++q)
        if (c0 + q < N) mem.J(i, c0 + q) = Fd[i].d[q];
  }
}

// factors of [I - c f_x, -c f_z; g_x, g_z] (the sibling of bdf_factor: the algebraic rows are not scaled by c)
template <int NX, int NZ, class MEM>
HD bool idas_factor(const MEM& mem, double c) {
  constexpr int N = NX + NZ;
#pragma unroll 1
  for (int i = 0; i < N; ++i)
    for (int j = 0; j < N; ++j) mem.LU(i, j) = i < NX ? (i == j ? 1.0 : 0.0) - c * mem.J(i, j) : mem.J(i, j);
  return bdf_lu<N>(mem);
}

// The consistent start of an integration from (x, z-guess) in w: z <- the root of g, the Jacobian at the consistent point, w', the
// first step and the difference table.  Called by idas_interval on the first call after bdf_init / bdf_restart; the roll-out calls
// it itself at row 0, whose z it records.  Returns c.status (SIM_OK or SIM_IC_FAILED).
template <class M, class MEM>
HD int idas_start(BdfCarry<M::NX + M::NZ>& c, const MEM& mem, double* w, const double* u, const double* p, double rtol, double atol,
                  double h0) {
  constexpr int NX = M::NX, NZ = M::NZ, N = NX + NZ;
  if (c.status != SIM_OK || c.started) return c.status;
  if (!idas_newton_z<M>(w, w + NX, u, p)) return c.status = SIM_IC_FAILED;
  double wp[N];   // [x'; z']
  idas_rhs<M>(w, u, p, wp);
  ++c.n_rhs;
  idas_jacobian<M>(mem, w, u, p);
  ++c.n_jac;
  {
    double Jz[NZ * NZ];
#pragma unroll
    for (int a = 0; a < NZ; ++a) {
      double s = 0.0;
#pragma unroll
      for (int j = 0; j < NX; ++j) s += mem.J(NX + a, j) * wp[j];
      wp[NX + a] = -s;
#pragma unroll
      for (int q = 0; q < NZ; ++q) Jz[a * NZ + q] = mem.J(NX + a, NX + q);
    }
    bool ok = idas_dense_solve<NZ>(Jz, wp + NX);
#pragma unroll
    for (int i = 0; i < N; ++i) ok = ok && ::fabs(wp[i]) < INFINITY;
    if (!ok) return c.status = SIM_IC_FAILED;
  }
  if (h0 > 0.0)
    c.h = ::fmin(h0, c.t_bound);
  else   // select_initial_step with order = 1 on dx/dt = f(x, zeta(x)): the norms run over the differential states
    c.h = select_initial_step<NX>(PlainNorm<NX>{rtol, atol}, w, wp, c.t_bound, 0.5, [&](double, const double* x1, double* f1) {
      double w1[N], F1[N];
#pragma unroll
      for (int i = 0; i < N; ++i) w1[i] = i < NX ? x1[i] : w[i];
      if (!idas_newton_z<M>(w1, w1 + NX, u, p)) return false;   // the algebraic equations have no root at the trial point
      idas_rhs<M>(w1, u, p, F1);
      ++c.n_rhs;
#pragma unroll
      for (int i = 0; i < NX; ++i) f1[i] = F1[i];
      return true;
    });
  ndf_begin(c, mem, w, wp);
  return c.status;
}

// bdf_change_D as ONE function of the kernel instead of five inlined copies (the five copies' registers are what pushed the widest
// models' kernels into live-range splits at the loop exits).  Not `HD`: that macro forces inlining.
template <int N, class MEM>
__host__ __device__ __attribute__((noinline)) void idas_change_D(MEM mem, int order, double factor) {
  bdf_change_D<N>(mem, order, factor);
}

// the DAE in w = [x; z] as a system of ndf_interval (autonomous: a time-variant DAE is not built)
template <class M>
struct DaeSystem {
  static constexpr int NX = M::NX, NZ = M::NZ, N = NX + NZ, ND = NX;
  static constexpr bool TV = false;
  const double *u, *p;
  HD double time(const BdfCarry<N>&, double t) const { return t; }   // (not read)
  HD void rhs(double, const double* w, double* F) const { idas_rhs<M>(w, u, p, F); }   // one pair; n_rhs counts pairs
  template <class MEM>
  HD void jacobian(const MEM& mem, double, const double* w) const { idas_jacobian<M>(mem, w, u, p); }
  template <class MEM>
  HD bool factor(const MEM& mem, double cc) const { return idas_factor<NX, NZ>(mem, cc); }
  // deliberately ONE non-inlined function for the five sites, where OdeSystem inlines: see idas_change_D
  template <class MEM>
  HD void change_D(const MEM& mem, int order, double factor) const { idas_change_D<N>(mem, order, factor); }
  template <class MEM>
  HD int start(BdfCarry<N>& c, const MEM& mem, double* w, double rtol, double atol, double h0) const {
    return idas_start<M>(c, mem, w, u, p, rtol, atol, h0);
  }
  // z of the interpolated pair onto g(x, z) = 0 (sweeps not counted in n_rhs; the integrator's own state is not touched)
  HD bool finish(double* w) const { return idas_newton_z<M>(w, w + NX, u, p); }
};

// ndf_interval on the DAE: advances until the integration time reaches t_target (<= c.t_bound) and reads w = [x; z] at t_target off
// the interpolant, z corrected onto g(x, z) = 0.  On the first call after bdf_init / bdf_restart w holds the initial x and the
// start of the Newton iteration for z.  Returns c.status; on a failure w is left as it was (the caller discards it).  The correction
// of z at t_target is held to the exit test of the consistent start: where its sweeps do not bring the residual to round-off - a
// badly scaled g, a singular dg/dz on the way - the instance ends with SIM_IC_FAILED at THAT instant, whichever it is.  The other
// arguments: bdf_interval's.
template <class M, class MEM>
HD int idas_interval(BdfCarry<M::NX + M::NZ>& c, const MEM& mem, double* w, const double* u, const double* p, double t_target,
                     double rtol, double atol, double h0, int max_steps) {
  return ndf_interval(DaeSystem<M>{u, p}, c, mem, w, t_target, rtol, atol, h0, max_steps);
}

constexpr int ROLLOUT_TPB = 64;   // one wave per workgroup: a slow instance holds back 63 others, not 255

// ---- what the roll-out bodies below and the closed loop (hilo_pid.h::pid_loop_instance) share ---------------------------------
// the row [u; p] of interval k and instance b into upv (strides: see rollout_body)
template <class M>
HD void rollout_load_up(const double* __restrict__ up, int64_t up_step, int64_t up_stride, int k, int64_t b, double* upv) {
  const double* src = up + (int64_t)k * up_step + b * up_stride;
#pragma unroll
  for (int i = 0; i < M::NU + M::NP; ++i) upv[i] = src[i];
}

// stats [batch][4] (or null) of instance b from its carry
template <class C>
HD void rollout_write_stats(int* __restrict__ stats, int64_t b, const C& c) {
  if (stats == nullptr) return;
  stats[b * 4 + 0] = c.status;
  stats[b * 4 + 1] = c.n_acc;
  stats[b * 4 + 2] = c.n_rej;
  stats[b * 4 + 3] = c.n_rhs;
}

// The plant over one sampling interval that starts at tk, in place in x: the handle's map or the pair, chosen by METHOD (SIM_MAP /
// SIM_DOPRI5 builds that path alone, -1 chooses by sp.method at run time).  The pair is built for continuous models up to
// DOPRI5_MAX_NX states - the host refuses the others - and carries its state in PlantCarry.  False: the integration failed.
template <class M>
constexpr bool plant_adaptive = !M::DISCRETE && M::NX <= DOPRI5_MAX_NX;
template <class M>
using PlantCarry = Dopri5Carry<plant_adaptive<M> ? M::NX : 1>;
template <class M, int METHOD, class KP>
HD bool plant_interval(const KP& kp, const SimParams& sp, PlantCarry<M>& c, double* x, const double* u, const double* p, double tk) {
  constexpr int NX = M::NX;
  bool ok = true;
  if (METHOD == SIM_DOPRI5 || (METHOD < 0 && sp.method == SIM_DOPRI5)) {
    if constexpr (plant_adaptive<M> && METHOD != SIM_MAP) ok = dopri5_interval<M>(c, x, u, p, kp.dt, sp.rtol, sp.atol, sp.max_steps) == SIM_OK;
  } else if constexpr (METHOD != SIM_DOPRI5) {
    double xo[NX];
    if (kp.continuous && !M::DISCRETE) model_step<M>(4, kp.n_sub, x, u, p, kp.dt, xo, NoExt(), tk);
    else model_step<M>(kp.erk_order, kp.n_sub, x, u, p, kp.dt, xo, NoExt(), tk);
#pragma unroll
    for (int i = 0; i < NX; ++i) x[i] = xo[i];
  }
  return ok;
}

// One instance per lane.  X [steps + 1][batch][NX] (row 0: x0), Y [steps][batch][NY] or null, stats [batch][4] (status, accepted,
// rejected, right-hand-side evaluations) or null; up: rows [u; p] of instance b at up + k up_step + b up_stride (up_step 0: held
// over the roll-out, up_stride 0: shared by the batch).  sp.method SIM_MAP: the map of the handle - the statements of pf_body
// (hilo_kf_kernel.h), what Model.step computes; SIM_DOPRI5: the pair above (continuous models up to DOPRI5_MAX_NX states - the host
// refuses the others).  The lanes of a wave run their own step sequences (a lane that rejects recomputes while its neighbours
// commit, a lane that has reached the sampling instant idles until the slowest has: the divergent loop runs while any lane is
// active); no value crosses lanes, so an instance's result does not depend on the instances it shares the wave with.  An
// instance that fails (SIM_MAX_STEPS, SIM_STEP_TOO_SMALL) gets NaN for the sampling instant it did not reach and every later one.
// METHOD: SIM_MAP / SIM_DOPRI5 builds that path alone (the library's kernels: each with the registers of its own path), -1 chooses
// by sp.method at run time between those two (the one kernel of a run-time compiled model that serves both).  SIM_BDF is a kernel
// of its own in either case (rollout_bdf_body below): it needs `lds`, bdf_entries(NX) * ROLLOUT_TPB doubles of the workgroup.
// t0: the time of row 0 of X, one value for the batch; read for a time-variant functor only (the header's section on time).
// hc [batch] or null (the host passes it with SIM_DOPRI5 only): the step-size proposal of each instance, taken over where positive
// and written back at the end.  With the slope at the start recomputed at the same time and state it is all the pair carries across
// a sampling instant, so a roll-out continued in a second launch takes the steps that one launch would have taken.
template <class M, class KP>
__device__ __forceinline__ void rollout_bdf_body(const KP& kp, const SimParams& sp, int64_t batch, int steps,
                                                 const double* __restrict__ x0, const double* __restrict__ up, int64_t up_stride,
                                                 int64_t up_step, double* __restrict__ X, double* __restrict__ Y,
                                                 int* __restrict__ stats, lds_double* lds, double t0 = 0.0);

template <class M, int METHOD = -1, class KP>
__device__ __forceinline__ void rollout_body(const KP& kp, const SimParams& sp, int64_t batch, int steps,
                                             const double* __restrict__ x0, const double* __restrict__ up, int64_t up_stride,
                                             int64_t up_step, double* __restrict__ X, double* __restrict__ Y,
                                             int* __restrict__ stats, lds_double* lds = nullptr, double t0 = 0.0,
                                             double* __restrict__ hc = nullptr) {
  if constexpr (METHOD == SIM_BDF) {
    rollout_bdf_body<M>(kp, sp, batch, steps, x0, up, up_stride, up_step, X, Y, stats, lds, t0);
    return;
  }
  constexpr int NX = M::NX, NU = M::NU, NP = M::NP, NY = M::NY;
  constexpr bool TV = model_time_variant<M>::value;
  const int64_t b = (int64_t)blockIdx.x * ROLLOUT_TPB + threadIdx.x;
  if (b >= batch) return;
  double x[NX], upv[NU + NP > 0 ? NU + NP : 1];
#pragma unroll
  for (int i = 0; i < NX; ++i) {
    x[i] = x0[b * NX + i];
    X[b * NX + i] = x[i];
  }
  constexpr bool ADAPTIVE = plant_adaptive<M>;
  PlantCarry<M> c;
  dopri5_init(c, sp.h0);
  if constexpr (TV) c.t0 = t0;
  if constexpr (ADAPTIVE && METHOD != SIM_MAP) {
    if (hc != nullptr && hc[b] > 0.0) c.h = hc[b];   // a roll-out that goes on where another ended, with the step it would have tried
  }
  const double nan = __builtin_nan("");
  for (int k = 0; k < steps; ++k) {
    double tk = 0.0;   // the start of this sampling interval
    if constexpr (TV) {
      c.t = k * kp.dt;
      tk = t0 + c.t;
    }
    if (k == 0 || up_step != 0) {
      rollout_load_up<M>(up, up_step, up_stride, k, b, upv);
      c.have_k1 = false;   // the slope kept from the last step belongs to the previous interval's inputs
    }
    const double* u = upv;
    const double* p = upv + NU;
    const bool ok = plant_interval<M, METHOD>(kp, sp, c, x, u, p, tk);
    double* Xk = X + ((int64_t)(k + 1) * batch + b) * NX;
#pragma unroll
    for (int i = 0; i < NX; ++i) Xk[i] = ok ? x[i] : nan;
    if constexpr (NY > 0) {
      if (Y != nullptr) {
        double yy[NY];
        // a continuous model is measured at the end of the interval, a discrete one at the time its map was handed
        model_meas_at<M>(M::DISCRETE ? tk : tk + kp.dt, x, u, p, kp.dt, yy);
        double* Yk = Y + ((int64_t)k * batch + b) * NY;
#pragma unroll
        for (int i = 0; i < NY; ++i) Yk[i] = ok ? yy[i] : nan;
      }
    }
  }
  rollout_write_stats(stats, b, c);
  if constexpr (ADAPTIVE && METHOD != SIM_MAP) {
    if (hc != nullptr) hc[b] = c.h;
  }
}

// The SIM_BDF path.  Inputs held over the roll-out (up_step == 0): ONE integration over [0, steps dt] whose state - difference
// table, order, step size, Jacobian, factors - is carried across the sampling instants; a step may pass one or several of them and
// their states are read off the interpolant (scipy's solve_ivp with t_eval, CVODES in normal mode).  An input sequence: the
// right-hand side jumps at every instant, so each interval is an integration of its own from order 1 with a fresh first step.
// A time-variant functor sees the integration's own clock plus its start: t0 with the inputs held, t0 + k dt at a restart.
template <class M, class KP>
__device__ __forceinline__ void rollout_bdf_body(const KP& kp, const SimParams& sp, int64_t batch, int steps,
                                                 const double* __restrict__ x0, const double* __restrict__ up, int64_t up_stride,
                                                 int64_t up_step, double* __restrict__ X, double* __restrict__ Y,
                                                 int* __restrict__ stats, lds_double* lds, double t0) {
  constexpr int NX = M::NX, NU = M::NU, NP = M::NP, NY = M::NY;
  constexpr bool TV = model_time_variant<M>::value;
  static_assert(!M::DISCRETE && NX <= BDF_MAX_NX, "SIM_BDF integrates a continuous model of at most BDF_MAX_NX states");
  const int64_t b = (int64_t)blockIdx.x * ROLLOUT_TPB + threadIdx.x;
  if (b >= batch) return;
  double x[NX], upv[NU + NP > 0 ? NU + NP : 1];
#pragma unroll
  for (int i = 0; i < NX; ++i) {
    x[i] = x0[b * NX + i];
    X[b * NX + i] = x[i];
  }
  const BdfMem<NX, ROLLOUT_TPB, lds_double*> mem = {lds + threadIdx.x};
  BdfCarry<NX> c;
  const bool held = up_step == 0;
  bdf_init(c, held ? steps * kp.dt : kp.dt);
  if constexpr (TV) c.t0 = t0;
  const double nan = __builtin_nan("");
  for (int k = 0; k < steps; ++k) {
    if (k == 0 || !held) {
      rollout_load_up<M>(up, up_step, up_stride, k, b, upv);
      if (k > 0) {
        bdf_restart(c, kp.dt);
        if constexpr (TV) c.t0 = t0 + k * kp.dt;
      }
    }
    const double* u = upv;
    const double* p = upv + NU;
    const bool ok = bdf_interval<M>(c, mem, x, u, p, kp.dt, held ? (k + 1) * kp.dt : kp.dt, sp.rtol, sp.atol, sp.h0, sp.max_steps) == SIM_OK;
    double* Xk = X + ((int64_t)(k + 1) * batch + b) * NX;
#pragma unroll
    for (int i = 0; i < NX; ++i) Xk[i] = ok ? x[i] : nan;
    if constexpr (NY > 0) {
      if (Y != nullptr) {
        double yy[NY];
        model_meas_at<M>(t0 + (k + 1) * kp.dt, x, u, p, kp.dt, yy);
        double* Yk = Y + ((int64_t)k * batch + b) * NY;
#pragma unroll
        for (int i = 0; i < NY; ++i) Yk[i] = ok ? yy[i] : nan;
      }
    }
  }
  rollout_write_stats(stats, b, c);
}

// The SIM_IDAS path: rollout_bdf_body for a model with algebraic states (idas_interval in w = [x; z]).  z0 [batch][NZ] or null: the
// start of the Newton iteration for the consistent initial z (null: M::z_guess); Z [steps + 1][batch][NZ] or null: the algebraic
// states at the sampling instants, row 0 the consistent initial values.  Inputs held: one integration over the roll-out.  An input
// sequence: a restart at every instant - a consistent start with the new inputs from the z of the previous instant (z jumps when g
// names u), order 1, a fresh first step.  Y[k] = meas_z(x_{k+1}, z_{k+1}, u_k, p) on the pair written to X and Z: no further solve.
// An instance that fails gets NaN in X, Z and Y from the first instant it did not reach; with SIM_IC_FAILED at the very start that is
// row 1 of X and row 0 of Z.
template <class M, class KP>
__device__ __forceinline__ void rollout_idas_body(const KP& kp, const SimParams& sp, int64_t batch, int steps,
                                                  const double* __restrict__ x0, const double* __restrict__ z0,
                                                  const double* __restrict__ up, int64_t up_stride, int64_t up_step,
                                                  double* __restrict__ X, double* __restrict__ Z, double* __restrict__ Y,
                                                  int* __restrict__ stats, lds_double* lds) {
  constexpr int NX = M::NX, NZ = M::NZ, N = NX + NZ, NU = M::NU, NP = M::NP, NY = M::NY;
  static_assert(!M::DISCRETE && NZ > 0 && N <= BDF_MAX_NX, "SIM_IDAS integrates a continuous model with algebraic states, NX + NZ <= BDF_MAX_NX");
  const int64_t b = (int64_t)blockIdx.x * ROLLOUT_TPB + threadIdx.x;
  if (b >= batch) return;
  double w[N], upv[NU + NP > 0 ? NU + NP : 1];
#pragma unroll
  for (int i = 0; i < NX; ++i) {
    w[i] = x0[b * NX + i];
    X[b * NX + i] = w[i];
  }
#pragma unroll
  for (int i = 0; i < NZ; ++i) w[NX + i] = z0 != nullptr ? z0[b * NZ + i] : M::z_guess(i);
  const BdfMem<N, ROLLOUT_TPB, lds_double*> mem = {lds + threadIdx.x};
  BdfCarry<N> c;
  const bool held = up_step == 0;
  bdf_init(c, held ? steps * kp.dt : kp.dt);
  const double nan = __builtin_nan("");
  for (int k = 0; k < steps; ++k) {
    if (k == 0 || !held) {
      rollout_load_up<M>(up, up_step, up_stride, k, b, upv);
      if (k > 0) bdf_restart(c, kp.dt);
    }
    const double* u = upv;
    const double* p = upv + NU;
    if (k == 0) {
      const bool ok0 = idas_start<M>(c, mem, w, u, p, sp.rtol, sp.atol, sp.h0) == SIM_OK;
      if (Z != nullptr) {
#pragma unroll
        for (int i = 0; i < NZ; ++i) Z[b * NZ + i] = ok0 ? w[NX + i] : nan;
      }
    }
    const bool ok = idas_interval<M>(c, mem, w, u, p, held ? (k + 1) * kp.dt : kp.dt, sp.rtol, sp.atol, sp.h0, sp.max_steps) == SIM_OK;
    double* Xk = X + ((int64_t)(k + 1) * batch + b) * NX;
#pragma unroll
    for (int i = 0; i < NX; ++i) Xk[i] = ok ? w[i] : nan;
    if (Z != nullptr) {
      double* Zk = Z + ((int64_t)(k + 1) * batch + b) * NZ;
#pragma unroll
      for (int i = 0; i < NZ; ++i) Zk[i] = ok ? w[NX + i] : nan;
    }
    if constexpr (NY > 0) {
      if (Y != nullptr) {
        double yy[NY];
        M::meas_z(w, w + NX, u, p, yy);
        double* Yk = Y + ((int64_t)k * batch + b) * NY;
#pragma unroll
        for (int i = 0; i < NY; ++i) Yk[i] = ok ? yy[i] : nan;
      }
    }
  }
  rollout_write_stats(stats, b, c);
}

// ---- forward sensitivities of the Dormand-Prince roll-out, one instance on a team of lanes -------------------------------------
// `dopri5_sens_interval` integrates the augmented system
//   dx/dt = f(t, x, u, p),   dS/dt = f_x S + f_theta,   theta = [x0; u; p],   S(0) = [I | 0 | 0]
// with the pair, the controller and every convention of `dopri5_interval` above - the same `dopri5_core`, on duals - (stage times, first same as last, clipping at the
// sampling instant, model_ode_at): what scipy's RK45 does when it is handed the vector [x; vec S].  The error norm and the norms
// of the first-step estimate run over all NX (1 + NS) components, each with its own scale atol + rtol max(|.|, |.+|); n_rhs counts
// one evaluation of the augmented right-hand side as one, so n_rhs == 6 (acc + rej) + 2 holds as before.
//
// Layout.  The NS selected columns of S are spread over a team of T lanes, T the smallest power of two >= NS (T <= 64).  A lane
// carries the state x and NC columns as Dual<NC> numbers: the tangent of x is the column, the tangent of [u; p] is 1 at the
// column's own entry and 0 elsewhere (the caller sets the seeds as DATA: no lane branches on its column), and one evaluation of
// the functor on those duals is f next to f_x s + f_theta.  Every lane of a team carries x redundantly; a lane whose columns lie
// behind NS carries zero columns, which stay zero and add nothing to a norm - the divisor is NX (1 + NS), not a count over lanes.
// The device runs NC = 1 on the lane team; the host test (tests/test_sens_host.py) runs the same statements with every column in
// one "lane" and a team of one.  NC > 1 on the device - fewer redundant copies of x for small models - is a tuning knob not used.
//
// Uniformity.  The value parts of x, of the slopes and of the trial point are computed from values alone - the same operations
// on the same operands in every lane of a team - so the team's copies of x agree bit for bit as long as every lane takes the
// same steps.  The ONE thing a step decides on that differs between lanes is the columns' share of the sum of squares, and it
// enters every decision through `team.sum` only: the accept / reject test, the step-size factor, the loop exit, the step count,
// max_steps and the too-small-step test read team-uniform values (a NaN in any lane's share makes the sum NaN in all of them: a
// rejection for the team).  `LaneTeam::sum` is an xor butterfly: at each level a lane and its partner add the same two numbers,
// and addition commutes, so after log2 T levels all T lanes hold the same bits - no broadcast.  Teams are aligned to T within the
// wave, so the partner c ^ m, m < T, is a lane of the same team, which is in the loop whenever this lane is; the teams of a wave
// run their own step sequences and no value crosses from one team to another.
struct TeamOfOne {   // the host: every column in the one "lane"
  HD double sum(double s) const { return s; }
};
struct LaneTeam {    // T lanes of a wave, aligned to T
  int T;
  __device__ __forceinline__ double sum(double s) const {
    const int lane = (int)threadIdx.x;
#pragma unroll 1
    for (int m = 1; m < T; m <<= 1) {   // xor butterfly (see above)
      const int src = (lane ^ m) << 2;
      const int lo = __builtin_amdgcn_ds_bpermute(src, __double2loint(s));
      const int hi = __builtin_amdgcn_ds_bpermute(src, __double2hiint(s));
      s += __hiloint2double(hi, lo);
    }
    return s;
  }
};

// Widest model the team kernel is built for.  A lane holds the ten vectors of a step (seven slopes, the state, the stage point and
// the trial point) 2 NX doubles wide - value and tangent - next to the duals of [u; p] and the functor's temporaries, which are
// twice as many as in doubles.  Measured like DOPRI5_MAX_NX, with a dense synthetic right-hand side (a sine, an exponential and two
// products per state) on Dual<1>, cross-compiled for gfx950, registers of a lane's 512 / bytes of scratch per lane: 4 states 422 / 0,
// 5 states 512 / 60, 6 states 512 / 284, 8 states 512 / 1092, 12 states 512 / 2872.  The zoo: Linear2 150, Bioreactor3 196,
// Chemostat4 238, Pendulum4 260, no scratch.  A wider model is refused by the host (HILO_ENOTSUP) instead of being left to spill;
// so is a run-time compiled one whose kernel reports scratch.
constexpr int SENS_MAX_NX = 4;
constexpr int SENS_X0 = 1, SENS_U = 2, SENS_P = 4;   // HILO_SENS_*: the groups of theta whose columns are carried, in this order

template <int NX, int NC>
using SensCarry = Dopri5Carry<NX, Dual<NC>>;   // the slope at the current state as duals

template <int NX, int NC>
HD void sens_init(SensCarry<NX, NC>& c, double h0) {
  dopri5_init(c, h0);
}

// The seeds of the lane (or host "lane") whose first column is col0: x gets its values and the unit tangents of the x0 group,
// [u; p] theirs.  Column j of the selection is entry j of [x0 | u | p] restricted to the groups of `wrt`; a column >= NS has no
// entry anywhere and is a zero column.  Comparisons turned into 0.0 / 1.0: data, not branches.
template <class M, int NC>
HD void sens_seed_x(int wrt, int col0, const double* xv, Dual<NC>* x) {
#pragma unroll
  for (int i = 0; i < M::NX; ++i) {
    x[i].v = xv[i];
#pragma unroll
    for (int q = 0; q < NC; ++q) x[i].d[q] = (double)((wrt & SENS_X0) != 0 && col0 + q == i);
  }
}
template <class M, int NC>
HD void sens_seed_up(int wrt, int col0, const double* upv, Dual<NC>* u, Dual<NC>* p) {
  const int off_u = (wrt & SENS_X0) ? M::NX : 0, off_p = off_u + ((wrt & SENS_U) ? M::NU : 0);
#pragma unroll
  for (int i = 0; i < M::NU; ++i) {
    u[i].v = upv[i];
#pragma unroll
    for (int q = 0; q < NC; ++q) u[i].d[q] = (double)((wrt & SENS_U) != 0 && col0 + q == off_u + i);
  }
#pragma unroll
  for (int i = 0; i < M::NP; ++i) {
    p[i].v = upv[M::NU + i];
#pragma unroll
    for (int q = 0; q < NC; ++q) p[i].d[q] = (double)((wrt & SENS_P) != 0 && col0 + q == off_p + i);
  }
}
template <class M>
HD int sens_columns(int wrt) {
  return ((wrt & SENS_X0) ? M::NX : 0) + ((wrt & SENS_U) ? M::NU : 0) + ((wrt & SENS_P) ? M::NP : 0);
}

// sum over the augmented vector of (v / (atol + rtol max(|a|, |b|)))^2: the state's share (identical in every lane of a team,
// counted once) plus the team's sum of the columns' shares
template <int NX, int NC, class TEAM>
HD double sens_sumsq(const TEAM& team, const Dual<NC>* v, const Dual<NC>* a, const Dual<NC>* b, double rtol, double atol) {
  double sx = 0.0, sc = 0.0;
#pragma unroll
  for (int i = 0; i < NX; ++i) {
    const double q = v[i].v / (atol + ::fmax(::fabs(a[i].v), ::fabs(b[i].v)) * rtol);
    sx += q * q;
#pragma unroll
    for (int j = 0; j < NC; ++j) {
      const double r = v[i].d[j] / (atol + ::fmax(::fabs(a[i].d[j]), ::fabs(b[i].d[j])) * rtol);
      sc += r * r;
    }
  }
  return sx + team.sum(sc);
}

// the norm policy of the augmented vector (PlainNorm's sibling): NX (1 + ns) components, the columns' share through team.sum
template <int NX, int NC, class TEAM>
struct SensNorm {
  const TEAM& team;
  int ns;
  double rtol, atol;
  template <class V>
  HD double sumsq(const V& v, const Dual<NC>* a, const Dual<NC>* b) const {
    Dual<NC> w[NX];   // (a Lazy is written out first: the vector, then its sum, as the kernel had it)
#pragma unroll
    for (int i = 0; i < NX; ++i) w[i] = v[i];
    return sens_sumsq<NX>(team, w, a, b, rtol, atol);
  }
  HD double divisor() const { return (double)(NX * (1 + ns)); }
};

// One sampling interval of the augmented system, in place in x (values and columns): dopri5_core on duals.  ns: the number of
// selected columns (the norms' divisor is NX (1 + ns)); u, p: the inputs and parameters with their seeds.  Returns c.status, the
// same in every lane of a team (tl, c.h and the step count are team-uniform); on a failure x holds whatever the integration
// stopped at (the caller discards it).
template <class M, int NC, class TEAM>
HD int dopri5_sens_interval(SensCarry<M::NX, NC>& c, const TEAM& team, int ns, Dual<NC>* x, const Dual<NC>* u, const Dual<NC>* p,
                            double dt, double rtol, double atol, int max_steps) {
  return dopri5_core<M>(c, SensNorm<M::NX, NC, TEAM>{team, ns, rtol, atol}, x, u, p, dt, max_steps);
}

// The roll-out with sensitivities: 64 / T instances per wave, lane c of a team carries x and column c (NC = 1).  wrt: HILO_SENS_*
// groups; T: the team size for sens_columns(wrt), chosen by the host.  X, Y, stats as in rollout_body, written by the team's first
// lane (Y: the value part of the measurement on the duals);  SX [steps + 1][batch][NS][NX]: a lane writes its column as NX
// contiguous doubles, row 0 the seed;  SY [steps][batch][NS][NY] = h_x S + h_theta at the end of each interval, or null.  An input
// sequence (up_step != 0): the columns go on across the sampling instants with the new inputs' values (the host refuses SENS_U:
// each interval's input would be a parameter of its own).  A failed instance gets NaN in SX / SY wherever it gets NaN in X.
// A team whose instance lies behind the batch leaves as a whole, before the first exchange.
template <class M, class KP>
__device__ __forceinline__ void rollout_sens_body(const KP& kp, const SimParams& sp, int64_t batch, int steps,
                                                  const double* __restrict__ x0, const double* __restrict__ up, int64_t up_stride,
                                                  int64_t up_step, int wrt, int T, double* __restrict__ X, double* __restrict__ Y,
                                                  double* __restrict__ SX, double* __restrict__ SY, int* __restrict__ stats,
                                                  double t0) {
  constexpr int NX = M::NX, NU = M::NU, NP = M::NP, NY = M::NY;
  constexpr bool TV = model_time_variant<M>::value;
  static_assert(!M::DISCRETE && NX <= SENS_MAX_NX, "the sensitivity roll-out integrates a continuous model of at most SENS_MAX_NX states");
  const int lane = (int)threadIdx.x, col = lane & (T - 1);
  const int64_t b = (int64_t)blockIdx.x * (ROLLOUT_TPB / T) + lane / T;
  if (b >= batch) return;   // (b is the same in all T lanes of the team)
  const int ns = sens_columns<M>(wrt);
  const bool first = col == 0, mine = col < ns;
  const LaneTeam team = {T};
  Dual<1> x[NX], u[NU > 0 ? NU : 1], p[NP > 0 ? NP : 1];
  double upv[NU + NP > 0 ? NU + NP : 1];
  {
    double xv[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) xv[i] = x0[b * NX + i];
    sens_seed_x<M>(wrt, col, xv, x);
  }
#pragma unroll
  for (int i = 0; i < NX; ++i) {
    if (first) X[b * NX + i] = x[i].v;
    if (mine) SX[(b * ns + col) * NX + i] = x[i].d[0];
  }
  SensCarry<NX, 1> c;
  sens_init(c, sp.h0);
  if constexpr (TV) c.t0 = t0;
  const double nan = __builtin_nan("");
  for (int k = 0; k < steps; ++k) {
    double tk = 0.0;   // the start of this sampling interval
    if constexpr (TV) {
      c.t = k * kp.dt;
      tk = t0 + c.t;
    }
    if (k == 0 || up_step != 0) {
      rollout_load_up<M>(up, up_step, up_stride, k, b, upv);
      sens_seed_up<M>(wrt, col, upv, u, p);
      c.have_k1 = false;   // the slope kept from the last step belongs to the previous interval's inputs
    }
    const bool ok = dopri5_sens_interval<M>(c, team, ns, x, u, p, kp.dt, sp.rtol, sp.atol, sp.max_steps) == SIM_OK;
    const int64_t row = (int64_t)(k + 1) * batch + b;
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      if (first) X[row * NX + i] = ok ? x[i].v : nan;
      if (mine) SX[(row * ns + col) * NX + i] = ok ? x[i].d[0] : nan;
    }
    if constexpr (NY > 0) {
      if (Y != nullptr || SY != nullptr) {
        Dual<1> yy[NY];
        model_meas_at<M>(tk + kp.dt, x, u, p, kp.dt, yy);
        const int64_t rowy = (int64_t)k * batch + b;
#pragma unroll
        for (int i = 0; i < NY; ++i) {
          if (first && Y != nullptr) Y[rowy * NY + i] = ok ? yy[i].v : nan;
          if (mine && SY != nullptr) SY[(rowy * ns + col) * NY + i] = ok ? yy[i].d[0] : nan;
        }
      }
    }
  }
  if (first) rollout_write_stats(stats, b, c);
}
}  // namespace hilo
