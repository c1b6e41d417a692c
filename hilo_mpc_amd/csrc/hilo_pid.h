// The PID law and the closed loop around the roll-out: one launch advances a batch of control loops - controller and plant - over
// many sampling intervals, one instance per lane, with the input computed inside the launch instead of read from memory.
//
// Reference: `PID.setup` / `PID.call` (hilo_mpc/modules/controller/pid.py:244-365), a velocity-form law per loop j
//   e = sp - pv on the windows [-3, -2, -1] of process value and set point
//   delta  = e[-1] - e[-2]                                  or  -(pv[-1] - pv[-2])                    (proportional on the process value)
//   delta += dt / t_i e[-1]                                                                           (t_i = inf: nothing)
//   delta += t_d / dt (e[-1] - 2 e[-2] + e[-3])             or  -t_d / dt (pv[-1] - 2 pv[-2] + pv[-3]) (derivative on the process value)
//   u = u_prev + k_p delta
// What a loop remembers is pv[-2], pv[-1], sp[-2], sp[-1] and u_prev - PID_MEM doubles, all zero after a reset.  The set-point
// history starts at zero like the reference's, so the first call sees a set-point step (its known answers depend on it).  Beyond
// the reference (pid.py:278 "TODO: Add anti-windup"): with PID_LIMITS u is clamped to [lo, hi] and the CLAMPED value is what is
// remembered as u_prev - in velocity form that is the anti-windup.
//
// Every product that feeds a sum is an explicit fma, so the two kernels (hilo_pid.hip::pid_call_kernel, pid_loop_body) and a host
// build of this header compute the same bits from the same inputs whichever way a compiler would have contracted them.
//
// Everything up to `pid_loop_body` is `HD` like dopri5_interval: the same statements compile for the host (tests/test_pid_host.py).
#pragma once
#include "hilo_integrate.h"

namespace hilo {

constexpr int PID_MAX_LOOPS = 4;   // HILO_PID_MAX_LOOPS: the regulator's input cap (HILO_LQR_MAX_NU)
constexpr int PID_MEM = 5;         // HILO_PID_MEM: pv[-2], pv[-1], sp[-2], sp[-1], u_prev
constexpr int PID_P_ON_PV = 1, PID_D_ON_PV = 2, PID_LIMITS = 4;   // HILO_PID_* flags

struct PidParams {   // mirrors hilo_pid_opts (include/hilo_hip.h)
  int nsp, flags;
  int pv_index[PID_MAX_LOOPS];      // loop j controls measurement (or, pv_is_state[j], state) number pv_index[j] ...
  int pv_is_state[PID_MAX_LOOPS];
  int out_index[PID_MAX_LOOPS];     // ... through input number out_index[j]
  double lo[PID_MAX_LOOPS], hi[PID_MAX_LOOPS];
};

// One call of the law for one loop: shifts pv and sp into the memory m [PID_MEM], returns u (m[4] afterwards) and the current
// error sp - pv in *e.  A NaN passes through the clamp.
HD double pid_update(double* m, double pv, double sp, double k_p, double t_i, double t_d, double dt, int flags, double lo,
                     double hi, double* e) {
  const double pv3 = m[0], pv2 = m[1], sp3 = m[2], sp2 = m[3];
  const double e1 = sp - pv, e2 = sp2 - pv2, e3 = sp3 - pv3;
  double delta = (flags & PID_P_ON_PV) ? -(pv - pv2) : e1 - e2;
  delta = ::fma(dt / t_i, e1, delta);
  const double dd = (flags & PID_D_ON_PV) ? -(::fma(-2.0, pv2, pv) + pv3) : ::fma(-2.0, e2, e1) + e3;
  delta = ::fma(t_d / dt, dd, delta);
  double u = ::fma(k_p, delta, m[4]);
  if (flags & PID_LIMITS) {
    u = u < lo ? lo : u;
    u = u > hi ? hi : u;
  }
  m[0] = pv2;
  m[1] = pv;
  m[2] = sp2;
  m[3] = sp;
  m[4] = u;
  *e = e1;
  return u;
}

// The closed loop of instance b (rollout_body with the input computed each interval).  Per sampling interval k:
//   pv_j  the selected measurement h(t_k, x[k], u_applied, p) or the selected state; u_applied: the input vector of the previous
//         interval - at k = 0 the held row of `up` with the driven entries taken from the memory's u_prev
//   u_j   pid_update with this interval's set point; the driven entries of the input vector are overwritten, the others keep the
//         held value
//   plant model_step (SIM_MAP) or dopri5_interval (SIM_DOPRI5; the input jumps, so the slope kept from the last step is dropped
//         every interval - the step-size proposal is carried): rollout_body's plant_interval
//   X[k + 1], U[k] (the nsp controller outputs), Y[k] = h(x[k + 1], u[k], p); each of X, U, Y may be null (the sweep: only J,
//   x_final and stats leave the chip)
//   J [batch][nsp][4]: ISE += e^2 dt, IAE += |e| dt, ITAE += (k dt) |e| dt, TVU += |u_k - u_{k-1}|, in k order
// up: the row [u; p] of instance b at up + b up_stride (0: shared), held; spt: the set points of interval k and instance b at
// spt + k sp_step + b sp_stride (either 0: held / shared); gains: rows k_p [nsp], t_i [nsp], t_d [nsp] at gains + b gain_stride
// (0: shared); mem [batch][nsp][PID_MEM] read at the start and left where the loop ended.  An instance whose integration fails
// gets NaN rows from the instant it did not reach (the law stops there), NaN in J and x_final.  t0, hc as in rollout_body.
// The loops over the controller's loops j are unrolled to min(M::NU, PID_MAX_LOOPS) under the predicate j < nsp, and "measurement
// number i" / "input number i" are unrolled selects: no private array is indexed at run time.
template <class M, int METHOD = -1, class KP>
HD void pid_loop_instance(const KP& kp, const SimParams& sp, const PidParams& po, int64_t b, int64_t batch, int steps,
                          const double* __restrict__ x0, const double* __restrict__ up, int64_t up_stride,
                          const double* __restrict__ spt, int64_t sp_stride, int64_t sp_step, const double* __restrict__ gains,
                          int64_t gain_stride, double* __restrict__ mem, double* __restrict__ X, double* __restrict__ U,
                          double* __restrict__ Y, double* __restrict__ J, double* __restrict__ x_final, int* __restrict__ stats,
                          double t0, double* __restrict__ hc) {
  constexpr int NX = M::NX, NU = M::NU, NP = M::NP, NY = M::NY;
  constexpr int NL = NU < PID_MAX_LOOPS ? NU : PID_MAX_LOOPS;
  constexpr bool TV = model_time_variant<M>::value;
  static_assert(NU > 0, "a closed loop needs an input to drive");
  const int nsp = po.nsp;
  double x[NX], upv[NU + NP], m[NL][PID_MEM], g[NL][3], acc[NL][4];
#pragma unroll
  for (int i = 0; i < NX; ++i) {
    x[i] = x0[b * NX + i];
    if (X != nullptr) X[b * NX + i] = x[i];
  }
  rollout_load_up<M>(up, 0, up_stride, 0, b, upv);   // held
  bool any_meas = false;
#pragma unroll
  for (int j = 0; j < NL; ++j) {
    const bool on = j < nsp;
#pragma unroll
    for (int r = 0; r < PID_MEM; ++r) m[j][r] = on ? mem[(b * nsp + j) * PID_MEM + r] : 0.0;
#pragma unroll
    for (int r = 0; r < 3; ++r) g[j][r] = on ? gains[b * gain_stride + (int64_t)r * nsp + j] : 0.0;
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[j][r] = 0.0;
    if (on) {
      any_meas = any_meas || !po.pv_is_state[j];
#pragma unroll
      for (int i = 0; i < NU; ++i) upv[i] = po.out_index[j] == i ? m[j][4] : upv[i];
    }
  }
  constexpr bool ADAPTIVE = plant_adaptive<M>;
  PlantCarry<M> c;
  dopri5_init(c, sp.h0);
  if constexpr (TV) c.t0 = t0;
  if constexpr (ADAPTIVE && METHOD != SIM_MAP) {
    if (hc != nullptr && hc[b] > 0.0) c.h = hc[b];
  }
  const double nan = __builtin_nan("");
  const double* p = upv + NU;
  bool ok = true;
  for (int k = 0; k < steps; ++k) {
    double tk = 0.0;   // the start of this sampling interval
    if constexpr (TV) {
      c.t = k * kp.dt;
      tk = t0 + c.t;
    }
    if (ok) {
      double yy[NY > 0 ? NY : 1];
#pragma unroll
      for (int i = 0; i < (NY > 0 ? NY : 1); ++i) yy[i] = 0.0;
      if constexpr (NY > 0) {
        if (any_meas) model_meas_at<M>(tk, x, upv, p, kp.dt, yy);
      }
#pragma unroll
      for (int j = 0; j < NL; ++j) {
        if (j < nsp) {
          double pv = 0.0;
          const int idx = po.pv_index[j];
          if (po.pv_is_state[j]) {
#pragma unroll
            for (int i = 0; i < NX; ++i) pv = idx == i ? x[i] : pv;
          } else {
#pragma unroll
            for (int i = 0; i < NY; ++i) pv = idx == i ? yy[i] : pv;
          }
          const double u_before = m[j][4];
          double e;
          const double uj = pid_update(m[j], pv, spt[(int64_t)k * sp_step + b * sp_stride + j], g[j][0], g[j][1], g[j][2], kp.dt,
                                       po.flags, po.lo[j], po.hi[j], &e);
#pragma unroll
          for (int i = 0; i < NU; ++i) upv[i] = po.out_index[j] == i ? uj : upv[i];
          if (U != nullptr) U[((int64_t)k * batch + b) * nsp + j] = uj;
          const double ae = ::fabs(e);
          acc[j][0] = ::fma(e * e, kp.dt, acc[j][0]);
          acc[j][1] = ::fma(ae, kp.dt, acc[j][1]);
          acc[j][2] = ::fma((k * kp.dt) * ae, kp.dt, acc[j][2]);
          acc[j][3] += ::fabs(uj - u_before);
        }
      }
      c.have_k1 = false;   // the input has jumped: the slope kept from the last step belongs to the previous interval
      ok = plant_interval<M, METHOD>(kp, sp, c, x, upv, p, tk);
    } else if (U != nullptr) {
      for (int j = 0; j < nsp; ++j) U[((int64_t)k * batch + b) * nsp + j] = nan;
    }
    if (X != nullptr) {
      double* Xk = X + ((int64_t)(k + 1) * batch + b) * NX;
#pragma unroll
      for (int i = 0; i < NX; ++i) Xk[i] = ok ? x[i] : nan;
    }
    if constexpr (NY > 0) {
      if (Y != nullptr) {
        double yy[NY];
#pragma unroll
        for (int i = 0; i < NY; ++i) yy[i] = nan;
        // a continuous model is measured at the end of the interval, a discrete one at the time its map was handed
        if (ok) model_meas_at<M>(M::DISCRETE ? tk : tk + kp.dt, x, upv, p, kp.dt, yy);
        double* Yk = Y + ((int64_t)k * batch + b) * NY;
#pragma unroll
        for (int i = 0; i < NY; ++i) Yk[i] = yy[i];
      }
    }
  }
#pragma unroll
  for (int j = 0; j < NL; ++j) {
    if (j < nsp) {
#pragma unroll
      for (int r = 0; r < PID_MEM; ++r) mem[(b * nsp + j) * PID_MEM + r] = m[j][r];
#pragma unroll
      for (int r = 0; r < 4; ++r) J[(b * nsp + j) * 4 + r] = ok ? acc[j][r] : nan;
    }
  }
#pragma unroll
  for (int i = 0; i < NX; ++i) x_final[b * NX + i] = ok ? x[i] : nan;
  rollout_write_stats(stats, b, c);
  if constexpr (ADAPTIVE && METHOD != SIM_MAP) {
    if (hc != nullptr) hc[b] = c.h;
  }
}

// one instance per lane, ROLLOUT_TPB lanes per workgroup; no value crosses lanes
template <class M, int METHOD = -1, class KP>
__device__ __forceinline__ void pid_loop_body(const KP& kp, const SimParams& sp, const PidParams& po, int64_t batch, int steps,
                                              const double* __restrict__ x0, const double* __restrict__ up, int64_t up_stride,
                                              const double* __restrict__ spt, int64_t sp_stride, int64_t sp_step,
                                              const double* __restrict__ gains, int64_t gain_stride, double* __restrict__ mem,
                                              double* __restrict__ X, double* __restrict__ U, double* __restrict__ Y,
                                              double* __restrict__ J, double* __restrict__ x_final, int* __restrict__ stats,
                                              double t0 = 0.0, double* __restrict__ hc = nullptr) {
  const int64_t b = (int64_t)blockIdx.x * ROLLOUT_TPB + threadIdx.x;
  if (b >= batch) return;
  pid_loop_instance<M, METHOD>(kp, sp, po, b, batch, steps, x0, up, up_stride, spt, sp_stride, sp_step, gains, gain_stride, mem, X, U,
                               Y, J, x_final, stats, t0, hc);
}
}  // namespace hilo
