// Data generation for learning a model term: one launch excites a batch of plants - each with its own initial state, parameters and
// random stream - over T sampling intervals, with the excitation signal evaluated inside the launch, and writes features and labels
// directly in training layout, measurement noise included.
//
// Reference: `DataGenerator` (hilo_mpc/util/data.py:642-1167) - `random_uniform`, `random_normal`, `chirp`, and the slicing algebra of
// `run` for use_input_as_label=False.
//
// Signals (one kind per run), evaluated per sampling interval k:
//   DG_UNIFORM  a staircase: sample s = k / hold, u_i = fma(ub_i - lb_i, U, lb_i)
//   DG_NORMAL   the same with u_i = fma(sqrt(variance_i), Z, mean_i)
//   DG_CHIRP    per input up to DG_MAX_SEG segments {type, point count, amplitude, mean, chirp rate, initial phase, initial
//               frequency, initial frequency ratio} of a table in global memory, [NU][DG_MAX_SEG][DG_SEG_FIELDS]; the local time of
//               a segment is i dt, counted from the segment's start (data.py:968: np.arange(0., length, dt))
// Draws: Philox4x32-10 (hilo_philox.h) on the counter
//     (0, index, b + instance_offset, stream << 16 | d)        key = (seed low, seed high)
// where block d supplies values 2d and 2d+1; `index` is the sample number s for inputs (value i: input i) and the time index j for
// noise (value i: state i, under that state's own key); streams 8 input uniforms, 9 input normals, 10 noise uniforms, 11 noise
// normals.  A row therefore depends on nothing but (seed, instance number, time index).
//
// Assembly (data.py:1048-1141).  nk kept states (skip_mask removes states), N = T - shift rows, F [N][B][(shift + 1) nk + NU],
// L [N][B][nk].  The noisy kept state xt_j = x_j + n_j, j = 0..T, is scattered: for s = 0..shift to row j - s, block s; u_k to row
// k - shift, last block; the label of row j - shift - 1 is xt_j, or with `difference` (x_j - x_{j-1}) + (n_j - n_{j-1}) in that order
// (np.diff of the states plus np.diff of one noise array: the n_j of a label is the n_j of the next row's feature).  No history is
// kept beyond the previous state and noise.  All stores are [row][instance][column]: the lanes of a wave write adjacent memory.
//
// Every product that feeds a sum in the signal and the noise is an explicit fma, as in hilo_pid.h, so a host build of this header
// computes the same bits from the same draws.  Everything up to `datagen_body` is `HD`: tests/test_datagen_host.py compiles it.
#pragma once
#include "hilo_integrate.h"
#include "hilo_philox.h"

namespace hilo {

constexpr int DG_MAX_NU = 4;     // HILO_DATAGEN_MAX_NU (HILO_PID_MAX_LOOPS)
constexpr int DG_MAX_NX = 12;    // HILO_DATAGEN_MAX_NX (HILO_SIM_DOPRI5_MAX_NX)
constexpr int DG_MAX_SEG = 8, DG_SEG_FIELDS = 8;
constexpr int DG_UNIFORM = 0, DG_NORMAL = 1, DG_CHIRP = 2;                       // HILO_DATAGEN_* signal kinds
constexpr int DG_CHIRP_LINEAR = 0, DG_CHIRP_EXPONENTIAL = 1, DG_CHIRP_HYPERBOLIC = 2;
constexpr int DG_NOISE_NONE = 0, DG_NOISE_UNIFORM = 1, DG_NOISE_NORMAL = 2;
constexpr unsigned DG_STREAM_INPUT_UNIFORM = 8, DG_STREAM_INPUT_NORMAL = 9, DG_STREAM_NOISE_UNIFORM = 10, DG_STREAM_NOISE_NORMAL = 11;

struct DatagenParams {   // mirrors hilo_datagen_opts (include/hilo_hip.h)
  unsigned long long seed;
  long long instance_offset;         // global number of instance 0 of this batch
  int kind, hold;                    // DG_UNIFORM / DG_NORMAL / DG_CHIRP; sampling intervals per sample of a staircase
  int shift, difference;             // past states in a feature row; labels x_{k+1} - x_k instead of x_{k+1}
  int skip_mask, reserved;           // bit i: state i is left out of features and labels
  double a[DG_MAX_NU], b[DG_MAX_NU]; // per input: lower / upper bound (DG_UNIFORM), mean / variance (DG_NORMAL)
  int noise_kind[DG_MAX_NX];         // per state: DG_NOISE_*
  unsigned long long noise_seed[DG_MAX_NX];
  double na[DG_MAX_NX], nb[DG_MAX_NX];   // lower / upper bound (DG_NOISE_UNIFORM), standard deviation in na (DG_NOISE_NORMAL)
};

// point k of the chirp signal of one input: seg = that input's DG_MAX_SEG segments (data.py:687-755; the defaults pi / 2 and 1e-4 of
// the initial phase and frequency are filled in by the host).  The host sees to it that the counts add up to the run's length.
HD double datagen_chirp(const double* __restrict__ seg, int k, double dt) {
  int i = k;
  for (int s = 0; s < DG_MAX_SEG; ++s) {
    const double* q = seg + s * DG_SEG_FIELDS;
    const int n = (int)q[1];
    if (i < n) {
      const int type = (int)q[0];
      const double t = i * dt, rate = q[4], phase = q[5], f0 = q[6];
      double arg;
      if (type == DG_CHIRP_LINEAR) {
        arg = phase + 2. * 3.141592653589793 * (rate / 2. * t + f0) * t;
      } else if (type == DG_CHIRP_EXPONENTIAL) {
        arg = phase + 2. * 3.141592653589793 * f0 * (::pow(rate, t) - 1) / ::log(rate);
      } else {
        const double fraction = 1. - 1. / q[7];
        arg = phase - 2. * 3.141592653589793 * dt * f0 / fraction * ::log(1. - fraction / dt * t);
      }
      return ::fma(q[2], ::sin(arg), q[3]);
    }
    i -= n;
  }
  return __builtin_nan("");
}

// Instance b of the run.  T sampling intervals; x0 [batch][NX]; up: the row [u; p] of instance b at up + b up_stride (0: shared) - its
// parameters are held, its inputs overwritten by the signal; F, L as above; X [T + 1][batch][NX] the clean states, U [T][batch][NU]
// the inputs, stats [batch][4] as rollout_body writes them: each of the three may be null.  The plant advances as in rollout_body
// with an input sequence - the slope kept from the last step dropped every interval, the step-size proposal carried, tk = t0 + k dt
// for a time-variant functor - so U handed to the roll-out as a sequence reproduces X bit for bit.  An instance whose integration
// fails gets NaN for every state it did not reach, in X and in every entry of F and L made of such a state.
template <class M, int METHOD = -1, class KP>
HD void datagen_instance(const KP& kp, const SimParams& sp, const DatagenParams& dg, const double* __restrict__ chirp, int64_t b,
                         int64_t batch, int T, const double* __restrict__ x0, const double* __restrict__ up, int64_t up_stride,
                         double* __restrict__ F, double* __restrict__ L, double* __restrict__ X, double* __restrict__ U,
                         int* __restrict__ stats, double t0) {
  constexpr int NX = M::NX, NU = M::NU, NP = M::NP;
  constexpr bool TV = model_time_variant<M>::value;
  static_assert(NU > 0 && NU <= DG_MAX_NU && NX <= DG_MAX_NX, "the parameter struct holds DG_MAX_NU inputs and DG_MAX_NX states");
  const int shift = dg.shift, N = T - shift;
  int nk = 0;
#pragma unroll
  for (int i = 0; i < NX; ++i) nk += (dg.skip_mask >> i & 1) ? 0 : 1;
  const int64_t nf = (int64_t)(shift + 1) * nk + NU;
  double x[NX], upv[NU + NP], x_prev[NX], n_prev[NX];
#pragma unroll
  for (int i = 0; i < NX; ++i) {
    x[i] = x0[b * NX + i];
    x_prev[i] = 0.0;
    n_prev[i] = 0.0;
  }
  rollout_load_up<M>(up, 0, up_stride, 0, b, upv);
  const double* p = upv + NU;
  const unsigned inst = (unsigned)(b + dg.instance_offset);
  const unsigned key0 = (unsigned)dg.seed, key1 = (unsigned)(dg.seed >> 32);
  PlantCarry<M> c;
  dopri5_init(c, sp.h0);
  if constexpr (TV) c.t0 = t0;
  const double nan = __builtin_nan("");
  bool ok = true;
  for (int j = 0; j <= T; ++j) {
    // ---- state j: the clean row, the noise of time index j, the scatter into features and labels
    int col = 0;
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      const double xc = ok ? x[i] : nan;
      if (X != nullptr) X[((int64_t)j * batch + b) * NX + i] = xc;
      if (!(dg.skip_mask >> i & 1)) {
        const int noise = dg.noise_kind[i];
        double n = 0.0;
        if (noise != DG_NOISE_NONE) {
          const unsigned nk0 = (unsigned)dg.noise_seed[i], nk1 = (unsigned)(dg.noise_seed[i] >> 32);
          if (noise == DG_NOISE_UNIFORM) {
            const Philox4 r = philox4x32_10(0u, (unsigned)j, inst, DG_STREAM_NOISE_UNIFORM << 16 | (unsigned)(i >> 1), nk0, nk1);
            n = ::fma(dg.nb[i] - dg.na[i], (i & 1) ? pf_uniform(r.r2, r.r3) : pf_uniform(r.r0, r.r1), dg.na[i]);
          } else {
            double z0, z1;
            pf_box_muller(philox4x32_10(0u, (unsigned)j, inst, DG_STREAM_NOISE_NORMAL << 16 | (unsigned)(i >> 1), nk0, nk1), z0, z1);
            n = dg.na[i] * ((i & 1) ? z1 : z0);
          }
        }
        const double xt = noise != DG_NOISE_NONE ? xc + n : xc;
        const int s_lo = j - N + 1 > 0 ? j - N + 1 : 0, s_hi = j < shift ? j : shift;
        for (int s = s_lo; s <= s_hi; ++s) F[((int64_t)(j - s) * batch + b) * nf + (int64_t)s * nk + col] = xt;
        const int r = j - shift - 1;
        if (r >= 0) {
          double lab = xt;
          if (dg.difference) lab = noise != DG_NOISE_NONE ? (xc - x_prev[i]) + (n - n_prev[i]) : xc - x_prev[i];
          L[((int64_t)r * batch + b) * nk + col] = lab;
        }
        x_prev[i] = xc;
        n_prev[i] = n;
        ++col;
      }
    }
    if (j == T) break;
    // ---- interval k = j: the input vector, then the plant
    const int k = j;
    if (dg.kind == DG_CHIRP) {
#pragma unroll
      for (int i = 0; i < NU; ++i) upv[i] = datagen_chirp(chirp + i * DG_MAX_SEG * DG_SEG_FIELDS, k, kp.dt);
    } else if (k % dg.hold == 0) {
      const unsigned s = (unsigned)(k / dg.hold);
#pragma unroll
      for (int d = 0; d < (NU + 1) / 2; ++d) {
        double v0, v1;
        if (dg.kind == DG_UNIFORM) {
          const Philox4 r = philox4x32_10(0u, s, inst, DG_STREAM_INPUT_UNIFORM << 16 | (unsigned)d, key0, key1);
          v0 = pf_uniform(r.r0, r.r1);
          v1 = pf_uniform(r.r2, r.r3);
          upv[2 * d] = ::fma(dg.b[2 * d] - dg.a[2 * d], v0, dg.a[2 * d]);
          if (2 * d + 1 < NU) upv[2 * d + 1] = ::fma(dg.b[2 * d + 1] - dg.a[2 * d + 1], v1, dg.a[2 * d + 1]);
        } else {
          pf_box_muller(philox4x32_10(0u, s, inst, DG_STREAM_INPUT_NORMAL << 16 | (unsigned)d, key0, key1), v0, v1);
          upv[2 * d] = ::fma(::sqrt(dg.b[2 * d]), v0, dg.a[2 * d]);
          if (2 * d + 1 < NU) upv[2 * d + 1] = ::fma(::sqrt(dg.b[2 * d + 1]), v1, dg.a[2 * d + 1]);
        }
      }
    }
#pragma unroll
    for (int i = 0; i < NU; ++i) {
      if (U != nullptr) U[((int64_t)k * batch + b) * NU + i] = upv[i];
      if (k >= shift) F[((int64_t)(k - shift) * batch + b) * nf + (int64_t)(shift + 1) * nk + i] = upv[i];
    }
    double tk = 0.0;   // the start of this sampling interval
    if constexpr (TV) {
      c.t = k * kp.dt;
      tk = t0 + c.t;
    }
    // the input has jumped: the slope kept from the last step belongs to the previous interval.  (The condition always holds.  It is
    // rollout_body's `k == 0 || up_step != 0`: with a condition the compiler cannot fold, the slope at the start of an interval is
    // evaluated in a block of its own, as there, and shares no product with the steps that follow - sharing one changes which product
    // of dx = .. + u p the compiler contracts into the sum, and with it the last bit of the trajectory.)
    if (k == 0 || dg.hold >= 0) c.have_k1 = false;
    ok = plant_interval<M, METHOD>(kp, sp, c, x, upv, p, tk);   // (a failure is kept: the pair answers its status from then on)
  }
  rollout_write_stats(stats, b, c);
}

// one instance per lane, ROLLOUT_TPB lanes per workgroup; no value crosses lanes
template <class M, int METHOD = -1, class KP>
__device__ __forceinline__ void datagen_body(const KP& kp, const SimParams& sp, const DatagenParams& dg, const double* __restrict__ chirp,
                                             int64_t batch, int T, const double* __restrict__ x0, const double* __restrict__ up,
                                             int64_t up_stride, double* __restrict__ F, double* __restrict__ L, double* __restrict__ X,
                                             double* __restrict__ U, int* __restrict__ stats, double t0 = 0.0) {
  const int64_t b = (int64_t)blockIdx.x * ROLLOUT_TPB + threadIdx.x;
  if (b >= batch) return;
  datagen_instance<M, METHOD>(kp, sp, dg, chirp, b, batch, T, x0, up, up_stride, F, L, X, U, stats, t0);
}
}  // namespace hilo
