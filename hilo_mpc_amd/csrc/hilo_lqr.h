// Linear-quadratic regulator for a batch of instances: linearisation of a handle's map at a per-instance operating point, the
// Riccati equation (finite horizon or stationary), and the feedback  u = u_eq - K (x - x_eq)  - all three in one launch.
//
// Reference semantics: `LinearQuadraticRegulator` (hilo_mpc/modules/controller/lqr.py:236-245): from P = Q, `horizon` backward steps
//   P <- A'PA - (A'PB + N) (R + B'PB)^-1 (B'PA + N') + Q,   then   K = (R + B'PB)^-1 (B'PA + N').
// The reference raises NotImplementedError for `horizon = None`; here that is the stationary gain, from the discrete algebraic
// Riccati equation solved with the structure-preserving doubling algorithm (Chu, Fan, Lin, Wang 2004):
//   A0 = A - B R^-1 N',  G0 = B R^-1 B',  H0 = Q - N R^-1 N';   W = I + G H,
//   A+ = A W^-1 A,   G+ = G + A W^-1 G A',   H+ = H + A' H W^-1 A      (G and H symmetrised every step)
// until max|H+ - H| <= tol max(1, max|H+|); P = H.  It squares the closed-loop matrix every step (5 to 14 steps where the plain
// fixed-point recursion takes hundreds to thousands at small sampling intervals).
//
// Lane mapping: one instance per lane, and every matrix of the instance in LDS - element e of lane l at lds[e * lanes + l], so a
// wave's 64 lanes read 64 consecutive doubles (no bank conflict) and no lane ever touches another lane's column.  The only
// cross-lane operation is the vote that ends the doubling loop when the last lane of the wave is done (no lane-dependent loop
// exit: DESIGN.md 5.1); a lane that is done - converged or failed (status and NaN rows) - keeps its result untouched while its
// neighbours go on, so a lane's result cannot depend on them.  The elimination's pivot search and row swaps index the matrices
// dynamically, which costs nothing in LDS and would put a register array into scratch memory (a one-lane all-registers
// prototype of the doubling loop: 204 registers at 4 states, 506 at 6, scratch at 8).  The price is occupancy: lqr_work_doubles
// per lane, so lqr_lanes() lanes per workgroup share the 160 KB of a compute unit.
// Divisions and square roots here are the IEEE ones: a gain is computed once and used for many steps, and P reaches 1e5.
//
// Everything up to the kernel bodies is `HD` and takes its storage as a view (LaneVec): the same statements compile for the host
// (tests/test_lqr_cpu.py builds a driver around this header and runs it on the CPU with plain arrays).
#pragma once
#include "hilo_common.h"
#include "hilo_models.h"

namespace hilo {

constexpr int LQR_MAX_NX = 8, LQR_MAX_NU = 4;          // HILO_LQR_MAX_NX / _NU
constexpr int LQR_OK = 0, LQR_MAX_ITER = 1, LQR_FAILED = 2;   // HILO_LQR_STATUS_*
constexpr int LQR_LDS_BYTES = 160 * 1024;

struct LqrParams {   // mirrors hilo_lqr_opts (include/hilo_hip.h)
  int horizon, max_iter;   // horizon 0: stationary
  double tol;
};

// doubles of one instance's workspace: A, P, Ad, G, W, V2 (n x n), V1 (n x n in the doubling loop, n x m = A'PB + N in the
// finite-horizon step: the larger of the two), B, PB (n x m), M, K (m x n), S (m x m)
HD constexpr int lqr_work_doubles(int n, int m) { return 6 * n * n + (m > n ? n * m : n * n) + 4 * n * m + m * m; }
// lanes of a workgroup: the most of 64, 32, 16 whose workspaces fit a compute unit's LDS (8 states, 4 inputs: 32)
HD constexpr int lqr_lanes(int n, int m) {
  return 64 * 8 * lqr_work_doubles(n, m) <= LQR_LDS_BYTES ? 64 : (32 * 8 * lqr_work_doubles(n, m) <= LQR_LDS_BYTES ? 32 : 16);
}

// element i of a lane's private array: p[i * stride] (device: p points at the lane's first element in LDS, stride = lanes of the
// workgroup; host: stride 1)
template <class PTR>
struct LaneVec {
  PTR p;
  int stride;
  HD auto& operator[](int i) const { return p[i * stride]; }
  HD LaneVec at(int off) const { return LaneVec{p + off * stride, stride}; }
};

template <class V>
struct LqrWork {   // the views of one instance's matrices
  V A, P, Ad, G, W, V1, V2, B, PB, M, K, S;
  HD LqrWork(V w, int n, int m) {
    const int nn = n * n, nm = n * m, t = 6 * nn + (m > n ? nm : nn);
    A = w; P = w.at(nn); Ad = w.at(2 * nn); G = w.at(3 * nn); W = w.at(4 * nn); V2 = w.at(5 * nn); V1 = w.at(6 * nn);
    B = w.at(t); PB = w.at(t + nm); M = w.at(t + 2 * nm); K = w.at(t + 3 * nm); S = w.at(t + 4 * nm);
  }
};

HD bool lqr_finite(double v) { return __builtin_isfinite(v); }

// Is the predicate true for any lane of the wave?  (host: for this instance)
HD bool lqr_any(bool v) {
#if defined(__HIP_DEVICE_COMPILE__)
  return __any(v) != 0;
#else
  return v;
#endif
}

// Control flow: every loop below has a wave-uniform trip count and every decision that depends on an instance's data is a select
// (no lane-dependent loop exit or branch in device code).  A failure is recorded in a flag and the arithmetic goes
// on (on NaN or infinity, in the lane's own column of the workspace); the caller turns the flag into the status and the NaN rows.

// C (r x c, row-major) = beta C + alpha sum_l A(i, l) B(l, j), with A(i, l) = A[i ar + l ac], B(l, j) = B[l br + j bc]: a transposed
// factor swaps its two strides
template <class VA, class VB, class VC>
HD void lqr_mm(int r, int k, int c, const VA& A, int ar, int ac, const VB& B, int br, int bc, const VC& C, double alpha, double beta) {
  for (int i = 0; i < r; ++i)
    for (int j = 0; j < c; ++j) {
      double s = 0.0;
      for (int l = 0; l < k; ++l) s += A[i * ar + l * ac] * B[l * br + j * bc];
      C[i * c + j] = beta == 0.0 ? alpha * s : beta * C[i * c + j] + alpha * s;
    }
}

// S = L L' in place (lower triangle); false at a pivot that is not positive (or not a number)
template <class V>
HD bool lqr_chol(int m, const V& S) {
  bool ok = true;
  for (int j = 0; j < m; ++j) {
    double d = S[j * m + j];
    for (int l = 0; l < j; ++l) d -= S[j * m + l] * S[j * m + l];
    ok = ok && d > 0.0 && lqr_finite(d);
    d = ::sqrt(d);
    S[j * m + j] = d;
    for (int i = j + 1; i < m; ++i) {
      double s = S[i * m + j];
      for (int l = 0; l < j; ++l) s -= S[i * m + l] * S[j * m + l];
      S[i * m + j] = s / d;
    }
  }
  return ok;
}

// X (m x c) <- (L L')^-1 X
template <class V, class VX>
HD void lqr_chol_solve(int m, int c, const V& L, const VX& X) {
  for (int j = 0; j < c; ++j) {
    for (int i = 0; i < m; ++i) {
      double s = X[i * c + j];
      for (int l = 0; l < i; ++l) s -= L[i * m + l] * X[l * c + j];
      X[i * c + j] = s / L[i * m + i];
    }
    for (int i = m - 1; i >= 0; --i) {
      double s = X[i * c + j];
      for (int l = i + 1; l < m; ++l) s -= L[l * m + i] * X[l * c + j];
      X[i * c + j] = s / L[i * m + i];
    }
  }
}

// X1 <- W^-1 X1, X2 <- W^-1 X2 (all n x n; W is not symmetric): elimination with partial pivoting, the row operations applied to
// the right-hand sides as they are made; W is destroyed.  false at a pivot that is zero or not a number.  The pivot row is a
// per-lane index (free in LDS); a row is swapped with itself where no exchange is needed.
template <class V>
HD bool lqr_lu_solve2(int n, const V& W, const V& X1, const V& X2) {
  bool ok = true;
  for (int k = 0; k < n; ++k) {
    int piv = k;
    double big = ::fabs(W[k * n + k]);
    for (int i = k + 1; i < n; ++i) {
      const double a = ::fabs(W[i * n + k]);
      const bool up = a > big;
      big = up ? a : big;
      piv = up ? i : piv;
    }
    ok = ok && big > 0.0 && lqr_finite(big);
    for (int j = 0; j < n; ++j) {
      double t = W[k * n + j], q = W[piv * n + j];
      W[piv * n + j] = t; W[k * n + j] = q;
      t = X1[k * n + j]; q = X1[piv * n + j];
      X1[piv * n + j] = t; X1[k * n + j] = q;
      t = X2[k * n + j]; q = X2[piv * n + j];
      X2[piv * n + j] = t; X2[k * n + j] = q;
    }
    const double d = W[k * n + k];
    for (int i = k + 1; i < n; ++i) {
      const double f = W[i * n + k] / d;
      for (int j = k + 1; j < n; ++j) W[i * n + j] -= f * W[k * n + j];
      for (int j = 0; j < n; ++j) {
        X1[i * n + j] -= f * X1[k * n + j];
        X2[i * n + j] -= f * X2[k * n + j];
      }
    }
  }
  for (int i = n - 1; i >= 0; --i) {
    const double d = W[i * n + i];
    for (int j = 0; j < n; ++j) {
      double s1 = X1[i * n + j], s2 = X2[i * n + j];
      for (int l = i + 1; l < n; ++l) {
        s1 -= W[i * n + l] * X1[l * n + j];
        s2 -= W[i * n + l] * X2[l * n + j];
      }
      X1[i * n + j] = s1 / d;
      X2[i * n + j] = s2 / d;
    }
  }
  return ok;
}

template <class V>
HD void lqr_symmetrise(int n, const V& H) {
  for (int i = 0; i < n; ++i)
    for (int j = i + 1; j < n; ++j) {
      const double s = 0.5 * (H[i * n + j] + H[j * n + i]);
      H[i * n + j] = s;
      H[j * n + i] = s;
    }
}

// K = (R + B'PB)^-1 (B'PA + N') from w.P (into w.K; destroys W, PB, M, S); false: R + B'PB is not positive definite
template <class V>
HD bool lqr_gain_from_p(int n, int m, const LqrWork<V>& w, const double* R, const double* N) {
  lqr_mm(n, n, n, w.P, n, 1, w.A, n, 1, w.W, 1.0, 0.0);     // W = P A
  lqr_mm(n, n, m, w.P, n, 1, w.B, m, 1, w.PB, 1.0, 0.0);    // PB = P B
  lqr_mm(m, n, n, w.B, 1, m, w.W, n, 1, w.K, 1.0, 0.0);     // K = B' P A
  lqr_mm(m, n, m, w.B, 1, m, w.PB, m, 1, w.S, 1.0, 0.0);    // S = B' P B
  for (int i = 0; i < m; ++i) {
    for (int j = 0; j < m; ++j) w.S[i * m + j] += R[i * m + j];
    if (N != nullptr)
      for (int j = 0; j < n; ++j) w.K[i * n + j] += N[j * m + i];
  }
  const bool ok = lqr_chol(m, w.S);
  for (int i = 0; i < m * n; ++i) w.M[i] = w.K[i];          // M = B'PA + N' (the finite-horizon step needs it next to K)
  lqr_chol_solve(m, n, w.S, w.K);
  return ok;
}

// The gain of one instance from w.A and w.B (n x n, n x m); Q (n x n), R (m x m) and N (n x m, or null: zero) are read where they
// are.  Leaves P in w.P and K in w.K; returns the status and the number of steps made (backward steps / doubling steps).  On the
// device every lane of the wave must call it (it votes): the doubling loop runs until the last lane of the wave is done, and a lane
// that is done no longer writes its P - what it returns does not depend on how long its neighbours go on.
template <class V>
HD int lqr_solve(int n, int m, const LqrParams& o, const LqrWork<V>& w, const double* Q, const double* R, const double* N, int* iters) {
  const int nn = n * n;
  if (o.horizon > 0) {
    bool ok = true;
    for (int i = 0; i < nn; ++i) w.P[i] = Q[i];
    for (int k = 0; k < o.horizon; ++k) {
      ok = lqr_gain_from_p(n, m, w, R, N) && ok;
      // P+ = A' (P A) - (A' P B + N) K + Q
      lqr_mm(n, n, m, w.A, 1, n, w.PB, m, 1, w.V1, 1.0, 0.0);                   // V1 (n x m) = A' P B
      if (N != nullptr)
        for (int i = 0; i < n * m; ++i) w.V1[i] += N[i];
      lqr_mm(n, n, n, w.A, 1, n, w.W, n, 1, w.V2, 1.0, 0.0);                    // V2 = A' P A
      lqr_mm(n, m, n, w.V1, m, 1, w.K, n, 1, w.V2, -1.0, 1.0);
      for (int i = 0; i < nn; ++i) {
        const double v = w.V2[i] + Q[i];
        ok = ok && lqr_finite(v);
        w.P[i] = v;
      }
    }
    ok = lqr_gain_from_p(n, m, w, R, N) && ok;
    *iters = o.horizon;
    return ok ? LQR_OK : LQR_FAILED;
  }
  // ---- stationary: doubling on (Ad, G, H), H in w.P ----
  for (int i = 0; i < m * m; ++i) w.S[i] = R[i];
  bool failed = !lqr_chol(m, w.S);
  for (int i = 0; i < m; ++i)
    for (int j = 0; j < n; ++j) {
      w.M[i * n + j] = N != nullptr ? N[j * m + i] : 0.0;   // N'
      w.K[i * n + j] = w.B[j * m + i];                      // B'
    }
  lqr_chol_solve(m, n, w.S, w.M);   // R^-1 N'
  lqr_chol_solve(m, n, w.S, w.K);   // R^-1 B'
  for (int i = 0; i < nn; ++i) { w.Ad[i] = w.A[i]; w.P[i] = Q[i]; }
  lqr_mm(n, m, n, w.B, m, 1, w.M, n, 1, w.Ad, -1.0, 1.0);   // A0 = A - B R^-1 N'
  lqr_mm(n, m, n, w.B, m, 1, w.K, n, 1, w.G, 1.0, 0.0);     // G0 = B R^-1 B'
  if (N != nullptr) lqr_mm(n, m, n, N, m, 1, w.M, n, 1, w.P, -1.0, 1.0);   // H0 = Q - N R^-1 N'
  lqr_symmetrise(n, w.G);
  lqr_symmetrise(n, w.P);
  bool converged = false;
  int made = 0;
  for (int it = 0; it < o.max_iter; ++it) {
    const bool done = converged || failed;
    if (!lqr_any(!done)) break;                              // (wave-uniform)
    made += done ? 0 : 1;
    lqr_mm(n, n, n, w.G, n, 1, w.P, n, 1, w.W, 1.0, 0.0);   // W = I + G H
    for (int i = 0; i < n; ++i) w.W[i * n + i] += 1.0;
    for (int i = 0; i < nn; ++i) { w.V1[i] = w.Ad[i]; w.V2[i] = w.G[i]; }
    bool ok = lqr_lu_solve2(n, w.W, w.V1, w.V2);             // V1 = W^-1 Ad, V2 = W^-1 G
    lqr_mm(n, n, n, w.V2, n, 1, w.Ad, 1, n, w.W, 1.0, 0.0);                   // W = W^-1 G Ad'
    lqr_mm(n, n, n, w.Ad, n, 1, w.W, n, 1, w.G, 1.0, 1.0);                    // G += Ad W^-1 G Ad'
    lqr_symmetrise(n, w.G);
    lqr_mm(n, n, n, w.P, n, 1, w.V1, n, 1, w.W, 1.0, 0.0);                    // W = H W^-1 Ad
    for (int i = 0; i < nn; ++i) w.V2[i] = w.P[i];
    lqr_mm(n, n, n, w.Ad, 1, n, w.W, n, 1, w.V2, 1.0, 1.0);                   // V2 = H + Ad' H W^-1 Ad
    lqr_symmetrise(n, w.V2);
    double delta = 0.0, hmax = 0.0;
    for (int i = 0; i < nn; ++i) {
      const double hn = w.V2[i], h = w.P[i];
      ok = ok && lqr_finite(hn);
      delta = ::fmax(delta, ::fabs(hn - h));
      hmax = ::fmax(hmax, ::fabs(hn));
      w.P[i] = done ? h : hn;                                // a lane that is done keeps its H
    }
    lqr_mm(n, n, n, w.Ad, n, 1, w.V1, n, 1, w.W, 1.0, 0.0);                   // Ad <- Ad W^-1 Ad
    for (int i = 0; i < nn; ++i) {
      ok = ok && lqr_finite(w.W[i]) && lqr_finite(w.G[i]);
      w.Ad[i] = w.W[i];
    }
    failed = failed || (!done && !ok);
    converged = converged || (!done && ok && delta <= o.tol * ::fmax(1.0, hmax));
  }
  *iters = made;
  const bool gain_ok = lqr_gain_from_p(n, m, w, R, N);
  return failed ? LQR_FAILED : (!converged ? LQR_MAX_ITER : (gain_ok ? LQR_OK : LQR_FAILED));
}

// Directions of one forward-mode pass: all NX + NU at once up to six (the zoo: at most 4 + 2), otherwise passes of four - the
// slopes of the Runge-Kutta step carry (1 + directions) doubles per state.
// A functor may ask for narrower passes with `static constexpr int LQR_CHUNK` (emitted for models that carry a neural network:
// every value of the network is multiplied by 1 + directions, and with all six the Runge-Kutta step no longer fits the registers).
// The Jacobian columns do not depend on how they are grouped.
template <class M, class = void> struct LqrChunkHint { static constexpr int value = 0; };
template <class M> struct LqrChunkHint<M, decltype((void)M::LQR_CHUNK)> { static constexpr int value = M::LQR_CHUNK; };
template <class M> struct LqrChunk {
  static constexpr int full = M::NX + M::NU <= 6 ? (M::NX + M::NU > 0 ? M::NX + M::NU : 1) : 4;
  static constexpr int value = LqrChunkHint<M>::value > 0 && LqrChunkHint<M>::value < full ? LqrChunkHint<M>::value : full;
};

// The passes of a functor that asked for narrower ones are unrolled like any (the unit seeds stay constants, and most products with
// them fold away), but they are kept apart: each pass reads its operating point through a value the compiler cannot see through -
// otherwise every value of the first pass, the same in all passes, is kept alive for the later ones - and a scheduling fence
// follows it.  HINT = 0: nothing happens.
template <int HINT> HD double lqr_pass_value(double v) {
#if defined(__HIP_DEVICE_COMPILE__)
  if constexpr (HINT > 0) asm volatile("" : "+v"(v));
#endif
  return v;
}
template <int HINT> HD void lqr_pass_fence() {
#if defined(__HIP_DEVICE_COMPILE__)
  if constexpr (HINT > 0) __builtin_amdgcn_sched_barrier(0);
#endif
}

// A = dPhi/dx (NX x NX), B = dPhi/du (NX x NU) of Phi = model_step<M>(order, nsub, .) - the map of the handle's step, roll-out and
// extended Kalman filter - and, with WANT_C, C = dh/dx (NY x NX), at (x, u, p); A, B, C: any indexable views, row-major.
template <class M, bool WANT_C, class VA, class VB, class VC>
HD void lqr_linearize(int order, int nsub, const double* x, const double* u, const double* p, double dt, const VA& A, const VB& B,
                      const VC& C) {
  constexpr int NX = M::NX, NU = M::NU, NY = M::NY, CH = LqrChunk<M>::value;
  using D = Dual<CH>;
  for (int base = 0; base < NX + NU; base += CH) {
    D xd[NX], ud[NU > 0 ? NU : 1], xn[NX];
#pragma unroll
    for (int i = 0; i < NX; ++i) {
      xd[i] = D(lqr_pass_value<LqrChunkHint<M>::value>(x[i]));
#pragma unroll
      for (int j = 0; j < CH; ++j) xd[i].d[j] = (i == base + j) ? 1.0 : 0.0;
    }
#pragma unroll
    for (int i = 0; i < NU; ++i) {
      ud[i] = D(lqr_pass_value<LqrChunkHint<M>::value>(u[i]));
#pragma unroll
      for (int j = 0; j < CH; ++j) ud[i].d[j] = (NX + i == base + j) ? 1.0 : 0.0;
    }
    model_step<M>(order, nsub, xd, ud, p, dt, xn);
#pragma unroll
    for (int i = 0; i < NX; ++i)
#pragma unroll
      for (int j = 0; j < CH; ++j) {
        const int col = base + j;
        if (col < NX) A[i * NX + col] = xn[i].d[j];
        else if (col < NX + NU) B[i * NU + (col - NX)] = xn[i].d[j];
      }
    if constexpr (WANT_C && NY > 0) {
      if (base < NX) {
        D yd[NY];
        M::meas(xd, ud, p, dt, yd);
#pragma unroll
        for (int i = 0; i < NY; ++i)
#pragma unroll
          for (int j = 0; j < CH; ++j)
            if (base + j < NX) C[i * NX + base + j] = yd[i].d[j];
      }
    }
    lqr_pass_fence<LqrChunkHint<M>::value>();
  }
}

// u = u_eq - K (x - x_eq) (x_eq, u_eq: null = zero)
template <class VK>
HD void lqr_feedback(int n, int m, const VK& K, const double* x, const double* x_eq, const double* u_eq, double* u) {
  for (int i = 0; i < m; ++i) {
    double s = 0.0;
    for (int j = 0; j < n; ++j) s += K[i * n + j] * (x[j] - (x_eq != nullptr ? x_eq[j] : 0.0));
    u[i] = (u_eq != nullptr ? u_eq[i] : 0.0) - s;
  }
}

// can the fused kernel be built for this functor?  (a model with algebraic states solves for them inside `ode` in the scalar type of
// the STATES; differentiating with respect to the inputs as well is not built)
template <class M> struct LqrModelOk {
  static constexpr bool value = M::NU > 0 && M::NX <= LQR_MAX_NX && M::NU <= LQR_MAX_NU && model_nz<M>::value == 0 && !model_has_ext<M>::value;
};

#if defined(__HIPCC__) || defined(__HIPCC_RTC__)
using LdsVec = LaneVec<lds_double*>;
using GlbVec = LaneVec<double*>;

// results of one instance to global memory; a failed instance gets NaN rows
__device__ __forceinline__ void lqr_store(int n, int m, const LqrWork<LdsVec>& w, int status, int iters, int64_t b, double* __restrict__ K,
                                          double* __restrict__ P, int* __restrict__ stats) {
  const double nan = __builtin_nan("");
  for (int i = 0; i < m * n; ++i) K[b * m * n + i] = status == LQR_OK ? (double)w.K[i] : nan;
  if (P != nullptr)
    for (int i = 0; i < n * n; ++i) P[b * n * n + i] = status == LQR_OK ? (double)w.P[i] : nan;
  if (stats != nullptr) {
    stats[b * 2 + 0] = status;
    stats[b * 2 + 1] = iters;
  }
}

// gains from given matrices: A [n x n], B [n x m] of instance b at A + b a_stride, ... (stride 0: shared by the batch); sizes are
// run-time values (one kernel for every admitted size); lds: lqr_work_doubles(n, m) * blockDim.x doubles
__device__ __forceinline__ void lqr_gain_body(lds_double* lds, int n, int m, const LqrParams& o, int64_t batch, const double* __restrict__ A,
                                              int64_t a_stride, const double* __restrict__ B, int64_t b_stride, const double* __restrict__ Q,
                                              int64_t q_stride, const double* __restrict__ R, int64_t r_stride, const double* __restrict__ N,
                                              int64_t n_stride, double* __restrict__ K, double* __restrict__ P, int* __restrict__ stats) {
  const int64_t lane = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool active = lane < batch;
  const int64_t b = active ? lane : batch - 1;   // (the solver votes: a lane past the batch works on the last instance and stores nothing)
  const LqrWork<LdsVec> w(LdsVec{lds + threadIdx.x, (int)blockDim.x}, n, m);
  for (int i = 0; i < n * n; ++i) w.A[i] = A[b * a_stride + i];
  for (int i = 0; i < n * m; ++i) w.B[i] = B[b * b_stride + i];
  int iters = 0;
  const int status = lqr_solve(n, m, o, w, Q + b * q_stride, R + b * r_stride, N != nullptr ? N + b * n_stride : nullptr, &iters);
  if (active) lqr_store(n, m, w, status, iters, b, K, P, stats);
}

// Linearise, gain and feedback of one instance per lane.  x [B, NX] (null: no feedback, u is not written), x_eq [B, NX] and u_eq
// [B, NU] the operating point (null: the origin), p rows of NP parameters (stride 0: shared); Q, R, N shared by the batch.
template <class M, class KP>
__device__ __forceinline__ void lqr_call_body(lds_double* lds, const KP& kp, const LqrParams& o, int64_t batch, const double* __restrict__ x,
                                              const double* __restrict__ x_eq, const double* __restrict__ u_eq,
                                              const double* __restrict__ p, int64_t p_stride, const double* __restrict__ Q,
                                              const double* __restrict__ R, const double* __restrict__ N, double* __restrict__ K,
                                              double* __restrict__ P, double* __restrict__ u, int* __restrict__ stats) {
  if constexpr (LqrModelOk<M>::value) {
    constexpr int NX = M::NX, NU = M::NU, NP = M::NP;
    const int64_t lane = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const bool active = lane < batch;
    const int64_t b = active ? lane : batch - 1;   // (the solver votes: a lane past the batch works on the last instance and stores nothing)
    const LqrWork<LdsVec> w(LdsVec{lds + threadIdx.x, (int)blockDim.x}, NX, NU);
    double xe[NX], ue[NU], pv[NP > 0 ? NP : 1];
#pragma unroll
    for (int i = 0; i < NX; ++i) xe[i] = x_eq != nullptr ? x_eq[b * NX + i] : 0.0;
#pragma unroll
    for (int i = 0; i < NU; ++i) ue[i] = u_eq != nullptr ? u_eq[b * NU + i] : 0.0;
#pragma unroll
    for (int i = 0; i < NP; ++i) pv[i] = p[b * p_stride + i];
    lqr_linearize<M, false>(kp.erk_order, kp.n_sub, xe, ue, pv, kp.dt, w.A, w.B, w.A);
    int iters = 0;
    const int status = lqr_solve(NX, NU, o, w, Q, R, N, &iters);
    if (active) {
      lqr_store(NX, NU, w, status, iters, b, K, P, stats);
      if (x != nullptr) {
        double xv[NX], uv[NU];
#pragma unroll
        for (int i = 0; i < NX; ++i) xv[i] = x[b * NX + i];
        lqr_feedback(NX, NU, w.K, xv, xe, ue, uv);
#pragma unroll
        for (int i = 0; i < NU; ++i) u[b * NU + i] = status == LQR_OK ? uv[i] : __builtin_nan("");
      }
    }
  }
}

// the Jacobians alone, one instance per lane, written where they go: A [B, NX, NX], B [B, NX, NU], C [B, NY, NX] (or null);
// up: rows [u; p]
template <class M, class KP>
__device__ __forceinline__ void lqr_linearize_body(const KP& kp, int64_t batch, const double* __restrict__ x, const double* __restrict__ up,
                                                   int64_t up_stride, double* __restrict__ A, double* __restrict__ B, double* __restrict__ C) {
  if constexpr (LqrModelOk<M>::value) {
    constexpr int NX = M::NX, NU = M::NU, NP = M::NP, NY = M::NY;
    const int64_t b = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (b >= batch) return;
    double xv[NX], upv[NU + NP];
#pragma unroll
    for (int i = 0; i < NX; ++i) xv[i] = x[b * NX + i];
#pragma unroll
    for (int i = 0; i < NU + NP; ++i) upv[i] = up[b * up_stride + i];
    const GlbVec Ab{A + b * NX * NX, 1}, Bb{B + b * NX * NU, 1};
    if (C != nullptr && NY > 0) lqr_linearize<M, true>(kp.erk_order, kp.n_sub, xv, upv, upv + NU, kp.dt, Ab, Bb, GlbVec{C + b * NY * NX, 1});
    else lqr_linearize<M, false>(kp.erk_order, kp.n_sub, xv, upv, upv + NU, kp.dt, Ab, Bb, Ab);
  }
}
#endif

}  // namespace hilo
