/*
 * hilo_hip.h - C ABI of libhilo_hip.so: MI355X-native batched MPC / MHE / Kalman / GP solve path.
 *
 * This is the drop-in boundary.  HILO-MPC (the reference, pure Python on CasADi) has no C ABI;
 * its boundary is a Python callable stored in `self._solver` / `self._function` at `setup()` time.  Each entry
 * point below names the reference interface it replaces (file:line relative to the reference root).
 * INTEGRATION.md shows the ctypes stub a reference maintainer would add.
 *
 * Conventions
 *  - every data pointer is a DEVICE pointer (HBM resident) unless its name ends in `_host`;
 *    hilo_malloc / hilo_memcpy_* are exported so that a binding needs nothing but this library
 *  - all floating point data is IEEE fp64 (the reference computes in fp64 throughout); indices are int32/int64
 *  - arrays are row-major with the batch index leading: [batch][...]
 *  - a `*_stride` argument is the distance in doubles between consecutive instances; 0 = shared by the batch
 *  - `stream` is a hipStream_t (NULL = default stream); calls are asynchronous w.r.t. the host unless noted
 *  - every function returns 0 on success or a negative HILO_E* code; hilo_last_error() gives the message
 *  - handles are not thread-safe; use one handle per host thread / stream
 */
#ifndef HILO_HIP_H
#define HILO_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define HILO_ABI_VERSION 1

/* error codes */
#define HILO_OK 0
#define HILO_EINVAL (-1)   /* bad argument (dimension mismatch, unknown id, NULL pointer) */
#define HILO_ENOMEM (-2)   /* device allocation failed */
#define HILO_EHIP (-3)     /* HIP runtime error */
#define HILO_ENOTSUP (-4)  /* combination not built into this library */
#define HILO_COMPILED_ONLY 1 /* not an error: with HILO_JIT_COMPILE_ONLY set in the environment, hilo_nmpc_create / hilo_kf_create of a
                               run-time compiled problem stop after compiling it into the cache (machines without a GPU: image builds) */
#define HILO_ENOTPD (-5)   /* covariance matrix K + sn2 I not positive definite (the reference adds no jitter, inference.py:206) */

/* model zoo ids (device functors in hilo_mpc_amd/csrc/hilo_models.h) */
#define HILO_MODEL_LTI 0         /* x+ = A x + B u, y = C x; p = [A|B|C] row-major (mpc.py:2198-2245 LMPC; KF) */
#define HILO_MODEL_TOY1D 1       /* tests/test_KFs.py:548-556 */
#define HILO_MODEL_BIOREACTOR3 2 /* tests/test_KFs.py:691-712 */
#define HILO_MODEL_CHEMOSTAT4 3  /* hilo_mpc/library/models.py:163-198 + rate laws :143-148 */
#define HILO_MODEL_PENDULUM4 4   /* tests/test_NMPC.py:12-43 */
#define HILO_MODEL_ROBOT6 5
#define HILO_MODEL_CSTR3 6
#define HILO_MODEL_LINEAR2 7     /* tests/test_KFs.py:247-255 */
#define HILO_MODEL_CHEMOSTAT4_GP 8 /* CHEMOSTAT4 with the biomass growth rate `mu` replaced by a GP mean over (S, I):
                                      Model.substitute_from(gp), dynamic_model.py:3040-3125 (NMPC only) */

/* solver status codes: hilo_mpc/modules/optimizer.py:1085-1104 */
#define HILO_STATUS_SOLVED 1
#define HILO_STATUS_ACCEPTABLE 2
#define HILO_STATUS_INFEASIBLE 3
#define HILO_STATUS_RESTORATION_FAILED 4
#define HILO_STATUS_MAXITER 5
#define HILO_STATUS_OTHER (-1)

/* ------------------------------------------------------------------------------------------------------- */
/* library                                                                                                  */
/* ------------------------------------------------------------------------------------------------------- */
int hilo_abi_version(void);
const char* hilo_last_error(void);           /* thread-local, valid until the next failing call */
int hilo_device_count(int* count);
int hilo_model_dims(int model_id, int* nx, int* nu, int* np, int* ny, int* discrete);

int hilo_malloc(void** dptr, uint64_t bytes, int device);
int hilo_free(void* dptr);
int hilo_memcpy_h2d(void* dst, const void* src_host, uint64_t bytes, void* stream);
int hilo_memcpy_d2h(void* dst_host, const void* src, uint64_t bytes, void* stream);
int hilo_stream_sync(void* stream);

/* ------------------------------------------------------------------------------------------------------- */
/* Kalman filters: KF / EKF / UKF                                                                           */
/* replaces the `ca.Function`s built by `_KalmanFilter.setup` (hilo_mpc/modules/estimator/kf.py:207-277):   */
/*   prediction_step(x0=[x|P], p=[u;p], Q)        kf.py:129-133 (UKF :550-554)                              */
/*   update_step(x0=[x|P](|X), y, p=[u;p], R)     kf.py:182-186 (UKF :600-604)                              */
/*   function(x0, y, p, Q, R) = update(predict())  kf.py:258-265, called from `estimate` kf.py:296-306       */
/* ------------------------------------------------------------------------------------------------------- */
#define HILO_KF_KF 0
#define HILO_KF_EKF 1
#define HILO_KF_UKF 2

typedef struct hilo_kf hilo_kf;

typedef struct hilo_kf_desc {
  int32_t model_id;   /* HILO_MODEL_* */
  int32_t kind;       /* HILO_KF_*; KF and EKF share the arithmetic (kf.py:89-96) */
  int32_t continuous; /* 0: model is (or was discretised to) a map x+ = Phi(x): P- = F P F^T + Q (kf.py:95-96)
                         1: continuous model: [x; vec P] integrated over dt (kf.py:97-110); the reference uses
                            CVODES, this library fixed-step RK4 with n_sub sub-steps */
  int32_t erk_order;  /* `Model.discretize('erk', order)` order 1..4 for continuous==0 on a continuous model */
  int32_t n_sub;      /* sub-steps per sampling interval (>=1) */
  int32_t lti_nx, lti_nu, lti_ny; /* only for HILO_MODEL_LTI */
  double dt;          /* sampling interval */
  double alpha, beta, kappa; /* UKF tuning (kf.py:446-454 defaults 1e-3, 2, 0) */
  /* model_id = HILO_MODEL_USER (100): the model is the C++ source of `struct UserModel` (the shape of csrc/hilo_models.h; what
     hilo_mpc_amd/codegen.py emits for `Model.set_dynamical_equations` / `set_measurement_equations`), compiled with hiprtc at
     create and cached like the controllers' (hilo_nmpc_desc.user_source).  NULL for the zoo models. */
  const char* user_source;
  /* learned terms of the user model (`Model.substitute_from(gp)` before `EKF(model)` / `UKF(model)` / `ParticleFilter(model)`): the
     source refers to them as hilo_user_gp[k] exactly like a controller's (hilo_nmpc_desc.user_gp); the filter gets a module
     instance of its own, so two filters compiled from the same source keep their own tables.  The GPs must outlive nothing:
     their posterior is packed at create. */
  int32_t n_user_gp;
  const struct hilo_gp* user_gp[4];   /* trained handles of hilo_gp_create (section 4) */
} hilo_kf_desc;

int hilo_kf_create(const hilo_kf_desc* desc, int device, hilo_kf** out);
/* compile the filter kernels of a model source into the cache without loading them (no GPU needed; CPU test-suite, container builds) */
int hilo_jit_precompile_kf(const char* user_source);
void hilo_kf_destroy(hilo_kf* kf);

/* Particle filter (hilo_mpc/modules/estimator/pf.py).  The reference assembles ONE function at setup() (pf.py:300-318) and
   calls it once per estimate (:372); this is that function for a batch of filters of `n_samples` particles each, on the model
   / sampling interval / discretisation of a filter handle (the `kind` of the handle is irrelevant):
       X_prop = Phi(X, u, p) + w      Y = h(X_prop, u, p) + v      q_j = normpdf(Y_j; y, sqrt(R)) / sum_j ...   (pf.py:99, :140-158)
   All particle arrays are particle-major, [B][n_samples][nx] / [B][n_samples][ny] (the memory order of CasADi's column-major
   nx x n_samples matrices); y [B][ny]; R [B][ny][ny] (r_stride 0: shared), only its diagonal is used (pf.py:155-156); a model
   without measurement equations measures all states (pf.py:131-134: ny := nx).  The random draws w, v stay with the caller
   (pf.py:364-368 draws them with numpy). */
int hilo_pf_function(hilo_kf* kf, int64_t batch, int n_samples, const double* X, const double* y,
                     const double* up, int64_t up_stride, const double* w, const double* v,
                     const double* R, int64_t r_stride, double* X_prop, double* Y, double* q, void* stream);
/* `ind = np.random.choice(N, size=N, replace=True, p=q); X = X[:, ind]; Y = Y[:, ind]` (pf.py:404-407) with the caller's
   uniform draws in [0, 1) - numpy's own algorithm: index = searchsorted(cumsum(q) / sum(q), u, side='right').
   uniforms [B][n_samples]; index (int32) [B][n_samples]; n_samples <= 8192. */
int hilo_pf_resample(hilo_kf* kf, int64_t batch, int n_samples, const double* X_prop, const double* Y, const double* q,
                     const double* uniforms, double* X, double* Y_out, int32_t* index, void* stream);
/* Statistics of the particle set (pf.py:409-420): x_mean [B][nx], y_mean [B][ny], P = np.cov(X) [B][nx][nx] (unbiased),
   x_min / x_max [B][nx] (the spread the roughening scales its noise with).  `add` (NULL or [B][n_samples][nx]) is added to
   the particles first: the roughening step `X += dx` (pf.py:415). */
int hilo_pf_stats(hilo_kf* kf, int64_t batch, int n_samples, double* X, const double* Y, const double* add,
                  double* x_mean, double* y_mean, double* P, double* x_min, double* x_max, void* stream);
/* The whole of `ParticleFilter.estimate` (pf.py:340-422) for `steps` steps of a batch of filters in ONE launch, every random number
   drawn on the device (the reference draws with numpy on the host, pf.py:364-368, :404-415, and stops at steps > 1, pf.py:360).
   A draw is a pure function of (seed, filter, absolute step, particle, purpose): Philox4x32-10 with key (seed low, seed high) on the
   counter (j, k, b + filter_offset, stream << 16 | d) - j the particle, k = step0 + the step within the call, b the filter, d the
   block; streams 0 initial sample (k = 0), 1 process noise, 2 measurement noise, 3 resampling, 4 roughening.  One output
   (r0, r1, r2, r3) gives u1 = (((r0 >> 5) << 26 | r1 >> 6) + 0.5) 2^-53 and u2 likewise from (r2, r3); normals 2d and 2d+1 of a
   vector are sqrt(-2 ln u1) cos(2 pi u2) and sqrt(-2 ln u1) sin(2 pi u2) of block d.  Per step:
     X_prop = Phi(X, u, p) + L_Q z (pf.py:140-146; L_Q the lower Cholesky factor of Q, a non-positive pivot zeroes its column)
     Y = h(X_prop, u, p) + sqrt(diag R) z (pf.py:131-138)
     q_j proportional to exp(l_j - max l), l_j the log-likelihood of particle j (pf.py:148-166 up to rounding wherever the
       reference's weights are finite); ess = 1 / sum q_j^2
     resampling (pf.py:404-407): numpy's `choice` on u1 of block 0 per particle, or with HILO_PF_SYSTEMATIC u_j = (j + u) / N from
       the one uniform of particle 0
     HILO_PF_ROUGHENING (pf.py:409-415): particle j gains sqrt(K (max_i - min_i) N^(-1/nx)) z_i in state i
     x = mean, P = np.cov, y = mean of the resampled measurements (pf.py:418-420)
   X [B][n_samples][nx] in and out (particle-major); P0 not NULL: X is drawn first as x0 [B][nx] + L_P0 z, P0 [B][nx][nx]
   (pf.py:168-188).  work [B][n_samples][nx + ny]: scratch (the propagated particles and their measurements).  y [steps][B][ny];
   [u; p] of step k and filter b at up + k up_step + b up_stride (0: held / shared); Q, R as for hilo_pf_function.
   x_out [steps][B][nx], P_out [steps][B][nx][nx], y_out [steps][B][ny], ess_out [steps][B]; index_out [steps][B][n_samples] or
   NULL; X_prop_out, Y_out, q_out: the last step's intermediates, each may be NULL.  status [B][2] (code, step): written once, when
   a filter's code still is 0 - HILO_PF_STATUS_NOT_FINITE: the weights of that step were not finite (NaN measurement or state, or
   every particle infinitely far); the step then leaves the propagated particles unresampled (index = identity) and the run goes
   on.  n_samples 2..8192 (up to 64: one wave per filter, four filters per workgroup; above: one workgroup per filter), nx <= 16. */
#define HILO_PF_SYSTEMATIC 1
#define HILO_PF_ROUGHENING 2
#define HILO_PF_STATUS_NOT_FINITE 1
typedef struct hilo_pf_opts {
  uint64_t seed;
  int64_t step0;          /* absolute number of the first step of this call */
  int64_t filter_offset;  /* global number of filter 0 of this batch */
  int32_t flags;          /* HILO_PF_* */
  int32_t reserved;
  double K;               /* read with HILO_PF_ROUGHENING */
} hilo_pf_opts;
int hilo_pf_run(hilo_kf* kf, const hilo_pf_opts* opts, int64_t batch, int n_samples, int steps, double* X, double* work,
                const double* y, const double* up, int64_t up_stride, int64_t up_step, const double* Q, int64_t q_stride,
                const double* R, int64_t r_stride, const double* x0, const double* P0, double* x_out, double* P_out,
                double* y_out, double* ess_out, int32_t* index_out, double* X_prop_out, double* Y_out, double* q_out,
                int32_t* status, void* stream);
/* widths of the packed tiles: xp = nx+1 ([x|P]); pred = nx+1 (KF/EKF) or 1+nx+(2nx+1) (UKF [x|P|X]) */
int hilo_kf_dims(const hilo_kf* kf, int* nx, int* nu, int* np, int* ny, int* pred_width);

int hilo_kf_predict(hilo_kf* kf, int64_t batch,
                    const double* xP,                 /* [B][nx][nx+1] */
                    const double* up, int64_t up_stride, /* [B][nu+np] = vertcat(u, p) (kf.py:130) */
                    const double* Q, int64_t q_stride,   /* [B][nx][nx] */
                    double* pred,                     /* [B][nx][pred_width] */
                    void* stream);
int hilo_kf_update(hilo_kf* kf, int64_t batch,
                   const double* pred,                /* [B][nx][pred_width] */
                   const double* y,                   /* [B][ny] */
                   const double* up, int64_t up_stride,
                   const double* R, int64_t r_stride, /* [B][ny][ny] */
                   double* xP_out,                    /* [B][nx][nx+1] */
                   double* y_pred,                    /* [B][ny] */
                   void* stream);
/* one `estimate()` step: update(predict(.)), fused in one kernel */
int hilo_kf_step(hilo_kf* kf, int64_t batch, const double* xP, const double* y,
                 const double* up, int64_t up_stride, const double* Q, int64_t q_stride,
                 const double* R, int64_t r_stride, double* xP_out, double* y_pred, void* stream);

/* `steps` estimate() steps in ONE launch: `self._function.mapaccum(steps)` (kf.py:296-306).  y [steps][B][ny]; inputs / parameters
   the same for every step (up_step_stride = 0) or [steps][B][nu+np] (up_step_stride = elements between two steps); Q, R as
   for a single step.  keep_all != 0: xP_out [steps][B][nx][nx+1] holds the tile after every step (what mapaccum returns), else
   [B][nx][nx+1] the last one; y_pred [steps][B][ny]. */
int hilo_kf_steps(hilo_kf* kf, int64_t batch, int steps, const double* xP, const double* y,
                  const double* up, int64_t up_stride, int64_t up_step_stride, const double* Q, int64_t q_stride,
                  const double* R, int64_t r_stride, double* xP_out, int keep_all, double* y_pred, void* stream);
/* The same with the inputs u [steps or 1][B][nu] and the parameters p [B][np] in their OWN arrays (strides in doubles; 0 = one row   */
/* shared by the batch) - they are separate arguments of the reference's function (kf.py:130), and a binding need not pack them.    */
int hilo_kf_steps_split(hilo_kf* kf, int64_t batch, int steps, const double* xP, const double* y,
                        const double* u, int64_t u_stride, int64_t u_step_stride, const double* p, int64_t p_stride,
                        const double* Q, int64_t q_stride, const double* R, int64_t r_stride, double* xP_out, int keep_all,
                        double* y_pred, void* stream);

/* Roll-out: `steps` sampling intervals of `batch` instances of the handle's model in ONE launch - the plant simulation of
   `Model.simulate` (hilo_mpc/modules/dynamic_model/dynamic_model.py:3911-4000) for batches (the `kind` of the handle is
   irrelevant).  opts NULL or method 0: the handle's own map x+ = Phi(x, u, p) - a discrete model, or the explicit Runge-Kutta
   recipe of `discretize` (the arithmetic of hilo_pf_function without noise).  method HILO_SIM_DOPRI5: a continuous model
   integrated with the Dormand-Prince 5(4) pair under step-size control (csrc/hilo_integrate.h: error norm and controller of
   scipy's RK45), where the reference integrates with CVODES; inputs are held over a sampling interval, the step size is carried
   across sampling instants, and every sampling instant is hit exactly.  HILO_ENOTSUP for method 1 on a discrete handle, and for a
   model of more than HILO_SIM_DOPRI5_MAX_NX states or a run-time compiled one whose kernel needs scratch memory (the pair keeps its
   slopes in registers).  method HILO_SIM_BDF: a continuous model integrated with variable-order (1..5) backward differentiation
   formulas, step size and order chosen per instance (csrc/hilo_integrate.h: scipy's BDF statement by statement, the Jacobian
   exact) - the method for a stiff model.  Inputs held over the roll-out (up_step 0): one integration whose state is carried across
   the sampling instants, which are read off the interpolant, only the end of the roll-out clips a step; an input sequence: one
   integration per sampling interval from order 1.  HILO_ENOTSUP for method 2 on a discrete handle, and for a model of more than
   HILO_SIM_BDF_MAX_NX states or a run-time compiled one whose kernel needs scratch memory.
     x0 [B][nx];  up rows [u; p] like hilo_kf_steps: up_stride between instances (0: shared), up_step between sampling intervals
     (0: held over the roll-out, else [steps][B][nu+np]);  X [steps+1][B][nx] (row 0 is x0);  Y [steps][B][ny] = h(x_{k+1}, u_k, p)
     or NULL;  stats [B][4] int32 (status, accepted steps, rejected steps, right-hand-side evaluations) or NULL.
   An instance whose integration fails - more than max_steps attempted steps within ONE sampling interval
   (HILO_SIM_STATUS_MAX_STEPS; HILO_SIM_BDF: between two consecutive sampling instants), or a step below 16 eps |t| (HILO_SIM_BDF: ten
   spacings of t) (HILO_SIM_STATUS_STEP_TOO_SMALL) - ends with that status, and its rows
   from the sampling instant it did not reach onwards are NaN; the other instances are not affected and the call returns HILO_OK.
   Time.  A run-time compiled model may name the time t in its equations (a functor that declares TIME_VARIANT).  opts->t0 (NULL
   opts: 0) is the time of row 0 of X, one value for the batch; sampling interval k starts at t_k = t0 + k dt.  Over the interval a
   continuous model's right-hand side is f(t_k + tau, x, u_k, p), tau in [0, dt] - the inputs are held, time is not: stage i of a
   Runge-Kutta sub-step of length h that starts at s is evaluated at s + c_i h, HILO_SIM_DOPRI5 uses the stage times of scipy's RK45,
   HILO_SIM_BDF evaluates fun(t_new, y) and the Jacobian df/dx at the current (t, x), with inputs held on the clock of its one
   integration plus t0, with an input sequence restarted at every t_k - and Y[k] = h(t_k + dt, x_{k+1}, u_k, p).  A discrete model's
   map and measurement of interval k both see t_k: x_{k+1} = f(t_k, x_k, u_k, p), Y[k] = h(t_k, x_{k+1}, u_k, p).  The smallest
   admissible step is measured against the absolute time.  Every other entry that takes a filter handle - hilo_kf_*,
   hilo_pf_function, hilo_model_linearize, hilo_lqr_call - returns HILO_ENOTSUP for a time-variant model. */
#define HILO_SIM_MAP 0
#define HILO_SIM_DOPRI5 1
#define HILO_SIM_DOPRI5_MAX_NX 12
#define HILO_SIM_BDF 2
#define HILO_SIM_BDF_MAX_NX 8
#define HILO_SIM_STATUS_OK 0
#define HILO_SIM_STATUS_MAX_STEPS 1
#define HILO_SIM_STATUS_STEP_TOO_SMALL 2
typedef struct hilo_sim_opts {
  int32_t method;     /* HILO_SIM_* */
  int32_t max_steps;  /* attempted steps per sampling interval (<= 0: 10000) */
  double rtol, atol;  /* <= 0: 1e-6, 1e-8 */
  double h0;          /* first step (<= 0: estimated) */
  double t0;          /* time of row 0 of X, one value for the batch (read by a time-variant model only) */
} hilo_sim_opts;
int hilo_model_rollout(hilo_kf* kf, const hilo_sim_opts* opts, int64_t batch, int steps, const double* x0,
                       const double* up, int64_t up_stride, int64_t up_step, double* X, double* Y, int32_t* stats,
                       void* stream);
/* The same roll-out as one piece of a longer one.  h [B] (device) or NULL: the step-size proposal of HILO_SIM_DOPRI5 per instance -
   an entry > 0 is the first step that instance tries (any other: opts->h0, or the estimate), and every entry is overwritten with
   the proposal the instance ended with.  Inputs unchanged, a second call that starts from the last row of X, at the time
   t0 + steps dt, with the h the first call left takes the steps ONE call over both stretches would have taken: the proposal
   is all the pair carries across a sampling instant (the slope at the start is evaluated again, at the same time and state).
   The other methods ignore h.  HILO_ENOTSUP for a non-NULL h with HILO_SIM_DOPRI5 on a model of the zoo: the run-time compiled
   kernels alone hand the proposal on. */
int hilo_model_rollout_resume(hilo_kf* kf, const hilo_sim_opts* opts, int64_t batch, int steps, const double* x0,
                              const double* up, int64_t up_stride, int64_t up_step, double* X, double* Y, int32_t* stats,
                              double* h, void* stream);
/* The roll-out of a model with algebraic states, dx/dt = f(x, z, u, p), 0 = g(x, z, u, p) (semi-explicit, index 1), under
   HILO_SIM_IDAS: variable-order (1..5) backward differentiation formulas in the combined vector [x; z], where the reference
   integrates such a model with IDAS (csrc/hilo_integrate.h::idas_interval: the method of HILO_SIM_BDF, the algebraic rows of the
   Newton system unscaled, the error test over all components).  opts->method must be HILO_SIM_IDAS; the other fields as above
   (t0 is not read: such a model does not name the time).
     z0 [B][nz] or NULL: where the Newton iteration for the consistent initial z starts (NULL: the guess compiled into the model);
     Z [steps+1][B][nz] or NULL: the algebraic states at the sampling instants, row 0 the consistent initial values;
     Y [steps][B][ny] = h(x_{k+1}, z_{k+1}, u_k, p) on the pair written to X and Z;  every other argument as for hilo_model_rollout.
   At the start, and with an input sequence at every sampling instant, z is made consistent by Newton's method (at most 40 sweeps);
   an instance for which that fails - no convergence, a singular dg/dz, a non-finite value - ends with
   HILO_SIM_STATUS_IC_FAILED.  The same status ends an instance at ANY sampling instant at which the correction of the interpolated z
   onto g(x, z) = 0 - the same iteration with the same exit test, residual at most 1e-13 (1 + |z|) - does not get there, for
   instance with a badly scaled g; its rows are NaN from that instant on.  Rows of X, Z and Y from the first instant an instance did not reach are NaN (a failure at the very
   start: from row 1 of X and row 0 of Z).  HILO_ENOTSUP for a handle whose model has no algebraic states, for nx + nz >
   HILO_SIM_BDF_MAX_NX, for a kernel that needs scratch memory and for a method other than HILO_SIM_IDAS. */
#define HILO_SIM_IDAS 3
#define HILO_SIM_STATUS_IC_FAILED 3
int hilo_model_rollout_dae(hilo_kf* kf, const hilo_sim_opts* opts, int64_t batch, int steps, const double* x0,
                           const double* z0 /* [batch][nz] or NULL */, const double* up, int64_t up_stride, int64_t up_step,
                           double* X, double* Z /* [steps+1][batch][nz] or NULL */, double* Y, int32_t* stats, void* stream);

/* The HILO_SIM_DOPRI5 roll-out with FORWARD SENSITIVITIES: next to x the kernel integrates S = dx / d theta, theta = [x0; u; p]
   restricted to the groups of `wrt` (HILO_SENS_X0 | HILO_SENS_U | HILO_SENS_P; columns in the order x0, u, p of the selected groups,
   NS of them), as the augmented system dS/dt = f_x S + f_theta, S(0) = [I | 0 | 0], with the same pair and controller - what
   scipy's RK45 does when handed [x; vec S], and what a CasADi integrator's forward sensitivities are in the reference.  The error
   norm runs over all nx (1 + NS) components, each with its own scale atol + rtol max(|.|, |.+|), so the step sequence is NOT that of
   hilo_model_rollout and X differs from its X within the tolerance; stats count one evaluation of the augmented right-hand side
   as one (n_rhs == 6 (accepted + rejected) + 2).  One instance runs on a team of T lanes, T the smallest power of two >= NS
   (csrc/hilo_integrate.h::rollout_sens_body); derivatives come from the model functor on dual numbers.
     opts->method must be HILO_SIM_DOPRI5; the other fields, x0, up, up_stride, up_step, X, Y, stats as for hilo_model_rollout;
     SX [steps+1][B][NS][nx]: column j of S at every sampling instant as nx contiguous doubles (row 0: the seed);
     SY [steps][B][NS][ny] = h_x S + h_theta at the end of each interval, or NULL.
   With an input sequence (up_step != 0) the columns of x0 and p go on across the sampling instants; HILO_SENS_U is refused there
   (every interval's input would be a parameter of its own).  A failed instance gets NaN in SX / SY wherever it gets NaN in X.
   HILO_ENOTSUP for another method, a discrete or discretised handle, a model with a learned term or with algebraic states, more than
   HILO_SIM_SENS_MAX_NX states, NS > 64, HILO_SENS_U with an input sequence, and a run-time compiled model whose kernel needs scratch
   memory; HILO_EINVAL for a `wrt` that selects no column. */
#define HILO_SENS_X0 1
#define HILO_SENS_U 2
#define HILO_SENS_P 4
#define HILO_SIM_SENS_MAX_NX 4
int hilo_model_rollout_sens(hilo_kf* kf, const hilo_sim_opts* opts, int64_t batch, int steps, const double* x0, const double* up,
                            int64_t up_stride, int64_t up_step, int32_t wrt, double* X, double* Y, double* SX, double* SY,
                            int32_t* stats, void* stream);

/* ------------------------------------------------------------------------------------------------------- */
/* PID: the batched law and closed loops of controller and plant in one launch                              */
/* replaces `PID.setup / call` (hilo_mpc/modules/controller/pid.py:244-365)                                 */
/* ------------------------------------------------------------------------------------------------------- */
/* The velocity-form law per loop j (csrc/hilo_pid.h::pid_update): with e = sp - pv on three-sample windows,
     delta = e[-1] - e[-2] (HILO_PID_P_ON_PV: -(pv[-1] - pv[-2])) + dt / t_i e[-1]
             + t_d / dt (e[-1] - 2 e[-2] + e[-3]) (HILO_PID_D_ON_PV: -t_d / dt (pv[-1] - 2 pv[-2] + pv[-3]))
     u = u_prev + k_p delta, with HILO_PID_LIMITS clamped to [lo[j], hi[j]]; the clamped value is the next u_prev (anti-windup)
   A loop's memory is HILO_PID_MEM doubles - pv[-2], pv[-1], sp[-2], sp[-1], u_prev - all zero after a reset; the set-point history
   starts at zero like the reference's, so the first call sees a set-point step.  nsp loops, at most HILO_PID_MAX_LOOPS.
   pv_index / pv_is_state / out_index are read by hilo_pid_loop alone: loop j controls measurement number pv_index[j] of the
   plant - or, with pv_is_state[j], state number pv_index[j] - through input number out_index[j]. */
#define HILO_PID_MAX_LOOPS 4
#define HILO_PID_MEM 5
#define HILO_PID_P_ON_PV 1
#define HILO_PID_D_ON_PV 2
#define HILO_PID_LIMITS 4
typedef struct hilo_pid_opts {
  int32_t nsp;
  int32_t flags;                              /* HILO_PID_* */
  int32_t pv_index[HILO_PID_MAX_LOOPS];
  int32_t pv_is_state[HILO_PID_MAX_LOOPS];
  int32_t out_index[HILO_PID_MAX_LOOPS];
  double lo[HILO_PID_MAX_LOOPS], hi[HILO_PID_MAX_LOOPS];   /* read with HILO_PID_LIMITS */
} hilo_pid_opts;
/* One call of the law for a batch (no handle; on the current device), one loop per lane: pv [B][nsp] (NULL: zeros); the set points
   sp at sp + b sp_stride and the gains - rows k_p [nsp], t_i [nsp], t_d [nsp] - at gains + b gain_stride (a stride of 0: shared by
   the batch); mem [B][nsp][HILO_PID_MEM] updated in place; u [B][nsp]. */
int hilo_pid_call(const hilo_pid_opts* opts, int64_t batch, double dt, const double* pv, const double* sp, int64_t sp_stride,
                  const double* gains, int64_t gain_stride, double* mem, double* u, void* stream);
/* The closed loop in ONE launch, one instance per lane (csrc/hilo_pid.h::pid_loop_instance): per sampling interval k the process
   values - the selected measurements h(t_k, x[k], u_applied, p) or states, u_applied the input vector of the previous interval (at
   k = 0 the held inputs with the driven entries taken from the memory's u_prev) - the law with the set points of interval k at
   sp + k sp_step + b sp_stride (either 0: held / shared), the driven entries of the input vector overwritten (the others keep the
   held value of `up`, one row [u; p] per instance, up_stride 0: shared), and the plant advanced as hilo_model_rollout advances it.
     sim     as for hilo_model_rollout; HILO_SIM_MAP and HILO_SIM_DOPRI5 alone (an input that jumps every interval would restart
             the implicit methods every interval): HILO_ENOTSUP for the others
     X [steps + 1][B][nx], U [steps][B][nsp] the controller outputs, Y [steps][B][ny] = h(x[k + 1], u[k], p): each may be NULL
     J [B][nsp][4]   ISE = sum e_k^2 dt, IAE = sum |e_k| dt, ITAE = sum (k dt) |e_k| dt, TVU = sum |u_k - u_{k-1}|
     x_final [B][nx], mem left where the loop ended, stats [B][4] or NULL as for hilo_model_rollout
     h [B] or NULL: the step-size proposal of HILO_SIM_DOPRI5, taken over where positive and written back
   An instance whose integration fails gets NaN rows from the instant it did not reach, NaN in J and x_final.  HILO_EINVAL for
   nsp outside 1..min(nu, HILO_PID_MAX_LOOPS) and selectors out of range; HILO_ENOTSUP for a model with algebraic states and a
   run-time compiled model whose kernel needs scratch memory under HILO_SIM_DOPRI5. */
int hilo_pid_loop(hilo_kf* kf, const hilo_sim_opts* sim, const hilo_pid_opts* opts, int64_t batch, int steps, const double* x0,
                  const double* up, int64_t up_stride, const double* sp, int64_t sp_stride, int64_t sp_step, const double* gains,
                  int64_t gain_stride, double* mem, double* X, double* U, double* Y, double* J, double* x_final, int32_t* stats,
                  double* h, void* stream);

/* ------------------------------------------------------------------------------------------------------- */
/* Data generation: excitation signals, plant and data set in one launch                                   */
/* replaces `DataGenerator.random_uniform / random_normal / chirp / run` (hilo_mpc/util/data.py:642-1167)   */
/* ------------------------------------------------------------------------------------------------------- */
/* One instance per lane (csrc/hilo_datagen.h::datagen_instance): per sampling interval k = 0..total_steps-1 the input vector u_k is
   evaluated inside the kernel, the plant advanced as hilo_model_rollout advances it under an input sequence, and the states
   scattered into features and labels in training layout.
     kind   HILO_DATAGEN_UNIFORM  a staircase, sample s = k / hold: u_i = fma(b_i - a_i, U, a_i)            (a: lower, b: upper bound)
            HILO_DATAGEN_NORMAL   the same with u_i = fma(sqrt(b_i), Z, a_i)                                (a: mean, b: variance)
            HILO_DATAGEN_CHIRP    chirp_table [nu][HILO_DATAGEN_MAX_SEG][8] on the device, a segment being {type (0 linear,
                                  1 exponential, 2 hyperbolic), point count, amplitude, mean, chirp rate, initial phase, initial
                                  frequency, initial frequency ratio}; the local time of a segment is i dt from its start; the point
                                  counts of every input must add up to total_steps (the host's duty)
     draws  Philox4x32-10 on the counter (0, index, b + instance_offset, stream << 16 | d), key (seed low, seed high); block d
            supplies values 2d and 2d+1; index = s for inputs (value i: input i), = j for the noise on state j (value i: state i,
            key from noise_seed[i]); streams 8 / 9 input uniforms / normals, 10 / 11 noise uniforms / normals
     noise  per state: 0 none, 1 uniform n = fma(nb - na, U, na), 2 normal n = na Z
     F [N][B][(shift + 1) nk + nu], L [N][B][nk], N = total_steps - shift, nk the states not in skip_mask: the noisy kept state
            xt_j = x_j + n_j goes to row j - s, block s (s = 0..shift); u_k to row k - shift, last block; the label of row
            j - shift - 1 is xt_j, with `difference` (x_j - x_{j-1}) + (n_j - n_{j-1})
     X [total_steps + 1][B][nx] the clean states, U [total_steps][B][nu], stats [B][4] as for hilo_model_rollout: each may be NULL
   up: one row [u; p] per instance (up_stride 0: shared); its inputs are not read.  An instance whose integration fails gets NaN in
   every entry made of a state it did not reach.  HILO_EINVAL for arguments out of range; HILO_ENOTSUP for HILO_SIM_BDF /
   HILO_SIM_IDAS, a model with algebraic states, more than HILO_DATAGEN_MAX_NX states or HILO_DATAGEN_MAX_NU inputs, a model without
   inputs, and a run-time compiled model whose kernel needs scratch memory under HILO_SIM_DOPRI5. */
#define HILO_DATAGEN_MAX_NU 4
#define HILO_DATAGEN_MAX_NX 12
#define HILO_DATAGEN_MAX_SEG 8
#define HILO_DATAGEN_UNIFORM 0
#define HILO_DATAGEN_NORMAL 1
#define HILO_DATAGEN_CHIRP 2
typedef struct hilo_datagen_opts {
  uint64_t seed;
  int64_t instance_offset;                  /* global number of instance 0 of this batch */
  int32_t kind, hold;                       /* HILO_DATAGEN_*; sampling intervals per sample of a staircase */
  int32_t shift, difference;
  int32_t skip_mask, reserved;              /* bit i: state i is left out */
  double a[HILO_DATAGEN_MAX_NU], b[HILO_DATAGEN_MAX_NU];
  int32_t noise_kind[HILO_DATAGEN_MAX_NX];
  uint64_t noise_seed[HILO_DATAGEN_MAX_NX];
  double na[HILO_DATAGEN_MAX_NX], nb[HILO_DATAGEN_MAX_NX];
} hilo_datagen_opts;
int hilo_datagen_run(hilo_kf* kf, const hilo_sim_opts* sim, const hilo_datagen_opts* opts, const double* chirp_table, int64_t batch,
                     int total_steps, const double* x0, const double* up, int64_t up_stride, double* F, double* L, double* X,
                     double* U, int32_t* stats, void* stream);

/* ------------------------------------------------------------------------------------------------------- */
/* Linear-quadratic regulator: batched linearisation, Riccati gains and feedback                            */
/* replaces `LinearQuadraticRegulator.setup / call` (hilo_mpc/modules/controller/lqr.py:204-306)            */
/* ------------------------------------------------------------------------------------------------------- */
/* The gain of x+ = A x + B u under the cost sum x'Qx + u'Ru + 2 x'Nu, one instance per lane (csrc/hilo_lqr.h):
     horizon > 0   lqr.py:236-245: from P = Q, `horizon` steps P <- A'PA - (A'PB + N)(R + B'PB)^-1 (B'PA + N') + Q, then
                   K = (R + B'PB)^-1 (B'PA + N')  (Cholesky factorisation of R + B'PB)
     horizon = 0   the stationary gain (the reference: NotImplementedError): the discrete algebraic Riccati equation by the
                   structure-preserving doubling algorithm, at most max_iter steps, until max|H+ - H| <= tol max(1, max|H+|)
   Per-instance status: 0 ok; HILO_LQR_STATUS_MAX_ITER: max_iter doubling steps without convergence; HILO_LQR_STATUS_FAILED: an iterate
   that is not finite, a singular I + G H, or R + B'PB not positive definite.  An instance with a non-zero status gets NaN rows in K, P
   and u; the other instances are not affected and the call returns HILO_OK.  stats [B][2] int32: status, steps made.
   All matrices row-major.  HILO_ENOTSUP for more than HILO_LQR_MAX_NX states or HILO_LQR_MAX_NU inputs, for a handle whose model is
   continuous and was not discretised (the gains are discrete-time), for a model without inputs or with algebraic states, and for
   a run-time compiled model whose kernels need scratch memory. */
#define HILO_LQR_MAX_NX 8
#define HILO_LQR_MAX_NU 4
#define HILO_LQR_STATUS_OK 0
#define HILO_LQR_STATUS_MAX_ITER 1
#define HILO_LQR_STATUS_FAILED 2
typedef struct hilo_lqr_opts {
  int32_t horizon;   /* backward Riccati steps; 0 = stationary */
  int32_t max_iter;  /* doubling steps (<= 0: 50) */
  double tol;        /* (<= 0: 1e-12) */
} hilo_lqr_opts;
/* A = dPhi/dx [B][nx][nx], B = dPhi/du [B][nx][nu] and, unless NULL, C = dh/dx [B][ny][nx] of the handle's map x+ = Phi(x, u, p) - the
   one of hilo_pf_function, hilo_model_rollout and the extended Kalman filter - at x [B][nx] and the rows [u; p] of `up` (up_stride
   between instances, 0: shared), in forward mode. */
int hilo_model_linearize(hilo_kf* kf, int64_t batch, const double* x, const double* up, int64_t up_stride, double* A,
                         double* B, double* C, void* stream);
/* Gains from given matrices (no handle; on the current device): A [nx][nx], B [nx][nu], Q [nx][nx], R [nu][nu], N [nx][nu] (NULL: zero)
   of instance b at A + b a_stride, ... (a stride of 0: shared by the batch); opts NULL: stationary with the defaults.
   K [B][nu][nx]; P [B][nx][nx] the Riccati solution, or NULL; stats or NULL. */
int hilo_lqr_gain(int nx, int nu, int64_t batch, const double* A, int64_t a_stride, const double* B, int64_t b_stride,
                  const double* Q, int64_t q_stride, const double* R, int64_t r_stride, const double* N, int64_t n_stride,
                  const hilo_lqr_opts* opts, double* K, double* P, int32_t* stats, void* stream);
/* Linearise, gain and feedback in ONE launch (the gain-scheduled path): the Jacobians of the handle's map at the operating point
   x_eq [B][nx], u_eq [B][nu] (NULL: the origin) with the parameters p (rows of np, p_stride between instances, 0: shared), the gain
   for Q, R, N (shared by the batch; N NULL: zero), and u [B][nu] = u_eq - K (x - x_eq) for x [B][nx].  x and u both NULL: the
   gains alone.  K, P, stats as above. */
int hilo_lqr_call(hilo_kf* kf, const hilo_lqr_opts* opts, int64_t batch, const double* x, const double* x_eq,
                  const double* u_eq, const double* p, int64_t p_stride, const double* Q, const double* R, const double* N,
                  double* K, double* P, double* u, int32_t* stats, void* stream);
/* u [B][nu] = u_eq - K (x - x_eq) with a gain computed before: K at K + b k_stride (0: one gain for the batch); x_eq, u_eq [B][.] or
   NULL (zero). */
int hilo_lqr_apply(int nx, int nu, int64_t batch, const double* K, int64_t k_stride, const double* x, const double* x_eq,
                   const double* u_eq, double* u, void* stream);

/* ------------------------------------------------------------------------------------------------------- */
/* Gaussian process: exact inference + prediction                                                           */
/* replaces `ca.Function('prediction',[X,w,p],[mean,var])` (hilo_mpc/modules/machine_learning/gp/gp.py:      */
/* 623-629, called from `predict` gp.py:709) whose body is `ExactInference.get_posterior`                   */
/* (gp/inference.py:172-221) over `Kernel.__call__` (gp/kernel.py:97-205) and `Mean.__call__` (mean.py:90)  */
/* ------------------------------------------------------------------------------------------------------- */
/* kernel / mean programs: postfix list of nodes, each node = [opcode, n_active, active_dims..., n_par, par...]
   stored as doubles.  opcodes: */
#define HILO_K_CONST 0       /* par: c = bias^2                                      kernel.py:465-485 */
#define HILO_K_GAMMAEXP 1    /* par: sf2, alpha, p/2, M[n_active]  (SE: .5, 1)       kernel.py:650-701 */
#define HILO_K_MATERN 2      /* par: sf2, sqrt(2nu), ncoef, coef..., M[n_active]     kernel.py:783-826 */
#define HILO_K_RQ 3          /* par: sf2, alpha, M[n_active]                         kernel.py:972-1003 */
#define HILO_K_PP 4          /* par: sf2, q, j, M[n_active]                          kernel.py:1069-1109 */
#define HILO_K_POLY 5        /* par: sf2, offset, degree                             kernel.py:1202-1234 */
#define HILO_K_NN 6          /* par: sf2, w                                          kernel.py:1309-1332 */
#define HILO_K_PERIODIC 7    /* par: 2*log(sf), l, period  (1 active dim)            kernel.py:1394-1423 */
#define HILO_K_SUM 16        /* pops 2                                               kernel.py:1562-1593 */
#define HILO_K_PRODUCT 17    /* pops 2                                               kernel.py:1596-1627 */
#define HILO_K_POWER 18      /* par: power; child evaluated at (x,x)                 kernel.py:1630-1666 */
#define HILO_M_CONST 32      /* par: bias                                            mean.py:280-305 */
#define HILO_M_POLY 33       /* par: offset, degree, coef[n_active]                  mean.py:422-470 */
#define HILO_M_SUM 48
#define HILO_M_PRODUCT 49
#define HILO_M_POWER 50      /* par: power */
#define HILO_M_SCALE 51      /* par: scale */

typedef struct hilo_gp hilo_gp;

/* Builds K(X,X) + sn2 I, its Cholesky factor, alpha and the log marginal likelihood on the device
   (inference.py:199-210).  X_train is feature-major [nf][n] exactly like the reference's X (gp.py:605). */
int hilo_gp_create(int device, int nf, int n,
                   const double* X_train_host,  /* [nf][n] */
                   const double* y_train_host,  /* [n] */
                   const double* kprog_host, int kprog_len,
                   const double* mprog_host, int mprog_len,
                   double noise_variance,       /* sn2 = exp(2 * log sqrt(noise_variance)) (inference.py:199) */
                   hilo_gp** out);
void hilo_gp_destroy(hilo_gp* gp);
int hilo_gp_log_marginal_likelihood(hilo_gp* gp, double* lml_host);
/* New hyper-parameters on the same training data (one objective value of `GaussianProcess.fit_model`, gp.py:660-697): uploads
   the kernel program (same length: the kernel structure is fixed) and the noise variance, re-factorises into the handle's
   buffers.  Returns HILO_ENOTPD at an indefinite trial point (the handle then needs another refit before it predicts). */
int hilo_gp_refit(hilo_gp* gp, const double* kprog_host, int kprog_len, double noise_variance);
/* New hyper-parameters of the mean function (`Mean` hyper-parameters are fitted together with the kernel's, gp.py:408-414): same
   program length; the next hilo_gp_refit evaluates the mean with them. */
int hilo_gp_set_mean_program(hilo_gp* gp, const double* mprog_host, int mprog_len);
/* Gradient of the log marginal likelihood (inference.py:210) at the handle's current hyper-parameters by the trace formula
   1/2 tr((alpha alpha^T - K_y^-1) dK_y/dtheta_j) on the device, one factorisation for all j.  Per theta_j the
   caller passes the kernel programs and noise variances at theta +- h_j e_j (HOST: [n_theta][2][kprog_len], [n_theta][2],
   [n_theta]); dK_y/dtheta_j is their central difference, evaluated element-wise inside the trace kernel. */
int hilo_gp_lml_gradient(hilo_gp* gp, int n_theta, const double* kprogs_pm_host, const double* noise_pm_host,
                         const double* h_host, double* grad_host);
/* gp.py:699-718.  Xq feature-major [nf][m]; mean/var [m]; var may be NULL (mean only). */
int hilo_gp_predict(hilo_gp* gp, int64_t m, const double* Xq, int noise_free, double* mean, double* var,
                    void* stream);
/* covariance matrix only (Kernel.__call__, kernel.py:97-140): K [n1][n2] for feature-major X1 [nf][n1], X2 [nf][n2] */
int hilo_gp_kernel_matrix(int device, int nf, const double* kprog_host, int kprog_len, int64_t n1,
                          const double* X1, int64_t n2, const double* X2, double* K, void* stream);
int hilo_gp_mean(int device, int nf, const double* mprog_host, int mprog_len, int64_t n, const double* X,
                 double* mu, void* stream);

/* Hyper-parameter fits of many GPs in ONE launch (GPArray.fit_model): a problem is one training set with one start point, one
   workgroup maximises its log marginal likelihood (inference.py:210) by BFGS with Armijo backtracking entirely on the device.
   theta = logarithms of the free hyper-parameter values, theta[0] = log(noise variance).  The device rebuilds the kernel
   program from theta through the slot map: program[slot] = exp(coef * theta[index]) (HILO_GPFIT_EXP) or coef * theta[index]
   (HILO_GPFIT_LIN); every other entry keeps the value of `kprog`.  The mean program is evaluated as given.
   Limits: n <= HILO_GPFIT_MAX_N, n_theta <= HILO_GPFIT_MAX_THETA, kprog_len <= HILO_GPFIT_MAX_PROG, n_map <= HILO_GPFIT_MAX_MAP
   (HILO_ENOTSUP beyond them); the device workspace is 2 n^2 doubles per problem (HILO_ENOMEM with the byte count when it does not
   fit).  All pointers are HOST pointers. */
#define HILO_GPFIT_EXP 0
#define HILO_GPFIT_LIN 1
#define HILO_GPFIT_MAX_N 256
#define HILO_GPFIT_MAX_THETA 16
#define HILO_GPFIT_MAX_PROG 256
#define HILO_GPFIT_MAX_MAP 64
/* status per problem */
#define HILO_GPFIT_CONVERGED 0     /* max |d LML / d theta| <= gtol */
#define HILO_GPFIT_MAXITER 1
#define HILO_GPFIT_LINESEARCH 2    /* no decrease within 40 halvings, or step * g.d no longer changes the objective's value */
#define HILO_GPFIT_START_NOT_PD 3  /* K + sn2 I at theta0 not positive definite or LML not finite: only the status is written */
typedef struct hilo_gp_fit_problem {
  int32_t nf, n;                 /* X is feature-major [nf][n] */
  int32_t kprog_len, mprog_len;
  int32_t n_theta, n_map;
  const double* X;               /* [nf][n] */
  const double* y;               /* [n] */
  const double* kprog;           /* [kprog_len] kernel program at any admissible hyper-parameters (the fixed ones count) */
  const double* mprog;           /* [mprog_len] */
  const int32_t* map_slot;       /* [n_map] index into kprog of a parameter entry */
  const int32_t* map_theta;      /* [n_map] index into theta */
  const int32_t* map_kind;       /* [n_map] HILO_GPFIT_EXP / HILO_GPFIT_LIN */
  const double* map_coef;        /* [n_map] */
  const double* theta0;          /* [n_theta] start point */
} hilo_gp_fit_problem;
typedef struct hilo_gp_fit_opts {
  int32_t maxiter;               /* 0 = evaluate only: LML and gradient at theta0 */
  int32_t reserved;
  double gtol;
} hilo_gp_fit_opts;
/* theta_out, grad_out: [n_problems][HILO_GPFIT_MAX_THETA] (the first n_theta entries of a row are written; grad = d LML / d theta at
   theta_out); lml_out, iters_out, nfev_out, status_out: [n_problems].  A problem's result does not depend on the batch it runs
   in nor on its position (fixed reduction order, no atomics). */
int hilo_gp_fit_batch(int device, int n_problems, const hilo_gp_fit_problem* problems, const hilo_gp_fit_opts* options,
                      double* theta_out, double* lml_out, double* grad_out, int32_t* iters_out, int32_t* nfev_out,
                      int32_t* status_out, void* stream);

/* ------------------------------------------------------------------------------------------------------- */
/* NMPC: batched direct multiple shooting + interior point                                                  */
/* replaces `ca.nlpsol('solver','ipopt',{'f','x','p','g'})` built at hilo_mpc/modules/controller/mpc.py:      */
/* 1778-1787 and called as `solver(x0=v0, lbx, ubx, lbg, ubg, p)` at mpc.py:722 by `NMPC._optimize`; the       */
/* transcription it embodies is mpc.py:1455-1787 for a pre-discretised model + `integration_method='discrete'`  */
/* ------------------------------------------------------------------------------------------------------- */
typedef struct hilo_nmpc hilo_nmpc;

typedef struct hilo_nmpc_desc {
  int32_t model_id;     /* HILO_MODEL_* */
  int32_t N;            /* prediction horizon (mpc.py `horizon`) */
  int32_t Nc;           /* control horizon (mpc.py:1629-1630); 0 = N.  Nc < N needs user_policy 2 (run-time compiled) */
  int32_t erk_order;    /* `model.discretize('rk4')` = 4, `('erk', order)` = 1..4 (modeling.py:1239-1250) */
  int32_t n_sub;        /* sub-steps per interval (1 = the reference's single ERK step) */
  int32_t max_iter;     /* 0 -> 3000 (IPOPT default) */
  int32_t acceptable_iter; /* 0 -> 15 */
  int32_t reserved;
  double dt;            /* sampling interval (mpc.py:511) */
  double tol;           /* 0 -> 1e-8 */
  double acceptable_tol;/* 0 -> 1e-6 */
  double mu_init;       /* 0 -> 0.1 */
  double bound_relax_factor; /* < 0 -> 1e-8 (IPOPT default); 0 disables */
  /* HOST pointers, all optional (NULL = zero weight / no bound / unit scaling / zero guess).
     Quadratic costs in the form QuadraticCost builds (modeling.py:243-283), on scaled z = (x, u):
       stage: (z - zref)^T Wz (z - zref);  terminal: (x - xrefN)^T WN (x - xrefN);
       input change (only interval 0, mpc.py:1631-1635): (u_0 - u_old)^T Wdu (u_0 - u_old) */
  const double* Wz;     /* [nz][nz], nz = nx+nu */
  const double* zref;   /* [nz]  already divided by the scaling (modeling.py:310) */
  const double* WN;     /* [nx][nx] */
  const double* xrefN;  /* [nx] */
  const double* Wdu;    /* [nu][nu] */
  const double* x_lb; const double* x_ub; const double* u_lb; const double* u_ub;  /* original units */
  const double* x_scaling; const double* u_scaling;                                /* optimizer.py:1476-1506 */
  const double* x_guess; const double* u_guess;                                    /* original units */
  /* learned term of the model (`Model.substitute_from(gp)`, dynamic_model.py:3040-3125): required for
     HILO_MODEL_CHEMOSTAT4_GP (label `mu`, features S, I; the posterior mean is copied at create), else NULL */
  const hilo_gp* learned;
  /* ---- path following (mpc.py:1025-1053 `create_path_variable`, :1173-1204): at most one path variable theta.  It
     becomes state index nx with the virtual input u_theta (input index nu), theta+ = theta + dt u_theta (:1191);
     theta_0 is a free bounded variable (:785-789 pins only the original states).  Path cost terms
     (x[idx] - r(theta))^T W (x[idx] - r(theta)) (hilo_mpc/util/modeling.py:252-283), stage and terminal. ---- */
  int32_t n_path_var;                    /* 0 or 1 */
  int32_t has_u_pf_ref;                  /* adds (u_theta - u_pf_ref)^2 u_pf_weight to the stage cost (:1202-1204) */
  double theta_guess, theta_lb, theta_ub, u_pf_lb, u_pf_ub, u_pf_ref, u_pf_weight;
  int32_t n_path_stage, n_path_term;     /* tracked states per cost, <= 4 each */
  const int32_t* path_stage_idx; const double* path_stage_W;   /* [n], [n][n] */
  const int32_t* path_term_idx;  const double* path_term_W;
  const double* path_prog;               /* n_path_stage + n_path_term expression programs r(theta) (HILO_X_*) */
  int32_t path_prog_len;
  /* ---- nonlinear stage constraint lb <= c(x_k,u_k) <= ub, k = 0..N-1 (`GenericConstraint`, modeling.py:820-1005;
     mpc.py:1271-1283, :1700-1725), on un-scaled variables (modeling.py:843-849).  soft: one slack vector e >= 0 shared by
     all stages (mpc.py:1529-1537), rows c - e <= ub, -c - e <= -lb, e^T W e added once per stage (:1708); e is appended
     to the decision vector. ---- */
  int32_t n_con;                         /* expressions, <= 2 */
  int32_t con_soft;
  int32_t con_prog_len;
  const double* con_prog;                /* n_con programs in the model states (VARX), inputs (VARU), parameters */
  const double* con_lb; const double* con_ub;      /* [n_con]; -inf / +inf allowed */
  const double* con_weight;              /* [n_con][n_con] or NULL -> 1e4 I (modeling.py:875) */
  const double* con_max_violation;       /* [n_con] or NULL -> inf */
  /* terminal constraint; hard: lb <= c_T(x_end) <= ub on the integrated end state Phi(x_{N-1}, u_{N-1}) (mpc.py:1693-1700;
     `nmpc.terminal_constraint`), un-scaled states; its rows sit between the last defect and the last stage rows in g */
  int32_t n_tcon;                        /* expressions, n_con + n_tcon rows <= 4 in this build */
  int32_t tcon_prog_len;
  const double* tcon_prog;
  const double* tcon_lb; const double* tcon_ub;
  /* soft terminal constraint (mpc.py:1684-1692): c_T(x_{N-1}) - e_T <= ub, -c_T(x_{N-1}) - e_T <= -lb on the state the last
     interval starts from, one slack e_T in [0, max_violation] after the stage slack in v (mpc.py:1540-1548), e_T^T W e_T once
     in the objective.  One shared slack in total in this build: n_tcon = 1 and the stage constraint hard or absent. */
  int32_t tcon_soft; int32_t reserved4;
  const double* tcon_weight;             /* [n_tcon][n_tcon] or NULL -> 1e4 I */
  const double* tcon_max_violation;      /* [n_tcon] or NULL -> inf */
  /* ---- integration_method = 'collocation' on the CONTINUOUS model (the reference's default, optimizer.py:1410-1418;
     hilo_mpc/util/modeling.py:1091-1211, mpc.py:1307-1372): degree d Lagrange basis at Radau / Legendre points.  The caller
     passes the basis it built (modeling.py:1091-1127): coll_A = (C[1:,1:]^T)^-1 (d x d, the method's Runge-Kutta matrix)
     and coll_D = D[0..d].  v gains the collocation states ([x | u | ip], mpc.py:1497-1518), g the collocation rows
     (per stage [collocation rows | continuity], :1657-1669).  0 = explicit Runge-Kutta / discrete model. ---- */
  int32_t collocation_degree;            /* 0, or 3 (1..4 for chemostat4) in this build */
  int32_t reserved2;
  const double* coll_A;                  /* [d][d] */
  const double* coll_D;                  /* [d+1] */
  /* ---- per-stage data: trajectory-tracking references (mpc.py:365-463; modeling.py:262-283) and time-varying parameters
     (mpc.py:335-364, optimizer.py:905-929).  With time_varying != 0 the handle is solved through hilo_nmpc_solve_tv. ---- */
  int32_t time_varying;
  int32_t reserved3;
  /* ---- models and problem functions compiled at RUN TIME (what `Model.set_dynamical_equations` /
     `nmpc.stage_cost.cost = ...` accept as CasADi graphs in the reference, dynamic_model.py:1293-1553, modeling.py:38-87).
     `user_source` is HIP source text that defines, inside namespace hilo,
        UserModel   a functor shaped like the zoo of csrc/hilo_models.h (NX, NU, NP, NY, DISCRETE, templated `ode`, `meas`),
                    or an alias of a zoo functor (`using UserModel = Chemostat4;`)
        UserFun     (user_has_fun != 0) the problem's free-form functions, csrc/hilo_nmpc_user.h: generic stage / terminal
                    cost on the SCALED variables (see that header for the reference quirk), constraint expressions on the
                    un-scaled ones, path references
     It is compiled with hiprtc for gfx950 against the engine headers that ship next to the library (csrc/), the code object
     is cached (HILO_JIT_CACHE or <library dir>/jit_cache).  model_id = HILO_MODEL_USER takes the model from the source;
     a zoo model_id with user_source set compiles the general policy for that zoo functor.
     user_policy: 0 = the tracking policy (same code path as the zoo models), 1 = the general policy with expression
     programs (path following / constraints as above), 2 = the policy of csrc/hilo_nmpc_user.h, which adds: generic costs,
     the continuous objective, collocation together with path following, control horizon Nc < N, per-stage data. ---- */
  const char* user_source;
  int32_t user_nx, user_nu, user_np, user_ny, user_discrete;   /* dimensions of UserModel (checked against the compiled code) */
  int32_t user_has_fun;
  int32_t user_policy;
  int32_t objective_continuous;   /* 1: integrate the Lagrange term with the shooting map (optimizer.py:1423-1426) */
  const double* coll_B;           /* [d+1] quadrature weights B_i of the collocation basis (modeling.py:1124), continuous objective */
  /* learned terms of a run-time compiled model (`Model.substitute_from(gp)`, dynamic_model.py:3040-3125): up to 4 trained GPs
     (squared-exponential kernel over up to 8 features, constant / zero mean); the emitted model refers to them as
     gp_se_mean(hilo_user_gp[k], features) (csrc/hilo_models.h) */
  int32_t n_user_gp;
  int32_t user_nz;                /* algebraic states of the user model (semi-explicit DAE, `set_algebraic_states`): the source's
                                     UserModel::NZ; v / g gain the z blocks and rows of mpc.py:1488-1518 (collocation only) */
  const hilo_gp* user_gp[4];
  /* with user_policy 2 the constraint / path expressions are compiled into UserFun: n_con, n_tcon, n_path_stage, n_path_term
     count them as above, the *_prog pointers stay NULL */
  /* user_policy 2: structural sparsity of the Hessian of an interval's Lagrangian, [mza][mza] bytes over the augmented model
     z = [x, theta | u, u_theta] (1 = the entry can be non-zero; symmetric; NULL = dense).  CasADi evaluates only the non-zero
     Hessian entries of the graph it is given (mpc.py:1778-1787); here a zero entry drops the Taylor sweep of its direction. */
  const unsigned char* hess_pattern;
  double max_hessian_perturbation;   /* IPOPT option of that name (delta_w^max of W&B Alg. IC, default 1e20 there, 1e40 here =
                                        the oracle's): beyond it the inertia correction gives up -> status 4; <= 0 keeps the default */
  /* finite bounds on algebraic states (`set_box_constraints(z_lb=, z_ub=)`, mpc.py:645-701 -> the box of the zp blocks of v,
     :1512-1518): UserFun::con evaluates n_zbound further expressions behind the n_con constraint expressions - the bounded
     algebraic states - which become rows at the collocation points only (the algebraic states are eliminated);
     they do not appear in lam_g */
  int32_t n_zbound;
  int32_t x0_free_mask;    /* run-time compiled problems: bit i set = component i of the model state x_0 is NOT pinned to the measured
                              state but a variable inside the state box (the sampling-interval state of a minimum-time problem,
                              hilo_mpc_amd/nmpc.py::_setup_min_time); 0 = all of x_0 is pinned (mpc.py:785-789) */
  const double* zb_lb; const double* zb_ub;        /* [n_zbound]; -inf / +inf allowed on one side */
  /* custom constraint function over the whole decision vector (`set_custom_constraints_function`, optimizer.py:1180-1208; rows
     lb <= fun(v, x_ind, u_ind) <= ub at the END of g, mpc.py:1729-1745), in the stage-additive form the host derives from it
     (hilo_mpc_amd/custom.py):  c_r(v) = sum_{k=0..N} sum_j acc_coef[r][k][j] psi_j(x_k, u_k)  with the n_acc_expr expressions psi_j
     compiled into UserFun::acc (user_policy 2).  Each of the n_acc rows is carried by an accumulator state of the engine and becomes
     a hard row on the end of the horizon (csrc/hilo_nmpc_user.h): hilo_nmpc_dims reports n_v INCLUDING the n_acc hidden accumulator
     entries at the end of v, and the rows are the last n_acc TERMINAL rows of g / lam_g (in front of the last node's stage rows);
     the reference appends them to g (mpc.py:1744-1745) - hilo_mpc_amd/nmpc.py::_g_order is that permutation. */
  int32_t n_acc, n_acc_expr;
  const double* acc_coef;      /* [n_acc][N + 1][n_acc_expr] */
  const double* acc_lb; const double* acc_ub;      /* [n_acc] bounds of the rows (constant parts of the function already removed) */
  /* soft = True (mpc.py:1551-1556, :1731-1740): one slack e_cus per row in [0, max_violation] BEHIND the other slacks in v,
     1e4 e_cus^T e_cus once in the objective, and two rows per function in g: fun - e_cus <= ub, then fun + e_cus >= lb (rows with an
     infinite bound are not imposed and keep a zero multiplier) */
  int32_t acc_soft;
  const double* acc_max_violation;                 /* [n_acc] or NULL -> inf */
} hilo_nmpc_desc;

#define HILO_MODEL_USER 100    /* model defined by desc.user_source */
/* Compile a user problem into the cache without loading it (no GPU needed): what `__graft_entry__.build()` uses to pre-warm
   the cache, and what the CPU test-suite uses to check that generated sources compile for gfx950. */
int hilo_jit_precompile(const char* user_source, int policy, int nth, int ne, int nc, int coll_d, int N, int hold, int cont,
                        int tv, int big, int has_fun);

/* expression programs: [len, (op, arg) * len/2] back to back; postfix, stack of 8 */
#define HILO_X_CONST 0   /* arg = value */
#define HILO_X_VARX 1    /* arg = state index */
#define HILO_X_VARU 2    /* arg = input index */
#define HILO_X_VARP 3    /* arg = parameter index */
#define HILO_X_ADD 10
#define HILO_X_SUB 11
#define HILO_X_MUL 12
#define HILO_X_DIV 13
#define HILO_X_NEG 14
#define HILO_X_SQ 15
#define HILO_X_SIN 16
#define HILO_X_COS 17
#define HILO_X_EXP 18
#define HILO_X_LOG 19
#define HILO_X_SQRT 20
#define HILO_X_POWI 21   /* arg = integer exponent in [-16, 16] */

int hilo_nmpc_create(const hilo_nmpc_desc* desc, int device, hilo_nmpc** out);   /* = NMPC.setup(), mpc.py:1789 */
void hilo_nmpc_destroy(hilo_nmpc* h);
int hilo_nmpc_dims(const hilo_nmpc* h, int* n_v, int* n_g, int* nx, int* nu, int* np);
int hilo_nmpc_reset_warm_start(hilo_nmpc* h);
/* The other two vectors of the reference's solver result (`self._nlp_solution = sol`, mpc.py:722-723): bound multipliers
   lam_x [batch][n_v] (layout of v; CasADi's sign z_U - z_L; 0 for the pinned x_0) and constraint values g [batch][n_g] (layout
   of lam_g; written when the solve is given a lam_g buffer).  DEVICE buffers the following solves write, or NULL to stop.
   Layouts with a collocation output pass do not fill them (HILO leaves the buffers untouched). */
int hilo_nmpc_set_aux_outputs(hilo_nmpc* h, double* g, double* lam_x);
/* Sharded batches (one process per GPU, hilo_mpc_amd/dist.py): let the solve write row b = [u0 (nu) | status | iterations]
   (fp64) of the device table [batch][stride] itself - the send buffer of the per-step result gather.  NULL switches it off.
   Honoured by plain tracking problems; the reference has no counterpart (single instance, no batching). */
int hilo_nmpc_set_gather(hilo_nmpc* h, double* table, int stride);
/* Closed loops whose plant is the controller's own model (benchmarks, simulations; hilo_nmpc_plant_step): the solve advances the
   plant itself - row b of x_next [B][nx] receives Phi(x0_b, u_0, p_b) for the input it has just computed (one launch per step
   instead of two).  x_next may be the x0 buffer of the call (in-place closed loop); NULL switches it off.  HILO_ENOTSUP for problem
   kinds whose kernel does not offer it (general / run-time compiled policies, the hybrid model, long horizons). */
int hilo_nmpc_set_plant_out(hilo_nmpc* h, double* x_next);
/* lbx / ubx of the reference's solver call, `self._solver(x0=v0, lbx=self._v_lb, ubx=self._v_ub, ...)` (mpc.py:722): DEVICE rows
   [batch][n_v] in the layout of v (scaled variables, original bound values: IPOPT's bound_relax_factor is applied by the solve),
   read by every following hilo_nmpc_solve; NULL, NULL = back to the bounds of the description.  Per instance and per call, so that
   a caller can move bounds between steps as the reference does (mpc.py:797-807).  The entries of a pinned x_0 are ignored (the
   solve pins x_0 to the `x0` argument, which is what mpc.py:801-802 writes into both arrays); lb < ub elsewhere. */
int hilo_nmpc_set_var_bounds(hilo_nmpc* h, const double* lbx, const double* ubx);
/* optimize(fix_x0=...) of mpc.py:797-807: 1 (default) pins x_0 to the measured state; 0 leaves x_0 free inside the state
   box [x_lb, x_ub] (the `x0` argument of hilo_nmpc_solve is then ignored, the start value comes from the warm start / guess).
   Synchronises the device when the setting changes. */
int hilo_nmpc_set_fix_x0(hilo_nmpc* h, int fix_x0);
/* optimize(fix_x0=False, x0_lb=..., x0_ub=...) of mpc.py:803-807: an own box for x_0 (HOST pointers [nx], original units;
   NULL / NULL restores the state box).  Synchronises the device when the setting changes. */
int hilo_nmpc_set_x0_box(hilo_nmpc* h, const double* x0_lb_host, const double* x0_ub_host);
/* One optimize() for `batch` independent instances (mpc.py:744-857).
   v layout = the reference's decision vector [x_0..x_N | u_0..u_{N-1}] in scaled variables (mpc.py:1462-1485). */
int hilo_nmpc_solve(hilo_nmpc* h, int64_t batch,
                    const double* x0,                 /* [B][nx]  measured state, original units (mpc.py:801) */
                    const double* p, int64_t p_stride,/* [B][np]  constant parameters `cp` (mpc.py:496-497) */
                    const double* v0,                 /* [B][n_v] initial guess or NULL -> previous solution
                                                         (warm start, mpc.py:725-726) / tiled guess (:1468-1482) */
                    const double* u_old,              /* [B][nu]  previous input for the change penalty or NULL */
                    double* v_opt,                    /* [B][n_v] */
                    double* f_opt,                    /* [B] */
                    double* lam_g,                    /* [B][n_g] multipliers of g (sign: L = f + lam^T g) or NULL */
                    double* u0,                       /* [B][nu]  first input, un-scaled (mpc.py:856) */
                    int32_t* status,                  /* [B] HILO_STATUS_* (optimizer.py:1093-1104) */
                    int32_t* iters,                   /* [B] interior-point iterations */
                    double* kkt,                      /* [B] scaled optimality error at the returned point or NULL */
                    void* stream);
/* optimize() with per-stage data (handles created with desc.time_varying): stage_data[b][k] = [zref_k (nz, scaled like the
   references of QuadraticCost, modeling.py:329) | p_k (np)] for k = 0..N; row N holds the terminal reference in its first nx
   entries.  sd_stride = 0 shares one table among the batch, else >= (N+1)(nz+np).  The constant references of the desc are
   not used. */
int hilo_nmpc_solve_tv(hilo_nmpc* h, int64_t batch, const double* x0, const double* stage_data, int64_t sd_stride,
                       const double* v0, const double* u_old, double* v_opt, double* f_opt, double* lam_g, double* u0,
                       int32_t* status, int32_t* iters, double* kkt, void* stream);
/* developer aid: per-phase shader-clock totals of instance 0 (derivatives, errors, Riccati, step, line search,
   update, number of factorisations, number of line-search trial points, then the two per-launch slots: setup =
   everything in front of the first iteration, finish = the write-back); enable != 0 starts collecting,
   cycles_host[10] (may be NULL) receives the last launch's counters */
int hilo_nmpc_profile(hilo_nmpc* h, int enable, long long* cycles_host);
/* the capacity horizon of a precompiled tracking model's LDS layout (taylor != 0: of its form with Taylor sweeps): the largest
   horizon whose per-instance footprint stays within 40 KB - 64 B, so that four instances share a CU.  Horizons up to n_cap run
   on a kernel whose array offsets are compile-time constants and request lds_cap bytes; lds_next: the footprint at n_cap + 1.
   Needs no device. */
int hilo_nmpc_layout_capacity(int model_id, int taylor, int* n_cap, long long* lds_cap, long long* lds_next);
/* developer aid: one wave runs the interior-point engine's n-value wave reduction in its transposing and its plain form on the
   same lane values.  n in 1..8; ops[n] (host): 0 sum, 1 NaN-propagating maximum, 2 minimum, 3 plain maximum - only the mixes
   compiled in are accepted (HILO_EINVAL otherwise); in[64][n], out_new[n], out_plain[n] device memory */
int hilo_ocp_reduce_selftest(int n, const int* ops, const double* in, double* out_new, double* out_plain, void* stream);
/* developer aid: every operation of the derivative arithmetic (csrc/hilo_ad.h) at n points in each scalar type - double, FastD,
   Dual<1>, Dual<12>, Jet2.  in[n][7] = operation (AD_* of csrc/hilo_ad_selftest.h), a, b, da, db, dda, ddb; out[n][20] in the layout
   stated there; device memory */
int hilo_ad_selftest(int64_t n, const double* in, double* out, void* stream);
/* developer aid: the postfix interpreter (csrc/hilo_expr.h) on its own, for 4 states, 2 inputs and 3 parameters.  block (HOST,
   block_len doubles): `count` programs back to back, validated like a solver's; program `which` is evaluated at n points in double
   and in Jet2.  in[n][18] = x[4] dx[4] ddx[4] u[2] du[2] ddu[2], p[3], out[n][4] = value, then Jet2 v a b; device memory.
   Returns after the launch has finished. */
int hilo_expr_selftest(const double* block, int block_len, int count, int which, int64_t n, const double* in, const double* p,
                       double* out, void* stream);
/* developer aid: a model given as source (`struct UserModel`, the form the controllers and filters take) evaluated on its own at n
   points, in a small run-time compiled unit apart from the filter unit: ode and meas in double, FastD, Dual<nx+nu> seeded with the
   identity and Jet2 along a direction, and - where the source carries them - the generated jx / jh / mjh.  trig_calls != 0 compiles
   sine and cosine behind calls (HILO_TRIG_CALLS, as the filter unit does).  Row layouts of in / out: csrc/hilo_jit.hip;
   flags[2] (device): the source has symbolic derivatives, and their measurement part.  Returns after the launch has finished. */
int hilo_jit_probe(const char* user_source, int trig_calls, int nx, int nu, int np, int ny, int64_t n, const double* in, double* out,
                   int* flags, void* stream);
/* x+ = Phi(x, u, p) with the controller's own shooting map: closed-loop harness (control_loop.py:343-396) */
int hilo_nmpc_plant_step(hilo_nmpc* h, int64_t batch, const double* x, const double* u, const double* p,
                         int64_t p_stride, double* x_next, void* stream);

/* ------------------------------------------------------------------------------------------------------- */
/* MHE: batched moving-horizon estimation                                                                   */
/* replaces `ca.nlpsol("solver",'ipopt',...)` built at hilo_mpc/modules/estimator/mhe.py:782-790 and called as */
/* `solver(x0=v0, lbx, ubx, lbg, ubg, p=param)` at mhe.py:375 by `MovingHorizonEstimator.estimate`; transcription  */
/* mhe.py:596-760 for a pre-discretised model + `integration_method='discrete'`, state noise, pinned parameters   */
/* ------------------------------------------------------------------------------------------------------- */
typedef struct hilo_mhe hilo_mhe;

typedef struct hilo_mhe_desc {
  int32_t model_id, N, erk_order, n_sub, max_iter, acceptable_iter;
  double dt, tol, acceptable_tol, mu_init, bound_relax_factor;   /* 0 / <0 -> IPOPT defaults, see hilo_nmpc_desc */
  /* HOST pointers (NULL = zero weight / no bound / unit scaling / zero guess); costs act on un-scaled quantities
     (hilo_mpc/util/modeling.py:665-672) */
  const double* Wx;   /* [nx][nx] arrival weight   (modeling.py:747-777, mhe.py:742-745) */
  const double* Wy;   /* [ny][ny] measurement weight (modeling.py:686-712) */
  const double* Ww;   /* [nx][nx] state-noise weight (modeling.py:735-745); NULL: an estimator WITHOUT state noise (no w block in v,
                         mhe.py:599) - models given as source (user_source) */
  const double* x_lb; const double* x_ub; const double* w_lb; const double* w_ub;   /* original units */
  const double* x_scaling; const double* w_scaling; const double* u_scaling;
  const double* x_guess; const double* w_guess;
  /* ---- parameter estimation (mhe.py:614-623: the parameters head the decision vector with bounds p_lb / p_ub and guess
     p_guess; arrival term (p - p_arrival)^T Wp (p - p_arrival), modeling.py:747-777).  estimate_parameters = 0: all
     parameters are pinned to the `p` handed to hilo_mhe_estimate.  != 0: parameter j is estimated iff p_lb[j] < p_ub[j]
     (NULL bound = unbounded = estimated), `p` then carries p_arrival for the estimated and the value for the pinned ones;
     the estimate is the prefix of v_opt (scaled by p_scaling). ---- */
  int32_t estimate_parameters;
  int32_t reserved;
  const double* Wp;          /* [np][np] */
  const double* p_lb; const double* p_ub; const double* p_scaling; const double* p_guess;   /* [np], original units */
  /* ---- run-time compiled estimator (round 3): the model as HIP source of `UserModel` (hilo_nmpc_desc.user_source: the
     functor emitted from the model's expressions, or the alias of a zoo functor), compiled with hiprtc around the estimator's
     policy at create (what `MovingHorizonEstimator.setup` -> `ca.nlpsol` does with the CasADi graph, mhe.py:782-790).
     model_id = HILO_MODEL_USER takes the dimensions below.  collocation_degree > 0: the reference's DEFAULT transcription
     (mhe.py:512-561; needs a continuous model and user_source): v gains the collocation block behind the noise block,
     [p | x | w | ip_0..ip_{N-1}] (mhe.py:657-671), lam_g the per-stage rows [collocation (d nx) | continuity (nx)]. ---- */
  const char* user_source;
  int32_t user_nx, user_nu, user_np, user_ny, user_discrete, collocation_degree;
  const double* coll_A;      /* [d][d]  Runge-Kutta matrix of the collocation method (hilo_nmpc_desc.coll_A) */
  const double* coll_D;      /* [d + 1] continuity weights */
  /* ---- stage constraint of the estimator (`mhe.stage_constraint`, mhe.py:498-508, :536-553, :749-757): n_con expressions of the
     SCALED states and parameters, compiled into `UserFun::con(x, p, c)` behind UserModel in user_source; hard rows
     con_lb <= c <= con_ub at every node k < N and, under collocation, at every collocation point.  (The reference's soft branch
     cannot run in its estimator: the penalty function is never created.) ---- */
  int32_t n_con; int32_t reserved6;
  const double* con_lb; const double* con_ub;   /* [n_con]; -inf / +inf allowed on one side */
} hilo_mhe_desc;

int hilo_mhe_create(const hilo_mhe_desc* desc, int device, hilo_mhe** out);          /* = setup(), mhe.py:418 */
void hilo_mhe_destroy(hilo_mhe* h);
int hilo_mhe_dims(const hilo_mhe* h, int* n_v, int* n_g, int* nx, int* nu, int* np, int* ny);
int hilo_mhe_reset_warm_start(hilo_mhe* h);
/* One estimate() for `batch` independent estimators over a full window (mhe.py:311-416).
   v layout = the reference's decision vector [p | x_0..x_N | w_0..w_{N-1} (| collocation states)] (scaled, mhe.py:614-671). */
int hilo_mhe_estimate(hilo_mhe* h, int64_t batch,
                      const double* x_arrival,            /* [B][nx]   arrival guess, original units (mhe.py:347-351) */
                      const double* p, int64_t p_stride,  /* [B][np]   pinned model parameters */
                      const double* u_meas,               /* [B][N][nu] = param['u_meas'] transposed (mhe.py:361-362) */
                      const double* y_meas,               /* [B][N][ny] = param['y_meas'] transposed (mhe.py:358-359) */
                      const double* v0,                   /* [B][n_v] or NULL -> previous solution (mhe.py:385) / guess */
                      double* v_opt, double* f_opt, double* lam_g,
                      double* x_opt,                      /* [B][nx]  x_N un-scaled: one-step-ahead state (mhe.py:381-384) */
                      int32_t* status, int32_t* iters, double* kkt, void* stream);

/* ------------------------------------------------------------------------------------------------------- */
/* LMPC: batched dense convex QP                                                                            */
/* replaces `ca.conic("solver",'qpoases',{'h': H.sparsity(),'a': Aeq.sparsity()})` built at                    */
/* hilo_mpc/modules/controller/mpc.py:2268-2276 and called as                                                */
/* `solver(h=H, g=g, a=Ad, lbx=v_lb, ubx=v_ub, lba=Ad_lb, uba=Ad_ub)` at mpc.py:2374 by `LMPC.optimize`         */
/*     min 1/2 x^T H x + g^T x   s.t.  lba <= A x <= uba (rows must be equalities),  lbx <= x <= ubx          */
/* ------------------------------------------------------------------------------------------------------- */
typedef struct hilo_qp hilo_qp;
int hilo_qp_create(int n, int m, int device, hilo_qp** out);
void hilo_qp_destroy(hilo_qp* h);
int hilo_qp_set_options(hilo_qp* h, double tol /* <=0 keeps 1e-12 */, int max_iter /* <=0 keeps 100 */);
/* The QP has the stage shape of `LMPC.setup` (mpc.py:2198-2266): v = [x_0 .. x_N | u_0 .. u_{N-1}], H block diagonal over the  */
/* stages (:2252-2256), rows k: A_k x_k + B_k u_k - x_{k+1} = b_k (:2209-2240; NOT the `kron(B, I_N)` input block of :2243),      */
/* x_0 - and only x_0 - pinned by lbx == ubx (:2361-2362).  hilo_qp_solve then takes its Newton steps by a Riccati recursion over */
/* the stages (csrc/hilo_qp_ocp.h) instead of the dense Schur complement; same arguments, same iteration, same outputs.          */
/* *used = 1 if a stage kernel exists for (nx, nu, N <= 63), 0 = the dense kernels stay.  N = 0 withdraws the declaration.        */
int hilo_qp_set_stages(hilo_qp* h, int nx, int nu, int N, int* used);
int hilo_qp_solve(hilo_qp* h, int64_t batch,
                  const double* H, int64_t h_stride,       /* [B][n][n] row-major (stride 0 = shared) */
                  const double* g, int64_t g_stride,       /* [B][n] */
                  const double* A, int64_t a_stride,       /* [B][m][n] */
                  const double* lbx, const double* ubx, int64_t bx_stride, /* [B][n]; lbx == ubx pins a variable */
                  const double* lba, const double* uba, int64_t ba_stride, /* [B][m] */
                  double* x,                               /* [B][n] */
                  double* f,                               /* [B] */
                  double* lam_a,                           /* [B][m] or NULL;  H x + g + A^T lam_a + lam_x = 0 */
                  double* lam_x,                           /* [B][n] or NULL */
                  int32_t* status, int32_t* iters, void* stream);
/* The same solve with the first `npin` variables FIXED at xpin[b][0..npin) - what `LMPC.optimize` does with the measured state:    */
/* `self._lbx[:nx] = self._ubx[:nx] = x0` before every solver call (mpc.py:2361-2362).  lbx / ubx may then be ONE row shared by the   */
/* batch (bx_stride = 0); their first npin entries are not read.  One launch per step instead of two bound-row writes + the solve.    */
int hilo_qp_solve_pinned(hilo_qp* h, int64_t batch, const double* H, int64_t h_stride, const double* g, int64_t g_stride,
                         const double* A, int64_t a_stride, const double* lbx, const double* ubx, int64_t bx_stride,
                         const double* xpin, int npin, int64_t xpin_stride /* >= npin */, const double* lba, const double* uba,
                         int64_t ba_stride, double* x, double* f, double* lam_a, double* lam_x, int32_t* status, int32_t* iters,
                         void* stream);

/* ------------------------------------------------------------------------------------------------------- */
/* ANN: batched inference of a feed-forward network                                                         */
/* replaces `ArtificialNeuralNetwork.predict` (hilo_mpc/modules/machine_learning/nn/nn.py:536-544): input     */
/* scaling (x - mean) / scale, dense layers h <- act(W h + b), a linear output layer, output scaling           */
/* y * scale + mean - the chain `net_to_casadi_graph` writes (util/machine_learning.py:521-578).             */
/* One fused kernel on the f64 matrix cores (csrc/hilo_ann.hip); training stays with the caller's framework.   */
/* ------------------------------------------------------------------------------------------------------- */
#define HILO_ANN_ACT_LINEAR 0
#define HILO_ANN_ACT_SIGMOID 1
#define HILO_ANN_ACT_TANH 2
#define HILO_ANN_ACT_RELU 3
#define HILO_ANN_ACT_SOFTPLUS 4
#define HILO_ANN_MAX_FEATURES 32
#define HILO_ANN_MAX_LABELS 16
#define HILO_ANN_MAX_WIDTH 64
#define HILO_ANN_MAX_HIDDEN 8
#define HILO_ANN_MAX_LDS_BYTES 131072   /* staged weights + biases + scaling vectors of one network */
typedef struct hilo_ann hilo_ann;
/* The network has n_hidden + 1 dense maps: hidden layer l (widths[l] neurons, activation acts[l]) and the linear output layer.
   Weights and biases arrive zero padded, map after map: W_l row-major [n_out_pad][n_in_pad] (the `nn.Linear` orientation),
   b_l [n_out_pad], with n_out_pad = widths[l] rounded up to 16 (16 for the output layer), n_in_pad = nf rounded up to 4 for the
   first map and the n_out_pad of the map before otherwise.  x_mean / x_scale [nf], y_mean / y_scale [nl]: host vectors, a NULL
   pair = no scaling.  HILO_ENOTSUP beyond the limits above. */
int hilo_ann_create(int device, int nf, int nl, int n_hidden, const int32_t* widths, const int32_t* acts,
                    const double* W_packed, const double* b_packed, const double* x_mean, const double* x_scale,
                    const double* y_mean, const double* y_scale, hilo_ann** out);
void hilo_ann_destroy(hilo_ann* h);
/* Y [nl][m] (row pitch ldy) = network(X [nf][m] (row pitch ldx)): device pointers, queries along the unit stride.  A query's
   result depends on its own column only and not on m or on its position in the batch. */
int hilo_ann_predict(hilo_ann* h, int64_t m, const double* X, int64_t ldx, double* Y, int64_t ldy, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* HILO_HIP_H */
