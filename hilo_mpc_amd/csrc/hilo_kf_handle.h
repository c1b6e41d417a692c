// The filter handle behind the C ABI and the list of zoo functors the filter kernels are instantiated for (shared by the filters'
// unit, hilo_kf.hip, and the roll-out's, hilo_sim.hip).
#pragma once
#include "hilo_jit.h"
#include "hilo_kf_params.h"

struct hilo_kf {
  hilo_kf_desc desc;
  int device;
  int nx, nu, np, ny;
  bool discrete;
  hilo::KfParams kp;
  hilo::JitKfKernels jit;   // model given as source (HILO_MODEL_USER): kernels compiled at create
  double* user_gp_pack[4] = {nullptr, nullptr, nullptr, nullptr};   // packed learned terms of that model (gp_pack_se)
};

// A time-variant model (hilo_models.h::model_time_variant) is handed the time by hilo_model_rollout alone.  Its other kernels are
// compiled against the functor's autonomous `ode` / `meas`, which evaluate at t = 0, and the entries that would launch them refuse.
#define HILO_REFUSE_TIME_VARIANT(kf, who)                                                                                        \
  do {                                                                                                                          \
    if ((kf)->jit.time_variant)                                                                                                 \
      return hilo::fail(HILO_ENOTSUP, "%s: the model depends on time explicitly; only hilo_model_rollout hands a model the time "  \
                                      "(Model.step, rollout, simulate)", who);                                                  \
  } while (0)

#define HILO_KF_MODELS(X)                 \
  X(HILO_MODEL_TOY1D, Toy1D)              \
  X(HILO_MODEL_BIOREACTOR3, Bioreactor3)  \
  X(HILO_MODEL_CHEMOSTAT4, Chemostat4)    \
  X(HILO_MODEL_PENDULUM4, Pendulum4)      \
  X(HILO_MODEL_LINEAR2, Linear2)
