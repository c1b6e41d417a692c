// Launch parameters of the filter kernels (csrc/hilo_kf_kernel.h) and of the roll-out (csrc/hilo_integrate.h): what a filter handle
// knows about its model's sampling interval and discretisation.
#pragma once

namespace hilo {

struct KfParams {
  int kind, continuous, erk_order, n_sub;
  double dt, gamma, wm0, wc0, wi;  // UKF: W_m[0], W_c[0], W[1:] (kf.py:493-500)
  // hilo_kf_steps_split: the parameters in their own array (rows of np doubles, stride pp_stride or 0 = shared) - `up` then holds
  // the inputs alone (rows of nu doubles); nullptr: `up` holds the packed rows [u; p]
  const double* pp = nullptr;
  long long pp_stride = 0;
};

// most states of a model whose filters are compiled at run time: kf_body's static LDS (UKF: 64 tiles of NX (3 NX + 2) doubles)
// passes the 160 KB of a workgroup at NX = 10 (csrc/hilo_kf_kernel.h, refused in csrc/hilo_jit.hip::jit_kf_kernels)
constexpr int KF_MAX_NX = 9;

}  // namespace hilo
