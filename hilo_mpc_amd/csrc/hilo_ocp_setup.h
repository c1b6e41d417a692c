// Host-side setup shared by the creates of the NMPC handle (hilo_nmpc.hip: precompiled policies, hilo_nmpc_user.hip: general
// run-time compiled policy) and of the MHE handle (hilo_mhe.hip): the engine's constants from a description, the NMPC start guess,
// the device copies and the per-batch device buffers.  The transcription rules restated here are the reference's
// (hilo_mpc/modules/controller/mpc.py, hilo_mpc/modules/estimator/mhe.py); the callers write them into their policy's layout.
#pragma once
#include <string.h>

#include <memory>
#include <vector>

#include "hilo_ocp.h"

namespace hilo {

// owner of a handle under construction: destroys it on every return except the one that hands it over (release())
template <class H>
using HandleGuard = std::unique_ptr<H, void (*)(H*)>;

template <class H>
HandleGuard<H> new_handle(void (*destroy)(H*)) {
  H* h = new H();
  memset(h, 0, sizeof(*h));
  return HandleGuard<H>(h, destroy);
}

// IPOPT's bound_relax_factor; a description leaves it at IPOPT's default with a negative value
inline double ocp_bound_relax(double factor) { return factor >= 0.0 ? factor : 1e-8; }

// IPOPT relaxes every finite bound outwards by relax * max(1, |bound|)
inline void relax_box(double& lb, double& ub, double relax) {
  if (lb > -INFINITY) lb -= relax * fmax(1.0, fabs(lb));
  if (ub < INFINITY) ub += relax * fmax(1.0, fabs(ub));
}

// OcpConst of a new problem: the engine's defaults, horizons and integrator, the collocation basis of degree D (coll_B NULL: zero
// quadrature weights), the solver options the description sets (IPOPT's options of those names) and the bound relaxation
template <class Desc>
void ocp_init_const(OcpConst& c, const Desc* d, int Nc, int D, const double* coll_B) {
  memset(&c, 0, sizeof(c));
  ocp_default_options(c);
  c.N = d->N; c.Nc = Nc; c.order = d->erk_order >= 1 ? d->erk_order : 4; c.nsub = d->n_sub >= 1 ? d->n_sub : 1;
  c.dt = d->dt;
  if (D) {
    c.coll.d = D;
    for (int i = 0; i < D * D; ++i) c.coll.A[i] = d->coll_A[i];
    for (int i = 0; i <= D; ++i) { c.coll.Dc[i] = d->coll_D[i]; c.coll.Bq[i] = coll_B ? coll_B[i] : 0.0; }
  }
  if (d->max_iter > 0) c.max_iter = d->max_iter;
  if (d->acceptable_iter > 0) c.acceptable_iter = d->acceptable_iter;
  if (d->tol > 0) c.tol = d->tol;
  if (d->acceptable_tol > 0) c.acceptable_tol = d->acceptable_tol;
  if (d->mu_init > 0) c.mu_init = d->mu_init;
  c.bound_relax = ocp_bound_relax(d->bound_relax_factor);
}

// inequality rows of one kind (stage or terminal) in the engine's order: expression index, sign, slack index (-1: none), bounds and
// the row's place in the reference's g
struct OcpRows {
  int n = 0, nref = 0, nslack = 0;   // rows; rows in the reference's g (dropped ones included); slacks they use
  int expr[OCP_MAXNC], sign[OCP_MAXNC], e[OCP_MAXNC], ref[OCP_MAXNC];
  double lb[OCP_MAXNC], ub[OCP_MAXNC];
  void add(int x, int s, int slack, double l, double u, int r) {
    expr[n] = x; sign[n] = s; e[n] = slack; lb[n] = l; ub[n] = u; ref[n++] = r;
  }
};

// rows of `count` constraint expressions lb_j <= c_j <= ub_j (NULL bounds: unbounded) behind `used` rows of other kinds.  Hard: one
// row per expression (with drop_free, per expression with a finite bound).  Soft: the pair c - e <= ub | -c - e <= -lb on the
// slack e0 + j; a row without a finite bound constrains nothing and is dropped.  The reference's g keeps `count` rows, 2 `count`
// when soft (mpc.py:1687-1690, :1696-1698, :1711-1712).
inline int ocp_con_rows(OcpRows& r, int count, const double* lbs, const double* ubs, bool soft, int e0, int used, bool drop_free,
                        const char* what) {
  if (count <= 0) return HILO_OK;
  r.nref = soft ? 2 * count : count;
  r.nslack = soft ? count : 0;
  for (int j = 0; j < count; ++j) {
    const double lb = lbs ? lbs[j] : -INFINITY, ub = ubs ? ubs[j] : INFINITY;
    HILO_REQUIRE(lb <= ub, "hilo_nmpc_create: %s %d has lb > ub", what, j);
    if (soft) {
      if (ub < INFINITY) {
        HILO_REQUIRE(used + r.n < OCP_MAXNC, "too many constraint rows");
        r.add(j, 1, e0 + j, -INFINITY, ub, j);
      }
      if (lb > -INFINITY) {
        HILO_REQUIRE(used + r.n < OCP_MAXNC, "too many constraint rows");
        r.add(j, -1, e0 + j, -INFINITY, -lb, count + j);
      }
    } else if (!drop_free || lb > -INFINITY || ub < INFINITY) {
      HILO_REQUIRE(used + r.n < OCP_MAXNC, "too many constraint rows");
      r.add(j, 1, -1, lb, ub, j);
    }
  }
  return HILO_OK;
}

// the stage constraint's rows (their slacks come first) and the terminal constraint's (slacks from e0, behind `used` stage rows)
inline int nmpc_stage_rows(const hilo_nmpc_desc* d, OcpRows& s) {
  return ocp_con_rows(s, d->n_con, d->con_lb, d->con_ub, d->con_soft, 0, 0, true, "constraint");
}
inline int nmpc_term_rows(const hilo_nmpc_desc* d, int e0, int used, OcpRows& t) {
  return ocp_con_rows(t, d->n_tcon, d->tcon_lb, d->tcon_ub, d->tcon_soft, e0, used, false, "terminal constraint");
}

// where a policy keeps the description's quadratic cost (QuadraticCost, hilo_mpc/util/modeling.py:243-283) in OcpConst::cost: the
// block offsets, the policy's index of the first model input (model z = [x | u] -> policy z = [x, theta, ... | u, u_theta]) and
// the row lengths of Wz and WN
struct QuadCostLayout {
  int o_wz, o_zref, o_wn, o_xrefn, o_wdu, o_hasdu, iu, zw, xw;
};

inline void pack_quad_cost(double* cost, const QuadCostLayout& l, const hilo_nmpc_desc* d, int nx, int nu, int nth) {
  auto z = [&](int i) { return i < nx ? i : l.iu + (i - nx); };
  const int mz = nx + nu;
  for (int i = 0; i < mz; ++i) {
    for (int j = 0; j < mz; ++j) cost[l.o_wz + z(i) * l.zw + z(j)] = d->Wz ? d->Wz[i * mz + j] : 0.0;
    cost[l.o_zref + z(i)] = d->zref ? d->zref[i] : 0.0;
  }
  for (int i = 0; i < nx; ++i) {
    for (int j = 0; j < nx; ++j) cost[l.o_wn + i * l.xw + j] = d->WN ? d->WN[i * nx + j] : 0.0;
    cost[l.o_xrefn + i] = d->xrefN ? d->xrefN[i] : 0.0;
  }
  for (int i = 0; i < nu * nu; ++i) cost[l.o_wdu + i] = d->Wdu ? d->Wdu[i] : 0.0;
  cost[l.o_hasdu] = d->Wdu ? 1.0 : 0.0;
  if (nth && d->has_u_pf_ref) {   // mpc.py:1202-1204
    const int iu = l.iu + nu;
    cost[l.o_wz + iu * l.zw + iu] = d->u_pf_weight;
    cost[l.o_zref + iu] = d->u_pf_ref;
  }
}

// e^T W e of n slacks as the block cost[o + a * w + b] (W NULL: 1e4 I, modeling.py:875)
inline void pack_slack_weight(double* cost, int o, int w, const double* W, int n) {
  for (int a = 0; a < n; ++a)
    for (int b = 0; b < n; ++b) cost[o + a * w + b] = W ? W[a * n + b] : (a == b ? 1e4 : 0.0);
}

// scaling and boxes of the engine's z = [x | theta | slacks | free states | u | u_theta].  x and u are scaled (mpc.py:253-259), the
// rest has unit scaling (mpc.py:1200-1201); the slacks of the stage constraint, the terminal constraint (from ne_stage) and the
// custom rows (from ne_cus0) lie in [0, max violation] (mpc.py:1533-1534, :1544-1545); the free states (accumulators, held inputs)
// have no box.  Bounds arrive in original units and are relaxed like IPOPT's.
inline int nmpc_scale_boxes(OcpConst& c, const hilo_nmpc_desc* d, int nx, int nu, int nth, int ne_stage, int ne_cus0, int ne,
                            int nfree) {
  const int nxe = nx + nth + ne + nfree, nz = nxe + nu + nth;
  for (int i = 0; i < nz; ++i) c.sz[i] = 1.0;
  for (int i = 0; i < nx; ++i) c.sz[i] = d->x_scaling ? d->x_scaling[i] : 1.0;
  for (int i = 0; i < nu; ++i) c.sz[nxe + i] = d->u_scaling ? d->u_scaling[i] : 1.0;
  for (int i = 0; i < nz; ++i) {
    double lb = -INFINITY, ub = INFINITY;
    if (i < nx) { if (d->x_lb) lb = d->x_lb[i] / c.sz[i]; if (d->x_ub) ub = d->x_ub[i] / c.sz[i]; }
    else if (i < nx + nth) { lb = d->theta_lb; ub = d->theta_ub; }                                 // mpc.py:1198-1199
    else if (i < nx + nth + ne) {
      const int a = i - nx - nth;
      lb = 0.0;
      ub = a < ne_stage ? (d->con_max_violation ? d->con_max_violation[a] : INFINITY)
           : a < ne_cus0 ? (d->tcon_max_violation ? d->tcon_max_violation[a - ne_stage] : INFINITY)
                         : (d->acc_max_violation ? d->acc_max_violation[a - ne_cus0] : INFINITY);
    }
    else if (i < nxe) {}
    else if (i < nxe + nu) { const int j = i - nxe; if (d->u_lb) lb = d->u_lb[j] / c.sz[i]; if (d->u_ub) ub = d->u_ub[j] / c.sz[i]; }
    else { lb = d->u_pf_lb; ub = d->u_pf_ub; }                                                     // mpc.py:1196-1197
    relax_box(lb, ub, c.bound_relax);
    HILO_REQUIRE(lb < ub, "hilo_nmpc_create: empty box for variable %d", i);
    c.lbz[i] = lb; c.ubz[i] = ub;
  }
  return HILO_OK;
}

// the NMPC start guess v (mpc.py:1468-1482): x_guess and u_guess scaled by sx / su (mpc.py:255, 259) and tiled over the N + 1
// stages of [x | theta] and the Nc of [u | u_theta], theta at theta_guess and its virtual input at u_pf_lb + 1e-4
// (mpc.py:1194-1195); the states of the D collocation points of interval k start at the state guess from v[coll + k coll_w]
// (mpc.py:1321); zeros elsewhere, the slacks among them (mpc.py:1535)
inline std::vector<double> nmpc_guess(const hilo_nmpc_desc* d, int n_v, const double* sx, const double* su, int nx, int nu, int nth,
                                      int Nc, int D, int coll, int coll_w) {
  std::vector<double> g(n_v, 0.0);
  const int N = d->N, nxv = nx + nth, nuv = nu + nth;
  for (int k = 0; k <= N; ++k) {
    for (int i = 0; i < nx; ++i) g[k * nxv + i] = (d->x_guess ? d->x_guess[i] : 0.0) / sx[i];
    if (nth) g[k * nxv + nx] = d->theta_guess;
  }
  for (int k = 0; k < Nc; ++k) {
    for (int i = 0; i < nu; ++i) g[(N + 1) * nxv + k * nuv + i] = (d->u_guess ? d->u_guess[i] : 0.0) / su[i];
    if (nth) g[(N + 1) * nxv + k * nuv + nu] = d->u_pf_lb + 0.0001;
  }
  for (int k = 0; k < N && D; ++k)
    for (int i = 0; i < D * nxv; ++i) {
      const int a = i % nxv;
      g[coll + k * coll_w + i] = a < nx ? (d->x_guess ? d->x_guess[a] : 0.0) / sx[a] : d->theta_guess;
    }
  return g;
}

// a device copy of `bytes` host bytes in a new allocation *dst (owned by the caller's handle)
template <class T>
hipError_t ocp_upload(T** dst, const void* src, size_t bytes) {
  hipError_t e = hipMalloc((void**)dst, bytes);
  return e == hipSuccess ? hipMemcpy(*dst, src, bytes, hipMemcpyHostToDevice) : e;
}

// (re)allocates a per-batch device buffer; on failure HILO_ENOMEM with the caller's text, whose last conversion takes the HIP error
template <class T, class... A>
int batch_realloc(T** buf, size_t bytes, const char* fmt, A... args) {
  if (*buf) HILO_HIP_CHECK(hipFree(*buf));
  *buf = nullptr;
  const hipError_t e = hipMalloc((void**)buf, bytes);
  return e == hipSuccess ? HILO_OK : fail(HILO_ENOMEM, fmt, args..., hipGetErrorString(e));
}

}  // namespace hilo
