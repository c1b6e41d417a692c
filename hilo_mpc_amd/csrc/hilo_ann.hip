// Batched inference of a feed-forward network on the f64 matrix cores + C ABI.
//
// Reference semantics (hilo_mpc/modules/machine_learning/nn/nn.py:536-544 `predict`, util/machine_learning.py:521-578
// `net_to_casadi_graph`): h_0 = (x - mean_x) / scale_x,  h_{l+1} = act_l(W_l h_l + b_l),  y = (W_L h_L + b_L) * scale_y + mean_y.
//
// The kernel evaluates the TRANSPOSED network  H_{l+1}^T = act(W_l H_l^T + b_l)  for a tile of 16 queries per wave with
// v_mfma_f64_16x16x4_f64:
//   A operand (weights)      A[n = 16 nt + (lane & 15)][k = 4 ks + (lane >> 4)]
//   B operand (activations)  B[k = 4 ks + (lane >> 4)][q = lane & 15]
//   C / D                    col = lane & 15 (query), row = (lane >> 4) + 4 reg
// so accumulator register r of output tile nt holds, in lane (q, g), neuron 16 nt + 4 r + g of query q - which is exactly the B
// operand of k-step 4 nt + r of the next layer.  The layers therefore chain in registers: bias in the accumulator, activation on
// the four accumulator registers, and on to the next product; no LDS round trip and no cross-lane move between layers.  A
// column of C depends on the same column of B only, so a query never sees its neighbours (a NaN query stays in its column).
//
// Weights are staged once per workgroup in LDS in operand order (block (nt, ks) = 64 doubles in lane order: a wave-wide operand
// read is 512 contiguous bytes, conflict free), biases and scaling vectors behind them.  Zero padding (widths to 16, the first
// n_in to 4) makes every loop wave-uniform; a padded neuron's activation is some finite number its zero outgoing weights drop.
#include <math.h>
#include <stdlib.h>
#include <string.h>

#include "hilo_common.h"

namespace hilo {

constexpr int ANN_MAX_MAPS = HILO_ANN_MAX_HIDDEN + 1;
constexpr int ANN_TPB = 256, ANN_WAVES = ANN_TPB / 64;

constexpr int ANN_HDR = 5 * ANN_MAX_MAPS + 3;   // the layer table heads the staged block (as doubles): row l = nt, nk, act, woff, boff

// host-side description of a packed network
struct AnnLayout {
  int nt[ANN_MAX_MAPS];               // output tiles of 16 neurons
  int nk[ANN_MAX_MAPS];               // k-steps of 4 inputs
  int act[ANN_MAX_MAPS];
  int woff[ANN_MAX_MAPS];             // operand-order weights: block (nt, ks) at woff + (nt * nk + ks) * 64
  int boff[ANN_MAX_MAPS];             // biases [16 nt]
};
// kernel argument: scalars only - the per-layer table is read from LDS (indexed by the layer loop, it would otherwise sit in
// some fifty scalar registers for the whole kernel)
struct AnnDev {
  int n_maps, nf, nl, total;          // dense maps (hidden layers + output layer); doubles staged in LDS
  int nk0, xoff, yoff;                // x_mean [4 nk0] | x_scale [4 nk0];  y_mean [16] | y_scale [16]
  const double* pack;
};

typedef double ann_v4d __attribute__((ext_vector_type(4)));

template <int ACT>
__device__ __forceinline__ double ann_act(double v) {
  if (ACT == HILO_ANN_ACT_SIGMOID) return 1.0 / (1.0 + exp(-v));
  if (ACT == HILO_ANN_ACT_TANH) return 2.0 / (1.0 + exp(-2.0 * v)) - 1.0;
  if (ACT == HILO_ANN_ACT_RELU) return fmax(v, 0.0);
  if (ACT == HILO_ANN_ACT_SOFTPLUS) return fmax(v, 0.0) + log1p(exp(-fabs(v)));
  return v;
}

// acc = b + W h for a layer of NTL output tiles: bias in the accumulators, then k outer, tiles inner - NTL independent
// accumulator chains share one B operand.  The k-steps go in groups of four (= one tile of the layer before; the first map's
// inputs are padded likewise), each group fenced so that its operand reads stay next to its products.
template <int WT, int NTL>
__device__ __forceinline__ void ann_mma(const double* Wl, const double* bl, int nkl, const double (&h)[4 * WT], ann_v4d (&acc)[WT]) {
#pragma unroll
  for (int nt = 0; nt < NTL; ++nt) {
#pragma unroll
    for (int r = 0; r < 4; ++r) acc[nt][r] = bl[16 * nt + 4 * r];
  }
#pragma unroll
  for (int pt = 0; pt < WT; ++pt) {
    if (4 * pt < nkl) {
#pragma unroll
      for (int j = 0; j < 4; ++j) {
        const int ks = 4 * pt + j;
#pragma unroll
        for (int nt = 0; nt < NTL; ++nt)
          acc[nt] = __builtin_amdgcn_mfma_f64_16x16x4f64(Wl[(nt * nkl + ks) * 64], h[ks], acc[nt], 0, 0, 0);
      }
    }
    __builtin_amdgcn_sched_barrier(0);
  }
}

// WT: tiles of 16 the widest layer (or the padded input) needs; the activations of a query tile are 4 WT registers per lane
template <int WT>
__global__ __launch_bounds__(ANN_TPB) void ann_predict_kernel(const AnnDev d, int64_t m, const double* __restrict__ X, int64_t ldx,
                                                              double* __restrict__ Y, int64_t ldy) {
  extern __shared__ double sm[];
  for (int e = threadIdx.x; e < d.total; e += ANN_TPB) sm[e] = d.pack[e];
  __syncthreads();
  const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6, q = lane & 15, g = lane >> 4;
  const int64_t ntile = (m + 15) >> 4;
  const double* xm = sm + d.xoff;
  const double* xs = xm + 4 * d.nk0;
  const double* ym = sm + d.yoff;
  const double* ys = ym + 16;
  // persistent grid: the waves of all workgroups walk the query tiles
  for (int64_t tile = (int64_t)blockIdx.x * ANN_WAVES + wave; tile < ntile; tile += (int64_t)gridDim.x * ANN_WAVES) {
    const int64_t qi = tile * 16 + q;
    const bool valid = qi < m;          // a partial tile is masked on load and store only
    double h[4 * WT];
    // the feature count is made opaque once per tile: the sixteen comparisons below then stay here, next to their use, instead of
    // being carried through the whole kernel as loop invariants (two scalar registers each)
    int nf = d.nf;
    asm volatile("" : "+s"(nf));
    constexpr int KIN = 4 * WT < HILO_ANN_MAX_FEATURES / 4 ? 4 * WT : HILO_ANN_MAX_FEATURES / 4;
#pragma unroll
    for (int ks = 0; ks < 4 * WT; ++ks) h[ks] = 0.0;
#pragma unroll
    for (int ks = 0; ks < KIN; ++ks) {
      if (4 * ks < nf) {                // wave-uniform
        const int k = 4 * ks + g;
        const double x = (valid && k < nf) ? X[(int64_t)k * ldx + qi] : 0.0;   // 16 lanes of a row group: 128 contiguous bytes
        h[ks] = (x - xm[k]) / xs[k];    // padded inputs: (0 - 0) / 1
      }
    }
    for (int l = 0; l < d.n_maps; ++l) {
      const double* row = sm + 5 * l;   // the same address in every lane: the values are made scalar again below
      const int ntl = __builtin_amdgcn_readfirstlane((int)row[0]), nkl = __builtin_amdgcn_readfirstlane((int)row[1]);
      const int act = __builtin_amdgcn_readfirstlane((int)row[2]);
      const double* Wl = sm + __builtin_amdgcn_readfirstlane((int)row[3]) + lane;
      const double* bl = sm + __builtin_amdgcn_readfirstlane((int)row[4]) + g;
      ann_v4d acc[WT];
      switch (ntl) {                    // wave-uniform: the products of a layer are straight-line code for its number of tiles
        case 1: ann_mma<WT, 1>(Wl, bl, nkl, h, acc); break;
        case 2: ann_mma<WT, (WT >= 2 ? 2 : 1)>(Wl, bl, nkl, h, acc); break;
        case 3: ann_mma<WT, (WT >= 4 ? 3 : 1)>(Wl, bl, nkl, h, acc); break;
        default: ann_mma<WT, (WT >= 4 ? 4 : 1)>(Wl, bl, nkl, h, acc); break;
      }
      // (tiles beyond this layer's keep stale values: the next map's k-steps end at 4 ntl and never read them)
#define ANN_APPLY(A)                                                                  \
  _Pragma("unroll") for (int nt = 0; nt < WT; ++nt) {                                 \
    if (nt < ntl) {                                                                   \
      _Pragma("unroll") for (int r = 0; r < 4; ++r) h[4 * nt + r] = ann_act<A>(acc[nt][r]); \
    }                                                                                 \
    __builtin_amdgcn_sched_barrier(0);                                                \
  }
      switch (act) {                    // wave-uniform
        case HILO_ANN_ACT_SIGMOID: ANN_APPLY(HILO_ANN_ACT_SIGMOID) break;
        case HILO_ANN_ACT_TANH: ANN_APPLY(HILO_ANN_ACT_TANH) break;
        case HILO_ANN_ACT_RELU: ANN_APPLY(HILO_ANN_ACT_RELU) break;
        case HILO_ANN_ACT_SOFTPLUS: ANN_APPLY(HILO_ANN_ACT_SOFTPLUS) break;
        default: ANN_APPLY(HILO_ANN_ACT_LINEAR) break;
      }
#undef ANN_APPLY
    }
    // the output layer is one tile: register r holds label 4 r + g of query q
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      const int n = 4 * r + g;
      if (valid && n < d.nl) Y[(int64_t)n * ldy + qi] = h[r] * ys[n] + ym[n];
    }
  }
}

}  // namespace hilo

using namespace hilo;

struct hilo_ann {
  int device, wt, n_cu;
  AnnDev d;
  double* pack;
};

extern "C" void hilo_ann_destroy(hilo_ann* a) {
  if (!a) return;
  if (a->pack) (void)hipFree(a->pack);
  delete a;
}

extern "C" int hilo_ann_create(int device, int nf, int nl, int n_hidden, const int32_t* widths, const int32_t* acts,
                               const double* W_packed, const double* b_packed, const double* x_mean, const double* x_scale,
                               const double* y_mean, const double* y_scale, hilo_ann** out) {
  HILO_REQUIRE(out && W_packed && b_packed, "hilo_ann_create: NULL argument");
  HILO_REQUIRE(nf >= 1 && nl >= 1 && n_hidden >= 0, "hilo_ann_create: need nf >= 1, nl >= 1 and n_hidden >= 0 (got %d, %d, %d)", nf, nl,
               n_hidden);
  HILO_REQUIRE(n_hidden == 0 || (widths && acts), "hilo_ann_create: hidden layers without widths / activations");
  HILO_REQUIRE((x_mean == nullptr) == (x_scale == nullptr) && (y_mean == nullptr) == (y_scale == nullptr),
               "hilo_ann_create: a scaling needs both its mean and its scale");
  if (nf > HILO_ANN_MAX_FEATURES) return fail(HILO_ENOTSUP, "ANN: %d features, at most %d are built", nf, HILO_ANN_MAX_FEATURES);
  if (nl > HILO_ANN_MAX_LABELS) return fail(HILO_ENOTSUP, "ANN: %d labels, at most %d are built", nl, HILO_ANN_MAX_LABELS);
  if (n_hidden > HILO_ANN_MAX_HIDDEN)
    return fail(HILO_ENOTSUP, "ANN: %d hidden layers, at most %d are built", n_hidden, HILO_ANN_MAX_HIDDEN);
  for (int l = 0; l < n_hidden; ++l) {
    HILO_REQUIRE(widths[l] >= 1, "ANN: hidden layer %d has %d neurons", l, widths[l]);
    if (widths[l] > HILO_ANN_MAX_WIDTH)
      return fail(HILO_ENOTSUP, "ANN: hidden layer %d has %d neurons, at most %d are built", l, widths[l], HILO_ANN_MAX_WIDTH);
    HILO_REQUIRE(acts[l] >= HILO_ANN_ACT_LINEAR && acts[l] <= HILO_ANN_ACT_SOFTPLUS, "ANN: unknown activation code %d of hidden layer %d",
                 acts[l], l);
  }
  for (int k = 0; x_scale && k < nf; ++k) HILO_REQUIRE(x_scale[k] != 0.0, "ANN: zero input scale of feature %d", k);
  AnnDev dv;
  AnnLayout d;
  memset(&dv, 0, sizeof(dv));
  memset(&d, 0, sizeof(d));
  dv.n_maps = n_hidden + 1; dv.nf = nf; dv.nl = nl;
  int wt = (nf + 15) / 16, off = ANN_HDR;
  for (int l = 0; l < dv.n_maps; ++l) {
    d.nt[l] = l < n_hidden ? (widths[l] + 15) / 16 : 1;
    d.nk[l] = l == 0 ? 4 * ((nf + 15) / 16) : 4 * d.nt[l - 1];   // the first map's k-steps padded to a group of four
    d.act[l] = l < n_hidden ? acts[l] : HILO_ANN_ACT_LINEAR;
    d.woff[l] = off;
    off += d.nt[l] * d.nk[l] * 64;
    if (d.nt[l] > wt) wt = d.nt[l];
  }
  for (int l = 0; l < dv.n_maps; ++l) { d.boff[l] = off; off += 16 * d.nt[l]; }
  dv.nk0 = d.nk[0];
  dv.xoff = off; off += 8 * d.nk[0];
  dv.yoff = off; off += 32;
  dv.total = off;
  if ((size_t)off * sizeof(double) > HILO_ANN_MAX_LDS_BYTES)
    return fail(HILO_ENOTSUP, "ANN: the network needs %zu bytes of staged weights, at most %d fit the LDS the kernel requests",
                (size_t)off * sizeof(double), HILO_ANN_MAX_LDS_BYTES);
  wt = wt <= 1 ? 1 : wt <= 2 ? 2 : 4;
  // host pack: padded row-major maps -> operand order
  double* pk = new double[off];
  memset(pk, 0, sizeof(double) * off);
  const double* Wsrc = W_packed;
  const double* bsrc = b_packed;
  for (int l = 0; l < dv.n_maps; ++l) {
    const int rowv[5] = {d.nt[l], d.nk[l], d.act[l], d.woff[l], d.boff[l]};
    for (int c = 0; c < 5; ++c) pk[5 * l + c] = rowv[c];
    const int nout = 16 * d.nt[l], nin = l == 0 ? 4 * ((nf + 3) / 4) : 4 * d.nk[l];   // columns of the caller's padded map
    for (int nt = 0; nt < d.nt[l]; ++nt)
      for (int ks = 0; ks < d.nk[l]; ++ks)
        for (int lane = 0; lane < 64; ++lane) {
          const int k = 4 * ks + (lane >> 4);
          pk[d.woff[l] + (nt * d.nk[l] + ks) * 64 + lane] = k < nin ? Wsrc[(size_t)(16 * nt + (lane & 15)) * nin + k] : 0.0;
        }
    memcpy(pk + d.boff[l], bsrc, sizeof(double) * nout);
    Wsrc += (size_t)nout * nin;
    bsrc += nout;
  }
  for (int k = 0; k < 4 * d.nk[0]; ++k) {
    pk[dv.xoff + k] = (x_mean && k < nf) ? x_mean[k] : 0.0;
    pk[dv.xoff + 4 * d.nk[0] + k] = (x_scale && k < nf) ? x_scale[k] : 1.0;
  }
  for (int n = 0; n < 16; ++n) {
    pk[dv.yoff + n] = (y_mean && n < nl) ? y_mean[n] : 0.0;
    pk[dv.yoff + 16 + n] = (y_scale && n < nl) ? y_scale[n] : 1.0;
  }
  for (int e = 0; e < off; ++e)
    if (!isfinite(pk[e])) {
      delete[] pk;
      return fail(HILO_EINVAL, "ANN: non-finite weight, bias or scaling value");
    }
  hipError_t e = hipSetDevice(device);
  hipDeviceProp_t prop;
  if (e == hipSuccess) e = hipGetDeviceProperties(&prop, device);
  hilo_ann* a = new hilo_ann();
  a->device = device; a->wt = wt; a->pack = nullptr;
  if (e == hipSuccess) e = hipMalloc((void**)&a->pack, sizeof(double) * off);
  if (e == hipSuccess) e = hipMemcpy(a->pack, pk, sizeof(double) * off, hipMemcpyHostToDevice);
  delete[] pk;
  if (e != hipSuccess) {
    hilo_ann_destroy(a);
    return fail(HILO_EHIP, "hilo_ann_create: %s", hipGetErrorString(e));
  }
  a->n_cu = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 1;
  dv.pack = a->pack;
  a->d = dv;
  *out = a;
  return HILO_OK;
}

template <int WT>
static int ann_launch(hilo_ann* a, int64_t m, const double* X, int64_t ldx, double* Y, int64_t ldy, hipStream_t s) {
  const size_t lds = sizeof(double) * (size_t)a->d.total;
  if (lds > 64 * 1024)
    HILO_HIP_CHECK(hipFuncSetAttribute((const void*)ann_predict_kernel<WT>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  // workgroups resident per CU: bounded by the LDS (160 KiB per CU) and by eight workgroups of four waves
  int per_cu = (int)((160 * 1024) / (lds ? lds : 1));
  per_cu = per_cu < 1 ? 1 : per_cu > 8 ? 8 : per_cu;
  const int64_t want = ((m + 15) / 16 + ANN_WAVES - 1) / ANN_WAVES, cap = (int64_t)a->n_cu * per_cu;
  const int grid = (int)(want < cap ? want : cap);
  hipLaunchKernelGGL(ann_predict_kernel<WT>, dim3(grid), dim3(ANN_TPB), lds, s, a->d, m, X, ldx, Y, ldy);
  HILO_HIP_CHECK(hipGetLastError());
  return HILO_OK;
}

extern "C" int hilo_ann_predict(hilo_ann* a, int64_t m, const double* X, int64_t ldx, double* Y, int64_t ldy, void* stream) {
  HILO_REQUIRE(a, "hilo_ann_predict: NULL handle");
  HILO_REQUIRE(m >= 0, "hilo_ann_predict: negative number of queries");
  if (m == 0) return HILO_OK;
  HILO_REQUIRE(X && Y, "hilo_ann_predict: NULL argument");
  HILO_REQUIRE(ldx >= m && ldy >= m, "hilo_ann_predict: leading dimensions (%lld, %lld) smaller than the %lld queries", (long long)ldx,
               (long long)ldy, (long long)m);
  HILO_HIP_CHECK(hipSetDevice(a->device));
  hipStream_t s = (hipStream_t)stream;
  switch (a->wt) {
    case 1: return ann_launch<1>(a, m, X, ldx, Y, ldy, s);
    case 2: return ann_launch<2>(a, m, X, ldx, Y, ldy, s);
    default: return ann_launch<4>(a, m, X, ldx, Y, ldy, s);
  }
}
