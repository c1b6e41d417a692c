// The counter-based generator that the particle filter (hilo_kf_kernel.h::pf_run_body) and the data generator (hilo_datagen.h) draw
// from: Philox4x32-10 (Salmon et al., SC'11), the map from two of its words to a uniform, and Box-Muller on one block of four
// words.  The statements are the particle filter's own, moved here unchanged - tests/test_pf_device_gpu.py pins their bits.
#pragma once
#include "hilo_ad.h"

namespace hilo {

struct Philox4 { unsigned r0, r1, r2, r3; };
HD unsigned pf_mulhi(unsigned a, unsigned b) { return (unsigned)(((unsigned long long)a * b) >> 32); }
HD Philox4 philox4x32_10(unsigned c0, unsigned c1, unsigned c2, unsigned c3, unsigned k0, unsigned k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned h0 = pf_mulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0, h1 = pf_mulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0; c1 = l1; c2 = h0 ^ c3 ^ k1; c3 = l0;
    k0 += 0x9E3779B9u; k1 += 0xBB67AE85u;
  }
  return Philox4{c0, c1, c2, c3};
}
// 53 bits of two words, centred in their cell: never 0, so the logarithm is safe (the topmost cell rounds to 1)
HD double pf_uniform(unsigned a, unsigned b) {
  return ((double)(((unsigned long long)(a >> 5) << 26) | (unsigned long long)(b >> 6)) + 0.5) * 0x1p-53;
}
// Box-Muller on one block: two normals from its four words
HD void pf_box_muller(const Philox4& r, double& z0, double& z1) {
  const double rad = ::sqrt(-2.0 * ::log(pf_uniform(r.r0, r.r1)));
  double s, c;
  sin_cos(6.283185307179586 * pf_uniform(r.r2, r.r3), s, c);
  z0 = rad * c;
  z1 = rad * s;
}
}  // namespace hilo
