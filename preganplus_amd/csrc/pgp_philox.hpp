// pgp_philox.hpp — the dropout masks of the fused batch-1 tuning step
// (models.py:300,311,354: p = 0.1 at the positional encoding, the attention
// probabilities, dropout1, the feed-forward dropout and dropout2).
//
// Counter-based, so a mask is a pure function of (seed, optimizer step, site,
// element): Philox4x32-10 (Salmon et al., SC'11) in plain C++.  For element e
// of site s in step n: key = (seed_lo, seed_hi), counter = (e >> 2, s, n_lo,
// n_hi), the word used is output word e & 3; the element is DROPPED iff
// word < thr, thr = (uint32)(p * 2^32) computed in double on the host.
//
// Sites and element order (token t = w*H + h, D = H):
//   0          PE output                         t*D + c               3H^2
//   1 + 4l     layer l attention probabilities   (t*2 + head)*3 + key  18H
//   2 + 4l     out_proj output (dropout1)        t*D + c               3H^2
//   3 + 4l     relu(linear1)   (dropout)         t*64 + k              192H
//   4 + 4l     linear2 output  (dropout2)        t*D + c               3H^2
// The keep bytes of one step (1 = kept) lie in that site order, one byte per
// element: DropGeo<H>::TOTAL bytes.
#pragma once
#include <hip/hip_runtime.h>

#include "pgp_device.hpp"

namespace pgp {

struct Philox4 {
  unsigned int w[4];
};

PGP_DEV Philox4 philox4x32_10(unsigned int c0, unsigned int c1, unsigned int c2, unsigned int c3, unsigned int k0,
                              unsigned int k1) {
#pragma unroll
  for (int r = 0; r < 10; ++r) {
    const unsigned int h0 = __umulhi(0xD2511F53u, c0), l0 = 0xD2511F53u * c0;
    const unsigned int h1 = __umulhi(0xCD9E8D57u, c2), l1 = 0xCD9E8D57u * c2;
    c0 = h1 ^ c1 ^ k0;
    c1 = l1;
    c2 = h0 ^ c3 ^ k1;
    c3 = l0;
    k0 += 0x9E3779B9u;
    k1 += 0xBB67AE85u;
  }
  return Philox4{{c0, c1, c2, c3}};
}

template <int H>
struct DropGeo {
  static constexpr int N_PE = 3 * H * H, N_AT = 18 * H, N_D = 3 * H * H, N_FF = 192 * H;
  static constexpr int LAYER = N_AT + N_D + N_FF + N_D;
  static constexpr int TOTAL = N_PE + 2 * LAYER;
  static constexpr int NSITES = 9;
  // byte offsets within one step's keep bytes
  static constexpr int O_PE = 0;
  static constexpr int o_at(int l) { return N_PE + l * LAYER; }
  static constexpr int o_d1(int l) { return o_at(l) + N_AT; }
  static constexpr int o_ff(int l) { return o_d1(l) + N_D; }
  static constexpr int o_d2(int l) { return o_ff(l) + N_FF; }
  static_assert(N_PE % 4 == 0 && N_AT % 4 == 0 && N_FF % 4 == 0, "sites are whole Philox blocks");
};

// Every keep byte of one step, four per Philox block (one 32-bit store), the
// blocks dealt to `nthreads` threads; `keep` is 4-byte aligned (LDS or global).
template <int H>
PGP_DEV void drop_fill_masks(unsigned char* keep, unsigned int thr, unsigned long long seed, unsigned long long step,
                             int tid, int nthreads) {
  using DG = DropGeo<H>;
  const unsigned int k0 = (unsigned int)seed, k1 = (unsigned int)(seed >> 32);
  const unsigned int n0 = (unsigned int)step, n1 = (unsigned int)(step >> 32);
  unsigned int* out = reinterpret_cast<unsigned int*>(keep);
  for (int b = tid; b < DG::TOTAL / 4; b += nthreads) {
    int site = 0, q = b;  // q: block index within the site
    if (q >= DG::N_PE / 4) {
      q -= DG::N_PE / 4;
      const int l = q >= DG::LAYER / 4 ? 1 : 0;
      q -= l * (DG::LAYER / 4);
      site = 1 + 4 * l;
      if (q >= DG::N_AT / 4) {
        q -= DG::N_AT / 4;
        ++site;
        if (q >= DG::N_D / 4) {
          q -= DG::N_D / 4;
          ++site;
          if (q >= DG::N_FF / 4) {
            q -= DG::N_FF / 4;
            ++site;
          }
        }
      }
    }
    const Philox4 r = philox4x32_10((unsigned int)q, (unsigned int)site, n0, n1, k0, k1);
    out[b] = (r.w[0] >= thr ? 1u : 0u) | (r.w[1] >= thr ? 0x100u : 0u) | (r.w[2] >= thr ? 0x10000u : 0u) |
             (r.w[3] >= thr ? 0x1000000u : 0u);
  }
}

}  // namespace pgp
