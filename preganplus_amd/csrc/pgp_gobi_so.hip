// pgp_gobi_so.hip — second-order GOBI (SOGOBI): scheduler/SOGOBI.py:18-40 ->
// scheduler/BaGTI/src/opt.py:35-51 (so_opt) with Adahessian
// (scheduler/BaGTI/src/adahessian.py:49-168) over the energy_latency_16
// surrogate, for a batch of independent environments.
//
// pgp_gobi.hip's layout (pgp_gobi.hpp: one 512-thread workgroup, fixed lane
// roles, layers 2-3 and the input-gradient slices of W1 in registers, W1's
// allocation columns in LDS, 4 right-hand-side columns sharing every weight
// read and barrier), but the 4 columns are {value, tangent} x 2 environments:
// column 2e is environment e's forward / gradient, column 2e + 1 its tangent
// along the step's Hutchinson probe v (+-1 per input entry).  Both go through
// the same weights (forward-over-reverse):
//   tangent forward   da1 = W1 v;  dh = phi'(a) da;  da_{l+1} = W_{l+1} dh_l
//   backward          d4 = c o(1-o), dd4 = c o(1-o)(1-2o) da4, c = (0.8, 0.2)
//                     g_l = W_{l+1}^T d_{l+1},  dg_l = W_{l+1}^T dd_{l+1}
//                     d_l = g_l phi'(a_l),  dd_l = dg_l phi'(a_l) + g_l phi''(a_l) da_l
//                     g = W1^T d1,  hv = W1^T dd1 = H v
// softplus: phi' = z/(z+1), phi'' = phi'(1-phi') (threshold 20: 1 and 0);
// tanhshrink: phi' = th^2, phi'' = 2 th (1 - th^2).
// The value column's layer 1 is the one-hot column gather (dense at iteration
// 0 for a non-one-hot init); the tangent's is a dense +-1 combination of all
// 288 columns (allocation columns from LDS, cpu / ips columns from registers).
// Adahessian's moments live with the entry's lane; the per-iteration scalars
// come from a host table computed in double (gobi_so_table).  No atomics and a
// fixed order: an environment's bits do not depend on the batch, its position
// or its workgroup partner, and a converged environment is frozen while its
// partner continues.
#include <hip/hip_runtime.h>

#include <cmath>
#include <string>

#include "../../include/preganplus.h"
#include "pgp_device.hpp"
#include "pgp_gobi.hpp"
#include "pgp_philox.hpp"

namespace pgp {
namespace {

constexpr int kSE = 2;       // environments per workgroup
constexpr int kSignW = 9;    // 288 sign bits = 9 words per step
constexpr int kTapLen = 3 * kIn;

struct SoLds {
  float w1a[kN1 * kSA];  // W1[o][c*18 + 2 + h] at [o][c*16 + h]
  float x[kSE][kIn];
  alignas(8) float vs[kIn][kSE];  // this step's probe, +-1.0, [input entry][env]
  // the dot products' inputs k-major, [k][column] (pgp_gobi.hip's layout)
  alignas(16) float h1[kP1][kNE], h2[kP1][kNE], g2[kP1][kNE], g3[kP3][kNE], g1[kP1][kNE];
  // layer 3 per environment: h3 and its tangent dh3, tanh(a3), q3 = phi''(a3) da3
  float h3[kSE][kN3], dh3[kSE][kN3], th3[kSE][kN3], q3[kSE][kN3];
  float o[kSE][4];
  alignas(16) float tab[kMaxIt][4];  // lr, 1 - 0.9^t, sqrt(1 - 0.999^t)
  int hs[kSE][kH];   // each container's host (the one-hot column of its allocation row)
  int dense[kSE];    // the init's allocation is not one-hot (iteration 0 takes the dense layer 1)
  alignas(8) int flag[2][kSE];  // "some entry changed" of the current / next iteration
};

// sum over the wave's 64 lanes, the same bits in every lane
__device__ __forceinline__ float wave_sum(float p) {
  const auto a = __builtin_amdgcn_permlane32_swap(__float_as_uint(p), __float_as_uint(p), false, false);
  p = __uint_as_float(a[0]) + __uint_as_float(a[1]);
  p = pair_sum(p);
  p += dppf<kDppRor8>(p);
  p += dppf_xor4(p);
  p += dppf<kDppX2>(p);
  p += dppf<kDppX1>(p);
  return p;
}

// Forward of the surrogate for the columns in act (all threads; act is
// wave-uniform, act[2e + 1] implies act[2e]).  z = 0.8 o0 + 0.2 o1 in
// L.o[e][2]; with a tangent column active, the head's backward too: g3 holds
// d3 and dd3.  K: what the lane keeps of the activations it owns for the
// backward: a value lane a and exp(a), a tangent lane phi'(a) and phi''(a) da.
__device__ void so_fwd(const float* __restrict__ W, const GobiRegs& R, SoLds& L, FwdKeep& K, const bool (&act)[kNE],
                       const bool (&dense)[kSE]) {
#pragma clang fp contract(off)
  // the lane's roles recomputed per call from an opaque copy of its id: hoisted out of the
  // iteration loop, the phases' LDS addresses outnumber the registers the weights leave
  int t = threadIdx.x;
  asm volatile("" : "+v"(t));
  const int o = (t >> 6) * 16 + (t & 15), sp = (t >> 4) & 3, o3 = t >> 3, sp3 = t & 7;
  const bool tang = act[1] || act[3];
  bool act_sp = false, act_sp3 = false;
#pragma unroll
  for (int q = 0; q < kNE; ++q) {
    act_sp = sp == q ? act[q] : act_sp;
    act_sp3 = (sp3 >> 1) == q ? act[q] : act_sp3;
  }
  // layer 1 (288 -> 128): k-chunk sp = containers 4sp .. 4sp + 3
  float l1[kNE] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int e = 0; e < kSE; ++e) {
    if (!act[2 * e]) continue;
    float acc = 0.f;
    if (dense[e]) {  // any allocation
      const float* wr = W + GobiW::W1 + o * kIn + sp * 72;
      const float* xr = L.x[e] + sp * 72;
#pragma unroll 8
      for (int k = 0; k < 72; ++k) acc = fmaf(wr[k], xr[k], acc);
    } else {  // one-hot allocation: cpu, ips FMAs + the host's column (LDS)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c = 4 * sp + q;
        acc = fmaf(R.w1x[2 * q], L.x[e][c * kF], acc);
        acc = fmaf(R.w1x[2 * q + 1], L.x[e][c * kF + 1], acc);
        acc = acc + L.w1a[o * kSA + c * kH + L.hs[e][c]];
      }
    }
    l1[2 * e] = acc;
  }
  if (tang) {  // da1 = W1 v: the chunk's 72 columns in input order, both environments on every weight read
    float t0 = 0.f, t1 = 0.f;
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int c = 4 * sp + q;
      const float2 vc = *reinterpret_cast<const float2*>(L.vs[c * kF]);
      const float2 vi = *reinterpret_cast<const float2*>(L.vs[c * kF + 1]);
      t0 = fmaf(R.w1x[2 * q], vc.x, t0);
      t1 = fmaf(R.w1x[2 * q], vc.y, t1);
      t0 = fmaf(R.w1x[2 * q + 1], vi.x, t0);
      t1 = fmaf(R.w1x[2 * q + 1], vi.y, t1);
#pragma unroll 4
      for (int j = 0; j < kH; ++j) {
        const float w = L.w1a[o * kSA + c * kH + j];
        const float2 v = *reinterpret_cast<const float2*>(L.vs[c * kF + 2 + j]);
        t0 = fmaf(w, v.x, t0);
        t1 = fmaf(w, v.y, t1);
      }
    }
    l1[1] = t0;
    l1[3] = t1;
  }
  // the elementwise tail once per lane, for its own column sp; a tangent lane
  // also takes its environment's value sum (every lane holds all four)
  float mine = sum_rows(l1, act, sp);
  float val = (sp & 2) ? l1[2] : l1[0];
  if (act_sp) {
    const float a = val + R.b1;
    if (!(sp & 1)) {
      K.a1 = a;
      L.h1[kp(o)][sp] = softplus_keep(a, K.z1);
    } else {
      const float z = expf(a);
      const float p1 = a > 20.f ? 1.f : z / (z + 1.f);
      K.a1 = p1;
      K.z1 = (a > 20.f ? 0.f : p1 / (z + 1.f)) * mine;  // phi'' = phi' (1 - phi'), 1 - phi' = 1 / (z + 1) uncancelled
      L.h1[kp(o)][sp] = p1 * mine;
    }
  }
  __syncthreads();
  float r[kNE];
  // layer 2 (128 -> 128): W2 row o, k-chunk sp
  dotb<32>(&L.h1[kp(sp * 32)], R.w2f, act, r);
  mine = sum_rows(r, act, sp);
  val = (sp & 2) ? r[2] : r[0];
  if (act_sp) {
    const float a = val + R.b2;
    if (!(sp & 1)) {
      K.a2 = a;
      L.h2[kp(o)][sp] = softplus_keep(a, K.z2);
    } else {
      const float z = expf(a);
      const float p1 = a > 20.f ? 1.f : z / (z + 1.f);
      K.a2 = p1;
      K.z2 = (a > 20.f ? 0.f : p1 / (z + 1.f)) * mine;  // phi'' = phi' (1 - phi'), 1 - phi' = 1 / (z + 1) uncancelled
      L.h2[kp(o)][sp] = p1 * mine;
    }
  }
  __syncthreads();
  // layer 3 (128 -> 64), Tanhshrink: W3 row o3, k-chunk sp3; lanes 2q, 2q + 1 hold column q, lane 2q writes
  dot4<16>(R.w3f, &L.h2[kp(sp3 * 16)], r);
  mine = sum_pick<8>(r, sp3 >> 1);
  val = (sp3 & 4) ? r[2] : r[0];
  if (act_sp3 && !(sp3 & 1)) {
    const int e = sp3 >> 2;
    const float a = val + R.b3;
    const float th = tanhf(a);
    if (!(sp3 & 2)) {
      L.th3[e][o3] = th;
      L.h3[e][o3] = a - th;
    } else {
      L.dh3[e][o3] = th * th * mine;
      L.q3[e][o3] = 2.f * th * (1.f - th * th) * mine;
    }
  }
  __syncthreads();
  // layer 4 (64 -> 2), sigmoid, z, and the head's backward: wave e, lane = o3
  if (t < 64 * kSE) {
    const int e = t >> 6, l = t & 63;
    const bool on = e ? act[2] : act[0], ontan = e ? act[3] : act[1];
    if (on) {
      const float h3 = L.h3[e][l];
      const float p0 = wave_sum(R.w40 * h3), p1 = wave_sum(R.w41 * h3);
      const float a0 = p0 + R.b40, a1 = p1 + R.b41;
      const float e0 = expf(-a0), e1 = expf(-a1);
      const float o0 = 1.f / (1.f + e0), o1 = 1.f / (1.f + e1);  // sigmoid_f's bits
      if (l == 0) {
        L.o[e][0] = o0;
        L.o[e][1] = o1;
        L.o[e][2] = 0.8f * o0 + 0.2f * o1;
      }
      if (ontan) {
        const float dh3 = L.dh3[e][l];
        const float da0 = wave_sum(R.w40 * dh3), da1 = wave_sum(R.w41 * dh3);
        // o (1 - o) as o^2 e^-a where the sigmoid saturates upwards: 1 - o cancels there (torch's
        // g (1 - y) y is off by 2^-24 / (1 - o), 1e-5 of the whole gradient at a = 6)
        const float s0 = a0 > 0.f ? o0 * o0 * e0 : (1.f - o0) * o0, s1 = a1 > 0.f ? o1 * o1 * e1 : (1.f - o1) * o1;
        const float d0 = 0.8f * s0, d1 = 0.2f * s1;
        const float dd0 = d0 * (1.f - 2.f * o0) * da0, dd1 = d1 * (1.f - 2.f * o1) * da1;
        const float gh = R.w40 * d0 + R.w41 * d1, dgh = R.w40 * dd0 + R.w41 * dd1;
        const float th = L.th3[e][l];
        L.g3[kp(l)][2 * e] = gh - gh * (1.f - th * th);
        L.g3[kp(l)][2 * e + 1] = dgh * (th * th) + gh * L.q3[e][l];
      }
    }
  }
  __syncthreads();
}

// The whole optimisation of a workgroup's 2 environments on the surrogate W.
// GROUPED = false: environments 2 blockIdx.x, 2 blockIdx.x + 1 of the batch.
// GROUPED = true: the environments env[0..1] (< 0: the slot is empty), every
// array indexed by environment id.
template <bool GROUPED>
__device__ __forceinline__ void so_run(SoLds& L, int E, const float* __restrict__ W, const float* __restrict__ tab,
                                       const float* __restrict__ init, float* __restrict__ result,
                                       int* __restrict__ iterations, float* __restrict__ fitness, int max_it,
                                       const unsigned int* __restrict__ signs, int sign_steps,
                                       const unsigned long long* __restrict__ seeds, float* __restrict__ taps,
                                       const int (&env)[kSE]) {
#pragma clang fp contract(off)  // elementwise steps as torch's separate mul/add
  const long e0 = (long)blockIdx.x * kSE;
  auto envid = [&](int e) -> long {
    if constexpr (GROUPED)
      return e ? env[1] : env[0];
    else
      return e0 + e;
  };
  auto live = [&](int e) -> bool {
    if constexpr (GROUPED)
      return (e ? env[1] : env[0]) >= 0;
    else
      return e0 + e < E;
  };
  const int t = threadIdx.x;
  for (int k = t; k < kN1 * kA; k += kT) {
    const int oo = k / kA, a = k - oo * kA;
    L.w1a[oo * kSA + a] = W[GobiW::W1 + oo * kIn + (a >> 4) * kF + 2 + (a & 15)];
  }
  for (int k = t; k < kSE * kIn; k += kT) {
    const int e = k / kIn;
    L.x[e][k - e * kIn] = live(e) ? init[envid(e) * kIn + (k - e * kIn)] : 0.f;
  }
  for (int k = t; k < kMaxIt * 4; k += kT) (&L.tab[0][0])[k] = tab[k];
  if (t < kSE) {
    L.dense[t] = 0;
    L.flag[0][t] = L.flag[1][t] = 0;
  }
  // step `step`'s probe of every live environment: entry k's bit of its word
  // (explicit: signs[env][step][k >> 5]; generated: Philox4x32-10, key = the
  // environment's seed, counter = (k >> 5, step, 0, 0), output word 0), set = +1
  unsigned int k0[kSE] = {0u, 0u}, k1[kSE] = {0u, 0u};
  if (!signs) {
#pragma unroll
    for (int e = 0; e < kSE; ++e)
      if (live(e)) {
        const unsigned long long s = seeds[envid(e)];
        k0[e] = (unsigned int)s;
        k1[e] = (unsigned int)(s >> 32);
      }
  }
  auto probe = [&](int step, bool on0, bool on1) {
    for (int idx = t; idx < kSE * kIn; idx += kT) {
      const int e = idx >= kIn ? 1 : 0, k = idx - e * kIn;
      if (!(e ? on1 : on0)) continue;
      unsigned int w;
      if (signs)
        w = signs[((size_t)envid(e) * sign_steps + step) * kSignW + (k >> 5)];
      else
        w = philox4x32_10((unsigned int)(k >> 5), (unsigned int)step, 0u, 0u, e ? k0[1] : k0[0], e ? k1[1] : k1[0])
                .w[0];
      L.vs[k][e] = (w >> (k & 31)) & 1u ? 1.f : -1.f;
    }
  };
  for (int k = t; k < kSE * kIn; k += kT) (&L.vs[0][0])[k] = 1.f;
  GobiRegs R;
  load_regs(W, R);
  __syncthreads();
  if (max_it > 0) probe(0, live(0), live(1));
  if (t < kSE * kH) {  // is the init's allocation one-hot?  (then layer 1 is a column gather)
    const int e = t / kH, cc = t % kH;
    int ones = 0, other = 0, h = 0;
    for (int j = 0; j < kH; ++j) {
      const float xv = L.x[e][cc * kF + 2 + j];
      if (xv == 1.f) {
        ++ones;
        h = j;
      } else if (xv != 0.f) {
        ++other;
      }
    }
    L.hs[e][cc] = h;
    if (ones != 1 || other) L.dense[e] = 1;  // benign race: every writer stores 1
  }
  __syncthreads();
  float m = 0.f, s = 0.f;  // Adahessian's moments of this lane's entry (env sq)
  FwdKeep K{0.f, 0.f, 0.f, 0.f};
  bool act[kNE], dense[kSE];
  int equal[kSE], its[kSE];
#pragma unroll
  for (int e = 0; e < kSE; ++e) {
    act[2 * e] = act[2 * e + 1] = live(e);
    dense[e] = __builtin_amdgcn_readfirstlane(L.dense[e]) != 0;
    equal[e] = 0;
    its[e] = max_it;
  }
  int it = 0;
  while (it < max_it) {
    if (!act[0] && !act[2]) break;
    so_fwd(W, R, L, K, act, dense);
    // the lane's roles, recomputed per iteration (see so_fwd)
    int tl = threadIdx.x;
    asm volatile("" : "+v"(tl));
    const int o = (tl >> 6) * 16 + (tl & 15), sp = (tl >> 4) & 3;
    const int c = (tl >> 6) * 2 + ((tl >> 5) & 1), sq = (tl >> 4) & 1, hcol = tl & 15;
    const int xi = c * kF + 2 + hcol;  // this thread's allocation entry in the flattened input
    // ---- backward to the input: the gradient and its tangent side by side ----
    bool act_sp = false;
#pragma unroll
    for (int q = 0; q < kNE; ++q) act_sp = sp == q ? act[q] : act_sp;
    float r[kNE];
    // through layer 3 and layer 2's softplus (W3 column o, k-chunk sp)
    dotb<16>(&L.g3[kp(sp * 16)], R.w3b, act, r);
    float mine = sum_rows(r, act, sp);
    float val = (sp & 2) ? r[2] : r[0];
    if (act_sp) L.g2[kp(o)][sp] = (sp & 1) ? mine * K.a2 + val * K.z2 : softplus_grad(mine, K.a2, K.z2);
    if (t < kSE) L.flag[(it + 1) & 1][t] = 0;  // next iteration's flag; its last readers passed barriers since
    // the next step's probe (layer 1, its only reader, is barriers behind and ahead)
    if (it + 1 < max_it) probe(it + 1, act[0], act[2]);
    __syncthreads();
    // through layer 2 and layer 1's softplus (W2 column o, k-chunk sp)
    dotb<32>(&L.g2[kp(sp * 32)], R.w2b, act, r);
    mine = sum_rows(r, act, sp);
    val = (sp & 2) ? r[2] : r[0];
    if (act_sp) L.g1[kp(o)][sp] = (sp & 1) ? mine * K.a1 + val * K.z1 : softplus_grad(mine, K.a1, K.z1);
    __syncthreads();
    // test tap: g and hv of the 32 cpu / ips entries (their updates are discarded, so only a tap
    // wants them) from W1's transposed copy in memory; their "pre" is the value the projection restores
    if (taps && tl < 32 * kNE) {
      const int q = tl & 3, j = tl >> 2, e = q >> 1, k = (j >> 1) * kF + (j & 1);
      bool on = false;
#pragma unroll
      for (int u = 0; u < kNE; ++u) on = q == u ? act[u] : on;
      if (on) {
        const float* wr = W + GobiW::W1T + k * kN1;
        float acc = 0.f;
        for (int i = 0; i < kN1; ++i) acc = fmaf(wr[i], L.g1[kp(i)][q], acc);
        float* tp = taps + envid(e) * kTapLen;
        tp[(q & 1) * kIn + k] = acc;
        if (!(q & 1)) tp[2 * kIn + k] = L.x[e][k];
      }
    }
    // g and hv of the 256 allocation entries (W1[:, xi] . d1 / dd1, 2 k-chunks of 64)
    float gxa[kNE];
    dotb<64>(&L.g1[kp(sq * 64)], R.w1c, act, gxa);
    sum_pairs(gxa, act);
    const float4 sc = *reinterpret_cast<const float4*>(L.tab[it]);
    // lane sq owns the entry of env sq (register selects, not an indexed array)
    float g0 = gxa[0], h0 = gxa[1], g1 = gxa[2], h1 = gxa[3];
    asm volatile("" : "+v"(g0), "+v"(h0), "+v"(g1), "+v"(h1));
    const float gx = sq ? g1 : g0, hv = sq ? h1 : h0;
    const bool on = sq ? act[2] : act[0];
    const int e = sq;
    // ---- Adahessian (adahessian.py:153-168; hessian_power 1, weight decay 0) on the entry ----
    const float xold = L.x[e][xi];
    if (on) {
      m = fmaf(gx, 0.1f, m * 0.9f);             // exp_avg.mul_(beta1).add_(grad, alpha=1 - beta1): a fused a + alpha b
      s = s * 0.999f + 0.001f * hv * hv;        // exp_hessian_diag_sq.mul_(beta2).addcmul_(|hv|, |hv|, value=1 - beta2)
    }
    const float denom = sqrtf(s) / sc.z + 1e-4f;
    const float xv = xold - sc.x * (m / sc.y / denom);
    // ---- one-hot of the row's first argmax (opt.py:9-15) over the row's 16 lanes ----
    float best = xv;
    int bi = hcol;
    auto take = [&](float ov, int oi) {
      const bool b = ov > best || (ov == best && oi < bi);
      best = b ? ov : best;
      bi = b ? oi : bi;
    };
    take(dppf<kDppX1>(best), dppi<kDppX1>(bi));
    take(dppf<kDppX2>(best), dppi<kDppX2>(bi));
    take(dppf<kDppRor4>(best), dppi<kDppRor4>(bi));
    take(dppf<kDppRor8>(best), dppi<kDppRor8>(bi));
    if (on) {
      if (taps) {  // test tap: the step's g, hv and the values before the projection
        float* tp = taps + envid(e) * kTapLen;
        tp[xi] = gx;
        tp[kIn + xi] = hv;
        tp[2 * kIn + xi] = xv;
      }
      const float nv = bi == hcol ? 1.f : 0.f;
      if (nv != xold) L.flag[it & 1][e] = 1;  // benign race: every writer stores 1
      L.x[e][xi] = nv;
      if (bi == hcol) L.hs[e][c] = hcol;
    }
    __syncthreads();
    // convergence (opt.py:45-46), per environment, in every thread's registers
    const int2 fl = *reinterpret_cast<const int2*>(L.flag[it & 1]);
    const int flv[kSE] = {fl.x, fl.y};
#pragma unroll
    for (int q = 0; q < kSE; ++q) {
      dense[q] = false;  // one-hot from here on
      if (!act[2 * q]) continue;
      equal[q] = __builtin_amdgcn_readfirstlane(flv[q]) ? 0 : equal[q] + 1;
      if (equal[q] > kPatience) {
        its[q] = it;
        act[2 * q] = act[2 * q + 1] = false;
      }
    }
    ++it;
  }
  // final fitness of every real environment (value columns only)
#pragma unroll
  for (int e = 0; e < kSE; ++e) {
    act[2 * e] = live(e);
    act[2 * e + 1] = false;
  }
  so_fwd(W, R, L, K, act, dense);
  for (int k = t; k < kSE * kIn; k += kT) {
    const int e = k / kIn;
    if (live(e)) result[envid(e) * kIn + (k - e * kIn)] = L.x[e][k - e * kIn];
  }
  if (t < kSE && live(t)) {
    iterations[envid(t)] = t ? its[1] : its[0];
    fitness[envid(t)] = L.o[t][2];
  }
}

__global__ __launch_bounds__(kT) void gobi_so_kernel(int E, const float* __restrict__ W, const float* __restrict__ tab,
                                                     const float* __restrict__ init, float* __restrict__ result,
                                                     int* __restrict__ iterations, float* __restrict__ fitness,
                                                     int max_it, const unsigned int* __restrict__ signs,
                                                     int sign_steps, const unsigned long long* __restrict__ seeds,
                                                     float* __restrict__ taps) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  SoLds& L = *reinterpret_cast<SoLds*>(lds_raw);
  const int none[kSE] = {-1, -1};
  so_run<false>(L, E, W, tab, init, result, iterations, fitness, max_it, signs, sign_steps, seeds, taps, none);
}

// Workgroup b takes slots 2 (b & 1), 2 (b & 1) + 1 of row b >> 1 of
// pgp_gobi_plan_groups's table ([n_groups][5] int32: model, then 4 environment
// ids, -1 = empty).  The inert-slot rules are gobi_groups_kernel's: a model
// outside [0, M) ends the workgroup before it reads anything else, and an
// environment outside [0, E) or equal to an earlier slot of its row is empty.
__global__ __launch_bounds__(kT) void gobi_so_groups_kernel(int E, int M, const int* __restrict__ groups,
                                                            const float* __restrict__ W,
                                                            const float* __restrict__ tab,
                                                            const float* __restrict__ init,
                                                            float* __restrict__ result, int* __restrict__ iterations,
                                                            float* __restrict__ fitness, int max_it,
                                                            const unsigned int* __restrict__ signs, int sign_steps,
                                                            const unsigned long long* __restrict__ seeds,
                                                            float* __restrict__ taps) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  SoLds& L = *reinterpret_cast<SoLds*>(lds_raw);
  const int* row = groups + (size_t)(blockIdx.x >> 1) * (1 + kNE);
  const int model = row[0];
  if (model < 0 || model >= M) return;  // uniform: the whole workgroup
  int ids[kNE];
#pragma unroll
  for (int e = 0; e < kNE; ++e) {
    int id = row[1 + e];
    if (id < 0 || id >= E) id = -1;
#pragma unroll
    for (int q = 0; q < e; ++q)
      if (id == ids[q]) id = -1;
    ids[e] = id;
  }
  const bool hi = (blockIdx.x & 1) != 0;
  const int env[kSE] = {hi ? ids[2] : ids[0], hi ? ids[3] : ids[1]};
  if (env[0] < 0 && env[1] < 0) return;
  so_run<true>(L, E, W + (size_t)model * GobiW::SIZE, tab, init, result, iterations, fitness, max_it, signs,
               sign_steps, seeds, taps, env);
}

}  // namespace

// Per iteration i (step t = i + 1): lr_t of CosineAnnealingLR(T_max=10) in
// torch's recursive form from 0.8, bias_correction1 = 1 - 0.9^t and
// sqrt(bias_correction2) = sqrt(1 - 0.999^t), in double as the reference's
// Python does, rounded to fp32 where its tensor ops take them.
void gobi_so_table(float* h) {
  const double base = 0.8, T = 10.0;
  double lr = base;
  for (int i = 0; i < kMaxIt; ++i) {
    const int step = i + 1;
    h[i * 4 + 0] = (float)lr;
    h[i * 4 + 1] = (float)(1.0 - std::pow(0.9, step));
    h[i * 4 + 2] = (float)std::sqrt(1.0 - std::pow(0.999, step));
    h[i * 4 + 3] = 0.f;
    if ((step - 1 - 10) % 20 == 0)
      lr = lr + base * (1 - std::cos(M_PI / T)) / 2;
    else
      lr = (1 + std::cos(M_PI * step / T)) / (1 + std::cos(M_PI * (step - 1) / T)) * lr;
  }
}

// Reserves the two kernels' dynamic LDS on the current device, once per handle
// (pgp_gobi_create_many, where the first-order kernels reserve theirs).
bool gobi_so_reserve_lds() {
  return hipFuncSetAttribute(reinterpret_cast<const void*>(&gobi_so_kernel),
                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(SoLds)) == hipSuccess &&
         hipFuncSetAttribute(reinterpret_cast<const void*>(&gobi_so_groups_kernel),
                             hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(SoLds)) == hipSuccess;
}

}  // namespace pgp

using namespace pgp;

namespace {
// the argument checks both entries share, the handle's last (the others need no device); PGP_OK with
// *mi = the effective step limit
int so_check(pgp_gobi* g, int n_env, const void* init, const void* result, const void* iterations,
             const void* fitness, int max_iters, const void* signs, int sign_steps, const void* seeds, int* mi) {
  if (n_env < 0) return gobi_fail(PGP_ERR_ARG, "negative batch");
  *mi = (max_iters <= 0 || max_iters > kMaxIt) ? kMaxIt : max_iters;
  if (n_env == 0) return PGP_OK;
  if (!init || !result || !iterations || !fitness) return gobi_fail(PGP_ERR_ARG, "NULL input/output pointer");
  if ((signs != nullptr) == (seeds != nullptr))
    return gobi_fail(PGP_ERR_ARG, "second-order GOBI: pass signs (explicit probes) or seeds (generated), not both");
  if (signs && sign_steps < *mi)
    return gobi_fail(PGP_ERR_ARG, "second-order GOBI: sign_steps below the step limit (max_iters, or 200)");
  if (!g) return gobi_fail(PGP_ERR_ARG, "NULL optimiser");
  if (g->H != kH) return gobi_fail(PGP_ERR_UNSUPPORTED, "second-order GOBI: 16 hosts only (energy_latency_16)");
  return PGP_OK;
}
}  // namespace

extern "C" {

int pgp_gobi_so_optimize(pgp_gobi* g, int n_env, const float* init, float* result, int* iterations, float* fitness,
                         int max_iters, const unsigned int* signs, int sign_steps, const unsigned long long* seeds,
                         float* taps, void* stream) {
  int mi = 0;
  const int rc = so_check(g, n_env, init, result, iterations, fitness, max_iters, signs, sign_steps, seeds, &mi);
  if (rc != PGP_OK || n_env == 0) return rc;
  gobi_so_kernel<<<(n_env + kSE - 1) / kSE, kT, sizeof(SoLds), reinterpret_cast<hipStream_t>(stream)>>>(
      n_env, g->d_w, g->d_so, init, result, iterations, fitness, mi, signs, sign_steps, seeds, taps);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return gobi_fail(PGP_ERR_HIP, std::string("gobi_so_kernel: ") + hipGetErrorString(e));
  return PGP_OK;
}

int pgp_gobi_so_optimize_groups(pgp_gobi* g, int n_env, int n_groups, const int* groups, const float* init,
                                float* result, int* iterations, float* fitness, int max_iters,
                                const unsigned int* signs, int sign_steps, const unsigned long long* seeds,
                                float* taps, void* stream) {
  int mi = 0;
  if (n_groups < 0) return gobi_fail(PGP_ERR_ARG, "negative group count");
  if (n_env > 0 && n_groups > 0 && !groups) return gobi_fail(PGP_ERR_ARG, "NULL group table");
  const int rc = so_check(g, n_env, init, result, iterations, fitness, max_iters, signs, sign_steps, seeds, &mi);
  if (rc != PGP_OK || n_env == 0 || n_groups == 0) return rc;
  gobi_so_groups_kernel<<<2 * n_groups, kT, sizeof(SoLds), reinterpret_cast<hipStream_t>(stream)>>>(
      n_env, g->M, groups, g->d_w, g->d_so, init, result, iterations, fitness, mi, signs, sign_steps, seeds, taps);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return gobi_fail(PGP_ERR_HIP, std::string("gobi_so_groups_kernel: ") + hipGetErrorString(e));
  return PGP_OK;
}

}  // extern "C"
