// pgp_gobi.hip — GOBI, the schedule producer of the decision path (SURVEY §8f
// row f3): scheduler/GOBI.py:19-42 -> scheduler/BaGTI/src/opt.py:17-33 over
// the energy_latency_16 surrogate (scheduler/BaGTI/src/models.py:8-27), for a
// batch of independent environments.
//
// One 512-thread workgroup (8 waves, 2 per SIMD) runs the whole optimisation
// of kNE = 4 environments in-kernel (the reference's loop: up to 200 AdamW
// steps on the input matrix, one-hot projection after each, stop after 31
// unchanged steps); the four share the weight registers and every barrier,
// and the launch lasts as long as its slowest workgroup's iteration chain.
// The MLP (288-128-128-64-2) and its input gradient are VALU dot products
// split over the threads in fixed k-chunks whose association every variant
// keeps (the trajectories are bit-identical to round 2's v7): the 128-output
// layers and the input gradient on DPP rows (a row's chunk inputs spread over
// its 16 lanes and broadcast by v_fmac_f32_dpp row_newbcast, the chunk sums by
// permlane swaps), layer 3 and the head on lane groups (DPP butterflies).
// Layer 1's allocation columns sit in LDS (the forward's one-hot column
// gather); the other weights live in registers.  Once some environments of a
// workgroup have converged, only the active ones' chains run.  Elementwise
// semantics follow torch's CPU kernels (softplus threshold 20, tanhshrink =
// x - tanh x composite, sigmoid backward g(1-y)y, AdamW single-tensor op
// order); per-iteration AdamW scalars (cosine lr) are computed on the host in
// double, as torch does.
//
// gobi_groups_kernel is the same optimisation with one surrogate per
// workgroup, picked by a group table (a fleet whose environments have their
// own surrogates, scheduler/GOBI.py:11-17): see gobi_run<GROUPED>.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <string>
#include <vector>

#include "../../include/preganplus.h"
#include "pgp_device.hpp"
#include "pgp_gobi.hpp"

namespace pgp {
namespace {

// phase timing study (variant builds only): -DPGP_GOBI_PROF accumulates, in
// workgroup 0, the wall clock of each barrier-delimited phase over the run;
// pgp_gobi_prof_read copies the sums out
#ifdef PGP_GOBI_PROF
constexpr int kProfWG = 256, kProfSlots = 32;
__device__ unsigned long long g_gobi_prof[kProfWG][kProfSlots];
// (summed in the workgroup's LDS, L.prof, and added to g_gobi_prof once at
// the end: a global read-modify-write per mark stalled wave 0 for a memory
// round trip that the next barrier then charged to every phase)
#define GMARK(i)                                                        \
  do {                                                                  \
    if (threadIdx.x == 0) {                                             \
      const unsigned long long now_ = wall_clock64();                   \
      L.prof[i] += now_ - gmark_t_;                                     \
      if ((i) < 7 && act[0] + act[1] + act[2] + act[3] == 1)            \
        L.prof[16 + (i)] += now_ - gmark_t_;                            \
      gmark_t_ = now_;                                                  \
    }                                                                   \
  } while (0)
#else
#define GMARK(i) \
  do {           \
  } while (0)
#endif

// Layer 1's allocation columns (the forward's one-hot column gather) and the
// per-environment activations; the other weights are in registers.
struct GobiLds {
  float w1a[kN1 * kSA];  // W1[o][c*18 + 2 + h] at [o][c*16 + h]
  float x[kNE][kIn];
  // the dot products' inputs k-major ([k][env]: one 16-byte read gives the
  // four environments' k-th value), one pad row after every 16 (kp(k)) so the
  // lanes' chunks (16 or 32 rows each) start in different banks; the head's
  // and the input gradient's inputs per environment
  alignas(16) float h1[kP1][kNE], h2[kP1][kNE], g2[kP1][kNE], g3[kP3][kNE], g1[kP1][kNE];
  float h3[kNE][kN3], th3[kNE][kN3];
  float o[kNE][4];
  alignas(16) float adam[kMaxIt][4];  // the per-iteration AdamW scalars (GobiW::ADAM), read from LDS in the loop
  int hs[kNE][kH];   // each container's host (the one-hot column of its allocation row)
  int dense[kNE];    // the init's allocation is not one-hot (iteration 0 takes the dense layer 1)
  alignas(16) int flag[2][kNE];  // "some entry changed" of the current / next iteration (one 16-byte read)
#ifdef PGP_GOBI_PROF
  unsigned long long prof[kProfSlots];
#endif
};

// forward of the surrogate for the environments in act (all threads);
// z = 0.8 o0 + 0.2 o1 in L.o[e][2]; with grad, g3 = dz/dh3 through Tanhshrink.
// act / dense are wave-uniform (the same in every thread).
__device__ void surrogate_fwd(const float* __restrict__ W, const GobiRegs& R, GobiLds& L, FwdKeep& K, bool grad,
                              const bool (&act)[kNE], const bool (&dense)[kNE], unsigned long long& gmark_t_) {
  (void)gmark_t_;
  const int t = threadIdx.x, o = (t >> 6) * 16 + (t & 15), sp = (t >> 4) & 3, o3 = t >> 3, sp3 = t & 7;
  bool act_sp = false, act_sp3 = false;  // this lane's owned environments (sp; sp3 / 2) are active
#pragma unroll
  for (int e = 0; e < kNE; ++e) {
    act_sp = sp == e ? act[e] : act_sp;
    act_sp3 = (sp3 >> 1) == e ? act[e] : act_sp3;
  }
  float mine = 0.f;
  // layer 1 (288 -> 128)
  float l1[kNE] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
  for (int e = 0; e < kNE; ++e) {
    if (!act[e]) continue;
    float acc = 0.f;
    if (dense[e]) {  // any allocation: k-chunk sp of 72
      const float* wr = W + GobiW::W1 + o * kIn + sp * 72;
      const float* xr = L.x[e] + sp * 72;
#pragma unroll 8
      for (int k = 0; k < 72; ++k) acc = fmaf(wr[k], xr[k], acc);
    } else {  // one-hot allocation: containers 4sp..4sp+3: cpu, ips FMAs + their host's column (LDS)
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int c = 4 * sp + q;
        acc = fmaf(R.w1x[2 * q], L.x[e][c * kF], acc);
        acc = fmaf(R.w1x[2 * q + 1], L.x[e][c * kF + 1], acc);
        acc = acc + L.w1a[o * kSA + c * kH + L.hs[e][c]];  // w * 1.0; the other columns multiply 0
      }
    }
    l1[e] = acc;
  }
  mine = sum_rows(l1, act, sp);
  // the elementwise tail once per lane, for its own environment sp (not once
  // per environment under a quarter of the lanes)
  if (act_sp) {
    const float a = mine + R.b1;
    K.a1 = a;
    L.h1[kp(o)][sp] = softplus_keep(a, K.z1);
  }
  __syncthreads();
  GMARK(0);
  float r[kNE];
  // layer 2 (128 -> 128): W2 row o, k-chunk sp
  dotb<32>(&L.h1[kp(sp * 32)], R.w2f, act, r);
  mine = sum_rows(r, act, sp);
  if (act_sp) {
    const float a = mine + R.b2;
    K.a2 = a;
    L.h2[kp(o)][sp] = softplus_keep(a, K.z2);
  }
  __syncthreads();
  GMARK(1);
  // layer 3 (128 -> 64), Tanhshrink: W3 row o3, k-chunk sp3
  dot4<16>(R.w3f, &L.h2[kp(sp3 * 16)], r);
  mine = sum_pick<8>(r, sp3 >> 1);
  if (act_sp3) {  // lanes 2e and 2e + 1 both hold env e's sum; lane 2e writes
    const float a = mine + R.b3;
    const float th = tanhf(a);
    if (!(sp3 & 1)) {
      L.th3[sp3 >> 1][o3] = th;
      L.h3[sp3 >> 1][o3] = a - th;
    }
  }
  __syncthreads();
  GMARK(2);
  // layer 4 (64 -> 2), sigmoid, z; wave e, lane = o3
  if (t < 64 * kNE) {
    const int e = t >> 6, l = t & 63;
    bool on = false;
#pragma unroll
    for (int q = 0; q < kNE; ++q) on = e == q ? act[q] : on;
    if (on) {
      const float h3 = L.h3[e][l];
      float p0 = R.w40 * h3, p1 = R.w41 * h3;
      // 64-lane xor butterfly, offsets 32, 16, 8, 4, 2, 1 (the same bits in every
      // lane): 32 and 16 by permlane swaps instead of ds_bpermute round trips,
      // 8 = row_ror 8, 4 = two bank-masked row shifts, 2 and 1 = quad_perm.
      // The first step keeps the form the compiler gave the shuffle version:
      // the lane's own product fused into the add, fma(w, h3, partner's
      // rounded product)
      {
        const bool hi = (l & 32) != 0;
        const auto a0 = __builtin_amdgcn_permlane32_swap(__float_as_uint(p0), __float_as_uint(p0), false, false);
        const auto a1 = __builtin_amdgcn_permlane32_swap(__float_as_uint(p1), __float_as_uint(p1), false, false);
        p0 = fmaf(R.w40, h3, __uint_as_float(hi ? a0[0] : a0[1]));
        p1 = fmaf(R.w41, h3, __uint_as_float(hi ? a1[0] : a1[1]));
        p0 = pair_sum(p0);
        p1 = pair_sum(p1);
      }
      p0 += dppf<kDppRor8>(p0);
      p1 += dppf<kDppRor8>(p1);
      p0 += dppf_xor4(p0);
      p1 += dppf_xor4(p1);
      p0 += dppf<kDppX2>(p0);
      p1 += dppf<kDppX2>(p1);
      p0 += dppf<kDppX1>(p0);
      p1 += dppf<kDppX1>(p1);
      const float o0 = sigmoid_f(p0 + R.b40), o1 = sigmoid_f(p1 + R.b41);
      if (l == 0) {
        // the row address recomputed here (the compiler kept it in a scratch
        // slot across the loop and reloaded it every iteration)
        int ee = e;
        asm volatile("" : "+v"(ee));
        L.o[ee][0] = o0;
        L.o[ee][1] = o1;
        L.o[ee][2] = 0.8f * o0 + 0.2f * o1;
      }
      if (grad) {  // dz/do = (0.8, 0.2) through the sigmoids, dh3 = W4^T do, through Tanhshrink
        const float d0 = 0.8f * (1.f - o0) * o0, d1 = 0.2f * (1.f - o1) * o1;
        const float gh = R.w40 * d0 + R.w41 * d1;
        const float th = L.th3[e][l];
        L.g3[kp(l)][e] = gh - gh * (1.f - th * th);
      }
    }
  }
  __syncthreads();
  GMARK(3);
}

// The whole optimisation of a workgroup's kNE environments on the surrogate W.
// GROUPED = false (gobi_kernel): environments e0 .. e0 + 3 of the batch, e0 =
// 4 blockIdx.x.  GROUPED = true (gobi_groups_kernel): the environments env[0..3]
// of a group table's row (wave-uniform; < 0: the slot is empty), every array
// indexed by environment id.  Everything else is the same code, and the
// ungrouped instantiation is the kernel as it was.
template <bool GROUPED>
__device__ __forceinline__ void gobi_run(GobiLds& L, int E, const float* __restrict__ W,
                                         const float* __restrict__ init, float* __restrict__ result,
                                         int* __restrict__ iterations, float* __restrict__ fitness, int max_it,
                                         float* __restrict__ pre, const int (&env)[kNE]) {
#pragma clang fp contract(off)  // elementwise steps as torch's separate mul/add
  // slot e holds an environment / its id (a select chain: no dynamic index into the uniform ids)
  auto live = [&](int e) -> bool {
    if constexpr (GROUPED) {
      int id = env[0];
#pragma unroll
      for (int q = 1; q < kNE; ++q) id = e == q ? env[q] : id;
      return id >= 0;
    } else {
      return (long)blockIdx.x * kNE + e < E;
    }
  };
  auto envid = [&](int e) -> long {
    if constexpr (GROUPED) {
      int id = env[0];
#pragma unroll
      for (int q = 1; q < kNE; ++q) id = e == q ? env[q] : id;
      return id;
    } else {
      return (long)blockIdx.x * kNE + e;
    }
  };
  unsigned long long gmark_t_ = 0;
#ifdef PGP_GOBI_PROF
  gmark_t_ = wall_clock64();
#endif
  const int t = threadIdx.x, o = (t >> 6) * 16 + (t & 15), sp = (t >> 4) & 3;
  const int c = (t >> 6) * 2 + ((t >> 5) & 1), sq = (t >> 4) & 1, hcol = t & 15, entry = c * kH + hcol;
  const int xi = c * kF + 2 + hcol;  // this thread's allocation entry in the flattened input
  const long e0 = (long)blockIdx.x * kNE;
  for (int k = t; k < kN1 * kA; k += kT) {
    const int oo = k / kA, a = k - oo * kA;
    L.w1a[oo * kSA + a] = W[GobiW::W1 + oo * kIn + (a >> 4) * kF + 2 + (a & 15)];
  }
  for (int k = t; k < kNE * kIn; k += kT) {
    const int e = k / kIn;
    if constexpr (GROUPED)
      L.x[e][k - e * kIn] = live(e) ? init[envid(e) * kIn + (k - e * kIn)] : 0.f;
    else
      L.x[e][k - e * kIn] = e0 + e < E ? init[e0 * kIn + k] : 0.f;
  }
  for (int k = t; k < kMaxIt * 4; k += kT) (&L.adam[0][0])[k] = W[GobiW::ADAM + k];
  if (t < kNE) {
    L.dense[t] = 0;
    L.flag[0][t] = L.flag[1][t] = 0;
  }
#ifdef PGP_GOBI_PROF
  if (t < kProfSlots) L.prof[t] = 0;
#endif
  GobiRegs R;
  load_regs(W, R);
  __syncthreads();
  if (t < kNE * kH) {  // is the init's allocation one-hot?  (then layer 1 is a column gather)
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
#ifdef PGP_GOBI_PROF
  {
    const bool act[kNE] = {false, false, false, false};  // the prologue's mark
    GMARK(7);
  }
#endif
  float m[kNE / 2], v[kNE / 2];  // AdamW moments of this lane's entries (envs sq, sq + 2)
#pragma unroll
  for (int k = 0; k < kNE / 2; ++k) m[k] = v[k] = 0.f;
  FwdKeep K{0.f, 0.f, 0.f, 0.f};
  bool act[kNE], dense[kNE];
  int equal[kNE], its[kNE];
#pragma unroll
  for (int e = 0; e < kNE; ++e) {
    if constexpr (GROUPED)
      act[e] = env[e] >= 0;
    else
      act[e] = e0 + e < E;
    dense[e] = __builtin_amdgcn_readfirstlane(L.dense[e]) != 0;
    equal[e] = 0;
    its[e] = max_it;
  }
  int it = 0;
  while (it < max_it) {
    bool any = false;
#pragma unroll
    for (int e = 0; e < kNE; ++e) any |= act[e];
    if (!any) break;
#ifdef PGP_GOBI_PROF
    int nact_ = 0;
#pragma unroll
    for (int e = 0; e < kNE; ++e) nact_ += act[e];
    const unsigned long long it_t0_ = wall_clock64();
#endif
    surrogate_fwd(W, R, L, K, true, act, dense, gmark_t_);
    // ---- backward to the input (autograd of z; g3 came with the forward) ----
    bool act_sp = false;
#pragma unroll
    for (int e = 0; e < kNE; ++e) act_sp = sp == e ? act[e] : act_sp;
    float mine = 0.f;
    // dh2 = W3^T g3 through softplus (W3 column o, k-chunk sp)
    float r[kNE];
    dotb<16>(&L.g3[kp(sp * 16)], R.w3b, act, r);
    mine = sum_rows(r, act, sp);
    if (act_sp) L.g2[kp(o)][sp] = softplus_grad(mine, K.a2, K.z2);
    if (t < kNE) L.flag[(it + 1) & 1][t] = 0;  // next iteration's flag; its last readers passed barriers since
    __syncthreads();
    GMARK(4);
    // dh1 = W2^T g2 through softplus (W2 column o, k-chunk sp)
    dotb<32>(&L.g2[kp(sp * 32)], R.w2b, act, r);
    mine = sum_rows(r, act, sp);
    if (act_sp) L.g1[kp(o)][sp] = softplus_grad(mine, K.a1, K.z1);
    __syncthreads();
    GMARK(5);
    // dx for the 256 allocation entries (W1[:, xi] . g1, 2 k-chunks of 64), AdamW, one-hot
    // the row's chunk of g1 (64 k x 4 envs) spread over its 16 lanes (four
    // 16-byte reads instead of 64), every k broadcast into the active
    // environments' chains (dotb), then the chunk pair of rows 2m, 2m + 1
    // (c0 + c1 in both) by a permlane swap
    float gxa[kNE];
    dotb<64>(&L.g1[kp(sq * 64)], R.w1c, act, gxa);
    sum_pairs(gxa, act);
    // this iteration's AdamW scalars, from LDS (scalar loads from memory at the
    // loop top made the first phase's LDS waits wait for them too: one lgkmcnt
    // counts both; 0.714 -> see DESIGN §17)
    const float4 ad = *reinterpret_cast<const float4*>(L.adam[it]);
    const float a0 = ad.x, a1 = ad.y, a2 = ad.z;
    // lane sq owns the entry of envs e = sq + 2k: AdamW and the one-hot once
    // per k with every lane busy (rows sq = 0 and 1 on envs 2k and 2k + 1)
#pragma unroll
    for (int k = 0; k < kNE / 2; ++k) {
      if (!act[2 * k] && !act[2 * k + 1]) continue;
      const int e = sq + 2 * k;
      const bool on = sq ? act[2 * k + 1] : act[2 * k];
      // a lane select of two registers: written as `sq ? gxa[2k+1] : gxa[2k]`
      // the compiler made it an indexed load of gxa[2k + sq], i.e. gxa stored
      // to scratch and read back every iteration (4 stores + 2 loads in the
      // AdamW chain); the opaque copies keep it a v_cndmask
      float ga = gxa[2 * k], gb = gxa[2 * k + 1];
      asm volatile("" : "+v"(ga), "+v"(gb));
      const float gx = sq ? gb : ga;
      // ---- AdamW (torch single-tensor, opt.py:18 defaults) on the entry ----
      const float xold = L.x[e][xi];
      float& mm = m[k];
      float& vv = v[k];
      float xv = xold * a0;
      if (on) {
        mm = mm + 0.1f * (gx - mm);           // exp_avg.lerp_(grad, 1 - beta1)
        vv = vv * 0.999f + 0.001f * gx * gx;  // exp_avg_sq.mul_(beta2).addcmul_(grad, grad, 1 - beta2)
      }
      const float denom = sqrtf(vv) / a2 + 1e-8f;
      xv = xv + (-a1) * mm / denom;           // addcdiv_: self + value * t1 / t2 (ATen's order)
      // ---- one-hot of the row's first argmax (opt.py:9-15): the row's lanes of this sq ----
      // (max value, then lowest column) over the row's 16 lanes: xor 1, xor 2,
      // then the quads by rotations of 4 and 8 (each lane then holds the winner)
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
        // test tap: the step's values before the projection
        if constexpr (GROUPED) {
          if (pre) pre[envid(e) * kH * kH + entry] = xv;
        } else {
          if (pre) pre[(e0 + e) * kH * kH + entry] = xv;
        }
        const float nv = bi == hcol ? 1.f : 0.f;
        if (nv != xold) L.flag[it & 1][e] = 1;  // benign race: every writer stores 1
        L.x[e][xi] = nv;
        if (bi == hcol) L.hs[e][c] = hcol;
      }
    }
    __syncthreads();
    GMARK(6);
    // convergence (opt.py:28-31), per environment, in every thread's registers
    // (the four flags in one 16-byte read)
    const int4 fl = *reinterpret_cast<const int4*>(L.flag[it & 1]);
    const int flv[kNE] = {fl.x, fl.y, fl.z, fl.w};
#pragma unroll
    for (int e = 0; e < kNE; ++e) {
      dense[e] = false;  // one-hot from here on
      if (!act[e]) continue;
      equal[e] = __builtin_amdgcn_readfirstlane(flv[e]) ? 0 : equal[e] + 1;
      if (equal[e] > kPatience) {
        its[e] = it;
        act[e] = false;
      }
    }
#ifdef PGP_GOBI_PROF
    if (blockIdx.x < kProfWG && t == 0) {  // iteration time and count by active environments
      L.prof[7 + nact_] += wall_clock64() - it_t0_;
      L.prof[11 + nact_] += 1;
    }
#endif
    ++it;
  }
  // final fitness of every real environment
#pragma unroll
  for (int e = 0; e < kNE; ++e) {
    if constexpr (GROUPED)
      act[e] = env[e] >= 0;
    else
      act[e] = e0 + e < E;
  }
  surrogate_fwd(W, R, L, K, false, act, dense, gmark_t_);
  for (int k = t; k < kNE * kIn; k += kT) {
    const int e = k / kIn;
    if constexpr (GROUPED) {
      if (live(e)) result[envid(e) * kIn + (k - e * kIn)] = L.x[e][k - e * kIn];
    } else {
      if (e0 + e < E) result[e0 * kIn + k] = L.x[e][k - e * kIn];
    }
  }
  if (t < kNE && live(t)) {
    int n = its[0];
#pragma unroll
    for (int e = 1; e < kNE; ++e) n = t == e ? its[e] : n;  // no dynamic register-array index
    iterations[envid(t)] = n;
    fitness[envid(t)] = L.o[t][2];
  }
#ifdef PGP_GOBI_PROF
  if (blockIdx.x < kProfWG && t == 0) {
    for (int i = 0; i < 31; ++i) g_gobi_prof[blockIdx.x][i] += L.prof[i];
    g_gobi_prof[blockIdx.x][31] = (unsigned long long)it;
  }
#endif
}

__global__ __launch_bounds__(kT) void gobi_kernel(int E, const float* __restrict__ W, const float* __restrict__ init,
                                                  float* __restrict__ result, int* __restrict__ iterations,
                                                  float* __restrict__ fitness, int max_it, float* __restrict__ pre) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  GobiLds& L = *reinterpret_cast<GobiLds*>(lds_raw);
  const int none[kNE] = {-1, -1, -1, -1};
  gobi_run<false>(L, E, W, init, result, iterations, fitness, max_it, pre, none);
}

// One surrogate per group of up to kNE environments: workgroup b takes row b of
// groups ([n_groups][1 + kNE] int32: model, then environment ids, -1 = empty),
// loads model groups[b][0] of the M packed ones at W (GobiW::SIZE floats each)
// and runs the row's environments.  A table entry never becomes an address
// unchecked: a model outside [0, M) ends the workgroup before it reads
// anything else, and an environment outside [0, E) or equal to an earlier slot
// of its row is an empty slot.
__global__ __launch_bounds__(kT) void gobi_groups_kernel(int E, int M, const int* __restrict__ groups,
                                                         const float* __restrict__ W,
                                                         const float* __restrict__ init, float* __restrict__ result,
                                                         int* __restrict__ iterations, float* __restrict__ fitness,
                                                         int max_it, float* __restrict__ pre) {
  extern __shared__ __attribute__((aligned(16))) unsigned char lds_raw[];
  GobiLds& L = *reinterpret_cast<GobiLds*>(lds_raw);
  const int* row = groups + (size_t)blockIdx.x * (1 + kNE);
  const int model = row[0];
  if (model < 0 || model >= M) return;  // uniform: the whole workgroup
  int env[kNE];
#pragma unroll
  for (int e = 0; e < kNE; ++e) {
    int id = row[1 + e];
    if (id < 0 || id >= E) id = -1;
#pragma unroll
    for (int q = 0; q < e; ++q)
      if (id == env[q]) id = -1;
    env[e] = id;
  }
  gobi_run<true>(L, E, W + (size_t)model * GobiW::SIZE, init, result, iterations, fitness, max_it, pre, env);
}

}  // namespace
}  // namespace pgp

using namespace pgp;

namespace {
thread_local std::string g_gerr;
int gfail(int code, const std::string& msg) {
  g_gerr = msg;
  return code;
}

// one surrogate's device image (GobiW) from its state dict
void gobi_pack(const float* weights, float* h) {
  // state-dict order: find.0.weight [128,288], find.0.bias, find.2.weight [128,128], find.2.bias,
  //                   find.4.weight [64,128], find.4.bias, find.6.weight [2,64], find.6.bias
  const float* w1 = weights;
  const float* b1 = w1 + kN1 * kIn;
  const float* w2 = b1 + kN1;
  const float* b2 = w2 + kN2 * kN1;
  const float* w3 = b2 + kN2;
  const float* b3 = w3 + kN3 * kN2;
  const float* w4 = b3 + kN3;
  const float* b4 = w4 + 2 * kN3;
  for (int k = 0; k < GobiW::SIZE; ++k) h[k] = 0.f;
  for (int o = 0; o < kN1; ++o)
    for (int k = 0; k < kIn; ++k) {
      h[GobiW::W1 + o * kIn + k] = w1[o * kIn + k];
      h[GobiW::W1T + k * kN1 + o] = w1[o * kIn + k];
    }
  for (int o = 0; o < kN2; ++o)
    for (int k = 0; k < kN1; ++k) {
      h[GobiW::W2 + o * kN1 + k] = w2[o * kN1 + k];
      h[GobiW::W2T + k * kN2 + o] = w2[o * kN1 + k];
    }
  for (int o = 0; o < kN3; ++o)
    for (int k = 0; k < kN2; ++k) {
      h[GobiW::W3 + o * kN2 + k] = w3[o * kN2 + k];
      h[GobiW::W3T + k * kN3 + o] = w3[o * kN2 + k];
    }
  for (int i = 0; i < kN1; ++i) h[GobiW::B1 + i] = b1[i];
  for (int i = 0; i < kN2; ++i) h[GobiW::B2 + i] = b2[i];
  for (int i = 0; i < kN3; ++i) h[GobiW::B3 + i] = b3[i];
  for (int i = 0; i < 2 * kN3; ++i) h[GobiW::W4 + i] = w4[i];
  h[GobiW::B4] = b4[0];
  h[GobiW::B4 + 1] = b4[1];
  // AdamW(lr=0.8, betas (0.9, 0.999), eps 1e-8, weight_decay 1e-2) under
  // CosineAnnealingLR(T_max=10), torch's recursive update, in double as torch does
  const double base = 0.8, wd = 1e-2, T = 10.0;
  double lr = base;
  for (int i = 0; i < kMaxIt; ++i) {
    const int step = i + 1;
    h[GobiW::ADAM + i * 4 + 0] = (float)(1.0 - lr * wd);
    h[GobiW::ADAM + i * 4 + 1] = (float)(lr / (1.0 - std::pow(0.9, step)));
    h[GobiW::ADAM + i * 4 + 2] = (float)std::sqrt(1.0 - std::pow(0.999, step));
    h[GobiW::ADAM + i * 4 + 3] = (float)lr;
    const int ep = i + 1;
    if ((ep - 1 - 10) % 20 == 0)
      lr = lr + base * (1 - std::cos(M_PI / T)) / 2;
    else
      lr = (1 + std::cos(M_PI * ep / T)) / (1 + std::cos(M_PI * (ep - 1) / T)) * lr;
  }
}

constexpr const char* kGobiHosts = "GOBI surrogate: only energy_latency_16 exists (16 hosts)";
}  // namespace

int pgp::gobi_fail(int code, const std::string& msg) { return gfail(code, msg); }

extern "C" {

size_t pgp_gobi_weight_len(int n_hosts) {
  if (n_hosts != kH) return 0;
  return (size_t)kN1 * kIn + kN1 + kN2 * kN1 + kN2 + kN3 * kN2 + kN3 + 2 * kN3 + 2;
}

int pgp_gobi_create_many(int n_hosts, int n_models, const float* weights, size_t len, pgp_gobi** out) {
  if (!out) return gfail(PGP_ERR_ARG, "out is NULL");
  *out = nullptr;
  if (n_hosts != kH) return gfail(PGP_ERR_UNSUPPORTED, kGobiHosts);
  if (n_models < 1) return gfail(PGP_ERR_ARG, "GOBI: at least one model");
  const size_t wl = pgp_gobi_weight_len(n_hosts);
  if (!weights || len != wl * (size_t)n_models) return gfail(PGP_ERR_ARG, "GOBI weight length mismatch");
  std::vector<float> h((size_t)GobiW::SIZE * n_models);
  for (int m = 0; m < n_models; ++m) gobi_pack(weights + wl * m, h.data() + (size_t)GobiW::SIZE * m);
  pgp_gobi* g = new pgp_gobi();
  g->H = n_hosts;
  g->M = n_models;
  if (hipFuncSetAttribute(reinterpret_cast<const void*>(&gobi_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                          (int)sizeof(GobiLds)) != hipSuccess ||
      hipFuncSetAttribute(reinterpret_cast<const void*>(&gobi_groups_kernel),
                          hipFuncAttributeMaxDynamicSharedMemorySize, (int)sizeof(GobiLds)) != hipSuccess ||
      !gobi_so_reserve_lds()) {
    delete g;
    return gfail(PGP_ERR_HIP, "GOBI: cannot reserve LDS");
  }
  std::vector<float> so(kMaxIt * 4);  // so_opt()'s scalars (pgp_gobi_so_optimize)
  gobi_so_table(so.data());
  if (hipMalloc(&g->d_w, h.size() * sizeof(float)) != hipSuccess ||
      hipMemcpy(g->d_w, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess ||
      hipMalloc(&g->d_so, so.size() * sizeof(float)) != hipSuccess ||
      hipMemcpy(g->d_so, so.data(), so.size() * sizeof(float), hipMemcpyHostToDevice) != hipSuccess) {
    if (g->d_w) (void)hipFree(g->d_w);
    if (g->d_so) (void)hipFree(g->d_so);
    delete g;
    return gfail(PGP_ERR_HIP, "GOBI weight upload failed");
  }
  *out = g;
  return PGP_OK;
}

int pgp_gobi_create(int n_hosts, const float* weights, size_t len, pgp_gobi** out) {
  return pgp_gobi_create_many(n_hosts, 1, weights, len, out);
}

int pgp_gobi_model_count(const pgp_gobi* g) { return g ? g->M : 0; }

int pgp_gobi_set_model(pgp_gobi* g, int m, const float* weights, size_t len) {
  if (!g) return gfail(PGP_ERR_ARG, "NULL optimiser");
  if (m < 0 || m >= g->M) return gfail(PGP_ERR_ARG, "GOBI: model index outside the handle");
  if (!weights || len != pgp_gobi_weight_len(g->H)) return gfail(PGP_ERR_ARG, "GOBI weight length mismatch");
  std::vector<float> h(GobiW::SIZE);
  gobi_pack(weights, h.data());
  if (hipMemcpy(g->d_w + (size_t)GobiW::SIZE * m, h.data(), h.size() * sizeof(float), hipMemcpyHostToDevice) !=
      hipSuccess)
    return gfail(PGP_ERR_HIP, "GOBI weight upload failed");
  return PGP_OK;
}

int pgp_gobi_plan_groups(int n_env, const int* model_of_env, int n_models, int* groups_out, int cap) {
  if (n_env < 0 || n_models < 0 || cap < 0) return gfail(PGP_ERR_ARG, "plan_groups: negative count");
  if (n_env == 0) return 0;
  if (!model_of_env) return gfail(PGP_ERR_ARG, "plan_groups: NULL model_of_env");
  std::vector<long> count(n_models, 0), first(n_models + 1, 0);
  for (int e = 0; e < n_env; ++e) {
    if (model_of_env[e] < 0 || model_of_env[e] >= n_models)
      return gfail(PGP_ERR_ARG, "plan_groups: model index outside [0, n_models)");
    ++count[model_of_env[e]];
  }
  for (int m = 0; m < n_models; ++m) first[m + 1] = first[m] + (count[m] + kNE - 1) / kNE;  // groups before model m
  const long n_groups = first[n_models];
  if (n_groups > cap || !groups_out) return gfail(PGP_ERR_ARG, "plan_groups: cap too small for the groups");
  for (long k = 0; k < n_groups * (1 + kNE); ++k) groups_out[k] = -1;
  std::fill(count.begin(), count.end(), 0);
  for (int e = 0; e < n_env; ++e) {  // ascending id within each model
    const int m = model_of_env[e];
    const long g = first[m] + count[m] / kNE, slot = count[m] % kNE;
    groups_out[g * (1 + kNE)] = m;
    groups_out[g * (1 + kNE) + 1 + slot] = e;
    ++count[m];
  }
  return (int)n_groups;
}

int pgp_gobi_destroy(pgp_gobi* g) {
  if (!g) return PGP_OK;
  if (g->d_w) (void)hipFree(g->d_w);
  if (g->d_so) (void)hipFree(g->d_so);
  delete g;
  return PGP_OK;
}

const char* pgp_gobi_last_error(void) { return g_gerr.c_str(); }

#ifdef PGP_GOBI_PROF
int pgp_gobi_prof_read(unsigned long long* out) {  // phase sums of workgroup 0 (timing variant only)
  return hipMemcpyFromSymbol(out, HIP_SYMBOL(g_gobi_prof), sizeof(g_gobi_prof)) == hipSuccess ? 0 : -1;
}
int pgp_gobi_prof_reset(void) {
  static const unsigned long long z[kProfWG * kProfSlots] = {};
  return hipMemcpyToSymbol(HIP_SYMBOL(g_gobi_prof), z, sizeof(z)) == hipSuccess ? 0 : -1;
}
#endif

int pgp_gobi_optimize(pgp_gobi* g, int n_env, const float* init, float* result, int* iterations, float* fitness,
                      int max_iters, float* pre, void* stream) {
  if (!g) return gfail(PGP_ERR_ARG, "NULL optimiser");
  if (n_env < 0) return gfail(PGP_ERR_ARG, "negative batch");
  if (n_env == 0) return PGP_OK;
  if (!init || !result || !iterations || !fitness) return gfail(PGP_ERR_ARG, "NULL input/output pointer");
  const int mi = (max_iters <= 0 || max_iters > kMaxIt) ? kMaxIt : max_iters;
  gobi_kernel<<<(n_env + kNE - 1) / kNE, kT, sizeof(GobiLds), reinterpret_cast<hipStream_t>(stream)>>>(n_env, g->d_w, init, result,
                                                                                          iterations, fitness, mi, pre);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return gfail(PGP_ERR_HIP, std::string("gobi_kernel: ") + hipGetErrorString(e));
  return PGP_OK;
}

int pgp_gobi_optimize_groups(pgp_gobi* g, int n_env, int n_groups, const int* groups, const float* init,
                             float* result, int* iterations, float* fitness, int max_iters, float* pre,
                             void* stream) {
  if (!g) return gfail(PGP_ERR_ARG, "NULL optimiser");
  if (n_env < 0 || n_groups < 0) return gfail(PGP_ERR_ARG, "negative batch or group count");
  if (n_env == 0 || n_groups == 0) return PGP_OK;
  if (!groups || !init || !result || !iterations || !fitness)
    return gfail(PGP_ERR_ARG, "NULL table or input/output pointer");
  const int mi = (max_iters <= 0 || max_iters > kMaxIt) ? kMaxIt : max_iters;
  gobi_groups_kernel<<<n_groups, kT, sizeof(GobiLds), reinterpret_cast<hipStream_t>(stream)>>>(
      n_env, g->M, groups, g->d_w, init, result, iterations, fitness, mi, pre);
  const hipError_t e = hipGetLastError();
  if (e != hipSuccess) return gfail(PGP_ERR_HIP, std::string("gobi_groups_kernel: ") + hipGetErrorString(e));
  return PGP_OK;
}

}  // extern "C"
