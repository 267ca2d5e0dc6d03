// pgp_gobi.hpp — what GOBI's optimiser kernels share: the surrogate's packed
// image (GobiW), the handle, the thread roles' weight registers and the DPP /
// permlane dot-product helpers over 4 right-hand-side columns.  pgp_gobi.hip
// (opt(), AdamW: the columns are 4 environments) and pgp_gobi_so.hip (so_opt(),
// Adahessian: {value, tangent} x 2 environments) include it; every helper is
// internal to its translation unit.
#pragma once
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/preganplus.h"
#include "pgp_device.hpp"

struct pgp_gobi {
  int H = 0;
  int M = 0;              // surrogates in d_w
  float* d_w = nullptr;   // [M][GobiW::SIZE]
  float* d_so = nullptr;  // [200][4]: so_opt()'s per-iteration scalars (pgp::gobi_so_table)
};

namespace pgp {

// pgp_gobi_last_error()'s message (pgp_gobi.hip); returns code
int gobi_fail(int code, const std::string& msg);
// so_opt()'s per-iteration scalars, 200 x 4 floats (pgp_gobi_so.hip)
void gobi_so_table(float* h);
// reserves the second-order kernels' dynamic LDS on the current device (pgp_gobi_so.hip)
bool gobi_so_reserve_lds();

namespace {

constexpr int kH = 16, kF = 2 + kH, kIn = kH * kF;  // 16 containers x [cpu, ips, one-hot 16] = 288
constexpr int kN1 = 128, kN2 = 128, kN3 = 64;
constexpr int kMaxIt = 200, kPatience = 30;

struct GobiW {  // device offsets (floats) into one buffer
  static constexpr int W1T = 0;                    // [288][128]
  static constexpr int W1 = W1T + kIn * kN1;       // [128][288]
  static constexpr int B1 = W1 + kN1 * kIn;        // [128]
  static constexpr int W2T = B1 + kN1;             // [128][128]
  static constexpr int W2 = W2T + kN1 * kN2;       // [128][128]
  static constexpr int B2 = W2 + kN2 * kN1;
  static constexpr int W3T = B2 + kN2;             // [128][64]
  static constexpr int W3 = W3T + kN2 * kN3;       // [64][128]
  static constexpr int B3 = W3 + kN3 * kN2;
  static constexpr int W4 = B3 + kN3;              // [2][64]
  static constexpr int B4 = W4 + 2 * kN3;
  static constexpr int ADAM = B4 + 4;              // [200][4]: decay, step size, sqrt(bc2), lr
  static constexpr int SIZE = ADAM + kMaxIt * 4;
};

__device__ __forceinline__ float sigmoid_f(float x) { return 1.f / (1.f + expf(-x)); }

constexpr int kT = 512;  // threads per workgroup (8 waves, 2 per SIMD: 256 VGPRs for the weight slices)
constexpr int kNE = 4;   // right-hand-side columns per workgroup: they share the weight registers and every barrier

constexpr int kA = kH * kH;  // allocation entries
__host__ __device__ constexpr int kp(int k) { return k + (k >> 4); }  // padded k-major row
constexpr int kP1 = kp(kN1), kP3 = kp(kN3);
constexpr int kSA = kA + 1;  // LDS row stride of layer 1's allocation columns (257 = 1 mod 64)

// Thread roles (fixed for the whole run; every weight slice is loaded once):
//   128-output layers (1, 2 and the backward's dh2, dh1): wave w, row r, row
//     lane i: o = 16w + i, k-chunk sp = r; the rows' sums (row_sum4: the bits
//     of the 4-lane butterfly) in every lane, and row sp == e owns env e's
//     activation and keeps its pre-activation for the backward;
//   layer 3 (64 outputs): o3 = t >> 3, k-chunk sp3 = t & 7, owner lane 2e;
//   the head: wave e (t < 256), lane = o3;
//   allocation entries: a DPP row of 16 lanes (row r of wave w) is container
//     c = 2w + (r >> 1), lane = host, k-chunk sq = r & 1 of the input gradient
//     (the chunk pair of an entry in lanes l and l ^ 16); the lane owns the
//     entry of envs e = sq, sq + 2 (their AdamW moments).
struct GobiRegs {
  float w2f[32], w2b[32], w3f[16], w3b[16], w1c[64];
  float w1x[8];  // layer 1's cpu / ips weights of this lane's 4 containers
  float b1, b2, b3, w40, w41, b40, b41;
};

__device__ void load_regs(const float* __restrict__ W, GobiRegs& R) {
  const int t = threadIdx.x, o = (t >> 6) * 16 + (t & 15), sp = (t >> 4) & 3, o3 = t >> 3, sp3 = t & 7;
  const int sq = (t >> 4) & 1, xi = ((t >> 6) * 2 + ((t >> 5) & 1)) * kF + 2 + (t & 15);
#pragma unroll
  for (int j = 0; j < 64; ++j) R.w1c[j] = W[GobiW::W1T + xi * kN1 + sq * 64 + j];  // W1[k][xi]
#pragma unroll
  for (int j = 0; j < 32; ++j) R.w2f[j] = W[GobiW::W2 + o * kN1 + sp * 32 + j];   // W2[o][k]
#pragma unroll
  for (int j = 0; j < 32; ++j) R.w2b[j] = W[GobiW::W2T + o * kN2 + sp * 32 + j];  // W2[k][o]
#pragma unroll
  for (int j = 0; j < 16; ++j) R.w3f[j] = W[GobiW::W3 + o3 * kN2 + sp3 * 16 + j];  // W3[o3][k]
#pragma unroll
  for (int j = 0; j < 16; ++j) R.w3b[j] = W[GobiW::W3T + o * kN3 + sp * 16 + j];   // W3[k][o]
#pragma unroll
  for (int q = 0; q < 4; ++q) {
    const int c = 4 * sp + q;
    R.w1x[2 * q] = W[GobiW::W1 + o * kIn + c * kF];
    R.w1x[2 * q + 1] = W[GobiW::W1 + o * kIn + c * kF + 1];
  }
  R.b1 = W[GobiW::B1 + o];
  R.b2 = W[GobiW::B2 + o];
  R.b3 = W[GobiW::B3 + o3];
  R.w40 = W[GobiW::W4 + (t & 63)];
  R.w41 = W[GobiW::W4 + kN3 + (t & 63)];
  R.b40 = W[GobiW::B4];
  R.b41 = W[GobiW::B4 + 1];
}

// cross-lane moves inside a 16-lane row as DPP operand modifiers (a few cycles)
// instead of ds_bpermute round trips (__shfl_xor): quad_perm [1,0,3,2] = xor 1,
// [2,3,0,1] = xor 2; row_half_mirror (lane i <- 7 - i of its 8) pairs the two
// quads of an 8-lane group; row_ror 8 = xor 8; row_ror 4 rotates the row.  Every
// sum keeps the butterfly's association (bitwise as the shuffles)
constexpr int kDppX1 = 0xB1, kDppX2 = 0x4E, kDppHalfMirror = 0x141, kDppRor4 = 0x124, kDppRor8 = 0x128;
template <int CTRL>
__device__ __forceinline__ float dppf(float v) {
  return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), CTRL, 0xF, 0xF, false));
}
template <int CTRL>
__device__ __forceinline__ int dppi(int v) {
  return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, false);
}
// lane i <- lane i ^ 4 (row_shl 4 into banks 0 / 2, row_shr 4 into banks 1 / 3)
__device__ __forceinline__ float dppf_xor4(float v) {
  const int b = __float_as_int(v);
  const int lo = __builtin_amdgcn_update_dpp(0, b, 0x104, 0xF, 0x5, false);  // row_shl:4, banks 0, 2
  return __int_as_float(__builtin_amdgcn_update_dpp(lo, b, 0x114, 0xF, 0xA, false));  // row_shr:4, banks 1, 3
}

// sum over N aligned adjacent lanes (N = 2, 4, 8), the same bits in all of them:
// xor 1, xor 2, then the two 4-lane halves (whose lanes already agree) exchanged
template <int N>
__device__ __forceinline__ float lane_sum(float v) {
  static_assert(N == 2 || N == 4 || N == 8, "lane groups of 2, 4 or 8");
  v += dppf<kDppX1>(v);
  if constexpr (N >= 4) v += dppf<kDppX2>(v);
  if constexpr (N >= 8) v += dppf<kDppHalfMirror>(v);  // == lane i ^ 4's value: the quads already agree
  return v;
}

// the four environments' partial dot products over this lane's N-k chunk:
// w[j] times h[kp(j)][e] (h at the chunk's first row, a multiple of 16), one
// 16-byte LDS read per k feeding four independent fmaf chains (one per
// environment, each in k order as before).  The reads go in groups of 2 k,
// the next group's issued before this group's FMAs; the scheduling barriers
// keep the compiler from hoisting every read of the chunk (it would spill the
// weight registers to hold them)
template <int N>
__device__ __forceinline__ void dot4(const float* w, const float (*h)[kNE], float (&r)[kNE]) {
  constexpr int G = 2;
  static_assert(N % G == 0, "chunk of whole groups");
  auto ld = [&](int j) { return *reinterpret_cast<const float4*>(h[kp(j)]); };
#pragma unroll
  for (int e = 0; e < kNE; ++e) r[e] = 0.f;
  float4 cur[G], nxt[G];
#pragma unroll
  for (int q = 0; q < G; ++q) cur[q] = ld(q);
#pragma unroll
  for (int g = 0; g < N / G; ++g) {
    if (g + 1 < N / G) {
#pragma unroll
      for (int q = 0; q < G; ++q) nxt[q] = ld((g + 1) * G + q);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < G; ++q) {
      const float wj = w[g * G + q];
      r[0] = fmaf(wj, cur[q].x, r[0]);
      r[1] = fmaf(wj, cur[q].y, r[1]);
      r[2] = fmaf(wj, cur[q].z, r[2]);
      r[3] = fmaf(wj, cur[q].w, r[3]);
    }
    __builtin_amdgcn_sched_barrier(0);
#pragma unroll
    for (int q = 0; q < G; ++q) cur[q] = nxt[q];
  }
}
// the k-chunk dot products of the 128-output layers for the four environments:
// row r of the wave holds chunk sp = r; its N inputs x 4 envs (k-major rows h,
// from the chunk's first) are spread over the row's 16 lanes, P = N / 16
// consecutive k each (P 16-byte reads), and k = J is broadcast from row lane
// J / P (component J % P) into each environment's fmaf chain, in k order as
// dot4's.  All four active: the chains side by side; otherwise only the
// active environments' chains run (the others' sums are left at 0, unused).
// Each multiply-add is one v_fmac_f32 with a row_newbcast source (the builtin
// form costs a separate v_mov_b32_dpp).  A DPP instruction reads its swizzled
// source as of 2 wait states back, and inline asm hides it from the compiler's
// hazard check.  The sources here are LDS loads (no VALU writes them), and
// tools/dpp_hazard_check.py checks the BUILT kernel for any VALU write of a
// DPP source within 2 wait states (tests/test_roofline_isa.py runs it on the
// library's gobi_kernel, tests/test_sogobi_oracle.py on the second-order
// kernels, so a compiler-inserted copy fails the CPU suite).  A tied s_nop
// before the chains instead made the loads complete before the first FMA
// (0.731 -> 0.756 ms).
// acc += (row lane L's g) * w
template <int L>
__device__ __forceinline__ void fmac_bcast(float& acc, float g, float w) {
  asm("v_fmac_f32_dpp %0, %1, %2 row_newbcast:%3 row_mask:0xf bank_mask:0xf" : "+v"(acc) : "v"(g), "v"(w), "i"(L));
}
// chain1: one environment's chain (k = J)
template <int P, int E, int J, int N>
__device__ __forceinline__ void chain1(const float4 (&gq)[P], const float* w, float& a) {
  const float4 g = gq[J % P];
  fmac_bcast<J / P>(a, E == 0 ? g.x : E == 1 ? g.y : E == 2 ? g.z : g.w, w[J]);
  if constexpr (J + 1 < N) chain1<P, E, J + 1, N>(gq, w, a);
}
// chain4: the four chains side by side
template <int P, int J, int N>
__device__ __forceinline__ void chain4(const float4 (&gq)[P], const float* w, float (&a)[kNE]) {
  const float4 g = gq[J % P];
  fmac_bcast<J / P>(a[0], g.x, w[J]);
  fmac_bcast<J / P>(a[1], g.y, w[J]);
  fmac_bcast<J / P>(a[2], g.z, w[J]);
  fmac_bcast<J / P>(a[3], g.w, w[J]);
  if constexpr (J + 1 < N) chain4<P, J + 1, N>(gq, w, a);
}
template <int N, int P>
__device__ __forceinline__ void dotb_regs(const float4 (&gq)[P], const float* w, const bool (&act)[kNE],
                                          float (&r)[kNE]) {
  static_assert(P == N / 16, "P inputs per row lane");
#pragma unroll
  for (int e = 0; e < kNE; ++e) r[e] = 0.f;
  if (act[0] && act[1] && act[2] && act[3]) {
    chain4<P, 0, N>(gq, w, r);
  } else {
    if (act[0]) chain1<P, 0, 0, N>(gq, w, r[0]);
    if (act[1]) chain1<P, 1, 0, N>(gq, w, r[1]);
    if (act[2]) chain1<P, 2, 0, N>(gq, w, r[2]);
    if (act[3]) chain1<P, 3, 0, N>(gq, w, r[3]);
  }
}
template <int N>
__device__ __forceinline__ void dotb(const float (*h)[kNE], const float* w, const bool (&act)[kNE], float (&r)[kNE]) {
  constexpr int P = N / 16;
  const int lane = threadIdx.x & 15;
  float4 gq[P];
#pragma unroll
  for (int q = 0; q < P; ++q) gq[q] = *reinterpret_cast<const float4*>(h[kp(P * lane + q)]);
  dotb_regs<N, P>(gq, w, act, r);
}
// sum over the wave's 4 rows (lanes l ^ 16, then l ^ 32) by permlane swaps:
// every lane gets (c0 + c1) + (c2 + c3), the bits of the 4-lane butterfly
__device__ __forceinline__ float row_sum4(float v) {
  const auto a = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  v = __uint_as_float(a[0]) + __uint_as_float(a[1]);
  const auto b = __builtin_amdgcn_permlane32_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(b[0]) + __uint_as_float(b[1]);
}
// the row sums of the active environments' partials (all four: side by side,
// no branch); the one of env `mine_e`
__device__ __forceinline__ float sum_rows(float (&r)[kNE], const bool (&act)[kNE], int mine_e) {
  float m = 0.f;
  if (act[0] && act[1] && act[2] && act[3]) {
#pragma unroll
    for (int e = 0; e < kNE; ++e) {
      r[e] = row_sum4(r[e]);
      m = mine_e == e ? r[e] : m;
    }
  } else {
#pragma unroll
    for (int e = 0; e < kNE; ++e) {
      if (!act[e]) continue;
      r[e] = row_sum4(r[e]);
      m = mine_e == e ? r[e] : m;
    }
  }
  return m;
}
// the same for the chunk pair of rows 2m, 2m + 1 (c0 + c1 in both)
__device__ __forceinline__ float pair_sum(float v) {
  const auto pr = __builtin_amdgcn_permlane16_swap(__float_as_uint(v), __float_as_uint(v), false, false);
  return __uint_as_float(pr[0]) + __uint_as_float(pr[1]);
}
__device__ __forceinline__ void sum_pairs(float (&r)[kNE], const bool (&act)[kNE]) {
  if (act[0] && act[1] && act[2] && act[3]) {
#pragma unroll
    for (int e = 0; e < kNE; ++e) r[e] = pair_sum(r[e]);
  } else {
#pragma unroll
    for (int e = 0; e < kNE; ++e)
      if (act[e]) r[e] = pair_sum(r[e]);
  }
}
// the lane-group sums of the four environments' partials; the one of env `mine_e`
template <int G>
__device__ __forceinline__ float sum_pick(float (&r)[kNE], int mine_e) {
  float m = 0.f;
#pragma unroll
  for (int e = 0; e < kNE; ++e) {
    r[e] = lane_sum<G>(r[e]);
    m = mine_e == e ? r[e] : m;
  }
  return m;
}

// pre-activations (and their exp) of the activations this lane owns
struct FwdKeep {
  float a1, z1, a2, z2;
};
__device__ __forceinline__ float softplus_keep(float a, float& z) {  // softplus (threshold 20), z = exp(a)
  z = expf(a);
  return a > 20.f ? a : log1pf(z);
}
__device__ __forceinline__ float softplus_grad(float g, float a, float z) {  // torch: g * z / (z + 1)
  return a > 20.f ? g : g * z / (z + 1.f);
}

}  // namespace
}  // namespace pgp
