// pgp_gobitrain.hip — training of GOBI's surrogate on the device: the
// reference's `python train.py energy_latency_16 train`
// (scheduler/BaGTI/train.py:69-94) over the energy_latency_16 model
// (scheduler/BaGTI/src/models.py:8-27: 288-128-128-64-2, Softplus, Softplus,
// Tanhshrink, Sigmoid; all fp32).
//
// gobi_train_steps_kernel: n sequential batch-1 steps of backprop
// (train.py:18-31) in one launch of ONE 1024-thread workgroup (16 waves, 4 per
// SIMD).  A step is
//   forward      4 dot-product phases, each weight row read coalesced by one
//                wave (layer 1 reads its whole rows: see gt_forward);
//   loss         sum((y - t)^2), train.py:13-16;
//   backward     the four deltas (d4, d3, d2, d1), with the weights as they
//                were before the step; layer 1 needs no input gradient;
//   Adam         torch.optim.Adam(lr, weight_decay) (train.py:53), i.e. L2
//                folded into the gradient.  A batch-1 weight gradient is the
//                rank-1 delta (x) activation, formed inside the update: the pass
//                reads p, m, v and writes p, m, v; there is no gradient buffer.
// The parameters and both moments (3 x 61,890 floats, 742 KB) fit neither the
// workgroup's LDS (160 KB) nor its registers, so they stay in global memory
// (L2-resident) and every step streams them once; the activations and deltas
// (with the bias-correction table, 17 KB) live in LDS.  A workgroup's waves
// share one CU and its vector L1, so the stores of one step are visible to the
// loads of the next after the workgroup barrier; nothing synchronises across
// workgroups.
// Every sum has a fixed order (lane butterflies, then fixed chunk order), no
// atomics: the same inputs give the same bits, and n launches of one step equal
// one launch of n steps.  The bias corrections of step k = step0 + i + 1 come
// from double-precision powers, 1024 steps at a time into an LDS table, each
// from k alone (so they do not depend on where a launch starts).
// Elementwise semantics follow torch's CPU kernels (softplus threshold 20,
// tanhshrink = x - tanh x composite, sigmoid backward g(1-y)y, Adam's
// single-tensor op order).
//
// gobi_train_eval_kernel: accuracy()'s per-sample loss (train.py:33-42), one
// workgroup per sample, the same forward.
//
// gobi_train_steps_many_kernel / gobi_train_eval_many_kernel: the same step
// loop / loss for M surrogates in one launch (the reference keeps one dataset
// and checkpoint per environment, scheduler/GOBI.py:11-17): one workgroup per
// model / per (sample, model) pair, each on its own slot of P, m, v and its own
// job (pgp_gobi_job, read from a device table).  The workgroups share nothing
// they write, so a model's bits are those of the single kernels.
#include <hip/hip_runtime.h>

#include <cmath>

#include "../../include/preganplus.h"
#include "pgp_device.hpp"

namespace pgp {
namespace {

constexpr int kGtT = 1024;     // threads of the workgroup
constexpr int kGtTab = 1024;   // steps per refill of the bias-correction table

// the surrogate for H hosts: the first layer's width is the only H-dependent
// size (the reference defines energy_latency_16 alone; another host count is
// another instantiation)
template <int H>
struct GtGeo {
  static constexpr int F = H + 2, IN = H * F, N1 = 128, N2 = 128, N3 = 64, NO = 2;
  // state-dict order (pgp_gobi_weight_len): find.0.weight [N1][IN], find.0.bias, find.2.weight [N2][N1], ...
  static constexpr int W1 = 0, B1 = W1 + N1 * IN, W2 = B1 + N1, B2 = W2 + N2 * N1, W3 = B2 + N2,
                       B3 = W3 + N3 * N2, W4 = B3 + N3, B4 = W4 + NO * N3, SIZE = B4 + NO;
  static_assert(kGtT == 16 * 64 && N1 % 16 == 0 && N1 == 128 && N2 == 128 && N3 == 64, "thread roles");
  static_assert(IN <= kGtT, "one thread per input element");
};

template <int H>
struct GtLds {
  using G = GtGeo<H>;
  float x[G::IN];
  float a1[G::N1], h1[G::N1], a2[G::N2], h2[G::N2], th3[G::N3], h3[G::N3];
  float d1[G::N1], d2[G::N2], d3[G::N3], d4[G::NO];
  float red[8][128];        // the backward's chunk partials
  float tab[kGtTab][2];     // per step: lr / (1 - beta1^k), sqrt(1 - beta2^k)
};

struct GtAdam {  // the step's scalars as torch casts them to the tensors' fp32
  float wd, omb1, b2, omb2, eps, step_size, bc2s;
};

__device__ __forceinline__ float gt_softplus(float a) { return a > 20.f ? a : log1pf(expf(a)); }
__device__ __forceinline__ float gt_softplus_grad(float g, float a) {  // torch: g * z / (z + 1), z = exp(a)
  const float z = expf(a);
  return a > 20.f ? g : g * z / (z + 1.f);
}
__device__ __forceinline__ float gt_sigmoid(float x) { return 1.f / (1.f + expf(-x)); }

// sum over N aligned adjacent lanes, the same bits in all of them (xor butterfly, fixed order)
template <int N>
__device__ __forceinline__ float gt_lane_sum(float v) {
#pragma unroll
  for (int s = 1; s < N; s <<= 1) v += __shfl_xor(v, s);
  return v;
}

// Forward of the surrogate on L.x (all kGtT threads): leaves a1, h1, a2, h2,
// th3, h3 in LDS and returns the two outputs in every lane of wave 0 (other
// waves: unspecified).  The caller synchronises L.x before and the LDS results
// after.
template <int H>
__device__ __forceinline__ void gt_forward(const float* P, GtLds<H>& L, float& y0, float& y1) {
  using G = GtGeo<H>;
  const int t = threadIdx.x, w = t >> 6;
  int l = t & 63;
  asm volatile("" : "+v"(l));  // opaque per call: keeps the rows' addresses out of the step loop's invariants
  // Layers 1-3: wave w owns N / 16 consecutive outputs; for each, lane l
  // multiplies inputs l, l + 64, ... (coalesced weight rows, every load
  // independent), then the 64 lanes' partials are summed by the butterfly.
  // Layer 1 reads its whole rows: a zero input adds an exact zero, and the
  // Adam pass streams the same rows through L2 in any case.
  {
    constexpr int R = (G::IN + 63) / 64, Q = G::N1 / 16;
    float xr[R], acc[Q];
#pragma unroll
    for (int r = 0; r < R; ++r) xr[r] = l + 64 * r < G::IN ? L.x[l + 64 * r] : 0.f;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const float* wr = P + G::W1 + (w * Q + q) * G::IN;
      float a = 0.f;
#pragma unroll
      for (int r = 0; r < R; ++r)
        if (l + 64 * r < G::IN) a = fmaf(wr[l + 64 * r], xr[r], a);
      acc[q] = a;
    }
    float mine = 0.f;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      acc[q] = gt_lane_sum<64>(acc[q]);
      mine = l == q ? acc[q] : mine;
    }
    if (l < Q) {
      const int o = w * Q + l;
      const float a = mine + P[G::B1 + o];
      L.a1[o] = a;
      L.h1[o] = gt_softplus(a);
    }
  }
  __syncthreads();
  {
    constexpr int Q = G::N2 / 16;
    const float h0 = L.h1[l], h1 = L.h1[l + 64];
    float mine = 0.f;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const float* wr = P + G::W2 + (w * Q + q) * G::N1;
      const float a = gt_lane_sum<64>(fmaf(wr[l + 64], h1, wr[l] * h0));
      mine = l == q ? a : mine;
    }
    if (l < Q) {
      const int o = w * Q + l;
      const float a = mine + P[G::B2 + o];
      L.a2[o] = a;
      L.h2[o] = gt_softplus(a);
    }
  }
  __syncthreads();
  {  // Tanhshrink
    constexpr int Q = G::N3 / 16;
    const float h0 = L.h2[l], h1 = L.h2[l + 64];
    float mine = 0.f;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      const float* wr = P + G::W3 + (w * Q + q) * G::N2;
      const float a = gt_lane_sum<64>(fmaf(wr[l + 64], h1, wr[l] * h0));
      mine = l == q ? a : mine;
    }
    if (l < Q) {
      const int o = w * Q + l;
      const float a = mine + P[G::B3 + o];
      const float th = tanhf(a);
      L.th3[o] = th;
      L.h3[o] = a - th;
    }
  }
  __syncthreads();
  y0 = y1 = 0.f;
  if (t < 64) {  // the head: wave 0, lane = k; Sigmoid
    const float h = L.h3[t];
    const float p0 = gt_lane_sum<64>(P[G::W4 + t] * h), p1 = gt_lane_sum<64>(P[G::W4 + G::N3 + t] * h);
    y0 = gt_sigmoid(p0 + P[G::B4]);
    y1 = gt_sigmoid(p1 + P[G::B4 + 1]);
  }
}

// torch.optim.Adam's single-tensor step on one element (weight_decay as L2):
//   g += wd p; m.lerp_(g, 1 - beta1); v = v beta2 + (1 - beta2) g g;
//   denom = sqrt(v) / sqrt(1 - beta2^k) + eps; p += -(lr / (1 - beta1^k)) m / denom
__device__ __forceinline__ void gt_adam_regs(float& p, float& m, float& v, float g, const GtAdam& A) {
#pragma clang fp contract(off)  // torch's separate multiplies and adds
  g = g + A.wd * p;
  m = m + A.omb1 * (g - m);
  v = v * A.b2 + A.omb2 * g * g;
  const float denom = sqrtf(v) / A.bc2s + A.eps;
  p = p + (-A.step_size) * m / denom;
}
__device__ __forceinline__ void gt_adam(float* p_, float* m_, float* v_, float g, const GtAdam& A) {
  float p = *p_, m = *m_, v = *v_;
  gt_adam_regs(p, m, v, g, A);
  *p_ = p;
  *m_ = m;
  *v_ = v;
}
// the update over CNT consecutive elements, element q's gradient from grad(q):
// U elements per thread at a time, their 3 U loads issued before the first
// store (P, M and V may alias as far as the compiler knows, so a load after a
// store would wait for it).  A wave takes U * 64 consecutive elements, lane l
// the elements l, l + 64, ...: coalesced, and one address per array with the
// others as immediate offsets (256 u bytes)
template <int U, int CNT, class GradFn>
__device__ __forceinline__ void gt_adam_span(float* P, float* M, float* V, const GtAdam& A, GradFn grad) {
  static_assert(CNT % (U * kGtT) == 0, "whole groups");
  int first = (threadIdx.x >> 6) * (U * 64) + (threadIdx.x & 63);
  // opaque per call: otherwise every element's row / column index (loop-invariant over the steps) is
  // hoisted out of the step loop and the hundred of them spill
  asm volatile("" : "+v"(first));
#pragma unroll 1
  for (int q0 = first; q0 < CNT; q0 += U * kGtT) {
    float p[U], m[U], v[U];
#pragma unroll
    for (int u = 0; u < U; ++u) {
      p[u] = P[q0 + u * 64];
      m[u] = M[q0 + u * 64];
      v[u] = V[q0 + u * 64];
    }
#pragma unroll
    for (int u = 0; u < U; ++u) gt_adam_regs(p[u], m[u], v[u], grad(q0 + u * 64), A);
#pragma unroll
    for (int u = 0; u < U; ++u) {
      P[q0 + u * 64] = p[u];
      M[q0 + u * 64] = m[u];
      V[q0 + u * 64] = v[u];
    }
  }
}

// the step loop of one surrogate: all kGtT threads of the workgroup, n steps on
// P / M / V over the samples order[0..n) of feats / targets [N]
template <int H>
__device__ __forceinline__ void gt_steps(GtLds<H>& L, int N, int n, const float* __restrict__ feats,
                                         const float* __restrict__ targets, const int* __restrict__ order, float* P,
                                         float* M, float* V, long long step0, const GobiTrainHyper& hy,
                                         float* __restrict__ loss) {
  using G = GtGeo<H>;
  const int tid = threadIdx.x;
  GtAdam A;
  A.wd = (float)hy.wd;
  A.omb1 = (float)(1.0 - hy.beta1);
  A.b2 = (float)hy.beta2;
  A.omb2 = (float)(1.0 - hy.beta2);
  A.eps = (float)hy.eps;
  for (int i = 0; i < n; ++i) {
    int t = tid;
    asm volatile("" : "+v"(t));  // opaque per step: the roles' indices are recomputed, not kept (and spilled)
    if ((i & (kGtTab - 1)) == 0) {  // the next kGtTab steps' bias corrections, each from its k alone
      __syncthreads();
      if (i + t < n) {
        const double k = (double)(step0 + i + t + 1);  // in double, as torch computes them
        L.tab[t][0] = (float)(hy.lr / (1.0 - pow(hy.beta1, k)));
        L.tab[t][1] = (float)sqrt(1.0 - pow(hy.beta2, k));
      }
    }
    const int s = order[i];
    if (s < 0 || s >= N) {  // not a sample: no step, and a loss nobody can mistake for one
      if (t == 0) loss[i] = __builtin_nanf("");
      continue;
    }
    if (t < G::IN) L.x[t] = feats[(long)s * G::IN + t];
    __syncthreads();
    float y0, y1;
    gt_forward<H>(P, L, y0, y1);
    if (t < 64) {  // loss, and the deltas of the head and of layer 3 (wave 0, lane = layer 3's output)
      const float e0 = y0 - targets[2 * (long)s], e1 = y1 - targets[2 * (long)s + 1];
      const float g0 = 2.f * e0 * (1.f - y0) * y0, g1 = 2.f * e1 * (1.f - y1) * y1;
      const float gh = P[G::W4 + t] * g0 + P[G::W4 + G::N3 + t] * g1;
      const float th = L.th3[t];
      L.d3[t] = gh - gh * (1.f - th * th);
      if (t == 0) {
        loss[i] = e0 * e0 + e1 * e1;
        L.d4[0] = g0;
        L.d4[1] = g1;
      }
    }
    __syncthreads();
    {  // d2 = (W3^T d3) through Softplus: column k = t % 128, rows 8c .. 8c + 7 of chunk c = t / 128
      const int k = t & 127, c = t >> 7;
      float acc = 0.f;
#pragma unroll
      for (int o = 0; o < 8; ++o) acc = fmaf(P[G::W3 + (c * 8 + o) * G::N2 + k], L.d3[c * 8 + o], acc);
      L.red[c][k] = acc;
    }
    __syncthreads();
    if (t < G::N2) {
      const float g = ((L.red[0][t] + L.red[1][t]) + (L.red[2][t] + L.red[3][t])) +
                      ((L.red[4][t] + L.red[5][t]) + (L.red[6][t] + L.red[7][t]));
      L.d2[t] = gt_softplus_grad(g, L.a2[t]);
    }
    __syncthreads();
    {  // d1 = (W2^T d2) through Softplus: column k, rows 16c .. 16c + 15
      const int k = t & 127, c = t >> 7;
      float acc = 0.f;
#pragma unroll
      for (int o = 0; o < 16; ++o) acc = fmaf(P[G::W2 + (c * 16 + o) * G::N1 + k], L.d2[c * 16 + o], acc);
      L.red[c][k] = acc;
    }
    __syncthreads();
    if (t < G::N1) {
      const float g = ((L.red[0][t] + L.red[1][t]) + (L.red[2][t] + L.red[3][t])) +
                      ((L.red[4][t] + L.red[5][t]) + (L.red[6][t] + L.red[7][t]));
      L.d1[t] = gt_softplus_grad(g, L.a1[t]);
    }
    __syncthreads();
    // ---- Adam over every parameter, the rank-1 gradient formed on the fly ----
    A.step_size = L.tab[i & (kGtTab - 1)][0];
    A.bc2s = L.tab[i & (kGtTab - 1)][1];
    gt_adam_span<9, G::N1 * G::IN>(P + G::W1, M + G::W1, V + G::W1, A,
                                   [&](int q) { return L.d1[q / G::IN] * L.x[q % G::IN]; });
    gt_adam_span<8, G::N2 * G::N1>(P + G::W2, M + G::W2, V + G::W2, A,
                                   [&](int q) { return L.d2[q / G::N1] * L.h1[q % G::N1]; });
    gt_adam_span<8, G::N3 * G::N2>(P + G::W3, M + G::W3, V + G::W3, A,
                                   [&](int q) { return L.d3[q / G::N2] * L.h2[q % G::N2]; });
    // the small tensors, one per group of waves: find.0.bias | find.2.bias | find.4.bias, find.6.weight | find.6.bias
    if (t < G::N1) {
      gt_adam(P + G::B1 + t, M + G::B1 + t, V + G::B1 + t, L.d1[t], A);
    } else if (t < 256) {
      const int q = t - 128;
      gt_adam(P + G::B2 + q, M + G::B2 + q, V + G::B2 + q, L.d2[q], A);
    } else if (t < 320) {
      const int q = t - 256;
      gt_adam(P + G::B3 + q, M + G::B3 + q, V + G::B3 + q, L.d3[q], A);
    } else if (t < 448) {
      const int q = t - 320;
      gt_adam(P + G::W4 + q, M + G::W4 + q, V + G::W4 + q, L.d4[q / G::N3] * L.h3[q % G::N3], A);
    } else if (t < 448 + G::NO) {
      const int q = t - 448;
      gt_adam(P + G::B4 + q, M + G::B4 + q, V + G::B4 + q, L.d4[q], A);
    }
    __syncthreads();  // the next step reads the updated P and overwrites L.x
  }
}

template <int H>
__global__ __launch_bounds__(kGtT) void gobi_train_steps_kernel(int N, int n, const float* __restrict__ feats,
                                                                const float* __restrict__ targets,
                                                                const int* __restrict__ order, float* P, float* M,
                                                                float* V, long long step0, GobiTrainHyper hy,
                                                                float* __restrict__ loss) {
  __shared__ GtLds<H> L;
  gt_steps<H>(L, N, n, feats, targets, order, P, M, V, step0, hy, loss);
}

// M surrogates in one launch: workgroup b runs job b's step loop on slot b of
// P / M / V (GtGeo::SIZE floats apart), its own sample range of the pools and
// its own scalars.  The workgroups share nothing they write, so there is no
// synchronisation between them and any number of them may queue.
template <int H>
__global__ __launch_bounds__(kGtT) void gobi_train_steps_many_kernel(const pgp_gobi_job* __restrict__ jobs,
                                                                     const float* __restrict__ feats,
                                                                     const float* __restrict__ targets,
                                                                     const int* __restrict__ order, float* P, float* M,
                                                                     float* V, float* __restrict__ loss) {
  using G = GtGeo<H>;
  __shared__ GtLds<H> L;
  const pgp_gobi_job j = jobs[blockIdx.x];
  if (j.n <= 0) return;
  const GobiTrainHyper hy{j.lr, j.weight_decay, j.beta1, j.beta2, j.eps};
  const size_t slot = (size_t)blockIdx.x * G::SIZE;
  gt_steps<H>(L, j.n_samples, j.n, feats + j.sample_off * G::IN, targets + j.sample_off * 2, order + j.order_off,
              P + slot, M + slot, V + slot, j.step0, hy, loss + j.order_off);
}

// accuracy()'s loss of sample order[i] under P into loss[i] (all kGtT threads)
template <int H>
__device__ __forceinline__ void gt_eval(GtLds<H>& L, int N, int i, const float* __restrict__ feats,
                                        const float* __restrict__ targets, const int* __restrict__ order,
                                        const float* __restrict__ P, float* __restrict__ loss) {
  using G = GtGeo<H>;
  const int t = threadIdx.x;
  const int s = order[i];
  if (s < 0 || s >= N) {
    if (t == 0) loss[i] = __builtin_nanf("");
    return;
  }
  if (t < G::IN) L.x[t] = feats[(long)s * G::IN + t];
  __syncthreads();
  float y0, y1;
  gt_forward<H>(P, L, y0, y1);
  if (t == 0) {
    const float e0 = y0 - targets[2 * (long)s], e1 = y1 - targets[2 * (long)s + 1];
    loss[i] = e0 * e0 + e1 * e1;
  }
}

template <int H>
__global__ __launch_bounds__(kGtT) void gobi_train_eval_kernel(int N, const float* __restrict__ feats,
                                                               const float* __restrict__ targets,
                                                               const int* __restrict__ order,
                                                               const float* __restrict__ P,
                                                               float* __restrict__ loss) {
  __shared__ GtLds<H> L;
  gt_eval<H>(L, N, blockIdx.x, feats, targets, order, P, loss);
}

// workgroup (i, b): sample i of job model0 + b under that model's slot; a job
// shorter than the grid's width leaves its spare workgroups idle
template <int H>
__global__ __launch_bounds__(kGtT) void gobi_train_eval_many_kernel(const pgp_gobi_job* __restrict__ jobs, int model0,
                                                                    const float* __restrict__ feats,
                                                                    const float* __restrict__ targets,
                                                                    const int* __restrict__ order,
                                                                    const float* __restrict__ P,
                                                                    float* __restrict__ loss) {
  using G = GtGeo<H>;
  __shared__ GtLds<H> L;
  const int mdl = model0 + blockIdx.y;
  const pgp_gobi_job j = jobs[mdl];
  if ((int)blockIdx.x >= j.n) return;
  gt_eval<H>(L, j.n_samples, blockIdx.x, feats + j.sample_off * G::IN, targets + j.sample_off * 2,
             order + j.order_off, P + (size_t)mdl * G::SIZE, loss + j.order_off);
}

}  // namespace

bool gobi_train_supported(int H) { return H == 16; }

hipError_t launch_gobi_train_steps(int n_hosts, int n_samples, int n, const float* feats, const float* targets,
                                   const int* order, float* P, float* m, float* v, long long step0,
                                   const GobiTrainHyper& hy, float* loss, hipStream_t st) {
  if (n_hosts != 16) return hipErrorInvalidValue;
  static_assert(GtGeo<16>::SIZE == 61890, "pgp_gobi_weight_len(16)");
  gobi_train_steps_kernel<16><<<1, kGtT, 0, st>>>(n_samples, n, feats, targets, order, P, m, v, step0, hy, loss);
  return hipGetLastError();
}

hipError_t launch_gobi_train_eval(int n_hosts, int n_samples, int n, const float* feats, const float* targets,
                                  const int* order, const float* P, float* loss, hipStream_t st) {
  if (n_hosts != 16) return hipErrorInvalidValue;
  gobi_train_eval_kernel<16><<<n, kGtT, 0, st>>>(n_samples, feats, targets, order, P, loss);
  return hipGetLastError();
}

hipError_t launch_gobi_train_steps_many(int n_hosts, int n_models, const pgp_gobi_job* jobs_dev, const float* feats,
                                        const float* targets, const int* order, float* P, float* m, float* v,
                                        float* loss, hipStream_t st) {
  if (n_hosts != 16) return hipErrorInvalidValue;
  gobi_train_steps_many_kernel<16><<<n_models, kGtT, 0, st>>>(jobs_dev, feats, targets, order, P, m, v, loss);
  return hipGetLastError();
}

hipError_t launch_gobi_train_eval_many(int n_hosts, int n_models, int max_n, const pgp_gobi_job* jobs_dev,
                                       const float* feats, const float* targets, const int* order, const float* P,
                                       float* loss, hipStream_t st) {
  if (n_hosts != 16) return hipErrorInvalidValue;
  constexpr int kMaxY = 65535;  // the grid's y limit: more models take more launches
  for (int m0 = 0; m0 < n_models; m0 += kMaxY) {
    const int my = n_models - m0 < kMaxY ? n_models - m0 : kMaxY;
    gobi_train_eval_many_kernel<16><<<dim3(max_n, my), kGtT, 0, st>>>(jobs_dev, m0, feats, targets, order, P, loss);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

}  // namespace pgp
