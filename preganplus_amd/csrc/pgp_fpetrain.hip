// pgp_fpetrain.hip — offline training of PreGAN's FPE_16 encoder
// (PreGAN.py:26-27, 39-49: a new FPE is trained for num_epochs when no
// checkpoint exists; train.py:42-57 backprop, sequential batch-1 steps),
// compiled for H = 16 hosts and for H = 50 (FPE_16's architecture with its
// constants set for 50 hosts, as K4's 50-host forward: the reference's FPE_50
// class cannot run).
//
// fpe_step_kernel<H, TRAIN>: ONE window per workgroup (256 threads), the whole step:
//   forward of FPE_16 (models.py:65-115) from the natural fp32 master P —
//     GRU(3H -> 3) over the 3 window rows from the given h0 (the reference
//     draws it with torch.randn inside encode, models.py:70; the host draws it
//     the same way and passes it in), GAT on each row (H nodes, graph-wise
//     edge softmax, node mean), concat, MultiheadAttention(H + 3, 1 head) over
//     the 3 rows, encoder Linear(3(H + 3) -> 10H) (LeakyReLU(True) = identity),
//     per host Softmax(Linear(10, 2)) and Sigmoid(Linear(10, 2));
//   custom_loss / triplet_loss bookkeeping of the window on the device state
//     (pgp_tunetargets.hpp, fp64, the reference's order; the anomaly decoder
//     ends in a Softmax, so CrossEntropyLoss sees probabilities);
//   the backward of aloss + tloss into G (every element written).
// The TRAIN = false instantiation stops after the forward and writes the
// window's probabilities / prototypes (fp64), one workgroup per window:
// accuracy()'s forwards (train.py:94-109) after an epoch.  It holds none of
// the backward's LDS.
// The model is tiny (11,401 parameters at 16 hosts, 93,137 at 50): every phase
// is a few hundred independent dot products over LDS-resident activations, so
// one workgroup per step is latency-bound by construction; the step count
// (windows x epochs) is what the offline training costs.
//
// H = 16 keeps one thread per item and its summation orders.  At H = 50 the
// `if constexpr (H > 16)` forms replace what does not scale:
//   - the H^2 edge arrays (softmax, its gradient) and the dz array are not
//     kept: an edge weight is exp(lrelu(s_i + t_j) - max) / sum and is
//     recomputed where the backward needs it, d a_ij does not depend on j, and
//     dz is consumed as it is produced.  LDS stays static (z is the one large
//     array, 30.6 KB);
//   - reductions over the H nodes of a row run on one wave per row, and long
//     dot products (the GRU input gates, the encoder Linear, the attn_fc / fc
//     gradients) on 16 lanes per output with lanes striding the terms, both
//     reduced by a shuffle butterfly: a fixed order, the same bits every run;
//   - every one-thread-per-item phase with more than 256 items is a strided
//     loop (for_items picks the form from the item count); the others are
//     covered by the static_asserts in the kernel.
//
// The kernel also has a cell-indexed form (template parameter CELLS, above the kernel): a
// model's whole step loop with its AdamW in one workgroup, one workgroup per model of a fleet
// (TRAIN), and the forwards of many models in one launch.
//
// GATE (pgp_fpe_forward1 / pgp_fpe_forward1_many, instantiated in pgp_fpe1_cells.hip): the
// forward above for one window per cell, each cell on its own slot of P, continued in the same
// workgroup by PreGANRecovery.run_model's rest of the interval's forward (PreGAN.py:105-126):
// detect / embed / get_classes on the cell's prototypes and Gen_16 / Disc_16 on [emb; sched]
// from the cell's training master (see FpeGateArgs).
#include <hip/hip_runtime.h>

#include <type_traits>

#include "../../include/preganplus.h"
#include "pgp_device.hpp"
#include "pgp_gemm.hpp"
#include "pgp_train.hpp"
#include "pgp_tunetargets.hpp"

namespace pgp {
namespace {

// natural parameter blob (state_dict order, weights.fpe_shapes)
template <int H_>
struct FP {
  static constexpr int H = H_, F = 3 * H, W = 3, G3 = 9, E = H + 3, L = 10, D = H, Q = 3 * E, NL = H * L, NF = W * E;
  static constexpr int IH = 0, HH = IH + G3 * F, BIH = HH + G3 * 3, BHH = BIH + G3, FC = BHH + G3, ATT = FC + D * 3,
                       IN = ATT + 2 * D, INB = IN + Q * E, OUT = INB + Q, OUTB = OUT + E * E, ENC = OUTB + E,
                       ENCB = ENC + NL * NF, AN = ENCB + NL, ANB = AN + 2 * L, PR = ANB + 2, PRB = PR + 2 * L,
                       SIZE = PRB + 2;
};
static_assert(FP<16>::SIZE == 11401, "FPE_16 parameter count");
static_assert(FP<50>::SIZE == 93137, "FPE_16 at 50 hosts: parameter count");

constexpr int kFT = 256;
constexpr int kSub = 16;  // lanes per output of a long dot product (H > 16)

__device__ __forceinline__ float sigm(float x) { return 1.f / (1.f + expf(-x)); }

// Butterfly reductions (H > 16): every lane of the wave calls them and gets the
// result; the order of the additions is fixed, so a step repeats bit for bit.
__device__ __forceinline__ float sub_sum(float v) {  // over the kSub lanes of a thread's group
#pragma unroll
  for (int m = kSub / 2; m > 0; m >>= 1) v += __shfl_xor(v, m, kSub);
  return v;
}
__device__ __forceinline__ float wave_sum(float v) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v += __shfl_xor(v, m, 64);
  return v;
}
__device__ __forceinline__ float wave_max(float v) {
#pragma unroll
  for (int m = 32; m > 0; m >>= 1) v = fmaxf(v, __shfl_xor(v, m, 64));
  return v;
}

// N items over the workgroup: one thread per item where they fit (every such phase at 16
// hosts), a strided loop where they do not
template <int N, class F>
__device__ __forceinline__ void for_items(int t, F f) {
  if constexpr (N <= kFT) {
    if (t < N) f(t);
  } else {
    for (int k = t; k < N; k += kFT) f(k);
  }
}

// CELLS (pgp_fpe_train_steps / pgp_fpe_train_steps_many / pgp_fpe_forward_many_cells): the
// cell-indexed form, instantiated and launched from pgp_fpetrain_cells.hip.
//   TRAIN: workgroup m is model m.  It runs job m's n steps in sequence on slot m of P / G /
//     the moments (FP<H>::SIZE floats apart) and on state row m: each step is the step below on
//     window row window_off + i with h0 / loss row step_off + i, then the AdamW of that step
//     over the slot (adamw_elem_slot, the code pgp_adamw_table_d runs) from row step_off + i of
//     the table adam.sched [steps][ntensors][3].  The parameters are rewritten by the kernel
//     that reads them, and G is read back by the update: both are plain pointers here, so
//     every parameter read is a vector load that the barriers order against the update's
//     stores (a scalar load would go through a cache those stores do not update).  A job
//     without steps returns before the first barrier; the workgroups share nothing they
//     write and never wait for one another, so any number of them queue on grid x.
//   forward: workgroup (i, y) is window i of job model0 + y under that model's slot of P; a
//     job shorter than the grid's width leaves its spare workgroups idle.
struct FpeCellArgs {
  const pgp_fpe_job* jobs;  // [models] on the device; nullptr: the one job `one` on slot 0
  pgp_fpe_job one;
  int model0;               // forward: the launch's first model (models on grid y)
  AdamArgs adam;            // TRAIN: param / grad / m / v name slot 0, sched the pool's first row
};
// GATE (pgp_fpe_forward1 / pgp_fpe_forward1_many): workgroup b is cell b.  The forward runs on
// window b / h0 row b under slot b of P (FP<H>::SIZE floats apart), then, after its last barrier,
//   detect / embed / get_classes (PreGAN.py:110-120) with K4's conventions: host h is anomalous iff
//     an[h][1] > an[h][0], its embedding row is pr[h] where anomalous and zero otherwise, cls[h] the first
//     argmin over the K prototypes (fp64, read as float) of the mean squared distance, -1 for a zero row;
//   Gen_16 / Disc_16 on [emb; sched] from the gen / disc sections of slot b of the training master
//     (TGeo<H>::ALL floats apart), infer1_kernel's arithmetic and lane mapping (pgp_tune1.hip) in four
//     passes of 256 threads: 16 lanes per output of the two 64-output layers, 4 per output of Gen's
//     second layer, DPP xor butterflies; the gate and both argmax targets.
// The GAN part always runs, so every output is defined.  An inactive cell leaves before the first barrier.
struct FpeGateArgs {
  const int* active;     // [cells] or nullptr (all)
  const float* sched;    // [cells][H][H]
  const float* master;   // [cells][TGeo<H>::ALL]
  const double* protos;  // [cells][proto_stride], the first 2K doubles of a row
  long long proto_stride;
  float* scores;         // [cells][H][2] anomaly softmax
  float* protos_out;     // [cells][H][2]
  int* cls;              // [cells][H]
  int* any_anom;         // [cells]
  float* probs;          // [cells][2]
  int* keep;             // [cells]
  int* final_t;          // [cells][H]
  int* gen_t;            // [cells][H]
};
template <bool CELLS, bool GATE>
using FpeCell = std::conditional_t<GATE, FpeGateArgs, std::conditional_t<CELLS, FpeCellArgs, int>>;
template <bool LOOP>
using FpeParam = std::conditional_t<LOOP, float*, const float* __restrict__>;
template <bool LOOP>
using FpeGrad = std::conditional_t<LOOP, float*, float* __restrict__>;

// The looped form at 16 hosts asks for two waves per SIMD (two workgroups per CU: 256 VGPRs, 7 of them spilled
// in the prologue); at 50 hosts that spills inside the step, so it keeps one.  The other forms: as before.
template <int H_, bool TRAIN, bool CELLS = false, bool GATE = false>
__global__ __launch_bounds__(kFT, TRAIN && CELLS && H_ <= 16 ? 2 : 1)
void fpe_step_kernel(int K, const float* __restrict__ wins, const float* __restrict__ h0s,
                     const int* __restrict__ ys, const int* __restrict__ clss, FpeParam<TRAIN && CELLS> Pk,
                     FpeGrad<TRAIN && CELLS> Gk, double* __restrict__ state, double update_min, double decay,
                     double* __restrict__ loss, double* __restrict__ probs_out, double* __restrict__ protos_out,
                     FpeCell<CELLS, GATE> cell) {
  static_assert(!GATE || (!TRAIN && !CELLS && H_ == 16), "the gated forward: 16 hosts, forward only");
  using C = FP<H_>;
  constexpr int H = C::H, W = C::W, E = C::E, D = C::D, L = C::L;
  constexpr bool kWide = H > 16;         // the 50-host forms
  constexpr int HA = kWide ? 1 : H;      // the H^2 edge arrays and dz are kept at 16 hosts only
  static_assert(H <= 64 && W <= kFT / 64, "one 64-lane wave (gfx950) reduces the H nodes of a row");
  static_assert(W * H <= kFT && W * D + W * 3 <= kFT && 4 * H <= kFT, "one thread per item");
  static_assert(64 + W * E <= kFT && C::Q <= kFT && C::NF <= kFT && 3 * D <= kFT, "one thread per item");
  const int t = threadIdx.x;
  // window (forward-only launches: one per window; training: 0, the looped form moves the row pointers)
  const int b = TRAIN && CELLS ? 0 : blockIdx.x;
  const int wv = t >> 6, ln = t & 63;    // wave and lane (kWide: wave w reduces row w)
  const int sg = t / kSub, sl = t % kSub;  // group of kSub lanes and lane in it (kWide: one output per group)
  __shared__ float x[W][C::F];
  __shared__ float hs[W + 1][3];           // GRU states h_0 .. h_3
  __shared__ float gi[W][9], gh[W][9], gr[W][3], gz[W][3], gn[W][3];
  __shared__ float z[W][H][D + 1];         // GAT fc outputs
  __shared__ float sv[W][H], tv[W][H];     // attention halves a1.z_i, a2.z_j
  __shared__ float al[W][HA][HA + 1];      // edge softmax
  __shared__ float red[W][H];
  __shared__ float mx[W], sm[W];
  __shared__ float c[W][E];                // concat
  __shared__ float qkv[W][C::Q];
  __shared__ float pa[W][W];               // attention probabilities
  __shared__ float ao[W][E];               // attention output before out_proj
  __shared__ float fl[C::NF];              // out_proj output, flattened
  __shared__ float lat[C::NL];
  __shared__ float pr[H][2], an[H][2];     // prototypes (sigmoid), anomaly probs
  // backward (no use in the TRAIN = false instantiation: not allocated there)
  __shared__ float mult[H], tgt[H][2];
  __shared__ double lsum[2];
  __shared__ float dan[H][2], dpr[H][2];
  __shared__ float dlat[C::NL];
  __shared__ float dfl[C::NF];
  __shared__ float dao[W][E], dP[W][W], dS[W][W];
  __shared__ float dqkv[W][C::Q];
  __shared__ float dc[W][E];
  __shared__ float dh[W + 1][3];
  __shared__ float dgi[W][9], dgh[W][9];
  __shared__ float dz[W][HA][HA + 1];
  __shared__ float dal[W][HA][HA + 1];
  __shared__ float dsv[W][H], dtv[W][H];
  __shared__ float dav[W][H], ss[W];       // kWide: d a_ij (the same for every j), sum over edges of a . da

  [[maybe_unused]] int steps_left = 1;
  [[maybe_unused]] long slot = 0;
  [[maybe_unused]] const float* sched = nullptr;
  if constexpr (CELLS) {  // the job's rows of the pools and the model's slot
    const long mdl = TRAIN ? (long)blockIdx.x : (long)cell.model0 + blockIdx.y;
    const pgp_fpe_job j = cell.jobs ? cell.jobs[mdl] : cell.one;
    if (TRAIN ? j.n <= 0 : (int)blockIdx.x >= j.n) return;  // uniform over the workgroup, ahead of every barrier
    wins += j.window_off * (W * C::F);
    h0s += j.step_off * 3;
    slot = mdl * C::SIZE;
    if constexpr (TRAIN) {
      steps_left = j.n;
      ys += j.window_off * H;
      clss += j.window_off * H;
      state += mdl * (2 * K + 3);
      loss += j.step_off * 2;
      sched = cell.adam.sched + j.step_off * (3 * cell.adam.ntensors);
    } else {
      probs_out += j.step_off * (2 * H);
      protos_out += j.step_off * (2 * H);
    }
  }
  if constexpr (GATE) {  // the cell's slot; an inactive cell touches nothing
    if (cell.active && !cell.active[blockIdx.x]) return;  // uniform over the workgroup, ahead of every barrier
    slot = (long)blockIdx.x * C::SIZE;
  }
[[maybe_unused]] next_step:  // TRAIN && CELLS: the job's following steps re-enter here, the row pointers moved on
  // P / G: the model's slot of the kernel's Pk / Gk (the lone forms: slot 0, Pk / Gk themselves).  The step loop
  // would let the compiler hoist every per-thread address of P and G out of it (256 VGPRs and 124-190 AGPRs of
  // parked addresses): an offset it cannot see through keeps that arithmetic inside the step.
  [[maybe_unused]] long base = slot;
  if constexpr (TRAIN && CELLS) asm volatile("" : "+v"(base));
  const auto P = Pk + base;
  const auto G = Gk + base;
  const float* win = wins + (long)b * W * C::F;
  for (int k = t; k < W * C::F; k += kFT) x[k / C::F][k % C::F] = win[k];
  if (t < 3) hs[0][t] = h0s[(long)b * 3 + t];
  __syncthreads();

  // ---- GRU (torch gate order r, z, n), one row at a time ----
  if constexpr (kWide) {  // the input gates of all rows ahead of the recurrence, kSub lanes per gate
    for (int base = 0; base < W * 9; base += kFT / kSub) {
      const int o = base + sg, w = o / 9, g = o % 9;
      float a = 0.f;
      if (o < W * 9)
        for (int k = sl; k < C::F; k += kSub) a = fmaf(P[C::IH + g * C::F + k], x[w][k], a);
      a = sub_sum(a);
      if (o < W * 9 && sl == 0) gi[w][g] = P[C::BIH + g] + a;
    }
    __syncthreads();
  }
  for (int w = 0; w < W; ++w) {
    if (t < 9) {
      if constexpr (!kWide) {
        float a = P[C::BIH + t];
        for (int k = 0; k < C::F; ++k) a = fmaf(P[C::IH + t * C::F + k], x[w][k], a);
        gi[w][t] = a;
      }
    } else if (t < 18) {
      const int o = t - 9;
      float a = P[C::BHH + o];
      for (int k = 0; k < 3; ++k) a = fmaf(P[C::HH + o * 3 + k], hs[w][k], a);
      gh[w][o] = a;
    }
    __syncthreads();
    if (t < 3) {
      const float r = sigm(gi[w][t] + gh[w][t]);
      const float zz = sigm(gi[w][3 + t] + gh[w][3 + t]);
      const float n = tanhf(gi[w][6 + t] + r * gh[w][6 + t]);
      gr[w][t] = r;
      gz[w][t] = zz;
      gn[w][t] = n;
      hs[w + 1][t] = (1.f - zz) * n + zz * hs[w][t];
    }
    __syncthreads();
  }

  // ---- GAT on every row (dlutils.py:304-348), node mean ----
  for (int k = t; k < W * H * D; k += kFT) {  // z = fc x
    const int w = k / (H * D), i = (k / D) % H, d = k % D;
    const float* fc = P + C::FC + d * 3;
    z[w][i][d] = fc[0] * x[w][3 * i] + fc[1] * x[w][3 * i + 1] + fc[2] * x[w][3 * i + 2];
  }
  __syncthreads();
  for_items<2 * W * H>(t, [&](int k) {
    const int half = k / (W * H), w = (k / H) % W, i = k % H;
    const float* a = P + C::ATT + half * D;
    float s = 0.f;
    for (int d = 0; d < D; ++d) s = fmaf(a[d], z[w][i][d], s);
    (half ? tv : sv)[w][i] = s;
  });
  __syncthreads();
  if constexpr (kWide) {
    // softmax over all H^2 edges of the row's graph without keeping them.  lrelu and the
    // sum s_i + t_j are monotone, so the largest edge is lrelu(max s + max t) exactly.
    if (wv < W) {
      const float a = wave_max(ln < H ? sv[wv][ln] : -INFINITY), c2 = wave_max(ln < H ? tv[wv][ln] : -INFINITY);
      const float e = a + c2;
      if (ln == 0) mx[wv] = e > 0.f ? e : 0.01f * e;
    }
    __syncthreads();
    if (t < W * H) {  // sum_j exp(e_ij - max) of source i
      const int w = t / H, i = t % H;
      float s = 0.f;
      for (int j = 0; j < H; ++j) {
        const float e = sv[w][i] + tv[w][j];
        s += expf((e > 0.f ? e : 0.01f * e) - mx[w]);
      }
      red[w][i] = s;
    }
    __syncthreads();
    if (wv < W) {
      const float s = wave_sum(ln < H ? red[wv][ln] : 0.f);
      if (ln == 0) sm[wv] = s;
    }
    __syncthreads();
    if (t < W * H) red[t / H][t % H] /= sm[t / H];  // column weight of source i: sum_j a_ij
    __syncthreads();
  } else {
    for (int k = t; k < W * H * H; k += kFT) {  // e_ij = lrelu(a1.z_i + a2.z_j), src i -> dst j
      const int w = k / (H * H), i = (k / H) % H, j = k % H;
      const float e = sv[w][i] + tv[w][j];
      al[w][i][j] = e > 0.f ? e : 0.01f * e;
    }
    __syncthreads();
    if (t < W * H) {  // softmax over all H^2 edges of the row's graph: max, then sum
      const int w = t / H, i = t % H;
      float m = -INFINITY;
      for (int j = 0; j < H; ++j) m = fmaxf(m, al[w][i][j]);
      red[w][i] = m;
    }
    __syncthreads();
    if (t < W) {
      float m = -INFINITY;
      for (int i = 0; i < H; ++i) m = fmaxf(m, red[t][i]);
      mx[t] = m;
    }
    __syncthreads();
    for (int k = t; k < W * H * H; k += kFT) {
      const int w = k / (H * H), i = (k / H) % H, j = k % H;
      al[w][i][j] = expf(al[w][i][j] - mx[w]);
    }
    __syncthreads();
    if (t < W * H) {
      const int w = t / H, i = t % H;
      float s = 0.f;
      for (int j = 0; j < H; ++j) s += al[w][i][j];
      red[w][i] = s;
    }
    __syncthreads();
    if (t < W) {
      float s = 0.f;
      for (int i = 0; i < H; ++i) s += red[t][i];
      sm[t] = s;
    }
    __syncthreads();
    for (int k = t; k < W * H * H; k += kFT) {
      const int w = k / (H * H), i = (k / H) % H, j = k % H;
      al[w][i][j] = al[w][i][j] / sm[w];
    }
    __syncthreads();
    if (t < W * H) {  // column weight of source i: sum_j a_ij
      const int w = t / H, i = t % H;
      float s = 0.f;
      for (int j = 0; j < H; ++j) s += al[w][i][j];
      red[w][i] = s;
    }
    __syncthreads();
  }
  if (t < W * D) {  // gat_w[d] = mean_j sum_i a_ij z_i[d] = (1/H) sum_i red_i z_i[d]
    const int w = t / D, d = t % D;
    float s = 0.f;
    for (int i = 0; i < H; ++i) s = fmaf(red[w][i], z[w][i][d], s);
    c[w][3 + d] = s / (float)H;
  } else if (t < W * D + W * 3) {
    const int k = t - W * D, w = k / 3, o = k % 3;
    c[w][o] = hs[w + 1][o];
  }
  __syncthreads();

  // ---- MultiheadAttention(E, 1 head) over the 3 rows ----
  for (int k = t; k < W * C::Q; k += kFT) {
    const int w = k / C::Q, o = k % C::Q;
    float a = P[C::INB + o];
    for (int e = 0; e < E; ++e) a = fmaf(P[C::IN + o * E + e], c[w][e], a);
    qkv[w][o] = a;
  }
  __syncthreads();
  const float isq = 1.0f / sqrtf((float)E);
  if (t < W * W) {
    const int w = t / W, v = t % W;
    float s = 0.f;
    for (int e = 0; e < E; ++e) s = fmaf(qkv[w][e], qkv[v][E + e], s);
    pa[w][v] = s * isq;
  }
  __syncthreads();
  if (t < W) {
    const float m = fmaxf(pa[t][0], fmaxf(pa[t][1], pa[t][2]));
    const float e0 = expf(pa[t][0] - m), e1 = expf(pa[t][1] - m), e2 = expf(pa[t][2] - m);
    const float s = e0 + e1 + e2;
    pa[t][0] = e0 / s;
    pa[t][1] = e1 / s;
    pa[t][2] = e2 / s;
  }
  __syncthreads();
  if (t < W * E) {
    const int w = t / E, e = t % E;
    ao[w][e] = pa[w][0] * qkv[0][2 * E + e] + pa[w][1] * qkv[1][2 * E + e] + pa[w][2] * qkv[2][2 * E + e];
  }
  __syncthreads();
  if (t < W * E) {
    const int w = t / E, o = t % E;
    float a = P[C::OUTB + o];
    for (int e = 0; e < E; ++e) a = fmaf(P[C::OUT + o * E + e], ao[w][e], a);
    fl[w * E + o] = a;
  }
  __syncthreads();
  // ---- encoder Linear(3E -> 10H) ----
  if constexpr (kWide) {  // kSub lanes per output row, striding k: the row is read in 64-byte pieces
    for (int base = 0; base < C::NL; base += kFT / kSub) {
      const int r = base + sg;
      float a = 0.f;
      if (r < C::NL)
        for (int k = sl; k < C::NF; k += kSub) a = fmaf(P[C::ENC + r * C::NF + k], fl[k], a);
      a = sub_sum(a);
      if (r < C::NL && sl == 0) lat[r] = P[C::ENCB + r] + a;
    }
  } else {
    if (t < C::NL) {
      float a = P[C::ENCB + t];
      for (int k = 0; k < C::NF; ++k) a = fmaf(P[C::ENC + t * C::NF + k], fl[k], a);
      lat[t] = a;
    }
  }
  __syncthreads();
  // ---- per-host decoders ----
  if (t < 4 * H) {
    const int h = t >> 2, which = (t >> 1) & 1, o = t & 1;
    const float* Wd = P + (which ? C::PR : C::AN) + o * L;
    float a = P[(which ? C::PRB : C::ANB) + o];
    for (int l = 0; l < L; ++l) a = fmaf(Wd[l], lat[h * L + l], a);
    (which ? pr : an)[h][o] = a;
  }
  __syncthreads();
  if (t < H) {
    const float a0 = an[t][0], a1 = an[t][1], m = fmaxf(a0, a1);
    const float e0 = expf(a0 - m), e1 = expf(a1 - m);
    an[t][0] = e0 / (e0 + e1);
    an[t][1] = e1 / (e0 + e1);
    pr[t][0] = sigm(pr[t][0]);
    pr[t][1] = sigm(pr[t][1]);
  }
  __syncthreads();
  if constexpr (GATE) {
    using TG = TGeo<H>;
    constexpr int H2 = H * H, GIN = TG::GIN, DIN = TG::DIN;
    static_assert(H <= kFT && 64 % (kFT / 16) == 0 && (4 * H2) % kFT == 0 && DIN % 16 == 0, "whole passes");
    __shared__ float xin[GIN];  // Gen input [emb; s]
    __shared__ float sd[DIN];   // Disc input [s; ns]
    __shared__ float hg[64], hd[64];
    __shared__ int anyf;
    const long cb = blockIdx.x;
    const float* __restrict__ sch = cell.sched + cb * H2;
    const float* __restrict__ Gp = cell.master + cb * TG::ALL + TG::OFF_GEN;
    const float* __restrict__ Dp = cell.master + cb * TG::ALL + TG::OFF_DISC;
    const double* __restrict__ pk = cell.protos + cb * cell.proto_stride;
    if (t == 0) anyf = 0;
    __syncthreads();
    if (t < 2 * H) {
      cell.scores[cb * 2 * H + t] = an[t >> 1][t & 1];
      cell.protos_out[cb * 2 * H + t] = pr[t >> 1][t & 1];
    }
    if (t < H) {  // detect + embed + get_classes
      const float l0 = an[t][0], l1 = an[t][1];
      const bool anom = l1 > l0;  // torch.argmax: ties -> index 0
      const float e0 = anom ? pr[t][0] : 0.f, e1 = anom ? pr[t][1] : 0.f;
      int cl = -1;
      if (!(e0 == 0.f && e1 == 0.f)) {
        float best = INFINITY;
        for (int k = 0; k < K; ++k) {
          const float d0 = e0 - (float)pk[2 * k], d1 = e1 - (float)pk[2 * k + 1];
          const float dist = (d0 * d0 + d1 * d1) * 0.5f;  // torch.mean over PROTO_DIM = 2
          if (dist < best) {                              // np.argmin: first minimum
            best = dist;
            cl = k;
          }
        }
      }
      cell.cls[cb * H + t] = cl;
      xin[2 * t] = e0;
      xin[2 * t + 1] = e1;
      if (anom) anyf = 1;  // every writer stores 1
    }
    for (int i = t; i < H2; i += kFT) {
      xin[2 * H + i] = sch[i];
      sd[i] = sch[i];
    }
    __syncthreads();
    // Gen1: 64 outputs, 16 lanes each (k-chunks), xor-butterfly sum; LeakyReLU(True) = identity
    for (int o = t >> 4; o < 64; o += kFT / 16) {
      const int sp = t & 15;
      constexpr int KC = (GIN + 15) / 16;
      float acc = 0.f;
      for (int k = sp * KC; k < sp * KC + KC && k < GIN; ++k) acc = fmaf(Gp[TG::G_W1 + o * GIN + k], xin[k], acc);
      acc = xadd<8>(xadd<4>(xadd<2>(xadd<1>(acc))));
      if (sp == 0) hg[o] = acc + Gp[TG::G_B1 + o];
    }
    __syncthreads();
    // Gen2: H^2 outputs, 4 lanes each: ns = s + 4 tanh(W2 hg + b2)
    for (int i = t; i < 4 * H2; i += kFT) {
      const int o = i >> 2, sp = i & 3;
      float acc = 0.f;
#pragma unroll
      for (int k = 0; k < 16; ++k) acc = fmaf(Gp[TG::G_W2 + o * 64 + sp * 16 + k], hg[sp * 16 + k], acc);
      acc = xadd<2>(xadd<1>(acc));
      if (sp == 0) sd[H2 + o] = xin[2 * H + o] + 4.0f * tanhf(acc + Gp[TG::G_B2 + o]);
    }
    __syncthreads();
    // Disc1: 64 outputs over [s; ns], 16 lanes each
    for (int o = t >> 4; o < 64; o += kFT / 16) {
      const int sp = t & 15;
      constexpr int KC = DIN / 16;
      float acc = 0.f;
      for (int k = sp * KC; k < sp * KC + KC; ++k) acc = fmaf(Dp[TG::D_W1 + o * DIN + k], sd[k], acc);
      acc = xadd<8>(xadd<4>(xadd<2>(xadd<1>(acc))));
      if (sp == 0) hd[o] = acc + Dp[TG::D_B1 + o];
    }
    __syncthreads();
    if (t < 64) {  // Disc2 + softmax + gate (PreGAN.py:74-76), one wave
      float z0 = Dp[TG::D_W2 + ln] * hd[ln], z1 = Dp[TG::D_W2 + 64 + ln] * hd[ln];
      z0 = pgp::wave_sum(z0);  // xor 32 .. 1 (pgp_gemm.hpp)
      z1 = pgp::wave_sum(z1);
      z0 += Dp[TG::D_B2];
      z1 += Dp[TG::D_B2 + 1];
      const float m = fmaxf(z0, z1), e0 = expf(z0 - m), e1 = expf(z1 - m), inv = 1.0f / (e0 + e1);
      if (ln == 0) {
        cell.probs[cb * 2] = e0 * inv;
        cell.probs[cb * 2 + 1] = e1 * inv;
        cell.keep[cb] = e0 * inv > e1 * inv ? 1 : 0;
        cell.any_anom[cb] = anyf;
      }
    } else if (t < 64 + H) {  // first argmax of each schedule row (original / generated)
      const int c2 = t - 64;
      float bs = -INFINITY, bn = -INFINITY;
      int is = 0, in = 0;
      for (int h = 0; h < H; ++h) {
        const float v = sd[c2 * H + h], w = sd[H2 + c2 * H + h];
        if (v > bs) {
          bs = v;
          is = h;
        }
        if (w > bn) {
          bn = w;
          in = h;
        }
      }
      cell.final_t[cb * H + c2] = is;
      cell.gen_t[cb * H + c2] = in;
    }
    return;
  } else if constexpr (!TRAIN) {
    if (t < 2 * H) {
      probs_out[(long)b * 2 * H + t] = (double)an[t >> 1][t & 1];
      protos_out[(long)b * 2 * H + t] = (double)pr[t >> 1][t & 1];
    }
    return;
  }

  // ---- custom_loss / triplet_loss bookkeeping (fp64, sequential, one lane) ----
  if (t == 0) {
    double ls[2];
    tune_targets_one(H, K, &an[0][0], &pr[0][0], ys, clss, state, update_min, decay, mult, &tgt[0][0], ls);
    lsum[0] = ls[0];
    lsum[1] = ls[1];
    loss[0] = ls[0];
    loss[1] = ls[1];
  }
  __syncthreads();

  // ---- loss gradients at the decoder outputs ----
  if (t < H) {
    // aloss: mult * CrossEntropy(probs as logits, y): d/dp = mult (softmax(p) - e_y);
    // through the decoder's Softmax: da = p (dp - p . dp)
    const int y = ys[t];
    const float p0 = an[t][0], p1 = an[t][1], m = fmaxf(p0, p1);
    const float e0 = expf(p0 - m), e1 = expf(p1 - m);
    const float q0 = e0 / (e0 + e1), q1 = e1 / (e0 + e1);
    const float dp0 = mult[t] * (q0 - (y == 0 ? 1.f : 0.f)), dp1 = mult[t] * (q1 - (y == 1 ? 1.f : 0.f));
    const float s = p0 * dp0 + p1 * dp1;
    dan[t][0] = p0 * (dp0 - s);
    dan[t][1] = p1 * (dp1 - s);
    // tloss: MSE(anchor, P[c]) over 2 values (negatives are constants): d = (a - P[c]); through the Sigmoid
    const bool pos = y > 0;
    const float a0 = pr[t][0], a1 = pr[t][1];
    dpr[t][0] = pos ? (a0 - tgt[t][0]) * a0 * (1.f - a0) : 0.f;
    dpr[t][1] = pos ? (a1 - tgt[t][1]) * a1 * (1.f - a1) : 0.f;
  }
  __syncthreads();
  // decoder weight gradients (sum over hosts) and d latent
  if (t < 2 * 2 * (L + 1)) {
    const int which = t / (2 * (L + 1)), o = (t / (L + 1)) % 2, l = t % (L + 1);
    float s = 0.f;
    for (int h = 0; h < H; ++h) {
      const float d = which ? dpr[h][o] : dan[h][o];
      s = fmaf(d, l < L ? lat[h * L + l] : 1.f, s);
    }
    if (l < L)
      G[(which ? C::PR : C::AN) + o * L + l] = s;
    else
      G[(which ? C::PRB : C::ANB) + o] = s;
  }
  for_items<C::NL>(t, [&](int k) {
    const int h = k / L, l = k % L;
    dlat[k] = P[C::AN + l] * dan[h][0] + P[C::AN + L + l] * dan[h][1] + P[C::PR + l] * dpr[h][0] +
              P[C::PR + L + l] * dpr[h][1];
  });
  __syncthreads();
  // encoder
  for (int k = t; k < C::NL * C::NF; k += kFT) G[C::ENC + k] = dlat[k / C::NF] * fl[k % C::NF];
  for_items<C::NL>(t, [&](int k) { G[C::ENCB + k] = dlat[k]; });
  if (t < C::NF) {
    float s = 0.f;
    for (int r = 0; r < C::NL; ++r) s = fmaf(P[C::ENC + r * C::NF + t], dlat[r], s);
    dfl[t] = s;
  }
  __syncthreads();
  // out_proj: d ao = Wo^T d out; dWo = sum_w d out_w ao_w^T
  for (int k = t; k < E * E; k += kFT) {
    const int o = k / E, e = k % E;
    G[C::OUT + k] = dfl[o] * ao[0][e] + dfl[E + o] * ao[1][e] + dfl[2 * E + o] * ao[2][e];
  }
  if (t < E) G[C::OUTB + t] = dfl[t] + dfl[E + t] + dfl[2 * E + t];
  if (t < W * E) {
    const int w = t / E, e = t % E;
    float s = 0.f;
    for (int o = 0; o < E; ++o) s = fmaf(P[C::OUT + o * E + e], dfl[w * E + o], s);
    dao[w][e] = s;
  }
  __syncthreads();
  // attention: dP[w][v] = dao_w . v_v; dv_v = sum_w P[w][v] dao_w
  if (t < W * W) {
    const int w = t / W, v = t % W;
    float s = 0.f;
    for (int e = 0; e < E; ++e) s = fmaf(dao[w][e], qkv[v][2 * E + e], s);
    dP[w][v] = s;
  }
  if (t >= 64 && t < 64 + W * E) {
    const int k = t - 64, v = k / E, e = k % E;
    dqkv[v][2 * E + e] = pa[0][v] * dao[0][e] + pa[1][v] * dao[1][e] + pa[2][v] * dao[2][e];
  }
  __syncthreads();
  if (t < W) {  // softmax backward per query row, then the 1/sqrt(E) scale
    const float s = pa[t][0] * dP[t][0] + pa[t][1] * dP[t][1] + pa[t][2] * dP[t][2];
    for (int v = 0; v < W; ++v) dS[t][v] = pa[t][v] * (dP[t][v] - s) * isq;
  }
  __syncthreads();
  for_items<2 * W * E>(t, [&](int k) {  // dq_w = sum_v dS[w][v] k_v; dk_v = sum_w dS[w][v] q_w
    const int part = k / (W * E), w = (k / E) % W, e = k % E;
    if (part == 0)
      dqkv[w][e] = dS[w][0] * qkv[0][E + e] + dS[w][1] * qkv[1][E + e] + dS[w][2] * qkv[2][E + e];
    else
      dqkv[w][E + e] = dS[0][w] * qkv[0][e] + dS[1][w] * qkv[1][e] + dS[2][w] * qkv[2][e];
  });
  __syncthreads();
  // in_proj: dWin = sum_w dqkv_w c_w^T, dc_w = Win^T dqkv_w
  for (int k = t; k < C::Q * E; k += kFT) {
    const int o = k / E, e = k % E;
    G[C::IN + k] = dqkv[0][o] * c[0][e] + dqkv[1][o] * c[1][e] + dqkv[2][o] * c[2][e];
  }
  if (t < C::Q) G[C::INB + t] = dqkv[0][t] + dqkv[1][t] + dqkv[2][t];
  if (t >= 64 && t < 64 + W * E) {
    const int k = t - 64, w = k / E, e = k % E;
    float s = 0.f;
    for (int o = 0; o < C::Q; ++o) s = fmaf(P[C::IN + o * E + e], dqkv[w][o], s);
    dc[w][e] = s;
  }
  __syncthreads();

  // ---- GRU backward through the rows (h0 gets no gradient) ----
  if (t < 3) dh[W][t] = 0.f;
  __syncthreads();
  for (int w = W - 1; w >= 0; --w) {
    if (t < 3) {
      const float d = dh[w + 1][t] + dc[w][t];   // grad of h_{w+1}
      const float r = gr[w][t], zz = gz[w][t], n = gn[w][t];
      const float dn = d * (1.f - zz), dzz = d * (hs[w][t] - n);
      const float dan_ = dn * (1.f - n * n);
      const float dr = dan_ * gh[w][6 + t];
      const float dar = dr * r * (1.f - r), daz = dzz * zz * (1.f - zz);
      dgi[w][t] = dar;
      dgi[w][3 + t] = daz;
      dgi[w][6 + t] = dan_;
      dgh[w][t] = dar;
      dgh[w][3 + t] = daz;
      dgh[w][6 + t] = dan_ * r;
      dh[w][t] = d * zz;   // + Whh^T dgh below
    }
    __syncthreads();
    if (t < 3) {
      float s = dh[w][t];
      for (int o = 0; o < 9; ++o) s = fmaf(P[C::HH + o * 3 + t], dgh[w][o], s);
      dh[w][t] = s;
    }
    __syncthreads();
  }
  for (int k = t; k < 9 * C::F; k += kFT) {
    const int o = k / C::F, f = k % C::F;
    G[C::IH + k] = dgi[0][o] * x[0][f] + dgi[1][o] * x[1][f] + dgi[2][o] * x[2][f];
  }
  if (t < 27) {
    const int o = t / 3, k = t % 3;
    G[C::HH + t] = dgh[0][o] * hs[0][k] + dgh[1][o] * hs[1][k] + dgh[2][o] * hs[2][k];
  } else if (t >= 32 && t < 41) {
    const int o = t - 32;
    G[C::BIH + o] = dgi[0][o] + dgi[1][o] + dgi[2][o];
    G[C::BHH + o] = dgh[0][o] + dgh[1][o] + dgh[2][o];
  }

  // ---- GAT backward: gat_w = (1/H) sum_i (sum_j a_ij) z_i ----
  // d a_ij = (1/H) z_i . dgat_w; d z_i = (1/H)(sum_j a_ij) dgat_w (+ the score terms)
  if constexpr (kWide) {
    if (t < W * H) {
      const int w = t / H, i = t % H;
      float s = 0.f;
      for (int d = 0; d < D; ++d) s = fmaf(z[w][i][d], dc[w][3 + d], s);
      dav[w][i] = s / (float)H;
    }
    __syncthreads();
    if (wv < W) {  // sum over edges of a . da = sum_i (sum_j a_ij) da_i
      const float s = wave_sum(ln < H ? red[wv][ln] * dav[wv][ln] : 0.f);
      if (ln == 0) ss[wv] = s;
    }
    __syncthreads();
    // softmax backward, the LeakyReLU, and d s_i = sum_j de_ij | d t_j = sum_i de_ij, the edge
    // weights recomputed as the forward made them
    for (int k = t; k < 2 * W * H; k += kFT) {
      const int half = k / (W * H), w = (k / H) % W, n = k % H;
      const float m = mx[w], inv = 1.f / sm[w], sw = ss[w];
      float s = 0.f;
      for (int q = 0; q < H; ++q) {
        const int i = half ? q : n, j = half ? n : q;
        const float e = sv[w][i] + tv[w][j];
        const float de = expf((e > 0.f ? e : 0.01f * e) - m) * inv * (dav[w][i] - sw);
        s += e > 0.f ? de : 0.01f * de;
      }
      (half ? dtv : dsv)[w][n] = s;
    }
    __syncthreads();
    // attn_fc: sum over rows and nodes of (d s_i) z_i | (d t_j) z_j; fc: of dz_i x_i^T with
    // dz_i = (1/H)(sum_j a_ij) dgat_w + (d s_i) a1 + (d t_i) a2 made in place; kSub lanes per output
    for (int base = 0; base < 2 * D + 3 * D; base += kFT / kSub) {
      const int o = base + sg;
      float s = 0.f;
      if (o < 2 * D) {
        const int half = o / D, d = o % D;
        for (int n = sl; n < W * H; n += kSub) {
          const int w = n / H, i = n % H;
          s = fmaf(half ? dtv[w][i] : dsv[w][i], z[w][i][d], s);
        }
      } else if (o < 5 * D) {
        const int d = (o - 2 * D) / 3, f = (o - 2 * D) % 3;
        const float a1 = P[C::ATT + d], a2 = P[C::ATT + D + d];
        for (int n = sl; n < W * H; n += kSub) {
          const int w = n / H, i = n % H;
          const float dzv = red[w][i] / (float)H * dc[w][3 + d] + dsv[w][i] * a1 + dtv[w][i] * a2;
          s = fmaf(dzv, x[w][3 * i + f], s);
        }
      }
      s = sub_sum(s);
      if (o < 5 * D && sl == 0) G[(o < 2 * D ? C::ATT : C::FC - 2 * D) + o] = s;
    }
  } else {
    for (int k = t; k < W * H * H; k += kFT) {
      const int w = k / (H * H), i = (k / H) % H, j = k % H;
      float s = 0.f;
      for (int d = 0; d < D; ++d) s = fmaf(z[w][i][d], dc[w][3 + d], s);
      dal[w][i][j] = s / (float)H;   // independent of j
    }
    __syncthreads();
    if (t < W) {  // sum over edges of a . da
      float s = 0.f;
      for (int i = 0; i < H; ++i)
        for (int j = 0; j < H; ++j) s = fmaf(al[t][i][j], dal[t][i][j], s);
      sm[t] = s;
    }
    __syncthreads();
    for (int k = t; k < W * H * H; k += kFT) {  // softmax backward, then the LeakyReLU
      const int w = k / (H * H), i = (k / H) % H, j = k % H;
      const float de = al[w][i][j] * (dal[w][i][j] - sm[w]);
      const float e = sv[w][i] + tv[w][j];
      dal[w][i][j] = e > 0.f ? de : 0.01f * de;
    }
    __syncthreads();
    if (t < 2 * W * H) {  // d s_i = sum_j de_ij, d t_j = sum_i de_ij
      const int half = t / (W * H), w = (t / H) % W, i = t % H;
      float s = 0.f;
      for (int k = 0; k < H; ++k) s += half ? dal[w][k][i] : dal[w][i][k];
      (half ? dtv : dsv)[w][i] = s;
    }
    __syncthreads();
    for (int k = t; k < W * H * D; k += kFT) {
      const int w = k / (H * D), i = (k / D) % H, d = k % D;
      dz[w][i][d] = red[w][i] / (float)H * dc[w][3 + d] + dsv[w][i] * P[C::ATT + d] + dtv[w][i] * P[C::ATT + D + d];
    }
    if (t < 2 * D) {  // attn_fc: sum over rows and nodes of (d s_i) z_i | (d t_j) z_j
      const int half = t / D, d = t % D;
      float s = 0.f;
      for (int w = 0; w < W; ++w)
        for (int i = 0; i < H; ++i) s = fmaf(half ? dtv[w][i] : dsv[w][i], z[w][i][d], s);
      G[C::ATT + t] = s;
    }
    __syncthreads();
    if (t < D * 3) {  // fc: sum over rows and nodes of dz_i x_i^T
      const int d = t / 3, f = t % 3;
      float s = 0.f;
      for (int w = 0; w < W; ++w)
        for (int i = 0; i < H; ++i) s = fmaf(dz[w][i][d], x[w][3 * i + f], s);
      G[C::FC + t] = s;
    }
  }

  if constexpr (TRAIN && CELLS) {
    __syncthreads();  // every element of this step's G is written (by other threads than those that read it now)
    // ---- torch.optim.AdamW.step of this step, from its row of the table ----
    const AdamArgs& a = cell.adam;
    for (int i = 0; i < a.ntensors; ++i) {
      const float* r = sched + 3 * i;
      if (r[0] == 0.f) continue;  // no gradient this step: P and both moments stay as they are
      const float step_size = r[1], bc2_sqrt = r[2];
      for (int o = t; o < a.t[i].n; o += kFT) adamw_elem_slot(a, slot, a.t[i].off + o, step_size, bc2_sqrt);
    }
    if (--steps_left > 0) {  // uniform over the workgroup
      wins += W * C::F;
      h0s += 3;
      ys += H;
      clss += H;
      loss += 2;
      sched += 3 * a.ntensors;
      __syncthreads();  // the next step reads the updated P and overwrites x
      goto next_step;
    }
  }
}

}  // namespace

// The cell-indexed instantiations and their launches live in a translation unit of their own
// (pgp_fpetrain_cells.hip includes this file with PGP_FPE_CELLS_TU), as pgp_gan1_cells.hip's: each
// unit instantiates one family only, and the four lone kernels are built as before.  The gated
// forward's likewise (pgp_fpe1_cells.hip, PGP_FPE_GATE_TU).
#if defined(PGP_FPE_GATE_TU)

// One workgroup per cell on grid x (no cap of its own); LDS is static.
hipError_t launch_fpe_gate_cells(int n_hosts, int K, int n_cells, const int* active, const float* wins,
                                 const float* h0s, const float* sched, const float* P, const float* master,
                                 const double* protos, long long proto_stride, float* scores, float* protos_out,
                                 int* cls, int* any_anom, float* probs, int* keep, int* final_t, int* gen_t,
                                 hipStream_t st) {
  if (n_hosts != 16) return hipErrorInvalidValue;
  if (n_cells <= 0) return hipSuccess;
  const FpeGateArgs g{active, sched,    master, protos, proto_stride, scores, protos_out,
                      cls,    any_anom, probs,  keep,   final_t,      gen_t};
  fpe_step_kernel<16, false, false, true><<<n_cells, kFT, 0, st>>>(K, wins, h0s, nullptr, nullptr, P, nullptr, nullptr,
                                                                   0.0, 0.0, nullptr, nullptr, nullptr, g);
  return hipGetLastError();
}

#elif !defined(PGP_FPE_CELLS_TU)

int fpe_param_count(int H) { return H == 16 ? FP<16>::SIZE : H == 50 ? FP<50>::SIZE : 0; }

// LDS is static in all four instantiations (below the 64 KB limit), so a launch needs no
// per-device function attribute.
hipError_t launch_fpe_step(int n_hosts, const float* win, const float* h0, const int* y, const int* cls,
                           const float* P, float* G, int K, double* state, double update_min, double decay,
                           double* loss, hipStream_t st) {
  if (n_hosts == 16)
    fpe_step_kernel<16, true><<<1, kFT, 0, st>>>(K, win, h0, y, cls, P, G, state, update_min, decay, loss, nullptr,
                                                 nullptr, 0);
  else if (n_hosts == 50)
    fpe_step_kernel<50, true><<<1, kFT, 0, st>>>(K, win, h0, y, cls, P, G, state, update_min, decay, loss, nullptr,
                                                 nullptr, 0);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

hipError_t launch_fpe_forward_many(int n_hosts, int n, const float* wins, const float* h0s, const float* P,
                                   double* probs, double* protos, hipStream_t st) {
  if (n_hosts == 16)
    fpe_step_kernel<16, false><<<n, kFT, 0, st>>>(3, wins, h0s, nullptr, nullptr, P, nullptr, nullptr, 0.0, 0.0,
                                                  nullptr, probs, protos, 0);
  else if (n_hosts == 50)
    fpe_step_kernel<50, false><<<n, kFT, 0, st>>>(3, wins, h0s, nullptr, nullptr, P, nullptr, nullptr, 0.0, 0.0,
                                                  nullptr, probs, protos, 0);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

#else  // PGP_FPE_CELLS_TU

// One workgroup per model on grid x (no cap of its own).  jobs_dev == nullptr: the one job `one` on slot 0
// (a names slot 0 of P / G / the moments and row 0 of the table pool).  LDS is static here too.
hipError_t launch_fpe_train_steps_cells(int n_hosts, int n_models, const pgp_fpe_job* jobs_dev, const pgp_fpe_job& one,
                                        const float* wins, const float* h0s, const int* ys, const int* clss, int K,
                                        double* state, double update_min, double decay, double* loss,
                                        const AdamArgs& a, hipStream_t st) {
  if (n_models <= 0) return hipSuccess;
  const FpeCellArgs cell{jobs_dev, one, 0, a};
  if (n_hosts == 16)
    fpe_step_kernel<16, true, true><<<n_models, kFT, 0, st>>>(K, wins, h0s, ys, clss, a.param, a.grad, state,
                                                              update_min, decay, loss, nullptr, nullptr, cell);
  else if (n_hosts == 50)
    fpe_step_kernel<50, true, true><<<n_models, kFT, 0, st>>>(K, wins, h0s, ys, clss, a.param, a.grad, state,
                                                              update_min, decay, loss, nullptr, nullptr, cell);
  else
    return hipErrorInvalidValue;
  return hipGetLastError();
}

// workgroup (i, m): window i of job m under slot m of P; max_n the longest job
hipError_t launch_fpe_forward_cells(int n_hosts, int n_models, int max_n, const pgp_fpe_job* jobs_dev,
                                    const float* wins, const float* h0s, const float* P, double* probs,
                                    double* protos, hipStream_t st) {
  if (n_hosts != 16 && n_hosts != 50) return hipErrorInvalidValue;
  constexpr int kMaxY = 65535;  // the grid's y limit: more models take more launches
  for (int m0 = 0; m0 < n_models; m0 += kMaxY) {
    const int my = n_models - m0 < kMaxY ? n_models - m0 : kMaxY;
    const FpeCellArgs cell{jobs_dev, pgp_fpe_job{}, m0, AdamArgs{}};
    if (n_hosts == 16)
      fpe_step_kernel<16, false, true><<<dim3(max_n, my), kFT, 0, st>>>(3, wins, h0s, nullptr, nullptr, P, nullptr,
                                                                        nullptr, 0.0, 0.0, nullptr, probs, protos, cell);
    else
      fpe_step_kernel<50, false, true><<<dim3(max_n, my), kFT, 0, st>>>(3, wins, h0s, nullptr, nullptr, P, nullptr,
                                                                        nullptr, 0.0, 0.0, nullptr, probs, protos, cell);
    const hipError_t e = hipGetLastError();
    if (e != hipSuccess) return e;
  }
  return hipSuccess;
}

#endif  // PGP_FPE_CELLS_TU

}  // namespace pgp
