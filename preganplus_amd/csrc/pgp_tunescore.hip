// pgp_tunescore.hip — accuracy()'s scores of every cell of a fleet
// (recovery/PreGANSrc/src/train.py:60-109: anomaly_accuracy, class_accuracy and
// accuracy's accumulation over the windows), from the fp64 logits / protos
// pgp_tune_forward_cells wrote and the cell's prototypes after its last tuning
// step.  The literal restatement of train.accuracy_scores (and of
// train.accuracy_scores_many, its form over a leading cell axis): fp64, the
// reference's operation order, FMA contraction off, correctly rounded
// divisions — every score has the bits the host function gives.
//
// One 64-lane workgroup per cell (cells on grid x; more cells than the device
// holds at once queue).  Lane h < H is host h of the current window; the
// per-window counts are integers (ballots and a butterfly sum), every lane
// then runs the same fp64 accumulation over the windows in order and lane 0
// writes.  An inactive cell returns before it reads or writes anything of its
// slot; the slots are disjoint, no workgroup waits for another.
#include "pgp_tunescore.hpp"

namespace pgp {
namespace {

constexpr int kScoreLanes = 64;

__global__ __launch_bounds__(kScoreLanes) void tune_scores_cells_kernel(
    int H, int K, int n, const int* __restrict__ active, const double* __restrict__ logits64,
    const double* __restrict__ protos64, const int* __restrict__ y, const int* __restrict__ cls,
    const double* __restrict__ state, double* __restrict__ scores, int* __restrict__ flag) {
#pragma clang fp contract(off)
  const long b = blockIdx.x;
  if (active && !active[b]) return;
  const int lane = threadIdx.x;
  const bool host = lane < H;
  const double* P = state + b * (2 * K + 3);  // prototypes 0-2 lead the slot
  const double P00 = P[0], P01 = P[1], P10 = P[2], P11 = P[3], P20 = P[4], P21 = P[5];
  const long base = b * (long)n * H;
  double anomaly_correct = 0.0, class_correct = 0.0, class_total = 0.0;
  for (int w = 0; w < n; ++w) {
    bool ok = false, positive = false, hit = false;
    int yi = 0;
    if (host) {
      const long i = base + (long)w * H + lane;
      const double l0 = logits64[2 * i], l1 = logits64[2 * i + 1];
      const double p0 = protos64[2 * i], p1 = protos64[2 * i + 1];
      yi = y[i];
      const int res = l1 > l0 ? 1 : 0;  // torch.argmax, ties -> 0
      ok = res == yi;
      // MSE over the 2 dims, numpy's mean: one add, one divide
      const double d0 = ((p0 - P00) * (p0 - P00) + (p1 - P01) * (p1 - P01)) / 2.0;
      const double d1 = ((p0 - P10) * (p0 - P10) + (p1 - P11) * (p1 - P11)) / 2.0;
      const double d2 = ((p0 - P20) * (p0 - P20) + (p1 - P21) * (p1 - P21)) / 2.0;
      const int ci = cls[i];
      const int c = ci < 0 ? 0 : (ci > 2 ? 2 : ci);
      const double pos = c == 0 ? d0 : (c == 1 ? d1 : d2);
      const double n0 = c == 0 ? d1 : d0, n1 = c == 2 ? d1 : d2;  // negatives in class order
      positive = yi > 0;
      hit = positive && pos <= n0 && pos <= n1;
    }
    const int correct = __popcll(__ballot(ok));
    const int npos = __popcll(__ballot(positive));
    const int hits = __popcll(__ballot(hit));
    int ysum = yi;  // sum(y): lanes >= H hold 0
    for (int o = kScoreLanes / 2; o > 0; o >>= 1) ysum += __shfl_xor(ysum, o, kScoreLanes);
    anomaly_correct += (double)correct / (double)H;
    if (ysum > 0) {
      class_total += 1.0;
      double total = 1e-4;
      for (int k = 0; k < npos; ++k) total += 1.0;
      class_correct += (double)hits / total;
    }
  }
  if (lane == 0) {
    scores[2 * b] = anomaly_correct / (double)n;
    if (class_total == 0.0) {
      flag[b] = 1;  // train.py:109 divides by zero here; scores[b][1] stays unwritten
    } else {
      flag[b] = 0;
      scores[2 * b + 1] = class_correct / class_total;
    }
  }
}

}  // namespace

hipError_t launch_tune_scores_cells(int H, int K, int n_cells, int n, const int* active, const double* logits64,
                                    const double* protos64, const int* y, const int* cls, const double* state,
                                    double* scores, int* flag, hipStream_t st) {
  if (n_cells <= 0 || n <= 0) return hipSuccess;
  if (H < 1 || H > kScoreLanes || K < 3) return hipErrorInvalidValue;  // one lane per host, prototypes 0-2
  tune_scores_cells_kernel<<<n_cells, kScoreLanes, 0, st>>>(H, K, n, active, logits64, protos64, y, cls, state,
                                                           scores, flag);
  return hipGetLastError();
}

}  // namespace pgp
