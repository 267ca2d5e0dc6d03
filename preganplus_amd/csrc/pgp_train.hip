// pgp_train.hip — AdamW (utils.py:65: torch.optim.AdamW, single-tensor
// semantics) over the master weights of the online training steps.  The
// steps themselves: pgp_tune.hip (tuning step), pgp_gantrain.hip (GAN step).
#include <hip/hip_runtime.h>

#include "pgp_device.hpp"
#include "pgp_train.hpp"

namespace pgp {
namespace {

// AdamW (adamw_elem, pgp_train.hpp) over the tensors of a.t on a flat grid:
// tensor i owns blocks [g.bx0[i], g.bx0[i+1]), kAdamChunk elements each (a
// grid of one row per tensor sized by the largest dispatched ~1,000 idle
// workgroups per small tensor: 17-20 us per call for the tuning step's
// section).  Each element's update is independent, so the results are the
// same as any other order.
constexpr int kAdamChunk = 1024;
struct AdamGrid {
  int bx0[kMaxTensors + 1];
};
// the tensor that owns block bx: the last one whose first block is <= bx
__device__ __forceinline__ int block_tensor(const AdamGrid& g, int ntensors, int bx) {
  int lo = 0, hi = ntensors - 1;
  while (lo < hi) {
    const int mid = (lo + hi + 1) >> 1;
    if (bx >= g.bx0[mid]) lo = mid;
    else hi = mid - 1;
  }
  return lo;
}
__global__ __launch_bounds__(256) void adamw_kernel(AdamArgs a, AdamGrid g) {
  const int bx = blockIdx.x, lo = block_tensor(g, a.ntensors, bx);
  const AdamTensor& t = a.t[lo];
  float step_size = t.step_size, bc2_sqrt = t.bc2_sqrt;
  if (a.sched && (t.active & kAdamFromTable)) {  // per-step scalars from the device (graph-captured loops)
    const float* r = a.sched + 3 * lo;
    if (r[0] == 0.f) return;
    step_size = r[1];
    bc2_sqrt = r[2];
  } else if (!t.active) {
    return;
  }
  const long base = (long)(bx - g.bx0[lo]) * kAdamChunk;
#pragma unroll
  for (int k = 0; k < kAdamChunk / 256; ++k) {
    const long i = base + k * 256 + threadIdx.x;
    if (i < t.n) adamw_elem(a, t.off + i, step_size, bc2_sqrt);
  }
}

// The table-driven update for a fleet of cells (pgp_adamw_table_many): grid
// (blocks of one slot, cells).  Cell c = blockIdx.y updates slot c of the four
// buffers (slot_len floats each, offsets in 64 bits) with its own table row
// a.sched + c * sched_stride; an inactive cell leaves before it reads anything
// of its slot.  Per element the same adamw_update as adamw_kernel.
__global__ __launch_bounds__(256) void adamw_cells_kernel(AdamArgs a, AdamGrid g, const int* __restrict__ active,
                                                          long slot_len, long sched_stride) {
  const long c = blockIdx.y;
  if (active && !active[c]) return;
  const int bx = blockIdx.x, lo = block_tensor(g, a.ntensors, bx);
  const AdamTensor& t = a.t[lo];
  const float* r = a.sched + c * sched_stride + 3 * lo;
  if (r[0] == 0.f) return;
  const float step_size = r[1], bc2_sqrt = r[2];
  const long slot = c * slot_len, base = (long)(bx - g.bx0[lo]) * kAdamChunk;
#pragma unroll
  for (int k = 0; k < kAdamChunk / 256; ++k) {
    const long i = base + k * 256 + threadIdx.x;
    if (i < t.n) adamw_elem_slot(a, slot, t.off + i, step_size, bc2_sqrt);
  }
}

}  // namespace

// ---------------------------------------------------------------------------
// host launchers
// ---------------------------------------------------------------------------
static int adam_grid(const AdamArgs& a, AdamGrid* g) {  // fills g->bx0, returns the grid's blocks
  int nb = 0;
  for (int i = 0; i < a.ntensors; ++i) {
    g->bx0[i] = nb;
    nb += (int)((a.t[i].n + kAdamChunk - 1) / kAdamChunk);
  }
  return g->bx0[a.ntensors] = nb;
}

hipError_t launch_adamw(const AdamArgs& a, hipStream_t st) {
  AdamGrid g{};
  const int nb = adam_grid(a, &g);
  if (nb == 0) return hipSuccess;
  adamw_kernel<<<nb, 256, 0, st>>>(a, g);
  return hipGetLastError();
}

hipError_t launch_adamw_cells(const AdamArgs& a, int n_cells, long slot_len, const int* active,
                              long sched_cell_stride, hipStream_t st) {
  if (!a.sched || n_cells > 65535) return hipErrorInvalidValue;  // table-driven only; cells on grid y
  AdamGrid g{};
  const int nb = adam_grid(a, &g);
  if (nb == 0 || n_cells <= 0) return hipSuccess;
  adamw_cells_kernel<<<dim3(nb, n_cells), 256, 0, st>>>(a, g, active, slot_len, sched_cell_stride);
  return hipGetLastError();
}

}  // namespace pgp
