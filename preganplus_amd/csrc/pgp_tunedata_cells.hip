// pgp_tunedata_cells.hip — the on-the-fly tuning datasets of a fleet of cells
// on the device, each cell on its own training series:
//
//   tune_dataset_cells_kernel  tune_dataset_kernel (pgp_tunedp.hip) over a
//                              leading cell axis: load_on_the_fly_dataset
//                              (utils.py:40-47) — the cell's last R rows,
//                              normalised by ITS training series' column max
//                              (utils.py:94-95), cut into windows
//                              (convert_to_windows, utils.py:7-14), labelled by
//                              form_test_dataset (utils.py:16-24) — plus
//                              run_encoder's inference window of the same rows
//                              (PreGANPlus.py:107-112), and per window whether
//                              any host carries a positive label (what the
//                              AdamW schedule of the cell's tuning step needs)
//
// fp64 with FMA contraction off; every value goes through tune_dataset_kernel's
// operations in its order, so a cell's outputs have the bits that kernel gives
// for the cell alone with its train_max.  The C-ABI entry lives here as well.
#include <hip/hip_runtime.h>

#include <string>

#include "../../include/preganplus.h"
#include "pgp_device.hpp"
#include "pgp_tunedata_cells.hpp"
#include "pgp_tunedp.hpp"

namespace pgp {
namespace {

constexpr int kWin = 3;  // models.py:320 n_window
constexpr int kDcThreads = kDcLanes * kMaxTuneRows;  // 1024

// ---------------------------------------------------------------------------
// Lane map: wave = dataset row r (kMaxTuneRows waves, those with r >= R idle),
// lane = (cell within the workgroup, host): a cell takes 2^shift >= H lanes,
// 64 >> shift whole cells share a workgroup (8 at H = 8, 4 at H = 16, 1 at
// H = 50), so a row's hosts of one cell always sit in ONE wave and the row's
// `positive` flag is one ballot.  A thread holds its host's three columns of
// its row.  Each lane takes its own cell's divisor and active flag; a lane
// without work (inactive cell, cell >= M, host >= H, row >= R) loads and
// stores nothing but runs to both barriers and the ballot.
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(kDcThreads) void tune_dataset_cells_kernel(
    int H, int M, int R, int shift, const int* __restrict__ active, const double* __restrict__ series,
    const double* __restrict__ train_max, float* __restrict__ windows, int* __restrict__ y, int* __restrict__ cls,
    int* __restrict__ positive, float* __restrict__ infer) {
#pragma clang fp contract(off)
  __shared__ double sv[3][kMaxTuneRows][kDcLanes];  // normalised rows
  __shared__ double sab[3][2][kDcLanes];            // the percentile's order statistics (ranks ilo, ihi)
  const int lane = threadIdx.x & (kDcLanes - 1), r = threadIdx.x / kDcLanes;
  const int cl = lane >> shift, h = lane & ((1 << shift) - 1);
  const long m = (long)blockIdx.x * (kDcLanes >> shift) + cl;
  const bool in = m < M && h < H;
  const bool on = in && (active == nullptr || active[m] != 0);
  const bool live = on && r < R;
  const int F = 3 * H;
  double v[3] = {0.0, 0.0, 0.0};
  if (live) {
    const double* s = series + ((long)m * R + r) * F + 3 * h;
    const double* tm = train_max + (long)m * F + 3 * h;
#pragma unroll
    for (int c = 0; c < 3; ++c) v[c] = s[c] / (tm[c] + 1e-8);  // np.max(train, axis=0) + 1e-8
  }
#pragma unroll
  for (int c = 0; c < 3; ++c) sv[c][r][lane] = v[c];
  // 98th percentile of the column, numpy 'linear': virtual index (R-1)*0.98,
  // gamma = frac, lerp(a, b, g) = g >= 0.5 ? b - (b-a)(1-g) : a + (b-a) g.
  // The order statistics ilo, ihi by stable rank, as tune_dataset_kernel.
  const double vi = (double)(R - 1) * (98.0 / 100.0);
  const double lo = floor(vi);
  const double gm = vi - lo;
  const int ilo = (int)lo, ihi = ilo + 1 < R ? ilo + 1 : R - 1;
  __syncthreads();
  if (live) {
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      int rank = 0;
#pragma unroll
      for (int j = 0; j < kMaxTuneRows; ++j) {
        const double vj = sv[c][j][lane];
        if (j != r && j < R) rank += (vj < v[c] || (j < r && vj == v[c])) ? 1 : 0;
      }
      if (rank == ilo) sab[c][0][lane] = v[c];
      if (rank == ihi) sab[c][1][lane] = v[c];
    }
  }
  __syncthreads();
  bool an = false;
  if (live) {
    // convert_to_windows: window r = rows r-3..r-1, row 0 repeated for r < 3
#pragma unroll
    for (int w = 0; w < kWin; ++w) {
      const int src = r >= kWin ? r - kWin + w : (w < kWin - r ? 0 : w - (kWin - r));
      float* o = windows + (((long)m * R + r) * kWin + w) * F + 3 * h;
#pragma unroll
      for (int c = 0; c < 3; ++c) o[c] = (float)sv[c][src][lane];
    }
    if (infer && r == 0) {  // run_encoder: [R-3, R-3, R-2]; R = 1, 2: row 0 three times
      const int ra = R >= kWin ? R - 3 : 0, rb = R >= kWin ? R - 2 : 0;
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        const double u0 = sv[c][ra][lane], u1 = sv[c][rb][lane];
#pragma unroll
        for (int w = 0; w < kWin; ++w) infer[((long)m * kWin + w) * F + 3 * h + c] = (float)(w < 2 ? u0 : u1);
      }
    }
    double thr[3];
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const double a = sab[c][0][lane], b = sab[c][1][lane];
      const double d = b - a;
      thr[c] = gm >= 0.5 ? b - d * (1.0 - gm) : a + d * gm;
    }
    an = v[0] > thr[0] || v[1] > thr[1] || v[2] > thr[2];
    int am = 0;  // np.argmax: first maximum
    double best = v[0];
    if (v[1] > best) {
      am = 1;
      best = v[1];
    }
    if (v[2] > best) am = 2;
    y[((long)m * R + r) * H + h] = an ? 1 : 0;
    cls[((long)m * R + r) * H + h] = am;
  }
  // any positive label among the row's hosts of the cell: the wave's ballot, cut to the cell's lanes
  const unsigned long long bal = __ballot(an);
  if (positive && live && h == 0) {
    const unsigned long long seg = shift == 6 ? bal : (bal >> (cl << shift)) & ((1ull << (1 << shift)) - 1ull);
    positive[(long)m * R + r] = seg != 0ull ? 1 : 0;
  }
}

}  // namespace

hipError_t launch_tune_dataset_cells(int H, int M, int R, const int* active, const double* series,
                                     const double* train_max, float* windows, int* y, int* cls, int* positive,
                                     float* infer, hipStream_t st) {
  static_assert(kDcLanes == 64, "a row's ballot covers one wave");
  const int shift = dc_cell_shift(H);
  const int per = kDcLanes >> shift;
  const int grid = (int)(((long)M + per - 1) / per);
  tune_dataset_cells_kernel<<<grid, kDcThreads, 0, st>>>(H, M, R, shift, active, series, train_max, windows, y, cls,
                                                         positive, infer);
  return hipGetLastError();
}

}  // namespace pgp

using namespace pgp;

extern "C" {

int pgp_tune_dataset_cells(int n_hosts, int n_cells, int n_rows, const int* active, const double* series,
                           const double* train_max, float* windows, int* y, int* cls, int* positive, float* infer,
                           void* stream) {
  if (n_hosts <= 0 || n_hosts > kDcLanes)
    return set_error(PGP_ERR_UNSUPPORTED, "pgp_tune_dataset_cells: 1 <= hosts <= 64");
  if (n_cells < 0) return set_error(PGP_ERR_ARG, "pgp_tune_dataset_cells: n_cells >= 0");
  if (n_rows < 1 || n_rows > kMaxTuneRows) return set_error(PGP_ERR_ARG, "pgp_tune_dataset_cells: 1 <= n_rows <= 16");
  if (n_cells == 0) return PGP_OK;
  if (!series || !train_max || !windows || !y || !cls)
    return set_error(PGP_ERR_ARG, "pgp_tune_dataset_cells: NULL pointer");
  const hipError_t e = launch_tune_dataset_cells(n_hosts, n_cells, n_rows, active, series, train_max, windows, y, cls,
                                                 positive, infer, reinterpret_cast<hipStream_t>(stream));
  if (e != hipSuccess)
    return set_error(PGP_ERR_HIP, std::string("tune_dataset_cells_kernel: ") + hipGetErrorString(e));
  return PGP_OK;
}

}  // extern "C"
