// pgp_tunedata_cells.hpp — launcher of a fleet's on-the-fly datasets
// (pgp_tunedata_cells.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace pgp {

// one workgroup: kMaxTuneRows waves (wave = dataset row), 64 lanes = whole cells
// of 2^dc_cell_shift(H) lanes each (lane = host)
constexpr int kDcLanes = 64;
constexpr int dc_cell_shift(int H) {  // log2 of the lanes a cell takes: the next power of two >= H
  int s = 0;
  while ((1 << s) < H) ++s;
  return s;
}

// tune_dataset_kernel (pgp_tunedp.hip) for M cells, each normalised by its own
// train_max [M][3H]; active [M] or nullptr (all); positive [M][R] and infer
// [M][3][3H] may be nullptr
hipError_t launch_tune_dataset_cells(int H, int M, int R, const int* active, const double* series,
                                     const double* train_max, float* windows, int* y, int* cls, int* positive,
                                     float* infer, hipStream_t st);

}  // namespace pgp
