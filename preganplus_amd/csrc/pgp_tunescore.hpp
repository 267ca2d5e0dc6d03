// pgp_tunescore.hpp — accuracy()'s scores (train.py:60-109) of a fleet's cells
// on the device (pgp_tunescore.hip, pgp_tune_scores_many).
#pragma once
#include <hip/hip_runtime.h>

namespace pgp {

// One 64-lane workgroup per cell, cells on grid x.  logits64 / protos64
// [n_cells][n][H][2] fp64 (launch_fwd_cells' outputs), y / cls [n_cells][n][H],
// state [n_cells][2K+3] fp64; scores [n_cells][2] fp64, flag [n_cells].
// H is 8 or 16 (tune1_supported), K >= 3, n >= 1.
hipError_t launch_tune_scores_cells(int H, int K, int n_cells, int n, const int* active, const double* logits64,
                                    const double* protos64, const int* y, const int* cls, const double* state,
                                    double* scores, int* flag, hipStream_t st);

}  // namespace pgp
