// pgp_fpetrain_cells.hip — the cell-indexed instantiations of the FPE's offline
// training step (fpe_step_kernel<H, true, true>: a model's n sequential steps with
// their AdamW in one workgroup, one workgroup per model; fpe_step_kernel<H, false,
// true>: the forwards of many models' windows) and their launches
// (launch_fpe_train_steps_cells, launch_fpe_forward_cells), for pgp_fpe_train_steps,
// pgp_fpe_train_steps_many and pgp_fpe_forward_many_cells: PreGAN.py:39-49's
// train_model for a fleet that keeps one FPE per PreGANRecovery.
//
// The kernel is the template of pgp_fpetrain.hip, compiled here in a translation
// unit of its own so that the four lone kernels of pgp_fpetrain.hip are built
// exactly as before.
#define PGP_FPE_CELLS_TU 1
#include "pgp_fpetrain.hip"
