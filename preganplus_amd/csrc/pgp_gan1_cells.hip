// pgp_gan1_cells.hip — the cell-indexed instantiations of the fused batch-1 GAN
// step (gan1_forward_kernel<H, true>, gan1_step_kernel<H, true>) and their
// launches (launch_gan1_forward_cells, launch_gan1_step_cells), for a fleet of
// cells that each train their own Gen / Disc (pgp_gan_forward1_many,
// pgp_gan_step1_many; recovery/PreGANPlus.py:60-81 per PreGANPlusRecovery).
//
// The kernels are the templates of pgp_gan1.hip, compiled here in a translation
// unit of their own so that the single-cell kernels of pgp_gan1.hip are built
// exactly as before (see the note above its launches).
#define PGP_G1_CELLS_TU 1
#include "pgp_gan1.hip"
