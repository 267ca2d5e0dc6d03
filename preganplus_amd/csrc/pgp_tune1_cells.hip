// pgp_tune1_cells.hip — the cell-indexed instantiations of the fused batch-1
// kernels (tune1_kernel<H, DROP, true>, infer1_kernel<H, true>,
// fwd_cells_kernel<H>) and their launches (launch_tune1_cells, launch_fwd_cells,
// launch_infer1_cells), for a fleet of cells that each train their own weights
// (pgp_tune_step1_many, pgp_tune_forward_cells, pgp_forward1_many).
//
// The kernels are the templates of pgp_tune1.hip, compiled here in a translation
// unit of their own so that the single-cell kernels of pgp_tune1.hip are built
// exactly as before (see the note above its launches).  The phase-timing study
// (PGP_T1_PROF) covers the single-cell step only.
#undef PGP_T1_PROF
#define PGP_T1_CELLS_TU 1
#include "pgp_tune1.hip"
