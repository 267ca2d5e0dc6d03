// pgp_fpe1_cells.hip — the gated instantiation of the FPE's forward
// (fpe_step_kernel<16, false, false, true>: one window per cell under the cell's own
// slot of the natural FPE blob, then detect / embed / get_classes on the cell's
// prototypes and Gen_16 / Disc_16 from the cell's training master, one workgroup per
// cell) and its launch (launch_fpe_gate_cells), for pgp_fpe_forward1 and
// pgp_fpe_forward1_many: PreGANRecovery.run_model's forward (PreGAN.py:97-126) for a
// fleet that keeps one FPE, one set of prototypes and one Gen / Disc per
// PreGANRecovery.
//
// The kernel is the template of pgp_fpetrain.hip, compiled here in a translation
// unit of its own so that the kernels of pgp_fpetrain.hip and
// pgp_fpetrain_cells.hip are built exactly as before.
#define PGP_FPE_GATE_TU 1
#include "pgp_fpetrain.hip"
