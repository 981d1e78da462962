// kernels_rrlu_reg_r2.hip — the instantiations of the register-resident rrLU kernel with 2 rows per thread (rrlu_reg_launch_rpt2) as
// their own translation unit, so that they compile beside the others.
#define T4A_REG_RPT 2
#include "kernels_rrlu_reg.hip"
