// kernels_rrlu_reg_r4.hip — the instantiations of the register-resident rrLU kernel with 4 rows per thread (rrlu_reg_launch_rpt4) as
// their own translation unit, so that they compile beside the others.
#define T4A_REG_RPT 4
#include "kernels_rrlu_reg.hip"
