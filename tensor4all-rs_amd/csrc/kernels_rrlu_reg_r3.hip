// kernels_rrlu_reg_r3.hip — the instantiations of the register-resident rrLU kernel with 3 rows per thread (rrlu_reg_launch_rpt3) as
// their own translation unit, so that they compile beside the others.
#define T4A_REG_RPT 3
#include "kernels_rrlu_reg.hip"
