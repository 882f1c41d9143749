// cnf_grad2_coty.hip - the cotangent form of cnf_grad2.hip's kernel (cnf_grad2_cot.hip) with the cotangent of the conditions, ys_bar:
// the pullback of the fixed-step solve of a conditioned flow with respect to ys as well (cnf_integrate_fixed_vjp_cond /
// cnf_integrate_grid_vjp_cond).  Instantiation-only translation unit; the conditioned shapes of the table only.
#define G2_COT true
#define G2_YB true
#define G2_FIND grad2_coty_kernel
#define G2_ONLY G2_SHAPES(4, CNF_ACT_TANH), G2_SHAPES(4, CNF_ACT_SOFTPLUS)
#include "cnf_grad2.hip"
