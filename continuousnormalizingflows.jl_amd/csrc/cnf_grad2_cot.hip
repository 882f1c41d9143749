// cnf_grad2_cot.hip - the barrier-free gradient kernel of cnf_grad2.hip instantiated in its cotangent form: the pullback of the
// fixed-step solve (cnf_integrate_fixed_vjp / cnf_integrate_grid_vjp), one probe.  Instantiation-only translation unit.
#define G2_COT true
#define G2_FIND grad2_cot_kernel
#include "cnf_grad2.hip"
