// Backward rollout, component-parallel lane mapping (rollout_bwd_cp_kernel.h): float32 fast-math instantiations, default integrator
// (dynamics(): rollout_bwd_dyn_cp_fast.hip).
#include "rollout_bwd_cp_kernel.h"

namespace mf {

int launch_rollout_bwd_cp_f32(const RolloutBwdArgs<float>& a, const BwdRoute& r, int integ, hipStream_t st) {
  if (integ == MF_INTEG_DYNAMICS) return launch_rollout_bwd_cp_dynamics_f32(a, r, st);
  return launch_rollout_bwd_cp_variant<float, MF_INTEG_ODEINT_EULER>(a, r, st);
}

}  // namespace mf
