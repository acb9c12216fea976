// Backward rollout, float32 fast-math instantiations (-ffp-contract=fast + hardware rcp / rsq / exp2).
#include "rollout_bwd_kernel.h"

namespace mf {
int launch_rollout_bwd_fast_f32(const RolloutBwdArgs<float>& a, const BwdRoute& r, int integ, hipStream_t st) {
  return launch_rollout_bwd<float, true, false, false>(a, r, integ, st);   // plain flush: fewest instructions per step
}
}  // namespace mf
