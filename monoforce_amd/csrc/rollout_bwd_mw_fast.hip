// Backward rollout of one rollout over several waves (rollout_bwd_mw_kernel.h): float32 fast-math instantiations.
#include "rollout_bwd_mw_kernel.h"

namespace mf {

int launch_rollout_bwd_mw_f32(const RolloutBwdArgs<float>& a, const BwdRoute& r, int integ, hipStream_t st) {
  return launch_rollout_bwd_mw_t<float>(a, r, integ, st);
}

}  // namespace mf
