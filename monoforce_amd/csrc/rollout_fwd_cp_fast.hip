// Forward rollout, component-parallel lane mapping (rollout_fwd_cp_kernel.h): float32 fast-math instantiations.  Built with FMA
// contraction like the other *_fast units.
#include "rollout_fwd_cp_kernel.h"

namespace mf {

int launch_rollout_fwd_cp_f32(const RolloutArgs<float>& a, const FwdRoute& r, int integ, hipStream_t st) {
  return launch_rollout_fwd_cp_t<float>(a, r, integ, st);
}

}  // namespace mf
