// Forward rollout, float32 fast-math instantiations: this TU is compiled with -ffp-contract=fast (FMA), and the
// kernels use the hardware reciprocal / rsqrt / exp2 (Mth<float, true> in rollout_fwd_kernel.h).
#include "rollout_fwd_kernel.h"

namespace mf {
int launch_rollout_fwd_fast_f32(const RolloutArgs<float>& a, const FwdRoute& r, int integ, hipStream_t st) {
  if (r.record)      // the record of rollout_bwd_mw_kernel.h
    return r.forces ? launch_rollout_fwd_mw_rec<true>(a, r, integ, st) : launch_rollout_fwd_mw_rec<false>(a, r, integ, st);
  if (!r.forces) return launch_rollout_fwd<float, true, false, false>(a, r, integ, st);   // states only
  return launch_rollout_fwd<float, true>(a, r, integ, st);
}
}  // namespace mf
