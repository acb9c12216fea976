// Float32 fast-math forward kernels reading ONE shared (height, friction) map pair interleaved cell by cell (ZMU): a point's
// footprint in both maps is two 16-byte loads instead of eight 4-byte ones.  Built with FMA contraction like the other
// *_fast units; same arithmetic, same bits as the kernels of rollout_fwd_fast.hip / _split_fast.hip / _cost.hip.
#include "rollout_fwd_kernel.h"

namespace mf {
int launch_rollout_fwd_zmu_f32(const RolloutArgs<float>& a, const FwdRoute& r, int integ, hipStream_t st) {
  if (r.cost == 2 && integ == MF_INTEG_ODEINT_EULER) return launch_rollout_fwd<float, true, false, false, 2, false, true>(a, r, integ, st);
  if (r.cost) return launch_rollout_fwd<float, true, false, false, 1, false, true>(a, r, integ, st);
  if (r.split && r.record)      // the record of rollout_bwd_mw_kernel.h, split stores
    return r.forces ? launch_rollout_fwd_mw_rec<true, true, true>(a, r, integ, st) : launch_rollout_fwd_mw_rec<false, true, true>(a, r, integ, st);
  if (r.split) {
    if (!r.forces) return launch_rollout_fwd<float, true, false, false, 0, true, true>(a, r, integ, st);
    return launch_rollout_fwd<float, true, false, true, 0, true, true>(a, r, integ, st);
  }
  if (r.record)      // the record of rollout_bwd_mw_kernel.h
    return r.forces ? launch_rollout_fwd_mw_rec<true, true>(a, r, integ, st) : launch_rollout_fwd_mw_rec<false, true>(a, r, integ, st);
  if (!r.forces) return launch_rollout_fwd<float, true, false, false, 0, false, true>(a, r, integ, st);
  return launch_rollout_fwd<float, true, false, true, 0, false, true>(a, r, integ, st);
}
}  // namespace mf
