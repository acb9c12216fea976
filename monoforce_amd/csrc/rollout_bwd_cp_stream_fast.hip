// Backward rollout, component-parallel lane mapping, default integrator, from the forward's per-step record STREAMED through LDS by
// two more waves of the workgroup (MODE = kCpStream, rollout_bwd_cp_kernel.h): a translation unit of its own -- four kernels, and
// the only ones whose computing loop has no memory latency of its own to schedule around.
#include "rollout_bwd_cp_kernel.h"

#ifdef MF_STREAM_PROFILE
namespace mf { __device__ unsigned long long mf_stream_prof[32]; }
extern "C" int mf_debug_stream_profile(unsigned long long* out32, int reset) {
  if (out32) { if (hipMemcpyFromSymbol(out32, HIP_SYMBOL(mf::mf_stream_prof), sizeof(mf::mf_stream_prof)) != hipSuccess) return 1; }
  if (reset) { unsigned long long z[32] = {}; if (hipMemcpyToSymbol(HIP_SYMBOL(mf::mf_stream_prof), z, sizeof(z)) != hipSuccess) return 2; }
  return 0;
}
#endif
namespace mf {

// Workgroup = the computing wave + two fetching waves.  Ring: twelve slots or six (rollout_route.hip; the positions-only variants of the
// six-slot form, held to 256 registers there, fetch in batches of TWO steps: no scratch).
void launch_rollout_bwd_cp_stream_f32(const RolloutBwdArgs<float>& a, const BwdRoute& r, hipStream_t st) {
  constexpr int I = MF_INTEG_ODEINT_EULER;
  const bool gc = a.gcontrols != nullptr, xs_only = r.xs_only;
  const unsigned grid = r.grid;
#define MF_BCPS(XS_, GC_) do { if (r.ring_slots == 12) MF_KLAUNCH((rollout_bwd_cp_kernel<float, I, XS_, GC_, kCpStream, 12>), dim3(grid), dim3(r.block), 0, st, a); \
                               else MF_KLAUNCH((rollout_bwd_cp_kernel<float, I, XS_, GC_, kCpStream, 6, (XS_ ? 2 : 3)>), dim3(grid), dim3(r.block), 0, st, a); } while (0)
  if (xs_only) { if (gc) MF_BCPS(true, true); else MF_BCPS(true, false); }
  else         { if (gc) MF_BCPS(false, true); else MF_BCPS(false, false); }
#undef MF_BCPS
}

}  // namespace mf
