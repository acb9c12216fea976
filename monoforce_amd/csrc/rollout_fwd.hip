// Forward rollout: host side of mf_rollout_fwd_* (validate, fill the arguments, plan the route -- rollout_route.hip --, launch) and the
// reference-order (exact) kernel instantiations.
// This TU is compiled with -ffp-contract=off; the FMA-contracted float32 kernels live in rollout_fwd_fast.hip.
#include "rollout_fwd_cp_kernel.h"

namespace mf {
int launch_rollout_fwd_mw_rec_f64(const RolloutArgs<double>& a, const FwdRoute& r, int integ, hipStream_t st);   // rollout_mw_f64.hip

template <typename S>
static int fill_args(const MfRolloutDesc* d, const MfRolloutFwdBufs* p, RolloutArgs<S>* a) {
  MF_REQUIRE(d && p, MF_ERR_INVALID, "rollout_fwd: null descriptor");
  MF_REQUIRE(d->B > 0 && d->N > 0 && d->H > 1 && d->W > 0, MF_ERR_INVALID, "rollout_fwd: B, N, H, W must be positive");
  MF_REQUIRE(d->T >= 1, MF_ERR_INVALID, "rollout_fwd: T must be >= 1");
  MF_REQUIRE(d->n_tracks == 2 || d->n_tracks == 4, MF_ERR_INVALID, "n_tracks must be 2 or 4");
  MF_REQUIRE(d->integrator == MF_INTEG_DYNAMICS || d->integrator == MF_INTEG_ODEINT_EULER, MF_ERR_INVALID,
             "rollout_fwd: unknown integrator");
  MF_REQUIRE(d->layout == MF_LAYOUT_BATCH_MAJOR || d->layout == MF_LAYOUT_TIME_MAJOR, MF_ERR_INVALID,
             "rollout_fwd: unknown layout");
  MF_REQUIRE(d->math_mode == MF_MATH_EXACT || d->math_mode == MF_MATH_FAST, MF_ERR_INVALID, "rollout_fwd: unknown math_mode");
  MF_REQUIRE(p->z && p->controls && p->ts && p->points && p->part && p->x0 && p->xd0 && p->R0 && p->w0, MF_ERR_INVALID,
             "rollout_fwd: null input buffer");
  MF_REQUIRE(p->Xs && p->Rs && (p->cost_rows || (p->Xds && p->Omegas)), MF_ERR_INVALID, "rollout_fwd: null output buffer");
  MF_REQUIRE((p->Fs != nullptr) == (p->Ff != nullptr), MF_ERR_INVALID, "rollout_fwd: pass both force buffers or neither");
  MF_REQUIRE((long long)d->H * d->W < (1ll << 30), MF_ERR_UNSUPPORTED, "rollout_fwd: grid too large");
  MF_REQUIRE(d->H < (1 << 23), MF_ERR_UNSUPPORTED, "rollout_fwd: grid too large (H must be below 2^23)");
  MF_REQUIRE(d->H >= 2, MF_ERR_INVALID, "rollout_fwd: the grid needs at least 2 x 2 cells");
  MF_REQUIRE(d->N <= 512, MF_ERR_UNSUPPORTED, "rollout_fwd: more than 512 contact points");
  MF_REQUIRE(d->map_shared || (long long)d->B * d->H * d->W * (long long)sizeof(S) < (1ll << 32), MF_ERR_UNSUPPORTED,
             "rollout_fwd: per-rollout maps of 4 GiB or more in total (use a shared map or split the batch)");
  MF_REQUIRE(d->block == 0 || d->block == 64 || d->block == 128 || d->block == 256, MF_ERR_INVALID, "rollout_fwd: block must be 64, 128 or 256");
  const LaneMap m = fwd_lane_map(d, false);
  const int fstride = d->force_stride ? d->force_stride : d->N;
  MF_REQUIRE(!p->Fs || fstride >= m.G * m.PPL, MF_ERR_INVALID,
             "rollout_fwd: force_stride too small -- allocate Fs/Ff with mf_rollout_force_stride(desc) point slots per row");

  a->B = d->B; a->T = d->T; a->N = d->N; a->H = d->H; a->W = d->W;
  a->n_tracks = d->n_tracks; a->layout = d->layout; a->map_shared = d->map_shared; a->skip_snap = d->skip_snap; a->default_state = d->default_state; a->b0 = 0;
  const bool strided = d->controls_stride_b != 0 || d->controls_stride_t != 0;
  a->ctrl_sb = strided ? d->controls_stride_b : d->T * 2; a->ctrl_st = strided ? d->controls_stride_t : 2;
  MF_REQUIRE(a->ctrl_sb >= 0 && a->ctrl_st >= 0, MF_ERR_INVALID, "rollout_fwd: negative controls stride");
  a->fstride = fstride;
  a->mass = (S)d->mass; a->inv_mass = (S)(1.0 / d->mass); a->mg = (S)(d->mass * d->gravity); a->k = (S)d->stiffness;
  a->damp = (S)d->damping; a->omega_max = (S)d->omega_max; a->res = (S)d->grid_res; a->inv_res = (S)(1.0 / (double)(S)d->grid_res);   // RN(1 / res) of the ROUNDED res (Mth::cell_coord)
  a->d_max = (S)d->d_max; a->dt = (S)d->dt;
  a->half_ly = (S)(d->robot_size_y / 2.0);
  a->sink = (S)(d->mass * d->gravity / (d->stiffness + 1e-6));
  for (int i = 0; i < 9; ++i) a->Iinv[i] = (S)d->Iinv[i];
  a->z = (const S*)p->z; a->mu = (const S*)p->mu; a->controls = (const S*)p->controls; a->ts = (const S*)p->ts;
  a->points = (const S*)p->points; a->part = p->part;
  a->x0 = (S*)p->x0; a->xd0 = (const S*)p->xd0; a->R0 = (const S*)p->R0; a->w0 = (const S*)p->w0;
  a->Xs = (S*)p->Xs; a->Xds = (S*)p->Xds; a->Rs = (S*)p->Rs; a->Om = (S*)p->Omegas; a->Fs = (S*)p->Fs; a->Ff = (S*)p->Ff;
  a->Xraw = (S*)p->Xraw;
  a->joint_angles = (const S*)p->joint_angles;
  a->cost_rows = (S*)p->cost_rows; a->pose_stride = d->pose_stride > 0 ? d->pose_stride : 1;
  a->path_cost = (S*)p->path_cost;
  a->zmu = nullptr;
  a->rec = nullptr;
  a->loss_T2 = 0; a->loss_gt = nullptr; a->loss_row_w = nullptr; a->loss_partial = nullptr; a->loss_ticket = nullptr;
  a->loss_out = nullptr; a->loss_inv_count = (S)0; a->loss_poison = nullptr;
  for (int i = 0; i < 12; ++i) a->joint_xyz[i] = (S)d->joint_xyz[i];
  if (p->joint_angles) {
    MF_REQUIRE(d->n_tracks == 4, MF_ERR_UNSUPPORTED, "rollout_fwd: joint angles need 4 driving parts (fl, fr, rl, rr)");
    const LaneMap mj = fwd_lane_map(d, true);
    MF_REQUIRE(fstride >= mj.G * mj.PPL, MF_ERR_INVALID, "rollout_fwd: force_stride too small for the articulated kernels");
  }
  return MF_OK;
}


// (z, mu) of the shared maps interleaved for the ZMU kernels; without a friction map the second component is never used
template <typename S>
__global__ void __launch_bounds__(256) interleave_maps_kernel(const S* __restrict__ z, const S* __restrict__ mu, int n,
                                                             cp::Pk2<S>* __restrict__ out) {
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) out[i] = cp::Pk2<S>{z[i], mu ? mu[i] : (S)1};
}
template <typename S>
const S* interleaved_maps(const void* staged, void* scratch, const S* z, const S* mu, int n, hipStream_t st) {
  if (staged) return (const S*)staged;
  hipLaunchKernelGGL((interleave_maps_kernel<S>), dim3((n + 255) / 256), dim3(256), 0, st, z, mu, n, (cp::Pk2<S>*)scratch);
  return (const S*)scratch;
}
template const float* interleaved_maps<float>(const void*, void*, const float*, const float*, int, hipStream_t);
template const double* interleaved_maps<double>(const void*, void*, const double*, const double*, int, hipStream_t);

static FwdBits fwd_bits(const MfRolloutFwdBufs* p) {
  FwdBits b{};
  b.joints = p->joint_angles != nullptr; b.cost_rows = p->cost_rows != nullptr; b.forces = p->Fs != nullptr;
  b.xds = p->Xds != nullptr; b.omegas = p->Omegas != nullptr; b.xraw = p->Xraw != nullptr;
  b.rec = p->rec != nullptr; b.zmu = p->zmu != nullptr; b.zmu_scratch = p->zmu_scratch != nullptr; b.mu = p->mu != nullptr;
  b.rec_low = (unsigned)((uintptr_t)p->rec & 31); b.zmu_low = (unsigned)(((uintptr_t)p->zmu_scratch | (uintptr_t)p->zmu) & 15);
  if (const MfRolloutLoss* L = p->loss) {
    b.loss = true; b.loss_flags = L->flags; b.loss_T2 = L->T2; b.loss_out = L->loss != nullptr;
    b.loss_complete = L->T2 > 0 && L->gt && L->row_w && L->partial && L->ticket && L->loss;
  }
  return b;
}

inline int launch_rollout_fwd_cp_any(const RolloutArgs<float>& a, const FwdRoute& r, int integ, hipStream_t st) { return launch_rollout_fwd_cp_f32(a, r, integ, st); }
inline int launch_rollout_fwd_cp_any(const RolloutArgs<double>& a, const FwdRoute& r, int integ, hipStream_t st) { return launch_rollout_fwd_cp_f64(a, r, integ, st); }

template <typename S>
static int rollout_fwd(const MfRolloutDesc* d, const MfRolloutFwdBufs* p, void* s) {
  RolloutArgs<S> a;
  const int rc = fill_args<S>(d, p, &a);
  if (rc != MF_OK) return rc;
  const FwdRoute r = plan_fwd(d, (int)sizeof(S), fwd_bits(p));
  MF_REQUIRE(r.rc == MF_OK, r.rc, r.msg);
  hipStream_t st = (hipStream_t)s;
  const int integ = d->integrator;
  if (r.zmu) a.zmu = interleaved_maps<S>(r.interleave ? nullptr : p->zmu, p->zmu_scratch, a.z, a.mu, d->H * d->W, st);
  if (r.record) a.rec = (S*)p->rec;
  if (r.loss == kLossValueInBackward) a.loss_poison = (S*)p->loss->loss;      // the backward will form the value: mark it as not yet known
  if (r.loss == kLossInLaunch) {      // physics_loss inside the launch (MfRolloutLoss)
    const MfRolloutLoss* L = p->loss;
    a.loss_T2 = L->T2; a.loss_gt = (const S*)L->gt; a.loss_row_w = (const S*)L->row_w;
    a.loss_partial = (S*)L->partial; a.loss_ticket = L->ticket; a.loss_out = (S*)L->loss;
    a.loss_inv_count = (S)(1.0 / ((double)d->B * L->T2 * 3));
  }
  switch (r.family) {
    case kFwdCp: return launch_rollout_fwd_cp_any(a, r, integ, st);
    case kFwdGeneral:
      if (p->joint_angles) return launch_rollout_fwd<S, false, true>(a, r, integ, st);
      return launch_rollout_fwd<S, false>(a, r, integ, st);
    default: break;
  }
  if constexpr (sizeof(S) == 8) return launch_rollout_fwd_mw_rec_f64(a, r, integ, st);      // kFwdMwRecF64
  else switch (r.family) {
    case kFwdJointsFast: return launch_rollout_fwd_joints_fast_f32(a, r, integ, st);
    case kFwdCost: return launch_rollout_fwd_cost_f32(a, r, integ, st);
    case kFwdZmu: return launch_rollout_fwd_zmu_f32(a, r, integ, st);
    case kFwdSplit: return launch_rollout_fwd_split_fast_f32(a, r, integ, st);
    default: return launch_rollout_fwd_fast_f32(a, r, integ, st);      // kFwdFast
  }
}

}  // namespace mf

extern "C" int mf_rollout_fwd_f32(const MfRolloutDesc* d, const MfRolloutFwdBufs* p, void* s) { return mf::rollout_fwd<float>(d, p, s); }
extern "C" int mf_rollout_fwd_f64(const MfRolloutDesc* d, const MfRolloutFwdBufs* p, void* s) { return mf::rollout_fwd<double>(d, p, s); }

namespace mf {
template <typename S>
__global__ void default_state_kernel(int B, int T, const S* __restrict__ controls, S* __restrict__ x0, S* __restrict__ xd0,
                                     S* __restrict__ R0, S* __restrict__ w0) {
  const int b = blockIdx.x * blockDim.x + threadIdx.x;
  if (b >= B) return;
  const S v = controls[(size_t)b * T * 2 + 0], w = controls[(size_t)b * T * 2 + 1];
  const S zero = (S)0, one = (S)1;
  x0[b * 3 + 0] = zero; x0[b * 3 + 1] = zero; x0[b * 3 + 2] = zero;
  xd0[b * 3 + 0] = v; xd0[b * 3 + 1] = zero; xd0[b * 3 + 2] = zero;
  w0[b * 3 + 0] = zero; w0[b * 3 + 1] = zero; w0[b * 3 + 2] = w;
#pragma unroll
  for (int c = 0; c < 9; ++c) R0[b * 9 + c] = (c % 4 == 0) ? one : zero;
}
template <typename S>
static int default_state(int B, int T, const S* controls, S* x0, S* xd0, S* R0, S* w0, void* s) {
  MF_REQUIRE(B > 0 && T > 0 && controls && x0 && xd0 && R0 && w0, MF_ERR_INVALID, "rollout_default_state: bad argument");
  hipLaunchKernelGGL((default_state_kernel<S>), dim3((B + 255) / 256), dim3(256), 0, (hipStream_t)s, B, T, controls, x0, xd0, R0, w0);
  hipError_t e = hipGetLastError();
  MF_REQUIRE(e == hipSuccess, MF_ERR_LAUNCH, std::string("rollout_default_state launch: ") + hipGetErrorString(e));
  return MF_OK;
}
}  // namespace mf

extern "C" int mf_rollout_default_state_f32(int32_t B, int32_t T, const float* controls, float* x0, float* xd0, float* R0, float* w0, void* s) {
  return mf::default_state<float>(B, T, controls, x0, xd0, R0, w0, s);
}
extern "C" int mf_rollout_default_state_f64(int32_t B, int32_t T, const double* controls, double* x0, double* xd0, double* R0, double* w0, void* s) {
  return mf::default_state<double>(B, T, controls, x0, xd0, R0, w0, s);
}
