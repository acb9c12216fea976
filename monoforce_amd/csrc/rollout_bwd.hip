// Backward rollout: host side of mf_rollout_bwd_* (validate, fill the arguments, plan the route -- rollout_route.hip --, launch) and the
// reference-order (exact) kernel instantiations.
// Compiled with -ffp-contract=off; the FMA-contracted float32 kernels live in rollout_bwd_fast.hip.
#include "rollout_bwd_cp_kernel.h"
#include "rollout_bwd_mw_kernel.h"

namespace mf {

static BwdBits bwd_bits(const MfRolloutBwdBufs* p) {
  BwdBits b{};
  b.joints = p->joint_angles != nullptr; b.rec = p->rec != nullptr; b.zmu = p->zmu != nullptr; b.zmu_scratch = p->zmu_scratch != nullptr;
  b.mu = p->mu != nullptr; b.zeros = p->zeros != nullptr;
  b.gXs = p->gXs != nullptr; b.gXds = p->gXds != nullptr; b.gRs = p->gRs != nullptr; b.gOmegas = p->gOmegas != nullptr;
  b.gFs = p->gFs != nullptr; b.gFf = p->gFf != nullptr;
  b.rec_low = (unsigned)((uintptr_t)p->rec & 31); b.zmu_low = (unsigned)(((uintptr_t)p->zmu_scratch | (uintptr_t)p->zmu) & 15);
  if (const MfRolloutLoss* L = p->loss) {
    b.loss = true; b.loss_flags = L->flags; b.loss_T2 = L->T2;
    b.loss_near_w = L->near && L->w;
    b.loss_rows = L->T2 > 0 && L->gt && L->row_stamp && L->row_w && L->gloss && L->Xs;
    b.loss_value = L->partial && L->ticket && L->loss;
  }
  return b;
}

template <typename S>
static int rollout_bwd(const MfRolloutDesc* d, const MfRolloutBwdBufs* p, void* stream) {
  MF_REQUIRE(d && p, MF_ERR_INVALID, "rollout_bwd: null descriptor");
  MF_REQUIRE(d->B > 0 && d->N > 0 && d->H > 1 && d->W > 0 && d->T >= 1, MF_ERR_INVALID, "rollout_bwd: B, T, N, H, W must be positive");
  MF_REQUIRE(d->n_tracks == 2 || d->n_tracks == 4, MF_ERR_INVALID, "n_tracks must be 2 or 4");
  MF_REQUIRE(d->integrator == MF_INTEG_DYNAMICS || d->integrator == MF_INTEG_ODEINT_EULER, MF_ERR_INVALID,
             "rollout_bwd: unknown integrator");
  MF_REQUIRE(p->z && p->controls && p->ts && p->points && p->part && p->x_init && p->xd0 && p->R0 && p->w0, MF_ERR_INVALID,
             "rollout_bwd: null input buffer");
  MF_REQUIRE(p->Xraw && p->Xds && p->Rs && p->Omegas, MF_ERR_INVALID, "rollout_bwd: null saved-state buffer");
  MF_REQUIRE(p->gz && p->gxd0 && p->gR0 && p->gw0, MF_ERR_INVALID, "rollout_bwd: null gradient output buffer");
  MF_REQUIRE(d->N <= 512, MF_ERR_UNSUPPORTED, "rollout_bwd: more than 512 contact points");
  MF_REQUIRE(d->H < (1 << 23), MF_ERR_UNSUPPORTED, "rollout_bwd: grid too large (H must be below 2^23)");
  MF_REQUIRE(d->H >= 2, MF_ERR_INVALID, "rollout_bwd: the grid needs at least 2 x 2 cells");
  MF_REQUIRE(d->controls_stride_b == 0 && d->controls_stride_t == 0, MF_ERR_UNSUPPORTED, "rollout_bwd: controls must be contiguous [B][T][2]");
  MF_REQUIRE(d->map_shared || (long long)d->B * d->H * d->W * (long long)sizeof(S) < (1ll << 32), MF_ERR_UNSUPPORTED,
             "rollout_bwd: per-rollout maps of 4 GiB or more in total (use a shared map or split the batch)");
  MF_REQUIRE((long long)(d->grad_copies > 1 ? d->grad_copies : 1) * d->H * d->W * (long long)sizeof(S) < (1ll << 32), MF_ERR_UNSUPPORTED,
             "rollout_bwd: gradient copies of 4 GiB or more in total");
  MF_REQUIRE(d->block == 0 || d->block == 64 || d->block == 128 || d->block == 256, MF_ERR_INVALID, "rollout_bwd: block must be 64, 128 or 256");

  RolloutBwdArgs<S> a;
  a.B = d->B; a.T = d->T; a.N = d->N; a.H = d->H; a.W = d->W;
  a.n_tracks = d->n_tracks; a.layout = d->layout; a.map_shared = d->map_shared; a.skip_snap = d->skip_snap;
  a.grad_copies = d->grad_copies > 1 ? d->grad_copies : 1;
  a.mass = (S)d->mass; a.inv_mass = (S)(1.0 / d->mass); a.inv_res = (S)(1.0 / (double)(S)d->grid_res); a.mg = (S)(d->mass * d->gravity); a.k = (S)d->stiffness; a.damp = (S)d->damping;
  a.omega_max = (S)d->omega_max; a.res = (S)d->grid_res; a.d_max = (S)d->d_max; a.dt = (S)d->dt;
  a.half_ly = (S)(d->robot_size_y / 2.0);
  a.sink = (S)(d->mass * d->gravity / (d->stiffness + 1e-6));
  for (int i = 0; i < 9; ++i) a.Iinv[i] = (S)d->Iinv[i];
  for (int i = 0; i < 12; ++i) a.joint_xyz[i] = (S)d->joint_xyz[i];
  a.joint_angles = (const S*)p->joint_angles;
  a.gjoint = (S*)p->gjoint_angles;
  a.rec = nullptr;
  a.zmu = nullptr;
  a.loss_T2 = 0; a.loss_gt = nullptr; a.loss_row_stamp = nullptr; a.loss_row_w = nullptr; a.loss_gloss = nullptr; a.loss_inv_count = (S)0;
  a.loss_partial = nullptr; a.loss_ticket = nullptr; a.loss_out = nullptr; a.loss_near = nullptr; a.loss_w = nullptr;
  MF_REQUIRE(!p->gjoint_angles || p->joint_angles, MF_ERR_INVALID, "rollout_bwd: gjoint_angles without joint_angles");
  MF_REQUIRE(!d->has_joints == !p->joint_angles, MF_ERR_INVALID, "rollout_bwd: joint_angles must be given exactly when desc->has_joints is set");
  MF_REQUIRE(!p->joint_angles || d->n_tracks == 4, MF_ERR_INVALID, "rollout_bwd: joint angles need the 4 driving parts of robot 'marv'");
  a.z = (const S*)p->z; a.mu = (const S*)p->mu; a.controls = (const S*)p->controls; a.ts = (const S*)p->ts;
  a.points = (const S*)p->points; a.part = p->part;
  a.x_init = (const S*)p->x_init; a.xd0 = (const S*)p->xd0; a.R0 = (const S*)p->R0; a.w0 = (const S*)p->w0;
  a.Xraw = (const S*)p->Xraw; a.Xds = (const S*)p->Xds; a.Rs = (const S*)p->Rs; a.Om = (const S*)p->Omegas;
  const BwdRoute r = plan_bwd(d, (int)sizeof(S), bwd_bits(p));
  MF_REQUIRE(r.rc == MF_OK, r.rc, r.msg);
  hipStream_t st = (hipStream_t)stream;
  if (const MfRolloutLoss* L = p->loss) {      // the forward's fused physics loss: dL/dXs is formed inside the kernel from Xs, the ground truth and gloss
    a.loss_T2 = L->T2; a.loss_gt = (const S*)L->gt; a.loss_row_stamp = L->row_stamp; a.loss_row_w = (const S*)L->row_w; a.loss_gloss = (const S*)L->gloss;
    a.loss_inv_count = (S)(1.0 / ((double)d->B * L->T2 * 3));
    a.loss_near = L->near; a.loss_w = (const S*)L->w;
    if (L->flags & MF_LOSS_VALUE_IN_BACKWARD) {      // the fetching waves also form the loss value
      a.loss_partial = (S*)L->partial; a.loss_ticket = L->ticket; a.loss_out = (S*)L->loss;
    }
  }
  const S* zr = (const S*)p->zeros;
  a.gXs = p->gXs ? (const S*)p->gXs : zr;       a.sXs = p->gXs ? 3 : 0;
  if (p->loss) { a.gXs = (const S*)p->loss->Xs; a.sXs = 3; }      // the fetching waves read Xs rows where they would read dL/dXs rows
  a.gXds = p->gXds ? (const S*)p->gXds : zr;    a.sXds = p->gXds ? 3 : 0;
  a.gOm = p->gOmegas ? (const S*)p->gOmegas : zr; a.sOm = p->gOmegas ? 3 : 0;
  a.gRs = p->gRs ? (const S*)p->gRs : zr;       a.sRs = p->gRs ? 9 : 0;
  a.gFs = p->gFs ? (const S*)p->gFs : zr;       a.sFs = p->gFs ? 3 : 0;
  a.gFf = p->gFf ? (const S*)p->gFf : zr;       a.sFf = p->gFf ? 3 : 0;
  a.gz = (S*)p->gz; a.gmu = (S*)p->gmu; a.gcontrols = (S*)p->gcontrols;
  a.gc_sb = 2 * d->T; a.gc_st = 2;
  // without the buffer the one-point-per-lane kernels send the rows to a dump (RolloutBwdArgs.gc_sb); the component-parallel kernels
  // compile the control gradient out instead (GCTRL), the multi-wave ones test for NULL
  if (!p->gcontrols && r.family != kBwdCp && r.family != kBwdMw) { a.gcontrols = (S*)p->gw0; a.gc_sb = 3; a.gc_st = 0; }
  a.gx0 = (S*)p->gx0; a.gxd0 = (S*)p->gxd0; a.gR0 = (S*)p->gR0; a.gw0 = (S*)p->gw0;
  if (r.record) a.rec = (const S*)p->rec;
  if (r.zmu) a.zmu = interleaved_maps<S>(r.interleave ? nullptr : p->zmu, p->zmu_scratch, a.z, a.mu, d->H * d->W, st);

  const int integ = d->integrator;
  if constexpr (sizeof(S) == 8) {
    switch (r.family) {
      case kBwdJoints: return launch_rollout_bwd_joints_f64(a, r, integ, st);
      case kBwdCp: return launch_rollout_bwd_cp_f64(a, r, integ, st);
      case kBwdMw: return launch_rollout_bwd_mw_f64(a, r, integ, st);
      default: return launch_rollout_bwd<S, false>(a, r, integ, st);      // kBwdGeneral
    }
  } else {
    switch (r.family) {
      case kBwdJoints: return r.fast ? launch_rollout_bwd_joints_fast_f32(a, r, integ, st) : launch_rollout_bwd_joints_f32(a, r, integ, st);
      case kBwdCp: return launch_rollout_bwd_cp_f32(a, r, integ, st);
      case kBwdMw: return launch_rollout_bwd_mw_f32(a, r, integ, st);
      case kBwdXs:
        if (r.win) return r.loss ? launch_rollout_bwd_xs_win_loss_fast_f32(a, r, integ, st) : launch_rollout_bwd_xs_win_fast_f32(a, r, integ, st);
        return r.loss ? launch_rollout_bwd_xs_loss_fast_f32(a, r, integ, st) : launch_rollout_bwd_xs_fast_f32(a, r, integ, st);
      case kBwdXsPpl: return launch_rollout_bwd_xs_ppl_fast_f32(a, r, integ, st);
      case kBwdCarry: return launch_rollout_bwd_carry_fast_f32(a, r, integ, st);
      case kBwdFast: return launch_rollout_bwd_fast_f32(a, r, integ, st);
      default: return launch_rollout_bwd<S, false>(a, r, integ, st);      // kBwdGeneral
    }
  }
}

}  // namespace mf

extern "C" int mf_rollout_bwd_f32(const MfRolloutDesc* d, const MfRolloutBwdBufs* p, void* s) {
  return mf::rollout_bwd<float>(d, p, s);
}
extern "C" int mf_rollout_bwd_f64(const MfRolloutDesc* d, const MfRolloutBwdBufs* p, void* s) {
  return mf::rollout_bwd<double>(d, p, s);
}
