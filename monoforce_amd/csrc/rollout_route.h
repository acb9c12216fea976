// Which rollout kernel a launch runs: the A/B switches, the policy helpers and the two planners (rollout_route.hip).  Host code only.
// mf_rollout_fwd_* / mf_rollout_bwd_* validate their input, fill the kernel arguments, call a planner ONCE and hand its route to a
// launcher, which only maps the route's fields to a template instantiation; the public policy queries read the same planners.
#pragma once
#include "../../include/monoforce_hip.h"

namespace mf {

// Lane mapping for (B, N): G lanes per rollout x PPL points per lane (rollout_fwd_kernel.h's header comment).
struct LaneMap { int G, PPL; };
// the forward's mapping: the descriptor's choice, or the articulated kernels' (the rows of Fs / Ff hold G * PPL point slots)
LaneMap fwd_lane_map(const MfRolloutDesc* d, bool joints);

// the forms of the component-parallel backward (rollout_bwd_cp_kernel.h MODE): recompute early / late, the forward's record read by the
// computing wave itself, or streamed through LDS by two more waves
enum { kCpEarly = 0, kCpLate = 1, kCpSaved = 2, kCpStream = 3 };

enum FwdFamily {
  kFwdGeneral,      // reference-order arithmetic (rollout_fwd.hip): float64, float32 MF_MATH_EXACT; rigid or articulated
  kFwdJointsFast,   // rollout_fwd_joints_fast.hip
  kFwdFast,         // rollout_fwd_fast.hip
  kFwdSplit,        // rollout_fwd_split_fast.hip
  kFwdZmu,          // rollout_fwd_zmu_fast.hip
  kFwdCost,         // rollout_fwd_cost.hip
  kFwdCp,           // component-parallel: rollout_fwd_cp_fast.hip, rollout_fwd_cp_f64.hip
  kFwdMwRecF64      // rollout_mw_f64.hip
};
enum { kLossNone = 0, kLossInLaunch = 1, kLossValueInBackward = 2 };

// what the forward's planner reads of MfRolloutFwdBufs: which buffers are there, and the low address bits the alignment rules test
struct FwdBits {
  bool joints, cost_rows, forces, xds, omegas, xraw, rec, zmu, zmu_scratch, mu;
  bool loss, loss_complete, loss_out;      // MfRolloutLoss: given; T2, gt, row_w, partial, ticket and loss all set; loss set
  int loss_flags, loss_T2;
  unsigned rec_low, zmu_low;               // rec & 31; (zmu | zmu_scratch) & 15
};
struct FwdRoute {
  int rc;                  // MF_OK, or the refusal's code with its text in msg
  const char* msg;
  FwdFamily family;
  LaneMap m;
  int block;               // workgroup size
  int chunk_B;             // rollouts per launch (kFwdGeneral .. kFwdCost without a record go out in chunks of so many)
  int touch_lo, touch_hi;  // the controls of a chunk are read once in front of it when it holds touch_lo .. touch_hi rollouts
  bool forces, split, record, zmu, interleave;      // interleave: zmu comes from the pass into zmu_scratch, not from the caller's pair
  int cost;                // 0: output rows; 1: cost rows; 2: cost rows with the projected rotation row
  int loss;                // kLoss*
};
FwdRoute plan_fwd(const MfRolloutDesc* d, int scalar_bytes, const FwdBits& p);

enum BwdFamily {
  kBwdGeneral,      // reference-order arithmetic (rollout_bwd.hip)
  kBwdJoints,       // rollout_bwd_joints.hip, rollout_bwd_joints_fast.hip (float32 MF_MATH_FAST)
  kBwdFast,         // rollout_bwd_fast.hip
  kBwdCarry,        // rollout_bwd_carry_fast.hip
  kBwdXs,           // rollout_bwd_xs_fast.hip and its _win / _loss / _win_loss siblings
  kBwdXsPpl,        // rollout_bwd_xs_ppl_fast.hip
  kBwdCp,           // component-parallel: rollout_bwd_cp_fast.hip, rollout_bwd_dyn_cp_fast.hip, the two _stream_ units, the _f64 builds
  kBwdMw            // rollout_bwd_mw_fast.hip, rollout_mw_f64.hip
};
struct BwdBits {
  bool joints, rec, zmu, zmu_scratch, mu, zeros;
  bool gXs, gXds, gRs, gOmegas, gFs, gFf;
  bool loss, loss_near_w, loss_rows, loss_value;      // MfRolloutLoss: given; near and w set; T2, gt, row_stamp, row_w, gloss, Xs set; partial, ticket, loss set
  int loss_flags, loss_T2;
  unsigned rec_low, zmu_low;
};
struct BwdRoute {
  int rc;
  const char* msg;
  BwdFamily family;
  LaneMap m;
  unsigned grid, block;
  bool fast;               // kBwdJoints: the fast-math build
  bool xs_only, record, zmu, interleave, loss;
  bool win, carry;         // kBwdXs / kBwdCp: the LDS gradient window; kBwdXs with it: accumulator carry-over (512 threads)
  int cp_mode;             // kBwdCp: kCp*
  int ring_slots;          // ... kCpStream: 12 or 6
  bool one1;               // ... the fused loss of the one-wave forms
  bool tile;               // kBwdMw: LDS gradient tiles
};
BwdRoute plan_bwd(const MfRolloutDesc* d, int scalar_bytes, const BwdBits& p);

}  // namespace mf
