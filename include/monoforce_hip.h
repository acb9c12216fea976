/*
 * monoforce_hip.h -- C ABI of libmonoforce_hip.so (gfx950 / MI355X).
 *
 * The drop-in boundary of the MonoForce hot path.  Every entry point takes plain device pointers, sizes and a
 * HIP stream (as void*); nothing here knows about torch.  All launches are asynchronous on the given stream; no
 * entry point synchronises or allocates.  Return value: MF_OK or an MF_ERR_* code (text via mf_last_error()).
 *
 * Reference interfaces replaced (paths under /root/reference/monoforce/src/monoforce/models/):
 *   mf_rollout_fwd_*   traj_predictor/dphysics.py:530-594  DPhysics.dphysics()  = forward_kinematics (:172-272)
 *                      + dynamics (:467-497) / dynamics_odeint (:499-528) + interpolate_grid (:385-455)
 *                      + update_joints (:326-358); in path-cost mode also the reductions the planning nodes apply to its
 *                      outputs (monoforce_ros/nodes/monoforce_node.py:91, diff_physics.py:263-266)
 *   mf_rollout_bwd_*   the autograd graph the reference builds through the same functions (loss.backward(),
 *                      scripts/fit_terrain.py:53-62, scripts/train.py:399-406)
 *   mf_bev_splat_*     terrain_encoder/lss.py:238-280 LiftSplatShoot.voxel_pooling() + terrain_encoder/utils.py:144-181
 *                      (cumsum_trick / QuickCumsum forward and backward)
 *   mf_bev_lift_splat_*  the same with the lift of lss.py:63-71 (depth distribution x context features) fused in
 *   mf_physics_loss_*  losses.py:102-127 physics_loss (position term) and its gradient, on the nearest-time-stamp
 *                      subset of the predicted poses
 *   mf_pose_loss_*     losses.py:102-138 physics_loss(rotation_loss=True): the position term and the geodesic rotation term
 *                      (rotation_difference, :48-65) in one launch, and their gradients in another
 *   mf_bev_splat_prepare_cameras  the voxel plan straight from the camera models: LiftSplatShoot.get_geometry()
 *                      (lss.py:204-224) evaluated inside the key pass
 */
#ifndef MONOFORCE_HIP_H
#define MONOFORCE_HIP_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

enum {
  MF_OK = 0,
  MF_ERR_INVALID = 1,     /* bad argument (shape / null pointer / enum) */
  MF_ERR_UNSUPPORTED = 2, /* valid request outside what the kernels cover (e.g. > 512 contact points) */
  MF_ERR_LAUNCH = 3       /* HIP reported an error at launch */
};

/* Integrators of DPhysics (dphys_config.py:150-153). */
enum {
  MF_INTEG_DYNAMICS = 0,    /* use_odeint=False: dynamics() -- semi-implicit Euler + Rodrigues, records state AFTER each step */
  MF_INTEG_ODEINT_EULER = 1 /* use_odeint=True (reference default): torchdiffeq fixed-grid explicit Euler on the
                               extended state; output 0 = initial state; "forces" are running impulses */
};

/* Output layout.  The reference's default path returns permuted views of time-major tensors (dphysics.py:515-526),
 * its dynamics() path returns contiguous [B,T,...] stacks (dphysics.py:490-495).  Both are supported; time-major lets a
 * wavefront's per-step stores land in one contiguous segment. */
enum {
  MF_LAYOUT_BATCH_MAJOR = 0, /* X[b][t][...] */
  MF_LAYOUT_TIME_MAJOR = 1   /* X[t][b][...] */
};

/* Arithmetic of the float32 kernels (float64 is always exact). */
enum {
  MF_MATH_EXACT = 0, /* IEEE divide/sqrt, libm exp/sincos, no FMA contraction: the reference's eager op sequence, bit-for-bit
                        for the first ~100 steps of a rollout */
  MF_MATH_FAST = 1   /* hardware rcp/rsq/exp2 (1 ulp) + FMA: ~1.5x faster per step; same parity tolerances hold */
};

/* MfRolloutDesc.points_per_lane, besides 0 / 1 / 4: the component-parallel mapping -- a rollout over a 16-lane row, four lanes
 * per contact point (lane = vector component / footprint cell).  float32 MF_MATH_FAST rigid bodies of <= 4 points, full or
 * states-only outputs, BOTH integrators (forward and backward); with points_per_lane = 0 it is chosen by itself for small
 * launches (forward: up to 1024 waves = B <= 4096, backward: up to 2048 waves = B <= 8192), where a step costs ~2x fewer
 * instructions per wave than one point per lane.  Other configurations fall back to the automatic choice. */
enum { MF_LANES_COMPONENT = 16 };

/* Shapes and physical constants of one rollout launch.  Scalars are double here and are rounded ONCE to the
 * kernel's arithmetic type, like the Python floats of DPhysConfig are when they meet a tensor. */
typedef struct MfRolloutDesc {
  int32_t B;          /* rollouts */
  int32_t T;          /* grid points N_ts = outputs per rollout (dphysics.py:573) */
  int32_t N;          /* contact points (cfg.robot_points.shape[0]) */
  int32_t H, W;       /* grid size; flat index = iy + H*ix, first grid axis = x (dphysics.py:427-430) */
  int32_t n_tracks;   /* len(cfg.driving_parts): 2 or 4 (dphysics.py:75-104) */
  int32_t integrator; /* MF_INTEG_* */
  int32_t layout;     /* MF_LAYOUT_* of all outputs */
  int32_t map_shared; /* 1: z/mu are one [H,W] map shared by all rollouts; 0: [B,H,W] */
  int32_t block;      /* threads per workgroup: 0 = default (64); otherwise 64, 128 or 256.  Ignored where one rollout
                         spans a whole workgroup (bodies of 65..512 points at small batch sizes: 128, 256 or 512 threads) */
  int32_t skip_snap;  /* 1: do NOT move x0.z onto the terrain first (dphysics.py:567-571) -- for continuing a rollout
                         from a mid-trajectory state (chunked horizons, teacher-forced single steps) */
  int32_t points_per_lane; /* lane mapping: 0 = choose from B and N; 1 = one contact point per lane (fewest instructions per
                         wave, best when the launch is latency-bound); 4 = four points per lane (least redundant work,
                         best when the chip is full).  Results differ only in float summation order.  With 0 or 1, bodies of
                         65..512 points are spread over 2, 4 or 8 waves per rollout while the launch has <= 2048 waves. */
  int32_t math_mode;    /* MF_MATH_* */
  int32_t force_stride; /* point slots per row of the Fs / Ff buffers, >= mf_rollout_force_stride(desc); 0 means N
                           (only valid when N is a multiple of the lane tile, e.g. N = 4).  Padding slots get zeros. */
  int32_t grad_copies;  /* backward, shared map only: number of private copies of the gz / gmu maps (rollout b scatters into
                           copy b % grad_copies -- the LDS-window kernels: a workgroup's window into copy workgroup % grad_copies; the caller sums the copies).  Thousands of rollouts of one batch cross the
                           same cells, and same-address float atomics serialise in L2 at ~20 ns each; 0 or 1 = one copy.
                           Measured: 32 copies for bodies of up to 4 points (~64 rollouts per copy beyond 2048 rollouts), at least
                           64 for larger bodies, whose points sit on nearly the same cells in every rollout of a batch
                           (1024 rollouts x 32 points: backward 0.98 ms at 16 copies, 0.81 ms at 64). */
  int32_t has_joints;   /* 1: MfRolloutFwdBufs.joint_angles will be given (selects the articulated kernels / force stride) */
  int32_t pose_stride;  /* path-cost mode (MfRolloutFwdBufs.cost_rows): Xs / Rs keep every pose_stride-th output row; else 0 */
  int32_t cost_project; /* path-cost mode, MF_INTEG_ODEINT_EULER: 1 = the cost rows carry the third row of the NEAREST ROTATION to
                           the (drifting) R -- what scipy's Rotation.from_matrix(R).as_euler() reads roll / pitch from
                           (diff_physics.py:263-266); 0 = the raw third row (enough for the force cost; ~20 % faster) */
  int32_t default_state; /* forward only: 1 = start from the reference's default state (dphysics.py:554-559: x = 0,
                           xd = (v_0, 0, 0), R = I, omega = (0, 0, w_0) with (v_0, w_0) = controls[b][0]); the kernel computes it
                           and WRITES x0 / xd0 / R0 / w0 (for the caller and the backward pass) instead of reading them --
                           saves the separate mf_rollout_default_state_* launch */
  int32_t controls_stride_b, controls_stride_t; /* forward only: element strides of `controls` over rollouts and over time
                           ((v, w) stay adjacent); both 0 = contiguous [B][T][2].  controls_stride_t = 0 reads ONE (v, w) per
                           rollout for the whole horizon -- the constant-in-time samples of trajectory shooting
                           (generate_controls, dphysics.py:42-72; monoforce_node.py:41-52) as the [B,1,2] tensor they are,
                           instead of a materialised [B,T,2] copy that every step of every rollout would fetch from HBM */
  double mass, gravity, stiffness, damping, omega_max;
  double grid_res, d_max;
  double dt;           /* cfg.dt: step of MF_INTEG_DYNAMICS (ODEINT takes its steps from ts[]) */
  double robot_size_y; /* Ly = cfg.robot_size[1] */
  double Iinv[9];      /* inverse body inertia, row-major (dphysics.py:152-153) */
  double joint_xyz[12]; /* joint positions of the 4 driving parts [fl, fr, rl, rr][xyz] (cfg.joint_positions); has_joints only */
} MfRolloutDesc;

/* physics_loss (losses.py:102-127: time-discounted position MSE at the output rows nearest to the ground-truth stamps) INSIDE the
 * rollout kernels: the forward accumulates  mean_{b,j,c} (Xs[b, near[j], c] w_j - gt[b, j, c] w_j)^2  at the
 * <= T2 stamped rows while it writes them, and the backward synthesises dL/dXs at those rows from Xs and gt instead of reading a
 * [T][B][3] gradient tensor -- a train step loses two launches and 6 MB of rows.  Float32, component-parallel kernels with the
 * streaming backward only: ask mf_rollout_loss_fusable(desc).  The ground-truth stamps must be the SAME for every rollout
 * (near / w / row_stamp are per stamp, not per rollout) and `near` strictly increasing. */
/* MfRolloutLoss.flags.  MF_LOSS_VALUE_IN_BACKWARD: a caller that ALWAYS runs the backward after the forward (a train step) lets the
 * backward form the loss VALUE as well -- its fetching waves hold Xs, the ground truth and the weight of every stamped row anyway and
 * have issue slots to spare, the forward (one wave per SIMD, issue-bound) has none: the forward then only marks loss[0] as not yet
 * known (NaN; needs `loss` alone), the backward fills it (needs partial, ticket, loss besides gloss / Xs / the tables).  One launch
 * and ~10 us less per step than forming the value in a launch of its own. */
#define MF_LOSS_VALUE_IN_BACKWARD 1
typedef struct MfRolloutLoss {
  int32_t T2;               /* ground-truth stamps per rollout */
  int32_t flags;            /* 0, or MF_LOSS_VALUE_IN_BACKWARD */
  const void* gt;           /* S[B][T2][3] ground-truth positions */
  const int32_t* near;      /* int32[T2]: output row nearest in time to stamp j (losses.py:116), strictly increasing, < T */
  const void* w;            /* S[T2]: time weights 1 / (1 + gamma t_j) (losses.py:122) */
  const int32_t* row_stamp; /* int32[T]: stamp index j of output row t, -1 where the row carries none (the inverse of `near`) */
  const void* row_w;        /* S[T]: w[row_stamp[t]], 0 where the row carries no stamp (the kernels read the stamps through the two
                               row tables; near / w document them and serve mf_physics_loss_* callers) */
  void* partial;            /* scratch of the direction that forms the value: S[ceil(B / 4)] per-workgroup partial sums */
  uint32_t* ticket;         /* the same direction: ONE zero-initialised counter; the launch leaves it zero again */
  void* loss;               /* out: S[1], the mean over B x T2 x 3 (written by the forward, or by the backward: flags) */
  const void* gloss;        /* backward: S[1] upstream gradient of the loss (device scalar) */
  const void* Xs;           /* backward: the forward's Xs rows (shifted positions, layout of the launch) */
} MfRolloutLoss;

/* Device buffers of the forward rollout; S = float for _f32, double for _f64.  All contiguous. */
typedef struct MfRolloutFwdBufs {
  const void* z;        /* S[map_shared ? 1 : B][H][W] height map */
  const void* mu;       /* same shape friction map, or NULL = all ones (cfg.friction, dphysics.py:562) */
  const void* controls; /* S[B][T][2] = (v, w) */
  const void* ts;       /* S[T] time grid (dphysics.py:167,581); only its differences are used (ODEINT) */
  const void* points;   /* S[N][3] body-frame contact points */
  const int32_t* part;  /* int32[N]: index of the LAST driving mask holding the point, -1 = not driving (:242-246) */
  void* x0;             /* S[B][3] IN/OUT: z component is overwritten with the terrain height under the robot (:567-571) */
  const void* xd0;      /* S[B][3] */
  const void* R0;       /* S[B][3][3] */
  const void* w0;       /* S[B][3] */
  void* Xs;             /* S[..][3]   positions, already shifted by R[:,2]*m*g/(k+1e-6) (:587-589) */
  void* Xds;            /* S[..][3]   */
  void* Rs;             /* S[..][3][3]*/
  void* Omegas;         /* S[..][3]   */
  void* Fs;             /* S[..][force_stride][3] spring forces (DYNAMICS) or their running impulses (ODEINT).  Fs and Ff
                           may both be NULL for float32 MF_MATH_FAST rigid-body rollouts: states-only kernels that skip
                           24 N of the 80 + 56 N bytes per step (training consumes only the states, scripts/train.py:243) */
  void* Ff;             /* S[..][force_stride][3] friction forces / impulses */
  void* Xraw;           /* optional S[..][3]: unshifted positions saved for the backward pass; may be NULL */
  const void* joint_angles; /* optional S[B][T][4] flipper angles: each driving part is rotated about the y-axis through
                           its joint and the body inertia recomputed EVERY step (update_joints, dphysics.py:192-197,
                           326-358; the reference does this for robot == 'marv' and non-zero angles).  All six
                           outputs must be given.  NULL = rigid body. */
  void* cost_rows;      /* optional S[T][B][4], float32 MF_MATH_FAST + MF_LAYOUT_TIME_MAJOR rigid-body rollouts: PATH-COST mode
                           for trajectory shooting.  Per output row the kernel writes (R[2][0], R[2][1], R[2][2], s) (see
                           desc->cost_project) with
                           s = unbiased std over the N contact points of |F_spring row| -- the inputs of the reference's
                           path costs (monoforce_node.py:91 `norm(F_springs).std(points).std(time)`; diff_physics.py:263-266
                           roll / pitch) -- instead of the full rows: Xds, Omegas, Fs, Ff, Xraw must be NULL, and Xs / Rs are
                           DECIMATED to S[1 + ceil((T-1) / pose_stride)][B][3 | 3x3]: pose row r holds output row
                           min(r * pose_stride, T - 1) (what the nodes publish: poses[::pose_step], plus the final pose). */
  void* path_cost;      /* optional S[B], with cost_rows: the force path cost itself, std over the T rows of s (unbiased, Welford
                           in registers) = norm(F_springs, dim=-1).std(dim=-1).std(dim=-1) of monoforce_node.py:91 */
  void* zmu_scratch;    /* optional scratch, 2*H*W floats (8-byte aligned): with a SHARED map (desc->map_shared), float32
                           MF_MATH_FAST, a rigid body of <= 64 contact points and >= 512 waves of rollouts the entry point first interleaves z and mu
                           into it, cell by cell, and the rollout kernel reads a point's footprint in both maps with two
                           16-byte loads instead of eight 4-byte ones (the L1 looks up one line per lane and cycle: at
                           >= 16 k rollouts that bounds the kernel).  Same results, bit for bit.  Contents are undefined
                           afterwards; NULL (or any other configuration) = the maps are read where they are. */
  const void* zmu;      /* optional, float32: the SHARED maps already interleaved, S[H][W][2] = (z, mu) per cell, holding the same
                           values as z / mu (mf_terrain_stage_fwd_f32 writes all three in one pass).  Kernels that gather from an
                           interleaved pair (float32 MF_MATH_FAST, rigid body of <= 64 points, one point per lane or component-
                           parallel) read it whatever the batch size and skip their own interleave pass; the others read z / mu. */
  void* rec;            /* optional, float32: mf_rollout_record_bytes(desc) bytes (16-byte aligned) that receive the forward's per-step
                           record for a backward that then reads it instead of recomputing (autograd saves every intermediate of
                           dphysics.py:172-272).  Two forms, chosen by the launch shape:
                           component-parallel kernels (rigid body of <= 4 points): [T][B * 16 lanes] quads (u, c, omega_d raw, A) --
                           cell coordinate, contact weight, unclamped angular acceleration component, A = k dh + d v_n -- 256 B per
                           rollout-step;
                           one point per lane, bodies of 5..512 points, either integrator, up to two waves per SIMD: [T][B] quads
                           (sum of the contact weights, omega_d before its clamp) -- 16 B per rollout-step, what the record-reading
                           backward (rollout_bwd_mw_kernel.h) cannot rebuild without a reduction over the contact points.
                           NULL, or a launch the record does not apply to: nothing is written and the backward recomputes. */
  const MfRolloutLoss* loss; /* optional: fuse physics_loss into the launch (mf_rollout_loss_fusable(desc) must be 1; Fs = Ff = NULL,
                           MF_LAYOUT_TIME_MAJOR): fills loss->loss.  NULL = plain rollout. */
} MfRolloutFwdBufs;

/* Can this launch carry the fused physics loss (MfRolloutLoss)?
 *   1  BOTH directions, on the component-parallel kernels with the streaming backward: float32 MF_MATH_FAST, rigid body of <= 4 points,
 *      time-major outputs, few enough rollouts (<= 2048; dynamics(): <= 1024).  The value: from the forward launch (default integrator),
 *      from the backward launch (MF_LOSS_VALUE_IN_BACKWARD), or from mf_physics_loss_value_* on the written rows.
 *   2  the BACKWARD of a saturated launch (round 6): the positions-only one-point-per-lane kernels (float32 MF_MATH_FAST, rigid body of <= 64
 *      points, time-major, beyond the component-parallel / record-reading ranges: > 8192 rollouts of a 4-point body) form dL/dXs at the
 *      stamped rows themselves -- pass MfRolloutBwdBufs.loss and NO MfRolloutFwdBufs.loss; the value comes from mf_physics_loss_value_* on
 *      the forward's rows or, with MF_LOSS_VALUE_IN_BACKWARD, from the backward launch (partial: S[B], near and w required).  The step loses the loss-gradient launch and the dense [T][B][3] gradient (98 MB at
 *      16 384 rollouts, a tenth of its rows non-zero).
 *   3  the BACKWARD of a component-parallel launch in its early-recompute form (no record, more than one wave per SIMD: 4097 .. 8192
 *      rollouts of a <= 4-point body, either integrator; round 6): as 2 -- MfRolloutBwdBufs.loss with near and w, no MfRolloutFwdBufs.loss --
 *      without MF_LOSS_VALUE_IN_BACKWARD (the value: mf_physics_loss_value_*).  The other one-wave launches (2049 .. 4096 rollouts;
 *      dynamics() from 1025) answer 0: there the fused kernel loses what the two loss launches cost (profiles/r6_ab_one_wave_loss.txt).
 *   0  neither: run mf_physics_loss_* on the outputs. */
int mf_rollout_loss_fusable(const MfRolloutDesc* desc);

/* 1 where mf_rollout_bwd_f32 with a positions-only upstream (gXs or a fused loss; the other five NULL) sends the cell gradients of this
 * launch through per-workgroup LDS windows (saturated launches of a <= 4-point body on ONE shared power-of-two map pair): a workgroup
 * adds its window to gradient copy blockIdx % grad_copies once, at its end, so desc->grad_copies may stay small (64) -- the caller's
 * reduction over the copies (mf_reduce_grad_copies_*) is what grows with them: 0.125 ms at 256 copies of a 256 x 256 pair. */
int mf_rollout_bwd_window(const MfRolloutDesc* desc);

/* Bytes of MfRolloutFwdBufs.rec / MfRolloutBwdBufs.rec for this launch shape; 0 where the kernels chosen for it keep no record
 * (then pass NULL).  The record pays while the launch is bound by the instruction stream of its waves: few rollouts of a small
 * body (forward +5 %, backward -17 % at 1024 rollouts x 4 points), and bodies of 5..512 points up to two waves per SIMD
 * (16 bytes per rollout-step; backward 2.05 -> 1.04 ms at 64 rollouts x 223 points, 1.38 -> 0.97 ms at 1024 x 32). */
long long mf_rollout_record_bytes(const MfRolloutDesc* desc);
/* 1 where mf_rollout_fwd_f32, given `zmu_scratch` and no `zmu`, fills the scratch with the interleaved (z, mu) pair (few-point bodies on the
 * component-parallel kernels from half a wave per SIMD up): the caller may hand that buffer to mf_rollout_bwd_f32 as `zmu` for the same
 * step and maps -- the backward then runs no interleave pass of its own. */
int mf_rollout_fwd_stages_zmu(const MfRolloutDesc* desc);
/* The same for the _f64 entry points: non-zero only for the float64 VALIDATION build of the component-parallel kernels
 * (points_per_lane = MF_LANES_COMPONENT: the float32 kernels' source instantiated on double, 32-byte quads), which exists so that the
 * code the BASELINE configurations run can be held to the float64 oracle (dphysics.py:172-272, 467-528 under float64) over the full
 * horizon, where float32 trajectories are chaotic. */
long long mf_rollout_record_bytes_f64(const MfRolloutDesc* desc);

/* Point slots per Fs/Ff row the kernels chosen for (B, N, points_per_lane) need (>= N; -1 on a bad descriptor). */
int mf_rollout_force_stride(const MfRolloutDesc* desc);
int mf_rollout_fwd_f32(const MfRolloutDesc* desc, const MfRolloutFwdBufs* bufs, void* hip_stream);
int mf_rollout_fwd_f64(const MfRolloutDesc* desc, const MfRolloutFwdBufs* bufs, void* hip_stream);

/* The start state DPhysics uses when the caller gives none (dphysics.py:554-559): x = 0, xd = (v_0, 0, 0), R = I,
 * omega = (0, 0, w_0) with (v_0, w_0) = controls[b][0]; one launch.  controls S[B][T][2]; outputs S[B][3], [3], [3][3], [3]. */
int mf_rollout_default_state_f32(int32_t B, int32_t T, const float* controls, float* x0, float* xd0, float* R0, float* w0, void* hip_stream);
int mf_rollout_default_state_f64(int32_t B, int32_t T, const double* controls, double* x0, double* xd0, double* R0, double* w0, void* hip_stream);

/* Device buffers of the backward rollout (reverse-time adjoint of the same scan; per-step intermediates are
 * recomputed from the saved per-step states, which are the forward's own outputs).  `desc` must be the forward's.
 * Upstream gradients use the outputs' layout and may each be NULL (= zeros).  Gradient outputs: gz/gmu are
 * ACCUMULATED with atomic adds (zero them first; S[1 or B][H][W] like z/mu); the others are overwritten. */
typedef struct MfRolloutBwdBufs {
  const void* z;        /* as forward */
  const void* mu;       /* as forward (NULL = ones) */
  const void* controls; /* S[B][T][2] */
  const void* ts;       /* S[T] */
  const void* points;   /* S[N][3] */
  const int32_t* part;  /* int32[N] */
  const void* x_init;   /* S[B][3] x0 AFTER the forward's terrain snap (the forward's in/out x0 buffer) */
  const void* xd0;      /* S[B][3] */
  const void* R0;       /* S[B][3][3] */
  const void* w0;       /* S[B][3] */
  const void* Xraw;     /* saved forward outputs: unshifted positions, */
  const void* Xds;      /*   velocities, */
  const void* Rs;       /*   rotations, */
  const void* Omegas;   /*   angular velocities */
  const void* gXs;      /* upstream dL/dXs (the SHIFTED positions the API returned) ... */
  const void* gXds;
  const void* gRs;
  const void* gOmegas;
  const void* gFs;
  const void* gFf;
  const void* zeros;    /* >= 9 zero scalars of type S; required when any of the six upstream pointers is NULL */
  void* gz;             /* out (atomic accumulate): dL/dz, S[map_shared ? max(grad_copies,1) : B][H][W] */
  void* gmu;            /* out (atomic accumulate): dL/dmu, same shape; NULL to skip */
  void* gcontrols;      /* out: S[B][T][2]; may be NULL = gradient not wanted (round 6: every kernel; before, only where
                           mf_rollout_bwd_wants_gcontrols(desc) returned 0) -- 8 B per rollout-step of stores less */
  void* gx0;            /* out: S[B][3] (z component is 0 unless skip_snap); NULL to skip */
  void* gxd0;           /* out: S[B][3] */
  void* gR0;            /* out: S[B][3][3] */
  void* gw0;            /* out: S[B][3] */
  const void* joint_angles; /* the forward's S[B][T][4] flipper angles (desc->has_joints), else NULL */
  void* gjoint_angles;      /* out: dL/d(joint_angles), S[B][T][4], through update_joints AND the per-step inertia
                               (dphysics.py:191-197, 326-358); NULL to skip.  Rows the scheme never reads (the last one of the
                               default integrator) are not written: hand in zeros. */
  const void* rec;          /* the record the forward wrote (MfRolloutFwdBufs.rec of the same desc), or NULL: recompute */
  const MfRolloutLoss* loss; /* the forward's fused physics loss (then all six upstream pointers are NULL: the kernel forms dL/dXs
                               itself from loss->Xs, gt, w and gloss), or NULL */
  void* zmu_scratch;        /* optional scratch, 2*H*W floats (8-byte aligned), as MfRolloutFwdBufs.zmu_scratch: with a SHARED float32 map
                               pair the record-reading backward (two to four waves of rollouts per CU) re-gathers a cell's (z, mu)
                               with ONE 8-byte load from an interleaved copy it stages here (B = 4096: 0.45 -> 0.40 ms) */
  const void* zmu;          /* optional, float32: the SHARED maps already interleaved (MfRolloutFwdBufs.zmu of the same step) */
} MfRolloutBwdBufs;

/* 1 if the backward kernels chosen for this descriptor always write the control gradient (gcontrols must then be a buffer), 0 if
 * they can skip it (gcontrols may be NULL).  Round 6: 0 for every descriptor -- the component-parallel kernels compile the gradient out
 * (its dot product, sums and stores), the others keep their instruction stream and drop the stores' traffic. */
int mf_rollout_bwd_wants_gcontrols(const MfRolloutDesc* desc);
int mf_rollout_bwd_f32(const MfRolloutDesc* desc, const MfRolloutBwdBufs* bufs, void* hip_stream);
int mf_rollout_bwd_f64(const MfRolloutDesc* desc, const MfRolloutBwdBufs* bufs, void* hip_stream);

/* ---- LSS BEV voxel pooling (lss.py:238-280) ------------------------------------------------------------------
 * Points are the B * n_per_sample frustum points of a batch (n_per_sample = cams * D * fH * fW), in the reference's
 * flattening order; features are row-major [point][C]; the output is the reference's [B][nz*C][nx][ny] grid
 * (channel index = iz*C + c, lss.py:274-278).  Voxel index = trunc((geom - off) / dx) in float32 with
 * off = bx - dx/2 (lss.py:246); points outside [0,n) on any axis are dropped (lss.py:253-255).
 * Usage: workspace = mf_bev_splat_workspace_bytes(desc) bytes of device memory; mf_bev_splat_prepare() once per
 * geometry; then any number of _fwd / _bwd calls with that workspace. */
typedef struct MfSplatDesc {
  int32_t B;            /* samples */
  int32_t n_per_sample; /* frustum points per sample */
  int32_t C;            /* feature channels per point */
  int32_t nx, ny, nz;   /* BEV grid (gen_dx_bx, terrain_encoder/utils.py:136-141) */
  float off[3];         /* bx - dx/2, computed in float32 like the reference */
  float dx[3];          /* voxel size */
  int32_t lift_D;       /* mf_bev_lift_splat_*: depth bins per pixel (D) ... */
  int32_t lift_hw;      /* ... and pixels per camera feature map (fH * fW); n_per_sample = cameras * lift_D * lift_hw.  0 otherwise */
} MfSplatDesc;

size_t mf_bev_splat_workspace_bytes(const MfSplatDesc* desc); /* 0 on a bad descriptor */
int mf_bev_splat_prepare(const MfSplatDesc* desc, const float* geom /* [B*n_per_sample][3] */, void* workspace, void* hip_stream);
/* The same plan from the camera models instead of a geometry tensor: get_geometry (lss.py:204-224) evaluated per point
 * inside the key pass, in the reference's order of float32 operations.  frustum[pts_per_cam][3] = (u, v, d) of
 * create_frustum (lss.py:191-202), pts_per_cam = D*fH*fW, n_per_sample = cameras * pts_per_cam;
 * cams[B*cameras][24] = post_trans[3], inverse(post_rots)[9], (rots x inverse(intrins))[9], trans[3], matrices row-major. */
int mf_bev_splat_prepare_cameras(const MfSplatDesc* desc, const float* frustum, int32_t pts_per_cam, const float* cams,
                                 void* workspace, void* hip_stream);
/* The same plan straight from the calibration tensors LiftSplatShoot.forward receives (lss.py:282-296): rots, intrins, post_rots
 * [B*cameras][3][3] and trans, post_trans [B*cameras][3], float32 row-major -- BOTH 3 x 3 inversions of get_geometry (lss.py:212, 218:
 * torch.inverse(post_rots), torch.inverse(intrins)) and the product rots x inverse(intrins) are formed inside the key kernel (float64
 * adjugate rounded once to float32), so a data loader with per-sample augmentation (terrain_encoder/utils.py:110-133) pays no
 * torch.inverse -- two LU launches and a host synchronisation -- per step.  For diagonal-plus-translation intrinsics and scale / flip /
 * crop augmentations the inverse is exact up to one rounding per entry and the keys equal mf_bev_splat_prepare_cameras' bit for bit;
 * an in-plane rotation (rot_lim) makes the two differ in the last bit of some entries, which moves a point only if it lies within
 * ~1e-6 voxel of a voxel face (tests/test_splat_gpu.py). */
int mf_bev_splat_prepare_rig(const MfSplatDesc* desc, const float* frustum, int32_t pts_per_cam, const float* rots, const float* trans,
                             const float* intrins, const float* post_rots, const float* post_trans, void* workspace, void* hip_stream);
/* out[B][nz*C][nx][ny] = per-voxel sums of x[B*n_per_sample][C]; every output element is written (zeros where empty) */
int mf_bev_splat_fwd_f32(const MfSplatDesc* desc, const float* x, const void* workspace, float* out, void* hip_stream);
int mf_bev_splat_fwd_f64(const MfSplatDesc* desc, const double* x, const void* workspace, double* out, void* hip_stream);
/* gx[B*n_per_sample][C] = gout at the point's voxel, 0 for dropped points (QuickCumsum.backward, utils.py:174-181) */
int mf_bev_splat_bwd_f32(const MfSplatDesc* desc, const float* gout, const void* workspace, float* gx, void* hip_stream);
int mf_bev_splat_bwd_f64(const MfSplatDesc* desc, const double* gout, const void* workspace, double* gx, void* hip_stream);

/* The lift fused into the splat (lss.py:63-71 + :238-280): point p = ((cam * D + d) * fHW + pixel) carries
 * depth[p] * ctx[cam * fHW + pixel][0..C) without the [points][C] tensor ever being materialised.
 *   depth  S[B*cameras][D][fH][fW]   softmax depth distribution (= point order)
 *   ctx    S[B*cameras][fH][fW][C]   context features, PIXEL-major
 * fwd: out[B][nz*C][nx][ny] as mf_bev_splat_fwd.  bwd: g_depth (like depth), g_ctx (like ctx); rows_scratch = S[B*nz*nx*ny][C]
 * (the BEV gradient re-laid voxel-major for the occupied tiles).  Same prepared workspace as the plain splat. */
int mf_bev_lift_splat_fwd_f32(const MfSplatDesc* desc, const float* depth, const float* ctx, const void* workspace, float* out, void* hip_stream);
int mf_bev_lift_splat_fwd_f64(const MfSplatDesc* desc, const double* depth, const double* ctx, const void* workspace, double* out, void* hip_stream);
int mf_bev_lift_splat_bwd_f32(const MfSplatDesc* desc, const float* depth, const float* ctx, const void* workspace, const float* gout,
                              float* rows_scratch, float* g_depth, float* g_ctx, void* hip_stream);
int mf_bev_lift_splat_bwd_f64(const MfSplatDesc* desc, const double* depth, const double* ctx, const void* workspace, const double* gout,
                              double* rows_scratch, double* g_depth, double* g_ctx, void* hip_stream);

/* ---- fused physics loss (losses.py:102-127) -------------------------------------------------------------------
 * loss = mean_{b,j,c} ((Xs[b, nearest[b,j], c] - Xgt[b,j,c]) * w[b,j])^2,  w = 1 / (1 + gamma * gt_ts[b,j]).
 * Xs is addressed as Xs[b*x_stride_b + t*x_stride_t + c] (elements), so both rollout output layouts work in place.
 * _fwd writes ceil(B*T2/256) per-workgroup partial sums (loss = sum(partial) / (B*T2*3)); _bwd writes d loss/d Xs into a gXs that is ZERO on entry (same
 * strides as Xs; stamps of one rollout that share a step add up, a step one stamp has to itself is stored) given the upstream scalar gradient gloss[0]. */
typedef struct MfLossDesc {
  int32_t B, T1, T2;            /* rollouts, predicted steps, ground-truth stamps */
  int32_t reserved;
  int64_t x_stride_b, x_stride_t;
  double gamma;
} MfLossDesc;
int mf_physics_loss_fwd_f32(const MfLossDesc* desc, const float* Xs, const float* Xgt, const float* gt_ts, const int32_t* nearest, float* partial, void* hip_stream);
int mf_physics_loss_fwd_f64(const MfLossDesc* desc, const double* Xs, const double* Xgt, const double* gt_ts, const int32_t* nearest, double* partial, void* hip_stream);
int mf_physics_loss_bwd_f32(const MfLossDesc* desc, const float* Xs, const float* Xgt, const float* gt_ts, const int32_t* nearest, const float* gloss, float* gXs, void* hip_stream);
int mf_physics_loss_bwd_f64(const MfLossDesc* desc, const double* Xs, const double* Xgt, const double* gt_ts, const int32_t* nearest, const double* gloss, double* gXs, void* hip_stream);
/* nearest[b][j] = argmin_t |pred_ts[b][t] - gt_ts[b][j]|, the first minimum (losses.py:116 `torch.argmin(torch.abs(pred_ts.unsqueeze(1) -
 * gt_ts.unsqueeze(2)), dim=2)`): the index table the entry points above take, without the two [B,T2,T1] temporaries of the reference's
 * form.  pred_ts rows of T1, gt_ts rows of T2 stamps, row strides in elements (0 = one row shared by all rollouts); nearest int32[B][T2]. */
int mf_nearest_steps_f32(int32_t B, int32_t T1, int32_t T2, const float* pred_ts, long long pred_stride_b, const float* gt_ts, long long gt_stride_b, int32_t* nearest, void* hip_stream);
int mf_nearest_steps_f64(int32_t B, int32_t T1, int32_t T2, const double* pred_ts, long long pred_stride_b, const double* gt_ts, long long gt_stride_b, int32_t* nearest, void* hip_stream);
/* The same loss, finished inside the launch: `loss[0]` receives the mean (what `partial.sum() / (3 B T2)` gives, summed in block
 * order).  `partial` holds ceil(B*T2/256) scalars of scratch; `ticket` is ONE zero-initialised uint32 the library resets itself --
 * reusable launch after launch by calls ordered on one stream (two streams need two tickets).  `zero_fill` (may be NULL): a buffer
 * of `zero_count` scalars cleared by the same launch -- the gXs a later mf_physics_loss_bwd_* scatters into. */
int mf_physics_loss_value_f32(const MfLossDesc* desc, const float* Xs, const float* Xgt, const float* gt_ts, const int32_t* nearest, float* partial, uint32_t* ticket, float* loss, float* zero_fill, long long zero_count, void* hip_stream);
int mf_physics_loss_value_f64(const MfLossDesc* desc, const double* Xs, const double* Xgt, const double* gt_ts, const int32_t* nearest, double* partial, uint32_t* ticket, double* loss, double* zero_fill, long long zero_count, void* hip_stream);
/* ---- fused pose loss: physics_loss(..., rotation_loss=True) (losses.py:102-138, rotation_difference :48-65) ----------------------
 * The call scripts/eval.py:151-153 makes on every batch.  With near = nearest[b,j], w = 1 / (1 + gamma * gt_ts[b,j]):
 *   loss[0] = mean_{b,j,c} ((Xs[b,near,c] - Xgt[b,j,c]) * w)^2                                   (the mf_physics_loss_* term, same arithmetic)
 *   loss[1] = mean_{b,j} theta^2 * w,  theta = acos(clip((tr - 1) / 2, -1, 1)),  tr = sum_{r,k} Rs[b,near,r,k] * Rgt[b,j,r,k] = trace(Rp Rg^T)
 * Xs is addressed as Xs[b*x_stride_b + t*x_stride_t + c], Rs as Rs[b*r_stride_b + t*r_stride_t + 3*r + k] (elements): the rollout's
 * time-major [T,B,3,3] buffers viewed as [B,T,3,3] and dense [B,T,3,3] tensors work in place.  Xgt [B][T2][3], Rgt [B][T2][3][3],
 * gt_ts [B][T2], nearest int32 [B][T2] (values in [0, T1)) are dense.  B * T2 must be below 2^31. */
typedef struct MfPoseLossDesc {
  int32_t B, T1, T2;            /* rollouts, predicted steps, ground-truth stamps */
  int32_t reserved;
  int64_t x_stride_b, x_stride_t;
  int64_t r_stride_b, r_stride_t;
  double gamma;
} MfPoseLossDesc;
/* losses.py:116-136 (both returned scalars), finished inside the launch like mf_physics_loss_value_*: `partial` holds
 * 2 * ceil(B*T2/256) scalars of scratch, `ticket` is ONE zero-initialised uint32 the library resets itself (calls ordered on one
 * stream may share it, also with mf_physics_loss_value_*), loss[0..1] receive the two means, summed in block order (deterministic).
 * `zero_x` / `zero_r` (each may be NULL with a count of 0): buffers of `zero_*_count` scalars cleared by the same launch -- the gXs /
 * gRs a later mf_pose_loss_bwd_* scatters into. */
int mf_pose_loss_value_f32(const MfPoseLossDesc* desc, const float* Xs, const float* Rs, const float* Xgt, const float* Rgt, const float* gt_ts,
                           const int32_t* nearest, float* partial, uint32_t* ticket, float* loss, float* zero_x, long long zero_x_count,
                           float* zero_r, long long zero_r_count, void* hip_stream);
int mf_pose_loss_value_f64(const MfPoseLossDesc* desc, const double* Xs, const double* Rs, const double* Xgt, const double* Rgt, const double* gt_ts,
                           const int32_t* nearest, double* partial, uint32_t* ticket, double* loss, double* zero_x, long long zero_x_count,
                           double* zero_r, long long zero_r_count, void* hip_stream);
/* The autograd backward of losses.py:116-136 with respect to states_pred[0] and states_pred[2] (the gather's index_put_, the matmul,
 * clip and arccos backward), given the upstream gradients gloss[0..1] of the two scalars.  gXs / gRs have the strides of Xs / Rs and are
 * ZERO on entry; either may be NULL (that half is skipped), not both.  Stamps of one rollout that share a step add up (float atomics),
 * a step one stamp has to itself is stored.
 *   gXs[b,near,c] (+)= gloss[0] * 2 w (Xs w - Xgt w) / (3 B T2)
 *   gRs[b,near,:] (+)= gloss[1] * w / (B T2) * dtheta2 * Rgt[b,j,:],   dtheta2 = -theta / sqrt((1-c)(1+c)) for -1 < c < 1, else 0
 * ONE difference from autograd: at c == +-1 exactly (inside the clip range) torch's arccos backward gives 0 * inf = NaN for identical
 * rotations and inf at exactly pi; here the rotation gradient is 0 there.  For tr outside [-1, 3] both give 0 (clip's mask). */
int mf_pose_loss_bwd_f32(const MfPoseLossDesc* desc, const float* Xs, const float* Rs, const float* Xgt, const float* Rgt, const float* gt_ts,
                         const int32_t* nearest, const float* gloss, float* gXs, float* gRs, void* hip_stream);
int mf_pose_loss_bwd_f64(const MfPoseLossDesc* desc, const double* Xs, const double* Rs, const double* Xgt, const double* Rgt, const double* gt_ts,
                         const int32_t* nearest, const double* gloss, double* gXs, double* gRs, void* hip_stream);
/* ---- height-map losses: hm_loss (losses.py:77-99) and total_variation (losses.py:68-74) ------------------------------------------------
 * Maps are addressed as [M][H][W]: element (m, h, w) of a tensor sits at m*stride_m + h*stride_h + w (elements; unit stride along W), every
 * tensor with its own pair of strides -- `hm_geom[:, 0:1]` / `hm_geom[:, 1:2]` of a [B,2,H,W] label tensor, `terrain['geom'][:, 0]`, a
 * row-strided crop and a plain [H,W] map (M = 1) are read in place.  p_* address the prediction (total variation: the map z), g_* the
 * label, w_* the weights, o_* the gradient a backward entry writes.  M * H * W must be below 2^31.  Every value entry finishes inside
 * its launch like mf_pose_loss_value_*: `partial` holds ceil(M*H*W / 1024) scalars of scratch, `ticket` is ONE zero-initialised uint32
 * the last workgroup resets (calls ordered on one stream may share it, also with mf_physics_loss_value_* / mf_pose_loss_value_*); the
 * partial sums are added in block order: bit-identical from launch to launch.  No entry synchronises or allocates (capturable). */
typedef struct MfMapLossDesc {
  int32_t M, H, W;              /* maps, rows, columns */
  int32_t use_h_max;            /* hm_loss: 1 = the prediction is h_max * tanh(pred) (losses.py:83-86), 0 = as it is (h_max=None) */
  int64_t p_stride_m, p_stride_h;
  int64_t g_stride_m, g_stride_h;
  int64_t w_stride_m, w_stride_h;
  int64_t o_stride_m, o_stride_h;
  double h_max;
} MfMapLossDesc;
/* losses.py:77-99.  Per cell p' = use_h_max ? h_max * tanh(pred) : pred; the cell counts iff neither p' nor gt is NaN (:89);
 *   loss[0] = sum_valid (p'*w - gt*w)^2 / n_valid (:95-97),   n_valid_out[0] = n_valid (an exact count, kept on the device for the backward)
 * `w` may be NULL: all ones (:79-80).  `counts`: ceil(M*H*W / 1024) uint32 of scratch next to `partial`.  n_valid == 0 gives NaN, the
 * reference's mean of an empty selection. */
int mf_hm_loss_value_f32(const MfMapLossDesc* desc, const float* pred, const float* gt, const float* w, float* partial, uint32_t* counts,
                         uint32_t* ticket, float* loss, int32_t* n_valid_out, void* hip_stream);
int mf_hm_loss_value_f64(const MfMapLossDesc* desc, const double* pred, const double* gt, const double* w, double* partial, uint32_t* counts,
                         uint32_t* ticket, double* loss, int32_t* n_valid_out, void* hip_stream);
/* The autograd backward of losses.py:83-97 with respect to height_pred, given the upstream gradient gloss[0] and the count the value
 * entry left in n_valid[0].  EVERY cell of g_pred (its own strides, o_*) is stored, not accumulated: it need not be zero on entry.
 *   valid cells:  g_pred = gloss[0] * 2 w (p'*w - gt*w) / n_valid  [* h_max * (1 - tanh(pred)^2) under use_h_max];   masked cells: 0
 * ONE difference from autograd: under use_h_max a NaN PREDICTION gets the reference's tanh backward 0 * (1 - NaN^2) = NaN at that cell;
 * here it is 0.  Without use_h_max both give 0 there; with every cell masked both give all zeros. */
int mf_hm_loss_bwd_f32(const MfMapLossDesc* desc, const float* pred, const float* gt, const float* w, const int32_t* n_valid,
                       const float* gloss, float* g_pred, void* hip_stream);
int mf_hm_loss_bwd_f64(const MfMapLossDesc* desc, const double* pred, const double* gt, const double* w, const int32_t* n_valid,
                       const double* gloss, double* g_pred, void* hip_stream);
/* losses.py:68-74: loss[0] = (sum |z[m,h,w+1] - z[m,h,w]| + sum |z[m,h+1,w] - z[m,h,w]|) / (H * W).  The differences stay inside each of
 * the M maps and the divisor is H * W whatever M is (:69, :73); H == 1 or W == 1 has no differences along that axis.  Strides: p_*. */
int mf_total_variation_value_f32(const MfMapLossDesc* desc, const float* z, float* partial, uint32_t* ticket, float* loss, void* hip_stream);
int mf_total_variation_value_f64(const MfMapLossDesc* desc, const double* z, double* partial, uint32_t* ticket, double* loss, void* hip_stream);
/* The autograd backward of losses.py:71-73: every cell of g_z (strides o_*) is STORED with gloss[0] / (H * W) times the signed sum of its up
 * to four neighbour terms, sgn(z - left) - sgn(right - z) + sgn(z - up) - sgn(down - z); sgn(0) = 0 as torch's abs backward has it (a flat
 * map has an exactly zero gradient).  A gather per cell: no atomics. */
int mf_total_variation_bwd_f32(const MfMapLossDesc* desc, const float* z, const float* gloss, float* g_z, void* hip_stream);
int mf_total_variation_bwd_f64(const MfMapLossDesc* desc, const double* z, const double* gloss, double* g_z, void* hip_stream);
/* ---- the optimisation loop of scripts/fit_terrain.py:46-69 around a fit step: Adam on both maps + best-so-far, ONE launch ---------------
 * Everything the loop keeps between iterations lives on the device, so an iteration needs no host read (no `loss.item()`) and the launch
 * can sit behind the step's launches in one hipGraph.  For both maps (n_z height cells, n_mu friction cells; the counts may differ, n_mu
 * may be 0 with NULL friction pointers) and t = state[0] + 1, torch.optim.Adam's default single-tensor step (fit_terrain.py:46-49, :62;
 * amsgrad=False, weight_decay=0, maximize=False), in ATen's order of operations and rounded op by op:
 *   m = b1 m + (1 - b1) g  (as lerp(m, g, 1 - b1));   v = b2 v + (1 - b2) g g;   bc1 = 1 - b1^t,  bc2 = 1 - b2^t  (double, on the device)
 *   p = p + (-(lr / bc1) m) / (sqrt(v) / sqrt(bc2) + eps),   lr per map;   a cell whose g, m, v are 0 keeps its bits
 *   then, per map and only under its flag, the box projection p = min(max(p, lo), hi) (no reference equivalent; a NaN stays a NaN).  The
 *   moments never see the projection.
 * Best-so-far as fit_terrain.py:61-69 has it: loss[0] is the loss at the parameters BEFORE this update; improved = loss[0] < loss_min[0]
 * (strict: a tie or a NaN is no improvement); when improved, z_best / mu_best take the parameters AFTER this update (the reference clones
 * z_grid behind optimizer.step(); mu_best is an extension), loss_min[0] = loss[0], state[1] = state[0].
 *   state[4] int32 = (step, best_step, ticket, reserved), at reset (0, -1, 0, 0);  loss_min[0] = +inf at reset
 *   history[max_iters]: history[step] = loss[0] while step < max_iters; beyond that the write is dropped and step keeps counting
 * Every workgroup reads step, loss and loss_min before its cells; behind them it fences and takes a ticket, and the workgroup that draws
 * the last one commits the four scalars and resets the ticket (mf_pose_loss_value_*'s finish): no workgroup of the launch can see the
 * next iteration's scalars.  Calls that share a state must be ordered on one stream.  Contiguous buffers; g_*, loss are read only; no
 * entry synchronises or allocates (capturable).  The grid is min(mf_terrain_fit_grid_cap(), ceil((n_z + n_mu) / 256)) workgroups of 256
 * threads in a grid-stride loop. */
#define MF_FIT_CLAMP_Z 1
#define MF_FIT_CLAMP_MU 2
typedef struct MfFitDesc {
  int64_t n_z, n_mu;            /* cells of the height map (> 0) and of the friction map (>= 0) */
  int32_t max_iters;            /* length of `history` (>= 0; 0: history may be NULL) */
  int32_t flags;                /* MF_FIT_CLAMP_*: which map is projected into its box */
  double lr_z, lr_mu;           /* >= 0 */
  double beta1, beta2;          /* in [0, 1) */
  double eps;                   /* > 0 */
  double z_lo, z_hi, mu_lo, mu_hi; /* read under the map's flag only; lo <= hi */
} MfFitDesc;
int mf_terrain_fit_update_f32(const MfFitDesc* desc, float* z, float* mu, const float* g_z, const float* g_mu, float* m_z, float* v_z,
                              float* m_mu, float* v_mu, const float* loss, float* z_best, float* mu_best, int32_t* state, float* loss_min,
                              float* history, void* hip_stream);
int mf_terrain_fit_update_f64(const MfFitDesc* desc, double* z, double* mu, const double* g_z, const double* g_mu, double* m_z, double* v_z,
                              double* m_mu, double* v_mu, const double* loss, double* z_best, double* mu_best, int32_t* state,
                              double* loss_min, double* history, void* hip_stream);
/* The most workgroups an mf_terrain_fit_update_* launch uses (more than cap x 256 cells: further trips of the grid-stride loop). */
int mf_terrain_fit_grid_cap(void);
/* The reduction that follows a shared-map mf_rollout_bwd_* (MfRolloutDesc.grad_copies private copies of each map gradient,
 * pool = [n_maps][copies][n]):  out[m][i] = sum_c pool[m][c][i], and pool is left ZEROED -- a caller that keeps the pool across
 * steps never fills it again (replaces a zero fill + `maps.sum(1)`, scripts/train.py's optimizer step reads `out`). */
int mf_reduce_grad_copies_f32(float* pool, int n_maps, int copies, long long n, float* out, void* hip_stream);
int mf_reduce_grad_copies_f64(double* pool, int n_maps, int copies, long long n, double* out, void* hip_stream);

/* ---- terrain staging between the BEV heads and the rollout (scripts/train.py:93-99, 233-235; lss.py:158) ------------------
 * One pass over the head outputs geom, diff, friction (each float32 [B][H][W]):
 *   terrain[B][H][W] = geom - diff (may be NULL);  z / mu [B][h][w] = k x k average pooling (stride k, h = H / k, w = W / k,
 *   overhanging cells dropped like torch.nn.AvgPool2d) of terrain / friction;  zmu[B][h][w][2] = (z, mu) interleaved -- what
 *   MfRolloutFwdBufs.zmu takes (may be NULL).
 * _bwd: g_geom = g_terrain + upsample(gz) / k^2, g_diff = -g_geom, g_friction = upsample(gmu) / k^2; g_terrain, gz, gmu may
 * each be NULL (= zeros); every element of the three outputs is written. */
typedef struct MfStageDesc {
  int32_t B, H, W, k;
} MfStageDesc;
int mf_terrain_stage_fwd_f32(const MfStageDesc* desc, const float* geom, const float* diff, const float* friction, float* terrain,
                             float* z, float* mu, float* zmu, void* hip_stream);
int mf_terrain_stage_bwd_f32(const MfStageDesc* desc, const float* g_terrain, const float* gz, const float* gmu, float* g_geom,
                             float* g_diff, float* g_friction, void* hip_stream);

/* ---- estimate_heightmap (cloudproc.py:88-148): per-cell maximum height of a point cloud + measurement mask ------------
 * points[n][3] float32 (rows with NaNs, points within r_min of the origin in xy, and points outside the open box
 * (-d_max, d_max)^2 x (h_min, h_max) are dropped); x_bins[nx] / y_bins[ny] are the bin edges the reference builds with
 * torch.arange(-d_max, d_max, grid_res) -- a point falls into bin torch.bucketize(x, bins) - 1; scratch = nx*ny int32;
 * hm[2][nx][ny]: hm[0][ix][iy] = max z of the cell (0 where empty), hm[1][ix][iy] = 1.0 where measured (the reference's
 * transposed output layout: first axis = x). */
typedef struct MfHeightmapDesc {
  int32_t n_points, nx, ny;
  float d_max, h_min, h_max;
  float r_min;   /* < 0: no inner radius filter */
  float inv_res; /* 1 / grid_res: first guess of the bin (the edges decide) */
} MfHeightmapDesc;
int mf_estimate_heightmap_f32(const MfHeightmapDesc* desc, const float* points, const float* x_bins, const float* y_bins,
                              int32_t* scratch, float* hm, void* hip_stream);

/* ---- Rigid-terrain label maps (datasets/rough.py:621-649 with :343-365 and :545-601) for S samples at once -------------------------------
 * What the reference builds per sample on the host -- the cloud projected into every camera's segmentation mask, the points with a rigid
 * label gravity-aligned, the robot's footprint swept along the recorded poses, estimate_heightmap of both -- as one launch sequence.
 * Inputs, all device pointers.  points [n_points][3] float32: the clouds of the S samples one after the other; offsets [S+1] int32: sample s
 *   owns the rows offsets[s] .. offsets[s+1]-1 (N_s of them, possibly none; the range is clamped into [0, n_points]).  seg [S][C][Hi][Wi]
 *   uint8: the label masks.  rots [S][C][3][3], trans [S][C][3], intrins [S][C][3][3] float32: camera c of sample s starts at
 *   s * *_stride_s + c * 9 (3 for trans) elements; a stride of 0 shares one set of cameras among the samples.  pose_align [S][3][4] float64:
 *   the gravity alignment of the sample's cloud.  poses [S][T][3][4] float64: the recorded poses, already aligned (T may be 0).  fx [Fx],
 *   fy [Fy] float32: the footprint's coordinates.  x_bins, y_bins [n] float32: the bin edges of estimate_heightmap, torch.arange(-d_max,
 *   d_max, grid_res).  scratch: S*n*n int32, initialised by the call.
 * Items.  Sample s has N_s + T*Fx*Fy items: its cloud points, then its footprint points.
 * Cloud point p, for each camera c with rotation R, translation t, intrinsics K -- float32, every operation rounded on its own, in this
 *   order (the translation unit is built with -ffp-contract=off and IEEE division):
 *     p' = p - t;   q_i = (R[0][i] p'_x + R[1][i] p'_y) + R[2][i] p'_z   (R^T p');   w_i = (K[i][0] q_0 + K[i][1] q_1) + K[i][2] q_2;
 *     u = w_0 / w_2,  v = w_1 / w_2;   the camera SEES p iff  w_2 > 0 && u > 1 && u < Wi-1 && v > 1 && v < Hi-1  (false when anything is
 *     NaN; utils.py:38-43);  its label is seg[s][c][(int)v][(int)u] (truncation).
 *   p is KEPT iff some camera sees it with a label l in the class set: bit (l & 31) of class_set[l >> 5].  A row with a NaN is never kept.
 *   A kept point becomes g = pose_align[s] . p in float64, per row ((r0 x + r1 y) + r2 z) + t, each component then rounded to float32.
 * Footprint point (t, j, i), item index (t * Fy + j) * Fx + i: in float64, g = poses[s][t] . (fx[i], fy[j], 0) by the same row formula,
 *   where the z row's translation is first reduced by |clearance|; then rounded to float32.  It is not aligned again.
 * Every g then passes estimate_heightmap's filters, bin search and per-cell maximum exactly (MfHeightmapDesc above): rows with a NaN,
 *   points within r_min of the origin in xy (r_min < 0: no such filter) and points outside the open box (-d_max, d_max)^2 x (h_min, h_max)
 *   are dropped; the cell is (torch.bucketize(g_x, x_bins) - 1, torch.bucketize(g_y, y_bins) - 1).
 * Outputs.  hm [S][2][n][n] float32: hm[s][0][ix][iy] = the largest g_z of the cell (0 where empty), hm[s][1][ix][iy] = 1.0 where something
 *   fell; every element is written.  point_labels (may be NULL) [n_points][C] int16: the label camera c sees at the point, -1 where it does
 *   not see it; written for every row some sample owns.  The maximum is an integer atomic on an order-preserving key: two launches on the
 *   same input are bit-identical.
 * Launch.  Three launches on the stream: sentinel fill, one thread per item with the sample in the grid's second dimension, finalize.
 *   max_points: an upper bound of every N_s known on the host (n_points always is one) -- it sizes the grid, the offsets are read on the
 *   device only.  The entry neither synchronises nor allocates nor reads anything back (capturable).  S <= 65535, S*n*n < 2^31. */
typedef struct MfTerrainLabelsDesc {
  int32_t S, C, Hi, Wi;          /* samples, cameras per sample, mask rows and columns */
  int32_t T, Fx, Fy;             /* poses per sample, footprint points along x and y */
  int32_t n;                     /* bin edges per axis: the map is n x n */
  int32_t n_points, max_points;  /* rows of points; upper bound of a sample's rows */
  int64_t rots_stride_s, trans_stride_s, intrins_stride_s; /* elements between two samples' cameras, or 0: shared */
  uint32_t class_set[8];         /* 256 bits: the labels that count as rigid */
  double clearance;              /* |clearance| is taken off the z translation of every pose */
  float d_max, h_min, h_max;
  float r_min;                   /* < 0: no inner radius filter */
  float inv_res;                 /* 1 / grid_res: first guess of the bin (the edges decide) */
  int32_t reserved;
} MfTerrainLabelsDesc;
int mf_terrain_labels_f32(const MfTerrainLabelsDesc* desc, const float* points, const int32_t* offsets, const uint8_t* seg, const float* rots,
                          const float* trans, const float* intrins, const double* pose_align, const double* poses, const float* fx,
                          const float* fy, const float* x_bins, const float* y_bins, int32_t* scratch, float* hm, int16_t* point_labels,
                          void* hip_stream);

/* ---- interpolate_grid (dphysics.py:385-455) on its own: the reference's public sampling method, bug for bug --
 * grid[Bg][H][W] with Bg = B, or one map for all rows (map_shared); xq, yq [B][N] query positions; z_out [B][N];
 * n_out [B][N][3] unit normals (may be NULL: return_normals=False); cells_out [B][N][4] int32 (may be NULL) = the CLAMPED flat
 * indices (c, f, l, fl) the value was read from, and frac_out [B][N][2] (may be NULL) = (x_frac, y_frac): the integer half of
 * the function, exposed so a test can compare it with `((q + d_max) / grid_res).long()` directly.  The device code is the
 * rollout kernels' own (locate_m / gather / blend of rollout_fwd_kernel.h), in either arithmetic mode. */
typedef struct MfInterpDesc {
  int32_t B, N, H, W;
  int32_t map_shared;
  int32_t math_mode; /* MF_MATH_* (float32; float64 is always exact) */
  double grid_res, d_max;
} MfInterpDesc;
int mf_interpolate_grid_f32(const MfInterpDesc* desc, const float* grid, const float* xq, const float* yq, float* z_out, float* n_out,
                            int32_t* cells_out, float* frac_out, void* hip_stream);
int mf_interpolate_grid_f64(const MfInterpDesc* desc, const double* grid, const double* xq, const double* yq, double* z_out, double* n_out,
                            int32_t* cells_out, double* frac_out, void* hip_stream);

/* ---- MPPI trajectory optimiser around the path-cost rollout (no reference equivalent: the reference's node scores constant (v, w)
 * samples once and takes argmin, monoforce_node.py:41-126) --------------------------------------------------------------------------
 * One iteration: perturb the nominal control sequence, roll the B sequences out (mf_rollout_fwd_f32 in path-cost mode), score them,
 * replace the nominal by the softmin-weighted average of the sequences.  Float32; plain device pointers (8-byte aligned where they hold
 * (v, w) pairs); every entry validates before its first launch and never synchronises. */
typedef struct MfMppiDesc {
  int32_t B, T;                        /* sampled sequences, steps */
  int32_t keep_nominal, reserved;      /* 1: sequence 0 carries no noise */
  int64_t row_stride_b, row_stride_t;  /* cost rows: rows[b*sb + t*st + k], k < 4 (elements) */
  int64_t x_stride_b;                  /* final poses: x_last[b*x_stride_b + c] */
  float sigma[2], lo[2], hi[2];        /* noise scale and control limits for (v, w) */
  float w_incl, w_force, w_goal, lambda;
} MfMppiDesc;
/* controls[b][t][k] = min(max(nominal[t][k] + sigma[k] * noise[b][t][k], lo[k]), hi[k]) -- multiply, add, clamp, each rounded like the
 * ATen ops they replace; with keep_nominal row 0 is clamp(nominal) (its noise is not read).  One launch. */
int mf_mppi_perturb_f32(const MfMppiDesc* desc, const float* nominal /* [T][2] */, const float* noise /* [B][T][2] */,
                        float* controls /* [B][T][2] */, void* hip_stream);
/* Path costs of B rollouts from the rows the path-cost rollout wrote (MfRolloutFwdBufs.cost_rows, either layout through the strides; the
 * time-major one is read with one 16-byte load per rollout-step):
 *   incl  = mean_t |atan2(r1, r2)| + mean_t |asin(clamp(-r0, -1, 1))|     (planner.costs_from_rows; diff_physics.py:263-266)
 *   force = force_cost[b]                                                  (MfRolloutFwdBufs.path_cost; NULL iff w_force == 0: term 0)
 *   goal  = |x_last[b][0:2] - goal|                                        (goal: two floats in DEVICE memory)
 *   costs[b] = w_incl incl + w_force force + w_goal goal;   terms[b] = (incl, force, goal)   (terms may be NULL)
 * The sum over t has a fixed order for a given (B, T); non-finite rows propagate by IEEE rules.  One launch. */
int mf_path_costs_f32(const MfMppiDesc* desc, const float* cost_rows, const float* force_cost, const float* x_last, const float* goal,
                      float* costs, float* terms, void* hip_stream);
/* Softmin update over the FINITE costs: c_min their minimum, weights[b] = exp(-(c_b - c_min) / lambda) / sum (exactly 0 for a non-finite
 * cost), nominal_out[t][k] = sum_b weights[b] controls[b][t][k]; best[0] = index of the first minimum among the finite costs (-1: none),
 * n_valid[0] = their number; with none, nominal_out = nominal_in and all weights are 0.  nominal_out may be nominal_in.  Three launches
 * (statistics in one workgroup, partial sums over 64-rollout chunks, their sum); every sum has a fixed order: results are bit-identical
 * from call to call.  scratch: mf_mppi_scratch_bytes(desc) bytes, 8-byte aligned (-1 on a bad descriptor). */
long long mf_mppi_scratch_bytes(const MfMppiDesc* desc);
int mf_mppi_update_f32(const MfMppiDesc* desc, const float* costs, const float* controls, const float* nominal_in, float* weights,
                       float* nominal_out, int32_t* best, int32_t* n_valid, void* scratch, long long scratch_bytes, void* hip_stream);

/* ---- Planner costs from the kept poses of a path-cost rollout: a 2-D cost map under the footprint, and path following ---------------
 * (no reference equivalent).  Xs / Rs are the decimated poses exactly as DPhysics.rollout_costs hands them out (sink-shifted Xs, the
 * drifting R of the default integrator), read in place through the strides.  For rollout b, kept pose p, footprint point n:
 *   q = Xs[b,p,0:2] + Rs[b,p,0:2,:] . points[n];   u = (q.x + d_max) / grid_res, v = (q.y + d_max) / grid_res
 *   the point is on the map iff 0 <= u <= H-1 and 0 <= v <= W-1 (a NaN is off the map).  Off the map s = off_map; on it
 *   ix = min(floor(u), H-2), iy = min(floor(v), W-2), fx = u - ix, fy = v - iy,
 *   s = (1-fx)(1-fy) m[ix][iy] + fx(1-fy) m[ix+1][iy] + (1-fx) fy m[ix][iy+1] + fx fy m[ix+1][iy+1],   m[i][j] = cost_map[i*W + j]
 * cost_map[i][j] sits on node (i, j) of z_grid (the node interpolate_grid calls c): first axis x, the same d_max and grid_res.  The
 * blend is the CORRECT bilinear one, deliberately not interpolate_grid's bug-for-bug form (swapped fraction weights, discontinuous
 * across cell edges): a cost map is no reference quantity, so there is no bug to stay compatible with, and a continuous sample keeps
 * float32 from flipping costs at cell edges.
 *   map term   f[b,p] = max_n s;  map[b] = (1/Tp) sum_p f[b,p];  if any sample of the rollout is NOT < lethal, map[b] = +inf and the
 *              cost takes +inf for it whatever w_map is (never 0 x inf).  NaN cells, and NaN rotations under an infinite off_map, end here.
 *   path term  (P > 0) d[b,p] = distance of Xs[b,p,0:2] to the polyline path[0..P-1]: the minimum over the P-1 segments, the projection
 *              parameter clamped to [0,1], a zero-length segment is its point, P = 1 is the distance to that point;
 *              xtrack[b] = (1/Tp) sum_p d[b,p]   (a NaN position gives a NaN term)
 *   costs[b] = (base_costs ? base_costs[b] : 0) + w_map map[b] + w_path xtrack[b];   terms[b] = (map[b], xtrack[b])
 * A NULL cost_map requires w_map == 0: its term is exactly 0 and is not evaluated; P == 0 requires w_path == 0 and a NULL path, likewise.
 * A given cost_map is always evaluated (the lethal rule holds with w_map == 0).  One launch; no float atomics, a fixed summation order
 * for a given (B, Tp, N): bit-identical from call to call and between the rollout's time-major views and a contiguous copy; never
 * synchronises, everything is read on the device (capturable); costs may alias base_costs.  Limits: N <= 1024, P <= 256,
 * H * W and the index range of the pose rows below 2^31. */
typedef struct MfPoseCostDesc {
  int32_t B, Tp, N, P;            /* rollouts, kept poses per rollout, footprint points, path vertices (0: no path term) */
  int32_t H, W;                   /* cost map cells */
  int64_t x_stride_b, x_stride_t; /* Xs[b*sb + t*st + c], c < 3 (elements) */
  int64_t r_stride_b, r_stride_t; /* Rs[b*sb + t*st + 3*i + j] */
  float grid_res, d_max;
  float lethal;                   /* a sample that is NOT < lethal makes the rollout's cost +inf; +inf: no such rule */
  float off_map;                  /* sample value of a footprint point off the map (may be +inf) */
  float w_map, w_path;
} MfPoseCostDesc;
int mf_pose_costs_f32(const MfPoseCostDesc* desc, const float* Xs, const float* Rs, const float* points /* [N][3] body frame */,
                      const float* cost_map /* [H][W] or NULL */, const float* path /* [P][2] or NULL iff P == 0 */,
                      const float* base_costs /* [B] or NULL */, float* costs /* [B] */, float* terms /* [B][2] or NULL */, void* hip_stream);

/* ---- Planner cost WITH its gradient, from the full outputs of the differentiable rollout (no reference equivalent) ------------------------
 * What an MPPI step scores (mf_pose_costs_f32 + mf_path_costs_f32 without the force term), as one differentiable objective, value and
 * gradient in ONE launch.  Xs [B][T][3] (the sink-shifted positions DPhysics.forward returns) and Rs [B][T][3][3] are read in place through
 * the strides.  Kept steps, by the rule of DPhysics.rollout_costs: t_p = min(p * pose_stride, T - 1) for p < Tp = 1 + ceil((T-1) / pose_stride).
 *   J[b] = w_map  (1/Tp) sum_p max_n s(b,p,n)  +  w_path (1/Tp) sum_p d(b,p)  +  w_goal |Xs[b,T-1,0:2] - goal|
 *        + w_incl (1/Tp) sum_p (|roll| + |pitch|)
 * s and d are the footprint sample and the polyline distance of mf_pose_costs_f32 above, word for word (the correct bilinear blend, off_map,
 * the clamped projection parameter, P = 1, zero-length segments); any sample NOT < lethal makes J[b] = +inf whatever w_map is.  goal: two
 * floats in DEVICE memory.  roll = atan2(r1, r2), pitch = asin(clamp(-r0, -1, 1)) with r = Rs[b,t,2,:] / |Rs[b,t,2,:]|, the NORMALISED third
 * row -- NOT the nearest-rotation projection the path-cost rollout applies (MfRolloutDesc.cost_project): the default integrator's R drifts
 * away from a rotation, and normalising the row is the differentiable stand-in for that projection.  A row of norm 0 gives a NaN term, as a
 * NaN pose does; the terms are summed by IEEE rules (a NaN term makes the cost NaN, whatever its weight).
 *   costs[b] = J[b];  terms[b] = (map, xtrack, goal, incl), the four unweighted terms (map = +inf for a lethal rollout)
 *   gXs / gRs (both given or both NULL: value only): gcosts[b] dJ[b]/dXs and gcosts[b] dJ[b]/dRs (gcosts NULL = ones), DENSE in the
 *   strides of Xs / Rs: the rows of the steps that are not kept are written as zeros, so that mf_rollout_bwd_* takes both buffers as its
 *   upstream gradients as they are.
 * The gradient is that of the finite expression: max_n -> the first maximum (smallest n on a tie); the nearest segment -> the smallest k
 * on a tie; |.| has derivative 0 at 0, and so have a zero path distance and a zero goal distance; an off-map sample and a clamped pitch
 * have zero gradient; a lethal rollout keeps the gradient of its finite map term (it is what pushes the rollout out: only its VALUE is
 * +inf).  Every (b, p) owns its gradient rows: no float atomics, nothing accumulated across threads, a fixed summation order -- results
 * are bit-identical from call to call and between the rollout's time-major views and a contiguous copy.
 * A NULL cost_map requires w_map == 0, P == 0 a NULL path and w_path == 0 (terms exactly 0, not evaluated).  One launch on the caller's
 * stream, nothing read on the host (capturable): one workgroup of 256 threads per rollout, a 16-lane DPP row per kept pose (the lanes
 * of a row deal the footprint points and the path's segments among themselves; maximum and minimum travel the row WITH their index).
 * Limits: N <= 1024, P <= 256, H * W and the index range of the pose rows below 2^31. */
typedef struct MfTrajObjDesc {
  int32_t B, T, N, P;             /* rollouts, steps, footprint points, path vertices (0: no path term) */
  int32_t H, W;                   /* cost map cells */
  int32_t pose_stride, reserved;  /* >= 1 */
  int64_t x_stride_b, x_stride_t; /* Xs[b*sb + t*st + c], c < 3 (elements); gXs likewise */
  int64_t r_stride_b, r_stride_t; /* Rs[b*sb + t*st + 3*i + j]; gRs likewise */
  float grid_res, d_max, lethal, off_map;
  float w_map, w_path, w_goal, w_incl;
} MfTrajObjDesc;
int mf_traj_objective_f32(const MfTrajObjDesc* desc, const float* Xs, const float* Rs, const float* points /* [N][3] body frame */,
                          const float* cost_map /* [H][W] or NULL */, const float* path /* [P][2] or NULL iff P == 0 */,
                          const float* goal /* [2], device */, const float* gcosts /* [B] or NULL */, float* costs /* [B] */,
                          float* terms /* [B][4] or NULL */, float* gXs, float* gRs, void* hip_stream);

/* ---- Gradient descent on K control sequences: Adam + per-sequence best-so-far, ONE launch per iteration -------------------------------
 * controls / grad / m / v / best_controls [K][T][2] contiguous, costs / best_cost [K], best_iter [K] int32, history [max_iters][K],
 * state int32 [2] = (step, ticket), at reset (0, 0); best_cost = +inf, best_iter = -1, history = NaN at reset.  One workgroup of 256
 * threads per sequence k, its 2 T elements in trips of 256.  With i = state[0], in this order:
 *   1. history[i][k] = costs[k] while i < max_iters (beyond that the write is dropped and the step keeps counting)
 *   2. costs[k] < best_cost[k] (strict: a tie, a NaN and +inf never improve): best_controls[k] = controls[k] BEFORE this update -- the
 *      controls the cost belongs to (mf_terrain_fit_update_* snapshots AFTER the update, a quirk of the reference's loop that has no
 *      counterpart here) --, best_cost[k] = costs[k], best_iter[k] = i
 *   3. costs[k] is NaN, or any of the 2 T entries of grad[k] is not finite: controls[k], m[k], v[k] stay untouched in this iteration
 *      (decided for the whole sequence, in one pass over the row ahead of any store)
 *   4. else torch.optim.Adam's default single-tensor step as mf_terrain_fit_update_* writes it out (ATen's order of operations, rounded
 *      op by op; bias corrections from t = i + 1 in double on the device), lr = lr[channel]
 *   5. controls = min(max(controls, lo[channel]), hi[channel])   (the moments never see the projection)
 * state[0] = i + 1 is committed by the workgroup that draws the last ticket (as mf_terrain_fit_update_*).  Calls that share a state
 * must be ordered on one stream; no entry synchronises or allocates (capturable). */
typedef struct MfRefineDesc {
  int32_t K, T;                   /* sequences, steps */
  int32_t max_iters, reserved;    /* rows of `history` (>= 0; 0: history may be NULL) */
  double lr[2];                   /* (v, w); >= 0 */
  double beta1, beta2;            /* in [0, 1) */
  double eps;                     /* > 0 */
  float lo[2], hi[2];             /* control limits of (v, w), lo <= hi (either may be infinite) */
} MfRefineDesc;
int mf_control_refine_update_f32(const MfRefineDesc* desc, float* controls, const float* grad, const float* costs, float* m, float* v,
                                 float* best_controls, float* best_cost, int32_t* best_iter, float* history, int32_t* state,
                                 void* hip_stream);

/* ---- Planner cost maps from terrain: slope, roughness and step height under a disc, ONE launch ------------------------------------------
 * (No reference equivalent: its planning node scores rollouts by inclination only and its elevation-mapping pipeline has the surface-normal
 * filter commented out.  The result is what mf_pose_costs_f32 / mf_traj_objective_f32 take as `cost_map`.)
 * Inputs.  z: S maps of H x W heights, element (s, h, w) at s*z_stride_s + h*z_stride_h + w (elements; unit stride along W: a squeeze(1) of
 *   [S,1,H,W] and a row-strided crop are read in place).  valid (may be NULL): the same shape with its own strides v_*, nonzero = usable.
 *   base (may be NULL): the same shape with its own strides b_*, a keep-out map to merge.  Scalars as C floats: grid_res > 0 (metres per
 *   cell), lo[k] < hi[k] for k = (slope, roughness, step), unknown.  Integers: the window radius r in cells, 1 <= r <=
 *   MF_TRAVERSABILITY_MAX_RADIUS, and min_valid >= 3.
 * Window of cell (i, j): the cells (i + di, j + dj) with di^2 + dj^2 <= r^2 (in integers) that lie inside the map, where z is finite and,
 *   with `valid` given, valid is nonzero.  n = their number.
 * Known cells.  With the sums over the window  A = n sum di^2 - (sum di)^2,  B = n sum dj^2 - (sum dj)^2,  C = n sum di dj - sum di sum dj
 *   in 64-bit integers, the cell is KNOWN iff  n >= min_valid  and  A B - C^2 > 0  (the window cells are not collinear).  This is the only
 *   discontinuous rule of the definition, and it is decided in integers so that every implementation agrees on it exactly.  It depends on
 *   the window, not on whether the centre cell itself is usable.
 * Terms of a known cell.  With u = di grid_res, v = dj grid_res, the least-squares plane  z ~ zbar + a (u - ubar) + b (v - vbar)  over the
 *   window (centred 2 x 2 normal equations):
 *     slope     = sqrt(a^2 + b^2)                    rise over run
 *     roughness = sqrt(sum residual^2 / n)           the residuals themselves are squared and summed, not a moment identity
 *     step      = max z - min z over the window
 *   An unknown cell's three terms are NaN.
 * Cost.  ramp_k = min(max((term_k - lo[k]) / (hi[k] - lo[k]), 0), 1);  cost = max_k ramp_k for a known cell, `unknown` otherwise; with
 *   `base`, cost = max(cost, base) wherever base is not NaN, unknown cells included.  cost is in [0,1] when `unknown` and `base` are.
 * Outputs.  cost [S][H][W] contiguous; terms [S][3][H][W] contiguous = (slope, roughness, step), or NULL.  Every cell is STORED (plain
 *   stores, no atomics): the buffers need not be initialised, and two launches on the same input are bit-identical.  Neither output may
 *   alias an input.  There is no backward: cost maps feed planners.
 * Launch.  One workgroup per tile of MF_TRAVERSABILITY_TILE^2 output cells stages the tile and a halo of r cells into LDS once (validity
 *   folded in) and reads every window from there; S * ceil(H / TILE) * ceil(W / TILE) must be below 2^31.  The entry neither synchronises
 *   nor allocates (capturable).  float32 centres the heights on the window mean before any product is formed; _f64 is the validation build
 *   of the same source. */
#define MF_TRAVERSABILITY_TILE 16
#define MF_TRAVERSABILITY_MAX_RADIUS 16
typedef struct MfTraversabilityDesc {
  int32_t S, H, W;                /* maps, rows, columns */
  int32_t r;                      /* window radius in cells */
  int32_t min_valid, reserved;
  int64_t z_stride_s, z_stride_h;
  int64_t v_stride_s, v_stride_h; /* ignored when valid is NULL */
  int64_t b_stride_s, b_stride_h; /* ignored when base is NULL */
  float grid_res, unknown;
  float lo[3], hi[3];             /* (slope [rise/run], roughness [m], step [m]) */
} MfTraversabilityDesc;
int mf_traversability_f32(const MfTraversabilityDesc* desc, const float* z, const float* valid, const float* base, float* cost, float* terms,
                          void* hip_stream);
int mf_traversability_f64(const MfTraversabilityDesc* desc, const double* z, const double* valid, const double* base, double* cost,
                          double* terms, void* hip_stream);

/* ---- Global routes on a cost map: the cost-to-go field towards a goal and the optimal route as a polyline ---------------------------------
 * (No reference equivalent: its planning node follows a hand-given goal.  The inputs are the `cost_map` of mf_pose_costs_f32 -- e.g. the
 * result of mf_traversability_* -- and the result is the `path` [P][2] mf_pose_costs_f32 / mf_traj_objective_f32 read.)
 * Grid.  cost: S maps of H x W node costs, element (s, i, j) at s*c_stride_s + i*c_stride_h + j (elements; unit stride along W, read in
 *   place), with the convention of MfPoseCostDesc: the first axis is x, node (i, j) sits at x = i*grid_res - d_max, y = j*grid_res - d_max.
 * Arithmetic.  The scalar type T of the entry point (_f32: float, _f64: double).  grid_res, d_max, lethal and alpha are carried as C floats
 *   and converted to T once.  EVERY operation below is rounded separately in T (the translation unit is built with -ffp-contract=off).
 * Passable.  A node is passable iff its cost is finite and < lethal.  NaN, +-inf and costs >= lethal are walls.
 * Factor.  s[c] = 1 + alpha * max(cost[c], 0)   (0 <= alpha < inf; one multiply, one add).
 * Moves.  Eight neighbours (di, dj) in this order:  (-1,0) (1,0) (0,-1) (0,1) (-1,-1) (-1,1) (1,-1) (1,1).  A move needs both ends on the
 *   map and passable; a diagonal move (di, dj) from (i, j) needs (i + di, j) and (i, j + dj) passable as well (no corner of a wall is cut).
 * Edge weight.  w(u, v) = len * ((s[u] + s[v]) * 0.5),  len = grid_res for an axial move and fl(grid_res * 1.4142135623730951) for a
 *   diagonal one.  w(u, v) = w(v, u) to the bit.
 * Field.  The goal node is (round((g_x + d_max) / grid_res), round((g_y + d_max) / grid_res)), ties to even, for the goal position g of
 *   the map (goal [S][2], T).  d[goal node] = 0; elsewhere d[v] = min over the permitted neighbours u of fl(d[u] + w(u, v)); +inf on
 *   impassable and unreachable nodes.  Rounded addition is monotone and every weight is positive, so this fixed point is unique and every
 *   relaxation order reaches it: the field is bit-equal to a heap Dijkstra in T.  A goal off the map (or NaN) or on an impassable node:
 *   the whole field is +inf and status gets MF_ROUTE_GOAL_BLOCKED.
 * mf_cost_to_go_*.  field [S][H][W] contiguous, fully written.  status [S] and rounds_used [S] int32, written (not accumulated) by the call.
 *   One initialisation launch and n_rounds launches of one round kernel; a workgroup owns a tile of MF_ROUTE_TILE^2 nodes, relaxes it in LDS
 *   against a one-node halo until it stops changing, and wakes the neighbour tiles whose halo it changed for the next round; tiles nobody
 *   woke, and every tile once a round changed nothing, leave at once (round 0 starts from the tiles that hold the goal node or have it in
 *   their halo).  No workgroup waits on another: all ordering across workgroups is the
 *   launch boundary.  rounds_used = the rounds that changed the field.  MF_ROUTE_NOT_CONVERGED iff the last round still changed it; the
 *   field is then an upper bound of the true one everywhere.  work: int32 scratch of at least mf_cost_to_go_work_ints(desc) words, which
 *   the call initialises itself.  A map without walls needs about tiles_h + tiles_w rounds, a serpentine one round per tile border its
 *   route crosses; empty rounds cost a launch each.
 * Route.  v_0 = the nearest node to the start position (start [S][2], T; rounded as the goal).  v_(k+1) = argmin over the permitted
 *   neighbours u of v_k of fl(d[u] + w(u, v_k)), ties to the earlier neighbour in the order above; the walk ends at the goal node.
 * mf_extract_route_*.  field as above and the cost it was made from (w is recomputed).  nodes [S][max_nodes] int32 = i*W + j, the first
 *   n_nodes [S] of each row written; route_cost [S] (T) = d[v_0]; path [S][P][2] FLOAT always (what the planners read): with L = n_nodes,
 *   vertex p is the position of nodes[(p * (L - 1)) / (P - 1)] (integer division), coordinates fl(fl(i * grid_res) - d_max) in float.
 *   status [S] int32 is read-modify-written: the two field bits are kept, the two route bits are set or cleared.
 *     start off the map (or NaN) or d[v_0] not finite: MF_ROUTE_START_UNREACHABLE, n_nodes = 0, route_cost = +inf, every vertex = the start
 *       position as given (converted to float);
 *     the walk reaches max_nodes nodes before the goal, or finds no neighbour with a finite value (a field that is not this cost's):
 *       MF_ROUTE_TRUNCATED, the path is resampled from the nodes walked;
 *     L = 1 (the start node is the goal node): P copies of it.
 *   One launch, one wave per map: eight lanes fetch the eight candidates, a DPP minimum carrying the neighbour's index picks the next node.
 * Neither entry synchronises, allocates or reads anything on the host (capturable); H * W must be below 2^31. */
#define MF_ROUTE_TILE 32
#define MF_ROUTE_MAX_VERTICES 256
#define MF_ROUTE_GOAL_BLOCKED 1
#define MF_ROUTE_NOT_CONVERGED 2
#define MF_ROUTE_START_UNREACHABLE 4
#define MF_ROUTE_TRUNCATED 8
typedef struct MfCostToGoDesc {
  int32_t S, H, W;                /* maps, rows (x), columns (y) */
  int32_t n_rounds;               /* launches of the round kernel, >= 1 */
  int64_t c_stride_s, c_stride_h; /* strides of cost in elements */
  float grid_res, d_max;
  float lethal, alpha;            /* lethal may be +inf (only non-finite costs are walls); alpha finite, >= 0 */
} MfCostToGoDesc;
typedef struct MfRouteDesc {
  int32_t S, H, W;
  int32_t P;                      /* vertices of the polyline, 2 .. MF_ROUTE_MAX_VERTICES */
  int32_t max_nodes, reserved;    /* row length of nodes, >= 2 */
  int64_t c_stride_s, c_stride_h;
  float grid_res, d_max;
  float lethal, alpha;
} MfRouteDesc;
/* int32 words of `work` for this descriptor: S * (2 * tiles + n_rounds) with tiles = ceil(H / TILE) * ceil(W / TILE); -1 for a bad descriptor */
long long mf_cost_to_go_work_ints(const MfCostToGoDesc* desc);
int mf_cost_to_go_f32(const MfCostToGoDesc* desc, const float* cost, const float* goal, float* field, int32_t* status, int32_t* rounds_used,
                      int32_t* work, void* hip_stream);
int mf_cost_to_go_f64(const MfCostToGoDesc* desc, const double* cost, const double* goal, double* field, int32_t* status,
                      int32_t* rounds_used, int32_t* work, void* hip_stream);
int mf_extract_route_f32(const MfRouteDesc* desc, const float* field, const float* cost, const float* start, const float* goal, int32_t* nodes,
                         int32_t* n_nodes, float* route_cost, float* path, int32_t* status, void* hip_stream);
int mf_extract_route_f64(const MfRouteDesc* desc, const double* field, const double* cost, const double* start, const double* goal,
                         int32_t* nodes, int32_t* n_nodes, double* route_cost, float* path, int32_t* status, void* hip_stream);

/* Text of the calling thread's last error ("" if none).  THREAD-LOCAL: host threads driving different streams each read the message
 * of their own failed call (the reference raises a Python exception in the calling thread, dphysics.py:575,579 asserts). */
const char* mf_last_error(void);
/* Which rollout kernel the calling thread's last mf_rollout_fwd_* / mf_rollout_bwd_* call launched: the demangled kernel template
 * with its parameters (lane mapping, integrator, arithmetic, record / streaming mode ...), grid, workgroup size and the thread's
 * launch count, e.g. "mf::rollout_bwd_cp_kernel<float, 1, true, false, 3, 12, 3, false> grid=256 block=192 launches=7"; "" before
 * the first launch.  Diagnostic only (bench.py reports it as config.launch; the reference has one code path, dphysics.py:530-594,
 * this library has a dispatcher).  Thread-local. */
const char* mf_last_launch(void);
/* Library version, e.g. "monoforce_hip 0.1 gfx950". */
const char* mf_version(void);
/* sizeof() of an ABI struct by name ("MfRolloutDesc", ...), -1 if unknown: lets bindings verify their mirrors. */
int mf_sizeof(const char* struct_name);

#ifdef __cplusplus
}
#endif
#endif /* MONOFORCE_HIP_H */
