// The rollout's dispatch policy in one place: the MF_* switches, the thresholds with the measurements behind them, the planners that turn
// (descriptor, scalar size, which buffers are there) into the route of a launch, and the public policy queries, which read the planners.
// Host code only: nothing here launches, allocates or formats; a refusal is a code and a static text.
#include "rollout_route.h"
#include "mf_common.h"

namespace mf {

// Every MF_* switch the rollout's native code reads (INTEGRATION.md lists names, defaults and meanings), parsed once per process.
// A limit below 0 is "not set" (bwd_xs_min_waves: kSwitchUnset): its default is a property of the device the launch goes to.
constexpr long long kSwitchUnset = -0x7fffffffffffffffll - 1;
struct RouteSwitches {
  long long cp_max_waves, cp_bwd_max_waves, cp_record_max_waves, bwd_xs_min_waves, chunk_waves;
  int cp_bwd_mode, cp_stream_max_grid, cp_stream_big_ring_max_grid, cp_block;
  bool cp_record_dynamics;
  bool cp_bwd_zmu_off, cp_loss_one_wave_off, mw_bwd_off, mw_tile_off, bwd_xs_off, bwd_xs_zmu_off, bwd_xs_loss_off, bwd_xs_ppl_off, bwd_win_off,
      fwd_touch_controls_off;
};
static long long env_ll(const char* v, long long dflt) { return v ? atoll(v) : dflt; }
static int env_int(const char* v, int dflt) { return v ? atoi(v) : dflt; }
static bool env_is_zero(const char* v) { return v && atoi(v) == 0; }

static const RouteSwitches& route_switches() {
  static const RouteSwitches s = [] {
    RouteSwitches v;
    v.cp_max_waves = env_ll(getenv("MF_CP_MAX_WAVES"), -1);
    v.cp_bwd_max_waves = env_ll(getenv("MF_CP_BWD_MAX_WAVES"), -1);
    v.cp_record_max_waves = env_ll(getenv("MF_CP_RECORD_MAX_WAVES"), -1);
    v.bwd_xs_min_waves = env_ll(getenv("MF_BWD_XS_MIN_WAVES"), kSwitchUnset);
    v.chunk_waves = env_ll(getenv("MF_CHUNK_WAVES"), -1);
    v.cp_bwd_mode = env_int(getenv("MF_CP_BWD_MODE"), -1);      // A/B (tools/ab_cp.py): 0 early, 1 late, 2 record read by one wave
    v.cp_stream_max_grid = env_int(getenv("MF_CP_STREAM_MAX_GRID"), -1);
    v.cp_stream_big_ring_max_grid = env_int(getenv("MF_CP_STREAM_BIG_RING_MAX_GRID"), -1);
    v.cp_block = env_int(getenv("MF_CP_BLOCK"), 0);             // A/B (tools/ab_block.sh): 64 / 128 / 256
    v.cp_record_dynamics = env_int(getenv("MF_CP_RECORD_DYNAMICS"), 0) != 0;
    v.cp_bwd_zmu_off = env_is_zero(getenv("MF_CP_BWD_ZMU"));
    v.cp_loss_one_wave_off = env_is_zero(getenv("MF_CP_LOSS_ONE_WAVE"));      // A/B: the unfused route
    v.mw_bwd_off = env_is_zero(getenv("MF_MW_BWD"));
    v.mw_tile_off = env_is_zero(getenv("MF_MW_TILE"));
    v.bwd_xs_off = env_is_zero(getenv("MF_BWD_XS"));
    v.bwd_xs_zmu_off = env_is_zero(getenv("MF_BWD_XS_ZMU"));
    v.bwd_xs_loss_off = env_is_zero(getenv("MF_BWD_XS_LOSS"));                // A/B: the unfused route (dense dL/dXs rows)
    v.bwd_xs_ppl_off = env_is_zero(getenv("MF_BWD_XS_PPL"));                  // A/B: the general kernel
    v.bwd_win_off = env_is_zero(getenv("MF_BWD_WIN"));
    v.fwd_touch_controls_off = env_is_zero(getenv("MF_FWD_TOUCH_CONTROLS"));
    return v;
  }();
  return s;
}

// ---------------------------------------------------------------------------------------------------------------------------------
// lane mappings and workgroup sizes
// ---------------------------------------------------------------------------------------------------------------------------------
static LaneMap choose_lane_map(int B, int N, int points_per_lane) {
  int g1 = 4;
  while (g1 < N) g1 <<= 1;  // lanes per rollout at one point per lane
  // One point per lane whenever the body fits a wave: measured faster than 4 points per lane over the whole range
  // B = 256 .. 65536 (N = 4) once the fast-math kernels cut the per-lane instruction count (tools/sweep_mapping.py).
  bool wide = g1 <= 64;
  if (points_per_lane == 1 && g1 <= 64) wide = true;
  if (points_per_lane == 4) wide = false;
  if (N <= 4) return wide ? LaneMap{4, 1} : LaneMap{1, 4};
  if (N <= 8) return wide ? LaneMap{8, 1} : LaneMap{2, 4};
  if (N <= 16) return wide ? LaneMap{16, 1} : LaneMap{4, 4};
  if (N <= 32) return wide ? LaneMap{32, 1} : LaneMap{8, 4};
  if (N <= 64) return wide ? LaneMap{64, 1} : LaneMap{16, 4};
  // Larger bodies: one wave per rollout with 2 / 4 / 8 points per lane -- unless the batch is so small that this leaves
  // most of the chip idle (the reference's own use: 4 .. 64 rollouts of a 175- or 223-point robot).  Then ONE rollout is
  // spread over 2, 4 or 8 waves of a workgroup, one point per lane (GroupSum exchanges through LDS): ~2.3x fewer instructions
  // per wave and step.  Measured at N = 223: forward 0.79 vs 1.85 ms, backward 2.0 vs 5.6 ms for B <= 256; 0.98 / 2.9 vs
  // 1.38 / 4.4 ms at B = 512 (2 waves per SIMD); a tie at B = 1024 -- so up to 2048 waves per launch.
  if (points_per_lane != 4) {
    const int g = N <= 128 ? 128 : (N <= 256 ? 256 : 512);
    if ((long long)B * (g / 64) <= 2 * device_simds()) return LaneMap{g, 1};      // two waves per SIMD (MI355X: 2048)
  }
  if (N <= 128) return points_per_lane != 4 ? LaneMap{64, 2} : LaneMap{32, 4};
  if (N <= 256) return LaneMap{64, 4};
  return LaneMap{64, 8};
}
static LaneMap desc_lane_map(const MfRolloutDesc* d) {
  return choose_lane_map(d->B, d->N, d->points_per_lane == MF_LANES_COMPONENT ? 0 : d->points_per_lane);
}
LaneMap fwd_lane_map(const MfRolloutDesc* d, bool joints) {
  if (!joints) return desc_lane_map(d);
  const LaneMap m = choose_lane_map(d->B, d->N, 0);      // the articulated kernels exist for the multi-wave mappings (small batches of
  return m.G <= 64 ? choose_lane_map(d->B, d->N, 4) : m;   // a large body) and the 4-points-per-lane ones
}

// Workgroup size of the kernels whose unit of work is ONE wave (four component-parallel rollouts) with nothing shared between waves.
// Measured (profiles/r4_ab_block.txt, twice, on different boxes): with three or four waves per CU the same launch is 20-30 % faster
// as 256-thread workgroups (ONE per CU) than as 64-thread ones -- record-reading backward at 4096 rollouts 0.54 -> 0.44 ms, recording
// forward 0.265 -> 0.193 ms, and 0.373 -> 0.248 ms for an A/B build of the backward with every memory operation compiled out
// (profiles/r4_ab_saved_variants.txt).  The cause is NOT identified: the dispatcher spreads the waves evenly over the SIMDs either way
// (tools/microbench/wave_placement.hip, also with 208 registers and LDS), they start within 2 us of each other, and a plain 8 / 32 KB
// FMA loop runs equally fast in both forms (tools/microbench/ifetch_lockstep.hip).  Below two waves per CU 64-thread workgroups reach
// more CUs; from two waves per SIMD up the forms measure the same.  So the rule is the measured one: 256 threads between two and four
// waves per CU, 64 elsewhere.
static unsigned wave_unit_block(unsigned waves) {
  const int env = route_switches().cp_block;
  if (env == 64 || env == 128 || env == 256) return (unsigned)env;
  const unsigned cus = (unsigned)device_cus();
  return waves > 2u * cus && waves <= 4u * cus ? 256u : 64u;
}
static unsigned ceil_div(long long a, long long b) { return (unsigned)((a + b - 1) / b); }
static long long cp_waves(const MfRolloutDesc* d) { return ((long long)d->B * 16 + 63) / 64; }      // one wave = 4 component-parallel rollouts

// ---------------------------------------------------------------------------------------------------------------------------------
// the component-parallel kernels' range (a rollout over a 16-lane row: rollout_fwd_cp_kernel.h, rollout_bwd_cp_kernel.h)
// ---------------------------------------------------------------------------------------------------------------------------------
// Waves of a component-parallel launch up to which it beats the one-point-per-lane mapping (4 rollouts per wave here, 16 there).
// Measured, forward with all six outputs, N = 4 (tools/ab_cp.py; ms component-parallel vs one point per lane): B = 256 0.16 / 0.29,
// 1024 0.16 / 0.29, 2048 0.17 / 0.29, 4096 0.18 / 0.30 (43 % of the HBM roofline), 8192 0.41 / 0.32 -- so up to 1024 waves, one per
// SIMD.  MF_CP_MAX_WAVES overrides (tuning / A-B runs; 0 disables the mapping).
static long long cp_max_waves() {
  const long long v = route_switches().cp_max_waves;
  return v >= 0 ? v : device_simds();      // one wave per SIMD (MI355X: 1024)
}
// true when the component-parallel kernels cover this launch: float32 fast math (8: the float64 validation build), a rigid body of <= 4
// points, full outputs (or states only), and few enough rollouts that the launch is bound by the instruction stream of its waves
static bool use_component_parallel(const MfRolloutDesc* d, bool joints, bool cost_rows, int scalar_bytes) {
  if (d->math_mode != MF_MATH_FAST || d->N > 4 || joints || cost_rows) return false;
  if (d->points_per_lane != 0 && d->points_per_lane != MF_LANES_COMPONENT) return false;   // an explicit other mapping
  const long long waves = ((long long)d->B + 3) / 4;
  if (d->points_per_lane == 0 && waves > cp_max_waves()) return false;
  // 32-bit byte offsets into every output and into the controls
  const long long fs = d->force_stride ? d->force_stride : d->N;
  const long long row = fs * 3 > 9 ? fs * 3 : 9;
  if ((long long)d->T * d->B * row * scalar_bytes >= (1ll << 32)) return false;
  if (fs < 4) return false;   // quads of absent points write their (zero) slots
  return true;
}

// Measured, backward, N = 4 (tools/ab_cp.py; ms component-parallel vs one point per lane): B = 256 0.38 / 0.88, 1024 0.39 / 0.89,
// 2048 0.45 / 0.90, 4096 0.63 / 0.95, 8192 0.81 / 0.99, 16384 1.63 / 1.62, 32768 3.19 / 2.89 -- up to two waves per SIMD (a lane
// owns one footprint cell here: its gradient accumulator flushes with one atomic per map, which is what bounds the one-point-
// per-lane kernel once the chip is full); MF_CP_BWD_MAX_WAVES overrides (0 disables)
static long long cp_bwd_max_waves() {
  const long long v = route_switches().cp_bwd_max_waves;
  return v >= 0 ? v : 2 * device_simds();      // two waves per SIMD (MI355X: 2048)
}
static bool cp_bwd_covers(const MfRolloutDesc* d, bool joints, int scalar_bytes) {
  if (d->math_mode != MF_MATH_FAST || d->N > 4 || joints) return false;
  if (d->points_per_lane != 0 && d->points_per_lane != MF_LANES_COMPONENT) return false;
  const long long waves = ((long long)d->B + 3) / 4;
  if (d->points_per_lane == 0 && waves > cp_bwd_max_waves()) return false;
  // 32-bit byte offsets into the saved rows and the upstream gradients
  const long long row = (long long)d->N * 3 > 9 ? (long long)d->N * 3 : 9;
  if ((long long)d->T * d->B * row * scalar_bytes >= (1ll << 32)) return false;
  return true;
}

// Largest grid (workgroups = waves of rollouts) the streaming form takes: its LDS ring allows two workgroups per CU with six slots
// (2 x 60 / 72 KB of the CU's 160 KB), one with twelve; dynamics() carries six more planes per slot (96 / 108 KB with six slots: one
// workgroup per CU).  MF_CP_STREAM_MAX_GRID overrides the default integrator's limit (A/B runs).
static unsigned cp_stream_max_grid(int integ) {
  const int env = route_switches().cp_stream_max_grid;
  const unsigned cus = (unsigned)device_cus();
  const unsigned v = env >= 0 ? (unsigned)env : 2u * cus;      // two workgroups per CU (MI355X: 512); dynamics(): one
  return integ == MF_INTEG_ODEINT_EULER ? v : (v < cus ? v : cus);
}
// float64 (validation build): a ring slot is twice the bytes -- six slots of the default integrator's planes fit a CU's LDS (123 / 147 KB,
// one workgroup per CU), dynamics()' sixteen / eighteen planes do not: its record is read by the computing wave itself (kCpSaved)
static unsigned cp_stream_max_grid_of(int scalar_bytes, int integ) {
  if (scalar_bytes == 8) return integ == MF_INTEG_ODEINT_EULER ? cp_stream_max_grid(integ) : 0u;
  return cp_stream_max_grid(integ);
}
// The form the component-parallel backward runs in.  The forward's record when there is one: two more waves per workgroup stream it
// through LDS (while the rings fit the CUs' LDS), else one wave reads it itself; without a record at most one wave per SIMD: late recompute
static int cp_bwd_mode(const MfRolloutDesc* d, int scalar_bytes, bool record) {
  const int forced = route_switches().cp_bwd_mode;
  const long long waves = cp_waves(d);
  if (record) return waves <= (long long)cp_stream_max_grid_of(scalar_bytes, d->integrator) && forced != kCpSaved ? kCpStream : kCpSaved;
  return forced >= 0 && forced < kCpSaved ? forced : (waves <= device_simds() ? kCpLate : kCpEarly);
}

// The compact per-step record (rollout_fwd_cp_kernel.h REC, layout in rollout_cp_common.h): kept where BOTH directions run
// component-parallel and the launch has at most one wave per SIMD -- 256 B per rollout and step (131 MB at B = 1024, T = 500; round
// 2's record was 1 KiB and stopped paying at B = 2048, where its stores bound the forward): one more store per wave-step forward;
// backward no contact chain to recompute (~65 instructions, 7 transcendentals), and the forward's own values at every clamp and
// kink.  Its backward streams the record through LDS with two more waves per workgroup (default integrator: <= 512 workgroups;
// dynamics(), whose ring slots carry the Rodrigues coefficients as well: <= 256) or, default integrator only, reads it in the
// computing wave itself up to 1024 waves.  dynamics() read by the one wave LOSES against recomputing (B = 1024: 0.499 vs 0.436 ms
// backward), so beyond its streaming range it keeps no record (MF_CP_RECORD_DYNAMICS=1 forces one: A/B runs, parity tests of that
// kernel).  MF_CP_RECORD_MAX_WAVES overrides the size limit (0 disables).
static long long cp_record_bytes(const MfRolloutDesc* d, int scalar_bytes) {
  const RouteSwitches& sw = route_switches();
  const long long max_waves = sw.cp_record_max_waves >= 0 ? sw.cp_record_max_waves : device_simds();      // one wave per SIMD
  if (!d || d->B <= 0 || d->T <= 0) return 0;
  if (d->has_joints) return 0;
  if (!use_component_parallel(d, false, false, scalar_bytes) || !cp_bwd_covers(d, false, scalar_bytes)) return 0;
  const long long waves = ((long long)d->B + 3) / 4;
  if (waves > max_waves) return 0;
  if (d->integrator != MF_INTEG_ODEINT_EULER && !sw.cp_record_dynamics && cp_bwd_mode(d, 4, true) != kCpStream) return 0;
  const long long bytes = (long long)d->T * d->B * 16 * 4 * scalar_bytes;      // cp::kRecBytesPerLane<S> per lane and step
  if (bytes >= (1ll << 32)) return 0;
  return bytes;
}

// The fused physics loss rides on the STREAMING backward (its fetching waves form dL/dXs -- and, with MF_LOSS_VALUE_IN_BACKWARD, the
// value): a launch that keeps a record and streams it, either integrator (dynamics(): <= 256 workgroups).  The forward half -- the
// LOSS kernels that accumulate the value while they write the rows -- exists for the default integrator only (cp_loss_in_forward);
// dynamics() takes the value from the backward launch or from mf_physics_loss_value_* on the written rows.
static bool cp_loss_fusable(const MfRolloutDesc* d) {
  if (!d || d->layout != MF_LAYOUT_TIME_MAJOR) return false;
  if (d->integrator != MF_INTEG_ODEINT_EULER && d->integrator != MF_INTEG_DYNAMICS) return false;
  return cp_record_bytes(d, 4) > 0 && cp_bwd_mode(d, 4, true) == kCpStream;
}
static bool cp_loss_in_forward(const MfRolloutDesc* d) { return cp_loss_fusable(d) && d->integrator == MF_INTEG_ODEINT_EULER; }
// ... and on the component-parallel backward in its EARLY-RECOMPUTE form (no record, more than one wave per SIMD: 4097 .. 8192 rollouts of
// a <= 4-point body, either integrator): dL/dXs formed where the row is consumed (rollout_bwd_cp_kernel.h ONE1 -- instantiations of their
// own, the kernels without the loss are untouched); the value comes from mf_physics_loss_value_* on the forward's rows.  In the
// record-reading form and in late recompute (up to one wave per SIMD, also where MF_CP_BWD_MODE forces early recompute there) the kernel
// loses what the loss's own two small launches cost: no gain (profiles/r6_ab_one_wave_loss.txt)
static bool cp_loss_one_wave(const MfRolloutDesc* d, int scalar_bytes) {
  if (route_switches().cp_loss_one_wave_off || !d || d->layout != MF_LAYOUT_TIME_MAJOR || d->has_joints || cp_loss_fusable(d)) return false;
  if (scalar_bytes != 4 && d->points_per_lane != MF_LANES_COMPONENT) return false;
  if (cp_record_bytes(d, scalar_bytes) > 0 || cp_waves(d) <= device_simds() || cp_bwd_mode(d, scalar_bytes, false) != kCpEarly) return false;
  return cp_bwd_covers(d, false, scalar_bytes);
}

// ---------------------------------------------------------------------------------------------------------------------------------
// one rollout over several waves, from the forward's 16-byte record (rollout_bwd_mw_kernel.h)
// ---------------------------------------------------------------------------------------------------------------------------------
// The launches these kernels serve: float32 MF_MATH_FAST, either integrator, rigid body, one point per lane --
//   * bodies of 65..512 points spread over 2 / 4 / 8 waves by choose_lane_map (<= 2048 waves per launch), and
//   * bodies of 5..64 points (8 / 16 / 32 / 64 lanes per rollout) up to two waves per SIMD (the positions-only instantiations hold
//     237 registers; beyond, the forward goes out in chunks and the general kernels take over).  N <= 4 has the component-parallel kernels.
// MF_MW_BWD=0 keeps the general kernel (A/B runs, parity tests of the two against each other).
static bool mw_shape(const MfRolloutDesc* d) {
  if (route_switches().mw_bwd_off || !d || d->B <= 0 || d->T <= 0 || d->N <= 4 || d->N > 512) return false;
  if (d->math_mode != MF_MATH_FAST || d->has_joints) return false;
  if (d->integrator != MF_INTEG_ODEINT_EULER && d->integrator != MF_INTEG_DYNAMICS) return false;
  if (d->points_per_lane == 4) return false;
  const LaneMap m = desc_lane_map(d);
  if (m.PPL != 1 || m.G < 8) return false;
  return m.G > 64 || (long long)d->B * m.G <= 2 * device_simds() * 64;      // two waves per SIMD
}
static long long mw_record_bytes(const MfRolloutDesc* d, int scalar_bytes) {
  if (!mw_shape(d)) return 0;
  return (long long)d->T * d->B * 4 * (long long)scalar_bytes;      // kMwRecFloats scalars per rollout and step
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the one-point-per-lane kernels (rollout_fwd_kernel.h, rollout_bwd_kernel.h)
// ---------------------------------------------------------------------------------------------------------------------------------
// the launch shapes whose forward kernels read the shared maps interleaved ...
static bool zmu_shape(const MfRolloutDesc* d, bool joints, const LaneMap& m, int scalar_bytes) {
  if (!d->map_shared || d->math_mode != MF_MATH_FAST || joints || m.PPL != 1 || m.G > 64) return false;
  return (long long)d->H * d->W * (long long)scalar_bytes < (1ll << 31);   // 32-bit byte offsets into the (z, mu) cells
}
// ... and those that run the interleave pass into a scratch they are offered:
// below ~half a wave per SIMD the launch is bound by the instruction stream of its waves; the extra pass (a second launch in
// front of the rollout, ~10 us) then costs what the two saved gathers bring (measured: B = 1024 path costs 0.306 -> 0.323 ms)
// (the float64 validation build takes the pass whenever it is offered: its purpose is to run the ZMU kernels)
static bool zmu_pass(const MfRolloutDesc* d, const LaneMap& m, int scalar_bytes) {
  return scalar_bytes != 4 || (long long)d->B * m.G >= device_simds() / 2 * 64;      // (half a wave per SIMD)
}
// whether the forward reads the interleaved copy, and whose: the caller's staged pair, or the scratch it offers, filled by the pass
static void fwd_interleaved_maps(const MfRolloutDesc* d, const FwdBits& p, int scalar_bytes, FwdRoute* r) {
  r->zmu = r->interleave = false;
  if ((!p.zmu_scratch && !p.zmu) || !zmu_shape(d, p.joints, r->m, scalar_bytes)) return;
  if (p.zmu && p.mu) { r->zmu = true; return; }   // the caller staged the interleaved pair itself (mf_terrain_stage_fwd_f32): no pass, no batch-size condition
  if (!p.zmu_scratch || !zmu_pass(d, r->m, scalar_bytes)) return;
  r->zmu = r->interleave = true;
}

// The launches of a positions-only upstream that go to the XS_ONLY one-point-per-lane kernels (rollout_bwd_kernel.h): float32 fast math, rigid
// body, beyond the component-parallel range (N <= 4: > two waves per SIMD) and the record-reading multi-wave range (5..64 points: > two waves per
// SIMD), one point per lane inside a wave, from half a wave per SIMD up.  These kernels carry the fused physics loss (LOSS) as well.
// (from half a wave per SIMD: right above the component-parallel kernels' range -- 10 240 / 12 288 / 14 336 rollouts of the 4-point body
//  1.14 / 1.39 / 1.60 ms on the general kernels, 0.91 / 0.90 / 0.93 here, tools/ab_between.sh; MF_BWD_XS_MIN_WAVES overrides)
static long long xs_bwd_min_waves() {
  const long long v = route_switches().bwd_xs_min_waves;
  return v != kSwitchUnset ? v : device_simds() / 2;
}
static bool xs_bwd_shape(const MfRolloutDesc* d, const LaneMap& m) {
  return !route_switches().bwd_xs_off && m.PPL == 1 && m.G <= 64 && (long long)d->B * m.G >= xs_bwd_min_waves() * 64;
}
// the positions-only launches whose cell gradients leave through the workgroup's LDS window (rollout_bwd_kernel.h WIN): four lanes per rollout
// on ONE shared map pair with a power-of-two side (cell -> window row / column by shift and mask)
static bool xs_win_shape(const MfRolloutDesc* d, const LaneMap& m) {
  return !route_switches().bwd_win_off && d->map_shared && m.G == 4 && d->H == d->W && (d->H & (d->H - 1)) == 0;
}
// the shapes whose positions-only backward forms dL/dXs itself (LOSS): those the planner sends to the XS_ONLY kernels, time-major rows, the
// descriptor's own one-point-per-lane mapping, outside the record-reading multi-wave kernels' range
static bool xs_loss_fusable(const MfRolloutDesc* d) {
  if (route_switches().bwd_xs_loss_off || !d || d->B <= 0 || d->T <= 0 || d->N <= 0 || d->N > 64 || d->has_joints) return false;
  if (d->math_mode != MF_MATH_FAST || d->layout != MF_LAYOUT_TIME_MAJOR) return false;
  if (d->integrator != MF_INTEG_ODEINT_EULER && d->integrator != MF_INTEG_DYNAMICS) return false;
  if (d->points_per_lane == MF_LANES_COMPONENT || d->points_per_lane == 4) return false;
  if (cp_bwd_covers(d, false, 4)) return false;      // the component-parallel kernels' range
  if (mw_shape(d)) return false;                     // the record-reading multi-wave kernels' range
  return xs_bwd_shape(d, desc_lane_map(d));
}

// ---------------------------------------------------------------------------------------------------------------------------------
// the planners
// ---------------------------------------------------------------------------------------------------------------------------------
#define MF_ROUTE_REQUIRE(cond, code, text) \
  do {                                     \
    if (!(cond)) {                         \
      r.rc = (code);                       \
      r.msg = (text);                      \
      return r;                            \
    }                                      \
  } while (0)

// the one-point-per-lane forward launches (every family but kFwdCp, and without a record): workgroup, chunks, the pass over the controls
static void fwd_general_launch(const MfRolloutDesc* d, int scalar_bytes, FwdRoute* r) {
  const RouteSwitches& sw = route_switches();
  const LaneMap m = r->m;
  r->block = m.G > 64 ? m.G : (d->block ? d->block : 64);   // a rollout spread over several waves: exactly one rollout per workgroup (LDS + barrier)
  r->chunk_B = d->B;
  r->touch_lo = 1; r->touch_hi = 0;
  if (r->record) { r->block = m.G > 64 ? m.G : 64; return; }      // the recording kernels: one launch of one-wave (or one-rollout) workgroups
  // More than two waves per SIMD do not help these kernels -- their gathers then miss the CU's L1 more often -- so a very
  // large batch goes out as consecutive launches of <= kChunkWaves waves on the same stream (measured: B = 65536 1.81 -> 1.73 ms,
  // B = 131072 4.23 -> 3.90 ms; MF_CHUNK_WAVES=0 disables).  The chunk is a whole number of workgroups; results do not depend on it.
  const long long kChunkWaves = sw.chunk_waves >= 0 ? sw.chunk_waves : 2 * device_simds();      // two waves per SIMD (MI355X: 2048)
  if (m.G <= 64 && kChunkWaves > 0 && (long long)d->B * m.G > kChunkWaves * 64) r->chunk_B = (int)(kChunkWaves * 64 / m.G);
  // Round 6: the controls of a saturated launch read ONCE in front of it.  A step loads the next step's (v, w) one step ahead (~0.7 us at
  // 16 384 rollouts) inside its dependent chain, and vmcnt retires loads in order: while the [B][T][2] array sits in the memory-side cache
  // (forward after forward) that is free, but the forward of a fit / train step follows a backward that has streamed ~700 MB through the
  // caches, and every 64-byte line of controls then costs an HBM round trip in front of the step's gathers -- forward 0.34 -> 0.43 ms at
  // 16 384 rollouts, 0.35 again with this 16 us pass (tools/ab_step_fwd2.py, profiles/r6_ab_step_fwd.txt).  A deeper in-kernel prefetch does
  // not help: a load that misses stalls the younger gathers behind it wherever it is issued.  MF_FWD_TOUCH_CONTROLS=0: A/B.
  const bool strided = d->controls_stride_b != 0 || d->controls_stride_t != 0;
  const int ctrl_sb = strided ? d->controls_stride_b : d->T * 2, ctrl_st = strided ? d->controls_stride_t : 2;
  if (sw.fwd_touch_controls_off || ctrl_st == 0 || ctrl_sb != d->T * 2 || m.G > 64) return;      // (one pair per rollout, or rows that are not adjacent: nothing to stream)
  const long long row = (long long)d->T * 2 * scalar_bytes;      // bytes of a rollout's controls
  const long long lo_waves = (device_simds() / 2 * 64 + m.G - 1) / m.G;      // (below half a wave per SIMD a step is longer than the round trip)
  const long long lo_bytes = ((8ll << 20) + row - 1) / row, hi = (192ll << 20) / row;      // (a few MB stay resident anyway; more than the cache holds is futile)
  r->touch_lo = (int)(lo_waves > lo_bytes ? lo_waves : lo_bytes); r->touch_hi = (int)hi;
}

// The component-parallel launch (a rollout over a 16-lane row, rollout_fwd_cp_kernel.h) with everything that rides on it: the
// interleaved maps, the per-step record for the backward, the fused physics loss.  4: the kernels the dispatcher picks for
// few rollouts of a small body; 8: their validation build, on explicit request (points_per_lane = MF_LANES_COMPONENT).
static FwdRoute plan_fwd_cp(const MfRolloutDesc* d, int scalar_bytes, const FwdBits& p, FwdRoute r) {
  r.family = kFwdCp;
  r.m = LaneMap{16, 1};
  fwd_interleaved_maps(d, p, scalar_bytes, &r);
  if (p.rec && cp_record_bytes(d, scalar_bytes) > 0) {      // the per-step record for the backward (MfRolloutFwdBufs.rec)
    MF_ROUTE_REQUIRE((p.rec_low & 15) == 0, MF_ERR_INVALID, "rollout_fwd: rec must be 16-byte aligned");
    r.record = true;
  }
  if (p.loss && (p.loss_flags & MF_LOSS_VALUE_IN_BACKWARD)) {      // the backward will form the value: mark it as not yet known
    MF_ROUTE_REQUIRE(cp_loss_fusable(d), MF_ERR_UNSUPPORTED, "rollout_fwd: this launch cannot carry the fused physics loss (mf_rollout_loss_fusable)");
    MF_ROUTE_REQUIRE(p.loss_out, MF_ERR_INVALID, "rollout_fwd: MF_LOSS_VALUE_IN_BACKWARD needs MfRolloutLoss.loss");
    r.loss = kLossValueInBackward;
  } else if (p.loss) {      // physics_loss inside the launch (MfRolloutLoss)
    MF_ROUTE_REQUIRE(cp_loss_in_forward(d), MF_ERR_UNSUPPORTED, "rollout_fwd: this launch cannot accumulate the physics loss itself (the LOSS kernels ride on the "
                     "default integrator; dynamics(): MF_LOSS_VALUE_IN_BACKWARD, or mf_physics_loss_value_* on the rows)");
    MF_ROUTE_REQUIRE(!p.forces && d->layout == MF_LAYOUT_TIME_MAJOR, MF_ERR_INVALID, "rollout_fwd: the fused physics loss needs Fs = Ff = NULL and MF_LAYOUT_TIME_MAJOR");
    MF_ROUTE_REQUIRE(p.loss_complete, MF_ERR_INVALID, "rollout_fwd: incomplete MfRolloutLoss");
    MF_ROUTE_REQUIRE((long long)d->B * p.loss_T2 * 3 * (long long)scalar_bytes < (1ll << 32), MF_ERR_UNSUPPORTED, "rollout_fwd: ground truth of 4 GiB or more");
    r.loss = kLossInLaunch;
  }
  // one wave = 4 rollouts: B = 1024 puts one wave on each of the 256 CUs; workgroups of one wave, or of four where the dispatcher would
  // otherwise stack waves on a SIMD (wave_unit_block; the kernels that carry the fused loss -- <= two waves per CU -- are one-wave workgroups)
  r.block = r.loss == kLossInLaunch ? 64 : (int)wave_unit_block((unsigned)cp_waves(d));
  return r;
}

FwdRoute plan_fwd(const MfRolloutDesc* d, int scalar_bytes, const FwdBits& p) {
  FwdRoute r{};
  r.rc = MF_OK; r.msg = "";
  r.family = kFwdGeneral;
  r.m = fwd_lane_map(d, p.joints);
  r.forces = p.forces;
  r.chunk_B = d->B; r.touch_lo = 1; r.touch_hi = 0;
  r.loss = kLossNone;
  const bool fast = d->math_mode == MF_MATH_FAST;
  if (scalar_bytes == 8) {
    // the float64 VALIDATION build of the component-parallel kernels (rollout_fwd_cp_f64.hip): on explicit request only
    if (d->points_per_lane == MF_LANES_COMPONENT && use_component_parallel(d, p.joints, p.cost_rows, 8)) {
      MF_ROUTE_REQUIRE((p.zmu_low & 15) == 0, MF_ERR_INVALID, "rollout_fwd: zmu_scratch / zmu must be 16-byte aligned");
      return plan_fwd_cp(d, 8, p, r);
    }
    // ... and of the recording one-point-per-lane kernels of 5..512-point bodies (rollout_fwd_kernel.h FAST / REC, whose backward is
    // rollout_bwd_mw_kernel.h): same request, with the record buffer
    if (d->points_per_lane == MF_LANES_COMPONENT && p.rec && !p.joints && !p.cost_rows && !p.loss && mw_record_bytes(d, 8) > 0) {
      MF_ROUTE_REQUIRE((p.rec_low & 31) == 0, MF_ERR_INVALID, "rollout_fwd: rec must be 32-byte aligned");
      r.family = kFwdMwRecF64;
      r.record = true;
      r.block = r.m.G > 64 ? r.m.G : 64;
      return r;
    }
    MF_ROUTE_REQUIRE(p.forces, MF_ERR_UNSUPPORTED, "rollout_fwd: float64 needs the force buffers (states only: the component-parallel validation build, points_per_lane = MF_LANES_COMPONENT)");
    MF_ROUTE_REQUIRE(!p.cost_rows, MF_ERR_UNSUPPORTED, "rollout_fwd: cost rows exist for float32 only");
    MF_ROUTE_REQUIRE(!p.loss, MF_ERR_UNSUPPORTED, "rollout_fwd: the fused physics loss exists for the component-parallel kernels only");
    fwd_general_launch(d, 8, &r);      // float64 is always exact
    return r;
  }
  MF_ROUTE_REQUIRE((p.zmu_low & 7) == 0, MF_ERR_INVALID, "rollout_fwd: zmu_scratch / zmu must be 8-byte aligned");
  if (p.joints) {
    MF_ROUTE_REQUIRE(p.forces && !p.cost_rows, MF_ERR_UNSUPPORTED, "rollout_fwd: articulated rollouts write all six outputs");
    r.family = fast ? kFwdJointsFast : kFwdGeneral;
    fwd_general_launch(d, 4, &r);
    return r;
  }
  if (p.cost_rows) {   // path-cost mode: cost rows + decimated poses (see MfRolloutFwdBufs.cost_rows)
    MF_ROUTE_REQUIRE(fast && d->layout == MF_LAYOUT_TIME_MAJOR && d->pose_stride >= 1, MF_ERR_UNSUPPORTED,
                     "rollout_fwd: cost rows need float32 MF_MATH_FAST, MF_LAYOUT_TIME_MAJOR and pose_stride >= 1");
    MF_ROUTE_REQUIRE(!p.xds && !p.omegas && !p.forces && !p.xraw, MF_ERR_INVALID,
                     "rollout_fwd: with cost_rows only Xs and Rs (decimated) are written -- pass NULL for Xds, Omegas, Fs, Ff, Xraw");
    if (r.m.PPL == 4 && r.m.G < 64) r.m = choose_lane_map(d->B, d->N, 1);
    r.cost = d->cost_project != 0 ? 2 : 1;
    fwd_interleaved_maps(d, p, 4, &r);
    r.family = r.zmu ? kFwdZmu : kFwdCost;
    fwd_general_launch(d, 4, &r);
    return r;
  }
  MF_ROUTE_REQUIRE(p.forces || fast, MF_ERR_UNSUPPORTED,
                   "rollout_fwd: the states-only kernels (Fs = Ff = NULL) exist for float32 MF_MATH_FAST rigid-body rollouts only");
  if (!fast) {
    MF_ROUTE_REQUIRE(!p.loss, MF_ERR_UNSUPPORTED, "rollout_fwd: the fused physics loss exists for the float32 fast-math kernels only");
    fwd_general_launch(d, 4, &r);
    return r;
  }
  if (use_component_parallel(d, p.joints, p.cost_rows, 4))   // few rollouts of a small body: a rollout over 16 lanes (rollout_fwd_cp_kernel.h)
    return plan_fwd_cp(d, 4, p, r);
  MF_ROUTE_REQUIRE(!p.loss, MF_ERR_UNSUPPORTED, "rollout_fwd: this launch cannot carry the fused physics loss (mf_rollout_loss_fusable)");
  if (!p.forces && r.m.PPL == 4 && r.m.G < 64) r.m = choose_lane_map(d->B, d->N, 1);
  // >= one wave per SIMD and a one-point-per-lane mapping within a wave: the split-store kernels (rollout_fwd_kernel.h)
  r.split = r.m.PPL == 1 && r.m.G <= 64 && (long long)d->B * r.m.G >= device_simds() * 64;
  if (p.rec && mw_record_bytes(d, 4) > 0) {      // the 16-byte record of rollout_bwd_mw_kernel.h
    MF_ROUTE_REQUIRE((p.rec_low & 15) == 0, MF_ERR_INVALID, "rollout_fwd: rec must be 16-byte aligned");
    r.record = true;
  }
  fwd_interleaved_maps(d, p, 4, &r);
  r.family = r.zmu ? kFwdZmu : (r.split ? kFwdSplit : kFwdFast);
  fwd_general_launch(d, 4, &r);
  return r;
}

BwdRoute plan_bwd(const MfRolloutDesc* d, int scalar_bytes, const BwdBits& p) {
  const RouteSwitches& sw = route_switches();
  BwdRoute r{};
  r.rc = MF_OK; r.msg = "";
  r.family = kBwdGeneral;
  const bool f32 = scalar_bytes == 4, component = d->points_per_lane == MF_LANES_COMPONENT;
  const unsigned dblock = (unsigned)(d->block ? d->block : 64);
  r.loss = p.loss;
  if (p.loss) {      // the forward's fused physics loss: dL/dXs is formed inside the kernel from Xs, the ground truth and gloss
    const bool loss_cp = (f32 || component) && cp_loss_fusable(d) && p.rec && !p.joints;
    const bool loss_xs = !loss_cp && f32 && xs_loss_fusable(d) && !p.joints;
    // (3: the one-wave forms of the component-parallel backward -- record read by the computing wave, early / late recompute)
    const bool loss_cp1 = !loss_cp && !loss_xs && cp_loss_one_wave(d, scalar_bytes) && !p.joints && !(p.loss_flags & MF_LOSS_VALUE_IN_BACKWARD);
    MF_ROUTE_REQUIRE(!(loss_cp1 || loss_xs) || p.loss_near_w, MF_ERR_INVALID, "rollout_bwd: this fused loss reads MfRolloutLoss.near and .w");
    MF_ROUTE_REQUIRE(loss_cp || loss_xs || loss_cp1, MF_ERR_UNSUPPORTED,
                     "rollout_bwd: this launch cannot carry the fused physics loss (mf_rollout_loss_fusable: 1 = the streaming component-parallel backward, "
                     "the forward's record required; 2 = the saturated positions-only kernels)");
    MF_ROUTE_REQUIRE((long long)d->B * p.loss_T2 * 3 * (long long)scalar_bytes < (1ll << 32), MF_ERR_UNSUPPORTED, "rollout_bwd: ground truth of 4 GiB or more");
    MF_ROUTE_REQUIRE(!p.gXs && !p.gXds && !p.gRs && !p.gOmegas && !p.gFs && !p.gFf, MF_ERR_INVALID,
                     "rollout_bwd: with a fused loss the six upstream gradients must be NULL");
    MF_ROUTE_REQUIRE(p.loss_rows, MF_ERR_INVALID, "rollout_bwd: incomplete MfRolloutLoss");
    MF_ROUTE_REQUIRE(!(p.loss_flags & MF_LOSS_VALUE_IN_BACKWARD) || p.loss_value, MF_ERR_INVALID,      // the fetching waves also form the loss value
                     "rollout_bwd: MF_LOSS_VALUE_IN_BACKWARD needs MfRolloutLoss.partial / ticket / loss");
  }
  const bool any_null = !p.gXs || !p.gXds || !p.gRs || !p.gOmegas || !p.gFs || !p.gFf;
  MF_ROUTE_REQUIRE(!any_null || p.zeros, MF_ERR_INVALID,
                   "rollout_bwd: an upstream gradient is NULL but `zeros` (>= max(9, 3) zero scalars) was not provided");
  const bool no_other = !p.gXds && !p.gRs && !p.gOmegas && !p.gFs && !p.gFf;
  if (p.joints) {   // articulated body: exact arithmetic, default lane mappings (the backward recomputes every step, so it
                    // need not mirror the forward's mapping)
    r.family = kBwdJoints;
    r.fast = f32 && d->math_mode == MF_MATH_FAST;
    r.m = choose_lane_map(d->B, d->N, 0);
    r.block = r.m.G > 64 ? (unsigned)r.m.G : dblock;
    r.grid = ceil_div((long long)d->B * r.m.G, r.block);
    return r;
  }
  // float32: the dispatcher's choice for few rollouts of a small body; float64: the VALIDATION build of the same kernels, on explicit
  // request only (points_per_lane = MF_LANES_COMPONENT; rollout_bwd_cp_f64.hip)
  if ((f32 || component) && cp_bwd_covers(d, false, scalar_bytes)) {   // few rollouts of a small body: a rollout over 16 lanes
    r.family = kBwdCp;
    r.m = LaneMap{16, 1};
    if (p.rec && cp_record_bytes(d, scalar_bytes) > 0) {      // the forward kept its per-step record: read it instead of recomputing
      MF_ROUTE_REQUIRE((p.rec_low & 15) == 0, MF_ERR_INVALID, "rollout_bwd: rec must be 16-byte aligned");
      r.record = true;
    }
    r.xs_only = (p.gXs || p.loss) && no_other;
    r.cp_mode = cp_bwd_mode(d, scalar_bytes, r.record);
    // The record-reading kernel (kCpSaved: beyond the streaming form's grid, up to one wave per SIMD) re-gathers every cell's (z, mu); with
    // a shared float32 pair it reads them interleaved (the caller's staged pair, or the scratch it offers, filled by the pass).
    // MF_CP_BWD_ZMU=0: two 4-byte loads per cell (A/B runs, parity of the two).
    if (f32 && (p.zmu || p.zmu_scratch) && !sw.cp_bwd_zmu_off && r.cp_mode == kCpSaved && d->map_shared && p.mu && d->integrator == MF_INTEG_ODEINT_EULER &&
        (long long)d->H * d->W * 8 < (1ll << 31)) {      // (32-bit byte offsets into the (z, mu) cells)
      MF_ROUTE_REQUIRE((p.zmu_low & 7) == 0, MF_ERR_INVALID, "rollout_bwd: zmu_scratch / zmu must be 8-byte aligned");
      r.zmu = true;
      r.interleave = !p.zmu;
    }
    const long long threads = (long long)d->B * 16;
    const unsigned waves = (unsigned)cp_waves(d);
    // early recompute beyond one wave per SIMD on ONE shared power-of-two map pair: the cell writes through an LDS window per workgroup of
    // eight waves (one workgroup per CU: 128 KB); every workgroup must be full (no early exit in front of its barriers).  MF_BWD_WIN=0: A/B.
    // (measured and dropped, round 5: the LDS gradient window in the record-reading form -- 3072 / 4096 rollouts: 0.382 / 0.406 ms with or without)
    r.win = f32 && !sw.bwd_win_off && r.cp_mode == kCpEarly && d->map_shared && d->H == d->W && (d->H & (d->H - 1)) == 0 && threads % 512 == 0;
    // ONE1: the fused physics loss of the one-wave forms (float32) -- instantiations of their own, for the early-recompute form only
    // (cp_loss_one_wave); the streaming form carries the loss in its fetching waves
    r.one1 = f32 && p.loss && r.cp_mode == kCpEarly;
    MF_ROUTE_REQUIRE(!p.loss || r.cp_mode == kCpStream || r.one1, MF_ERR_UNSUPPORTED, "rollout_bwd: the one-wave fused physics loss exists for float32 positions-only launches");
    if (r.cp_mode == kCpStream) {
      // Workgroup = the computing wave + two fetching waves.  Ring: twelve slots while a CU holds one workgroup (B <= 1024: 120 / 144 KB
      // of its 160 KB LDS -- the fetching waves run up to four batches ahead), six for two workgroups per CU (60 / 72 KB each; the
      // positions-only variants, held to 256 registers there, fetch in batches of TWO steps: no scratch).  dynamics() and the float64
      // build: six slots (96 / 108 KB, 123 / 147 KB: one workgroup per CU)
      const unsigned big_ring_max = sw.cp_stream_big_ring_max_grid >= 0 ? (unsigned)sw.cp_stream_big_ring_max_grid : (unsigned)device_cus();      // one workgroup per CU
      r.ring_slots = f32 && d->integrator == MF_INTEG_ODEINT_EULER && waves <= big_ring_max ? 12 : 6;
      r.grid = waves; r.block = 192;
    } else if (r.win) {
      r.grid = (unsigned)(threads / 512); r.block = 512;
    } else {
      r.block = wave_unit_block(waves);
      r.grid = ceil_div(threads, r.block);
    }
    return r;
  }
  r.m = desc_lane_map(d);
  // one rollout over several waves, from the forward's 16-byte record (float64: the validation build, on explicit request)
  if ((f32 || component) && mw_shape(d) && p.rec && !p.loss) {
    MF_ROUTE_REQUIRE((p.rec_low & (4u * (unsigned)scalar_bytes - 1u)) == 0, MF_ERR_INVALID, "rollout_bwd: rec must be aligned to its quads");
    r.family = kBwdMw;
    r.record = true;
    r.xs_only = no_other;
    r.block = r.m.G > 64 ? (unsigned)r.m.G : 64u;
    r.grid = ceil_div((long long)d->B * r.m.G, r.block);
    // LDS gradient tiles (rollout_bwd_mw_kernel.h) while every workgroup of the launch is resident with its tiles: 160 KB per CU,
    // 256 CUs.  MF_MW_TILE=0 keeps the register accumulators (A/B runs, parity of the two routes).
    // cells per side of a rollout's tile: measured (B = 64 x N = 223: 1.094 -> 1.038 ms; 256 x 64: 0.861 -> 0.845;
    // 1024 x 32: 0.971 -> 0.967; 256 x 16: 0.692 -> 0.883 -- four tiles per wave collide in the LDS): whole-wave groups only
    const int te = r.m.G >= 64 ? 64 : 0;
    const long long lds = (long long)(r.m.G > 64 ? 1 : 64 / r.m.G) * 2 * (te + 1) * te * (long long)scalar_bytes + 4096;
    const unsigned cus = (unsigned)device_cus();
    r.tile = te > 0 && !sw.mw_tile_off && (long long)((r.grid + cus - 1) / cus) * lds <= 160 * 1024 && (long long)d->H * d->W < (1ll << 30);
    return r;
  }
  r.block = r.m.G > 64 ? (unsigned)r.m.G : dblock;
  r.grid = ceil_div((long long)d->B * r.m.G, r.block);
  if (!f32 || d->math_mode != MF_MATH_FAST) {
    MF_ROUTE_REQUIRE(!p.loss, MF_ERR_UNSUPPORTED, "rollout_bwd: this launch cannot carry the fused physics loss (mf_rollout_loss_fusable)");
    return r;
  }
  // positions-only upstream (physics_loss) on a one-point-per-lane mapping inside a wave, from half a wave per SIMD up: the XS_ONLY
  // kernels -- and, for ONE shared map pair with a friction map, the interleaved (z, mu) copy (the caller's staged pair, or the
  // scratch it offers, refilled by the pass: one 65 536-cell pass in front of a launch of >= 1 ms).  MF_BWD_XS=0 / MF_BWD_XS_ZMU=0: A/B.
  r.xs_only = (p.gXs || p.loss) && no_other;
  if (r.xs_only && xs_bwd_shape(d, r.m)) {
    r.family = kBwdXs;
    if (!sw.bwd_xs_zmu_off && d->map_shared && p.mu && (p.zmu || p.zmu_scratch) && (long long)d->H * d->W * 8 < (1ll << 31)) {
      MF_ROUTE_REQUIRE((p.zmu_low & 7) == 0, MF_ERR_INVALID, "rollout_bwd: zmu_scratch / zmu must be 8-byte aligned");
      r.zmu = true;
      r.interleave = !p.zmu;
    }
    // ... and, four lanes per rollout on ONE shared map pair: the accumulators' writes go to a 128 x 128-cell LDS window per workgroup
    // (rollout_bwd_kernel.h WIN; 128 KB of LDS = one workgroup per CU: 256 threads at one wave per SIMD, 512 from two up).  MF_BWD_WIN=0: A/B.
    if (xs_win_shape(d, r.m)) {
      const long long waves = ((long long)d->B * r.m.G + 63) / 64;
      r.win = true;
      r.carry = waves >= 2ll * device_simds();      // (two waves per SIMD: eight-wave workgroups, accumulator carry-over)
      r.block = r.carry ? 512 : 256;
    } else {
      r.block = dblock;
    }
    r.grid = ceil_div((long long)d->B * r.m.G, r.block);
    return r;
  }
  MF_ROUTE_REQUIRE(!p.loss, MF_ERR_UNSUPPORTED, "rollout_bwd: this launch cannot carry the fused physics loss (mf_rollout_loss_fusable)");
  // ... and one rollout per wave with several points per lane (65 .. 512 points beyond the multi-wave range), positions-only upstream
  if (!sw.bwd_xs_ppl_off && !sw.bwd_xs_off && r.xs_only && r.m.G == 64 && (r.m.PPL == 2 || r.m.PPL == 4 || r.m.PPL == 8) && (long long)d->B >= xs_bwd_min_waves()) {
    r.family = kBwdXsPpl;
    r.block = dblock;
    r.grid = ceil_div((long long)d->B * r.m.G, r.block);
    return r;
  }
  // accumulator carry-over between adjacent cells (rollout_bwd_kernel.h): ~55 more instructions per step, half the atomics --
  // a gain from ~3 waves per 4 CUs upwards (B = 4096 at N = 4: 1.00 -> 0.94 ms; B = 65536: 9.5 -> 5.5 ms), a loss below
  r.family = (long long)d->B * r.m.G >= 3ll * device_cus() / 4 * 64 ? kBwdCarry : kBwdFast;
  return r;
}
#undef MF_ROUTE_REQUIRE

}  // namespace mf

// ---------------------------------------------------------------------------------------------------------------------------------
// the public policy queries
// ---------------------------------------------------------------------------------------------------------------------------------
extern "C" long long mf_rollout_record_bytes(const MfRolloutDesc* d) {
  const long long cp = mf::cp_record_bytes(d, 4);
  return cp > 0 ? cp : mf::mw_record_bytes(d, 4);
}
// the float64 validation build of the component-parallel kernels (points_per_lane = MF_LANES_COMPONENT): 32-byte quads
extern "C" long long mf_rollout_record_bytes_f64(const MfRolloutDesc* d) {
  if (!d || d->points_per_lane != MF_LANES_COMPONENT) return 0;
  const long long cp = mf::cp_record_bytes(d, 8);
  return cp > 0 ? cp : mf::mw_record_bytes(d, 8);      // (bodies of 5..512 points: rollout_bwd_mw_kernel.h's record, 32 bytes per rollout-step)
}
// 0 = no; 1 = both directions on the component-parallel kernels with the streaming backward (value in the forward launch, in the backward
// launch -- MF_LOSS_VALUE_IN_BACKWARD -- or from mf_physics_loss_value_*); 2 = the BACKWARD of a saturated launch (positions-only one-point-
// per-lane kernels): pass MfRolloutBwdBufs.loss with flags = 0, take the value from mf_physics_loss_value_* on the forward's rows
// 3 = the BACKWARD of a component-parallel launch in its early-recompute form (4097 .. 8192 rollouts): as 2, without MF_LOSS_VALUE_IN_BACKWARD
// -- read off the route of a float32 backward that is given the record and a complete MfRolloutLoss
extern "C" int mf_rollout_loss_fusable(const MfRolloutDesc* d) {
  if (!d || d->N > 512 || d->has_joints) return 0;
  mf::BwdBits p{};
  p.rec = p.zeros = p.loss = p.loss_near_w = p.loss_rows = p.loss_value = true;
  p.loss_T2 = 1;
  const mf::BwdRoute r = mf::plan_bwd(d, 4, p);
  if (r.rc != MF_OK) return 0;
  if (r.family == mf::kBwdCp) return r.cp_mode == mf::kCpStream ? 1 : (r.one1 ? 3 : 0);
  return r.family == mf::kBwdXs ? 2 : 0;
}
// 1 where a positions-only backward of this shape (float32) sends its cell gradients through the workgroups' LDS windows: a workgroup then adds
// its window to gradient copy blockIdx % grad_copies ONCE, at its end -- few copies suffice (the caller's reduction over them is what grows)
extern "C" int mf_rollout_bwd_window(const MfRolloutDesc* d) {
  if (!d || d->B <= 0 || d->N <= 0 || d->N > 4 || d->has_joints || d->math_mode != MF_MATH_FAST) return 0;
  if (d->points_per_lane == MF_LANES_COMPONENT || d->points_per_lane == 4) return 0;
  mf::BwdBits p{};
  p.gXs = p.zeros = true;
  const mf::BwdRoute r = mf::plan_bwd(d, 4, p);
  return r.rc == MF_OK && r.family == mf::kBwdXs && r.win ? 1 : 0;
}
// 1 where mf_rollout_fwd_f32 given `zmu_scratch` (and no `zmu`) fills it with the interleaved (z, mu) pair on the component-parallel route:
// the caller may then hand the same buffer to mf_rollout_bwd_f32 as `zmu` (same step, same maps) and spare the backward its own pass
extern "C" int mf_rollout_fwd_stages_zmu(const MfRolloutDesc* d) {
  if (!d || d->B <= 0 || d->T <= 0 || d->N > 512 || d->has_joints) return 0;
  mf::FwdBits p{};
  p.xds = p.omegas = p.zmu_scratch = true;
  const mf::FwdRoute r = mf::plan_fwd(d, 4, p);
  return r.rc == MF_OK && r.family == mf::kFwdCp && r.interleave ? 1 : 0;
}
extern "C" int mf_rollout_force_stride(const MfRolloutDesc* d) {
  if (!d || d->B <= 0 || d->N <= 0 || d->N > 512) return -1;
  const mf::LaneMap m = mf::fwd_lane_map(d, d->has_joints != 0);
  const int lanes = m.G * m.PPL;
  return lanes > d->N ? lanes : d->N;
}
// (round 6: no kernel needs the buffer any more -- the component-parallel kernels compile the control gradient out, the multi-wave ones test
//  for NULL, the one-point-per-lane ones send the rows to a 3-float dump per rollout; kept for callers that ask)
extern "C" int mf_rollout_bwd_wants_gcontrols(const MfRolloutDesc* d) { (void)d; return 0; }
