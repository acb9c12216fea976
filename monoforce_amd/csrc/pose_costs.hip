// Planner costs from the poses a path-cost rollout keeps (DPhysics.rollout_costs: Xs / Rs, every pose_stride-th pose as decimated
// time-major rows): a 2-D cost map sampled under the robot's footprint, and the distance to a polyline path.  One entry point, float32,
// ONE launch on the caller's stream, nothing read on the host (capturable), no float atomics, fixed summation order.
//
//   footprint   q = Xs[b,p,0:2] + Rs[b,p,0:2,:] . points[n]                                   (sink-shifted Xs, the drifting R, as handed out)
//   sample      u = (q.x + d_max) / grid_res, v = (q.y + d_max) / grid_res
//               on the map iff 0 <= u <= H-1 and 0 <= v <= W-1 (a NaN is off the map); off the map: s = off_map; on it:
//               ix = min(floor(u), H-2), iy = min(floor(v), W-2), fx = u - ix, fy = v - iy
//               s = (1-fx)(1-fy) m[ix][iy] + fx(1-fy) m[ix+1][iy] + (1-fx) fy m[ix][iy+1] + fx fy m[ix+1][iy+1],  m[i][j] = cost_map[i*W + j]
//   map term    f[b,p] = max_n s;  map[b] = (1/Tp) sum_p f[b,p];  any sample of the rollout NOT < lethal: map[b] = +inf, which the
//               cost takes as +inf whatever w_map is (NaN cells and NaN rotations land here too)
//   path term   d[b,p] = min over the P-1 segments of |Xs[b,p,0:2] - closest point| (projection parameter clamped to [0,1], a zero-length
//               segment is its point, P = 1: the distance to that point);  xtrack[b] = (1/Tp) sum_p d[b,p]
//   result      costs[b] = (base_costs ? base_costs[b] : 0) + w_map map[b] + w_path xtrack[b];  terms[b] = (map[b], xtrack[b])
//
// cost_map[i][j] sits on node (i, j) of z_grid (first axis x, the same d_max and grid_res).  The blend is the CORRECT bilinear one, not
// interpolate_grid's bug-for-bug form (which swaps the fraction weights and jumps across cell edges): a cost map is no reference
// quantity, there is no bug to stay compatible with, and a continuous sample keeps float32 from flipping costs at cell edges.
//
// Two wave64 mappings, chosen by the body alone (N <= kLaneBodyMax):
//   lanes = rollouts   the few points loop in-lane; the kept poses of a 64-rollout group are dealt round-robin to the S waves of its
//                      workgroup (the time-major rows make a pose row's loads coalesce across the lanes), the S partial sums added in wave order
//   lanes = points     a 16-lane DPP row per kept pose (four poses per wave): the row loads the pose's 8 numbers once, its lanes take the
//                      points n = l, l+16, ... from LDS, max over the row on DPP (no LDS crossbar); a workgroup of 1, 2 or 4 waves per rollout,
//                      the rows' partial sums added in row order
// The path's vertices (<= 256) are staged in LDS; the map (256 x 256: 256 KB) stays in L2.  Built by the plain rule (-ffp-contract=off).
#include "mf_common.h"

#include <math.h>

namespace mf {

constexpr int kPosePointsMax = 1024;   // footprint points (LDS: 16 KB as float4)
constexpr int kPosePathMax = 256;      // path vertices (LDS: 2 KB)
constexpr int kLaneBodyMax = 8;        // up to this many points a lane is a rollout
constexpr int kPoseSlicesMax = 16;     // waves that share the kept poses of one 64-rollout group (lanes = rollouts)
constexpr int kRowWavesMax = 4;        // waves per rollout (lanes = points)

// NaN-propagating minimum (fminf would drop the NaN of a NaN pose)
__device__ __forceinline__ float nan_min(float a, float b) { return (a < b || a != a) ? a : b; }

// max / NaN-propagating min over the 16 lanes of a DPP row, every lane gets the result (mirror steps: the merged halves hold equal values)
__device__ __forceinline__ float row_max(float v) {
  v = fmaxf(v, dpp_mov<0xB1>(v));
  v = fmaxf(v, dpp_mov<0x4E>(v));
  v = fmaxf(v, dpp_mov<0x141>(v));
  return fmaxf(v, dpp_mov<0x140>(v));
}
__device__ __forceinline__ float row_nan_min(float v) {
  v = nan_min(v, dpp_mov<0xB1>(v));
  v = nan_min(v, dpp_mov<0x4E>(v));
  v = nan_min(v, dpp_mov<0x141>(v));
  return nan_min(v, dpp_mov<0x140>(v));
}

// One footprint sample.  Branch-free: an off-map (or NaN) point reads cell (0, 0) and selects off_map, so every index is in [0, H*W).
__device__ __forceinline__ float sample_map(const MfPoseCostDesc& d, const float* __restrict__ map, float qx, float qy) {
  const float u = (qx + d.d_max) / d.grid_res, v = (qy + d.d_max) / d.grid_res;
  const bool on = u >= 0.0f && u <= (float)(d.H - 1) && v >= 0.0f && v <= (float)(d.W - 1);
  const float us = on ? u : 0.0f, vs = on ? v : 0.0f;
  const int ix = min((int)floorf(us), d.H - 2), iy = min((int)floorf(vs), d.W - 2);
  const float fx = us - (float)ix, fy = vs - (float)iy;
  const float* m = map + ix * d.W + iy;
  const float m00 = m[0], m01 = m[1], m10 = m[d.W], m11 = m[d.W + 1];
  const float gx = 1.0f - fx, gy = 1.0f - fy;
  const float s = (gx * gy) * m00 + (fx * gy) * m10 + (gx * fy) * m01 + (fx * fy) * m11;
  return on ? s : d.off_map;
}

// squared distance of (x, y) to the segment a -> b
__device__ __forceinline__ float seg_dist2(float x, float y, float2 a, float2 b) {
  const float abx = b.x - a.x, aby = b.y - a.y, apx = x - a.x, apy = y - a.y;
  const float len2 = abx * abx + aby * aby;
  const float t = len2 > 0.0f ? mf_clamp((apx * abx + apy * aby) / len2, 0.0f, 1.0f) : 0.0f;
  const float dx = apx - t * abx, dy = apy - t * aby;
  return dx * dx + dy * dy;
}

__device__ __forceinline__ void stage_path(const MfPoseCostDesc& d, const float* __restrict__ path, float2* s_path) {
  for (int i = threadIdx.x; i < d.P; i += blockDim.x) s_path[i] = make_float2(path[2 * i], path[2 * i + 1]);
}

// costs[b] and terms[b] from the two sums over the kept poses; costs may alias base_costs (read, then written, by this thread alone)
__device__ __forceinline__ void finish_rollout(const MfPoseCostDesc& d, int b, float map_sum, float path_sum, bool lethal, bool has_map,
                                               const float* base, float* costs, float* terms) {
  const float mp = has_map ? (lethal ? INFINITY : map_sum / (float)d.Tp) : 0.0f;
  const float xt = d.P > 0 ? path_sum / (float)d.Tp : 0.0f;
  float c = base ? base[b] : 0.0f;
  if (has_map) c = c + (lethal ? INFINITY : d.w_map * mp);
  if (d.P > 0) c = c + d.w_path * xt;
  costs[b] = c;
  if (terms) { terms[2 * b] = mp; terms[2 * b + 1] = xt; }
}

// ---- lanes = rollouts (N <= kLaneBodyMax) ---------------------------------------------------------------------------------------------------
__global__ void __launch_bounds__(64 * kPoseSlicesMax) pose_costs_lanes_kernel(const MfPoseCostDesc d, const float* __restrict__ Xs, const float* __restrict__ Rs,
                                                                               const float* __restrict__ points, const float* __restrict__ map,
                                                                               const float* __restrict__ path, const float* base, float* costs,
                                                                               float* __restrict__ terms) {
  __shared__ float2 s_path[kPosePathMax];
  __shared__ float s_pts[kLaneBodyMax * 3];
  __shared__ float s_map[kPoseSlicesMax][64], s_xt[kPoseSlicesMax][64];
  __shared__ int s_lethal[kPoseSlicesMax][64];
  const int lane = threadIdx.x & 63, s = threadIdx.x >> 6, S = blockDim.x >> 6;
  const int b = blockIdx.x * 64 + lane;
  stage_path(d, path, s_path);
  if ((int)threadIdx.x < 3 * d.N) s_pts[threadIdx.x] = points[threadIdx.x];
  __syncthreads();
  const bool has_map = map != nullptr;
  const int nseg = max(d.P - 1, 1);
  float map_sum = 0.0f, path_sum = 0.0f;
  bool lethal = false;
  if (b < d.B) {
    const float* xb = Xs + (int64_t)b * d.x_stride_b;
    const float* rb = Rs + (int64_t)b * d.r_stride_b;
    for (int p = s; p < d.Tp; p += S) {
      const float* xp = xb + (int64_t)p * d.x_stride_t;
      const float x = xp[0], y = xp[1];
      if (has_map) {
        const float* rp = rb + (int64_t)p * d.r_stride_t;
        const float r00 = rp[0], r01 = rp[1], r02 = rp[2], r10 = rp[3], r11 = rp[4], r12 = rp[5];
        float f = -INFINITY;
        for (int n = 0; n < d.N; ++n) {
          const float p0 = s_pts[3 * n], p1 = s_pts[3 * n + 1], p2 = s_pts[3 * n + 2];
          const float sv = sample_map(d, map, x + (r00 * p0 + r01 * p1 + r02 * p2), y + (r10 * p0 + r11 * p1 + r12 * p2));
          lethal = lethal || !(sv < d.lethal);
          f = fmaxf(f, sv);
        }
        map_sum += f;
      }
      if (d.P > 0) {
        float d2 = INFINITY;
        for (int k = 0; k < nseg; ++k) d2 = nan_min(seg_dist2(x, y, s_path[k], s_path[min(k + 1, d.P - 1)]), d2);
        path_sum += sqrtf(d2);
      }
    }
  }
  s_map[s][lane] = map_sum; s_xt[s][lane] = path_sum; s_lethal[s][lane] = lethal;
  __syncthreads();
  if (s != 0 || b >= d.B) return;
  for (int k = 1; k < S; ++k) { map_sum += s_map[k][lane]; path_sum += s_xt[k][lane]; lethal = lethal || s_lethal[k][lane] != 0; }
  finish_rollout(d, b, map_sum, path_sum, lethal, has_map, base, costs, terms);
}

// ---- lanes = points: one workgroup (blockDim / 64 waves) per rollout, one 16-lane row per kept pose --------------------------------------------
__global__ void __launch_bounds__(64 * kRowWavesMax) pose_costs_points_kernel(const MfPoseCostDesc d, const float* __restrict__ Xs, const float* __restrict__ Rs,
                                                                              const float* __restrict__ points, const float* __restrict__ map,
                                                                              const float* __restrict__ path, const float* base, float* costs,
                                                                              float* __restrict__ terms) {
  __shared__ float2 s_path[kPosePathMax];
  __shared__ float4 s_pts[kPosePointsMax];
  __shared__ float s_map[4 * kRowWavesMax], s_xt[4 * kRowWavesMax], s_lethal[4 * kRowWavesMax];
  const int l = threadIdx.x & 15, row = threadIdx.x >> 4, rows = blockDim.x >> 4;
  const int b = blockIdx.x;      // < d.B: the grid is B workgroups
  stage_path(d, path, s_path);
  for (int n = threadIdx.x; n < d.N; n += blockDim.x) s_pts[n] = make_float4(points[3 * n], points[3 * n + 1], points[3 * n + 2], 0.0f);
  __syncthreads();
  const bool has_map = map != nullptr;
  const int nseg = max(d.P - 1, 1);
  const float* xb = Xs + (int64_t)b * d.x_stride_b;
  const float* rb = Rs + (int64_t)b * d.r_stride_b;
  float map_sum = 0.0f, path_sum = 0.0f, lethal = 0.0f;
  for (int p = row; p < d.Tp; p += rows) {      // (a row enters or leaves the loop whole: the DPP steps below read active lanes only)
    const float* xp = xb + (int64_t)p * d.x_stride_t;
    const float x = xp[0], y = xp[1];
    if (has_map) {
      const float* rp = rb + (int64_t)p * d.r_stride_t;
      const float r00 = rp[0], r01 = rp[1], r02 = rp[2], r10 = rp[3], r11 = rp[4], r12 = rp[5];
      float f = -INFINITY, bad = 0.0f;
      for (int n = l; n < d.N; n += 16) {
        const float4 pt = s_pts[n];
        const float sv = sample_map(d, map, x + (r00 * pt.x + r01 * pt.y + r02 * pt.z), y + (r10 * pt.x + r11 * pt.y + r12 * pt.z));
        bad = sv < d.lethal ? bad : 1.0f;
        f = fmaxf(f, sv);
      }
      map_sum += row_max(f);
      lethal = fmaxf(lethal, row_max(bad));
    }
    if (d.P > 0) {
      float d2 = INFINITY;
      for (int k = l; k < nseg; k += 16) d2 = nan_min(seg_dist2(x, y, s_path[k], s_path[min(k + 1, d.P - 1)]), d2);
      path_sum += sqrtf(row_nan_min(d2));
    }
  }
  if (l == 0) { s_map[row] = map_sum; s_xt[row] = path_sum; s_lethal[row] = lethal; }
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (int k = 1; k < rows; ++k) { map_sum += s_map[k]; path_sum += s_xt[k]; lethal = fmaxf(lethal, s_lethal[k]); }
  finish_rollout(d, b, map_sum, path_sum, lethal != 0.0f, has_map, base, costs, terms);
}

}  // namespace mf

static int pose_costs_check(const MfPoseCostDesc* d, const float* Xs, const float* Rs, const float* points, const float* cost_map, const float* path,
                            const float* costs) {
  MF_REQUIRE(d, MF_ERR_INVALID, "pose_costs: null descriptor");
  MF_REQUIRE(Xs && Rs && points && costs, MF_ERR_INVALID, "pose_costs: null argument (Xs, Rs, points and costs are required)");
  MF_REQUIRE(d->B > 0 && d->Tp > 0 && d->N > 0, MF_ERR_INVALID, "pose_costs: B, Tp and N must be positive");
  MF_REQUIRE(d->N <= mf::kPosePointsMax, MF_ERR_UNSUPPORTED, "pose_costs: at most 1024 footprint points");
  MF_REQUIRE(d->P >= 0, MF_ERR_INVALID, "pose_costs: P must not be negative");
  MF_REQUIRE(d->P <= mf::kPosePathMax, MF_ERR_UNSUPPORTED, "pose_costs: at most 256 path vertices");
  MF_REQUIRE(d->H >= 2 && d->W >= 2, MF_ERR_INVALID, "pose_costs: the cost map needs H >= 2 and W >= 2");
  MF_REQUIRE(d->x_stride_b >= 0 && d->x_stride_t >= 0 && d->r_stride_b >= 0 && d->r_stride_t >= 0, MF_ERR_INVALID, "pose_costs: negative stride");
  MF_REQUIRE(d->grid_res > 0.0f, MF_ERR_INVALID, "pose_costs: grid_res must be positive");
  MF_REQUIRE(d->lethal == d->lethal && d->off_map == d->off_map, MF_ERR_INVALID, "pose_costs: lethal and off_map must not be NaN");
  MF_REQUIRE(cost_map || d->w_map == 0.0f, MF_ERR_INVALID, "pose_costs: w_map needs a cost_map (NULL requires w_map == 0)");
  MF_REQUIRE((path != nullptr) == (d->P > 0), MF_ERR_INVALID, "pose_costs: path must be NULL exactly when P is 0");
  MF_REQUIRE(d->P > 0 || d->w_path == 0.0f, MF_ERR_INVALID, "pose_costs: w_path needs a path (P == 0 requires w_path == 0)");
  const long long lim = 1ll << 31;
  MF_REQUIRE((long long)d->H * d->W < lim, MF_ERR_UNSUPPORTED, "pose_costs: H * W must stay below 2^31");
  // (each factor is below 2^31 and the strides are checked one at a time first, so the sums cannot overflow 64 bits unnoticed)
  MF_REQUIRE(d->x_stride_b < lim && d->x_stride_t < lim && d->r_stride_b < lim && d->r_stride_t < lim, MF_ERR_UNSUPPORTED,
             "pose_costs: strides must stay below 2^31");
  MF_REQUIRE((d->B - 1) * d->x_stride_b + (d->Tp - 1) * d->x_stride_t + 3 < lim && (d->B - 1) * d->r_stride_b + (d->Tp - 1) * d->r_stride_t + 9 < lim,
             MF_ERR_UNSUPPORTED, "pose_costs: the pose rows' index range must stay below 2^31");
  return MF_OK;
}

extern "C" int mf_pose_costs_f32(const MfPoseCostDesc* d, const float* Xs, const float* Rs, const float* points, const float* cost_map, const float* path,
                                 const float* base_costs, float* costs, float* terms, void* stream) {
  int rc = pose_costs_check(d, Xs, Rs, points, cost_map, path, costs);
  if (rc != MF_OK) return rc;
  hipStream_t st = (hipStream_t)stream;
  if (d->N <= mf::kLaneBodyMax) {
    // waves per 64-rollout group: enough of them to fill the chip (1024 SIMDs) at small B, fewer as the groups multiply (as path_costs)
    const int S = d->B <= 8192 ? 16 : (d->B <= 16384 ? 8 : 4);
    hipLaunchKernelGGL(mf::pose_costs_lanes_kernel, dim3((d->B + 63) / 64), dim3(64 * S), 0, st, *d, Xs, Rs, points, cost_map, path, base_costs, costs, terms);
  } else {
    const int waves = d->B <= 1024 ? 4 : (d->B <= 4096 ? 2 : 1);
    hipLaunchKernelGGL(mf::pose_costs_points_kernel, dim3(d->B), dim3(64 * waves), 0, st, *d, Xs, Rs, points, cost_map, path, base_costs, costs, terms);
  }
  hipError_t e = hipGetLastError();
  MF_REQUIRE(e == hipSuccess, MF_ERR_LAUNCH, std::string("pose_costs launch: ") + hipGetErrorString(e));
  return MF_OK;
}
