// The planner's cost as ONE differentiable objective over the full outputs of the autograd rollout (DPhysics.forward: Xs [B,T,3], Rs [B,T,3,3],
// read in place through the strides), value and gradient in ONE launch: the cost map under the footprint and the distance to a path
// (pose_costs.hip's terms), the distance to the goal and the inclination (mppi.hip's path_costs terms), at the steps DPhysics.rollout_costs
// keeps, t_p = min(p * pose_stride, T - 1).  Formulas and gradient rules: include/monoforce_hip.h at MfTrajObjDesc.
//
//   inclination   roll = atan2(r1, r2), pitch = asin(clamp(-r0, -1, 1)) with r = Rs[b,t,2,:] / |Rs[b,t,2,:]|: the NORMALISED third row, NOT the
//                 nearest-rotation projection the path-cost rollout applies -- the default integrator's R drifts away from a rotation, and
//                 normalising the row is the differentiable stand-in for that projection (a row of norm 0: a NaN term, like a NaN pose)
//
// Mapping: one workgroup of kObjBlock = 256 threads per rollout, a 16-lane DPP row per kept pose (16 poses in flight, further ones in trips of
// the pose loop).  The lanes of a row deal the footprint points (n = l, l + 16, ...) and the path's segments among themselves; the maximum
// sample and the nearest segment travel the row on DPP TOGETHER WITH THEIR INDEX (the smaller index wins a tie, so the first maximum / the
// first nearest segment is found whatever the deal), then every lane of the row re-evaluates that one sample / segment with its derivative
// and lanes 0 .. 11 store the twelve numbers of the pose's gradient rows.  Every (b, p) owns its rows and the rows of the steps that are not
// kept are zeroed by the same workgroup (disjoint addresses: no ordering needed): no float atomics, nothing accumulated across threads.  The
// sums over the kept poses are added per row in pose order and over the sixteen rows in row order: bit-identical from call to call and
// between the rollout's time-major views and a contiguous copy.  A 16-lane row serves small bodies as it serves large ones -- a refiner
// descends on a few hundred sequences, where the launch is bound by its latency, not by the idle lanes of a 4-point body.
// The three small device helpers (nan-free row reductions aside) are pose_costs.hip's, duplicated: that file is not to be touched.
// Built by the plain rule (-ffp-contract=off).
#include "mf_common.h"

#include <limits.h>
#include <math.h>

namespace mf {

constexpr int kObjPointsMax = 1024;   // footprint points (LDS: 16 KB as float4)
constexpr int kObjPathMax = 256;      // path vertices (LDS: 2 KB)
constexpr int kObjBlock = 256;        // threads of a workgroup: sixteen 16-lane rows
constexpr int kObjRows = kObjBlock / 16;

template <int CTRL>
__device__ __forceinline__ int dpp_mov_i(int v) { return __builtin_amdgcn_update_dpp(0, v, CTRL, 0xF, 0xF, true); }

// (value, index) over the 16 lanes of a DPP row, every lane gets the result: the larger / smaller value, on a tie the smaller index.  The
// values are never NaN (the callers' in-lane loops only take a value under a strict comparison), so both lanes of an exchange decide alike
// and the mirror steps meet merged halves that hold equal pairs.
template <int CTRL, bool MAX>
__device__ __forceinline__ void row_arg_step(float& v, int& n) {
  const float ov = dpp_mov<CTRL>(v);
  const int on = dpp_mov_i<CTRL>(n);
  const bool take = (MAX ? ov > v : ov < v) || (ov == v && on < n);
  v = take ? ov : v;
  n = take ? on : n;
}
template <bool MAX>
__device__ __forceinline__ void row_arg(float& v, int& n) {
  row_arg_step<0xB1, MAX>(v, n);
  row_arg_step<0x4E, MAX>(v, n);
  row_arg_step<0x141, MAX>(v, n);
  row_arg_step<0x140, MAX>(v, n);
}
__device__ __forceinline__ float row_max(float v) {
  v = fmaxf(v, dpp_mov<0xB1>(v));
  v = fmaxf(v, dpp_mov<0x4E>(v));
  v = fmaxf(v, dpp_mov<0x141>(v));
  return fmaxf(v, dpp_mov<0x140>(v));
}

// One footprint sample and its derivative by (qx, qy).  Branch-free: an off-map (or NaN) point reads cell (0, 0) and selects off_map with a
// zero derivative, so every index is in [0, H*W).
__device__ __forceinline__ float sample_map(const MfTrajObjDesc& d, const float* __restrict__ map, float qx, float qy, float* dsx, float* dsy) {
  const float u = (qx + d.d_max) / d.grid_res, v = (qy + d.d_max) / d.grid_res;
  const bool on = u >= 0.0f && u <= (float)(d.H - 1) && v >= 0.0f && v <= (float)(d.W - 1);
  const float us = on ? u : 0.0f, vs = on ? v : 0.0f;
  const int ix = min((int)floorf(us), d.H - 2), iy = min((int)floorf(vs), d.W - 2);
  const float fx = us - (float)ix, fy = vs - (float)iy;
  const float* m = map + ix * d.W + iy;
  const float m00 = m[0], m01 = m[1], m10 = m[d.W], m11 = m[d.W + 1];
  const float gx = 1.0f - fx, gy = 1.0f - fy;
  const float s = (gx * gy) * m00 + (fx * gy) * m10 + (gx * fy) * m01 + (fx * fy) * m11;
  if (dsx) {
    *dsx = on ? (gy * (m10 - m00) + fy * (m11 - m01)) / d.grid_res : 0.0f;
    *dsy = on ? (gx * (m01 - m00) + fx * (m11 - m10)) / d.grid_res : 0.0f;
  }
  return on ? s : d.off_map;
}

// (x, y) minus its closest point on the segment a -> b
__device__ __forceinline__ float2 seg_offset(float x, float y, float2 a, float2 b) {
  const float abx = b.x - a.x, aby = b.y - a.y, apx = x - a.x, apy = y - a.y;
  const float len2 = abx * abx + aby * aby;
  const float t = len2 > 0.0f ? mf_clamp((apx * abx + apy * aby) / len2, 0.0f, 1.0f) : 0.0f;
  return make_float2(apx - t * abx, apy - t * aby);
}

__global__ void __launch_bounds__(kObjBlock) traj_objective_kernel(const MfTrajObjDesc d, const int Tp, const float* __restrict__ Xs,
                                                                   const float* __restrict__ Rs, const float* __restrict__ points,
                                                                   const float* __restrict__ map, const float* __restrict__ path,
                                                                   const float* __restrict__ goal, const float* __restrict__ gcosts,
                                                                   float* __restrict__ costs, float* __restrict__ terms,
                                                                   float* __restrict__ gXs, float* __restrict__ gRs) {
  __shared__ float2 s_path[kObjPathMax];
  __shared__ float4 s_pts[kObjPointsMax];
  __shared__ float s_map[kObjRows], s_xt[kObjRows], s_incl[kObjRows], s_lethal[kObjRows], s_goal;
  const int l = threadIdx.x & 15, row = threadIdx.x >> 4;
  const int b = blockIdx.x;      // < d.B: the grid is B workgroups
  for (int i = threadIdx.x; i < d.P; i += kObjBlock) s_path[i] = make_float2(path[2 * i], path[2 * i + 1]);
  for (int n = threadIdx.x; n < d.N; n += kObjBlock) s_pts[n] = make_float4(points[3 * n], points[3 * n + 1], points[3 * n + 2], 0.0f);
  __syncthreads();
  const bool has_map = map != nullptr, want_grad = gXs != nullptr;
  const int nseg = max(d.P - 1, 1);
  const int64_t xb = (int64_t)b * d.x_stride_b, rb = (int64_t)b * d.r_stride_b;
  // the rows of the steps that are not kept: zeros (the kept steps are the multiples of the stride and T - 1; their rows are stored below)
  if (want_grad) {
    for (int t = threadIdx.x; t < d.T; t += kObjBlock) {
      if (t % d.pose_stride == 0 || t == d.T - 1) continue;
      float* gx = gXs + xb + (int64_t)t * d.x_stride_t;
      float* gr = gRs + rb + (int64_t)t * d.r_stride_t;
      gx[0] = 0.0f; gx[1] = 0.0f; gx[2] = 0.0f;
#pragma unroll
      for (int k = 0; k < 9; ++k) gr[k] = 0.0f;
    }
  }
  const float gc = gcosts ? gcosts[b] : 1.0f;
  const float c_map = gc * d.w_map / (float)Tp, c_path = gc * d.w_path / (float)Tp, c_incl = gc * d.w_incl / (float)Tp, c_goal = gc * d.w_goal;
  const float goal_x = goal[0], goal_y = goal[1];
  float map_sum = 0.0f, path_sum = 0.0f, incl_sum = 0.0f, lethal = 0.0f;
  for (int p = row; p < Tp; p += kObjRows) {      // (a row enters or leaves the loop whole: the DPP steps below read active lanes only)
    const int t = (int)min((long long)p * d.pose_stride, (long long)d.T - 1);
    const float* xp = Xs + xb + (int64_t)t * d.x_stride_t;
    const float* rp = Rs + rb + (int64_t)t * d.r_stride_t;
    const float x = xp[0], y = xp[1];
    float gx0 = 0.0f, gx1 = 0.0f;                 // d J / d (x, y) of this pose
    float ax = 0.0f, ay = 0.0f;                   // d J / d q of the arg-max footprint point
    float4 pt = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    if (has_map) {
      const float r00 = rp[0], r01 = rp[1], r02 = rp[2], r10 = rp[3], r11 = rp[4], r12 = rp[5];
      float f = -INFINITY, bad = 0.0f;
      int nb = l < d.N ? l : INT_MAX;
      for (int n = l; n < d.N; n += 16) {
        const float4 q = s_pts[n];
        const float sv = sample_map(d, map, x + (r00 * q.x + r01 * q.y + r02 * q.z), y + (r10 * q.x + r11 * q.y + r12 * q.z), nullptr, nullptr);
        bad = sv < d.lethal ? bad : 1.0f;
        if (sv > f) { f = sv; nb = n; }
      }
      row_arg<true>(f, nb);
      map_sum += f;
      lethal = fmaxf(lethal, row_max(bad));
      pt = s_pts[min(nb, d.N - 1)];               // (nb < N already: lane 0 of the row holds point 0 at least)
      float dsx, dsy;
      sample_map(d, map, x + (r00 * pt.x + r01 * pt.y + r02 * pt.z), y + (r10 * pt.x + r11 * pt.y + r12 * pt.z), &dsx, &dsy);
      ax = c_map * dsx; ay = c_map * dsy;
      gx0 = ax; gx1 = ay;
    }
    if (d.P > 0) {
      float d2 = INFINITY, bad = 0.0f;
      int kb = INT_MAX;
      for (int k = l; k < nseg; k += 16) {
        const float2 o = seg_offset(x, y, s_path[k], s_path[min(k + 1, d.P - 1)]);
        const float v = o.x * o.x + o.y * o.y;
        bad = v != v ? 1.0f : bad;
        if (v < d2) { d2 = v; kb = k; }
      }
      row_arg<false>(d2, kb);
      bad = row_max(bad);
      kb = kb == INT_MAX ? 0 : kb;                // (every distance infinite or NaN)
      const float2 o = seg_offset(x, y, s_path[kb], s_path[min(kb + 1, d.P - 1)]);
      float dist = sqrtf(o.x * o.x + o.y * o.y);
      dist = bad != 0.0f ? NAN : dist;            // a NaN position gives a NaN term
      path_sum += dist;
      gx0 += dist > 0.0f ? c_path * (o.x / dist) : (dist == 0.0f ? 0.0f : NAN);
      gx1 += dist > 0.0f ? c_path * (o.y / dist) : (dist == 0.0f ? 0.0f : NAN);
    }
    // inclination from the normalised third row
    float g20, g21, g22;
    {
      const float r0 = rp[6], r1 = rp[7], r2 = rp[8];
      const float nrm = sqrtf(r0 * r0 + r1 * r1 + r2 * r2);
      const float h0 = r0 / nrm, h1 = r1 / nrm, h2 = r2 / nrm;
      const float roll = atan2f(h1, h2);
      const float sp = mf_clamp(-h0, -1.0f, 1.0f);
      const float pitch = asinf(sp);
      incl_sum += fabsf(roll) + fabsf(pitch);
      // d roll / d r = (0, r2, -r1) / (r1^2 + r2^2): atan2 does not see the scale of r
      const float den = r1 * r1 + r2 * r2;
      const float s_roll = roll > 0.0f ? c_incl : (roll < 0.0f ? -c_incl : (roll == 0.0f ? 0.0f : NAN));
      const float dr1 = roll != 0.0f ? s_roll * (r2 / den) : 0.0f, dr2 = roll != 0.0f ? s_roll * (-r1 / den) : 0.0f;
      // d pitch / d r_j = -(delta_0j - h0 h_j) / (|r| sqrt(1 - h0^2)); zero where the clamp holds
      const bool open = -h0 > -1.0f && -h0 < 1.0f;
      const float s_pitch = pitch > 0.0f ? c_incl : (pitch < 0.0f ? -c_incl : (pitch == 0.0f ? 0.0f : NAN));
      const float c2 = 1.0f - h0 * h0;
      const float k = open && pitch != 0.0f ? s_pitch / (nrm * sqrtf(c2)) : 0.0f;
      g20 = -(k * c2);
      g21 = dr1 + k * (h0 * h1);
      g22 = dr2 + k * (h0 * h2);
    }
    // the distance to the goal, at the last kept pose (t = T - 1)
    if (p == Tp - 1) {
      const float ex = x - goal_x, ey = y - goal_y;
      const float dist = sqrtf(ex * ex + ey * ey);
      if (l == 0) s_goal = dist;
      gx0 += dist > 0.0f ? c_goal * (ex / dist) : (dist == 0.0f ? 0.0f : NAN);
      gx1 += dist > 0.0f ? c_goal * (ey / dist) : (dist == 0.0f ? 0.0f : NAN);
    }
    if (want_grad && l < 12) {
      if (l < 3) {
        gXs[xb + (int64_t)t * d.x_stride_t + l] = l == 0 ? gx0 : (l == 1 ? gx1 : 0.0f);
      } else {
        const int j = l - 3, i = j / 3, c = j - 3 * i;
        const float pc = c == 0 ? pt.x : (c == 1 ? pt.y : pt.z);
        const float g2 = c == 0 ? g20 : (c == 1 ? g21 : g22);
        gRs[rb + (int64_t)t * d.r_stride_t + j] = i == 0 ? ax * pc : (i == 1 ? ay * pc : g2);
      }
    }
  }
  if (l == 0) { s_map[row] = map_sum; s_xt[row] = path_sum; s_incl[row] = incl_sum; s_lethal[row] = lethal; }
  __syncthreads();
  if (threadIdx.x != 0) return;
  for (int k = 1; k < kObjRows; ++k) { map_sum += s_map[k]; path_sum += s_xt[k]; incl_sum += s_incl[k]; lethal = fmaxf(lethal, s_lethal[k]); }
  const bool is_lethal = lethal != 0.0f;
  const float mp = has_map ? (is_lethal ? INFINITY : map_sum / (float)Tp) : 0.0f;
  const float xt = d.P > 0 ? path_sum / (float)Tp : 0.0f;
  const float gl = s_goal, incl = incl_sum / (float)Tp;
  float c = 0.0f;
  if (has_map) c = is_lethal ? INFINITY : d.w_map * mp;
  if (d.P > 0) c = c + d.w_path * xt;
  c = c + d.w_goal * gl;
  c = c + d.w_incl * incl;
  costs[b] = c;
  if (terms) { terms[4 * b] = mp; terms[4 * b + 1] = xt; terms[4 * b + 2] = gl; terms[4 * b + 3] = incl; }
}

}  // namespace mf

static int traj_objective_check(const MfTrajObjDesc* d, const float* Xs, const float* Rs, const float* points, const float* cost_map,
                                const float* path, const float* goal, const float* costs, const float* gXs, const float* gRs) {
  MF_REQUIRE(d, MF_ERR_INVALID, "traj_objective: null descriptor");
  MF_REQUIRE(Xs && Rs && points && goal && costs, MF_ERR_INVALID, "traj_objective: null argument (Xs, Rs, points, goal and costs are required)");
  MF_REQUIRE((gXs != nullptr) == (gRs != nullptr), MF_ERR_INVALID, "traj_objective: gXs and gRs must both be given or both be NULL");
  MF_REQUIRE(d->B > 0 && d->T > 0 && d->N > 0, MF_ERR_INVALID, "traj_objective: B, T and N must be positive");
  MF_REQUIRE(d->pose_stride > 0, MF_ERR_INVALID, "traj_objective: pose_stride must be positive");
  MF_REQUIRE(d->N <= mf::kObjPointsMax, MF_ERR_UNSUPPORTED, "traj_objective: at most 1024 footprint points");
  MF_REQUIRE(d->P >= 0, MF_ERR_INVALID, "traj_objective: P must not be negative");
  MF_REQUIRE(d->P <= mf::kObjPathMax, MF_ERR_UNSUPPORTED, "traj_objective: at most 256 path vertices");
  MF_REQUIRE(d->H >= 2 && d->W >= 2, MF_ERR_INVALID, "traj_objective: the cost map needs H >= 2 and W >= 2");
  MF_REQUIRE(d->x_stride_b >= 0 && d->x_stride_t >= 0 && d->r_stride_b >= 0 && d->r_stride_t >= 0, MF_ERR_INVALID, "traj_objective: negative stride");
  MF_REQUIRE(d->grid_res > 0.0f, MF_ERR_INVALID, "traj_objective: grid_res must be positive");
  MF_REQUIRE(d->lethal == d->lethal && d->off_map == d->off_map, MF_ERR_INVALID, "traj_objective: lethal and off_map must not be NaN");
  MF_REQUIRE(cost_map || d->w_map == 0.0f, MF_ERR_INVALID, "traj_objective: w_map needs a cost_map (NULL requires w_map == 0)");
  MF_REQUIRE((path != nullptr) == (d->P > 0), MF_ERR_INVALID, "traj_objective: path must be NULL exactly when P is 0");
  MF_REQUIRE(d->P > 0 || d->w_path == 0.0f, MF_ERR_INVALID, "traj_objective: w_path needs a path (P == 0 requires w_path == 0)");
  const long long lim = 1ll << 31;
  MF_REQUIRE((long long)d->H * d->W < lim, MF_ERR_UNSUPPORTED, "traj_objective: H * W must stay below 2^31");
  // (each factor is below 2^31 and the strides are checked one at a time first, so the sums cannot overflow 64 bits unnoticed)
  MF_REQUIRE(d->x_stride_b < lim && d->x_stride_t < lim && d->r_stride_b < lim && d->r_stride_t < lim, MF_ERR_UNSUPPORTED,
             "traj_objective: strides must stay below 2^31");
  MF_REQUIRE((d->B - 1) * d->x_stride_b + (d->T - 1) * d->x_stride_t + 3 < lim && (d->B - 1) * d->r_stride_b + (d->T - 1) * d->r_stride_t + 9 < lim,
             MF_ERR_UNSUPPORTED, "traj_objective: the pose rows' index range must stay below 2^31");
  return MF_OK;
}

extern "C" int mf_traj_objective_f32(const MfTrajObjDesc* d, const float* Xs, const float* Rs, const float* points, const float* cost_map,
                                     const float* path, const float* goal, const float* gcosts, float* costs, float* terms, float* gXs, float* gRs,
                                     void* stream) {
  int rc = traj_objective_check(d, Xs, Rs, points, cost_map, path, goal, costs, gXs, gRs);
  if (rc != MF_OK) return rc;
  const int Tp = 1 + (int)(((long long)d->T - 1 + d->pose_stride - 1) / d->pose_stride);
  hipLaunchKernelGGL(mf::traj_objective_kernel, dim3(d->B), dim3(mf::kObjBlock), 0, (hipStream_t)stream, *d, Tp, Xs, Rs, points, cost_map, path, goal,
                     gcosts, costs, terms, gXs, gRs);
  hipError_t e = hipGetLastError();
  MF_REQUIRE(e == hipSuccess, MF_ERR_LAUNCH, std::string("traj_objective launch: ") + hipGetErrorString(e));
  return MF_OK;
}
