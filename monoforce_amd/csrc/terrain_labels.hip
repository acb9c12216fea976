// Rigid-terrain label maps (the reference's datasets/rough.py:621-649 with :343-365 and :545-601) on the GPU for a batch of samples: the cloud
// projected into every camera's segmentation mask, the points with a rigid label gravity-aligned, the robot's footprint swept along the
// recorded poses, and the per-cell maximum of both -- without a cloud in between.  Three launches on one stream, as in heightmap.hip:
// sentinel fill, one thread per item (a cloud point or a footprint point), finalize; blockIdx.y is the sample.  The definition is the
// comment of MfTerrainLabelsDesc in include/monoforce_hip.h; this unit is built with -ffp-contract=off, and every operation below rounds
// on its own, in the order written.
#include <math.h>

#include "mf_common.h"

namespace mf {

// The three helpers of heightmap.hip, restated (that unit stays as it is): the same order-preserving key, the same bucket search.
__device__ __forceinline__ int tl_order_key(float v) {
  const int b = __builtin_bit_cast(int, v);
  return b >= 0 ? b : (b ^ 0x7FFFFFFF);
}
__device__ __forceinline__ float tl_order_value(int k) { return __builtin_bit_cast(float, k >= 0 ? k : (k ^ 0x7FFFFFFF)); }
// torch.bucketize(x, bins) - 1 with right = False: (number of edges strictly below x) - 1
__device__ __forceinline__ int tl_bucket(const float* __restrict__ bins, int n, float x, float inv_res) {
  int g = (int)floorf((x - bins[0]) * inv_res);
  g = min(max(g, 0), n - 1);
  while (g + 1 < n && bins[g + 1] < x) ++g;
  while (g >= 0 && !(bins[g] < x)) --g;
  return g;
}

__global__ void __launch_bounds__(256) tl_fill_kernel(int* __restrict__ keys, long long n) {
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) keys[i] = INT_MIN;
}

// row r of a [3][4] float64 pose applied to (x, y, z), the translation given separately
__device__ __forceinline__ double pose_row(const double* __restrict__ P, int r, double x, double y, double z, double t) {
  return ((P[r * 4 + 0] * x + P[r * 4 + 1] * y) + P[r * 4 + 2] * z) + t;
}

__global__ void __launch_bounds__(256) tl_scatter_kernel(const MfTerrainLabelsDesc d, const float* __restrict__ pts, const int* __restrict__ offsets,
                                                         const uint8_t* __restrict__ seg, const float* __restrict__ rots,
                                                         const float* __restrict__ trans, const float* __restrict__ intrins,
                                                         const double* __restrict__ pose_align, const double* __restrict__ poses,
                                                         const float* __restrict__ fx, const float* __restrict__ fy, const float* __restrict__ xb,
                                                         const float* __restrict__ yb, int* __restrict__ keys, int16_t* __restrict__ labels) {
  const int s = blockIdx.y;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;
  // the sample's slice of the cloud, held inside [0, n_points] whatever the offsets say
  const int o0 = min(max(offsets[s], 0), d.n_points), o1 = min(max(offsets[s + 1], o0), d.n_points);
  const int n_s = o1 - o0, F = d.Fx * d.Fy;
  float gx, gy, gz;
  if (i < n_s) {
    const size_t row = (size_t)(o0 + i);
    const float px = pts[row * 3 + 0], py = pts[row * 3 + 1], pz = pts[row * 3 + 2];
    bool kept = false;
    for (int c = 0; c < d.C; ++c) {
      const float* __restrict__ R = rots + (size_t)s * d.rots_stride_s + c * 9;
      const float* __restrict__ t = trans + (size_t)s * d.trans_stride_s + c * 3;
      const float* __restrict__ K = intrins + (size_t)s * d.intrins_stride_s + c * 9;
      const float ax = px - t[0], ay = py - t[1], az = pz - t[2];                       // utils.py:16
      float q[3], w[3];
#pragma unroll
      for (int k = 0; k < 3; ++k) q[k] = (R[0 + k] * ax + R[3 + k] * ay) + R[6 + k] * az;       // :17 rot^T
#pragma unroll
      for (int k = 0; k < 3; ++k) w[k] = (K[k * 3 + 0] * q[0] + K[k * 3 + 1] * q[1]) + K[k * 3 + 2] * q[2];       // :19
      const float u = w[0] / w[2], v = w[1] / w[2];                                       // :20
      const bool seen = w[2] > 0.0f && u > 1.0f && u < (float)(d.Wi - 1) && v > 1.0f && v < (float)(d.Hi - 1);       // :38-43 (false for NaN)
      int lab = -1;
      if (seen) lab = seg[(((size_t)s * d.C + c) * d.Hi + (int)v) * d.Wi + (int)u];       // rough.py:574-575: truncation; 1 < u < Wi - 1 keeps it inside
      if (labels) labels[row * d.C + c] = (int16_t)lab;
      if (lab >= 0 && ((d.class_set[lab >> 5] >> (lab & 31)) & 1u)) kept = true;
      if (kept && !labels) break;
    }
    if (!kept) return;
    if (isnan(px) || isnan(py) || isnan(pz)) return;       // (a NaN row is seen by no camera; stated for the definition's sake)
    const double* __restrict__ A = pose_align + (size_t)s * 12;
    gx = (float)pose_row(A, 0, (double)px, (double)py, (double)pz, A[3]);          // rough.py:591-592, float64 like the reference's
    gy = (float)pose_row(A, 1, (double)px, (double)py, (double)pz, A[7]);
    gz = (float)pose_row(A, 2, (double)px, (double)py, (double)pz, A[11]);
  } else {
    const int j = i - n_s;
    if (j >= d.T * F) return;
    const int t = j / F, r = j - t * F, iy = r / d.Fx, ix = r - iy * d.Fx;       // rough.py:348-350: meshgrid(x, y) rows are y
    const double* __restrict__ P = poses + ((size_t)s * d.T + t) * 12;
    const double x = (double)fx[ix], y = (double)fy[iy];
    gx = (float)pose_row(P, 0, x, y, 0.0, P[3]);
    gy = (float)pose_row(P, 1, x, y, 0.0, P[7]);
    gz = (float)pose_row(P, 2, x, y, 0.0, P[11] - fabs(d.clearance));       // :358
  }
  // estimate_heightmap's filters (heightmap.hip, cloudproc.py:88-133) on the float32 point
  if (isnan(gx) || isnan(gy) || isnan(gz)) return;
  if (d.r_min >= 0.0f) {
    const float dist = (float)sqrt((double)gx * (double)gx + (double)gy * (double)gy);
    if (!(dist > d.r_min)) return;
  }
  if (!(gx > -d.d_max && gx < d.d_max && gy > -d.d_max && gy < d.d_max && gz > d.h_min && gz < d.h_max)) return;
  const int bx = tl_bucket(xb, d.n, gx, d.inv_res), by = tl_bucket(yb, d.n, gy, d.inv_res);
  if (bx < 0 || by < 0) return;
  atomicMax(&keys[((size_t)s * d.n + by) * d.n + bx], tl_order_key(gz));
}

// hm[s][0][x][y] = max height (0 where nothing fell), hm[s][1][x][y] = 1 / 0
__global__ void __launch_bounds__(256) tl_finalize_kernel(const MfTerrainLabelsDesc d, const int* __restrict__ keys, float* __restrict__ hm) {
  const int s = blockIdx.y, cells = d.n * d.n;
  const int i = blockIdx.x * blockDim.x + threadIdx.x;      // output-major: i = x * n + y
  if (i >= cells) return;
  const int x = i / d.n, y = i - x * d.n;
  const int k = keys[(size_t)s * cells + y * d.n + x];
  const bool got = k != INT_MIN;
  float* __restrict__ out = hm + (size_t)s * 2 * cells;
  out[i] = got ? tl_order_value(k) : 0.0f;
  out[cells + i] = got ? 1.0f : 0.0f;
}

}  // namespace mf

extern "C" int mf_terrain_labels_f32(const MfTerrainLabelsDesc* d, const float* points, const int32_t* offsets, const uint8_t* seg,
                                     const float* rots, const float* trans, const float* intrins, const double* pose_align, const double* poses,
                                     const float* fx, const float* fy, const float* x_bins, const float* y_bins, int32_t* scratch, float* hm,
                                     int16_t* point_labels, void* stream) {
  MF_REQUIRE(d, MF_ERR_INVALID, "terrain_labels: null descriptor");
  MF_REQUIRE(d->S > 0 && d->S <= 65535 && d->n > 0 && d->C >= 0 && d->T >= 0 && d->Fx >= 0 && d->Fy >= 0 && d->n_points >= 0 && d->max_points >= 0 &&
                 d->max_points <= d->n_points,
             MF_ERR_INVALID, "terrain_labels: bad sizes (S in 1..65535, n > 0, the counts non-negative, max_points <= n_points)");
  MF_REQUIRE(d->C == 0 || (d->Hi >= 3 && d->Wi >= 3), MF_ERR_INVALID, "terrain_labels: masks must be at least 3 x 3");
  MF_REQUIRE(offsets && x_bins && y_bins && scratch && hm, MF_ERR_INVALID, "terrain_labels: null argument (offsets, bins, scratch and hm are required)");
  MF_REQUIRE(d->n_points == 0 || (points && pose_align), MF_ERR_INVALID, "terrain_labels: a cloud needs points and pose_align");
  MF_REQUIRE(d->n_points == 0 || d->C == 0 || (seg && rots && trans && intrins), MF_ERR_INVALID, "terrain_labels: cameras need seg, rots, trans and intrins");
  const long long F = (long long)d->Fx * d->Fy, TF = F * d->T;
  MF_REQUIRE(TF == 0 || (poses && fx && fy), MF_ERR_INVALID, "terrain_labels: a footprint sweep needs poses, fx and fy");
  MF_REQUIRE((d->rots_stride_s == 0 || d->rots_stride_s == 9ll * d->C) && (d->trans_stride_s == 0 || d->trans_stride_s == 3ll * d->C) &&
                 (d->intrins_stride_s == 0 || d->intrins_stride_s == 9ll * d->C),
             MF_ERR_INVALID, "terrain_labels: a camera stride is 0 (shared) or the size of one sample's cameras");
  MF_REQUIRE((long long)d->n * d->n < (1ll << 30) && (long long)d->S * d->n * d->n < (1ll << 31), MF_ERR_UNSUPPORTED, "terrain_labels: grid too large");
  MF_REQUIRE(d->max_points + TF < (1ll << 31) - 256, MF_ERR_UNSUPPORTED, "terrain_labels: too many items per sample");
  hipStream_t st = (hipStream_t)stream;
  const int cells = d->n * d->n;
  const long long all = (long long)d->S * cells;
  const long long items = d->max_points + TF;
  hipLaunchKernelGGL(mf::tl_fill_kernel, dim3((unsigned)((all + 255) / 256)), dim3(256), 0, st, scratch, all);
  if (items > 0)
    hipLaunchKernelGGL(mf::tl_scatter_kernel, dim3((unsigned)((items + 255) / 256), d->S), dim3(256), 0, st, *d, points, offsets, seg, rots, trans,
                       intrins, pose_align, poses, fx, fy, x_bins, y_bins, scratch, point_labels);
  hipLaunchKernelGGL(mf::tl_finalize_kernel, dim3((cells + 255) / 256, d->S), dim3(256), 0, st, *d, scratch, hm);
  hipError_t e = hipGetLastError();
  MF_REQUIRE(e == hipSuccess, MF_ERR_LAUNCH, std::string("terrain_labels launch: ") + hipGetErrorString(e));
  return MF_OK;
}
