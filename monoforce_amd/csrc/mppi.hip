// MPPI (model-predictive path integral) iteration around the path-cost rollout: perturb the nominal controls, score the rolled-out
// sequences, average them with softmin weights.  Three entry points, float32, each a few small launches on the caller's stream:
//   mf_mppi_perturb_f32   controls = clamp(nominal + sigma * noise)                          one launch, one pass over [B][T][2]
//   mf_path_costs_f32     inclination / force / goal cost of every rollout from its rows     one launch: a rollout per lane, the steps of a
//                         rollout dealt round-robin to the S waves of its workgroup, the S partial sums added in wave order
//   mf_mppi_update_f32    weights and the new nominal                                        statistics (one workgroup) -> partial sums over
//                         (64-rollout chunk, 64-step tile) -> sum of the chunks; no float atomics: bit-identical from call to call
// Built by the plain rule (-ffp-contract=off): a product and the sum it feeds round separately, like the ATen ops this replaces.
#include "mf_common.h"

#include <limits.h>
#include <math.h>

namespace mf {

constexpr int kCostSlicesMax = 16;   // waves that share the steps of one 64-rollout group (path costs)
constexpr int kUpdChunk = 64;        // rollouts per partial sum of the update
constexpr int kStatsBlock = 1024;    // threads of the statistics workgroup
constexpr int kFinishSlices = 16;    // waves that share the chunks of one 64-step tile (finish)

__global__ void __launch_bounds__(256) mppi_perturb_kernel(const MfMppiDesc d, const float2* __restrict__ nominal, const float2* __restrict__ noise,
                                                           float2* __restrict__ controls) {
  const int i = blockIdx.x * 256 + threadIdx.x;      // (b, t); B * T < 2^29
  if (i >= d.B * d.T) return;
  const int b = i / d.T, t = i - b * d.T;
  float2 u = nominal[t];
  if (!(d.keep_nominal && b == 0)) {
    const float2 n = noise[i];
    u.x = u.x + d.sigma[0] * n.x;
    u.y = u.y + d.sigma[1] * n.y;
  }
  controls[i] = make_float2(mf_clamp(u.x, d.lo[0], d.hi[0]), mf_clamp(u.y, d.lo[1], d.hi[1]));
}

// VEC: rows are 16-byte aligned (the rollout's own [T][B][4] buffer, or any layout whose strides are multiples of four elements)
template <bool VEC>
__global__ void __launch_bounds__(64 * kCostSlicesMax) path_costs_kernel(const MfMppiDesc d, const float* __restrict__ rows, const float* __restrict__ force,
                                                                         const float* __restrict__ x_last, const float* __restrict__ goal,
                                                                         float* __restrict__ costs, float* __restrict__ terms) {
  __shared__ float2 part[kCostSlicesMax][64];
  const int lane = threadIdx.x & 63, s = threadIdx.x >> 6, S = blockDim.x >> 6;
  const int b = blockIdx.x * 64 + lane;
  float roll = 0.0f, pitch = 0.0f;
  if (b < d.B) {
    const float* p = rows + (int64_t)b * d.row_stride_b;
#pragma unroll 4
    for (int t = s; t < d.T; t += S) {
      const float* q = p + (int64_t)t * d.row_stride_t;
      float r0, r1, r2;
      if (VEC) {
        const float4 r = *reinterpret_cast<const float4*>(q);
        r0 = r.x; r1 = r.y; r2 = r.z;
      } else {
        r0 = q[0]; r1 = q[1]; r2 = q[2];
      }
      roll += fabsf(atan2f(r1, r2));
      pitch += fabsf(asinf(mf_clamp(-r0, -1.0f, 1.0f)));
    }
  }
  part[s][lane] = make_float2(roll, pitch);
  __syncthreads();
  if (s != 0 || b >= d.B) return;
  float2 tot = part[0][lane];
  for (int k = 1; k < S; ++k) { tot.x += part[k][lane].x; tot.y += part[k][lane].y; }
  const float incl = tot.x / (float)d.T + tot.y / (float)d.T;
  const float f = force ? force[b] : 0.0f;
  const float dx = x_last[(int64_t)b * d.x_stride_b] - goal[0], dy = x_last[(int64_t)b * d.x_stride_b + 1] - goal[1];
  const float g = sqrtf(dx * dx + dy * dy);
  costs[b] = d.w_incl * incl + d.w_force * f + d.w_goal * g;
  if (terms) { terms[3 * b] = incl; terms[3 * b + 1] = f; terms[3 * b + 2] = g; }
}

// One workgroup: number, minimum and first arg-minimum of the finite costs, then the normalised weights.  Thread i owns the costs
// i, i + 1024, ...; its values meet the others' in a fixed binary tree over LDS.
__global__ void __launch_bounds__(kStatsBlock) mppi_stats_kernel(const MfMppiDesc d, const float* __restrict__ costs, float* __restrict__ weights,
                                                                 int32_t* __restrict__ best, int32_t* __restrict__ n_valid) {
  __shared__ float s_val[kStatsBlock];
  __shared__ int s_idx[kStatsBlock], s_cnt[kStatsBlock];
  const int tid = threadIdx.x;
  float mn = INFINITY;
  int idx = INT_MAX, cnt = 0;
  for (int b = tid; b < d.B; b += kStatsBlock) {
    const float c = costs[b];
    if (isfinite(c)) {
      ++cnt;
      if (c < mn) { mn = c; idx = b; }      // strict: the first of equal costs stays (b grows)
    }
  }
  s_val[tid] = mn; s_idx[tid] = idx; s_cnt[tid] = cnt;
  __syncthreads();
  for (int off = kStatsBlock / 2; off > 0; off >>= 1) {
    if (tid < off) {
      const float ov = s_val[tid + off];
      const int oi = s_idx[tid + off];
      if (ov < s_val[tid] || (ov == s_val[tid] && oi < s_idx[tid])) { s_val[tid] = ov; s_idx[tid] = oi; }
      s_cnt[tid] += s_cnt[tid + off];
    }
    __syncthreads();
  }
  const float cmin = s_val[0];
  const int nv = s_cnt[0], first = s_idx[0];
  __syncthreads();
  float acc = 0.0f;
  for (int b = tid; b < d.B; b += kStatsBlock) {
    const float c = costs[b];
    const float e = isfinite(c) ? expf(-(c - cmin) / d.lambda) : 0.0f;
    weights[b] = e;
    acc += e;
  }
  s_val[tid] = acc;
  __syncthreads();
  for (int off = kStatsBlock / 2; off > 0; off >>= 1) {
    if (tid < off) s_val[tid] += s_val[tid + off];
    __syncthreads();
  }
  const float sum = s_val[0];      // >= 1 when nv > 0: the minimum itself contributes exp(0)
  if (nv > 0)
    for (int b = tid; b < d.B; b += kStatsBlock) weights[b] = weights[b] / sum;      // (each thread re-reads only what it wrote)
  if (tid == 0) { best[0] = nv > 0 ? first : -1; n_valid[0] = nv; }
}

// partial[chunk][t] = sum over the chunk's rollouts, in order, of weights[b] * controls[b][t]: a wave = one chunk x 64 steps (the weight is
// wave-uniform, a step's (v, w) pair one 8-byte load), four chunks per workgroup.
__global__ void __launch_bounds__(256) mppi_partial_kernel(const MfMppiDesc d, int t_tiles, const float* __restrict__ weights,
                                                           const float2* __restrict__ controls, float2* __restrict__ partial) {
  const int cb = blockIdx.x / t_tiles, tb = blockIdx.x - cb * t_tiles;
  const int chunk = cb * 4 + (int)(threadIdx.x >> 6), t = tb * 64 + (int)(threadIdx.x & 63);
  const int n_chunks = (d.B + kUpdChunk - 1) / kUpdChunk;
  if (chunk >= n_chunks || t >= d.T) return;
  const int b0 = chunk * kUpdChunk, b1 = min(d.B, b0 + kUpdChunk);
  float2 acc = make_float2(0.0f, 0.0f);
#pragma unroll 8
  for (int b = b0; b < b1; ++b) {
    const float w = weights[b];
    const float2 u = controls[(size_t)b * d.T + t];
    acc.x = acc.x + w * u.x;
    acc.y = acc.y + w * u.y;
  }
  partial[(size_t)chunk * d.T + t] = acc;
}

// nominal_out[t] = sum of the chunks' partial sums: the chunks of a 64-step tile are split into 16 consecutive runs, one per wave, each
// added in order; wave 0 adds the 16 run totals in order.  No finite cost: the old nominal.
__global__ void __launch_bounds__(64 * kFinishSlices) mppi_finish_kernel(const MfMppiDesc d, const float2* __restrict__ partial, const float2* nominal_in,
                                                                         const int32_t* __restrict__ n_valid, float2* nominal_out) {
  __shared__ float2 part[kFinishSlices][64];
  const int lane = threadIdx.x & 63, s = threadIdx.x >> 6;
  const int t = blockIdx.x * 64 + lane;
  const int n_chunks = (d.B + kUpdChunk - 1) / kUpdChunk, per = (n_chunks + kFinishSlices - 1) / kFinishSlices;
  float2 acc = make_float2(0.0f, 0.0f);
  if (t < d.T) {
    const int c1 = min(n_chunks, (s + 1) * per);
#pragma unroll 4
    for (int c = s * per; c < c1; ++c) {
      const float2 p = partial[(size_t)c * d.T + t];
      acc.x += p.x; acc.y += p.y;
    }
  }
  part[s][lane] = acc;
  __syncthreads();
  if (s != 0 || t >= d.T) return;
  float2 tot = part[0][lane];
#pragma unroll
  for (int k = 1; k < kFinishSlices; ++k) { tot.x += part[k][lane].x; tot.y += part[k][lane].y; }
  if (n_valid[0] == 0) tot = nominal_in[t];
  nominal_out[t] = tot;
}

}  // namespace mf

static int mppi_check(const MfMppiDesc* d, const char* what) {
  const std::string w(what);
  MF_REQUIRE(d, MF_ERR_INVALID, w + ": null descriptor");
  MF_REQUIRE(d->B > 0 && d->T > 0, MF_ERR_INVALID, w + ": B and T must be positive");
  MF_REQUIRE(d->lambda > 0.0f, MF_ERR_INVALID, w + ": lambda must be positive");
  MF_REQUIRE(d->sigma[0] >= 0.0f && d->sigma[1] >= 0.0f, MF_ERR_INVALID, w + ": sigma must not be negative");
  MF_REQUIRE(d->lo[0] <= d->hi[0] && d->lo[1] <= d->hi[1], MF_ERR_INVALID, w + ": control limits need lo <= hi");
  MF_REQUIRE((long long)d->B * d->T * 4 < (1ll << 31), MF_ERR_UNSUPPORTED, w + ": B * T * 4 must stay below 2^31");
  return MF_OK;
}

static inline bool aligned(const void* p, uintptr_t a) { return ((uintptr_t)p & (a - 1)) == 0; }

#define MPPI_LAUNCHED(what)                                                                                   \
  do {                                                                                                        \
    hipError_t e_ = hipGetLastError();                                                                        \
    MF_REQUIRE(e_ == hipSuccess, MF_ERR_LAUNCH, std::string(what " launch: ") + hipGetErrorString(e_));       \
  } while (0)

extern "C" int mf_mppi_perturb_f32(const MfMppiDesc* d, const float* nominal, const float* noise, float* controls, void* stream) {
  int rc = mppi_check(d, "mppi_perturb");
  if (rc != MF_OK) return rc;
  MF_REQUIRE(nominal && noise && controls, MF_ERR_INVALID, "mppi_perturb: null argument");
  MF_REQUIRE(aligned(nominal, 8) && aligned(noise, 8) && aligned(controls, 8), MF_ERR_INVALID, "mppi_perturb: (v, w) buffers must be 8-byte aligned");
  const int n = d->B * d->T;
  hipLaunchKernelGGL(mf::mppi_perturb_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, *d, (const float2*)nominal, (const float2*)noise,
                     (float2*)controls);
  MPPI_LAUNCHED("mppi_perturb");
  return MF_OK;
}

extern "C" int mf_path_costs_f32(const MfMppiDesc* d, const float* cost_rows, const float* force_cost, const float* x_last, const float* goal,
                                 float* costs, float* terms, void* stream) {
  int rc = mppi_check(d, "path_costs");
  if (rc != MF_OK) return rc;
  MF_REQUIRE(cost_rows && x_last && goal && costs, MF_ERR_INVALID, "path_costs: null argument");
  MF_REQUIRE((force_cost == nullptr) == (d->w_force == 0.0f), MF_ERR_INVALID, "path_costs: force_cost must be NULL exactly when w_force is 0");
  MF_REQUIRE(d->row_stride_b >= 0 && d->row_stride_t >= 0 && d->x_stride_b >= 0, MF_ERR_INVALID, "path_costs: negative stride");
  // waves per 64-rollout group: enough of them to fill the chip (1024 SIMDs) twice over at small B, fewer as the groups multiply
  const int S = d->B <= 8192 ? 16 : (d->B <= 16384 ? 8 : 4);
  const bool vec = aligned(cost_rows, 16) && d->row_stride_b % 4 == 0 && d->row_stride_t % 4 == 0;
  const dim3 grid((d->B + 63) / 64), block(64 * S);
  if (vec)
    hipLaunchKernelGGL(mf::path_costs_kernel<true>, grid, block, 0, (hipStream_t)stream, *d, cost_rows, force_cost, x_last, goal, costs, terms);
  else
    hipLaunchKernelGGL(mf::path_costs_kernel<false>, grid, block, 0, (hipStream_t)stream, *d, cost_rows, force_cost, x_last, goal, costs, terms);
  MPPI_LAUNCHED("path_costs");
  return MF_OK;
}

extern "C" long long mf_mppi_scratch_bytes(const MfMppiDesc* d) {
  if (mppi_check(d, "mppi_scratch_bytes") != MF_OK) return -1;
  return (long long)((d->B + mf::kUpdChunk - 1) / mf::kUpdChunk) * d->T * (long long)sizeof(float2);
}

extern "C" int mf_mppi_update_f32(const MfMppiDesc* d, const float* costs, const float* controls, const float* nominal_in, float* weights,
                                  float* nominal_out, int32_t* best, int32_t* n_valid, void* scratch, long long scratch_bytes, void* stream) {
  int rc = mppi_check(d, "mppi_update");
  if (rc != MF_OK) return rc;
  MF_REQUIRE(costs && controls && nominal_in && weights && nominal_out && best && n_valid && scratch, MF_ERR_INVALID, "mppi_update: null argument");
  MF_REQUIRE(scratch_bytes >= mf_mppi_scratch_bytes(d), MF_ERR_INVALID, "mppi_update: scratch buffer too small (mf_mppi_scratch_bytes)");
  MF_REQUIRE(aligned(controls, 8) && aligned(nominal_in, 8) && aligned(nominal_out, 8) && aligned(scratch, 8), MF_ERR_INVALID,
             "mppi_update: (v, w) buffers and scratch must be 8-byte aligned");
  hipStream_t st = (hipStream_t)stream;
  hipLaunchKernelGGL(mf::mppi_stats_kernel, dim3(1), dim3(mf::kStatsBlock), 0, st, *d, costs, weights, best, n_valid);
  MPPI_LAUNCHED("mppi_update (statistics)");
  const int n_chunks = (d->B + mf::kUpdChunk - 1) / mf::kUpdChunk, t_tiles = (d->T + 63) / 64;
  hipLaunchKernelGGL(mf::mppi_partial_kernel, dim3((unsigned)((n_chunks + 3) / 4) * t_tiles), dim3(256), 0, st, *d, t_tiles, weights,
                     (const float2*)controls, (float2*)scratch);
  MPPI_LAUNCHED("mppi_update (partial sums)");
  hipLaunchKernelGGL(mf::mppi_finish_kernel, dim3(t_tiles), dim3(64 * mf::kFinishSlices), 0, st, *d, (const float2*)scratch, (const float2*)nominal_in,
                     n_valid, (float2*)nominal_out);
  MPPI_LAUNCHED("mppi_update (finish)");
  return MF_OK;
}
