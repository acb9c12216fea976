// Fused pose loss: physics_loss(..., rotation_loss=True) of the reference's monoforce/losses.py:102-138 (the position MSE of
// :116-127 AND the geodesic rotation term of :129-136 / rotation_difference :48-65) as one gather-reduce kernel and one scatter kernel --
// the call scripts/eval.py:151-153 makes on every batch, and the only supervision of the rollout's orientation.  The ATen form adds an
// advanced-index gather of [B,T2,3,3], a batched 3x3 matmul, diagonal, clip, arccos and a second sorting index_put_ backward to the ~25
// launches of the position term.  For i = b*T2 + j, near = nearest[i], w = 1 / (1 + gamma * gt_ts[i]):
//   loss     = (1 / 3BT2) sum_i sum_c (Xs[b,near,c]*w - Xgt[i,c]*w)^2                                (physics_loss.hip's term, same arithmetic)
//   loss_rot = (1 /  BT2) sum_i theta_i^2 * w,   theta = acos(clip((tr - 1) / 2, -1, 1)),   tr = sum_{r,k} Rs[b,near,r,k] * Rgt[i,r,k]
// (tr = trace(Rp Rg^T), the nine products added in row-major order).  The backward scatters d/dXs and d/dRs in the layout of the inputs
// (the rollout's time-major buffers: mf_rollout_bwd_* takes gXs / gRs in place):
//   gRs[b,near,:] (+)= gloss[1] * w / (BT2) * dtheta2 * Rgt[i,:],   dtheta2 = -theta / sqrt((1-c)(1+c)) for -1 < c < 1, else 0
// ONE difference from autograd: at c == +-1 exactly torch's arccos backward gives 0 * inf = NaN (identical rotations) or inf (an angle of
// exactly pi); here the rotation gradient is 0 there.  Outside the clip range both give 0.
// IEEE acos / sqrt / division (this TU is built without -ffast-math and with -ffp-contract=off, like physics_loss.hip).
#include "mf_common.h"

namespace mf {

__device__ __forceinline__ void pose_atomic_add(float* p, float v) { unsafeAtomicAdd(p, v); }
__device__ __forceinline__ void pose_atomic_add(double* p, double v) { unsafeAtomicAdd(p, v); }
__device__ __forceinline__ float pose_acos(float v) { return acosf(v); }
__device__ __forceinline__ double pose_acos(double v) { return acos(v); }

// clears `count` scalars at `p` with 16-byte stores (unaligned head and tail: scalar stores); thread i of n
template <typename S>
__device__ __forceinline__ void pose_zero_fill(S* __restrict__ p, long long count, long long i, long long n) {
  const long long head = min(count, (long long)(((16u - (unsigned)((uintptr_t)p & 15u)) & 15u) / sizeof(S)));
  const long long n16 = (count - head) * (long long)sizeof(S) / 16, tail0 = head + n16 * (16 / (long long)sizeof(S));
  int4* z16 = reinterpret_cast<int4*>(p + head);
  for (long long k = i; k < n16; k += n) z16[k] = make_int4(0, 0, 0, 0);
  if (i < head) p[i] = (S)0;
  if (tail0 + i < count) p[tail0 + i] = (S)0;
}

// cos of the geodesic angle between Rp and Rg (9 contiguous scalars each), clipped like torch.clip (a NaN stays a NaN)
template <typename S>
__device__ __forceinline__ S pose_cos(const S* __restrict__ rp, const S* __restrict__ rg) {
  S tr = rp[0] * rg[0];
#pragma unroll
  for (int k = 1; k < 9; ++k) tr += rp[k] * rg[k];
  return mf_clamp((tr - (S)1) / (S)2, (S)-1, (S)1);
}

// one thread per (rollout, ground-truth stamp); two per-block partial sums in a fixed order, the block that takes the last ticket turns
// them into the two means and resets the ticket (physics_loss_value_kernel's finish: deterministic, reusable launch after launch)
template <typename S>
__global__ void __launch_bounds__(256) pose_loss_value_kernel(const S* __restrict__ Xs, long long sb, long long st, const S* __restrict__ Rs,
                                                             long long rsb, long long rst, const S* __restrict__ Xgt,
                                                             const S* __restrict__ Rgt, const S* __restrict__ gt_ts,
                                                             const int* __restrict__ nearest, int B, int T2, S gamma, S* __restrict__ partial,
                                                             unsigned* __restrict__ ticket, S inv_xyz, S inv_rot, S* __restrict__ loss,
                                                             S* __restrict__ zero_x, long long zero_x_count, S* __restrict__ zero_r,
                                                             long long zero_r_count) {
  __shared__ S wave_sum[2][4];
  __shared__ bool last;
  const long long i = (long long)blockIdx.x * blockDim.x + threadIdx.x;        // = b * T2 + j
  const long long nthreads = (long long)gridDim.x * blockDim.x;
  // the buffers the backward will scatter into are cleared here (no fill launches in front of the rollout backward)
  if (zero_x_count > 0) pose_zero_fill(zero_x, zero_x_count, i, nthreads);
  if (zero_r_count > 0) pose_zero_fill(zero_r, zero_r_count, i, nthreads);
  S acc = (S)0, rot = (S)0;
  if (i < (long long)B * T2) {
    const int b = (int)(i / T2);
    const S w = (S)1 / ((S)1 + gamma * gt_ts[i]);
    const int nr = nearest[i];
    const S* x = Xs + b * sb + (long long)nr * st;
    const S* g = Xgt + (size_t)i * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) { const S d = x[c] * w - g[c] * w; acc += d * d; }   // (pred*w - gt*w)^2, as the reference
    const S th = pose_acos(pose_cos(Rs + b * rsb + (long long)nr * rst, Rgt + (size_t)i * 9));
    rot = th * th * w;
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) { acc += __shfl_xor(acc, d, 64); rot += __shfl_xor(rot, d, 64); }
  if ((threadIdx.x & 63) == 0) { wave_sum[0][threadIdx.x >> 6] = acc; wave_sum[1][threadIdx.x >> 6] = rot; }
  __syncthreads();
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = (wave_sum[0][0] + wave_sum[0][1]) + (wave_sum[0][2] + wave_sum[0][3]);
    partial[gridDim.x + blockIdx.x] = (wave_sum[1][0] + wave_sum[1][1]) + (wave_sum[1][2] + wave_sum[1][3]);
    __threadfence();
    last = atomicAdd(ticket, 1u) == gridDim.x - 1;
  }
  __syncthreads();
  if (!last) return;
  __threadfence();
  // 256 threads stride over the partial sums in index order, then the same butterfly
  S tx = (S)0, tr = (S)0;
  for (unsigned k = threadIdx.x; k < gridDim.x; k += 256) {
    tx += __builtin_nontemporal_load(partial + k);
    tr += __builtin_nontemporal_load(partial + gridDim.x + k);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) { tx += __shfl_xor(tx, d, 64); tr += __shfl_xor(tr, d, 64); }
  if ((threadIdx.x & 63) == 0) { wave_sum[0][threadIdx.x >> 6] = tx; wave_sum[1][threadIdx.x >> 6] = tr; }
  __syncthreads();
  if (threadIdx.x == 0) {
    loss[0] = ((wave_sum[0][0] + wave_sum[0][1]) + (wave_sum[0][2] + wave_sum[0][3])) * inv_xyz;
    loss[1] = ((wave_sum[1][0] + wave_sum[1][1]) + (wave_sum[1][2] + wave_sum[1][3])) * inv_rot;
    *ticket = 0u;
  }
}

template <typename S>
__global__ void __launch_bounds__(256) pose_loss_bwd_kernel(const S* __restrict__ Xs, long long sb, long long st, const S* __restrict__ Rs,
                                                           long long rsb, long long rst, const S* __restrict__ Xgt,
                                                           const S* __restrict__ Rgt, const S* __restrict__ gt_ts,
                                                           const int* __restrict__ nearest, int B, int T2, S gamma,
                                                           const S* __restrict__ gloss, S inv_xyz, S inv_rot, S* __restrict__ gXs,
                                                           S* __restrict__ gRs) {
  const long long t = (long long)blockIdx.x * blockDim.x + threadIdx.x;
  if (t >= (long long)B * T2) return;
  // time-major rows (sb < st): neighbouring threads take neighbouring ROLLOUTS of one stamp; batch-major rows: neighbouring stamps of
  // one rollout (physics_loss_bwd_kernel's mapping)
  const bool jm = sb < st;
  const int b = (int)(jm ? t % B : t / T2), j = (int)(jm ? t / B : t % T2);
  const long long i = (long long)b * T2 + j;
  const S w = (S)1 / ((S)1 + gamma * gt_ts[i]);
  const int nr = nearest[i];
  // stamps of a rollout may share a step (then the contributions add up: atomics); a step this stamp has to itself is stored
  bool shared = false;
  for (int k = 0; k < T2; ++k) shared |= (k != j) & (nearest[(long long)b * T2 + k] == nr);
  if (gXs) {
    const S scale = (S)2 * gloss[0] * inv_xyz;
    const long long o = b * sb + (long long)nr * st;
    const S* g = Xgt + (size_t)i * 3;
#pragma unroll
    for (int c = 0; c < 3; ++c) {
      const S v = scale * w * (Xs[o + c] * w - g[c] * w);
      if (shared) pose_atomic_add(gXs + o + c, v); else gXs[o + c] = v;
    }
  }
  if (gRs) {
    const long long o = b * rsb + (long long)nr * rst;
    const S* rg = Rgt + (size_t)i * 9;
    const S c = pose_cos(Rs + o, rg);
    // d theta^2 / d tr = 2 theta * (-1 / sqrt(1 - c^2)) * (1/2); 0 on and outside the clip bounds (and for a NaN)
    S dth2 = (S)0;
    if (c > (S)-1 && c < (S)1) dth2 = -pose_acos(c) / mf_sqrt(((S)1 - c) * ((S)1 + c));
    const S scale = gloss[1] * w * inv_rot * dth2;
#pragma unroll
    for (int k = 0; k < 9; ++k) {
      const S v = scale * rg[k];
      if (shared) pose_atomic_add(gRs + o + k, v); else gRs[o + k] = v;
    }
  }
}

static bool pose_desc_ok(const MfPoseLossDesc* d, const char* what) {
  if (!d) { set_error(std::string(what) + ": null descriptor"); return false; }
  if (!(d->B > 0 && d->T1 > 0 && d->T2 > 0)) { set_error(std::string(what) + ": B, T1, T2 must be positive"); return false; }
  if ((long long)d->B * d->T2 >= (1ll << 31)) { set_error(std::string(what) + ": B * T2 must be below 2^31"); return false; }
  return true;
}

template <typename S>
static int pose_value(const MfPoseLossDesc* d, const S* Xs, const S* Rs, const S* Xgt, const S* Rgt, const S* gt_ts, const int* nearest,
                      S* partial, unsigned* ticket, S* loss, S* zero_x, long long zero_x_count, S* zero_r, long long zero_r_count,
                      hipStream_t st) {
  if (!pose_desc_ok(d, "pose_loss_value")) return MF_ERR_INVALID;
  MF_REQUIRE(Xs && Rs && Xgt && Rgt && gt_ts && nearest && partial && ticket && loss, MF_ERR_INVALID, "pose_loss_value: null argument");
  MF_REQUIRE(zero_x_count >= 0 && (zero_x || zero_x_count == 0), MF_ERR_INVALID, "pose_loss_value: zero_x_count without zero_x");
  MF_REQUIRE(zero_r_count >= 0 && (zero_r || zero_r_count == 0), MF_ERR_INVALID, "pose_loss_value: zero_r_count without zero_r");
  const long long n = (long long)d->B * d->T2;
  hipLaunchKernelGGL((pose_loss_value_kernel<S>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, Xs, (long long)d->x_stride_b,
                     (long long)d->x_stride_t, Rs, (long long)d->r_stride_b, (long long)d->r_stride_t, Xgt, Rgt, gt_ts, nearest, d->B, d->T2,
                     (S)d->gamma, partial, ticket, (S)(1.0 / (3.0 * (double)n)), (S)(1.0 / (double)n), loss, zero_x, zero_x_count, zero_r,
                     zero_r_count);
  hipError_t e = hipGetLastError();
  MF_REQUIRE(e == hipSuccess, MF_ERR_LAUNCH, std::string("pose_loss_value launch: ") + hipGetErrorString(e));
  return MF_OK;
}

template <typename S>
static int pose_bwd(const MfPoseLossDesc* d, const S* Xs, const S* Rs, const S* Xgt, const S* Rgt, const S* gt_ts, const int* nearest,
                    const S* gloss, S* gXs, S* gRs, hipStream_t st) {
  if (!pose_desc_ok(d, "pose_loss_bwd")) return MF_ERR_INVALID;
  MF_REQUIRE(Xs && Rs && Xgt && Rgt && gt_ts && nearest && gloss, MF_ERR_INVALID, "pose_loss_bwd: null argument");
  MF_REQUIRE(gXs || gRs, MF_ERR_INVALID, "pose_loss_bwd: neither gXs nor gRs given");
  const long long n = (long long)d->B * d->T2;
  hipLaunchKernelGGL((pose_loss_bwd_kernel<S>), dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, Xs, (long long)d->x_stride_b,
                     (long long)d->x_stride_t, Rs, (long long)d->r_stride_b, (long long)d->r_stride_t, Xgt, Rgt, gt_ts, nearest, d->B, d->T2,
                     (S)d->gamma, gloss, (S)(1.0 / (3.0 * (double)n)), (S)(1.0 / (double)n), gXs, gRs);
  hipError_t e = hipGetLastError();
  MF_REQUIRE(e == hipSuccess, MF_ERR_LAUNCH, std::string("pose_loss_bwd launch: ") + hipGetErrorString(e));
  return MF_OK;
}

}  // namespace mf

extern "C" int mf_pose_loss_value_f32(const MfPoseLossDesc* d, const float* Xs, const float* Rs, const float* Xgt, const float* Rgt,
                                      const float* gt_ts, const int32_t* nearest, float* partial, uint32_t* ticket, float* loss,
                                      float* zero_x, long long zero_x_count, float* zero_r, long long zero_r_count, void* s) {
  return mf::pose_value<float>(d, Xs, Rs, Xgt, Rgt, gt_ts, nearest, partial, ticket, loss, zero_x, zero_x_count, zero_r, zero_r_count, (hipStream_t)s);
}
extern "C" int mf_pose_loss_value_f64(const MfPoseLossDesc* d, const double* Xs, const double* Rs, const double* Xgt, const double* Rgt,
                                      const double* gt_ts, const int32_t* nearest, double* partial, uint32_t* ticket, double* loss,
                                      double* zero_x, long long zero_x_count, double* zero_r, long long zero_r_count, void* s) {
  return mf::pose_value<double>(d, Xs, Rs, Xgt, Rgt, gt_ts, nearest, partial, ticket, loss, zero_x, zero_x_count, zero_r, zero_r_count, (hipStream_t)s);
}
extern "C" int mf_pose_loss_bwd_f32(const MfPoseLossDesc* d, const float* Xs, const float* Rs, const float* Xgt, const float* Rgt,
                                    const float* gt_ts, const int32_t* nearest, const float* gloss, float* gXs, float* gRs, void* s) {
  return mf::pose_bwd<float>(d, Xs, Rs, Xgt, Rgt, gt_ts, nearest, gloss, gXs, gRs, (hipStream_t)s);
}
extern "C" int mf_pose_loss_bwd_f64(const MfPoseLossDesc* d, const double* Xs, const double* Rs, const double* Xgt, const double* Rgt,
                                    const double* gt_ts, const int32_t* nearest, const double* gloss, double* gXs, double* gRs, void* s) {
  return mf::pose_bwd<double>(d, Xs, Rs, Xgt, Rgt, gt_ts, nearest, gloss, gXs, gRs, (hipStream_t)s);
}
