// The two losses of the reference's monoforce/losses.py that sit on a terrain map: hm_loss (:77-99, the weighted MSE over the cells where
// prediction and label are both numbers -- twice per encoder train step, scripts/train.py:388-398, twice per evaluation batch, eval.py:146-147)
// and total_variation (:68-74, the regulariser of scripts/fit_terrain.py:58).  Each as one value launch (finished inside the launch: per-block
// partial sums in a fixed order and a ticket, pose_loss.hip's finish) and one backward launch that STORES every cell of the gradient (a gather
// per cell: no atomics, nothing to clear first).  The ATen forms are ~12 launches and as many full-map temporaries forward, as many backward.
// Maps are [M][H][W], every tensor with its own (stride_m, stride_h) in elements and unit stride along W: channel views of a [B,2,H,W] label
// tensor, row-strided crops and plain [H,W] maps are read in place.  A cell's linear index i = (m*H + h)*W + w (below 2^31) picks the thread.
//   hm_loss:  p' = use_h_max ? h_max * tanh(p) : p;  valid = !isnan(p') && !isnan(gt);  loss = sum_valid (p'*w - gt*w)^2 / n_valid
//             g_pred = valid ? gloss * 2 w (p'*w - gt*w) / n_valid [* h_max (1 - tanh(p)^2)] : 0
//   tv:       loss = (sum |z[h][w+1] - z[h][w]| + sum |z[h+1][w] - z[h][w]|) / (H W),  differences inside each of the M maps
//             g_z[h][w] = gloss / (H W) * (sgn(z - z[w-1]) - sgn(z[w+1] - z) + sgn(z - z[h-1]) - sgn(z[h+1] - z)),  sgn(0) = sgn(NaN) = 0
// ONE difference from autograd (hm_loss with use_h_max and a NaN prediction): torch's tanh backward gives 0 * (1 - NaN^2) = NaN at that
// cell; here the masked cell's gradient is 0 like every other masked cell's.
// IEEE tanh / division (this TU is built without -ffast-math and with -ffp-contract=off, like pose_loss.hip).
#include "mf_common.h"

namespace mf {

constexpr int kMapBlock = 256;     // threads of a workgroup
constexpr int kMapCells = 4;       // cells per thread, kMapBlock apart (coalesced rows of loads, four in flight per lane)
constexpr int kMapChunk = kMapBlock * kMapCells;

__device__ __forceinline__ float map_tanh(float v) { return tanhf(v); }
__device__ __forceinline__ double map_tanh(double v) { return tanh(v); }

// element offsets of cell i = (m*H + h)*W + w in a tensor with strides (sm, sh, 1)
struct MapCell {
  unsigned m, h, w;
  __device__ __forceinline__ MapCell(unsigned i, unsigned H, unsigned W) {
    const unsigned r = i / W;
    w = i - r * W;
    m = r / H;
    h = r - m * H;
  }
  __device__ __forceinline__ long long at(long long sm, long long sh) const { return (long long)m * sm + (long long)h * sh + (long long)w; }
};

// The finish of a value kernel: this block's sum (and count) to partial[blockIdx] / counts[blockIdx]; the block that takes the last
// ticket adds the partials in index order, hands the totals to `finish` (thread 0) and resets the ticket (pose_loss_value_kernel's
// finish: deterministic, reusable launch after launch).  `counts` may be NULL (no count).  All 256 threads must call.
template <typename S, typename Finish>
__device__ __forceinline__ void map_block_finish(S acc, unsigned cnt, S* __restrict__ partial, unsigned* __restrict__ counts,
                                                 unsigned* __restrict__ ticket, Finish finish) {
  __shared__ S wave_sum[4];
  __shared__ unsigned wave_cnt[4];
  __shared__ bool last;
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) { acc += __shfl_xor(acc, d, 64); cnt += (unsigned)__shfl_xor((int)cnt, d, 64); }
  if ((threadIdx.x & 63) == 0) { wave_sum[threadIdx.x >> 6] = acc; wave_cnt[threadIdx.x >> 6] = cnt; }
  __syncthreads();
  if (threadIdx.x == 0) {
    partial[blockIdx.x] = (wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3]);
    if (counts) counts[blockIdx.x] = (wave_cnt[0] + wave_cnt[1]) + (wave_cnt[2] + wave_cnt[3]);
    __threadfence();
    last = atomicAdd(ticket, 1u) == gridDim.x - 1;
  }
  __syncthreads();
  if (!last) return;
  __threadfence();
  S ts = (S)0;
  unsigned tc = 0u;
  for (unsigned k = threadIdx.x; k < gridDim.x; k += kMapBlock) {
    ts += __builtin_nontemporal_load(partial + k);
    if (counts) tc += __builtin_nontemporal_load(counts + k);
  }
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) { ts += __shfl_xor(ts, d, 64); tc += (unsigned)__shfl_xor((int)tc, d, 64); }
  __syncthreads();      // (every wave has read the first round's wave sums)
  if ((threadIdx.x & 63) == 0) { wave_sum[threadIdx.x >> 6] = ts; wave_cnt[threadIdx.x >> 6] = tc; }
  __syncthreads();
  if (threadIdx.x == 0) {
    finish((wave_sum[0] + wave_sum[1]) + (wave_sum[2] + wave_sum[3]), (wave_cnt[0] + wave_cnt[1]) + (wave_cnt[2] + wave_cnt[3]));
    *ticket = 0u;
  }
}

template <typename S>
__global__ void __launch_bounds__(kMapBlock) hm_loss_value_kernel(const S* __restrict__ pred, long long psm, long long psh,
                                                                  const S* __restrict__ gt, long long gsm, long long gsh,
                                                                  const S* __restrict__ wt, long long wsm, long long wsh, unsigned n,
                                                                  unsigned H, unsigned W, bool use_h_max, S h_max, S* __restrict__ partial,
                                                                  unsigned* __restrict__ counts, unsigned* __restrict__ ticket,
                                                                  S* __restrict__ loss, int* __restrict__ n_valid_out) {
  S acc = (S)0;
  unsigned cnt = 0u;
  const unsigned base = blockIdx.x * (unsigned)kMapChunk + threadIdx.x;      // (n < 2^31 and the grid covers n: no overflow)
#pragma unroll
  for (int k = 0; k < kMapCells; ++k) {
    const unsigned i = base + (unsigned)k * kMapBlock;
    if (i < n) {
      const MapCell c(i, H, W);
      S p = pred[c.at(psm, psh)];
      const S g = gt[c.at(gsm, gsh)];
      const S w = wt ? wt[c.at(wsm, wsh)] : (S)1;
      if (use_h_max) p = h_max * map_tanh(p);
      if (!(p != p) && !(g != g)) {
        const S d = p * w - g * w;       // (pred*w - gt*w)^2, as the reference
        acc += d * d;
        ++cnt;
      }
    }
  }
  map_block_finish(acc, cnt, partial, counts, ticket, [&](S total, unsigned n_valid) {
    loss[0] = total / (S)n_valid;        // no valid cell: 0 / 0 = NaN, the reference's mean of an empty selection
    n_valid_out[0] = (int)n_valid;
  });
}

template <typename S>
__global__ void __launch_bounds__(kMapBlock) hm_loss_bwd_kernel(const S* __restrict__ pred, long long psm, long long psh,
                                                                const S* __restrict__ gt, long long gsm, long long gsh,
                                                                const S* __restrict__ wt, long long wsm, long long wsh, unsigned n, unsigned H,
                                                                unsigned W, bool use_h_max, S h_max, const int* __restrict__ n_valid,
                                                                const S* __restrict__ gloss, S* __restrict__ g_pred, long long osm,
                                                                long long osh) {
  const S up = gloss[0], count = (S)n_valid[0];
  const unsigned base = blockIdx.x * (unsigned)kMapChunk + threadIdx.x;
#pragma unroll
  for (int k = 0; k < kMapCells; ++k) {
    const unsigned i = base + (unsigned)k * kMapBlock;
    if (i < n) {
      const MapCell c(i, H, W);
      const S p0 = pred[c.at(psm, psh)];
      const S g = gt[c.at(gsm, gsh)];
      const S w = wt ? wt[c.at(wsm, wsh)] : (S)1;
      const S t = use_h_max ? map_tanh(p0) : (S)0;
      const S p = use_h_max ? h_max * t : p0;
      S v = (S)0;
      if (!(p != p) && !(g != g)) {
        // autograd's order: the mean's 1 / n_valid, the square's 2 d, the weight, then h_max and tanh's (1 - t^2)
        v = up / count * ((S)2 * (p * w - g * w)) * w;
        if (use_h_max) v = v * h_max * ((S)1 - t * t);
      }
      g_pred[c.at(osm, osh)] = v;
    }
  }
}

template <typename S>
__device__ __forceinline__ S map_abs(S v) { return v < (S)0 ? -v : v; }      // (a NaN stays a NaN)
template <typename S>
__device__ __forceinline__ int map_sgn(S v) { return (int)(v > (S)0) - (int)(v < (S)0); }      // torch's sgn: 0 at 0 and for a NaN

template <typename S>
__global__ void __launch_bounds__(kMapBlock) total_variation_value_kernel(const S* __restrict__ z, long long zsm, long long zsh, unsigned n,
                                                                          unsigned H, unsigned W, S cells, S* __restrict__ partial,
                                                                          unsigned* __restrict__ ticket, S* __restrict__ loss) {
  S acc = (S)0;
  const unsigned base = blockIdx.x * (unsigned)kMapChunk + threadIdx.x;
#pragma unroll
  for (int k = 0; k < kMapCells; ++k) {
    const unsigned i = base + (unsigned)k * kMapBlock;
    if (i < n) {
      const MapCell c(i, H, W);
      const S* p = z + c.at(zsm, zsh);
      const S v = p[0];
      // each cell owns the difference to its right and the one below it; both stay inside the cell's own map
      if (c.w + 1 < W) acc += map_abs(p[1] - v);
      if (c.h + 1 < H) acc += map_abs(p[zsh] - v);
    }
  }
  map_block_finish(acc, 0u, partial, (unsigned*)nullptr, ticket, [&](S total, unsigned) { loss[0] = total / cells; });
}

template <typename S>
__global__ void __launch_bounds__(kMapBlock) total_variation_bwd_kernel(const S* __restrict__ z, long long zsm, long long zsh, unsigned n,
                                                                        unsigned H, unsigned W, S cells, const S* __restrict__ gloss,
                                                                        S* __restrict__ g_z, long long osm, long long osh) {
  const S scale = gloss[0] / cells;
  const unsigned base = blockIdx.x * (unsigned)kMapChunk + threadIdx.x;
#pragma unroll
  for (int k = 0; k < kMapCells; ++k) {
    const unsigned i = base + (unsigned)k * kMapBlock;
    if (i < n) {
      const MapCell c(i, H, W);
      const S* p = z + c.at(zsm, zsh);
      const S v = p[0];
      int s = 0;
      if (c.w > 0) s += map_sgn(v - p[-1]);
      if (c.w + 1 < W) s -= map_sgn(p[1] - v);
      if (c.h > 0) s += map_sgn(v - p[-zsh]);
      if (c.h + 1 < H) s -= map_sgn(p[zsh] - v);
      g_z[c.at(osm, osh)] = (S)s * scale;
    }
  }
}

static bool map_desc_ok(const MfMapLossDesc* d, const char* what) {
  if (!d) { set_error(std::string(what) + ": null descriptor"); return false; }
  if (!(d->M > 0 && d->H > 0 && d->W > 0)) { set_error(std::string(what) + ": M, H, W must be positive"); return false; }
  if ((long long)d->M * d->H * d->W >= (1ll << 31)) { set_error(std::string(what) + ": M * H * W must be below 2^31"); return false; }
  return true;
}

static unsigned map_blocks(const MfMapLossDesc* d) { return (unsigned)(((long long)d->M * d->H * d->W + kMapChunk - 1) / kMapChunk); }

#define MF_MAP_LAUNCHED(what)                                                                              \
  do {                                                                                                     \
    hipError_t e_ = hipGetLastError();                                                                     \
    MF_REQUIRE(e_ == hipSuccess, MF_ERR_LAUNCH, std::string(what " launch: ") + hipGetErrorString(e_));   \
    return MF_OK;                                                                                          \
  } while (0)

template <typename S>
static int hm_value(const MfMapLossDesc* d, const S* pred, const S* gt, const S* w, S* partial, unsigned* counts, unsigned* ticket, S* loss,
                    int* n_valid, hipStream_t st) {
  if (!map_desc_ok(d, "hm_loss_value")) return MF_ERR_INVALID;
  MF_REQUIRE(pred && gt && partial && counts && ticket && loss && n_valid, MF_ERR_INVALID, "hm_loss_value: null argument");
  hipLaunchKernelGGL((hm_loss_value_kernel<S>), dim3(map_blocks(d)), dim3(kMapBlock), 0, st, pred, (long long)d->p_stride_m,
                     (long long)d->p_stride_h, gt, (long long)d->g_stride_m, (long long)d->g_stride_h, w, (long long)d->w_stride_m,
                     (long long)d->w_stride_h, (unsigned)(d->M * d->H * d->W), (unsigned)d->H, (unsigned)d->W, d->use_h_max != 0, (S)d->h_max,
                     partial, counts, ticket, loss, n_valid);
  MF_MAP_LAUNCHED("hm_loss_value");
}

template <typename S>
static int hm_bwd(const MfMapLossDesc* d, const S* pred, const S* gt, const S* w, const int* n_valid, const S* gloss, S* g_pred, hipStream_t st) {
  if (!map_desc_ok(d, "hm_loss_bwd")) return MF_ERR_INVALID;
  MF_REQUIRE(pred && gt && n_valid && gloss && g_pred, MF_ERR_INVALID, "hm_loss_bwd: null argument");
  hipLaunchKernelGGL((hm_loss_bwd_kernel<S>), dim3(map_blocks(d)), dim3(kMapBlock), 0, st, pred, (long long)d->p_stride_m,
                     (long long)d->p_stride_h, gt, (long long)d->g_stride_m, (long long)d->g_stride_h, w, (long long)d->w_stride_m,
                     (long long)d->w_stride_h, (unsigned)(d->M * d->H * d->W), (unsigned)d->H, (unsigned)d->W, d->use_h_max != 0, (S)d->h_max,
                     n_valid, gloss, g_pred, (long long)d->o_stride_m, (long long)d->o_stride_h);
  MF_MAP_LAUNCHED("hm_loss_bwd");
}

template <typename S>
static int tv_value(const MfMapLossDesc* d, const S* z, S* partial, unsigned* ticket, S* loss, hipStream_t st) {
  if (!map_desc_ok(d, "total_variation_value")) return MF_ERR_INVALID;
  MF_REQUIRE(z && partial && ticket && loss, MF_ERR_INVALID, "total_variation_value: null argument");
  hipLaunchKernelGGL((total_variation_value_kernel<S>), dim3(map_blocks(d)), dim3(kMapBlock), 0, st, z, (long long)d->p_stride_m,
                     (long long)d->p_stride_h, (unsigned)(d->M * d->H * d->W), (unsigned)d->H, (unsigned)d->W, (S)((long long)d->H * d->W),
                     partial, ticket, loss);
  MF_MAP_LAUNCHED("total_variation_value");
}

template <typename S>
static int tv_bwd(const MfMapLossDesc* d, const S* z, const S* gloss, S* g_z, hipStream_t st) {
  if (!map_desc_ok(d, "total_variation_bwd")) return MF_ERR_INVALID;
  MF_REQUIRE(z && gloss && g_z, MF_ERR_INVALID, "total_variation_bwd: null argument");
  hipLaunchKernelGGL((total_variation_bwd_kernel<S>), dim3(map_blocks(d)), dim3(kMapBlock), 0, st, z, (long long)d->p_stride_m,
                     (long long)d->p_stride_h, (unsigned)(d->M * d->H * d->W), (unsigned)d->H, (unsigned)d->W, (S)((long long)d->H * d->W),
                     gloss, g_z, (long long)d->o_stride_m, (long long)d->o_stride_h);
  MF_MAP_LAUNCHED("total_variation_bwd");
}

}  // namespace mf

extern "C" int mf_hm_loss_value_f32(const MfMapLossDesc* d, const float* pred, const float* gt, const float* w, float* partial, uint32_t* counts,
                                    uint32_t* ticket, float* loss, int32_t* n_valid_out, void* s) {
  return mf::hm_value<float>(d, pred, gt, w, partial, counts, ticket, loss, n_valid_out, (hipStream_t)s);
}
extern "C" int mf_hm_loss_value_f64(const MfMapLossDesc* d, const double* pred, const double* gt, const double* w, double* partial,
                                    uint32_t* counts, uint32_t* ticket, double* loss, int32_t* n_valid_out, void* s) {
  return mf::hm_value<double>(d, pred, gt, w, partial, counts, ticket, loss, n_valid_out, (hipStream_t)s);
}
extern "C" int mf_hm_loss_bwd_f32(const MfMapLossDesc* d, const float* pred, const float* gt, const float* w, const int32_t* n_valid,
                                  const float* gloss, float* g_pred, void* s) {
  return mf::hm_bwd<float>(d, pred, gt, w, n_valid, gloss, g_pred, (hipStream_t)s);
}
extern "C" int mf_hm_loss_bwd_f64(const MfMapLossDesc* d, const double* pred, const double* gt, const double* w, const int32_t* n_valid,
                                  const double* gloss, double* g_pred, void* s) {
  return mf::hm_bwd<double>(d, pred, gt, w, n_valid, gloss, g_pred, (hipStream_t)s);
}
extern "C" int mf_total_variation_value_f32(const MfMapLossDesc* d, const float* z, float* partial, uint32_t* ticket, float* loss, void* s) {
  return mf::tv_value<float>(d, z, partial, ticket, loss, (hipStream_t)s);
}
extern "C" int mf_total_variation_value_f64(const MfMapLossDesc* d, const double* z, double* partial, uint32_t* ticket, double* loss, void* s) {
  return mf::tv_value<double>(d, z, partial, ticket, loss, (hipStream_t)s);
}
extern "C" int mf_total_variation_bwd_f32(const MfMapLossDesc* d, const float* z, const float* gloss, float* g_z, void* s) {
  return mf::tv_bwd<float>(d, z, gloss, g_z, (hipStream_t)s);
}
extern "C" int mf_total_variation_bwd_f64(const MfMapLossDesc* d, const double* z, const double* gloss, double* g_z, void* s) {
  return mf::tv_bwd<double>(d, z, gloss, g_z, (hipStream_t)s);
}
