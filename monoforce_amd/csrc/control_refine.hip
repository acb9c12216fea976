// Gradient descent on K control sequences [K,T,2] as ONE launch per iteration: torch.optim.Adam on the controls with a rate per channel
// (v, w), the box of the control limits behind it, and per-sequence best-so-far bookkeeping -- with the iteration count, each sequence's
// smallest cost, its iteration and the cost history kept on the device, so that the host neither reads a cost back nor decides anything and
// the launch can follow the rollout's and the objective's launches inside one hipGraph (terrain_fit.hip's pattern, per sequence).
//   t = step + 1;  m = lerp(m, g, 1 - b1);  v = b2 v + ((1 - b2) g) g;  p = p + (-(lr / (1 - b1^t)) m) / (sqrt(v) / sqrt(1 - b2^t) + eps)
// is ATen's single-tensor Adam operation by operation (this TU is built with -ffp-contract=off: each rounds on its own).
// One workgroup of 256 threads per sequence, its 2 T elements in trips of 256.  Order within iteration i (include/monoforce_hip.h at
// MfRefineDesc): history[i][k]; on a strict improvement the snapshot of the controls BEFORE the update -- the controls the cost belongs to
// (terrain_fit.hip snapshots AFTER it, a quirk of the reference's loop that has no counterpart here); a NaN cost or a non-finite entry
// anywhere in the sequence's gradient row leaves controls and moments untouched (one pass over the row, one workgroup-wide OR, ahead of any
// store); else Adam and the clamp.  A sequence's scalars (cost, best cost, best iteration, its history column) are read and written by its
// own workgroup alone; the shared step count is read by every workgroup first and committed by the one that draws the last ticket
// (terrain_fit.hip's finish), so no workgroup can meet the next iteration's count.
#include "mf_common.h"

#include <math.h>

namespace mf {

constexpr int kRefineBlock = 256;     // threads of a workgroup, one element each per trip

struct RefineArgs {
  float* p;
  const float* g;
  const float* costs;
  float* m;
  float* v;
  float* best;
  float* best_cost;
  int* best_iter;
  float* history;
  int* state;                 // step, ticket
  int K, n, max_iters;        // sequences, elements of a sequence (2 T)
  double lr[2], beta1, beta2;
  float w1, b2, w2, eps;      // 1 - beta1, beta2, 1 - beta2 and eps as the tensor operations take a Python scalar: rounded to float once
  float lo[2], hi[2];
};

__global__ void __launch_bounds__(kRefineBlock) control_refine_update_kernel(const RefineArgs a) {
  const int k = blockIdx.x;
  // the iteration's scalars, before anything of this launch can have replaced them
  const int step = a.state[0];
  const float cost = a.costs[k];
  const bool improved = cost < a.best_cost[k];      // strict; false for a NaN and for +inf
  const long long base = (long long)k * a.n;
  const float* g = a.g + base;
  int bad = 0;
  for (int i = threadIdx.x; i < a.n; i += kRefineBlock) bad |= !(fabsf(g[i]) < INFINITY);      // NaN or +-inf
  // (a barrier too: every thread has read best_cost[k] before thread 0 replaces it below)
  const bool skip = __syncthreads_or(bad) != 0 || cost != cost;

  const double t = (double)step + 1.0;
  const double bc1 = 1.0 - pow(a.beta1, t), bc2 = 1.0 - pow(a.beta2, t);
  const float bc2_sqrt = (float)sqrt(bc2);
  const float neg_v = (float)(-(a.lr[0] / bc1)), neg_w = (float)(-(a.lr[1] / bc1));
  const bool small_w = a.w1 < 0.5f;                 // lerp's two forms (ATen: by the size of the weight)
  for (int i = threadIdx.x; i < a.n; i += kRefineBlock) {
    float p = a.p[base + i];
    if (improved) a.best[base + i] = p;             // the controls this cost was computed from
    if (skip) continue;
    const int ch = i & 1;
    const float gi = g[i];
    float m = a.m[base + i], v = a.v[base + i];
    const float d = gi - m;
    m = small_w ? m + a.w1 * d : gi - d * (1.0f - a.w1);
    v = a.b2 * v;
    v = v + (a.w2 * gi) * gi;
    const float denom = sqrtf(v) / bc2_sqrt + a.eps;
    p = p + ((ch ? neg_w : neg_v) * m) / denom;
    p = mf_clamp(p, ch ? a.lo[1] : a.lo[0], ch ? a.hi[1] : a.hi[0]);
    a.p[base + i] = p;
    a.m[base + i] = m;
    a.v[base + i] = v;
  }
  if (threadIdx.x == 0) {
    if (step < a.max_iters) a.history[(long long)step * a.K + k] = cost;
    if (improved) {
      a.best_cost[k] = cost;
      a.best_iter[k] = step;
    }
  }
  __syncthreads();      // every thread of the workgroup has read the step
  if (threadIdx.x == 0) {
    unsigned* const ticket = reinterpret_cast<unsigned*>(a.state + 1);
    __threadfence();
    if (atomicAdd(ticket, 1u) == gridDim.x - 1) {      // every other workgroup has taken its ticket: none reads the step any more
      a.state[0] = step + 1;
      *ticket = 0u;
    }
  }
}

}  // namespace mf

extern "C" int mf_control_refine_update_f32(const MfRefineDesc* d, float* controls, const float* grad, const float* costs, float* m, float* v,
                                            float* best_controls, float* best_cost, int32_t* best_iter, float* history, int32_t* state, void* stream) {
  MF_REQUIRE(d, MF_ERR_INVALID, "control_refine_update: null descriptor");
  MF_REQUIRE(d->K > 0 && d->T > 0, MF_ERR_INVALID, "control_refine_update: K and T must be positive");
  MF_REQUIRE(d->max_iters >= 0, MF_ERR_INVALID, "control_refine_update: max_iters must not be negative");
  MF_REQUIRE(d->beta1 >= 0.0 && d->beta1 < 1.0 && d->beta2 >= 0.0 && d->beta2 < 1.0, MF_ERR_INVALID,
             "control_refine_update: beta1, beta2 must be in [0, 1)");
  MF_REQUIRE(d->eps > 0.0, MF_ERR_INVALID, "control_refine_update: eps must be positive");
  MF_REQUIRE(d->lr[0] >= 0.0 && d->lr[1] >= 0.0, MF_ERR_INVALID, "control_refine_update: lr must not be negative");
  MF_REQUIRE(d->lo[0] <= d->hi[0] && d->lo[1] <= d->hi[1], MF_ERR_INVALID, "control_refine_update: bounds need lo <= hi");
  const long long lim = 1ll << 31;
  MF_REQUIRE(2ll * d->K * d->T < lim && (long long)d->max_iters * d->K < lim, MF_ERR_UNSUPPORTED,
             "control_refine_update: 2 K T and max_iters K must stay below 2^31");
  MF_REQUIRE(controls && grad && costs && m && v && best_controls && best_cost && best_iter && state && (history || d->max_iters == 0),
             MF_ERR_INVALID, "control_refine_update: null argument");
  mf::RefineArgs a;
  a.p = controls; a.g = grad; a.costs = costs; a.m = m; a.v = v; a.best = best_controls; a.best_cost = best_cost; a.best_iter = best_iter;
  a.history = history; a.state = state;
  a.K = d->K; a.n = 2 * d->T; a.max_iters = d->max_iters;
  a.lr[0] = d->lr[0]; a.lr[1] = d->lr[1]; a.beta1 = d->beta1; a.beta2 = d->beta2;
  a.w1 = (float)(1.0 - d->beta1); a.b2 = (float)d->beta2; a.w2 = (float)(1.0 - d->beta2); a.eps = (float)d->eps;
  a.lo[0] = d->lo[0]; a.lo[1] = d->lo[1]; a.hi[0] = d->hi[0]; a.hi[1] = d->hi[1];
  hipLaunchKernelGGL(mf::control_refine_update_kernel, dim3(d->K), dim3(mf::kRefineBlock), 0, (hipStream_t)stream, a);
  hipError_t e = hipGetLastError();
  MF_REQUIRE(e == hipSuccess, MF_ERR_LAUNCH, std::string("control_refine_update launch: ") + hipGetErrorString(e));
  return MF_OK;
}
