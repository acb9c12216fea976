// The loop of the reference's scripts/fit_terrain.py:46-69 around one fit step, as ONE launch per iteration: torch.optim.Adam on the
// height and the friction map (two parameter groups, :46-49, :62) and the best-so-far bookkeeping (:61-69: `if loss < loss_min`, clone the
// map) -- with the iteration count, the smallest loss, its iteration and the loss history kept on the device, so that the host neither
// reads the loss back nor decides anything and the launch can follow the step's launches inside one hipGraph.
//   t = step + 1;  m = lerp(m, g, 1 - b1);  v = b2 v + ((1 - b2) g) g;  p = p + (-(lr / (1 - b1^t)) m) / (sqrt(v) / sqrt(1 - b2^t) + eps)
// is ATen's single-tensor Adam operation by operation (this TU is built with -ffp-contract=off: each rounds on its own); the box
// projection behind it is an extension and off by default.  The loss of iteration i belongs to the parameters BEFORE update i, the
// snapshot taken on an improvement holds the parameters AFTER it -- the reference clones behind optimizer.step().
// The scalars are read by every workgroup and written by one: each workgroup reads them first, updates its cells, fences and takes a
// ticket; the workgroup that draws the last ticket stores step + 1, loss_min, best_step and history[step] and resets the ticket
// (map_losses.hip's / pose_loss.hip's finish).  No workgroup can therefore meet the next iteration's scalars, and z_best is never a mixture.
#include "mf_common.h"

namespace mf {

constexpr int kFitBlock = 256;        // threads of a workgroup, one cell each per trip
constexpr int kFitMaxBlocks = 512;    // workgroups of a launch at most (two per CU): 2 x 256^2 cells are one trip of the loop

template <typename S>
struct FitMap {
  S* p;
  const S* g;
  S* m;
  S* v;
  S* best;
  double lr;
  S lo, hi;
  bool clamp;
};

template <typename S>
struct FitArgs {
  FitMap<S> z, mu;
  long long n_z, n;          // height cells, all cells
  double beta1, beta2;
  S w1, b2, w2, eps;         // 1 - beta1, beta2, 1 - beta2 and eps as the tensor operations take a Python scalar: rounded to S once
  const S* loss;
  S* loss_min;
  S* history;
  int* state;                // step, best_step, ticket, reserved
  int max_iters;
};

template <typename S>
__global__ void __launch_bounds__(kFitBlock) terrain_fit_update_kernel(const FitArgs<S> a) {
  // the iteration's scalars, before anything of this launch can have replaced them
  const int step = a.state[0];
  const S loss = a.loss[0];
  const bool improved = loss < a.loss_min[0];      // strict; false for a NaN
  const double t = (double)step + 1.0;
  const double bc1 = 1.0 - pow(a.beta1, t), bc2 = 1.0 - pow(a.beta2, t);
  const S bc2_sqrt = (S)sqrt(bc2);
  const S neg_z = (S)(-(a.z.lr / bc1)), neg_mu = (S)(-(a.mu.lr / bc1));
  const bool small_w = a.w1 < (S)0.5;              // lerp's two forms (ATen: by the size of the weight)

  const long long stride = (long long)gridDim.x * kFitBlock;
  for (long long i = (long long)blockIdx.x * kFitBlock + threadIdx.x; i < a.n; i += stride) {
    const bool is_mu = i >= a.n_z;
    const long long j = is_mu ? i - a.n_z : i;
    S* const pp = (is_mu ? a.mu.p : a.z.p) + j;
    S* const mp = (is_mu ? a.mu.m : a.z.m) + j;
    S* const vp = (is_mu ? a.mu.v : a.z.v) + j;
    const S g = (is_mu ? a.mu.g : a.z.g)[j];
    S p = *pp, m = *mp, v = *vp;
    const S d = g - m;
    m = small_w ? m + a.w1 * d : g - d * ((S)1 - a.w1);
    v = a.b2 * v;
    v = v + (a.w2 * g) * g;
    const S denom = mf_sqrt(v) / bc2_sqrt + a.eps;
    p = p + ((is_mu ? neg_mu : neg_z) * m) / denom;
    if (is_mu ? a.mu.clamp : a.z.clamp) p = mf_clamp(p, is_mu ? a.mu.lo : a.z.lo, is_mu ? a.mu.hi : a.z.hi);
    *pp = p;
    *mp = m;
    *vp = v;
    if (improved) (is_mu ? a.mu.best : a.z.best)[j] = p;
  }

  __syncthreads();      // every thread of the workgroup has read the scalars and stored its cells
  if (threadIdx.x == 0) {
    unsigned* const ticket = reinterpret_cast<unsigned*>(a.state + 2);
    __threadfence();
    if (atomicAdd(ticket, 1u) == gridDim.x - 1) {      // every other workgroup has taken its ticket: none reads the scalars any more
      if (step < a.max_iters) a.history[step] = loss;
      if (improved) {
        a.loss_min[0] = loss;
        a.state[1] = step;
      }
      a.state[0] = step + 1;
      *ticket = 0u;
    }
  }
}

template <typename S>
static int fit_update(const MfFitDesc* d, S* z, S* mu, const S* g_z, const S* g_mu, S* m_z, S* v_z, S* m_mu, S* v_mu, const S* loss, S* z_best,
                      S* mu_best, int* state, S* loss_min, S* history, hipStream_t st) {
  MF_REQUIRE(d, MF_ERR_INVALID, "terrain_fit_update: null descriptor");
  MF_REQUIRE(d->n_z > 0, MF_ERR_INVALID, "terrain_fit_update: n_z must be positive");
  MF_REQUIRE(d->n_mu >= 0, MF_ERR_INVALID, "terrain_fit_update: n_mu must not be negative");
  MF_REQUIRE(d->max_iters >= 0, MF_ERR_INVALID, "terrain_fit_update: max_iters must not be negative");
  MF_REQUIRE(d->beta1 >= 0.0 && d->beta1 < 1.0 && d->beta2 >= 0.0 && d->beta2 < 1.0, MF_ERR_INVALID,
             "terrain_fit_update: beta1, beta2 must be in [0, 1)");
  MF_REQUIRE(d->eps > 0.0, MF_ERR_INVALID, "terrain_fit_update: eps must be positive");
  MF_REQUIRE(d->lr_z >= 0.0 && d->lr_mu >= 0.0, MF_ERR_INVALID, "terrain_fit_update: lr must not be negative");
  const bool clamp_z = (d->flags & MF_FIT_CLAMP_Z) != 0, clamp_mu = (d->flags & MF_FIT_CLAMP_MU) != 0;
  MF_REQUIRE((!clamp_z || d->z_lo <= d->z_hi) && (!clamp_mu || d->mu_lo <= d->mu_hi), MF_ERR_INVALID,
             "terrain_fit_update: bounds need lo <= hi");
  MF_REQUIRE(z && g_z && m_z && v_z && z_best && loss && state && loss_min && (history || d->max_iters == 0), MF_ERR_INVALID,
             "terrain_fit_update: null argument");
  MF_REQUIRE(d->n_mu == 0 || (mu && g_mu && m_mu && v_mu && mu_best), MF_ERR_INVALID, "terrain_fit_update: null friction argument");
  FitArgs<S> a;
  a.z = FitMap<S>{z, g_z, m_z, v_z, z_best, d->lr_z, (S)d->z_lo, (S)d->z_hi, clamp_z};
  a.mu = FitMap<S>{mu, g_mu, m_mu, v_mu, mu_best, d->lr_mu, (S)d->mu_lo, (S)d->mu_hi, clamp_mu};
  a.n_z = d->n_z;
  a.n = d->n_z + d->n_mu;
  a.beta1 = d->beta1;
  a.beta2 = d->beta2;
  a.w1 = (S)(1.0 - d->beta1);
  a.b2 = (S)d->beta2;
  a.w2 = (S)(1.0 - d->beta2);
  a.eps = (S)d->eps;
  a.loss = loss;
  a.loss_min = loss_min;
  a.history = history;
  a.state = state;
  a.max_iters = d->max_iters;
  const long long blocks = (a.n + kFitBlock - 1) / kFitBlock;
  hipLaunchKernelGGL((terrain_fit_update_kernel<S>), dim3((unsigned)(blocks < kFitMaxBlocks ? blocks : kFitMaxBlocks)), dim3(kFitBlock), 0, st, a);
  hipError_t e = hipGetLastError();
  MF_REQUIRE(e == hipSuccess, MF_ERR_LAUNCH, std::string("terrain_fit_update launch: ") + hipGetErrorString(e));
  return MF_OK;
}

}  // namespace mf

extern "C" int mf_terrain_fit_update_f32(const MfFitDesc* d, float* z, float* mu, const float* g_z, const float* g_mu, float* m_z, float* v_z,
                                         float* m_mu, float* v_mu, const float* loss, float* z_best, float* mu_best, int32_t* state,
                                         float* loss_min, float* history, void* s) {
  return mf::fit_update<float>(d, z, mu, g_z, g_mu, m_z, v_z, m_mu, v_mu, loss, z_best, mu_best, state, loss_min, history, (hipStream_t)s);
}
extern "C" int mf_terrain_fit_update_f64(const MfFitDesc* d, double* z, double* mu, const double* g_z, const double* g_mu, double* m_z,
                                         double* v_z, double* m_mu, double* v_mu, const double* loss, double* z_best, double* mu_best,
                                         int32_t* state, double* loss_min, double* history, void* s) {
  return mf::fit_update<double>(d, z, mu, g_z, g_mu, m_z, v_z, m_mu, v_mu, loss, z_best, mu_best, state, loss_min, history, (hipStream_t)s);
}
extern "C" int mf_terrain_fit_grid_cap(void) { return mf::kFitMaxBlocks; }
