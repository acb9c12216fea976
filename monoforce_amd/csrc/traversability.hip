// Planner cost maps from terrain: slope, roughness and step height of the terrain under a disc of r cells around every cell, ramped and
// merged into one cost in [0,1] (definition: include/monoforce_hip.h at MfTraversabilityDesc).  ONE launch per call writes cost [S][H][W] and,
// when asked, terms [S][3][H][W]; no reduction across workgroups, no atomics, nothing to clear first, no host read: capturable.
// A workgroup of kTravTile x kTravTile threads owns that tile of output cells of one map.  It stages the tile plus a halo of r cells into
// LDS once, with validity folded in: a cell off the map, non-finite, or with valid == 0 is a NaN in the image.  Every window read then comes
// from LDS; the lanes of a wave (4 tile rows x 16 columns) read 16 adjacent words per row at every window offset, rows kTravPitch = 48 words
// apart (48, 96, 144 mod 64 = 48, 32, 16: the four rows fall on disjoint banks).  The loop bounds (the disc's half width per row) are the
// same for every thread, so a wave never diverges on them.
// Three passes over the window, all on the LDS image:
//   1  n, the integer moments of (di, dj), sum z, min z, max z                     -> known?, mean1 = sum z / n
//   2  dz = z - mean1:  sum dz (the mean's rounding error, fed back),  sum (n di - sum di) dz,  sum (n dj - sum dj) dz     -> plane
//   3  the residuals themselves, squared and summed
// The heights are centred before any product is formed; the centred offsets n di - sum di are integers below 2^24, exact in float32.
// Summation: every row of the disc (at most 33 cells) is summed in S with fused multiply-adds (one rounding per term), the row sums are
// added up and the 2 x 2 system, the square roots and the ramps are evaluated in double -- a dozen double operations per row and cell
// next to the row's 33 float ones.  A plain float32 chain over the 805 cells of the largest disc measured 2.4 x the error of the ATen
// form's tree reductions on the same inputs.
// With A = n sum di^2 - (sum di)^2, B, C likewise and D = A B - C^2 (64-bit integers, include/monoforce_hip.h), the centred normal
// equations give the plane's rise per CELL as  pa = (B suz - C svz) / D,  pb = (A svz - C suz) / D  with suz = sum (n di - sum di) dz.
// IEEE division / square root (this TU is built without -ffast-math and with -ffp-contract=off, like map_losses.hip); the float64
// instantiation is the validation build of the same source.
#include "mf_common.h"

namespace mf {

constexpr int kTravTile = MF_TRAVERSABILITY_TILE;          // output cells per workgroup edge
constexpr int kTravMaxR = MF_TRAVERSABILITY_MAX_RADIUS;
constexpr int kTravPitch = kTravTile + 2 * kTravMaxR;      // row pitch of the LDS image in scalars (the image of the largest radius)
constexpr int kTravBlock = kTravTile * kTravTile;

template <typename S>
struct TravArgs {
  const S* z; const S* valid; const S* base;
  S* cost; S* terms;
  long long zss, zsh, vss, vsh, bss, bsh;
  int H, W, r, min_valid, tiles_w, tiles_h;
  S grid_res, unknown;
  double lo[3], span[3];      // span[k] = hi[k] - lo[k]
};

__device__ __forceinline__ double trav_ramp(double t, double lo, double span) { return mf_clamp((t - lo) / span, 0.0, 1.0); }

template <typename S>
__global__ void __launch_bounds__(kTravBlock) traversability_kernel(const TravArgs<S> a) {
  __shared__ S img[kTravPitch * kTravPitch];
  __shared__ int half_w[2 * kTravMaxR + 1];
  const int r = a.r, H = a.H, W = a.W;
  const unsigned tile = blockIdx.x;
  const unsigned per_map = (unsigned)a.tiles_w * (unsigned)a.tiles_h;
  const unsigned s = tile / per_map, t_in = tile - s * per_map;
  const int th = (int)(t_in / (unsigned)a.tiles_w), tw = (int)(t_in - (unsigned)th * (unsigned)a.tiles_w);
  const int h0 = th * kTravTile - r, w0 = tw * kTravTile - r;      // map cell of image element (0, 0)
  const int edge = kTravTile + 2 * r;                             // <= kTravPitch

  // half width of the disc at row di: the largest dj with di^2 + dj^2 <= r^2, in integers
  if ((int)threadIdx.x <= 2 * r) {
    const int di = (int)threadIdx.x - r, rem = r * r - di * di;
    int wj = 0;
    while ((wj + 1) * (wj + 1) <= rem) ++wj;
    half_w[threadIdx.x] = wj;
  }
  // the tile and its halo, validity folded in as NaN
  const S nan = __builtin_nan("");
  const S* zs = a.z + (long long)s * a.zss;
  const S* vs = a.valid ? a.valid + (long long)s * a.vss : nullptr;
  for (int e = (int)threadIdx.x; e < edge * edge; e += kTravBlock) {
    const int ih = e / edge, iw = e - ih * edge;
    const int h = h0 + ih, w = w0 + iw;
    S v = nan;
    if (h >= 0 && h < H && w >= 0 && w < W) {
      v = zs[(long long)h * a.zsh + w];
      if (!(v - v == (S)0)) v = nan;                               // +-inf and NaN: not a window cell
      if (vs && vs[(long long)h * a.vsh + w] == (S)0) v = nan;     // (valid: nonzero means usable; a NaN there is nonzero)
    }
    img[ih * kTravPitch + iw] = v;
  }
  __syncthreads();

  const int ty = (int)threadIdx.x / kTravTile, tx = (int)threadIdx.x - ty * kTravTile;
  const S* centre = img + (ty + r) * kTravPitch + (tx + r);

  // pass 1: the count, the integer moments, the sum and the range
  int n = 0, si = 0, sj = 0, sii = 0, sjj = 0, sij = 0;
  double sz = 0.0;
  S zmin = (S)INFINITY, zmax = -(S)INFINITY;
  for (int di = -r; di <= r; ++di) {
    const int hw = half_w[di + r];
    const S* row = centre + di * kTravPitch;
    S r_z = (S)0;
    for (int dj = -hw; dj <= hw; ++dj) {
      const S v = row[dj];
      if (v == v) {
        ++n; si += di; sj += dj; sii += di * di; sjj += dj * dj; sij += di * dj;
        r_z += v;
        zmin = v < zmin ? v : zmin;
        zmax = v > zmax ? v : zmax;
      }
    }
    sz += (double)r_z;
  }
  const long long A = (long long)n * sii - (long long)si * si, B = (long long)n * sjj - (long long)sj * sj,
                  C = (long long)n * sij - (long long)si * sj;
  const long long D = A * B - C * C;
  const bool known = n >= a.min_valid && D > 0;

  double slope = (double)nan, rough = (double)nan;
  S step = nan;
  if (known) {      // (per lane: an unknown cell's lanes idle through the two passes of their wave)
    const double fn = (double)n;
    const S mean1 = (S)(sz / fn);
    // pass 2: heights centred on mean1; ci = n di - sum di, cj = n dj - sum dj are exact integers (in S too: below 2^24)
    double sdz = 0.0, suz = 0.0, svz = 0.0;
    for (int di = -r; di <= r; ++di) {
      const int hw = half_w[di + r];
      const S* row = centre + di * kTravPitch;
      S r_dz = (S)0, r_jdz = (S)0;
      for (int dj = -hw; dj <= hw; ++dj) {
        const S v = row[dj];
        if (v == v) {
          const S dz = v - mean1;
          r_dz += dz;
          r_jdz = mf_fma((S)(n * dj - sj), dz, r_jdz);
        }
      }
      sdz += (double)r_dz;
      suz += (double)(n * di - si) * (double)r_dz;
      svz += (double)r_jdz;
    }
    const double dbar = sdz / fn;                  // what mean1 missed of the mean (the plane's own sums do not see it: sum ci = 0)
    const double pa = ((double)B * suz - (double)C * svz) / (double)D;   // rise per cell along H and W
    const double pb = ((double)A * svz - (double)C * suz) / (double)D;
    // pass 3: the residuals themselves, e = (dz - dbar) - (pa ci + pb cj) / n
    const S q = (S)(pb / fn);
    double see = 0.0;
    for (int di = -r; di <= r; ++di) {
      const int hw = half_w[di + r];
      const S* row = centre + di * kTravPitch;
      const S off = (S)(dbar + pa * (double)(n * di - si) / fn);
      S r_ee = (S)0;
      for (int dj = -hw; dj <= hw; ++dj) {
        const S v = row[dj];
        if (v == v) {
          const S e = mf_fma(-q, (S)(n * dj - sj), (v - mean1) - off);
          r_ee = mf_fma(e, e, r_ee);
        }
      }
      see += (double)r_ee;
    }
    slope = sqrt(pa * pa + pb * pb) / (double)a.grid_res;
    rough = sqrt(see / fn);
    step = zmax - zmin;
  }

  const int h = th * kTravTile + ty, w = tw * kTravTile + tx;
  if (h >= H || w >= W) return;      // (after the only barrier)
  S cost = a.unknown;
  if (known) {
    const double c0 = trav_ramp(slope, a.lo[0], a.span[0]), c1 = trav_ramp(rough, a.lo[1], a.span[1]),
                 c2 = trav_ramp((double)step, a.lo[2], a.span[2]);
    cost = (S)mf_max(mf_max(c0, c1), c2);
  }
  if (a.base) {
    const S b = a.base[(long long)s * a.bss + (long long)h * a.bsh + w];
    if (b == b) cost = mf_max(cost, b);
  }
  const long long cells = (long long)H * W, at = (long long)h * W + w;
  a.cost[(long long)s * cells + at] = cost;
  if (a.terms) {
    S* t = a.terms + (long long)s * 3 * cells + at;
    t[0] = (S)slope;
    t[cells] = (S)rough;
    t[2 * cells] = step;
  }
}

// The launch of a validated descriptor (capi.hip: mf_traversability_*).
template <typename S>
int traversability_launch(const MfTraversabilityDesc* d, const S* z, const S* valid, const S* base, S* cost, S* terms, hipStream_t st) {
  TravArgs<S> a;
  a.z = z; a.valid = valid; a.base = base; a.cost = cost; a.terms = terms;
  a.zss = d->z_stride_s; a.zsh = d->z_stride_h; a.vss = d->v_stride_s; a.vsh = d->v_stride_h; a.bss = d->b_stride_s; a.bsh = d->b_stride_h;
  a.H = d->H; a.W = d->W; a.r = d->r; a.min_valid = d->min_valid;
  a.tiles_w = (d->W + kTravTile - 1) / kTravTile;
  a.tiles_h = (d->H + kTravTile - 1) / kTravTile;
  a.grid_res = (S)d->grid_res; a.unknown = (S)d->unknown;
  for (int k = 0; k < 3; ++k) { a.lo[k] = (double)d->lo[k]; a.span[k] = (double)d->hi[k] - (double)d->lo[k]; }
  const long long tiles = (long long)a.tiles_w * a.tiles_h * d->S;
  MF_REQUIRE(tiles < (1ll << 31), MF_ERR_UNSUPPORTED, "traversability: S * ceil(H/16) * ceil(W/16) must be below 2^31");
  hipLaunchKernelGGL((traversability_kernel<S>), dim3((unsigned)tiles), dim3(kTravBlock), 0, st, a);
  hipError_t e = hipGetLastError();
  MF_REQUIRE(e == hipSuccess, MF_ERR_LAUNCH, std::string("traversability launch: ") + hipGetErrorString(e));
  return MF_OK;
}

template int traversability_launch<float>(const MfTraversabilityDesc*, const float*, const float*, const float*, float*, float*, hipStream_t);
template int traversability_launch<double>(const MfTraversabilityDesc*, const double*, const double*, const double*, double*, double*, hipStream_t);

}  // namespace mf
