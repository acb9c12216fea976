// Global routes on a cost map (definition: include/monoforce_hip.h at MfCostToGoDesc): the cost-to-go field towards a goal by tiled
// block-asynchronous relaxation, and the optimal route from a start as a [P][2] polyline.
//
// Field.  A 256 x 256 field does not fit one CU's LDS, and nothing here may wait on another workgroup, so a call is ONE initialisation
// launch plus n_rounds launches of cost_to_go_round; the launch boundary is the only ordering across workgroups.  A workgroup of 256
// threads owns a tile of kTile x kTile nodes (four per thread).  In a round, a tile that somebody woke
//   loads its nodes and a one-node halo of d and of the factor s (walls: s = -1, d = +inf) into LDS,
//   forms the eight edge weights of each of its nodes once (+inf for a move that is not permitted),
//   relaxes in place in LDS until a whole sweep changes nothing (racing reads inside the tile see an old or a new value; both are upper
//     bounds of the fixed point and the sweep repeats until nothing moves),
//   stores the nodes that changed, wakes the neighbour tiles whose halo those nodes are in (flags of the NEXT round's parity) and counts
//     itself in the round's `changed` word.
// Round 0 starts from the tiles that have the goal node among their nodes or in their halo (a goal on a tile border behind a doorway is
// seen by the tile across the border although no node of its own tile on that border ever changes).
// A tile nobody woke leaves at once, and so does every tile when the previous round's `changed` word is zero: after convergence the
// remaining rounds are empty launches.  A halo read may see the neighbour's value of this round or of the last one; the neighbour's flag
// brings the tile back.  The field only ever decreases towards the fixed point, which is unique (rounded addition is monotone, the weights
// are positive): the result is bit-equal to a heap Dijkstra whatever the order.  No float atomics, no FMA contraction (Makefile default).
//
// Route.  One wave per map walks the chain v -> argmin_u fl(d[u] + w(u, v)).  Lane l handles neighbour l & 7 (all eight groups of a wave
// compute the same step, so the next node is in every lane without a broadcast), the minimum with its index goes through three DPP
// exchanges inside the group, and lane 0 appends the node.  Afterwards the wave writes the P vertices in parallel.
#include <cmath>

#include "mf_common.h"

namespace mf {

constexpr int kTile = MF_ROUTE_TILE;      // nodes per tile edge
constexpr int kPitch = kTile + 2;         // row pitch of the LDS images (tile + halo)
constexpr int kCtgBlock = 256;
constexpr int kPerThread = kTile * kTile / kCtgBlock;
static_assert(kTile * kTile % kCtgBlock == 0 && kCtgBlock % kTile == 0, "a thread's nodes share a column");

template <typename S>
struct CtgArgs {
  const S* cost; const S* goal;
  S* field;
  int32_t* status; int32_t* rounds_used; int32_t* flags; int32_t* changed;
  long long css, csh;
  int nS, H, W, tiles_h, tiles_w, n_rounds, round;
  S res, d_max, lethal, alpha, len_ax, len_dg;
};

template <typename S>
__device__ __forceinline__ bool ctg_finite(S v) { return v - v == (S)0; }
template <typename S>
__device__ __forceinline__ bool ctg_passable(S c, S lethal) { return ctg_finite(c) && c < lethal; }
template <typename S>
__device__ __forceinline__ S ctg_factor(S c, S alpha) { return (S)1 + alpha * (c > (S)0 ? c : (S)0); }
__device__ __forceinline__ float ctg_rint(float v) { return rintf(v); }
__device__ __forceinline__ double ctg_rint(double v) { return rint(v); }

// Nearest node of a position: false when it is off the map (or NaN).
template <typename S>
__device__ __forceinline__ bool ctg_node(S px, S py, S d_max, S res, int H, int W, int* i, int* j) {
  const S fi = ctg_rint((px + d_max) / res), fj = ctg_rint((py + d_max) / res);
  if (!(fi >= (S)0 && fi <= (S)(H - 1) && fj >= (S)0 && fj <= (S)(W - 1))) return false;
  *i = (int)fi; *j = (int)fj;
  return true;
}

// neighbour k of the fixed order
__device__ __forceinline__ int ctg_di(int k) { return k < 4 ? (k == 0 ? -1 : (k == 1 ? 1 : 0)) : ((k & 2) ? 1 : -1); }
__device__ __forceinline__ int ctg_dj(int k) { return k < 4 ? (k == 2 ? -1 : (k == 3 ? 1 : 0)) : ((k & 1) ? 1 : -1); }

// ---- initialisation: the field, the status words and the scratch ------------------------------------------------------------------------
template <typename S>
__global__ void __launch_bounds__(kCtgBlock) cost_to_go_init(const CtgArgs<S> a, long long n_cells, long long n_work) {
  const long long id = (long long)blockIdx.x * kCtgBlock + threadIdx.x;
  const long long cells = (long long)a.H * a.W;
  const int per_map = a.tiles_h * a.tiles_w;
  const long long n_flags = 2ll * a.nS * per_map;
  int s = -1;      // the map this thread's word belongs to, when it needs that map's goal
  if (id < n_cells) s = (int)(id / cells);
  else if (id < n_cells + (long long)a.nS * per_map) s = (int)((id - n_cells) / per_map);      // flags of parity 0
  else if (id >= n_cells + n_work && id < n_cells + n_work + a.nS) s = (int)(id - n_cells - n_work);
  int gi = 0, gj = 0;
  bool ok = false;
  if (s >= 0) {
    ok = ctg_node(a.goal[2 * s], a.goal[2 * s + 1], a.d_max, a.res, a.H, a.W, &gi, &gj);
    if (ok) ok = ctg_passable(a.cost[(long long)s * a.css + (long long)gi * a.csh + gj], a.lethal);
  }
  if (id < n_cells) {
    const long long at = id - (long long)s * cells;
    a.field[id] = (ok && at == (long long)gi * a.W + gj) ? (S)0 : (S)INFINITY;
  } else if (id < n_cells + n_work) {
    const long long k = id - n_cells;
    int v = 0;
    if (s >= 0 && ok) {      // round 0 wakes every tile that has the goal node among its nodes OR IN ITS HALO: the goal's 0 is written here, not
      const int t = (int)(k - (long long)s * per_map), th = t / a.tiles_w, tw = t - th * a.tiles_w;      // by a round, so no round reports it
      v = (gi >= th * kTile - 1 && gi <= th * kTile + kTile && gj >= tw * kTile - 1 && gj <= tw * kTile + kTile) ? 1 : 0;
    }
    a.flags[k] = v;      // flags [2][S][tiles] and changed [S][n_rounds] are one array
  } else if (s >= 0) {
    a.status[s] = ok ? 0 : MF_ROUTE_GOAL_BLOCKED;
    a.rounds_used[s] = 0;
  }
}

// ---- one round ---------------------------------------------------------------------------------------------------------------------------
template <typename S>
__global__ void __launch_bounds__(kCtgBlock) cost_to_go_round(const CtgArgs<S> a) {
  __shared__ S sd[kPitch * kPitch];
  __shared__ S ss[kPitch * kPitch];
  __shared__ int sh_active, sh_moved, sh_wake;
  const int per_map = a.tiles_h * a.tiles_w;
  const int s = (int)(blockIdx.x / (unsigned)per_map), t = (int)(blockIdx.x - (unsigned)s * (unsigned)per_map);
  const int r = a.round;
  int32_t* cur = a.flags + ((long long)(r & 1) * a.nS + s) * per_map;
  int32_t* nxt = a.flags + ((long long)((r + 1) & 1) * a.nS + s) * per_map;
  int32_t* changed = a.changed + (long long)s * a.n_rounds;
  // one thread reads (and clears, for the round after next) the tile's flag; everybody leaves or stays on ITS answer
  if (threadIdx.x == 0) {
    int act = 0;
    if (r == 0 || changed[r - 1] != 0) {
      act = cur[t];
      if (act) cur[t] = 0;
    }
    sh_active = act;
    sh_moved = 0;
    sh_wake = 0;
  }
  __syncthreads();
  if (!sh_active) return;

  const int th = t / a.tiles_w, tw = t - th * a.tiles_w;
  const int i0 = th * kTile - 1, j0 = tw * kTile - 1;      // map node of image element (0, 0)
  const S* cs = a.cost + (long long)s * a.css;
  S* fs = a.field + (long long)s * a.H * a.W;
  const S inf = (S)INFINITY;
  for (int e = (int)threadIdx.x; e < kPitch * kPitch; e += kCtgBlock) {
    const int li = e / kPitch, lj = e - li * kPitch;
    const int i = i0 + li, j = j0 + lj;
    S sv = (S)-1, dv = inf;
    if (i >= 0 && i < a.H && j >= 0 && j < a.W) {
      const S c = cs[(long long)i * a.csh + j];
      if (ctg_passable(c, a.lethal)) {
        sv = ctg_factor(c, a.alpha);
        dv = fs[(long long)i * a.W + j];
      }
    }
    sd[e] = dv;
    ss[e] = sv;
  }
  __syncthreads();

  // this thread's nodes: column tx, rows ty + k * (kCtgBlock / kTile)
  const int tx = (int)threadIdx.x % kTile, ty = (int)threadIdx.x / kTile;
  S w[kPerThread][8], d0[kPerThread];
  bool mine[kPerThread];
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) {
    const int c = (ty + k * (kCtgBlock / kTile) + 1) * kPitch + tx + 1;
    const S sv = ss[c];
    mine[k] = sv >= (S)0;
    d0[k] = sd[c];
#pragma unroll
    for (int m = 0; m < 8; ++m) {
      const int di = ctg_di(m), dj = ctg_dj(m);
      const S su = ss[c + di * kPitch + dj];
      bool ok = mine[k] && su >= (S)0;
      if (m >= 4) ok = ok && ss[c + di * kPitch] >= (S)0 && ss[c + dj] >= (S)0;
      const S len = m < 4 ? a.len_ax : a.len_dg;
      w[k][m] = ok ? len * ((su + sv) * (S)0.5) : inf;
    }
  }

  // relax in place until a whole sweep of the tile changes nothing
  for (;;) {
    bool moved = false;
#pragma unroll
    for (int k = 0; k < kPerThread; ++k) {
      if (!mine[k]) continue;
      const int c = (ty + k * (kCtgBlock / kTile) + 1) * kPitch + tx + 1;
      const S have = sd[c];
      S best = have;
#pragma unroll
      for (int m = 0; m < 8; ++m) {
        const S cand = sd[c + ctg_di(m) * kPitch + ctg_dj(m)] + w[k][m];
        best = cand < best ? cand : best;
      }
      if (best < have) {
        sd[c] = best;
        moved = true;
      }
    }
    if (moved) sh_moved = 1;
    __syncthreads();
    const int any = sh_moved;      // the same word for every thread: the exit is uniform
    __syncthreads();
    if (!any) break;
    if (threadIdx.x == 0) sh_moved = 0;
    __syncthreads();
  }

  // store what changed; which neighbour tiles have those nodes in their halo (bit m = neighbour m of the move order)
  int wake = 0;
#pragma unroll
  for (int k = 0; k < kPerThread; ++k) {
    const int li = ty + k * (kCtgBlock / kTile);
    const S v = sd[(li + 1) * kPitch + tx + 1];
    if (mine[k] && v < d0[k]) {
      fs[(long long)(i0 + 1 + li) * a.W + (j0 + 1 + tx)] = v;
      const bool n = li == 0, so = li == kTile - 1, we = tx == 0, ea = tx == kTile - 1;
      wake |= 0x100 | (n ? 1 : 0) | (so ? 2 : 0) | (we ? 4 : 0) | (ea ? 8 : 0) | (n && we ? 16 : 0) | (n && ea ? 32 : 0) | (so && we ? 64 : 0) |
              (so && ea ? 128 : 0);
    }
  }
  if (wake) atomicOr(&sh_wake, wake);
  __syncthreads();
  const int all = sh_wake;
  if (threadIdx.x < 8 && ((all >> threadIdx.x) & 1)) {
    const int nh = th + ctg_di((int)threadIdx.x), nw = tw + ctg_dj((int)threadIdx.x);
    if (nh >= 0 && nh < a.tiles_h && nw >= 0 && nw < a.tiles_w) nxt[nh * a.tiles_w + nw] = 1;
  }
  if (threadIdx.x == 8 && all) {
    atomicAdd(&changed[r], 1);
    atomicMax(&a.rounds_used[s], r + 1);
    if (r == a.n_rounds - 1) atomicOr(&a.status[s], MF_ROUTE_NOT_CONVERGED);
  }
}

template <typename S>
int cost_to_go_launch(const MfCostToGoDesc* d, const S* cost, const S* goal, S* field, int32_t* status, int32_t* rounds_used, int32_t* work,
                      hipStream_t st) {
  CtgArgs<S> a;
  a.cost = cost; a.goal = goal; a.field = field; a.status = status; a.rounds_used = rounds_used;
  a.css = d->c_stride_s; a.csh = d->c_stride_h;
  a.nS = d->S; a.H = d->H; a.W = d->W; a.n_rounds = d->n_rounds; a.round = 0;
  a.tiles_h = (d->H + kTile - 1) / kTile;
  a.tiles_w = (d->W + kTile - 1) / kTile;
  a.res = (S)d->grid_res; a.d_max = (S)d->d_max; a.lethal = (S)d->lethal; a.alpha = (S)d->alpha;
  a.len_ax = a.res;
  a.len_dg = a.res * (S)1.4142135623730951;
  const long long per_map = (long long)a.tiles_h * a.tiles_w, tiles = per_map * d->S;
  const long long n_cells = (long long)d->S * d->H * d->W, n_work = 2 * tiles + (long long)d->S * d->n_rounds;
  a.flags = work;
  a.changed = work + 2 * tiles;
  const long long init_blocks = (n_cells + n_work + d->S + kCtgBlock - 1) / kCtgBlock;
  MF_REQUIRE(tiles < (1ll << 31) && init_blocks < (1ll << 31), MF_ERR_UNSUPPORTED, "cost_to_go: S * H * W is too large for one launch");
  hipLaunchKernelGGL((cost_to_go_init<S>), dim3((unsigned)init_blocks), dim3(kCtgBlock), 0, st, a, n_cells, n_work);
  for (int r = 0; r < d->n_rounds; ++r) {
    a.round = r;
    hipLaunchKernelGGL((cost_to_go_round<S>), dim3((unsigned)tiles), dim3(kCtgBlock), 0, st, a);
  }
  hipError_t e = hipGetLastError();
  MF_REQUIRE(e == hipSuccess, MF_ERR_LAUNCH, std::string("cost_to_go launch: ") + hipGetErrorString(e));
  return MF_OK;
}

// ---- the route ---------------------------------------------------------------------------------------------------------------------------
template <typename S>
struct RouteArgs {
  const S* field; const S* cost; const S* start; const S* goal;
  int32_t* nodes; int32_t* n_nodes; S* route_cost; float* path; int32_t* status;
  long long css, csh;
  int H, W, P, max_nodes;
  float res_f, d_max_f;
  S res, d_max, lethal, alpha, len_ax, len_dg;
};

// (value, index) of the smaller candidate, ties to the smaller index
template <int CTRL, typename S>
__device__ __forceinline__ void route_min_step(S& v, int& k) {
  const S ov = dpp_mov<CTRL>(v);
  const int ok = __builtin_amdgcn_update_dpp(0, k, CTRL, 0xF, 0xF, true);
  const bool take = ov < v || (ov == v && ok < k);
  v = take ? ov : v;
  k = take ? ok : k;
}

template <typename S>
__global__ void __launch_bounds__(64) extract_route_kernel(const RouteArgs<S> a) {
  const int s = (int)blockIdx.x, lane = (int)threadIdx.x;
  const int H = a.H, W = a.W, P = a.P;
  const S* cs = a.cost + (long long)s * a.css;
  const S* fs = a.field + (long long)s * H * W;
  int32_t* nodes = a.nodes + (long long)s * a.max_nodes;
  float* path = a.path + (long long)s * P * 2;
  const S inf = (S)INFINITY;
  const S px = a.start[2 * s], py = a.start[2 * s + 1];
  int i = 0, j = 0, gi = -1, gj = -1;
  const bool on_map = ctg_node(px, py, a.d_max, a.res, H, W, &i, &j);
  ctg_node(a.goal[2 * s], a.goal[2 * s + 1], a.d_max, a.res, H, W, &gi, &gj);
  const S d_start = on_map ? fs[(long long)i * W + j] : inf;
  int bits = a.status[s] & (MF_ROUTE_GOAL_BLOCKED | MF_ROUTE_NOT_CONVERGED);
  if (!(on_map && ctg_finite(d_start))) {      // (uniform: every lane computed the same)
    for (int p = lane; p < P; p += 64) {
      path[2 * p] = (float)px;
      path[2 * p + 1] = (float)py;
    }
    if (lane == 0) {
      a.n_nodes[s] = 0;
      a.route_cost[s] = inf;
      a.status[s] = bits | MF_ROUTE_START_UNREACHABLE;
    }
    return;
  }
  const int m = lane & 7, di = ctg_di(m), dj = ctg_dj(m);
  const S len = m < 4 ? a.len_ax : a.len_dg;
  int L = 0;
  for (;;) {
    if (lane == 0) nodes[L] = i * W + j;
    ++L;
    if (i == gi && j == gj) break;
    if (L == a.max_nodes) { bits |= MF_ROUTE_TRUNCATED; break; }
    const int ui = i + di, uj = j + dj;
    S cand = inf;
    if (ui >= 0 && ui < H && uj >= 0 && uj < W) {
      const S cu = cs[(long long)ui * a.csh + uj], cv = cs[(long long)i * a.csh + j];
      const S du = fs[(long long)ui * W + uj];
      bool ok = ctg_passable(cu, a.lethal);
      if (m >= 4) ok = ok && ctg_passable(cs[(long long)ui * a.csh + j], a.lethal) && ctg_passable(cs[(long long)i * a.csh + uj], a.lethal);
      if (ok) cand = du + len * ((ctg_factor(cu, a.alpha) + ctg_factor(cv, a.alpha)) * (S)0.5);
    }
    int k = m;
    route_min_step<0xB1>(cand, k);       // quad_perm [1,0,3,2]
    route_min_step<0x4E>(cand, k);       // quad_perm [2,3,0,1]
    route_min_step<0x141>(cand, k);      // row_half_mirror: the other quad of the eight
    if (!(cand < inf)) { bits |= MF_ROUTE_TRUNCATED; break; }
    i += ctg_di(k);
    j += ctg_dj(k);
  }
  __threadfence_block();      // lane 0's nodes, read below by every lane of this (one-wave) workgroup
  __syncthreads();
  for (int p = lane; p < P; p += 64) {
    const int node = nodes[(int)(((long long)p * (L - 1)) / (P - 1))];
    const int ni = node / W, nj = node - ni * W;
    path[2 * p] = (float)ni * a.res_f - a.d_max_f;
    path[2 * p + 1] = (float)nj * a.res_f - a.d_max_f;
  }
  if (lane == 0) {
    a.n_nodes[s] = L;
    a.route_cost[s] = d_start;
    a.status[s] = bits;
  }
}

template <typename S>
int extract_route_launch(const MfRouteDesc* d, const S* field, const S* cost, const S* start, const S* goal, int32_t* nodes, int32_t* n_nodes,
                         S* route_cost, float* path, int32_t* status, hipStream_t st) {
  RouteArgs<S> a;
  a.field = field; a.cost = cost; a.start = start; a.goal = goal;
  a.nodes = nodes; a.n_nodes = n_nodes; a.route_cost = route_cost; a.path = path; a.status = status;
  a.css = d->c_stride_s; a.csh = d->c_stride_h;
  a.H = d->H; a.W = d->W; a.P = d->P; a.max_nodes = d->max_nodes;
  a.res_f = d->grid_res; a.d_max_f = d->d_max;
  a.res = (S)d->grid_res; a.d_max = (S)d->d_max; a.lethal = (S)d->lethal; a.alpha = (S)d->alpha;
  a.len_ax = a.res;
  a.len_dg = a.res * (S)1.4142135623730951;
  hipLaunchKernelGGL((extract_route_kernel<S>), dim3((unsigned)d->S), dim3(64), 0, st, a);
  hipError_t e = hipGetLastError();
  MF_REQUIRE(e == hipSuccess, MF_ERR_LAUNCH, std::string("extract_route launch: ") + hipGetErrorString(e));
  return MF_OK;
}

template int cost_to_go_launch<float>(const MfCostToGoDesc*, const float*, const float*, float*, int32_t*, int32_t*, int32_t*, hipStream_t);
template int cost_to_go_launch<double>(const MfCostToGoDesc*, const double*, const double*, double*, int32_t*, int32_t*, int32_t*, hipStream_t);
template int extract_route_launch<float>(const MfRouteDesc*, const float*, const float*, const float*, const float*, int32_t*, int32_t*, float*,
                                         float*, int32_t*, hipStream_t);
template int extract_route_launch<double>(const MfRouteDesc*, const double*, const double*, const double*, const double*, int32_t*, int32_t*,
                                          double*, float*, int32_t*, hipStream_t);

}  // namespace mf
