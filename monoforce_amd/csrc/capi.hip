// Library-wide pieces of the C ABI: error text and version.
#include "mf_common.h"

namespace mf {
static thread_local std::string g_last_error;
void set_error(const std::string& msg) { g_last_error = msg; }
}  // namespace mf

namespace mf {
int device_cus() {
  static thread_local int cached_dev = -2, cached_cus = 256;
  int dev = -1;
  if (hipGetDevice(&dev) != hipSuccess) { (void)hipGetLastError(); return 256; }
  if (dev != cached_dev) {
    int cus = 0;
    if (hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || cus <= 0) { (void)hipGetLastError(); cus = 256; }
    cached_dev = dev; cached_cus = cus;
  }
  return cached_cus;
}
}  // namespace mf

namespace mf {
static thread_local const void* g_launch_stub = nullptr;
static thread_local unsigned g_launch_grid = 0, g_launch_block = 0, g_launch_count = 0;
static thread_local std::string g_launch_text;
void note_launch(const void* kernel_stub, unsigned grid, unsigned block) {
  g_launch_stub = kernel_stub; g_launch_grid = grid; g_launch_block = block; ++g_launch_count;
}
}  // namespace mf

#include <cxxabi.h>
// The last rollout kernel THIS thread launched through the library: "<demangled kernel template> grid=G block=B launches=N" (N = rollout-kernel
// launches of this thread so far; "" before the first).  Thread-local like mf_last_error: concurrent streams / threads read their own.
extern "C" const char* mf_last_launch(void) {
  if (!mf::g_launch_stub) return "";
  const char* mangled = hipKernelNameRefByPtr(mf::g_launch_stub, nullptr);
  std::string name = mangled ? mangled : "?";
  if (mangled) {
    int status = 1;
    char* dem = abi::__cxa_demangle(mangled, nullptr, nullptr, &status);
    if (status == 0 && dem) {
      name = dem;
      const size_t paren = name.find('(');      // drop the parameter list
      if (paren != std::string::npos) name.resize(paren);
      if (name.compare(0, 5, "void ") == 0) name.erase(0, 5);
    }
    free(dem);
  }
  mf::g_launch_text = name + " grid=" + std::to_string(mf::g_launch_grid) + " block=" + std::to_string(mf::g_launch_block) +
                      " launches=" + std::to_string(mf::g_launch_count);
  return mf::g_launch_text.c_str();
}

// (thread-local: two host threads driving two streams each read the message of their own failed call)
extern "C" const char* mf_last_error(void) { return mf::g_last_error.c_str(); }
extern "C" const char* mf_version(void) { return "monoforce_hip 0.1 gfx950"; }

// sizeof() of the ABI structs, so language bindings can verify their mirrors (tests/test_capi_cpu.py)
#include <string.h>
extern "C" int mf_sizeof(const char* name) {
  if (!strcmp(name, "MfRolloutDesc")) return (int)sizeof(MfRolloutDesc);
  if (!strcmp(name, "MfRolloutFwdBufs")) return (int)sizeof(MfRolloutFwdBufs);
  if (!strcmp(name, "MfRolloutBwdBufs")) return (int)sizeof(MfRolloutBwdBufs);
  if (!strcmp(name, "MfSplatDesc")) return (int)sizeof(MfSplatDesc);
  if (!strcmp(name, "MfLossDesc")) return (int)sizeof(MfLossDesc);
  if (!strcmp(name, "MfHeightmapDesc")) return (int)sizeof(MfHeightmapDesc);
  if (!strcmp(name, "MfStageDesc")) return (int)sizeof(MfStageDesc);
  if (!strcmp(name, "MfInterpDesc")) return (int)sizeof(MfInterpDesc);
  if (!strcmp(name, "MfRolloutLoss")) return (int)sizeof(MfRolloutLoss);
  if (!strcmp(name, "MfMppiDesc")) return (int)sizeof(MfMppiDesc);
  if (!strcmp(name, "MfPoseCostDesc")) return (int)sizeof(MfPoseCostDesc);
  if (!strcmp(name, "MfPoseLossDesc")) return (int)sizeof(MfPoseLossDesc);
  if (!strcmp(name, "MfMapLossDesc")) return (int)sizeof(MfMapLossDesc);
  if (!strcmp(name, "MfFitDesc")) return (int)sizeof(MfFitDesc);
  if (!strcmp(name, "MfTrajObjDesc")) return (int)sizeof(MfTrajObjDesc);
  if (!strcmp(name, "MfRefineDesc")) return (int)sizeof(MfRefineDesc);
  if (!strcmp(name, "MfTraversabilityDesc")) return (int)sizeof(MfTraversabilityDesc);
  if (!strcmp(name, "MfTerrainLabelsDesc")) return (int)sizeof(MfTerrainLabelsDesc);
  if (!strcmp(name, "MfCostToGoDesc")) return (int)sizeof(MfCostToGoDesc);
  if (!strcmp(name, "MfRouteDesc")) return (int)sizeof(MfRouteDesc);
  return -1;
}

// ---- mf_traversability_*: the descriptor is validated here (no device needed), the launch is traversability.hip's
namespace mf {
template <typename S>
int traversability_launch(const MfTraversabilityDesc* d, const S* z, const S* valid, const S* base, S* cost, S* terms, hipStream_t st);

template <typename S>
static int traversability(const MfTraversabilityDesc* d, const S* z, const S* valid, const S* base, S* cost, S* terms, void* st) {
  MF_REQUIRE(d, MF_ERR_INVALID, "traversability: null descriptor");
  MF_REQUIRE(d->S > 0 && d->H > 0 && d->W > 0, MF_ERR_INVALID, "traversability: S, H, W must be positive");
  MF_REQUIRE(z && cost, MF_ERR_INVALID, "traversability: null input (z and cost are required)");
  MF_REQUIRE(d->r >= 1 && d->r <= MF_TRAVERSABILITY_MAX_RADIUS, MF_ERR_INVALID,
             "traversability: the window radius r must be in 1.." + std::to_string(MF_TRAVERSABILITY_MAX_RADIUS) + " cells, got " +
                 std::to_string(d->r));
  MF_REQUIRE(d->min_valid >= 3, MF_ERR_INVALID, "traversability: min_valid must be at least 3 (a plane has three parameters)");
  MF_REQUIRE(d->grid_res > 0.f, MF_ERR_INVALID, "traversability: grid_res must be positive");
  for (int k = 0; k < 3; ++k)
    MF_REQUIRE(d->hi[k] > d->lo[k], MF_ERR_INVALID, "traversability: hi must be above lo for every term (slope, roughness, step)");
  return traversability_launch<S>(d, z, valid, base, cost, terms, (hipStream_t)st);
}
}  // namespace mf

extern "C" int mf_traversability_f32(const MfTraversabilityDesc* d, const float* z, const float* valid, const float* base, float* cost,
                                     float* terms, void* s) {
  return mf::traversability<float>(d, z, valid, base, cost, terms, s);
}
extern "C" int mf_traversability_f64(const MfTraversabilityDesc* d, const double* z, const double* valid, const double* base, double* cost,
                                     double* terms, void* s) {
  return mf::traversability<double>(d, z, valid, base, cost, terms, s);
}

// ---- mf_cost_to_go_* / mf_extract_route_*: the descriptors are validated here (no device needed), the launches are cost_to_go.hip's
namespace mf {
template <typename S>
int cost_to_go_launch(const MfCostToGoDesc* d, const S* cost, const S* goal, S* field, int32_t* status, int32_t* rounds_used, int32_t* work,
                      hipStream_t st);
template <typename S>
int extract_route_launch(const MfRouteDesc* d, const S* field, const S* cost, const S* start, const S* goal, int32_t* nodes, int32_t* n_nodes,
                         S* route_cost, float* path, int32_t* status, hipStream_t st);

static int cost_to_go_desc_ok(const MfCostToGoDesc* d) {
  MF_REQUIRE(d, MF_ERR_INVALID, "cost_to_go: null descriptor");
  MF_REQUIRE(d->S > 0 && d->H > 0 && d->W > 0, MF_ERR_INVALID, "cost_to_go: S, H, W must be positive");
  MF_REQUIRE((long long)d->H * d->W < (1ll << 31), MF_ERR_INVALID, "cost_to_go: H * W must be below 2^31 (nodes are int32 indices)");
  MF_REQUIRE(d->grid_res > 0.f, MF_ERR_INVALID, "cost_to_go: grid_res must be positive");
  MF_REQUIRE(d->alpha >= 0.f && d->alpha <= 3.402823466e38f, MF_ERR_INVALID, "cost_to_go: alpha must be finite and not negative");
  MF_REQUIRE(d->n_rounds >= 1, MF_ERR_INVALID, "cost_to_go: n_rounds must be at least 1, got " + std::to_string(d->n_rounds));
  return MF_OK;
}

template <typename S>
static int cost_to_go(const MfCostToGoDesc* d, const S* cost, const S* goal, S* field, int32_t* status, int32_t* rounds_used, int32_t* work,
                      void* st) {
  if (int rc = cost_to_go_desc_ok(d)) return rc;
  MF_REQUIRE(cost && goal && field && status && rounds_used && work, MF_ERR_INVALID,
             "cost_to_go: null input (cost, goal, field, status, rounds_used and work are required)");
  return cost_to_go_launch<S>(d, cost, goal, field, status, rounds_used, work, (hipStream_t)st);
}

template <typename S>
static int extract_route(const MfRouteDesc* d, const S* field, const S* cost, const S* start, const S* goal, int32_t* nodes, int32_t* n_nodes,
                         S* route_cost, float* path, int32_t* status, void* st) {
  MF_REQUIRE(d, MF_ERR_INVALID, "extract_route: null descriptor");
  MF_REQUIRE(d->S > 0 && d->H > 0 && d->W > 0, MF_ERR_INVALID, "extract_route: S, H, W must be positive");
  MF_REQUIRE((long long)d->H * d->W < (1ll << 31), MF_ERR_INVALID, "extract_route: H * W must be below 2^31 (nodes are int32 indices)");
  MF_REQUIRE(d->P >= 2 && d->P <= MF_ROUTE_MAX_VERTICES, MF_ERR_INVALID,
             "extract_route: P must be in 2.." + std::to_string(MF_ROUTE_MAX_VERTICES) + " vertices, got " + std::to_string(d->P));
  MF_REQUIRE(d->max_nodes >= 2, MF_ERR_INVALID, "extract_route: max_nodes must be at least 2, got " + std::to_string(d->max_nodes));
  MF_REQUIRE(d->grid_res > 0.f, MF_ERR_INVALID, "extract_route: grid_res must be positive");
  MF_REQUIRE(d->alpha >= 0.f && d->alpha <= 3.402823466e38f, MF_ERR_INVALID, "extract_route: alpha must be finite and not negative");
  MF_REQUIRE(field && cost && start && goal && nodes && n_nodes && route_cost && path && status, MF_ERR_INVALID,
             "extract_route: null input (every pointer is required)");
  return extract_route_launch<S>(d, field, cost, start, goal, nodes, n_nodes, route_cost, path, status, (hipStream_t)st);
}
}  // namespace mf

extern "C" long long mf_cost_to_go_work_ints(const MfCostToGoDesc* d) {
  if (mf::cost_to_go_desc_ok(d) != MF_OK) return -1;
  const long long tiles = (long long)((d->H + MF_ROUTE_TILE - 1) / MF_ROUTE_TILE) * ((d->W + MF_ROUTE_TILE - 1) / MF_ROUTE_TILE);
  return (long long)d->S * (2 * tiles + d->n_rounds);
}
extern "C" int mf_cost_to_go_f32(const MfCostToGoDesc* d, const float* cost, const float* goal, float* field, int32_t* status,
                                 int32_t* rounds_used, int32_t* work, void* s) {
  return mf::cost_to_go<float>(d, cost, goal, field, status, rounds_used, work, s);
}
extern "C" int mf_cost_to_go_f64(const MfCostToGoDesc* d, const double* cost, const double* goal, double* field, int32_t* status,
                                 int32_t* rounds_used, int32_t* work, void* s) {
  return mf::cost_to_go<double>(d, cost, goal, field, status, rounds_used, work, s);
}
extern "C" int mf_extract_route_f32(const MfRouteDesc* d, const float* field, const float* cost, const float* start, const float* goal,
                                    int32_t* nodes, int32_t* n_nodes, float* route_cost, float* path, int32_t* status, void* s) {
  return mf::extract_route<float>(d, field, cost, start, goal, nodes, n_nodes, route_cost, path, status, s);
}
extern "C" int mf_extract_route_f64(const MfRouteDesc* d, const double* field, const double* cost, const double* start, const double* goal,
                                    int32_t* nodes, int32_t* n_nodes, double* route_cost, float* path, int32_t* status, void* s) {
  return mf::extract_route<double>(d, field, cost, start, goal, nodes, n_nodes, route_cost, path, status, s);
}
