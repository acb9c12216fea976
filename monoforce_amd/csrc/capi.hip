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
