// C-ABI of the batched frontend pieces (include/okvis_amd_frontend.h).  Host buffers in and out: the inputs of one call are
// packed into one pinned staging block and go to the device with one copy, one kernel runs, the outputs come back with one
// copy.  No CPU path: every entry fails with OKVIS_BA_ERR_NO_DEVICE / a HIP status when there is no GPU.
// This file: the context, the staging helper (Staged / Stage), the camera helpers, create / destroy.  The entries are in the
// fe_capi_*.inc parts included at the end.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cassert>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <type_traits>
#include <vector>

#include "fe_kernels.hpp"
#include "fe_match.hpp"
#include "fe_sac.hpp"
#include "fe_sac_solve.hpp"
#include "fe_sac_gp3p.hpp"
#include "fe_vmatch.hpp"
#include "fe_propagate.hpp"
#include "fe_keyframe.hpp"
#include "fe_sac_loop.hpp"
#include "fe_detect.hpp"
#include "fe_describe.hpp"
#include "fe_detect_scale.hpp"

struct okvis_fe_context {
  int device = 0;
  hipStream_t stream = nullptr;
  char* h_stage = nullptr;  // pinned
  char* d_stage = nullptr;
  size_t cap = 0;
};

namespace {

#define FE_TRY(expr)                                                  \
  do {                                                                \
    hipError_t _e = (expr);                                           \
    if (_e != hipSuccess) return OKVIS_BA_HIP_ERROR_BASE + (int)_e;   \
  } while (0)

int reserve(okvis_fe_context* c, size_t bytes) {
  if (bytes <= c->cap) return OKVIS_BA_OK;
  size_t cap = c->cap ? c->cap : (size_t)1 << 16;
  while (cap < bytes) cap *= 2;
  if (c->h_stage) FE_TRY(hipHostFree(c->h_stage));
  if (c->d_stage) FE_TRY(hipFree(c->d_stage));
  c->h_stage = c->d_stage = nullptr;
  c->cap = 0;
  FE_TRY(hipHostMalloc((void**)&c->h_stage, cap, hipHostMallocDefault));
  FE_TRY(hipMalloc((void**)&c->d_stage, cap));
  c->cap = cap;
  return OKVIS_BA_OK;
}

// One array of the staging block: element type and count; `on` = false for an optional array that is absent (no space, null
// pointers, copies skipped).  Its offset comes from Stage::in / scratch / out, and the copy into the pinned block, the typed
// pointers on both sides and the copy out to the caller are formed from this description alone.
template <class T>
struct Staged {
  size_t off = 0, n = 0;
  bool on = false;
  size_t bytes() const { return sizeof(T) * n; }
  size_t end() const { return off + bytes(); }
};

// The staging block of one call, every array aligned to 16 bytes: the inputs first (one copy to the device), then what only the
// device sees, then the outputs (one copy back, from the first to the last of them).  Every array is planned before reserve(),
// which may move both blocks; pointers are formed from the context's blocks when they are asked for, never kept.
struct Stage {
  okvis_fe_context* c;
  size_t size = 0, in_end = 0, back_lo = 0, back_hi = 0;

  template <class T>
  Staged<T> scratch(size_t n, bool on = true) {
    Staged<T> a;
    if (!on) return a;
    a.off = size, a.n = n, a.on = true;
    size += (a.bytes() + 15) & ~(size_t)15;
    return a;
  }
  template <class T>
  Staged<T> in(size_t n, bool on = true) {
    assert(in_end == size);  // the inputs are one prefix of the block
    const Staged<T> a = scratch<T>(n, on);
    in_end = size;
    return a;
  }
  template <class T>
  Staged<T> out(size_t n, bool on = true) {
    if (back_hi == 0) back_lo = size;
    const Staged<T> a = scratch<T>(n, on);
    back_hi = size;
    return a;
  }
  int reserve() const { return ::reserve(c, size); }
  template <class T>
  T* host(const Staged<T>& a) const { return a.on ? reinterpret_cast<T*>(c->h_stage + a.off) : nullptr; }
  template <class T>
  T* dev(const Staged<T>& a) const { return a.on ? reinterpret_cast<T*>(c->d_stage + a.off) : nullptr; }
  template <class T>
  void put(const Staged<T>& a, const T* src) const { if (a.on) std::memcpy(host(a), src, a.bytes()); }
  template <class T>
  void get(const Staged<T>& a, T* dst) const { if (a.on && dst) std::memcpy(dst, host(a), a.bytes()); }
  int upload() const {
    FE_TRY(hipMemcpyAsync(c->d_stage, c->h_stage, in_end, hipMemcpyHostToDevice, c->stream));
    return OKVIS_BA_OK;
  }
  int download() const {
    FE_TRY(hipMemcpyAsync(c->h_stage + back_lo, c->d_stage + back_lo, back_hi - back_lo, hipMemcpyDeviceToHost, c->stream));
    FE_TRY(hipStreamSynchronize(c->stream));
    return OKVIS_BA_OK;
  }
};

bool camera_ok(const okvis_fe_camera* c) {
  return c && c->model >= OKVIS_BA_DIST_NONE && c->model <= OKVIS_BA_DIST_RADTAN8 && c->intr[0] > 0 && c->intr[1] > 0 &&
         c->width > 0 && c->height > 0;
}
fe::Camera to_device(const okvis_fe_camera* c) {
  fe::Camera d;
  std::memcpy(d.intr, c->intr, sizeof(d.intr));
  d.model = c->model, d.width = c->width, d.height = c->height;
  return d;
}

}  // namespace

extern "C" {

int okvis_fe_create(okvis_fe_context** out, int device) {
  if (!out) return OKVIS_BA_ERR_ARG;
  *out = nullptr;
  int n = 0;
  if (hipGetDeviceCount(&n) != hipSuccess || n <= 0) return OKVIS_BA_ERR_NO_DEVICE;
  if (device < 0 || device >= n) return OKVIS_BA_ERR_ARG;
  FE_TRY(hipSetDevice(device));
  okvis_fe_context* c = new (std::nothrow) okvis_fe_context();
  if (!c) return OKVIS_BA_ERR_ARG;
  c->device = device;
  hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
  if (e != hipSuccess) {
    delete c;
    return OKVIS_BA_HIP_ERROR_BASE + (int)e;
  }
  *out = c;
  return OKVIS_BA_OK;
}

void okvis_fe_destroy(okvis_fe_context* c) {
  if (!c) return;
  (void)hipSetDevice(c->device);
  if (c->stream) (void)hipStreamSynchronize(c->stream), (void)hipStreamDestroy(c->stream);
  if (c->h_stage) (void)hipHostFree(c->h_stage);
  if (c->d_stage) (void)hipFree(c->d_stage);
  delete c;
}

}  // extern "C"

// One translation unit, in parts: the entries by group.  Where a kernel's code lands in the code object follows from two orders,
// which stay as they are (the same code layout, the same timing; see capi_launch.inc): the plain kernels come in the order of the
// headers above, the kernel templates behind them in the order in which the parts first name them (hamming_rows, best_lists,
// verified_lists).
#include "fe_capi_reprojection.inc"   // stereo triangulation (+ _gn), landmark projection, the 3D-2D gate
#include "fe_capi_matching.inc"       // Hamming candidates, descriptor matching, verified matching and their host helpers
#include "fe_capi_ransac.inc"         // bearing vectors, the consensus stage, consensus scoring, the minimal solvers
#include "fe_capi_propagation.inc"    // IMU state propagation
#include "fe_capi_keyframe.inc"       // the keyframe decision
#include "fe_capi_ransac_loop.inc"    // whole RANSAC runs: the sampler and the loop around the solvers and the consensus stage
#include "fe_capi_detect.inc"         // keypoint detection: Harris scores and candidates per tile, selection per image
#include "fe_capi_describe.inc"       // keypoint description: the angle and the descriptor, alone and chained behind the detection
#include "fe_capi_detect_scale.inc"   // keypoint detection over a scale space (octaves > 0), alone and with the description behind it
