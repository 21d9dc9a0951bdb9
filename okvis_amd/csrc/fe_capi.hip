// C-ABI of the batched frontend pieces (include/okvis_amd_frontend.h).  Host buffers in and out: the inputs of one call are
// packed into one pinned staging block and go to the device with one copy, one kernel runs, the outputs come back with one
// copy.  No CPU path: every entry fails with OKVIS_BA_ERR_NO_DEVICE / a HIP status when there is no GPU.
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
#include "fe_vmatch.hpp"
#include "fe_propagate.hpp"
#include "fe_keyframe.hpp"

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

// inverse of a symmetric positive definite 6x6 (row-major) through its Cholesky factor; false when not positive definite
bool spd_inverse6(const double* A, double* inv) {
  double L[36] = {0};
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j <= i; ++j) {
      double s = A[6 * i + j];
      for (int k = 0; k < j; ++k) s -= L[6 * i + k] * L[6 * j + k];
      if (i == j) {
        if (!(s > 0)) return false;
        L[6 * i + i] = std::sqrt(s);
      } else {
        L[6 * i + j] = s / L[6 * j + j];
      }
    }
  double Li[36] = {0};  // L^-1
  for (int c = 0; c < 6; ++c)
    for (int i = c; i < 6; ++i) {
      double s = (i == c) ? 1.0 : 0.0;
      for (int k = c; k < i; ++k) s -= L[6 * i + k] * Li[6 * k + c];
      Li[6 * i + c] = s / L[6 * i + i];
    }
  for (int i = 0; i < 6; ++i)
    for (int j = 0; j < 6; ++j) {
      double s = 0;
      for (int k = (i > j ? i : j); k < 6; ++k) s += Li[6 * k + i] * Li[6 * k + j];
      inv[6 * i + j] = s;
    }
  return true;
}

bool desc_bytes_ok(int32_t n) { return n == 16 || n == 32 || n == 48 || n == 64; }
constexpr int32_t MATCH_MAX_KEYPOINTS = 65536;

// f(std::integral_constant<int, W>) for a descriptor of W x 16 bytes
template <class F>
void with_words(int words, F f) {
  switch (words) {
    case 1: f(std::integral_constant<int, 1>()); break;
    case 2: f(std::integral_constant<int, 2>()); break;
    case 3: f(std::integral_constant<int, 3>()); break;
    default: f(std::integral_constant<int, 4>()); break;
  }
}

template <bool WRITE>
void launch_hamming_rows(int words, const fe::CandParams& P, hipStream_t stream) {
  const dim3 grid((P.n_a + fe::MATCH_WAVES - 1) / fe::MATCH_WAVES), block(fe::MATCH_THREADS);
  with_words(words, [&](auto w) { hipLaunchKernelGGL((fe::hamming_rows_kernel<w(), WRITE>), grid, block, 0, stream, P); });
}

// every pair (first, second) inside [0, n_first) x [0, n_second)
bool pairs_in_range(const int32_t* pairs, int32_t n_pairs, int32_t n_first, int32_t n_second) {
  for (int i = 0; i < n_pairs; ++i)
    if (pairs[2 * i] < 0 || pairs[2 * i] >= n_first || pairs[2 * i + 1] < 0 || pairs[2 * i + 1] >= n_second) return false;
  return true;
}

// stereo_triangulate_kernel over P.n_pairs pairs.  The caller has set the counts, info6 and the device pointers; the cameras, T_AB
// and the default sigma are filled here, cov (where asked) and gn zeroed: the kernel writes them for some pairs only
int launch_triangulate(okvis_fe_context* c, fe::TriParams& P, const okvis_fe_camera* cam_a, const okvis_fe_camera* cam_b,
                       const double* T_AB, bool zero_cov) {
  P.cam_a = to_device(cam_a), P.cam_b = to_device(cam_b);
  std::memcpy(P.T_AB, T_AB, sizeof(P.T_AB));
  P.sigma_ray_own = 0.5 / std::fmin(cam_a->intr[0], cam_b->intr[0]);
  if (zero_cov) FE_TRY(hipMemsetAsync(P.cov, 0, sizeof(double) * 9 * P.n_pairs, c->stream));
  if (P.gn) FE_TRY(hipMemsetAsync(P.gn, 0, sizeof(double) * 81 * P.n_pairs, c->stream));
  hipLaunchKernelGGL(fe::stereo_triangulate_kernel, dim3((P.n_pairs + fe::TRI_THREADS - 1) / fe::TRI_THREADS), dim3(fe::TRI_THREADS),
                     0, c->stream, P);
  FE_TRY(hipGetLastError());
  return OKVIS_BA_OK;
}

// raySigmasA_ / raySigmasB_ of doSetup (VioKeyframeWindowMatchingAlgorithm.cpp:210-221, :251-261) in the reference's operation
// order; products and quotients only, so the host and any IEEE device give the same bits
double ray_sigma(float size, double fu) {
  const double sd = 0.8 * (double)size / 12.0;
  return std::sqrt(std::sqrt(2.0)) * sd / fu;
}

// DenseMatcher::assignbest (okvis_matcher/src/DenseMatcher.cpp:69-111) for row a, its recursion written as a loop: a taker has to
// be strictly better than the holder, and the holder it displaces goes on from position 1 of its own list
void assign_best(int a, int num_best, const int32_t* list_idx, const float* list_dist, int32_t* pair_a, float* pair_dist) {
  int cur = a, start = 0;
  for (;;) {
    const int32_t* li = list_idx + (size_t)cur * num_best;
    const float* ld = list_dist + (size_t)cur * num_best;
    int displaced = -1;
    for (int k = start; k < num_best && li[k] != -1; ++k) {
      const int b = li[k];
      if (pair_a[b] == -1) {
        pair_a[b] = cur, pair_dist[b] = ld[k];
        return;
      }
      if (ld[k] < pair_dist[b]) {
        displaced = pair_a[b];
        pair_a[b] = cur, pair_dist[b] = ld[k];
        break;
      }
    }
    if (displaced < 0) return;
    cur = displaced, start = 1;
  }
}


// the checks the two matching entries share: of the call ...
bool match_call_ok(const okvis_fe_context* c, int32_t n_jobs, const void* jobs, int32_t desc_bytes, int32_t num_best, int32_t use_ratio) {
  return c && n_jobs >= 0 && (n_jobs == 0 || jobs) && desc_bytes_ok(desc_bytes) && num_best >= 1 && num_best <= fe::MATCH_MAX_BEST &&
         !(use_ratio && num_best < 2);
}
// ... and of one job (okvis_fe_match_job or okvis_fe_vmatch_job): its sizes, its descriptors and its three result arrays
template <class Job>
bool match_job_ok(const Job& J) {
  if (J.n_a < 0 || J.n_b < 0 || J.n_a > MATCH_MAX_KEYPOINTS || J.n_b > MATCH_MAX_KEYPOINTS) return false;
  return !(J.n_a > 0 && !J.desc_a) && !(J.n_b > 0 && (!J.desc_b || !J.pair_a || !J.pair_dist || !J.accepted));
}

// What the host does with one job's lists li / ld (its rows of list_idx / list_dist): the assignment chains (sequential by
// nature, O(n_a * num_best)) and matchBody's final loop (DenseMatcher.hpp:92-122).  accepted(b, o) is called for every b the
// loop accepts, o = the first list entry of the row it is paired with.
template <class Job, class Accepted>
void assign_and_accept(const Job& J, const int32_t* li, const float* ld, int32_t num_best, float threshold, int32_t use_ratio,
                       float ratio_threshold, Accepted accepted) {
  for (int b = 0; b < J.n_b; ++b) J.pair_a[b] = -1, J.pair_dist[b] = FLT_MAX, J.accepted[b] = 0;
  if (J.n_a == 0 || J.n_b == 0) return;
  for (int a = 0; a < J.n_a; ++a)
    if (!(J.skip_a && J.skip_a[a])) assign_best(a, num_best, li, ld, J.pair_a, J.pair_dist);
  for (int b = 0; b < J.n_b; ++b) {
    if (!(J.pair_dist[b] < threshold)) continue;
    const size_t o = (size_t)J.pair_a[b] * (size_t)num_best;
    if (use_ratio && li[o + 1] != -1) {
      const float best = ld[o], second = ld[o + 1];
      J.accepted[b] = (best == 0 || second / best > ratio_threshold) ? 1 : 0;
    } else {
      J.accepted[b] = 1;
    }
    if (J.accepted[b]) accepted(b, o);
  }
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

int okvis_fe_stereo_triangulate(okvis_fe_context* c, const okvis_fe_camera* cam_a, const okvis_fe_camera* cam_b,
                                const double* T_AB, const double* UOplus, int32_t n_a, const float* kp_a, int32_t n_b,
                                const float* kp_b, int32_t n_pairs, const int32_t* pairs, const double* sigma_ray,
                                int32_t want_uncertainty, double* hp_a, double* cov, uint8_t* flags) {
  return okvis_fe_stereo_triangulate_gn(c, cam_a, cam_b, T_AB, UOplus, n_a, kp_a, n_b, kp_b, n_pairs, pairs, sigma_ray, want_uncertainty, hp_a,
                                        cov, flags, nullptr);
}

int okvis_fe_stereo_triangulate_gn(okvis_fe_context* c, const okvis_fe_camera* cam_a, const okvis_fe_camera* cam_b,
                                   const double* T_AB, const double* UOplus, int32_t n_a, const float* kp_a, int32_t n_b,
                                   const float* kp_b, int32_t n_pairs, const int32_t* pairs, const double* sigma_ray,
                                   int32_t want_uncertainty, double* hp_a, double* cov, uint8_t* flags, double* gn) {
  if (!c || !camera_ok(cam_a) || !camera_ok(cam_b) || !T_AB || !UOplus || n_a < 0 || n_b < 0 || n_pairs < 0) return OKVIS_BA_ERR_ARG;
  if (n_pairs == 0) return OKVIS_BA_OK;
  if (!kp_a || !kp_b || !pairs || n_a == 0 || n_b == 0 || !pairs_in_range(pairs, n_pairs, n_a, n_b)) return OKVIS_BA_ERR_ARG;
  fe::TriParams P;
  if (!spd_inverse6(UOplus, P.info6)) return OKVIS_BA_ERR_NUMERIC;
  P.n_a = n_a, P.n_b = n_b, P.n_pairs = n_pairs, P.want_uncertainty = want_uncertainty;
  FE_TRY(hipSetDevice(c->device));
  Stage st{c};
  const size_t np = (size_t)n_pairs;
  const auto s_ka = st.in<float>(3 * (size_t)n_a), s_kb = st.in<float>(3 * (size_t)n_b);
  const auto s_pairs = st.in<int32_t>(2 * np);
  const auto s_sig = st.in<double>(np, sigma_ray != nullptr);
  const auto s_hp = st.out<double>(4 * np), s_cov = st.out<double>(9 * np);
  const auto s_fl = st.out<uint8_t>(np);
  const auto s_gn = st.out<double>(81 * np, gn != nullptr);
  if (int rc = st.reserve()) return rc;
  st.put(s_ka, kp_a), st.put(s_kb, kp_b), st.put(s_pairs, pairs), st.put(s_sig, sigma_ray);
  if (int rc = st.upload()) return rc;
  P.kp_a = st.dev(s_ka), P.kp_b = st.dev(s_kb), P.pairs = st.dev(s_pairs), P.sigma_ray = st.dev(s_sig);
  P.hp = st.dev(s_hp), P.cov = st.dev(s_cov), P.flags = st.dev(s_fl), P.gn = st.dev(s_gn);
  if (int rc = launch_triangulate(c, P, cam_a, cam_b, T_AB, cov != nullptr)) return rc;
  if (int rc = st.download()) return rc;
  st.get(s_hp, hp_a), st.get(s_cov, cov), st.get(s_fl, flags), st.get(s_gn, gn);
  return OKVIS_BA_OK;
}

int okvis_fe_project_landmarks(okvis_fe_context* c, const okvis_fe_camera* cam_b, const double* T_CbW, const double* P3,
                               int32_t n, const double* hp_W, double* uv, double* U, uint8_t* status) {
  if (!c || !camera_ok(cam_b) || !T_CbW || !P3 || n < 0) return OKVIS_BA_ERR_ARG;
  if (n == 0) return OKVIS_BA_OK;
  if (!hp_W) return OKVIS_BA_ERR_ARG;
  fe::ProjParams P;
  P.cam = to_device(cam_b);
  std::memcpy(P.T_CbW, T_CbW, sizeof(P.T_CbW));
  std::memcpy(P.P3, P3, sizeof(P.P3));
  P.n = n;
  FE_TRY(hipSetDevice(c->device));
  Stage st{c};
  const auto s_hp = st.in<double>(4 * (size_t)n);
  const auto s_uv = st.out<double>(2 * (size_t)n), s_U = st.out<double>(4 * (size_t)n);
  const auto s_st = st.out<uint8_t>((size_t)n);
  if (int rc = st.reserve()) return rc;
  st.put(s_hp, hp_W);
  if (int rc = st.upload()) return rc;
  P.hp_W = st.dev(s_hp), P.uv = st.dev(s_uv), P.U = st.dev(s_U), P.status = st.dev(s_st);
  hipLaunchKernelGGL(fe::project_landmarks_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, P);
  FE_TRY(hipGetLastError());
  if (int rc = st.download()) return rc;
  st.get(s_uv, uv), st.get(s_U, U), st.get(s_st, status);
  return OKVIS_BA_OK;
}

int okvis_fe_gate_3d2d(okvis_fe_context* c, int32_t n_proj, const double* uv, const double* U, int32_t n_b, const float* kp_b,
                       int32_t n_pairs, const int32_t* pairs, double* chi2, uint8_t* flags) {
  if (!c || n_proj < 0 || n_b < 0 || n_pairs < 0) return OKVIS_BA_ERR_ARG;
  if (n_pairs == 0) return OKVIS_BA_OK;
  if (!uv || !U || !kp_b || !pairs || n_proj == 0 || n_b == 0 || !pairs_in_range(pairs, n_pairs, n_proj, n_b)) return OKVIS_BA_ERR_ARG;
  fe::GateParams P;
  P.n_proj = n_proj, P.n_b = n_b, P.n_pairs = n_pairs;
  FE_TRY(hipSetDevice(c->device));
  Stage st{c};
  const auto s_uv = st.in<double>(2 * (size_t)n_proj), s_U = st.in<double>(4 * (size_t)n_proj);
  const auto s_kb = st.in<float>(3 * (size_t)n_b);
  const auto s_pairs = st.in<int32_t>(2 * (size_t)n_pairs);
  const auto s_chi = st.out<double>((size_t)n_pairs);
  const auto s_fl = st.out<uint8_t>((size_t)n_pairs);
  if (int rc = st.reserve()) return rc;
  st.put(s_uv, uv), st.put(s_U, U), st.put(s_kb, kp_b), st.put(s_pairs, pairs);
  if (int rc = st.upload()) return rc;
  P.uv = st.dev(s_uv), P.U = st.dev(s_U), P.kp_b = st.dev(s_kb), P.pairs = st.dev(s_pairs);
  P.chi2 = st.dev(s_chi), P.flags = st.dev(s_fl);
  hipLaunchKernelGGL(fe::gate_3d2d_kernel, dim3((n_pairs + 255) / 256), dim3(256), 0, c->stream, P);
  FE_TRY(hipGetLastError());
  if (int rc = st.download()) return rc;
  st.get(s_chi, chi2), st.get(s_fl, flags);
  return OKVIS_BA_OK;
}

int okvis_fe_hamming_candidates(okvis_fe_context* c, int32_t desc_bytes, int32_t n_a, const uint8_t* desc_a, const uint8_t* skip_a,
                                int32_t n_b, const uint8_t* desc_b, const uint8_t* skip_b, float threshold, int32_t capacity,
                                int32_t* pairs, float* dist, int32_t* n_pairs) {
  if (!c || !desc_bytes_ok(desc_bytes) || n_a < 0 || n_b < 0 || n_a > MATCH_MAX_KEYPOINTS || n_b > MATCH_MAX_KEYPOINTS || capacity < 0 ||
      !n_pairs || (capacity > 0 && !pairs))
    return OKVIS_BA_ERR_ARG;
  *n_pairs = 0;
  if (n_a == 0 || n_b == 0) return OKVIS_BA_OK;
  if (!desc_a || !desc_b) return OKVIS_BA_ERR_ARG;
  FE_TRY(hipSetDevice(c->device));
  const size_t na = (size_t)n_a, nb = (size_t)n_b, cap = (size_t)capacity, db = (size_t)desc_bytes;
  Stage st{c};
  const auto s_da = st.in<uint8_t>(db * na), s_db = st.in<uint8_t>(db * nb);
  const auto s_sa = st.in<uint8_t>(na, skip_a != nullptr), s_sb = st.in<uint8_t>(nb, skip_b != nullptr);
  const auto s_cnt = st.scratch<int32_t>(na);
  const auto s_off = st.scratch<unsigned long long>(na);
  const auto s_tot = st.out<unsigned long long>(1);  // back: from the total onward
  const auto s_pairs = st.out<int32_t>(2 * cap);
  const auto s_dist = st.out<float>(cap);
  if (int rc = st.reserve()) return rc;
  st.put(s_da, desc_a), st.put(s_db, desc_b), st.put(s_sa, skip_a), st.put(s_sb, skip_b);
  if (int rc = st.upload()) return rc;
  fe::CandParams P;
  P.desc_a = st.dev(s_da), P.desc_b = st.dev(s_db), P.skip_a = st.dev(s_sa), P.skip_b = st.dev(s_sb);
  P.n_a = n_a, P.n_b = n_b, P.threshold = threshold;
  P.counts = st.dev(s_cnt), P.offsets = st.dev(s_off);
  P.capacity = capacity, P.pairs = st.dev(s_pairs), P.dist = st.dev(s_dist);
  launch_hamming_rows<false>(desc_bytes / 16, P, c->stream);
  FE_TRY(hipGetLastError());
  hipLaunchKernelGGL(fe::row_offsets_kernel, dim3(1), dim3(fe::SCAN_THREADS), 0, c->stream, (const int32_t*)P.counts, st.dev(s_off),
                     st.dev(s_tot), n_a);
  FE_TRY(hipGetLastError());
  if (capacity > 0) {
    launch_hamming_rows<true>(desc_bytes / 16, P, c->stream);
    FE_TRY(hipGetLastError());
  }
  if (int rc = st.download()) return rc;
  const unsigned long long total = *st.host(s_tot);
  *n_pairs = total > (unsigned long long)INT32_MAX ? INT32_MAX : (int32_t)total;
  const size_t n = total < cap ? (size_t)total : cap;  // of the capacity, the pairs there are
  if (n) std::copy_n(st.host(s_pairs), 2 * n, pairs);
  if (n && dist) std::copy_n(st.host(s_dist), n, dist);
  return OKVIS_BA_OK;
}

int okvis_fe_match_descriptors(okvis_fe_context* c, int32_t n_jobs, const okvis_fe_match_job* jobs, int32_t desc_bytes, float threshold,
                               int32_t num_best, int32_t use_ratio, float ratio_threshold) {
  if (!match_call_ok(c, n_jobs, jobs, desc_bytes, num_best, use_ratio)) return OKVIS_BA_ERR_ARG;
  size_t rows = 0, blocks = 0, n_live = 0;  // n_live: jobs with keypoints on both sides; the others yield nothing
  for (int j = 0; j < n_jobs; ++j) {
    const okvis_fe_match_job& J = jobs[j];
    if (!match_job_ok(J)) return OKVIS_BA_ERR_ARG;
    if (J.n_a > 0 && J.n_b > 0) ++n_live, rows += (size_t)J.n_a, blocks += (size_t)(J.n_a + fe::MATCH_WAVES - 1) / fe::MATCH_WAVES;
  }
  if (blocks > (size_t)INT32_MAX || rows > (size_t)INT32_MAX) return OKVIS_BA_ERR_ARG;
  const size_t db = (size_t)desc_bytes, nbest = (size_t)num_best;
  Stage st{c};
  Staged<int32_t> s_lidx;
  Staged<float> s_ldist;
  if (rows > 0) {
    FE_TRY(hipSetDevice(c->device));
    // every job's descriptors and masks, then the job table
    struct Plan {
      Staged<uint8_t> da, db, sa, sb;
    };
    std::vector<Plan> plan((size_t)n_jobs);
    for (int j = 0; j < n_jobs; ++j) {
      const okvis_fe_match_job& J = jobs[j];
      if (J.n_a == 0 || J.n_b == 0) continue;
      Plan& p = plan[j];
      p.da = st.in<uint8_t>(db * J.n_a), p.db = st.in<uint8_t>(db * J.n_b);
      p.sa = st.in<uint8_t>((size_t)J.n_a, J.skip_a != nullptr), p.sb = st.in<uint8_t>((size_t)J.n_b, J.skip_b != nullptr);
    }
    const auto s_table = st.in<fe::MatchJob>(n_live);
    s_lidx = st.out<int32_t>(rows * nbest), s_ldist = st.out<float>(rows * nbest);
    if (int rc = st.reserve()) return rc;
    fe::MatchJob* table = st.host(s_table);
    int32_t block0 = 0, row0 = 0;
    for (int j = 0; j < n_jobs; ++j) {
      const okvis_fe_match_job& J = jobs[j];
      if (J.n_a == 0 || J.n_b == 0) continue;
      const Plan& p = plan[j];
      st.put(p.da, J.desc_a), st.put(p.db, J.desc_b), st.put(p.sa, J.skip_a), st.put(p.sb, J.skip_b);
      fe::MatchJob D;
      D.desc_a = st.dev(p.da), D.desc_b = st.dev(p.db), D.skip_a = st.dev(p.sa), D.skip_b = st.dev(p.sb);
      D.n_a = J.n_a, D.n_b = J.n_b, D.block0 = block0, D.row0 = row0;
      *table++ = D;
      block0 += (J.n_a + fe::MATCH_WAVES - 1) / fe::MATCH_WAVES, row0 += J.n_a;
    }
    if (int rc = st.upload()) return rc;
    fe::BestParams P;
    P.jobs = st.dev(s_table), P.n_jobs = (int32_t)n_live;
    P.threshold = threshold, P.initial = use_ratio ? FLT_MAX : threshold, P.num_best = num_best;
    P.list_idx = st.dev(s_lidx), P.list_dist = st.dev(s_ldist);
    with_words(desc_bytes / 16, [&](auto w) {
      hipLaunchKernelGGL(fe::best_lists_kernel<w()>, dim3((unsigned)blocks), dim3(fe::MATCH_THREADS), 0, c->stream, P);
    });
    FE_TRY(hipGetLastError());
    if (int rc = st.download()) return rc;
  }
  size_t row0 = 0;
  for (int j = 0; j < n_jobs; ++j) {
    const okvis_fe_match_job& J = jobs[j];
    assign_and_accept(J, st.host(s_lidx) + row0 * nbest, st.host(s_ldist) + row0 * nbest, num_best, threshold, use_ratio, ratio_threshold,
                      [](int, size_t) {});
    if (J.n_a > 0 && J.n_b > 0) row0 += (size_t)J.n_a;
  }
  return OKVIS_BA_OK;
}

int okvis_fe_match_verified(okvis_fe_context* c, int32_t n_jobs, const okvis_fe_vmatch_job* jobs, int32_t desc_bytes, float threshold,
                            int32_t num_best, int32_t use_ratio, float ratio_threshold) {
  if (!match_call_ok(c, n_jobs, jobs, desc_bytes, num_best, use_ratio)) return OKVIS_BA_ERR_ARG;
  // per job: live = keypoints on both sides (lists are built); pre = the per-keypoint pass has something to do (a 3D2D step
  // reports its projections even against an empty image B); tri = the accepted pairs' uncertainty is wanted
  struct Plan {
    bool live, pre, tri;
    Staged<uint8_t> da, db, sa, sb;       // in
    Staged<float> ka, kb;
    Staged<double> hp, sga, sgb;
    Staged<double> ra, rb;                // device only: the rays
    Staged<double> uv, U;                 // back
    Staged<uint8_t> st;
    Staged<int32_t> t_pairs;              // the uncertainty launch takes ...
    Staged<double> t_sig;
    Staged<double> t_hp, t_cov;           // ... and gives
    Staged<uint8_t> t_fl;
    double info6[36];
  };
  std::vector<Plan> plan((size_t)n_jobs);
  size_t rows = 0, blocks = 0, pre_blocks = 0, n_work = 0;
  for (int j = 0; j < n_jobs; ++j) {
    const okvis_fe_vmatch_job& J = jobs[j];
    Plan& p = plan[j];
    const bool is2d = J.kind == OKVIS_FE_MATCH_2D2D;
    if ((!is2d && J.kind != OKVIS_FE_MATCH_3D2D) || !match_job_ok(J) || !camera_ok(&J.cam_a) || !camera_ok(&J.cam_b)) return OKVIS_BA_ERR_ARG;
    if (!J.kp_b || (is2d && !J.kp_a) || (!is2d && J.n_a > 0 && !J.hp_W)) return OKVIS_BA_ERR_ARG;
    p.live = J.n_a > 0 && J.n_b > 0;
    p.pre = is2d ? p.live : J.n_a > 0;
    p.tri = is2d && (J.hp_a || J.cov || J.tri_flags);
    if (p.tri && !spd_inverse6(J.UOplus, p.info6)) return OKVIS_BA_ERR_ARG;
    p.tri = p.tri && p.live;
    if (p.live) rows += (size_t)J.n_a, blocks += (size_t)(J.n_a + fe::MATCH_WAVES - 1) / fe::MATCH_WAVES;
    if (p.pre) ++n_work, pre_blocks += ((size_t)J.n_a + (is2d ? (size_t)J.n_b : 0) + fe::VMATCH_PRE_THREADS - 1) / fe::VMATCH_PRE_THREADS;
  }
  if (blocks > (size_t)INT32_MAX || rows > (size_t)INT32_MAX || pre_blocks > (size_t)INT32_MAX) return OKVIS_BA_ERR_ARG;
  const size_t db = (size_t)desc_bytes, nbest = (size_t)num_best;
  Stage st{c};
  Staged<int32_t> s_lidx;
  Staged<float> s_ldist;
  Staged<double> s_lchi;
  Staged<uint8_t> s_lfl;
  if (n_work > 0) {
    FE_TRY(hipSetDevice(c->device));
    // in: every job's descriptors, masks, keypoints, landmarks and ray sigmas, then the job table; device only: the rays;
    // back: the projections and the lists; then what the uncertainty launches take and give
    for (int j = 0; j < n_jobs; ++j) {
      const okvis_fe_vmatch_job& J = jobs[j];
      Plan& p = plan[j];
      if (!p.pre) continue;
      const bool is2d = J.kind == OKVIS_FE_MATCH_2D2D;
      const size_t na = (size_t)J.n_a, nb = (size_t)J.n_b;
      p.da = st.in<uint8_t>(db * na, p.live), p.db = st.in<uint8_t>(db * nb, p.live), p.kb = st.in<float>(3 * nb, p.live);
      p.sa = st.in<uint8_t>(na, J.skip_a != nullptr), p.sb = st.in<uint8_t>(nb, p.live && J.skip_b);
      p.ka = st.in<float>(3 * na, is2d), p.sga = st.in<double>(na, is2d), p.sgb = st.in<double>(nb, is2d);
      p.hp = st.in<double>(4 * na, !is2d);
    }
    const auto s_table = st.in<fe::VJob>(n_work);
    for (int j = 0; j < n_jobs; ++j) {
      const bool rays = plan[j].pre && jobs[j].kind == OKVIS_FE_MATCH_2D2D;
      plan[j].ra = st.scratch<double>(3 * (size_t)jobs[j].n_a, rays), plan[j].rb = st.scratch<double>(3 * (size_t)jobs[j].n_b, rays);
    }
    for (int j = 0; j < n_jobs; ++j) {
      const bool proj = plan[j].pre && jobs[j].kind == OKVIS_FE_MATCH_3D2D;
      const size_t na = (size_t)jobs[j].n_a;
      plan[j].uv = st.out<double>(2 * na, proj), plan[j].U = st.out<double>(4 * na, proj), plan[j].st = st.out<uint8_t>(na, proj);
    }
    s_lidx = st.out<int32_t>(rows * nbest), s_ldist = st.out<float>(rows * nbest);
    s_lchi = st.out<double>(rows * nbest), s_lfl = st.out<uint8_t>(rows * nbest);
    for (int j = 0; j < n_jobs; ++j) {
      const size_t nb = (size_t)jobs[j].n_b;
      plan[j].t_pairs = st.scratch<int32_t>(2 * nb, plan[j].tri), plan[j].t_sig = st.scratch<double>(nb, plan[j].tri);
    }
    for (int j = 0; j < n_jobs; ++j) {
      const size_t nb = (size_t)jobs[j].n_b;
      Plan& p = plan[j];
      p.t_hp = st.scratch<double>(4 * nb, p.tri), p.t_cov = st.scratch<double>(9 * nb, p.tri), p.t_fl = st.scratch<uint8_t>(nb, p.tri);
    }
    if (int rc = st.reserve()) return rc;
    fe::VJob* table = st.host(s_table);
    int32_t block0 = 0, row0 = 0, pre0 = 0;
    for (int j = 0; j < n_jobs; ++j) {
      const okvis_fe_vmatch_job& J = jobs[j];
      const Plan& p = plan[j];
      if (!p.pre) continue;
      const bool is2d = J.kind == OKVIS_FE_MATCH_2D2D;
      const size_t na = (size_t)J.n_a, nb = (size_t)J.n_b;
      st.put(p.da, J.desc_a), st.put(p.db, J.desc_b), st.put(p.kb, J.kp_b), st.put(p.sa, J.skip_a), st.put(p.sb, J.skip_b);
      st.put(p.ka, J.kp_a), st.put(p.hp, J.hp_W);
      fe::VJob D;
      std::memset(&D, 0, sizeof(D));
      D.desc_a = st.dev(p.da), D.desc_b = st.dev(p.db), D.kp_b = st.dev(p.kb), D.skip_a = st.dev(p.sa), D.skip_b = st.dev(p.sb);
      D.kp_a = st.dev(p.ka), D.sig_a = st.dev(p.sga), D.sig_b = st.dev(p.sgb), D.ray_a = st.dev(p.ra), D.ray_b = st.dev(p.rb);
      D.hp_W = st.dev(p.hp), D.uv = st.dev(p.uv), D.U = st.dev(p.U), D.status = st.dev(p.st);
      if (is2d) {
        double *sga = st.host(p.sga), *sgb = st.host(p.sgb);
        for (size_t k = 0; k < na; ++k) sga[k] = ray_sigma(J.kp_a[3 * k + 2], J.cam_a.intr[0]);
        for (size_t k = 0; k < nb; ++k) sgb[k] = ray_sigma(J.kp_b[3 * k + 2], J.cam_b.intr[0]);
        std::memcpy(D.T, J.T_AB, sizeof(D.T));
      } else {
        std::memcpy(D.T, J.T_CbW, sizeof(D.T));
        std::memcpy(D.P3, J.P3, sizeof(D.P3));
      }
      D.cam_a = to_device(&J.cam_a), D.cam_b = to_device(&J.cam_b);
      D.kind = J.kind, D.n_a = J.n_a, D.n_b = J.n_b, D.block0 = block0, D.row0 = row0, D.pre0 = pre0;
      *table++ = D;
      if (p.live) block0 += (J.n_a + fe::MATCH_WAVES - 1) / fe::MATCH_WAVES, row0 += J.n_a;
      pre0 += (int32_t)((na + (is2d ? nb : 0) + fe::VMATCH_PRE_THREADS - 1) / fe::VMATCH_PRE_THREADS);
    }
    if (int rc = st.upload()) return rc;
    hipLaunchKernelGGL(fe::vmatch_prepass_kernel, dim3((unsigned)pre_blocks), dim3(fe::VMATCH_PRE_THREADS), 0, c->stream,
                       (const fe::VJob*)st.dev(s_table), (int)n_work);
    FE_TRY(hipGetLastError());
    if (blocks > 0) {
      fe::VListParams P;
      P.jobs = st.dev(s_table), P.n_jobs = (int32_t)n_work;
      P.threshold = threshold, P.initial = use_ratio ? FLT_MAX : threshold, P.num_best = num_best;
      P.list_idx = st.dev(s_lidx), P.list_dist = st.dev(s_ldist), P.list_chi2 = st.dev(s_lchi), P.list_flags = st.dev(s_lfl);
      with_words(desc_bytes / 16, [&](auto w) {
        hipLaunchKernelGGL(fe::verified_lists_kernel<w()>, dim3((unsigned)blocks), dim3(fe::MATCH_THREADS), 0, c->stream, P);
      });
      FE_TRY(hipGetLastError());
    }
    if (int rc = st.download()) return rc;
  }
  // the assignment chains and matchBody's final loop on the host, as okvis_fe_match_descriptors; then what setBestMatch computes
  // again for the accepted pairs: 3D2D from the list entry, 2D2D through one launch of stereo_triangulate_kernel per job
  size_t row0 = 0, tri_lo = SIZE_MAX, tri_hi = 0, tri_out_lo = SIZE_MAX, tri_out_hi = 0;
  std::vector<int32_t> n_acc((size_t)n_jobs, 0);
  for (int j = 0; j < n_jobs; ++j) {
    const okvis_fe_vmatch_job& J = jobs[j];
    const Plan& p = plan[j];
    const bool is2d = J.kind == OKVIS_FE_MATCH_2D2D;
    const size_t na = (size_t)J.n_a, nb = (size_t)J.n_b;
    const auto zero = [](auto* dst, size_t n) { if (dst) std::fill_n(dst, n, 0); };
    zero(J.chi2, nb), zero(J.gate_flags, nb), zero(J.hp_a, 4 * nb), zero(J.cov, 9 * nb), zero(J.tri_flags, nb);
    if (p.st.on) st.get(p.st, J.proj_status), st.get(p.uv, J.uv), st.get(p.U, J.U);
    else zero(J.proj_status, na), zero(J.uv, 2 * na), zero(J.U, 4 * na);
    const int32_t* li = st.host(s_lidx) + row0 * nbest;
    const float* ld = st.host(s_ldist) + row0 * nbest;
    const double* lc = st.host(s_lchi) + row0 * nbest;
    const uint8_t* lf = st.host(s_lfl) + row0 * nbest;
    int32_t* t_pairs = st.host(p.t_pairs);
    double* t_sig = st.host(p.t_sig);
    assign_and_accept(J, li, ld, num_best, threshold, use_ratio, ratio_threshold, [&](int b, size_t o) {
      if (!is2d) {
        for (size_t k = 0; k < nbest; ++k)
          if (li[o + k] == b) {
            if (J.chi2) J.chi2[b] = lc[o + k];
            if (J.gate_flags) J.gate_flags[b] = lf[o + k];
            break;
          }
      } else if (p.tri) {
        const int32_t a = J.pair_a[b], i = n_acc[j]++;
        t_pairs[2 * i] = a, t_pairs[2 * i + 1] = b;
        t_sig[i] = std::fmax(ray_sigma(J.kp_a[3 * a + 2], J.cam_a.intr[0]), ray_sigma(J.kp_b[3 * b + 2], J.cam_b.intr[0]));
      }
    });
    if (p.live) row0 += na;
    if (n_acc[j] > 0) {
      tri_lo = std::min(tri_lo, p.t_pairs.off), tri_hi = std::max(tri_hi, p.t_sig.end());
      tri_out_lo = std::min(tri_out_lo, p.t_hp.off), tri_out_hi = std::max(tri_out_hi, p.t_fl.end());
    }
  }
  if (tri_hi > 0) {
    // by hand: a second copy in and a second copy back, over the jobs that accepted something
    FE_TRY(hipMemcpyAsync(c->d_stage + tri_lo, c->h_stage + tri_lo, tri_hi - tri_lo, hipMemcpyHostToDevice, c->stream));
    for (int j = 0; j < n_jobs; ++j) {
      if (n_acc[j] == 0) continue;
      const okvis_fe_vmatch_job& J = jobs[j];
      const Plan& p = plan[j];
      fe::TriParams P;
      std::memcpy(P.info6, p.info6, sizeof(P.info6));
      P.n_a = J.n_a, P.n_b = J.n_b, P.n_pairs = n_acc[j], P.want_uncertainty = 1;
      P.kp_a = st.dev(p.ka), P.kp_b = st.dev(p.kb), P.pairs = st.dev(p.t_pairs), P.sigma_ray = st.dev(p.t_sig);
      P.hp = st.dev(p.t_hp), P.cov = st.dev(p.t_cov), P.flags = st.dev(p.t_fl), P.gn = nullptr;
      if (int rc = launch_triangulate(c, P, &J.cam_a, &J.cam_b, J.T_AB, true)) return rc;
    }
    FE_TRY(hipMemcpyAsync(c->h_stage + tri_out_lo, c->d_stage + tri_out_lo, tri_out_hi - tri_out_lo, hipMemcpyDeviceToHost, c->stream));
    FE_TRY(hipStreamSynchronize(c->stream));
    for (int j = 0; j < n_jobs; ++j) {
      const okvis_fe_vmatch_job& J = jobs[j];
      const Plan& p = plan[j];
      const int32_t* t_pairs = st.host(p.t_pairs);
      for (int i = 0; i < n_acc[j]; ++i) {
        const size_t b = (size_t)t_pairs[2 * i + 1];
        if (J.hp_a) std::copy_n(st.host(p.t_hp) + 4 * i, 4, J.hp_a + 4 * b);
        if (J.cov) std::copy_n(st.host(p.t_cov) + 9 * i, 9, J.cov + 9 * b);
        if (J.tri_flags) J.tri_flags[b] = st.host(p.t_fl)[i];
      }
    }
  }
  return OKVIS_BA_OK;
}

int okvis_fe_bearing_vectors(okvis_fe_context* c, const okvis_fe_camera* cam, int32_t n, const float* kp, double* bearing,
                             double* sigma_angle, uint8_t* ok) {
  if (!c || !camera_ok(cam) || n < 0) return OKVIS_BA_ERR_ARG;
  if (n == 0) return OKVIS_BA_OK;
  if (!kp) return OKVIS_BA_ERR_ARG;
  fe::BearingParams P;
  P.cam = to_device(cam), P.n = n;
  FE_TRY(hipSetDevice(c->device));
  Stage st{c};
  const auto s_kp = st.in<float>(3 * (size_t)n);
  const auto s_b = st.out<double>(3 * (size_t)n), s_s = st.out<double>((size_t)n);
  const auto s_ok = st.out<uint8_t>((size_t)n);
  if (int rc = st.reserve()) return rc;
  st.put(s_kp, kp);
  if (int rc = st.upload()) return rc;
  P.kp = st.dev(s_kp), P.bearing = st.dev(s_b), P.sigma = st.dev(s_s), P.ok = st.dev(s_ok);
  hipLaunchKernelGGL(fe::bearing_vectors_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, P);
  FE_TRY(hipGetLastError());
  if (int rc = st.download()) return rc;
  st.get(s_b, bearing), st.get(s_s, sigma_angle), st.get(s_ok, ok);
  return OKVIS_BA_OK;
}

int okvis_fe_sac_consensus(okvis_fe_context* c, int32_t n_jobs, const okvis_fe_sac_job* jobs) {
  if (!c || n_jobs < 0 || (n_jobs > 0 && !jobs)) return OKVIS_BA_ERR_ARG;
  size_t blocks = 0, n_live = 0, n_counts = 0, n_words = 0;  // n_live: jobs with correspondences
  for (int j = 0; j < n_jobs; ++j) {
    const okvis_fe_sac_job& J = jobs[j];
    if (J.kind < OKVIS_FE_SAC_ABSOLUTE || J.kind > OKVIS_FE_SAC_RELATIVE || J.n < 0 || J.n > fe::SAC_MAX_N || J.n_models < 1 ||
        J.n_models > fe::SAC_MAX_MODELS || !J.models)
      return OKVIS_BA_ERR_ARG;
    if (J.kind == OKVIS_FE_SAC_ABSOLUTE) {
      if (J.n_cams < 1 || J.n_cams > fe::SAC_MAX_CAMS) return OKVIS_BA_ERR_ARG;
      if (J.n > 0 && (!J.points || !J.bearing || !J.sigma || !J.cam_index || !J.cam_offsets || !J.cam_rotations)) return OKVIS_BA_ERR_ARG;
      for (int i = 0; i < J.n; ++i)
        if (J.cam_index[i] < 0 || J.cam_index[i] >= J.n_cams) return OKVIS_BA_ERR_ARG;
    } else if (J.n > 0 && (!J.bearing1 || !J.bearing2 || !J.sigma1 || !J.sigma2)) {
      return OKVIS_BA_ERR_ARG;
    }
    if (J.n == 0) continue;
    const size_t tiles = ((size_t)J.n + fe::SAC_THREADS - 1) / fe::SAC_THREADS;
    ++n_live, blocks += tiles * (((size_t)J.n_models + fe::SAC_MODEL_TILE - 1) / fe::SAC_MODEL_TILE);
    n_counts += (size_t)J.n_models, n_words += (size_t)J.n_models * (((size_t)J.n + 63) / 64);
  }
  if (blocks > (size_t)INT32_MAX || n_counts > (size_t)INT32_MAX) return OKVIS_BA_ERR_ARG;
  Stage st{c};
  Staged<int32_t> s_counts;
  Staged<unsigned long long> s_ballots;
  struct Plan {
    Staged<double> models, a, b, s1, s2, cams, scores;
    Staged<int32_t> ci;
  };
  std::vector<Plan> plan((size_t)n_jobs);
  if (n_live > 0) {
    FE_TRY(hipSetDevice(c->device));
    for (int j = 0; j < n_jobs; ++j) {
      const okvis_fe_sac_job& J = jobs[j];
      if (J.n == 0) continue;
      Plan& p = plan[j];
      const size_t n = (size_t)J.n;
      const bool absolute = J.kind == OKVIS_FE_SAC_ABSOLUTE;
      p.models = st.in<double>((size_t)(J.kind == OKVIS_FE_SAC_ROTATION_ONLY ? 9 : 12) * J.n_models);
      p.a = st.in<double>(3 * n), p.b = st.in<double>(3 * n), p.s1 = st.in<double>(n), p.s2 = st.in<double>(n, !absolute);
      p.ci = st.in<int32_t>(n, absolute), p.cams = st.in<double>(12 * (size_t)J.n_cams, absolute);
    }
    const auto s_table = st.in<fe::SacJob>(n_live);
    s_counts = st.out<int32_t>(n_counts), s_ballots = st.out<unsigned long long>(n_words);
    for (int j = 0; j < n_jobs; ++j)  // a score matrix comes back only where a job asked for it
      plan[j].scores = st.out<double>((size_t)jobs[j].n_models * (size_t)jobs[j].n, jobs[j].n > 0 && jobs[j].scores);
    if (int rc = st.reserve()) return rc;
    fe::SacJob* table = st.host(s_table);
    size_t block0 = 0, count0 = 0, word0 = 0;
    for (int j = 0; j < n_jobs; ++j) {
      const okvis_fe_sac_job& J = jobs[j];
      if (J.n == 0) continue;
      const size_t n = (size_t)J.n;
      const bool absolute = J.kind == OKVIS_FE_SAC_ABSOLUTE;
      const Plan& p = plan[j];
      st.put(p.models, J.models);
      // by hand: the [n][3] arrays go to the device as [3][n], so that a wave reads 64 consecutive doubles
      const double *src_a = absolute ? J.points : J.bearing1, *src_b = absolute ? J.bearing : J.bearing2;
      double *dst_a = st.host(p.a), *dst_b = st.host(p.b);
      for (size_t i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k) dst_a[k * n + i] = src_a[3 * i + k], dst_b[k * n + i] = src_b[3 * i + k];
      st.put(p.s1, absolute ? J.sigma : J.sigma1), st.put(p.s2, J.sigma2), st.put(p.ci, J.cam_index);
      if (absolute) {
        double* cams = st.host(p.cams);
        for (int k = 0; k < J.n_cams; ++k) {
          std::copy_n(J.cam_offsets + 3 * k, 3, cams + 12 * k);
          std::copy_n(J.cam_rotations + 9 * k, 9, cams + 12 * k + 3);
        }
      }
      fe::SacJob D;
      D.models = st.dev(p.models), D.a = st.dev(p.a), D.b = st.dev(p.b), D.sigma1 = st.dev(p.s1), D.sigma2 = st.dev(p.s2);
      D.cam_index = st.dev(p.ci), D.cams = st.dev(p.cams), D.scores = st.dev(p.scores);
      D.threshold = J.threshold, D.kind = J.kind, D.n = J.n, D.n_models = J.n_models;
      D.block0 = (int32_t)block0, D.tiles = (int32_t)((n + fe::SAC_THREADS - 1) / fe::SAC_THREADS);
      D.count0 = (int32_t)count0, D.word0 = (int64_t)word0;
      *table++ = D;
      block0 += (size_t)D.tiles * (((size_t)J.n_models + fe::SAC_MODEL_TILE - 1) / fe::SAC_MODEL_TILE);
      count0 += (size_t)J.n_models, word0 += (size_t)J.n_models * ((n + 63) / 64);
    }
    if (int rc = st.upload()) return rc;
    FE_TRY(hipMemsetAsync(st.dev(s_counts), 0, s_counts.bytes(), c->stream));
    fe::SacParams P;
    P.jobs = st.dev(s_table), P.n_jobs = (int32_t)n_live;
    P.counts = st.dev(s_counts), P.ballots = st.dev(s_ballots);
    hipLaunchKernelGGL(fe::sac_consensus_kernel, dim3((unsigned)blocks), dim3(fe::SAC_THREADS), 0, c->stream, P);
    FE_TRY(hipGetLastError());
    if (int rc = st.download()) return rc;
  }
  // Ransac::computeModel's book-keeping on the counts (a hypothesis replaces the best only with strictly more inliers), and the
  // best hypothesis's row of ballot words expanded into indices
  size_t count0 = 0, word0 = 0;
  for (int j = 0; j < n_jobs; ++j) {
    const okvis_fe_sac_job& J = jobs[j];
    if (J.n == 0) {
      if (J.counts) std::fill_n(J.counts, J.n_models, 0);
      if (J.best) *J.best = 0;
      if (J.n_inliers) *J.n_inliers = 0;
      continue;
    }
    const size_t words = ((size_t)J.n + 63) / 64;
    const int32_t* counts = st.host(s_counts) + count0;
    const unsigned long long* ballots = st.host(s_ballots) + word0;
    count0 += (size_t)J.n_models, word0 += (size_t)J.n_models * words;
    int best = 0;
    for (int m = 1; m < J.n_models; ++m)
      if (counts[m] > counts[best]) best = m;
    if (J.counts) std::copy_n(counts, J.n_models, J.counts);
    if (J.best) *J.best = best;
    if (J.n_inliers) *J.n_inliers = counts[best];
    if (J.inliers) {
      int32_t k = 0;
      for (size_t w = 0; w < words; ++w)
        for (unsigned long long m = ballots[(size_t)best * words + w]; m; m &= m - 1) J.inliers[k++] = (int32_t)(64 * w) + __builtin_ctzll(m);
    }
    st.get(plan[j].scores, J.scores);
  }
  return OKVIS_BA_OK;
}

// The solvers in front of the consensus kernel: one staging copy in, sac_solve_kernel for all jobs, sac_consensus_kernel (as
// okvis_fe_sac_consensus launches it) on the hypotheses where the solver left them, one copy back.
int okvis_fe_sac_solve(okvis_fe_context* c, int32_t n_jobs, const okvis_fe_sac_solve_job* jobs) {
  if (!c || n_jobs < 0 || (n_jobs > 0 && !jobs)) return OKVIS_BA_ERR_ARG;
  if (n_jobs == 0) return OKVIS_BA_OK;
  size_t solve_blocks = 0, blocks = 0, n_scored = 0, n_counts = 0, n_words = 0;
  for (int j = 0; j < n_jobs; ++j) {
    const okvis_fe_sac_solve_job& J = jobs[j];
    if ((J.kind != OKVIS_FE_SAC_ROTATION_ONLY && J.kind != OKVIS_FE_SAC_RELATIVE) || J.n < 0 || J.n > fe::SAC_MAX_N || J.n_models < 1 ||
        J.n_models > fe::SAC_MAX_MODELS || !J.samples || (J.n > 0 && (!J.bearing1 || !J.bearing2)))
      return OKVIS_BA_ERR_ARG;
    const bool scored = J.counts || J.best || J.n_inliers || J.inliers || J.scores;
    if (scored && (!J.sigma1 || !J.sigma2)) return OKVIS_BA_ERR_ARG;
    const bool relative = J.kind == OKVIS_FE_SAC_RELATIVE;
    const size_t width = relative ? OKVIS_FE_SAC_SAMPLE_RELATIVE : OKVIS_FE_SAC_SAMPLE_ROTATION_ONLY;
    for (size_t i = 0; i < width * (size_t)J.n_models; ++i)
      if (J.samples[i] < 0 || J.samples[i] >= J.n) return OKVIS_BA_ERR_ARG;  // n = 0 ends here: every job past this line has n >= 1
    solve_blocks += relative ? (size_t)J.n_models : ((size_t)J.n_models + 63) / 64;
    if (!scored) continue;
    const size_t tiles = ((size_t)J.n + fe::SAC_THREADS - 1) / fe::SAC_THREADS;
    ++n_scored, blocks += tiles * (((size_t)J.n_models + fe::SAC_MODEL_TILE - 1) / fe::SAC_MODEL_TILE);
    n_counts += (size_t)J.n_models, n_words += (size_t)J.n_models * (((size_t)J.n + 63) / 64);
  }
  if (solve_blocks > (size_t)INT32_MAX || blocks > (size_t)INT32_MAX || n_counts > (size_t)INT32_MAX) return OKVIS_BA_ERR_ARG;
  FE_TRY(hipSetDevice(c->device));
  Stage st{c};
  struct Plan {
    Staged<double> a, b, s1, s2, models, essentials, scores;
    Staged<int32_t> samples, n_roots;
    Staged<uint8_t> valid;
    bool scored = false;
  };
  std::vector<Plan> plan((size_t)n_jobs);
  for (int j = 0; j < n_jobs; ++j) {
    const okvis_fe_sac_solve_job& J = jobs[j];
    Plan& p = plan[j];
    const size_t n = (size_t)J.n;
    p.scored = J.counts || J.best || J.n_inliers || J.inliers || J.scores;
    p.a = st.in<double>(3 * n), p.b = st.in<double>(3 * n);
    p.s1 = st.in<double>(n, J.sigma1 != nullptr), p.s2 = st.in<double>(n, J.sigma2 != nullptr);
    p.samples = st.in<int32_t>((size_t)J.n_models * (J.kind == OKVIS_FE_SAC_RELATIVE ? 8 : 2));
  }
  const auto s_solve = st.in<fe::SolveJob>((size_t)n_jobs);
  const auto s_table = st.in<fe::SacJob>(n_scored, n_scored > 0);
  const auto model_doubles = [&](int j) { return (size_t)jobs[j].n_models * (jobs[j].kind == OKVIS_FE_SAC_RELATIVE ? 12 : 9); };
  for (int j = 0; j < n_jobs; ++j)  // hypotheses the caller does not take stay on the device
    if (!jobs[j].models) plan[j].models = st.scratch<double>(model_doubles(j));
  for (int j = 0; j < n_jobs; ++j) {
    const okvis_fe_sac_solve_job& J = jobs[j];
    const bool relative = J.kind == OKVIS_FE_SAC_RELATIVE;
    if (J.models) plan[j].models = st.out<double>(model_doubles(j));
    plan[j].valid = st.out<uint8_t>((size_t)J.n_models, J.valid != nullptr);
    plan[j].n_roots = st.out<int32_t>((size_t)J.n_models, relative && J.n_roots);
    plan[j].essentials = st.out<double>(90 * (size_t)J.n_models, relative && J.essentials);
  }
  const auto s_counts = st.out<int32_t>(n_counts, n_scored > 0);
  const auto s_ballots = st.out<unsigned long long>(n_words, n_scored > 0);
  for (int j = 0; j < n_jobs; ++j) plan[j].scores = st.out<double>((size_t)jobs[j].n_models * (size_t)jobs[j].n, jobs[j].scores != nullptr);
  if (int rc = st.reserve()) return rc;
  fe::SolveJob* solve_table = st.host(s_solve);
  fe::SacJob* table = st.host(s_table);
  size_t solve_block0 = 0, block0 = 0, count0 = 0, word0 = 0;
  for (int j = 0; j < n_jobs; ++j) {
    const okvis_fe_sac_solve_job& J = jobs[j];
    const Plan& p = plan[j];
    const size_t n = (size_t)J.n;
    const bool relative = J.kind == OKVIS_FE_SAC_RELATIVE;
    double *dst_a = st.host(p.a), *dst_b = st.host(p.b);  // [n][3] -> [3][n], as the consensus kernel reads them
    for (size_t i = 0; i < n; ++i)
      for (int k = 0; k < 3; ++k) dst_a[k * n + i] = J.bearing1[3 * i + k], dst_b[k * n + i] = J.bearing2[3 * i + k];
    st.put(p.s1, J.sigma1), st.put(p.s2, J.sigma2), st.put(p.samples, J.samples);
    fe::SolveJob S;
    S.a = st.dev(p.a), S.b = st.dev(p.b), S.sigma1 = st.dev(p.s1), S.sigma2 = st.dev(p.s2), S.samples = st.dev(p.samples);
    S.models = st.dev(p.models), S.valid = st.dev(p.valid), S.n_roots = st.dev(p.n_roots), S.essentials = st.dev(p.essentials);
    S.kind = J.kind, S.n = J.n, S.n_models = J.n_models, S.block0 = (int32_t)solve_block0;
    solve_table[j] = S;
    solve_block0 += relative ? (size_t)J.n_models : ((size_t)J.n_models + 63) / 64;
    if (!p.scored) continue;
    fe::SacJob D;
    D.models = st.dev(p.models), D.a = st.dev(p.a), D.b = st.dev(p.b), D.sigma1 = st.dev(p.s1), D.sigma2 = st.dev(p.s2);
    D.cam_index = nullptr, D.cams = nullptr, D.scores = st.dev(p.scores);
    D.threshold = J.threshold, D.kind = J.kind, D.n = J.n, D.n_models = J.n_models;
    D.block0 = (int32_t)block0, D.tiles = (int32_t)((n + fe::SAC_THREADS - 1) / fe::SAC_THREADS);
    D.count0 = (int32_t)count0, D.word0 = (int64_t)word0;
    *table++ = D;
    block0 += (size_t)D.tiles * (((size_t)J.n_models + fe::SAC_MODEL_TILE - 1) / fe::SAC_MODEL_TILE);
    count0 += (size_t)J.n_models, word0 += (size_t)J.n_models * ((n + 63) / 64);
  }
  if (int rc = st.upload()) return rc;
  // essentials past n_roots are not written by the kernel: NaN, so that the copy back never hands out stale staging bytes
  for (int j = 0; j < n_jobs; ++j)
    if (plan[j].essentials.on) FE_TRY(hipMemsetAsync(st.dev(plan[j].essentials), 0xff, plan[j].essentials.bytes(), c->stream));
  fe::SolveParams SP;
  SP.jobs = st.dev(s_solve), SP.n_jobs = n_jobs;
  hipLaunchKernelGGL(fe::sac_solve_kernel, dim3((unsigned)solve_blocks), dim3(64), 0, c->stream, SP);
  FE_TRY(hipGetLastError());
  if (n_scored > 0) {
    FE_TRY(hipMemsetAsync(st.dev(s_counts), 0, s_counts.bytes(), c->stream));
    fe::SacParams P;
    P.jobs = st.dev(s_table), P.n_jobs = (int32_t)n_scored;
    P.counts = st.dev(s_counts), P.ballots = st.dev(s_ballots);
    hipLaunchKernelGGL(fe::sac_consensus_kernel, dim3((unsigned)blocks), dim3(fe::SAC_THREADS), 0, c->stream, P);
    FE_TRY(hipGetLastError());
  }
  if (int rc = st.download()) return rc;
  count0 = word0 = 0;
  for (int j = 0; j < n_jobs; ++j) {
    const okvis_fe_sac_solve_job& J = jobs[j];
    const Plan& p = plan[j];
    if (J.models) st.get(p.models, J.models);
    st.get(p.valid, J.valid), st.get(p.n_roots, J.n_roots), st.get(p.essentials, J.essentials);
    if (!p.scored) continue;
    // Ransac::computeModel's book-keeping, as in okvis_fe_sac_consensus
    const size_t words = ((size_t)J.n + 63) / 64;
    const int32_t* counts = st.host(s_counts) + count0;
    const unsigned long long* ballots = st.host(s_ballots) + word0;
    count0 += (size_t)J.n_models, word0 += (size_t)J.n_models * words;
    int best = 0;
    for (int m = 1; m < J.n_models; ++m)
      if (counts[m] > counts[best]) best = m;
    if (J.counts) std::copy_n(counts, J.n_models, J.counts);
    if (J.best) *J.best = best;
    if (J.n_inliers) *J.n_inliers = counts[best];
    if (J.inliers) {
      int32_t k = 0;
      for (size_t w = 0; w < words; ++w)
        for (unsigned long long m = ballots[(size_t)best * words + w]; m; m &= m - 1) J.inliers[k++] = (int32_t)(64 * w) + __builtin_ctzll(m);
    }
    st.get(p.scores, J.scores);
  }
  return OKVIS_BA_OK;
}

int okvis_fe_imu_propagate(okvis_fe_context* c, int32_t n_params, const okvis_ba_imu_params* params, int32_t n_samples,
                           const int64_t* s_t, const double* s_gyr, const double* s_acc, int32_t n_ends, const int64_t* ends,
                           int32_t n_jobs, const okvis_fe_imu_job* jobs, double* T_WS, double* sb, double* cov, double* jac,
                           int32_t* count) {
  if (!c || n_params < 0 || n_samples < 0 || n_ends < 0 || n_jobs < 0) return OKVIS_BA_ERR_ARG;
  if (n_jobs == 0) return OKVIS_BA_OK;
  if (!jobs || !params || !ends || !T_WS || !sb || !count || (n_samples > 0 && (!s_t || !s_gyr || !s_acc))) return OKVIS_BA_ERR_ARG;
  // every check before anything is enqueued; the outputs are packed in job order: rows = calls, n_cov / n_jac = those that ask
  size_t rows = 0, n_cov = 0, n_jac = 0;
  for (int j = 0; j < n_jobs; ++j) {
    const okvis_fe_imu_job& J = jobs[j];
    if (J.s_begin < 0 || J.s_count < 0 || (int64_t)J.s_begin + J.s_count > n_samples) return OKVIS_BA_ERR_ARG;
    if (J.e_begin < 0 || J.e_count < 1 || (int64_t)J.e_begin + J.e_count > n_ends) return OKVIS_BA_ERR_ARG;
    if (J.prm < 0 || J.prm >= n_params || (J.flags & ~(OKVIS_FE_IMU_COV | OKVIS_FE_IMU_JAC))) return OKVIS_BA_ERR_ARG;
    if (((J.flags & OKVIS_FE_IMU_COV) && !cov) || ((J.flags & OKVIS_FE_IMU_JAC) && !jac)) return OKVIS_BA_ERR_ARG;
    for (int i = 1; i < J.s_count; ++i)
      if (!(s_t[J.s_begin + i - 1] < s_t[J.s_begin + i])) return OKVIS_BA_ERR_ARG;
    if (J.s_count >= 2 && s_t[J.s_begin] > J.t_start) return OKVIS_BA_ERR_ARG;  // ImuError.cpp:300
    int64_t before = J.t_start;
    for (int k = 0; k < J.e_count; ++k) {
      if (ends[J.e_begin + k] < before) return OKVIS_BA_ERR_ARG;
      before = ends[J.e_begin + k];
    }
    rows += (size_t)J.e_count;
    if (J.flags & OKVIS_FE_IMU_COV) n_cov += (size_t)J.e_count;
    if (J.flags & OKVIS_FE_IMU_JAC) n_jac += (size_t)J.e_count;
  }
  if (rows > (size_t)INT32_MAX) return OKVIS_BA_ERR_ARG;
  FE_TRY(hipSetDevice(c->device));
  Stage st{c};
  const auto s_prm = st.in<okvis_ba_imu_params>((size_t)n_params);
  const auto s_ts = st.in<long long>((size_t)n_samples);
  const auto s_g = st.in<double>(3 * (size_t)n_samples), s_a = st.in<double>(3 * (size_t)n_samples);
  const auto s_ends = st.in<long long>((size_t)n_ends);
  const auto s_table = st.in<fe::PropJob>((size_t)n_jobs);
  const auto s_T = st.out<double>(7 * rows), s_sb = st.out<double>(9 * rows);
  const auto s_cnt = st.out<int32_t>(rows);
  const auto s_cov = st.out<double>(225 * n_cov, n_cov > 0), s_jac = st.out<double>(225 * n_jac, n_jac > 0);
  if (int rc = st.reserve()) return rc;
  static_assert(sizeof(long long) == sizeof(int64_t), "the stamps are copied as they are");
  st.put(s_prm, params), st.put(s_g, s_gyr), st.put(s_a, s_acc);
  st.put(s_ts, reinterpret_cast<const long long*>(s_t)), st.put(s_ends, reinterpret_cast<const long long*>(ends));
  fe::PropJob* table = st.host(s_table);
  size_t row0 = 0, cov0 = 0, jac0 = 0;
  for (int j = 0; j < n_jobs; ++j) {
    const okvis_fe_imu_job& J = jobs[j];
    fe::PropJob D;
    D.job = J, D.row0 = (int32_t)row0, D.cov0 = (int32_t)cov0, D.jac0 = (int32_t)jac0, D.reserved = 0;
    table[j] = D;
    row0 += (size_t)J.e_count;
    if (J.flags & OKVIS_FE_IMU_COV) cov0 += (size_t)J.e_count;
    if (J.flags & OKVIS_FE_IMU_JAC) jac0 += (size_t)J.e_count;
  }
  if (int rc = st.upload()) return rc;
  fe::PropParams P;
  P.params = st.dev(s_prm), P.s_t = st.dev(s_ts), P.s_gyr = st.dev(s_g), P.s_acc = st.dev(s_a), P.ends = st.dev(s_ends);
  P.jobs = st.dev(s_table), P.n_jobs = n_jobs;
  P.T_WS = st.dev(s_T), P.sb = st.dev(s_sb), P.count = st.dev(s_cnt), P.cov = st.dev(s_cov), P.jac = st.dev(s_jac);
  hipLaunchKernelGGL(fe::imu_propagate_kernel, dim3((unsigned)((n_jobs + fe::PROP_WAVES - 1) / fe::PROP_WAVES)), dim3(fe::PROP_THREADS),
                     0, c->stream, P);
  FE_TRY(hipGetLastError());
  if (int rc = st.download()) return rc;
  // by hand: the packed rows go to the ends' places in the pool; a call that returned early (count -1, or a deque of fewer than two samples) wrote no covariance and no Jacobian
  const double *h_T = st.host(s_T), *h_sb = st.host(s_sb), *h_cov = st.host(s_cov), *h_jac = st.host(s_jac);
  const int32_t* h_cnt = st.host(s_cnt);
  for (int j = 0; j < n_jobs; ++j) {
    const fe::PropJob& D = table[j];
    const size_t e0 = (size_t)D.job.e_begin, n = (size_t)D.job.e_count;
    std::copy_n(h_T + 7 * (size_t)D.row0, 7 * n, T_WS + 7 * e0);
    std::copy_n(h_sb + 9 * (size_t)D.row0, 9 * n, sb + 9 * e0);
    std::copy_n(h_cnt + D.row0, n, count + e0);
    for (size_t k = 0; k < n; ++k) {
      if (h_cnt[D.row0 + k] < 0 || D.job.s_count < 2) continue;
      if (D.job.flags & OKVIS_FE_IMU_COV) std::copy_n(h_cov + 225 * ((size_t)D.cov0 + k), 225, cov + 225 * (e0 + k));
      if (D.job.flags & OKVIS_FE_IMU_JAC) std::copy_n(h_jac + 225 * ((size_t)D.jac0 + k), 225, jac + 225 * (e0 + k));
    }
  }
  return OKVIS_BA_OK;
}

int okvis_fe_keyframe_decision(okvis_fe_context* c, int32_t n_kp, const float* kp, const uint8_t* matched, int32_t n_images,
                               const okvis_fe_kf_image* images, int32_t n_jobs, const okvis_fe_kf_job* jobs, uint8_t* decision,
                               double* overlap, double* ratio, int32_t* n_matched, int32_t* hull_all_size, int32_t* hull_matched_size,
                               double* area_all, double* area_matched, int32_t* n_inside, uint8_t* flags, int32_t* hull_all,
                               int32_t* hull_matched) {
  if (!c || n_kp < 0 || n_images < 0 || n_jobs < 0) return OKVIS_BA_ERR_ARG;
  if ((n_jobs > 0 && !jobs) || (n_images > 0 && !images) || (n_kp > 0 && (!kp || !matched))) return OKVIS_BA_ERR_ARG;
  // every check before anything is enqueued
  size_t n_hull = 0;
  int32_t n_max = 0;
  for (int i = 0; i < n_images; ++i) {
    const okvis_fe_kf_image& I = images[i];
    if (I.kp_begin < 0 || I.kp_count < 0 || I.kp_count > fe::KF_MAX_KEYPOINTS || (int64_t)I.kp_begin + I.kp_count > n_kp) return OKVIS_BA_ERR_ARG;
    for (int k = I.kp_begin; k < I.kp_begin + I.kp_count; ++k)
      if (!std::isfinite(kp[3 * (size_t)k]) || !std::isfinite(kp[3 * (size_t)k + 1])) return OKVIS_BA_ERR_ARG;
    n_hull += (size_t)I.kp_count;
    n_max = std::max(n_max, I.kp_count);
  }
  if (n_hull > (size_t)INT32_MAX) return OKVIS_BA_ERR_ARG;
  for (int j = 0; j < n_jobs; ++j) {
    const okvis_fe_kf_job& J = jobs[j];
    if (J.n_cams < 1 || J.n_cams > fe::KF_MAX_CAMS || J.im_begin < 0 || (int64_t)J.im_begin + J.n_cams > n_images || J.num_frames < 0)
      return OKVIS_BA_ERR_ARG;
  }
  if (n_images == 0) return OKVIS_BA_OK;  // then there is no job either
  FE_TRY(hipSetDevice(c->device));
  Stage st{c};
  const auto s_xy = st.in<fe::KfPoint>((size_t)n_kp);
  const auto s_m = st.in<uint8_t>((size_t)n_kp);
  const auto s_table = st.in<fe::KfImage>((size_t)n_images);
  const bool want_hulls = hull_all || hull_matched;
  // the hull lists are the kernel's working memory; they come back only where a referee asks for them
  const auto s_ha_tmp = st.scratch<int32_t>(n_hull, !want_hulls), s_hm_tmp = st.scratch<int32_t>(n_hull, !want_hulls);
  const auto s_rec = st.out<fe::KfRecord>((size_t)n_images);
  const auto s_ha = want_hulls ? st.out<int32_t>(n_hull) : s_ha_tmp, s_hm = want_hulls ? st.out<int32_t>(n_hull) : s_hm_tmp;
  if (int rc = st.reserve()) return rc;
  // by hand: the size column stays behind
  fe::KfPoint* xy = st.host(s_xy);
  for (size_t k = 0; k < (size_t)n_kp; ++k) xy[k].x = kp[3 * k], xy[k].y = kp[3 * k + 1];
  if (n_kp > 0) st.put(s_m, matched);
  fe::KfImage* table = st.host(s_table);
  size_t hull0 = 0;
  for (int i = 0; i < n_images; ++i) {
    table[i] = fe::KfImage{images[i].kp_begin, images[i].kp_count, (int32_t)hull0, 0};
    hull0 += (size_t)images[i].kp_count;
  }
  if (int rc = st.upload()) return rc;
  fe::KfParams P;
  P.xy = st.dev(s_xy), P.matched = st.dev(s_m), P.images = st.dev(s_table), P.rec = st.dev(s_rec);
  P.hull_all = st.dev(s_ha), P.hull_matched = st.dev(s_hm);
  hipLaunchKernelGGL(fe::keyframe_kernel, dim3((unsigned)n_images), dim3(fe::KF_THREADS), sizeof(fe::KfPoint) * (size_t)n_max, c->stream, P);
  FE_TRY(hipGetLastError());
  if (int rc = st.download()) return rc;
  const fe::KfRecord* rec = st.host(s_rec);
  for (int i = 0; i < n_images; ++i) {
    const fe::KfRecord& R = rec[i];
    if (n_matched) n_matched[i] = R.n_matched;
    if (hull_all_size) hull_all_size[i] = R.hull_all_size;
    if (hull_matched_size) hull_matched_size[i] = R.hull_matched_size;
    if (area_all) area_all[i] = R.area_all;
    if (area_matched) area_matched[i] = R.area_matched;
    if (n_inside) n_inside[i] = R.n_inside;
    if (flags) flags[i] = (uint8_t)R.flags;
    const size_t at = (size_t)table[i].hull0, n = (size_t)table[i].n;
    if (hull_all) {
      std::copy_n(st.host(s_ha) + at, (size_t)R.hull_all_size, hull_all + at);
      std::fill(hull_all + at + R.hull_all_size, hull_all + at + n, -1);
    }
    if (hull_matched) {
      std::copy_n(st.host(s_hm) + at, (size_t)R.hull_matched_size, hull_matched + at);
      std::fill(hull_matched + at + R.hull_matched_size, hull_matched + at + n, -1);
    }
  }
  // Frontend.cpp:307-368 per job, from the records of its images
  for (int j = 0; j < n_jobs; ++j) {
    const okvis_fe_kf_job& J = jobs[j];
    double o, r;
    const int d = fe::kf_fold(rec + J.im_begin, J.n_cams, J.num_frames, J.initialized, J.overlap_threshold, J.ratio_threshold, &o, &r);
    if (decision) decision[j] = (uint8_t)d;
    if (overlap) overlap[j] = o;
    if (ratio) ratio[j] = r;
  }
  return OKVIS_BA_OK;
}

}  // extern "C"
