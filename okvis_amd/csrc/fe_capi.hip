// C-ABI of the batched frontend pieces (include/okvis_amd_frontend.h).  Host buffers in and out: the inputs of one call are
// packed into one pinned staging block and go to the device with one copy, one kernel runs, the outputs come back with one
// copy.  No CPU path: every entry fails with OKVIS_BA_ERR_NO_DEVICE / a HIP status when there is no GPU.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cfloat>
#include <cmath>
#include <cstdlib>
#include <cstring>
#include <new>
#include <vector>

#include "fe_kernels.hpp"
#include "fe_match.hpp"
#include "fe_sac.hpp"
#include "fe_vmatch.hpp"

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

// sequential layout of the staging block, every array aligned to 16 bytes
struct Layout {
  size_t size = 0;
  size_t add(size_t bytes) {
    const size_t o = size;
    size += (bytes + 15) & ~(size_t)15;
    return o;
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

template <bool WRITE>
void launch_hamming_rows(int words, const fe::CandParams& P, hipStream_t stream) {
  const dim3 grid((P.n_a + fe::MATCH_WAVES - 1) / fe::MATCH_WAVES), block(fe::MATCH_THREADS);
  switch (words) {
    case 1: hipLaunchKernelGGL((fe::hamming_rows_kernel<1, WRITE>), grid, block, 0, stream, P); break;
    case 2: hipLaunchKernelGGL((fe::hamming_rows_kernel<2, WRITE>), grid, block, 0, stream, P); break;
    case 3: hipLaunchKernelGGL((fe::hamming_rows_kernel<3, WRITE>), grid, block, 0, stream, P); break;
    default: hipLaunchKernelGGL((fe::hamming_rows_kernel<4, WRITE>), grid, block, 0, stream, P); break;
  }
}

void launch_best_lists(int words, int blocks, const fe::BestParams& P, hipStream_t stream) {
  const dim3 grid(blocks), block(fe::MATCH_THREADS);
  switch (words) {
    case 1: hipLaunchKernelGGL(fe::best_lists_kernel<1>, grid, block, 0, stream, P); break;
    case 2: hipLaunchKernelGGL(fe::best_lists_kernel<2>, grid, block, 0, stream, P); break;
    case 3: hipLaunchKernelGGL(fe::best_lists_kernel<3>, grid, block, 0, stream, P); break;
    default: hipLaunchKernelGGL(fe::best_lists_kernel<4>, grid, block, 0, stream, P); break;
  }
}

void launch_verified_lists(int words, int blocks, const fe::VListParams& P, hipStream_t stream) {
  const dim3 grid(blocks), block(fe::MATCH_THREADS);
  switch (words) {
    case 1: hipLaunchKernelGGL(fe::verified_lists_kernel<1>, grid, block, 0, stream, P); break;
    case 2: hipLaunchKernelGGL(fe::verified_lists_kernel<2>, grid, block, 0, stream, P); break;
    case 3: hipLaunchKernelGGL(fe::verified_lists_kernel<3>, grid, block, 0, stream, P); break;
    default: hipLaunchKernelGGL(fe::verified_lists_kernel<4>, grid, block, 0, stream, P); break;
  }
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
  if (!kp_a || !kp_b || !pairs || n_a == 0 || n_b == 0) return OKVIS_BA_ERR_ARG;
  for (int i = 0; i < n_pairs; ++i)
    if (pairs[2 * i] < 0 || pairs[2 * i] >= n_a || pairs[2 * i + 1] < 0 || pairs[2 * i + 1] >= n_b) return OKVIS_BA_ERR_ARG;
  fe::TriParams P;
  P.cam_a = to_device(cam_a), P.cam_b = to_device(cam_b);
  std::memcpy(P.T_AB, T_AB, sizeof(P.T_AB));
  if (!spd_inverse6(UOplus, P.info6)) return OKVIS_BA_ERR_NUMERIC;
  P.sigma_ray_own = 0.5 / std::fmin(cam_a->intr[0], cam_b->intr[0]);
  P.n_a = n_a, P.n_b = n_b, P.n_pairs = n_pairs, P.want_uncertainty = want_uncertainty;
  FE_TRY(hipSetDevice(c->device));
  Layout in, all;
  const size_t o_ka = in.add(sizeof(float) * 3 * n_a), o_kb = in.add(sizeof(float) * 3 * n_b);
  const size_t o_pairs = in.add(sizeof(int32_t) * 2 * n_pairs), o_sig = sigma_ray ? in.add(sizeof(double) * n_pairs) : 0;
  all = in;
  const size_t o_hp = all.add(sizeof(double) * 4 * n_pairs), o_cov = all.add(sizeof(double) * 9 * n_pairs);
  const size_t o_fl = all.add(n_pairs);
  const size_t o_gn = gn ? all.add(sizeof(double) * 81 * n_pairs) : 0;
  if (int rc = reserve(c, all.size)) return rc;
  std::memcpy(c->h_stage + o_ka, kp_a, sizeof(float) * 3 * n_a);
  std::memcpy(c->h_stage + o_kb, kp_b, sizeof(float) * 3 * n_b);
  std::memcpy(c->h_stage + o_pairs, pairs, sizeof(int32_t) * 2 * n_pairs);
  if (sigma_ray) std::memcpy(c->h_stage + o_sig, sigma_ray, sizeof(double) * n_pairs);
  FE_TRY(hipMemcpyAsync(c->d_stage, c->h_stage, in.size, hipMemcpyHostToDevice, c->stream));
  if (cov) FE_TRY(hipMemsetAsync(c->d_stage + o_cov, 0, sizeof(double) * 9 * n_pairs, c->stream));
  if (gn) FE_TRY(hipMemsetAsync(c->d_stage + o_gn, 0, sizeof(double) * 81 * n_pairs, c->stream));
  P.gn = gn ? (double*)(c->d_stage + o_gn) : nullptr;
  P.kp_a = (const float*)(c->d_stage + o_ka), P.kp_b = (const float*)(c->d_stage + o_kb);
  P.pairs = (const int32_t*)(c->d_stage + o_pairs);
  P.sigma_ray = sigma_ray ? (const double*)(c->d_stage + o_sig) : nullptr;
  P.hp = (double*)(c->d_stage + o_hp), P.cov = (double*)(c->d_stage + o_cov), P.flags = (uint8_t*)(c->d_stage + o_fl);
  hipLaunchKernelGGL(fe::stereo_triangulate_kernel, dim3((n_pairs + fe::TRI_THREADS - 1) / fe::TRI_THREADS), dim3(fe::TRI_THREADS),
                     0, c->stream, P);
  FE_TRY(hipGetLastError());
  FE_TRY(hipMemcpyAsync(c->h_stage + o_hp, c->d_stage + o_hp, all.size - o_hp, hipMemcpyDeviceToHost, c->stream));
  FE_TRY(hipStreamSynchronize(c->stream));
  if (hp_a) std::memcpy(hp_a, c->h_stage + o_hp, sizeof(double) * 4 * n_pairs);
  if (cov) std::memcpy(cov, c->h_stage + o_cov, sizeof(double) * 9 * n_pairs);
  if (flags) std::memcpy(flags, c->h_stage + o_fl, n_pairs);
  if (gn) std::memcpy(gn, c->h_stage + o_gn, sizeof(double) * 81 * n_pairs);
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
  Layout in, all;
  const size_t o_hp = in.add(sizeof(double) * 4 * n);
  all = in;
  const size_t o_uv = all.add(sizeof(double) * 2 * n), o_U = all.add(sizeof(double) * 4 * n), o_st = all.add(n);
  if (int rc = reserve(c, all.size)) return rc;
  std::memcpy(c->h_stage + o_hp, hp_W, sizeof(double) * 4 * n);
  FE_TRY(hipMemcpyAsync(c->d_stage, c->h_stage, in.size, hipMemcpyHostToDevice, c->stream));
  P.hp_W = (const double*)(c->d_stage + o_hp);
  P.uv = (double*)(c->d_stage + o_uv), P.U = (double*)(c->d_stage + o_U), P.status = (uint8_t*)(c->d_stage + o_st);
  hipLaunchKernelGGL(fe::project_landmarks_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, P);
  FE_TRY(hipGetLastError());
  FE_TRY(hipMemcpyAsync(c->h_stage + o_uv, c->d_stage + o_uv, all.size - o_uv, hipMemcpyDeviceToHost, c->stream));
  FE_TRY(hipStreamSynchronize(c->stream));
  if (uv) std::memcpy(uv, c->h_stage + o_uv, sizeof(double) * 2 * n);
  if (U) std::memcpy(U, c->h_stage + o_U, sizeof(double) * 4 * n);
  if (status) std::memcpy(status, c->h_stage + o_st, n);
  return OKVIS_BA_OK;
}

int okvis_fe_gate_3d2d(okvis_fe_context* c, int32_t n_proj, const double* uv, const double* U, int32_t n_b, const float* kp_b,
                       int32_t n_pairs, const int32_t* pairs, double* chi2, uint8_t* flags) {
  if (!c || n_proj < 0 || n_b < 0 || n_pairs < 0) return OKVIS_BA_ERR_ARG;
  if (n_pairs == 0) return OKVIS_BA_OK;
  if (!uv || !U || !kp_b || !pairs || n_proj == 0 || n_b == 0) return OKVIS_BA_ERR_ARG;
  for (int i = 0; i < n_pairs; ++i)
    if (pairs[2 * i] < 0 || pairs[2 * i] >= n_proj || pairs[2 * i + 1] < 0 || pairs[2 * i + 1] >= n_b) return OKVIS_BA_ERR_ARG;
  fe::GateParams P;
  P.n_proj = n_proj, P.n_b = n_b, P.n_pairs = n_pairs;
  FE_TRY(hipSetDevice(c->device));
  Layout in, all;
  const size_t o_uv = in.add(sizeof(double) * 2 * n_proj), o_U = in.add(sizeof(double) * 4 * n_proj);
  const size_t o_kb = in.add(sizeof(float) * 3 * n_b), o_pairs = in.add(sizeof(int32_t) * 2 * n_pairs);
  all = in;
  const size_t o_chi = all.add(sizeof(double) * n_pairs), o_fl = all.add(n_pairs);
  if (int rc = reserve(c, all.size)) return rc;
  std::memcpy(c->h_stage + o_uv, uv, sizeof(double) * 2 * n_proj);
  std::memcpy(c->h_stage + o_U, U, sizeof(double) * 4 * n_proj);
  std::memcpy(c->h_stage + o_kb, kp_b, sizeof(float) * 3 * n_b);
  std::memcpy(c->h_stage + o_pairs, pairs, sizeof(int32_t) * 2 * n_pairs);
  FE_TRY(hipMemcpyAsync(c->d_stage, c->h_stage, in.size, hipMemcpyHostToDevice, c->stream));
  P.uv = (const double*)(c->d_stage + o_uv), P.U = (const double*)(c->d_stage + o_U);
  P.kp_b = (const float*)(c->d_stage + o_kb), P.pairs = (const int32_t*)(c->d_stage + o_pairs);
  P.chi2 = (double*)(c->d_stage + o_chi), P.flags = (uint8_t*)(c->d_stage + o_fl);
  hipLaunchKernelGGL(fe::gate_3d2d_kernel, dim3((n_pairs + 255) / 256), dim3(256), 0, c->stream, P);
  FE_TRY(hipGetLastError());
  FE_TRY(hipMemcpyAsync(c->h_stage + o_chi, c->d_stage + o_chi, all.size - o_chi, hipMemcpyDeviceToHost, c->stream));
  FE_TRY(hipStreamSynchronize(c->stream));
  if (chi2) std::memcpy(chi2, c->h_stage + o_chi, sizeof(double) * n_pairs);
  if (flags) std::memcpy(flags, c->h_stage + o_fl, n_pairs);
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
  Layout in, all;
  const size_t o_da = in.add(db * na), o_db = in.add(db * nb);
  const size_t o_sa = skip_a ? in.add(na) : 0, o_sb = skip_b ? in.add(nb) : 0;
  all = in;
  const size_t o_cnt = all.add(sizeof(int32_t) * na), o_off = all.add(sizeof(unsigned long long) * na);
  const size_t o_tot = all.add(sizeof(unsigned long long)), o_pairs = all.add(sizeof(int32_t) * 2 * cap), o_dist = all.add(sizeof(float) * cap);
  if (int rc = reserve(c, all.size)) return rc;
  std::memcpy(c->h_stage + o_da, desc_a, db * na);
  std::memcpy(c->h_stage + o_db, desc_b, db * nb);
  if (skip_a) std::memcpy(c->h_stage + o_sa, skip_a, na);
  if (skip_b) std::memcpy(c->h_stage + o_sb, skip_b, nb);
  FE_TRY(hipMemcpyAsync(c->d_stage, c->h_stage, in.size, hipMemcpyHostToDevice, c->stream));
  fe::CandParams P;
  P.desc_a = (const uint8_t*)(c->d_stage + o_da), P.desc_b = (const uint8_t*)(c->d_stage + o_db);
  P.skip_a = skip_a ? (const uint8_t*)(c->d_stage + o_sa) : nullptr, P.skip_b = skip_b ? (const uint8_t*)(c->d_stage + o_sb) : nullptr;
  P.n_a = n_a, P.n_b = n_b, P.threshold = threshold;
  P.counts = (int32_t*)(c->d_stage + o_cnt), P.offsets = (const unsigned long long*)(c->d_stage + o_off);
  P.capacity = capacity, P.pairs = (int32_t*)(c->d_stage + o_pairs), P.dist = (float*)(c->d_stage + o_dist);
  launch_hamming_rows<false>(desc_bytes / 16, P, c->stream);
  FE_TRY(hipGetLastError());
  hipLaunchKernelGGL(fe::row_offsets_kernel, dim3(1), dim3(fe::SCAN_THREADS), 0, c->stream, (const int32_t*)P.counts,
                     (unsigned long long*)(c->d_stage + o_off), (unsigned long long*)(c->d_stage + o_tot), n_a);
  FE_TRY(hipGetLastError());
  if (capacity > 0) {
    launch_hamming_rows<true>(desc_bytes / 16, P, c->stream);
    FE_TRY(hipGetLastError());
  }
  FE_TRY(hipMemcpyAsync(c->h_stage + o_tot, c->d_stage + o_tot, all.size - o_tot, hipMemcpyDeviceToHost, c->stream));
  FE_TRY(hipStreamSynchronize(c->stream));
  unsigned long long total = 0;
  std::memcpy(&total, c->h_stage + o_tot, sizeof(total));
  *n_pairs = total > (unsigned long long)INT32_MAX ? INT32_MAX : (int32_t)total;
  const size_t n = total < cap ? (size_t)total : cap;
  if (n) std::memcpy(pairs, c->h_stage + o_pairs, sizeof(int32_t) * 2 * n);
  if (n && dist) std::memcpy(dist, c->h_stage + o_dist, sizeof(float) * n);
  return OKVIS_BA_OK;
}

int okvis_fe_match_descriptors(okvis_fe_context* c, int32_t n_jobs, const okvis_fe_match_job* jobs, int32_t desc_bytes, float threshold,
                               int32_t num_best, int32_t use_ratio, float ratio_threshold) {
  if (!c || n_jobs < 0 || (n_jobs > 0 && !jobs) || !desc_bytes_ok(desc_bytes) || num_best < 1 || num_best > fe::MATCH_MAX_BEST ||
      (use_ratio && num_best < 2))
    return OKVIS_BA_ERR_ARG;
  size_t rows = 0, blocks = 0, n_live = 0;  // n_live: jobs with keypoints on both sides; the others yield nothing
  for (int j = 0; j < n_jobs; ++j) {
    const okvis_fe_match_job& J = jobs[j];
    if (J.n_a < 0 || J.n_b < 0 || J.n_a > MATCH_MAX_KEYPOINTS || J.n_b > MATCH_MAX_KEYPOINTS) return OKVIS_BA_ERR_ARG;
    if ((J.n_a > 0 && !J.desc_a) || (J.n_b > 0 && (!J.desc_b || !J.pair_a || !J.pair_dist || !J.accepted))) return OKVIS_BA_ERR_ARG;
    if (J.n_a > 0 && J.n_b > 0) ++n_live, rows += (size_t)J.n_a, blocks += (size_t)(J.n_a + fe::MATCH_WAVES - 1) / fe::MATCH_WAVES;
  }
  if (blocks > (size_t)INT32_MAX || rows > (size_t)INT32_MAX) return OKVIS_BA_ERR_ARG;
  const size_t db = (size_t)desc_bytes, nbest = (size_t)num_best;
  Layout in, all;
  size_t o_lidx = 0, o_ldist = 0;
  if (rows > 0) {
    FE_TRY(hipSetDevice(c->device));
    // every job's descriptors and masks, then the job table
    struct Offsets {
      size_t da, db, sa, sb;
    };
    std::vector<Offsets> off((size_t)n_jobs);
    std::vector<fe::MatchJob> table;
    for (int j = 0; j < n_jobs; ++j) {
      const okvis_fe_match_job& J = jobs[j];
      if (J.n_a == 0 || J.n_b == 0) continue;
      off[j].da = in.add(db * J.n_a), off[j].db = in.add(db * J.n_b);
      off[j].sa = J.skip_a ? in.add((size_t)J.n_a) : 0, off[j].sb = J.skip_b ? in.add((size_t)J.n_b) : 0;
    }
    const size_t o_table = in.add(sizeof(fe::MatchJob) * n_live);
    all = in;
    o_lidx = all.add(sizeof(int32_t) * rows * nbest), o_ldist = all.add(sizeof(float) * rows * nbest);
    if (int rc = reserve(c, all.size)) return rc;
    int32_t block0 = 0, row0 = 0;
    for (int j = 0; j < n_jobs; ++j) {
      const okvis_fe_match_job& J = jobs[j];
      if (J.n_a == 0 || J.n_b == 0) continue;
      std::memcpy(c->h_stage + off[j].da, J.desc_a, db * J.n_a);
      std::memcpy(c->h_stage + off[j].db, J.desc_b, db * J.n_b);
      if (J.skip_a) std::memcpy(c->h_stage + off[j].sa, J.skip_a, (size_t)J.n_a);
      if (J.skip_b) std::memcpy(c->h_stage + off[j].sb, J.skip_b, (size_t)J.n_b);
      fe::MatchJob D;
      D.desc_a = (const uint8_t*)(c->d_stage + off[j].da), D.desc_b = (const uint8_t*)(c->d_stage + off[j].db);
      D.skip_a = J.skip_a ? (const uint8_t*)(c->d_stage + off[j].sa) : nullptr;
      D.skip_b = J.skip_b ? (const uint8_t*)(c->d_stage + off[j].sb) : nullptr;
      D.n_a = J.n_a, D.n_b = J.n_b, D.block0 = block0, D.row0 = row0;
      table.push_back(D);
      block0 += (J.n_a + fe::MATCH_WAVES - 1) / fe::MATCH_WAVES, row0 += J.n_a;
    }
    std::memcpy(c->h_stage + o_table, table.data(), sizeof(fe::MatchJob) * n_live);
    FE_TRY(hipMemcpyAsync(c->d_stage, c->h_stage, in.size, hipMemcpyHostToDevice, c->stream));
    fe::BestParams P;
    P.jobs = (const fe::MatchJob*)(c->d_stage + o_table), P.n_jobs = (int32_t)n_live;
    P.threshold = threshold, P.initial = use_ratio ? FLT_MAX : threshold, P.num_best = num_best;
    P.list_idx = (int32_t*)(c->d_stage + o_lidx), P.list_dist = (float*)(c->d_stage + o_ldist);
    launch_best_lists(desc_bytes / 16, (int)blocks, P, c->stream);
    FE_TRY(hipGetLastError());
    FE_TRY(hipMemcpyAsync(c->h_stage + o_lidx, c->d_stage + o_lidx, all.size - o_lidx, hipMemcpyDeviceToHost, c->stream));
    FE_TRY(hipStreamSynchronize(c->stream));
  }
  // the assignment chains (sequential by nature, O(n_a * num_best)) and matchBody's final loop (DenseMatcher.hpp:92-122) on the host
  size_t row0 = 0;
  for (int j = 0; j < n_jobs; ++j) {
    const okvis_fe_match_job& J = jobs[j];
    for (int b = 0; b < J.n_b; ++b) J.pair_a[b] = -1, J.pair_dist[b] = FLT_MAX, J.accepted[b] = 0;
    if (J.n_a == 0 || J.n_b == 0) continue;
    const int32_t* li = (const int32_t*)(c->h_stage + o_lidx) + row0 * nbest;
    const float* ld = (const float*)(c->h_stage + o_ldist) + row0 * nbest;
    row0 += (size_t)J.n_a;
    for (int a = 0; a < J.n_a; ++a)
      if (!(J.skip_a && J.skip_a[a])) assign_best(a, num_best, li, ld, J.pair_a, J.pair_dist);
    for (int b = 0; b < J.n_b; ++b) {
      if (!(J.pair_dist[b] < threshold)) continue;
      if (use_ratio) {
        const size_t o = (size_t)J.pair_a[b] * nbest;
        if (li[o + 1] != -1) {
          const float best = ld[o], second = ld[o + 1];
          J.accepted[b] = (best == 0 || second / best > ratio_threshold) ? 1 : 0;
        } else {
          J.accepted[b] = 1;
        }
      } else {
        J.accepted[b] = 1;
      }
    }
  }
  return OKVIS_BA_OK;
}

int okvis_fe_match_verified(okvis_fe_context* c, int32_t n_jobs, const okvis_fe_vmatch_job* jobs, int32_t desc_bytes, float threshold,
                            int32_t num_best, int32_t use_ratio, float ratio_threshold) {
  if (!c || n_jobs < 0 || (n_jobs > 0 && !jobs) || !desc_bytes_ok(desc_bytes) || num_best < 1 || num_best > fe::MATCH_MAX_BEST ||
      (use_ratio && num_best < 2))
    return OKVIS_BA_ERR_ARG;
  // per job: live = keypoints on both sides (lists are built); pre = the per-keypoint pass has something to do (a 3D2D step
  // reports its projections even against an empty image B); tri = the accepted pairs' uncertainty is wanted
  struct Plan {
    bool live, pre, tri;
    size_t da, db, sa, sb, ka, kb, hp, sga, sgb, ra, rb, uv, U, st;  // offsets, phase one
    size_t t_pairs, t_sig, t_hp, t_cov, t_fl;                         // offsets, the uncertainty launch
    double info6[36];
  };
  std::vector<Plan> plan((size_t)n_jobs);
  size_t rows = 0, blocks = 0, pre_blocks = 0, n_work = 0;
  for (int j = 0; j < n_jobs; ++j) {
    const okvis_fe_vmatch_job& J = jobs[j];
    Plan& p = plan[j];
    const bool is2d = J.kind == OKVIS_FE_MATCH_2D2D;
    if (!is2d && J.kind != OKVIS_FE_MATCH_3D2D) return OKVIS_BA_ERR_ARG;
    if (J.n_a < 0 || J.n_b < 0 || J.n_a > MATCH_MAX_KEYPOINTS || J.n_b > MATCH_MAX_KEYPOINTS) return OKVIS_BA_ERR_ARG;
    if (!camera_ok(&J.cam_a) || !camera_ok(&J.cam_b)) return OKVIS_BA_ERR_ARG;
    if (!J.kp_b || (is2d && !J.kp_a) || (!is2d && J.n_a > 0 && !J.hp_W)) return OKVIS_BA_ERR_ARG;
    if ((J.n_a > 0 && !J.desc_a) || (J.n_b > 0 && (!J.desc_b || !J.pair_a || !J.pair_dist || !J.accepted))) return OKVIS_BA_ERR_ARG;
    p.live = J.n_a > 0 && J.n_b > 0;
    p.pre = is2d ? p.live : J.n_a > 0;
    p.tri = is2d && (J.hp_a || J.cov || J.tri_flags);
    if (p.tri && !spd_inverse6(J.UOplus, p.info6)) return OKVIS_BA_ERR_ARG;
    p.tri = p.tri && p.live;
    if (p.live) rows += (size_t)J.n_a, blocks += (size_t)(J.n_a + fe::MATCH_WAVES - 1) / fe::MATCH_WAVES;
    if (p.pre) ++n_work, pre_blocks += ((size_t)J.n_a + (is2d ? (size_t)J.n_b : 0) + fe::VMATCH_PRE_THREADS - 1) / fe::VMATCH_PRE_THREADS;
  }
  if (blocks > (size_t)INT32_MAX || rows > (size_t)INT32_MAX || pre_blocks > (size_t)INT32_MAX) return OKVIS_BA_ERR_ARG;
  const size_t db = (size_t)desc_bytes, nbest = (size_t)num_best, dbl = sizeof(double);
  size_t o_lidx = 0, o_ldist = 0, o_lchi = 0, o_lfl = 0;
  if (n_work > 0) {
    FE_TRY(hipSetDevice(c->device));
    // in: every job's descriptors, masks, keypoints, landmarks and ray sigmas, then the job table; device only: the rays;
    // back: the projections and the lists; then what the uncertainty launches take and give
    Layout in, all;
    for (int j = 0; j < n_jobs; ++j) {
      const okvis_fe_vmatch_job& J = jobs[j];
      Plan& p = plan[j];
      if (!p.pre) continue;
      const bool is2d = J.kind == OKVIS_FE_MATCH_2D2D;
      const size_t na = (size_t)J.n_a, nb = (size_t)J.n_b;
      if (p.live) p.da = in.add(db * na), p.db = in.add(db * nb), p.kb = in.add(sizeof(float) * 3 * nb);
      p.sa = J.skip_a ? in.add(na) : 0, p.sb = (p.live && J.skip_b) ? in.add(nb) : 0;
      if (is2d) p.ka = in.add(sizeof(float) * 3 * na), p.sga = in.add(dbl * na), p.sgb = in.add(dbl * nb);
      else p.hp = in.add(dbl * 4 * na);
    }
    const size_t o_table = in.add(sizeof(fe::VJob) * n_work);
    all = in;
    for (int j = 0; j < n_jobs; ++j)
      if (plan[j].pre && jobs[j].kind == OKVIS_FE_MATCH_2D2D)
        plan[j].ra = all.add(dbl * 3 * jobs[j].n_a), plan[j].rb = all.add(dbl * 3 * jobs[j].n_b);
    const size_t o_back = all.size;
    for (int j = 0; j < n_jobs; ++j)
      if (plan[j].pre && jobs[j].kind == OKVIS_FE_MATCH_3D2D) {
        const size_t na = (size_t)jobs[j].n_a;
        plan[j].uv = all.add(dbl * 2 * na), plan[j].U = all.add(dbl * 4 * na), plan[j].st = all.add(na);
      }
    o_lidx = all.add(sizeof(int32_t) * rows * nbest), o_ldist = all.add(sizeof(float) * rows * nbest);
    o_lchi = all.add(dbl * rows * nbest), o_lfl = all.add(rows * nbest);
    const size_t o_back_end = all.size;
    for (int j = 0; j < n_jobs; ++j)
      if (plan[j].tri) plan[j].t_pairs = all.add(sizeof(int32_t) * 2 * jobs[j].n_b), plan[j].t_sig = all.add(dbl * jobs[j].n_b);
    for (int j = 0; j < n_jobs; ++j)
      if (plan[j].tri) {
        const size_t nb = (size_t)jobs[j].n_b;
        plan[j].t_hp = all.add(dbl * 4 * nb), plan[j].t_cov = all.add(dbl * 9 * nb), plan[j].t_fl = all.add(nb);
      }
    if (int rc = reserve(c, all.size)) return rc;
    std::vector<fe::VJob> table;
    int32_t block0 = 0, row0 = 0, pre0 = 0;
    for (int j = 0; j < n_jobs; ++j) {
      const okvis_fe_vmatch_job& J = jobs[j];
      const Plan& p = plan[j];
      if (!p.pre) continue;
      const bool is2d = J.kind == OKVIS_FE_MATCH_2D2D;
      const size_t na = (size_t)J.n_a, nb = (size_t)J.n_b;
      char *h = c->h_stage, *d = c->d_stage;
      fe::VJob D;
      std::memset(&D, 0, sizeof(D));
      if (p.live) {
        std::memcpy(h + p.da, J.desc_a, db * na);
        std::memcpy(h + p.db, J.desc_b, db * nb);
        std::memcpy(h + p.kb, J.kp_b, sizeof(float) * 3 * nb);
        D.desc_a = (const uint8_t*)(d + p.da), D.desc_b = (const uint8_t*)(d + p.db), D.kp_b = (const float*)(d + p.kb);
      }
      if (J.skip_a) std::memcpy(h + p.sa, J.skip_a, na), D.skip_a = (const uint8_t*)(d + p.sa);
      if (p.live && J.skip_b) std::memcpy(h + p.sb, J.skip_b, nb), D.skip_b = (const uint8_t*)(d + p.sb);
      if (is2d) {
        std::memcpy(h + p.ka, J.kp_a, sizeof(float) * 3 * na);
        double *sga = (double*)(h + p.sga), *sgb = (double*)(h + p.sgb);
        for (size_t k = 0; k < na; ++k) sga[k] = ray_sigma(J.kp_a[3 * k + 2], J.cam_a.intr[0]);
        for (size_t k = 0; k < nb; ++k) sgb[k] = ray_sigma(J.kp_b[3 * k + 2], J.cam_b.intr[0]);
        D.kp_a = (const float*)(d + p.ka), D.sig_a = (const double*)(d + p.sga), D.sig_b = (const double*)(d + p.sgb);
        D.ray_a = (double*)(d + p.ra), D.ray_b = (double*)(d + p.rb);
        std::memcpy(D.T, J.T_AB, sizeof(D.T));
      } else {
        std::memcpy(h + p.hp, J.hp_W, dbl * 4 * na);
        D.hp_W = (const double*)(d + p.hp);
        D.uv = (double*)(d + p.uv), D.U = (double*)(d + p.U), D.status = (uint8_t*)(d + p.st);
        std::memcpy(D.T, J.T_CbW, sizeof(D.T));
        std::memcpy(D.P3, J.P3, sizeof(D.P3));
      }
      D.cam_a = to_device(&J.cam_a), D.cam_b = to_device(&J.cam_b);
      D.kind = J.kind, D.n_a = J.n_a, D.n_b = J.n_b, D.block0 = block0, D.row0 = row0, D.pre0 = pre0;
      table.push_back(D);
      if (p.live) block0 += (J.n_a + fe::MATCH_WAVES - 1) / fe::MATCH_WAVES, row0 += J.n_a;
      pre0 += (int32_t)((na + (is2d ? nb : 0) + fe::VMATCH_PRE_THREADS - 1) / fe::VMATCH_PRE_THREADS);
    }
    std::memcpy(c->h_stage + o_table, table.data(), sizeof(fe::VJob) * n_work);
    FE_TRY(hipMemcpyAsync(c->d_stage, c->h_stage, in.size, hipMemcpyHostToDevice, c->stream));
    const fe::VJob* d_table = (const fe::VJob*)(c->d_stage + o_table);
    hipLaunchKernelGGL(fe::vmatch_prepass_kernel, dim3((unsigned)pre_blocks), dim3(fe::VMATCH_PRE_THREADS), 0, c->stream, d_table,
                       (int)n_work);
    FE_TRY(hipGetLastError());
    if (blocks > 0) {
      fe::VListParams P;
      P.jobs = d_table, P.n_jobs = (int32_t)n_work;
      P.threshold = threshold, P.initial = use_ratio ? FLT_MAX : threshold, P.num_best = num_best;
      P.list_idx = (int32_t*)(c->d_stage + o_lidx), P.list_dist = (float*)(c->d_stage + o_ldist);
      P.list_chi2 = (double*)(c->d_stage + o_lchi), P.list_flags = (uint8_t*)(c->d_stage + o_lfl);
      launch_verified_lists(desc_bytes / 16, (int)blocks, P, c->stream);
      FE_TRY(hipGetLastError());
    }
    FE_TRY(hipMemcpyAsync(c->h_stage + o_back, c->d_stage + o_back, o_back_end - o_back, hipMemcpyDeviceToHost, c->stream));
    FE_TRY(hipStreamSynchronize(c->stream));
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
    for (int b = 0; b < J.n_b; ++b) J.pair_a[b] = -1, J.pair_dist[b] = FLT_MAX, J.accepted[b] = 0;
    if (J.chi2) std::memset(J.chi2, 0, dbl * nb);
    if (J.gate_flags) std::memset(J.gate_flags, 0, nb);
    if (J.hp_a) std::memset(J.hp_a, 0, dbl * 4 * nb);
    if (J.cov) std::memset(J.cov, 0, dbl * 9 * nb);
    if (J.tri_flags) std::memset(J.tri_flags, 0, nb);
    if (!is2d && p.pre) {
      if (J.proj_status) std::memcpy(J.proj_status, c->h_stage + p.st, na);
      if (J.uv) std::memcpy(J.uv, c->h_stage + p.uv, dbl * 2 * na);
      if (J.U) std::memcpy(J.U, c->h_stage + p.U, dbl * 4 * na);
    } else {
      if (J.proj_status) std::memset(J.proj_status, 0, na);
      if (J.uv) std::memset(J.uv, 0, dbl * 2 * na);
      if (J.U) std::memset(J.U, 0, dbl * 4 * na);
    }
    if (!p.live) continue;
    const int32_t* li = (const int32_t*)(c->h_stage + o_lidx) + row0 * nbest;
    const float* ld = (const float*)(c->h_stage + o_ldist) + row0 * nbest;
    const double* lc = (const double*)(c->h_stage + o_lchi) + row0 * nbest;
    const uint8_t* lf = (const uint8_t*)(c->h_stage + o_lfl) + row0 * nbest;
    row0 += na;
    for (int a = 0; a < J.n_a; ++a)
      if (!(J.skip_a && J.skip_a[a])) assign_best(a, num_best, li, ld, J.pair_a, J.pair_dist);
    int32_t* t_pairs = p.tri ? (int32_t*)(c->h_stage + p.t_pairs) : nullptr;
    double* t_sig = p.tri ? (double*)(c->h_stage + p.t_sig) : nullptr;
    for (int b = 0; b < J.n_b; ++b) {
      if (!(J.pair_dist[b] < threshold)) continue;
      const size_t o = (size_t)J.pair_a[b] * nbest;
      if (use_ratio && li[o + 1] != -1) {
        const float best = ld[o], second = ld[o + 1];
        J.accepted[b] = (best == 0 || second / best > ratio_threshold) ? 1 : 0;
      } else {
        J.accepted[b] = 1;
      }
      if (!J.accepted[b]) continue;
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
    }
    if (n_acc[j] > 0) {
      tri_lo = std::min(tri_lo, p.t_pairs), tri_hi = std::max(tri_hi, p.t_sig + dbl * nb);
      tri_out_lo = std::min(tri_out_lo, p.t_hp), tri_out_hi = std::max(tri_out_hi, p.t_fl + nb);
    }
  }
  if (tri_hi > 0) {
    FE_TRY(hipMemcpyAsync(c->d_stage + tri_lo, c->h_stage + tri_lo, tri_hi - tri_lo, hipMemcpyHostToDevice, c->stream));
    for (int j = 0; j < n_jobs; ++j) {
      if (n_acc[j] == 0) continue;
      const okvis_fe_vmatch_job& J = jobs[j];
      const Plan& p = plan[j];
      fe::TriParams P;
      P.cam_a = to_device(&J.cam_a), P.cam_b = to_device(&J.cam_b);
      std::memcpy(P.T_AB, J.T_AB, sizeof(P.T_AB));
      std::memcpy(P.info6, p.info6, sizeof(P.info6));
      P.sigma_ray_own = 0.5 / std::fmin(J.cam_a.intr[0], J.cam_b.intr[0]);
      P.n_a = J.n_a, P.n_b = J.n_b, P.n_pairs = n_acc[j], P.want_uncertainty = 1;
      P.kp_a = (const float*)(c->d_stage + p.ka), P.kp_b = (const float*)(c->d_stage + p.kb);
      P.pairs = (const int32_t*)(c->d_stage + p.t_pairs), P.sigma_ray = (const double*)(c->d_stage + p.t_sig);
      P.hp = (double*)(c->d_stage + p.t_hp), P.cov = (double*)(c->d_stage + p.t_cov), P.flags = (uint8_t*)(c->d_stage + p.t_fl);
      P.gn = nullptr;
      FE_TRY(hipMemsetAsync(P.cov, 0, dbl * 9 * n_acc[j], c->stream));
      hipLaunchKernelGGL(fe::stereo_triangulate_kernel, dim3((n_acc[j] + fe::TRI_THREADS - 1) / fe::TRI_THREADS), dim3(fe::TRI_THREADS), 0,
                         c->stream, P);
      FE_TRY(hipGetLastError());
    }
    FE_TRY(hipMemcpyAsync(c->h_stage + tri_out_lo, c->d_stage + tri_out_lo, tri_out_hi - tri_out_lo, hipMemcpyDeviceToHost, c->stream));
    FE_TRY(hipStreamSynchronize(c->stream));
    for (int j = 0; j < n_jobs; ++j) {
      const okvis_fe_vmatch_job& J = jobs[j];
      const Plan& p = plan[j];
      const int32_t* t_pairs = (const int32_t*)(c->h_stage + p.t_pairs);
      for (int i = 0; i < n_acc[j]; ++i) {
        const size_t b = (size_t)t_pairs[2 * i + 1];
        if (J.hp_a) std::memcpy(J.hp_a + 4 * b, c->h_stage + p.t_hp + dbl * 4 * i, dbl * 4);
        if (J.cov) std::memcpy(J.cov + 9 * b, c->h_stage + p.t_cov + dbl * 9 * i, dbl * 9);
        if (J.tri_flags) J.tri_flags[b] = *(const uint8_t*)(c->h_stage + p.t_fl + i);
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
  Layout in, all;
  const size_t o_kp = in.add(sizeof(float) * 3 * n);
  all = in;
  const size_t o_b = all.add(sizeof(double) * 3 * n), o_s = all.add(sizeof(double) * n), o_ok = all.add(n);
  if (int rc = reserve(c, all.size)) return rc;
  std::memcpy(c->h_stage + o_kp, kp, sizeof(float) * 3 * n);
  FE_TRY(hipMemcpyAsync(c->d_stage, c->h_stage, in.size, hipMemcpyHostToDevice, c->stream));
  P.kp = (const float*)(c->d_stage + o_kp);
  P.bearing = (double*)(c->d_stage + o_b), P.sigma = (double*)(c->d_stage + o_s), P.ok = (uint8_t*)(c->d_stage + o_ok);
  hipLaunchKernelGGL(fe::bearing_vectors_kernel, dim3((n + 255) / 256), dim3(256), 0, c->stream, P);
  FE_TRY(hipGetLastError());
  FE_TRY(hipMemcpyAsync(c->h_stage + o_b, c->d_stage + o_b, all.size - o_b, hipMemcpyDeviceToHost, c->stream));
  FE_TRY(hipStreamSynchronize(c->stream));
  if (bearing) std::memcpy(bearing, c->h_stage + o_b, sizeof(double) * 3 * n);
  if (sigma_angle) std::memcpy(sigma_angle, c->h_stage + o_s, sizeof(double) * n);
  if (ok) std::memcpy(ok, c->h_stage + o_ok, n);
  return OKVIS_BA_OK;
}

int okvis_fe_sac_consensus(okvis_fe_context* c, int32_t n_jobs, const okvis_fe_sac_job* jobs) {
  if (!c || n_jobs < 0 || (n_jobs > 0 && !jobs)) return OKVIS_BA_ERR_ARG;
  size_t blocks = 0, n_live = 0, n_counts = 0, n_words = 0, n_scores = 0;  // n_live: jobs with correspondences
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
    if (J.scores) n_scores += (size_t)J.n_models * (size_t)J.n;
  }
  if (blocks > (size_t)INT32_MAX || n_counts > (size_t)INT32_MAX) return OKVIS_BA_ERR_ARG;
  Layout in, all;
  size_t o_counts = 0, o_ballots = 0;
  struct Offsets {
    size_t models, a, b, s1, s2, ci, cams, scores;
  };
  std::vector<Offsets> off((size_t)n_jobs);
  if (n_live > 0) {
    FE_TRY(hipSetDevice(c->device));
    for (int j = 0; j < n_jobs; ++j) {
      const okvis_fe_sac_job& J = jobs[j];
      if (J.n == 0) continue;
      const size_t n = (size_t)J.n, dbl = sizeof(double);
      const bool absolute = J.kind == OKVIS_FE_SAC_ABSOLUTE;
      off[j].models = in.add(dbl * (J.kind == OKVIS_FE_SAC_ROTATION_ONLY ? 9 : 12) * J.n_models);
      off[j].a = in.add(dbl * 3 * n), off[j].b = in.add(dbl * 3 * n), off[j].s1 = in.add(dbl * n);
      off[j].s2 = absolute ? 0 : in.add(dbl * n);
      off[j].ci = absolute ? in.add(sizeof(int32_t) * n) : 0, off[j].cams = absolute ? in.add(dbl * 12 * J.n_cams) : 0;
    }
    const size_t o_table = in.add(sizeof(fe::SacJob) * n_live);
    all = in;
    o_counts = all.add(sizeof(int32_t) * n_counts), o_ballots = all.add(sizeof(unsigned long long) * n_words);
    const size_t back = all.size;  // the normal call copies back [o_counts, back): no score matrix
    for (int j = 0; j < n_jobs; ++j)
      if (jobs[j].n > 0 && jobs[j].scores) off[j].scores = all.add(sizeof(double) * jobs[j].n_models * (size_t)jobs[j].n);
    if (int rc = reserve(c, all.size)) return rc;
    std::vector<fe::SacJob> table;
    size_t block0 = 0, count0 = 0, word0 = 0;
    for (int j = 0; j < n_jobs; ++j) {
      const okvis_fe_sac_job& J = jobs[j];
      if (J.n == 0) continue;
      const size_t n = (size_t)J.n;
      const bool absolute = J.kind == OKVIS_FE_SAC_ABSOLUTE;
      std::memcpy(c->h_stage + off[j].models, J.models, sizeof(double) * (J.kind == OKVIS_FE_SAC_ROTATION_ONLY ? 9 : 12) * J.n_models);
      // the [n][3] arrays go to the device as [3][n], so that a wave reads 64 consecutive doubles
      const double *src_a = absolute ? J.points : J.bearing1, *src_b = absolute ? J.bearing : J.bearing2;
      double *dst_a = (double*)(c->h_stage + off[j].a), *dst_b = (double*)(c->h_stage + off[j].b);
      for (size_t i = 0; i < n; ++i)
        for (int k = 0; k < 3; ++k) dst_a[k * n + i] = src_a[3 * i + k], dst_b[k * n + i] = src_b[3 * i + k];
      std::memcpy(c->h_stage + off[j].s1, absolute ? J.sigma : J.sigma1, sizeof(double) * n);
      if (absolute) {
        std::memcpy(c->h_stage + off[j].ci, J.cam_index, sizeof(int32_t) * n);
        double* cams = (double*)(c->h_stage + off[j].cams);
        for (int k = 0; k < J.n_cams; ++k) {
          std::memcpy(cams + 12 * k, J.cam_offsets + 3 * k, sizeof(double) * 3);
          std::memcpy(cams + 12 * k + 3, J.cam_rotations + 9 * k, sizeof(double) * 9);
        }
      } else {
        std::memcpy(c->h_stage + off[j].s2, J.sigma2, sizeof(double) * n);
      }
      fe::SacJob D;
      D.models = (const double*)(c->d_stage + off[j].models);
      D.a = (const double*)(c->d_stage + off[j].a), D.b = (const double*)(c->d_stage + off[j].b);
      D.sigma1 = (const double*)(c->d_stage + off[j].s1), D.sigma2 = absolute ? nullptr : (const double*)(c->d_stage + off[j].s2);
      D.cam_index = absolute ? (const int32_t*)(c->d_stage + off[j].ci) : nullptr;
      D.cams = absolute ? (const double*)(c->d_stage + off[j].cams) : nullptr;
      D.scores = J.scores ? (double*)(c->d_stage + off[j].scores) : nullptr;
      D.threshold = J.threshold, D.kind = J.kind, D.n = J.n, D.n_models = J.n_models;
      D.block0 = (int32_t)block0, D.tiles = (int32_t)((n + fe::SAC_THREADS - 1) / fe::SAC_THREADS);
      D.count0 = (int32_t)count0, D.word0 = (int64_t)word0;
      table.push_back(D);
      block0 += (size_t)D.tiles * (((size_t)J.n_models + fe::SAC_MODEL_TILE - 1) / fe::SAC_MODEL_TILE);
      count0 += (size_t)J.n_models, word0 += (size_t)J.n_models * ((n + 63) / 64);
    }
    std::memcpy(c->h_stage + o_table, table.data(), sizeof(fe::SacJob) * n_live);
    FE_TRY(hipMemcpyAsync(c->d_stage, c->h_stage, in.size, hipMemcpyHostToDevice, c->stream));
    FE_TRY(hipMemsetAsync(c->d_stage + o_counts, 0, sizeof(int32_t) * n_counts, c->stream));
    fe::SacParams P;
    P.jobs = (const fe::SacJob*)(c->d_stage + o_table), P.n_jobs = (int32_t)n_live;
    P.counts = (int32_t*)(c->d_stage + o_counts), P.ballots = (unsigned long long*)(c->d_stage + o_ballots);
    hipLaunchKernelGGL(fe::sac_consensus_kernel, dim3((unsigned)blocks), dim3(fe::SAC_THREADS), 0, c->stream, P);
    FE_TRY(hipGetLastError());
    FE_TRY(hipMemcpyAsync(c->h_stage + o_counts, c->d_stage + o_counts, (n_scores ? all.size : back) - o_counts, hipMemcpyDeviceToHost,
                          c->stream));
    FE_TRY(hipStreamSynchronize(c->stream));
  }
  // Ransac::computeModel's book-keeping on the counts (a hypothesis replaces the best only with strictly more inliers), and the
  // best hypothesis's row of ballot words expanded into indices
  size_t count0 = 0, word0 = 0;
  for (int j = 0; j < n_jobs; ++j) {
    const okvis_fe_sac_job& J = jobs[j];
    if (J.n == 0) {
      if (J.counts) std::memset(J.counts, 0, sizeof(int32_t) * J.n_models);
      if (J.best) *J.best = 0;
      if (J.n_inliers) *J.n_inliers = 0;
      continue;
    }
    const size_t words = ((size_t)J.n + 63) / 64;
    const int32_t* counts = (const int32_t*)(c->h_stage + o_counts) + count0;
    const unsigned long long* ballots = (const unsigned long long*)(c->h_stage + o_ballots) + word0;
    count0 += (size_t)J.n_models, word0 += (size_t)J.n_models * words;
    int best = 0;
    for (int m = 1; m < J.n_models; ++m)
      if (counts[m] > counts[best]) best = m;
    if (J.counts) std::memcpy(J.counts, counts, sizeof(int32_t) * J.n_models);
    if (J.best) *J.best = best;
    if (J.n_inliers) *J.n_inliers = counts[best];
    if (J.inliers) {
      int32_t k = 0;
      for (size_t w = 0; w < words; ++w)
        for (unsigned long long m = ballots[(size_t)best * words + w]; m; m &= m - 1) J.inliers[k++] = (int32_t)(64 * w) + __builtin_ctzll(m);
    }
    if (J.scores) std::memcpy(J.scores, c->h_stage + off[j].scores, sizeof(double) * J.n_models * (size_t)J.n);
  }
  return OKVIS_BA_OK;
}

}  // extern "C"
