// Part of fe_capi.hip (one translation unit).  Stereo triangulation (with and without the Gauss-Newton record), landmark
// projection and the 3D-2D gate; launch_triangulate and spd_inverse6 serve okvis_fe_match_verified (fe_capi_matching.inc) too.
namespace {

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

}  // namespace

extern "C" {

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

}  // extern "C"
