// Part of fe_capi.hip (one translation unit).  Batched IMU state propagation.
extern "C" {

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

}  // extern "C"
