// Part of ba_capi.hip, inside its extern "C" block, behind capi_landmark_covariance.inc.  okvis_ba_predicted_measurement (DESIGN.md
// "Predicted measurement covariance"): the assembly okvis_ba_state_covariance and okvis_ba_landmark_covariance share
// (cov_assemble_and_run, capi_covariance.inc) for a range of windows, then cov_pose_kernel (ba_cov.hpp; P = the pose-type part of
// S0^-1, one workgroup per window) and predcov_kernel (ba_predcov.hpp; one wave per query, all windows in one launch).  One copy up,
// one copy back, one synchronisation.  V, W and the state are read where the assembly left them, under the control record's `acc`
// (capi_landmark_covariance.inc has the argument); the kernels run in front of the restore.
namespace {

struct PredJob {
  int D = 0, Dp = 0, n = 0, n_lm = 0, n_pair = 0;
  ExportAt ex;
  size_t o_q = 0, o_P = 0, o_tail = 0, o_uv = 0, o_cov = 0, o_flags = 0, o_V = 0, o_W = 0, o_jac = 0;
};

int pred_check(const okvis_ba_solver* s, int w, const okvis_ba_pred_spec* spec, const okvis_ba_pred_result* res, PredJob& J) {
  const HostWin& H = s->wins[w];
  if (!res->uv || !res->cov || !res->flags) return OKVIS_BA_ERR_ARG;
  const int n = spec->n_q;
  if (n < 0) return OKVIS_BA_ERR_ARG;
  if (n > 0 && (!spec->q_lm || !spec->q_pose || !spec->q_ext || !spec->q_cam)) return OKVIS_BA_ERR_ARG;
  for (int i = 0; i < n; ++i) {
    if (spec->q_lm[i] < 0 || spec->q_lm[i] >= H.n_lm || spec->q_cam[i] < 0 || spec->q_cam[i] >= H.ptrs.n_cam) return OKVIS_BA_ERR_ARG;
    if (spec->q_pose[i] < 0 || spec->q_pose[i] >= H.n_pose || spec->q_ext[i] < 0 || spec->q_ext[i] >= H.n_pose) return OKVIS_BA_ERR_ARG;
    if (spec->q_pose[i] == spec->q_ext[i]) return OKVIS_BA_ERR_ARG;
  }
  if (res->capacity < n) return OKVIS_BA_ERR_ARG;
  if (H.D > OKVIS_BA_COV_MAX_WINDOW_DIM || H.ptrs.Sg != nullptr) return OKVIS_BA_ERR_UNSUPPORTED;
  J = PredJob{};
  J.D = H.D, J.Dp = H.Dp, J.n = n, J.n_lm = H.n_lm, J.n_pair = H.n_pair;
  return OKVIS_BA_OK;
}

}  // namespace

int okvis_ba_predicted_measurement(okvis_ba_solver* s, int w0, int n, const okvis_ba_pred_spec* specs, okvis_ba_pred_result* results) {
  if (!s || !specs || !results) return OKVIS_BA_ERR_ARG;
  if (!s->uploaded || s->begun || s->marg_pending.active) return OKVIS_BA_ERR_STATE;
  if (n <= 0 || w0 < 0 || (int64_t)w0 + n > (int64_t)s->wins.size()) return OKVIS_BA_ERR_ARG;
  // every window's arguments before anything is enqueued
  std::vector<PredJob> jobs((size_t)n);
  for (int i = 0; i < n; ++i)
    if (int rc = pred_check(s, w0 + i, &specs[i], &results[i], jobs[i])) return rc;
  HIP_TRY(hipSetDevice(s->device));
  if (int rc = cov_refresh_acc(s)) return rc;

  // ---- one scratch allocation: what the host writes (with the queries) | what is kept | workspaces | every window's outputs ----
  Arena A;
  CovAssembly ca;
  ca.o_wins = A.alloc(sizeof(WinPtrs) * (size_t)n);
  const size_t o_pargs = A.alloc(sizeof(CovPoseArgs) * (size_t)n), o_qargs = A.alloc(sizeof(PredcovArgs) * (size_t)n);
  ca.o_opt = A.alloc(sizeof(OptD));
  for (int i = 0; i < n; ++i) jobs[i].o_q = A.alloc(sizeof(int4) * (size_t)std::max(1, jobs[i].n));
  const size_t host_part = A.size;   // ONE copy up
  cov_alloc_keep(s, A, ca);
  int Dmax = 1, nmax = 0;
  bool tap_vw = false;
  for (int i = 0; i < n; ++i) {
    PredJob& J = jobs[i];
    const okvis_ba_pred_result& R = results[i];
    J.ex.o_rhs = A.alloc(8 * (size_t)J.D), J.ex.o_d2 = A.alloc(8 * (size_t)J.D);
    if (!R.S0) J.ex.o_S = A.alloc(8 * (size_t)J.D * J.D);
    if (!R.Spp) J.o_P = A.alloc(8 * (size_t)std::max(1, J.Dp * J.Dp));
    Dmax = std::max(Dmax, J.D), nmax = std::max(nmax, J.n);
    tap_vw = tap_vw || R.V || R.W;
  }
  size_t out_base = 0;
  for (int i = 0; i < n; ++i) {   // min_pivot | info | uv | cov | flags | the taps asked for: contiguous over the range, ONE copy back
    PredJob& J = jobs[i];
    const okvis_ba_pred_result& R = results[i];
    J.o_tail = A.alloc(16);
    if (i == 0) out_base = J.o_tail;
    J.o_uv = A.alloc(16 * (size_t)std::max(1, J.n));
    J.o_cov = A.alloc(32 * (size_t)std::max(1, J.n));
    J.o_flags = A.alloc((size_t)std::max(1, J.n));
    if (R.S0) J.ex.o_S = A.alloc(8 * (size_t)J.D * J.D);
    if (R.Spp) J.o_P = A.alloc(8 * (size_t)std::max(1, J.Dp * J.Dp));
    if (R.V) J.o_V = A.alloc(48 * (size_t)std::max(1, J.n_lm));
    if (R.W) J.o_W = A.alloc(144 * (size_t)std::max(1, J.n_pair));
    if (R.jac) J.o_jac = A.alloc(8 * PREDCOV_JAC * (size_t)std::max(1, J.n));
  }
  const size_t out_total = A.size - out_base;
  s->stage_marg.resize(host_part);
  unsigned char* const hb = s->stage_marg.data();
  if (int rc = marg_reserve_scratch(s, A.size)) return rc;
  unsigned char* d = s->marg_scratch;
  {
    std::vector<ExportAt> ex((size_t)n);
    for (int i = 0; i < n; ++i) ex[i] = jobs[i].ex;
    cov_fill_host(s, w0, n, hb, d, ca, ex.data());
  }
  for (int i = 0; i < n; ++i) {
    const PredJob& J = jobs[i];
    const okvis_ba_pred_result& R = results[i];
    CovPoseArgs p;
    std::memset(&p, 0, sizeof(p));
    p.S = reinterpret_cast<const double*>(d + J.ex.o_S);
    p.P = reinterpret_cast<double*>(d + J.o_P);
    p.tail = reinterpret_cast<double*>(d + J.o_tail);
    p.D = J.D, p.Dp = J.Dp;
    std::memcpy(&hb[o_pargs + sizeof(CovPoseArgs) * (size_t)i], &p, sizeof(p));
    PredcovArgs a;
    std::memset(&a, 0, sizeof(a));
    a.P = p.P;
    a.q = reinterpret_cast<const int4*>(d + J.o_q);
    a.uv = reinterpret_cast<double*>(d + J.o_uv);
    a.cov = reinterpret_cast<double*>(d + J.o_cov);
    a.flags = reinterpret_cast<uint8_t*>(d + J.o_flags);
    a.jac = R.jac ? reinterpret_cast<double*>(d + J.o_jac) : nullptr;
    a.tapV = R.V ? reinterpret_cast<double*>(d + J.o_V) : nullptr;
    a.tapW = R.W ? reinterpret_cast<double*>(d + J.o_W) : nullptr;
    a.n = J.n;
    std::memcpy(&hb[o_qargs + sizeof(PredcovArgs) * (size_t)i], &a, sizeof(a));
    for (int k = 0; k < J.n; ++k) {
      const int32_t q[4] = {specs[i].q_lm[k], specs[i].q_pose[k], specs[i].q_ext[k], specs[i].q_cam[k]};
      std::memcpy(&hb[J.o_q + sizeof(q) * (size_t)k], q, sizeof(q));
    }
  }
  for (auto& ev : s->ev_pred)
    if (!ev) HIP_TRY(hipEventCreate(&ev));
  int rc = cov_assemble_and_run(s, w0, n, d, hb, host_part, ca, s->ev_pred[0], s->ev_pred[1], [&](const WinPtrs* d_wins) {
    const PredcovArgs* qargs = reinterpret_cast<const PredcovArgs*>(d + o_qargs);
    hipLaunchKernelGGL(cov_pose_kernel, dim3((unsigned)n), dim3(COV_THREADS), cov_lds_bytes(Dmax), s->stream,
                       reinterpret_cast<const CovPoseArgs*>(d + o_pargs));
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipEventRecord(s->ev_pred[2], s->stream);
    if (e == hipSuccess && nmax > 0) {
      hipLaunchKernelGGL(predcov_kernel, dim3((unsigned)((nmax + PREDCOV_WAVES - 1) / PREDCOV_WAVES), (unsigned)n), dim3(PREDCOV_THREADS), 0, s->stream, d_wins, qargs);
      e = hipGetLastError();
    }
    if (e == hipSuccess && tap_vw) {
      hipLaunchKernelGGL(predcov_tap_kernel, dim3((unsigned)n), dim3(256), 0, s->stream, d_wins, qargs);
      e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipEventRecord(s->ev_pred[3], s->stream);
    return e;
  });
  if (rc != OKVIS_BA_OK) return rc;
  s->stage_dl.resize(out_total);
  HIP_TRY(hipMemcpyAsync(s->stage_dl.data(), d + out_base, out_total, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  for (int i = 0; i < n; ++i) {
    const PredJob& J = jobs[i];
    okvis_ba_pred_result& R = results[i];
    const unsigned char* o = s->stage_dl.data();
    auto at = [&](size_t off) { return o + (off - out_base); };
    std::memcpy(&R.min_pivot, at(J.o_tail), 8);
    std::memcpy(&R.info, at(J.o_tail) + 8, sizeof(int32_t));
    R.n = J.n;
    std::memcpy(R.uv, at(J.o_uv), 16 * (size_t)J.n);
    std::memcpy(R.cov, at(J.o_cov), 32 * (size_t)J.n);
    std::memcpy(R.flags, at(J.o_flags), (size_t)J.n);
    if (R.info != 0) {   // (a window whose S0 could not be inverted: P is NaN, so every cov already is; every flag says so)
      for (int k = 0; k < J.n; ++k) R.flags[k] |= PREDCOV_NO_COV;
      rc = OKVIS_BA_ERR_NUMERIC;
    }
    if (R.S0) std::memcpy(R.S0, at(J.ex.o_S), 8 * (size_t)J.D * J.D);
    if (R.Spp) std::memcpy(R.Spp, at(J.o_P), 8 * (size_t)J.Dp * J.Dp);
    if (R.V) std::memcpy(R.V, at(J.o_V), 48 * (size_t)J.n_lm);
    if (R.W) std::memcpy(R.W, at(J.o_W), 144 * (size_t)J.n_pair);
    if (R.jac) std::memcpy(R.jac, at(J.o_jac), 8 * PREDCOV_JAC * (size_t)J.n);
  }
  return rc;
}

int okvis_ba_last_predicted_measurement_ms(okvis_ba_solver* s, float* assembly_ms, float* inverse_ms, float* query_ms) {
  if (!s || !assembly_ms || !inverse_ms || !query_ms) return OKVIS_BA_ERR_ARG;
  if (!s->ev_pred[3]) return OKVIS_BA_ERR_STATE;
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipEventSynchronize(s->ev_pred[3]));
  HIP_TRY(hipEventElapsedTime(assembly_ms, s->ev_pred[0], s->ev_pred[1]));
  HIP_TRY(hipEventElapsedTime(inverse_ms, s->ev_pred[1], s->ev_pred[2]));
  HIP_TRY(hipEventElapsedTime(query_ms, s->ev_pred[2], s->ev_pred[3]));
  return OKVIS_BA_OK;
}
