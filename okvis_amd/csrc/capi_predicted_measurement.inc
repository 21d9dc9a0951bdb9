// Part of ba_capi.hip, inside its extern "C" block, behind capi_landmark_covariance.inc.  okvis_ba_predicted_measurement (DESIGN.md
// "Predicted measurement covariance") runs on the plan of a covariance call (CovPlan, capi_covariance.inc: guard, scratch layout, host
// records, stage runner, download and scatter of the shared arrays) and keeps here what is its own: its check, its job, its
// argument records with the queries, the launch of predcov_kernel (ba_predcov.hpp; one wave per query, all windows in one launch)
// behind cov_pose_kernel, and the scatter of uv, cov, flags and the Jacobians.  V, W and the state are read where the assembly left
// them, under the control record's `acc` (capi_landmark_covariance.inc has the argument); the kernels run in front of the restore.
namespace {

struct PredJob : CovWin {
  double* jac = nullptr;   // the caller's array, or null
  size_t o_q = 0, o_uv = 0, o_cov = 0, o_flags = 0, o_jac = 0;
};

int pred_check(const okvis_ba_solver* s, int w, const okvis_ba_pred_spec* spec, okvis_ba_pred_result* res, PredJob& J) {
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
  J = PredJob{};
  if (int rc = cov_win_init(H, CovTaps{res->S0, res->Spp, res->V, res->W, &res->min_pivot, &res->info}, J)) return rc;
  J.n = n;
  J.jac = res->jac;
  return OKVIS_BA_OK;
}

}  // namespace

int okvis_ba_predicted_measurement(okvis_ba_solver* s, int w0, int n, const okvis_ba_pred_spec* specs, okvis_ba_pred_result* results) {
  std::vector<PredJob> jobs;
  if (int rc = cov_enter(s, w0, n, specs, results, jobs, pred_check)) return rc;
  CovPlan P{s, w0, n, true};
  P.head(sizeof(PredcovArgs));
  for (PredJob& J : jobs) J.o_q = P.A.alloc(sizeof(int4) * (size_t)std::max(1, J.n));   // the queries are host-written
  if (int rc = P.layout(jobs, [&](PredJob& J) {   // min_pivot | info | uv | cov | flags | the taps asked for
        J.o_uv = P.A.alloc(16 * (size_t)std::max(1, J.n));
        J.o_cov = P.A.alloc(32 * (size_t)std::max(1, J.n));
        J.o_flags = P.A.alloc((size_t)std::max(1, J.n));
        P.alloc_taps(J);
        if (J.jac) J.o_jac = P.A.alloc(8 * PREDCOV_JAC * (size_t)std::max(1, J.n));
      }))
    return rc;
  for (int i = 0; i < n; ++i) {
    const PredJob& J = jobs[i];
    PredcovArgs a;
    std::memset(&a, 0, sizeof(a));
    static_cast<CovWaveArgs&>(a) = P.wave_args(J);
    a.q = reinterpret_cast<const int4*>(P.d + J.o_q);
    a.uv = reinterpret_cast<double*>(P.d + J.o_uv);
    a.cov = reinterpret_cast<double*>(P.d + J.o_cov);
    a.flags = reinterpret_cast<uint8_t*>(P.d + J.o_flags);
    a.jac = J.jac ? reinterpret_cast<double*>(P.d + J.o_jac) : nullptr;
    std::memcpy(P.item_args(i), &a, sizeof(a));
    for (int k = 0; k < J.n; ++k) {
      const int32_t q[4] = {specs[i].q_lm[k], specs[i].q_pose[k], specs[i].q_ext[k], specs[i].q_cam[k]};
      std::memcpy(&P.hb[J.o_q + sizeof(q) * (size_t)k], q, sizeof(q));
    }
  }
  if (int rc = P.run(s->ev_pred, [&](const WinPtrs* d_wins) {
        hipLaunchKernelGGL(predcov_kernel, dim3((unsigned)((P.nmax + PREDCOV_WAVES - 1) / PREDCOV_WAVES), (unsigned)n), dim3(PREDCOV_THREADS), 0, s->stream, d_wins,
                           reinterpret_cast<const PredcovArgs*>(P.d + P.o_iargs));
      }))
    return rc;
  return P.finish(jobs, [&](const PredJob& J, int i) {
    okvis_ba_pred_result& R = results[i];
    R.n = J.n;
    std::memcpy(R.uv, P.at(J.o_uv), 16 * (size_t)J.n);
    std::memcpy(R.cov, P.at(J.o_cov), 32 * (size_t)J.n);
    std::memcpy(R.flags, P.at(J.o_flags), (size_t)J.n);
    // (a window whose S0 could not be inverted: P is NaN, so every cov already is; every flag says so)
    for (int k = 0; R.info != 0 && k < J.n; ++k) R.flags[k] |= PREDCOV_NO_COV;
    if (R.jac) std::memcpy(R.jac, P.at(J.o_jac), 8 * PREDCOV_JAC * (size_t)J.n);
  });
}

int okvis_ba_last_predicted_measurement_ms(okvis_ba_solver* s, float* assembly_ms, float* inverse_ms, float* query_ms) {
  if (!s) return OKVIS_BA_ERR_ARG;
  float* const ms[] = {assembly_ms, inverse_ms, query_ms};
  return cov_last_ms(s, s->ev_pred, 3, ms);
}
