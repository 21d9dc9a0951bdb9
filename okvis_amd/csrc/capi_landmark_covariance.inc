// Part of ba_capi.hip, inside its extern "C" block, behind capi_covariance.inc, whose plan of a covariance call (CovPlan: guard,
// scratch layout, host records, stage runner, download and scatter of the shared arrays) it uses.  okvis_ba_landmark_covariance
// (DESIGN.md "Landmark covariance") keeps here what is its own: its check, its job, its argument records with the selections, the
// launch of lmcov_kernel (ba_lmcov.hpp; one wave per selected landmark, all windows in one launch) behind cov_pose_kernel, and the
// scatter of cov and flags.  V and W are read where the assembly left them: okvis_ba_begin linearises into the trial
// buffer, the Schur launch and the solve launch (final_only = 2) take the same decision on it and reduce / accept it, and the
// control record the solve launch writes names that buffer — on the piece path and the staged path, with the fused reduction or a
// Schur launch of its own, with helper workgroups or without: all of them read W.V[acc] / W.W[acc] of the buffer the decision names
// and none writes to them (damping is added to a copy).  The kernels run in front of the restore and read the record's `acc`.
namespace {

struct LmcovJob : CovWin {
  const int32_t* sel = nullptr;   // the caller's list, or null = window order
  size_t o_sel = 0, o_cov = 0, o_flags = 0;
};

int lmcov_check(const okvis_ba_solver* s, int w, const okvis_ba_lmcov_spec* spec, okvis_ba_lmcov_result* res, LmcovJob& J) {
  const HostWin& H = s->wins[w];
  if (!res->cov || !res->flags) return OKVIS_BA_ERR_ARG;
  int n = H.n_lm;
  if (spec->lm_idx) {
    n = spec->n_lm;
    if (n < 0) return OKVIS_BA_ERR_ARG;
    for (int i = 0; i < n; ++i)
      if (spec->lm_idx[i] < 0 || spec->lm_idx[i] >= H.n_lm) return OKVIS_BA_ERR_ARG;
  }
  if (res->capacity < n) return OKVIS_BA_ERR_ARG;
  J = LmcovJob{};
  if (int rc = cov_win_init(H, CovTaps{res->S0, res->Spp, res->V, res->W, &res->min_pivot, &res->info}, J)) return rc;
  J.n = n;
  J.sel = spec->lm_idx;
  return OKVIS_BA_OK;
}

}  // namespace

int okvis_ba_landmark_covariance(okvis_ba_solver* s, int w0, int n, const okvis_ba_lmcov_spec* specs, okvis_ba_lmcov_result* results) {
  std::vector<LmcovJob> jobs;
  if (int rc = cov_enter(s, w0, n, specs, results, jobs, lmcov_check)) return rc;
  CovPlan P{s, w0, n, true};
  P.head(sizeof(LmcovArgs));
  for (LmcovJob& J : jobs)   // the selections are host-written
    if (J.sel) J.o_sel = P.A.alloc(sizeof(int32_t) * (size_t)std::max(1, J.n));
  if (int rc = P.layout(jobs, [&](LmcovJob& J) {   // min_pivot | info | cov | flags | the taps asked for
        J.o_cov = P.A.alloc(72 * (size_t)std::max(1, J.n));
        J.o_flags = P.A.alloc((size_t)std::max(1, J.n));
        P.alloc_taps(J);
      }))
    return rc;
  for (int i = 0; i < n; ++i) {
    const LmcovJob& J = jobs[i];
    LmcovArgs a;
    std::memset(&a, 0, sizeof(a));
    static_cast<CovWaveArgs&>(a) = P.wave_args(J);
    a.sel = J.sel ? reinterpret_cast<const int*>(P.d + J.o_sel) : nullptr;
    a.cov = reinterpret_cast<double*>(P.d + J.o_cov);
    a.flags = reinterpret_cast<uint8_t*>(P.d + J.o_flags);
    std::memcpy(P.item_args(i), &a, sizeof(a));
    if (J.sel && J.n > 0) std::memcpy(&P.hb[J.o_sel], J.sel, sizeof(int32_t) * (size_t)J.n);
  }
  if (int rc = P.run(s->ev_lmcov, [&](const WinPtrs* d_wins) {
        hipLaunchKernelGGL(lmcov_kernel, dim3((unsigned)((P.nmax + LMCOV_WAVES - 1) / LMCOV_WAVES), (unsigned)n), dim3(LMCOV_THREADS), 0, s->stream, d_wins,
                           reinterpret_cast<const LmcovArgs*>(P.d + P.o_iargs));
      }))
    return rc;
  return P.finish(jobs, [&](const LmcovJob& J, int i) {
    okvis_ba_lmcov_result& R = results[i];
    R.n = J.n;
    std::memcpy(R.cov, P.at(J.o_cov), 72 * (size_t)J.n);
    std::memcpy(R.flags, P.at(J.o_flags), (size_t)J.n);
    // (a window whose S0 could not be inverted: P is NaN, so every row already is; every flag says so)
    if (R.info != 0) std::memset(R.flags, 1, (size_t)J.n);
  });
}

int okvis_ba_last_landmark_covariance_ms(okvis_ba_solver* s, float* assembly_ms, float* inverse_ms, float* landmark_ms) {
  if (!s) return OKVIS_BA_ERR_ARG;
  float* const ms[] = {assembly_ms, inverse_ms, landmark_ms};
  return cov_last_ms(s, s->ev_lmcov, 3, ms);
}
