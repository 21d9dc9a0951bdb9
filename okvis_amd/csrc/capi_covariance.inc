// Part of ba_capi.hip, inside its extern "C" block, behind capi_marginalize.inc (whose shared pieces it uses: the scratch block, the
// window record with export buffers, the option-record swap, schur_and_export).  okvis_ba_state_covariance (DESIGN.md "State covariance"): for a range of windows, linearise at the
// state the solver holds, eliminate the landmarks with the plain inverse and no damping (OptD::marg_mode = 2), export the reduced
// system S0 (solve_kernel final_only = 2) — one launch each, as okvis_ba_marginalize_batch does — then cov_kernel (ba_cov.hpp), one
// workgroup per window.  One copy up, one copy back, one synchronisation.  The control records and the IMU terms' preintegration
// records are kept in front of the launches and put back behind them (cov_keep_kernel): the solver is left as it was.
// The assembly (keep, linearise, eliminate, export, restore) is one helper, cov_assemble_and_run, which okvis_ba_landmark_covariance
// (capi_landmark_covariance.inc) calls with its own kernels.
namespace {

struct CovJob {
  int D = 0, k = 0;
  int rows[COV_MAX_DIM];   // the selected reduced rows, ascending (what the kernel works on)
  int at[COV_MAX_DIM];     // row p of the result (list order) = row at[p] of the kernel's
  ExportAt ex;             // where S0, rhs and the damping are exported to
  size_t o_out = 0;
};

int cov_check(const okvis_ba_solver* s, int w, const okvis_ba_cov_spec* spec, const okvis_ba_cov_result* res, CovJob& J) {
  const HostWin& H = s->wins[w];
  if (spec->n_blocks < 1 || !spec->block_type || !spec->block_idx || !res->cov) return OKVIS_BA_ERR_ARG;
  int k = 0, list[COV_MAX_DIM];
  for (int b = 0; b < spec->n_blocks; ++b) {
    const int t = spec->block_type[b], idx = spec->block_idx[b];
    if (t != OKVIS_BA_BLOCK_POSE && t != OKVIS_BA_BLOCK_SPEEDBIAS) return OKVIS_BA_ERR_ARG;
    const bool pose = t == OKVIS_BA_BLOCK_POSE;
    if (idx < 0 || idx >= (pose ? H.n_pose : H.n_sb)) return OKVIS_BA_ERR_ARG;
    const int off = pose ? H.pose_off[idx] : H.sb_off[idx], rows = pose ? 6 : 9;
    if (off < 0) return OKVIS_BA_ERR_ARG;   // a fixed block
    for (int q = 0; q < k; ++q)
      if (list[q] == off) return OKVIS_BA_ERR_ARG;   // named twice
    if (k + rows > COV_MAX_DIM) return OKVIS_BA_ERR_ARG;
    for (int r = 0; r < rows; ++r) list[k++] = off + r;
  }
  if ((int64_t)res->capacity < (int64_t)k * k) return OKVIS_BA_ERR_ARG;
  if (H.D > OKVIS_BA_COV_MAX_WINDOW_DIM || H.ptrs.Sg != nullptr) return OKVIS_BA_ERR_UNSUPPORTED;
  J = CovJob{};
  J.D = H.D, J.k = k;
  std::copy(list, list + k, J.rows);
  std::sort(J.rows, J.rows + k);
  for (int p = 0; p < k; ++p) J.at[p] = (int)(std::lower_bound(J.rows, J.rows + k, list[p]) - J.rows);
  return OKVIS_BA_OK;
}

// ---- What okvis_ba_state_covariance and okvis_ba_landmark_covariance (capi_landmark_covariance.inc) share: the assembly ----
// The scratch block of a call starts with what the host writes (window records with the export buffers attached | the entry's own
// records | the private option record), then what is kept of the solver, then workspaces and outputs.
struct CovAssembly {
  size_t o_wins = 0, o_opt = 0, o_keep = 0, keep_stride = 0;
  int max_imu = 0;
};

// (okvis_ba_begin starts from the accepted buffers as the host knows them)
int cov_refresh_acc(okvis_ba_solver* s) {
  if (s->acc_fresh) return OKVIS_BA_OK;
  std::vector<Ctrl> cs;
  if (int rc = fetch_ctrl(s, cs)) return rc;
  for (size_t i = 0; i < s->wins.size(); ++i) s->wins[i].acc = cs[i].acc & 1;
  s->acc_fresh = true;
  return OKVIS_BA_OK;
}

// the part of the scratch block that is kept of the solver (after the host-written part has been laid out)
void cov_alloc_keep(const okvis_ba_solver* s, Arena& A, CovAssembly& ca) {
  ca.max_imu = std::max(0, s->max.imu);
  ca.keep_stride = COV_KEEP_CTRL + 2 * (size_t)ca.max_imu * (sizeof(ImuCacheD) / 8);
  ca.o_keep = A.alloc(8 * ca.keep_stride * s->wins.size());
}

// window w0 + i's record with the export buffers attached, and the option record (marg_mode = 2), into the host block
void cov_fill_host(const okvis_ba_solver* s, int w0, int n, unsigned char* hb, unsigned char* d, const CovAssembly& ca, const ExportAt* ex) {
  for (int i = 0; i < n; ++i) {
    const WinPtrs P = win_with_export(s->wins[w0 + i], d, ex[i]);
    std::memcpy(&hb[ca.o_wins + sizeof(WinPtrs) * (size_t)i], &P, sizeof(P));
  }
  OptD od = marg_optd(s);
  od.marg_mode = 2;
  std::memcpy(&hb[ca.o_opt], &od, sizeof(od));
}

// One copy up; keep; linearise + landmark elimination + export, one launch each for the range (schur_and_export); the entry's
// own kernels (`stage`, which records its events itself and returns a hipError_t); whatever happened, what was kept goes back.
// ev_begin / ev_assembled are recorded in front of and behind the assembly.  On an error everything enqueued is waited for.
extern "C++" {   // (this file sits inside ba_capi.hip's extern "C" block)
template <class Stage>
int cov_assemble_and_run(okvis_ba_solver* s, int w0, int n, unsigned char* d, const unsigned char* hb, size_t host_part, const CovAssembly& ca,
                         hipEvent_t ev_begin, hipEvent_t ev_assembled, Stage&& stage) {
  const int nw = (int)s->wins.size();
  const WinPtrs* d_wins = reinterpret_cast<const WinPtrs*>(d + ca.o_wins);
  double* d_keep = reinterpret_cast<double*>(d + ca.o_keep);
  HIP_TRY(hipMemcpyAsync(d, hb, host_part, hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipEventRecord(ev_begin, s->stream));
  hipLaunchKernelGGL(cov_keep_kernel, dim3((unsigned)nw), dim3(256), 0, s->stream, s->d_wins, d_keep, ca.keep_stride, ca.max_imu, 0);
  HIP_TRY(hipGetLastError());
  struct HostFlags {
    okvis_ba_solver* s;
    bool evaluated, res_staged, acc_fresh, mirror_fresh;
    long long slots;
    ~HostFlags() {
      s->begun = false;
      s->evaluated = evaluated, s->res_staged = res_staged, s->acc_fresh = acc_fresh, s->mirror_fresh = mirror_fresh, s->slots = slots;
    }
  } host_flags{s, s->evaluated, s->res_staged, s->acc_fresh, s->mirror_fresh, s->slots};
  int rc;
  {
    MargSwapOptions swap_options{s, s->d_opt};
    s->d_opt = reinterpret_cast<OptD*>(d + ca.o_opt);
    rc = okvis_ba_begin(s);
    if (rc == OKVIS_BA_OK) {
      const hipError_t e = schur_and_export(s, w0, n, d_wins);
      if (e != hipSuccess) {
        s->last_hip_error = (int)e;
        rc = OKVIS_BA_HIP_ERROR_BASE + (int)e;
      }
    }
  }
  if (rc == OKVIS_BA_OK) {
    (void)hipEventRecord(ev_assembled, s->stream);
    const hipError_t e = stage(d_wins);
    if (e != hipSuccess) {
      s->last_hip_error = (int)e;
      rc = OKVIS_BA_HIP_ERROR_BASE + (int)e;
    }
  }
  hipLaunchKernelGGL(cov_keep_kernel, dim3((unsigned)nw), dim3(256), 0, s->stream, s->d_wins, d_keep, ca.keep_stride, ca.max_imu, 1);
  HIP_TRY(hipGetLastError());
  if (rc != OKVIS_BA_OK) HIP_TRY(hipStreamSynchronize(s->stream));
  return rc;
}
}  // extern "C++"

}  // namespace

int okvis_ba_state_covariance(okvis_ba_solver* s, int w0, int n, const okvis_ba_cov_spec* specs, okvis_ba_cov_result* results) {
  if (!s || !specs || !results) return OKVIS_BA_ERR_ARG;
  if (!s->uploaded || s->begun || s->marg_pending.active) return OKVIS_BA_ERR_STATE;
  if (n <= 0 || w0 < 0 || (int64_t)w0 + n > (int64_t)s->wins.size()) return OKVIS_BA_ERR_ARG;
  // every window's arguments before anything is enqueued
  std::vector<CovJob> jobs((size_t)n);
  for (int i = 0; i < n; ++i)
    if (int rc = cov_check(s, w0 + i, &specs[i], &results[i], jobs[i])) return rc;
  HIP_TRY(hipSetDevice(s->device));
  if (int rc = cov_refresh_acc(s)) return rc;

  // ---- one scratch allocation: what the host writes | what is kept of the solver | workspaces | every window's outputs ----
  Arena A;
  CovAssembly ca;
  ca.o_wins = A.alloc(sizeof(WinPtrs) * (size_t)n);
  const size_t o_args = A.alloc(sizeof(CovArgs) * (size_t)n);
  ca.o_opt = A.alloc(sizeof(OptD));
  const size_t host_part = A.size;   // ONE copy up
  cov_alloc_keep(s, A, ca);
  std::vector<ExportAt> ex((size_t)n);
  int Dmax = 1;
  for (int i = 0; i < n; ++i) {
    CovJob& J = jobs[i];
    J.ex.o_rhs = A.alloc(8 * (size_t)J.D), J.ex.o_d2 = A.alloc(8 * (size_t)J.D);
    if (!results[i].S0) J.ex.o_S = A.alloc(8 * (size_t)J.D * J.D);
    Dmax = std::max(Dmax, J.D);
  }
  size_t out_base = 0;
  for (int i = 0; i < n; ++i) {   // cov | min_pivot | info | the tap, if asked for: contiguous over the range, ONE copy back
    CovJob& J = jobs[i];
    J.o_out = A.alloc(8 * cov_out_doubles(J.k));
    if (i == 0) out_base = J.o_out;
    if (results[i].S0) J.ex.o_S = A.alloc(8 * (size_t)J.D * J.D);
    ex[i] = J.ex;
  }
  const size_t out_total = A.size - out_base;
  s->stage_marg.resize(host_part);
  unsigned char* const hb = s->stage_marg.data();
  if (int rc = marg_reserve_scratch(s, A.size)) return rc;
  unsigned char* d = s->marg_scratch;
  cov_fill_host(s, w0, n, hb, d, ca, ex.data());
  for (int i = 0; i < n; ++i) {
    const CovJob& J = jobs[i];
    CovArgs a;
    std::memset(&a, 0, sizeof(a));
    a.S = reinterpret_cast<const double*>(d + J.ex.o_S);
    a.out = reinterpret_cast<double*>(d + J.o_out);
    a.D = J.D, a.k = J.k;
    std::copy(J.rows, J.rows + J.k, a.rows);
    std::memcpy(&hb[o_args + sizeof(CovArgs) * (size_t)i], &a, sizeof(a));
  }
  for (auto& ev : s->ev_cov)
    if (!ev) HIP_TRY(hipEventCreate(&ev));
  int rc = cov_assemble_and_run(s, w0, n, d, hb, host_part, ca, s->ev_cov[0], s->ev_cov[1], [&](const WinPtrs*) {
    hipLaunchKernelGGL(cov_kernel, dim3((unsigned)n), dim3(COV_THREADS), cov_lds_bytes(Dmax), s->stream, reinterpret_cast<const CovArgs*>(d + o_args));
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipEventRecord(s->ev_cov[2], s->stream);
    return e;
  });
  if (rc != OKVIS_BA_OK) return rc;
  s->stage_dl.resize(out_total);
  HIP_TRY(hipMemcpyAsync(s->stage_dl.data(), d + out_base, out_total, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  for (int i = 0; i < n; ++i) {
    const CovJob& J = jobs[i];
    okvis_ba_cov_result& R = results[i];
    const int k = J.k;
    const double* o = reinterpret_cast<const double*>(s->stage_dl.data() + (J.o_out - out_base));
    for (int a = 0; a < k; ++a)
      for (int b = 0; b < k; ++b) R.cov[a * k + b] = o[J.at[a] * k + J.at[b]];
    R.dim = k;
    R.min_pivot = o[k * k];
    std::memcpy(&R.info, o + k * k + 1, sizeof(int32_t));
    if (R.S0) std::memcpy(R.S0, s->stage_dl.data() + (J.ex.o_S - out_base), 8 * (size_t)J.D * J.D);
    if (R.info != 0) rc = OKVIS_BA_ERR_NUMERIC;
  }
  return rc;
}

int okvis_ba_last_covariance_ms(okvis_ba_solver* s, float* assembly_ms, float* kernel_ms) {
  if (!s || !assembly_ms || !kernel_ms) return OKVIS_BA_ERR_ARG;
  if (!s->ev_cov[2]) return OKVIS_BA_ERR_STATE;
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipEventSynchronize(s->ev_cov[2]));
  HIP_TRY(hipEventElapsedTime(assembly_ms, s->ev_cov[0], s->ev_cov[1]));
  HIP_TRY(hipEventElapsedTime(kernel_ms, s->ev_cov[1], s->ev_cov[2]));
  return OKVIS_BA_OK;
}
