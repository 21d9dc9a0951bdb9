// Part of ba_capi.hip, inside its extern "C" block, behind capi_marginalize.inc (whose shared pieces it uses: the scratch block, the
// window record with export buffers, the option-record swap, schur_and_export).  It holds what the three covariance entries share
// (DESIGN.md "State covariance", "The plan of a covariance call") and the first of them:
//   - the plan of a call, CovPlan: the entry guard (cov_enter), the layout of the scratch block, the host-written records every
//     entry has, the stage runner of the two-stage entries, the download and the scatter of what every result has;
//   - the assembly, cov_assemble_and_run: keep, linearise at the state the solver holds, eliminate the landmarks with the plain
//     inverse and no damping (OptD::marg_mode = 2), export the reduced system S0 (solve_kernel final_only = 2) — one launch each, as
//     okvis_ba_marginalize_batch does — the entry's own kernels, restore (cov_keep_kernel): the solver is left as it was;
//   - the elapsed-time getter, cov_last_ms;
//   - okvis_ba_state_covariance: its check, its job, cov_kernel (ba_cov.hpp, one workgroup per window) and its scatter.
// One copy up, one copy back, one synchronisation.  okvis_ba_landmark_covariance (capi_landmark_covariance.inc) and
// okvis_ba_predicted_measurement (capi_predicted_measurement.inc) keep their checks, jobs, argument records, item kernels and scatters.
namespace {

// ---- The assembly ----
// The scratch block of a call starts with what the host writes (window records with the export buffers attached | the entry's own
// records | the private option record), then what is kept of the solver, then workspaces and outputs.
struct CovAssembly {
  size_t o_wins = 0, o_opt = 0, o_keep = 0, keep_stride = 0;
  int max_imu = 0;
};

// (okvis_ba_begin starts from the accepted buffers as the host knows them)
int cov_refresh_acc(okvis_ba_solver* s) {
  if (s->host.acc_fresh) return OKVIS_BA_OK;
  std::vector<Ctrl> cs;
  if (int rc = fetch_ctrl(s, cs)) return rc;
  for (size_t i = 0; i < s->wins.size(); ++i) s->wins[i].acc = cs[i].acc & 1;
  s->host.acc_read();
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
  struct KeepHostView {   // (okvis_ba_begin tramples the host's view; the call leaves it as it found it, not begun)
    okvis_ba_solver* s;
    HostView kept;
    ~KeepHostView() {
      s->host = kept;
      s->host.not_begun();
    }
  } keep_host_view{s, s->host};
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

// ---- The plan of a covariance call ----
// What a window's job has in every entry (the entry's job record derives from it): the window's sizes, where the caller wants what
// every result has, and where the plan put it in the scratch block.
struct CovTaps {
  double *S0, *Spp, *V, *W;   // null or the caller's arrays (okvis_ba_*_result)
  double* min_pivot;
  int32_t* info;
};
struct CovWin {
  int D = 0, Dp = 0, n = 0, n_lm = 0, n_pair = 0;   // n: the window's items (landmarks, queries) in the two-stage entries
  CovTaps out{};
  ExportAt ex;   // where S0, rhs and the damping are exported to
  size_t o_P = 0, o_tail = 0, o_V = 0, o_W = 0;
};

// The end of every entry's check: the windows the kernels serve, and the window's part of the job.
int cov_win_init(const HostWin& H, const CovTaps& out, CovWin& J) {
  if (H.D > OKVIS_BA_COV_MAX_WINDOW_DIM || H.ptrs.Sg != nullptr) return OKVIS_BA_ERR_UNSUPPORTED;
  J.D = H.D, J.Dp = H.Dp, J.n_lm = H.n_lm, J.n_pair = H.n_pair;
  J.out = out;
  return OKVIS_BA_OK;
}

// The entry guard: null pointers, the solver's state, the range, then every window's arguments (`check`, the entry's own) in window
// order — all before anything is enqueued.
template <class Spec, class Result, class Job, class Check>
int cov_enter(okvis_ba_solver* s, int w0, int n, const Spec* specs, Result* results, std::vector<Job>& jobs, Check check) {
  if (!s || !specs || !results) return OKVIS_BA_ERR_ARG;
  if (!s->host.uploaded || s->host.begun || s->marg_pending.active) return OKVIS_BA_ERR_STATE;
  if (n <= 0 || w0 < 0 || (int64_t)w0 + n > (int64_t)s->wins.size()) return OKVIS_BA_ERR_ARG;
  jobs.resize((size_t)n);
  for (int i = 0; i < n; ++i)
    if (int rc = check(s, w0 + i, &specs[i], &results[i], jobs[i])) return rc;
  HIP_TRY(hipSetDevice(s->device));
  return cov_refresh_acc(s);
}

// One scratch allocation: what the host writes | what is kept of the solver | workspaces | every window's outputs, contiguous
// over the range (ONE copy back).  An entry calls head, allocates its host-written lists, calls layout with the order of a
// window's outputs, fills its argument records, runs (run: the two-stage entries) and calls finish with its own scatter.
struct CovPlan {
  okvis_ba_solver* s;
  int w0, n;
  bool two_stage;   // cov_pose_kernel, an item kernel and the taps behind the assembly (landmarks, queries), not cov_kernel
  Arena A;
  CovAssembly ca;
  size_t o_pargs = 0, o_iargs = 0, item_bytes = 0, host_part = 0, out_base = 0, out_total = 0;
  int Dmax = 1, nmax = 0;
  bool tap_vw = false;
  unsigned char *hb = nullptr, *d = nullptr;

  // window records | CovPoseArgs (two-stage) | the entry's argument records of item_bytes each | the option record
  void head(size_t item_bytes_) {
    item_bytes = item_bytes_;
    ca.o_wins = A.alloc(sizeof(WinPtrs) * (size_t)n);
    if (two_stage) o_pargs = A.alloc(sizeof(CovPoseArgs) * (size_t)n);
    o_iargs = A.alloc(item_bytes * (size_t)n);
    ca.o_opt = A.alloc(sizeof(OptD));
  }
  // a tapped array is an output, an untapped one a workspace
  void alloc_taps(CovWin& J) {
    if (J.out.S0) J.ex.o_S = A.alloc(8 * (size_t)J.D * J.D);
    if (J.out.Spp) J.o_P = A.alloc(8 * (size_t)std::max(1, J.Dp * J.Dp));
    if (J.out.V) J.o_V = A.alloc(48 * (size_t)std::max(1, J.n_lm));
    if (J.out.W) J.o_W = A.alloc(144 * (size_t)std::max(1, J.n_pair));
  }
  // Behind the host-written part: keep, every window's rhs / d2 / S0 / P where they are workspaces, then every window's outputs in
  // the order `own` allocates them (min_pivot | info first in the two-stage entries; own calls alloc_taps where the taps go).
  // Then the host block: window records, option record and CovPoseArgs.
  template <class Job, class Own>
  int layout(std::vector<Job>& jobs, Own own) {
    host_part = A.size;   // ONE copy up
    cov_alloc_keep(s, A, ca);
    for (CovWin& J : jobs) {
      J.ex.o_rhs = A.alloc(8 * (size_t)J.D), J.ex.o_d2 = A.alloc(8 * (size_t)J.D);
      if (!J.out.S0) J.ex.o_S = A.alloc(8 * (size_t)J.D * J.D);
      if (two_stage && !J.out.Spp) J.o_P = A.alloc(8 * (size_t)std::max(1, J.Dp * J.Dp));
      Dmax = std::max(Dmax, J.D), nmax = std::max(nmax, J.n);
      tap_vw = tap_vw || J.out.V || J.out.W;
    }
    out_base = (A.size + 255) & ~size_t(255);   // (where Arena::alloc puts the next block)
    for (Job& J : jobs) {
      if (two_stage) J.o_tail = A.alloc(16);
      own(J);
    }
    out_total = A.size - out_base;
    s->stage_marg.resize(host_part);
    hb = s->stage_marg.data();
    if (int rc = marg_reserve_scratch(s, A.size)) return rc;
    d = s->marg_scratch;
    std::vector<ExportAt> ex((size_t)n);
    for (int i = 0; i < n; ++i) ex[i] = jobs[i].ex;
    cov_fill_host(s, w0, n, hb, d, ca, ex.data());
    for (int i = 0; two_stage && i < n; ++i) {
      const CovWin& J = jobs[i];
      CovPoseArgs p;
      std::memset(&p, 0, sizeof(p));
      p.S = reinterpret_cast<const double*>(d + J.ex.o_S);
      p.P = reinterpret_cast<double*>(d + J.o_P);
      p.tail = reinterpret_cast<double*>(d + J.o_tail);
      p.D = J.D, p.Dp = J.Dp;
      std::memcpy(&hb[o_pargs + sizeof(CovPoseArgs) * (size_t)i], &p, sizeof(p));
    }
    return OKVIS_BA_OK;
  }
  // the leading part of window J's argument record in a two-stage entry, and where record i goes in the host block
  CovWaveArgs wave_args(const CovWin& J) const {
    return CovWaveArgs{reinterpret_cast<const double*>(d + J.o_P), J.out.V ? reinterpret_cast<double*>(d + J.o_V) : nullptr,
                       J.out.W ? reinterpret_cast<double*>(d + J.o_W) : nullptr, J.n};
  }
  unsigned char* item_args(int i) const { return &hb[o_iargs + item_bytes * (size_t)i]; }
  // The stages of a two-stage entry behind the assembly: cov_pose_kernel | event | the item kernel (`item` launches it; only with
  // an item anywhere in the range) | the taps of V and W, if any is wanted | event.
  template <class Item>
  int run(CovEvents& ev, Item item) {
    if (int rc = cov_events_create(s, ev)) return rc;
    return cov_assemble_and_run(s, w0, n, d, hb, host_part, ca, ev.e[0], ev.e[1], [&](const WinPtrs* d_wins) {
      hipLaunchKernelGGL(cov_pose_kernel, dim3((unsigned)n), dim3(COV_THREADS), cov_lds_bytes(Dmax), s->stream,
                         reinterpret_cast<const CovPoseArgs*>(d + o_pargs));
      hipError_t e = hipGetLastError();
      if (e == hipSuccess) e = hipEventRecord(ev.e[2], s->stream);
      if (e == hipSuccess && nmax > 0) {
        item(d_wins);
        e = hipGetLastError();
      }
      if (e == hipSuccess && tap_vw) {
        hipLaunchKernelGGL(cov_tap_kernel, dim3((unsigned)n), dim3(256), 0, s->stream, d_wins, reinterpret_cast<const CovWaveArgs*>(d + o_iargs), item_bytes);
        e = hipGetLastError();
      }
      if (e == hipSuccess) e = hipEventRecord(ev.e[3], s->stream);
      return e;
    });
  }
  // The copy back, the synchronisation, and per window min_pivot, info, the entry's own arrays (`own`, which sees info) and the taps.
  // OKVIS_BA_ERR_NUMERIC if any window's S0 could not be inverted.
  const unsigned char* at(size_t off) const { return s->stage_dl.data() + (off - out_base); }
  template <class Job, class Own>
  int finish(const std::vector<Job>& jobs, Own own) {
    s->stage_dl.resize(out_total);
    HIP_TRY(hipMemcpyAsync(s->stage_dl.data(), d + out_base, out_total, hipMemcpyDeviceToHost, s->stream));
    HIP_TRY(hipStreamSynchronize(s->stream));
    int rc = OKVIS_BA_OK;
    for (int i = 0; i < n; ++i) {
      const Job& J = jobs[i];
      const CovTaps& T = J.out;
      std::memcpy(T.min_pivot, at(J.o_tail), 8);
      std::memcpy(T.info, at(J.o_tail) + 8, sizeof(int32_t));
      own(J, i);
      if (T.S0) std::memcpy(T.S0, at(J.ex.o_S), 8 * (size_t)J.D * J.D);
      if (T.Spp) std::memcpy(T.Spp, at(J.o_P), 8 * (size_t)J.Dp * J.Dp);
      if (T.V) std::memcpy(T.V, at(J.o_V), 48 * (size_t)J.n_lm);
      if (T.W) std::memcpy(T.W, at(J.o_W), 144 * (size_t)J.n_pair);
      if (*T.info != 0) rc = OKVIS_BA_ERR_NUMERIC;
    }
    return rc;
  }
};
}  // extern "C++"

// The HIP-event times of an entry's last call: ms[i] = from event i to event i + 1, `intervals` of them.
int cov_last_ms(okvis_ba_solver* s, const CovEvents& ev, int intervals, float* const* ms) {
  for (int i = 0; i < intervals; ++i)
    if (!ms[i]) return OKVIS_BA_ERR_ARG;
  if (!ev.e[intervals]) return OKVIS_BA_ERR_STATE;
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipEventSynchronize(ev.e[intervals]));
  for (int i = 0; i < intervals; ++i) HIP_TRY(hipEventElapsedTime(ms[i], ev.e[i], ev.e[i + 1]));
  return OKVIS_BA_OK;
}

// ---- okvis_ba_state_covariance ----
struct CovJob : CovWin {
  int k = 0;
  int rows[COV_MAX_DIM];   // the selected reduced rows, ascending (what the kernel works on)
  int at[COV_MAX_DIM];     // row p of the result (list order) = row at[p] of the kernel's
  size_t o_out = 0;
};

int cov_check(const okvis_ba_solver* s, int w, const okvis_ba_cov_spec* spec, okvis_ba_cov_result* res, CovJob& J) {
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
  J = CovJob{};
  if (int rc = cov_win_init(H, CovTaps{res->S0, nullptr, nullptr, nullptr, &res->min_pivot, &res->info}, J)) return rc;
  J.k = k;
  std::copy(list, list + k, J.rows);
  std::sort(J.rows, J.rows + k);
  for (int p = 0; p < k; ++p) J.at[p] = (int)(std::lower_bound(J.rows, J.rows + k, list[p]) - J.rows);
  return OKVIS_BA_OK;
}

}  // namespace

int okvis_ba_state_covariance(okvis_ba_solver* s, int w0, int n, const okvis_ba_cov_spec* specs, okvis_ba_cov_result* results) {
  std::vector<CovJob> jobs;
  if (int rc = cov_enter(s, w0, n, specs, results, jobs, cov_check)) return rc;
  CovPlan P{s, w0, n, false};
  P.head(sizeof(CovArgs));
  if (int rc = P.layout(jobs, [&](CovJob& J) {   // cov | min_pivot | info | the tap, if asked for
        J.o_out = P.A.alloc(8 * cov_out_doubles(J.k));
        J.o_tail = J.o_out + 8 * (size_t)J.k * J.k;
        P.alloc_taps(J);
      }))
    return rc;
  for (int i = 0; i < n; ++i) {
    const CovJob& J = jobs[i];
    CovArgs a;
    std::memset(&a, 0, sizeof(a));
    a.S = reinterpret_cast<const double*>(P.d + J.ex.o_S);
    a.out = reinterpret_cast<double*>(P.d + J.o_out);
    a.D = J.D, a.k = J.k;
    std::copy(J.rows, J.rows + J.k, a.rows);
    std::memcpy(P.item_args(i), &a, sizeof(a));
  }
  if (int rc = cov_events_create(s, s->ev_cov)) return rc;
  int rc = cov_assemble_and_run(s, w0, n, P.d, P.hb, P.host_part, P.ca, s->ev_cov.e[0], s->ev_cov.e[1], [&](const WinPtrs*) {
    hipLaunchKernelGGL(cov_kernel, dim3((unsigned)n), dim3(COV_THREADS), cov_lds_bytes(P.Dmax), s->stream, reinterpret_cast<const CovArgs*>(P.d + P.o_iargs));
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipEventRecord(s->ev_cov.e[2], s->stream);
    return e;
  });
  if (rc != OKVIS_BA_OK) return rc;
  return P.finish(jobs, [&](const CovJob& J, int i) {
    okvis_ba_cov_result& R = results[i];
    const int k = J.k;
    const double* o = reinterpret_cast<const double*>(P.at(J.o_out));
    for (int a = 0; a < k; ++a)
      for (int b = 0; b < k; ++b) R.cov[a * k + b] = o[J.at[a] * k + J.at[b]];
    R.dim = k;
  });
}

int okvis_ba_last_covariance_ms(okvis_ba_solver* s, float* assembly_ms, float* kernel_ms) {
  if (!s) return OKVIS_BA_ERR_ARG;
  float* const ms[] = {assembly_ms, kernel_ms};
  return cov_last_ms(s, s->ev_cov, 2, ms);
}
