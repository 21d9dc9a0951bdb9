// Part of ba_capi.hip, inside its extern "C" block.  What reads or sets an uploaded solver without optimising: state get / set, the
// staging of the packed results record and the fetches, the queries, okvis_ba_download and the measurement hooks.

int okvis_ba_set_state(okvis_ba_solver* s, int w, const double* pose, const double* sb, const double* lm) {
  if (int rc = enter(s, ENTER_RESULTS, w)) return rc;
  if (int rc = refresh_acc(s, w)) return rc;
  HostWin& H = s->wins[w];
  if (pose) HIP_TRY(hipMemcpyAsync(H.ptrs.pose[H.acc], pose, 56 * (size_t)H.n_pose, hipMemcpyHostToDevice, s->stream));
  if (sb) HIP_TRY(hipMemcpyAsync(H.ptrs.sb[H.acc], sb, 72 * (size_t)H.n_sb, hipMemcpyHostToDevice, s->stream));
  if (lm) HIP_TRY(hipMemcpyAsync(H.ptrs.lm[H.acc], lm, 32 * (size_t)H.n_lm, hipMemcpyHostToDevice, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  s->host.values_set();
  return OKVIS_BA_OK;
}

int okvis_ba_get_state(okvis_ba_solver* s, int w, double* pose, double* sb, double* lm) {
  if (int rc = enter(s, ENTER_RESULTS, w)) return rc;
  if (int rc = refresh_acc(s, w)) return rc;
  HostWin& H = s->wins[w];
  if (pose) HIP_TRY(hipMemcpyAsync(pose, H.ptrs.pose[H.acc], 56 * (size_t)H.n_pose, hipMemcpyDeviceToHost, s->stream));
  if (sb) HIP_TRY(hipMemcpyAsync(sb, H.ptrs.sb[H.acc], 72 * (size_t)H.n_sb, hipMemcpyDeviceToHost, s->stream));
  if (lm) HIP_TRY(hipMemcpyAsync(lm, H.ptrs.lm[H.acc], 32 * (size_t)H.n_lm, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  return OKVIS_BA_OK;
}

// the packed results record of window w (ResultsLayout) in page-locked host memory
static int stage_results(okvis_ba_solver* s, int w, const unsigned char** rec) {
  HostWin& H = s->wins[w];
  *rec = nullptr;
  if (s->marg_pending.active) return OKVIS_BA_ERR_STATE;   // (okvis_ba_marginalize_end first: its numbers wait in the same staging)
  const size_t total = ResultsLayout(H.n_pose, H.n_sb, H.n_lm, H.n_imu).total;
  if (total == 0) return OKVIS_BA_OK;
  if (s->host.res_staged && w == 0 && s->wins.size() == 1) {   // packed and copied by okvis_ba_finish already
    *rec = s->stage_res.data();
    return OKVIS_BA_OK;
  }
  if (int rc = refresh_acc(s, w)) return rc;
  s->stage_dl.resize(total);
  HIP_TRY(launch_imu_take_back(s, w, 1));
  hipLaunchKernelGGL(pack_results_kernel, dim3(8), dim3(256), 0, s->stream, s->d_wins + w, H.acc);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(s->stage_dl.data(), H.ptrs.results, total, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  *rec = s->stage_dl.data();
  return OKVIS_BA_OK;
}

int okvis_ba_fetch_results(okvis_ba_solver* s, int w, double* pose, double* sb, double* lm, double* lm_quality,
                           double* imu_sb_ref) {
  if (int rc = enter(s, ENTER_RESULTS, w)) return rc;
  HostWin& H = s->wins[w];
  // everything is gathered on the device into one contiguous record (ResultsLayout): one small kernel + ONE copy into page-locked
  // staging instead of five copies (each costs ~15 us of its own)
  const ResultsLayout R(H.n_pose, H.n_sb, H.n_lm, H.n_imu);
  if (R.caches.off == 0) return OKVIS_BA_OK;   // (nothing in front of the preintegration records: nothing to hand out)
  const unsigned char* st = nullptr;
  if (int rc = stage_results(s, w, &st)) return rc;
  const std::pair<double*, ResultsLayout::Part> parts[] = {{pose, R.pose}, {sb, R.sb}, {lm, R.lm}, {lm_quality, R.quality}, {imu_sb_ref, R.sb_ref}};
  for (const auto& p : parts)
    if (p.first && p.second.bytes) std::memcpy(p.first, st + p.second.off, p.second.bytes);
  return OKVIS_BA_OK;
}

int okvis_ba_fetch_imu_caches(okvis_ba_solver* s, int w, double* caches) {
  if (int rc = enter(s, ENTER_RESULTS | ENTER_PTRS_LAST, w, caches != nullptr)) return rc;
  HostWin& H = s->wins[w];
  if (H.n_imu == 0) return OKVIS_BA_OK;
  const ResultsLayout R(H.n_pose, H.n_sb, H.n_lm, H.n_imu);
  const unsigned char* st = nullptr;
  if (int rc = stage_results(s, w, &st)) return rc;
  std::memcpy(caches, st + R.caches.off, R.caches.bytes);
  return OKVIS_BA_OK;
}

int okvis_ba_last_iterate_ms(okvis_ba_solver* s, float* total_ms) {
  if (int rc = enter(s, ENTER_DEVICE, 0, total_ms != nullptr)) return rc;
  HIP_TRY(hipEventSynchronize(s->ev1));
  HIP_TRY(hipEventElapsedTime(total_ms, s->ev0, s->ev1));
  return OKVIS_BA_OK;
}

int okvis_ba_reduced_dim(okvis_ba_solver* s, int w, int32_t* dim) {
  if (int rc = enter(s, ENTER_WINDOW, w, dim != nullptr)) return rc;   // (no look at the upload: see profiles/ba_entries_notes.md)
  *dim = s->wins[w].D;
  return OKVIS_BA_OK;
}
int okvis_ba_helper_timeouts(okvis_ba_solver* s, int64_t* count) {
  if (int rc = enter(s, ENTER_UPLOADED | ENTER_DEVICE, 0, count != nullptr)) return rc;
  HIP_TRY(hipStreamSynchronize(s->stream));
  *count = 0;
  for (const HostWin& H : s->wins) {
    int n = 0;
    HIP_TRY(hipMemcpy(&n, H.ptrs.sum_sync + 2, sizeof(int), hipMemcpyDeviceToHost));
    *count += n;
  }
  return OKVIS_BA_OK;
}
int okvis_ba_launch_route(okvis_ba_solver* s, int32_t* route) {
  if (int rc = enter(s, ENTER_UPLOADED, 0, route != nullptr)) return rc;
  const LaunchPlan& p = s->plan;
  const Extent& big = *std::max_element(p.subs.begin(), p.subs.end(), [](const Extent& a, const Extent& b) { return a.nw < b.nw; });
  route[OKVIS_BA_ROUTE_WINDOWS] = p.whole.nw;
  route[OKVIS_BA_ROUTE_FUSED] = p.fused;
  route[OKVIS_BA_ROUTE_DECISION_FREE_SCHUR] = p.nodec;
  route[OKVIS_BA_ROUTE_PIECE_PATH] = p.lin2;
  route[OKVIS_BA_ROUTE_SPLIT_SMALL] = p.split_small;
  route[OKVIS_BA_ROUTE_SUB_BATCHES] = (int)p.subs.size();
  route[OKVIS_BA_ROUTE_SUB_BATCH_MAX_WINDOWS] = big.nw;
  // (the riding kernel is schur_mfma_kernel<3>'s; 4 = either of them with the serial batch loop, OKVIS_BA_TUNE_SCHUR_SERIAL_BATCHES)
  route[OKVIS_BA_ROUTE_SCHUR_KERNEL] = p.schur.k == SCHUR_RIDE3 ? SCHUR_MFMA3 : p.schur.k >= SCHUR_MFMA3_SERIAL ? 4 : p.schur.k;
  route[OKVIS_BA_ROUTE_SOLVE_DBUF] = p.solve.k == SOLVE_DENSE_DBUF || p.solve.k == SOLVE_CHAIN_DBUF;
  route[OKVIS_BA_ROUTE_SOLVE_TILED] = p.tiled.k != SOLVE_NONE;
  route[OKVIS_BA_ROUTE_SOLVE_HELPERS] = big.helpers;
  route[OKVIS_BA_ROUTE_GRAPH] = p.graph;
  route[OKVIS_BA_ROUTE_MAX_CHUNKS] = s->max.chunks;
  route[OKVIS_BA_ROUTE_SLOTS] = (int32_t)std::min<long long>(s->host.slots, 0x7fffffff);
  route[OKVIS_BA_ROUTE_SMALL_RIDES] = p.rides;
  // (linearize2_rec_kernel: the group launch records; 0 = linearize2_kernel through the window record, OKVIS_BA_TUNE_LIN_NO_RECORDS)
  route[OKVIS_BA_ROUTE_LIN_RECORDS] = p.grec_stride > 0;
  route[OKVIS_BA_ROUTE_SOLVE_MODE] = p.solve.k == SOLVE_NONE ? 0 : p.solve.k >= SOLVE_CHAIN ? OKVIS_BA_SOLVE_CHAIN : OKVIS_BA_SOLVE_DENSE;
  route[OKVIS_BA_ROUTE_THREE_LAUNCH] = p.three;
  return OKVIS_BA_OK;
}
int okvis_ba_pause_count(okvis_ba_solver* s, int64_t* count) {
  if (int rc = enter(s, ENTER_UPLOADED | ENTER_DEVICE, 0, count != nullptr)) return rc;
  HIP_TRY(hipStreamSynchronize(s->stream));
  *count = __atomic_load_n(s->h_pause, __ATOMIC_ACQUIRE) - s->pause_begin;
  return OKVIS_BA_OK;
}
int okvis_ba_pair_count(okvis_ba_solver* s, int w, int32_t* n_pair) {
  if (int rc = enter(s, ENTER_WINDOW, w, n_pair != nullptr)) return rc;
  *n_pair = s->wins[w].n_pair;
  return OKVIS_BA_OK;
}
int okvis_ba_pairs(okvis_ba_solver* s, int w, int32_t* pair_lm, int32_t* pair_block) {
  if (int rc = enter(s, ENTER_WINDOW, w, pair_lm && pair_block)) return rc;
  const HostWin& H = s->wins[w];
  for (int i = 0; i < H.n_pair; ++i) {
    pair_lm[i] = H.pair_lm[i];
    pair_block[i] = H.pair_block[i];
  }
  return OKVIS_BA_OK;
}

// the diagnostic arrays of okvis_ba_array_size / okvis_ba_download (not in the public header: tools and tests name them by number)
enum { ARR_DIAG_GROUP_RECS = 95, ARR_DIAG_SLOTS = 96, ARR_DIAG_CTRL = 97, ARR_DIAG_REDO_COUNT = 98, ARR_DIAG_PROF = 99 };

// the size table of the arrays, and where the ones that are one plain array of the arena live (null: okvis_ba_download gathers them)
static int locate(okvis_ba_solver* s, int w, int which, const double** ptr, int64_t* n) {
  const HostWin& H = s->wins[w];
  const WinPtrs& P = H.ptrs;
  const int a = H.acc;
  switch (which) {
    case OKVIS_BA_ARR_POSE: *ptr = P.pose[a]; *n = 7 * (int64_t)H.n_pose; return 0;
    case OKVIS_BA_ARR_SB: *ptr = P.sb[a]; *n = 9 * (int64_t)H.n_sb; return 0;
    case OKVIS_BA_ARR_LM: *ptr = P.lm[a]; *n = 4 * (int64_t)H.n_lm; return 0;
    case OKVIS_BA_ARR_OBS_RESIDUAL: *ptr = P.obs_r[a]; *n = 2 * (int64_t)H.n_obs; return P.obs_r[a] ? 0 : OKVIS_BA_ERR_STATE;
    case OKVIS_BA_ARR_LM_V: *ptr = P.V[a]; *n = 6 * (int64_t)H.n_lm; return 0;
    case OKVIS_BA_ARR_LM_B: *ptr = P.bl[a]; *n = 3 * (int64_t)H.n_lm; return 0;
    case OKVIS_BA_ARR_LM_HQ: *ptr = P.Hq[a]; *n = 6 * (int64_t)H.n_lm; return 0;
    case OKVIS_BA_ARR_PAIR_W: *ptr = P.W[a]; *n = 18 * (int64_t)H.n_pair; return 0;
    case OKVIS_BA_ARR_REDUCED_S: *ptr = P.S; *n = (int64_t)H.D * H.D; return P.S ? 0 : OKVIS_BA_ERR_STATE;
    case OKVIS_BA_ARR_REDUCED_RHS: *ptr = P.rhs; *n = H.D; return P.rhs ? 0 : OKVIS_BA_ERR_STATE;
    case OKVIS_BA_ARR_STEP: *ptr = P.step; *n = H.D; return 0;
    case OKVIS_BA_ARR_LM_QUALITY: *ptr = P.quality; *n = H.n_lm; return 0;
    case OKVIS_BA_ARR_GRADIENT: *ptr = P.grad; *n = H.D; return 0;
    case OKVIS_BA_ARR_DAMPING: *ptr = P.Dp2; *n = H.D; return P.Dp2 ? 0 : OKVIS_BA_ERR_STATE;
    case ARR_DIAG_PROF: *ptr = P.prof; *n = 64 + 4 * 160; return P.prof ? 0 : OKVIS_BA_ERR_STATE;
    case ARR_DIAG_REDO_COUNT: *ptr = nullptr; *n = H.n_imu; return 0;  // diagnostics: re-preintegration count per IMU factor
    case ARR_DIAG_CTRL: *ptr = nullptr; *n = 24; return 0;       // diagnostics: trust-region control record
    case ARR_DIAG_SLOTS: *ptr = nullptr; *n = 1; return 0;        // diagnostics: launch slots since okvis_ba_begin
    case ARR_DIAG_GROUP_RECS: *ptr = nullptr; *n = 1 + (int64_t)s->max.grec_stride * LIN_REC_INTS; return 0;   // diagnostics: [0] the batch's group launch
                                    // records per window (0 = none), then the slots of window w, all of them, as the DEVICE holds them
    case OKVIS_BA_ARR_IMU_SB_REF: *ptr = nullptr; *n = 9 * (int64_t)H.n_imu; return 0;
    case OKVIS_BA_ARR_IMU_RESIDUAL: *ptr = nullptr; *n = 15 * (int64_t)H.n_imu; return 0;
    case OKVIS_BA_ARR_IMU_LIN: *ptr = nullptr; *n = OKVIS_BA_IMU_LIN_DOUBLES * (int64_t)H.n_imu; return 0;
  }
  return OKVIS_BA_ERR_ARG;
}

int okvis_ba_array_size(okvis_ba_solver* s, int w, int which, int64_t* n_doubles) {
  if (int rc = enter(s, ENTER_UPLOADED | ENTER_UPLOAD_IS_ARG | ENTER_WINDOW, w, n_doubles != nullptr)) return rc;
  const double* p;
  return locate(s, w, which, &p, n_doubles);
}

int okvis_ba_download(okvis_ba_solver* s, int w, int which, double* out, int64_t n_doubles) {
  if (int rc = enter(s, ENTER_MARG_FIRST | ENTER_UPLOADED | ENTER_UPLOAD_IS_ARG | ENTER_WINDOW | ENTER_DEVICE, w, out != nullptr)) return rc;
  const double* p = nullptr;
  int64_t n = 0;
  if (int rc0 = refresh_acc(s, w)) return rc0;
  int rc = locate(s, w, which, &p, &n);
  if (rc != 0) return rc;
  if (n != n_doubles) return OKVIS_BA_ERR_ARG;
  const HostWin& H = s->wins[w];
  switch (which) {
  case OKVIS_BA_ARR_IMU_SB_REF: {
    HIP_TRY(launch_imu_take_back(s, w, 1));
    HIP_TRY(hipStreamSynchronize(s->stream));
    // one strided copy gathers the reference biases out of the per-factor cache records
    if (H.n_imu > 0)
      HIP_TRY(hipMemcpy2D(out, 9 * sizeof(double), reinterpret_cast<const unsigned char*>(H.ptrs.imu_cache) + offsetof(ImuCacheD, sb_ref),
                          sizeof(ImuCacheD), 9 * sizeof(double), (size_t)H.n_imu, hipMemcpyDeviceToHost));
    return OKVIS_BA_OK;
  }
  case ARR_DIAG_SLOTS: {   // diagnostics: launch slots since okvis_ba_begin (the same for every window of the batch)
    out[0] = (double)s->host.slots;
    return OKVIS_BA_OK;
  }
  case ARR_DIAG_GROUP_RECS: {
    const int stride = s->max.grec_stride;
    std::vector<int> r((size_t)stride * LIN_REC_INTS);
    HIP_TRY(hipStreamSynchronize(s->stream));   // (the upload's copy of the arena)
    if (stride) HIP_TRY(hipMemcpy(r.data(), s->d_grecs + (size_t)w * stride * LIN_REC_INTS, r.size() * sizeof(int), hipMemcpyDeviceToHost));
    out[0] = stride;
    for (size_t i = 0; i < r.size(); ++i) out[1 + i] = r[i];
    return OKVIS_BA_OK;
  }
  case ARR_DIAG_CTRL: {
    Ctrl c;
    HIP_TRY(hipMemcpy(&c, s->wins[w].ptrs.ctrl, sizeof(c), hipMemcpyDeviceToHost));
    const double v[24] = {c.radius, c.mu, c.cost, c.cA, c.beta, c.dl_norm, c.pend_model, c.tot_A, c.tot_C, c.tot_E, c.gd_p,
                          c.ddd_p, c.last_rho, c.last_model_change, (double)c.iter, (double)c.successful, (double)c.tr_kind,
                          (double)c.explicit_next, (double)c.pending, (double)c.acc, (double)c.done, (double)c.max_iter,
                          (double)c.invalid_steps, (double)c.chol_fail};
    for (int i = 0; i < 24; ++i) out[i] = v[i];
    return OKVIS_BA_OK;
  }
  case ARR_DIAG_REDO_COUNT: {
    for (int f = 0; f < H.n_imu; ++f) {
      ImuCacheD c;
      HIP_TRY(hipMemcpy(&c, H.ptrs.imu_cache + f, sizeof(c), hipMemcpyDeviceToHost));
      out[f] = c.redo_count;
    }
    return OKVIS_BA_OK;
  }
  case OKVIS_BA_ARR_IMU_RESIDUAL: {
    for (int f = 0; f < H.n_imu; ++f)
      HIP_TRY(hipMemcpy(out + 15 * f, H.ptrs.imu_lin[H.acc] + (size_t)f * IMU_LIN_STRIDE + IMU_R, 15 * 8, hipMemcpyDeviceToHost));
    return OKVIS_BA_OK;
  }
  case OKVIS_BA_ARR_IMU_LIN: {
    // the factors' records of the accepted buffer, H | g brought back from the order the factor workgroup wrote them in
    // (W.imu_pos, read back from the device: the list the kernel itself used) to the packed triangle over the factor's own columns
    if (H.n_imu == 0) return OKVIS_BA_OK;
    static_assert(OKVIS_BA_IMU_LIN_DOUBLES == IMU_COST + 1 && IMU_G == 465 && IMU_R == 495, "H | g | r | cost");
    std::vector<double> rec((size_t)IMU_LIN_STRIDE * H.n_imu);
    std::vector<int> pos((size_t)IMU_LIN_STRIDE * H.n_imu);
    HIP_TRY(hipStreamSynchronize(s->stream));
    HIP_TRY(hipMemcpy(rec.data(), H.ptrs.imu_lin[H.acc], rec.size() * 8, hipMemcpyDeviceToHost));
    HIP_TRY(hipMemcpy(pos.data(), H.ptrs.imu_pos, pos.size() * sizeof(int), hipMemcpyDeviceToHost));
    for (int f = 0; f < H.n_imu; ++f) {
      const double* r = rec.data() + (size_t)IMU_LIN_STRIDE * f;
      const int* ps = pos.data() + (size_t)IMU_LIN_STRIDE * f;
      double* o = out + (size_t)OKVIS_BA_IMU_LIN_DOUBLES * f;
      for (int e = 0; e < IMU_R; ++e) {
        if (ps[e] < 0 || ps[e] >= IMU_R) return OKVIS_BA_ERR_STATE;
        o[e] = r[ps[e]];
      }
      for (int e = IMU_R; e < OKVIS_BA_IMU_LIN_DOUBLES; ++e) o[e] = r[e];
    }
    return OKVIS_BA_OK;
  }
  default: break;   // one plain array of the arena
  }
  if (n > 0) HIP_TRY(hipMemcpy(out, p, (size_t)n * 8, hipMemcpyDeviceToHost));
  return OKVIS_BA_OK;
}

static int profile_impl(okvis_ba_solver* s, int n, float* ms4, float* per_launch) {
  if (s) s->host.work_enqueued();
  if (int rc = enter(s, ENTER_BEGUN | ENTER_DEVICE, 0, n > 0)) return rc;
  s->host.iterations_enqueued();
  // queue all n iterations with events between the kernels and synchronise ONCE: the kernels run
  // back-to-back on the GPU, so the event intervals are kernel durations, not host launch latency
  std::vector<hipEvent_t> ev(5 * (size_t)n);
  for (auto& e : ev) HIP_TRY(hipEventCreate(&e));
  if (ms4)
    for (int k = 0; k < 4; ++k) ms4[k] = 0.f;
  HIP_TRY(launch_budget(s, whole(s), n));
  for (int i = 0; i < n; ++i) {
    hipEvent_t* e = &ev[5 * (size_t)i];
    HIP_TRY(hipEventRecord(e[0], s->stream));
    HIP_TRY(launch_schur(s, whole(s)));
    HIP_TRY(hipEventRecord(e[1], s->stream));
    HIP_TRY(launch_solve(s, whole(s), 0));
    HIP_TRY(hipEventRecord(e[2], s->stream));
    HIP_TRY(hipEventRecord(e[3], s->stream));   // (the small factors run inside the linearise launch)
    HIP_TRY(launch_lin(s, whole(s), 0));
    HIP_TRY(hipEventRecord(e[4], s->stream));
  }
  HIP_TRY(hipStreamSynchronize(s->stream));
  for (int i = 0; i < n; ++i)
    for (int k = 0; k < 4; ++k) {
      float t = 0;
      HIP_TRY(hipEventElapsedTime(&t, ev[5 * (size_t)i + k], ev[5 * (size_t)i + k + 1]));
      if (ms4) ms4[k] += t;
      if (per_launch) per_launch[4 * (size_t)i + k] = t;
    }
  for (auto& e : ev) (void)hipEventDestroy(e);
  return OKVIS_BA_OK;
}
int okvis_ba_profile_iterations(okvis_ba_solver* s, int n, float* ms4) {
  if (!ms4) return OKVIS_BA_ERR_ARG;
  return profile_impl(s, n, ms4, nullptr);
}
int okvis_ba_profile_launches(okvis_ba_solver* s, int n, float* ms) {
  if (!ms) return OKVIS_BA_ERR_ARG;
  return profile_impl(s, n, nullptr, ms);
}

int okvis_ba_algorithmic_bytes(okvis_ba_solver* s, int64_t* lin, int64_t* schur, int64_t* solve, int64_t* small) {
  if (int rc = enter(s, ENTER_UPLOADED | ENTER_UPLOAD_IS_ARG)) return rc;
  int64_t a = 0, b = 0, c = 0, d = 0;
  for (auto& H : s->wins) {
    a += H.bytes_lin;
    b += H.bytes_schur;
    // (the ring kernels read one chunk launch record per workgroup)
    if (s->plan.rec_stride) b += (int64_t)H.n_chunk * SCHUR_REC_INTS * (int64_t)sizeof(int);
    // (... and the record instantiations of the linearise kernel one group launch record)
    if (s->plan.grec_stride) a += (int64_t)H.n_group * LIN_REC_INTS * (int64_t)sizeof(int);
    c += H.bytes_solve;
    d += H.bytes_small;
  }
  if (lin) *lin = a;
  if (schur) *schur = b;
  if (solve) *solve = c;
  if (small) *small = d;
  return OKVIS_BA_OK;
}
