// Part of ba_capi.hip, inside its extern "C" block.  What puts windows on the device: the early preintegration (pre_launch), the
// upload as a list of stages (upload_impl), okvis_ba_upload, the okvis_ba_check_window pair, and the edits of an uploaded batch -
// okvis_ba_patch_window, okvis_ba_set_marg_prior_values, okvis_ba_patched_view.

// Host time of a call's sections: lap() gives the ms since the previous lap (or the start) and, under OKVIS_BA_DEBUG=build, books
// them to the named section of g_build_times (printed at exit with build_window's)
struct SectionTimer {
  std::chrono::steady_clock::time_point t = std::chrono::steady_clock::now();
  double lap(const char* name) {
    const auto now = std::chrono::steady_clock::now();
    const double ms = std::chrono::duration<double, std::milli>(now - t).count();
    t = now;
    if (name && g_build_times.on) g_build_times.ms[name] += ms;
    return ms;
  }
};

// H0 = J^T J of window w's prior (Dm rows), formed on the device behind the copy of J (HostWin::h0_on_device)
static hipError_t launch_marg_h0(okvis_ba_solver* s, int w, int Dm) {
  hipLaunchKernelGGL(marg_h0_kernel, dim3((unsigned)(((size_t)Dm * Dm + 255) / 256), 1), dim3(256), 0, s->stream, s->d_wins, w);
  return hipGetLastError();
}

// IMU terms that arrive without a preintegration (flag 0) get theirs started now, at the bias their first evaluation will see (the
// uploaded value of their first speed/bias block), so that it runs while the host builds the index lists (imu_pre_kernel,
// ba_linearize2.hpp).  A handful of terms only — the new term of a sliding window; a batch of fresh windows re-preintegrates inside
// its first linearise launch as before (hundreds of terms fill the device either way).  Returns the number started; where[k] =
// (window, term) and the device records wait at *src for imu_pre_place_kernel.  OKVIS_BA_TUNE_NO_EARLY_PREINTEGRATION switches it off (A/B).
constexpr int PRE_MAX_TERMS = 8;
static int pre_launch(okvis_ba_solver* s, int n_windows, const okvis_ba_window* windows, const int2** where_dev, const ImuCacheD** src_dev) {
  if (s->opt.tuning.flags & OKVIS_BA_TUNE_NO_EARLY_PREINTEGRATION) return 0;
  struct Item {
    int w, f;
  };
  Item items[PRE_MAX_TERMS];
  int K = 0;
  size_t samples = 0;
  for (int i = 0; i < n_windows; ++i) {
    const okvis_ba_window& w = windows[i];
    if (w.n_imu <= 0) continue;
    if (!w.imu_pose0 || !w.imu_sb0 || !w.imu_t0 || !w.imu_t1 || !w.imu_s_begin || !w.imu_s_count || !w.imu_s_t || !w.imu_s_gyr || !w.imu_s_acc || !w.sb)
      return 0;   // (the index build reports it)
    for (int f = 0; f < w.n_imu; ++f) {
      if (w.imu_sb_ref && w.imu_sb_ref_valid && w.imu_sb_ref_valid[f]) continue;
      const int64_t b = w.imu_s_begin[f], c = w.imu_s_count[f];
      if (w.imu_sb0[f] < 0 || w.imu_sb0[f] >= w.n_sb || b < 0 || c < 2 || c > MAX_IMU_SAMPLES || b + c > (int64_t)w.n_imu_samples) return 0;
      if (!(w.imu_s_t[b + c - 1] >= w.imu_t1[f])) return 0;   // (ImuError::redoPreintegration's -1: the upload refuses the window)
      if (K == PRE_MAX_TERMS) return 0;
      items[K++] = Item{i, f};
      samples += (size_t)c;
    }
  }
  if (K == 0) return 0;
  // the staged block: stand-in window records | biases | (window, term) | t0 | t1 | sample begin (0) | sample count | samples | records
  auto up8 = [](size_t x) { return (x + 7) & ~size_t(7); };
  const size_t o_mini = 0, o_sb = o_mini + sizeof(WinPtrs) * K, o_where = o_sb + 72 * (size_t)K, o_t0 = o_where + sizeof(int2) * K,
               o_t1 = o_t0 + 8 * (size_t)K, o_beg = o_t1 + 8 * (size_t)K, o_cnt = up8(o_beg + 4 * (size_t)K), o_st = up8(o_cnt + 4 * (size_t)K),
               o_gyr = o_st + 8 * samples, o_acc = o_gyr + 24 * samples, total = o_acc + 24 * samples;
  // The device reads the block where the host writes it: page-locked host memory is mapped into the device's address space, the
  // few KB cross PCIe once, coalesced, and the host saves the copy call.  Only the records live in device memory (imu_redo writes
  // every field but the counter of re-preintegrations, which it counts up: imu_pre_place_kernel sets that to 1).
  if (!s->d_pre) {
    if (hipMalloc(&s->d_pre, sizeof(ImuCacheD) * PRE_MAX_TERMS) != hipSuccess) return 0;
  }
  if (s->stage_pre.size() < total) s->stage_pre.resize(total + total / 2);
  if (!stage_is_pinned(s->stage_pre)) return 0;   // (pageable memory: the device cannot read it in place)
  unsigned char* h = s->stage_pre.data();
  unsigned char* d = h;                // (inputs: the staging block itself)
  unsigned char* rec = s->d_pre;       // (outputs)
  std::memset(h, 0, o_st);             // (the fixed-size head; the samples are written in full below)
  size_t at = 0;   // samples placed so far
  for (int k = 0; k < K; ++k) {
    const okvis_ba_window& w = windows[items[k].w];
    const int f = items[k].f, b = w.imu_s_begin[f], c = w.imu_s_count[f];
    WinPtrs P;
    std::memset(&P, 0, sizeof(P));
    P.n_imu = 1;
    P.imu.sigma_g_c = w.imu_params.sigma_g_c; P.imu.sigma_a_c = w.imu_params.sigma_a_c;
    P.imu.sigma_gw_c = w.imu_params.sigma_gw_c; P.imu.sigma_aw_c = w.imu_params.sigma_aw_c;
    P.imu.g = w.imu_params.g; P.imu.g_max = w.imu_params.g_max; P.imu.a_max = w.imu_params.a_max;
    OFF(imu_t0, (size_t)(uintptr_t)(d + o_t0 + 8 * (size_t)k));
    OFF(imu_t1, (size_t)(uintptr_t)(d + o_t1 + 8 * (size_t)k));
    OFF(imu_s_begin, (size_t)(uintptr_t)(d + o_beg + 4 * (size_t)k));
    OFF(imu_s_count, (size_t)(uintptr_t)(d + o_cnt + 4 * (size_t)k));
    OFF(imu_s_t, (size_t)(uintptr_t)(d + o_st + 8 * at));
    OFF(imu_s_gyr, (size_t)(uintptr_t)(d + o_gyr + 24 * at));
    OFF(imu_s_acc, (size_t)(uintptr_t)(d + o_acc + 24 * at));
    OFF(imu_cache, (size_t)(uintptr_t)(rec + sizeof(ImuCacheD) * (size_t)k));
    std::memcpy(h + o_mini + sizeof(WinPtrs) * (size_t)k, &P, sizeof(P));
    std::memcpy(h + o_sb + 72 * (size_t)k, w.sb + 9 * (size_t)w.imu_sb0[f], 72);
    const int2 wf = make_int2(items[k].w, f);
    std::memcpy(h + o_where + sizeof(int2) * (size_t)k, &wf, sizeof(wf));
    const long long t0 = w.imu_t0[f], t1 = w.imu_t1[f];
    std::memcpy(h + o_t0 + 8 * (size_t)k, &t0, 8);
    std::memcpy(h + o_t1 + 8 * (size_t)k, &t1, 8);
    const int32_t cnt = c;
    std::memcpy(h + o_cnt + 4 * (size_t)k, &cnt, 4);
    for (int j = 0; j < c; ++j) {
      const long long t = w.imu_s_t[b + j];
      std::memcpy(h + o_st + 8 * (at + j), &t, 8);
    }
    std::memcpy(h + o_gyr + 24 * at, w.imu_s_gyr + 3 * (size_t)b, 24 * (size_t)c);
    std::memcpy(h + o_acc + 24 * at, w.imu_s_acc + 3 * (size_t)b, 24 * (size_t)c);
    at += (size_t)c;
  }
  // On the solver's own stream (idle here: upload_impl has waited for it, so the block of the previous call is no longer read).
  // A stream of their own with an event in front of imu_pre_place_kernel was measured too: the arena copy then no longer
  // queues up behind the recursion, but the cross-stream wait costs what that buys (replay optimize() 0.91 against 0.89 ms).
  hipLaunchKernelGGL(imu_pre_kernel, dim3((unsigned)K), dim3(IMU_THREADS), small_smem(), s->stream, reinterpret_cast<const WinPtrs*>(d + o_mini),
                     reinterpret_cast<const double*>(d + o_sb));
  if (hipGetLastError() != hipSuccess) return 0;
  *where_dev = reinterpret_cast<const int2*>(d + o_where);
  *src_dev = reinterpret_cast<const ImuCacheD*>(rec);
  return K;
}

// ---- okvis_ba_upload / okvis_ba_patch_window: the upload, stage by stage ----
// What the stages of one upload hand on to one another.
struct Upload {
  okvis_ba_solver* s;
  int n;                            // windows
  const okvis_ba_window* windows;
  Arena A;
  std::vector<HostWin> wins;
  BatchLayout L;
  BatchMax M;
  int n_pre = 0;                    // early preintegrations (pre_launch): how many, their (window, term) and their records
  const int2* pre_where = nullptr;
  const ImuCacheD* pre_src = nullptr;
  size_t rec_off = 0, grec_off = 0;     // the chunk / group launch records in the arena
  int rec_stride = 0, grec_stride = 0;
  unsigned char* zbase = nullptr;       // the arena's zero part on the device
};

// the layout the batch asks for, then the index build: the piece path unless a window does not fit it (free extrinsics, a landmark
// with more than LIN2_PIECES pieces), the chain solver where allowed if EVERY LDS-resident window fits it, else the dense LDL^T;
// then the launch records
static int upload_index(Upload& U) {
  U.L = batch_layout(U.s->opt, U.n);
  if (int rc = build_batch(U.windows, U.n, U.s->opt, U.L, U.A, U.wins.data())) return rc;
  U.rec_stride = build_chunk_records(U.A, U.wins.data(), U.n, &U.rec_off);
  U.grec_stride = build_group_records(U.A, U.wins.data(), U.n, &U.grec_off);
  return OKVIS_BA_OK;
}

// the arena: room for it, its zero part cleared on the device, its data part copied
static int upload_arena(Upload& U) {
  okvis_ba_solver* s = U.s;
  Arena& A = U.A;
  // grow-only device allocations: the per-frame re-upload of okvis_amd::Estimator must not pay hipFree/hipMalloc
  if (A.host.size() < A.size) A.host.resize(A.size, 0);
  if (A.total() > s->arena_capacity) {
    if (s->d_arena) HIP_TRY(hipFree(s->d_arena));
    s->d_arena = nullptr;
    s->arena_capacity = 0;
    const size_t cap = A.total() + A.total() / 4;
    HIP_TRY(hipMalloc(&s->d_arena, cap));
    s->arena_capacity = cap;
  }
  s->arena_bytes = A.total();
  U.zbase = s->d_arena + A.data_bytes();
  if (A.zsize) HIP_TRY(hipMemsetAsync(U.zbase, 0, A.zsize, s->stream));   // overlaps with the copy below
  HIP_TRY(hipMemcpyAsync(s->d_arena, A.host.data(), A.size, hipMemcpyHostToDevice, s->stream));
  return OKVIS_BA_OK;
}

// room for the records, the windows' offsets turned into pointers, and the one copy of option, window and control records
static int upload_records(Upload& U) {
  okvis_ba_solver* s = U.s;
  const int n_windows = U.n;
  std::vector<HostWin>& wins = U.wins;
  if ((size_t)n_windows > s->wins_capacity) {   // [OptD, padded | WinPtrs x n | CtrlSlot x n], see okvis_ba_create
    if (s->d_opt) HIP_TRY(hipFree(s->d_opt));
    s->d_opt = nullptr;
    s->d_wins = nullptr;
    s->d_ctrl = nullptr;
    s->wins_capacity = 0;
    HIP_TRY(hipMalloc(&s->d_opt, records_bytes((size_t)n_windows)));
    s->d_wins = reinterpret_cast<WinPtrs*>(reinterpret_cast<unsigned char*>(s->d_opt) + OPT_PAD);
    s->wins_capacity = (size_t)n_windows;
  }
  // (the control records follow the records of the windows that are there: n_windows of them, not the capacity)
  s->d_ctrl = reinterpret_cast<CtrlSlot*>(reinterpret_cast<unsigned char*>(s->d_opt) + ctrl_off((size_t)n_windows));
  std::vector<WinPtrs> ptrs(n_windows);
  for (int i = 0; i < n_windows; ++i) {
    relocate(wins[i].ptrs, s->d_arena, U.zbase, s->opt.debug_arrays);
    wins[i].ptrs.ctrl = (decltype(wins[i].ptrs.ctrl))(&s->d_ctrl[i].c);   // (not the arena's slot: see CtrlSlot)
    ptrs[i] = wins[i].ptrs;
  }
  U.M = batch_max(wins.data(), ptrs.data(), n_windows);
  U.M.rec_stride = U.rec_stride;
  s->d_recs = U.rec_stride ? reinterpret_cast<const int*>(s->d_arena + U.rec_off) : nullptr;
  U.M.grec_stride = U.grec_stride;
  s->d_grecs = U.grec_stride ? reinterpret_cast<const int*>(s->d_arena + U.grec_off) : nullptr;
  // one copy: option record, window records and the (zeroed) control records behind them
  const size_t wb = sizeof(WinPtrs) * (size_t)n_windows, all = records_bytes((size_t)n_windows);
  s->stage_small.resize(all);
  std::memset(s->stage_small.data(), 0, all);
  const OptD d = make_optd(s->opt, n_windows);
  std::memcpy(s->stage_small.data(), &d, sizeof(d));
  std::memcpy(s->stage_small.data() + OPT_PAD, ptrs.data(), wb);
  HIP_TRY(hipMemcpyAsync(s->d_opt, s->stage_small.data(), all, hipMemcpyHostToDevice, s->stream));
  return OKVIS_BA_OK;
}

// the records started before the index build take their places in the window; the large priors' H0 is formed; the solver takes
// the windows over
static int upload_place(Upload& U) {
  okvis_ba_solver* s = U.s;
  if (U.n_pre > 0) {
    hipLaunchKernelGGL(imu_pre_place_kernel, dim3((unsigned)U.n_pre), dim3(64), 0, s->stream, s->d_wins, U.pre_where, U.pre_src);
    HIP_TRY(hipGetLastError());
  }
  for (int i = 0; i < U.n; ++i)
    if (U.wins[i].h0_on_device) HIP_TRY(launch_marg_h0(s, i, U.wins[i].marg_dim));
  s->wins.swap(U.wins);
  return OKVIS_BA_OK;
}

// the sub-batches' streams (the first is the solver's own)
static int upload_streams(okvis_ba_solver* s) {
  const int nsub = (int)s->plan.subs.size();
  const bool same = (nsub > 1 ? (int)s->sub_streams.size() == nsub : s->sub_streams.empty());
  if (!same) {
    for (auto st : s->sub_streams)
      if (st != s->stream) (void)hipStreamDestroy(st);
    for (auto ev : s->sub_events) (void)hipEventDestroy(ev);
    s->sub_streams.clear();
    s->sub_events.clear();
  }
  if (nsub > 1 && !same) {
    for (int k = 0; k < nsub; ++k) {
      hipStream_t st;
      hipEvent_t ev;
      // the first sub-batch runs on the solver's own stream (round 6): an idle stream still holds one of the process's hardware
      // queues, and the runtime runs four of them side by side, not more (profiles/r06_notes.md: 64 windows on 3 + 1 idle streams
      // 479 k, on the solver's stream + 2: 486 k window-iterations/s; a fifth active stream halves the rate)
      if (k == 0) st = s->stream;
      else HIP_TRY(hipStreamCreateWithFlags(&st, hipStreamNonBlocking));
      HIP_TRY(hipEventCreateWithFlags(&ev, hipEventDisableTiming));
      s->sub_streams.push_back(st);
      s->sub_events.push_back(ev);
    }
  }
  return OKVIS_BA_OK;
}

static int upload_impl(okvis_ba_solver* s, int n_windows, const okvis_ba_window* windows) {
  if (s->marg_pending.active) return OKVIS_BA_ERR_STATE;   // (okvis_ba_marginalize_end first)
  SectionTimer tm;
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipStreamSynchronize(s->stream));
  const double ms_sync = tm.lap("upload_impl: wait for the stream");
  s->host.upload_started();
  Upload U{s, n_windows, windows};
  U.A.host.swap(s->stage);   // page-locked, kept (with its size) from the previous upload (the stream is idle: see the sync above)
  GiveBack give_back{U.A.host, s->stage};
  U.wins.resize((size_t)n_windows);
  U.n_pre = pre_launch(s, n_windows, windows, &U.pre_where, &U.pre_src);   // (runs on the device while the lists are built)
  const double ms_pre = tm.lap(nullptr);
  if (int rc = upload_index(U)) return rc;
  const double ms_index = tm.lap("upload_impl: index build (sum of the sections)");
  if (int rc = upload_arena(U)) return rc;
  if (int rc = upload_records(U)) return rc;
  if (int rc = upload_place(U)) return rc;
  s->layout = U.L, s->max = U.M;
  s->plan = make_plan(U.L, U.M, s->opt, n_windows);
  if (int rc = upload_streams(s)) return rc;
  keep_graphs(s);
  s->host.upload_done();
  const double ms_enqueue = tm.lap("upload_impl: staging + enqueue");
  if (g_build_times.on) g_build_times.ms["upload_impl calls"] += 1.0;
  if (debug_word().upload)
    std::fprintf(stderr, "upload: sync %.3f ms, graphs %.3f ms, index build %.3f ms, staging + enqueue %.3f ms, arena %zu bytes data + %zu zero\n",
                 ms_sync, ms_pre, ms_index, ms_enqueue, (size_t)U.A.size, (size_t)U.A.zsize);
  return OKVIS_BA_OK;
}

int okvis_ba_upload(okvis_ba_solver* s, int n_windows, const okvis_ba_window* windows) {
  if (!s || n_windows <= 0 || !windows) return OKVIS_BA_ERR_ARG;
  const int rc = upload_impl(s, n_windows, windows);
  s->host.containers_match(false);
  if (rc != OKVIS_BA_OK || !s->patchable) {
    s->mirrors.clear();
    return rc;
  }
  struct Note {   // (booked however the copy ends)
    SectionTimer tm;
    ~Note() { tm.lap("upload: copy into the container"); }
  } note;
  try {   // a patchable solver keeps what it was given (ba_store.hpp)
    s->mirrors.resize((size_t)n_windows);
    for (int i = 0; i < n_windows; ++i)
      if (int rs = s->mirrors[i].assign(windows[i])) {
        s->mirrors.clear();
        return rs;
      }
  } catch (const std::bad_alloc&) {
    s->mirrors.clear();
    return OKVIS_BA_ERR_ARG;
  }
  s->host.containers_match(true);
  return OKVIS_BA_OK;
}

int okvis_ba_check_window(const okvis_ba_window* w, const okvis_ba_options* opt, int64_t* stats) {
  if (!w) return OKVIS_BA_ERR_ARG;
  okvis_ba_options o;
  if (opt) o = *opt; else okvis_ba_default_options(&o);
  Arena A;
  HostWin H;
  // (the staging bytes are kept between calls like a solver keeps them between uploads — except for a dump, whose alignment
  // gaps must be zero)
  static thread_local StageVec kept;
  const bool dumping = !debug_word().arena.empty();
  if (!dumping) A.host.swap(kept);
  GiveBack give_back{A.host, kept, !dumping};
  BatchLayout L = batch_layout(o, 1);   // (the route okvis_ba_upload takes for a one-window batch)
  if (int rc = build_batch(w, 1, o, L, A, &H)) return rc;
  if (dumping) {   // diagnostics (OKVIS_BA_DEBUG=arena=<file>): the index build's output, byte for byte
    if (FILE* f = std::fopen(debug_word().arena.c_str(), "wb")) {
      std::fwrite(A.host.data(), 1, A.size, f);
      std::fwrite(&H.ptrs, 1, sizeof(H.ptrs), f);
      std::fclose(f);
    }
  }
  if (stats) {
    stats[0] = H.D; stats[1] = H.Dp; stats[2] = H.n_pair; stats[3] = H.n_group; stats[4] = H.n_chunk;
    stats[5] = H.ptrs.n_task; stats[6] = H.ptrs.gpart_size; stats[7] = (int64_t)A.total();
  }
  return OKVIS_BA_OK;
}

int okvis_ba_check_window_lists(const okvis_ba_window* w, const okvis_ba_options* opt, int32_t n_windows, int32_t which,
                                int32_t* out, int64_t capacity, int64_t* n) {
  if (!w || !n || n_windows <= 0 || capacity < 0 || (capacity > 0 && !out)) return OKVIS_BA_ERR_ARG;
  okvis_ba_options o;
  if (opt) o = *opt; else okvis_ba_default_options(&o);
  Arena A;
  HostWin H;
  BatchLayout L = batch_layout(o, n_windows);   // (the window as one of a batch of n_windows)
  if (int rc = build_batch(w, 1, o, L, A, &H)) return rc;
  const WinPtrs& P = H.ptrs;   // (the pointer members still hold offsets into the arena's data part)
  const unsigned char* base = A.host.data();
  auto at = [&](const void* field) { return base + reinterpret_cast<size_t>(field); };
  const int nb = P.Dp / 6;
  const void* src = nullptr;
  int64_t count = 0;
  int width = 4;   // bytes per entry
  std::vector<int32_t> plan_ints;
  switch (which) {
    case OKVIS_BA_LIST_GROUPS: src = at((const void*)P.groups), count = 16 * (int64_t)P.n_group; break;
    case OKVIS_BA_LIST_LM_OBS_BEGIN: src = at((const void*)P.lm_obs_begin), count = P.n_lm + 1; break;
    case OKVIS_BA_LIST_LM_PAIR_BEGIN: src = at((const void*)P.lm_pair_begin), count = P.n_lm + 1; break;
    case OKVIS_BA_LIST_PAIR_LM: src = at((const void*)P.pair_lm), count = P.n_pair; break;
    case OKVIS_BA_LIST_PAIR_BLOCK: src = at((const void*)P.pair_block), count = P.lin2 ? P.n_pair : 0; break;
    case OKVIS_BA_LIST_PAIR_OFF: src = at((const void*)P.pair_off), count = P.n_pair; break;
    case OKVIS_BA_LIST_PAIR_ROLE: src = at((const void*)P.pair_role), count = P.n_pair; break;
    case OKVIS_BA_LIST_LM_PIECE_BEGIN: src = at((const void*)P.lm_piece_begin), count = P.lin2 ? P.n_lm + 1 : 0; break;
    case OKVIS_BA_LIST_PAIR_PIECE: src = at((const void*)P.pair_piece), count = P.lin2 ? P.n_pair : 0; break;
    case OKVIS_BA_LIST_PAIR_LIST_BEGIN: src = at((const void*)P.pair_list_begin), count = P.n_pair + 1; break;
    case OKVIS_BA_LIST_PAIR_LIST:
      src = at((const void*)P.pair_list), width = 2;
      count = reinterpret_cast<const int*>(at((const void*)P.pair_list_begin))[P.n_pair];
      break;
    case OKVIS_BA_LIST_TASKS: src = at((const void*)P.tasks), count = 6 * (int64_t)P.n_task; break;
    case OKVIS_BA_LIST_TASK_LIST: {
      src = at((const void*)P.task_list), width = 2;
      const Group* g = reinterpret_cast<const Group*>(at((const void*)P.groups));
      count = P.n_group ? g[P.n_group - 1].tlist_end : 0;
      break;
    }
    case OKVIS_BA_LIST_CHUNKS: src = at((const void*)P.chunks), count = 2 * (int64_t)P.n_chunk; break;
    case OKVIS_BA_LIST_CHUNK_DIAG_BEGIN: src = at((const void*)P.chunk_diag_begin), count = (int64_t)P.n_chunk * nb + 1; break;
    case OKVIS_BA_LIST_CHUNK_DIAG_OUT:
      src = at((const void*)P.chunk_diag_out);
      count = reinterpret_cast<const int*>(at((const void*)P.chunk_diag_begin))[(size_t)P.n_chunk * nb];
      break;
    case OKVIS_BA_LIST_CHUNK_DESC: src = at((const void*)P.chunk_desc), count = (int64_t)P.n_chunk * SCHUR_DESC_INTS; break;
    case OKVIS_BA_LIST_PIECE_PATH: count = 1; break;
    case OKVIS_BA_LIST_LDL_COMP: count = 1; break;
    case OKVIS_BA_LIST_CHAIN: count = 1; break;
    case OKVIS_BA_LIST_CHUNK_RECS: {
      size_t off = 0;
      const int stride = build_chunk_records(A, &H, 1, &off);   // (appends to the arena: the lists above stay where they are)
      src = A.host.data() + off, count = (int64_t)stride * SCHUR_REC_INTS;
      break;
    }
    case OKVIS_BA_LIST_GROUP_RECS: {
      size_t off = 0;
      const int stride = build_group_records(A, &H, 1, &off);   // (appends to the arena too)
      src = A.host.data() + off, count = (int64_t)stride * LIN_REC_INTS;
      break;
    }
    case OKVIS_BA_LIST_PLAN: {
      // the launch plan of a batch of n_windows windows shaped like this one (host only: make_plan on what the index build says)
      size_t off = 0;
      BatchMax M = batch_max(&H, &H.ptrs, 1);
      M.rec_stride = build_chunk_records(A, &H, 1, &off);
      M.grec_stride = build_group_records(A, &H, 1, &off);
      const LaunchPlan p = make_plan(L, M, o, n_windows);
      plan_ints = {p.three, p.rides, p.small_iter.k == SMALL_PREPARE, p.budget, p.fused, p.solve.k, graph_key(10, false), graph_key(10, true)};
      src = plan_ints.data(), count = (int64_t)plan_ints.size();
      break;
    }
    default: return OKVIS_BA_ERR_ARG;
  }
  *n = count;
  if (capacity < count) return OKVIS_BA_ERR_ARG;
  if (which == OKVIS_BA_LIST_PIECE_PATH) {
    out[0] = P.lin2;
  } else if (which == OKVIS_BA_LIST_LDL_COMP) {
    out[0] = (int32_t)P.ldl_comp;
  } else if (which == OKVIS_BA_LIST_CHAIN) {
    out[0] = P.chain;
  } else if (width == 4) {
    if (count) std::memcpy(out, src, 4 * (size_t)count);
  } else {
    const uint16_t* s16 = static_cast<const uint16_t*>(src);
    for (int64_t i = 0; i < count; ++i) out[i] = s16[i];
  }
  return OKVIS_BA_OK;
}

// the containers take over the values the device holds
static int refresh_mirrors(okvis_ba_solver* s) {
  if (s->host.mirror_fresh) return OKVIS_BA_OK;
  for (size_t i = 0; i < s->wins.size(); ++i) {
    const unsigned char* rec = nullptr;
    if (int rc = stage_results(s, (int)i, &rec)) return rc;
    if (rec) s->mirrors[i].take_results(rec, s->host.evaluated);
  }
  s->host.containers_match(true);
  return OKVIS_BA_OK;
}

int okvis_ba_patch_window(okvis_ba_solver* s, int w, const okvis_ba_patch* p) {
  if (int rc = enter(s, ENTER_MARG_FIRST | ENTER_UPLOADED | ENTER_WINDOW | ENTER_DEVICE, w, p != nullptr,
                     s && s->patchable && s->mirrors.size() == s->wins.size()))
    return rc;
  SectionTimer tm;
  auto PT = [&](const char* name) { tm.lap(name); };
  if (int rc = refresh_mirrors(s)) return rc;
  PT("patch: values from the device");
  // All or nothing.  The edit is applied to a COPY of window w's container; the solver's own container only changes (one swap,
  // which cannot throw) after the edited window has been indexed and uploaded.  Whatever fails before that — a rejected patch, a
  // structure limit, an allocation, the device — leaves the containers as they were; if the device no longer holds the old
  // windows (a failed upload has dropped them), they are uploaded again from the untouched containers.
  WindowStore& after = s->mirror_edit;   // (kept between calls: the copy reuses its storage)
  bool upload_started = false;
  int rc = OKVIS_BA_OK;
  try {
    after = s->mirrors[w];
    PT("patch: copy of the container");
    rc = after.apply(*p);   // (checks the whole patch before it touches `after`; `after` is discarded on failure anyway)
    PT("patch: edit");
    if (rc == OKVIS_BA_OK) {
      std::vector<okvis_ba_window> views(s->mirrors.size());
      for (size_t i = 0; i < s->mirrors.size(); ++i) ((int)i == w ? after : s->mirrors[i]).view(&views[i]);
      upload_started = true;
      rc = upload_impl(s, (int)views.size(), views.data());
      PT("patch: index + upload");
    }
  } catch (const std::bad_alloc&) {
    rc = OKVIS_BA_ERR_ARG;
  }
  if (rc != OKVIS_BA_OK) {
    if (upload_started && !s->host.uploaded) {   // the old windows back on the device (the containers still hold them)
      try {
        std::vector<okvis_ba_window> views(s->mirrors.size());
        for (size_t i = 0; i < s->mirrors.size(); ++i) s->mirrors[i].view(&views[i]);
        (void)upload_impl(s, (int)views.size(), views.data());
      } catch (const std::bad_alloc&) {
      }
    }
    // (after a successful re-upload the device holds exactly what the containers hold)
    s->host.containers_match(s->host.uploaded);
    return rc;
  }
  std::swap(s->mirrors[w], after);   // (moves of vectors: cannot throw)
  s->host.containers_match(true);   // the device holds exactly what the containers hold
  return OKVIS_BA_OK;
}

int okvis_ba_set_marg_prior_values(okvis_ba_solver* s, int w, const double* J, const double* e0) {
  if (int rc = enter(s, ENTER_UPLOADED | ENTER_NO_MARG | ENTER_WINDOW, w, J && e0)) return rc;
  HostWin& H = s->wins[w];
  const int Dm = H.marg_dim;
  if (Dm <= 0) return OKVIS_BA_ERR_ARG;
  HIP_TRY(hipSetDevice(s->device));
  // J | H0 | e0 sit behind one another in the arena (each on its 256-byte boundary): one staged image of that span, one copy
  const uintptr_t aJ = reinterpret_cast<uintptr_t>(H.ptrs.marg_J), aH0 = reinterpret_cast<uintptr_t>(H.ptrs.marg_H0),
                  ae0 = reinterpret_cast<uintptr_t>(H.ptrs.marg_e0);
  unsigned char* const dJ = reinterpret_cast<unsigned char*>(aJ);
  const size_t o_H0 = (size_t)(aH0 - aJ), o_e0 = (size_t)(ae0 - aJ);
  const size_t nJ = 8 * (size_t)Dm * Dm, span = o_e0 + 8 * (size_t)Dm;
  if (!(nJ <= o_H0 && o_H0 + nJ <= o_e0)) return OKVIS_BA_ERR_STATE;   // (the layout build_window gives them)
  try {
    if (s->stage_marg_vals.size() < span) s->stage_marg_vals.resize(span);
  } catch (const std::bad_alloc&) {
    return OKVIS_BA_ERR_ARG;
  }
  unsigned char* h = s->stage_marg_vals.data();
  // (the staging of the previous call must have been read: an event behind its copy, long reached in the steady state)
  if (!s->ev_marg_vals) HIP_TRY(hipEventCreateWithFlags(&s->ev_marg_vals, hipEventDisableTiming));
  else HIP_TRY(hipEventSynchronize(s->ev_marg_vals));
  std::memcpy(h, J, nJ);
  if (!H.h0_on_device) {
    double* H0 = reinterpret_cast<double*>(h + o_H0);
    std::memset(H0, 0, nJ);
    marg_h0_host(J, Dm, H0);
  }
  std::memcpy(h + o_e0, e0, 8 * (size_t)Dm);
  if (H.h0_on_device) {   // (H0 stays where it is and is formed again on the device behind the copy)
    HIP_TRY(hipMemcpyAsync(dJ, h, nJ, hipMemcpyHostToDevice, s->stream));
    HIP_TRY(hipMemcpyAsync(dJ + o_e0, h + o_e0, 8 * (size_t)Dm, hipMemcpyHostToDevice, s->stream));
    HIP_TRY(launch_marg_h0(s, w, Dm));
  } else {
    HIP_TRY(hipMemcpyAsync(dJ, h, span, hipMemcpyHostToDevice, s->stream));
  }
  HIP_TRY(hipEventRecord(s->ev_marg_vals, s->stream));
  if (s->patchable && (size_t)w < s->mirrors.size()) {   // the container holds what the device holds
    try {
      s->mirrors[w].marg_J.assign(J, J + (size_t)Dm * Dm);
      s->mirrors[w].marg_e0.assign(e0, e0 + Dm);
    } catch (const std::bad_alloc&) {
      s->mirrors.clear();   // (no container any more: the next patch is refused and the caller uploads)
      s->host.containers_match(false);
    }
  }
  s->host.prior_values_replaced();
  return OKVIS_BA_OK;
}

int okvis_ba_patched_view(okvis_ba_solver* s, int w, okvis_ba_window* out) {
  // (the window index is one of the containers: as many as uploaded windows once the state check has passed)
  if (int rc = enter(s, ENTER_WINDOW, w, out != nullptr, s && s->patchable && s->mirrors.size() == s->wins.size() && !s->mirrors.empty())) return rc;
  if (s->host.uploaded) {
    HIP_TRY(hipSetDevice(s->device));
    if (int rc = refresh_mirrors(s)) return rc;
  }
  s->mirrors[w].view(out);
  return OKVIS_BA_OK;
}
