// Part of ba_capi.hip (see capi_solver.inc).  The index build: everything okvis_ba_upload / okvis_ba_patch_window / okvis_ba_check_window
// derive from a window description on the host — the arrays that replace okvis::ceres::Map's pointer graph (groups, pieces, pairs,
// chunks, Schur tile lists, IMU / prior assembly lists, the solver layouts) appended to the arena as OFFSETS.
// build_window is the list of its stages, member functions of one BuildCtx that carries what a stage derives to the ones behind it:
//   check_window_args (ba_store.hpp, shared with the window container) + check_build_limits: every argument check that is not part
//     of the observation walk, before anything is read through an index.  So the order of precedence of the status is: a malformed
//     argument (OKVIS_BA_ERR_ARG), what only the index build requires (limits: OKVIS_BA_ERR_UNSUPPORTED; samples: _ARG), the size
//     of the reduced system, then the observation walk, where the first offending observation decides, in list order;
//   ordering, observations (records written in place, pairs), form_groups (with the piece layout), lists_pieces OR lists_staged,
//   form_chunks, imu_colouring, prior_h0, layout (chain fit, ldl_comp, fuse_fast, sizes);
//   the arena in its order: put_lists, put_imu_tables, put_zeroed, put_caller_arrays; host_record (sizes, algorithmic bytes).
// The order of the put / put_n / put_zero calls IS the arena layout.
namespace {

// ---------------------------------------------------------------------------------------------------
// structure building for one window; appends into the arena and fills HostWin/WinPtrs with OFFSETS
// (converted to device pointers after the arena is allocated).
// ---------------------------------------------------------------------------------------------------
template <class T>
size_t put(Arena& A, const std::vector<T>& v) {
  size_t off = A.alloc(std::max<size_t>(v.size(), 1) * sizeof(T));
  // (the staging buffer keeps its size from upload to upload: in steady state nothing is value-initialised here, the bytes are
  // written once by the copy below; the alignment gaps between arrays carry whatever they carried and are never read)
  if (A.host.size() < A.size) A.host.resize(A.size + A.size / 2, 0);
  if (!v.empty()) std::memcpy(A.host.data() + off, v.data(), v.size() * sizeof(T));
  else std::memset(A.host.data() + off, 0, sizeof(T));
  return off;
}
size_t put_zero(Arena& A, size_t bytes) { return A.zalloc(std::max<size_t>(bytes, 8)); }
// a caller's array straight into the arena (n elements; a null pointer or n = 0 leaves one zeroed element, like an empty vector)
template <class T>
size_t put_n(Arena& A, const T* p, size_t n) {
  if (!p) n = 0;
  size_t off = A.alloc(std::max<size_t>(n, 1) * sizeof(T));
  if (A.host.size() < A.size) A.host.resize(A.size + A.size / 2, 0);
  if (n) std::memcpy(A.host.data() + off, p, n * sizeof(T));
  else std::memset(A.host.data() + off, 0, sizeof(T));
  return off;
}

#define OFF(field, off) P.field = reinterpret_cast<std::remove_reference<decltype(P.field)>::type>(off)

// diagnostics: OKVIS_BA_DEBUG=build accumulates the host time of build_window's sections and prints them at exit
struct BuildTimes {
  bool on = debug_word().build;
  struct Acc {   // (`+=` keeps the call sites of the mean-only version)
    std::vector<double> v;
    Acc& operator+=(double x) {
      v.push_back(x);
      return *this;
    }
  };
  std::map<std::string, Acc> ms;
  long calls = 0;
  ~BuildTimes() {
    if (!on || !calls) return;
    std::fprintf(stderr, "build_window: %ld calls, median ms per section (number of samples):", calls);
    for (auto& kv : ms) {
      std::vector<double>& v = kv.second.v;
      if (v.empty()) continue;
      std::sort(v.begin(), v.end());
      std::fprintf(stderr, "  %s %.4f (%zu)", kv.first.c_str(), v[v.size() / 2], v.size());
    }
    std::fprintf(stderr, "\n");
  }
};
BuildTimes g_build_times;
// the host time since the previous mark (or the start of the call) goes to the named section
struct BuildTimer {
  std::chrono::steady_clock::time_point t0;
  BuildTimer() {
    if (!g_build_times.on) return;
    g_build_times.calls++;
    t0 = std::chrono::steady_clock::now();
  }
  void mark(const char* name) {
    if (!g_build_times.on) return;
    const auto t = std::chrono::steady_clock::now();
    g_build_times.ms[name] += std::chrono::duration<double, std::milli>(t - t0).count();
    t0 = t;
  }
};

constexpr int GROUP_LM_DEFAULT = 32;   // landmarks the index build puts into one linearise group (see build_window) ...
constexpr int GROUP_LM_FEW = 16, GROUP_LM_FEW_WINDOWS = 8;   // ... and when at most this many windows share the device
constexpr int H0_DEVICE_MIN = 128;   // rows of a marginalisation prior from which H0 = J^T J is formed on the device

// H0 = J^T J of window blockIdx.y's prior, one entry per work-item, the terms of an entry added in row order and without
// contraction into fused multiply-adds: bit for bit what build_window computes on the host for the small priors
__global__ __launch_bounds__(256) void marg_h0_kernel(const WinPtrs* __restrict__ wins, int w0) {
  const WinPtrs& W = wins[w0 + blockIdx.y];
  const int Dm = W.marg_dim;
  const size_t k = (size_t)blockIdx.x * 256 + threadIdx.x;
  if (Dm <= H0_DEVICE_MIN || k >= (size_t)Dm * Dm) return;
  const int i = (int)(k / Dm), j = (int)(k - (size_t)i * Dm);
  const int lo = i < j ? i : j, hi = i < j ? j : i;   // (the host fills the upper triangle and mirrors it)
  const BA_G double* J = W.marg_J;
  double sacc = 0.0;
  {
#pragma clang fp contract(off)   // (the host's index build has no fused multiply-add: product and sum are rounded separately)
    for (int r = 0; r < Dm; ++r) {
      const double pr = J[(size_t)r * Dm + lo] * J[(size_t)r * Dm + hi];
      sacc = sacc + pr;
    }
  }
  const_cast<BA_G double*>(W.marg_H0)[k] = sacc;
}

// Work vectors of build_window, one set per host thread, kept between calls (capacity only: every call assigns what it reads)
struct BuildScratch {
  // destination of every entry of the IMU factors' H | g records (BuildCtx::put_imu_tables).  The tables only depend on where the terms'
  // blocks sit in the reduced system: a window that slides keeps them from frame to frame (9 us of a 70 us upload).  Four
  // entries, replaced in turn: the estimator alternates between the window it optimises and the sub-window it marginalises.
  struct ImuAsmCache {
    int D = -1, Dp = -1, chain = -1;
    std::vector<int> coloff, color;
    std::vector<int4> table;
    std::vector<int> fastw, pos;
  } asm_caches[4];
  int asm_next = 0;
  // block -> observations of the current group (own role), staged path.  Every list is left empty: the lists grow to a few hundred
  // entries each, once, instead of through ten reallocations per block in every upload
  std::vector<std::vector<uint16_t>> blk_obs;
  std::vector<int> pose_off, sb_off, role, lm_obs_begin, pair_lm, pair_block, pair_off, pair_role, lm_pair_begin, blocks, seen;
  std::vector<int> chunk_diag_begin, chunk_diag_out, chunk_cross_begin, chunk_cross, chunk_desc, blk_cursor;
  std::vector<int> pair_list_begin, blk_slot, touched, lm_piece_begin, pair_piece, blk_cnt;
  std::vector<uint16_t> pair_list, task_list;
  std::vector<Group> groups;
  std::vector<Task> tasks;
  std::vector<Chunk> chunks;
};
BuildScratch& build_scratch() {
  static thread_local BuildScratch S;
  return S;
}

// H0 = J^T J on the host (H0 zeroed by the caller): the upper triangle as a sum of row outer products, then mirrored
inline void marg_h0_host(const double* J, int Dm, double* H0) {
  for (int r = 0; r < Dm; ++r) {
    const double* Jr = J + (size_t)r * Dm;
    for (int i = 0; i < Dm; ++i) {
      const double a = Jr[i];
      if (a == 0.0) continue;   // (J of the reference's prior is upper triangular up to the rank: 0 * x adds nothing)
      double* Hi = H0 + (size_t)i * Dm;
      for (int j = i; j < Dm; ++j) Hi[j] += a * Jr[j];
    }
  }
  for (int i = 0; i < Dm; ++i)
    for (int j = i + 1; j < Dm; ++j) H0[(size_t)j * Dm + i] = H0[(size_t)i * Dm + j];
}

// Internal status of build_window(lin2 = true): the window does not fit the piece path of the linearise launch
// (ba_linearize2.hpp: free extrinsics, or one landmark with more than LIN2_PIECES pieces); the caller rebuilds the batch
// for ba_linearize.hpp.
constexpr int BW_LIN2_UNFIT = -1000;
// ... (chain = true): the window's speed/bias blocks do not form a chain in the order of the reduced system, or the chain solver
// does not pay for it (okvis_ba_upload then lays the whole batch out for the dense LDL^T)
constexpr int BW_CHAIN_UNFIT = -1001;
// OKVIS_BA_SOLVE_AUTO: the chain solver from this many speed/bias blocks on.  Measured (tools/gpu_chain_shapes.py, device ticks of
// one solve, chain / dense): 10 poses + 10 blocks 0.92, 12 + 10: 0.93, 10 + 8: 0.96, 10 + 6: 0.97, 10 + 5: 1.06, 10 + 3: 1.12,
// 8 + 3 (the sliding window of the replay): 1.32 — two sweeps, the pose system's update and the back-substitution are fixed costs
// that a short chain does not earn back.
constexpr int CHAIN_AUTO_MIN_BLOCKS = 8;

// The layout a batch of n_windows asks for under the options o (BatchLayout), before any window is looked at
BatchLayout batch_layout(const okvis_ba_options& o, int n_windows) {
  BatchLayout L;
  // the piece path unless options.reserved0 bit 3 asks for the staged kernel; the chain solve where the options allow it (every
  // LDS-resident window then needs at least chain_min speed/bias blocks in a chain)
  L.lin2 = !(o.reserved0 & 8);
  L.chain = o.tuning.solve_mode != OKVIS_BA_SOLVE_DENSE;
  L.chain_min = o.tuning.solve_mode == OKVIS_BA_SOLVE_CHAIN ? 1 : CHAIN_AUTO_MIN_BLOCKS;
  // fused mode (the linearise workgroup reduces its own group, no Schur launch: DOGLEG and fixed-radius runs) up to
  // fused_max_windows; options.reserved0 bit 2 keeps the separate launch (A/B switch)
  L.fuse = !(o.reserved0 & 4) && o.schur_lm_per_block == 0 && n_windows <= fused_max_windows(o) && decision_free(o);
  L.spec = !(o.tuning.flags & OKVIS_BA_TUNE_SCHUR_DECIDES) && schur_mfma_allowed(o) && o.schur_lm_per_block == 0 && decision_free(o);
  // landmarks per Schur workgroup: 48 (three staged batches of 16) keeps the workgroup count low when many windows share
  // the device; a few windows have the device to themselves and finish sooner with 32 (measured, tools/gpu_chunk_diag.py:
  // one window 114.7 vs 119.7 us per iteration, 64 windows 239 vs 217)
  L.schur_lm = std::min(o.schur_lm_per_block > 0 ? o.schur_lm_per_block : (n_windows <= 8 ? 16 : n_windows < SMALL_BATCH_WINDOWS ? 32 : n_windows < 128 ? 48 : 64), SCHUR_CHUNK_LM_MAX);   // (round 4 sweep with the matrix-core kernel, 64 windows: 12: 382 k, 24: 436 k, 48: 448 k, 64: 448 k it/s; 256 windows: 48: 585 k, 64: 597 k)
  // Landmarks per group: GROUP_LM (64) is what the kernels hold; the index build fills 32, and 16 when at most GROUP_LM_FEW_WINDOWS
  // windows share the device.  A group of 64 short tracks (landmarks that entered the window with the last frame or two: 2 - 4
  // observations each) is the slowest workgroup of its launch — the landmark elimination loops over the landmarks of the group —
  // and OKVIS hands its landmark ids out in increasing order, so a real window has its short tracks side by side at the end.
  // Measured (profiles/r04_notes.md; windows whose groups close at 256 observations first — configs[1]: 12 landmarks per group —
  // are not touched): one 8-frame window in age order 77.3 us per iteration with 64, 69.0 with 32 (= random order); batches of
  // short-track windows (8 frames, 430 landmarks, 8 observations each), us per step with 64 / 32 / 24 / 16 landmarks per group:
  // 1 window 68.7 / 68.9 / 65.5 / 64.3, 8: 72.1 / 72.3 / 69.0 / 68.6, 64: 124.8 / 125.5 / 115.1 / 121.1, 256: 302 / 304 / 304 / 331;
  // the replay's ten iterations per frame 0.830 (ids by first sighting) / 0.817 / 0.785 / 0.783 ms.  okvis_ba_tuning::group_lm overrides.
  L.group_lm = std::max(1, std::min(o.tuning.group_lm > 0 ? o.tuning.group_lm : (n_windows <= GROUP_LM_FEW_WINDOWS ? GROUP_LM_FEW : GROUP_LM_DEFAULT), GROUP_LM));
  // IMU / prior factors in a launch of their own when the batch fills the device (then four linearise workgroups share a
  // CU); one launch for everything when a few windows wait for one another's latency
  L.split_small = n_windows >= (o.tuning.split_small_min > 0 ? o.tuning.split_small_min : SMALL_BATCH_WINDOWS);
  L.fp32 = o.fp32_linearize != 0;
  return L;
}

// What only the index build requires of a window that check_window_args (ba_store.hpp) has passed, and what needs no derived
// quantity: checked in front of the first use of what it guards
int check_build_limits(const okvis_ba_window& w) {
  if (w.n_obs && (!w.obs_lm || !w.obs_pose || !w.obs_ext || !w.obs_cam || !w.obs_uv || !w.obs_sqrtw || !w.cam_intr ||
                  !w.cam_model))
    return OKVIS_BA_ERR_ARG;
  if (w.n_pose > 65535 || w.n_lm >= (1 << 24) || w.n_cam > 255) return OKVIS_BA_ERR_UNSUPPORTED;
  for (int f = 0; f < w.n_imu; ++f) {
    if (w.imu_s_count[f] < 2) return OKVIS_BA_ERR_ARG;
    if (w.imu_s_count[f] > MAX_IMU_SAMPLES) return OKVIS_BA_ERR_UNSUPPORTED;
    // ImuError::redoPreintegration returns -1 when the samples do not cover [t0,t1] (ImuError.cpp:87-89)
    if (!(w.imu_s_t[w.imu_s_begin[f] + w.imu_s_count[f] - 1] >= w.imu_t1[f])) return OKVIS_BA_ERR_ARG;
  }
  if (w.marg_dim > MAX_MARG_DIM) return OKVIS_BA_ERR_UNSUPPORTED;
  for (int b = 1; b < (w.marg_dim > 0 ? w.marg_nblocks : 0); ++b)
    if (w.marg_block_off[b] <= w.marg_block_off[b - 1]) return OKVIS_BA_ERR_ARG;
  if (w.imu_sb_ref && w.imu_sb_ref_valid)
    for (int f = 0; f < w.n_imu; ++f) {
      // (the rule of WindowStore::assign: a window a patchable solver refuses is refused here as well)
      if (w.imu_sb_ref_valid[f] > 2 || (w.imu_sb_ref_valid[f] == 2 && !w.imu_cache)) return OKVIS_BA_ERR_ARG;
      if (w.imu_sb_ref_valid[f] != 2) continue;
      ImuCacheD rec;   // the preintegration itself (okvis_ba_fetch_imu_caches): taken as it stands by BuildCtx::put_caller_arrays
      std::memcpy(&rec, w.imu_cache + (size_t)OKVIS_BA_IMU_CACHE_DOUBLES * f, sizeof(ImuCacheD));
      if (rec.valid != 1) return OKVIS_BA_ERR_ARG;   // (a record of a term that was never evaluated)
      for (int k = 0; k < 225; ++k)
        if (!std::isfinite(rec.sqrt_info[k])) return OKVIS_BA_ERR_ARG;
      for (int k = 0; k < 4; ++k)
        if (!std::isfinite(rec.Delta_q[k])) return OKVIS_BA_ERR_ARG;
    }
  return OKVIS_BA_OK;
}

// What the stages of build_window share: the arguments, and what a stage derives for the stages behind it (named with the stage
// that sets it).  The index lists themselves live in BuildScratch.
struct BuildCtx {
  const okvis_ba_window& w;
  const okvis_ba_options& opt;
  const BatchLayout& lay;
  Arena& A;
  HostWin& H;
  WinPtrs& P;        // = H.ptrs; the pointer members hold arena OFFSETS until relocate()
  BuildScratch& S;   // (one set of vectors per host thread: a frame's upload allocates nothing once they have grown)
  std::vector<int>&pose_off, &sb_off, &lm_obs_begin, &lm_pair_begin, &pair_block;   // (of S: read by most stages)
  std::vector<Group>& groups;
  std::vector<Task>& tasks;
  const bool lin2;
  const int npose, nsb, nlm, nobs;
  int D = 0, Dp = 0;                      // ordering
  int npair = 0;                          // observations
  bool has_ext = false;
  int ngroup = 0;                         // form_groups
  int gpart_size = 0;                     // lists_pieces / lists_staged
  int nchunk = 0;                         // form_chunks
  int n_imu_color = 0;                    // imu_colouring
  std::vector<int> imu_color, imu_order, imu_color_begin, imu_coloff;
  int Dm = 0, nmb = 0;                    // prior_h0
  std::vector<double> H0;
  int ntile = 1, spart_stride = 0;        // layout
  bool use_chain = false;
  BuildCtx(const okvis_ba_window& w_, const okvis_ba_options& opt_, const BatchLayout& lay_, Arena& A_, HostWin& H_)
      : w(w_), opt(opt_), lay(lay_), A(A_), H(H_), P(H_.ptrs), S(build_scratch()), pose_off(S.pose_off), sb_off(S.sb_off),
        lm_obs_begin(S.lm_obs_begin), lm_pair_begin(S.lm_pair_begin), pair_block(S.pair_block), groups(S.groups), tasks(S.tasks),
        lin2(lay_.lin2), npose(w_.n_pose), nsb(w_.n_sb), nlm(w_.n_lm), nobs(w_.n_obs) {}
  // the stages, in the order build_window runs them
  int ordering();
  int observations();
  int form_groups();
  void lists_reset();
  void lists_pieces();
  void lists_staged();
  void form_chunks();
  void imu_colouring();
  void prior_h0();
  int layout();
  void put_lists();
  int put_imu_tables();
  void put_zeroed();
  void put_caller_arrays();
  void host_record();
};

// ---- reduced ordering: free pose blocks (6 each) then free speed/bias blocks (9 each) ----
int BuildCtx::ordering() {
  pose_off.assign(w.n_pose, -1);
  sb_off.assign(w.n_sb, -1);
  int off = 0;
  for (int i = 0; i < w.n_pose; ++i)
    if (!w.pose_fixed[i]) {
      pose_off[i] = off;
      off += 6;
    }
  Dp = off;
  for (int i = 0; i < w.n_sb; ++i)
    if (!w.sb_fixed[i]) {
      sb_off[i] = off;
      off += 9;
    }
  D = off;
  return (D > MAX_D || D == 0) ? OKVIS_BA_ERR_UNSUPPORTED : OKVIS_BA_OK;
}

// ---- one pass over the observations, landmark by landmark: validation, roles, observation records and the
//      (landmark, free block) pairs ----
int BuildCtx::observations() {
  // (locals and local references, here and in form_groups: their loops are the bulk of the build's time)
  const int npose = w.n_pose, nsb = w.n_sb, nlm = w.n_lm, nobs = w.n_obs;
  std::vector<int>&pose_off = S.pose_off, &sb_off = S.sb_off;
  std::vector<int>&role = S.role, &lm_obs_begin = S.lm_obs_begin;   // role: 0 pose role, 1 extrinsics role
  role.assign(npose, -1);
  lm_obs_begin.resize((size_t)nlm + 1);
  // The arena's first arrays have sizes known by now, so the observation records are written where they stay (the arena is not
  // touched again before the pass below ends; a failed or unfit window's bytes are discarded by the caller).
  std::memset(&P, 0, sizeof(P));
  for (int b = 0; b < 2; ++b) {
    OFF(pose[b], put_n(A, w.pose, 7 * (size_t)npose));
    OFF(sb[b], put_n(A, w.sb, 9 * (size_t)nsb));
    OFF(lm[b], put_n(A, w.lm, 4 * (size_t)nlm));
  }
  OFF(pose_off, put(A, pose_off));
  OFF(sb_off, put(A, sb_off));
  OFF(cam_intr, put_n(A, w.cam_intr, 12 * (size_t)w.n_cam));
  OFF(cam_model, put_n(A, w.cam_model, (size_t)w.n_cam));
  const size_t recs_off = put_n(A, (const ObsRec*)nullptr, 0);   // (an empty array's single zeroed element ...)
  if (nobs > 1) {                                                // (... grown to n_obs records)
    A.size = recs_off + (size_t)nobs * sizeof(ObsRec);
    if (A.host.size() < A.size) A.host.resize(A.size + A.size / 2, 0);
  }
  OFF(obs, recs_off);
  ObsRec* const recs = reinterpret_cast<ObsRec*>(A.host.data() + recs_off);
  std::vector<int>&pair_lm = S.pair_lm, &pair_block = S.pair_block, &pair_off = S.pair_off, &pair_role = S.pair_role, &lm_pair_begin = S.lm_pair_begin;
  int npair_run = 0;   // (the pair vectors are work space of at least 2 n_obs entries: the first npair_run are this window's)
  lm_pair_begin.resize((size_t)nlm + 1);
  bool has_ext = false;
  {
    const size_t guess = 2 * (size_t)nobs;
    if (pair_lm.size() < guess) pair_lm.resize(guess), pair_block.resize(guess), pair_off.resize(guess), pair_role.resize(guess);
    int *const pl = pair_lm.data(), *const pb = pair_block.data(), *const po = pair_off.data(), *const pr = pair_role.data();
    std::vector<int>&blocks = S.blocks, &seen = S.seen;   // a "seen for this landmark" stamp per block
    seen.assign(npose, -1);
    if ((int)blocks.size() < npose + 2) blocks.resize((size_t)npose + 2);   // (a landmark's blocks are distinct; one slot for the store below)
    int* const bl = blocks.data();
    // what the separate passes of the earlier versions reported after the whole observation list had been checked
    bool obs_over = false, pairs_over = false;
    const unsigned unpose = (unsigned)npose, uncam = (unsigned)w.n_cam;
    int o = 0;
    for (int l = 0; l < nlm; ++l) {
      const int o0 = o;
      lm_obs_begin[l] = o0;
      int nb = 0, last = -1;         // blocks of this landmark so far, the last one taken
      bool ascending = true;
      int prev_ip = -1, prev_c = -1;
      // (the tests that depend on the data — same pose as the observation before? a block not seen yet? — are arithmetic, not
      // branches: they fail to predict about once per observation)
      for (; o < nobs && w.obs_lm[o] == l; ++o) {
        const int ip = w.obs_pose[o], ie = w.obs_ext[o], c = w.obs_cam[o];
        if ((int)((unsigned)ip >= unpose) | (int)((unsigned)ie >= unpose) | (int)((unsigned)c >= uncam)) return OKVIS_BA_ERR_ARG;
        // sorted by (landmark, pose, cam); REPEATED (landmark, pose, cam) entries are legal: the reference adds one residual
        // block per matched keypoint (implementation/Estimator.hpp:52-56 only rejects an identical KeypointIdentifier)
        if ((int)(prev_ip > ip) | ((int)(prev_ip == ip) & (int)(prev_c > c))) return OKVIS_BA_ERR_ARG;  // unsorted
        if ((int)(role[ip] == 1) | (int)(role[ie] == 0) | (int)(ip == ie)) return OKVIS_BA_ERR_UNSUPPORTED;
        role[ip] = 0;
        role[ie] = 1;
        ObsRec& R = recs[o];
        R.lm_cam = (uint32_t)l | ((uint32_t)c << 24);
        R.pose = (uint16_t)ip;
        R.ext = (uint16_t)ie;
        R.u = w.obs_uv[2 * o];
        R.v = w.obs_uv[2 * o + 1];
        R.sw = w.obs_sqrtw[o];
        // a landmark's observations are sorted by pose and no block has both roles: a pose-role block is new exactly when the
        // pose index changes; an extrinsics block needs the stamp
        const int newp = (int)(ip != prev_ip) & (int)(pose_off[ip] >= 0);
        ascending &= !(newp & (int)(ip < last));
        bl[nb] = ip;
        nb += newp;
        last = newp ? ip : last;
        prev_ip = ip;
        prev_c = c;
        if (pose_off[ie] >= 0) {
          has_ext = true;
          if (seen[ie] != l) {
            seen[ie] = l;
            if (ie < last) ascending = false;
            bl[nb++] = ie;
            last = ie;
          }
        }
      }
      if (o - o0 > GROUP_OBS) obs_over = true;
      if (!ascending) std::sort(bl, bl + nb);   // (only extrinsics blocks can come out of order)
      lm_pair_begin[l] = npair_run;
      for (int k = 0; k < nb; ++k) {
        const int b = bl[k];
        pl[npair_run] = l;
        pb[npair_run] = b;
        po[npair_run] = pose_off[b];
        pr[npair_run] = role[b];
        ++npair_run;
      }
      // (the earlier version stopped at the first landmark with too many blocks; an unsorted or out-of-range observation
      // further on still comes first, see below)
      if (nb > GROUP_PAIRS) pairs_over = true;
    }
    lm_obs_begin[nlm] = o;
    // an observation the walk did not consume names a landmark out of range or before its predecessor's
    if (o < nobs) return OKVIS_BA_ERR_ARG;
    if (obs_over) return OKVIS_BA_ERR_UNSUPPORTED;
    if (lin2 && has_ext) return BW_LIN2_UNFIT;
    if (pairs_over) return OKVIS_BA_ERR_UNSUPPORTED;
  }
  lm_pair_begin[nlm] = npair_run;
  npair = npair_run;
  this->has_ext = has_ext;
  return OKVIS_BA_OK;
}

// ---- groups, with the piece layout of the piece path ----
int BuildCtx::form_groups() {
  const bool lin2 = lay.lin2;
  const int nlm = w.n_lm, npair = this->npair;
  std::vector<int>&pose_off = S.pose_off, &lm_obs_begin = S.lm_obs_begin, &lm_pair_begin = S.lm_pair_begin;
  std::vector<Group>& groups = S.groups;
  groups.clear();
  // okvis_ba_tuning::group_work (sweeps): a group also closes when the block products of its landmark elimination, sum of
  // pairs (pairs + 1) / 2, reach this number.  Measured (profiles/r04_notes.md): a window that has the device to itself finishes
  // sooner with more, lighter groups (cap 250: replay 0.833 -> 0.805 ms per frame for the ten iterations, one configs[1] window
  // 73.1 -> 72.2 us per iteration), with more windows the additional workgroups cost more than they bring (4 windows: 74 -> 78 us per
  // step, 64: 451 k -> 358 k it/s).  Not the default: the other grouping moves the rounding of every single-window run, and one
  // of the ill-conditioned DOGLEG cases that sit at the 1e-6 bound (test_dogleg_rejected_steps) lands at 1.25e-6.
  const long group_work_cap = opt.tuning.group_work > 0 ? opt.tuning.group_work : 0L;
  // piece path (ba_linearize2.hpp): pieces instead of per-observation lists.  A piece = one or two adjacent observations of the same
  // pose inside one row of 16 lanes, greedy from the start of the run (the rule of linearize2_kernel's phase B).  The pieces of a
  // landmark depend on the lane its first observation takes, i.e. on the group it joins, so they are laid out while the groups
  // are formed: lm_piece_begin[l] = the landmark's first piece in the window, pair_piece[p] = the pair's first piece in its group
  // | its number of pieces << 16, per group the pieces before waves 1..3.
  std::vector<int>&lm_piece_begin = S.lm_piece_begin, &pair_piece = S.pair_piece;
  if (lin2) {
    lm_piece_begin.resize((size_t)nlm + 1);
    pair_piece.resize((size_t)npair + 1);   // (one more: where the pieces of fixed poses count)
  }
  {
    int l = 0;
    int piece_total = 0;
    int* const ppc = pair_piece.data();
    while (l < nlm) {
      Group G;
      G.lm_begin = l;
      G.obs_begin = lm_obs_begin[l];
      G.pair_begin = lm_pair_begin[l];
      int no = 0, np = 0, nl = 0, npc = 0;
      int wave_count[4] = {0, 0, 0, 0};
      long work = 0;   // block products of the group's landmark elimination: sum of pairs (pairs + 1) / 2
      while (l < nlm) {
        const int o0 = lm_obs_begin[l], o1 = lm_obs_begin[l + 1], p0 = lm_pair_begin[l], p1 = lm_pair_begin[l + 1];
        const int lo = o1 - o0, lp = p1 - p0;
        if (group_work_cap > 0 && nl > 0 && work + (long)lp * (lp + 1) / 2 > group_work_cap) break;
        if (nl > 0 && (no + lo > GROUP_OBS || np + lp > GROUP_PAIRS || nl + 1 > lay.group_lm)) break;
        int lpc = 0;
        int wc[4] = {0, 0, 0, 0};
        if (lin2) {   // piece path: at most LIN2_PIECES pieces per group (a pair has at least one piece)
          // One walk over the landmark's observations; the tests that depend on the data are arithmetic.  An observation opens a
          // piece when it opens a run (new pose, or first lane of a row) or sits at an even place of its run.
          int pnext = p0, cur = npair, prev = -1, par = 0, local = npc;
          int v = 0;   // first piece | pieces << 16 of the pair the walk is in: kept in a register, stored (never re-read) every step
          int w0 = 0, w1 = 0, w2 = 0, w3 = 0;
          for (int o = o0; o < o1; ++o) {
            const int lane = no + (o - o0), pose = w.obs_pose[o];
            const int changed = pose != prev, freeb = pose_off[pose] >= 0;
            cur = changed ? (freeb ? pnext : npair) : cur;   // (the pairs of a landmark are its free poses in this order)
            pnext += changed & freeb;
            const int start = changed | (int)((lane & 15) == 0);
            par = start ? 0 : par ^ 1;
            const int newp = par == 0;
            v = changed ? 0 : v;   // (every pair is entered once: it starts empty)
            v = (newp & (int)((v >> 16) == 0)) ? local : v;
            v += newp << 16;
            ppc[cur] = v;
            const int wv = lane >> 6;
            w0 += newp & (int)(wv == 0), w1 += newp & (int)(wv == 1), w2 += newp & (int)(wv == 2), w3 += newp & (int)(wv == 3);
            local += newp;
            prev = pose;
          }
          wc[0] = w0, wc[1] = w1, wc[2] = w2, wc[3] = w3;
          lpc = local - npc;
          if (nl == 0 && lpc > LIN2_PIECES) return BW_LIN2_UNFIT;
          if (nl > 0 && npc + lpc > LIN2_PIECES) break;   // (the landmark opens the next group and is laid out again from lane 0)
          lm_piece_begin[l] = piece_total + npc;
          for (int k = 0; k < 4; ++k) wave_count[k] += wc[k];
        }
        work += (long)lp * (lp + 1) / 2;
        no += lo;
        np += lp;
        npc += lpc;
        ++nl;
        ++l;
      }
      G.lm_end = l;
      G.obs_end = lm_obs_begin[l];
      G.pair_end = lm_pair_begin[l];
      G.task_begin = G.task_end = 0;
      G.plist_begin = G.plist_end = G.tlist_begin = G.tlist_end = 0;
      G.piece_begin = piece_total;
      G.pw1 = wave_count[0];
      G.pw2 = wave_count[0] + wave_count[1];
      G.pw3 = wave_count[0] + wave_count[1] + wave_count[2];
      if (!lin2) G.piece_begin = 0;
      piece_total += npc;
      groups.push_back(G);
    }
    if (lin2) lm_piece_begin[nlm] = piece_total;
  }
  ngroup = (int)groups.size();
  return OKVIS_BA_OK;
}

// ---- per-group tasks and their lists: empty lists for both paths to start from ----
void BuildCtx::lists_reset() {
  S.pair_list_begin.assign((size_t)npair + 1, 0);
  S.pair_list.clear(), S.task_list.clear(), S.tasks.clear();
  S.pair_list.reserve(2 * (size_t)nobs);
  S.task_list.reserve(3 * (size_t)nobs);
  S.touched.clear();
  gpart_size = 0;
}

// ---- piece path (ba_linearize2.hpp): one task per free block of a group, the slots of its pairs' block records; no
//      per-observation lists ----
void BuildCtx::lists_pieces() {
  lists_reset();
  std::vector<int>& touched = S.touched;
  std::vector<uint16_t>& task_list = S.task_list;
  std::vector<int>& blk_cnt = S.blk_cnt;   // pairs of the current group per block, then the next slot of the block
  blk_cnt.assign(npose, 0);
  for (Group& G : S.groups) {
    G.tlist_begin = (int)task_list.size();
    // tasks: one per free block seen by the group, ascending; its list = the group-local pairs of that block
    G.task_begin = (int)tasks.size();
    touched.clear();
    for (int p = G.pair_begin; p < G.pair_end; ++p) {
      const int b = pair_block[p];
      if (blk_cnt[b]++ == 0) touched.push_back(b);
    }
    std::sort(touched.begin(), touched.end());
    task_list.resize(task_list.size() + (size_t)(G.pair_end - G.pair_begin));
    int slot = 0;
    for (int b : touched) {
      Task T;
      T.type = 0;
      T.off_a = pose_off[b];
      T.off_b = -1;
      // task_list holds, per group-local pair, the SLOT of its block record: the records of one block are contiguous
      // [list_begin, list_end) in slot order (pairs ascending), which is the order they are summed in
      T.list_begin = G.tlist_begin + slot;
      const int n = blk_cnt[b];
      blk_cnt[b] = slot;   // from here on: the slot the block's next pair takes
      slot += n;
      T.list_end = G.tlist_begin + slot;
      T.out = gpart_size;
      gpart_size += 27;
      tasks.push_back(T);
    }
    for (int p = G.pair_begin; p < G.pair_end; ++p) task_list[(size_t)G.tlist_begin + (p - G.pair_begin)] = (uint16_t)blk_cnt[pair_block[p]]++;
    for (int b : touched) blk_cnt[b] = 0;
    G.task_end = (int)tasks.size();
    G.tlist_end = (int)task_list.size();
  }
}

// ---- staged path (ba_linearize.hpp): per-pair observation lists; tasks per block (own role), then one per (pose, extrinsics)
//      pair of free blocks ----
void BuildCtx::lists_staged() {
  lists_reset();
  std::vector<int>&role = S.role, &pair_list_begin = S.pair_list_begin, &touched = S.touched;
  std::vector<uint16_t>&pair_list = S.pair_list, &task_list = S.task_list;
  std::vector<int>& blk_slot = S.blk_slot;              // scratch: block -> pair of the current landmark / task of the group
  blk_slot.assign(npose, -1);
  std::vector<std::vector<uint16_t>>& blk_obs = S.blk_obs;
  if ((int)blk_obs.size() < npose) blk_obs.resize(npose);
  for (auto& v : blk_obs) v.clear();   // (whatever an interrupted call may have left)
  for (Group& G : S.groups) {
    G.plist_begin = (int)pair_list.size();
    G.tlist_begin = (int)task_list.size();
    // per-pair observation lists: one pass over a landmark's observations (two-pass counting fill)
    for (int l = G.lm_begin; l < G.lm_end; ++l) {
      const int p0 = lm_pair_begin[l], p1 = lm_pair_begin[l + 1];
      for (int p = p0; p < p1; ++p) blk_slot[pair_block[p]] = p;
      for (int p = p0; p < p1; ++p) pair_list_begin[p] = 0;
      for (int o = lm_obs_begin[l]; o < lm_obs_begin[l + 1]; ++o) {
        const int pp = blk_slot[w.obs_pose[o]], pe = blk_slot[w.obs_ext[o]];
        if (pp >= 0) ++pair_list_begin[pp];
        if (pe >= 0) ++pair_list_begin[pe];
      }
      int run = (int)pair_list.size();
      for (int p = p0; p < p1; ++p) {
        const int c = pair_list_begin[p];
        pair_list_begin[p] = run;
        run += c;
      }
      pair_list.resize((size_t)run);
      std::vector<int>& cur = touched;   // reuse as the per-pair fill cursor
      cur.assign(p1 - p0, 0);
      for (int o = lm_obs_begin[l]; o < lm_obs_begin[l + 1]; ++o) {
        const int cand[2] = {blk_slot[w.obs_pose[o]], blk_slot[w.obs_ext[o]]};
        for (int c = 0; c < 2; ++c)
          if (cand[c] >= 0) pair_list[(size_t)pair_list_begin[cand[c]] + cur[cand[c] - p0]++] = (uint16_t)(o - G.obs_begin);
      }
      for (int p = p0; p < p1; ++p) blk_slot[pair_block[p]] = -1;
    }
    G.task_begin = (int)tasks.size();
    touched.clear();
    std::map<std::pair<int, int>, std::vector<uint16_t>> cross;  // (pose, ext) -> obs (only with free extrinsics)
    for (int o = G.obs_begin; o < G.obs_end; ++o) {
      const int ip = w.obs_pose[o], ie = w.obs_ext[o];
      const uint16_t lo = (uint16_t)(o - G.obs_begin);
      const int cand[2] = {ip, ie};
      for (int c = 0; c < 2; ++c)
        if (pose_off[cand[c]] >= 0) {
          if (blk_obs[cand[c]].empty()) touched.push_back(cand[c]);
          blk_obs[cand[c]].push_back(lo);
        }
      if (pose_off[ip] >= 0 && pose_off[ie] >= 0) cross[{ip, ie}].push_back(lo);
    }
    std::sort(touched.begin(), touched.end());   // ascending block index, as a std::map would iterate
    for (int b : touched) {
      Task T;
      T.type = role[b];
      T.off_a = pose_off[b];
      T.off_b = -1;
      T.list_begin = (int)task_list.size();
      task_list.insert(task_list.end(), blk_obs[b].begin(), blk_obs[b].end());
      T.list_end = (int)task_list.size();
      T.out = gpart_size;
      gpart_size += 27;
      tasks.push_back(T);
      blk_obs[b].clear();
    }
    for (auto& kv : cross) {
      Task T;
      T.type = 2;
      T.off_a = pose_off[kv.first.first];
      T.off_b = pose_off[kv.first.second];
      T.list_begin = (int)task_list.size();
      task_list.insert(task_list.end(), kv.second.begin(), kv.second.end());
      T.list_end = (int)task_list.size();
      T.out = gpart_size;
      gpart_size += 36;
      tasks.push_back(T);
    }
    G.task_end = (int)tasks.size();
    G.plist_end = (int)pair_list.size();
    G.tlist_end = (int)task_list.size();
  }
  pair_list_begin[npair] = (int)pair_list.size();
}

// ---- chunks (Schur workgroups), their diag / cross lists and descriptors ----
void BuildCtx::form_chunks() {
  std::vector<Chunk>& chunks = S.chunks;
  chunks.clear();
  {
    // fused mode, where the batch allows it: the reduced system is solved in LDS, the pose part is one Schur tile and the
    // reduction's landmark tables fit the observation stage of the linearise kernel; then chunk = group
    const int stage = opt.fp32_linearize ? (has_ext ? LinCfg<true, float>::STAGE_DOUBLES : LinCfg<false, float>::STAGE_DOUBLES)
                                         : (has_ext ? LinCfg<true, double>::STAGE_DOUBLES : LinCfg<false, double>::STAGE_DOUBLES);
    H.group_chunks = lay.fuse && D <= MAX_D_LDS && Dp <= TILE_DIM && 2 * SCHUR_LM_BATCH * 3 * Dp <= stage;
    const int per = H.group_chunks ? 1 : lay.schur_lm;
    H.spec_ok = lay.spec && D <= MAX_D_LDS && !has_ext && schur_small_tiles(Dp);
    int g = 0;
    while (g < ngroup) {
      Chunk C;
      C.group_begin = g;
      int nl = 0;
      while (g < ngroup && (nl == 0 || nl + (groups[g].lm_end - groups[g].lm_begin) <= per)) {
        nl += groups[g].lm_end - groups[g].lm_begin;
        ++g;
      }
      C.group_end = g;
      chunks.push_back(C);
    }
  }   // (no landmarks: one empty chunk is not representable; handled by n_chunk = 0)
  nchunk = (int)chunks.size();
  // ---- per-chunk lists: which per-group partials sum into which pose block / cross block ----
  const int npose_blk_c = Dp / 6;
  std::vector<int>&chunk_diag_begin = S.chunk_diag_begin, &chunk_diag_out = S.chunk_diag_out, &chunk_cross_begin = S.chunk_cross_begin,
                   &chunk_cross = S.chunk_cross;
  chunk_diag_begin.assign((size_t)nchunk * npose_blk_c + 1, 0);
  chunk_cross_begin.assign((size_t)nchunk + 1, 0);
  chunk_cross.clear();
  {
    // per chunk and pose block: the partials (Task::out) of that block in (group, task) order — counted, then placed
    int n_diag = 0;
    for (const Task& T : tasks) n_diag += T.type < 2;
    chunk_diag_out.resize((size_t)n_diag);
    std::vector<int>& cur = S.blk_cursor;
    cur.resize((size_t)npose_blk_c + 1);
    int run = 0;
    for (int c = 0; c < nchunk; ++c) {
      chunk_cross_begin[c] = (int)chunk_cross.size() / 3;
      int* const begin = chunk_diag_begin.data() + (size_t)c * npose_blk_c;   // (zeroed above: counts first)
      const int t0 = groups[chunks[c].group_begin].task_begin, t1 = groups[chunks[c].group_end - 1].task_end;   // (tasks are laid out group by group)
      for (int t = t0; t < t1; ++t) {
        const Task& T = tasks[t];
        if (T.type < 2) {
          ++begin[T.off_a / 6];
        } else {
          chunk_cross.push_back(T.off_a);
          chunk_cross.push_back(T.off_b);
          chunk_cross.push_back(T.out);
        }
      }
      for (int bkk = 0; bkk < npose_blk_c; ++bkk) {
        const int n = begin[bkk];
        begin[bkk] = cur[bkk] = run;
        run += n;
      }
      for (int t = t0; t < t1; ++t) {
        const Task& T = tasks[t];
        if (T.type < 2) chunk_diag_out[(size_t)cur[T.off_a / 6]++] = T.out;
      }
    }
  }
  chunk_diag_begin[(size_t)nchunk * npose_blk_c] = (int)chunk_diag_out.size();
  chunk_cross_begin[nchunk] = (int)chunk_cross.size() / 3;
  // chunk descriptors of the matrix-core Schur kernel: one record instead of the chain chunks -> groups -> lm_pair_begin
  std::vector<int>& chunk_desc = S.chunk_desc;
  chunk_desc.assign((size_t)nchunk * SCHUR_DESC_INTS, 0);
  for (int c = 0; c < nchunk; ++c) {
    int* d = chunk_desc.data() + (size_t)c * SCHUR_DESC_INTS;
    const int lb = groups[chunks[c].group_begin].lm_begin, le = groups[chunks[c].group_end - 1].lm_end;
    d[0] = lb;
    d[1] = le;
    for (int i = 0; i <= SCHUR_CHUNK_LM_MAX / 4; ++i) d[2 + i] = lm_pair_begin[std::min(lb + 4 * i, le)];
  }
}

// ---- greedy colouring of the IMU factors: factors of one colour share no parameter block ----
void BuildCtx::imu_colouring() {
  imu_color.assign(w.n_imu, 0);
  for (int f = 0; f < w.n_imu; ++f) {
    int col = 0;
    for (;; ++col) {
      bool clash = false;
      for (int g2 = 0; g2 < f && !clash; ++g2) {
        if (imu_color[g2] != col) continue;
        const int pa[2] = {w.imu_pose0[f], w.imu_pose1[f]}, pb[2] = {w.imu_pose0[g2], w.imu_pose1[g2]};
        const int sa[2] = {w.imu_sb0[f], w.imu_sb1[f]}, sbb[2] = {w.imu_sb0[g2], w.imu_sb1[g2]};
        for (int i = 0; i < 2; ++i)
          for (int j = 0; j < 2; ++j) clash = clash || pa[i] == pb[j] || sa[i] == sbb[j];
      }
      if (!clash) break;
    }
    imu_color[f] = col;
    n_imu_color = std::max(n_imu_color, col + 1);
  }
  imu_color_begin.assign(n_imu_color + 1, 0);
  imu_coloff.assign(30 * (size_t)w.n_imu, -1);
  for (int c = 0; c < n_imu_color; ++c) {
    imu_color_begin[c] = (int)imu_order.size();
    for (int f = 0; f < w.n_imu; ++f)
      if (imu_color[f] == c) imu_order.push_back(f);
  }
  imu_color_begin[n_imu_color] = (int)imu_order.size();
  for (int f = 0; f < w.n_imu; ++f) {
    const int offs[4] = {pose_off[w.imu_pose0[f]], sb_off[w.imu_sb0[f]], pose_off[w.imu_pose1[f]], sb_off[w.imu_sb1[f]]};
    const int start[4] = {0, 6, 15, 21}, dims[4] = {6, 9, 6, 9};
    for (int b = 0; b < 4; ++b)
      for (int k = 0; k < dims[b]; ++k) imu_coloff[30 * (size_t)f + start[b] + k] = offs[b] < 0 ? -1 : offs[b] + k;
  }
}

// ---- marginalisation prior: H0 = J^T J ----
void BuildCtx::prior_h0() {
  Dm = w.marg_dim;
  H0.assign((size_t)Dm * Dm, 0.0);
  if (Dm > 0) {
    // a prior of more than H0_DEVICE_MIN rows: the O(Dm^3) product is left to the device (marg_h0_kernel, launched behind the
    // upload: the same sums in the same order)
    H.h0_on_device = Dm > H0_DEVICE_MIN && !(opt.tuning.flags & OKVIS_BA_TUNE_H0_ON_HOST);   // (the switch: A/B test of the two)
    // upper triangle as a sum of row outer products: every entry still adds its terms in row order (same value as the
    // column-by-column dot products), but the inner loop runs along a row of J (contiguous: 10 us -> 3 us at 45 rows)
    if (!H.h0_on_device) marg_h0_host(w.marg_J, Dm, H0.data());
  }
  nmb = Dm > 0 ? w.marg_nblocks : 0;
}

// ---- layout decisions: the sizes of the window record, the chain solver's fit, ldl_comp, fuse_fast ----
int BuildCtx::layout() {
  const int npose_blk = Dp / 6;
  spart_stride = npose_blk * (npose_blk + 1) / 2 * 36 + 3 * Dp;
  ntile = std::max(1, (Dp / 6 + SCHUR_TILE_BLOCKS - 1) / SCHUR_TILE_BLOCKS);
  P.n_pose = npose; P.n_sb = nsb; P.n_lm = nlm; P.n_cam = w.n_cam; P.n_obs = nobs; P.n_imu = w.n_imu;
  P.n_pprior = w.n_pprior; P.n_sbprior = w.n_sbprior; P.n_rel = w.n_relpose;
  P.marg_dim = Dm; P.marg_nb = nmb;
  P.D = D; P.Dp = Dp; P.n_pair = npair; P.n_group = ngroup; P.n_chunk = nchunk; P.n_task = (int)S.tasks.size();
  P.has_ext = has_ext ? 1 : 0;
  P.lin2 = lin2 ? 1 : 0;
  // ---- chain solver (ba_chain.hpp): the speed/bias blocks must couple only to their neighbours in the order of the reduced
  //      system (an IMU term links consecutive blocks; a marginalisation prior may span two adjacent ones) — what a sliding
  //      window's blocks do, in time order.  Windows solved in HBM (D > MAX_D_LDS) are not concerned.
  if (D <= MAX_D_LDS) {
    const int Ks = (D - Dp) / 9;
    bool fits = Dp >= 6 && Ks >= lay.chain_min && Ks <= CH_MAX_KS && LChain::tiles_fit(Dp) &&
                (int)solve_smem_chain(LChain::make(D, Dp).total, ((D + 5) / 6) * 6) <= SOLVE_LDS_LIMIT_CHAIN;
    auto rank = [&](int b) { return sb_off[b] < 0 ? -1 : (sb_off[b] - Dp) / 9; };
    for (int f = 0; f < w.n_imu && fits; ++f) {
      const int r0 = rank(w.imu_sb0[f]), r1 = rank(w.imu_sb1[f]);
      if (r0 >= 0 && r1 >= 0 && r0 != r1 + 1 && r1 != r0 + 1) fits = false;
    }
    int lo = INT_MAX, hi = -1;
    for (int b = 0; b < nmb && fits; ++b)
      if (w.marg_block_type[b] != OKVIS_BA_BLOCK_POSE) {
        const int r = rank(w.marg_block_idx[b]);
        if (r >= 0) lo = std::min(lo, r), hi = std::max(hi, r);
      }
    if (hi - lo > 1) fits = false;
    if (lay.chain && !fits) return BW_CHAIN_UNFIT;
    use_chain = lay.chain;
  }
  H.chain = use_chain;
  P.chain = use_chain ? (D - Dp) / 9 : 0;
  {
    // Diagonal blocks of the dense solver that carry a pose prior or the marginalisation prior: information of a few directions
    // that is orders of magnitude above everything else in the block (the yaw prior of the first pose: 1e16 n n^T across three
    // rotation rows), whose elimination cancels the leading digits of the block.  ba_ldl16.hpp eliminates them with compensated
    // products (profiles/r05_notes.md, "the referee").  The solver numbers the speed/bias part first (L16::perm).
    unsigned m = 0;
    if (D <= MAX_D_LDS && !(opt.tuning.flags & OKVIS_BA_TUNE_NO_LDL_COMP)) {   // (the tiled solver of larger systems: not compensated, ba_chol_tiles.hpp)
      // (chain solver: the blocks of the POSE system, which ldl16_solve factorises on its own; the speed/bias blocks are
      // eliminated 9 x 9, in the order of their rows, without the blocked solver's row / column asymmetry)
      const L16 LY = use_chain ? L16{ldl16_nb(Dp), 0, Dp} : L16{ldl16_nb(D), D - Dp, D};
      auto mark = [&](int off, int n) {
        if (off >= 0 && !(use_chain && off >= Dp))
          for (int k = 0; k < n; ++k) m |= 1u << (LY.perm(off + k) >> 4);
      };
      for (int i = 0; i < w.n_pprior; ++i) mark(pose_off[w.pprior_pose[i]], 6);
      for (int b = 0; b < nmb; ++b) {
        const bool pose = w.marg_block_type[b] == OKVIS_BA_BLOCK_POSE;
        mark(pose ? pose_off[w.marg_block_idx[b]] : sb_off[w.marg_block_idx[b]], pose ? 6 : 9);
      }
      if (opt.tuning.flags & OKVIS_BA_TUNE_LDL_COMP_ALL) m = ~0u;
    }
    P.ldl_comp = m;
  }
  P.gpart_size = gpart_size;
  P.n_tile = ntile;
  P.n_imu_color = n_imu_color;
  P.spart_stride = spart_stride;
  P.spart_buf_stride = (H.group_chunks || H.spec_ok) ? std::max(nchunk, 1) * spart_stride : 0;
  {
    int max_tasks = 0, max_pairs = 0;
    for (const Group& Gq : groups) {
      max_tasks = std::max(max_tasks, Gq.task_end - Gq.task_begin);
      max_pairs = std::max(max_pairs, Gq.pair_end - Gq.pair_begin);
    }
    const int stage = opt.fp32_linearize ? LinCfg<false, float>::STAGE_DOUBLES : LinCfg<false, double>::STAGE_DOUBLES;
    P.fuse_fast = H.group_chunks && !has_ext && max_tasks <= FUSE_MAX_TASKS && (lin2 || 6 * max_pairs <= FUSE_WIT * LIN_THREADS) &&
                  fuse_nlb(Dp, stage) >= 4;
  }
  P.cauchy_b = w.cauchy_b;
  P.imu.sigma_g_c = w.imu_params.sigma_g_c; P.imu.sigma_a_c = w.imu_params.sigma_a_c;
  P.imu.sigma_gw_c = w.imu_params.sigma_gw_c; P.imu.sigma_aw_c = w.imu_params.sigma_aw_c;
  P.imu.g = w.imu_params.g; P.imu.g_max = w.imu_params.g_max; P.imu.a_max = w.imu_params.a_max;
  return OKVIS_BA_OK;
}

// ---- arena: index lists (the state arrays and the observation records are in place, see BuildCtx::observations) ----
void BuildCtx::put_lists() {
  std::vector<int>& pair_off = S.pair_off;
  OFF(groups, put(A, S.groups));
  OFF(pair_lm, put_n(A, S.pair_lm.data(), (size_t)npair));
  OFF(pair_off, put_n(A, pair_off.data(), (size_t)npair));
  OFF(pair_role, put_n(A, S.pair_role.data(), (size_t)npair));
  OFF(pair_list_begin, put(A, S.pair_list_begin));
  OFF(pair_list, put(A, S.pair_list));
  OFF(lm_pair_begin, put(A, lm_pair_begin));
  OFF(lm_obs_begin, put(A, S.lm_obs_begin));
  OFF(lm_piece_begin, put_n(A, S.lm_piece_begin.data(), lin2 ? (size_t)nlm + 1 : 0));
  OFF(pair_piece, put_n(A, S.pair_piece.data(), lin2 ? (size_t)npair : 0));
  OFF(pair_block, put_n(A, S.pair_block.data(), lin2 ? (size_t)npair : 0));
  OFF(tasks, put(A, S.tasks));
  OFF(task_list, put(A, S.task_list));
  OFF(chunks, put(A, S.chunks));
  OFF(chunk_diag_begin, put(A, S.chunk_diag_begin));
  OFF(chunk_diag_out, put(A, S.chunk_diag_out));
  OFF(chunk_cross_begin, put(A, S.chunk_cross_begin));
  OFF(chunk_cross, put(A, S.chunk_cross));
  OFF(chunk_desc, put(A, S.chunk_desc));
  {
    // several Schur tiles per dimension (pose part beyond 96 rows): where the (landmark, block) pairs of every tile start, so that
    // a tile pair's workgroup touches its own pairs only (the pairs of a landmark are sorted by block)
    std::vector<int> lm_tile_begin;
    if (ntile > 1) {
      lm_tile_begin.resize((size_t)nlm * (ntile + 1));
      for (int l = 0; l < nlm; ++l) {
        int p = lm_pair_begin[l];
        for (int t = 0; t <= ntile; ++t) {
          while (p < lm_pair_begin[l + 1] && pair_off[p] < t * SCHUR_TILE_BLOCKS * 6) ++p;
          lm_tile_begin[(size_t)l * (ntile + 1) + t] = p;
        }
      }
    }
    OFF(lm_tile_begin, put(A, lm_tile_begin));
  }
  OFF(imu_order, put(A, imu_order));
  OFF(imu_color_begin, put(A, imu_color_begin));
  OFF(imu_coloff, put(A, imu_coloff));
}

// ---- arena: destination of every entry of the IMU factors' H (30x30 lower, packed) | g records in the solve kernel's matrix
//      layout (SLayout, ba_solve.hpp), so that the kernel can prefetch value + destination in one round trip; kept from call to
//      call (BuildScratch::ImuAsmCache) ----
int BuildCtx::put_imu_tables() {
  typedef BuildScratch::ImuAsmCache ImuAsmCache;
  ImuAsmCache* const asm_caches = S.asm_caches;
  int& asm_next = S.asm_next;
  int hit = -1;
  for (int k = 0; k < 4 && hit < 0; ++k)
    if (asm_caches[k].D == D && asm_caches[k].Dp == Dp && asm_caches[k].chain == (int)use_chain && asm_caches[k].coloff == imu_coloff &&
        asm_caches[k].color == imu_color)
      hit = k;
  const bool asm_hit = hit >= 0;
  ImuAsmCache& asm_cache = asm_caches[asm_hit ? hit : asm_next];
  if (!asm_hit) asm_next = (asm_next + 1) & 3;
  std::vector<int4>& imu_asm = asm_cache.table;
  std::vector<int>& imu_fastw = asm_cache.fastw;
  std::vector<int>& imu_pos = asm_cache.pos;
  if (!asm_hit) {
    asm_cache.D = D;
    asm_cache.Dp = Dp;
    asm_cache.chain = (int)use_chain;
    asm_cache.coloff = imu_coloff;
    asm_cache.color = imu_color;
    const int nbk = (D + 5) / 6;   // (the HBM matrix of the large windows has the same block layout)
    auto at = [&](int i, int j) {
      const int bi = i / 6, bj = j / 6;
      return (bj * nbk - (bj * (bj - 1)) / 2 + (bi - bj)) * SBS + (i - 6 * bi) * 6 + (j - 6 * bj);
    };
    // the same entry in the LDS layout of the LDL^T solver (L16::at, ba_ldl16.hpp): i >= j, stored at the mirrored position
    const L16 ly16{ldl16_nb(D), D - Dp, D};   // (the solver's ordering: speed/bias part first)
    const LChain lych = LChain::make(D, Dp);  // (chain solver: ba_chain.hpp)
    auto at16 = [&](int i, int j) { return use_chain ? lych.at(i, j) : ly16.at(i, j); };
    imu_asm.assign(512 * (size_t)w.n_imu, make_int4(-1, -1, 0, 0));
    imu_fastw.assign(512 * (size_t)w.n_imu, -1);
    // (the solve kernel's dynamic LDS: matrix area, then rhs, gradient, diagonal, solution — Dpad doubles each, ba_solve.hpp)
    const bool lds_system = D <= MAX_D_LDS;
    const int goff16 = lds_system ? (use_chain ? lych.total : ldl16_area_doubles(D)) + ((D + 5) / 6) * 6 : 0;
    // Where the entries of a factor's H | g record sit in the record (imu_pos, read by the factor workgroup that writes it): for a
    // system solved in LDS in the order of their places there, so that the lanes of a wave of the solve kernel — consecutive
    // record entries — add to ascending, mostly consecutive LDS addresses.  (In the packed order of the triangle the 64 entries
    // of a wave landed on one bank pair — a row of a 16x16 block lies 128 bytes behind the previous one — and the scatter
    // took 4 us.)  Windows solved in HBM keep the packed order.
    imu_pos.assign(512 * (size_t)w.n_imu, 0);
    std::vector<std::pair<int, int>> keys(495);
    for (int f = 0; f < w.n_imu; ++f) {
      const int* co = imu_coloff.data() + 30 * (size_t)f;
      int e = 0;
      for (int a = 0; a < 30; ++a)
        for (int b = 0; b <= a; ++b, ++e) {
          const int ra = co[a], rb = co[b];
          keys[e] = {(ra < 0 || rb < 0) ? INT_MAX : (lds_system ? at16(ra, rb) : e), e};
        }
      for (int a = 0; a < 30; ++a) keys[465 + a] = {co[a] < 0 ? INT_MAX : (lds_system ? goff16 + co[a] : 465 + a), 465 + a};
      if (lds_system) std::sort(keys.begin(), keys.end());
      int* pos = imu_pos.data() + 512 * (size_t)f;
      for (int rank = 0; rank < 495; ++rank) pos[keys[rank].second] = rank;
      for (int k = 495; k < 512; ++k) pos[k] = k;
      e = 0;
      for (int a = 0; a < 30; ++a)
        for (int b = 0; b <= a; ++b, ++e) {
          const int ra = co[a], rb = co[b];
          if (ra < 0 || rb < 0) continue;
          const size_t at_rec = 512 * (size_t)f + pos[e];
          imu_asm[at_rec] = make_int4((ra >= rb ? at(ra, rb) : at(rb, ra)) | (imu_color[f] << 24), a == b ? ra : -1,
                                      ra >= rb ? (ra << 16 | rb) : (rb << 16 | ra),   // z: the reduced indices
                                      0);
          if (lds_system && imu_color[f] < 16) imu_fastw[at_rec] = at16(ra, rb) | ((a == b ? ra + 1 : 0) << 16) | (imu_color[f] << 24);
        }
      for (int a = 0; a < 30; ++a)
        if (co[a] >= 0) {
          const size_t at_rec = 512 * (size_t)f + pos[465 + a];
          imu_asm[at_rec] = make_int4(co[a] | (1 << 20) | (imu_color[f] << 24), -1, 0, 0);
          if (lds_system && imu_color[f] < 16) imu_fastw[at_rec] = (goff16 + co[a]) | (imu_color[f] << 24);
        }
    }
  }
  if (imu_asm.empty()) OFF(imu_asm, put(A, std::vector<int4>(1, make_int4(-1, -1, 0, 0))));
  else OFF(imu_asm, put(A, imu_asm));
  if (imu_fastw.empty()) OFF(imu_fastw, put(A, std::vector<int>(1, -1)));
  else OFF(imu_fastw, put(A, imu_fastw));
  if (imu_pos.empty()) OFF(imu_pos, put(A, std::vector<int>(1, 0)));
  else OFF(imu_pos, put(A, imu_pos));
  // large windows: the reverse map, so that the tile export (many workgroups) gathers the IMU contributions instead of one
  // workgroup scattering them into HBM.  At most two factors meet in one entry (the chain couples consecutive states).
  std::vector<int2> imu_rev;
  if (D > MAX_D_LDS) {
    const size_t nbk = (D + 5) / 6;
    imu_rev.assign(nbk * (nbk + 1) / 2 * SBS, make_int2(-1, -1));
    for (size_t idx = 0; idx < 512 * (size_t)w.n_imu; ++idx) {
      const int4 d = imu_asm[idx];
      if (d.x < 0 || (d.x & (1 << 20))) continue;   // nothing / an entry of g
      int2& r = imu_rev[d.x & 0xFFFFF];
      if (r.x < 0) r.x = (int)idx;
      else if (r.y < 0) r.y = (int)idx;
      else return OKVIS_BA_ERR_UNSUPPORTED;   // three IMU factors on one block: not a chain
    }
  }
  if (imu_rev.empty()) imu_rev.push_back(make_int2(-1, -1));
  OFF(imu_rev, put(A, imu_rev));
  return OKVIS_BA_OK;
}

// ---- arena: the zeroed part (everything the device writes before it reads) ----
void BuildCtx::put_zeroed() {
  for (int b = 0; b < 2; ++b) {
    OFF(V[b], put_zero(A, 48 * (size_t)nlm));
    OFF(bl[b], put_zero(A, 24 * (size_t)nlm));
    OFF(Hq[b], put_zero(A, 48 * (size_t)nlm));
    OFF(W[b], put_zero(A, 144 * (size_t)npair));
    OFF(gpart[b], put_zero(A, 8 * (size_t)gpart_size));
    OFF(gscal[b], put_zero(A, 8 * (size_t)GS_COUNT * ngroup));
    OFF(imu_lin[b], put_zero(A, 8 * (size_t)IMU_LIN_STRIDE * w.n_imu));
    OFF(pp_lin[b], put_zero(A, 8 * 42 * (size_t)w.n_pprior));
    OFF(sbp_lin[b], put_zero(A, 8 * 9 * (size_t)w.n_sbprior));
    OFF(rel_lin[b], put_zero(A, 8 * 78 * (size_t)w.n_relpose));
    OFF(marg_lin_e[b], put_zero(A, 8 * 2 * (size_t)Dm));
    OFF(marg_lin_M[b], put_zero(A, 8 * 9 * (size_t)nmb));
    OFF(small_cost[b], put_zero(A, 16));
    if (opt.debug_arrays) OFF(obs_r[b], put_zero(A, 16 * (size_t)nobs));
  }
  OFF(spart, put_zero(A, 8 * (size_t)std::max(nchunk, 1) * (size_t)spart_stride * ((H.group_chunks || H.spec_ok) ? 2 : 1)));
  OFF(spart_sum, put_zero(A, 8 * (size_t)std::max(spart_stride, 1)));
  OFF(sum_sync, put_zero(A, 16));
  OFF(dec, put_zero(A, 8 * (size_t)DEC_COUNT));
  if (opt.debug_arrays) {
    OFF(S, put_zero(A, 8 * (size_t)D * D));
    OFF(rhs, put_zero(A, 8 * (size_t)D));
    OFF(Dp2, put_zero(A, 8 * (size_t)D));
  }
  if (D > MAX_D_LDS) {
    const size_t nbk = (D + 5) / 6;
    OFF(Sg, put_zero(A, 8 * nbk * (nbk + 1) / 2 * 38));
    const size_t nT = (D + CT_TB - 1) / CT_TB, ntile = nT * (nT + 1) / 2;
    P.ct_nT = (int)nT;
    OFF(ct_T, put_zero(A, 8 * ntile * CT_TILE));
    OFF(ct_Linv, put_zero(A, 8 * nT * CT_TILE));
    OFF(ct_rhs, put_zero(A, 8 * nT * CT_TB));
    OFF(ct_y, put_zero(A, 8 * nT * CT_TB));
    OFF(ct_x, put_zero(A, 8 * nT * CT_TB));
    OFF(ct_flag, put_zero(A, sizeof(int) * (ntile + 4 + 2 * nT)));
    OFF(ct_g, put_zero(A, 8 * nT * CT_TB));
    OFF(ct_d2, put_zero(A, 8 * nT * CT_TB));
  }
  OFF(step, put_zero(A, 8 * (size_t)D));
  OFF(scale_p, put_zero(A, 8 * (size_t)D));
  OFF(lm_scale, put_zero(A, 24 * (size_t)nlm));
  OFF(grad, put_zero(A, 8 * (size_t)D));
  OFF(quality, put_zero(A, 8 * (size_t)nlm));
  OFF(results, put_zero(A, results_bytes(w.n_pose, w.n_sb, nlm, w.n_imu) + 8));
  if (opt.debug_arrays) OFF(prof, put_zero(A, 8 * (64 + 4 * 160)));   // clock64() phase stamps + tile task timeline: diagnostics only
  OFF(ctrl, put_zero(A, sizeof(Ctrl)));
}

// ---- arena: the caller's arrays (IMU terms with their preintegration records, priors, the marginalisation prior) ----
void BuildCtx::put_caller_arrays() {
  OFF(imu_pose0, put_n(A, w.imu_pose0, (size_t)w.n_imu));
  OFF(imu_sb0, put_n(A, w.imu_sb0, (size_t)w.n_imu));
  OFF(imu_pose1, put_n(A, w.imu_pose1, (size_t)w.n_imu));
  OFF(imu_sb1, put_n(A, w.imu_sb1, (size_t)w.n_imu));
  {
    std::vector<long long> t0(w.n_imu), t1(w.n_imu), st(w.n_imu ? w.n_imu_samples : 0);
    for (int f = 0; f < w.n_imu; ++f) {
      t0[f] = w.imu_t0[f];
      t1[f] = w.imu_t1[f];
    }
    for (size_t i = 0; i < st.size(); ++i) st[i] = w.imu_s_t[i];
    OFF(imu_t0, put(A, t0));
    OFF(imu_t1, put(A, t1));
    OFF(imu_s_t, put(A, st));
  }
  OFF(imu_s_begin, put_n(A, w.imu_s_begin, (size_t)w.n_imu));
  OFF(imu_s_count, put_n(A, w.imu_s_count, (size_t)w.n_imu));
  OFF(imu_s_gyr, put_n(A, w.imu_s_gyr, w.n_imu ? 3 * (size_t)w.n_imu_samples : 0));
  OFF(imu_s_acc, put_n(A, w.imu_s_acc, w.n_imu ? 3 * (size_t)w.n_imu_samples : 0));
  {
    std::vector<ImuCacheD> caches((size_t)w.n_imu);
    if (!caches.empty()) std::memset(caches.data(), 0, sizeof(ImuCacheD) * caches.size());
    if (w.imu_sb_ref && w.imu_sb_ref_valid) {
      for (int f = 0; f < w.n_imu; ++f) {
        if (w.imu_sb_ref_valid[f] == 2) {
          // the preintegration itself (okvis_ba_fetch_imu_caches, checked by check_build_limits): valid as it stands, nothing is
          // rebuilt on first use
          std::memcpy(&caches[f], w.imu_cache + (size_t)OKVIS_BA_IMU_CACHE_DOUBLES * f, sizeof(ImuCacheD));
          caches[f].redo_count = 0;
        } else if (w.imu_sb_ref_valid[f]) {
          caches[f].valid = 2;
          for (int k = 0; k < 9; ++k) caches[f].sb_ref[k] = w.imu_sb_ref[9 * (size_t)f + k];
        }
      }
    }
    OFF(imu_cache, put(A, caches));
    OFF(imu_cache_prev, put_zero(A, sizeof(ImuCacheD) * (size_t)w.n_imu));
  }
  OFF(pprior_pose, put_n(A, w.pprior_pose, (size_t)w.n_pprior));
  OFF(pprior_meas, put_n(A, w.pprior_meas, 7 * (size_t)w.n_pprior));
  OFF(pprior_sqrtinfo, put_n(A, w.pprior_sqrtinfo, 36 * (size_t)w.n_pprior));
  OFF(sbprior_sb, put_n(A, w.sbprior_sb, (size_t)w.n_sbprior));
  OFF(sbprior_meas, put_n(A, w.sbprior_meas, 9 * (size_t)w.n_sbprior));
  OFF(sbprior_sqrtinfo, put_n(A, w.sbprior_sqrtinfo, 81 * (size_t)w.n_sbprior));
  OFF(rel_pose0, put_n(A, w.rel_pose0, (size_t)w.n_relpose));
  OFF(rel_pose1, put_n(A, w.rel_pose1, (size_t)w.n_relpose));
  OFF(rel_sqrtinfo, put_n(A, w.rel_sqrtinfo, 36 * (size_t)w.n_relpose));
  OFF(marg_block_type, put_n(A, w.marg_block_type, (size_t)nmb));
  OFF(marg_block_idx, put_n(A, w.marg_block_idx, (size_t)nmb));
  OFF(marg_block_off, put_n(A, w.marg_block_off, (size_t)nmb));
  OFF(marg_J, put_n(A, w.marg_J, (size_t)Dm * Dm));
  OFF(marg_H0, put(A, H0));
  OFF(marg_e0, put_n(A, w.marg_e0, (size_t)Dm));
  OFF(marg_lin, put_n(A, w.marg_lin, 9 * (size_t)nmb));
  {
    // where the columns of the pose / speed-bias priors sit in the reduced system (the solve kernel used to look this up
    // through two dependent loads per column)
    std::vector<int> prior_col(6 * (size_t)w.n_pprior + 9 * (size_t)w.n_sbprior + 1, -1);
    for (int i = 0; i < w.n_pprior; ++i) {
      const int off = pose_off[w.pprior_pose[i]];
      for (int k = 0; k < 6; ++k) prior_col[6 * (size_t)i + k] = off < 0 ? -1 : off + k;
    }
    for (int i = 0; i < w.n_sbprior; ++i) {
      const int off = sb_off[w.sbprior_sb[i]];
      for (int k = 0; k < 9; ++k) prior_col[6 * (size_t)w.n_pprior + 9 * (size_t)i + k] = off < 0 ? -1 : off + k;
    }
    OFF(prior_col, put(A, prior_col));
  }
}

// ---- what the host keeps of the window, and its algorithmic (compulsory) bytes per iteration, DESIGN.md §4 ----
void BuildCtx::host_record() {
  H.n_pose = npose; H.n_sb = nsb; H.n_lm = nlm; H.n_obs = nobs; H.n_imu = w.n_imu; H.D = D; H.Dp = Dp;
  H.pose_off = S.pose_off; H.sb_off = S.sb_off; H.marg_dim = Dm;
  H.n_pair = npair; H.n_group = ngroup; H.n_chunk = nchunk;
  H.pair_lm.assign(S.pair_lm.data(), S.pair_lm.data() + npair);
  H.pair_block.assign(S.pair_block.data(), S.pair_block.data() + npair);
  H.acc = 0;
  const int64_t O = nobs, L = nlm, Pn = npair;
  H.bytes_lin = 32 * O + 56 * (int64_t)npose + 32 * L + 8 * (int64_t)D + 72 * L + 144 * Pn  // reads
                + 32 * L + 120 * L + 144 * Pn + 8 * (int64_t)gpart_size + 8 * GS_COUNT * (int64_t)ngroup;  // writes
  H.bytes_schur = 72 * L + 144 * Pn + 8 * (int64_t)nchunk * spart_stride;
  H.bytes_solve = 8 * (int64_t)nchunk * spart_stride + 8 * (int64_t)gpart_size + 8 * (int64_t)IMU_LIN_STRIDE * w.n_imu +
                  8 * (int64_t)Dm * Dm + 8 * (int64_t)D + 2 * (56 * (int64_t)npose + 72 * (int64_t)nsb);
  H.bytes_small = (int64_t)w.n_imu * (8 * IMU_LIN_STRIDE + (int64_t)sizeof(ImuCacheD) + 2 * 56 + 2 * 72) +
                  8 * (int64_t)Dm * Dm * 2;
}

int build_window(const okvis_ba_window& w, const okvis_ba_options& opt, const BatchLayout& lay, Arena& A, HostWin& H) {
  BuildTimer T;   // (the sections OKVIS_BA_DEBUG=build prints)
  if (int rc = check_window_args(w)) return rc;
  if (int rc = check_build_limits(w)) return rc;
  T.mark("imu checks");
  BuildCtx cx(w, opt, lay, A, H);
  if (int rc = cx.ordering()) return rc;
  if (int rc = cx.observations()) return rc;   // (or BW_LIN2_UNFIT: free extrinsics)
  T.mark("observations + pairs");
  if (int rc = cx.form_groups()) return rc;   // (BW_LIN2_UNFIT: a landmark with more than LIN2_PIECES pieces)
  T.mark("groups");
  if (lay.lin2) cx.lists_pieces();
  else cx.lists_staged();
  T.mark("lists+tasks");
  cx.form_chunks();
  T.mark("chunks");
  cx.imu_colouring();
  T.mark("imu colouring");
  cx.prior_h0();
  if (int rc = cx.layout()) return rc;   // (BW_CHAIN_UNFIT)
  T.mark("prior + sizes");
  cx.put_lists();
  T.mark("arena: arrays");
  if (int rc = cx.put_imu_tables()) return rc;   // (OKVIS_BA_ERR_UNSUPPORTED: three IMU factors on one block of a large window)
  T.mark("arena: imu tables");
  cx.put_zeroed();
  cx.put_caller_arrays();
  cx.host_record();
  T.mark("arena");
  return OKVIS_BA_OK;
}

// The index build of a batch laid out by L: windows w[0 .. n) into A and H[0 .. n).  A window that does not fit the piece path or the
// chain solve sends the whole batch back to the staged kernel's lists / the dense solve's layout (L says which it got).
int build_batch(const okvis_ba_window* w, int n, const okvis_ba_options& o, BatchLayout& L, Arena& A, HostWin* H) {
  for (int i = 0; i < n; ++i) {
    const int rc = build_window(w[i], o, L, A, H[i]);
    if (rc == BW_LIN2_UNFIT || rc == BW_CHAIN_UNFIT) {   // start over with every window
      (rc == BW_LIN2_UNFIT ? L.lin2 : L.chain) = false;
      A.size = A.zsize = 0;
      i = -1;
    } else if (rc != OKVIS_BA_OK)
      return rc;
    // The chain solve launch is sized from the batch's largest LChain::total and its largest padded dimension (batch_max,
    // make_plan), which may come from different windows: every window fits alone (BuildCtx::layout) and the pair does not.
    // Such a batch is answered like one with an unfit window: the dense layout for every window.  (Reached under a forced
    // SOLVE_CHAIN only: every pair that overflows contains the shape (156, 120), whose four speed/bias blocks are fewer than
    // CHAIN_AUTO_MIN_BLOCKS, so that under AUTO the per-window rule has sent the batch to the dense layout already.)
    if (i == n - 1 && L.chain) {
      int chain_doubles = 0, Dpad = 0;
      for (int k = 0; k < n; ++k) {
        const WinPtrs& Pk = H[k].ptrs;
        if (Pk.D > MAX_D_LDS) continue;
        Dpad = std::max(Dpad, ((Pk.D + 5) / 6) * 6);
        if (Pk.chain) chain_doubles = std::max(chain_doubles, LChain::make(Pk.D, Pk.Dp).total);
      }
      if (chain_doubles > 0 && (int)solve_smem_chain(chain_doubles, Dpad) > SOLVE_LDS_LIMIT_CHAIN) {
        L.chain = false;
        A.size = A.zsize = 0;
        i = -1;
      }
    }
  }
  L.split_small = L.split_small && L.lin2;
  return OKVIS_BA_OK;
}

// What the batch's windows ask of make_plan (BatchMax), the other half of what the index build tells it; the records P of a batch
// that is not fused / not decision-free as a whole lose what only such a batch uses
BatchMax batch_max(const HostWin* H, WinPtrs* P, int n) {
  BatchMax M;
  M.group_chunks = M.spec_schur = true;
  for (int i = 0; i < n; ++i) {
    const WinPtrs& Pi = P[i];
    M.group = std::max(M.group, Pi.n_group);
    M.imu = std::max(M.imu, Pi.n_imu);
    M.schur_blocks = std::max(M.schur_blocks, Pi.n_chunk * (Pi.n_tile * (Pi.n_tile + 1) / 2));
    M.lm = std::max(M.lm, Pi.n_lm);
    M.Dp = std::max(M.Dp, Pi.Dp);
    M.chunks = std::max(M.chunks, Pi.n_chunk);
    if (Pi.D <= MAX_D_LDS) {
      M.Dpad_small = std::max(M.Dpad_small, ((Pi.D + 5) / 6) * 6);
      if (Pi.chain) {
        M.chain = true;
        M.chain_doubles = std::max(M.chain_doubles, LChain::make(Pi.D, Pi.Dp).total);
      }
    } else
      M.Dpad_large = std::max(M.Dpad_large, ((Pi.D + 5) / 6) * 6);
    M.any_ext = M.any_ext || Pi.has_ext;
    M.group_chunks = M.group_chunks && H[i].group_chunks;
    M.spec_schur = M.spec_schur && H[i].spec_ok;
  }
  // a batch is fused as a whole or not at all; a batch that is not takes the decision-free Schur launch as a whole or not at all;
  // otherwise one set of partials for everybody
  if (M.group_chunks) M.spec_schur = false;
  if (!M.group_chunks)
    for (int i = 0; i < n; ++i) P[i].fuse_fast = 0;
  if (!M.group_chunks && !M.spec_schur)
    for (int i = 0; i < n; ++i) P[i].spart_buf_stride = 0;
  return M;
}

// The chunk launch records of a batch (SCHUR_REC_INTS, ba_types.hpp): what a workgroup of the ring instantiations of the matrix-core
// Schur kernel reads before its first data load — the chunk descriptor and, per pose block, the range and the head of its list of
// J^T J / J^T r partials — gathered from chunk_desc / chunk_diag_begin / chunk_diag_out (which stay: the serial loop, schur_kernel and
// the fused reduction read them) into one array of the arena's data part, [window][stride][SCHUR_REC_INTS]; slots behind a window's
// last chunk are zero (an empty chunk).  H[i].ptrs still hold arena offsets.  Returns the stride = the batch's largest chunk count,
// or 0 = no records: a window with free extrinsics or a pose part beyond the small tiles, where make_plan selects no ring kernel.
int build_chunk_records(Arena& A, const HostWin* H, int n, size_t* off) {
  int stride = 0;
  for (int i = 0; i < n; ++i) {
    const WinPtrs& P = H[i].ptrs;
    if (P.has_ext || !schur_small_tiles(P.Dp) || P.Dp / 6 > SCHUR_REC_BLOCKS) return 0;
    stride = std::max(stride, P.n_chunk);
  }
  if (stride == 0) return 0;
  const size_t bytes = (size_t)n * stride * SCHUR_REC_INTS * sizeof(int);
  *off = A.alloc(bytes);
  if (A.host.size() < A.size) A.host.resize(A.size, 0);
  std::memset(A.host.data() + *off, 0, bytes);
  for (int i = 0; i < n; ++i) {
    const WinPtrs& P = H[i].ptrs;
    auto list = [&](const void* field) { return reinterpret_cast<const int*>(A.host.data() + reinterpret_cast<size_t>(field)); };
    const int *desc = list((const void*)P.chunk_desc), *begin = list((const void*)P.chunk_diag_begin), *out = list((const void*)P.chunk_diag_out);
    const int nb = P.Dp / 6;
    for (int c = 0; c < P.n_chunk; ++c) {
      int* r = reinterpret_cast<int*>(A.host.data() + *off) + ((size_t)i * stride + c) * SCHUR_REC_INTS;
      std::memcpy(r, desc + (size_t)c * SCHUR_DESC_INTS, SCHUR_DESC_INTS * sizeof(int));
      for (int b = 0; b < nb; ++b) {
        int* e = r + SCHUR_REC_LISTS + 8 * b;
        const int q0 = begin[(size_t)c * nb + b], nq = begin[(size_t)c * nb + b + 1] - q0;
        e[0] = q0, e[1] = nq;
        for (int q = 0; q < std::min(nq, SCHUR_REC_LL); ++q) e[2 + q] = out[q0 + q];
      }
    }
  }
  return stride;
}

// The group launch records of a batch (LIN_REC_INTS, ba_types.hpp): what a workgroup of linearize2_rec_kernel reads before it can
// request its operands — the Group record and the group's four counts — copied from the windows' group arrays (which stay:
// linearize_kernel, the fused and the SMALL instantiations of linearize2_kernel read them) into one array of the arena's data part,
// [window][stride][LIN_REC_INTS]; slots behind a window's last group are zero.  H[i].ptrs still hold arena offsets.  Returns the
// stride = the batch's largest group count, or 0 = no records: a window that is not laid out for the piece path.
int build_group_records(Arena& A, const HostWin* H, int n, size_t* off) {
  int stride = 0;
  for (int i = 0; i < n; ++i) {
    const WinPtrs& P = H[i].ptrs;
    if (!P.lin2 || P.has_ext) return 0;
    stride = std::max(stride, P.n_group);
  }
  if (stride == 0) return 0;
  const size_t bytes = (size_t)n * stride * LIN_REC_INTS * sizeof(int);
  *off = A.alloc(bytes);
  if (A.host.size() < A.size) A.host.resize(A.size, 0);
  std::memset(A.host.data() + *off, 0, bytes);
  for (int i = 0; i < n; ++i) {
    const WinPtrs& P = H[i].ptrs;
    const Group* groups = reinterpret_cast<const Group*>(A.host.data() + reinterpret_cast<size_t>((const void*)P.groups));
    for (int g = 0; g < P.n_group; ++g) {
      const Group G = groups[g];   // (a copy: the records may lie in the same, just resized, buffer)
      int* r = reinterpret_cast<int*>(A.host.data() + *off) + ((size_t)i * stride + g) * LIN_REC_INTS;
      std::memcpy(r, &G, sizeof(Group));
      r[LIN_REC_COUNTS] = G.lm_end - G.lm_begin, r[LIN_REC_COUNTS + 1] = G.obs_end - G.obs_begin;
      r[LIN_REC_COUNTS + 2] = G.pair_end - G.pair_begin, r[LIN_REC_COUNTS + 3] = G.task_end - G.task_begin;
      r[LIN_REC_VALID] = 1;
    }
  }
  return stride;
}

// convert the arena offsets stored in the pointer fields to device addresses
void relocate(WinPtrs& P, unsigned char* base, unsigned char* zbase, int debug) {
  unsigned char** fields = reinterpret_cast<unsigned char**>(&P.pose[0]);
  // all pointer members are laid out contiguously from pose[0] to marg_lin; relocate by scanning the
  // struct region as an array of pointers (sizes/scalars precede pose[0])
  const size_t first = offsetof(WinPtrs, pose);
  const size_t n = (offsetof(WinPtrs, marg_lin) + sizeof(void*) - first) / sizeof(void*);   // (the record ends with alignment padding)
  for (size_t i = 0; i < n; ++i) {
    const size_t off = reinterpret_cast<size_t>(fields[i]);
    fields[i] = (off & ARENA_ZFLAG) ? zbase + (off & ~ARENA_ZFLAG) : base + off;
  }
  // optional arrays that were never allocated hold offset 0 -> must be null
  if (debug != 1) {   // 2 = phase stamps only: the copies of the linearisation / system would distort the stamps
    P.obs_r[0] = P.obs_r[1] = nullptr;
    P.S = nullptr;
    P.rhs = nullptr;
    P.Dp2 = nullptr;
  }
  if (!debug) P.prof = nullptr;
  P.Hpp = nullptr;
  if (P.D <= MAX_D_LDS) {
    P.Sg = nullptr;
    P.ct_T = P.ct_Linv = P.ct_rhs = P.ct_y = P.ct_x = P.ct_g = P.ct_d2 = nullptr;
    P.ct_flag = nullptr;
  }
}

}  // namespace
