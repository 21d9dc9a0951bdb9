// Part of ba_capi.hip (one translation unit; included there, in this order: capi_solver.inc, capi_index_build.inc, capi_launch.inc,
// then the entry points with capi_queries.inc and capi_upload.inc, capi_standalone.inc, capi_marginalize.inc and the covariance parts
// inside its extern "C" block).
// The solver record: host copies of what queries need, the staging allocator, the arena, the host view (HostView), okvis_ba_solver,
// the entry guard (enter), the diagnostics word.
namespace {

#define HIP_TRY(expr)                                              \
  do {                                                             \
    hipError_t _e = (expr);                                        \
    if (_e != hipSuccess) {                                        \
      s->last_hip_error = (int)_e;                                 \
      return OKVIS_BA_HIP_ERROR_BASE + (int)_e;                    \
    }                                                              \
  } while (0)

struct HostWin {  // host copy of what the queries and downloads need
  int n_pose = 0, n_sb = 0, n_lm = 0, n_obs = 0, n_imu = 0, D = 0, Dp = 0, n_pair = 0, n_group = 0, n_chunk = 0;
  std::vector<int> pair_lm, pair_block;
  std::vector<int> pose_off, sb_off;  // reduced ordering (host copy)
  int marg_dim = 0;
  bool h0_on_device = false;   // H0 = J^T J of a large prior is formed by marg_h0_kernel after the upload, not by build_window
  bool group_chunks = false;   // one Schur chunk per linearise group (what the fused linearise + reduce launch needs)
  bool spec_ok = false;        // the window can take a decision-free Schur launch (one set of partials per linearisation buffer, see spec_schur)
  bool chain = false;          // laid out for the chain solver (ba_chain.hpp): WinPtrs::chain > 0
  WinPtrs ptrs;  // device pointers
  int acc = 0;
  int64_t bytes_lin = 0, bytes_schur = 0, bytes_solve = 0, bytes_small = 0;
};

// Device arena of a batch = [data part, built on the host and copied over PCIe | zero part, cleared on the device].
// Offsets into the zero part carry ARENA_ZFLAG until relocate() turns them into pointers: the linearisation buffers,
// Schur partials and work areas are more than half of a window's bytes and need not cross PCIe as zeros.
constexpr size_t ARENA_ZFLAG = size_t(1) << 62;
// Page-locked host memory for the staging buffers (H2D copies from pinned memory are asynchronous and about twice as
// fast as from pageable memory); plain malloc when there is no device (okvis_ba_check_window on a CPU-only host).
template <class T>
struct StageAlloc {
  typedef T value_type;
  StageAlloc() = default;
  template <class U>
  StageAlloc(const StageAlloc<U>&) {}
  T* allocate(size_t n) {
    const size_t bytes = n * sizeof(T) + 16;
    void* p = nullptr;
    unsigned char tag = 1;
    if (hipHostMalloc(&p, bytes, hipHostMallocDefault) != hipSuccess || !p) {
      (void)hipGetLastError();
      p = std::malloc(bytes);
      tag = 0;
      if (!p) throw std::bad_alloc();
    }
    static_cast<unsigned char*>(p)[0] = tag;
    return reinterpret_cast<T*>(static_cast<unsigned char*>(p) + 16);
  }
  void deallocate(T* q, size_t) {
    unsigned char* p = reinterpret_cast<unsigned char*>(q) - 16;
    if (p[0]) (void)hipHostFree(p); else std::free(p);
  }
  template <class U>
  bool operator==(const StageAlloc<U>&) const { return true; }
  template <class U>
  bool operator!=(const StageAlloc<U>&) const { return false; }
};
typedef std::vector<unsigned char, StageAlloc<unsigned char>> StageVec;
// page-locked (and so readable by the device in place) or the plain-malloc fall-back?  (the tag StageAlloc keeps in front of the block)
inline bool stage_is_pinned(const StageVec& v) { return !v.empty() && (v.data() - 16)[0] == 1; }
struct Arena {
  StageVec host;   // data part
  size_t size = 0;                   // bytes of the data part
  size_t zsize = 0;                  // bytes of the zero part
  size_t alloc(size_t bytes) {
    size_t off = (size + 255) & ~size_t(255);
    size = off + bytes;
    return off;
  }
  size_t zalloc(size_t bytes) {
    size_t off = (zsize + 255) & ~size_t(255);
    zsize = off + bytes;
    return off | ARENA_ZFLAG;
  }
  size_t data_bytes() const { return (size + 255) & ~size_t(255); }
  size_t total() const { return data_bytes() + zsize; }
};

// What a batch asks of its windows' layout, from the options and the window count alone (batch_layout); build_window adds the
// conditions on a window's shape, build_batch clears lin2 / chain for the whole batch when a window does not fit them
struct BatchLayout {
  bool lin2 = false, chain = false;   // the piece path's lists (ba_linearize2.hpp), the chain solve's layout (ba_chain.hpp) ...
  int chain_min = 1;                  // ... for LDS-resident windows with at least this many speed/bias blocks
  bool fuse = false, spec = false;    // the fused linearise + reduce launch / the decision-free Schur launch allowed
  int schur_lm = 0, group_lm = 0;     // landmarks per Schur chunk / per linearise group (at most)
  bool split_small = false;           // piece path: IMU / prior factors in a launch of their own (small_kernel)
  bool fp32 = false;                  // the observation stage the fused reduction was sized for
};
// The per-window maxima of an uploaded batch that its launches are sized by, and what its windows' layouts have in common
struct BatchMax {
  int group = 0, imu = 0, schur_blocks = 0, lm = 0, Dp = 0, chunks = 0;
  int Dpad_small = 0, Dpad_large = 0, chain_doubles = 0;   // LDS-resident windows / solved in HBM; the chain solver's LChain::total
  bool any_ext = false, chain = false;   // free extrinsics somewhere; LDS-resident windows laid out for the chain solver
  bool group_chunks = false;             // every window has one Schur chunk per linearise group (fused mode possible)
  // Batches that are not fused but run DOGLEG or fixed-radius iterations on windows the matrix-core Schur kernel serves: the Schur
  // launch takes no decision (schur_mfma_kernel, nodec) and reduces the trial buffer into that buffer's own set of partials, the
  // solve kernel decides (its DBUF instantiation, as in fused mode).  OKVIS_BA_TUNE_SCHUR_DECIDES keeps the decision in the Schur launch.
  bool spec_schur = false;
  int rec_stride = 0;   // chunk launch records per window (build_chunk_records; 0 = the batch has none: no ring kernel)
  int grec_stride = 0;  // group launch records per window (build_group_records; 0 = none: linearize2_kernel reads the window record)
};
struct Launch {   // one launch: the instantiation (capi_launch.inc, 0 = none), grid.x (grid.y = windows), dynamic LDS in bytes
  int k = 0, gx = 0, lds = 0;
};
struct Extent {   // windows [w0, w0 + nw) of one launch, and the helper workgroups per window of their solve launch
  int w0 = 0, nw = 0, helpers = 0;
  bool operator==(const Extent& o) const { return w0 == o.w0 && nw == o.nw && helpers == o.helpers; }
};
// The launch plan of an uploaded batch (make_plan, capi_launch.inc): its route, every launch the solver issues and their scalar
// arguments.  (ints only, no padding: plans are compared byte for byte)
struct PlanFixed {
  int lin2 = 0, split_small = 0, fused = 0, nodec = 0, rides = 0, graph = 0;   // the route
  Launch schur; int trows = 0, nlb = 0, n_small = 0, rec_stride = 0;   // (nodec above; the chunk launch records per window)
  Launch solve, tiled; int nT = 0;                     // the LDS-resident windows / the windows solved in HBM (+ their tiles per dimension)
  Launch small_init, small_iter, lin; int lin_n_small = 0, sd = 0;   // the factors' launch of okvis_ba_begin / of an iteration; linearise
  int grec_stride = 0;   // > 0: lin names a record instantiation (LIN2R, capi_launch.inc); its group launch records per window
  Launch take_back; int budget = 0;                    // imu_take_back_kernel; add_budget_kernel in front of the iterations
  int three = 0;   // 1 = the three-launch iteration is this plan's default: Schur -> solve -> linearise, small_iter only for windows that paused
  Extent whole; int one_helpers = 0;                   // okvis_ba_begin / okvis_ba_finish; okvis_ba_marginalize (one window)
};
struct LaunchPlan : PlanFixed {
  std::vector<Extent> subs;   // okvis_ba_iterate's sub-batches, one stream each
  bool operator==(const LaunchPlan& o) const {
    return std::memcmp(static_cast<const PlanFixed*>(this), static_cast<const PlanFixed*>(&o), sizeof(PlanFixed)) == 0 && subs == o.subs;
  }
};

}  // namespace

// The stage events of a covariance entry's last call: in front of the assembly | behind it | behind cov_kernel (state covariance,
// which uses three) or cov_pose_kernel | behind the item kernel and the taps (the two-stage entries).
struct CovEvents { hipEvent_t e[4] = {nullptr, nullptr, nullptr, nullptr}; };

// What the host believes about the device.  The members are read everywhere and written HERE only: every entry that changes one
// calls a transition, and DESIGN.md (section 4c) tabulates which entry calls which.  A stale res_staged or acc_fresh does not
// crash, it hands out the previous frame's values, so a new member belongs in this record (okvis_ba_state_covariance and its
// siblings keep and restore the record as a whole).
struct HostView {
  bool uploaded = false, begun = false;
  bool evaluated = false;      // okvis_ba_begin ran since the last upload: every IMU term's cache has been (re)built
  bool acc_fresh = false;      // HostWin::acc mirrors the device's accepted-buffer index (no kernel launched since it was read)
  bool res_staged = false;     // stage_res holds window 0's packed results as of the last okvis_ba_finish (single-window solvers)
  bool mirror_fresh = false;   // the containers hold the values the device holds (nothing optimised / set since)
  long long slots = 0;         // launch slots (schur + solve + linearise triples) since okvis_ba_begin: diagnostics (ARR_DIAG_SLOTS)

  void upload_started() { uploaded = false, begun = false; }
  void upload_done() { uploaded = true, evaluated = false, res_staged = false, acc_fresh = true; }   // Ctrl starts zeroed: accepted buffer 0, like HostWin::acc
  void containers_match(bool yes) { mirror_fresh = yes; }    // taken from the caller / refreshed from the device / lost
  void values_set() { begun = false, res_staged = mirror_fresh = false; }                // okvis_ba_set_state
  void prior_values_replaced() { begun = false, evaluated = false, res_staged = false; } // okvis_ba_set_marg_prior_values
  void work_enqueued() { acc_fresh = false; }                                            // a kernel may move the accepted buffer
  void begin_entered() { acc_fresh = res_staged = mirror_fresh = false; }                // okvis_ba_begin, before its own checks
  void slots_restart() { slots = 0; }
  void slots_add(long long n) { slots += n; }
  void begin_done() { begun = true, evaluated = true; }
  void not_begun() { begun = false; }   // okvis_ba_begin was called for its linearisation alone (marginalisation, covariance)
  void iterations_enqueued() { mirror_fresh = false; }   // (a container refreshed between begin and finish is behind again)
  void finish_done(bool staged) { res_staged = staged, begun = false, acc_fresh = true, mirror_fresh = false; }
  void acc_read() { acc_fresh = true; }   // every window's accepted-buffer index was just read back
};

struct okvis_ba_solver {
  int device = 0;
  hipStream_t stream = nullptr;
  // sub-batches of windows run on their own streams so that the (latency-bound) phases of different
  // windows overlap on the 256 CUs
  std::vector<hipStream_t> sub_streams;
  std::vector<hipEvent_t> sub_events;
  hipEvent_t ev0 = nullptr, ev1 = nullptr, ev_fork = nullptr;
  okvis_ba_options opt;
  OptD* d_opt = nullptr;
  unsigned char* d_arena = nullptr;
  size_t arena_bytes = 0, arena_capacity = 0, wins_capacity = 0;
  WinPtrs* d_wins = nullptr;
  CtrlSlot* d_ctrl = nullptr;    // the control records of the uploaded windows (same allocation, behind the window records)
  const int* d_recs = nullptr;   // the chunk launch records of the uploaded windows (in the arena; BatchMax::rec_stride of them per window)
  const int* d_grecs = nullptr;  // the group launch records (in the arena; BatchMax::grec_stride of them per window)
  StageVec stage_dl;             // pinned staging of result downloads (okvis_ba_marginalize[_batch]: every window's numbers, one copy)
  StageVec stage, stage_small;   // pinned staging of the arena's data part / of the WinPtrs + OptD records (kept across uploads)
  std::vector<HostWin> wins;
  HostView host;       // what the host believes about the device: written through its transitions only
  BatchLayout layout;   // of the uploaded batch
  BatchMax max;
  LaunchPlan plan;      // (upload, set_options)
  LaunchPlan graph_plan;                // what the captured graphs were captured under: the plan ...
  std::vector<const void*> graph_addr;  // ... and the device records and streams they name (see keep_graphs)
  unsigned char* h_ctrl_stage = nullptr;   // pinned / device staging of per-window control data (begin, fetch_ctrl)
  unsigned char* d_ctrl_stage = nullptr;
  size_t ctrl_stage_bytes = 0;
  // incremental structure updates (okvis_ba_patch_window): the container of every uploaded window, kept only on request
  bool patchable = false;
  std::vector<WindowStore> mirrors;
  WindowStore mirror_edit;   // okvis_ba_patch_window edits a copy: this one
  long marg_tiles_fallbacks = 0;   // windows of okvis_ba_marginalize[_batch] calls whose tiled tail gave way to the single workgroup (diagnostics)
  StageVec stage_res;   // window 0's packed results as of the last okvis_ba_finish (HostView::res_staged)
  StageVec stage_marg;           // host-written part of okvis_ba_marginalize's scratch block
  StageVec stage_marg_vals;      // okvis_ba_set_marg_prior_values: the staged J | H0 | e0 span ...
  hipEvent_t ev_marg_vals = nullptr;   // ... and the event behind its copy
  // okvis_ba_marginalize_begin / okvis_ba_marginalize_batch_begin without its _end yet (one implementation, marg_begin / marg_end):
  // what _end needs to hand the numbers over, one item per window of the call (the kept blocks are known at begin)
  struct MargPending {
    bool active = false;
    bool batch = false;   // begun by okvis_ba_marginalize_batch_begin: ended by okvis_ba_marginalize_batch_end only, and vice versa
    struct Item {
      int w = 0, na = 0;
      size_t nn = 0, n1 = 0, out_bytes = 0;
      size_t at = 0;   // where the window's H | J | b0 | e0 | info start in stage_dl
      std::vector<int> bt, bi, bo;
    };
    std::vector<Item> items;
  } marg_pending;
  StageVec stage_pre;            // first preintegrations started at upload (imu_pre_kernel): the staged block and its device copy
  unsigned char* d_pre = nullptr;   // (PRE_MAX_TERMS records)
  long long stagger_ticks = 0;   // start offset between consecutive sub-batch streams (wall_clock64 ticks, 100 MHz); okvis_ba_tuning::stagger_us
  bool skip_topup = false;   // okvis_ba_optimize_timed ran out of time: finish() must not grant the slots mis-speculated steps still owe
  // captured graphs, keyed on the call length and the route (graph_key, capi_launch.inc); per sub-batch: (key, sub) -> its chain's graph
  std::map<int, hipGraphExec_t> graphs;
  std::map<std::pair<int, int>, hipGraphExec_t> sub_graphs;
  // ---- the three-launch iteration (LaunchPlan::three) ----
  int* h_pause = nullptr;      // pinned, device-visible: [0] bumped by every solve workgroup that pauses its window (system-scope atomic)
  int* d_pause = nullptr;      // the device's address of h_pause
  int pause_seen = 0;          // h_pause[0] as of the last entry that looked at it
  int pause_begin = 0;         // ... as of okvis_ba_begin
  bool three_unseen = false;   // a three-launch call of this begin ... finish has not been waited for yet (it may hold pauses)
  bool start_four = false;     // the previous begin ... finish paused or re-preintegrated: this one runs on the four-launch route
  int* d_redo_mark = nullptr;  // [window] sum of its terms' redo_count behind okvis_ba_begin's evaluation (grow-only)
  size_t redo_mark_windows = 0;
  float last_iterate_ms = 0.f;
  int last_hip_error = 0;
  unsigned char* marg_scratch = nullptr;  // grow-only device scratch of okvis_ba_marginalize
  CovEvents ev_cov, ev_lmcov, ev_pred;   // okvis_ba_state_covariance, okvis_ba_landmark_covariance, okvis_ba_predicted_measurement
  size_t marg_scratch_bytes = 0;
};

namespace {

// okvis_ba_marginalize_end / _batch_end first: between the two halves of a marginalisation the solver takes no edits and hands out
// no results
#define REFUSE_BETWEEN_MARG_HALVES(s) do { if ((s) && (s)->marg_pending.active) return OKVIS_BA_ERR_STATE; } while (0)

// The entry guard: what an entry requires of the solver before it does anything, as a word of these.  The statuses and their
// precedence are part of the ABI (tests/test_gpu_entry_status.py pins them), so an entry's oddity is a bit here and not a second
// copy of the checks.  In this order:
//   ENTER_MARG_FIRST   between the halves of a marginalisation: ERR_STATE, even for arguments that are ERR_ARG otherwise
//   (always)           a null solver, or `ptrs_ok` false (the entry's required pointers and counts): ERR_ARG
//   ENTER_UPLOADED     no upload: ERR_STATE - ERR_ARG with ENTER_UPLOAD_IS_ARG (okvis_ba_array_size, okvis_ba_download, ...)
//   ENTER_NO_MARG      between the halves: ERR_STATE, behind the pointers (okvis_ba_set_marg_prior_values)
//   ENTER_BEGUN        not between okvis_ba_begin and okvis_ba_finish: ERR_STATE;  `state_ok` false (the entry's own): ERR_STATE
//   ENTER_WINDOW       w outside the uploaded windows: ERR_ARG
//   ENTER_PTRS_LAST    `ptrs_ok` is looked at here and not with the null solver (okvis_ba_fetch_imu_caches)
//   ENTER_DEVICE       hipSetDevice
enum : unsigned {
  ENTER_MARG_FIRST = 1, ENTER_UPLOADED = 2, ENTER_UPLOAD_IS_ARG = 4, ENTER_NO_MARG = 8, ENTER_BEGUN = 16, ENTER_WINDOW = 32,
  ENTER_PTRS_LAST = 64, ENTER_DEVICE = 128,
  ENTER_RESULTS = ENTER_MARG_FIRST | ENTER_UPLOADED | ENTER_WINDOW | ENTER_DEVICE   // state get / set and the fetches
};
int enter(okvis_ba_solver* s, unsigned need, int w = 0, bool ptrs_ok = true, bool state_ok = true) {
  if (need & ENTER_MARG_FIRST) REFUSE_BETWEEN_MARG_HALVES(s);
  if (!s || (!ptrs_ok && !(need & ENTER_PTRS_LAST))) return OKVIS_BA_ERR_ARG;
  const bool no_upload = (need & ENTER_UPLOADED) && !s->host.uploaded;
  if (no_upload && (need & ENTER_UPLOAD_IS_ARG)) return OKVIS_BA_ERR_ARG;
  if (no_upload || ((need & ENTER_NO_MARG) && s->marg_pending.active) || ((need & ENTER_BEGUN) && !s->host.begun) || !state_ok)
    return OKVIS_BA_ERR_STATE;
  if ((need & ENTER_WINDOW) && (w < 0 || w >= (int)s->wins.size())) return OKVIS_BA_ERR_ARG;
  if (!ptrs_ok) return OKVIS_BA_ERR_ARG;
  if (need & ENTER_DEVICE) HIP_TRY(hipSetDevice(s->device));
  return OKVIS_BA_OK;
}

// staging bytes lent to a call go back to their keeper whatever happens (on = false: the call keeps its own)
struct GiveBack {
  StageVec& a;
  StageVec& b;
  bool on = true;
  ~GiveBack() {
    if (on) a.swap(b);
  }
};

int cov_events_create(okvis_ba_solver* s, CovEvents& ev) {   // (lazily, by the entry's first call)
  for (auto& e : ev.e)
    if (!e) HIP_TRY(hipEventCreate(&e));
  return OKVIS_BA_OK;
}
void cov_events_destroy(CovEvents& ev) {
  for (auto& e : ev.e)
    if (e) (void)hipEventDestroy(e);
}

size_t solve_smem_chain(int chain_doubles, int Dpad);

constexpr int FUSED_MAX_WINDOWS = 48;   // up to here the fused linearise + reduce launch beats the separate Schur launch (tools/gpu_fused_sweep.py:
                                        // 48 windows 148.5 vs 151.3 us per step, 64 windows 176 vs 163)
// (okvis_ba_tuning::fused_max_windows overrides it: A/B sweeps)
int fused_max_windows(const okvis_ba_options& o) {
  return o.tuning.fused_max_windows > 0 ? o.tuning.fused_max_windows : o.tuning.fused_max_windows < 0 ? 0 : FUSED_MAX_WINDOWS;
}
// the options ask for a mode whose damping does not depend on the accept / reject decision (DOGLEG, or Gauss-Newton's fixed radius)
inline bool decision_free(const okvis_ba_options& o) { return o.strategy == OKVIS_BA_STRATEGY_DOGLEG || o.gauss_newton; }
// the Schur reduction may run on the fp64 matrix core (OKVIS_BA_TUNE_SCHUR_VALU keeps schur_kernel)
inline bool schur_mfma_allowed(const okvis_ba_options& o) { return !(o.tuning.flags & OKVIS_BA_TUNE_SCHUR_VALU); }
// a pose part of Dp rows fits the small tiles of the matrix-core Schur kernel (schur_mfma_kernel<3>)
inline bool schur_small_tiles(int Dp) { return std::min(TILE_DIM, Dp) + 1 <= SCH2_MAXT_SMALL_ROWS; }
// Print-only diagnostics: the ONE environment variable the library reads, once per process.  OKVIS_BA_DEBUG is a comma-separated
// list of "build" (host time of build_window's sections, printed at exit), "upload" (sections of every upload), "marg" (ranks and
// bounds of every marginalisation), "arena=<file>" (okvis_ba_check_window dumps the index build's output).  Nothing here changes a
// result; everything that does is a field of okvis_ba_options::tuning.
struct DebugWord {
  bool build = false, upload = false, marg = false;
  std::string arena;
  DebugWord() {
    const char* e = std::getenv("OKVIS_BA_DEBUG");
    if (!e) return;
    std::string w(e);
    size_t at = 0;
    while (at <= w.size()) {
      size_t c = w.find(',', at);
      if (c == std::string::npos) c = w.size();
      const std::string tok = w.substr(at, c - at);
      if (tok == "build") build = true;
      else if (tok == "upload") upload = true;
      else if (tok == "marg") marg = true;
      else if (tok.rfind("arena=", 0) == 0) arena = tok.substr(6);
      at = c + 1;
    }
  }
};
const DebugWord& debug_word() {
  static const DebugWord w;
  return w;
}
constexpr size_t OPT_PAD = (sizeof(OptD) + 255) & ~size_t(255);   // the option record in front of the window records (one allocation, one copy)
// [OptD, padded | WinPtrs x n | (padded) CtrlSlot x n]: where the control records of n windows start / how long the block is
constexpr size_t ctrl_off(size_t n) { return (OPT_PAD + sizeof(WinPtrs) * n + 255) & ~size_t(255); }
constexpr size_t records_bytes(size_t n) { return ctrl_off(n) + sizeof(CtrlSlot) * n; }
constexpr int SMALL_BATCH_WINDOWS = 40;   // below: the device is not full - settings that shorten one window's chain win

OptD make_optd(const okvis_ba_options& o, int n_windows) {
  OptD d;
  d.initial_radius = o.initial_radius;
  d.max_radius = o.max_radius;
  d.min_radius = o.min_radius;
  d.min_lm_diag2 = o.min_lm_diagonal;   // Ceres clamps the squared column norm itself to [min_lm_diagonal, max_lm_diagonal]
  d.max_lm_diag2 = o.max_lm_diagonal;
  d.min_relative_decrease = o.min_relative_decrease;
  d.function_tolerance = o.function_tolerance;
  d.gradient_tolerance = o.gradient_tolerance;
  d.parameter_tolerance = o.parameter_tolerance;
  d.gauss_newton = o.gauss_newton;
  d.marg_mode = 0;
  d.dogleg = o.strategy == OKVIS_BA_STRATEGY_DOGLEG;
  d.jacobi_scaling = o.jacobi_scaling != 0;
  d.max_invalid = o.max_consecutive_invalid_steps > 0 ? o.max_consecutive_invalid_steps : 5;
  d.helper_polls = (o.reserved0 & 16) ? 0 : 1 << 22;   // (bit 4: the test of the time-out route gives up at once)
  return d;
}

void destroy_graphs(okvis_ba_solver* s) {
  for (auto& kv : s->graphs) (void)hipGraphExecDestroy(kv.second);
  s->graphs.clear();
  for (auto& kv : s->sub_graphs) (void)hipGraphExecDestroy(kv.second);
  s->sub_graphs.clear();
}
// Captured graphs hold the plan's launches, the addresses of the window / option / control / chunk launch records and the sub-batch streams: a
// re-upload or an option change that leaves all of that as it was (equally shaped windows: the per-frame pattern) keeps them.
void keep_graphs(okvis_ba_solver* s) {
  std::vector<const void*> addr = {s->d_wins, s->d_opt, s->d_ctrl, s->d_recs, s->d_grecs};
  for (auto st : s->sub_streams) addr.push_back(st);
  if (s->plan == s->graph_plan && addr == s->graph_addr) return;
  destroy_graphs(s);
  s->graph_plan = s->plan;
  s->graph_addr.swap(addr);
}

}  // namespace
