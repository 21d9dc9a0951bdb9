// Part of ba_capi.hip (see capi_solver.inc).  Dynamic LDS sizes, the launch plan (make_plan: where every launch route is decided) and
// the launches that read it: Schur, solve, factors + linearise, the sub-batch fork / join; the control-record fetch.
namespace {

size_t lin_smem(bool ext, bool f32 = false) {
  const int d = f32 ? (ext ? LinCfg<true, float>::SMEM_DOUBLES : LinCfg<false, float>::SMEM_DOUBLES)
                    : (ext ? LinCfg<true, double>::SMEM_DOUBLES : LinCfg<false, double>::SMEM_DOUBLES);
  return (size_t)d * sizeof(double);
}
size_t solve_smem(int Dpad, bool large) {
  // LDS-resident: the matrix area of the LDL^T solver (ba_ldl16.hpp; Dpad >= D bounds it) + four vectors
  return ((large ? 0 : (size_t)ldl16_area_doubles(Dpad)) + 4 * (size_t)Dpad) * sizeof(double) + 16;
}
// chain solver (ba_chain.hpp): its matrix area (LChain::total of the batch's largest window) + the four vectors
size_t solve_smem_chain(int chain_doubles, int Dpad) { return ((size_t)chain_doubles + 4 * (size_t)Dpad) * sizeof(double) + 16; }
// dynamic LDS of linearize2_kernel: fixed part + the pose part of the step (fused: the aux area of the group reduction)
int lin2_step_doubles(int max_Dp, bool fuse, bool f32) {
  const int aux = fuse ? (f32 ? Lin2Cfg<float, true>::MIN_STEP_DOUBLES : Lin2Cfg<double, true>::MIN_STEP_DOUBLES) : Lin2Cfg<double, false>::MIN_STEP_DOUBLES;
  return ((max_Dp + 1) / 2) * 2 + 8 + aux;   // pose part of the step, then the aux area of the fused reduction
}
size_t lin2_smem(int max_Dp, bool fuse, bool f32, bool two_rounds = false) {
  const int fixed = two_rounds ? (f32 ? Lin2Cfg<float, false, 14>::FIXED_DOUBLES : Lin2Cfg<double, false, 14>::FIXED_DOUBLES)
                    : f32 ? (fuse ? Lin2Cfg<float, true>::FIXED_DOUBLES : Lin2Cfg<float, false>::FIXED_DOUBLES)
                          : (fuse ? Lin2Cfg<double, true>::FIXED_DOUBLES : Lin2Cfg<double, false>::FIXED_DOUBLES);
  return (size_t)(fixed + lin2_step_doubles(max_Dp, fuse, f32)) * sizeof(double);
}
size_t small_smem() { return (size_t)std::max<int>(std::max<int>(ImuLds::TOTAL, EvalLds::TOTAL), 2 * MAX_MARG_DIM) * sizeof(double); }

size_t small_eval_smem() { return (size_t)std::max<int>(EvalLds::TOTAL, 2 * MAX_MARG_DIM) * sizeof(double); }

// landmarks per batch of the serial loop of the matrix-core Schur kernel for tiles of trows rows
int sch2_serial_nlb(int trows) {
  const int nlb = sch2_nlb(trows, 5120);             // 40 KB of tiles: three workgroups per CU
  return nlb < 12 ? sch2_nlb(trows, 9216) : nlb;     // wide tiles: 72 KB, two per CU
}

// Every instantiation a launch plan can name, with the most dynamic LDS a plan gives it (okvis_ba_create allows it that much).
// It comes first on purpose: the first reference to a kernel template in this file fixes where its code lands in the code object,
// and this is the order the launches have always named them in (the same code layout, the same timing).
std::vector<std::pair<const void*, size_t>> plan_kernels() {
  auto f = [](auto k) { return reinterpret_cast<const void*>(k); };
  const size_t dense = std::max(solve_smem(((MAX_D_LDS + 5) / 6) * 6, false), (size_t)SOLVE_LDS_LIMIT), chain = SOLVE_LDS_LIMIT_CHAIN;
  // (the serial tiles of every pose part make_plan can meet: 66 - 78 rows stage 16 landmarks a batch, 62.7 KB — more than the 12 of a
  //  96-row tile, 61.6 KB)
  size_t wide = 0;
  for (int t = 1; t <= TILE_DIM; ++t) wide = std::max(wide, (size_t)sch2_tile_doubles(t, sch2_serial_nlb(t)) * sizeof(double));
  const size_t d = std::max(lin2_smem(MAX_D, true, false), small_smem()), s = std::max(lin2_smem(MAX_D, true, true), small_smem());
  const size_t ef = std::max(lin_smem(true, true), small_smem()), ed = std::max(lin_smem(true), small_smem());
  const size_t pf = std::max(lin_smem(false, true), small_smem()), pd = std::max(lin_smem(false), small_smem());
  return {{f(&solve_kernel<false, true, true>), chain}, {f(&solve_kernel<false, false, true>), chain},
          {f(&solve_kernel<false, true>), dense}, {f(&solve_kernel<false, false>), dense},
          {f(&schur_ride_kernel<3>), std::max(wide, small_eval_smem())}, {f(&schur_mfma_kernel<3>), wide}, {f(&schur_mfma_kernel<9>), wide},
          {f(&schur_kernel), 2 * SCHUR_LM_BATCH * TILE_DIM * 3 * sizeof(double)},
          {f(&solve_kernel<true, false>), solve_smem(((MAX_D + 5) / 6) * 6, true)},
          {f(&small_kernel), small_smem()}, {f(&small_prepare_kernel), small_smem()},
          {f(&linearize2_kernel<float, true, false>), s}, {f(&linearize2_kernel<float, false, false, 4, 14>), s},
          {f(&linearize2_kernel<float, false, false, 3>), s}, {f(&linearize2_kernel<double, true, false>), d},
          {f(&linearize2_kernel<double, false, false, 4, 14>), d}, {f(&linearize2_kernel<double, false, false, 3>), d},
          {f(&linearize2_kernel<float, true, true>), s}, {f(&linearize2_kernel<float, false, true>), s},
          {f(&linearize2_kernel<double, true, true>), d}, {f(&linearize2_kernel<double, false, true>), d},
          {f(&linearize_kernel<true, float, true>), ef}, {f(&linearize_kernel<true, float, false>), ef},
          {f(&linearize_kernel<true, double, true>), ed}, {f(&linearize_kernel<true, double, false>), ed},
          {f(&linearize_kernel<false, float, true>), pf}, {f(&linearize_kernel<false, float, false>), pf},
          {f(&linearize_kernel<false, double, true>), pd}, {f(&linearize_kernel<false, double, false>), pd},
          // (the serial batch loop of the small tiles: the referee of the pipelined one, OKVIS_BA_TUNE_SCHUR_SERIAL_BATCHES)
          {f(&schur_ride_kernel<3, true>), std::max(wide, small_eval_smem())}, {f(&schur_mfma_kernel<3, true>), wide},
          // (the record instantiations of the piece path, behind everything that was there before them)
          {f(&linearize2_rec_kernel<double, 3>), d}, {f(&linearize2_rec_kernel<double, 4, 14>), d},
          {f(&linearize2_rec_kernel<float, 3>), s}, {f(&linearize2_rec_kernel<float, 4, 14>), s},
          // (the ring loop's instantiations for the decision-free launch of an iteration: V^-1 in front of the first barrier)
          {f(&schur_ride_kernel<3, false, true>), std::max(wide, small_eval_smem())}, {f(&schur_mfma_kernel<3, false, true>), wide}};
}

// ---- The instantiations a launch plan names (Launch::k is the index in the table of its kind) ----
using LinFn = decltype(&linearize_kernel<false, double, false>);
using Lin2Fn = decltype(&linearize2_kernel<double, false, true>);
using SolveFn = decltype(&solve_kernel<false, false>);
// the staged kernel (ba_linearize.hpp): [4 * free extrinsics + 2 * fp32 + fused]
const LinFn LIN[8] = {&linearize_kernel<false, double, false>, &linearize_kernel<false, double, true>, &linearize_kernel<false, float, false>,
                      &linearize_kernel<false, float, true>,   &linearize_kernel<true, double, false>,  &linearize_kernel<true, double, true>,
                      &linearize_kernel<true, float, false>,   &linearize_kernel<true, float, true>};
// the piece path (ba_linearize2.hpp): [5 * fp32 + LIN2_*]
enum { LIN2_FUSED, LIN2_FUSED_SMALL, LIN2_SMALL, LIN2_OCC3, LIN2_OCC4 };
const Lin2Fn LIN2[10] = {&linearize2_kernel<double, true, false>, &linearize2_kernel<double, true, true>, &linearize2_kernel<double, false, true>,
                         &linearize2_kernel<double, false, false, 3>, &linearize2_kernel<double, false, false, 4, 14>,
                         &linearize2_kernel<float, true, false>, &linearize2_kernel<float, true, true>, &linearize2_kernel<float, false, true>,
                         &linearize2_kernel<float, false, false, 3>, &linearize2_kernel<float, false, false, 4, 14>};
// ... and its record instantiations (group launch records; LIN2_OCC3 / LIN2_OCC4 only): [2 * fp32 + (LIN2_* - LIN2_OCC3)]
using Lin2RecFn = decltype(&linearize2_rec_kernel<double, 3>);
const Lin2RecFn LIN2R[4] = {&linearize2_rec_kernel<double, 3>, &linearize2_rec_kernel<double, 4, 14>, &linearize2_rec_kernel<float, 3>,
                            &linearize2_rec_kernel<float, 4, 14>};
// the reduced solve: the LDS-resident windows (dense or chain; DBUF: one set of Schur partials per linearisation buffer), the tiled ones
enum { SOLVE_NONE, SOLVE_DENSE, SOLVE_DENSE_DBUF, SOLVE_CHAIN, SOLVE_CHAIN_DBUF, SOLVE_TILED };
const SolveFn SOLVE[6] = {nullptr, &solve_kernel<false, false>, &solve_kernel<false, true>, &solve_kernel<false, false, true>,
                          &solve_kernel<false, true, true>, &solve_kernel<true, false>};
// the Schur launch (the first four: OKVIS_BA_ROUTE_SCHUR_KERNEL) and the factors' own launch (their kernels' arguments differ)
enum { SCHUR_NONE, SCHUR_VALU, SCHUR_MFMA3, SCHUR_MFMA9, SCHUR_RIDE3, SCHUR_MFMA3_SERIAL, SCHUR_RIDE3_SERIAL };
enum { SMALL_NONE, SMALL_ALL, SMALL_PREPARE };
// The launch plan (LaunchPlan) of a batch of n_windows laid out by L whose windows have the maxima M, under the options o.  Host only:
// okvis_ba_upload computes it, okvis_ba_set_options again for the options of an uploaded batch, and every launch of the solver reads
// it.  The layout fixed at upload bounds what later options can select: a batch uploaded under LM keeps its deciding Schur launch
// after a switch to DOGLEG.
Extent make_extent(int w0, int nw) { return Extent{w0, nw, nw <= SOLVE_HELPED_MAX_WINDOWS ? SOLVE_HELPERS : 0}; }
LaunchPlan make_plan(const BatchLayout& L, const BatchMax& M, const okvis_ba_options& o, int n_windows) {
  LaunchPlan p;
  const bool f32 = o.fp32_linearize != 0;
  // fused mode: linearise reduces its groups, no Schur launch (the reduction was sized at upload for one precision's stage)
  p.fused = M.group_chunks && f32 == L.fp32 && decision_free(o);
  // the decision-free Schur launch (BatchMax::spec_schur) while the options still ask for a mode that allows it
  p.nodec = M.spec_schur && !p.fused && decision_free(o);
  p.lin2 = L.lin2, p.split_small = L.split_small, p.graph = o.use_graph != 0;
  p.n_small = M.imu + 1;
  // ---- Schur.  No pose x extrinsics cross blocks: the reduction as a GEMM on the fp64 matrix core (ba_schur2.hpp).  Pose parts
  //      beyond 63 rows (several 96-row tile pairs per chunk) keep schur_kernel unless OKVIS_BA_TUNE_SCHUR_MFMA_LARGE is set: every
  //      tile pair of a chunk scans all its (landmark, block) rows to fill its tiles, and at configs[2] that makes the matrix-core
  //      kernel the slower one (111 against 100 us per launch) ----
  p.trows = std::min(TILE_DIM, M.Dp);
  if (M.schur_blocks > 0 && !p.fused) {
    const bool small_tiles = schur_small_tiles(M.Dp);
    if (!M.any_ext && schur_mfma_allowed(o) && (small_tiles || (o.tuning.flags & OKVIS_BA_TUNE_SCHUR_MFMA_LARGE))) {
      p.nlb = sch2_serial_nlb(p.trows);
      // the small tiles: stages of four landmarks pipelined over a ring of three tile sets (39 KB at 60 rows: three per CU as well);
      // OKVIS_BA_TUNE_SCHUR_SERIAL_BATCHES keeps the batch loop above as the referee
      // (the ring loop's workgroups start from the batch's chunk launch records: a batch without them keeps the serial loop)
      const bool serial = !small_tiles || M.rec_stride == 0 || (o.tuning.flags & OKVIS_BA_TUNE_SCHUR_SERIAL_BATCHES);
      p.rec_stride = serial ? 0 : M.rec_stride;
      if (!serial) p.nlb = SCH2_STAGE_LM;
      const int sm = (serial ? sch2_tile_doubles(p.trows, p.nlb) : sch2_ring_doubles(p.trows)) * (int)sizeof(double);
      // The EVALUATION of the IMU / prior factors rides in the decision-free launch with the small tiles (schur_ride_kernel) where
      // they have a launch of their own (piece path, batches of 40 windows and more): small_prepare_kernel right behind the solve
      // launch keeps what may change a preintegration record, the rest leaves the chain of the sub-batch.
      // okvis_ba_tuning::flags & OKVIS_BA_TUNE_NO_SMALL_RIDE: the whole factors in small_kernel as until round 6.
      p.rides = small_tiles && p.nodec && L.split_small && !(o.tuning.flags & OKVIS_BA_TUNE_NO_SMALL_RIDE);
      if (p.rides) p.schur = Launch{serial ? SCHUR_RIDE3_SERIAL : SCHUR_RIDE3, p.n_small + M.schur_blocks, std::max(sm, (int)small_eval_smem())};
      else p.schur = Launch{!small_tiles ? SCHUR_MFMA9 : serial ? SCHUR_MFMA3_SERIAL : SCHUR_MFMA3, M.schur_blocks, sm};
    } else {
      p.schur = Launch{SCHUR_VALU, M.schur_blocks, (int)(2 * SCHUR_LM_BATCH * p.trows * 3 * sizeof(double))};
    }
  }
  if (M.Dpad_small > 0)   // (DBUF: one set of partials per linearisation buffer)
    p.solve = Launch{(M.chain ? SOLVE_CHAIN : SOLVE_DENSE) + (M.group_chunks || M.spec_schur), 0,
                     (int)(M.chain ? solve_smem_chain(M.chain_doubles, M.Dpad_small) : solve_smem(M.Dpad_small, false))};
  if (M.Dpad_large > 0) {   // large windows: assemble + export, tiled multi-workgroup Cholesky (fp64 MFMA), back-substitution + finish
    p.tiled = Launch{SOLVE_TILED, 0, (int)solve_smem(M.Dpad_large, true)};
    p.nT = (M.Dpad_large + CT_TB - 1) / CT_TB;
  }
  // ---- IMU / prior factors and linearise: one launch for everything that depends only on the trial state (factors first) ----
  const Launch small{SMALL_ALL, p.n_small, (int)small_smem()};
  if (L.lin2) {
    const int t = f32 ? 5 : 0, smem2 = (int)lin2_smem(M.Dp, p.fused, f32);
    p.sd = lin2_step_doubles(M.Dp, p.fused, f32);
    if (L.split_small) {
      // (the initial evaluation keeps the whole factors: okvis_ba_begin is followed by a Schur launch too, whose riding workgroups then
      //  evaluate the same states again — the same bits)
      p.small_init = small;
      p.small_iter = !p.rides ? small : M.imu > 0 ? Launch{SMALL_PREPARE, M.imu, (int)small_smem()} : Launch{};
      const int occ = o.tuning.lin2_occupancy > 0 ? o.tuning.lin2_occupancy : 4;
      const bool two_rounds = !p.fused && occ >= 4;   // block records in two rounds: 37 KB of LDS, four workgroups per CU
      p.lin = Launch{t + (p.fused ? LIN2_FUSED : occ >= 4 ? LIN2_OCC4 : LIN2_OCC3), M.group,
                     two_rounds ? (int)lin2_smem(M.Dp, false, f32, true) : smem2};
      // the workgroups of the unfused launch start from the batch's group launch records (linearize2_rec_kernel); a batch without
      // them, and OKVIS_BA_TUNE_LIN_NO_RECORDS (the referee), keep linearize2_kernel, which reads through the window record
      if (!p.fused && M.grec_stride > 0 && !(o.tuning.flags & OKVIS_BA_TUNE_LIN_NO_RECORDS)) p.grec_stride = M.grec_stride;
    } else {
      p.lin = Launch{t + (p.fused ? LIN2_FUSED_SMALL : LIN2_SMALL), p.n_small + M.group, std::max(smem2, (int)small_smem())};
      p.lin_n_small = p.n_small;
    }
  } else {
    p.lin = Launch{4 * M.any_ext + 2 * f32 + p.fused, p.n_small + M.group, (int)std::max(lin_smem(M.any_ext, f32), small_smem())};
    p.lin_n_small = p.n_small;
  }
  // the preintegrations a discarded speculative evaluation left behind (DOGLEG), taken back before results leave the device
  if (M.imu > 0 && o.strategy == OKVIS_BA_STRATEGY_DOGLEG && !o.gauss_newton) p.take_back = Launch{1, M.imu, 0};
  p.budget = o.strategy == OKVIS_BA_STRATEGY_DOGLEG;
  // The three-launch iteration: where the factors' launch of an iteration is small_prepare_kernel alone, that launch does nothing
  // while no IMU term needs a new preintegration.  The solve kernel's tail finds out (its DBUF instantiations, which the riding
  // route always names) and pauses the windows that need it; the host adds the launch for them (resume_paused).  It takes the
  // iteration budget (a paused window is level again after the slots it owes) and windows of at most PAUSE_MAX_TERMS IMU terms
  // solved in LDS.  okvis_ba_tuning::flags & OKVIS_BA_TUNE_FOUR_LAUNCH keeps small_prepare_kernel in every slot (the referee).
  p.three = p.small_iter.k == SMALL_PREPARE && p.budget && M.imu <= PAUSE_MAX_TERMS && p.solve.k != SOLVE_NONE && p.tiled.k == SOLVE_NONE &&
            !(o.tuning.flags & OKVIS_BA_TUNE_FOUR_LAUNCH);
  // ---- sub-batches: opt.n_streams (0 = auto).  Measured at 64 windows (scripts/sweep_streams.sh, r02): 1 stream 272 k,
  //      2: 300 k, 3: 325 k, 4: 198 k window-iterations/s — the streams of the process that have work, or ever had, must not
  //      exceed four (whatever GPU_MAX_HW_QUEUES and the stream priorities say: scripts/r06_streams.sh, r06_streams2.sh,
  //      tools/micro/stream_concurrency.hip).
  //      Measured on MI355X / ROCm 7.2 (profiles/r01_notes.md): branches inside ONE captured graph are not overlapped, but two
  //      independently replayed graphs on two streams are (+29 % at 64 windows); more than two streams lose again.
  //      (round 6, profiles/r06_notes.md: from 128 windows on two streams are ahead again — 128: 613 k against 601 k, 256: 692 k
  //      against 659 k, 512: 727 k against 700 k window-iterations/s; 96 windows: three, 568 k against 549 k) ----
  int nsub = o.n_streams > 0 ? o.n_streams : (n_windows >= 128 ? 2 : (n_windows >= 56 ? 3 : (n_windows >= 8 ? 2 : 1)));   // (48 windows: 2 is better)
  nsub = std::max(1, std::min(nsub, n_windows));
  // helper workgroups per window sum the Schur chunk partials for the solving one; launches of more windows sum inside the
  // solving workgroup (a helper takes a whole CU)
  auto extent = [](int w0, int nw) { return make_extent(w0, nw); };
  for (int k = 0; k < nsub; ++k) {
    const int w0 = (int)((int64_t)n_windows * k / nsub), w1 = (int)((int64_t)n_windows * (k + 1) / nsub);
    p.subs.push_back(extent(w0, w1 - w0));
  }
  p.whole = extent(0, n_windows);
  p.one_helpers = extent(0, 1).helpers;
  return p;
}

// okvis_ba_begin for every window in ONE launch (it used to be three device copies and one upload per window: 1 ms of API calls
// for 64 windows): the trial buffers start as copies of the accepted ones, the control record starts a new optimisation.
// `accs[w]` = the accepted buffer as the host knows it (okvis_ba_set_state wrote there).
__global__ void begin_kernel(const WinPtrs* wins, const int* accs, double initial_radius) {
  const WinPtrs& W = wins[blockIdx.x];
  const int acc = accs[blockIdx.x], tr = 1 - acc, tid = threadIdx.x;
  for (int i = tid; i < 7 * W.n_pose; i += blockDim.x) W.pose[tr][i] = W.pose[acc][i];
  for (int i = tid; i < 9 * W.n_sb; i += blockDim.x) W.sb[tr][i] = W.sb[acc][i];
  for (int i = tid; i < 4 * W.n_lm; i += blockDim.x) W.lm[tr][i] = W.lm[acc][i];
  if (tid == 0) {
    Ctrl c;
    for (size_t k = 0; k < sizeof(Ctrl) / 8; ++k) reinterpret_cast<double*>(&c)[k] = 0.0;
    c.acc = acc;
    c.pending = 1;
    c.first = 1;
    c.radius = initial_radius;
    c.decrease_factor = 2.0;
    c.lambda = 1.0 / initial_radius;
    c.mu = DL_MIN_MU;
    *W.ctrl = c;
  }
}
// the control records of all windows into one contiguous array (one device-to-host copy instead of one per window)
// (redo_mark != nullptr: the copy's spare word pad2 = the re-preintegrations of the window's IMU terms since redo_mark_kernel)
__global__ void gather_ctrl_kernel(const WinPtrs* wins, Ctrl* out, int n, const int* redo_mark) {
  const int w = blockIdx.x * (blockDim.x / 64) + threadIdx.x / 64, lane = threadIdx.x & 63;
  if (w >= n) return;
  constexpr int last = (int)(sizeof(Ctrl) / 8) - 1;   // (have_tot | pad2)
  static_assert(offsetof(Ctrl, pad2) == sizeof(Ctrl) - 4, "the spare word closes the record");
  if (lane > last) return;
  union { double d; int i[2]; } v;
  v.d = reinterpret_cast<const double*>(wins[w].ctrl)[lane];
  if (redo_mark && lane == last) {   // (a dozen terms: the work-item that copies the word)
    int r = 0;
    for (int f = 0; f < wins[w].n_imu; ++f) r += wins[w].imu_cache[f].redo_count;
    v.i[1] = r - redo_mark[w];
  }
  reinterpret_cast<double*>(out + w)[lane] = v.d;
}
// the re-preintegrations every window has seen so far (behind okvis_ba_begin's evaluation: what the iterations add is what counts)
__global__ void redo_mark_kernel(const WinPtrs* wins, int* redo_mark, int n) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w >= n) return;
  int r = 0;
  for (int f = 0; f < wins[w].n_imu; ++f) r += wins[w].imu_cache[f].redo_count;
  redo_mark[w] = r;
}
// a paused window runs again (its trial is still pending: the factors' launch and linearise come next)
__global__ void resume_kernel(const WinPtrs* wins, int n) {
  const int w = blockIdx.x * blockDim.x + threadIdx.x;
  if (w < n && wins[w].ctrl->done == DONE_PAUSED) wins[w].ctrl->done = 0;
}

// keeps one wave busy for `ticks` of the 100 MHz wall clock (the start stagger of the sub-batch streams)
__global__ void delay_kernel(long long ticks) {
  const long long t0 = wall_clock64();
  while (wall_clock64() - t0 < ticks) __builtin_amdgcn_s_sleep(32);
}

struct Sub { hipStream_t st; int w0, nw, helpers; };   // the windows of one launch (Extent) and its stream
Sub sub(hipStream_t st, const Extent& e) { return Sub{st, e.w0, e.nw, e.helpers}; }
Sub whole(okvis_ba_solver* s) { return sub(s->stream, s->plan.whole); }

// ---- The launches, each as the plan has it ----
// damped: the launch of an iteration (lambda from the control words).  The eliminations of the marginalisation and of the covariance
// entries (OptD::marg_mode, schur_and_export) take no damping and keep the instantiations that hold their inverses.
hipError_t launch_schur(okvis_ba_solver* s, Sub b, int final_call = 0, bool damped = true) {
  const LaunchPlan& p = s->plan;
  const bool free_ring = p.nodec && damped;   // (ring instantiations: the decision-free prologue, ba_schur2.hpp)
  const dim3 grid((unsigned)p.schur.gx, (unsigned)b.nw), blk(SCHUR_THREADS);
  const WinPtrs* wins = s->d_wins + b.w0;
  const CtrlSlot* ctrls = s->d_ctrl + b.w0;
  // (the ring instantiations only: the records of window b.w0 onwards, p.rec_stride of them per window)
  const int* recs = p.rec_stride ? s->d_recs + (size_t)b.w0 * p.rec_stride * SCHUR_REC_INTS : nullptr;
  switch (p.schur.k) {
    case SCHUR_NONE: return hipSuccess;
    case SCHUR_VALU: hipLaunchKernelGGL(schur_kernel, grid, blk, p.schur.lds, b.st, wins, s->d_opt, p.trows, final_call); break;
    case SCHUR_MFMA3:
      if (free_ring) hipLaunchKernelGGL((schur_mfma_kernel<3, false, true>), grid, blk, p.schur.lds, b.st, wins, s->d_opt, p.trows, final_call, p.nlb, ctrls, p.nodec, recs, p.rec_stride);
      else hipLaunchKernelGGL(schur_mfma_kernel<3>, grid, blk, p.schur.lds, b.st, wins, s->d_opt, p.trows, final_call, p.nlb, ctrls, p.nodec, recs, p.rec_stride); break;
    case SCHUR_MFMA9: hipLaunchKernelGGL(schur_mfma_kernel<9>, grid, blk, p.schur.lds, b.st, wins, s->d_opt, p.trows, final_call, p.nlb, ctrls, p.nodec, recs, p.rec_stride); break;
    case SCHUR_RIDE3:
      if (free_ring) hipLaunchKernelGGL((schur_ride_kernel<3, false, true>), grid, blk, p.schur.lds, b.st, wins, s->d_opt, p.trows, final_call, p.nlb, ctrls, p.nodec, p.n_small, recs, p.rec_stride);
      else hipLaunchKernelGGL(schur_ride_kernel<3>, grid, blk, p.schur.lds, b.st, wins, s->d_opt, p.trows, final_call, p.nlb, ctrls, p.nodec, p.n_small, recs, p.rec_stride); break;
    case SCHUR_MFMA3_SERIAL: hipLaunchKernelGGL((schur_mfma_kernel<3, true>), grid, blk, p.schur.lds, b.st, wins, s->d_opt, p.trows, final_call, p.nlb, ctrls, p.nodec, recs, p.rec_stride); break;
    case SCHUR_RIDE3_SERIAL: hipLaunchKernelGGL((schur_ride_kernel<3, true>), grid, blk, p.schur.lds, b.st, wins, s->d_opt, p.trows, final_call, p.nlb, ctrls, p.nodec, p.n_small, recs, p.rec_stride); break;
  }
  return hipGetLastError();
}
// one solve_kernel launch (l: the plan's solve or tiled) on the window records `wins`
// (pause: the three-launch iteration's word, nullptr on every other route and in every launch that is not an iteration's)
void launch_solve_kernel(okvis_ba_solver* s, const Launch& l, dim3 grid, hipStream_t st, const WinPtrs* wins, int final_only, CtrlSlot* ctrls,
                         int* pause = nullptr) {
  const SolveFn fn = SOLVE[l.k];
  hipLaunchKernelGGL(fn, grid, dim3(SOLVE_THREADS), l.lds, st, wins, s->d_opt, final_only, ctrls, pause);
}
hipError_t launch_solve(okvis_ba_solver* s, Sub b, int final_only, int* pause = nullptr) {
  const LaunchPlan& p = s->plan;
  if (p.solve.k) launch_solve_kernel(s, p.solve, dim3((unsigned)b.nw, 1 + b.helpers), b.st, s->d_wins + b.w0, final_only, s->d_ctrl + b.w0, pause);
  if (p.tiled.k) {
    launch_solve_kernel(s, p.tiled, dim3((unsigned)b.nw), b.st, s->d_wins + b.w0, final_only, s->d_ctrl + b.w0);
    if (!final_only) {
      const int nT = p.nT;   // (Cholesky tiles per dimension)
      hipLaunchKernelGGL(large_export_kernel, dim3(nT * (nT + 1) / 2, (unsigned)b.nw, CT_TILE / CT_THREADS), dim3(CT_THREADS), 0, b.st,
                         s->d_wins + b.w0);
      hipLaunchKernelGGL(chol_tiles_window_kernel, dim3(nT * (nT + 1) / 2 + nT, (unsigned)b.nw), dim3(CT_THREADS), CT_SMEM_DOUBLES * 8,
                         b.st, s->d_wins + b.w0);
      hipLaunchKernelGGL(solve_large_tail_kernel, dim3((unsigned)b.nw), dim3(SOLVE_THREADS), 0, b.st, s->d_wins + b.w0, s->d_opt);
    }
  }
  return hipGetLastError();
}
// the IMU / prior factors' launch of their own (init: okvis_ba_begin's), then the linearise launch
// (factors = false: the three-launch iteration, whose small_iter — small_prepare_kernel — runs only for windows that paused)
hipError_t launch_lin(okvis_ba_solver* s, Sub b, int init, bool factors = true) {
  const LaunchPlan& p = s->plan;
  const WinPtrs* wins = s->d_wins + b.w0;
  const Launch none;
  const Launch& f = !factors ? none : init ? p.small_init : p.small_iter;
  if (f.k == SMALL_ALL) hipLaunchKernelGGL(small_kernel, dim3((unsigned)f.gx, (unsigned)b.nw), dim3(LIN_THREADS), f.lds, b.st, wins, init);
  if (f.k == SMALL_PREPARE) hipLaunchKernelGGL(small_prepare_kernel, dim3((unsigned)f.gx, (unsigned)b.nw), dim3(LIN_THREADS), f.lds, b.st, wins);
  const dim3 grid((unsigned)p.lin.gx, (unsigned)b.nw);
  if (p.lin2 && p.grec_stride) {
    // (the records of window b.w0 onwards, p.grec_stride of them per window; the control records as in launch_schur)
    const Lin2RecFn fn = LIN2R[2 * (p.lin.k >= 5) + (p.lin.k % 5 - LIN2_OCC3)];
    hipLaunchKernelGGL(fn, grid, dim3(LIN_THREADS), p.lin.lds, b.st, wins, s->d_opt, init, p.sd, s->d_ctrl + b.w0,
                       s->d_grecs + (size_t)b.w0 * p.grec_stride * LIN_REC_INTS, p.grec_stride);
  } else if (p.lin2) {
    const Lin2Fn fn = LIN2[p.lin.k];
    hipLaunchKernelGGL(fn, grid, dim3(LIN_THREADS), p.lin.lds, b.st, wins, s->d_opt, init, p.lin_n_small, p.sd);
  } else {
    const LinFn fn = LIN[p.lin.k];
    hipLaunchKernelGGL(fn, grid, dim3(LIN_THREADS), p.lin.lds, b.st, wins, s->d_opt, init, p.lin_n_small);
  }
  return hipGetLastError();
}
hipError_t launch_imu_take_back(okvis_ba_solver* s, int w0, int nw) {
  if (!s->plan.take_back.k) return hipSuccess;
  hipLaunchKernelGGL(imu_take_back_kernel, dim3((unsigned)s->plan.take_back.gx, (unsigned)nw), dim3(64), 0, s->stream, s->d_wins + w0);
  return hipGetLastError();
}
// One iteration on the plan's route.  four = false asks for the three-launch iteration where the plan has it (LaunchPlan::three):
// Schur -> solve (with the pause check) -> linearise; otherwise every launch of the plan (four of them where three exists: the referee
// and the fall-back).
hipError_t launch_iteration(okvis_ba_solver* s, Sub b, bool four) {
  const bool three = s->plan.three && !four;
  hipError_t e;
  if ((e = launch_schur(s, b)) != hipSuccess) return e;
  if ((e = launch_solve(s, b, 0, three ? s->d_pause : nullptr)) != hipSuccess) return e;
  return launch_lin(s, b, 0, !three);
}
// captured graphs are keyed on the call length and the route
inline int graph_key(int n, bool four) { return 2 * n + (four ? 1 : 0); }
hipError_t launch_budget(okvis_ba_solver* s, Sub b, int n) {
  if (!s->plan.budget || n <= 0) return hipSuccess;
  hipLaunchKernelGGL(add_budget_kernel, dim3((unsigned)b.nw), dim3(64), 0, b.st, s->d_wins + b.w0, n);
  return hipGetLastError();
}
// the chain of one sub-batch: the iteration budget, then n iterations (eager, or captured into the sub-batch's graph)
hipError_t launch_chain(okvis_ba_solver* s, Sub b, int n, int budget, bool four) {
  hipError_t e = launch_budget(s, b, budget);
  for (int i = 0; i < n && e == hipSuccess; ++i) e = launch_iteration(s, b, four);
  return e;
}
// n iterations of every sub-batch: fork from the main stream, one chain per sub-stream, join
hipError_t launch_iterations_forked(okvis_ba_solver* s, int n, int budget, bool four) {
  const int nsub = (int)s->sub_streams.size();
  if (budget < 0) budget = n;
  if (nsub <= 1) return launch_chain(s, whole(s), n, budget, four);
  hipError_t e = hipEventRecord(s->ev_fork, s->stream);
  for (int k = 0; k < nsub && e == hipSuccess; ++k) {
    e = hipStreamWaitEvent(s->sub_streams[k], s->ev_fork, 0);
    if (e == hipSuccess) e = launch_chain(s, sub(s->sub_streams[k], s->plan.subs[k]), n, budget, four);
    if (e == hipSuccess) e = hipEventRecord(s->sub_events[k], s->sub_streams[k]);
    if (e == hipSuccess) e = hipStreamWaitEvent(s->stream, s->sub_events[k], 0);
  }
  return e;
}

// the accepted-buffer index lives on the device while iterations are in flight: read it back
int refresh_acc(okvis_ba_solver* s, int w) {
  if (s->host.acc_fresh) return OKVIS_BA_OK;   // read by okvis_ba_finish / set at upload, nothing launched since
  int acc = 0;
  HIP_TRY(hipMemcpyAsync(&acc, &s->wins[w].ptrs.ctrl->acc, sizeof(int), hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  s->wins[w].acc = acc & 1;
  return OKVIS_BA_OK;
}

// grow-only staging for begin_kernel's buffer indices and the gathered control records (pinned host + device)
hipError_t reserve_ctrl_stage(okvis_ba_solver* s, size_t n_windows) {
  const size_t bytes = std::max(sizeof(Ctrl), sizeof(int)) * n_windows;   // (begin_kernel's indices or the gathered records, never both)
  if (bytes <= s->ctrl_stage_bytes) return hipSuccess;
  if (s->h_ctrl_stage) (void)hipHostFree(s->h_ctrl_stage);
  if (s->d_ctrl_stage) (void)hipFree(s->d_ctrl_stage);
  s->h_ctrl_stage = s->d_ctrl_stage = nullptr;
  s->ctrl_stage_bytes = 0;
  hipError_t e = hipHostMalloc((void**)&s->h_ctrl_stage, bytes, hipHostMallocDefault);
  if (e == hipSuccess) e = hipMalloc((void**)&s->d_ctrl_stage, bytes);
  if (e == hipSuccess) s->ctrl_stage_bytes = bytes;
  return e;
}

// (redo: Ctrl::pad2 of the copies = the window's re-preintegrations since okvis_ba_begin's evaluation — plans with the three-launch
// iteration, whose okvis_ba_begin left the mark)
int fetch_ctrl(okvis_ba_solver* s, std::vector<Ctrl>& out, bool redo = false) {
  const size_t n = s->wins.size();
  out.resize(n);
  HIP_TRY(reserve_ctrl_stage(s, n));
  hipLaunchKernelGGL(gather_ctrl_kernel, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, s->stream, s->d_wins, reinterpret_cast<Ctrl*>(s->d_ctrl_stage), (int)n,
                     redo && s->redo_mark_windows >= n ? s->d_redo_mark : nullptr);
  HIP_TRY(hipGetLastError());
  HIP_TRY(hipMemcpyAsync(s->h_ctrl_stage, s->d_ctrl_stage, sizeof(Ctrl) * n, hipMemcpyDeviceToHost, s->stream));
  HIP_TRY(hipStreamSynchronize(s->stream));
  std::memcpy(out.data(), s->h_ctrl_stage, sizeof(Ctrl) * n);
  return OKVIS_BA_OK;
}

// The host's part of the three-launch iteration: the windows the solve kernel paused (cs: their control records, just fetched; the
// stream is idle) get what the skipped slots would have given them, on the four-launch route — the factors' launch and linearise for
// the trial that is pending, then the slots they owe of the budget granted so far.  Runs of neighbouring windows that owe the same
// number of slots share their launches; no other window is touched (a window that owes nothing must not meet a slot: the budget
// would end it for good).  *n_paused: how many there were.
int resume_paused(okvis_ba_solver* s, const std::vector<Ctrl>& cs, int* n_paused) {
  const int n = (int)cs.size();
  auto owes = [&](int w) { return cs[w].done == DONE_PAUSED ? std::max(0, cs[w].max_iter - cs[w].iter) : -1; };
  int most = 0;
  *n_paused = 0;
  for (int w0 = 0; w0 < n;) {
    const int need = owes(w0);
    int w1 = w0 + 1;
    if (need < 0) {
      w0 = w1;
      continue;
    }
    while (w1 < n && owes(w1) == need) ++w1;
    const Sub b = sub(s->stream, make_extent(w0, w1 - w0));
    hipLaunchKernelGGL(resume_kernel, dim3((unsigned)((b.nw + 63) / 64)), dim3(64), 0, b.st, s->d_wins + b.w0, b.nw);
    HIP_TRY(hipGetLastError());
    HIP_TRY(launch_lin(s, b, 0));
    HIP_TRY(launch_chain(s, b, need, 0, true));
    most = std::max(most, need);
    *n_paused += b.nw;
    w0 = w1;
  }
  s->host.slots_add(most);
  return OKVIS_BA_OK;
}

}  // namespace
