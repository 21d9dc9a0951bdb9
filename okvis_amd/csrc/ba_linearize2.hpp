// Kernel 1, piece path — back-substitute + (+)update + re-linearise the reprojection factors of windows WITHOUT free
// extrinsics (the stock configuration; windows with online extrinsics calibration keep ba_linearize.hpp).
//
// Same interface, same outputs as linearize_kernel (V, b, un-robustified H_l, W per (landmark, block) pair, per-group
// J^T J / J^T r partials, group scalars, fused group reduction), different reduction scheme.  ba_linearize.hpp stages the
// 2x15 Jacobian of every observation in LDS (47 KB per workgroup) and lets gather loops chase index lists through it: two
// workgroups per CU, waves parked on LDS round trips two thirds of their time.  Here nothing per-observation is staged:
//
//   * With T_SC fixed, the pose Jacobian of an observation is its landmark Jacobian times a 3x6 matrix that depends only
//     on (landmark, pose):  J_pose = J_l M,  M = [ -w I | rows e_i x d ],  d = hp_W - r_WS w
//     (implementation/ReprojectionError.hpp:156-167 against :188-206).  Hence for all observations of one (landmark, pose)
//     pair  sum J_p^T J_l = M^T Vp,  sum J_p^T J_p = M^T Vp M,  sum J_p^T r = M^T bp  with  Vp = sum J_l^T J_l (6 unique
//     entries), bp = sum J_l^T r: the pair blocks follow from NINE sums instead of 45.
//   * Observations are sorted by (landmark, pose, camera): the observations of a pair sit in adjacent lanes.  A PIECE is
//     one or two adjacent lanes of one pair inside one DPP row of 16 (greedy from the start of the run; the host
//     enumerates pieces with the same rule).  The 16 per-observation products (V 6, b 3, H_l 6, cost) are merged across
//     the two lanes of a piece with one DPP row shift and the piece heads store them as 16-value records in LDS
//     (<= LIN2_PIECES records).  Landmark sums, pair sums (a pair split by a row boundary has several pieces) and, after
//     the pair lanes have formed W / U / g in registers and stored the 27-entry block records in block order, the
//     per-block sums over the group's pairs are short contiguous fixed-order LDS sums: deterministic, no atomics.
//   * The window's poses and intrinsics are staged in LDS together with the other operands: phase B has no dependent
//     global load left.  (Several groups per workgroup with the next group's operands requested one group ahead were
//     measured slower, 104-118 against 83 us per 64-window launch: as a loop the body costs some hundred spilled registers,
//     the compiler hoists the constants and addresses of every phase in front of it.)
//
// LDS per workgroup: 27 KB records + 2 KB landmarks + 8 KB landmark results + 4 KB poses / intrinsics + 3 KB index lists
// + the pose part of the step: ~48 KB instead of 78 KB, 115 registers instead of 255 (three workgroups per CU), and no
// 2x12 pose Jacobian in registers.
#pragma once
#include "ba_linearize.hpp"

namespace ba {

constexpr int LIN2_REC = 27;     // entries of a pair's block record: 21 J^T J (upper triangle) + 6 J^T r
constexpr int LIN2_POSES = 64;   // poses of a window staged in LDS (more: phase B reads them from global memory)
constexpr int LIN2_CAMS = 8;     // cameras staged in LDS
constexpr int LIN2_IDX_INTS = 2 * (((GROUP_LM + 1) + 2 * LIN2_PIECES + LIN_TASK_CACHE * 6 + LIN2_PIECES / 2 + LIN2_PIECES / 4 + LIN2_CAMS + 1) / 2);

// UB: entries of the block records that go through LDS per round: all 27 (one round), or 14 (two rounds: the record area then
// is the 16 KB of the piece records, and four workgroups instead of three fit a CU)
template <class REAL, bool FUSE, int UB = LIN2_REC>
struct Lin2Cfg {
  // piece records [pieces][16], then block records [pairs][27]; the fused launch puts the tiles / tables of the group
  // reduction here afterwards (at least the observation stage of ba_linearize.hpp, which the host checked them against)
  static constexpr int PAIR_REC_DOUBLES = (LIN2_PIECES * (UB > 16 ? UB : 16) * (int)sizeof(REAL) + 7) / 8;
  static constexpr int STAGE = LinCfg<false, REAL>::STAGE_DOUBLES;
  static constexpr int REC_DOUBLES = FUSE ? (STAGE > PAIR_REC_DOUBLES ? STAGE : PAIR_REC_DOUBLES) : PAIR_REC_DOUBLES;
  static constexpr int FIXED_DOUBLES = REC_DOUBLES + GROUP_LM * 4 + GROUP_LM * 16 + 4 * 64 + LIN2_POSES * 7 + LIN2_CAMS * 12 + LIN2_IDX_INTS / 2;
  static constexpr int MIN_STEP_DOUBLES = FUSE ? 1024 : 0;   // aux area behind the step (fused: inverse landmark blocks, J^T J blocks, offsets)
};
static_assert(LIN2_PIECES * 3 * 2 <= LIN2_PIECES * 16, "phase A's pair sums alias the record area");
static_assert(LIN2_PIECES <= LIN_THREADS, "one pair per work-item");
// a * b + c in one rounding, in the precision of the arguments (where the contraction must not be left to the compiler)
__device__ __forceinline__ float fma_real(float a, float b, float c) { return fmaf(a, b, c); }
__device__ __forceinline__ double fma_real(double a, double b, double c) { return fma(a, b, c); }
// a * b - c * d with both products rounded before the subtraction (no contraction)
template <class T>
__device__ __forceinline__ T sub_of_rounded_products(T a, T b, T c, T d) {
#pragma clang fp contract(off)
  const T p = a * b, q = c * d;
  return p - q;
}

// value of lane + 1 of the same DPP row (0 for the last lane of a row): row_shl:1
template <class T>
__device__ __forceinline__ T row_next(T v) { return quad_xchg<0x101>(v); }
__device__ __forceinline__ int row_next_i(int v, int old) { return __builtin_amdgcn_update_dpp(old, v, 0x101, 0xF, 0xF, false); }
__device__ __forceinline__ int row_prev_i(int v, int old) { return __builtin_amdgcn_update_dpp(old, v, 0x111, 0xF, 0xF, false); }

// what a workgroup fetches for one group before it can start on it
struct Lin2Ops {     // records and index lists (20 registers)
  ObsRec rec;
  int lpb, pp, poff, plm, pblock, slot;
  Task task;
};
struct Lin2Heavy {   // operands of the back-substitution (54 registers)
  double Wp0[18];                      // pair lane: W row block of the accepted linearisation
  double bb[3], v[6], xx[4], sl[3];    // landmark lane: b, V, x of the accepted buffer, Jacobi scale
  int lp0, lp1;
};

// SMALL: the first n_small workgroups evaluate the IMU / prior factors (as in ba_linearize.hpp: one launch, one window's
// latency); without it the small factors have their own launch (small_kernel) and this kernel's register budget is its
// own.  OCC: workgroups per CU the kernel is compiled for (512 / OCC registers per work-item).
template <class REAL, bool FUSE, bool SMALL, int OCC = 2, int UB = LIN2_REC>
__global__ __launch_bounds__(LIN_THREADS, OCC) void linearize2_kernel(const WinPtrs* __restrict__ wins, const OptD* __restrict__ optp, int init,
                                                                      int n_small, int step_doubles) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  // (diagnostics: stamp 38, kept in registers until the end.  Only in the unfused instantiations without the small factors, the
  //  referee of linearize2_rec_kernel: the fused and SMALL instantiations keep exactly the code they had)
  long long t_entry = 0;
  if constexpr (!FUSE && !SMALL) t_entry = clock64();
  const WinPtrs& W = wins[blockIdx.y];
  int wg = blockIdx.x;
  if constexpr (SMALL) {
    if ((int)blockIdx.x < n_small) {
      small_body(W, init, blockIdx.x, smem);
      return;
    }
    wg -= n_small;
  }
  const int g = wg;
  if (g >= W.n_group) return;
#define LSTAMP(k) do { if (W.prof && threadIdx.x == 0 && g == 0) W.prof[k] = (double)clock64(); } while (0)
  const Ctrl* ctrl = W.ctrl;
  if (ctrl->done) return;
  const OptD opt = *optp;
#include "ba_linearize2_lds.inc"

  // ---- fused mode: see ba_linearize.hpp ----
  auto reduce_own_group = [&](int g, int buf, double lam) {
    const Group Gr = W.groups[g];
    const int trows = min(TILE_DIM, W.Dp);
    double* tables = smem;
    double* aux = s_aux;
    double(*vinv)[6] = reinterpret_cast<double(*)[6]>(aux);
    double(*bvec)[3] = reinterpret_cast<double(*)[3]>(aux + SCHUR_CHUNK_LM_MAX * 6);
    int* boff = reinterpret_cast<int*>(aux + SCHUR_CHUNK_LM_MAX * 9);
    const SchurPairBeginGlobal pb{W.lm_pair_begin, Gr.lm_begin, Gr.lm_end};
    const int n_tp = W.n_tile * (W.n_tile + 1) / 2;
    for (int tp = 0; tp < n_tp; ++tp) {
      schur_reduce_chunk(W, opt, g, tp, Gr.lm_begin, Gr.lm_end, buf, lam, trows, tables, vinv, bvec, boff, pb, g == 0 && blockIdx.y == 0);
      __syncthreads();
    }
  };
  if (!init && !ctrl->pending) {
    if constexpr (FUSE)
      reduce_own_group(g, ctrl->acc, opt.dogleg ? ctrl->mu : 1.0 / ctrl->radius);
    return;
  }
  const int acc = ctrl->acc, trial = 1 - acc;
  const double lambda = ctrl->lambda;
  const double lam_next = opt.dogleg ? ((init || ctrl->first || opt.gauss_newton) ? ctrl->mu : fmax(DL_MIN_MU, 2.0 * ctrl->mu / DL_MU_INCREASE))
                                     : 1.0 / ctrl->radius;
  const bool dl_explicit = opt.dogleg && ctrl->tr_kind == 1;
  const double dl_cA = ctrl->cA, dl_beta = ctrl->beta;
  const bool fast = FUSE && W.fuse_fast;
  const bool poses_staged = W.n_pose <= LIN2_POSES, cams_staged = W.n_cam <= LIN2_CAMS;

  // ---- once per workgroup: the window's trial poses and intrinsics into LDS (visible behind the first barrier) ----
  {
    const double* ps = W.pose[trial];
    const int np7 = 7 * min(W.n_pose, LIN2_POSES);
    for (int i = tid; i < np7; i += LIN_THREADS) s_pose[i] = ps[i];
    const int nc = min(W.n_cam, LIN2_CAMS);
    if (tid < 12 * nc) s_cam[tid] = W.cam_intr[tid];
    if (tid < nc) s_cmodel[tid] = W.cam_model[tid];
  }

  // everything a group needs that only depends on its Group record: requested in one go
  auto issue_loads = [&](const Group& G, Lin2Ops& o) {
    const int nlm = G.lm_end - G.lm_begin, nobs = G.obs_end - G.obs_begin, npair = G.pair_end - G.pair_begin, ntask = G.task_end - G.task_begin;
    o.rec.lm_cam = 0; o.rec.pose = 0; o.rec.ext = 0; o.rec.u = 0; o.rec.v = 0; o.rec.sw = 0;
    if (tid < nobs) o.rec = W.obs[G.obs_begin + tid];
    o.lpb = o.pp = o.poff = o.plm = o.pblock = o.slot = 0;
    if (tid <= nlm) o.lpb = W.lm_piece_begin[G.lm_begin + tid] - G.piece_begin;
    if (tid < npair) {
      o.pp = W.pair_piece[G.pair_begin + tid];
      o.poff = W.pair_off[G.pair_begin + tid];
      o.plm = W.pair_lm[G.pair_begin + tid] - G.lm_begin;
      o.pblock = W.pair_block[G.pair_begin + tid];
      o.slot = W.task_list[G.tlist_begin + tid];
    }
    if (ntask <= LIN_TASK_CACHE && tid < ntask) o.task = W.tasks[G.task_begin + tid];
  };
  // ... and the operands of the back-substitution (54 registers: requested at the top of the group's own turn)
  auto issue_heavy = [&](const Group& G, Lin2Heavy& o) {
    const int nlm = G.lm_end - G.lm_begin, npair = G.pair_end - G.pair_begin;
    o.sl[0] = o.sl[1] = o.sl[2] = 1.0;
    o.lp0 = o.lp1 = 0;
    if (!init) {
      if (tid < npair) {
        const double* Wp = W.W[acc] + (size_t)(G.pair_begin + tid) * 18;
#pragma unroll
        for (int i = 0; i < 18; ++i) o.Wp0[i] = Wp[i];
      }
      if (tid < nlm) {
        const int l = G.lm_begin + tid;
        const double* b = W.bl[acc] + 3 * (size_t)l;
        const double* Vl = W.V[acc] + 6 * (size_t)l;
        const double* x = W.lm[acc] + 4 * (size_t)l;
#pragma unroll
        for (int i = 0; i < 3; ++i) o.bb[i] = b[i];
#pragma unroll
        for (int i = 0; i < 6; ++i) o.v[i] = Vl[i];
#pragma unroll
        for (int i = 0; i < 4; ++i) o.xx[i] = x[i];
        o.lp0 = W.lm_pair_begin[l] - G.pair_begin;
        o.lp1 = W.lm_pair_begin[l + 1] - G.pair_begin;
        if (opt.dogleg) {
          const double* sl = W.lm_scale + 3 * (size_t)l;
          o.sl[0] = sl[0], o.sl[1] = sl[1], o.sl[2] = sl[2];
        }
      }
    } else if (tid < nlm) {
      const double* x = W.lm[trial] + 4 * (size_t)(G.lm_begin + tid);
#pragma unroll
      for (int i = 0; i < 4; ++i) o.xx[i] = x[i];
    }
  };

  const Group G = W.groups[g];
  Lin2Ops ops;
  issue_loads(G, ops);
  if (!init)
    for (int i = tid; i < W.Dp; i += LIN_THREADS) s_step[i] = W.step[i];   // (pairs only refer to pose blocks)

  {
    LSTAMP(40);
    Lin2Heavy hv;
    issue_heavy(G, hv);
#include "ba_linearize2_phases.inc"
    if constexpr (!FUSE && !SMALL) {
      if (W.prof && threadIdx.x == 0 && g == 0) W.prof[38] = (double)t_entry;   // the workgroup's first instruction
    }
  }
#undef LSTAMP
}

// The record instantiations of the unfused launch without the small factors (FUSE and SMALL are parameters only because the shared
// text names them; they are never set).  linearize2_kernel above reads W.n_group, W.ctrl, the control words, W.groups[g] and each
// pointer of the window record one after the other, where it first needs them: some twenty dependent fetches before phase A, most
// of them in front of the next request.  Here the workgroup starts from the batch's group launch records (LIN_REC_INTS,
// ba_types.hpp; build_group_records) and the control record array, whose addresses follow from kernel arguments and blockIdx:
//   trip 1  the group record, the control words, the options and one word of every scalar-cache line of the window record are
//           requested together at kernel entry (a branch that is never taken reads them all, which keeps the requests in front of
//           the first exit; the window record's fields then come from the scalar cache where they are used, as in solve_kernel);
//   trip 2  every operand — trial poses, intrinsics, camera models, observation record, piece / pair / task lists, the step and
//           the operands of the back-substitution — is requested in straight-line code before the first of them is waited for:
//           an index without an element is clamped to element 0 of the same array, the values of such lanes are set behind the
//           requests as issue_loads / issue_heavy of linearize2_kernel leave them, and what is staged in LDS is stored there.
// The phases are the text of linearize2_kernel (ba_linearize2_phases.inc): the same products in the same places, and
// linearize2_kernel stays as the referee (OKVIS_BA_TUNE_LIN_NO_RECORDS).  ctrls / grecs point to the control record and to the
// group launch records of the launch's first window, grec_stride records per window.  No inline assembly in here: see solve_kernel.
template <class REAL, int OCC = 2, int UB = LIN2_REC, bool FUSE = false, bool SMALL = false>
__global__ __launch_bounds__(LIN_THREADS, OCC) void linearize2_rec_kernel(const WinPtrs* __restrict__ wins, const OptD* __restrict__ optp, int init,
                                                                          int step_doubles, const CtrlSlot* __restrict__ ctrls,
                                                                          const int* __restrict__ grecs, int grec_stride) {
  static_assert(!FUSE && !SMALL, "the unfused launch without the small factors");
  extern __shared__ __attribute__((aligned(16))) double smem[];
  const long long t_entry = clock64();   // (diagnostics: stamp 38)
  const WinPtrs& W = wins[blockIdx.y];
  const int g = blockIdx.x;
  // ---- trip 1 ----
  const int* rec = grecs + ((size_t)blockIdx.y * grec_stride + g) * LIN_REC_INTS;
  int r[LIN_REC_COUNTS];
#pragma unroll
  for (int i = 0; i < LIN_REC_COUNTS; ++i) r[i] = rec[i];
  const int rec_nlm = rec[LIN_REC_COUNTS], rec_nobs = rec[LIN_REC_COUNTS + 1], rec_npair = rec[LIN_REC_COUNTS + 2], rec_ntask = rec[LIN_REC_COUNTS + 3];
  const int rec_valid = rec[LIN_REC_VALID];
  const Ctrl* ctrl = &ctrls[blockIdx.y].c;   // (== W.ctrl)
  const int c_done = ctrl->done, c_pending = ctrl->pending, c_acc = ctrl->acc, c_first = ctrl->first, c_tr_kind = ctrl->tr_kind;
  const double c_lambda = ctrl->lambda, c_mu = ctrl->mu, c_radius = ctrl->radius, c_cA = ctrl->cA, c_beta = ctrl->beta;
  const OptD opt = *optp;
  {
    // (never taken: `init` is 0 or 1.  The condition reads every word requested above and one word of every line of the window
    //  record, so none of the requests can move behind an exit.  This rests on what the compiler does with it, and only its
    //  output shows that it still holds.  To re-check after a toolchain change:
    //    hipcc --offload-arch=gfx950 -O3 -std=c++17 --cuda-device-only -S okvis_amd/csrc/ba_capi.hip
    //  and, in linearize2_rec_kernel<double, 4, 14>, count from the entry to the first s_barrier: every s_load of the record, the
    //  control words, the options and the 18 lines of the window record must stand in front of the first s_cbranch; no s_waitcnt
    //  vmcnt may stand between the first and the last operand global_load; profiles/lin_records_notes.md section 2 has the counts
    //  this was written with — 18 s_waitcnt in all, one for the kernel arguments and three lgkmcnt(0) in front of the exits.)
    constexpr int lines = (int)((sizeof(WinPtrs) + 63) / 64);   // (never a line beyond the record)
    static_assert(sizeof(WinPtrs) % 4 == 0 && (lines - 1) * 64 < (int)sizeof(WinPtrs), "lines touched below");
    const int* wi = reinterpret_cast<const int*>(&W);
    auto dw = [](double d) { return __double2loint(d) ^ __double2hiint(d); };
    int keep = rec_valid ^ rec_nlm ^ rec_nobs ^ rec_npair ^ rec_ntask;
#pragma unroll
    for (int k = 0; k < lines; ++k) keep ^= wi[16 * k];
#pragma unroll
    for (int i = 0; i < LIN_REC_COUNTS; ++i) keep ^= r[i];
    keep ^= c_done ^ c_pending ^ c_acc ^ c_first ^ c_tr_kind ^ dw(c_lambda) ^ dw(c_mu) ^ dw(c_radius) ^ dw(c_cA) ^ dw(c_beta);
    keep ^= opt.dogleg ^ opt.gauss_newton ^ opt.jacobi_scaling ^ dw(opt.min_lm_diag2) ^ dw(opt.max_lm_diag2);
    if (init == 0x7ffffff1 && keep == 0x5a5a5a5a) return;
  }
  if (!rec_valid) return;   // a slot behind the window's last group
#define LSTAMP(k) do { if (W.prof && threadIdx.x == 0 && g == 0) W.prof[k] = (double)clock64(); } while (0)
  if (c_done) return;
#include "ba_linearize2_lds.inc"
  [[maybe_unused]] auto reduce_own_group = [](int, int, double) {};
  if (!init && !c_pending) return;   // (also the launch behind a rejected trial under DOGLEG)
  const int acc = c_acc, trial = 1 - acc;
  const double lambda = c_lambda;
  [[maybe_unused]] const double lam_next = opt.dogleg ? ((init || c_first || opt.gauss_newton) ? c_mu : fmax(DL_MIN_MU, 2.0 * c_mu / DL_MU_INCREASE))
                                                      : 1.0 / c_radius;
  const bool dl_explicit = opt.dogleg && c_tr_kind == 1;
  const double dl_cA = c_cA, dl_beta = c_beta;
  const bool fast = false;
  const bool poses_staged = W.n_pose <= LIN2_POSES, cams_staged = W.n_cam <= LIN2_CAMS;
  const Group G{r[0], r[1], r[2], r[3], r[4], r[5], r[6], r[7], r[8], r[9], r[10], r[11], r[12], r[13], r[14], r[15]};
  Lin2Ops ops;
  {
    Lin2Heavy hv;
    // ---- trip 2: no branch and no store between the requests (a stamp stored in here would put a wait in front of whatever
    //      reuses its registers; on `init` the accepted linearisation is requested along and discarded) ----
    static_assert(7 * LIN2_POSES <= 2 * LIN_THREADS && 12 * LIN2_CAMS <= LIN_THREADS, "two pose entries and one intrinsics entry per lane");
    const int np7 = 7 * min(W.n_pose, LIN2_POSES), nc = min(W.n_cam, LIN2_CAMS), Dp = W.Dp;
    const bool in_lm = tid < rec_nlm, in_pair = tid < rec_npair, in_task = rec_ntask <= LIN_TASK_CACHE && tid < rec_ntask;
    const BA_G double* ps = W.pose[trial];
    const double st_pose0 = ps[tid < np7 ? tid : 0], st_pose1 = ps[tid + LIN_THREADS < np7 ? tid + LIN_THREADS : 0];
    const double st_cam = W.cam_intr[tid < 12 * nc ? tid : 0];
    const int st_cmodel = W.cam_model[tid < nc ? tid : 0];
    ops.rec = W.obs[tid < rec_nobs ? G.obs_begin + tid : 0];
    ops.lpb = W.lm_piece_begin[tid <= rec_nlm ? G.lm_begin + tid : 0];
    const int pi = in_pair ? G.pair_begin + tid : 0, l = in_lm ? G.lm_begin + tid : 0;
    ops.pp = W.pair_piece[pi];
    ops.poff = W.pair_off[pi];
    ops.plm = W.pair_lm[pi];
    ops.pblock = W.pair_block[pi];
    ops.slot = W.task_list[in_pair ? G.tlist_begin + tid : 0];
    ops.task = W.tasks[in_task ? G.task_begin + tid : 0];
    const double st_step = W.step[tid < Dp ? tid : 0];
    {
      const BA_G double* Wp = W.W[acc] + (size_t)pi * 18;
      const BA_G double* b = W.bl[acc] + 3 * (size_t)l;
      const BA_G double* Vl = W.V[acc] + 6 * (size_t)l;
      const BA_G double* x = W.lm[init ? trial : acc] + 4 * (size_t)l;
      const BA_G double* sl = W.lm_scale + 3 * (size_t)l;
#pragma unroll
      for (int i = 0; i < 18; ++i) hv.Wp0[i] = Wp[i];
#pragma unroll
      for (int i = 0; i < 3; ++i) hv.bb[i] = b[i];
#pragma unroll
      for (int i = 0; i < 6; ++i) hv.v[i] = Vl[i];
#pragma unroll
      for (int i = 0; i < 4; ++i) hv.xx[i] = x[i];
      hv.lp0 = W.lm_pair_begin[l];
      hv.lp1 = W.lm_pair_begin[l + 1];   // (the list has one entry more than the window has landmarks)
#pragma unroll
      for (int i = 0; i < 3; ++i) hv.sl[i] = sl[i];
    }
    const long long t_req = clock64();   // (diagnostics: stamp 40, every request is out)
    // ---- lanes without an element: as issue_loads / issue_heavy leave them ----
    if (!(tid < rec_nobs)) { ops.rec.lm_cam = 0; ops.rec.pose = 0; ops.rec.ext = 0; ops.rec.u = 0; ops.rec.v = 0; ops.rec.sw = 0; }
    ops.lpb = tid <= rec_nlm ? ops.lpb - G.piece_begin : 0;
    ops.plm = in_pair ? ops.plm - G.lm_begin : 0;
    if (!in_pair) ops.pp = ops.poff = ops.pblock = ops.slot = 0;
    hv.lp0 = in_lm && !init ? hv.lp0 - G.pair_begin : 0;
    hv.lp1 = in_lm && !init ? hv.lp1 - G.pair_begin : 0;
    if (!(in_lm && !init && opt.dogleg)) hv.sl[0] = hv.sl[1] = hv.sl[2] = 1.0;
    // ---- what is staged in LDS (visible behind the first barrier) ----
    if (tid < np7) s_pose[tid] = st_pose0;
    if (tid + LIN_THREADS < np7) s_pose[tid + LIN_THREADS] = st_pose1;
    if (tid < 12 * nc) s_cam[tid] = st_cam;
    if (tid < nc) s_cmodel[tid] = st_cmodel;
    if (!init) {
      if (tid < Dp) s_step[tid] = st_step;
      for (int i = tid + LIN_THREADS; i < Dp; i += LIN_THREADS) s_step[i] = W.step[i];   // (pose parts beyond 256 rows)
    }
#include "ba_linearize2_phases.inc"
    if (W.prof && tid == 0 && g == 0) W.prof[38] = (double)t_entry, W.prof[40] = (double)t_req;   // (kept in registers until here)
  }
#undef LSTAMP
}

// the IMU / prior factors of every window in a launch of their own (the companion of linearize2_kernel<.., SMALL = false>)
__global__ __launch_bounds__(LIN_THREADS, 2) void small_kernel(const WinPtrs* __restrict__ wins, int init) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  small_body(wins[blockIdx.y], init, blockIdx.x, smem);
}
// ... and its first half alone (imu_factor<1>: what may change an IMU term's preintegration record), where the evaluation rides in
// the decision-free Schur launch of the same slot (schur_ride_kernel, ba_schur2.hpp); grid: the IMU terms only
__global__ __launch_bounds__(LIN_THREADS, 2) void small_prepare_kernel(const WinPtrs* __restrict__ wins) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  small_body<1>(wins[blockIdx.y], 0, blockIdx.x, smem);
}

// First preintegration of IMU terms that arrive without one (okvis_ba_window::imu_sb_ref_valid = 0), started by okvis_ba_upload /
// okvis_ba_patch_window BEFORE the host builds the window's index lists, so that the 0.1 ms recursion runs while the host works
// instead of stretching the first linearise launch of the next optimisation.  Workgroup k integrates the one term of the
// stand-in window record mini[k] (its IMU arrays, noise parameters and cache pointer; everything else unset) at the bias sb0s[9 k ..]
// — imu_redo itself, so the record is the one the first evaluation would have built at that bias; imu_pre_place_kernel then
// copies it over the term's (empty) record in the uploaded window, behind the arena copy on the same stream.
__global__ __launch_bounds__(IMU_THREADS, 2) void imu_pre_kernel(const WinPtrs* __restrict__ mini, const double* __restrict__ sb0s) {
  extern __shared__ __attribute__((aligned(16))) double smem[];
  imu_redo(mini[blockIdx.x], 0, sb0s + 9 * (size_t)blockIdx.x, smem, threadIdx.x);
}
__global__ void imu_pre_place_kernel(const WinPtrs* __restrict__ wins, const int2* __restrict__ where, const ImuCacheD* __restrict__ src) {
  const int2 wf = where[blockIdx.x];
  const double* s = reinterpret_cast<const double*>(src + blockIdx.x);
  auto d = reinterpret_cast<BA_G double*>(wins[wf.x].imu_cache + wf.y);
  for (int i = threadIdx.x; i < (int)(sizeof(ImuCacheD) / 8) - 1; i += blockDim.x) d[i] = s[i];
  if (threadIdx.x == 0) {   // (the last double holds the two counters: one preintegration so far, valid at the bias it was built at —
                            // 3: imu_maybe_redo takes it for the first evaluation's only if that evaluation sees the same bias)
    wins[wf.x].imu_cache[wf.y].valid = 3;
    wins[wf.x].imu_cache[wf.y].redo_count = 1;
  }
}

}  // namespace ba
