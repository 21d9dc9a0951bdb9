// Part of ba_capi.hip, inside its extern "C" block.  okvis_ba_marginalize / _begin / _end (DESIGN.md section 5, "Marginalisation").
// MarginalizationError numerics (see include/okvis_amd_ba.h): linearise at the uploaded values, eliminate
// the landmarks (schur_kernel in marg_mode), export the dense system (solve_kernel final_only = 2), then the
// dense elimination + eigen-decomposition (marg_dense_kernel).
// There is ONE implementation, for a range of windows (marg_begin / marg_end): one linearisation, one Schur launch, one export
// launch, one launch of the dense tail with a workgroup per window for every run of windows on the LDS route, one copy each way.
// okvis_ba_marginalize_batch / _batch_begin / _batch_end are that call; okvis_ba_marginalize / _begin / _end are the range of one.
namespace {

// ---- What the three range entries share: okvis_ba_marginalize[_batch] (below), okvis_ba_state_covariance (capi_covariance.inc) and
//      okvis_ba_landmark_covariance (capi_landmark_covariance.inc).  Each lays its scratch block out with an Arena (capi_solver.inc),
//      what the host writes first so that it goes up in one copy, and keeps the block in s->marg_scratch. ----
int marg_reserve_scratch(okvis_ba_solver* s, size_t bytes) {
  if (bytes > s->marg_scratch_bytes) {
    if (s->marg_scratch) HIP_TRY(hipFree(s->marg_scratch));
    s->marg_scratch = nullptr;
    s->marg_scratch_bytes = 0;
    HIP_TRY(hipMalloc(&s->marg_scratch, bytes));
    s->marg_scratch_bytes = bytes;
  }
  return OKVIS_BA_OK;
}
// The pass has its own option record in the scratch block (no trust region: one linearisation, no damping); the launches read it
// through s->d_opt, which points there for the duration of the call.  The solver's own record is never touched, so nothing has to
// be restored on the device and captured launch graphs stay valid.
OptD marg_optd(const okvis_ba_solver* s) {
  OptD od = make_optd(s->opt, (int)s->wins.size());
  od.marg_mode = 1;
  od.dogleg = 0;
  return od;
}
struct MargSwapOptions {
  okvis_ba_solver* s;
  OptD* saved;
  ~MargSwapOptions() { s->d_opt = saved; }
};
// where a window's reduced system [D][D], its right-hand side [D] and its damping [D] are exported to (offsets in the scratch block d)
struct ExportAt { size_t o_S = 0, o_rhs = 0, o_d2 = 0; };
// the window's record with the export buffers attached
WinPtrs win_with_export(const HostWin& H, unsigned char* d, const ExportAt& ex) {
  WinPtrs P = H.ptrs;
  P.S = (decltype(P.S))(d + ex.o_S);
  P.rhs = (decltype(P.rhs))(d + ex.o_rhs);
  P.Dp2 = (decltype(P.Dp2))(d + ex.o_d2);
  P.grad = nullptr;
  return P;
}
// Landmark elimination + export (solve_kernel, final_only = 2) of windows w0 .. w0 + n - 1 behind okvis_ba_begin, one launch each;
// d_wins: their records with the export buffers attached.  Helper workgroups as the plan's own extents have them: up to
// SOLVE_HELPED_MAX_WINDOWS windows they sum the Schur chunk partials, longer ranges sum inside the solving workgroup.  Both add a
// chunk's partials in chunk order starting from zero (ba_solve.hpp), so a window's exported system has the same bits either way,
// and a range of one has okvis_ba_marginalize's launch shape.  lds_windows = false: every window of the range is assembled in HBM
// (such windows leave the solve launch at once; marg_export_large exports them one by one).
hipError_t schur_and_export(okvis_ba_solver* s, int w0, int n, const WinPtrs* d_wins, bool lds_windows = true) {
  const int helpers = n <= SOLVE_HELPED_MAX_WINDOWS ? s->plan.one_helpers : 0;
  const hipError_t e = launch_schur(s, sub(s->stream, Extent{w0, n, helpers}), 0, false);
  if (e != hipSuccess) return e;
  if (lds_windows && s->plan.solve.k) launch_solve_kernel(s, s->plan.solve, dim3((unsigned)n, 1 + helpers), s->stream, d_wins, 2, s->d_ctrl + w0);
  return hipGetLastError();
}

// One window of a marginalisation call: what the argument check found (the kept blocks, in reduced order: pose-type blocks first),
// the route its dense tail takes and where its pieces lie in the call's scratch block.
struct MargJob {
  int w = 0;
  const okvis_ba_marg_spec* spec = nullptr;
  std::vector<int> bt, bi, bo;
  int na = 0, nm = 0, D = 0, pd = 0, pnb = 0;   // kept / eliminated rows, reduced dimension, previous prior
  bool large = false;      // reduced system assembled in HBM (D > MAX_D_LDS)
  bool tiles = false;      // kept blocks beyond the single-workgroup LDS paths: the tail on many workgroups (ba_marg_tiles.hpp)
  bool lds_route = false;  // the single workgroup whose matrices stay in LDS
  size_t nn = 1, n1 = 1, out_bytes = 0;
  size_t o_pm = 0, o_sm = 0, o_pt = 0, o_pi = 0, o_po = 0, o_pH = 0, o_pb = 0;   // written by the host
  size_t o_again = 0;      // ... and, on the tiled route, the argument record of its fall-back
  size_t o_work = 0;       // workspace
  ExportAt ex;             // exported system
  size_t o_out = 0, o_info = 0;                                                  // H | J | b0 | e0 | info
  int mt_nT = 0, mt_ntiles = 0;
  size_t o_mtT = 0, o_mtZ = 0, o_mtL = 0, o_mtR = 0, o_mtY = 0, o_mtP = 0, o_mtF = 0, o_mtp = 0, o_mtS = 0, o_mtf = 0;
  size_t out_span() const { return out_bytes + sizeof(int) * (8 + std::max(1, D)); }
};

// The argument check of okvis_ba_marginalize for window w; on success J holds the kept blocks and the route.
int marg_check(okvis_ba_solver* s, int w, const okvis_ba_marg_spec* spec, const okvis_ba_marg_result* res, MargJob& J) {
  if (!spec || !res) return OKVIS_BA_ERR_ARG;
  if (w < 0 || w >= (int)s->wins.size()) return OKVIS_BA_ERR_ARG;
  const HostWin& H = s->wins[w];
  if (H.marg_dim != 0) return OKVIS_BA_ERR_ARG;                    // the previous prior comes in through spec
  if ((H.n_pose > 0 && !spec->pose_marg) || (H.n_sb > 0 && !spec->sb_marg)) return OKVIS_BA_ERR_ARG;
  const int pd = spec->prior_dim, pnb = spec->prior_nblocks;
  if (pd < 0 || pnb < 0 || pd > MAX_MARG_DIM) return pd > MAX_MARG_DIM ? OKVIS_BA_ERR_UNSUPPORTED : OKVIS_BA_ERR_ARG;
  if (pd > 0 && (!spec->prior_block_type || !spec->prior_block_idx || !spec->prior_block_off || !spec->prior_H ||
                 !spec->prior_b0 || pnb == 0))
    return OKVIS_BA_ERR_ARG;
  for (int k = 0, expect = 0; k < (pd > 0 ? pnb : 0); ++k) {
    const int t = spec->prior_block_type[k], idx = spec->prior_block_idx[k];
    if (spec->prior_block_off[k] != expect) return OKVIS_BA_ERR_ARG;
    if (t == OKVIS_BA_BLOCK_POSE) {
      if (idx < 0 || idx >= H.n_pose) return OKVIS_BA_ERR_ARG;
      expect += 6;
    } else if (t == OKVIS_BA_BLOCK_SPEEDBIAS) {
      if (idx < 0 || idx >= H.n_sb) return OKVIS_BA_ERR_ARG;
      expect += 9;
    } else {
      return OKVIS_BA_ERR_ARG;
    }
    if (k == pnb - 1 && expect != pd) return OKVIS_BA_ERR_ARG;
  }
  // kept blocks, in reduced order (pose-type blocks first); rows of the eliminated block
  J = MargJob{};
  int na = 0, nm = 0;
  for (int i = 0; i < H.n_pose; ++i)
    if (H.pose_off[i] >= 0 && !spec->pose_marg[i]) {
      J.bt.push_back(OKVIS_BA_BLOCK_POSE); J.bi.push_back(i); J.bo.push_back(na);
      na += 6;
    } else if (H.pose_off[i] >= 0) {
      nm += 6;
    }
  for (int i = 0; i < H.n_sb; ++i)
    if (H.sb_off[i] >= 0 && !spec->sb_marg[i]) {
      J.bt.push_back(OKVIS_BA_BLOCK_SPEEDBIAS); J.bi.push_back(i); J.bo.push_back(na);
      na += 9;
    } else if (H.sb_off[i] >= 0) {
      nm += 9;
    }
  if (na > res->capacity_dim || (int)J.bt.size() > res->capacity_blocks) return OKVIS_BA_ERR_ARG;
  if (na > 0 && (!res->H || !res->b0 || !res->J || !res->e0 || !res->block_type || !res->block_idx || !res->block_off))
    return OKVIS_BA_ERR_ARG;
  J.w = w, J.spec = spec, J.na = na, J.nm = nm, J.D = H.D, J.pd = pd, J.pnb = pnb;
  J.large = H.ptrs.Sg != nullptr;
  const bool no_tiles = (s->opt.tuning.flags & OKVIS_BA_TUNE_NO_MARG_TILES) != 0;   // (A/B switch)
  J.tiles = na > MARG_PC_NMAX && !no_tiles;
  J.lds_route = !J.large && pd <= MARG_SMALL_PRIOR && na <= MARG_PC_NMAX;
  J.nn = std::max<size_t>(1, (size_t)na * na), J.n1 = std::max(1, na);
  J.out_bytes = 8 * (2 * J.nn + 2 * J.n1);
  return OKVIS_BA_OK;
}

// ---- the pieces of a window in the scratch block, in the order a call lays them out ----
void marg_place_host(Arena& A, const HostWin& H, MargJob& J) {
  J.o_pm = A.alloc(std::max(1, H.n_pose)), J.o_sm = A.alloc(std::max(1, H.n_sb));
  J.o_pt = A.alloc(sizeof(int) * std::max(1, J.pnb)), J.o_pi = A.alloc(sizeof(int) * std::max(1, J.pnb)),
  J.o_po = A.alloc(sizeof(int) * std::max(1, J.pnb));
  J.o_pH = A.alloc(8 * std::max<size_t>(1, (size_t)J.pd * J.pd)), J.o_pb = A.alloc(8 * std::max(1, J.pd));
  if (J.tiles) J.o_again = A.alloc(sizeof(MargArgs));
}
void marg_place_work(Arena& A, MargJob& J) {
  const int D = J.D;
  J.o_work = A.alloc(8 * marg_work_doubles(std::max(1, D)));
  J.ex.o_S = A.alloc(8 * std::max<size_t>(1, (size_t)D * D)), J.ex.o_rhs = A.alloc(8 * std::max(1, D)), J.ex.o_d2 = A.alloc(8 * std::max(1, D));
}
void marg_place_out(Arena& A, MargJob& J) {   // H | J | b0 | e0 | info: contiguous, ONE copy back
  J.o_out = A.alloc(J.out_span());
  J.o_info = J.o_out + J.out_bytes;
}
void marg_place_tiles(Arena& A, MargJob& J) {
  const int D = J.D;
  J.mt_nT = J.tiles ? (J.na + CT_TB - 1) / CT_TB : 0, J.mt_ntiles = J.mt_nT * (J.mt_nT + 1) / 2;
  const int mt_nT = J.mt_nT, mt_ntiles = J.mt_ntiles;
  J.o_mtT = A.alloc(8 * (size_t)std::max(1, mt_ntiles) * CT_TILE), J.o_mtZ = A.alloc(8 * (size_t)std::max(1, mt_ntiles) * CT_TILE),
  J.o_mtL = A.alloc(8 * (size_t)std::max(1, mt_nT) * CT_TILE), J.o_mtR = A.alloc(8 * (size_t)std::max(1, CT_TB * mt_nT)),
  J.o_mtY = A.alloc(8 * (size_t)std::max(1, CT_TB * mt_nT)), J.o_mtP = A.alloc(8 * (size_t)std::max(1, CT_TB * mt_nT)),
  J.o_mtF = A.alloc(8 * (size_t)std::max(1, mt_ntiles)), J.o_mtp = A.alloc(8 * (size_t)std::max(1, D)),
  J.o_mtS = A.alloc(8 * (size_t)std::max(1, CT_TB * mt_nT)),
  J.o_mtf = A.alloc(sizeof(int) * (size_t)(mt_ntiles + 1 + 2 * mt_nT + 1 + mt_ntiles));
}
// the host-written pieces of a window (flags, the previous prior) into the staging block
void marg_fill_host(unsigned char* hb, const HostWin& H, const MargJob& J) {
  const okvis_ba_marg_spec* spec = J.spec;
  if (H.n_pose) std::memcpy(&hb[J.o_pm], spec->pose_marg, H.n_pose);
  if (H.n_sb) std::memcpy(&hb[J.o_sm], spec->sb_marg, H.n_sb);
  if (J.pd > 0) {
    std::memcpy(&hb[J.o_pt], spec->prior_block_type, sizeof(int) * J.pnb);
    std::memcpy(&hb[J.o_pi], spec->prior_block_idx, sizeof(int) * J.pnb);
    std::memcpy(&hb[J.o_po], spec->prior_block_off, sizeof(int) * J.pnb);
    std::memcpy(&hb[J.o_pH], spec->prior_H, 8 * (size_t)J.pd * J.pd);
    std::memcpy(&hb[J.o_pb], spec->prior_b0, 8 * (size_t)J.pd);
  }
}
void marg_args(unsigned char* d, const MargJob& J, MargArgs& ma) {
#define MARG_AT(field, off) ma.field = (decltype(ma.field))(d + (off))   // (the record's pointers are global-address-space ones)
  MARG_AT(pose_marg, J.o_pm);
  MARG_AT(sb_marg, J.o_sm);
  ma.prior_dim = J.pd;
  ma.prior_nb = J.pd > 0 ? J.pnb : 0;
  MARG_AT(pb_type, J.o_pt);
  MARG_AT(pb_idx, J.o_pi);
  MARG_AT(pb_off, J.o_po);
  MARG_AT(prior_H, J.o_pH);
  MARG_AT(prior_b0, J.o_pb);
  MARG_AT(work, J.o_work);
  MARG_AT(out_H, J.o_out);
  MARG_AT(out_J, J.o_out + 8 * J.nn);
  MARG_AT(out_b0, J.o_out + 8 * 2 * J.nn);
  MARG_AT(out_e0, J.o_out + 8 * (2 * J.nn + J.n1));
  MARG_AT(out_info, J.o_info);
  MARG_AT(p_out, J.o_mtp);
#undef MARG_AT
}
// the export of one window whose reduced system is assembled in HBM: assembly of the undamped system, then the kernel that completes
// it (Schur partials, IMU terms) and, because this copy of the window carries an S pointer, writes it out as one full symmetric
// D x D matrix
void marg_export_large(okvis_ba_solver* s, const MargJob& J, const WinPtrs* d_win) {
  launch_solve_kernel(s, s->plan.tiled, dim3(1), s->stream, d_win, 2, s->d_ctrl + J.w);
  const int nT = (((J.D + 5) / 6) * 6 + CT_TB - 1) / CT_TB;
  hipLaunchKernelGGL(large_export_kernel, dim3(nT * (nT + 1) / 2, 1, CT_TILE / CT_THREADS), dim3(CT_THREADS), 0, s->stream, d_win);
}
// marg_dense_kernel for n consecutive windows of J's size class: workgroup i takes d_win[i] with d_args[i] (both on the device)
void marg_dense_launch(okvis_ba_solver* s, const MargJob& J, const WinPtrs* d_win, const MargArgs* d_args, int stage, int n = 1) {
  if (J.large || J.pd > MARG_SMALL_PRIOR)
    hipLaunchKernelGGL((marg_dense_kernel<MAX_D, MAX_MARG_DIM>), dim3((unsigned)n), dim3(MARG_THREADS), MARG_LDS_DOUBLES_LARGE * 8, s->stream, d_win,
                       d_args, MARG_LDS_DOUBLES_LARGE, stage);
  else
    hipLaunchKernelGGL((marg_dense_kernel<MAX_D_LDS, MARG_SMALL_PRIOR>), dim3((unsigned)n), dim3(MARG_THREADS), MARG_LDS_DOUBLES * 8, s->stream, d_win,
                       d_args, MARG_LDS_DOUBLES, stage);
}
// The dense tail of one window off the LDS route, on the single workgroup or on the tiled route (mt: where that route leaves its
// verdict).  ma: the window's argument record, d_ma: where it lies on the device.
void marg_tail(okvis_ba_solver* s, const MargJob& J, unsigned char* d, const WinPtrs* d_win, const MargArgs& ma, const MargArgs* d_ma, MargTiles& mt) {
  if (!J.tiles) {
    marg_dense_launch(s, J, d_win, d_ma, 0);
    return;
  }
  // the single workgroup stops after M and b0; Schur complement, scaling, tiled factorisation (matrix core), L^-1 for the proof
  // of full rank, J and e0 on many workgroups
  const int mt_nT = J.mt_nT, mt_ntiles = J.mt_ntiles, na = J.na, nm = J.nm, pd = J.pd;
  mt.C.nT = mt_nT;
  mt.C.T = reinterpret_cast<double*>(d + J.o_mtT);
  mt.C.Linv = reinterpret_cast<double*>(d + J.o_mtL);
  mt.C.rhs = reinterpret_cast<double*>(d + J.o_mtR);
  mt.C.y = reinterpret_cast<double*>(d + J.o_mtY);
  mt.C.flag = reinterpret_cast<int*>(d + J.o_mtf);
  mt.C.pflag = mt.C.flag + mt_ntiles + 1;
  mt.Z = reinterpret_cast<double*>(d + J.o_mtZ);
  mt.fro = reinterpret_cast<double*>(d + J.o_mtF);
  mt.p2 = reinterpret_cast<double*>(d + J.o_mtP);
  mt.rowsum = reinterpret_cast<double*>(d + J.o_mtS);
  mt.ok = mt.C.flag + mt_ntiles + 1 + 2 * mt_nT;
  mt.zflag = mt.ok + 1;
  static const bool attrs = [] {
    (void)hipFuncSetAttribute(reinterpret_cast<const void*>(chol_tile_kernel), hipFuncAttributeMaxDynamicSharedMemorySize, CT_SMEM_DOUBLES * 8);
    return true;
  }();
  (void)attrs;
  if (pd > 0)
    hipLaunchKernelGGL(marg_prior_add_kernel, dim3((unsigned)(((size_t)pd * pd + MARG_TILES_THREADS - 1) / MARG_TILES_THREADS)),
                       dim3(MARG_TILES_THREADS), 0, s->stream, d_win, ma);
  if (nm > 0) {
    marg_dense_launch(s, J, d_win, d_ma, 1 | 2 | 4);
    hipLaunchKernelGGL(marg_M_kernel, dim3((unsigned)(((size_t)na * nm + MARG_TILES_THREADS - 1) / MARG_TILES_THREADS)), dim3(MARG_TILES_THREADS), 0,
                       s->stream, d_win, ma);
    hipLaunchKernelGGL(marg_b0_kernel, dim3((unsigned)((na + MARG_TILES_THREADS - 1) / MARG_TILES_THREADS)), dim3(MARG_TILES_THREADS), 0, s->stream,
                       d_win, ma);
  } else {
    marg_dense_launch(s, J, d_win, d_ma, 1 | 2);   // (nothing to eliminate densely: b0 is a gather)
  }
  const unsigned nb2 = (unsigned)(((size_t)na * na + MARG_TILES_THREADS - 1) / MARG_TILES_THREADS);
  hipLaunchKernelGGL(marg_schur_kernel, dim3(nb2), dim3(MARG_TILES_THREADS), 0, s->stream, d_win, ma);
  hipLaunchKernelGGL(marg_tiles_scale_kernel, dim3((CT_TB * mt_nT + MARG_TILES_THREADS - 1) / MARG_TILES_THREADS), dim3(MARG_TILES_THREADS), 0,
                     s->stream, ma, mt);
  hipLaunchKernelGGL(marg_tiles_fill_kernel, dim3(mt_ntiles), dim3(MARG_TILES_THREADS), 0, s->stream, ma, mt);
  hipLaunchKernelGGL(chol_tile_kernel, dim3(mt_ntiles), dim3(CT_THREADS), CT_SMEM_DOUBLES * 8, s->stream, mt.C);
  hipLaunchKernelGGL(marg_tiles_inverse_kernel, dim3(mt_ntiles), dim3(CT_THREADS), 2 * CT_TB * CT_LD * 8, s->stream, ma, mt);
  hipLaunchKernelGGL(marg_tiles_out_kernel, dim3(mt_ntiles), dim3(MARG_TILES_THREADS), 0, s->stream, ma, mt);
  hipLaunchKernelGGL(marg_tiles_rowsum_kernel, dim3((na + MARG_TILES_THREADS / 64 - 1) / (MARG_TILES_THREADS / 64)), dim3(MARG_TILES_THREADS), 0,
                     s->stream, ma, mt);
  hipLaunchKernelGGL(marg_tiles_decide_kernel, dim3(1), dim3(MARG_THREADS), 0, s->stream, ma, mt);
}
// No proof of full rank on the tiled route (a rank-deficient kept block, a pivot that is not positive): the single workgroup takes
// over — the previous prior is part of H already, everything else is done again — and goes on to the eigen-decomposition.
// d_again: the window's argument record without the previous prior (prior_dim = prior_nb = 0), which went up with the call's copy.
void marg_tiles_fallback(okvis_ba_solver* s, const MargJob& J, const WinPtrs* d_win, const MargArgs* d_again) {
  marg_dense_launch(s, J, d_win, d_again, 0);
  s->marg_tiles_fallbacks++;
}
// what is known without the numbers: the blocks the new prior connects
void marg_report_blocks(const okvis_ba_solver::MargPending::Item& it, okvis_ba_marg_result* res) {
  res->dim = it.na;
  res->nblocks = (int)it.bt.size();
  for (size_t k = 0; k < it.bt.size(); ++k) {
    res->block_type[k] = it.bt[k];
    res->block_idx[k] = it.bi[k];
    res->block_off[k] = it.bo[k];
  }
}
bool marg_result_has_room(const okvis_ba_solver::MargPending::Item& it, const okvis_ba_marg_result* res) {
  if (it.na > res->capacity_dim || (int)it.bt.size() > res->capacity_blocks) return false;
  return !(it.na > 0 && (!res->H || !res->b0 || !res->J || !res->e0 || !res->block_type || !res->block_idx || !res->block_off));
}
void marg_pending_item(MargJob& J, size_t at, okvis_ba_solver::MargPending::Item& it) {
  it.w = J.w, it.na = J.na, it.nn = J.nn, it.n1 = J.n1, it.out_bytes = J.out_bytes, it.at = at;
  it.bt.swap(J.bt), it.bi.swap(J.bi), it.bo.swap(J.bo);
}
// The numbers of one window out of the download staging into its result; the accepted-buffer index back to the host's window.
int marg_hand_over(okvis_ba_solver* s, const okvis_ba_solver::MargPending::Item& it, okvis_ba_marg_result* res) {
  const int na = it.na;
  const unsigned char* base = s->stage_dl.data() + it.at;
  int info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  std::memcpy(info, base + it.out_bytes, sizeof(info));
  if (na > 0) {
    const double* h = reinterpret_cast<const double*>(base);
    std::memcpy(res->H, h, 8 * (size_t)na * na);
    std::memcpy(res->J, h + it.nn, 8 * (size_t)na * na);
    std::memcpy(res->b0, h + 2 * it.nn, 8 * (size_t)na);
    std::memcpy(res->e0, h + 2 * it.nn + it.n1, 8 * (size_t)na);
  }
  if (info[0] != na) return OKVIS_BA_ERR_NUMERIC;
  res->rank = info[2];
  res->sweeps[0] = info[3];
  res->sweeps[1] = info[4];
  if (debug_word().marg)
    std::fprintf(stderr, "marginalize: kept dim %d rank %d sweeps %d %d  pivoted-Cholesky bounds: dropped %.3f tau_hi, kept %d tau_hi\n", info[0],
                 info[2], info[3], info[4], info[6] * 1e-3, info[7]);
  marg_report_blocks(it, res);
  s->wins[it.w].acc = info[5] & 1;   // read by marg_dense_kernel after the export: no separate copy + synchronisation
  return OKVIS_BA_OK;
}

// The first half of a call for windows w0 .. w0 + n - 1: everything is enqueued, the kept blocks are reported.  `batch`: which of
// the two _end entries ends it.
int marg_begin(okvis_ba_solver* s, int w0, int n, const okvis_ba_marg_spec* specs, okvis_ba_marg_result* results, bool batch) {
  if (s) s->host.work_enqueued();
  if (!s || !specs || !results) return OKVIS_BA_ERR_ARG;
  if (!s->host.uploaded || s->marg_pending.active) return OKVIS_BA_ERR_STATE;
  if (n <= 0 || w0 < 0 || (int64_t)w0 + n > (int64_t)s->wins.size()) return OKVIS_BA_ERR_ARG;
  // every window's arguments before anything is enqueued
  std::vector<MargJob> jobs((size_t)n);
  for (int i = 0; i < n; ++i)
    if (int rc = marg_check(s, w0 + i, &specs[i], &results[i], jobs[i])) return rc;
  HIP_TRY(hipSetDevice(s->device));

  // ---- one scratch allocation for the call: what the host writes | workspaces, exported systems | every window's outputs ----
  Arena A;
  for (int i = 0; i < n; ++i) marg_place_host(A, s->wins[w0 + i], jobs[i]);
  const size_t o_wins = A.alloc(sizeof(WinPtrs) * (size_t)n), o_args = A.alloc(sizeof(MargArgs) * (size_t)n), o_opt = A.alloc(sizeof(OptD));
  const size_t host_part = A.size;   // ONE copy up
  for (int i = 0; i < n; ++i) {
    marg_place_work(A, jobs[i]);
    marg_place_tiles(A, jobs[i]);
  }
  for (int i = 0; i < n; ++i) marg_place_out(A, jobs[i]);
  const size_t out_base = jobs[0].o_out, out_total = A.size - out_base;   // ONE copy back
  s->stage_marg.resize(host_part);   // page-locked: the one upload of this call is a true asynchronous copy
  unsigned char* const hb = s->stage_marg.data();
  if (int rc = marg_reserve_scratch(s, A.size)) return rc;
  unsigned char* d = s->marg_scratch;
  std::vector<MargArgs> args((size_t)n);
  bool any_small = false;
  for (int i = 0; i < n; ++i) {
    const HostWin& H = s->wins[w0 + i];
    const MargJob& J = jobs[i];
    marg_fill_host(hb, H, J);
    const WinPtrs P = win_with_export(H, d, J.ex);
    std::memcpy(&hb[o_wins + sizeof(WinPtrs) * (size_t)i], &P, sizeof(P));
    marg_args(d, J, args[i]);
    if (J.tiles) {   // what marg_tiles_fallback launches with: the previous prior is part of H by then
      MargArgs again = args[i];
      again.prior_dim = 0;
      again.prior_nb = 0;
      std::memcpy(&hb[J.o_again], &again, sizeof(again));
    }
    any_small = any_small || !J.large;
  }
  std::memcpy(&hb[o_args], args.data(), sizeof(MargArgs) * (size_t)n);
  const WinPtrs* d_wins = reinterpret_cast<const WinPtrs*>(d + o_wins);
  const MargArgs* d_args = reinterpret_cast<const MargArgs*>(d + o_args);
  const OptD od = marg_optd(s);
  std::memcpy(&hb[o_opt], &od, sizeof(od));
  HIP_TRY(hipMemcpyAsync(d, hb, host_part, hipMemcpyHostToDevice, s->stream));
  MargSwapOptions swap_options{s, s->d_opt};
  s->d_opt = reinterpret_cast<OptD*>(d + o_opt);

  // ---- linearise + landmark elimination + export: one launch each for the range ----
  int rc = okvis_ba_begin(s);
  if (rc != OKVIS_BA_OK) return rc;
  s->host.not_begun();
  HIP_TRY(schur_and_export(s, w0, n, d_wins, any_small));
  // ---- the dense tail: a workgroup per window, one launch per run of consecutive windows on the LDS route (a range of the
  //      pipeline's sizes is one run) ----
  for (int i = 0; i < n;) {
    if (!jobs[i].lds_route) {
      ++i;
      continue;
    }
    int j = i;
    while (j < n && jobs[j].lds_route) ++j;
    marg_dense_launch(s, jobs[i], d_wins + i, d_args + i, 0, j - i);
    i = j;
  }
  HIP_TRY(hipGetLastError());
  s->stage_dl.resize(out_total + sizeof(int));
  int* const tiles_ok = reinterpret_cast<int*>(s->stage_dl.data() + out_total);
  // ---- windows off the LDS route, one after the other (HBM workspace, tiled tail and its fall-back, which is decided on the
  //      host: waited for here) ----
  int last_off = -1;
  for (int i = 0; i < n; ++i)
    if (!jobs[i].lds_route) last_off = i;
  bool copied = false;   // every window's H | J | b0 | e0 | info in ONE copy; the wait is marg_end's
  for (int i = 0; i <= last_off; ++i) {
    const MargJob& J = jobs[i];
    if (J.lds_route) continue;
    if (J.large) marg_export_large(s, J, d_wins + i);
    MargTiles mt{};
    marg_tail(s, J, d, d_wins + i, args[i], d_args + i, mt);
    HIP_TRY(hipGetLastError());
    if (J.tiles) {
      // (behind the last such window nothing else is enqueued: the numbers travel in front of the verdict instead of behind a second
      //  wait, and once more in the rare case that the verdict asks for the fall-back)
      if (i == last_off) HIP_TRY(hipMemcpyAsync(s->stage_dl.data(), d + out_base, out_total, hipMemcpyDeviceToHost, s->stream));
      *tiles_ok = 1;
      HIP_TRY(hipMemcpyAsync(tiles_ok, mt.ok, sizeof(int), hipMemcpyDeviceToHost, s->stream));
      HIP_TRY(hipStreamSynchronize(s->stream));
      copied = i == last_off && *tiles_ok;
      if (!*tiles_ok) {
        marg_tiles_fallback(s, J, d_wins + i, reinterpret_cast<const MargArgs*>(d + J.o_again));
        HIP_TRY(hipGetLastError());
      }
    }
  }
  if (!copied) HIP_TRY(hipMemcpyAsync(s->stage_dl.data(), d + out_base, out_total, hipMemcpyDeviceToHost, s->stream));
  okvis_ba_solver::MargPending& mp = s->marg_pending;
  mp.items.assign((size_t)n, okvis_ba_solver::MargPending::Item{});
  for (int i = 0; i < n; ++i) {
    marg_pending_item(jobs[i], jobs[i].o_out - out_base, mp.items[i]);
    marg_report_blocks(mp.items[i], &results[i]);
  }
  mp.active = true;
  mp.batch = batch;
  return OKVIS_BA_OK;
}

// The second half: the wait and every window's numbers.
int marg_end(okvis_ba_solver* s, okvis_ba_marg_result* results, bool batch) {
  if (!s || !results) return OKVIS_BA_ERR_ARG;
  okvis_ba_solver::MargPending& mp = s->marg_pending;
  if (!mp.active || mp.batch != batch) return OKVIS_BA_ERR_STATE;   // (a pending call is ended by the _end of its own pair)
  // every result structure is looked at first: a call with too little room anywhere changes nothing and can be repeated with more
  for (size_t i = 0; i < mp.items.size(); ++i)
    if (!marg_result_has_room(mp.items[i], &results[i])) return OKVIS_BA_ERR_ARG;
  mp.active = false;   // (whatever happens below, the call is over)
  HIP_TRY(hipSetDevice(s->device));
  HIP_TRY(hipStreamSynchronize(s->stream));
  int rc = OKVIS_BA_OK;   // (a numeric failure of one window does not keep the others' numbers back: the first one is reported)
  for (size_t i = 0; i < mp.items.size(); ++i) {
    const int r = marg_hand_over(s, mp.items[i], &results[i]);
    if (rc == OKVIS_BA_OK) rc = r;
  }
  if (rc != OKVIS_BA_OK) return rc;
  s->host.acc_read();
  return OKVIS_BA_OK;
}

}  // namespace

int okvis_ba_marginalize_begin(okvis_ba_solver* s, int w, const okvis_ba_marg_spec* spec, okvis_ba_marg_result* res) {
  return marg_begin(s, w, 1, spec, res, false);
}
int okvis_ba_marginalize_end(okvis_ba_solver* s, okvis_ba_marg_result* res) { return marg_end(s, res, false); }
int okvis_ba_marginalize(okvis_ba_solver* s, int w, const okvis_ba_marg_spec* spec, okvis_ba_marg_result* res) {
  if (int rc = marg_begin(s, w, 1, spec, res, false)) return rc;
  return marg_end(s, res, false);
}

int okvis_ba_marginalize_batch_begin(okvis_ba_solver* s, int w0, int n, const okvis_ba_marg_spec* specs, okvis_ba_marg_result* results) {
  return marg_begin(s, w0, n, specs, results, true);
}
int okvis_ba_marginalize_batch_end(okvis_ba_solver* s, okvis_ba_marg_result* results) { return marg_end(s, results, true); }
int okvis_ba_marginalize_batch(okvis_ba_solver* s, int w0, int n, const okvis_ba_marg_spec* specs, okvis_ba_marg_result* results) {
  if (int rc = marg_begin(s, w0, n, specs, results, true)) return rc;
  return marg_end(s, results, true);
}
