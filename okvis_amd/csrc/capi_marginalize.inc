// Part of ba_capi.hip, inside its extern "C" block.  okvis_ba_marginalize / _begin / _end (DESIGN.md section 5, "Marginalisation").
// MarginalizationError numerics (see include/okvis_amd_ba.h): linearise at the uploaded values, eliminate
// the landmarks (schur_kernel in marg_mode), export the dense system (solve_kernel final_only = 2), then the
// dense elimination + eigen-decomposition (marg_dense_kernel).
int okvis_ba_marginalize(okvis_ba_solver* s, int w, const okvis_ba_marg_spec* spec, okvis_ba_marg_result* res) {
  if (int rc = okvis_ba_marginalize_begin(s, w, spec, res)) return rc;
  return okvis_ba_marginalize_end(s, res);
}

int okvis_ba_marginalize_begin(okvis_ba_solver* s, int w, const okvis_ba_marg_spec* spec, okvis_ba_marg_result* res) {
  if (s) s->acc_fresh = false;
  if (!s || !spec || !res) return OKVIS_BA_ERR_ARG;
  if (!s->uploaded || s->marg_pending.active) return OKVIS_BA_ERR_STATE;
  if (w < 0 || w >= (int)s->wins.size()) return OKVIS_BA_ERR_ARG;
  HostWin& H = s->wins[w];
  if (H.marg_dim != 0) return OKVIS_BA_ERR_ARG;                    // the previous prior comes in through spec
  const bool large_window = H.ptrs.Sg != nullptr;   // reduced system assembled in HBM (D > MAX_D_LDS)
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
  // kept blocks, in reduced order (pose-type blocks first)
  std::vector<int> bt, bi, bo;
  int na = 0;
  for (int i = 0; i < H.n_pose; ++i)
    if (H.pose_off[i] >= 0 && !spec->pose_marg[i]) {
      bt.push_back(OKVIS_BA_BLOCK_POSE); bi.push_back(i); bo.push_back(na);
      na += 6;
    }
  for (int i = 0; i < H.n_sb; ++i)
    if (H.sb_off[i] >= 0 && !spec->sb_marg[i]) {
      bt.push_back(OKVIS_BA_BLOCK_SPEEDBIAS); bi.push_back(i); bo.push_back(na);
      na += 9;
    }
  if (na > res->capacity_dim || (int)bt.size() > res->capacity_blocks) return OKVIS_BA_ERR_ARG;
  if (na > 0 && (!res->H || !res->b0 || !res->J || !res->e0 || !res->block_type || !res->block_idx || !res->block_off))
    return OKVIS_BA_ERR_ARG;
  HIP_TRY(hipSetDevice(s->device));

  // ---- one scratch allocation ----
  const int D = H.D;
  Arena A;
  const size_t o_pm = A.alloc(std::max(1, H.n_pose)), o_sm = A.alloc(std::max(1, H.n_sb));
  const size_t o_pt = A.alloc(sizeof(int) * std::max(1, pnb)), o_pi = A.alloc(sizeof(int) * std::max(1, pnb)),
               o_po = A.alloc(sizeof(int) * std::max(1, pnb));
  const size_t o_pH = A.alloc(8 * std::max<size_t>(1, (size_t)pd * pd)), o_pb = A.alloc(8 * std::max(1, pd));
  const size_t o_win = A.alloc(sizeof(WinPtrs)), o_opt = A.alloc(sizeof(OptD));
  const size_t host_part = A.size;   // everything up to here is written by the host: ONE copy
  const size_t o_work = A.alloc(8 * marg_work_doubles(std::max(1, D)));
  const size_t o_S = A.alloc(8 * std::max<size_t>(1, (size_t)D * D)), o_rhs = A.alloc(8 * std::max(1, D)),
               o_d2 = A.alloc(8 * std::max(1, D));
  // H | J | b0 | e0 | info: contiguous, ONE copy back
  const size_t nn = std::max<size_t>(1, (size_t)na * na), n1 = std::max(1, na);
  const size_t out_bytes = 8 * (2 * nn + 2 * n1);
  const size_t o_out = A.alloc(out_bytes + sizeof(int) * (8 + std::max(1, D)));
  const size_t o_info = o_out + out_bytes;
  // kept blocks beyond the single-workgroup LDS paths: the tail on many workgroups (ba_marg_tiles.hpp)
  const bool no_tiles = (s->opt.tuning.flags & OKVIS_BA_TUNE_NO_MARG_TILES) != 0;   // (A/B switch)
  const bool tiles = na > MARG_PC_NMAX && !no_tiles;
  const int mt_nT = tiles ? (na + CT_TB - 1) / CT_TB : 0, mt_ntiles = mt_nT * (mt_nT + 1) / 2;
  const size_t o_mtT = A.alloc(8 * (size_t)std::max(1, mt_ntiles) * CT_TILE), o_mtZ = A.alloc(8 * (size_t)std::max(1, mt_ntiles) * CT_TILE),
               o_mtL = A.alloc(8 * (size_t)std::max(1, mt_nT) * CT_TILE), o_mtR = A.alloc(8 * (size_t)std::max(1, CT_TB * mt_nT)),
               o_mtY = A.alloc(8 * (size_t)std::max(1, CT_TB * mt_nT)), o_mtP = A.alloc(8 * (size_t)std::max(1, CT_TB * mt_nT)),
               o_mtF = A.alloc(8 * (size_t)std::max(1, mt_ntiles)), o_mtp = A.alloc(8 * (size_t)std::max(1, D)),
               o_mtS = A.alloc(8 * (size_t)std::max(1, CT_TB * mt_nT)),
               o_mtf = A.alloc(sizeof(int) * (size_t)(mt_ntiles + 1 + 2 * mt_nT + 1 + mt_ntiles));
  s->stage_marg.resize(host_part);   // page-locked: the one upload of this call is a true asynchronous copy
  unsigned char* const hb = s->stage_marg.data();
  if (H.n_pose) std::memcpy(&hb[o_pm], spec->pose_marg, H.n_pose);
  if (H.n_sb) std::memcpy(&hb[o_sm], spec->sb_marg, H.n_sb);
  if (pd > 0) {
    std::memcpy(&hb[o_pt], spec->prior_block_type, sizeof(int) * pnb);
    std::memcpy(&hb[o_pi], spec->prior_block_idx, sizeof(int) * pnb);
    std::memcpy(&hb[o_po], spec->prior_block_off, sizeof(int) * pnb);
    std::memcpy(&hb[o_pH], spec->prior_H, 8 * (size_t)pd * pd);
    std::memcpy(&hb[o_pb], spec->prior_b0, 8 * (size_t)pd);
  }
  if (A.size > s->marg_scratch_bytes) {
    if (s->marg_scratch) HIP_TRY(hipFree(s->marg_scratch));
    s->marg_scratch = nullptr;
    s->marg_scratch_bytes = 0;
    HIP_TRY(hipMalloc(&s->marg_scratch, A.size));
    s->marg_scratch_bytes = A.size;
  }
  unsigned char* d = s->marg_scratch;
  WinPtrs P = H.ptrs;   // this window with the export buffers attached
  P.S = (decltype(P.S))(d + o_S);
  P.rhs = (decltype(P.rhs))(d + o_rhs);
  P.Dp2 = (decltype(P.Dp2))(d + o_d2);
  P.grad = nullptr;
  std::memcpy(&hb[o_win], &P, sizeof(P));
  const WinPtrs* d_win = reinterpret_cast<const WinPtrs*>(d + o_win);
  // the marginalisation pass has its own option record in the scratch block (no trust region: one linearisation, no damping);
  // the launches below read it through s->d_opt, which points there for the duration of this call.  The solver's own record is
  // never touched, so nothing has to be restored on the device and captured launch graphs stay valid.
  OptD od = make_optd(s->opt, (int)s->wins.size());
  od.marg_mode = 1;
  od.dogleg = 0;
  std::memcpy(&hb[o_opt], &od, sizeof(od));
  HIP_TRY(hipMemcpyAsync(d, hb, host_part, hipMemcpyHostToDevice, s->stream));
  struct SwapOptions {
    okvis_ba_solver* s;
    OptD* saved;
    ~SwapOptions() { s->d_opt = saved; }
  } swap_options{s, s->d_opt};
  s->d_opt = reinterpret_cast<OptD*>(d + o_opt);

  // ---- linearise + landmark elimination + export ----
  int rc = okvis_ba_begin(s);
  if (rc != OKVIS_BA_OK) return rc;
  s->begun = false;
  HIP_TRY(launch_schur(s, sub(s->stream, Extent{w, 1, s->plan.one_helpers})));
  if (large_window) {
    // assembly of the undamped system, then the kernel that completes it (Schur partials, IMU terms) and, because this copy of
    // the window carries an S pointer, writes it out as one full symmetric D x D matrix
    launch_solve_kernel(s, s->plan.tiled, dim3(1), s->stream, d_win, 2, s->d_ctrl + w);
    const int nT = (((D + 5) / 6) * 6 + CT_TB - 1) / CT_TB;
    hipLaunchKernelGGL(large_export_kernel, dim3(nT * (nT + 1) / 2, 1, CT_TILE / CT_THREADS), dim3(CT_THREADS), 0, s->stream, d_win);
  } else
    launch_solve_kernel(s, s->plan.solve, dim3(1, 1 + s->plan.one_helpers), s->stream, d_win, 2, s->d_ctrl + w);
  HIP_TRY(hipGetLastError());
  MargArgs ma;
  ma.pose_marg = d + o_pm;
  ma.sb_marg = d + o_sm;
  ma.prior_dim = pd;
  ma.prior_nb = pd > 0 ? pnb : 0;
  ma.pb_type = reinterpret_cast<const int*>(d + o_pt);
  ma.pb_idx = reinterpret_cast<const int*>(d + o_pi);
  ma.pb_off = reinterpret_cast<const int*>(d + o_po);
  ma.prior_H = reinterpret_cast<const double*>(d + o_pH);
  ma.prior_b0 = reinterpret_cast<const double*>(d + o_pb);
  ma.work = reinterpret_cast<double*>(d + o_work);
  double* outp = reinterpret_cast<double*>(d + o_out);
  ma.out_H = outp;
  ma.out_J = outp + nn;
  ma.out_b0 = outp + 2 * nn;
  ma.out_e0 = outp + 2 * nn + n1;
  ma.out_info = reinterpret_cast<int*>(d + o_info);
  ma.p_out = reinterpret_cast<double*>(d + o_mtp);
  auto dense = [&](const MargArgs& args, int stage) {
    if (large_window || pd > MARG_SMALL_PRIOR)
      hipLaunchKernelGGL((marg_dense_kernel<MAX_D, MAX_MARG_DIM>), dim3(1), dim3(MARG_THREADS), MARG_LDS_DOUBLES_LARGE * 8, s->stream, d_win, 0,
                         args, MARG_LDS_DOUBLES_LARGE, stage);
    else
      hipLaunchKernelGGL((marg_dense_kernel<MAX_D_LDS, MARG_SMALL_PRIOR>), dim3(1), dim3(MARG_THREADS), MARG_LDS_DOUBLES * 8, s->stream, d_win, 0,
                         args, MARG_LDS_DOUBLES, stage);
  };
  MargTiles mt{};
  if (tiles) {
    // the single workgroup stops after M and b0; Schur complement, scaling, tiled factorisation (matrix core), L^-1 for the proof
    // of full rank, J and e0 on many workgroups
    mt.C.nT = mt_nT;
    mt.C.T = reinterpret_cast<double*>(d + o_mtT);
    mt.C.Linv = reinterpret_cast<double*>(d + o_mtL);
    mt.C.rhs = reinterpret_cast<double*>(d + o_mtR);
    mt.C.y = reinterpret_cast<double*>(d + o_mtY);
    mt.C.flag = reinterpret_cast<int*>(d + o_mtf);
    mt.C.pflag = mt.C.flag + mt_ntiles + 1;
    mt.Z = reinterpret_cast<double*>(d + o_mtZ);
    mt.fro = reinterpret_cast<double*>(d + o_mtF);
    mt.p2 = reinterpret_cast<double*>(d + o_mtP);
    mt.rowsum = reinterpret_cast<double*>(d + o_mtS);
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
    int nm = 0;   // rows of the eliminated block
    for (int i = 0; i < H.n_pose; ++i) nm += (H.pose_off[i] >= 0 && spec->pose_marg[i]) ? 6 : 0;
    for (int i = 0; i < H.n_sb; ++i) nm += (H.sb_off[i] >= 0 && spec->sb_marg[i]) ? 9 : 0;
    if (nm > 0) {
      dense(ma, 1 | 2 | 4);
      hipLaunchKernelGGL(marg_M_kernel, dim3((unsigned)(((size_t)na * nm + MARG_TILES_THREADS - 1) / MARG_TILES_THREADS)), dim3(MARG_TILES_THREADS), 0,
                         s->stream, d_win, ma);
      hipLaunchKernelGGL(marg_b0_kernel, dim3((unsigned)((na + MARG_TILES_THREADS - 1) / MARG_TILES_THREADS)), dim3(MARG_TILES_THREADS), 0, s->stream,
                         d_win, ma);
    } else {
      dense(ma, 1 | 2);   // (nothing to eliminate densely: b0 is a gather)
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
  } else {
    dense(ma, 0);
  }
  HIP_TRY(hipGetLastError());
  // H | J | b0 | e0 | info are contiguous on the device: one copy into page-locked staging, one synchronisation
  int info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  s->stage_dl.resize(out_bytes + sizeof(info) + sizeof(int));
  int* const tiles_ok = reinterpret_cast<int*>(s->stage_dl.data() + out_bytes + sizeof(info));
  // (the tiled route may have to fall back on the single workgroup, which needs this call's arguments: it is waited for here;
  //  the route of the pipeline's sizes only enqueues the copy and leaves the wait to okvis_ba_marginalize_end)
  auto fetch = [&]() -> hipError_t {
    hipError_t e = hipMemcpyAsync(s->stage_dl.data(), outp, out_bytes + sizeof(info), hipMemcpyDeviceToHost, s->stream);
    if (e == hipSuccess && tiles) e = hipMemcpyAsync(tiles_ok, mt.ok, sizeof(int), hipMemcpyDeviceToHost, s->stream);
    if (e == hipSuccess && tiles) e = hipStreamSynchronize(s->stream);
    return e;
  };
  *tiles_ok = 1;
  HIP_TRY(fetch());
  if (tiles && !*tiles_ok) {
    // no proof of full rank (a rank-deficient kept block, a pivot that is not positive): the single workgroup takes over — the
    // previous prior is part of H already, everything else is done again — and goes on to the eigen-decomposition
    MargArgs again = ma;
    again.prior_dim = 0;
    again.prior_nb = 0;
    dense(again, 0);
    HIP_TRY(hipGetLastError());
    *tiles_ok = 1;
    hipError_t e = hipMemcpyAsync(s->stage_dl.data(), outp, out_bytes + sizeof(info), hipMemcpyDeviceToHost, s->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(s->stream);
    HIP_TRY(e);
    s->marg_tiles_fallbacks++;
  }
  // what is known without the numbers: the blocks the new prior connects
  res->dim = na;
  res->nblocks = (int)bt.size();
  for (size_t k = 0; k < bt.size(); ++k) {
    res->block_type[k] = bt[k];
    res->block_idx[k] = bi[k];
    res->block_off[k] = bo[k];
  }
  okvis_ba_solver::MargPending& mp = s->marg_pending;
  mp.active = true;
  mp.synced = tiles;
  mp.w = w, mp.na = na, mp.nn = nn, mp.n1 = n1, mp.out_bytes = out_bytes;
  mp.bt.swap(bt), mp.bi.swap(bi), mp.bo.swap(bo);
  return OKVIS_BA_OK;
}

int okvis_ba_marginalize_end(okvis_ba_solver* s, okvis_ba_marg_result* res) {
  if (!s || !res) return OKVIS_BA_ERR_ARG;
  okvis_ba_solver::MargPending& mp = s->marg_pending;
  if (!mp.active) return OKVIS_BA_ERR_STATE;
  // the result structure is looked at first: a call with too little room changes nothing and can be repeated with more
  if (mp.na > res->capacity_dim || (int)mp.bt.size() > res->capacity_blocks) return OKVIS_BA_ERR_ARG;
  if (mp.na > 0 && (!res->H || !res->b0 || !res->J || !res->e0 || !res->block_type || !res->block_idx || !res->block_off)) return OKVIS_BA_ERR_ARG;
  mp.active = false;   // (whatever happens below, the call is over)
  HIP_TRY(hipSetDevice(s->device));
  if (!mp.synced) HIP_TRY(hipStreamSynchronize(s->stream));
  const int na = mp.na;
  const size_t nn = mp.nn, n1 = mp.n1, out_bytes = mp.out_bytes;
  const std::vector<int>&bt = mp.bt, &bi = mp.bi, &bo = mp.bo;
  HostWin& H = s->wins[mp.w];
  if (na > res->capacity_dim || (int)bt.size() > res->capacity_blocks) return OKVIS_BA_ERR_ARG;
  if (na > 0 && (!res->H || !res->b0 || !res->J || !res->e0 || !res->block_type || !res->block_idx || !res->block_off)) return OKVIS_BA_ERR_ARG;
  int info[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  std::memcpy(info, s->stage_dl.data() + out_bytes, sizeof(info));
  if (na > 0) {
    const double* h = reinterpret_cast<const double*>(s->stage_dl.data());
    std::memcpy(res->H, h, 8 * (size_t)na * na);
    std::memcpy(res->J, h + nn, 8 * (size_t)na * na);
    std::memcpy(res->b0, h + 2 * nn, 8 * (size_t)na);
    std::memcpy(res->e0, h + 2 * nn + n1, 8 * (size_t)na);
  }
  if (info[0] != na) return OKVIS_BA_ERR_NUMERIC;
  res->dim = na;
  res->nblocks = (int)bt.size();
  res->rank = info[2];
  res->sweeps[0] = info[3];
  res->sweeps[1] = info[4];
  if (debug_word().marg)
    std::fprintf(stderr, "marginalize: kept dim %d rank %d sweeps %d %d  pivoted-Cholesky bounds: dropped %.3f tau_hi, kept %d tau_hi\n", info[0],
                 info[2], info[3], info[4], info[6] * 1e-3, info[7]);
  for (size_t k = 0; k < bt.size(); ++k) {
    res->block_type[k] = bt[k];
    res->block_idx[k] = bi[k];
    res->block_off[k] = bo[k];
  }
  H.acc = info[5] & 1;   // read by marg_dense_kernel after the export: no separate copy + synchronisation
  s->acc_fresh = true;
  return OKVIS_BA_OK;
}
