// Part of ba_capi.hip, inside its extern "C" block.  Entry points that do not need an uploaded solver: the sharding rule and one rank's
// batch run (DESIGN.md section 7), the tiled Cholesky and the LDS solvers stand-alone on a caller's matrix (diagnostics).
int okvis_ba_shard(int32_t n_total, int32_t rank, int32_t world, int32_t* ids_out, int32_t* n_out) {
  if (n_total < 0 || world <= 0 || rank < 0 || rank >= world || !ids_out || !n_out) return OKVIS_BA_ERR_ARG;
  int32_t n = 0;
  for (int32_t i = rank; i < n_total; i += world) ids_out[n++] = i;   // window i -> rank i mod world
  *n_out = n;
  return OKVIS_BA_OK;
}

int okvis_ba_batch_run(int device, int32_t rank, int32_t world, int32_t n_total, const okvis_ba_window* all_windows,
                       const okvis_ba_options* opt, int num_iter, okvis_ba_window_record* records_out, int32_t* n_out) {
  if (!all_windows || !records_out || !n_out || num_iter < 0) return OKVIS_BA_ERR_ARG;
  std::vector<int32_t> ids((size_t)std::max(1, (n_total + std::max(world, 1) - 1) / std::max(world, 1)));
  int32_t n = 0;
  int rc = okvis_ba_shard(n_total, rank, world, ids.data(), &n);
  if (rc != OKVIS_BA_OK) return rc;
  *n_out = n;
  if (n == 0) return OKVIS_BA_OK;
  std::vector<okvis_ba_window> mine((size_t)n);
  for (int32_t k = 0; k < n; ++k) mine[(size_t)k] = all_windows[ids[(size_t)k]];
  okvis_ba_solver* s = nullptr;
  rc = okvis_ba_create(&s, device);
  if (rc != OKVIS_BA_OK) return rc;
  if (opt) rc = okvis_ba_set_options(s, opt);
  if (rc == OKVIS_BA_OK) rc = okvis_ba_upload(s, n, mine.data());
  std::vector<okvis_ba_summary> sum((size_t)n);
  double seconds = 0;
  if (rc == OKVIS_BA_OK) {
    const auto t0 = std::chrono::steady_clock::now();
    rc = okvis_ba_optimize(s, num_iter, sum.data());   // ends with a stream synchronisation (summaries are read back)
    seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
  }
  if (rc == OKVIS_BA_OK)
    for (int32_t k = 0; k < n; ++k) {
      records_out[k].window_id = (uint32_t)ids[(size_t)k];
      records_out[k].iterations = (uint32_t)sum[(size_t)k].iterations;
      records_out[k].final_cost = sum[(size_t)k].final_cost;
      records_out[k].seconds = seconds;
    }
  (void)okvis_ba_destroy(s);
  return rc;
}

int okvis_ba_dense_solve(int device, int32_t n, const double* S, const double* rhs, double* x, int32_t* info) {
  if (n <= 0 || !S || !rhs || !x || !info) return OKVIS_BA_ERR_ARG;
  hipError_t e = hipSetDevice(device);
  if (e != hipSuccess) return OKVIS_BA_ERR_NO_DEVICE;
  const int nT = (n + CT_TB - 1) / CT_TB, ntiles = nT * (nT + 1) / 2, np = nT * CT_TB;
  std::vector<double> tiles((size_t)ntiles * CT_TILE, 0.0), r(np, 0.0);
  for (int i = 0; i < nT; ++i)
    for (int j = 0; j <= i; ++j) {
      double* t = &tiles[(size_t)(i * (i + 1) / 2 + j) * CT_TILE];
      for (int a = 0; a < CT_TB; ++a)
        for (int b = 0; b < CT_TB; ++b) {
          const int gi = CT_TB * i + a, gj = CT_TB * j + b;
          t[a * CT_TB + b] = (gi < n && gj < n) ? S[(size_t)gi * n + gj] : ((gi == gj) ? 1.0 : 0.0);
        }
    }
  for (int k = 0; k < n; ++k) r[k] = rhs[k];
  Arena A;
  const size_t oT = A.alloc(8 * tiles.size()), oL = A.alloc(8 * (size_t)nT * CT_TILE), oR = A.alloc(8 * (size_t)np),
               oY = A.alloc(8 * (size_t)np), oX = A.alloc(8 * (size_t)np), oF = A.alloc(sizeof(int) * (ntiles + 1 + 2 * nT));
  unsigned char* d = nullptr;
  if (hipMalloc(&d, A.size) != hipSuccess) return OKVIS_BA_HIP_ERROR_BASE + (int)hipGetLastError();
  struct Free { unsigned char* p; ~Free() { if (p) (void)hipFree(p); } } guard{d};
  auto chk = [](hipError_t err) { return err == hipSuccess ? OKVIS_BA_OK : OKVIS_BA_HIP_ERROR_BASE + (int)err; };
  int rc;
  if ((rc = chk(hipMemcpy(d + oT, tiles.data(), 8 * tiles.size(), hipMemcpyHostToDevice)))) return rc;
  if ((rc = chk(hipMemcpy(d + oR, r.data(), 8 * (size_t)np, hipMemcpyHostToDevice)))) return rc;
  if ((rc = chk(hipMemset(d + oF, 0, sizeof(int) * (ntiles + 1 + 2 * nT))))) return rc;
  {
    std::vector<unsigned long long> sentinel(np, CT_X_SENTINEL);
    if ((rc = chk(hipMemcpy(d + oX, sentinel.data(), 8 * (size_t)np, hipMemcpyHostToDevice)))) return rc;
  }
  CholTiles C;
  C.nT = nT;
  C.T = reinterpret_cast<double*>(d + oT);
  C.Linv = reinterpret_cast<double*>(d + oL);
  C.rhs = reinterpret_cast<double*>(d + oR);
  C.y = reinterpret_cast<double*>(d + oY);
  C.flag = reinterpret_cast<int*>(d + oF);
  C.pflag = C.flag + ntiles + 1;
  C.x = reinterpret_cast<double*>(d + oX);
  if ((rc = chk(hipFuncSetAttribute(reinterpret_cast<const void*>(chol_tile_kernel), hipFuncAttributeMaxDynamicSharedMemorySize,
                                    CT_SMEM_DOUBLES * 8))))
    return rc;
  hipLaunchKernelGGL(chol_tile_kernel, dim3(ntiles + nT), dim3(CT_THREADS), CT_SMEM_DOUBLES * 8, 0, C);
  if ((rc = chk(hipGetLastError()))) return rc;
  if ((rc = chk(hipDeviceSynchronize()))) return rc;
  std::vector<double> xs(np);
  int fail = 0;
  if ((rc = chk(hipMemcpy(xs.data(), d + oX, 8 * (size_t)np, hipMemcpyDeviceToHost)))) return rc;
  if ((rc = chk(hipMemcpy(&fail, d + oF + sizeof(int) * ntiles, sizeof(int), hipMemcpyDeviceToHost)))) return rc;
  for (int k = 0; k < n; ++k) x[k] = xs[k];
  *info = fail;
  return OKVIS_BA_OK;
}

int okvis_ba_reduced_solve(int device, int32_t D, int32_t Dp, int32_t mode, uint32_t comp_mask, const double* S, const double* rhs,
                           double* x, int64_t* ticks, int32_t* info, int32_t repeats, double* lds_dump, int64_t lds_capacity) {
  if (D <= 0 || D > MAX_D_LDS || Dp < 0 || Dp > D || (D - Dp) % 9 != 0 || !S || !rhs || !x || !info) return OKVIS_BA_ERR_ARG;
  const bool chain = mode == OKVIS_BA_SOLVE_CHAIN;
  if (chain && (Dp < 6 || D == Dp || !LChain::tiles_fit(Dp))) return OKVIS_BA_ERR_ARG;
  if (chain) {
    // the fit rule of the index build (BuildCtx::layout): what the upload refuses for LDS is not launched here either
    if ((D - Dp) / 9 > CH_MAX_KS || (int)solve_smem_chain(LChain::make(D, Dp).total, ((D + 5) / 6) * 6) > SOLVE_LDS_LIMIT_CHAIN)
      return OKVIS_BA_ERR_ARG;
    // the chain structure: a speed/bias block couples to its two neighbours only.  LChain::at sends every other coupling to the
    // always-zero words at oZ, which the sweeps read as zeros: the solve would return a wrong x with info = 0
    for (int i = Dp; i < D; ++i)
      for (int j = Dp; j < D; ++j) {
        const int a = (i - Dp) / 9, b = (j - Dp) / 9;
        if ((a > b + 1 || b > a + 1) && S[(size_t)i * D + j] != 0.0) return OKVIS_BA_ERR_ARG;
      }
  }
  if (hipSetDevice(device) != hipSuccess) return OKVIS_BA_ERR_NO_DEVICE;
  if (repeats < 1) repeats = 1;
  auto chk = [](hipError_t err) { return err == hipSuccess ? OKVIS_BA_OK : OKVIS_BA_HIP_ERROR_BASE + (int)err; };
  unsigned char* d = nullptr;
  const size_t n_lds = chain ? (size_t)LChain::make(D, Dp).total : (size_t)ldl16_area_doubles(D);
  const bool dumping = lds_dump && lds_capacity >= (int64_t)n_lds;
  const size_t nS = 8 * (size_t)D * D, total = nS + 16 * (size_t)D + 64 + (dumping ? 8 * n_lds : 0);
  if (hipMalloc(&d, total) != hipSuccess) return OKVIS_BA_HIP_ERROR_BASE + (int)hipGetLastError();
  struct Free { unsigned char* p; ~Free() { if (p) (void)hipFree(p); } } guard{d};
  int rc;
  if ((rc = chk(hipMemcpy(d, S, nS, hipMemcpyHostToDevice)))) return rc;
  if ((rc = chk(hipMemcpy(d + nS, rhs, 8 * (size_t)D, hipMemcpyHostToDevice)))) return rc;
  double* dx = reinterpret_cast<double*>(d + nS + 8 * (size_t)D);
  long long* dt = reinterpret_cast<long long*>(d + nS + 16 * (size_t)D);
  int* di = reinterpret_cast<int*>(dt + 1);
  double* dd = dumping ? reinterpret_cast<double*>(d + nS + 16 * (size_t)D + 64) : nullptr;
  const size_t smem = ((chain ? (size_t)LChain::make(D, Dp).total : (size_t)ldl16_area_doubles(D)) + (size_t)D + 8) * sizeof(double);
  const void* fn = chain ? reinterpret_cast<const void*>(&reduced_solve_kernel<true>) : reinterpret_cast<const void*>(&reduced_solve_kernel<false>);
  if ((rc = chk(hipFuncSetAttribute(fn, hipFuncAttributeMaxDynamicSharedMemorySize, (int)std::max<size_t>(smem, 65536))))) return rc;
  if (chain)
    hipLaunchKernelGGL(reduced_solve_kernel<true>, dim3(1), dim3(SOLVE_THREADS), smem, 0, reinterpret_cast<const double*>(d),
                       reinterpret_cast<const double*>(d + nS), D, Dp, comp_mask, dx, dt, di, repeats, dd);
  else
    hipLaunchKernelGGL(reduced_solve_kernel<false>, dim3(1), dim3(SOLVE_THREADS), smem, 0, reinterpret_cast<const double*>(d),
                       reinterpret_cast<const double*>(d + nS), D, Dp, comp_mask, dx, dt, di, repeats, dd);
  if ((rc = chk(hipGetLastError()))) return rc;
  if ((rc = chk(hipDeviceSynchronize()))) return rc;
  if ((rc = chk(hipMemcpy(x, dx, 8 * (size_t)D, hipMemcpyDeviceToHost)))) return rc;
  long long t = 0;
  int f = 0;
  if ((rc = chk(hipMemcpy(&t, dt, sizeof(t), hipMemcpyDeviceToHost)))) return rc;
  if ((rc = chk(hipMemcpy(&f, di, sizeof(f), hipMemcpyDeviceToHost)))) return rc;
  if (ticks) *ticks = t;
  *info = f;
  if (dumping && (rc = chk(hipMemcpy(lds_dump, dd, 8 * n_lds, hipMemcpyDeviceToHost)))) return rc;
  return OKVIS_BA_OK;
}
