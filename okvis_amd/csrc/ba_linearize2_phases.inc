// Part of ba_linearize2.hpp, included in the body of linearize2_kernel and of linearize2_rec_kernel behind their operand requests
// (G, ops, hv): phases A, B and C of one group.  One text for both kernels, so that they form the same products in the same places.
    const int nlm = G.lm_end - G.lm_begin;
    const int nobs = G.obs_end - G.obs_begin;
    const int npair = G.pair_end - G.pair_begin;
    const int ntask = G.task_end - G.task_begin;
    const bool has_obs = tid < nobs, has_pair = tid < npair;
    const bool tasks_cached = ntask <= LIN_TASK_CACHE;
    const ObsRec rec = ops.rec;
    const int pf_poff = ops.poff, pf_plm = ops.plm, pf_pblock = ops.pblock;
    double pf_sc[3] = {1.0, 1.0, 1.0};
    if (fast && !init && tid >= 64 && tid - 64 < nlm) {   // (the landmark work of the group reduction is done by wave 1)
      const double* sl = W.lm_scale + 3 * (size_t)(G.lm_begin + tid - 64);
      pf_sc[0] = sl[0], pf_sc[1] = sl[1], pf_sc[2] = sl[2];
    }
    LSTAMP(41);
    // ------------------------------------------------------------------ phase A: back-substitution
    if (!init) {
      __syncthreads();   // the step is in LDS
      if (has_pair) {
        const double* d = s_step + pf_poff;
        double t0 = 0, t1 = 0, t2 = 0;
#pragma unroll
        for (int i = 0; i < 6; ++i) {
          t0 += hv.Wp0[3 * i] * d[i];
          t1 += hv.Wp0[3 * i + 1] * d[i];
          t2 += hv.Wp0[3 * i + 2] * d[i];
        }
        s_pair[3 * tid] = t0;
        s_pair[3 * tid + 1] = t1;
        s_pair[3 * tid + 2] = t2;
      }
      __syncthreads();
      double sc_gd = 0, sc_ddd = 0, sc_s2 = 0, sc_x2 = 0;
      if (tid < nlm) {
        const int l = G.lm_begin + tid;
        double t[3] = {hv.bb[0], hv.bb[1], hv.bb[2]};
        for (int p = hv.lp0; p < hv.lp1; ++p) {
          const double* sp = s_pair + 3 * p;
          t[0] += sp[0];
          t[1] += sp[1];
          t[2] += sp[2];
        }
        double v[6] = {hv.v[0], hv.v[1], hv.v[2], hv.v[3], hv.v[4], hv.v[5]};
        const double d0 = damp_diag(v[0], hv.sl[0], opt);
        const double d1 = damp_diag(v[3], hv.sl[1], opt);
        const double d2 = damp_diag(v[5], hv.sl[2], opt);
        v[0] += lambda * d0;
        v[3] += lambda * d1;
        v[5] += lambda * d2;
        double vi[6];
        inv3sym(v, vi);
        // (dogleg: this is the landmark part of the Gauss-Newton point; the scalars g.delta and delta^T D^2 delta below
        //  always refer to it, they decide whether the point lies inside the trust region)
        const double dl0 = -(vi[0] * t[0] + vi[1] * t[1] + vi[2] * t[2]);
        const double dl1 = -(vi[1] * t[0] + vi[3] * t[1] + vi[4] * t[2]);
        const double dl2 = -(vi[2] * t[0] + vi[4] * t[1] + vi[5] * t[2]);
        double st0 = dl0, st1 = dl1, st2 = dl2;
        if (dl_explicit) {   // explicit dogleg step  -cA xv + beta dGN,  xv_l = b_l / Dt2_l
          st0 = -dl_cA * (hv.bb[0] / d0) + dl_beta * dl0;
          st1 = -dl_cA * (hv.bb[1] / d1) + dl_beta * dl1;
          st2 = -dl_cA * (hv.bb[2] / d2) + dl_beta * dl2;
        }
        const double x0 = hv.xx[0], x1 = hv.xx[1], x2 = hv.xx[2], x3 = hv.xx[3];
        double* xt = W.lm[trial] + 4 * (size_t)l;
        const double n0 = x0 + st0, n1 = x1 + st1, n2 = x2 + st2;
        xt[0] = n0; xt[1] = n1; xt[2] = n2; xt[3] = x3;
        s_lm[4 * tid] = n0; s_lm[4 * tid + 1] = n1; s_lm[4 * tid + 2] = n2; s_lm[4 * tid + 3] = x3;
        sc_gd = hv.bb[0] * dl0 + hv.bb[1] * dl1 + hv.bb[2] * dl2;
        sc_ddd = d0 * dl0 * dl0 + d1 * dl1 * dl1 + d2 * dl2 * dl2;
        sc_s2 = st0 * st0 + st1 * st1 + st2 * st2;
        sc_x2 = x0 * x0 + x1 * x1 + x2 * x2 + x3 * x3;
      }
      if (tid < 64) {
        s_sc[tid] = sc_gd;
        s_sc[64 + tid] = sc_ddd;
        s_sc[128 + tid] = sc_s2;
        s_sc[192 + tid] = sc_x2;
      }
    } else {
      if (tid < nlm) {
        s_lm[4 * tid] = hv.xx[0]; s_lm[4 * tid + 1] = hv.xx[1]; s_lm[4 * tid + 2] = hv.xx[2]; s_lm[4 * tid + 3] = hv.xx[3];
      }
      if (tid < 64) s_sc[tid] = s_sc[64 + tid] = s_sc[128 + tid] = s_sc[192 + tid] = 0.0;
    }
    // park the index lists of this group
    if (tid <= nlm) s_lpb[tid] = ops.lpb;
    if (has_pair) {
      s_pp[tid] = ops.pp;
      s_poff[tid] = pf_poff;
      s_plm[tid] = (uint8_t)pf_plm;
      s_slot[tid] = (uint16_t)ops.slot;
    }
    if (tasks_cached && tid < ntask) {
      int* t = s_task + 6 * tid;
      t[0] = ops.task.type; t[1] = ops.task.off_a; t[2] = ops.task.off_b;
      t[3] = ops.task.list_begin - G.tlist_begin; t[4] = ops.task.list_end - G.tlist_begin; t[5] = ops.task.out;
    }
    if (fast) {   // which of the group's tasks holds the J^T J block of pose block bi (behind the pose part of the step)
      int* blktask = reinterpret_cast<int*>(s_aux + GROUP_LM * 9 + FUSE_MAX_TASKS * 36);
      if (tid >= 64 && tid < 64 + 32) blktask[tid - 64] = -1;
    }
    __syncthreads();
    LSTAMP(42);
    if (fast && tid < ntask) reinterpret_cast<int*>(s_aux + GROUP_LM * 9 + FUSE_MAX_TASKS * 36)[ops.task.off_a / 6] = tid;

    // ------------------------------------------------------------------ phase B: one observation per lane
    // a[0..5] V, a[6..8] b, a[9..14] un-robustified H_l, a[15] cost of this observation
    REAL a[16];
#pragma unroll
    for (int e = 0; e < 16; ++e) a[e] = REAL(0);
    const int key_l = has_obs ? (int)(rec.lm_cam & 0xFFFFFFu) : -1;
    const int key_p = has_obs ? (int)rec.pose : -1;
    if (has_obs) {
      const int o = G.obs_begin + tid;
      const int cam = (int)(rec.lm_cam >> 24);
      double P[7], E[7], intr[12];
      int cam_model;
      if (poses_staged) {
#pragma unroll
        for (int i = 0; i < 7; ++i) {
          P[i] = s_pose[7 * (int)rec.pose + i];
          E[i] = s_pose[7 * (int)rec.ext + i];
        }
      } else {
        const double* pose = W.pose[trial] + 7 * (size_t)rec.pose;
        const double* ext = W.pose[trial] + 7 * (size_t)rec.ext;
#pragma unroll
        for (int i = 0; i < 7; ++i) {
          P[i] = pose[i];
          E[i] = ext[i];
        }
      }
      if (cams_staged) {
#pragma unroll
        for (int i = 0; i < 12; ++i) intr[i] = s_cam[12 * cam + i];
        cam_model = s_cmodel[cam];
      } else {
#pragma unroll
        for (int i = 0; i < 12; ++i) intr[i] = W.cam_intr[12 * cam + i];
        cam_model = W.cam_model[cam];
      }
      const double* lm = s_lm + 4 * (key_l - G.lm_begin);
      const double L4[4] = {lm[0], lm[1], lm[2], lm[3]};
      REAL r0, r1, jl[6];
      if constexpr (std::is_same<REAL, double>::value) {
        ReprojLin Jd;
        reproj_linearize(P, E, L4, intr, cam_model, rec.u, rec.v, rec.sw, false, &Jd);
        r0 = Jd.r[0], r1 = Jd.r[1];
#pragma unroll
        for (int i = 0; i < 6; ++i) jl[i] = Jd.Jl[i];
      } else {
        ReprojLinT<REAL> J;
        reproj_linearize_mixed<REAL>(P, E, L4, intr, cam_model, rec.u, rec.v, rec.sw, false, &J);
        r0 = J.r[0], r1 = J.r[1];
#pragma unroll
        for (int i = 0; i < 6; ++i) jl[i] = J.Jl[i];
      }
      if (W.obs_r[trial]) {
        W.obs_r[trial][2 * (size_t)o] = r0;
        W.obs_r[trial][2 * (size_t)o + 1] = r1;
      }
      // Cauchy corrector (Ceres Corrector with rho'' <= 0: scale r and J by sqrt(rho'))
      const REAL s = r0 * r0 + r1 * r1;
      REAL sr = REAL(1), irho = REAL(1), cost = REAL(0.5) * s;
      if (W.cauchy_b > 0) {
        const REAL bb = REAL(W.cauchy_b * W.cauchy_b);
        const REAL sum = REAL(1) + s / bb;
        const REAL rho1 = REAL(1) / sum;
        cost = REAL(0.5) * bb * log(sum);
        sr = sqrt(rho1);
        irho = sum;
      }
      r0 *= sr, r1 *= sr;
#pragma unroll
      for (int i = 0; i < 6; ++i) jl[i] *= sr;
      a[0] = jl[0] * jl[0] + jl[3] * jl[3];
      a[1] = jl[0] * jl[1] + jl[3] * jl[4];
      a[2] = jl[0] * jl[2] + jl[3] * jl[5];
      a[3] = jl[1] * jl[1] + jl[4] * jl[4];
      a[4] = jl[1] * jl[2] + jl[4] * jl[5];
      a[5] = jl[2] * jl[2] + jl[5] * jl[5];
      a[6] = jl[0] * r0 + jl[3] * r1;
      a[7] = jl[1] * r0 + jl[4] * r1;
      a[8] = jl[2] * r0 + jl[5] * r1;
#pragma unroll
      for (int e = 0; e < 6; ++e) a[9 + e] = a[e] * irho;
      a[15] = cost;
    }
    LSTAMP(43);
    // ---- pieces: runs of one (landmark, pose) inside a DPP row, cut into pairs of lanes from the start of the run ----
    // (the lane exchanges first, with every lane active: a DPP read inside a short-circuited condition would see disabled lanes)
    const int prev_l = row_prev_i(key_l, -2), prev_p = row_prev_i(key_p, -2);
    const int next_l = row_next_i(key_l, -2), next_p = row_next_i(key_p, -2);
    const bool brk = ((lane & 15) == 0) | (key_l != prev_l) | (key_p != prev_p);
    const bool same_next = has_obs & ((lane & 15) != 15) & (key_l == next_l) & (key_p == next_p);
    const unsigned long long brk_mask = __ballot(brk);
    const unsigned long long below = brk_mask & ((2ull << lane) - 1ull);   // (lane 0 of every row is a break: never empty)
    const int run_start = 63 - __builtin_clzll(below);
    const bool head = has_obs && (((lane - run_start) & 1) == 0);
    const bool merge = head && same_next;
    const unsigned long long head_mask = __ballot(head);
    const int pw = wave == 0 ? 0 : (wave == 1 ? G.pw1 : (wave == 2 ? G.pw2 : G.pw3));
    const int piece = pw + __builtin_amdgcn_mbcnt_hi((unsigned)(head_mask >> 32), __builtin_amdgcn_mbcnt_lo((unsigned)head_mask, 0));
#pragma unroll
    for (int e = 0; e < 16; ++e) {
      const REAL t = row_next(a[e]);
      a[e] += merge ? t : REAL(0);
    }
    if (head) {
      REAL* rp = s_rec + 16 * piece;
#pragma unroll
      for (int e = 0; e < 16; ++e) rp[e] = a[e];
    }
    __syncthreads();
    LSTAMP(44);

    // ------------------------------------------------------------------ phase C
    // (a) per landmark: 16 lanes, one per entry, sum the landmark's piece records in piece order
    {
      const int e = tid & 15;
      const bool is_cost = e == 15, is_b = e >= 6 && e < 9;
      double* obase = e < 6 ? W.V[trial] : (is_b ? W.bl[trial] : W.Hq[trial]);
      const int ostride = is_b ? 3 : 6, ooff = e < 6 ? e : (is_b ? e - 6 : e - 9);
      for (int wi = tid; wi < nlm * 16; wi += LIN_THREADS) {
        const int ll = wi >> 4;
        const int p0 = s_lpb[ll], p1 = s_lpb[ll + 1];
        REAL s0 = 0, s1 = 0;
        int p = p0;
        for (; p + 1 < p1; p += 2) {
          s0 += s_rec[16 * p + e];
          s1 += s_rec[16 * (p + 1) + e];
        }
        if (p < p1) s0 += s_rec[16 * p + e];
        const REAL sum = s0 + s1;
        if (!is_cost) obase[ostride * (size_t)(G.lm_begin + ll) + ooff] = sum;
        s_lmres[16 * ll + e] = sum;
        // first linearisation of an optimize() call: Jacobi scale of the landmark columns (Ceres EstimateScale)
        if (init && opt.dogleg && (e == 0 || e == 3 || e == 5))
          W.lm_scale[3 * (size_t)(G.lm_begin + ll) + (e == 0 ? 0 : (e == 3 ? 1 : 2))] = opt.jacobi_scaling ? 1.0 / (1.0 + sqrt((double)sum)) : 1.0;
      }
    }
    LSTAMP(45);
    // (b) per (landmark, block) pair, one lane each: Vp, bp from the pair's pieces; d and w from the trial state
    REAL vp[6] = {0, 0, 0, 0, 0, 0}, bp[3] = {0, 0, 0};
    REAL d0 = 0, d1 = 0, d2 = 0, hw = 0;
    int my_slot = 0;
    if (has_pair) {
      const int pp = s_pp[tid];
      const int p0 = pp & 0xFFFF, p1 = p0 + (pp >> 16);
      for (int p = p0; p < p1; ++p) {
        const REAL* rp = s_rec + 16 * p;
#pragma unroll
        for (int e = 0; e < 6; ++e) vp[e] += rp[e];
#pragma unroll
        for (int e = 0; e < 3; ++e) bp[e] += rp[6 + e];
      }
      double pt[3];
      if (poses_staged) {
        pt[0] = s_pose[7 * pf_pblock], pt[1] = s_pose[7 * pf_pblock + 1], pt[2] = s_pose[7 * pf_pblock + 2];
      } else {
        const double* t = W.pose[trial] + 7 * (size_t)pf_pblock;
        pt[0] = t[0], pt[1] = t[1], pt[2] = t[2];
      }
      const double* x = s_lm + 4 * pf_plm;
      const double w = x[3];
      d0 = REAL(x[0] - pt[0] * w);
      d1 = REAL(x[1] - pt[1] * w);
      d2 = REAL(x[2] - pt[2] * w);
      hw = REAL(w);
      my_slot = (int)s_slot[tid];
    }
    __syncthreads();   // the piece records are free, the landmark sums are complete
    LSTAMP(46);
    // (d) group scalars, by wave 3 (no pair lives there) in the shadow of the pair lanes' work
    if (wave == 3) {
      double cost = 0, gm = 0, sc_gd = 0, sc_ddd = 0, sc_s2 = 0, sc_x2 = 0;
      if (lane < nlm) {
        cost = s_lmres[16 * lane + 15];
        gm = fmax(fabs(s_lmres[16 * lane + 6]), fmax(fabs(s_lmres[16 * lane + 7]), fabs(s_lmres[16 * lane + 8])));
        sc_gd = s_sc[lane], sc_ddd = s_sc[64 + lane], sc_s2 = s_sc[128 + lane], sc_x2 = s_sc[192 + lane];
      }
      cost = wave_sum_full(cost);
      gm = wave_max_full(gm);
      sc_gd = wave_sum_full(sc_gd);
      sc_ddd = wave_sum_full(sc_ddd);
      sc_s2 = wave_sum_full(sc_s2);
      sc_x2 = wave_sum_full(sc_x2);
      if (lane == 0) {
        double* gs = W.gscal[trial] + (size_t)g * GS_COUNT;
        gs[GS_COST] = cost;
        gs[GS_GD] = sc_gd;
        gs[GS_DDD] = sc_ddd;
        gs[GS_STEP2] = sc_s2;
        gs[GS_X2] = sc_x2;
        gs[GS_GMAX] = gm;
      }
    }
    // W = M^T Vp (6x3), U = M^T Vp M (upper triangle, 21), g = M^T bp (6);  M = [ -w I | e_i x d ]
    REAL Wm[18];
    {
      const REAL V3[3][3] = {{vp[0], vp[1], vp[2]}, {vp[1], vp[3], vp[4]}, {vp[2], vp[4], vp[5]}};
#pragma unroll
      for (int c = 0; c < 3; ++c) {
        Wm[0 + c] = -hw * V3[0][c];
        Wm[3 + c] = -hw * V3[1][c];
        Wm[6 + c] = -hw * V3[2][c];
        // a b - c d leaves the compiler ways to contract (which product is rounded, or both), and the instantiations did not all
        // take the same one.  In float W of the UB = 14 kernel differed from the others' in the last bit of some entries
        // (tests/test_gpu_fp32_linearize.py); in double W[3][0] and W[5][2] of the fused kernels differed from the unfused
        // ones' (tests/test_gpu_fp64_linearize.py).  Spelled out, every instantiation of one precision forms the same bits.
        // In double: c d rounded first, as both families had it in seven of the nine entries; W[3][0] as the fused kernels
        // formed it (a b rounded first), W[5][2] as the unfused ones did (both products rounded), so that each family's
        // results move in one entry only (profiles/fp64_referee_notes.md, "Route pairs").
        constexpr bool dbl = std::is_same<REAL, double>::value;
        if (dbl && c == 0) Wm[9 + c] = fma_real(-d1, V3[2][c], d2 * V3[1][c]);
        else Wm[9 + c] = fma_real(d2, V3[1][c], -(d1 * V3[2][c]));
        Wm[12 + c] = fma_real(d0, V3[2][c], -(d2 * V3[0][c]));
        if (dbl && c == 2) Wm[15 + c] = sub_of_rounded_products(d1, V3[0][c], d0, V3[1][c]);
        else Wm[15 + c] = fma_real(d1, V3[0][c], -(d0 * V3[1][c]));
      }
    }
    if (has_pair) {
      double* Wt = W.W[trial] + (size_t)(G.pair_begin + tid) * 18;
#pragma unroll
      for (int i = 0; i < 18; ++i) Wt[i] = Wm[i];
    }
    // (c) per-block J^T J / J^T r partials.  The pair's record goes to its SLOT — the records of one block (task) are contiguous
    //     there — UB entries per round, and every (block, entry) is one contiguous sum in slot (= list) order
    auto urec_k = [&](int kk) -> REAL {   // entry kk of this pair's block record: k < 21: U[ra][b] at k = ut6(ra, b); 21 + a: g[a]
      REAL v = 0;
      int k = 0;
#pragma unroll
      for (int ra = 0; ra < 7; ++ra)
#pragma unroll
        for (int b = (ra < 6 ? ra : 0); b < 6; ++b, ++k)
          if (k == kk) {
            const REAL w0 = ra < 6 ? Wm[3 * (ra < 6 ? ra : 0)] : bp[0], w1 = ra < 6 ? Wm[3 * (ra < 6 ? ra : 0) + 1] : bp[1],
                       w2 = ra < 6 ? Wm[3 * (ra < 6 ? ra : 0) + 2] : bp[2];
            if constexpr (std::is_same<REAL, float>::value)   // (spelled out like the rows of W above: the same bits in one round and in two)
              v = b == 0 ? -hw * w0 : b == 1 ? -hw * w1 : b == 2 ? -hw * w2 : b == 3 ? fmaf(w1, d2, -(w2 * d1)) : b == 4 ? fmaf(w2, d0, -(w0 * d2)) : fmaf(w0, d1, -(w1 * d0));
            else
              v = b == 0 ? -hw * w0 : b == 1 ? -hw * w1 : b == 2 ? -hw * w2 : b == 3 ? w1 * d2 - w2 * d1 : b == 4 ? w2 * d0 - w0 * d2 : w0 * d1 - w1 * d0;
          }
      return v;
    };
#pragma unroll
    for (int r0 = 0; r0 < LIN2_REC; r0 += UB) {
      const int ne = (LIN2_REC - r0 < UB) ? LIN2_REC - r0 : UB;
      if (r0 > 0) __syncthreads();   // the previous round's sums are done with the records
      if (has_pair) {
        REAL* ur = s_rec + UB * my_slot;
#pragma unroll
        for (int k = 0; k < UB; ++k)
          if (k < ne) ur[k] = urec_k(r0 + k);
      }
      __syncthreads();
      if (r0 == 0) LSTAMP(47);
      for (int wi = tid; wi < ntask * ne; wi += LIN_THREADS) {
        const int tt = wi / ne, k = wi - tt * ne;
        int lb, le, out;
        if (tasks_cached) {
          const int* t = s_task + 6 * tt;
          lb = t[3], le = t[4], out = t[5];
        } else {
          const Task T = W.tasks[G.task_begin + tt];
          lb = T.list_begin - G.tlist_begin, le = T.list_end - G.tlist_begin, out = T.out;
        }
        REAL s0 = 0, s1 = 0;
        int j = lb;
        for (; j + 1 < le; j += 2) {
          s0 += s_rec[j * UB + k];
          s1 += s_rec[(j + 1) * UB + k];
        }
        if (j < le) s0 += s_rec[j * UB + k];
        const REAL sum = s0 + s1;
        W.gpart[trial][out + r0 + k] = sum;
        if (fast) s_aux[GROUP_LM * 9 + tt * 36 + r0 + k] = sum;   // the group's own J^T J / J^T r blocks for the reduction below
      }
    }
    LSTAMP(48);
    LSTAMP(49);
    if constexpr (FUSE) {
      __syncthreads();   // block records consumed (the tiles of the reduction take their place), J^T J blocks complete
      if (fast) {
        FuseItemsT<6> fit;
#pragma unroll
        for (int q = 0; q < 6; ++q) {
          fit.row[q] = has_pair ? pf_poff + q : -1;
          fit.lm[q] = pf_plm;
          fit.w[q][0] = Wm[3 * q], fit.w[q][1] = Wm[3 * q + 1], fit.w[q][2] = Wm[3 * q + 2];
        }
        fused_reduce_fast<RECD, 6>(W, opt, g, trial, lam_next, nlm, init != 0, pf_sc, fit, smem, s_lmres, s_aux);
      } else {
        reduce_own_group(g, trial, lam_next);
      }
    }
    LSTAMP(50);
    LSTAMP(51);
