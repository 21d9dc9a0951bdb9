// Dense tail of the marginalisation: what okvis::ceres::MarginalizationError does
// after its landmark blocks are gone.
//
//   marginalizeOut, dense part      okvis_ceres/src/MarginalizationError.cpp:686-736
//   updateErrorComputation          okvis_ceres/src/MarginalizationError.cpp:806-846
//   pseudoInverseSymmSqrt           okvis_ceres/include/okvis/ceres/implementation/MarginalizationError.hpp:215-243
//
// Input: the undamped system (H, b0) over all free pose-type / speed-bias blocks of a (sub-)window, exported
// by solve_kernel(final_only = 2) after the Schur kernel eliminated every landmark with the preconditioned
// pseudo-inverse, plus the previous prior (H_old, b0_old) over some of those blocks.  One workgroup per window.
// The symmetric eigen-decompositions (Eigen::SelfAdjointEigenSolver in the reference) are done by cyclic
// Jacobi in the round-robin parallel ordering: n/2 disjoint rotations per round, column phase then row phase.
#pragma once
#include "ba_device.hpp"
#include "ba_types.hpp"

namespace ba {

constexpr int MARG_THREADS = 1024;
constexpr int MARG_PC_NMAX = 96;     // largest matrix of the pivoted-Cholesky path (two n x n matrices in LDS)
constexpr int MARG_LDS_DOUBLES = 18 * 1024;  // 144 KB of dynamic LDS for the eigen-solver buffers
// Two instantiations of marg_dense_kernel: index lists and vectors of the reduced system are static LDS arrays sized by the
// template arguments.  The small one serves every sub-window whose reduced system is solved in LDS (D <= MAX_D_LDS) with a
// previous prior of up to MARG_SMALL_PRIOR rows; the large one takes everything up to MAX_D / MAX_MARG_DIM with less dynamic
// LDS (its matrices live in the HBM workspace: same code, same arithmetic, slower).
constexpr int MARG_SMALL_PRIOR = 192;
constexpr int MARG_LDS_DOUBLES_LARGE = 11 * 1024;

// (the pointers are typed as global-address-space pointers on the device, as WinPtrs' are — ba_types.hpp, BA_G: marg_dense_kernel reads
//  the record from memory, and a pointer read from memory is a generic one otherwise, whose accesses become FLAT instructions)
struct MargArgs {
  const BA_G unsigned char* pose_marg;  // [n_pose] 1 = eliminate this block in the dense step
  const BA_G unsigned char* sb_marg;    // [n_sb]
  int prior_dim, prior_nb;
  const BA_G int* pb_type;   // [prior_nb] 0 = pose-type, 1 = speed/bias
  const BA_G int* pb_idx;    // [prior_nb] block index in the window
  const BA_G int* pb_off;    // [prior_nb] offset inside the prior
  const BA_G double* prior_H;   // [prior_dim^2] row-major
  const BA_G double* prior_b0;  // [prior_dim]
  BA_G double* work;            // marg_work_doubles(D)
  BA_G double* out_H;           // [na*na]
  BA_G double* out_b0;          // [na]
  BA_G double* out_J;           // [na*na]
  BA_G double* out_e0;          // [na]
  BA_G int* out_info;           // [0] na, [1] nm, [2] rank, [3] Jacobi sweeps (V), [4] Jacobi sweeps (H), [8 + i] kept reduced index i
  // tiled route (ba_marg_tiles.hpp): the kernel stops after M and b0 (stage = 1) and leaves the scaling of the elimination here
  BA_G double* p_out = nullptr; // [D]
};

// workspace of marg_dense_kernel: A | Q | M (D^2 each), the 6-row panel of marg_chol_inverse, and the two padded matrices of the
// Cholesky fast path when they do not fit into LDS
__host__ __device__ inline size_t marg_work_doubles(int D) {
  return 3 * (size_t)D * D + 6 * ((size_t)D + 6) + 2 * ((size_t)D + 6) * ((size_t)D + 6);
}

// Round-robin pairing of m (even) players: round r in [0, m-1), pair k in [0, m/2) -> (p, q), p < q.
__device__ __forceinline__ void rr_pair(int m, int r, int k, int* p, int* q) {
  int a, b;
  if (k == 0) {
    a = m - 1;
    b = r;
  } else {
    a = r + k;   // r, k < m - 1: one conditional subtraction instead of an integer division
    if (a >= m - 1) a -= m - 1;
    b = r - k;
    if (b < 0) b += m - 1;
  }
  *p = a < b ? a : b;
  *q = a < b ? b : a;
}
// Jacobi rotation that annihilates X[p][q]: G = [[c, s], [-s, c]] (identity when already negligible or when
// q is the padding index of an odd-sized matrix).  Every work-item that needs the rotation of a pair recomputes
// it from the same three numbers, so all of them take the same decision.
__device__ __forceinline__ bool jacobi_rot(const double* X, int n, int p, int q, double thr, double* c, double* s) {
  *c = 1.0;
  *s = 0.0;
  if (q >= n) return false;
  const double apq = X[p * n + q], app = X[p * n + p], aqq = X[q * n + q];
  // negligible relative to the two diagonal entries, or below the absolute accuracy eps * max|diag| any
  // backward-stable symmetric eigen-solver delivers (graded matrices never reach the relative test)
  if (fabs(apq) <= thr || fabs(apq) <= 2.220446049250313e-16 * sqrt(fabs(app * aqq))) return false;
  // tan of the rotation angle: only needs to be accurate enough to keep the quadratic convergence, so the two
  // divisions and the square root use the hardware approximations (v_rcp_f64 / v_rsq_f64, ~1e-8 relative);
  // c = (1 + t^2)^-1/2 is refined by two Newton steps to full precision, which is what keeps Q orthogonal
  const double theta = (aqq - app) * (0.5 * __builtin_amdgcn_rcp(apq));
  const double h2 = theta * theta + 1.0;
  const double hyp = h2 * __builtin_amdgcn_rsq(h2);
  const double t = (theta >= 0 ? 1.0 : -1.0) * __builtin_amdgcn_rcp(fabs(theta) + hyp);
  const double u = t * t + 1.0;
  double y = __builtin_amdgcn_rsq(u);
  y = y * (1.5 - 0.5 * u * y * y);
  y = y * (1.5 - 0.5 * u * y * y);
  *c = y;
  *s = t * y;
  return true;
}

template <int MAXD>
struct JacobiTab {  // the n/2 disjoint rotations of one round
  int p[MAXD / 2 + 1], q[MAXD / 2 + 1];
  double c[MAXD / 2 + 1], s[MAXD / 2 + 1];
  int rotated;
  int round_rot[2];  // any rotation in the current round (two slots: rounds alternate, no extra barrier to reset)
  double thr;
};

// Symmetric eigen-decomposition by cyclic Jacobi, round-robin parallel ordering.  Per round: (1) n/2 work-items
// compute the disjoint rotations into LDS, (2) the rotations split the matrix into (n/2)^2 independent 2x2
// blocks B(k1,k2) <- G_k1^T B G_k2 — one work-item each, in place — and Q <- Q G by column pairs.
// X holds the input and the result (eigenvalues on the diagonal).  X / Q may live in LDS or in global memory.
template <class JT>
__device__ void jacobi_eig(double* X, double* Q, int n, int tid, JT& jt, int* sweeps) {
  for (int k = tid; k < n * n; k += MARG_THREADS) Q[k] = (k / n == k % n) ? 1.0 : 0.0;
  if (tid == 0) {
    double dmax = 0.0;
    for (int i = 0; i < n; ++i) dmax = fmax(dmax, fabs(X[i * n + i]));
    jt.thr = fmax(2.220446049250313e-16 * dmax, 1e-300);
  }
  __syncthreads();
  *sweeps = 0;
  if (n < 2) return;
  const double thr = jt.thr;
  const int m = (n + 1) & ~1, half = m / 2;
  // Which 2x2 block / which (pair, row) of Q a work-item updates does not depend on the round: decode the item
  // indices ONCE (the integer square root and the division cost more instructions than the update itself, and with
  // 16 waves per CU a round is bound by the number of instructions issued).  Two block items and two Q items per
  // lane are kept in registers; larger matrices decode the rest on the fly.
  const int nblk = half * (half + 1) / 2, nq = half * n;
  int xk1[2] = {-1, -1}, xk2[2] = {0, 0}, qk[2] = {-1, -1}, qi[2] = {0, 0};
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int it = tid + u * MARG_THREADS;
    if (it < nblk) {
      int k2 = (int)((sqrtf(8.0f * it + 1.0f) - 1.0f) * 0.5f);
      while ((k2 + 1) * (k2 + 2) / 2 <= it) ++k2;
      while (k2 * (k2 + 1) / 2 > it) --k2;
      xk2[u] = k2;
      xk1[u] = it - k2 * (k2 + 1) / 2;  // k1 <= k2
    }
    if (it < nq) {
      qk[u] = it / n;
      qi[u] = it - qk[u] * n;
    }
  }
  auto block_update = [&](int k1, int k2) {
    const double c1 = jt.c[k1], s1 = jt.s[k1], c2 = jt.c[k2], s2 = jt.s[k2];
    if (s1 == 0.0 && s2 == 0.0) return;
    const int p1 = jt.p[k1], q1 = jt.q[k1], p2 = jt.p[k2], q2 = jt.q[k2];
    const bool v1 = q1 >= 0, v2 = q2 >= 0;  // -1: padding index of an odd-sized matrix
    const double bpp = X[p1 * n + p2];
    const double bpq = v2 ? X[p1 * n + q2] : 0.0;
    const double bqp = v1 ? X[q1 * n + p2] : 0.0;
    const double bqq = (v1 && v2) ? X[q1 * n + q2] : 0.0;
    const double tpp = c2 * bpp - s2 * bpq, tpq = s2 * bpp + c2 * bpq;
    const double tqp = c2 * bqp - s2 * bqq, tqq = s2 * bqp + c2 * bqq;
    const double npp = c1 * tpp - s1 * tqp, npq = c1 * tpq - s1 * tqq;
    const double nqp = s1 * tpp + c1 * tqp, nqq = s1 * tpq + c1 * tqq;
    X[p1 * n + p2] = npp;
    if (v2) X[p1 * n + q2] = npq;
    if (v1) X[q1 * n + p2] = nqp;
    if (v1 && v2) X[q1 * n + q2] = nqq;
    if (k1 != k2) {
      X[p2 * n + p1] = npp;
      if (v2) X[q2 * n + p1] = npq;
      if (v1) X[p2 * n + q1] = nqp;
      if (v1 && v2) X[q2 * n + q1] = nqq;
    }
  };
  auto q_update = [&](int k, int i) {  // Q <- Q G
    const double sk = jt.s[k];
    if (sk == 0.0) return;
    const double ck = jt.c[k];
    const int p = jt.p[k], q = jt.q[k];
    const double qip = Q[i * n + p], qiq = Q[i * n + q];
    Q[i * n + p] = ck * qip - sk * qiq;
    Q[i * n + q] = sk * qip + ck * qiq;
  };
  int sweep = 0;
  for (; sweep < 60; ++sweep) {
    if (tid == 0) {
      jt.rotated = 0;
      jt.round_rot[0] = 0;
      jt.round_rot[1] = 0;
    }
    __syncthreads();
    for (int r = 0; r < m - 1; ++r) {
      const int slot = r & 1;
      if (tid == 0) jt.round_rot[slot ^ 1] = 0;  // the other slot: last read before the previous round's final barrier
      if (tid < half) {
        int p, q;
        rr_pair(m, r, tid, &p, &q);
        double c, s;
        const bool rot = jacobi_rot(X, n, p, q, thr, &c, &s);
        jt.p[tid] = p;
        jt.q[tid] = q < n ? q : -1;
        jt.c[tid] = c;
        jt.s[tid] = s;
        if (rot) {
          jt.rotated = 1;
          jt.round_rot[slot] = 1;
        }
      }
      __syncthreads();
      if (!jt.round_rot[slot]) continue;  // nothing to rotate in this round (late sweeps): skip the update phase
      // the matrix stays symmetric: update the blocks with k2 >= k1 and write each one and its mirror image
#pragma unroll
      for (int u = 0; u < 2; ++u)
        if (xk1[u] >= 0) block_update(xk1[u], xk2[u]);
      for (int it = tid + 2 * MARG_THREADS; it < nblk; it += MARG_THREADS) {
        int k2 = (int)((sqrtf(8.0f * it + 1.0f) - 1.0f) * 0.5f);
        while ((k2 + 1) * (k2 + 2) / 2 <= it) ++k2;
        while (k2 * (k2 + 1) / 2 > it) --k2;
        block_update(it - k2 * (k2 + 1) / 2, k2);
      }
#pragma unroll
      for (int u = 0; u < 2; ++u)
        if (qk[u] >= 0) q_update(qk[u], qi[u]);
      for (int it = tid + 2 * MARG_THREADS; it < nq; it += MARG_THREADS) q_update(it / n, it % n);
      __syncthreads();
    }
    if (!jt.rotated) break;
    __syncthreads();
  }
  *sweeps = sweep;
}

__device__ __forceinline__ double marg_rsqrt(double x) {  // v_rsq_f64 + two Newton steps
  double y = __builtin_amdgcn_rsq(x);
  y = y * (1.5 - 0.5 * x * y * y);
  y = y * (1.5 - 0.5 * x * y * y);
  return y;
}

// Second fast path, for a matrix that IS rank deficient (the prior that stays behind after a marginalisation
// typically has a null space of dimension 3): Cholesky with diagonal pivoting  Pi^T A Pi = [L11; L21][L11; L21]^T + R.
// It is taken only if the numerical rank is unambiguous with respect to the reference's truncation threshold
// tau = eps n lambda_max, using the bounds
//   * the r leading pivots:   lambda_r(A) >= lambda_min(A11) >= 1 / ||L11^-1||_F^2     (Cauchy interlacing),
//   * the rest:               lambda_(r+1)(A) <= (1 + ||L21 L11^-1||_F)^2 trace(R)      (Ostrowski, A = C diag(A11, R) C^T),
//   * the threshold itself:   eps n max_i A_ii <= tau <= eps n max_i sum_j |A_ij| =: tau_hi.
// The kept eigenvalues are PROVEN to lie above every possible threshold (> 4 tau_hi).  The remainder R of a
// rank-deficient matrix is rounding noise, so "below tau" cannot be proven for the dropped ones; required instead: the
// UPPER bound of the dropped eigenvalues is below 1e3 tau_hi AND there is a gap of at least 100 to the smallest kept one.
// Measured (OKVIS_BA_DEBUG=marg prints the bounds; tools/gpu_marg_bounds.py): after ONE marginalisation of a gauge-deficient
// window the bound is 0.02 .. 0.44 tau_hi; in the running pipeline, where every prior is built on the previous one, it is
// 2 .. 360 tau_hi (80-frame replay) - there the reference's own eigen decision flips between consecutive frames (rank 42 / 43
// of 45), i.e. the disputed direction sits at the cut itself.  A limit of 4 tau_hi was tried: every frame of the replay then
// takes the Jacobi eigen-solver (+0.57 ms per frame) for the same estimates.  NUMERICAL POLICY (the one place where this
// backend may decide differently from the reference): an eigen-direction with lambda in (tau, 1e3 tau_hi) - information
// below 1e-11 of the strongest direction - that is separated from the rest by two decades is dropped here, kept there.  The
// 20-case sweep (test_gauge_deficient_random_sweep) and the frame-by-frame comparison with the reference's own Estimator
// (test_gpu_estimator_vs_reference) see no difference in rank, prior size or states.  Then
// A_r = M M^T with M = Pi [L11; L21] differs from the reference's truncated eigen-sum by O(eps n lambda_max), and J, e0
// follow from M instead of the eigen-pairs (same J^T J, same J^T e0 up to that order).  B: n x n, stride n, full
// symmetric storage (destroyed: the lower trapezoid becomes L); X: n x n scratch (X11 = L11^-1, row-major).
// Returns the rank, or -1 when the bounds do not decide (the caller then runs the Jacobi eigen-solver).
__device__ int marg_pivoted_chol(double* B, double* X, int n, int* perm, double* rsc, double* red, int tid, double* prof,
                                 int* bounds_out) {
#define PSTAMP(k) do { if (prof && tid == 0) prof[k] = (double)clock64(); } while (0)
  const double EPS = 2.220446049250313e-16;
  __shared__ double s_rowmax, s_acc[2];
  // upper end of the threshold bracket: eps n max_i sum_j |A_ij|
  double rs = 0.0;
  if (tid < n)
    for (int c = 0; c < n; ++c) rs += fabs(B[tid * n + c]);
  rs = wave_max(rs);
  if ((tid & 63) == 0) red[tid >> 6] = rs;
  __syncthreads();
  if (tid == 0) {
    double b = 0;
    for (int i = 0; i < MARG_THREADS / 64; ++i) b = fmax(b, red[i]);
    s_rowmax = b;
  }
  __syncthreads();
  const double tau_hi = EPS * n * s_rowmax;
  PSTAMP(9);
  // Elimination WITHOUT interchanges and with ONE barrier per pivot: the matrix stays in place, a pivot only retires
  // its row and column.  Every work-item owns up to
  // PC_Q fixed entries (i, j) of the full symmetric storage and updates those whose row and column are still alive:
  //   B_ij -= B_i,piv B_j,piv / d     (column piv is dead from now on, so it keeps the UNSCALED l_i sqrt(d))
  // The factor is gathered into the permuted trapezoid afterwards:  L_ab = B[perm a][perm b] / sqrt(d_b).
  constexpr int PC_Q = (MARG_PC_NMAX * MARG_PC_NMAX + MARG_THREADS - 1) / MARG_THREADS;   // n <= MARG_PC_NMAX (caller)
  int eij[PC_Q];
  unsigned alive = 0u;
#pragma unroll
  for (int q = 0; q < PC_Q; ++q) {
    const int idx = q * MARG_THREADS + tid;
    const int i = idx / n, j = idx - i * n;
    eij[q] = (i << 8) | j;
    if (idx < n * n) alive |= 1u << q;
  }
  const int lane = tid & 63;
  const int nq = (n * n + MARG_THREADS - 1) / MARG_THREADS;
  // The pivot (largest remaining diagonal entry) is found by the owners of the diagonal entries themselves: after its
  // update each publishes  (bits of max(d, 0) with the low 7 bits replaced by the index)  with a 64-bit LDS atomic max,
  // which orders non-negative doubles like integers; the 128-ulp perturbation only touches the choice, the pivot value
  // is read back from the matrix.  Three rotating slots: read k, publish k + 1, clear k + 2.
  __shared__ unsigned long long s_key[3];
  auto pkey = [](double v, int i) -> unsigned long long {
    return ((unsigned long long)__double_as_longlong(fmax(v, 0.0)) & ~127ull) | (unsigned long long)i;
  };
  if (tid < 3) s_key[tid] = 0ull;
  __syncthreads();
#pragma unroll
  for (int q = 0; q < PC_Q; ++q) {
    if (q < nq && ((alive >> q) & 1u)) {
      const int i = eij[q] >> 8, j = eij[q] & 255;
      if (i == j) atomicMax(&s_key[0], pkey(B[i * n + i], i));
    }
  }
  __syncthreads();
  unsigned own = 0u;            // bit t: diagonal entry lane + 64 t has been a pivot (every wave keeps its own copy)
  int r = n;
  for (int k = 0; k < n; ++k) {
    const int piv = (int)(s_key[k % 3] & 127ull);
    const double m = B[piv * n + piv];
    if (!(m > 16.0 * tau_hi)) {  // everything that is left is a candidate for truncation
      r = k;
      break;
    }
    if ((piv & 63) == lane) own |= 1u << (piv >> 6);
    const double rs = marg_rsqrt(m);
    const double invd = rs * rs;
    if (tid == 0) {
      perm[k] = piv;
      rsc[k] = rs;             // 1 / sqrt(d_k)
      s_key[(k + 2) % 3] = 0ull;
    }
    unsigned long long* nxt = &s_key[(k + 1) % 3];
    const double* rowp = B + piv * n;
#pragma unroll
    for (int q = 0; q < PC_Q; ++q) {
      if (q < nq) {
        const int i = eij[q] >> 8, j = eij[q] & 255;
        if (i == piv || j == piv) alive &= ~(1u << q);
        if ((alive >> q) & 1u) {
          const double v = B[i * n + j] - rowp[i] * rowp[j] * invd;   // row piv = column piv bit for bit, without the stride-n bank conflicts
          B[i * n + j] = v;
          if (i == j) atomicMax(nxt, pkey(v, i));
        }
      }
    }
    __syncthreads();
  }
  PSTAMP(10);
  // the permutation is completed with the indices that never became a pivot (ascending), then the gather
  if (tid < 64) {
    int cnt = r;
#pragma unroll
    for (int t = 0; t < (MARG_PC_NMAX + 63) / 64; ++t) {
      const int i = lane + 64 * t;
      const bool left = i < n && !((own >> t) & 1u);
      const unsigned long long mk = __ballot(left);
      if (left) perm[cnt + __popcll(mk & ((1ull << lane) - 1ull))] = i;
      cnt += __popcll(mk);
    }
  }
  __syncthreads();
  {
    double val[PC_Q];
#pragma unroll
    for (int q = 0; q < PC_Q; ++q) {
      const int a_ = eij[q] >> 8, b_ = eij[q] & 255;
      val[q] = 0.0;
      if (q * MARG_THREADS + tid < n * n) {
        if (b_ < r && a_ >= b_) val[q] = B[perm[a_] * n + perm[b_]] * rsc[b_];
        else if (a_ == b_) val[q] = B[perm[a_] * n + perm[a_]];          // remainder diagonal (trace R)
      }
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < PC_Q; ++q)
      if (q * MARG_THREADS + tid < n * n) B[(eij[q] >> 8) * n + (eij[q] & 255)] = val[q];
  }
  __syncthreads();
  if (r == 0) return -1;
  PSTAMP(11);
  // X11 = L11^-1 by forward substitution, one column per group of 16 lanes (a DPP row): the column stays in registers
  // (lane t of the group holds X_mj for m = j + t + 16 s), a row costs one batch of reads of L, <= PC_S FMAs and a
  // four-step DPP sum; the same groups then form the rows of L21 X11.  ||X11||_F^2 and ||L21 X11||_F^2 on the fly.
  constexpr int PC_S = (MARG_PC_NMAX + 15) / 16;
  double xf = 0.0, wf = 0.0, tr = 0.0;
  {
    const int g = tid >> 4, t = tid & 15;
    for (int j0 = 0; j0 < r; j0 += MARG_THREADS / 16) {   // (uniform trip count: the DPP sums need whole rows of lanes)
      const int j = j0 + g;
      const bool col = j < r;
      double xr[PC_S];
#pragma unroll
      for (int sidx = 0; sidx < PC_S; ++sidx) xr[sidx] = 0.0;
      for (int i = j0; i < n; ++i) {
        double part = 0.0;
#pragma unroll
        for (int sidx = 0; sidx < PC_S; ++sidx) {
          const int m = j + t + 16 * sidx;
          const double bv = (col && m < i && m < r) ? B[i * n + m] : 0.0;
          part += bv * xr[sidx];
        }
        const double tot = row16_sum(part);
        if (col && i >= j) {
          if (i < r) {
            const double x = (i == j) ? rsc[j] : -tot * rsc[i];
            const int d = i - j;
            if ((d & 15) == t) {
#pragma unroll
              for (int sidx = 0; sidx < PC_S; ++sidx)
                if (sidx == (d >> 4)) xr[sidx] = x;
              X[i * n + j] = x;
              xf += x * x;
            }
          } else if (t == 0) {
            wf += tot * tot;
          }
        }
      }
    }
  }
  PSTAMP(12);
  for (int i = r + tid; i < n; i += MARG_THREADS) tr += fmax(B[i * n + i], 0.0);
  xf = wave_sum(xf);
  wf = wave_sum(wf);
  tr = wave_sum(tr);
  if ((tid & 63) == 0) {
    red[tid >> 6] = xf;
    red[MARG_THREADS / 64 + (tid >> 6)] = wf;
    red[2 * (MARG_THREADS / 64) + (tid >> 6)] = tr;
  }
  __syncthreads();
  if (tid == 0) {
    double a = 0, b = 0, c = 0;
    for (int i = 0; i < MARG_THREADS / 64; ++i) {
      a += red[i];
      b += red[MARG_THREADS / 64 + i];
      c += red[2 * (MARG_THREADS / 64) + i];
    }
    const double lam_kept = 1.0 / a;                       // <= lambda_r(A)
    const double cw = 1.0 + sqrt(b);
    const double lam_dropped = cw * cw * c;                // >= lambda_(r+1)(A)
    s_acc[0] = (lam_kept > 4.0 * tau_hi && lam_dropped < 1.0e3 * tau_hi && lam_kept > 100.0 * lam_dropped) ? 1.0 : 0.0;
    bounds_out[0] = (int)fmin(1.0e3 * lam_dropped / tau_hi, 2.0e9);   // diagnostics: 1000 x dropped bound / tau_hi, kept / tau_hi
    bounds_out[1] = (int)fmin(lam_kept / tau_hi, 2.0e9);
    if (prof) {   // diagnostics (debug_arrays): the bounds in units of the upper threshold bracket, the rank, the dimension
      prof[30] = lam_kept / tau_hi;
      prof[31] = lam_dropped / tau_hi;
      prof[32] = (double)r;
      prof[33] = (double)n;
      prof[34] = c / tau_hi;
      prof[35] = cw;
    }
  }
  __syncthreads();
  return s_acc[0] != 0.0 ? r : -1;
#undef PSTAMP
}

// Fast path of the two symmetric decompositions.  The reference eigen-decomposes the pre-scaled matrix and drops
// the eigenvalues <= eps * n * lambda_max.  If NO eigenvalue is that small the pseudo-inverse is the inverse and
// any square root serves, so a Cholesky factor L and L^-1 replace the eigen-pairs (J and e0 are only defined up
// to an orthogonal row transformation anyway).  "No eigenvalue that small" is PROVEN, not assumed:
//   lambda_min >= 1 / trace(A^-1) = 1 / ||L^-1||_F^2        lambda_max <= max row sum of |A|
// and the fast path is taken only if  1 / ||L^-1||_F^2 > 4 eps n (max row sum);  otherwise (or on a non-positive
// pivot) the caller falls back to the Jacobi eigen-decomposition.  M: n x n (stride n, n a multiple of 6, identity
// padded) -> L in the lower triangle; X <- L^-1 (full square, zeros above).  Returns true when the bound holds.
__device__ bool marg_chol_inverse(double* M, double* X, int n, int n_true, double* dinv, double* Tm, double* red,
                                  int* s_flag, int tid) {
  const int nb = n / 6;
  __shared__ double s_rowmax;
  // lambda_max bound: max absolute row sum (before M is overwritten)
  double rs = 0.0;
  if (tid < n_true)
    for (int c = 0; c < n_true; ++c) rs += fabs(M[tid * n + c]);
  rs = wave_max(rs);
  if ((tid & 63) == 0) red[tid >> 6] = rs;
  if (tid == 0) *s_flag = 0;
  __syncthreads();
  if (tid == 0) {
    double m = 0;
    for (int i = 0; i < MARG_THREADS / 64; ++i) m = fmax(m, red[i]);
    s_rowmax = m;
  }
  __syncthreads();
  for (int kb = 0; kb < nb; ++kb) {
    const int k0 = 6 * kb;
    if (tid == 0) {
      double a[6][6];
#pragma unroll
      for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c <= r; ++c) a[r][c] = M[(k0 + r) * n + k0 + c];
      bool bad = false;
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        double d = a[c][c];
#pragma unroll
        for (int m = 0; m < c; ++m) d -= a[c][m] * a[c][m];
        if (!(d > 0.0)) {
          bad = true;
          d = 1.0;
        }
        const double inv = marg_rsqrt(d);
        a[c][c] = d * inv;
        dinv[k0 + c] = inv;
#pragma unroll
        for (int r = c + 1; r < 6; ++r) {
          double v = a[r][c];
#pragma unroll
          for (int m = 0; m < c; ++m) v -= a[r][m] * a[c][m];
          a[r][c] = v * inv;
        }
      }
      if (bad) *s_flag = 1;
#pragma unroll
      for (int r = 0; r < 6; ++r)
#pragma unroll
        for (int c = 0; c <= r; ++c) M[(k0 + r) * n + k0 + c] = a[r][c];
    }
    __syncthreads();
    const int nrows = n - k0 - 6;
    if (tid < nrows) {
      double* row = M + (k0 + 6 + tid) * n + k0;
      double x[6];
#pragma unroll
      for (int c = 0; c < 6; ++c) {
        double v = row[c];
#pragma unroll
        for (int m = 0; m < c; ++m) v -= x[m] * M[(k0 + c) * n + k0 + m];
        x[c] = v * dinv[k0 + c];
      }
#pragma unroll
      for (int c = 0; c < 6; ++c) row[c] = x[c];
    }
    __syncthreads();
    const int ntri = nrows * (nrows + 1) / 2;
    for (int e = tid; e < ntri; e += MARG_THREADS) {
      int r = (int)((sqrtf(8.0f * e + 1.0f) - 1.0f) * 0.5f);
      while ((r + 1) * (r + 2) / 2 <= e) ++r;
      while (r * (r + 1) / 2 > e) --r;
      const int c = e - r * (r + 1) / 2;
      const double* a = M + (k0 + 6 + r) * n + k0;
      const double* b = M + (k0 + 6 + c) * n + k0;
      double sacc = 0;
#pragma unroll
      for (int m = 0; m < 6; ++m) sacc += a[m] * b[m];
      M[(k0 + 6 + r) * n + k0 + 6 + c] -= sacc;
    }
    __syncthreads();
  }
  if (*s_flag) return false;
  // X = L^-1, blocked by 6
  for (int e = tid; e < n * n; e += MARG_THREADS) X[e] = 0.0;
  __syncthreads();
  if (tid < nb) {
    const int k0 = 6 * tid;
#pragma unroll
    for (int c = 0; c < 6; ++c) {
      double x[6];
#pragma unroll
      for (int r = 0; r < 6; ++r) {
        if (r < c) {
          x[r] = 0.0;
          continue;
        }
        double v = (r == c) ? 1.0 : 0.0;
#pragma unroll
        for (int m = 0; m < r; ++m)
          if (m >= c) v -= M[(k0 + r) * n + k0 + m] * x[m];
        x[r] = v * dinv[k0 + r];
      }
#pragma unroll
      for (int r = c; r < 6; ++r) X[(k0 + r) * n + k0 + c] = x[r];
    }
  }
  __syncthreads();
  for (int bi = 1; bi < nb; ++bi) {
    const int ncol = 6 * bi;
    for (int e = tid; e < 6 * ncol; e += MARG_THREADS) {
      const int r = e / ncol, c = e - r * ncol;
      const int m0 = (c / 6) * 6;
      double sacc = 0;
      for (int m = m0; m < ncol; ++m) sacc += M[(6 * bi + r) * n + m] * X[m * n + c];
      Tm[r * n + c] = sacc;
    }
    __syncthreads();
    for (int e = tid; e < 6 * ncol; e += MARG_THREADS) {
      const int r = e / ncol, c = e - r * ncol;
      double sacc = 0;
#pragma unroll
      for (int m = 0; m < 6; ++m)
        if (m <= r) sacc += X[(6 * bi + r) * n + 6 * bi + m] * Tm[m * n + c];
      X[(6 * bi + r) * n + c] = -sacc;
    }
    __syncthreads();
  }
  // ||L^-1||_F^2 over the true part (the identity padding contributes nothing to either bound)
  double fs = 0.0;
  for (int e = tid; e < n_true * n_true; e += MARG_THREADS) {
    const double v = X[(e / n_true) * n + (e % n_true)];
    fs += v * v;
  }
  fs = wave_sum(fs);
  if ((tid & 63) == 0) red[tid >> 6] = fs;
  __syncthreads();
  __shared__ int s_okb;
  if (tid == 0) {
    double f = 0;
    for (int i = 0; i < MARG_THREADS / 64; ++i) f += red[i];
    s_okb = (f > 0.0 && 1.0 / f > 4.0 * 2.220446049250313e-16 * n_true * s_rowmax) ? 1 : 0;
  }
  __syncthreads();
  return s_okb != 0;
}

// The dense tail of one window on one workgroup: the body of marg_dense_kernel.
template <int MAXD, int MAXP>
__device__ __forceinline__ void marg_dense_body(const WinPtrs& W, const MargArgs& a, int lds_doubles, int stage) {
  extern __shared__ __attribute__((aligned(16))) double marg_lds[];
  const int tid = threadIdx.x;
  const int D = W.D;
  double* H = W.S;     // [D][D]
  double* b = W.rhs;   // [D]
  static_assert(MAXP >= MARG_PC_NMAX && MAXD >= MARG_PC_NMAX, "the pivoted factorisation borrows the index lists");
  __shared__ int s_kidx[MAXD], s_midx[MAXD], s_ridx[MAXP];
  __shared__ double s_p[MAXD], s_t[MAXD], s_lam[MAXD], s_ba[MAXD];
  __shared__ int s_na, s_nm, s_cflag;
  __shared__ double s_max;
  __shared__ JacobiTab<MAXD> jt;
  __shared__ double s_dinv[MAXD + 6], s_red[MARG_THREADS / 64], s_red_big[3 * (MARG_THREADS / 64)];
  const double EPS = 2.220446049250313e-16;
#define MSTAMP(k) do { if (W.prof && tid == 0) W.prof[k] = (double)clock64(); } while (0)   // diagnostics (debug_arrays)
  MSTAMP(0);

  // ---- previous prior: H_ and b0_ persist inside the reference's MarginalizationError object ----
  for (int rr = tid; rr < a.prior_dim; rr += MARG_THREADS) {
    int bi = 0;
    for (int k = 0; k < a.prior_nb; ++k)
      if (a.pb_off[k] <= rr) bi = k;
    const int base = a.pb_type[bi] == 0 ? W.pose_off[a.pb_idx[bi]] : W.sb_off[a.pb_idx[bi]];
    s_ridx[rr] = base < 0 ? -1 : base + (rr - a.pb_off[bi]);
  }
  if (tid == 0) {  // kept / eliminated reduced indices, in reduced order
    int na = 0, nm = 0;
    for (int i = 0; i < W.n_pose; ++i) {
      const int off = W.pose_off[i];
      if (off < 0) continue;
      for (int k = 0; k < 6; ++k) {
        if (a.pose_marg[i]) s_midx[nm++] = off + k; else s_kidx[na++] = off + k;
      }
    }
    // pose-type blocks come first in the reduced ordering, so both lists are still sorted after the sb blocks
    for (int i = 0; i < W.n_sb; ++i) {
      const int off = W.sb_off[i];
      if (off < 0) continue;
      for (int k = 0; k < 9; ++k) {
        if (a.sb_marg[i]) s_midx[nm++] = off + k; else s_kidx[na++] = off + k;
      }
    }
    s_na = na;
    s_nm = nm;
    a.out_info[0] = na;
    a.out_info[1] = nm;
    a.out_info[5] = W.ctrl->acc;   // accepted-buffer index after the export (saves the host a separate read)
    for (int i = 0; i < na; ++i) a.out_info[8 + i] = s_kidx[i];
  }
  __syncthreads();
  if (!(stage & 2)) {   // (stage bit 1: marg_prior_add_kernel has done this on many workgroups)
    for (int k = tid; k < a.prior_dim * a.prior_dim; k += MARG_THREADS) {
      const int rr = k / a.prior_dim, cc = k - rr * a.prior_dim;
      const int ri = s_ridx[rr], ci = s_ridx[cc];
      if (ri >= 0 && ci >= 0) H[ri * D + ci] += a.prior_H[k];
    }
    for (int rr = tid; rr < a.prior_dim; rr += MARG_THREADS)
      if (s_ridx[rr] >= 0) b[s_ridx[rr]] += a.prior_b0[rr];
  }
  __syncthreads();
  const int na = s_na, nm = s_nm;
  MSTAMP(1);
  // eigen-solver buffers (matrix + eigenvectors): in LDS when they fit, else in the HBM workspace
  double* M = a.work + 2 * (size_t)D * D;
  auto pick = [&](int n, double** Xp, double** Qp) {
    const int nn = n * n;
    *Xp = nn <= lds_doubles ? marg_lds : a.work;
    *Qp = 2 * nn <= lds_doubles ? marg_lds + nn : a.work + (size_t)D * D;
  };
  double *A, *Q;
  int sweeps_v = 0;
  double* const chol_panel = a.work + 3 * (size_t)D * D;
  // the two padded matrices of the Cholesky fast path: LDS when they fit, else the HBM workspace
  auto pick_chol = [&](int np6, double** Mp, double** Xp) {
    if (2 * np6 * np6 <= lds_doubles) {
      *Mp = marg_lds;
      *Xp = marg_lds + np6 * np6;
    } else {
      *Mp = chol_panel + 6 * ((size_t)D + 6);
      *Xp = *Mp + ((size_t)D + 6) * ((size_t)D + 6);
    }
  };

  if (nm > 0) {
    // ---- dense part of marginalizeOut (:686-736) ----
    for (int i = tid; i < D; i += MARG_THREADS) s_p[i] = H[i * D + i] > 1.0e-9 ? sqrt(H[i * D + i]) : 1.0e-3;  // :689
    __syncthreads();
    bool fast = false;
    {  // Cholesky fast path (see marg_chol_inverse): V^+ = V^-1 proven, "V^(+1/2)" := L^-T
      const int np6 = ((nm + 5) / 6) * 6;
      {
        double *Mp, *Xp;
        pick_chol(np6, &Mp, &Xp);
        for (int k = tid; k < np6 * np6; k += MARG_THREADS) {  // V1 = 0.5 (V + V^T) of the scaled system (:725), padded
          const int i = k / np6, j = k - i * np6;
          double v = (i == j) ? 1.0 : 0.0;
          if (i < nm && j < nm) {
            const int mi = s_midx[i], mj = s_midx[j];
            v = 0.5 * (H[mi * D + mj] / (s_p[mi] * s_p[mj]) + H[mj * D + mi] / (s_p[mj] * s_p[mi]));
          }
          Mp[k] = v;
        }
        __syncthreads();
        fast = marg_chol_inverse(Mp, Xp, np6, nm, s_dinv, chol_panel, s_red, &s_cflag, tid);
        if (fast) {
          Q = a.work + (size_t)D * D;
          for (int k = tid; k < nm * nm; k += MARG_THREADS) {
            const int c = k / nm, j = k - c * nm;
            Q[k] = Xp[j * np6 + c];            // (L^-T)[c][j] = Linv[j][c]
          }
        }
        __syncthreads();
      }
    }
    if (!fast) {
      pick(nm, &A, &Q);
      for (int k = tid; k < nm * nm; k += MARG_THREADS) {  // V1 = 0.5 (V + V^T) of the scaled system (:725)
        const int i = k / nm, j = k - i * nm;
        const int mi = s_midx[i], mj = s_midx[j];
        A[k] = 0.5 * (H[mi * D + mj] / (s_p[mi] * s_p[mj]) + H[mj * D + mi] / (s_p[mj] * s_p[mi]));
      }
      __syncthreads();
    }
    if (!fast) {
      jacobi_eig(A, Q, nm, tid, jt, &sweeps_v);
      if (tid == 0) {
        double mx = A[0];
        for (int i = 1; i < nm; ++i) mx = fmax(mx, A[i * nm + i]);
        s_max = mx;
      }
      __syncthreads();
      {
        const double tol = EPS * nm * s_max;  // pseudoInverseSymmSqrt (:225-233)
        for (int i = tid; i < nm; i += MARG_THREADS) s_lam[i] = A[i * nm + i] > tol ? sqrt(1.0 / A[i * nm + i]) : 0.0;
      }
      __syncthreads();
      for (int k = tid; k < nm * nm; k += MARG_THREADS) Q[k] *= s_lam[k % nm];  // V^(+1/2) = Q diag(l^-1/2)
      __syncthreads();
    }
    MSTAMP(2);
    if (stage & 4) {   // M, b0 and everything behind them on many workgroups (ba_marg_tiles.hpp): they need V^(+1/2), the scaling, the lists
      double* Qg = a.work + (size_t)D * D;
      if (Q != Qg)
        for (int k = tid; k < nm * nm; k += MARG_THREADS) Qg[k] = Q[k];
      for (int i = tid; i < D; i += MARG_THREADS) a.p_out[i] = s_p[i];
      for (int c = tid; c < nm; c += MARG_THREADS) a.out_info[8 + na + c] = s_midx[c];
      if (tid == 0) a.out_info[3] = sweeps_v;
      return;
    }
    for (int k = tid; k < na * nm; k += MARG_THREADS) {  // M = W V^(+1/2) (:729)
      const int i = k / nm, j = k - i * nm;
      const int ki = s_kidx[i];
      double s = 0;
      for (int c = 0; c < nm; ++c) s += H[ki * D + s_midx[c]] / (s_p[ki] * s_p[s_midx[c]]) * Q[c * nm + j];
      M[k] = s;
    }
    for (int j = tid; j < nm; j += MARG_THREADS) {  // V^(+1/2)^T b_b
      double s = 0;
      for (int c = 0; c < nm; ++c) s += Q[c * nm + j] * (b[s_midx[c]] / s_p[s_midx[c]]);
      s_t[j] = s;
    }
    __syncthreads();
    for (int i = tid; i < na; i += MARG_THREADS) {  // b0 = P_a (b_a - M V^(+1/2)^T b_b) (:732,:739)
      const int ki = s_kidx[i];
      double s = b[ki] / s_p[ki];
      for (int c = 0; c < nm; ++c) s -= M[i * nm + c] * s_t[c];
      const double v = s * s_p[ki];
      a.out_b0[i] = v;
      s_ba[i] = v;
    }
    if (stage & 1) {   // the rest on many workgroups (marg_schur_kernel ...): they need the scaling
      for (int i = tid; i < D; i += MARG_THREADS) a.p_out[i] = s_p[i];
      if (tid == 0) a.out_info[3] = sweeps_v;
      return;
    }
    for (int k = tid; k < na * na; k += MARG_THREADS) {  // H = P_a (U - M M^T) P_a (:736-738)
      const int i = k / na, j = k - i * na;
      const int ki = s_kidx[i], kj = s_kidx[j];
      double s = H[ki * D + kj] / (s_p[ki] * s_p[kj]);
      for (int c = 0; c < nm; ++c) s -= M[i * nm + c] * M[j * nm + c];
      a.out_H[k] = s * (s_p[ki] * s_p[kj]);
    }
  } else {
    for (int i = tid; i < na; i += MARG_THREADS) {
      a.out_b0[i] = b[s_kidx[i]];
      s_ba[i] = b[s_kidx[i]];
    }
    if (stage & 1) {
      if (tid == 0) a.out_info[3] = 0;
      return;
    }
    for (int k = tid; k < na * na; k += MARG_THREADS) a.out_H[k] = H[s_kidx[k / na] * D + s_kidx[k % na]];
  }
  __syncthreads();
  if (na == 0) {
    if (tid == 0) a.out_info[2] = 0;
    return;
  }

  MSTAMP(3);
  // ---- updateErrorComputation (:806-846) ----
  const double* Ha = a.out_H;
  for (int i = tid; i < na; i += MARG_THREADS) s_p[i] = Ha[i * na + i] > 1.0e-9 ? sqrt(Ha[i * na + i]) : 1.0e-3;
  __syncthreads();
  int sweeps_h = 0;
  {  // Cholesky fast path: full rank proven -> J = L^T P, e0 = -L^-1 P^-1 b0 (J^T J = H, J^T e0 = -b0)
    const int np6 = ((na + 5) / 6) * 6;
    // (with a previous prior the kept block carries its gauge null space: straight to the pivoted factorisation)
    if (!(a.prior_dim > 0 && na <= MARG_PC_NMAX)) {
      double *Mp, *Xp;
      pick_chol(np6, &Mp, &Xp);
      for (int k = tid; k < np6 * np6; k += MARG_THREADS) {
        const int i = k / np6, j = k - i * np6;
        Mp[k] = (i < na && j < na) ? 0.5 * (Ha[i * na + j] + Ha[j * na + i]) / (s_p[i] * s_p[j]) : (i == j ? 1.0 : 0.0);
      }
      __syncthreads();
      MSTAMP(4);
      const bool full = marg_chol_inverse(Mp, Xp, np6, na, s_dinv, chol_panel, s_red, &s_cflag, tid);
      MSTAMP(5);
      if (full) {
        for (int k = tid; k < na * na; k += MARG_THREADS) {
          const int r = k / na, c = k - r * na;
          a.out_J[k] = (c >= r) ? Mp[c * np6 + r] * s_p[c] : 0.0;
        }
        for (int r = tid; r < na; r += MARG_THREADS) {
          double sacc = 0;
          for (int c = 0; c <= r; ++c) sacc += Xp[r * np6 + c] * (s_ba[c] / s_p[c]);
          a.out_e0[r] = -sacc;
        }
        if (tid == 0) {
          a.out_info[2] = na;
          a.out_info[3] = sweeps_v;
          a.out_info[4] = 0;
        }
        MSTAMP(8);
        return;
      }
    }
  }
  if (2 * na * na <= lds_doubles && na <= MARG_PC_NMAX) {   // rank-deficient prior with an unambiguous numerical rank: pivoted Cholesky
    double* Bp = marg_lds;
    double* Xq = marg_lds + na * na;
    int* perm = s_midx;   // (the eliminated-index list is not needed any more)
    int* pos = s_ridx;    // (neither is the index map of the previous prior; na <= MARG_PC_NMAX entries)
    __syncthreads();
    for (int k = tid; k < na * na; k += MARG_THREADS) {
      const int i = k / na, j = k - i * na;
      Bp[k] = 0.5 * (Ha[i * na + j] + Ha[j * na + i]) / (s_p[i] * s_p[j]);
    }
    __syncthreads();
    MSTAMP(6);
    const int r = marg_pivoted_chol(Bp, Xq, na, perm, s_lam, s_red_big, tid, W.prof, a.out_info + 6);
    MSTAMP(7);
    if (r > 0) {
      if (tid < na) pos[perm[tid]] = tid;
      __syncthreads();
      for (int k = tid; k < na * na; k += MARG_THREADS) {   // J = [M^T; 0] P with M = Pi [L11; L21]
        const int t = k / na, j = k - t * na;
        a.out_J[k] = (t < r && pos[j] >= t) ? Bp[pos[j] * na + t] * s_p[j] : 0.0;
      }
      for (int t = tid; t < na; t += MARG_THREADS) {        // e0 = -[L11^-1 (Pi^T P^-1 b0)_(1..r); 0]
        double sacc = 0.0;
        if (t < r)
          for (int m = 0; m <= t; ++m) sacc += Xq[t * na + m] * (s_ba[perm[m]] / s_p[perm[m]]);
        a.out_e0[t] = t < r ? -sacc : 0.0;
      }
      if (tid == 0) {
        a.out_info[2] = r;
        a.out_info[3] = sweeps_v;
        a.out_info[4] = 0;
      }
      MSTAMP(8);
      return;
    }
    __syncthreads();
  }
  pick(na, &A, &Q);
  for (int k = tid; k < na * na; k += MARG_THREADS) {
    const int i = k / na, j = k - i * na;
    A[k] = 0.5 * (Ha[i * na + j] + Ha[j * na + i]) / (s_p[i] * s_p[j]);
  }
  __syncthreads();
  jacobi_eig(A, Q, na, tid, jt, &sweeps_h);
  if (tid == 0) {
    double mx = A[0];
    for (int i = 1; i < na; ++i) mx = fmax(mx, A[i * na + i]);
    const double tol = EPS * na * mx;
    int rank = 0;
    for (int i = 0; i < na; ++i) {
      const double l = A[i * na + i];
      if (l > tol) {
        s_lam[i] = l;
        ++rank;
      } else {
        s_lam[i] = 0.0;
      }
    }
    a.out_info[2] = rank;
    a.out_info[3] = sweeps_v;
    a.out_info[4] = sweeps_h;
  }
  __syncthreads();
  for (int k = tid; k < na * na; k += MARG_THREADS) {  // J = (P U S^1/2)^T (:832)
    const int r = k / na, c = k - r * na;
    a.out_J[k] = sqrt(s_lam[r]) * Q[c * na + r] * s_p[c];
  }
  for (int r = tid; r < na; r += MARG_THREADS) {  // e0 = -S^(+1/2) U^T P^-1 b0 (:835-837)
    double s = 0;
    for (int c = 0; c < na; ++c) s += Q[c * na + r] * (s_ba[c] / s_p[c]);
    a.out_e0[r] = s_lam[r] > 0.0 ? -sqrt(1.0 / s_lam[r]) * s : 0.0;
  }
#undef MSTAMP
}

// The kernel: workgroup i takes window record wins[i] with the arguments args[i] — a call for one window is a launch of one
// workgroup.  The kernel is LDS-bound to one workgroup per CU, so a range spreads over as many CUs as it has windows.  The argument
// record is copied once at the top, before anything is stored: a uniform index into read-only memory, so the copy is a handful of
// scalar loads and the fields live in scalar registers exactly as kernel arguments would.
template <int MAXD, int MAXP>
__global__ __launch_bounds__(MARG_THREADS) void marg_dense_kernel(const WinPtrs* __restrict__ wins, const MargArgs* __restrict__ args,
                                                                   int lds_doubles, int stage) {
  const MargArgs a = args[blockIdx.x];
  marg_dense_body<MAXD, MAXP>(wins[blockIdx.x], a, lds_doubles, stage);
}

}  // namespace ba
